"""Functional, state-dict-driven torch restatement of transformers' T5 encoder (modeling_t5.py: T5Stack of T5Block =
T5LayerSelfAttention + T5LayerFF with T5DenseGatedActDense, T5LayerNorm, the bidirectional relative-position bucket) as
flux/modules/conditioner.py:23-38 calls it -- ``attention_mask=None``: padding tokens attend and are attended to -- in the
dtype it is asked for (fp64 by default), plus an fp64 statement of each kernel of ca_t5.hip.  Test infrastructure:
pinned to tests/golden/t5_*.npz on the CPU and used as the reference of the GPU tests; the package never imports it.

Written from the formulas, not from conceptattention_amd/t5.py: the bucket uses exact integer / fp64 arithmetic (the
golden's table, made by transformers in fp32, is compared with both), weights stay unpacked."""
import math
import zlib

import numpy as np
import torch

# name -> (T5 geometry keywords, sequence length, real tokens per sequence); the rest of a sequence is padding id 0
CASES = {
    "tiny": (dict(vocab_size=512, d_model=256, num_heads=4, d_ff=512, num_layers=2), 256, (7, 3, 2)),
    "long": (dict(vocab_size=512, d_model=256, num_heads=4, d_ff=512, num_layers=1), 512, (9, 1)),
}
ROW_STEP = 8   # the goldens keep every 8th token row of every sequence, row 0 (the concept row) among them


def case_ids(name):
    """int64 [n_seq, L]: seeded token ids in [2, vocab), 1 = end of string after the real tokens, then padding 0."""
    geo, length, real = CASES[name]
    ids = torch.zeros(len(real), length, dtype=torch.long)
    for r, n in enumerate(real):
        g = torch.Generator(device="cpu")
        g.manual_seed(zlib.crc32(f"t5.{name}.{r}".encode()))
        ids[r, : n - 1] = torch.randint(2, geo["vocab_size"], (n - 1,), generator=g)
        ids[r, n - 1] = 1
    return ids


def kept_rows(length):
    return list(range(0, length, ROW_STEP))


# ---------------------------------------------------------------------------------------------------------- the encoder
def bucket_exact(rel: int, num_buckets: int = 32, max_distance: int = 128) -> int:
    """The bidirectional bucket of key - query = rel in exact arithmetic: floor(log(n / 8) / log(16) * 8) decided on
    integers (n^8 against powers of two) where the logarithm would sit on a boundary."""
    nb = num_buckets // 2
    out = nb if rel > 0 else 0
    n = abs(rel)
    max_exact = nb // 2
    if n < max_exact:
        return out + n
    # largest j with (max_distance / max_exact)^(j / span) <= n / max_exact, i.e. max_distance^j max_exact^span <= n^span max_exact^j
    span, j = nb - max_exact, 0
    while max_distance ** (j + 1) * max_exact ** span <= n ** span * max_exact ** (j + 1):
        j += 1
    return out + min(max_exact + j, nb - 1)


def bias_table(weight, length, num_buckets=32, max_distance=128):
    """[heads, 2 length - 1] in weight's dtype: [h, key - query + length - 1] = weight[bucket(key - query), h]."""
    b = torch.tensor([bucket_exact(o, num_buckets, max_distance) for o in range(-(length - 1), length)])
    return weight[b].t().contiguous()


def rmsnorm(x, w, eps=1e-6):
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w.to(x.dtype)


def gelu_tanh(x):
    """0.5 x (1 + tanh(c (x + 0.044715 x^3))), c = sqrt(2 / pi), written as x sigmoid(2 c (...)): the same function
    without the cancellation of 1 + tanh for x << 0."""
    return x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))


def attention(q, k, v, bias, n_seq, heads):
    """softmax(q k^T + bias) v per (sequence, head) on [n_seq * L, heads * 64] rows; bias [heads, 2 L - 1]."""
    rows = q.shape[0]
    length = rows // n_seq
    idx = torch.arange(length)
    rel = idx[None, :] - idx[:, None] + length - 1                      # [query, key]
    def split(t):
        return t.reshape(n_seq, length, heads, 64).permute(0, 2, 1, 3)
    s = split(q) @ split(k).transpose(-1, -2) + bias.to(q.dtype)[:, rel][None]
    return (torch.softmax(s, -1) @ split(v)).permute(0, 2, 1, 3).reshape(rows, heads * 64)


def encoder(sd, ids, num_heads, num_layers, eps=1e-6, num_buckets=32, max_distance=128, dtype=torch.float64):
    """last_hidden_state [n_seq, L, d_model] of T5EncoderModel(input_ids=ids, attention_mask=None)."""
    w = {k: v.to(dtype) for k, v in sd.items()}
    n_seq, length = ids.shape
    x = w["shared.weight"][ids.reshape(-1)]
    bias = bias_table(w["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], length, num_buckets,
                      max_distance)
    for i in range(num_layers):
        a, f = f"encoder.block.{i}.layer.0", f"encoder.block.{i}.layer.1"
        h = rmsnorm(x, w[f"{a}.layer_norm.weight"], eps)
        q, k, v = (h @ w[f"{a}.SelfAttention.{n}.weight"].t() for n in "qkv")
        x = x + attention(q, k, v, bias, n_seq, num_heads) @ w[f"{a}.SelfAttention.o.weight"].t()
        h = rmsnorm(x, w[f"{f}.layer_norm.weight"], eps)
        g = gelu_tanh(h @ w[f"{f}.DenseReluDense.wi_0.weight"].t()) * (h @ w[f"{f}.DenseReluDense.wi_1.weight"].t())
        x = x + g @ w[f"{f}.DenseReluDense.wo.weight"].t()
    return rmsnorm(x, w["encoder.final_layer_norm.weight"], eps).reshape(n_seq, length, -1)


def errors(got, ref):
    """(max-abs, relative rms) distance of two arrays."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()), float(np.sqrt(((got - ref) ** 2).mean() / (ref ** 2).mean()))
