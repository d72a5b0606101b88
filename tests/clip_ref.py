"""Functional, state-dict-driven torch restatement of transformers' CLIP text model (modeling_clip.py: CLIPTextEmbeddings,
CLIPEncoderLayer = LayerNorm + CLIPAttention + LayerNorm + CLIPMLP with quick_gelu, the final LayerNorm, the pooled
read-out) as flux/modules/conditioner.py calls it -- ``attention_mask=None``: a causal mask and nothing else -- in the dtype
it is asked for (fp64 by default), plus an fp64 statement of each kernel of ca_clip.hip.  Test infrastructure: pinned to
tests/golden/clip_*.npz on the CPU and used as the reference of the GPU tests; the package never imports it.

Written from the formulas, not from conceptattention_amd/clip.py: weights stay unpacked, the mask is an explicit
[L, L] comparison, both pooling rules are spelled out."""
import zlib

import numpy as np
import torch

# name -> (geometry keywords, sequence length, position of the end-of-text token per sequence, the config's
# eos_token_id, (bos, eos, pad) token ids).  A sequence is bos, eos_pos - 1 real tokens, eos, then padding.
#   tiny: the published config's eos_token_id = 2 (the arg-max rule) with CLIP's own padding (pad = eos = the highest id);
#   eos:  eos_token_id = the end-of-text id (the first-match rule) and a padding id that differs, 0.
# Positions: the empty prompt (1), a short one, the 64-row tile boundary on both sides, the full truncated prompt (76).
_GEO = dict(vocab_size=512, hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2)
EOS_POSITIONS = (1, 5, 22, 40, 63, 64, 65, 76)
CASES = {
    "tiny": (dict(_GEO, eos_token_id=2), 77, EOS_POSITIONS, 2, (510, 511, 511)),
    "eos": (dict(_GEO, eos_token_id=511), 77, EOS_POSITIONS, 511, (510, 511, 0)),
}
ROW_STEP = 4   # the goldens keep every 4th token row of every sequence and, always, the pooled row


def case_ids(name):
    """int64 [n_seq, L]: bos, seeded real tokens in [1, 510), eos, padding."""
    geo, length, eos_pos, _, (bos, eos, pad) = CASES[name]
    ids = torch.full((len(eos_pos), length), pad, dtype=torch.long)
    for r, e in enumerate(eos_pos):
        g = torch.Generator(device="cpu")
        g.manual_seed(zlib.crc32(f"clip.{name}.{r}".encode()))
        ids[r, 0] = bos
        ids[r, 1:e] = torch.randint(1, bos, (e - 1,), generator=g)
        ids[r, e] = eos
    return ids


def kept_rows(length, pooled):
    """The sorted rows the golden keeps of every sequence: every ROW_STEP-th and every sequence's pooled one."""
    return sorted(set(range(0, length, ROW_STEP)) | {int(p) for p in pooled})


# ---------------------------------------------------------------------------------------------------------- kernels
def layernorm(x, w, b, eps=1e-5):
    """(x - mean) / sqrt(var + eps) * w + b with the biased variance about the mean."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w.to(x.dtype) + b.to(x.dtype)


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def gelu_tanh(x):
    return x * torch.sigmoid(2.0 * (2.0 / np.pi) ** 0.5 * (x + 0.044715 * x ** 3))


def causal_attention(q, k, v, n_seq, heads, scale):
    """softmax(scale q k^T + mask) v per (sequence, head) on [n_seq * L, heads * 64] rows; mask[i, j] = 0 for j <= i and
    -inf otherwise."""
    rows = q.shape[0]
    length = rows // n_seq
    idx = torch.arange(length)
    mask = torch.zeros(length, length, dtype=q.dtype)
    mask[idx[None, :] > idx[:, None]] = -torch.inf                     # [query, key]

    def split(t):
        return t.reshape(n_seq, length, heads, 64).permute(0, 2, 1, 3)
    s = split(q) @ split(k).transpose(-1, -2) * scale + mask
    return (torch.softmax(s, -1) @ split(v)).permute(0, 2, 1, 3).reshape(rows, heads * 64)


def embed(tok, pos, ids, length):
    """tok[ids[r]] + pos[r % length]."""
    r = torch.arange(ids.shape[0])
    return tok[ids.long()] + pos[r % length]


def pooled_positions(ids, eos_token_id):
    """The pooled row per sequence, spelled out: with eos_token_id == 2 the first position holding the row's largest
    id, otherwise the first position equal to eos_token_id (0 if there is none)."""
    out = []
    for row in ids.tolist():
        if eos_token_id == 2:
            out.append(row.index(max(row)))
        else:
            out.append(row.index(eos_token_id) if eos_token_id in row else 0)
    return out


# ---------------------------------------------------------------------------------------------------------- the model
def text_model(sd, ids, num_heads, num_layers, eos_token_id=2, eps=1e-5, dtype=torch.float64, prefix=""):
    """(last_hidden_state [n_seq, L, hidden], pooler_output [n_seq, hidden]) of CLIPTextModel(input_ids=ids,
    attention_mask=None)."""
    w = {k[len(prefix):]: v.to(dtype) for k, v in sd.items() if k.startswith(prefix)}
    n_seq, length = ids.shape
    x = embed(w["embeddings.token_embedding.weight"], w["embeddings.position_embedding.weight"], ids.reshape(-1), length)
    d = x.shape[1]
    scale = (d // num_heads) ** -0.5
    for i in range(num_layers):
        b = f"encoder.layers.{i}"

        def lin(t, n):
            return t @ w[f"{b}.{n}.weight"].t() + w[f"{b}.{n}.bias"]
        h = layernorm(x, w[f"{b}.layer_norm1.weight"], w[f"{b}.layer_norm1.bias"], eps)
        a = causal_attention(lin(h, "self_attn.q_proj"), lin(h, "self_attn.k_proj"), lin(h, "self_attn.v_proj"), n_seq,
                             num_heads, scale)
        x = x + lin(a, "self_attn.out_proj")
        h = layernorm(x, w[f"{b}.layer_norm2.weight"], w[f"{b}.layer_norm2.bias"], eps)
        x = x + lin(quick_gelu(lin(h, "mlp.fc1")), "mlp.fc2")
    last = layernorm(x, w["final_layer_norm.weight"], w["final_layer_norm.bias"], eps).reshape(n_seq, length, d)
    pooled = last[torch.arange(n_seq), torch.tensor(pooled_positions(ids, eos_token_id))]
    return last, pooled


def rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((got - ref) ** 2).mean() / (ref ** 2).mean()))
