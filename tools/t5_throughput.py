"""HIP-event time of the T5 encoder at the real geometry (t5-v1_1-xxl: 24 blocks, d_model 4096, 64 heads, d_ff 10240)
for the 1 + 4 strings of one generate_image call -- 5 x 256 tokens (schnell) and 5 x 512 (dev) -- beside the same
network on plain torch bf16 ops in the same process, and the share of the HIP time per kernel family.  The weights are
drawn on the device straight into the packed operands (the CPU generator would have to produce 4.7 G values).  Warm-up,
then the median of the repeats.  Each step is a process of its own under its own time limit:
    python tools/t5_throughput.py          # runs every step: `timeout ... python tools/t5_throughput.py L`
    python tools/t5_throughput.py 256      # one step, one JSON line
No number printed here is a gate."""
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SEQ = 5


def timed(fn, warmup=2, repeats=5):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def device_encoder(p):
    """A T5Encoder whose packed operands are drawn on the device with synthetic_t5_state_dict's scales."""
    import torch
    from conceptattention_amd.t5 import T5Encoder
    enc = T5Encoder(p, "cuda")
    g = torch.Generator(device="cuda").manual_seed(0)

    def u(rows, cols, scale):
        return ((torch.rand(rows, cols, device="cuda", generator=g) * 2 - 1) * scale).to(torch.bfloat16)

    def ln():
        return 1 + 0.1 * (torch.rand(p.d_model, device="cuda", generator=g) * 2 - 1)
    inner, w = p.inner_dim, {}
    w["shared"], w["ones"], w["final_ln"] = u(p.vocab_size, p.d_model, 1.0), torch.ones(p.d_model, device="cuda"), ln()
    for i in range(p.num_layers):
        w[f"{i}.qkv"] = torch.cat([u(2 * inner, p.d_model, math.sqrt(0.75 / p.d_model)), u(inner, p.d_model, p.d_model ** -0.5)])
        w[f"{i}.o"] = u(p.d_model, inner, inner ** -0.5)
        w[f"{i}.wi"] = u(2 * p.d_ff, p.d_model, math.sqrt(3.0 / p.d_model))
        w[f"{i}.wo"] = u(p.d_model, p.d_ff, p.d_ff ** -0.5)
        w[f"{i}.ln0"], w[f"{i}.ln1"] = ln(), ln()
    enc.w = w
    enc.tensors["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"] = \
        (torch.rand(p.relative_attention_num_buckets, p.num_heads) * 8 - 4).to(torch.bfloat16).float()
    enc.loaded = True
    return enc


def torch_forward(enc, ids):
    """The same network on torch's bf16 ops (bf16 residual stream, as transformers runs the checkpoint)."""
    import torch
    import torch.nn.functional as F
    p, w = enc.params, enc.w
    n, L = ids.shape
    bias = enc._device_bias(L).to(torch.bfloat16)
    idx = torch.arange(L, device="cuda")
    rel = bias[:, idx[None, :] - idx[:, None] + L - 1][None]

    def norm(x, g):
        v = x.float()
        return (v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + p.layer_norm_epsilon)).to(torch.bfloat16) * g.to(torch.bfloat16)
    x = w["shared"][ids.reshape(-1)]
    for i in range(p.num_layers):
        q, k, v = (norm(x, w[f"{i}.ln0"]) @ w[f"{i}.qkv"].t()).view(n, L, 3, p.num_heads, 64).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=rel, scale=1.0)
        x = x + a.permute(0, 2, 1, 3).reshape(n * L, -1) @ w[f"{i}.o"].t()
        h = norm(x, w[f"{i}.ln1"]) @ w[f"{i}.wi"].t()
        x = x + (F.gelu(h[:, p.d_ff:], approximate="tanh") * h[:, : p.d_ff]) @ w[f"{i}.wo"].t()
    return norm(x, w["final_ln"]).view(n, L, -1)


def family_shares(enc, ids):
    """HIP-event time between consecutive launches of one forward, summed per kernel family."""
    import torch
    from conceptattention_amd import ops
    marks = []
    names = {"gemm": "gemm", "t5_attention": "attention", "t5_rmsnorm": "rmsnorm", "gated_mul": "gated_mul",
             "embed_rows": "embed"}
    saved = {n: getattr(ops, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            saved[n](*a, **k)
            e1.record()
            marks.append((names[n], e0, e1))
        return f
    try:
        for n in names:
            setattr(ops, n, wrap(n))
        enc.encode_ids(ids)
        torch.cuda.synchronize()
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
    ms = {}
    for fam, e0, e1 in marks:
        ms[fam] = ms.get(fam, 0.0) + e0.elapsed_time(e1)
    total = sum(ms.values())
    return {k: round(v / total, 3) for k, v in sorted(ms.items(), key=lambda kv: -kv[1])}


def step(L):
    import torch
    from conceptattention_amd.params import t5_params
    p = t5_params["t5-v1_1-xxl"]
    enc = device_encoder(p)
    ids = torch.zeros(N_SEQ, L, dtype=torch.long)
    ids[:, :12] = torch.randint(2, p.vocab_size, (N_SEQ, 12), generator=torch.Generator().manual_seed(1))
    dev_ids = ids.cuda()
    with torch.no_grad():
        hip = timed(lambda: enc.encode_ids(ids))
        ref = timed(lambda: torch_forward(enc, dev_ids))
        a, b = enc.encode_ids(ids).float(), torch_forward(enc, dev_ids).float()
        shares = family_shares(enc, ids)
    weight_gb = sum(t.numel() * t.element_size() for k, t in enc.w.items() if k != "shared") / 1e9
    print(json.dumps({"tokens": f"{N_SEQ}x{L}", "hip_ms": round(hip, 2), "torch_bf16_ms": round(ref, 2),
                      "weights_gb": round(weight_gb, 2), "weight_stream_gb_per_s": round(weight_gb / hip * 1e3, 1),
                      "rel_rms_vs_torch_bf16": round(float(((a - b).pow(2).mean() / b.pow(2).mean()).sqrt()), 5),
                      "share_of_hip_time": shares}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 2:
        step(int(sys.argv[1]))
    else:
        for L in (256, 512):
            rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), str(L)])
            if rc != 0:
                sys.exit(f"L={L} ended with {rc}")   # nothing more is started on the GPU
