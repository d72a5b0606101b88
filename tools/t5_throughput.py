"""HIP-event time of the T5 encoder at the real geometry (t5-v1_1-xxl: 24 blocks, d_model 4096, 64 heads, d_ff 10240)
for the 1 + 4 strings of one generate_image call -- 5 x 256 tokens (schnell) and 5 x 512 (dev) -- beside the same
network on plain torch bf16 ops in the same process, and the share of the HIP time per kernel family.  The weights are
drawn on the device straight into the packed operands (the CPU generator would have to produce 4.7 G values).  Warm-up,
then the median of the repeats.  Each step is a process of its own under its own time limit:
    python tools/t5_throughput.py          # runs every step: `timeout ... python tools/t5_throughput.py L`
    python tools/t5_throughput.py 256      # one step, one JSON line
    python tools/t5_throughput.py --precision fp8          # 1 x 256, 5 x 256 and 5 x 512 tokens, each its own process
    python tools/t5_throughput.py --precision fp8 1x256    # one step: the fp8 mode beside the bf16 mode, same process
With ``--precision fp8`` a step times ``T5Encoder(precision="fp8")`` (the same weights, quantised per output row)
against the bf16 encoder in one process and prints both family breakdowns; the plain torch network is not run.
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
             "embed_rows": "embed", "t5_rmsnorm_fp8": "rmsnorm_fp8", "gated_mul_fp8": "gated_mul_fp8",
             "quantize_rows_fp8": "quantize_rows_fp8"}
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


def fp8_encoder(bf):
    """The fp8-mode twin of a bf16 encoder: the same operands, quantised per output row as T5Encoder._pack does."""
    from conceptattention_amd import ops
    from conceptattention_amd.t5 import FP8_PROJECTIONS, T5Encoder
    enc = T5Encoder(bf.params, "cuda", precision="fp8")
    w = {}
    for k, t in bf.w.items():
        if k.split(".")[-1] in FP8_PROJECTIONS:
            w[k], w[k + ".scale"] = ops.quantize_rows_fp8(t)
        else:
            w[k] = t
    enc.w, enc.tensors, enc.loaded = w, bf.tensors, True
    return enc


def step_fp8(n_seq, L):
    import torch
    from conceptattention_amd.params import t5_params
    p = t5_params["t5-v1_1-xxl"]
    bf = device_encoder(p)
    f8 = fp8_encoder(bf)
    ids = torch.zeros(n_seq, L, dtype=torch.long)
    ids[:, :12] = torch.randint(2, p.vocab_size, (n_seq, 12), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ms = {"bf16": timed(lambda: bf.encode_ids(ids)), "fp8": timed(lambda: f8.encode_ids(ids))}
        ms["bf16_again"] = timed(lambda: bf.encode_ids(ids))        # the drift of the box between the two measurements
        a, b = f8.encode_ids(ids).float(), bf.encode_ids(ids).float()
        shares = {"bf16": family_shares(bf, ids), "fp8": family_shares(f8, ids)}
    print(json.dumps({"tokens": f"{n_seq}x{L}", "bf16_ms": round(ms["bf16"], 2), "fp8_ms": round(ms["fp8"], 2),
                      "bf16_again_ms": round(ms["bf16_again"], 2), "fp8_over_bf16": round(ms["fp8"] / ms["bf16"], 3),
                      "weights_gb": {"bf16": round(bf.weight_bytes(False) / 1e9, 2), "fp8": round(f8.weight_bytes(False) / 1e9, 2)},
                      "workspace_mb": {"bf16": round(bf.workspace_bytes() / 1e6, 1), "fp8": round(f8.workspace_bytes() / 1e6, 1)},
                      "rel_rms_fp8_vs_bf16": round(float(((a - b).pow(2).mean() / b.pow(2).mean()).sqrt()), 5),
                      "share_of_hip_time": shares}), flush=True)


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
    args = sys.argv[1:]
    precision = "bf16"
    if "--precision" in args:
        i = args.index("--precision")
        precision = args[i + 1]
        del args[i:i + 2]
    if precision not in ("bf16", "fp8") or len(args) > 1:
        sys.exit("usage: t5_throughput.py [--precision bf16|fp8] [L | NxL]")
    if args and precision == "fp8":
        n, _, L = args[0].rpartition("x")
        step_fp8(int(n or N_SEQ), int(L))
    elif args:
        step(int(args[0]))
    else:
        steps = ("256", "512") if precision == "bf16" else ("1x256", "5x256", "5x512")
        for s in steps:
            rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--precision",
                                  precision, s])
            if rc != 0:
                sys.exit(f"{s} ended with {rc}")   # nothing more is started on the GPU
