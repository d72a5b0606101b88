"""HIP-event time of the CLIP text encoder at the real geometry (clip-vit-large-patch14's text model: 12 layers, hidden
768, 12 heads, intermediate 3072, 77 tokens) for 1 prompt (what one generate_image call encodes) and 5, beside the same
network on plain torch bf16 ops in the same process, and the share of the HIP time per kernel family.  Synthetic
weights (``synthetic_clip_state_dict``: 123 M values from the CPU generator).  Warm-up, then the median of the repeats.
Each step is a process of its own under its own time limit:
    python tools/clip_throughput.py        # runs every step: `timeout ... python tools/clip_throughput.py N`
    python tools/clip_throughput.py 5      # one step, one JSON line
No number printed here is a gate."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L_TOKENS = 77


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


def torch_forward(enc, ids, pooled):
    """The same network on torch's bf16 ops (bf16 residual stream, as transformers runs the checkpoint), all sequences
    in one batch."""
    import torch
    import torch.nn.functional as F
    p, w = enc.params, enc.w
    n, L = ids.shape
    d, bf = p.hidden_size, torch.bfloat16
    x = w["tok"][ids.reshape(-1)] + w["pos"][:L].repeat(n, 1)
    for i in range(p.num_hidden_layers):
        h = F.layer_norm(x, (d,), w[f"{i}.ln1.w"].to(bf), w[f"{i}.ln1.b"].to(bf), p.layer_norm_eps)
        q, k, v = F.linear(h, w[f"{i}.qkv"], w[f"{i}.qkv.b"]).view(n, L, 3, p.num_attention_heads, 64).permute(2, 0, 3, 1, 4)
        a = F.scaled_dot_product_attention(q, k, v, is_causal=True)
        x = x + F.linear(a.permute(0, 2, 1, 3).reshape(n * L, d), w[f"{i}.o"], w[f"{i}.o.b"])
        h = F.layer_norm(x, (d,), w[f"{i}.ln2.w"].to(bf), w[f"{i}.ln2.b"].to(bf), p.layer_norm_eps)
        u = F.linear(h, w[f"{i}.fc1"], w[f"{i}.fc1.b"])
        x = x + F.linear(u * torch.sigmoid(1.702 * u), w[f"{i}.fc2"], w[f"{i}.fc2.b"])
    x = F.layer_norm(x, (d,), w["final.w"].to(bf), w["final.b"].to(bf), p.layer_norm_eps).view(n, L, d)
    return x[torch.arange(n, device=x.device), pooled]


def family_shares(enc, ids):
    """HIP-event time between consecutive launches of one forward, summed per kernel family."""
    import torch
    from conceptattention_amd import ops
    marks = []
    names = {"gemm": "gemm", "clip_attention": "attention", "layernorm": "layernorm", "quick_gelu": "quick_gelu",
             "clip_embed": "embed"}
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


def step(n_seq):
    import torch
    from conceptattention_amd.clip import load_clip, pooled_positions
    from conceptattention_amd.params import clip_params
    p = clip_params["clip-vit-large-patch14"]
    enc = load_clip(p, "cuda", "synthetic")
    ids = torch.full((n_seq, L_TOKENS), p.vocab_size - 1, dtype=torch.long)      # padded with end-of-text, as CLIP's tokenizer pads
    ids[:, 0] = p.vocab_size - 2
    ids[:, 1:12] = torch.randint(1, p.vocab_size - 2, (n_seq, 11), generator=torch.Generator().manual_seed(1))
    dev_ids, pooled = ids.cuda(), pooled_positions(ids, p.eos_token_id).cuda()
    with torch.no_grad():
        hip = timed(lambda: enc.encode_ids(ids))
        ref = timed(lambda: torch_forward(enc, dev_ids, pooled))
        a, b = enc.encode_ids(ids).float(), torch_forward(enc, dev_ids, pooled).float()
        shares = family_shares(enc, ids)
    weight_gb = sum(t.numel() * t.element_size() for k, t in enc.w.items() if k != "tok") / 1e9
    print(json.dumps({"tokens": f"{n_seq}x{L_TOKENS}", "hip_ms": round(hip, 2), "torch_bf16_ms": round(ref, 2),
                      "weights_gb": round(weight_gb, 3),
                      "rel_rms_vs_torch_bf16": round(float(((a - b).pow(2).mean() / b.pow(2).mean()).sqrt()), 5),
                      "share_of_hip_time": shares}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 2:
        step(int(sys.argv[1]))
    else:
        for n in (1, 5):
            rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), str(n)])
            if rc != 0:
                sys.exit(f"n_seq={n} ended with {rc}")   # nothing more is started on the GPU
