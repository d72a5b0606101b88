"""The two e4m3 producers of the DiT's fp8 mode at the model's row shape (development aid): ca_quantize_rows_fp8 and
ca_ln_modulate_f32in_fp8 on the 21780 x 3072 rows of a five-item group (5 x (4 concept + 256 text + 4096 image rows), 15
modulation segments).  Several repeats per kernel: their spread is the margin of an A/B between two builds, each run in
a process of its own, alternating.  usage: python tools/fp8_producer_bench.py [lib.so]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) > 1:
    from conceptattention_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
import torch
from conceptattention_amd import ops
from tools.bench_kernels import rnd, timeit
B, C, T, Li, H = 5, 4, 256, 4096, 3072
n = B * (C + T + Li)
x16, x32 = rnd(n, H), torch.randn(n, H, device="cuda")
q, s = torch.empty(n, H, device="cuda", dtype=torch.uint8), torch.empty(n, device="cuda")
sh = [torch.randn(H, device="cuda") for _ in range(15)]
sc = [torch.randn(H, device="cuda") * 0.3 for _ in range(15)]
ends = [(j + 1) * C for j in range(B)] + [B * C + (j + 1) * T for j in range(B)] + [B * (C + T) + (j + 1) * Li for j in range(B)]
segs = [(e, sh[i], sc[i]) for i, e in enumerate(ends)]
for name, fn, nbytes in (("quantize_rows_fp8", lambda: ops.quantize_rows_fp8(x16, q, s), 2 + 1),
                         ("ln_modulate_f32in_fp8", lambda: ops.ln_modulate(x32, q, segs, out_scale=s), 4 + 1)):
    ts = [timeit(fn, iters=50) for _ in range(5)]
    print(f"{name} {n}x{H}: " + " ".join(f"{t * 1e6:.1f}" for t in ts) + f" us  (best {min(ts) * 1e6:.1f} us, "
          f"{n * H * nbytes / min(ts) / 1e9:.0f} GB/s)", flush=True)
