"""HIP-event time of the autoencoder's 1024 x 1024 decode and encode at B = 1, and beside it the same network run
by torch in bf16 (the restatement of tests/vae_ref.py) in the same process, as the yardstick.  Warm-up, then the median
of the repeats.  Each step is a process of its own under its own time limit:
    python tools/vae_throughput.py            # runs every step: `timeout ... python tools/vae_throughput.py STEP B`
    python tools/vae_throughput.py decode 1   # one step, one JSON line"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def step(what, B):
    import torch
    import vae_ref
    from conceptattention_amd import ae_params
    from conceptattention_amd.vae import AutoEncoder, synthetic_ae_state_dict
    p = ae_params["flux-schnell"]
    sd = synthetic_ae_state_dict(p, 0)
    ae = AutoEncoder(p, "cuda")
    ae.load_state_dict(sd)
    sdb = {k: v.to("cuda", torch.bfloat16) for k, v in sd.items()}
    z = torch.randn(B, 16, 128, 128, device="cuda")
    x = torch.rand(B, 3, 1024, 1024, device="cuda") * 2 - 1
    with torch.no_grad():
        if what == "decode":
            hip = timed(lambda: ae.decode(z))
            ref = timed(lambda: vae_ref.decode(sdb, z.to(torch.bfloat16)))
        else:
            hip = timed(lambda: ae.encoder_moments(x))
            ref = timed(lambda: vae_ref.encoder(sdb, x.to(torch.bfloat16)))
    print(json.dumps({"step": what, "B": B, "hip_ms": round(hip, 2), "torch_bf16_ms": round(ref, 2)}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3:
        step(sys.argv[1], int(sys.argv[2]))
    else:
        for what in ("decode", "encode"):
            for B in (1,):
                rc = subprocess.call(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), what, str(B)])
                if rc != 0:
                    sys.exit(f"{what} B={B} ended with {rc}")   # nothing more is started on the GPU
