"""Write tests/golden/vae_*.npz from the reference's own AutoEncoder class (flux/modules/autoencoder.py), loaded with
``synthetic_ae_state_dict``: its fp32 decode output and encoder moments, the same under ``torch.autocast(bfloat16)``
(whose distance from fp32 is the parity yardstick of tests/test_vae_model_gpu.py), input checksums and the reference's
key names and shapes.  CPU only.  Usage: python tools/make_vae_goldens.py [REFERENCE_ROOT] [--full]"""
import dataclasses
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vae_ref  # noqa: E402
from conceptattention_amd.params import AutoEncoderParams  # noqa: E402
from conceptattention_amd.vae import synthetic_ae_state_dict  # noqa: E402


def reference_class(ref_root):
    pkg = types.ModuleType("concept_attention")       # the package itself fails to import (entmax); its path is enough
    pkg.__path__ = [os.path.join(ref_root, "concept_attention")]
    sys.modules["concept_attention"] = pkg
    from concept_attention.flux.src.flux.modules import autoencoder
    return autoencoder


def run(ref, name, ch, B, h, w, step, parts=("decode", "encode")):
    p = AutoEncoderParams(ch=ch)
    sd = synthetic_ae_state_dict(p, seed=0)
    kw = dataclasses.asdict(p)
    kw["ch_mult"] = list(p.ch_mult)
    model = ref.AutoEncoder(ref.AutoEncoderParams(**kw)).eval()
    model.load_state_dict(sd, strict=True)
    z, x = vae_ref.case_inputs(name, ch, B, h, w)
    keys = list(model.state_dict().keys())
    out = {"keys": np.array(keys), "shapes": np.array([",".join(map(str, model.state_dict()[k].shape)) for k in keys]),
           "geometry": np.array([ch, B, h, w, step]), "z_checksum": vae_ref.checksum(z), "x_checksum": vae_ref.checksum(x)}
    with torch.no_grad():
        for part, fn, inp in (("decode", model.decode, z), ("encode", model.encoder, x)):
            if part not in parts:
                continue
            f32 = fn(inp)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                b16 = fn(inp).float()
            f32s, b16s = vae_ref.subsample(f32.numpy(), step), vae_ref.subsample(b16.numpy(), step)
            key = "dec" if part == "decode" else "mom"
            out[key + "_f32"] = f32s
            out[key + "_bf16_err"] = np.array(vae_ref.errors(b16s, f32s))
            out[key + "_range"] = np.array([f32.min().item(), f32.max().item()])
            print(name, part, tuple(f32.shape), "range", out[key + "_range"], "bf16 err (max-abs, rel-rms)",
                  out[key + "_bf16_err"], flush=True)
    path = os.path.join(ROOT, "tests", "golden", f"vae_{name}.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    ref = reference_class(args[0] if args else os.environ.get("CA_REFERENCE_ROOT", "reference"))
    torch.manual_seed(0)
    if "--full" in sys.argv:
        for part, (ch, B, h, w, step) in vae_ref.FULL.items():
            run(ref, "full_" + part, ch, B, h, w, step, parts=(part,))
    else:
        for name, (ch, B, h, w, step) in vae_ref.CASES.items():
            run(ref, name, ch, B, h, w, step)
