"""Write tests/golden/clip_tiny.npz and clip_eos.npz with transformers' own CLIPTextModel (the class the reference's
HFEmbedder wraps for its CLIP side).  Run from the repository root: python tests/tools/make_clip_golden.py

For each case of tests/clip_ref.CASES: ``synthetic_clip_state_dict`` is loaded with strict=True into a CLIPTextModel
built from the matching CLIPTextConfig (this pins the key names and shapes), the fixed ids go through
``model(input_ids=ids, attention_mask=None)`` in fp32 and in bf16 (the reference's own precision), and the file keeps

  keys, shapes         the model's state-dict key list and shapes
  ids                  the input ids;  pooled: the row transformers pooled per sequence (recovered from its outputs)
  pooler_f32           the fp32 pooler_output [n_seq, hidden]
  rows                 the token rows kept (every 4th and every pooled one), hidden_f32 [n_seq, len(rows), hidden] the
                       fp32 last_hidden_state there
  bf16_err             the bf16 run's relative rms distance from the fp32 run: over the kept rows, over the pooled rows
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import clip_ref  # noqa: E402
from conceptattention_amd.clip import synthetic_clip_state_dict  # noqa: E402
from conceptattention_amd.params import tiny_clip_params  # noqa: E402


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float(torch.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


def main():
    from transformers import CLIPTextConfig, CLIPTextModel
    for name, (geo, length, _, eos_token_id, (bos, eos, pad)) in clip_ref.CASES.items():
        p = tiny_clip_params(**geo)
        cfg = CLIPTextConfig(vocab_size=p.vocab_size, hidden_size=p.hidden_size, intermediate_size=p.intermediate_size,
                             num_hidden_layers=p.num_hidden_layers, num_attention_heads=p.num_attention_heads,
                             max_position_embeddings=p.max_position_embeddings, hidden_act="quick_gelu",
                             layer_norm_eps=p.layer_norm_eps, attention_dropout=0.0, projection_dim=p.hidden_size,
                             pad_token_id=pad, bos_token_id=bos, eos_token_id=eos_token_id)
        model = CLIPTextModel(cfg).eval()
        assert cfg.eos_token_id == eos_token_id
        model.load_state_dict(synthetic_clip_state_dict(p, 0), strict=True)
        ids = clip_ref.case_ids(name)
        with torch.no_grad():
            o32 = model(input_ids=ids, attention_mask=None)
            o16 = model.to(torch.bfloat16)(input_ids=ids, attention_mask=None)
        h32, p32 = o32.last_hidden_state, o32.pooler_output
        h16, p16 = o16.last_hidden_state.float(), o16.pooler_output.float()
        pooled = [int((h32[s] == p32[s]).all(-1).nonzero()[0, 0]) for s in range(ids.shape[0])]
        rows = clip_ref.kept_rows(length, pooled)
        keys = list(model.state_dict().keys())
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        out = os.path.join(ROOT, "tests", "golden", f"clip_{name}.npz")
        err = np.array([rel_rms(h16[:, rows], h32[:, rows]), rel_rms(p16, p32)])
        np.savez_compressed(out, keys=np.array(keys), shapes=np.array([",".join(map(str, shapes[k])) for k in keys]),
                            ids=ids.numpy().astype(np.int32), pooled=np.array(pooled), pooler_f32=p32.numpy(),
                            rows=np.array(rows), hidden_f32=h32[:, rows].numpy(), bf16_err=err)
        print(name, os.path.getsize(out), "bytes; pooled rows", pooled, "; bf16 run rel rms", err)


if __name__ == "__main__":
    main()
