"""Write tests/golden/t5_tiny.npz and t5_long.npz with transformers' own T5EncoderModel (the class the reference's
HFEmbedder wraps, flux/modules/conditioner.py:6-38).  Run from the repository root: python tests/tools/make_t5_golden.py

For each case of tests/t5_ref.CASES: ``synthetic_t5_state_dict`` is loaded with strict=True into a T5EncoderModel built
from the matching T5Config (this pins the key names and shapes), the fixed ids go through
``model(input_ids=ids, attention_mask=None)`` in fp32 and in bf16 (the reference's own precision), and the file keeps

  keys, shapes         the model's state-dict key list and shapes
  ids                  the input ids
  buckets              transformers' bucket for key - query = -511 .. 511
  rows                 the token rows kept, out_f32 [n_seq, len(rows), d_model] the fp32 output there
  bf16_err             the bf16 run's relative rms distance from the fp32 run: over all rows, over the token-0 rows
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import t5_ref  # noqa: E402
from conceptattention_amd.params import tiny_t5_params  # noqa: E402
from conceptattention_amd.t5 import TIED_EMBEDDING, synthetic_t5_state_dict  # noqa: E402


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float(torch.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))


def main():
    from transformers import T5Config, T5EncoderModel
    from transformers.models.t5.modeling_t5 import T5Attention
    for name, (geo, length, _) in t5_ref.CASES.items():
        p = tiny_t5_params(**geo)
        cfg = T5Config(vocab_size=p.vocab_size, d_model=p.d_model, d_kv=p.d_kv, d_ff=p.d_ff, num_layers=p.num_layers,
                       num_heads=p.num_heads, relative_attention_num_buckets=p.relative_attention_num_buckets,
                       relative_attention_max_distance=p.relative_attention_max_distance, dropout_rate=0.0,
                       layer_norm_epsilon=p.layer_norm_epsilon, feed_forward_proj="gated-gelu", is_encoder_decoder=False,
                       use_cache=False, tie_word_embeddings=False)
        model = T5EncoderModel(cfg).eval()
        sd = synthetic_t5_state_dict(p, 0)
        keys = list(model.state_dict().keys())
        if TIED_EMBEDDING in keys:          # the tied twin of shared.weight
            sd[TIED_EMBEDDING] = sd["shared.weight"]
        model.load_state_dict(sd, strict=True)
        ids = t5_ref.case_ids(name)
        with torch.no_grad():
            f32 = model(input_ids=ids, attention_mask=None).last_hidden_state
            b16 = model.to(torch.bfloat16)(input_ids=ids, attention_mask=None).last_hidden_state.float()
        off = torch.arange(-511, 512)
        buckets = T5Attention._relative_position_bucket(off, bidirectional=True, num_buckets=32, max_distance=128)
        rows = t5_ref.kept_rows(length)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        out = os.path.join(ROOT, "tests", "golden", f"t5_{name}.npz")
        np.savez_compressed(out, keys=np.array(keys), shapes=np.array([",".join(map(str, shapes[k])) for k in keys]),
                            ids=ids.numpy(), buckets=buckets.numpy().astype(np.int16), rows=np.array(rows),
                            out_f32=f32[:, rows].numpy(),
                            bf16_err=np.array([rel_rms(b16, f32), rel_rms(b16[:, 0], f32[:, 0])]))
        print(name, os.path.getsize(out), "bytes; bf16 run rel rms", rel_rms(b16, f32), "token 0", rel_rms(b16[:, 0], f32[:, 0]))


if __name__ == "__main__":
    main()
