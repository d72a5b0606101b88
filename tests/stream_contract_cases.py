"""The probes of tests/test_stream_contract_gpu.py, part a: one small case per launch form of every entry point of
include/conceptattn.h that takes a stream, taken from the existing case tables, each with the entry points it expects
conceptattention_amd._lib.check to see, in order.  Nothing here needs a GPU: tests/test_stream_contract_cpu.py compares
the probed set with the header."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass

import address_range_cases as C
import clip_cases as CL
import gemm_route_cases as G
import rowop_cases as R
import vae_cases as V

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "conceptattn.h")
# entry points `check` also sees that take no stream (plans and counters): not part of the record that is compared
NO_STREAM = {"ca_gemm_plan", "ca_gemm_auto_tile", "ca_attn_stats"}

# ops wrappers that wait for the stream on purpose, and why (INTEGRATION.md names the same three).  Their C entry points
# are probed directly with device ids and must meet the contract; the wrappers must still give the right bytes.
WAITS_BY_DESIGN = {
    "embed_rows": "range-checks the ids on the host (int(ids.min()), int(ids.max())) before the launch",
    "clip_embed": "range-checks the ids on the host (int(ids.min()), int(ids.max())) before the launch",
    "layernorm(row_idx=...)": "range-checks row_idx on the host (int(row_idx.min()), int(row_idx.max())) before the launch",
}


@dataclass(frozen=True)
class Probe:
    id: str
    family: str            # which runner of the GPU file takes `arg`
    arg: object            # the case of the existing table (an id, a case object or a tuple, as that table's helper takes it)
    entries: tuple         # what check records, in order (NO_STREAM names left out)
    wrapper: str = None    # the key of WAITS_BY_DESIGN when the run goes through such a wrapper
    direct: bool = False   # the C entry point through L.load(), device ids, in place of the wrapper

    def __repr__(self):
        return self.id


def stream_entry_points(header: str = HEADER) -> set:
    """The functions of include/conceptattn.h whose declaration has a ca_stream_t parameter."""
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    out = set()
    for m in re.finditer(r"\bint\s+(ca_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if "ca_stream_t" in m.group(2):
            out.add(m.group(1))
    return out


def gemm_probes() -> list:
    """Every route of gemm_route_cases.ROUTES at K = 128 with one epilogue each; the routes walk round GEMM_EPIS, so that
    all four are used (a route that cannot take its turn's epilogue takes the next one it can)."""
    out = []
    for i, route in enumerate(G.ROUTES):
        epis = C.gemm_epis_for(route)
        epi = next(C.GEMM_EPIS[(i + j) % 4] for j in range(4) if C.GEMM_EPIS[(i + j) % 4] in epis)
        out.append(Probe(f"gemm-{route}-{epi}", "gemm", (route, epi),
                         ("ca_gemm_fp8" if G.ROUTES[route].fp8 else "ca_gemm_bf16",)))
    return out


def _first_per_form(cases) -> list:
    seen, out = set(), []
    for c in cases:
        if (c.entry, c.kernel) not in seen and not c.shape.get("big"):
            seen.add((c.entry, c.kernel))
            out.append(c)
    return out


ATTN_ENTRY = {"ca_attn_kernel<8>": "ca_attn_fwd_bf16", "ca_attn4_kernel": "ca_attn_fwd_bf16",
              "ca_attn4_qk16_kernel": "ca_attn_fwd_qk16"}
RENDER_CASES = {"bilinear-blend": "blend-alpha0.5", "nearest": "family-heat-nearest"}
SEGTAB_CASE = "flags-mean-down-blur"
# the helpers of these two launch twice (the second time in place, as the models do)
_TWICE = {"ca_gated_mul_bf16", "ca_quick_gelu_bf16"}
_WRAPPER = {"ca_embed_rows_f32": "embed_rows", "ca_clip_embed_f32": "clip_embed", "ca_layernorm_f32in": "layernorm(row_idx=...)"}


def text_probes() -> list:
    out = []
    for entry, case in C.TEXT_PLACEMENT.items():
        n = 2 if entry in _TWICE else 1
        if entry in _WRAPPER:
            out.append(Probe(f"text-{entry}-wrapper", "text", (entry, case), (entry,), wrapper=_WRAPPER[entry]))
            out.append(Probe(f"text-{entry}-direct", "text", (entry, case), (entry,), direct=True))
        else:
            out.append(Probe(f"text-{entry}", "text", (entry, case), (entry,) * n))
    # layernorm row by row (no row_idx): the wrapper has nothing to read on the host
    out.append(Probe("text-ca_layernorm_f32in-rows", "text", ("ca_layernorm_f32in", (256, CL.LN_ROWS, False)),
                     ("ca_layernorm_f32in",)))
    return out


def all_probes() -> list:
    out = gemm_probes()
    out += [Probe(f"attn-{k}", "attn", cid, (ATTN_ENTRY[k],)) for k, cid in C.ATTN_PLACEMENT.items()]
    out += [Probe(f"rowop-{c.id}", "rowop", c.id, (c.entry,)) for c in _first_per_form(R.CASES)]
    out += [Probe(f"vae-{c.id}", "vae", c.id, (c.entry,)) for c in _first_per_form(V.CASES)]
    out += text_probes()
    out.append(Probe("segtab", "segtab", SEGTAB_CASE, ("ca_segtab_score",)))
    out.append(Probe("mseg", "mseg", None, ("ca_mseg_score",)))
    out += [Probe(f"render-{k}", "render", name, ("ca_heatmap_render",)) for k, name in RENDER_CASES.items()]
    return out


PROBES = all_probes()
