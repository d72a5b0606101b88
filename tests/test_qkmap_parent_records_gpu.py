"""ca_token_maps and ca_query_maps against the bytes they wrote BEFORE their shared device code and entry checks moved
into csrc/ca_qkmap_core.h and their host plumbing into one builder (ops.py) and one launch splitter (flux_dit.py).

tests/golden/qkmap_parent_records.npz holds what the two entries, their ops wrappers and the model's capture wrote on an
MI355X for seeded inputs, recorded from the commit before the move (``record`` below wrote it; only outputs are stored).
Per family three arrays, as in tests/test_text_parent_records_gpu.py: ``<family>.sha`` uint8 [outputs, 32], the SHA-256 of
each output's bytes in the order ``computed`` yields them; ``<family>.len`` int32 [outputs], the byte count of every
output of at most 4 KB (0 for a larger one); ``<family>.bytes``, those outputs' bytes one after the other, so that a
failure can be read.  A NaN compares as a NaN (every NaN is replaced by one pattern before the bytes are taken);
everything else compares by bits.

  ``tokmap_cases``    every case of tokmap_cases.CASES launched alone: acc (from its seeded non-zero start, weight W1),
                      acc2 (the case module's second accumulator, weight W2) and lse after the call.
  ``querymap_cases``  the same for every case of querymap_cases.CASES, with the outputs the case asks for.
  ``launch_split``    17 problems in ONE ops.token_maps call (heads 1, nq 65, n0 4, n1 60, n_tok 3) and 17 in ONE
                      ops.query_maps call (heads 1, nq 17, n0 4, n1 65; workspace=None, so the wrapper sizes the one
                      buffer both of its launches share): the split after 16 problems.  The families and layouts
                      alternate and problem i's acc starts i higher; the 17 problems' acc, acc2 and lse are recorded
                      as one stacked output each.
  ``tiny_model``      HipFluxDiT on the tiny geometry of tests/test_querymap_model_gpu.py, one forward of two items that
                      captures both double blocks, asking for the token maps (5 tokens) and both kinds of query maps (8
                      and 3 text rows; the 3 concept rows), each with its per-layer table.  The two items share ONE
                      token_space and ONE concept_query_space, so both captures split their launch on the shared
                      accumulator; every accumulator and table is recorded, and the latent.

The inputs come from the case modules, generated on the CPU from their seeds."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import querymap_cases as Q  # noqa: E402
import tokmap_cases as T  # noqa: E402
from conceptattention_amd import ops  # noqa: E402

DEV = "cuda"
NAN = float("nan")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qkmap_parent_records.npz")
KEEP = 4096                                   # an output of at most this many bytes is stored whole
FAMILIES = ("tokmap_cases", "querymap_cases", "launch_split", "tiny_model")
SPLIT_N = 17                                  # one more than a launch takes
OUTS = ("acc", "acc2", "lse")


def canonical_bytes(t: torch.Tensor) -> bytes:
    """The bytes of a device tensor with every NaN replaced by one pattern."""
    t = t.detach().contiguous()
    t = torch.where(torch.isnan(t), torch.full_like(t, NAN), t)
    return t.cpu().view(torch.uint8).numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------- launches
def _place(mod, case, outs):
    """(q, k0, k1 as bf16-typed device views of the case's buffers, {name: output tensor at the case's start})."""
    inp = mod.make_inputs(case)
    bufs = {name: b.to(DEV) for name, b in inp["buffers"].items()}
    q, k0, k1 = (mod.view(case, bufs, name).view(torch.bfloat16) for name in ("q", "k0", "k1"))
    start = {"acc": lambda: inp["acc0"].to(DEV), "acc2": lambda: inp["acc20"].to(DEV),
             "lse": lambda: torch.full((case.heads, case.nq), NAN, device=DEV)}
    return q, k0, k1, {name: start[name]() for name in outs}


def _token_problem(case):
    q, k0, k1, out = _place(T, case, OUTS)
    return ops.TokenMaps(q, k0, k1 if case.n1 else None, case.n_tok, acc=out["acc"], weight=T.W1, acc2=out["acc2"],
                         weight2=T.W2, lse=out["lse"]), out


def _query_problem(case):
    q, k0, k1, out = _place(Q, case, case.outs)
    return ops.QueryMaps(q, k0 if case.n0 else None, k1, acc=out.get("acc"), weight=Q.W1, acc2=out.get("acc2"),
                         weight2=Q.W2, lse=out.get("lse")), out


def _call(fn, problems, case):
    fn(problems, case.heads, case.scale_log2, qk_f16=case.f16)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- families
def _tokmap_cases_family():
    for case in T.CASES:
        pr, out = _token_problem(case)
        _call(ops.token_maps, [pr], case)
        yield "token_maps " + case.id, [out[k] for k in OUTS]


def _querymap_cases_family():
    for case in Q.CASES:
        pr, out = _query_problem(case)
        _call(ops.query_maps, [pr], case)
        yield "query_maps " + case.id, [out[k] for k in case.outs]


def _launch_split_family():
    fams = ("unit", "peaky8")
    tok = [T.Case(heads=1, nq=65, n0=4, n_tok=3, n1=60, f16=False, family=fams[i & 1], layout=("qkv", "apart")[i >> 1 & 1],
                  prescaled=False) for i in range(SPLIT_N)]
    qry = [Q.Case(heads=1, nq=17, n0=4, n1=65, f16=False, family=fams[i & 1], layout=("qkv", "apart0", "apart1", "apart2")[i >> 1 & 3],
                  prescaled=False) for i in range(SPLIT_N)]
    for fn, cases, make in ((ops.token_maps, tok, _token_problem), (ops.query_maps, qry, _query_problem)):
        placed = [make(c) for c in cases]
        for i, (_, out) in enumerate(placed):       # (a case's seed is its id: problems of one family and layout are told
            out["acc"] += float(i)                  # apart by their accumulator's start)
        _call(fn, [pr for pr, _ in placed], cases[0])
        # (one output per name for the whole call: SHA-256 only, which keeps the fixture small)
        yield f"{fn.__name__} {SPLIT_N} problems", [torch.stack([out[k] for _, out in placed]) for k in OUTS]


def _tiny_model_family():
    import test_model_routes_gpu as TM
    import test_querymap_model_gpu as QM
    from conceptattention_amd.flux_dit import HeatmapRequest
    case = QM.case_of(2, (0, 1))
    nl, C, Li = len(case.layers), case.C, case.L
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    token_space, concept_query_space = z(5, Li), z(C, Li)          # shared by the two items
    reqs = [HeatmapRequest(tuple(case.layers), 0.5, z(C, Li), z(C, Li), per_layer_weight=0.75,
                           token_space=token_space, per_layer_token=z(nl, 5, Li),
                           token_query_space=z(n_tok, Li), per_layer_token_query=z(nl, n_tok, Li),
                           concept_query_space=concept_query_space, per_layer_concept_query=z(nl, C, Li))
            for n_tok in (8, 3)]
    pred = QM.run_model(TM.build(case), case, reqs, stop=False)
    yield "latent", pred
    yield "shared token_space", token_space
    yield "shared concept_query_space", concept_query_space
    for j, r in enumerate(reqs):
        for f in ("out_space", "cross_space", "per_layer_token", "token_query_space", "per_layer_token_query",
                  "per_layer_concept_query"):
            yield f"item {j} {f}", getattr(r, f)
    assert float(token_space.min()) > 0 and float(concept_query_space.min()) > 0


GENERATORS = {"tokmap_cases": _tokmap_cases_family, "querymap_cases": _querymap_cases_family,
              "launch_split": _launch_split_family, "tiny_model": _tiny_model_family}


@functools.lru_cache(maxsize=None)
def computed(family: str):
    """(names, sha uint8 [n, 32], len int32 [n], bytes uint8) of what the library in this tree writes for one family."""
    names, sha, lens, kept = [], [], [], []
    for name, outs in GENERATORS[family]():
        for i, t in enumerate(outs if isinstance(outs, list) else [outs]):
            raw = canonical_bytes(t)
            names.append(f"{name} [{i}]")
            sha.append(np.frombuffer(hashlib.sha256(raw).digest(), dtype=np.uint8))
            lens.append(len(raw) if len(raw) <= KEEP else 0)
            if len(raw) <= KEEP:
                kept.append(np.frombuffer(raw, dtype=np.uint8))
    return names, np.stack(sha), np.array(lens, dtype=np.int32), np.concatenate(kept) if kept else np.zeros(0, np.uint8)


def record(path: str) -> None:
    """Write the fixture from the library in this tree (run once, on the commit before the move)."""
    arrays = {}
    for f in FAMILIES:
        _, arrays[f + ".sha"], arrays[f + ".len"], arrays[f + ".bytes"] = computed(f)
    np.savez_compressed(path, **arrays)


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE)


@pytest.mark.parametrize("family", FAMILIES)
def test_the_outputs_are_the_parents_bit_for_bit(parent, family):
    names, sha, lens, kept = computed(family)
    print(family, len(names), "outputs,", int((lens > 0).sum()), "stored whole")
    assert sha.shape == parent[family + ".sha"].shape and np.array_equal(lens, parent[family + ".len"]), family
    ends = np.cumsum(lens)
    for i, name in enumerate(names):
        if lens[i]:         # readable: the first bytes that differ
            a, b = kept[ends[i] - lens[i]:ends[i]], parent[family + ".bytes"][ends[i] - lens[i]:ends[i]]
            assert np.array_equal(a, b), (name, np.nonzero(a != b)[0][:8], a[a != b][:8], b[a != b][:8])
        assert np.array_equal(sha[i], parent[family + ".sha"][i]), name
