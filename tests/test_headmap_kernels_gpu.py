"""ca_head_maps on the device, every case of tests/headmap_cases.py: every value inside the derived bound of the fp64
reference, a second launch over the restored accumulators giving the same bits, a patch's results bit-identical at
position 0 and 200 of a longer problem and alone versus among 16 problems; at norm = none NH x acc2 against
ops.heatmap_logits, and with one head of 128 columns acc against ops.heatmap_fused on the same rows.

Every buffer a launch sees is cut out of a larger allocation with GUARD elements of NaN on both sides and the vectors'
padding columns hold NaN: a guard or a padding column must come back byte for byte.  max err / bound is printed
(pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import headmap_cases as H  # noqa: E402
import rowop_cases as R  # noqa: E402
from conceptattention_amd import _lib as L  # noqa: E402
from conceptattention_amd import ops  # noqa: E402
from test_heatmap_many_kernels_gpu import Guarded, _bytes, assert_same_bits  # noqa: E402

DEV = "cuda"
NORM = {"none": L.NORM_NONE, **L.NORMS}
START = {"heads": "heads0", "acc": "acc0", "acc2": "acc20"}
_REF = {}                                      # case id -> (inputs, fp64 reference): computed once, shared, never changed


def inputs_and_reference(case):
    if case.id not in _REF:
        inp = H.make_inputs(case)
        _REF[case.id] = (inp, H.reference(case, inp, dev=DEV))
    return _REF[case.id]


def place(case, inp, al, only=None):
    """The device operands of every problem (`only`: that problem alone): the padded vectors and the accumulators' start
    values."""
    s = case.shape
    dev = []
    for i, pr in enumerate(inp["probs"]):
        if only is not None and i != only:
            continue
        d = dict(img=al.to(pr["img"], {f"img[{i}]": None}), con=al.to(pr["con"], {f"con[{i}]": None}))
        for name in H.OUTS[s["outs"]]:
            d[name] = al.to(pr[START[name]], {f"{name}[{i}]": None})
        dev.append(d)
    return dev


def problems(case, dev):
    W = case.shape["dim"]
    return [ops.HeadMaps(d["img"][:, :W], d["con"][:, :W], heads=d.get("heads"), weight_h=H.WH, acc=d.get("acc"),
                         weight=H.W1, acc2=d.get("acc2"), weight2=H.W2) for d in dev]


def outputs(dev):
    return [{k: v for k, v in d.items() if k in START} for d in dev]


def run(case, inp, al, only=None):
    dev = place(case, inp, al, only)
    before = [(d["img"].clone(), d["con"].clone()) for d in dev]
    ops.head_maps(problems(case, dev), case.shape["NH"], NORM[case.shape["norm"]])
    torch.cuda.synchronize()
    al.check_guards()
    for d, (i0, c0) in zip(dev, before):                       # the inputs and their NaN padding: byte for byte
        assert torch.equal(_bytes(d["img"]), _bytes(i0)) and torch.equal(_bytes(d["con"]), _bytes(c0))
    return outputs(dev)


@pytest.mark.parametrize("case", H.CASES, ids=lambda c: c.id)
def test_every_case_against_fp64_and_a_second_launch(case):
    inp, ref = inputs_and_reference(case)
    got = run(case, inp, Guarded())
    worst, n_over = H.over_the_bound(got, ref)
    print(f"\n  {case.id}: {case.kernel}  max err / bound = {worst:.3f}")
    assert_same_bits(got, run(case, inp, Guarded()), "second launch over the restored accumulators")
    assert n_over == 0, f"{case.id}: {n_over} elements over the bound (NaN = never written), max err / bound {worst:.3g}"


@pytest.mark.parametrize("cid", ["heads_NH4_L257_C16_sparsemax_n16_all", "heads_NH5_L257_C17_none_n16_all",
                                 "heads_NH1_L257_C8_softmax_n16_all"])
def test_a_problem_alone_gives_the_bits_it_gives_among_16(cid):
    case = H.BY_ID[cid]
    inp, _ = inputs_and_reference(case)
    together = run(case, inp, Guarded())
    for i in (0, 7, 15):
        assert_same_bits([together[i]], run(case, inp, Guarded(), only=i), f"problem {i} alone")


@pytest.mark.parametrize("norm", H.NORMS)
@pytest.mark.parametrize("C", [8, 17])
def test_a_patch_gives_the_same_bits_at_position_0_and_200(C, norm):
    """The rows of 5 patches at positions 0 .. 4 of a 5-patch problem and at 200 .. 204 of a 257-patch one (another
    workgroup, another wave, the other patch slot of a wave)."""
    NH, Lp = 5, 257
    g = torch.Generator().manual_seed(40 + C)
    img = torch.randn(Lp, NH * 128, generator=g).bfloat16().to(DEV)
    con = (torch.randn(C, NH * 128, generator=g) * 0.13).to(DEV)
    small = img[:5].clone()
    img[200:205] = small
    big = dict(heads=torch.zeros(NH, C, Lp, device=DEV), acc=torch.zeros(C, Lp, device=DEV))
    few = dict(heads=torch.zeros(NH, C, 5, device=DEV), acc=torch.zeros(C, 5, device=DEV))
    ops.head_maps([ops.HeadMaps(img, con, heads=big["heads"], weight_h=1.0, acc=big["acc"], weight=0.7)], NH, NORM[norm])
    ops.head_maps([ops.HeadMaps(small, con, heads=few["heads"], weight_h=1.0, acc=few["acc"], weight=0.7)], NH, NORM[norm])
    torch.cuda.synchronize()
    for lo in (0, 200):
        assert torch.equal(big["heads"][:, :, lo:lo + 5], few["heads"]), (norm, lo)
        assert torch.equal(big["acc"][:, lo:lo + 5], few["acc"]), (norm, lo)
    assert bool(few["acc"].abs().sum() > 0)


@pytest.mark.parametrize("cid", ["heads_NH24_L257_C12_none_n1_acc2", "heads_NH5_L257_C17_none_n16_all",
                                 "heads_NH32_L257_C9_none_n1_all"])
def test_at_norm_none_the_head_sum_is_the_full_width_logit_of_the_device(cid):
    """NH x acc2 (weight 1 on zeros: the mean itself) against ops.heatmap_logits on the same rows, inside the two kernels'
    bounds added (both are bounds against the same fp64 logits)."""
    case = H.BY_ID[cid]
    s = case.shape
    inp, ref = inputs_and_reference(case)
    al = Guarded()
    dev = place(case, inp, al)
    ops.head_maps(problems(case, dev), s["NH"], L.NORM_NONE)
    for d, pr, r in zip(dev, inp["probs"], ref):
        lg = torch.empty(s["C"], s["L"], device=DEV)
        ops.heatmap_logits(d["img"][:, :s["dim"]], d["con"][:, :s["dim"]], lg)
        z, e_z, kind = R.logits_reference(case, pr, DEV)["logits"]
        mean, pre, _ = r["acc2"]
        slack = s["NH"] * R.bound(mean, pre, "f32") + R.bound(z, e_z, kind)
        err = (s["NH"] * d["acc2"].double() - lg.double()).abs()
        assert bool((err <= slack).all()), float((err / slack).max())


@pytest.mark.parametrize("norm", ["softmax", "sparsemax", "entmax15"])
def test_one_head_of_128_columns_against_heatmap_fused(norm):
    """NH = 1, hidden 128, C <= 8: the head is the full width, so acc is ops.heatmap_fused's on the same rows inside the
    two kernels' bounds added."""
    case = H.BY_ID[{"softmax": "heads_NH1_L257_C8_softmax_n16_all", "sparsemax": "heads_NH1_L3_C8_sparsemax_n1_acc",
                    "entmax15": "heads_NH1_L257_C8_entmax15_n1_acc"}[norm]]
    s = case.shape
    inp, ref = inputs_and_reference(case)
    got = run(case, inp, Guarded())
    for pr, g, r in zip(inp["probs"], got, ref):
        img, con = pr["img"][:, :128].to(DEV), pr["con"][:, :128].to(DEV)
        acc = pr["acc0"].to(DEV)
        ops.heatmap_fused([ops.Heatmap(img, con, acc=acc, weight=H.W1)], norm=L.NORMS[norm])
        z = con.double() @ img.double().T
        e_z = 2 * (128 / 64 + 6 + 1) * R.U * (con.double().abs() @ img.double().abs().T)     # (rowop_cases.fused_reference's)
        o, pre = R.weighted(z, e_z, norm, H.W1, pr["acc0"].to(DEV).double())
        assert R.excess(acc, o, pre, "f32")[1] == 0
        mine, pre_mine, _ = r["acc"]
        slack = R.bound(mine, pre_mine, "f32") + R.bound(o, pre, "f32")
        err = (g["acc"].double() - acc.double()).abs()
        assert bool((err <= slack).all()), float((err / slack).max())
