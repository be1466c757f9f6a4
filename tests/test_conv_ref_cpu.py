"""The reference helper of test_conv_views_gpu.py, checked without a GPU: for every entry of that file's case tables
torch's own fp32 convolution (forward with the epilogue, and the fp32 autograd gradients) stays inside the
(K + 8) * 2^-24 * mag bound against the float64 reference of the same inputs, and elements nothing is added into are
exact.  That is what makes the bound one a correct fp32 implementation meets with these very inputs; a case that
missed it here would have badly scaled inputs, and the inputs would change, not the bound."""
import pytest
import torch

import _conv_ref as C
import test_conv_views_gpu as T


def _taps(case):
    return case["k"][0] * case["k"][1] * case["k"][2]


def _positions(case, t):
    n, to, ho, wo, _ = t["dz"].shape
    return n * to * ho * wo


def _inside(got, ref, mag, K, tag):
    r = C.rounds(got, ref, mag)   # asserts finiteness and exactness where mag == 0
    print("%-40s fp32 reference: worst %.3f of %.0f allowed" % (tag, r, C.bound(K)))
    assert r <= C.bound(K), (tag, r, C.bound(K))
    return r


def test_tables_hold_the_cases_they_claim():
    names = [c["name"] for c in T.FWD_CASES]
    assert len(set(names)) == len(names)
    with_res = sum(1 for c in T.FWD_CASES if c["res"])
    assert with_res * 2 >= len(T.FWD_CASES) and sum(1 for c in T.FWD_CASES if c["act"] == 6) == 1
    assert all(_taps(c) * c["cin"] <= 1200 for c in T.FWD_CASES)
    assert all(_taps(c) * c["cout"] <= 1200 for c in T.DGRAD_CASES)
    # positions not a multiple of 16 somewhere in every table, Cout = 72 in the forward one
    for table in (T.FWD_CASES, T.DGRAD_CASES, T.WGRAD_CASES):
        assert any((c["nthw"][0] * c["nthw"][1] * c["nthw"][2] * c["nthw"][3]) % 16 for c in table)
    assert any(c["cout"] == 72 for c in T.FWD_CASES)
    assert any(c["cin"] < (c["cin"] + 15) // 16 * 16 for c in T.WGRAD_CASES)


@pytest.mark.parametrize("case", T.FWD_CASES, ids=[c["name"] for c in T.FWD_CASES])
def test_forward_reference_bound(case):
    t = C.conv_inputs(case)
    res = t["res"] if case["res"] else None
    ref, mag = C.conv_ref(t["x"], t["w"], t["bias"], t["scale"], res, case["act"], case["s"], case["p"])
    got = C.conv_fp32(t["x"], t["w"], t["bias"], t["scale"], res, case["act"], case["s"], case["p"])
    assert ref.dtype == torch.float64 and mag.dtype == torch.float64 and got.dtype == torch.float32
    assert ref.shape == got.shape == mag.shape and bool((mag >= ref.abs() * (1 - 1e-12)).all())
    _inside(got, ref, mag, _taps(case) * case["cin"], "fwd/" + case["name"])
    if case["act"] == 6:  # both clamps are reached, and the open interval
        assert bool((ref == 0).any()) and bool((ref == 6).any()) and bool(((ref > 0) & (ref < 6)).any())


DGRAD = [(c, a) for c in T.DGRAD_CASES for a in c["modes"]]


@pytest.mark.parametrize("case,accumulate", DGRAD, ids=["%s-%s" % (c["name"], "acc" if a else "write") for c, a in DGRAD])
def test_dgrad_reference_bound(case, accumulate):
    t = C.conv_inputs(case)
    base = t["base_dx"] if accumulate else None
    ref, mag = C.dgrad_ref(t["dz"], t["w"], t["x"].shape, case["s"], case["p"], base=base)
    got = C.dgrad_fp32(t["dz"], t["w"], t["x"].shape, case["s"], case["p"], base=base)
    assert ref.shape == t["x"].shape
    _inside(got, ref, mag, _taps(case) * case["cout"], "dgrad/" + case["name"])
    if case["name"] == "pw_s2_64_128":  # three of four residue classes get no tap: mag == 0 there, and rounds() wants 0.0
        untapped = torch.ones(ref.shape[1:4], dtype=torch.bool)
        untapped[:, ::2, ::2] = False
        assert bool((mag[:, untapped] == 0).all()) and bool((mag[:, ~untapped] > 0).all())


WGRAD = T.WGRAD_CASES + [T.WGRAD_BX_CASE, T.PRESUM_CASE]


@pytest.mark.parametrize("case", WGRAD, ids=[c["name"] for c in WGRAD])
def test_wgrad_reference_bound(case):
    t = C.conv_inputs(case)
    K = _positions(case, t)
    if case in T.WGRAD_CASES and case["name"] != "rows_s3_8_8":
        assert K <= 1200, (case["name"], K)
    for base in (None, t["base_dw"]):
        ref, mag = C.wgrad_ref(t["x"], t["dz"], t["w"].shape, case["s"], case["p"], base=base)
        got = C.wgrad_fp32(t["x"], t["dz"], t["w"].shape, case["s"], case["p"], base=base)
        assert ref.shape == t["w"].shape
        _inside(got, ref, mag, K, "wgrad/%s/%s" % (case["name"], "finish" if base is not None else "packed"))


FINISH = [(c, a) for c in T.FINISH_CASES for a in (0, 1)]


@pytest.mark.parametrize("case,accumulate", FINISH, ids=["%s-%s" % (c["name"], "acc" if a else "write") for c, a in FINISH])
def test_finish_reference_bound(case, accumulate):
    t = C.finish_inputs(case)
    base = t["base"] if accumulate else None
    ref, mag = C.finish_ref(t["part"], case["cin"], case["fold_kw"], base)
    p32 = t["part"].sum(0)   # fp32 sum over the splits, then the same un-packing
    if case["fold_kw"] > 0:
        got = p32[:, :, :4 * case["fold_kw"]].reshape(case["cout"], case["taps"], case["fold_kw"], 4)[..., :case["cin"]]
        got = got.permute(0, 3, 1, 2).contiguous()
    else:
        got = p32[:, :, :case["cin"]].permute(0, 2, 1).contiguous()
    if accumulate:
        got = got + base.reshape(got.shape)
    assert ref.numel() == t["base"].numel() and bool(torch.isfinite(ref).all())
    assert float(ref.abs().max()) < 1000.0, "a padding column leaked into the reference"
    _inside(got, ref, mag, case["S"], "finish/" + case["name"])


def test_reference_catches_a_dropped_product():
    """The point of K <= 1200: one product left out of an element (about mag / K) stands clear of the bound."""
    case = next(c for c in T.FWD_CASES if c["name"] == "splitk_s3_128_64")   # the largest K of the forward table
    t = C.conv_inputs(case)
    ref, mag = C.conv_ref(t["x"], t["w"], None, None, None, False, case["s"], case["p"])
    x2 = t["x"].clone()
    x2[0, 1, 7, 8, 5] = 0.0   # every output that reads this input loses one product
    got = C.conv_fp32(x2, t["w"], None, None, None, False, case["s"], case["p"])
    err = (got.double() - ref).abs() / (C.U * mag)
    assert float(err.max()) > 10 * C.bound(_taps(case) * case["cin"])
