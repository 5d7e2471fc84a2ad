"""The exact mixture-of-experts cases (tests/moe_exact.py) without a device: the float64 reference, the integer form and the kernel-by-kernel
model agree bit for bit, every builder bound holds, every case has the property its table row claims, and every named mistake of
moe_exact.FAULTS changes at least one bit of what a call leaves in the case written for it."""
import numpy as np
import pytest

from tests import moe_exact as X

CASES = X.all_cases()
IDS = [c.name for c in CASES]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_reference_integer_form_and_model_agree(idx):
    c = CASES[idx].build()
    ids, p, y = X.reference(c)
    want = c.expected()
    assert (ids == c.ids).all()
    assert (p.view(np.uint32) == c.p.view(np.uint32)).all()
    assert (y.view(np.uint16) == want.view(np.uint16)).all()
    assert not np.isnan(want).any() and np.abs(want.astype(np.float64)).max() > 0
    m = X.model(c)
    assert (m["ids"] == c.ids).all() and (m["weights"].view(np.uint32) == c.p.view(np.uint32)).all()
    assert (m["y"].view(np.uint16) == want.view(np.uint16)).all()
    # placement: every pair once, an expert's rows in ascending pair order
    st = X.bucket(c.ids, c.E, X.tile_rows(c.T, c.k, c.E))
    assert sorted(st["inv"].tolist()) == sorted(set(st["inv"].tolist())) and (st["sorted"][st["inv"]] == np.arange(c.T * c.k)).all()
    assert X.layout(c.T, c.E, c.k, c.hidden, c.inter)["rows_cap"] >= len(st["sorted"])


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_bounds_and_claims(idx):
    c = CASES[idx].build()
    T, E, k = c.T, c.E, c.k
    # the builder's bounds, restated
    assert c.hidden * np.abs(c.xcode).max() * np.abs(c.gcode).max() <= 1 << 24
    assert np.abs(c.uint).max() <= 2048
    hv = np.abs(c.hcode[c.hcode != 0]) * c.uh
    assert hv.max() < 65504 and hv.min() >= 2.0 ** -14
    hsel = np.abs(np.take_along_axis(c.hcode, c.ids[:, :, None], 1))            # h of the pairs that exist, in units
    assert c.inter * hsel.max() * np.abs(c.w2code).max() <= 1 << 24 and np.abs(c.S2).max() <= 1 << 24
    unit2 = c.s2.min()
    assert c.e2 or k * np.abs(c.S2 * (c.s2[c.ids] / unit2)).max() <= 1 << 24
    assert set(np.unique(c.gval)) == {16, 0, 32, -64} or c.inter < 4
    if c.wq == 8:
        assert np.abs(c.w13.astype(np.int64)).max() <= 127 and len(np.unique(c.s13.astype(np.float64))) >= 3
        if not c.e2:
            s = np.log2(c.s2h.astype(np.float64))
            assert (s == np.round(s)).all() and len(np.unique(s)) >= 3
    if not c.distinct:
        assert (c.p == np.float32(1.0 / k)).all()
        low = [sorted(cl)[:k] for cl in c.classes]
        # the winners are the k lowest indices of one class, ascending, unless two classes tie by chance (then the rule decides)
        pure = [row.tolist() in low for row in c.ids]
        assert np.mean(pure) >= 0.9
        if c.plan is not None:
            assert all(pure)
    else:
        assert set(np.unique(c.p)) == {np.float32(0.0), np.float32(1.0)} and (np.diff(c.ids, axis=1) < 0).any()
    # every class that is larger than k: members not all adjacent
    for cl in c.classes:
        if len(cl) > 1 and len(cl) < E:
            assert max(cl) - min(cl) >= len(cl)
    claim = c.claim
    hist = c.histogram()
    assert hist[E:].sum() == 0 and hist.sum() == T * k
    for e, n in claim.get("hist", {}).items():
        assert hist[e] == n, (c.name, e, hist[:E])
    if "passes" in claim:
        assert c.passes() == claim["passes"]
    if "tied" in claim:
        assert c.tied_tokens() == claim["tied"]
    if "tied_is_hist" in claim:     # a winner from the larger class ties with the class's next member, a winner from a class of k does not
        assert 0 < c.tied_tokens() == hist[claim["tied_is_hist"]] < T
    assert X.tile_rows(T, k, E) == claim["tile"]
    if "live" in claim:
        assert X.bucket(c.ids, E, X.tile_rows(T, k, E))["live"] == claim["live"]
        assert claim["live"] <= (T * k + E * 127 + 127) // 128
    print(f"{c.name}: T {T} E {E} k {k} hidden {c.hidden} inter {c.inter}; histogram {hist[:E].tolist()}; passes {c.passes()}; tied tokens "
          f"{c.tied_tokens()}; tile rows {X.tile_rows(T, k, E)}; x codes <= {c.xm}, w2 codes <= {c.w2max}; double roundings {c.double_roundings()}")


def test_case_specific_properties():
    for wq in (0, 8):
        lo, hi = X.by_name(f"threshold_lo-w{wq}").build(), X.by_name(f"threshold_hi-w{wq}").build()
        assert lo.T == X.threshold_T(8, 2) and hi.T == lo.T + 1 and X.tile_rows(lo.T, 2, 8) == 32 and X.tile_rows(hi.T, 2, 8) == 128
        assert (lo.x == hi.x[:lo.T]).all() and (lo.w13 == hi.w13).all() and (lo.w2 == hi.w2).all() and (lo.gate == hi.gate).all()
        assert (lo.expected().view(np.uint16) == hi.expected()[:lo.T].view(np.uint16)).all()
        c = X.by_name(f"three_pass_k8-w{wq}").build()
        passes = [set((np.nonzero(c.ids.ravel() == e)[0] // X.BUCKET_NT).tolist()) for e in range(c.E)]
        first = [int(np.nonzero(c.ids.ravel() == e)[0][0]) // X.BUCKET_NT for e in range(c.E)]
        assert {0, 1, 2} in passes and 1 in first
        c = X.by_name(f"three_pass_k1-w{wq}").build()
        assert c.T * c.k == 2 * X.BUCKET_NT + 1
        assert any(len(set((np.nonzero(c.ids.ravel() == e)[0] // X.BUCKET_NT).tolist())) == 3 for e in range(c.E))
        c = X.by_name(f"two_pass-w{wq}").build()
        assert c.T * c.k == X.BUCKET_NT + 70 and 70 % 64
        c = X.by_name(f"e64_k8-w{wq}").build()
        assert c.E == 64 and c.k == 8
        c = X.by_name(f"one_token-w{wq}").build()
        assert c.hidden // 64 == 1 and c.hidden < 128
        for n in ("ragged_n192", "ragged_n320"):
            c = X.by_name(f"{n}-w{wq}").build()
            assert c.hidden % 128 and c.inter < c.inter_p and c.hidden // 64 >= 3
    assert X.by_name("k1-w8").e2 and [c.base for c in CASES if c.e2] == ["k1", "k_eq_e_odd3"]
    for c in CASES:
        if c.build().e2:
            assert c.double_roundings() >= 0.05 * c.T * c.hidden, (c.name, c.double_roundings())
    # the closed columns are really closed and the open ones open, on the honest silu
    g = np.array([16.0, 32.0, 0.0, -64.0])
    h = (g / (1.0 + np.exp(-g)) * 1000.0).astype(np.float16)
    assert h.tolist() == [16000.0, 32000.0, 0.0, 0.0]


@pytest.mark.parametrize("fault", sorted(X.FAULTS))
@pytest.mark.parametrize("wq", [0, 8])
def test_every_fault_changes_a_bit(fault, wq):
    c = X.by_name(f"{X.FAULTS[fault]}-w{wq}").build()
    prev = X.model(X.by_name(f"spread-w{wq}").build()) if fault.startswith("stale live") else None
    good, bad = X.model(c), X.model(c, fault=fault, prev=prev)
    assert not X.same_outputs(good, bad), f"{fault}: nothing changes in {c.name}"
    what = [n for n in ("ids", "weights", "y", "live", "tiles", "sorted", "inv") if not np.array_equal(np.asarray(good[n]), np.asarray(bad[n]), equal_nan=n == "y")]
    print(f"{fault}: caught by {c.name} in {what}")
