"""The direct collectives' cases without a device (tests/comm_ops.py): the case list reaches every slice, grid, width and granule class for
every rank count (asserted from the helper's mirror of the kernels' index arithmetic), the needles have the properties they are named
for, the reference passes its own checker and every mutant of it is rejected."""
import numpy as np
import pytest

from tests import comm_ops as Cm
from tests import row_ops as R


@pytest.mark.parametrize("n", Cm.RANKS)
def test_case_list_reaches_every_class(n):
    cs = Cm.cases(n)
    ar = [c for c in cs if c.kind == Cm.AR]
    got = set().union(*[c.classes() for c in ar])
    want = {"rank_owns_nothing", "short_last_slice", "past_the_end", "one_in_last_row_of_slices", "two_blocks", "family_exact", "family_random",
            "family_mixed"}
    if Cm.NEEDLE_KINDS(n):
        want.add("family_needles")
    if n in (2, 8):
        want.add("block_cap_and_trips")
    assert want <= got, want - got
    assert {c.granules for c in ar} >= {1, n - 1, n, n + 1, 2 * n + 1, 3 * n - 1}
    # granules < n and granules = n (per - 1) + 1: ranks that own nothing; n per - 1: a short last slice
    assert "rank_owns_nothing" in Cm.slice_classes(n, 1) and "short_last_slice" in Cm.slice_classes(n, 3 * n - 1)
    assert Cm.slices(n, 2 * n + 1)[0] == 3 and "one_in_last_row_of_slices" in Cm.slice_classes(n, 2 * n + 1)
    two = Cm.ar_geometry(n, n * Cm.GRANULES_PER_BLOCK + 1)
    assert two["blocks"] == 2 and Cm.ar_geometry(n, n * Cm.GRANULES_PER_BLOCK)["blocks"] == 1      # the smallest two-block shape
    if n in (2, 8):
        cap = Cm.ar_geometry(n, max(c.granules for c in ar))
        assert cap["blocks"] == Cm.BLOCK_CAP and cap["trips"] > 1
        assert Cm.ar_geometry(n, max(c.granules for c in ar) - 1)["blocks"] == Cm.BLOCK_CAP - 1    # ... and the smallest at the cap

    fu = [c for c in cs if c.kind == Cm.FUSED]
    got = set().union(*[c.classes() for c in fu])
    want = {"hidden_%d" % h for h in Cm.FUSED_WIDTHS} | {"rows_%s" % t for t in Cm.fused_rows(n)} | \
           {"rank_owns_nothing", "short_last_slice", "per_above_block_cap"}
    assert want <= got, want - got
    for rows in set(Cm.fused_rows(n).values()):
        assert len({c.hidden for c in fu if c.rows == rows}) >= 2, rows
    for hd in Cm.FUSED_WIDTHS:
        assert len({c.rows for c in fu if c.hidden == hd}) >= 2, hd
    g = Cm.fused_geometry(n, 33 * n - 1, 8)
    assert g["per"] == 33 and g["blocks"] == Cm.BLOCK_CAP and g["trips"] == 2
    # the widths sit on either side of the kernel's limits: one lane, 512 lanes exactly, 512 + 1, an unclamped second pass part, 1023, 1024
    geo = {h: Cm.fused_geometry(n, n, h) for h in Cm.FUSED_WIDTHS}
    assert [(geo[h]["chunks"], geo[h]["second_chunk"], geo[h]["clamped"]) for h in Cm.FUSED_WIDTHS] == \
           [(1, False, True), (512, False, False), (513, True, True), (640, True, True), (1023, True, True), (1024, True, False)]
    assert {c.family for c in fu} == ({"exact", "moderate", "needles"} if Cm.NEEDLE_KINDS(n) else {"exact", "moderate"})

    ga = [c for c in cs if c.kind == Cm.GATHER]
    got = set().union(*[c.classes() for c in ga])
    want = {"granule_8", "granule_16", "rows_1", "rows_5", "stride_wide", "stride_tight"} | {"cols_%d" % c for c in Cm.GATHER_COLS}
    assert want <= got, want - got
    for cols in Cm.GATHER_COLS:
        assert {(c.rows, c.stride > n * cols) for c in ga if c.cols == cols} >= {(1, False), (1, True), (5, False), (5, True)}
    assert len({c.name for c in cs}) == len(cs)


def _parts(X):
    want = Cm.reduce16(X)
    return want, {"exact": Cm.exact16(X), "reverse": Cm.reduce16(X, "reverse"), "tree": Cm.reduce16(X, "tree"), "f16acc": Cm.reduce16(X, "f16acc")}


@pytest.mark.parametrize("n", Cm.RANKS)
def test_needles_part_the_documented_sum_from_its_neighbours(n):
    nd = Cm.needles(n)
    want, other = _parts(nd)
    for kind in Cm.NEEDLE_KINDS(n):
        assert (Cm.bits16(want) != Cm.bits16(other[kind])).sum() >= 4, kind
    if n >= 3:
        assert nd[0, 0] == 32768 and nd[1, 0] == 16 and (nd[2:, 0] == 2.0 ** -9).all()
        assert want[0] == 32768 and other["exact"][0] == 32800
    if n == 8:
        assert other["reverse"][0] == 32800 and other["tree"][0] == 32800
    assert np.isfinite(want.astype(np.float32)).all() and (np.abs(want.astype(np.float32)) <= 40000).all()


def test_what_no_needle_can_show():
    """two ranks: every order, the tree, the float64 sum and fp16 accumulation are one function; three ranks: the adjacent-pairs tree is
    the rank order (tests/comm_ops.py, module docstring) -- searched over random finite bit patterns and over the needle pool"""
    rng = np.random.RandomState(7)
    for n, kinds in ((2, ("exact", "reverse", "tree", "f16acc")), (3, ("tree",))):
        b = rng.randint(0, 1 << 16, size=(n, 400000)).astype(np.uint16)
        b[(b & 0x7C00) == 0x7C00] &= np.uint16(0xFBFF)
        for X in (b.view(np.float16), Cm._needle_pool(n, 400000, rng)):
            # a near-cancelling pair as well: the exponents of a random pair rarely meet
            X = np.concatenate([X, np.stack([X[0], -X[0]] + [X[i] for i in range(2, n)])], axis=1) if n == 2 else X
            want, other = _parts(X)
            for kind in kinds:
                assert (Cm.bits16(want) == Cm.bits16(other[kind])).all(), (n, kind)


@pytest.mark.parametrize("n", Cm.RANKS)
def test_value_families(n):
    for c in Cm.cases(n):
        if c.kind != Cm.AR or not Cm.small(c):
            continue
        X = c.build()["data"][:, :c.count]
        want, exact = Cm.reduce16(X), Cm.exact16(X)
        f32 = X.astype(np.float32)
        assert np.isfinite(f32).all()
        if c.family == "exact":
            assert (Cm.bits16(want) == Cm.bits16(exact)).all()
            for mu in ("reverse", "tree", "f16acc"):
                assert (Cm.bits16(Cm.reduce16(X, mu)) == Cm.bits16(want)).all()
        if c.family == "random":
            sub = (np.abs(f32) < 2.0 ** -14) & (f32 != 0)
            wf = want.astype(np.float32)
            assert sub.all(0).any() and ((np.abs(wf) < 2.0 ** -14) & (wf != 0)).any()                # subnormal inputs and results
            assert (Cm.bits16(X) == 0x8000).all(0).any()                                            # -0.0 on every rank
            assert ((f32 != 0).any(0) & (Cm.bits16(want) == 0)).any()                               # total cancellation
            assert np.isposinf(wf).any() and np.isneginf(wf).any()
            assert not np.isnan(wf).any()
        if c.family == "needles":
            assert (Cm.bits16(want) != Cm.bits16(exact)).any()


@pytest.mark.parametrize("n", Cm.RANKS)
def test_reference_passes_its_own_checker(n):
    for c in Cm.cases(n):
        if Cm.small(c):
            inp = c.build()
            assert Cm.check(c, inp, Cm.emulate(c, inp)) == [], c.name


def fp32_model(case, inp):
    """the fused form's y from fp32 arithmetic in an order of its own (numpy's pairwise float32 sum; (r * inv) * w), on the reference
    residual: what a correct kernel may give and the interval must admit"""
    outs = Cm.emulate(case, inp)
    rows, hd = case.rows, case.hidden
    per, sl = Cm.slices(case.n, rows)
    r = np.concatenate([outs[q][0][lo * hd:hi * hd] for q, (lo, hi) in enumerate(sl) if hi > lo]).reshape(rows, hd).astype(np.float32)
    ss = (r * r).sum(-1, dtype=np.float32)
    inv = np.float32(1.0) / np.sqrt(ss / np.float32(hd) + np.float32(Cm.EPS))
    y = ((r * inv[:, None]) * inp["w"][0].astype(np.float32)).astype(np.float16)
    res = []
    for q in range(case.n):
        x = outs[q][1].copy()
        x[:rows * hd] = y.reshape(-1)
        res.append((outs[q][0], x))
    return res


@pytest.mark.parametrize("n", (2, 5, 8))
def test_interval_admits_an_fp32_kernel(n):
    for c in Cm.cases(n):
        if c.kind == Cm.FUSED and Cm.small(c):
            inp = c.build()
            assert Cm.check(c, inp, fp32_model(c, inp)) == [], c.name


@pytest.mark.parametrize("n", Cm.RANKS)
@pytest.mark.parametrize("mutant", Cm.MUTANTS)
def test_checker_rejects_mutant(n, mutant):
    """at least one case per rank count and family of collectives it applies to; the mutants that no input can show (test_what_no_needle_can_show)
    are the only ones allowed to apply to nothing"""
    kinds = {Cm.AR: 0, Cm.FUSED: 0, Cm.GATHER: 0}
    applied = 0
    for c in Cm.cases(n):
        if not (Cm.small(c) and Cm.mutant_applies(mutant, c)):
            continue
        applied += 1
        inp = c.build()
        if Cm.check(c, inp, Cm.emulate(c, inp, mutant)):
            kinds[c.kind] += 1
    if mutant in ("reverse", "tree", "f16acc") and mutant not in Cm.NEEDLE_KINDS(n):
        assert applied == 0
        return
    if mutant in ("no_inner_rounding", "h_rows_overwritten"):
        assert kinds[Cm.FUSED] >= 1
    elif mutant == "swap_8_in_16":
        assert kinds[Cm.GATHER] >= 1
    else:
        assert kinds[Cm.AR] >= 1 and kinds[Cm.FUSED] >= 1, kinds


def test_no_inner_rounding_needs_its_planted_columns():
    """fp16(h + sum) and fp16(h + fp16(sum)) part on the planted columns of every fused case (sum 1 + 2^-11, h 2^-11)"""
    c = next(c for c in Cm.cases(4) if c.kind == Cm.FUSED and c.hidden == 4104 and c.rows == 5)
    inp = c.build()
    a, b = Cm.emulate(c, inp), Cm.emulate(c, inp, "no_inner_rounding")
    d = np.nonzero(Cm.bits16(a[0][0]) != Cm.bits16(b[0][0]))[0]
    assert len(d) and set((d % c.hidden) % 24) >= {0}
    assert R.DELTA == 2.0 ** -16
