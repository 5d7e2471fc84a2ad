"""CPU checks of tests/row_ops.py: the cases of tests/test_gpu_row_ops.py reach every (Skip)RMSNorm kernel form, the interval checker
rejects every subtly wrong norm and accepts the kernel's own arithmetic, and the deferred split-K routes have the split counts the GPU
file relies on.  No device."""
import numpy as np
import pytest

from tests import row_ops as R
from tests.conftest import load_pplhip

INVALID = -2
TABLE_ROWS = [1, 4, 5, 37, 512, 513]
TABLE_HIDDEN = [8, 136, 2048, 2056, 4088, 4096, 4104, 4608, 5120, 8192, 8200, 16384, 16392]


def _rule(rows, hidden, wide_max_rows):
    """launch_rmsnorm's choice, restated: the pinned table"""
    chunks = hidden // 8
    if chunks > 2048:
        return None
    if 4 < rows <= wide_max_rows and 512 <= chunks <= 1024 and chunks % 64 == 0:
        return (1, 512 if chunks <= 512 else 1024)
    return (1 if chunks <= 256 else 2 if chunks <= 512 else 4 if chunks <= 1024 else 8, 256)


def test_form_table():
    m = load_pplhip()
    seen = set()
    for wide in (512, 0):
        for rows in TABLE_ROWS:
            for hidden in TABLE_HIDDEN:
                want = _rule(rows, hidden, wide)
                for quant in (0, 1, 2):
                    rc, text = m.rmsnorm_form(rows, hidden, quant, wide)
                    if want is None:
                        assert (rc, text) == (INVALID, ""), (rows, hidden, quant, wide, rc, text)
                    else:
                        assert rc == 0 and text == "rmsnorm_kernel<%d,%d%s>" % (want + (R.QUANT_TAGS[quant],)), (rows, hidden, quant, wide, rc, text)
                        seen.add(text)
    assert len(seen) == 18
    # a few fixed points spelled out (not through _rule)
    assert m.rmsnorm_form(4, 4096, 0)[1] == "rmsnorm_kernel<2,256>" and m.rmsnorm_form(5, 4096, 0)[1] == "rmsnorm_kernel<1,512>"
    assert m.rmsnorm_form(512, 8192, 2)[1] == "rmsnorm_kernel<1,1024,f8>" and m.rmsnorm_form(513, 8192, 1)[1] == "rmsnorm_kernel<4,256,i8>"
    assert m.rmsnorm_form(37, 4104, 0)[1] == "rmsnorm_kernel<4,256>" and m.rmsnorm_form(1, 16384, 0)[1] == "rmsnorm_kernel<8,256>"
    assert m.rmsnorm_form(5, 4096, 0, 0)[1] == "rmsnorm_kernel<2,256>"
    # refusals: the status of a launch; rows == 0 launches nothing
    assert m.rmsnorm_form(1, 16392)[0] == INVALID and m.rmsnorm_form(37, 4100)[0] == INVALID and m.rmsnorm_form(1, 4)[0] == INVALID
    assert m.rmsnorm_form(0, 4096) == (0, "") and m.rmsnorm_form(1, 4096, 3)[0] == INVALID and m.rmsnorm_form(-1, 4096)[0] == INVALID


def test_gpu_cases_reach_all_18_instantiations():
    """every (rows, hidden) tests/test_gpu_row_ops.py launches takes the form it is listed under, with each epilogue (default switch)"""
    m = load_pplhip()
    reached = set()
    for form, cases in R.FORM_CASES.items():
        for rows, hidden in cases:
            for quant in (0, 1, 2):
                rc, text = m.rmsnorm_form(rows, hidden, quant, 512)
                assert rc == 0 and text == R.form_text(form, quant), (rows, hidden, quant, text)
                reached.add(text)
    assert len(reached) == 18 and len(R.FORM_CASES) == 6
    assert sorted(R.ALL_FORM_CASES) == sorted(set(R.ALL_FORM_CASES))


def _sample(case):
    """the rows the CPU check looks at: every live row, or -- launch shapes of more than 64 rows -- up to 48 needle rows spread over the
    launch plus the edge rows (the rows are the ones the GPU sees: the case is built whole, then cut)"""
    live = case.live
    if case.rows <= 64:
        return live
    needles = live[case.kind[live] == "needle"]
    pick = needles[np.unique(np.linspace(0, len(needles) - 1, 48).astype(np.int64))]
    return np.concatenate([pick, live[case.kind[live] != "needle"]])


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("rows,hidden", R.ALL_FORM_CASES)
def test_checker_rejects_every_mutant_and_accepts_the_form(rows, hidden, skip):
    case = R.norm_case(rows, hidden, skip)
    idx = _sample(case)
    kind = case.kind[idx]
    want16 = np.concatenate([R.rn16(R.ref_rmsnorm_rows(case, idx[i:i + R.BLOCK])) for i in range(0, len(idx), R.BLOCK)])
    # the correctly rounded reference itself passes, at distance 0
    bad, worst = R.check_norm_rows(case, idx, want16)
    assert not bad.any() and worst == 0.0
    # the kernel's arithmetic in float32, in this form's summation order, passes -- with room
    maxc, nt = R.form_args(R.expected_form(rows, hidden))
    emu = R.emulate_form(case.residual(idx), case.w, maxc, nt, hidden)
    bad, worst = R.check_norm_rows(case, idx, emu)
    assert not bad.any(), (int(bad.sum()), kind[bad][:4])
    print(f"emulated {R.expected_form(rows, hidden)} rows={rows} hidden={hidden} skip={skip}: needed delta {worst:.4f} DELTA")
    assert worst <= 0.5, worst       # the derivation in tests/row_ops.py: under 0.33 DELTA
    # every mutant is rejected in every needle row
    needle = kind == "needle"
    for mut in R.MUTANTS:
        if not R.mutant_applies(mut, case):
            continue
        bad, _ = R.check_norm_rows(case, idx, want16, mutant=mut)
        if mut == "no_eps":
            # eps = 1e-5 against mean(x~^2) of a needle row: 2.3 at hidden 8 (a shift of 2e-6 = 0.14 DELTA, not an error the checker
            # may see), 1e-2 at hidden 2048 (a shift of 5e-4).  The tiny and the zero row are where eps decides: always rejected there
            assert bad[(kind == "tiny") | (kind == "zero")].all(), mut
            if hidden >= 2048:
                assert bad[needle].all(), (mut, int((~bad[needle]).sum()))
        else:
            assert bad[needle].all(), (mut, int((~bad[needle]).sum()), int(needle.sum()))


def test_needle_positions_cover_every_boundary():
    for chunks in (1, 256, 512, 640, 1024, 2048):
        p = set(R.needle_positions(chunks))
        assert {0, chunks - 1} <= p
        for nt in (256, 512, 1024):
            for b in range(nt, chunks, nt):
                assert {b - 1, b} <= p
        for b in range(64, chunks, 64):
            assert {b - 1, b} <= p
    # launches of more than 4 rows: row r carries chunk r % chunks; fewer rows than chunks: the boundary positions follow
    c = R.norm_case(37, 136, False)
    assert (c.needle[:37] == np.arange(37) % 17).all() and set(c.needle[:37]) == set(range(17)) and c.launches == 2
    c = R.norm_case(37, 4608, False)
    assert (c.needle[:37] == np.arange(37)).all() and set(R.needle_positions(576)) <= set(c.needle[c.kind == "needle"])
    c = R.norm_case(640, 5120, True)
    assert set(c.needle[:640]) == set(range(640)) and c.launches == 2


def test_slab_builder_and_reference():
    for splits in range(1, 9):
        for with_scale in (False, True):
            ws, scale = R.build_slabs(5, 64, splits, with_scale)
            assert np.isnan(ws[splits:]).all() and np.isfinite(ws[:splits]).all()
            got = R.slab_reduce(ws, splits, scale)
            assert np.isfinite(got.astype(np.float32)).all()
            # against float64: the float32 sequential sum is a rounding of it, not something else
            ref = ws[:splits].astype(np.float64).sum(0) * (1.0 if scale is None else scale.astype(np.float64))
            assert np.abs(got.astype(np.float64) - ref).max() <= 0.02 + 2.0 ** -10 * np.abs(ref).max()
    assert R.build_slabs(5, 64, 3, True)[0].dtype == np.float32


def test_kv_edge_rows_hit_their_edges():
    from tests import kv_fp8, kv_i4
    for D in (32, 64, 128):
        h = R.kv_edge_head_rows(D)
        x = h.astype(np.float32)
        # int8 group 8: scale fp16(max / 127), q = rint(x / scale)
        g = x.reshape(len(h), D // 8, 8)
        s = (np.abs(g).max(-1) / np.float32(127)).astype(np.float16).astype(np.float32)
        assert (s[0] == 0).all() and (s[1] == 0).all() and (np.abs(g[1]).max() > 0)
        assert (s[2] == 0.125).all()
        t = g[2] * np.float32(8)
        assert (np.abs(t - np.trunc(t)) == 0.5).sum() >= 6 * (D // 8) and (t == 127).any() and (t == -127).any()
        # fp8 rows
        q, e = kv_fp8.quantize_rows(h)
        assert e[0] == -15 and e[1] == -15 and e[5] == 0 and e[6] == 8 and (q[5] == 0x7e).any() and (q[5] == 0xfe).any()
        assert (q[1] & 0x7f).max() >= 17 and (q[6] & 0x7f).max() == 0x77      # ties region reached; saturation at 240
        # int4 groups
        q4, s4 = kv_i4.quantize_groups(h)
        s4 = s4.astype(np.float32)
        assert (s4[0] == 2.0 ** -14).all() and (q4[0] == 0).all() and (s4[1] == 2.0 ** -14).all() and (q4[1] == 0).all()
        assert (s4[3] == 2.0 ** -14).all() and (s4[4] == 0.125).all() and (q4[4] == 7).any() and (q4[4] == -7).any()
        t3, t4 = x[3] * np.float32(2.0 ** 14), x[4] * np.float32(8)
        assert (np.abs(t3 - np.trunc(t3)) == 0.5).all() and (np.abs(t4 - np.trunc(t4)) == 0.5).sum() >= D - D // 16
        assert s4[6].max() <= 9344 and np.abs(x[6]).max() == 60000


def test_deferred_routes_have_the_pinned_split_counts():
    m = load_pplhip()
    counts = set()
    for (M, N, K), want in R.DEFER_SHAPES.items():
        for wq, group in R.DEFER_WQ:
            rc, route, sp, sc = m.linear_defer(1 << 21, 1 << 22, (1 << 23) if wq else None, wq, group, M, N, K, 1 << 20, N, ws=1 << 24,
                                               ws_bytes=R.DEFER_WS_BYTES, dry_run=True)
            assert rc == 0 and sp == 0 and sc is None      # a dry run touches nothing and reports no slabs
            splits, reduce = R.route_splits(route)
            assert reduce == "deferred" and splits == want[wq], (M, N, K, wq, route)
            counts.add(splits)
            # the same call without `defer` picks the same kernel and split count and reduces itself
            rc, plain = m.linear_route(1 << 21, 1 << 22, (1 << 23) if wq else None, wq, group, M, N, K, 1 << 20, N, 0, ws=1 << 24,
                                       ws_bytes=R.DEFER_WS_BYTES, dry_run=True)
            assert rc == 0 and plain == route.replace("reduce=deferred", "reduce=splitk_reduce_kernel<f16>"), (plain, route)
    assert {2, 4, 8} <= counts and (3 in counts or 5 in counts)
    # no workspace: nothing to defer
    rc, route, _, _ = m.linear_defer(1 << 21, 1 << 22, None, 0, 128, 5, 1024, 4096, 1 << 20, 1024, ws=None, ws_bytes=0, dry_run=True)
    assert rc == 0 and "reduce=deferred" not in route
