"""Multi-LoRA without a device: the exact builder's conditions, the bound against an fp32 model of the kernels, the mutants, the tile list
and the refusals pplhip_op_lora decides before any device call (tests/lora.py)."""
import numpy as np
import pytest

from tests import lora as L
from tests.conftest import load_pplhip

CASES = L.all_cases()
BY_NAME = {c.name: c for c in CASES}


def _case(kind, T, rmap):
    return next(c for c in CASES if c.kind == kind and c.T == T and c.rmap == rmap)


def fp32_model(case):
    """what kernels of the documented arithmetic write, in numpy fp32 with a summation order of their own (K in four interleaved parts of
    32-column steps, the parts added last; the rank in steps of 32): output buffer bits"""
    c = case.build()
    out = c.ybuf.copy()
    for s, rows in L.build_tiles(c.row_slots):
        A, B, scale = c.adapters[s]
        A32, B32 = A.astype(np.float32), B.astype(np.float32)
        x = c.x[rows].astype(np.float32)
        part = np.zeros((4, len(rows), A32.shape[0]), dtype=np.float32)
        for k0 in range(0, c.K, 32):
            part[(k0 // 32) % 4] += x[:, k0:k0 + 32] @ A32[:, k0:k0 + 32].T
        t = (((part[0] + part[1]) + part[2]) + part[3]).astype(np.float16).astype(np.float32)
        acc = np.zeros((len(rows), c.N), dtype=np.float32)
        for j0 in range(0, A32.shape[0], 32):
            acc += t[:, j0:j0 + 32] @ B32[:, j0:j0 + 32].T
        y = c.y0[rows].astype(np.float32) + np.float32(scale) * acc
        out[np.array(rows), :c.N] = y.astype(np.float16).view(np.uint16)
    return out


def test_case_list_reaches_every_edge_the_issue_names():
    assert {(c.T, c.K, c.N) for c in CASES} == set(L.SHAPES)
    assert {c.rmap for c in CASES} == set(L.ROW_MAPS)
    used = set()
    for c in CASES:
        used |= set(c.ranks.values())
    assert used == set(L.RANKS)
    assert any(len(set(c.ranks.values())) >= 2 for c in CASES), "two different ranks in one launch"
    grid = [c for c in CASES if c.kind != "cancel"]
    assert sum(c.ldx > c.K for c in grid) * 2 == len(grid) and sum(c.ldy > c.N for c in grid) * 2 == len(grid)
    assert any(c.ldy > c.N and c.ldy % 4 == 0 for c in CASES) and any(c.ldy % 4 for c in CASES)
    runs = L.row_map("runs", 130)
    lens, n = [], 0
    for v in list(runs) + [-1]:
        if v >= 0:
            n += 1
        elif n:
            lens.append(n)
            n = 0
    assert {1, 15, 16, 17, 33} <= set(lens)
    assert set(L.row_map("ids", 130)) == {-1, 0, 5, 63}
    assert (L.row_map("mod3", 50) == np.arange(50) % 3 - 1).all()


@pytest.mark.parametrize("name", [c.name for c in CASES if c.kind == "exact"])
def test_exact_cases_meet_the_builders_conditions(name):
    c = BY_NAME[name].build()          # (asserts: t fp16-exact, every partial sum below 2^24, y0 fp16-exact)
    ref = c.expected()                 # (asserts: the float64 reference gives the integers' bits)
    assert L.judge(c, L.bits(ref)) == []
    if (c.row_slots >= 0).any():
        # the last rounding does something: many outputs need more than 11 significant bits
        a = c.row_slots >= 0
        v = np.abs(c.exact_int[a])
        low = v & -v
        sig = np.where(v > 0, np.floor(np.log2(np.maximum(v, 1))) - np.log2(np.maximum(low, 1)) + 1, 0)
        assert np.mean(sig > 11) >= 0.3, np.mean(sig > 11)
    # any summation order gives the same bits: the fp32 model is exact on these operands
    assert L.judge(c, fp32_model(c)) == []


@pytest.mark.parametrize("name", [c.name for c in CASES if c.kind != "exact"])
def test_bound_holds_for_an_fp32_model_and_is_not_slack(name):
    c = BY_NAME[name].build()
    assert L.judge(c, fp32_model(c)) == [], "the bound refuses correct fp32 arithmetic"
    assert L.judge(c, L.bits(c.expected())) == []
    a = c.row_slots >= 0
    if a.any():
        v = c.expected(rounded=False)[:c.T, :c.N][a]
        b = c.bound()[:c.T, :c.N][a]
        # not slack: a few fp16 ulps of the value it bounds (half an ulp is the last rounding alone; the rest is mostly t landing on the
        # other side of a rounding boundary, which the worst-case fp32 sum over K allows for about a quarter of the t at these sizes)
        # (K = 4096: the any-order worst case of the fp32 sum, K u sum |x A|, is several fp16 ulps of t by itself)
        if c.kind == "random" and c.K <= 320 and max(c.ranks.values()) <= 24:
            assert np.median(b / L.ulp16(np.abs(v))) <= 4.0, np.median(b / L.ulp16(np.abs(v)))


# the exact and the random case each mutant is built for (row 0 without an adapter and a padded tile; two slots; ldy > N; a rank above 16)
MUTANT_CASES = {
    "wrong slot for a tile": (("exact", 50, "mod3"), ("random", 50, "mod3")),
    "last row of a tile dropped": (("exact", 17, "all"), ("random", 17, "all")),
    "padding row written": (("exact", 50, "mod3"), ("random", 50, "mod3")),
    "scale omitted": (("exact", 130, "all"), ("random", 130, "all")),
    "rank truncated to 16": (("exact", 130, "all"), ("random", 130, "all")),
    "t not rounded": (("exact", 130, "runs"), ("cancel", 50, "runs")),
    "ldy taken as N": (("exact", 17, "runs"), ("random", 17, "runs")),
}


def test_every_mutant_has_its_cases():
    assert sorted(MUTANT_CASES) == sorted(L.MUTANTS)


@pytest.mark.parametrize("mutant", L.MUTANTS)
def test_mutants_are_caught(mutant):
    ex, rnd = (_case(*k).build() for k in MUTANT_CASES[mutant])
    if mutant == "t not rounded":
        # on exact operands t IS an fp16 number: the mutant changes nothing there -- that is what "exact" means -- so its exact case
        # only has to hold; the case built for it is the cancelling one
        assert L.judge(ex, L.bits(ex.expected(mutant=mutant))) == []
    else:
        assert L.judge(ex, L.bits(ex.expected(mutant=mutant))) != [], f"{mutant}: no asserted output of {ex.name} moves"
    got = rnd.expected(mutant=mutant)
    assert L.judge(rnd, L.bits(got)) != [], f"{mutant}: {rnd.name} accepts it"
    v, b = rnd.expected(rounded=False), rnd.bound()
    touched = b > 0
    with np.errstate(invalid="ignore"):
        moved = np.abs(got - v)
    outside = (L.bits(got) != rnd.ybuf) & ~touched            # canaries and rows without an adapter: any change counts
    assert outside.any() or (moved[touched] >= 4 * b[touched]).any(), (mutant, float(np.nanmax(moved[touched] / b[touched])))


def test_tile_list_properties():
    rng = np.random.RandomState(5)
    maps = [L.row_map(k, T) for k in L.ROW_MAPS for T in (1, 15, 16, 17, 33, 130)]
    maps += [rng.randint(-1, 64, size=n).astype(np.int32) for n in (1, 7, 100, 1000)]
    maps += [np.full(40, 63, dtype=np.int32), np.array([], dtype=np.int32)]
    for rs in maps:
        tiles = L.build_tiles(rs)
        L.check_tiles(rs, tiles)
        assert len(tiles) == sum(((rs == s).sum() + 15) // 16 for s in set(rs[rs >= 0].tolist()))
    # and the checker itself refuses: a row in two tiles, a row in none, an unassigned row in a tile, a tile that mixes slots
    for rs, bad in (([0, 0], [(0, [0, 1]), (0, [1])]), ([0, 0], [(0, [0])]), ([0, 0, -1], [(0, [0, 1, 2])]), ([0, 1], [(0, [0, 1])])):
        with pytest.raises(AssertionError):
            L.check_tiles(np.array(rs, dtype=np.int32), bad)


def test_op_lora_refusals_need_no_device():
    m = load_pplhip()
    X, Y, A, B, WS = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24   # fake, aligned addresses: a refusal never dereferences them
    ok = dict(x=X, ldx=256, y=Y, ldy=256, T=4, N=256, K=256, row_slots=[0, -1, 0, 0], A=[A], B=[B], ranks=[8], scales=[1.0], ws=WS,
              ws_bytes=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return m.op_lora(a["x"], a["ldx"], a["y"], a["ldy"], a["T"], a["N"], a["K"], a["row_slots"], a["A"], a["B"], a["ranks"], a["scales"],
                         a["ws"], a["ws_bytes"])

    INVALID = -2
    assert call(K=264, ldx=264) == INVALID                     # K % 32
    assert call(N=264, ldy=264) == INVALID                     # N % 16
    assert call(row_slots=[0, 1, 0, 0]) == INVALID             # slot out of range
    assert call(row_slots=[0, 64, 0, 0]) == INVALID
    assert call(row_slots=[0, -2, 0, 0]) == INVALID
    assert call(row_slots=[1, -1, -1, -1], A=[A, None], B=[B, None], ranks=[8, 0], scales=[1.0, 0.0]) == INVALID   # names an unloaded slot
    assert call(ranks=[0]) == INVALID and call(ranks=[129]) == INVALID
    assert call(ldx=248) == INVALID and call(ldy=128) == INVALID and call(ldx=260) == INVALID
    assert call(ws_bytes=64) == INVALID                        # workspace too small
    assert call(A=[A] * 65, B=[B] * 65, ranks=[8] * 65, scales=[1.0] * 65) == INVALID
    # nothing assigned: nothing to do, no device needed either
    assert call(row_slots=[-1, -1, -1, -1]) == 0
    assert call(T=0, row_slots=[]) == 0
    assert m.LORA_MAX_SLOTS == L.MAX_SLOTS == 64 and m.LORA_MAX_RANK == L.MAX_RANK == 128


def test_step_plan_with_adapter_rows_is_one_lane_and_defers_nothing():
    m = load_pplhip()
    base = dict(tp=1, dual_mode=1, has_stream2=1, dual_min_rows=96, dual_max_rows=512, defer_on=1, hidden_dim=4096, heads=32, kv_heads=32,
                head_dim=128, cache_quant_bit=8, cache_quant_group=8)
    plain = m.step_plan(base, 256, 256, 256, max_kv_len=512)
    assert plain["schedule"] == m.SCHED_TWO_LANES and plain["defer_qkv"] and plain["defer_reduce"]
    lora = m.step_plan(base, 256, 256, 256, max_kv_len=512, lora=True)
    assert lora["schedule"] == m.SCHED_ONE_LANE and len(lora["chunks"]) == 1 and lora["chunks"][0] == (0, 256, 0, 256, 256)
    assert not lora["defer_qkv"] and not lora["defer_reduce"]
    assert lora["decode_split"] == m.step_plan(dict(base, dual_mode=0), 256, 256, 256, max_kv_len=512)["decode_split"]


def test_the_widest_shape_still_tells_every_structural_mutant():
    """K = 4096: the any-order worst case of the fp32 sum over K makes the bound several fp16 ulps of t wide there, so a t that was not
    rounded cannot show (its case is the cancelling one at K = 320, and the exact cases hold every bit at K = 4096).  Every other mutant
    moves an output of the K = 4096 random cases by far more than four times that bound."""
    c = _case("random", 130, "runs").build()
    assert c.K == 4096 and c.ldy > c.N and max(c.ranks.values()) > 16 and len(c.ranks) == 2
    v, b = c.expected(rounded=False), c.bound()
    touched = b > 0
    for mutant in L.MUTANTS:
        if mutant == "t not rounded":
            continue
        got = c.expected(mutant=mutant)
        assert L.judge(c, L.bits(got)) != [], mutant
        with np.errstate(invalid="ignore"):
            assert np.nanmax(np.abs(got - v)[touched] / b[touched]) >= 4, mutant
