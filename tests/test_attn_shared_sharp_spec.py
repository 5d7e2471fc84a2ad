"""CPU specification of the sharp inputs of shared-prefix decode attention (tests/attn_sharp.py: SharedCase, f1_shared, f2_shared) that
tests/test_gpu_attn_shared_sharp.py runs through pplhip_op_attention_shared: F1 cases are exact gathers (the C oracle on the ordinary
page table agrees bit for bit), their winners stand on every edge of the shared launch's splits, wave strides and register buffers and
of the own launch's chunks, group / group_tokens as the cases write them down equal the product's grouping rule, the float64
reference of the three launches agrees with the oracle on F2, and every mutant of the shared path moves an F2 output by >= 4 x the bar
(and, where it changes which keys are visible, an F1 winner)."""
import functools
import math

import numpy as np
import pytest

from tests import attn_sharp as A
from tests.conftest import load_pplhip

TEETH = 4.0
F1_SPECS = A.f1_shared_specs()


@functools.lru_cache(maxsize=None)
def _f1(i):
    c = A.make_shared(F1_SPECS[i])
    return (c,) + A.expect_gather(c)


@functools.lru_cache(maxsize=None)
def _f2(i):
    family, where, spec = A.F2_SHARED_SPECS[i]
    return A.make_shared(spec, family, where)


def _ids(specs):
    return lambda i: specs[i]["name"]


@pytest.mark.parametrize("i", range(len(F1_SPECS)), ids=_ids(F1_SPECS))
def test_f1_oracle_equals_gather(i):
    """every (row, head) has one key >= GAP above all others (expect_gather asserts it on the dequantised slab) and the fp32 oracle,
    on the ordinary page table, produces exactly that key's V row"""
    c, want, top = _f1(i)
    got = c.oracle().astype(np.float16)
    assert (got.view(np.uint16) == want.view(np.uint16)).all(), A.explain_mismatch(c, got, want, top)


@pytest.mark.parametrize("i", range(len(F1_SPECS)), ids=_ids(F1_SPECS))
def test_f1_slab_and_page_table(i):
    """a group's members carry the same leading P / page_size page ids and nothing else in common; entries past a row's last page name
    the spare page; every slot of no request, the spare page and the whole other layer hold poison"""
    c, _, _ = _f1(i)
    ps = c.page_size
    owned = np.zeros(c.N, dtype=bool)
    holders = {}
    for b in range(c.B):
        npg = -(-int(c.kvlen[b]) // ps)
        assert (c.cache_idx[b, npg:] == c.spare_page).all()
        for j, pg in enumerate(c.cache_idx[b, :npg]):
            holders.setdefault(int(pg), []).append((b, j))
        owned[c.slots(b, np.arange(c.kvlen[b]))] = True
    for pg, hs in holders.items():
        b, j = hs[0]
        if c.group[b] >= 0 and j < c.P[b] // ps:   # a shared page: column j of every member of the group, of nobody else
            assert hs == [(r, j) for r in c.members[c.group[b]]], pg
        else:
            assert len(hs) == 1, pg
    assert not owned[c.spare_page * ps:(c.spare_page + 1) * ps].any()
    free = np.where(~owned)[0]
    for hk in range(c.Hkv):
        for layer, sl in ((c.layer, free), (1 - c.layer, np.arange(c.N))):
            lay, c.layer = c.layer, layer
            k, v = c.read(0, hk, sl), c.read(1, hk, sl)
            c.layer = lay
            assert (k[:, 0] == A.GAMMA).all() and (k[:, 1:] == 0).all() and (v == A.POISON_V).all()


def test_f1_spec_dimensions():
    """the dimensions the specs must span"""
    S = F1_SPECS
    assert {s["fmt"] for s in S} == {"f16", "i8"}
    assert {(s["H"], s["Hkv"], s["D"]) for s in S} == {(4, 4, 128), (6, 2, 64), (12, 2, 128), (8, 1, 128), (16, 1, 64)}
    assert {s["page_size"] for s in S} == {16, 32, 48, 64} and {s["layout"] for s in S} == {0, 1, 2, 3}
    assert {s["shared_split"] for s in S} == {1, 3, A.SP_SPLIT_MAX} == {1, 3, 4} and {s["own_split"] for s in S} == {2, 3}
    assert {n for s in S for _, n in s["rows"]} >= set(A.OWN_LENS)
    assert {p for s in S for p in s["groups"]} >= {16, 48, 272, 2048, 4096}
    assert all(24 <= len(s["rows"]) <= 40 for s in S)
    cases = [_f1(i)[0] for i in range(len(S))]
    assert {(c.grp, 16 // c.grp, 16 % c.grp if len(t["rows"]) == 16 // c.grp else None) for c in cases for t in c.tiles} >= \
        {(1, 16, 0), (3, 5, 1), (6, 2, 4), (8, 2, 0), (16, 1, 0)}
    # P = 2048 with 17 members at group 1: a full tile and a tile of one member and 15 padding columns
    assert any(c.grp == 1 and [(t["tokens"], len(t["rows"]), t["pad"]) for t in c.tiles if t["g"] == 0] == [(2048, 16, 0), (2048, 1, 15)]
               for c in cases)
    assert any(sorted(len(m) for m, p in zip(c.members, c.group_tokens) if p == 4096) == [2] for c in cases)
    # two groups whose tiles interleave in row order: a tile of one group opens between two tiles of the other
    def interleaved(c):
        firsts = sorted((t["rows"][0], t["g"]) for t in c.tiles)
        gs = [g for _, g in firsts]
        return any(gs[k] == gs[k + 2] != gs[k + 1] for k in range(len(gs) - 2))
    assert any(interleaved(c) for c in cases)
    for c in cases:   # loose rows between members; a member with start_pos == P
        assert any(c.group[b] < 0 and (c.group[:b] >= 0).any() and (c.group[b + 1:] >= 0).any() for b in range(c.B))
    assert any(((c.group >= 0) & (c.start_pos == c.P)).any() for c in cases)


def test_kernel_form_mirrors():
    """the mirrors of the shared launch's geometry"""
    assert A.shared_split_ranges(16, 3) == [(0, 1), (1, 1), (2, 1)]            # one sub-tile: every split but the first is empty ...
    assert sorted(A.shared_wave_steps(0, 1)) == [0]                             # ... and so are three of the four waves
    assert A.shared_split_ranges(272, 3) == [(0, 6), (6, 12), (12, 17)]         # 17 sub-tiles, uneven over 3 splits
    assert A.shared_split_ranges(48, 4) == [(0, 1), (1, 2), (2, 3), (3, 3)]
    st = A.shared_wave_steps(6, 17)
    assert st[6] == (0, 0, 0) and st[9] == (3, 0, 0) and st[10] == (0, 1, 1) and st[14] == (0, 2, 0) and st[16] == (2, 2, 0)
    assert A.own_chunks(130, 1, True) == [(0, 128), (128, 130)] and A.own_chunks(130, 2, False) == [(0, 65), (65, 130)]
    assert A.own_chunks(700, 3, True) == [(0, 256), (256, 512), (512, 700)] and A.own_chunks(1, 2, False) == [(0, 1)]
    t = A.shared_tiles([0, 1, 0, -1, 0, 1], [48, 272], 6)
    assert [(x["g"], x["rows"], x["lead"], x["pad"]) for x in t] == [(0, [0, 2], 2, 4), (0, [4], 4, 10), (1, [1, 5], 5, 4)]
    assert t[0]["cols"] == [0] * 6 + [2] * 6 + [-1] * 4


@pytest.mark.parametrize("i", range(len(F1_SPECS)), ids=_ids(F1_SPECS))
def test_groups_match_the_grouping_rule(i):
    """group / group_tokens as the case writes them down are what pplhip_op_shared_prefix_groups derives from its page table, and the
    tile mirror is what they imply: every member in exactly one tile, grp columns each, 16 // grp requests per tile, the lead its last"""
    c, _, _ = _f1(i)
    m = load_pplhip()
    group, tokens, n = np.full(c.B, 7, dtype=np.int32), np.zeros(c.B, dtype=np.int64), np.zeros(1, dtype=np.int32)
    pages, sp = np.ascontiguousarray(c.cache_idx), np.ascontiguousarray(c.start_pos)
    rc = m.lib().pplhip_op_shared_prefix_groups(pages.ctypes.data, c.max_pages, sp.ctypes.data, c.B, c.B, c.page_size, 2, 16,
                                                group.ctypes.data, tokens.ctypes.data, n.ctypes.data)
    assert rc == 0 and n[0] == len(c.group_tokens)
    assert (group == c.group).all() and (tokens[:n[0]] == c.group_tokens).all()
    assert A.shared_tiles(group, tokens, c.grp) == c.tiles
    per = 16 // c.grp
    cols = {}
    for t in c.tiles:
        assert 1 <= len(t["rows"]) <= per and t["lead"] == t["rows"][-1] and t["pad"] == 16 - len(t["rows"]) * c.grp
        assert all(c.group[r] == t["g"] for r in t["rows"]) and t["tokens"] == c.group_tokens[t["g"]]
        assert t["rows"] == sorted(t["rows"])
        for col, r in enumerate(t["cols"]):
            cols.setdefault(r, []).append(col % c.grp if r >= 0 else -1)
    for b in range(c.B):
        assert (cols.get(b) == list(range(c.grp))) == (c.group[b] >= 0)
    for g, mem in enumerate(c.members):   # all tiles of a group but its last are full
        sizes = [len(t["rows"]) for t in c.tiles if t["g"] == g]
        assert sizes[:-1] == [per] * (len(sizes) - 1) and sum(sizes) == len(mem)


@pytest.mark.parametrize("i", range(len(F1_SPECS)), ids=_ids(F1_SPECS))
def test_f1_directions_and_decoys(i):
    """queries are Hadamard rows; within one tile and KV head every column has another direction; about half the member rows win in
    the shared part and half in their own, and the losing part holds a real competitor (a needle of the same direction)"""
    c, _, top = _f1(i)
    Hd = A.hadamard(c.D)
    q = c.qkv[:, :c.H * c.D].astype(np.float64).reshape(c.B, c.H, c.D)
    d = (q @ Hd.T).argmax(-1)
    assert (Hd[d] == q).all()
    for t in c.tiles:
        for hk in range(c.Hkv):
            used = [d[r, hk * c.grp + g] for r in t["rows"] for g in range(c.grp)]
            assert len(set(used)) == len(used)
    in_shared = 0
    unit = A.alpha_of(c.D) * math.sqrt(c.D)
    members = [b for b in range(c.B) if c.group[b] >= 0]
    for b in members:
        P = int(c.P[b])
        for hq in range(c.H):
            s = c.Kd[b][hq // c.grp].astype(np.float64) @ q[b, hq] / math.sqrt(c.D)
            won_shared = top[b, hq] < P
            in_shared += won_shared
            loser = s[P:] if won_shared else s[:P]
            assert loser.max() >= 0.99 * unit and s.max() - loser.max() >= A.GAP
    assert 0.4 <= in_shared / (len(members) * c.H) <= 0.6


def test_f1_winners_cover_every_edge_kind():
    """over the whole set of specs the winners stand on: shared key 0 and P - 1, key P (key 0 of the shifted table), the current token,
    both sides of a sub-tile edge, a page edge, a shared-split start and a wave-stride edge, a sub-tile a wave reaches on its second
    buffer and one it reaches on the first buffer again, the last sub-tile of a split (prefetch clamp live), both sides of an own-split
    chunk start -- classified by the split / wave / chunk mirrors, from the winners expect_gather found"""
    cover = {}
    starts = set()
    for i, spec in enumerate(F1_SPECS):
        c, _, top = _f1(i)
        for b in range(c.B):
            for hq in range(c.H):
                for kind in A.shared_kinds(c, b, int(top[b, hq])):
                    cover.setdefault(kind, set()).add(spec["name"])
                if c.group[b] >= 0 and top[b, hq] < c.P[b] and top[b, hq] % A.SH_SUB in (0, A.SH_SUB - 1):   # (sub-tile, its first key?)
                    starts.add((i, int(c.group[b]), (int(top[b, hq]) + 1) // A.SH_SUB, int(top[b, hq]) % A.SH_SUB == 0))
    print("\n" + "\n".join(f"{kind:>13}: {', '.join(sorted(cover.get(kind, ())))}" for kind in A.SHARED_KINDS))
    assert cover.get("first"), "shared key 0"
    assert cover.get("last"), "shared key P - 1"
    assert cover.get("own_first"), "key P"
    assert cover.get("current"), "the current token"
    assert cover.get("subtile-") and cover.get("subtile+"), "sub-tile edge"
    assert cover.get("page-") and cover.get("page+"), "page edge"
    assert cover.get("split-") and cover.get("split+"), "shared-split start"
    assert cover.get("stride-") and cover.get("stride+"), "wave-stride edge"
    assert cover.get("buffer1"), "a sub-tile reached on the second register buffer"
    assert cover.get("buffer0again"), "a sub-tile reached on the first register buffer again"
    assert cover.get("split_last"), "the last sub-tile of a split"
    assert cover.get("own_split-") and cover.get("own_split+"), "own-split chunk start"
    for i in range(len(F1_SPECS)):   # BOTH sides of EVERY start of a non-empty shared split of every group hold a winner
        c = _f1(i)[0]
        for g, P in enumerate(c.group_tokens):
            for s0, s1 in A.shared_split_ranges(int(P), c.shared_split):
                assert s0 >= s1 or s0 == 0 or {(i, g, s0, False), (i, g, s0, True)} <= starts, (F1_SPECS[i]["name"], g, s0)


@pytest.mark.parametrize("mut", A.SHARED_F1_MUTANTS)
def test_f1_mutant_moves_a_winner(mut):
    """a mutant that changes which keys are visible changes the top key of some (row, head) of some F1 spec: the gather run as the
    three launches read the slab, under the mutation"""
    moved = []
    for i, spec in enumerate(F1_SPECS):
        c, _, top = _f1(i)
        base = A._ref64_shared(c, None, gather=True)
        own = np.array([[c.slots(b, top[b, h]) * c.Hkv + h // c.grp for h in range(c.H)] for b in range(c.B)])
        assert (base == own).all(), "the launches' view of the slab disagrees with the ordinary one"
        got = A._ref64_shared(c, mut, gather=True)
        if got is not None and (got != base).any():
            moved.append(spec["name"])
    print(f"\n{mut}: {', '.join(moved)}")
    assert moved, mut


F2 = [s for _, _, s in A.F2_SHARED_SPECS]


@pytest.mark.parametrize("i", range(len(F2)), ids=_ids(F2))
def test_f2_ref64_matches_oracle(i):
    """the float64 reference of the three launches equals the oracle on the ordinary page table: within half an fp16 ulp + 0.05 x bar"""
    c = _f2(i)
    want = A.ref64(c)
    got = c.oracle()
    half_ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64) / 2
    err = np.abs(got - want) - half_ulp
    bar = A.bar_of(c, want)
    assert (err <= 0.05 * bar).all(), float((err / bar).max())


def _shared_mass(c):
    """softmax mass on the shared keys, per (member row, head)"""
    out = []
    for b in range(c.B):
        if c.group[b] >= 0:
            for hq in range(c.H):
                s = c.Kd[b][hq // c.grp].astype(np.float64) @ c.qkv[b, hq * c.D:(hq + 1) * c.D].astype(np.float64) / math.sqrt(c.D)
                p = np.exp(s - s.max())
                out.append(p[:c.P[b]].sum() / p.sum())
    return np.array(out)


def test_f2_mass_lies_where_the_case_says():
    """every family has a case whose mass straddles P and one with it (nearly) wholly in each part"""
    assert {(f, w) for f, w, _ in A.F2_SHARED_SPECS} == {(f, w) for f in ("compete", "sink", "rising") for w in ("straddle", "shared", "own")}
    for i, (family, where, spec) in enumerate(A.F2_SHARED_SPECS):
        mass = _shared_mass(_f2(i))
        if where == "shared":
            assert np.median(mass) >= 0.8, (spec["name"], np.median(mass))
        elif where == "own":
            assert np.median(mass) <= 0.2, (spec["name"], np.median(mass))
        else:
            assert ((mass >= 0.25) & (mass <= 0.75)).any(), (spec["name"], mass.min(), mass.max())


def test_f2_mutants_have_teeth(capsys):
    """every mutant of the shared path moves the output of some F2 case by >= 4 x the GPU bar (table: max |mutant - ref64| / bar)"""
    rows = [(spec["name"], A.shared_teeth(_f2(i))) for i, (_, _, spec) in enumerate(A.F2_SHARED_SPECS)]
    w = max(len(r[0]) for r in rows)
    lines = [" " * w + " " + " ".join(f"{m:>16}" for m in A.SHARED_MUTANTS)]
    for name, t in rows:
        lines.append(f"{name:<{w}} " + " ".join(f"{'n/a':>16}" if t[m] is None else f"{t[m]:>16.3g}" for m in A.SHARED_MUTANTS))
    lines.append("(max |mutant - ref64| / bar)")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert set(A.SHARED_MUTANTS) <= A.APPLIES["shared"]
    for m in A.SHARED_MUTANTS:
        best = max((t[m] for _, t in rows if t[m] is not None), default=None)
        assert best is not None and best >= TEETH, (m, best)
    # a doubly counted key leaves a gather unchanged: F2 alone catches it
    c = _f1(1)[0]
    assert (A._ref64_shared(c, "own_recount", gather=True) == A._ref64_shared(c, None, gather=True)).all()
