"""CPU specification of the post-processor cases (tests/postproc.py) that tests/test_gpu_postproc.py runs on the device: the references
written from the specification agree with the C oracle where the oracle can say anything, every builder assertion holds, and the case
lists reach the branches of csrc/k_sample.hip they were written for."""
import numpy as np
import pytest

from oracle import ref
from tests import postproc as P

PENALTY = P.penalty_scenarios()
GREEDY = P.greedy_cases()
TOPK = P.topk_cases()


# ---- penalty ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(PENALTY)), ids=[s.name for s in PENALTY])
def test_penalty_builder_assertions_and_oracle(idx):
    """ids in range, poison placed, an off-by-one count detectable (check_penalty_scenario); and where every clear comes from
    start_pos == 0 and the rows are dense the C oracle's ref_penalty gives the same counts bit for bit and logits within the bound"""
    sc = PENALTY[idx].build()
    refs = P.check_penalty_scenario(sc)
    if not (P.clears_only_at_position_zero(sc) and sc.stride == sc.vocab):
        return
    cm = sc.cm0.copy()
    _p = lambda a: None if a is None else a.ctypes.data
    for st, (want_cm, want, bound, _) in zip(sc.steps, refs):
        lg = st.logits.copy()
        ref.lib().ref_penalty(lg.ctypes.data, _p(st.temps), _p(st.rep), _p(st.pres), _p(st.freq), st.slots.ctypes.data, st.tokens.ctypes.data,
                              st.seq_starts.ctypes.data, st.start_pos.ctypes.data, st.B, sc.vocab, cm.ctypes.data)
        assert (cm == want_cm).all()
        assert (np.abs(lg.astype(np.float64) - want) <= bound).all()


def test_oracle_comparison_is_not_empty():
    small = [s.build() for s in PENALTY if s.family != "shape"]
    n = {f: sum(1 for s in small if s.family == f and P.clears_only_at_position_zero(s) and s.stride == s.vocab) for f in ("contention", "logit")}
    assert n["contention"] >= 4 and n["logit"] >= 3, n
    assert sum(1 for V, s, B in P.SHAPE_GRID if V == s) >= 10


def test_penalty_cases_reach_what_they_were_written_for():
    small = [s.build() for s in PENALTY if s.family != "shape"]
    fam = lambda f: [s for s in small if s.family == f]
    # contention: both halves of one word fed in one launch, at both ends of the row, with an adjacent slot in the same launch
    ends = set()
    for sc in fam("contention"):
        st = sc.steps[0]
        a = int(st.seq(0)[0])
        assert {a, a ^ 1} == set(st.seq(0).tolist()) and abs(int(st.slots[0]) - int(st.slots[1])) == 1
        na = int((st.seq(0) == a).sum())
        ends.add((a, na))
        assert na != int((st.seq(0) == (a ^ 1)).sum())
    assert ends == {(a, n) for a in (0, 1022) for n in (1, 255, 256, 257, 4000)}
    # saturation: every preload on both halves beside 0 and beside 65535, fed three times, nothing clears, the stop is reached
    for sc in fam("saturation"):
        assert all((st.start_pos > 0).all() and st.dec == st.B for st in sc.steps)
        seen = set()
        for tok in np.unique(np.concatenate([st.tokens for st in sc.steps])):
            assert sum(int((st.tokens == tok).sum()) for st in sc.steps) == 3
            seen.add((int(sc.cm0[1, tok]), int(tok & 1), int(sc.cm0[1, tok ^ 1])))
        assert set(P.SAT_PRELOADS) <= seen
        final = P.check_penalty_scenario(sc)[-1][0]
        assert (final[1][np.unique(sc.steps[0].tokens)] == 65535).all()
    assert any(s.stride > s.vocab for s in fam("saturation"))
    # clear rules: each of the four situations occurs, with preloaded counts to keep or to lose
    kinds = set()
    for sc in fam("clear"):
        cm = sc.cm0
        for st, r in zip(sc.steps, P.check_penalty_scenario(sc)):
            for b in range(st.B):
                had = bool(cm[st.slots[b]].any())
                kinds.add((b < st.dec, bool(st.start_pos[b] > 0), had))
            assert list(range(st.dec)) == [b for b in range(st.B) if b < st.dec]           # decode rows first
            cm = r[0]
        assert any(sc.nslots - 1 in st.slots for st in sc.steps)
        assert any((np.diff(st.slots) < 0).any() for st in sc.steps) and any((np.abs(np.diff(np.sort(st.slots))) > 1).any() for st in sc.steps)
    assert {(True, True, True), (False, False, True), (False, True, True), (True, False, True)} <= kinds
    assert any(len(sc.steps) >= 5 and not P.clears_only_at_position_zero(sc) for sc in fam("clear"))
    # logit rule: the special values sit on counted tokens; rep on both sides of 1; every pointer NULL once; every kind of temperature
    none = {"temps": 0, "rep": 0, "pres": 0, "freq": 0}
    temps, reps = set(), set()
    for sc in fam("logit"):
        for st, r in zip(sc.steps[:1], P.check_penalty_scenario(sc)[:1]):
            for b in range(st.B):
                vals = set(st.logits[b][r[3][b] > 0].view(np.uint32).tolist())
                assert set(np.array(P.SPECIALS, dtype=np.float32).view(np.uint32).tolist()) <= vals
            for k in none:
                none[k] += getattr(st, k) is None
            temps |= set() if st.temps is None else {float(np.sign(t)) if t != 1 else 1.0 for t in st.temps} | {float(t > 0 and t != 1) for t in st.temps}
            reps |= set() if st.rep is None else {float(np.sign(x - 1)) for x in st.rep}
    assert all(v >= 1 for v in none.values()), none
    assert {-1.0, 0.0, 1.0} <= temps and {-1.0, 0.0, 1.0} <= reps
    # shapes
    assert {(V, s - V, B) for V, s, B in P.SHAPE_GRID if V != 128256} == {(V, d, B) for V in (2, 1024, 32000) for d in (0, 2, 6) for B in (1, 8, 64)}
    assert {(s - V, B) for V, s, B in P.SHAPE_GRID if V == 128256} == {(0, 1), (2, 8), (6, 64)}


# ---- samplers ---------------------------------------------------------------------------------------------------------------------
def _dense(c):
    """the oracle on a case (it reads dense rows)"""
    if c.top_k == 1:
        return ref.sample(c.logits, top_k=1, temperatures=c.temps)
    return ref.sample(c.logits, top_k=c.top_k, top_p=c.top_p, temperatures=c.temps, top_p_list=c.top_p_list, rnd=c.rnd)


@pytest.mark.parametrize("idx", range(len(GREEDY)), ids=[c.name for c in GREEDY])
def test_greedy_builder_assertions_and_oracle(idx):
    c = GREEDY[idx].build()
    rows, _ = c.check_assertions()                       # poison placed, gap >= 1.0 or an exact tie, the planted answer is the reference's
    tok, lp = _dense(c)
    for b, (wtok, wlp, _, _) in enumerate(rows):
        assert tok[b] == wtok and abs(lp[b] - wlp) <= P.LOGPROB_BAR, (c.name, b)


@pytest.mark.parametrize("idx", range(len(TOPK)), ids=[c.name for c in TOPK])
def test_topk_builder_assertions_and_oracle(idx):
    c = TOPK[idx].build()
    rows, _ = c.check_assertions()
    tok, lp = _dense(c)
    for b, (wtok, wlp, margin, cand) in enumerate(rows):
        assert 0 <= tok[b] < c.V and tok[b] in cand, (c.name, b)
        if margin >= P.MARGIN:
            assert tok[b] == wtok and abs(lp[b] - wlp) <= P.LOGPROB_BAR, (c.name, b, int(tok[b]), wtok, margin)


def test_uncompared_rows_stay_under_the_cap_per_family():
    n = {f: [0, 0] for f in P.TOPK_FAMILIES}
    for lz in TOPK:
        c = lz.build()
        n[c.family][0] += c.check_assertions()[1]
        n[c.family][1] += c.B
    for f, (unc, rows) in n.items():
        assert rows and unc <= P.UNCOMPARED_CAP * rows, (f, unc, rows)


def test_sampler_cases_reach_what_they_were_written_for():
    g = [(lz.name, lz.build()) for lz in GREEDY]
    Vs = {c.V for _, c in g}
    assert Vs == set(P.GREEDY_V)
    for V in P.GREEDY_V:
        lay = {(c.stride - V, c.off) for _, c in g if c.V == V}
        assert {s for s, _ in lay} >= {0, 1, 3, P.next8(V) - V} and {o for _, o in lay} == {0, 1, 2, 3}
    vec = [c for _, c in g if c.uses_vector_path()]
    assert any(c.V % 4 for c in vec), "scalar tail after the float4 part"
    assert any(c.V >= 4 and not c.uses_vector_path() and c.off for _, c in g) and any(c.stride % 4 and not c.off for _, c in g), "scalar fallback"
    assert any(P.guard_entered(c.V) and P.u3_chunks(c.V) for c in vec), "c < nv guard and a chunk only u = 3 loads"
    for c in vec:
        kinds = dict(P.greedy_plants(c.V))
        assert all(f"tail{i}" in kinds for i in range(c.V % 4))
        if c.V % 4 and c.V >= 4:
            a, b = kinds["tie-vec-tail"]
            assert a < 4 * (c.V // 4) <= b
    assert any(np.isneginf(c.logits).sum(axis=1).max() == c.V - 1 for _, c in g if c.V > 1)
    assert any(c.temps is None for _, c in g) and any(c.temps is not None and {0.0, -1.0, 0.5, 2.0} <= set(c.temps.tolist()) for _, c in g)
    assert any((c.logits.max(axis=1) < 0).any() and P.guard_entered(c.V) for c in vec), "all-negative row where the guard is entered"

    t = [lz.build() for lz in TOPK]
    assert {c.top_k for c in t} >= set(P.TOPK_KS)
    assert any(1 < c.top_k and c.top_k > c.V for c in t) and any(c.top_k == c.V for c in t) and any(c.V < 256 for c in t)
    assert any(c.V == 128256 for c in t)
    assert any(c.top_k <= 0 and c.V < P.TOPK_MAX for c in t), "pure top-p with fewer entries than the candidate cap"
    keff = lambda c: min(c.V, P.TOPK_MAX if c.top_k <= 0 else min(c.top_k, P.TOPK_MAX))
    assert any(keff(c) & (keff(c) - 1) for c in t), "padding to a power of two"
    assert any(c.stride > c.V for c in t) and any(c.off for c in t)
    f32 = lambda p: float(np.float32(p))
    all_ps = {f32(p) for p in P.TOPK_PS}
    ps = set()
    for c in t:
        ps |= {("default", f32(c.top_p))} if c.top_p_list is None else {("row", float(p)) for p in c.top_p_list}
    assert ps >= {(w, p) for w in ("default", "row") for p in (1.0, 2.0)} and {p for w, p in ps if w == "row"} >= all_ps
    assert {p for w, p in ps if w == "default"} >= all_ps
    assert all({0.0, 0.5, float(P.RND_TOP)} <= set(c.rnd.tolist()) for c in t)
    for c in t:
        if c.family == "topk-masked":
            finite = np.isfinite(c.logits).sum(axis=1)
            assert (finite < keff(c)).all()
            assert any(c.tp(b) >= 1 and c.rnd[b] == P.RND_TOP for b in range(c.B))
        if c.family == "topk-ties":
            assert c.V % 256
            for b in range(c.B):
                x = c.x(b)
                kth = np.sort(x)[::-1][keff(c) - 1]
                assert (x == kth).sum() > 1 and (x > kth).sum() < keff(c) < (x >= kth).sum(), (c.name, b)
