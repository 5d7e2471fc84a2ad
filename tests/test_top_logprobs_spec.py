"""Top-N logprobs on the CPU: the conditions every case of tests/top_logprobs.py has to meet before it may be held against the device
(planted gaps or exact ties between adjacent ranks, poison, the grid), the checker accepting the reference itself, and the checker
rejecting five mutated references in every family each is built for."""
import numpy as np
import pytest

from tests import postproc as P
from tests import top_logprobs as T


@pytest.fixture(scope="module")
def cases():
    """every case built once, its assertions held (the reference of each is computed here and kept)"""
    out = []
    for lz in T.all_cases():
        c = lz.build()
        c.check_assertions()
        out.append(c)
    return out


def test_reference_on_a_row_worked_by_hand():
    # t = 0.5: x = 2 * logits = [2, 6, 6, -inf, 0]; ranking 1, 2 (tie: lower index first), 0, 4, 3
    x = P.scaled(np.array([1.0, 3.0, 3.0, -np.inf, 0.0], dtype=np.float32), 0.5)
    tok, lp, log_s, lse = T.ref_row(x, 7)
    assert tok.tolist() == [1, 2, 0, 4, 3, -1, -1]
    want_lse = 6.0 + np.log(2.0 + np.exp(-4.0) + np.exp(-6.0))
    assert abs(lse - want_lse) < 1e-12 and abs(log_s - (want_lse - 6.0)) < 1e-12
    assert np.allclose(lp[:4], np.array([6.0, 6.0, 2.0, 0.0]) - want_lse, rtol=0, atol=1e-12)
    assert np.isneginf(lp[4:]).all()
    # -0 ties with +0: index order
    tok, _, _, _ = T.ref_row(np.array([-0.0, 0.0, -0.0, -1.0], dtype=np.float32), 3)
    assert tok.tolist() == [0, 1, 2]


def test_bound_is_the_formula():
    V = 32000
    assert T.mass_bound(V) == (125 + 8 + 2 * np.log(V) + 8) * 2.0 ** -24
    assert T.entry_bound(V, 1.5, 9.5, -60.0) == T.mass_bound(V) + (3.0 + 9.5 + 60.0) * 2.0 ** -24
    assert T.greedy_bound(V, 0.0, 0.0, 0.0) == (32 + 21 + 2 * np.log(V) + 8) * 2.0 ** -24
    assert T.entry_bound(128256, 11.8, 20.0, -70.0) < T.GAP / 100      # a swapped pair stands far outside it


def test_pattern_rows():
    for B in T.GRID_B:
        for pat in T.PATTERNS + ("none",):
            g = T.pattern_rows(pat, B)
            assert len(g) == B
            assert pat != "all" or all(g)
            assert pat != "none" or not any(g)
            if B >= 2 and pat == "first":
                assert g[0] and not g[-1]
            if B >= 2 and pat == "last":
                assert not g[0] and g[-1]
            if B >= 2 and pat == "alternating":
                assert g[0] and not g[1]


def test_cases_cover_the_grid(cases):
    fam = {f: {"V": set(), "n": set(), "vec": set()} for f in T.FAMILIES}
    seen = {"B": set(), "off": set(), "t": set(), "pattern": set(), "zero_mixed": 0}
    for c in cases:
        seen["B"].add(c.B); seen["off"].add(c.off)
        seen["t"] |= set([None] if c.temps is None else c.temps.tolist())
        seen["pattern"].add(c.name.split("-")[2])
        seen["zero_mixed"] += 0 < len(c.asked) < c.B
        assert c.stride > c.V
        if c.family in fam:
            fam[c.family]["V"].add(c.V); fam[c.family]["vec"].add(c.uses_vector_path())
            fam[c.family]["n"] |= set(int(c.nlp[b]) for b in c.asked)
    for f, s in fam.items():
        assert s["V"] == set(T.GRID_V) and s["n"] == set(T.NS) and s["vec"] == {True, False}, (f, s)
    assert seen["B"] == set(T.GRID_B) and seen["off"] == {0, 1, 2, 3} and seen["pattern"] == set(T.PATTERNS) | {"none"}
    assert set(np.float32(t) for t in T.TS) <= set(np.float32(t) for t in seen["t"] if t is not None) and None in seen["t"]
    assert seen["zero_mixed"] >= 10
    assert sum(1 for c in cases if c.family == "none" and not c.asked) == 3


def test_families_are_what_they_say(cases):
    n_straddle = n_zero_mix = n_short = 0
    for c in cases:
        for j, b in enumerate(c.asked):
            x, n = c.x(b), int(c.nlp[b])
            tok, lp, log_s, lse = c.reference()[j]
            if c.family == "ties" and c.V > n:
                order = np.argsort(-x, kind="stable")
                n_straddle += x[order[n - 1]] == x[order[n]]
                n_zero_mix += x[order[n - 1]] == 0 and np.signbit(x[order[:n + 1]]).any() and not np.signbit(x[order[:n + 1]]).all()
            if c.family == "masked":
                n_short += np.isfinite(x).sum() < min(n, c.V)
            if c.family == "flat":
                assert tok[:min(n, c.V)].tolist() == list(range(min(n, c.V)))
            if c.family == "needle" and c.V > 1:
                assert abs(log_s) < 1e-20 and (lp[1:min(n, c.V)] < -59.0).all() and (c.logits[b].max() - np.sort(c.logits[b])[-2]) == 60.0
    assert n_straddle >= 20 and n_zero_mix >= 3 and n_short >= 5, (n_straddle, n_zero_mix, n_short)


def test_checker_accepts_the_reference_and_sees_the_guards(cases):
    for c in cases:
        tok, lp = T.as_outputs(c, [r[:2] for r in c.reference()])
        fails, frac = T.check(c, tok, lp)
        assert not fails and frac < 1.0, (c.name, fails[:3], frac)      # (float32 rounding of the float64 answer: the bound's last term)
    c = next(c for c in cases if len(c.asked) >= 2 and int(c.nlp[c.asked[0]]) < T.NMAX)
    good = T.as_outputs(c, [r[:2] for r in c.reference()])
    for what, (r, e) in {"slot behind n": (0, int(c.nlp[c.asked[0]])), "row behind the last": (len(c.asked), 0)}.items():
        for which in (0, 1):
            out = [a.copy() for a in good]
            out[which][r, e] = 0
            assert T.check(c, *out)[0], (what, which)
    out = [a.copy() for a in good]
    lpf = out[1].view(np.float32)
    lpf[0, 0] += np.float32(4 * T.entry_bound(c.V, *c.reference()[0][2:], float(c.reference()[0][1][0])) + 1e-6)
    assert T.check(c, *out)[0]


@pytest.mark.parametrize("name", sorted(T.MUTANTS))
def test_checker_rejects_the_mutant(cases, name):
    caught = {f: 0 for f in T.MUTANTS[name][1]}
    for c in cases:
        if c.family in caught and c.asked:
            caught[c.family] += bool(T.check(c, *T.mutant_outputs(c, name))[0])
    assert all(v > 0 for v in caught.values()), (name, caught)
