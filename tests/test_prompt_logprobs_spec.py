"""Prompt logprobs on the CPU: the float64 reference on rows worked by hand, the listing of a step's positions, the conditions every case of
tests/prompt_logprobs.py has to meet before it may be held against the device, the checker accepting the reference itself and rejecting
seven mutated references in every family each is built for."""
import numpy as np
import pytest

from tests import postproc as P
from tests import prompt_logprobs as PL
from tests import top_logprobs as T


@pytest.fixture(scope="module")
def cases():
    """every case built once, its assertions held (the reference of each is computed here and kept)"""
    out = []
    for lz in PL.all_cases():
        c = lz.build()
        c.check_assertions()
        out.append(c)
    return out


def test_reference_on_rows_worked_by_hand():
    x = np.array([1.0, 3.0, 3.0, -np.inf, 0.0], dtype=np.float32)
    lse = 3.0 + np.log(2.0 + np.exp(-2.0) + np.exp(-3.0))
    for t, rank in ((1, 0), (2, 1), (0, 2), (4, 3), (3, 4)):          # 2 ties with 1: the lower index ranks first
        lp, r, tok, tlp, log_s, l2 = PL.ref_position(x, t, 3)
        assert r == rank and abs(l2 - lse) < 1e-12 and tok.tolist() == [1, 2, 0]
        assert (np.isneginf(lp) if t == 3 else abs(lp - (float(x[t]) - lse)) < 1e-12)
        if t in (1, 2, 0):
            assert lp == tlp[tok.tolist().index(t)]
    # -0 equals +0: index order; n = 0 gives no entries; entries behind the vocabulary are padding
    z = np.array([-0.0, 0.0, -0.0, -1.0], dtype=np.float32)
    assert [PL.ref_position(z, t, 0)[1] for t in range(4)] == [0, 1, 2, 3]
    assert PL.ref_position(z, 1, 0)[2].size == 0
    lp, r, tok, tlp, _, _ = PL.ref_position(z, 3, 6)
    assert tok.tolist() == [0, 1, 2, 3, -1, -1] and np.isneginf(tlp[4:]).all() and r == 3


def test_listing_and_clamp():
    seq = np.array([0, 1, 2, 4, 13, 16, 26])             # lengths 1 (decode), 1, 2, 9, 3, 10
    rows, ntop = PL.positions(seq, [0, 5, 0, 20, -1, 1])
    assert rows.tolist() == [2] + list(range(4, 12)) + list(range(16, 25))
    assert ntop.tolist() == [0] + [20] * 8 + [1] * 9
    assert PL.positions(seq, [-1] * 6)[0].size == 0 and PL.positions(seq, [3, 3, -1, -1, -1, -1])[0].size == 0
    assert [PL.clamp_ask(n) for n in (-7, -1, 0, 1, 20, 21, 1 << 30)] == [-1, -1, 0, 1, 20, 20, 20]


def test_cases_cover_the_grid(cases):
    fam = {f: {"V": set(), "vec": set()} for f in PL.FAMILIES}
    seen = {"R": set(), "off": set(), "n": set(), "kinds": {k: 0 for k in ("token0", "last", "tie", "mixed-zero", "masked", "in-top", "not-in-top")}}
    for c in cases:
        assert c.stride > c.V and (c.ask == -1).any()
        seen["R"].add(c.P); seen["off"].add(c.off); seen["n"] |= set(c.ntop.tolist())
        if c.family in fam:
            fam[c.family]["V"].add(c.V); fam[c.family]["vec"].add(c.uses_vector_path())
            assert ((c.seq[1:] - c.seq[:-1] == 1) & (c.ask >= 0)).any(), "an asking request of one token"
        for j, r in enumerate(c.rows):
            x, t = c.logits[int(r)], int(c.tokens[r + 1])
            k = seen["kinds"]
            k["token0"] += t == 0; k["last"] += t == c.V - 1; k["masked"] += bool(np.isneginf(x[t]))
            same = x == x[t]
            k["tie"] += same.sum() > 1
            k["mixed-zero"] += x[t] == 0 and np.signbit(x[same]).any() and not np.signbit(x[same]).all()
            hit = t in c.reference()[j][2].tolist()
            k["in-top"] += hit; k["not-in-top"] += c.ntop[j] > 0 and not hit
    for f, s in fam.items():
        assert s["V"] == set(PL.GRID_V) and s["vec"] == {True, False}, (f, s)
    assert seen["R"] >= {1, 2, 64} and seen["off"] == {0, 1, 2, 3} and seen["n"] == {0, 1, 5, 20}
    assert all(v >= 20 for v in seen["kinds"].values()), seen["kinds"]


def test_checker_accepts_the_reference_and_sees_the_guards(cases):
    for c in cases:
        fails, frac = PL.check(c, PL.as_outputs(c))
        assert not fails and frac < 1.0, (c.name, fails[:3], frac)      # (float32 rounding of the float64 answer: the bound's last term)
    c = next(c for c in cases if c.P == 64 and c.V == 257)
    j0 = int(np.flatnonzero(c.ntop == 0)[0])
    jn = int(np.flatnonzero((c.ntop > 0) & (c.ntop < PL.NMAX))[0])
    for what, key, idx in (("row behind the last", "lp", c.P), ("row behind the last", "rank", c.P), ("row behind the last", "top_tok", (c.P, 0)),
                           ("top slot of an n = 0 position", "top_lp", (j0, 0)), ("slot behind n", "top_tok", (jn, int(c.ntop[jn])))):
        out = PL.as_outputs(c)
        out[key][idx] = 0
        assert PL.check(c, out)[0], (what, key)
    out = PL.as_outputs(c)
    j = next(j for j in range(c.P) if np.isfinite(c.reference()[j][0]) and c.tokens[c.rows[j] + 1] not in c.reference()[j][2])
    lp, _, _, _, log_s, lse = c.reference()[j]
    out["lp"].view(np.float32)[j] += np.float32(4 * T.entry_bound(c.V, log_s, lse, lp) + 1e-6)
    assert PL.check(c, out)[0]
    out = PL.as_outputs(c)                               # the target inside its own top-n with other bits
    j = next(j for j in range(c.P) if np.isfinite(c.reference()[j][0]) and c.tokens[c.rows[j] + 1] in c.reference()[j][2])
    out["lp"][j] ^= 1
    assert any("differ from its own entry" in f for f in PL.check(c, out)[0])
    out = PL.as_outputs(c)
    out["rank"][0] += 1
    assert PL.check(c, out)[0]


@pytest.mark.parametrize("name", PL.ALL_MUTANTS)
def test_checker_rejects_the_mutant(cases, name):
    caught = {f: 0 for f in PL.mutant_families(name)}
    for c in cases:
        if c.family in caught and c.P:
            caught[c.family] += bool(PL.check(c, PL.mutant_outputs(c, name))[0])
    assert all(v > 0 for v in caught.values()), (name, caught)


def test_next_request_mutant_passes_where_nothing_follows(cases):
    """the two listing mutants differ: only "last-position-included" shows when the asking request is the step's last"""
    for c in cases:
        if c.family == "last-request":
            assert not PL.check(c, PL.mutant_outputs(c, "last-row-against-next-request"))[0]
            assert PL.check(c, PL.mutant_outputs(c, "last-position-included"))[0]
