"""tests/chain.py has teeth: every named mutant of the chain changes a compared output on the chain cases, a row that asks for nothing is
the plain chain bit for bit, and with the chosen seeds the reused sampler check leaves no row of any case out of its exact comparison.
CPU only: the reference against itself."""
import numpy as np
import pytest

from tests import chain as C
from tests import logit_rules as R
from tests import top_logprobs as T

CASES = [(batch, pen) for batch in (0, 1) for pen in (True, False)]


@pytest.fixture(scope="module")
def tables():
    tb = C.Tables()
    tb.assert_live()
    return tb


@pytest.fixture(scope="module")
def runs(tables):
    """the reference run of every case, computed once"""
    return {c: C.run_case(tables, *c) for c in CASES}


def test_the_pattern_table():
    seen = sorted(p for pats in C.PATTERNS for p in pats)
    assert seen == list(range(16))                       # every subset of the four features, once
    assert all(len(p) == 8 for p in C.PATTERNS)
    p0 = C.PATTERNS[0]
    assert p0[C.ROW_NONE] == 0 and p0[C.ROW_ALL] == 15 and p0[C.ROW_GUIDE_ONLY] == C.GUIDE
    assert p0[C.ROW_GREEDY_BEHIND_SAMPLING - 1] & C.SAMPLED and not p0[C.ROW_GREEDY_BEHIND_SAMPLING] & C.SAMPLED
    assert min(C.ROW_NONE, C.ROW_ALL, C.ROW_GUIDE_ONLY, C.ROW_GREEDY_BEHIND_SAMPLING) >= 1
    for pats, slots in zip(C.PATTERNS, C.SLOTS):
        assert sorted(slots) == list(range(C.CAP)) and list(slots) != list(range(C.CAP))
        assert any(pats[b] & C.SAMPLED and not pats[b + 1] & C.SAMPLED for b in range(7))
        for bit in (C.GUIDE, C.RULE, C.TOPN, C.SAMPLED):    # every list is interleaved: asking and non-asking rows on both sides
            asks = [bool(p & bit) for p in pats]
            assert 0 < sum(asks) < 8 and asks != sorted(asks) and asks != sorted(asks, reverse=True)
        for g in (0, 1):                                 # more than one row per guide in the two batches together
            assert sum(1 for ps in C.PATTERNS for b, p in enumerate(ps) if p & C.GUIDE and b % 2 == g) >= 2


def test_no_row_is_left_out_of_the_exact_comparison(runs):
    """postproc.check_sample compares a sampling row's token only where its margin is >= postproc.MARGIN: with chain.SEED_BASE every
    sampling row of every step of every case has that margin"""
    n = 0
    for c, run in runs.items():
        for s, (_, st, res) in enumerate(run):
            assert C.left_out(res) == [], (c, s, [(b, res.rows[b][2]) for b in C.left_out(res)])
            n += sum(1 for b in range(st.B) if not res.rcase.greedy(b))
            assert not C.check_tokens(res, res.tokens, res.logprobs)          # (the reference passes its own check)
    assert n == 4 * 2 * 2 * C.STEPS                      # four sampling rows per batch


def test_the_cases_reach_what_they_are_for(runs):
    for (batch, pen), run in runs.items():
        flags = np.array([st.flags for _, st, _ in run])
        assert (flags == 3).any() and (flags == 1).any()                      # the stop-suppress bit is there and leaves
        for b in range(8):
            if C.PATTERNS[batch][b] & C.RULE:
                gone = [s for s in range(C.STEPS) if not flags[s, b] & 2]
                assert gone and gone[0] == C.MIN_NEW[b % 4], (batch, b, gone)  # exactly at min_new_tokens
        states = np.array([st.guide_states for _, st, _ in run])
        assert (states[1:] != states[:-1]).any()                              # guides move
        assert [int(st.draws[0]) for _, st, _ in run] == list(range(C.STEPS))
        assert all(len(res.asked) == 4 for _, _, res in run)
        if pen:
            for s, (_, st, res) in enumerate(run):
                plain_rows = [b for b in range(8) if C.PATTERNS[batch][b] == 0]
                assert set(C.counts_show(st, res)) >= {b for b in range(8) if not C.PATTERNS[batch][b] & (C.GUIDE | C.RULE)} - set(plain_rows)


def _differs(st, ref, mut, state=None):
    """the compared outputs on which a mutated result differs from the reference: image bits, tokens, top-N tokens; logprobs only beyond
    the bound the device is held to"""
    out = []
    if not R.same_bits(ref.edited, mut.edited):
        out.append("edited image")
    if not R.same_bits(ref.front, mut.front):
        out.append("image in front of the sampler")
    if (ref.tokens != mut.tokens).any():
        out.append("tokens")
    for b in ref.asked:
        w, g = ref.top_of_row[b], mut.top_of_row.get(b)
        if g is None or len(g[0]) != len(w[0]) or (g[0] != w[0]).any():
            out.append(f"top-N tokens of row {b}")
            continue
        for e in range(len(w[0])):
            if np.isfinite(w[1][e]) and not abs(g[1][e] - w[1][e]) <= T.entry_bound(st.vocab, w[2], w[3], w[1][e]):
                out.append(f"top-N logprobs of row {b}")
                break
    return out


@pytest.mark.parametrize("mutant", C.STEP_MUTANTS)
def test_step_mutants_are_caught(tables, runs, mutant):
    hits = {}
    for (batch, pen), run in runs.items():
        if mutant in C.NEEDS_PENALTY and not pen:
            continue
        for s, (state, st, ref) in enumerate(run):
            d = _differs(st, ref, C.ref_chain(st, state, pen, mutant))
            if d:
                hits[(batch, pen, s)] = d
    print(mutant, {k: v[:3] for k, v in list(hits.items())[:4]})
    exact = [d for ds in hits.values() for d in ds if "logprobs" not in d]
    assert hits and exact, f"{mutant}: no case tells it from the reference by a token or an image bit"
    want = 2 if mutant in C.NEEDS_PENALTY else 4          # in every case it can act in
    assert len({k[:2] for k in hits}) == want, (mutant, sorted(hits))


@pytest.mark.parametrize("mutant", C.ADVANCE_MUTANTS)
def test_advance_mutants_are_caught(tables, runs, mutant):
    hits = {}
    for (batch, pen), run in runs.items():
        for s in range(C.STEPS - 1):
            state, st, ref = run[s]
            bad = state.copy()
            C.advance(bad, ref.tokens, ref.cm, mutant)
            nxt_state, nxt_st, nxt_ref = run[s + 1]
            d = _differs(nxt_st, nxt_ref, C.ref_chain(bad.step(nxt_st.logits), bad, pen))
            if d:
                hits[(batch, pen, s + 1)] = d
    print(mutant, {k: v[:3] for k, v in list(hits.items())[:4]})
    exact = [d for ds in hits.values() for d in ds if "logprobs" not in d]
    assert exact, f"{mutant}: no case tells it from the reference by a token or an image bit"
    assert len({k[:2] for k in hits}) == 4, (mutant, sorted(hits))


def test_advance_restates_itself(tables, runs):
    """advancing a copy of a step's state with the reference's tokens gives the next step's lists"""
    for (batch, pen), run in runs.items():
        for s in range(C.STEPS - 1):
            state, st, ref = run[s]
            nxt = state.copy()
            C.advance(nxt, ref.tokens, ref.cm)
            want = run[s + 1][0]
            for k in ("guide_states", "flags", "draws", "gen", "prompt_ask", "start_pos", "seqs", "dec"):
                assert getattr(nxt, k) == getattr(want, k), (batch, pen, s, k)
            assert (nxt.cm == want.cm).all()
            assert all(a == -1 for a in nxt.prompt_ask)
        assert any(a >= 0 for a in run[0][0].prompt_ask)


@pytest.mark.parametrize("batch,pen", CASES)
def test_a_row_that_asks_for_nothing_is_the_plain_chain(tables, runs, batch, pen):
    """rows that ask for nothing come out of the mixed chain as out of the chain in which nobody asks, bit for bit -- fed the same tokens"""
    mixed = runs[(batch, pen)]
    plain_rows = [b for b in range(8) if C.PATTERNS[batch][b] == 0]
    nobody = C.start_state(tables, batch, asking=())
    for s, (_, st, res) in enumerate(mixed):
        pst = nobody.step(st.logits)
        pres = C.ref_chain(pst, nobody, pen)
        assert R.same_bits(pres.edited, st.logits) and pres.asked == []
        for b in plain_rows:
            assert R.same_bits(res.edited[b], st.logits[b]) and R.same_bits(res.front[b], pres.front[b]), (s, b)
            assert res.tokens[b] == pres.tokens[b] and res.logprobs[b] == pres.logprobs[b], (s, b)
            assert R.same_bits(res.front[b], st.logits[b])                   # neutral penalties at temperature 1: nothing moves
        C.advance(nobody, res.tokens, pres.cm)           # (the mixed run's tokens: the same count map rows for the plain rows)
    # and a row asking alone gets what it got in the mixed batch
    for b in ((C.ROW_ALL, C.ROW_GUIDE_ONLY, C.ROW_GREEDY_BEHIND_SAMPLING) if batch == 0 else (0, 5)):
        alone = C.start_state(tables, batch, asking=(b,))
        for s, (_, st, res) in enumerate(mixed):
            ast = alone.step(st.logits)
            ares = C.ref_chain(ast, alone, pen)
            assert R.same_bits(ares.edited[b], res.edited[b]) and R.same_bits(ares.front[b], res.front[b]), (b, s)
            assert ares.tokens[b] == res.tokens[b] and ares.logprobs[b] == res.logprobs[b], (b, s)
            if b in res.top_of_row:
                assert ares.asked == [b] and (ares.top[0][0] == res.top_of_row[b][0]).all() and (ares.top[0][1] == res.top_of_row[b][1]).all()
            C.advance(alone, res.tokens, ares.cm)


def test_check_penalty_accepts_the_reference_and_sees_a_count(runs):
    for (batch, pen), run in runs.items():
        if not pen:
            continue
        for s, (_, st, res) in enumerate(run):
            assert C.check_penalty(st, res, res.front) == [], (batch, s)
            b = C.counts_show(st, res)[0]
            tok = int(st.seqs[b][-1])
            off = res.front.copy()                       # what a count one too high would leave in that token's logit
            off[b, tok] = np.float32(off[b, tok] - st.freq[b] / (st.temps[b] if st.temps[b] > 0 else 1.0))
            assert C.check_penalty(st, res, off), (batch, s, b)
            dead = np.argwhere(np.isneginf(res.edited[:, :st.vocab]))
            if dead.size:
                rz = res.front.copy()
                rz[tuple(dead[0])] = np.float32(-1e30)
                assert C.check_penalty(st, res, rz), (batch, s)
