"""The numpy reference of guided decoding (tests/guide.py) against a brute-force walk, token by token and state by state, and the named
mutants of tests/guide.py: each must differ from the reference somewhere on the operator test's own inputs, or that test could not tell
a kernel with that mistake from a correct one."""
import numpy as np
import pytest

from tests import guide as G

BUILD = G.build_cases(spm_pieces=None)
MASK = G.mask_cases()
BUILD_MUTANTS = ("skip_last_byte", "swap_ballot_words", "end_in_non_accepting", "allow_empty", "tail_bits", "dead_is_row_255")
MASK_MUTANTS = ("state_stride",)


def test_mutant_lists_cover_every_name():
    assert sorted(BUILD_MUTANTS + MASK_MUTANTS) == sorted(G.MUTANTS)


@pytest.mark.parametrize("idx", [i for i, c in enumerate(BUILD) if c.vocab <= 257], ids=lambda i: BUILD[i].name)
def test_reference_build_is_the_definition(idx):
    c = BUILD[idx]
    want = G.brute_build(c.trans, c.accept, c.toks, set(c.ends), c.vocab)
    got = G.ref_allowed(c.trans, c.accept, c.toks, c.ends, c.vocab)
    assert (want == got).all()
    mask, anyf = G.ref_build(c.trans, c.accept, c.toks, c.ends, c.vocab)
    for s in range(c.S):
        for t in range(c.vocab):
            assert bool((int(mask[s, t >> 5]) >> (t & 31)) & 1) == bool(want[s, t])
        assert int(anyf[s]) == int(want[s].any())
    tail = G.words(c.vocab) * 32 - c.vocab
    if tail:
        assert (mask[:, -1] >> np.uint32(32 - tail) == 0).all()


def test_reference_build_large_sample():
    """the big vocabularies: a sample of (state, token) pairs against the walk"""
    rng = np.random.default_rng(5)
    for c in BUILD:
        if c.vocab <= 257:
            continue
        mask, _ = G.ref_build(c.trans, c.accept, c.toks, c.ends, c.vocab)
        long_ids = [t for t in range(len(c.toks)) if len(c.toks[t]) == 64][:20]
        for t in list(rng.integers(0, c.vocab, size=300)) + long_ids + [0, c.vocab - 1, len(c.toks), len(c.toks) - 1]:
            s = int(rng.integers(0, c.S))
            t = int(t)
            if t in c.ends:
                want = bool(c.accept[s])
            else:
                want = t < len(c.toks) and len(c.toks[t]) > 0 and G.walk(c.trans, s, c.toks[t]) != G.DEAD
            assert bool((int(mask[s, t >> 5]) >> (t & 31)) & 1) == want, (c.name, s, t)


def test_reference_edit_is_the_definition():
    for c in MASK:
        got = c.expect()
        want = c.image()
        for b in range(c.B):
            g, s = int(c.guide_slots[b]), int(c.states[b])
            if g < 0:
                continue
            for v in range(c.V):
                if not (int(c.masks[g, s, v >> 5]) >> (v & 31)) & 1:
                    want[c.off + b * c.stride + v] = G.NINF
        assert G.same_bits(got, want), c.name
        # nothing outside the asking rows' [0, V) moved
        touched = np.zeros(len(want), dtype=bool)
        for b in range(c.B):
            if c.guide_slots[b] >= 0:
                touched[c.off + b * c.stride: c.off + b * c.stride + c.V] = True
        assert G.same_bits(got[~touched], c.image()[~touched])


@pytest.mark.parametrize("mutant", BUILD_MUTANTS)
def test_build_mutant_is_told_apart(mutant):
    hit = []
    for c in BUILD:
        if c.vocab > 257 and hit:
            continue
        ref_img, ref_any = c.expect()
        mut_img, mut_any = c.expect(mutant)
        if not (G.same_bits(ref_img, mut_img) and G.same_bits(ref_any, mut_any)):
            hit.append(c.name)
    assert hit, f"no build case tells {mutant} from the reference"


@pytest.mark.parametrize("mutant", MASK_MUTANTS)
def test_mask_mutant_is_told_apart(mutant):
    assert any(not G.same_bits(c.expect(), c.expect(mutant)) for c in MASK)


def test_cases_cover_the_shapes():
    vocabs = {c.vocab for c in BUILD}
    assert set(G.SMALL_V) | {32000, 128256} <= vocabs
    assert {1, 2, 255} <= {c.S for c in BUILD}
    for c in BUILD:
        assert 0 in c.ends and c.vocab - 1 in c.ends
    assert any(len(t) == 64 for c in BUILD if c.vocab >= 32000 for t in c.toks)
    assert any(len(t) == 0 for c in BUILD for t in c.toks)
    assert {c.V for c in MASK} == {33, 32000}
    assert any(c.stride == c.V for c in MASK) and any(c.stride > c.V and c.stride % 4 == 0 for c in MASK)
    assert any(c.off % 4 for c in MASK) and any(c.stride % 4 for c in MASK)
    for c in MASK:
        assert (c.guide_slots < 0).any() and {0, 1} <= set(c.guide_slots.tolist()) and {0, 254} <= set(c.states.tolist())
