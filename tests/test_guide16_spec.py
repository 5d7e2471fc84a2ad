"""The numpy reference of the wide guide build (tests/guide16.py) against a brute-force walk, and its named mutants: each must differ from
the reference somewhere on the operator test's own inputs, or that test could not tell a kernel with that mistake from a correct one.
No case is vacuous: every case of more than 256 states has rows with set and with clear bits at states >= 256, reaches state 255, crosses
255 / 256 in both directions and has a state >= 256 that differs from the state 256 below it in acceptance and in its row."""
import numpy as np
import pytest

from tests import guide as G8
from tests import guide16 as G

# the case on the golden model's 420 pieces gets stand-ins of the same kind here (letters, the space, byte pieces, multi-byte pieces, empty
# ids), so that its automaton goes through the same checks as the others; the GPU test reads the model's own
STAND_IN = ([b""] * 3 + [bytes([b]) for b in range(256)] + [b" " + w for w in (b"a", b"e", b"the", b"in", b"on", b"at")]
            + [bytes(np.random.default_rng(420).choice(list(b"aeinorst "), size=n)) for n in (2, 3, 4, 5, 7, 9, 12) * 22] + [b""])[:420]
SPECS = G.build_specs(spm_pieces=STAND_IN)
_MADE = {}


def case(i):
    if i not in _MADE:
        _MADE[i] = SPECS[i][1]()
    return _MADE[i]


SMALL = [i for i, (name, _) in enumerate(SPECS) if not name.startswith(("s4096", "s257_v128256", "s1000"))]
BRUTE = [i for i in SMALL if int(SPECS[i][0].split("_v")[1]) <= 65 or SPECS[i][0].startswith("chunk")]


def test_mutant_list():
    assert sorted(G.MUTANTS) == sorted(["state_low_byte", "dead_is_255", "dead_row_indexed", "last_chunk_dropped", "chunk_stride", "skip_last_byte",
                                        "end_in_non_accepting", "tail_bits"])


@pytest.mark.parametrize("idx", BRUTE, ids=lambda i: SPECS[i][0])
def test_reference_build_is_the_definition(idx):
    c = case(idx)
    want = G.brute_build(c.trans, c.accept, c.toks, set(c.ends), c.vocab)
    got = G.ref_allowed(c.trans, c.accept, c.toks, c.ends, c.vocab)
    assert (want == got).all()
    mask, anyf = G.ref_build(c.trans, c.accept, c.toks, c.ends, c.vocab)
    bits = np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")
    assert (bits[:, :c.vocab].astype(bool) == want).all()
    assert not bits[:, c.vocab:].any()
    assert (anyf == want.any(axis=1)).all()


def test_reference_build_large_sample():
    """the big cases: a sample of (state, token) pairs against the walk, the long tokens and the edges of the vocabulary among them"""
    rng = np.random.default_rng(5)
    for i in range(len(SPECS)):
        if i in BRUTE:
            continue
        c = case(i)
        mask, _ = G.ref_build(c.trans, c.accept, c.toks, c.ends, c.vocab)
        long_ids = [t for t in range(len(c.toks)) if len(c.toks[t]) >= 9][:20]
        for t in list(rng.integers(0, c.vocab, size=300)) + long_ids + [0, c.vocab - 1, len(c.toks), len(c.toks) - 1]:
            t = int(t)
            for s in (int(rng.integers(0, c.S)), min(255, c.S - 1), min(256, c.S - 1), c.S - 1):
                if t in c.ends:
                    want = bool(c.accept[s])
                else:
                    want = t < len(c.toks) and len(c.toks[t]) > 0 and G.walk(c.trans, s, c.toks[t]) != G.DEAD
                assert bool((int(mask[s, t >> 5]) >> (t & 31)) & 1) == want, (c.name, s, t)


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_build_mutant_is_told_apart(mutant):
    hit = []
    for i in SMALL:
        c = case(i)
        ref_img, ref_any = c.expect()
        mut_img, mut_any = c.expect(mutant)
        if not (G.same_bits(ref_img, mut_img) and G.same_bits(ref_any, mut_any)):
            hit.append(c.name)
    assert hit, f"no build case tells {mutant} from the reference"


def test_wide_mutants_need_wide_cases():
    """the three mistakes of a walk that is not really 16 bits wide show only beyond 255 states: the cases of up to 255 states do not see
    state_low_byte and dead_is_255, and every case of more than 256 states sees each of them"""
    for i in SMALL:
        c = case(i)
        ref = c.expect()
        for mutant in ("state_low_byte", "dead_is_255"):
            mut = c.expect(mutant)
            differs = not (G.same_bits(ref[0], mut[0]) and G.same_bits(ref[1], mut[1]))
            if c.S <= 255:
                assert not differs, (c.name, mutant)
            elif c.S > 256 and c.vocab >= 31:
                assert differs, (c.name, mutant)


@pytest.mark.parametrize("idx", range(len(SPECS)), ids=[n for n, _ in SPECS])
def test_case_is_not_vacuous(idx):
    c = case(idx)
    assert c.name == SPECS[idx][0]
    allowed = G.ref_allowed(c.trans, c.accept, c.toks, c.ends, c.vocab)
    assert c.trans.dtype == np.uint16 and ((c.trans < c.S) | (c.trans == G.DEAD)).all()
    assert 0 in c.ends and c.vocab - 1 in c.ends
    # what pplhip_guide_load16 demands: every state has a live byte or accepts
    assert ((c.trans != G.DEAD).any(axis=1) | (c.accept != 0)).all()
    if c.S * c.vocab > 1:
        assert allowed.any() and not allowed.all()
    if c.S <= 256:
        return
    hi = allowed[256:]
    if c.vocab > 1:
        assert any(r.any() and not r.all() for r in hi), "no row at a state >= 256 with set and clear bits"
    else:
        assert hi.any() or not hi.all()
    t = c.trans
    live = t != G.DEAD
    assert (t[0] == 255).any() and live[255].any(), "state 255 is not reached from the start, or is not live"
    assert (live[:256] & (t[:256] >= 256)).any() and (live[256:] & (t[256:] <= 255)).any(), "no transition across 255 / 256"
    assert any(c.accept[s] != c.accept[s - 256] and (t[s] != t[s - 256]).any() for s in range(256, c.S))


def test_cases_cover_the_shapes():
    shapes = {tuple(int(x) for x in n.replace("chunk_", "").replace("s", "").split("_v")) for n, _ in SPECS if "_v" in n}
    for S in (1, 255, 256, 257):
        for V in (1, 31, 32, 33, 63, 64, 65, 257):
            assert (S, V) in shapes
    assert {(4096, 2048), (257, 128256), (1000, 32000)} <= shapes
    assert {G.CHUNK - 1, G.CHUNK, G.CHUNK + 1, 2 * G.CHUNK + 1} <= {S for S, _ in shapes}
    assert len(STAND_IN) == 420 and "s4096_spm420" in [n for n, _ in SPECS]
    big = case([n for n, _ in SPECS].index("s1000_v32000"))
    assert any(len(t) == 64 for t in big.toks) and any(len(t) == 9 for t in big.toks) and any(len(t) == 0 for t in big.toks)


def test_widened_narrow_table_gives_the_narrow_reference():
    """a narrow automaton widened to 16 bits has the mask of tests/guide.py's reference: the two definitions agree where both apply"""
    rng = np.random.default_rng(11)
    trans, accept = G8.random_dfa(rng, 255)
    toks = G8.random_vocab(rng, 300)
    a, _ = G8.ref_build(trans, accept, toks, {0, 299}, 300)
    b, _ = G.ref_build(G.widen(trans), accept, toks, {0, 299}, 300)
    assert G.same_bits(a, b)
