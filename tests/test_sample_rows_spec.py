"""The per-request sampler's specification on the CPU: the generator's known answers and range, and the conditions every case of
tests/sample_rows.py has to meet before it may be held against the device (planted greedy answers, poison, the uncompared cap)."""
import numpy as np
import pytest

from tests import postproc as P
from tests import sample_rows as S

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = S.philox4x32_10(counter, key)
    assert tuple(int(w) for w in got) == want


def test_word0_places_seed_and_draw():
    """key = (seed lo, seed hi), counter = (n lo, n hi, 0, 0)"""
    seed, n = 0x299F31D0A4093822, 0x85A308D3243F6A88
    want = S.philox4x32_10((0x243F6A88, 0x85A308D3, 0, 0), (0xA4093822, 0x299F31D0))[0]
    assert int(S.word0([seed], [n])[0]) == int(want)
    assert int(S.word0([0], [0])[0]) == 0x6627E8D5
    assert int(S.word0([2 ** 64 - 1], [2 ** 64 - 1])[0]) == int(S.philox4x32_10((0xFFFFFFFF, 0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF))[0])


def test_uniform_range_and_exactness():
    w = np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint32)
    u = S.u_from_word(w)
    assert u.dtype == np.float32
    assert u[0] == 0 and u[1] == 0 and u[2] == np.float32(2.0 ** -24)
    assert u[-1] == u[-2] == P.RND_TOP == np.float32(1.0 - 2.0 ** -24)
    assert (u.astype(np.float64) == (w >> 8).astype(np.float64) / 2.0 ** 24).all()         # exact: no rounding anywhere
    rng = np.random.RandomState(0)
    seeds = rng.randint(0, 2 ** 63, size=4096).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    draws = rng.randint(0, 2 ** 40, size=4096).astype(np.uint64)
    w = S.word0(seeds, draws)
    u = S.uniform(seeds, draws)
    assert (u >= 0).all() and (u < 1).all()
    assert (u.astype(np.float64) * 2.0 ** 24 == (w >> 8)).all()
    assert 0.45 < float(u.mean()) < 0.55


def test_distinct_pairs_give_distinct_words():
    seeds = np.array([0, 1, 2, 3, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 64 - 1], dtype=np.uint64)
    draws = np.array([0, 1, 2, 3, 255, 256, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1], dtype=np.uint64)
    s, n = np.meshgrid(seeds, draws, indexing="ij")
    w = S.word0(s.ravel(), n.ravel())
    assert len(set(w.tolist())) == w.size


def test_splitmix64_known_answers():
    """the sequence of the reference implementation (Vigna) from state 0: splitmix64(0 + n * golden) is what we call splitmix64(x) at x = (n - 1) * golden"""
    assert S.splitmix64(0) == 0xE220A8397B1DCDAF
    assert S.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_pattern_rows():
    for B in S.GRID_B:
        for pat in S.PATTERNS:
            g = S.pattern_rows(pat, B)
            assert len(g) == B
            if pat == "all-greedy":
                assert all(g)
            if pat == "all-sampling":
                assert not any(g)
            if B >= 2 and pat == "sampling-greedy":
                assert not g[0] and g[-1]
            if B >= 2 and pat == "greedy-sampling":
                assert g[0] and not g[-1]


@pytest.fixture(scope="module")
def family_counts():
    """every case built once: {family: [sampling rows, uncompared]}, and the names seen"""
    counts = {f: [0, 0] for f in S.FAMILIES}
    seen = {"V": set(), "B": set(), "ds": set(), "off": set(), "k": set(), "p": set(), "t": set(), "pattern": set()}
    for lz in S.all_cases():
        c = lz.build()
        _, n_s, n_unc = c.check_assertions()
        counts[c.family][0] += n_s
        counts[c.family][1] += n_unc
        seen["V"].add(c.V); seen["B"].add(c.B); seen["ds"].add(c.stride - c.V); seen["off"].add(c.off)
        seen["k"] |= set(c.top_k.tolist()); seen["p"] |= set(c.top_p.tolist())
        seen["t"] |= set([None] if c.temps is None else c.temps.tolist())
    return counts, seen


def test_cases_hold_their_conditions_and_the_uncompared_cap(family_counts):
    counts, _ = family_counts
    for fam, (n_s, n_unc) in counts.items():
        assert n_s > 0, fam
        assert n_unc <= P.UNCOMPARED_CAP * n_s, (fam, n_unc, n_s)


def test_cases_cover_the_grid(family_counts):
    _, seen = family_counts
    assert set(S.GRID_V) <= seen["V"] and set(S.GRID_B) <= seen["B"] and {0, 2, 6} <= seen["ds"] and {0, 1, 2, 3} <= seen["off"]
    assert set(S.KS) <= seen["k"]
    assert set(np.float32(p) for p in S.PS) <= set(np.float32(p) for p in seen["p"])
    assert set(np.float32(t) for t in S.TS) <= set(np.float32(t) for t in seen["t"] if t is not None) and None in seen["t"]


def test_q3_case_has_teeth_on_the_cpu():
    c = S.q3_case()
    rows, _, n_unc = c.check_assertions()
    assert n_unc == 0 and rows[1][0] == 321
    # the same row under ONE batch-wide top_k of 50 and the same number: not the arg-max, and decided by a wide margin
    tok, margin, _, _ = P.topk_ref(c.x(1), 50, 1.0, c.rnd[1])
    assert tok != 321 and margin >= P.MARGIN
