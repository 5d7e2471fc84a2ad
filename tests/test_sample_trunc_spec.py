"""The min_p / typical_p rule without a GPU (tests/sample_trunc.py): trunc_ref against a brute-force chain of full-vocabulary filters, the
named mutants, the share of rows the margins leave out, and the exact cases' premises."""
import numpy as np
import pytest

from tests import postproc as P
from tests import sample_trunc as T


def _spec_rows():
    """(name, scaled row, top_k, top_p, min_p, typical_p, u): random rows, ties, -inf entries, k > V, V = 1"""
    rng = np.random.RandomState(5)
    out = []
    for i in range(60):
        V = (1, 2, 7, 33, 257, 1500)[i % 6]
        x = (rng.randn(V) * (0.5, 2.0, 4.0)[i % 3]).astype(np.float32)
        if i % 4 == 1 and V > 2:                        # plateaus, one of them at the maximum
            x[rng.choice(V, size=V // 2, replace=False)] = np.float32(0.25)
            x[rng.choice(V, size=min(3, V), replace=False)] = x.max()
        if i % 5 == 2 and V > 2:
            x[rng.choice(V, size=V // 3, replace=False)] = -np.inf
        k = (0, 5, 5000, -1, 40, 1024)[(i // 2) % 6]
        p = (2.0, 0.9, 0.5, 1.0)[(i // 3) % 4]
        mp = (0.0, 0.05, 0.5, 1.0, 3.0, float("nan"))[i % 6] if i % 7 else 0.2
        ty = (0.0, 0.2, 0.9, 0.5, 1.0)[(i // 2) % 5]
        out.append((f"spec{i}-V{V}", x, k, p, mp, ty, float(rng.rand())))
    # exact ties at the min_p edge: min_p = 1 keeps every tie of the maximum and nothing else
    x = np.array([1.0, 3.0, 3.0, -2.0, 3.0, 2.9999998], dtype=np.float32)
    out += [("tie-minp-one-u0", x, 0, 2.0, 1.0, 0.0, 0.0), ("tie-minp-one-u1", x, 0, 2.0, 1.0, 0.0, 0.99)]
    # a head and many equal others (tests/sample_trunc.py typical_head_case)
    c, _ = T.typical_head_case()
    out += [("typical-head", c.x(0), 0, 2.0, 0.0, 0.4, 0.1), ("typical-head-minp", c.x(0), 0, 2.0, 0.001, 0.4, 0.7)]
    # top-p cuts shorter than min_p does: keep = min, not max
    x = np.array([0.0, -0.1, -0.2, -0.3, -3.0, -9.0], dtype=np.float32)
    out += [("keep-min", x, 0, 0.5, 0.01, 0.0, 0.95), ("keep-min-typ", x, 0, 0.7, 0.01, 0.6, 0.95)]
    return out


ROWS = _spec_rows()


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_reference_equals_sequential_filters(row):
    name, x, k, p, mp, ty, u = row
    tok, margin, kept, lse = T.trunc_ref(x, k, p, mp, ty, u)
    btok, bkept = T.brute_ref(x, k, p, mp, ty, u)
    assert sorted(kept.tolist()) == bkept.tolist(), name
    assert tok == btok, name
    assert abs(lse - P._lse(x)) < 1e-12
    assert x[tok] > -np.inf


def test_defaults():
    x = ROWS[5][1]
    for mp, ty in ((0.0, 0.0), (-1.0, 1.0), (float("nan"), float("nan")), (0.0, 2.0)):
        assert not T.truncating(50, mp, ty)
        tok, _, kept, _ = T.trunc_ref(x, 50, 0.9, mp, ty, 0.37)
        wtok, _, cand, _ = P.topk_ref(x, 50, 0.9, 0.37)
        assert tok == wtok                               # both off: the top-k / top-p rule
    assert T.truncating(50, 0.1, 0.0) and T.truncating(0, 0.0, 0.5) and not T.truncating(1, 0.5, 0.5)
    assert T.trunc_ref(x, 0, 2.0, 7.0, 0.0, 0.5)[2].tolist() == T.trunc_ref(x, 0, 2.0, 1.0, 0.0, 0.5)[2].tolist()   # above 1 counts as 1


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_mutant_changes_a_kept_set(mutant):
    """every named wrong reading of the rule changes the kept set (or, for the pick's order, the token) of at least one committed row"""
    changed = []
    for name, x, k, p, mp, ty, u in ROWS:
        tok, _, kept, _ = T.trunc_ref(x, k, p, mp, ty, u)
        mtok, _, mkept, _ = T.trunc_ref(x, k, p, mp, ty, u, mutant=mutant)
        if sorted(kept.tolist()) != sorted(mkept.tolist()) or (mutant == "pick-s-order" and tok != mtok):
            changed.append(name)
    assert changed, mutant
    if mutant == "minp-strict":
        assert any(n.startswith("tie-minp-one") for n in changed)


@pytest.mark.parametrize("family", T.FAMILIES)
def test_margins_leave_out_at_most_the_cap(family):
    n_t = n_unc = 0
    for lz in T.all_cases():
        if lz.family != family:
            continue
        rows, t, unc = lz.build().check_assertions()
        n_t, n_unc = n_t + t, n_unc + unc
    assert n_t > 0 and n_unc <= P.UNCOMPARED_CAP * n_t, (family, n_unc, n_t)


def test_keep_edges_are_reached():
    """the keep-edge family reaches keep = 1, 2, 255, 256, 257, 1023 and 1024 on min_p alone, and kept sets cut by typical_p inside them"""
    seen, cut = set(), 0
    for lz in T.keep_cases():
        c = lz.build()
        for b in range(c.B):
            kept = T.trunc_ref(c.x(b), int(c.top_k[b]), float(c.top_p[b]), c.mp(b), c.ty(b), c.numbers()[b])[2]
            if T.norm_typical_p(c.ty(b)) == 0:
                seen.add(len(kept))
            else:
                cut += len(kept) < T.KEEPS[b // 5]
    assert seen >= set(T.KEEPS), seen
    assert cut >= 10


def test_exact_cases_premises():
    c, ties = T.minp_one_case()
    c.check_assertions()
    for b in range(c.B):
        tok, _, kept, _ = T.trunc_ref(c.x(b), int(c.top_k[b]), 2.0, c.mp(b), 0.0, c.rnd[b])
        assert sorted(kept.tolist()) == ties[b].tolist()
        assert tok == ties[b][min(int(float(c.rnd[b]) * len(ties[b])), len(ties[b]) - 1)]
    c, head = T.typical_head_case()
    assert abs(float(np.exp(c.x(0)[head] - P._lse(c.x(0)))) - 0.3) < 1e-6
    for b in range(c.B):
        tok, _, kept, _ = T.trunc_ref(c.x(b), 0, 2.0, 0.0, 0.5, c.rnd[b])
        assert head not in kept and tok != head and 300 <= len(kept) <= 520
    assert sum(P.topk_ref(c.x(b), 0, 2.0, c.rnd[b])[0] == head for b in range(c.B)) >= 8    # without the cut: u < 0.3 draws the head
    c, plain = T.mixed_case()
    assert 0 < len(plain) < c.B and any(c.greedy(b) for b in plain) and any(not c.greedy(b) for b in plain)


def test_hf_warpers_agree():
    """an extra where transformers is installed: MinPLogitsWarper and TypicalLogitsWarper keep the sets of steps 3 and 4"""
    tr = pytest.importorskip("transformers")
    torch = pytest.importorskip("torch")
    rng = np.random.RandomState(9)
    x = (rng.randn(300) * 2.0).astype(np.float32)
    scores = torch.from_numpy(x)[None]
    kept = T.trunc_ref(x, 0, 2.0, 0.1, 0.0, 0.5)[2]
    out = tr.MinPLogitsWarper(min_p=0.1)(None, scores)[0].numpy()
    assert sorted(kept.tolist()) == np.flatnonzero(out > -np.inf).tolist()
    kept = T.trunc_ref(x, 0, 2.0, 0.0, 0.6, 0.5)[2]
    out = tr.TypicalLogitsWarper(mass=0.6)(None, scores)[0].numpy()
    assert sorted(kept.tolist()) == np.flatnonzero(out > -np.inf).tolist()
