"""The logit rules reference itself (tests/logit_rules.py), without a GPU: the edit on hand-computed rows, the validator on every refusal and
on the boundary cases that must pass, and seven deliberate mistakes, each of which the GPU case list must be able to tell from the truth."""
import numpy as np
import pytest

from tests import logit_rules as R

INF = float("inf")
CASES = R.all_cases()


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


def test_pack_mask():
    m = R.pack_mask([0, 31, 32, 40], 41)
    assert m.tolist() == [0x80000001, 0x00000101]
    assert R.pack_mask([0], 33, tail_bits=0xFFFFFFFF).tolist() == [1, 0xFFFFFFFE]
    assert R.pack_mask([], 64, tail_bits=0xFFFFFFFF).tolist() == [0, 0]        # V a multiple of 32: no tail bits


def test_hand_computed_rows():
    x = np.array([1.0, -2.0, 0.5, 3.0, -0.0, 7.0], dtype=np.float32)
    rule = R.Rule(bias=[(0, 0.25), (1, -INF), (3, 1.0), (4, 0.0)], mask=R.pack_mask([0, 1, 2, 4, 5], 6, tail_bits=0xFFFFFFFF), stops=[5, 2])
    assert bits(R.ref_edit(x, rule, 0)) == bits(x)
    # bit 0: token 3 is masked (its bias does not resurrect it), token 1 banned, -0 + 0 = +0, the stops stay
    assert bits(R.ref_edit(x, rule, 1)) == bits([1.25, -INF, 0.5, -INF, 0.0, 7.0])
    # bit 1 alone: only the stops
    assert bits(R.ref_edit(x, rule, 2)) == bits([1.0, -2.0, -INF, 3.0, -0.0, -INF])
    assert bits(R.ref_edit(x, rule, 3)) == bits([1.25, -INF, -INF, -INF, 0.0, -INF])
    # no mask: every token allowed
    assert bits(R.ref_edit(x, R.Rule(bias=[(3, 1.0)]), 1)) == bits([1.0, -2.0, 0.5, 4.0, -0.0, 7.0])
    # one float32 addition: 2^24 + 1 rounds to even
    assert R.ref_edit(np.array([16777216.0], dtype=np.float32), R.Rule(bias=[(0, 1.0)]), 1)[0] == np.float32(16777216.0)
    # a logit that is -inf already stays -inf under a finite bias
    assert bits(R.ref_edit(np.array([-INF], dtype=np.float32), R.Rule(bias=[(0, 5.0)]), 1)) == bits([-INF])


def test_validator_refusals():
    V = 100
    assert R.validate(V, logit_bias=[(100, 1.0)]) == "logit_bias"
    assert R.validate(V, logit_bias=[(-1, 1.0)]) == "logit_bias"
    assert R.validate(V, allowed=[5, 100]) == "allowed_tokens"
    assert R.validate(V, banned=[-1]) == "banned_tokens"
    assert R.validate(V, stops=[100], min_new_tokens=1) == "stop_tokens"
    assert R.validate(V, logit_bias=[(1, float("nan"))]) == "logit_bias"
    assert R.validate(V, logit_bias=[(1, INF)]) == "logit_bias"
    assert R.validate(V, logit_bias=[(1, 1.0), (2, 0.5), (1, 1.0)]) == "logit_bias"
    assert R.validate(1000, logit_bias=[(t, 1.0) for t in range(513)]) == "logit_bias"
    assert R.validate(1000, logit_bias=[(t, 1.0) for t in range(512)], banned=[999]) == "logit_bias"     # 513 merged entries
    assert R.validate(1000, stops=range(65), min_new_tokens=2) == "stop_tokens"
    # rules that leave nothing alive on the first step
    assert R.validate(V, allowed=[]) == "allowed_tokens"
    assert R.validate(V, allowed=[3, 4], banned=[3], logit_bias=[(4, -INF)]) == "allowed_tokens"
    assert R.validate(V, allowed=[3], stops=[3], min_new_tokens=1) == "allowed_tokens"
    assert R.validate(4, banned=[0, 1, 2, 3]) == "banned_tokens"
    assert R.validate(2, stops=[0, 1], min_new_tokens=1) == "min_new_tokens"


def test_validator_boundaries_that_pass():
    V = 1000
    assert R.validate(V) is None
    assert R.validate(V, allowed=[3, 4], banned=[3]) is None                               # exactly one live token
    assert R.validate(V, allowed=[3], stops=[3], min_new_tokens=0) is None                  # the stops are not suppressed
    assert R.validate(4, banned=[0, 1, 2]) is None
    assert R.validate(V, logit_bias=[(t, -1.0) for t in range(512)]) is None
    assert R.validate(V, logit_bias=[(t, -1.0) for t in range(500)], banned=range(488, 512)) is None   # 512 merged entries
    assert R.validate(V, stops=range(64), min_new_tokens=1) is None
    assert R.validate(V, stops=range(900), min_new_tokens=0) is None                        # not suppressed: not counted
    assert R.validate(V, logit_bias=[(1, -INF), (1, -INF), (1, 2.0)], banned=[1]) is None   # bans merge; the ban wins
    assert R.validate(V, logit_bias=[(0, 3.4e38), (V - 1, -3.4e38)]) is None


def test_merge():
    r = R.merge(100, logit_bias=[(1, 2.0), (7, -INF), (9, 1.0)], allowed=[1, 2, 9], banned=[9], stops=[5, 2, 5], min_new_tokens=1)
    assert sorted(r.bias) == [(1, 2.0), (7, -INF), (9, -INF)]
    assert r.mask.tolist() == R.pack_mask([1, 2, 9], 100).tolist() and r.stops == [2, 5]
    assert R.merge(100, stops=[5], min_new_tokens=0).stops == []


def test_case_list_covers_what_the_issue_names():
    vs = {c.V for c in CASES}
    assert set(R.GRID_V) | {32000} <= vs
    assert max(c.B for c in CASES if c.V < 32000) == 6 and any(c.B == 64 and c.V == 32000 and len(c.asking) == 64 for c in CASES)
    for V in R.GRID_V:
        mine = [c for c in CASES if c.V == V and not c.name.startswith("hazard")]
        assert {c.stride for c in mine} == set(R.strides(V)) and {c.off for c in mine} == {0, 1, 2, 3}
        assert any(c.uses_vector_path() for c in mine) and any(not c.uses_vector_path() for c in mine)
    assert all((c.slots != np.arange(c.B)).any() for c in CASES)
    assert {int(f) for c in CASES for f in c.flags} == {0, 1, 2, 3}
    assert any({0, 1, 2, 3} <= {int(f) for f in c.flags} for c in CASES)
    kinds, nb, sizes = set(), set(), set()
    for c in CASES:
        for b in c.asking:
            r = c.rules[int(c.slots[b])]
            kinds.add((r.mask is not None, bool(r.bias), bool(r.stops)))
            nb.add(len(r.bias))
            if r.mask is not None:
                n = int(np.unpackbits(r.mask.view(np.uint8), bitorder="little")[:c.V].sum())
                sizes.add("1" if n == 1 else "V-1" if n == c.V - 1 and c.V > 2 else "V" if n == c.V else "")
    assert {(True, False, False), (False, True, False), (False, False, True), (True, True, True)} <= kinds
    assert set(R.N_BIAS) <= nb and {"1", "V-1", "V"} <= sizes
    assert len([c for c in CASES if c.name.startswith("hazard")]) == 16     # 24 permutations x 2 places x 2 paths, six rows a case


def test_image_reference_agrees_with_the_row_reference():
    """want_image (the table-driven form the mutants are made from) and ref_edit (the rule-driven form) are written separately"""
    for c in CASES:
        if c.B > 6:
            continue
        img, want = c.image(), c.want_image()
        for b in range(c.B):
            lo = c.off + b * c.stride
            row = R.ref_edit(c.logits[b], c.rules.get(int(c.slots[b]), R.Rule()), int(c.flags[b]))
            assert R.same_bits(want[lo:lo + c.V], row), (c.name, b)
            img[lo:lo + c.V] = row
        assert R.same_bits(img, want), c.name                  # and nothing outside the rows moved
        assert not R.diff(c, want)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_some_case_tells_the_mutant_from_the_truth(mutant):
    small = [c for c in CASES if c.V <= 4099]
    caught = [c.name for c in small if not R.same_bits(R.edited_image(c, mutant), c.want_image())]
    print(f"{mutant}: {len(caught)} of {len(small)} cases")
    assert caught, mutant
    c = next(c for c in small if c.name == caught[0])
    assert R.diff(c, R.edited_image(c, mutant))
