"""CPU specification of the sharp attention inputs (tests/attn_sharp.py) that tests/test_gpu_attn_sharp.py runs on the device:
F1 cases are exact gathers (the oracle agrees bit for bit), the float64 reference agrees with the oracle on F2 cases, every F2 case
catches the named mutations at >= 4 x the bar the GPU test uses, and the F1 needles straddle at least one edge of every kind.
Formats: fp16, int8-g8, fp8 and int4-g32; the int4 cases also show that their queries reach the format's own corrections."""
import numpy as np
import pytest

from tests import attn_sharp as A

TEETH = 4.0


def _gather_equals_oracle(spec):
    c = A.make(spec)
    want, top = A.expect_gather(c)
    got = c.oracle().astype(np.float16)
    assert (got.view(np.uint16) == want.view(np.uint16)).all(), A.explain_mismatch(c, got, want, top)


@pytest.mark.parametrize("spec", A.f1_decode_specs() + A.f1_prefill_specs(), ids=lambda s: s["name"])
def test_f1_oracle_equals_gather(spec):
    """the construction is sound: the fp32 oracle produces exactly the gathered V row for every (row, head)"""
    _gather_equals_oracle(spec)


def _f2(i):
    family, spec = A.F2_SPECS[i]
    return family, A.make(spec, family)


@pytest.mark.parametrize("i", range(len(A.F2_SPECS)), ids=lambda i: A.F2_SPECS[i][1]["name"])
def test_f2_ref64_matches_oracle(i):
    """the float64 reference is right: within half an fp16 ulp (the oracle rounds its output to fp16) + 0.05 x the GPU bar"""
    _, c = _f2(i)
    want = A.ref64(c)
    got = c.oracle()
    half_ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64) / 2
    err = np.abs(got - want) - half_ulp
    bar = A.bar_of(c, want)
    assert (err <= 0.05 * bar).all(), float((err / bar).max())


def test_f2_mutants_have_teeth(capsys):
    """every mutant a family applies to moves the output by >= 4 x the GPU bar somewhere (table: max |mutant - ref64| / bar).
    (Building a 'rising' case asserts its rise on the dequantised slab: A.check_rising.)"""
    rows, fails = [], []
    for family, spec in A.F2_SPECS:
        c = A.make(spec, family)
        t = A.teeth(c)
        rows.append((spec["name"], t))
        for mname, v in t.items():
            if mname in A.APPLIES[family] and v is not None and not v >= TEETH:
                fails.append(f"{spec['name']} {mname}: {v:.2f}")
            if mname in A.APPLIES[family] and v is None and mname in ("scale*1.01", "drop_last", "future_key"):
                fails.append(f"{spec['name']} {mname}: not applied")
    w = max(len(r[0]) for r in rows)
    lines = [" " * w + " " + " ".join(f"{m:>13}" for m in A.MUTANTS)]
    for name, t in rows:
        fam = dict((s["name"], f) for f, s in A.F2_SPECS)[name]
        cells = []
        for m in A.MUTANTS:
            v = t[m]
            cells.append(f"{'n/a':>13}" if v is None else f"{v:>12.3g}" + (" " if m in A.APPLIES[fam] else "*"))
        lines.append(f"{name:<{w}} " + " ".join(cells))
    lines.append("(max |mutant - ref64| / bar;  *: the family is not built for this mutant, not asserted)")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not fails, fails


I4_F1_SPECS = [s for s in A.f1_decode_specs() + A.f1_prefill_specs() + [A.F1_CONFIG4_I4] if s["fmt"] == "i4"]


@pytest.mark.parametrize("spec", I4_F1_SPECS, ids=lambda s: s["name"])
def test_f1_i4_queries_reach_the_corrections(spec):
    """int4 folds the + 8 of a stored nibble out of the score as 8 * sum(q) per 32-channel group, and packs two channels per byte:
    some needle query sums to non-zero over a group (a Hadamard row d with d & 31 == 0; every other row sums to 0 over every group and
    would hide a wrong correction), and some has an odd direction index (q[2j + 1] = -q[2j]: swapped nibbles negate its score).
    Every K row of the case round-trips through the encoder exactly (asserted while the slab is written)."""
    c = A.make(spec)
    D = c.D
    Hd = A.hadamard(D)
    q = c.Q.reshape(-1, D).astype(np.float64)
    d = (q @ Hd.T).argmax(-1)
    assert (Hd[d] == q).all(), "a query is not a Hadamard row"
    gsum = q.reshape(-1, D // 32, 32).sum(-1)
    assert (gsum != 0).any(), "no query sums to non-zero over a 32-channel group"
    assert ((gsum != 0).any(-1) == (d & 31 == 0)).all()
    assert (d & 1 == 1).any(), "no query with an odd direction index"
    if not getattr(c, "streamed", False):
        for b in range(c.B):   # (redundant with the assertion in Case._put; kept where the property is stated)
            k = c.read(0, np.arange(c.Hkv)[:, None], c.slots(b, np.arange(c.kvlen[b]))[None, :])
            assert all(A._i4_exact(row) for row in k[np.abs(k).max(-1) > 0])


def test_f1_config4_i4_is_a_gather():
    """config 4's decode launch on the int4 cache (the grouped-query kernel): an exact gather the oracle reproduces bit for bit"""
    assert A.F1_CONFIG4_I4["fmt"] == "i4" and A.gqa_form("i4", A.F1_CONFIG4_I4["H"], A.F1_CONFIG4_I4["Hkv"], A.F1_CONFIG4_I4["D"])
    _gather_equals_oracle(A.F1_CONFIG4_I4)


def test_i4_kernel_forms():
    """the mirrors of the int4 dispatch and geometry: the grouped-query kernel at head_dim 128 only; a lane piece of the multi-head
    kernel is a 32-channel group, so 16 / 32 / 64 rows per wave-load at head_dim 128 / 64 / 32 (x 4 in flight, x 4 waves)"""
    assert A.gqa_form("i4", 8, 1, 128) and A.gqa_form("i4", 16, 2, 128)
    assert not A.gqa_form("i4", 12, 2, 64) and not A.gqa_form("i4", 16, 1, 64) and not A.gqa_form("i4", 8, 4, 128)
    assert [A.dec_key_step("i4", D) for D in (128, 64, 32)] == [(64, 256), (128, 512), (256, 1024)]
    assert [A.dec_key_step("i8", D) for D in (128, 64, 32)] == [(32, 128), (64, 256), (128, 512)]


def _pairs(pos, s):
    return any(k * s - 1 in pos and k * s in pos for k in range(1, max(pos) // s + 2))


@pytest.mark.parametrize("spec", A.f1_decode_specs() + A.f1_prefill_specs(), ids=lambda s: s["name"])
def test_f1_positions_cover_edges(spec):
    """the needles sit on key 0, the last key, both sides of at least one edge of every stride of the kernel forms the launch
    reaches (pages, key steps, 32-key pairs, 64- / 128-key tiles) and of the split chunks, and (decode) deep inside the long ranges"""
    c = A.make(spec)
    allpos = set().union(*c.needles_b)
    assert 0 in allpos
    for b in range(c.nb):
        n = int(c.kvlen[b])
        assert any(n - 1 in c.needles_b[bb] and int(c.kvlen[bb]) == n for bb in range(c.nb)), f"last key of kv {n}"
    for s in c.edge_strides():
        if c.max_kv_len > s:
            assert any(_pairs(c.needles_b[b], s) for b in range(c.B) if c.kvlen[b] > s), f"stride {s}"
    if c.split > 1 and c.nb:
        assert any(any(beg - 1 in c.needles_b[b] and beg in c.needles_b[b] for beg, _ in c.decode_chunks(b)[1:])
                   for b in range(c.nb) if len(c.decode_chunks(b)) > 1), "decode split edges"
    if c.p32_split > 1:
        assert any(any(beg - 1 in c.needles_b[b] and beg in c.needles_b[b] for beg, _ in A.p32_chunks(int(c.start_pos[b]),
                   int(c.seqlens[b]), 0, c.p32_split)[1:]) for b in range(c.nb, c.B)), "split-KV edges"
    for b in range(c.nb):   # deep: a needle inside [4096, n - 2] of every long decode request length (not the current token)
        n = int(c.kvlen[b])
        if n > 4097:
            assert any(any(4096 <= p <= n - 2 for p in c.needles_b[bb]) for bb in range(c.nb) if int(c.kvlen[bb]) == n), f"deep, kv {n}"
