"""pplhip_op_rope_kv_write_prologue (csrc/k_rope_prologue.hip): Qwen's bias and head norms in front of the rotation, in the RoPE + KV-write
pass.  Every case is a mixed step on a paged cache: three decode rows and prefill rows of 5 and 37 tokens."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.conftest import load_pplhip
from tests.test_gpu_ops import ck, dev, _drop_device_tensors  # noqa: F401
from tests.test_gpu_row_ops import CANARY16, KV_FORMATS, P, bits, canary_like, kv_case, kv_units, kv_view

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GEOMETRIES = [(4, 4, 128), (28, 4, 128), (7, 1, 64), (2, 2, 32)]   # (28, 4, 128): Qwen2.5-7B, 320 items -- two blocks per token
FORMS = ["bias", "norm", "both"]
STEP = dict(layout=1, mode=1, seqlens=[1, 1, 1, 5, 37], start_pos=[6, 0, 11, 0, 3], seed=5)   # layout 1: a layer is [slot][k / v][head][D]
EPS = 1e-6


class Inputs:
    """the step, its rows and the prologue's tensors.  Rows and bias are multiples of 2^-8 below 4: their fp32 sum is exact."""

    def __init__(self, m, fmt, H, Hkv, D):
        self.case = c = kv_case(m, fmt, H, Hkv, D, **STEP)
        rng = np.random.RandomState(H * D)
        self.N = N = (H + 2 * Hkv) * D
        grid = lambda *shape: (rng.randint(-1023, 1024, size=shape) / 256.0).astype(np.float16)
        self.y, self.bias = grid(c.T, N), grid(N)
        self.q_norm, self.k_norm = (0.5 + 1.5 * rng.rand(D)).astype(np.float16), (0.5 + 1.5 * rng.rand(D)).astype(np.float16)
        self.identity = np.concatenate([np.ones((len(c.rope), D // 2), np.float32), np.zeros((len(c.rope), D // 2), np.float32)], 1)

    def parts(self, form):
        return (self.bias if form in ("bias", "both") else None, *((self.q_norm, self.k_norm) if form in ("norm", "both") else (None, None)))


def reference(x, form, H, Hkv, D, dtype=np.float64, flip=False):
    """the specification's arithmetic on x.y in `dtype`, rounded to fp16 at its two points; flip: the squares summed in reverse order"""
    bias, qw, kw = x.parts(form)
    a = x.y.astype(dtype)
    if bias is not None:
        a = (a + bias.astype(dtype)).astype(np.float16).astype(dtype)
    if qw is not None:
        T, nh = len(a), H + Hkv
        heads = a[:, :nh * D].reshape(T, nh, D)
        sq = (heads * heads)[..., ::-1] if flip else heads * heads
        ss = np.zeros((T, nh), dtype)
        for i in range(D):
            ss = ss + sq[..., i]
        w = np.concatenate([np.tile(qw, (H, 1)), np.tile(kw, (Hkv, 1))]).astype(dtype)
        a[:, :nh * D] = (heads * (1 / np.sqrt(ss / dtype(D) + dtype(EPS)))[..., None] * w).reshape(T, -1)
    return a.astype(np.float16)


def run(m, fmt, x, rows, table, form=None, old=False, slab=None):
    """one launch on `rows` (host fp16 [T, N]) over a canary cache -> (q rows with a canary row on either side, cache, scale)"""
    c, L = x.case, m.lib()
    cdt, epu, eps_ = kv_units(fmt, c.D)
    dq = canary_like((c.T + 2, x.N), torch.float16)
    dq[1:-1] = dev(rows)
    dcache = canary_like((c.cache.size // epu,), cdt)
    dscale = canary_like((c.cache.size // eps_,), torch.float16) if eps_ else None
    v = kv_view(fmt, c, dcache, dscale)
    ws, splits, M = slab if slab is not None else (None, 0, 0)
    args = [None, dq[1:].data_ptr(), P(dev(table)), C.byref(v), P(dev(c.seq_starts)), P(dev(c.start_pos)), P(dev(c.cache_idx)), c.max_pages,
            c.B, 0, c.T, c.H, P(ws), splits, None, M]
    if old:
        ck(L.pplhip_op_rope_kv_write_ex(*args))
    else:
        ck(L.pplhip_op_rope_kv_write_prologue(*args, *[P(dev(t)) if t is not None else None for t in x.parts(form)], EPS))
    return bits(dq), bits(dcache), (bits(dscale) if eps_ else None)


def token_slots(c):
    """cache slot of every token row of the paged step"""
    b = np.searchsorted(c.seq_starts, np.arange(c.T), side="right") - 1
    pos = c.start_pos[b] + np.arange(c.T) - c.seq_starts[b]
    ps = c.desc.page_size
    return c.cache_idx[b, pos // ps] * ps + pos % ps


@functools.lru_cache(maxsize=None)
def prologue_rows(H, Hkv, D, form):
    """what the prologue makes of the rows, from the device: the new operator under an identity rotation over an fp16 cache leaves n_q in
    place and n_k, v + bias in the cache -> (inputs, rows fp16 [T, N], q image, cache image, slots)"""
    m = load_pplhip()
    x = Inputs(m, "fp16", H, Hkv, D)
    q, cache, _ = run(m, "fp16", x, x.y, x.identity, form)
    slots = token_slots(x.case)
    layer = cache.reshape(x.case.L, x.case.N, 2 * Hkv * D)[x.case.layer]
    rows = np.concatenate([q[1:-1, :H * D], layer[slots]], 1).view(np.float16)
    return x, rows, q, cache, slots


def ordered(u16):
    """fp16 bits -> integers in value order (+-0 both 0): their difference counts ulps"""
    s = (u16 & 0x7fff).astype(np.int32)
    return np.where(u16 & 0x8000, -s, s)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("H,Hkv,D", GEOMETRIES)
def test_prologue_arithmetic(H, Hkv, D, form):
    """Against the float64 restatement of DESIGN.md's rule.  Bias only: bit for bit (the fp32 sum of the two fp16 numbers is exact).  With the
    norm: every element within one fp16 ulp, at most 5 % of them different at all -- a cap, not a measurement: a float32 numpy restatement
    that sums the squares in the reverse order differs from the float64 one in at most 0.06 % of these inputs' elements (checked on the
    CPU for all four geometries, both norm forms), always by one ulp.  Nothing but the q columns and the rows' cache slots is written."""
    x, rows, q, cache, slots = prologue_rows(H, Hkv, D, form)
    want = reference(x, form, H, Hkv, D)
    d = np.abs(ordered(rows.view(np.uint16)) - ordered(want.view(np.uint16)))
    share = float((d != 0).mean())
    print(f"rope prologue {form} ({H}, {Hkv}, {D}): {share:.5%} of the elements differ from float64, worst {d.max()} ulp")
    assert d.max() <= (0 if form == "bias" else 1) and share <= 0.05
    assert (q[0] == CANARY16).all() and (q[-1] == CANARY16).all() and (q[1:-1, H * D:] == x.y.view(np.uint16)[:, H * D:]).all()
    layer = cache.reshape(x.case.L, x.case.N, -1)
    unused = np.ones(x.case.N, bool)
    unused[slots] = False
    assert (layer[x.case.layer][unused] == CANARY16).all() and (np.delete(layer, x.case.layer, 0) == CANARY16).all()


@pytest.mark.parametrize("fmt", KV_FORMATS)
@pytest.mark.parametrize("H,Hkv,D", GEOMETRIES)
def test_rotation_and_cache_write_behind_the_prologue(H, Hkv, D, fmt):
    """bit for bit: the existing operator on the prologue's rows = the new operator on the original rows, real table, in the q rows (canary
    rows around them) and the whole cache and scale image (canaries in every unused slot)"""
    m = load_pplhip()
    _, rows, _, _, _ = prologue_rows(H, Hkv, D, "both")
    x = Inputs(m, fmt, H, Hkv, D)
    q0, c0, s0 = run(m, fmt, x, rows, x.case.rope, old=True)
    q1, c1, s1 = run(m, fmt, x, x.y, x.case.rope, "both")
    assert (q1[:, :H * D] == q0[:, :H * D]).all() and (q1[1:-1, H * D:] == x.y.view(np.uint16)[:, H * D:]).all() and (q1[0] == CANARY16).all()
    assert (c1 == c0).all() and (s0 is None or (s1 == s0).all())
    can = c0 == (CANARY16 if fmt == "fp16" else 0x5A)
    assert 0.05 < can.mean() < 1.0   # unused slots kept their canary, the rows' slots were written


@pytest.mark.parametrize("fmt", ["fp16", "i8"])
def test_rows_from_slabs(fmt):
    """three slabs of multiples of 2^-8 whose sum is the fp16 row exactly: the same bits as from the fp16 source"""
    m = load_pplhip()
    H, Hkv, D = 28, 4, 128
    x = Inputs(m, fmt, H, Hkv, D)
    rng = np.random.RandomState(1)
    total = np.rint(x.y.astype(np.float64) * 256).astype(np.int64)
    s0, s1 = rng.randint(-700, 700, size=total.shape), rng.randint(-700, 700, size=total.shape)
    ws = (np.stack([s0, s1, total - s0 - s1]) / 256.0).astype(np.float32)
    want = run(m, fmt, x, x.y, x.case.rope, "both")
    got = run(m, fmt, x, np.zeros_like(x.y), x.case.rope, "both", slab=(dev(ws), 3, x.case.T))
    assert (got[0][:, :H * D] == want[0][:, :H * D]).all() and (got[0][1:-1, H * D:] == 0).all()
    assert (got[1] == want[1]).all() and (want[2] is None or (got[2] == want[2]).all())


@pytest.mark.parametrize("fmt", KV_FORMATS)
def test_no_prologue_is_the_existing_operator(fmt):
    m = load_pplhip()
    x = Inputs(m, fmt, 7, 1, 64)
    want, got = run(m, fmt, x, x.y, x.case.rope, old=True), run(m, fmt, x, x.y, x.case.rope, form=None)
    assert all(w is None or (g == w).all() for g, w in zip(got, want))
