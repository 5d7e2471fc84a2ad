"""The row kernels between the GEMMs, one operator at a time (cases and references: tests/row_ops.py):
  1. (Skip)RMSNorm in every kernel form and epilogue: needle and edge rows against the float64 reference within the derived interval,
     the residual and the quantising epilogues bit for bit;
  2. the last-token gather of the norm and launch_gather_last_rows, bit for bit;
  3. unreduced split-K slabs as the norm's skip operand: synthetic slabs whose sum depends on its order, NaN behind the live slabs;
  4. the same slabs as the source of RoPE + KV write, in all four cache formats, on a chunk [t0, t0 + T) of the step; the write alone at
     70 and 300 requests and on the quantisation edge rows against the host references;
  5. the real split-K producer (launch_linear with `defer`) into both consumers against the producer reducing itself.
Every comparison is bit for bit except the norm's output against float64 (the interval of tests/row_ops.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref
from tests import f8f8 as F8
from tests import kv_fp8, kv_i4
from tests import row_ops as R
from tests.conftest import ROOT, load_pplhip
from tests.test_gpu_kv_fp8 import Fp8Case
from tests.test_gpu_kv_i4 import I4Case
from tests.test_gpu_ops import KvCase, ck, dev, _drop_device_tensors  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CANARY16 = 0x7D5A      # a NaN payload no kernel produces
CANARY8 = 0x5A


def P(t):
    return None if t is None else t.data_ptr()


def bits(t):
    """device / host fp16 -> uint16 numpy"""
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def canary_like(shape, dtype):
    if dtype == torch.float16:
        return torch.full(shape, CANARY16, dtype=torch.int16, device="cuda").view(torch.float16)
    if dtype == torch.float32:
        return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    return torch.full(shape, CANARY8, dtype=torch.int8, device="cuda").view(dtype)


def norm_ex(L, x, skip, w, rows, hidden, out=None, res=None, q=None, sx=None, f8=0, gather=None, slab=None):
    ws, splits, scale, M = slab if slab is not None else (None, 0, None, 0)
    ck(L.pplhip_op_rmsnorm_ex(None, P(x), P(skip), P(w), R.EPS, rows, hidden, P(gather), P(out), P(res), P(q), P(sx), f8, P(ws), splits,
                              P(scale), M))


def host_quant_i8(y16):
    y = np.ascontiguousarray(y16.astype(np.float32))
    q, sx = np.empty(y.shape, np.int8), np.empty(len(y), np.float32)
    ref.lib().ref_quant_act_rows(y.ctypes.data, len(y), y.shape[1], q.ctypes.data, sx.ctypes.data)
    return q, sx


def host_quant_f8(y16):
    q, e = F8.quantize_rows(y16)
    return q, np.ldexp(np.float32(1.0), e).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# 1. every form, every epilogue
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("rows,hidden", R.ALL_FORM_CASES)
def test_norm_forms(rows, hidden, skip):
    m = load_pplhip()
    L = m.lib()
    form = R.expected_form(rows, hidden)
    for quant in (0, 1, 2):
        assert m.rmsnorm_form(rows, hidden, quant) == (0, R.form_text(form, quant))
    case = R.norm_case(rows, hidden, skip)
    dw = dev(case.w)
    n = case.R
    got, gres = np.empty((n, hidden), np.float16), np.empty((n, hidden), np.float16)
    q8, s8 = np.empty((n, hidden), np.int8), np.empty(n, np.float32)
    qf, sf = np.empty((n, hidden), np.uint8), np.empty(n, np.float32)
    for l in range(case.launches):
        sl = slice(l * rows, (l + 1) * rows)
        dx = torch.from_numpy(case.x[sl]).cuda()
        dsk = torch.from_numpy(case.skip[sl]).cuda() if skip else None
        out, res = canary_like((rows, hidden), torch.float16), canary_like((rows, hidden), torch.float16)
        ck(L.pplhip_op_rmsnorm(None, P(dx), P(dsk), P(dw), R.EPS, rows, hidden, P(out), P(res)))
        got[sl], gres[sl] = out.cpu().numpy(), res.cpu().numpy()
        for f8, qh, sh in ((0, q8, s8), (1, qf, sf)):
            dq, dsx = canary_like((rows, hidden), torch.int8), canary_like((rows,), torch.float32)
            res2 = canary_like((rows, hidden), torch.float16)
            fn = L.pplhip_op_rmsnorm_quant_f8 if f8 else L.pplhip_op_rmsnorm_quant
            ck(fn(None, P(dx), P(dsk), P(dw), R.EPS, rows, hidden, P(res2), P(dq), P(dsx)))
            assert torch.equal(res2.view(torch.int16), res.view(torch.int16)), "residual of the quantising epilogue"
            qh[sl], sh[sl] = dq.cpu().numpy().view(qh.dtype), dsx.cpu().numpy()
        del dx, dsk, out, res
    live, pad = case.live, np.flatnonzero(case.kind == "pad")
    # residual_out = RN16(x + skip), every row, bit for bit
    assert (gres.view(np.uint16) == case.residual().view(np.uint16)).all()
    # the output: inside the interval of the float64 reference on every row that holds something, zero on the pad rows
    bad, worst = R.check_norm_rows(case, live, got[live])
    print(f"{form} rows={rows} hidden={hidden} skip={skip}: needed delta {worst:.4f} DELTA")
    assert not bad.any(), (int(bad.sum()), live[bad][:8], case.kind[live][bad][:8], worst)
    assert (got[pad].view(np.uint16) << 1 == 0).all()
    zero = live[case.kind[live] == "zero"]
    assert (got[zero].view(np.uint16) << 1 == 0).all()
    # the quantising epilogues: the host quantisers on the device's own fp16 output, all rows, bit for bit
    wq, wsx = host_quant_i8(got[live])
    assert (q8[live] == wq).all() and (s8[live] == wsx).all()
    wq, wsx = host_quant_f8(got[live])
    assert (qf[live] == wq).all() and (sf[live] == wsx).all()
    if len(pad):
        z = np.zeros((1, hidden), np.float16)
        (zq8, zs8), (zqf, zsf) = host_quant_i8(z), host_quant_f8(z)
        assert (q8[pad] == zq8).all() and (s8[pad] == zs8[0]).all() and (qf[pad] == zqf).all() and (sf[pad] == zsf[0]).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. the last-token gather
# ---------------------------------------------------------------------------------------------------------------
def _ragged(B):
    if B == 5:
        lens = [1, 1, 7, 1, 130]
    else:
        rng = np.random.default_rng(B)
        lens = [1] * (B // 2) + [int(v) for v in rng.integers(1, 12, size=B - B // 2)]   # decode rows, then ragged prefills
        lens[B // 2 + 1] = 1
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _rows_data(T, hidden, seed):
    """needle-like rows: background +-2^-4, a needle chunk per row"""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-1, 1, size=(T, hidden)) * 2.0 ** -4).astype(np.float16)
    x.reshape(T, hidden // 8, 8)[np.arange(T), rng.integers(0, hidden // 8, size=T)] = R.NEEDLE
    return x


@pytest.mark.parametrize("B,hidden", [(5, 4096), (5, 8192), (5, 16384), (70, 136), (70, 2056), (70, 4104), (70, 4096), (70, 5120)])
@pytest.mark.parametrize("skip", [False, True])
def test_norm_gather_equals_plain_rows(B, hidden, skip):
    m = load_pplhip()
    L = m.lib()
    ss = _ragged(B)
    T = int(ss[-1])
    last = ss[1:] - 1
    x = _rows_data(T, hidden, B + hidden)
    sk = (_rows_data(T, hidden, B + hidden + 1).astype(np.float32) * 0.25).astype(np.float16) if skip else None
    w = R.norm_weights(hidden)
    dx, dw, dss = dev(x), dev(w), dev(ss)
    dsk = dev(sk) if skip else None
    # the plain operator on the gathered rows: the same launch shape (B rows), hence the same form and the same bits
    gx, gsk = dev(x[last]), (dev(sk[last]) if skip else None)
    out0, res0 = canary_like((B, hidden), torch.float16), canary_like((B, hidden), torch.float16)
    ck(L.pplhip_op_rmsnorm(None, P(gx), P(gsk), P(dw), R.EPS, B, hidden, P(out0), P(res0)))
    out1, res1 = canary_like((B, hidden), torch.float16), canary_like((B, hidden), torch.float16)
    norm_ex(L, dx, dsk, dw, B, hidden, out=out1, res=res1, gather=dss)
    assert torch.equal(out1.view(torch.int16), out0.view(torch.int16)) and torch.equal(res1.view(torch.int16), res0.view(torch.int16))
    assert not (bits(out1) == CANARY16).any()
    for f8, fn in ((0, L.pplhip_op_rmsnorm_quant), (1, L.pplhip_op_rmsnorm_quant_f8)):
        q0, s0 = canary_like((B, hidden), torch.int8), canary_like((B,), torch.float32)
        q1, s1 = canary_like((B, hidden), torch.int8), canary_like((B,), torch.float32)
        ck(fn(None, P(gx), P(gsk), P(dw), R.EPS, B, hidden, None, P(q0), P(s0)))
        norm_ex(L, dx, dsk, dw, B, hidden, q=q1, sx=s1, f8=f8, gather=dss)
        assert torch.equal(q0, q1) and torch.equal(s0, s1) and not torch.isnan(s1).any()


@pytest.mark.parametrize("hidden", [8, 2056, 8192])
@pytest.mark.parametrize("B", [5, 70])
def test_gather_last_rows_bit_exact(hidden, B):
    L = load_pplhip().lib()
    ss = _ragged(B)
    T = int(ss[-1])
    x = _rows_data(T, hidden, hidden + B)
    out = canary_like((B + 1, hidden), torch.float16)
    ck(L.pplhip_op_gather_last_rows(None, P(dev(x)), P(dev(ss)), B, hidden, P(out)))
    got = bits(out)
    assert (got[:B] == x[ss[1:] - 1].view(np.uint16)).all() and (got[B] == CANARY16).all()
    assert L.pplhip_op_gather_last_rows(None, P(dev(x)), P(dev(ss)), B, hidden + 4, P(out)) == -2


# ---------------------------------------------------------------------------------------------------------------
# 3. slabs into the norm
# ---------------------------------------------------------------------------------------------------------------
SLAB_NORM_SHAPES = [(37, 136, "rmsnorm_kernel<1,256>"), (37, 3072, "rmsnorm_kernel<2,256>"), (37, 4096, "rmsnorm_kernel<1,512>"),
                    (37, 8192, "rmsnorm_kernel<1,1024>")]


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("rows,hidden,form", SLAB_NORM_SHAPES)
def test_slabs_into_norm(rows, hidden, form, gather):
    m = load_pplhip()
    L = m.lib()
    assert m.rmsnorm_form(rows, hidden, 0) == (0, form)
    if gather:   # `rows` requests: the slabs and x hold every token row, the norm reads each request's last
        rng = np.random.default_rng(rows)
        lens = [1] * 10 + [int(v) for v in rng.integers(1, 6, size=rows - 10)]
        ss = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        M, src, dss = int(ss[-1]), ss[1:] - 1, dev(ss)
    else:
        M, src, dss = rows, np.arange(rows), None
    x = _rows_data(M, hidden, hidden + gather)
    w = R.norm_weights(hidden)
    dx, dw = dev(x), dev(w)
    for splits in range(1, R.MAX_SLABS + 1):
        for with_scale in (False, True):
            ws, scale = R.build_slabs(M, hidden, splits, with_scale)
            red = R.slab_reduce(ws, splits, scale)                     # the skip operand, reduced on the host
            dws, dscale, dred = dev(ws), (dev(scale) if with_scale else None), dev(red)
            slab = (dws, splits, dscale, M)
            tag = (splits, with_scale)
            out0, res0 = canary_like((rows, hidden), torch.float16), canary_like((rows, hidden), torch.float16)
            out1, res1 = canary_like((rows, hidden), torch.float16), canary_like((rows, hidden), torch.float16)
            norm_ex(L, dx, dred, dw, rows, hidden, out=out0, res=res0, gather=dss)
            norm_ex(L, dx, None, dw, rows, hidden, out=out1, res=res1, gather=dss, slab=slab)
            want_res = R.rn16(x[src].astype(np.float64) + red[src].astype(np.float64))
            assert (bits(res1) == want_res.view(np.uint16)).all(), tag
            assert torch.equal(res1.view(torch.int16), res0.view(torch.int16)) and torch.equal(out1.view(torch.int16), out0.view(torch.int16)), tag
            assert not np.isnan(out1.float().cpu().numpy()).any(), tag      # the NaN slabs behind `splits` touched nothing
            for f8 in (0, 1):
                q0, s0 = canary_like((rows, hidden), torch.int8), canary_like((rows,), torch.float32)
                q1, s1 = canary_like((rows, hidden), torch.int8), canary_like((rows,), torch.float32)
                norm_ex(L, dx, dred, dw, rows, hidden, q=q0, sx=s0, f8=f8, gather=dss)
                norm_ex(L, dx, None, dw, rows, hidden, q=q1, sx=s1, f8=f8, gather=dss, slab=slab)
                assert torch.equal(q0, q1) and torch.equal(s0, s1) and not torch.isnan(s1).any(), (tag, f8)
            torch.cuda.synchronize()
    # refusals, decided before any device call
    bad = L.pplhip_op_rmsnorm_ex
    assert bad(None, P(dx), None, P(dw), R.EPS, rows, hidden, None, P(out1), None, None, None, 0, P(dws), 9, None, M) == -2
    assert bad(None, P(dx), None, P(dw), R.EPS, rows, hidden, None, P(out1), None, None, None, 0, None, 2, None, M) == -2
    assert bad(None, P(dx), None, P(dw), R.EPS, rows, hidden, None, P(out1), None, None, None, 0, P(dws), 2, None, rows - 1 if not gather else 0) == -2


# ---------------------------------------------------------------------------------------------------------------
# 4. RoPE + KV write: the four cache formats
# ---------------------------------------------------------------------------------------------------------------
KV_FORMATS = ("fp16", "i8", "fp8", "i4")
LAYOUT_MODES = [(0, 0), (1, 1), (2, 0), (3, 1), (3, 0)]


def kv_case(m, fmt, H, Hkv, D, layout, mode, seqlens, start_pos, seed):
    kw = dict(L=3, layer=1, layout=layout, mode=mode, seqlens=seqlens, start_pos=start_pos, seed=seed)
    if fmt == "fp8":
        return Fp8Case(m, H, Hkv, D, **kw)
    if fmt == "i4":
        return I4Case(m, H, Hkv, D, **kw)
    return KvCase(m, H, Hkv, D, quant=8 if fmt == "i8" else 0, **kw)


def kv_units(fmt, D):
    """(cache dtype, fp16 elements per cache unit, fp16 elements per scale or 0)"""
    return {"fp16": (torch.float16, 1, 0), "i8": (torch.int8, 1, 8), "fp8": (torch.int8, 1, D), "i4": (torch.int8, 2, 32)}[fmt]


def kv_view(fmt, case, dcache, dscale):
    return case.view8(dcache, dscale) if fmt == "fp8" else (case.view4(dcache, dscale) if fmt == "i4" else case.view(dcache, dscale))


def kv_owner(m, case, H, Hkv, D, layout, mode, seqlens, start_pos, seed):
    """token row + 1 that writes each fp16 element of the slab (0: none), from the oracle's own addressing: an fp16 write of rows whose
    k and v hold the row number under an identity rotation"""
    oc = KvCase(m, H, Hkv, D, L=3, layer=1, quant=0, layout=layout, mode=mode, seqlens=seqlens, start_pos=start_pos, seed=seed)
    assert (oc.cache_idx == case.cache_idx).all() and oc.N == case.N
    oc.qkv[:] = (np.arange(oc.T, dtype=np.float32) + 1)[:, None].astype(np.float16)
    oc.rope[:, :D // 2], oc.rope[:, D // 2:] = 1.0, 0.0
    oc.ref_write()
    return oc.cache.astype(np.float32).astype(np.int64)


def rope_ex(L, fmt, case, dq, dcache, dscale, t0, T, slab=None):
    v = kv_view(fmt, case, dcache, dscale)
    ws, splits, scale, M = slab if slab is not None else (None, 0, None, 0)
    ck(L.pplhip_op_rope_kv_write_ex(None, P(dq), P(dev(case.rope)), C.byref(v), P(dev(case.seq_starts)), P(dev(case.start_pos)),
                                    P(dev(case.cache_idx)), case.max_pages, case.B, t0, T, case.H, P(ws), splits, P(scale), M))


def check_chunk_from_slabs(m, fmt, H, Hkv, D, layout, mode, seqlens, start_pos, t0, Tc, slab_of, seed=0):
    """rows [t0, t0 + Tc) written from slabs (slab_of(Tc, N) -> (device slab description, host-reduced fp16 [Tc, N])) against
    pplhip_op_rope_kv_write of the whole step on a qkv that holds the reduced rows: rotated q, cache bytes and scales of the chunk's
    rows equal, everything else -- cache slots of other rows, qkv outside the chunk and its k / v columns inside -- keeps its canary"""
    L = m.lib()
    case = kv_case(m, fmt, H, Hkv, D, layout, mode, seqlens, start_pos, seed)
    N = (H + 2 * Hkv) * D
    slab, red = slab_of(Tc, N)
    assert t0 > 0 and t0 + Tc < case.T and case.seq_starts[-2] < t0 + Tc     # the chunk starts late and ends inside the last request
    cdt, epu, eps_ = kv_units(fmt, D)
    elems = case.cache.size
    # reference: the whole step through the plain entry
    qkv = case.qkv.copy()
    qkv[t0:t0 + Tc] = red
    dq0 = dev(qkv)
    c0 = canary_like((elems // epu,), cdt)
    s0 = canary_like((elems // eps_,), torch.float16) if eps_ else None
    v = kv_view(fmt, case, c0, s0)
    ck(L.pplhip_op_rope_kv_write(None, P(dq0), P(dev(case.rope)), C.byref(v), P(dev(case.seq_starts)), P(dev(case.start_pos)),
                                 P(dev(case.cache_idx)), case.max_pages, case.B, case.T, H))
    # the chunk from slabs
    dq1 = canary_like((case.T, N), torch.float16)
    c1 = canary_like((elems // epu,), cdt)
    s1 = canary_like((elems // eps_,), torch.float16) if eps_ else None
    rope_ex(L, fmt, case, dq1, c1, s1, t0, Tc, slab=slab)
    owner = kv_owner(m, case, H, Hkv, D, layout, mode, seqlens, start_pos, seed)
    mine = (owner > t0) & (owner <= t0 + Tc)
    assert mine.sum() == Tc * 2 * Hkv * D and ((owner > 0).sum() == case.T * 2 * Hkv * D)
    g0, g1 = bits(c0).reshape(-1), bits(c1).reshape(-1)
    can = np.array([CANARY16], np.uint16)[0] if fmt == "fp16" else np.array([CANARY8], np.int8)[0]
    mc = mine.reshape(-1, epu)[:, 0]
    assert (g1[mc] == g0[mc]).all() and (g1[~mc] == can).all() and not (g0[mc] == can).all()
    if eps_:
        ms = mine.reshape(-1, eps_)[:, 0]
        h0, h1 = bits(s0), bits(s1)
        assert (h1[ms] == h0[ms]).all() and (h1[~ms] == CANARY16).all() and (h0[ms] != CANARY16).all()
    q0, q1 = bits(dq0), bits(dq1)
    assert (q1[t0:t0 + Tc, :H * D] == q0[t0:t0 + Tc, :H * D]).all()
    q1[t0:t0 + Tc, :H * D] = CANARY16
    assert (q1 == CANARY16).all()


def synthetic_slabs(splits, with_scale):
    def make(Tc, N):
        ws, scale = R.build_slabs(Tc, N, splits, with_scale, seed=1)
        dws, dscale = dev(ws), (dev(scale) if with_scale else None)
        return (dws, splits, dscale, Tc), R.slab_reduce(ws, splits, scale)
    return make


SLAB_STEP = dict(seqlens=[1, 1, 1, 5, 9, 4], start_pos=[6, 0, 11, 0, 3, 2], t0=2, Tc=16)   # 3 decode rows, 3 prefills; rows [2, 18) of 21


@pytest.mark.parametrize("fmt", KV_FORMATS)
@pytest.mark.parametrize("layout,mode", LAYOUT_MODES)
@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 128), (8, 2, 64), (32, 8, 128)])      # the last: 2 blocks per token
def test_slabs_into_rope_kv_write(fmt, layout, mode, H, Hkv, D):
    m = load_pplhip()
    k = KV_FORMATS.index(fmt) * 5 + LAYOUT_MODES.index((layout, mode)) + D // 64
    splits, with_scale = 1 + k % R.MAX_SLABS, bool((k // R.MAX_SLABS + k) % 2)
    check_chunk_from_slabs(m, fmt, H, Hkv, D, layout, mode, slab_of=synthetic_slabs(splits, with_scale), seed=layout * 10 + mode, **SLAB_STEP)


def test_slabs_into_rope_kv_write_every_split_count():
    m = load_pplhip()
    for splits in range(1, R.MAX_SLABS + 1):
        for with_scale in (False, True):
            fmt = KV_FORMATS[(splits + with_scale) % 4]
            check_chunk_from_slabs(m, fmt, 4, 2, 128, 3, 1, slab_of=synthetic_slabs(splits, with_scale), seed=splits, **SLAB_STEP)


def test_slabs_into_rope_kv_write_three_blocks_per_token():
    """a block count that does not divide a token's work items (PPLHIP_ROPE_BLOCKS_PER_TOKEN=3; child process: the switch is read once)"""
    code = ("import tests.test_gpu_row_ops as t\n"
            "for fmt in t.KV_FORMATS:\n"
            "    t.test_slabs_into_rope_kv_write(fmt, 3, 1, 32, 8, 128)\n"
            "    t.test_slabs_into_rope_kv_write(fmt, 3, 0, 8, 2, 64)\n"
            "    t.test_write_many_requests_and_edge_rows(fmt, 70, 3, 1)\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PPLHIP_ROPE_BLOCKS_PER_TOKEN="3"), cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def many_requests(B):
    """decode rows (start_pos > 0), then ragged prefills, every third of them at position 0"""
    rng = np.random.default_rng(B)
    nd = B * 2 // 3
    lens = [1] * nd + [int(v) for v in rng.integers(1, 8, size=B - nd)]
    sp = [int(v) for v in rng.integers(1, 20, size=nd)] + [0 if i % 3 == 0 else int(rng.integers(1, 9)) for i in range(B - nd)]
    return lens, sp


@pytest.mark.parametrize("fmt", KV_FORMATS)
@pytest.mark.parametrize("B,layout,mode", [(70, 3, 1), (70, 0, 0), (300, 3, 0), (300, 1, 1)])
def test_write_many_requests_and_edge_rows(fmt, B, layout, mode):
    """the write alone at request counts where the request lookup is a binary search of several steps, with the quantisation edge
    rows of tests/row_ops.py in the k and v heads of tokens at position 0 and rotated magnitudes up to 60000 elsewhere, against
    ref_rope_kv_write and the fp8 / int4 host quantisers: bit for bit"""
    m = load_pplhip()
    L = m.lib()
    H, Hkv, D = 4, 2, 128
    lens, sp = many_requests(B)
    case = kv_case(m, fmt, H, Hkv, D, layout, mode, lens, sp, seed=B + layout)
    edge = R.kv_edge_head_rows(D)
    first = [int(case.seq_starts[b]) for b in range(case.B) if sp[b] == 0]
    assert len(first) >= len(edge)
    for i, t in enumerate(first):
        for h in range(2 * Hkv):                                  # k heads, then v heads
            case.qkv[t, (H + h) * D:(H + h + 1) * D] = edge[(i + h) % len(edge)]
    # a decode row at a position > 0 whose k heads hold +-60000 in the first half and 0 in the partner half: |rotated| <= 60000
    rng = np.random.default_rng(B)
    big = np.where(rng.integers(0, 2, size=D // 2) == 1, 60000.0, -60000.0) * rng.uniform(0.5, 1, size=D // 2)
    big[0] = 60000.0
    for h in range(Hkv):
        case.qkv[1, (H + h) * D:(H + h) * D + D // 2] = big.astype(np.float16)
        case.qkv[1, (H + h) * D + D // 2:(H + h + 1) * D] = 0
    assert sp[1] > 0
    cdt, epu, eps_ = kv_units(fmt, D)
    if fmt in ("fp16", "i8"):
        dcache = torch.zeros(case.cache.size, dtype=cdt, device="cuda")
        dscale = torch.zeros(case.cache.size // 8, dtype=torch.float16, device="cuda") if eps_ else None
    else:
        to = kv_fp8.slab_to_fp8 if fmt == "fp8" else kv_i4.slab_to_i4
        c8, s8 = to(case.cache, D)
        dcache, dscale = dev(c8), dev(s8)
    dq = dev(case.qkv)
    rope_ex(L, fmt, case, dq, dcache, dscale, 0, case.T)
    want_q = case.ref_write()
    assert np.isfinite(case.cache.astype(np.float32)).all() if fmt != "i8" else True
    assert (dq.cpu().numpy().astype(np.float32)[:, :H * D] == want_q[:, :H * D]).all()
    if fmt == "fp16":
        assert (bits(dcache) == case.cache.view(np.uint16)).all()
        assert np.abs(case.cache.astype(np.float32)).max() > 40000
    elif fmt == "i8":
        assert (bits(dscale) == case.scale.view(np.uint16)).all() and (dcache.cpu().numpy() == case.cache).all()
    else:
        wc, wsc = to(case.cache, D)
        assert (bits(dscale) == wsc.view(np.uint16)).all() and (dcache.cpu().numpy() == wc).all()


# ---------------------------------------------------------------------------------------------------------------
# 5. the real producer into the real consumers
# ---------------------------------------------------------------------------------------------------------------
def _weights(wq, group, N, K, rng):
    if wq == 0:
        return (rng.standard_normal((N, K)) * 0.05).astype(np.float16), None
    if wq == 8:
        return rng.integers(-127, 128, size=(N, K)).astype(np.int8), (0.0005 * (0.5 + rng.random(N))).astype(np.float16)
    return rng.integers(0, 256, size=(N, K // 2)).astype(np.uint8), (0.01 * (0.5 + rng.random((N, K // group)))).astype(np.float16)


@pytest.mark.parametrize("wq,group", R.DEFER_WQ)
@pytest.mark.parametrize("M,N,K", list(R.DEFER_SHAPES))
def test_deferred_linear_into_consumers(M, N, K, wq, group):
    m = load_pplhip()
    L = m.lib()
    rng = np.random.default_rng(M + N + K + wq)
    x = rng.standard_normal((M, K)).astype(np.float16)
    w, scale = _weights(wq, group, N, K, rng)
    dx, dw, ds = dev(x), dev(w), (dev(scale) if scale is not None else None)
    nws = R.DEFER_WS_BYTES // 4
    wsA = torch.full((nws,), float("nan"), dtype=torch.float32, device="cuda")
    wsB = torch.full((nws,), float("nan"), dtype=torch.float32, device="cuda")
    # producer A leaves its slabs, producer B reduces them itself: the same kernel, the same split count
    yA = canary_like((M, N), torch.float16)
    rc, routeA, splits, sc = m.linear_defer(P(dx), P(dw), P(ds), wq, group, M, N, K, P(yA), N, ws=P(wsA), ws_bytes=R.DEFER_WS_BYTES, dry_run=False)
    ck(rc)
    assert "reduce=deferred" in routeA and splits > 1 and splits == R.route_splits(routeA)[0] == R.DEFER_SHAPES[(M, N, K)][wq], routeA
    assert sc == (P(ds) if wq == 8 else None)
    assert (bits(yA) == CANARY16).all()                 # y was not written
    yB = canary_like((M, N), torch.float16)
    rc, routeB = m.linear_route(P(dx), P(dw), P(ds), wq, group, M, N, K, P(yB), N, 0, ws=P(wsB), ws_bytes=R.DEFER_WS_BYTES, dry_run=False)
    ck(rc)
    assert routeB == routeA.replace("reduce=deferred", "reduce=splitk_reduce_kernel<f16>")
    # the slabs themselves, reduced by the host reference, are the producer's own result
    slabs = wsA[:splits * M * N].cpu().numpy().reshape(splits, M, N)
    assert np.isfinite(slabs).all() and torch.isnan(wsA[splits * M * N:splits * M * N + 1024]).all()
    red = R.slab_reduce(slabs, splits, scale if wq == 8 else None)
    assert (red.view(np.uint16) == bits(yB)).all()
    slab = (wsA, splits, ds if wq == 8 else None, M)
    # ... into (Skip)RMSNorm
    h = _rows_data(M, N, M + N)
    dh, dnw = dev(h), dev(R.norm_weights(N))
    out0, res0 = canary_like((M, N), torch.float16), canary_like((M, N), torch.float16)
    out1, res1 = canary_like((M, N), torch.float16), canary_like((M, N), torch.float16)
    ck(L.pplhip_op_rmsnorm(None, P(dh), P(yB), P(dnw), R.EPS, M, N, P(out0), P(res0)))
    norm_ex(L, dh, None, dnw, M, N, out=out1, res=res1, slab=slab)
    assert torch.equal(out0.view(torch.int16), out1.view(torch.int16)) and torch.equal(res0.view(torch.int16), res1.view(torch.int16))
    assert not (bits(out1) == CANARY16).any()
    for f8, fn in ((0, L.pplhip_op_rmsnorm_quant), (1, L.pplhip_op_rmsnorm_quant_f8)):
        q0, s0 = canary_like((M, N), torch.int8), canary_like((M,), torch.float32)
        q1, s1 = canary_like((M, N), torch.int8), canary_like((M,), torch.float32)
        ck(fn(None, P(dh), P(yB), P(dnw), R.EPS, M, N, None, P(q0), P(s0)))
        norm_ex(L, dh, None, dnw, M, N, q=q1, sx=s1, f8=f8, slab=slab)
        assert torch.equal(q0, q1) and torch.equal(s0, s1) and not torch.isnan(s1).any()
    # ... into RoPE + KV write: the rows [3, 3 + M) of a step of M + 5 rows
    if N in R.ROPE_GEOMETRY:
        H, Hkv, D = R.ROPE_GEOMETRY[N]
        a = max(1, M // 3)
        seqlens, start_pos = [1, 1, 1, a, M - a + 2], [4, 9, 2, 0, 5]
        fmt = KV_FORMATS[(M + wq) % 4]
        check_chunk_from_slabs(m, fmt, H, Hkv, D, 3, 1, seqlens, start_pos, 3, M, slab_of=lambda Tc, n: (slab, yB.cpu().numpy()), seed=M)
