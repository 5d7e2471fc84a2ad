"""ALiBi attention as an operator (pplhip_op_attention_alibi, csrc/k_attn_alibi.hip) against float64 attention over the dequantised cache
with slope[h] * (j - p) on every score.  Bound: the one tests/test_gpu_attn_window.py and tests/test_gpu_attn_shared.py hold this comparison
to, 1.5e-3 + 1.5e-3 |want| elementwise.  The needle and zero-slope cases are exact."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import load_pplhip
from tests.test_gpu_attn_window import KV, PS, Case as WindowCase

gpu = pytest.mark.gpu
H = 3
SLOPES = [0.5, 2.0 ** -4, 0.0]


class Case(WindowCase):
    """the window test's requests, layout-3 cache and shuffled pages, multi-head; slopes None: the NULL pointer, "plain": pplhip_op_attention"""

    def __init__(self, fmt, paged, seqlens, start_pos, nd, needle=None, heads=(H, H), D=128):
        super().__init__(fmt, paged, heads[0], heads[1], seqlens, start_pos, nd, needle=needle, D=D)

    def reference(self, slopes):
        kv = self.cache[1].astype(np.float64)
        if self.scale is not None:
            kv = kv * np.repeat(self.scale[1].astype(np.float64), 8, axis=-1)
        q = self.qkv.astype(np.float64).reshape(self.T, -1, self.D)[:, :self.H]
        want, t = np.empty((self.T, self.H, self.D)), 0
        for b in range(self.B):
            for p in range(self.start_pos[b], self.kv_len[b]):
                j = np.arange(p + 1)
                sl = self.slots(b, j)
                for h in range(self.H):
                    s = kv[0, h, sl] @ q[t, h] / np.sqrt(self.D) + slopes[h] * (j - p)
                    e = np.exp(s - s.max())
                    want[t, h] = (e / e.sum()) @ kv[1, h, sl]
                t += 1
        return want.reshape(self.T, -1)

    def run(self, m, slopes, split=1):
        import torch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dq, dcache, dscale = dev(self.qkv), dev(self.cache), (dev(self.scale) if self.scale is not None else None)
        dseq, dsp, dtab = dev(np.concatenate([[0], np.cumsum(self.seqlens)])), dev(self.start_pos), dev(self.table)
        v = m.KvView()
        v.cache, v.scale = dcache.data_ptr(), (dscale.data_ptr() if dscale is not None else None)
        v.max_tokens, v.num_layers, v.kv_heads, v.head_dim = self.N, 2, self.Hkv, self.D
        v.quant_bit, v.quant_group = KV[self.fmt]
        v.layout, v.mode, v.page_size, v.layer = 3, int(self.paged), (PS if self.paged else 0), 1
        ws = torch.empty(self.nd * self.H * split * (self.D + 2) * 4 + 256, dtype=torch.uint8, device="cuda")
        out = torch.full((self.T, self.H * self.D), 7.0, dtype=torch.float16, device="cuda")
        args = [None, dq.data_ptr(), C.byref(v), dseq.data_ptr(), dsp.data_ptr(), dtab.data_ptr(), self.max_pages, self.B, self.T, self.nd,
                int(self.seqlens.max()), int(self.kv_len.max()), self.H, split, ws.data_ptr(), ws.numel(), out.data_ptr()]
        if slopes == "plain":
            rc = m.lib().pplhip_op_attention(*args)
        else:
            dslopes = None if slopes is None else dev(np.asarray(slopes, dtype=np.float32))
            rc = m.lib().pplhip_op_attention_alibi(*args, None if dslopes is None else dslopes.data_ptr())
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()


def check(case, split=1):
    rc, got = case.run(load_pplhip(), SLOPES, split)
    want = case.reference(SLOPES)
    err = np.abs(got.astype(np.float64) - want)
    print(f"split {split}: max err {err.max():.3e}, max |want| {np.abs(want).max():.3f}, worst err / bound {(err / (1.5e-3 + 1.5e-3 * np.abs(want))).max():.3f}")
    assert rc == 0 and np.isfinite(got).all() and (err <= 1.5e-3 + 1.5e-3 * np.abs(want)).all()


FORMS = pytest.mark.parametrize("fmt,paged", [(f, p) for f in ("fp16", "int8") for p in (False, True)])
MIXED = ([1, 1, 70, 33], [39, 200, 130, 0], 2)   # two decode rows, a cache-prefill and a prefill request in one call


@gpu
@FORMS
@pytest.mark.parametrize("split", [1, 3])
def test_alibi_decode(fmt, paged, split):
    """kv lengths around the wave's 16-token group and the block's 64-token stride; with 3 splits the short rows leave splits empty"""
    kv_len = [1, 16, 17, 64, 65, 257]
    check(Case(fmt, paged, [1] * len(kv_len), [n - 1 for n in kv_len], len(kv_len)), split)


@gpu
@FORMS
@pytest.mark.parametrize("seqlen,sp", [(33, 0), (64, 0), (65, 0), (130, 0), (40, 70), (5, 200)])
def test_alibi_prefill(fmt, paged, seqlen, sp):
    """A wave tile plus a row; a 64-key tile, and one key more; two query blocks; a cache-prefill, whose bias counts from the cache's first
    key; a short suffix behind a long prefix (launch_attn_prefill_alibi has no split-KV form at any length).  Measured on an MI355X: fp16 KV
    at most 9.8e-4 (0.21 of the bound); int8 KV at most 2.2e-3 at |want| 3.6, 0.49 .. 0.99 of the bound -- int8 x scale enters the MFMAs
    rounded to fp16 once, as in pplhip_op_attention's prefill kernel, whose bits a zero slope must give"""
    check(Case(fmt, paged, [seqlen], [sp], 0))


@gpu
@FORMS
def test_alibi_mixed_step(fmt, paged):
    check(Case(fmt, paged, *MIXED), split=2)


@gpu
@FORMS
@pytest.mark.parametrize("slopes", [[0.0] * H, None])
def test_alibi_zero_slopes_are_op_attention_bits(fmt, paged, slopes):
    case, m = Case(fmt, paged, *MIXED), load_pplhip()
    (rc0, a), (rc1, b) = case.run(m, slopes, 2), case.run(m, "plain", 2)
    assert rc0 == 0 and rc1 == 0 and (a.view(np.uint16) == b.view(np.uint16)).all()


@gpu
@FORMS
@pytest.mark.parametrize("kind", ["decode", "prefill"])
@pytest.mark.parametrize("back,want", [(50, -3.0), (120, 1.0)])
def test_alibi_needle(fmt, paged, kind, back, want):
    """q = 1, K = 0, V = 1 but one key with K = 8, V = -3, which leads by 90 nats unbiased.  Slope 1: 50 positions back it still leads by 40 nats
    and the output is its V exactly; 120 positions back each of the 30 nearest keys leads it and the output is their V exactly"""
    p = 157
    case = Case(fmt, paged, [1], [p], 1, needle=(0, p - back)) if kind == "decode" else Case(fmt, paged, [100], [100], 0, needle=(0, p - back))
    rc, got = case.run(load_pplhip(), [1.0] * H)
    assert rc == 0 and (got[0 if kind == "decode" else p - 100] == want).all()


@gpu
@pytest.mark.parametrize("fmt,dim,heads", [("fp16", 64, (4, 4)), ("fp8", 128, (4, 4)), ("int4", 128, (4, 4)), ("fp16", 128, (4, 2))])
def test_alibi_refusals(fmt, dim, heads):
    case = Case("fp16", True, [1, 60], [80, 0], 1, heads=heads, D=dim)
    case.fmt = fmt
    if fmt != "fp16":   # (the bytes are never read: the call refuses before any launch)
        case.cache, case.scale = np.zeros(case.cache.size // 2, dtype=np.uint8), np.zeros((2, 2, 4, case.N, 4), dtype=np.float16)
    rc, got = case.run(load_pplhip(), [0.5] * heads[0])
    assert rc == -7 and (got == 7.0).all()


@pytest.mark.parametrize("heads", [8, 40])
def test_alibi_standard_slopes(heads):
    n = 2 ** int(np.floor(np.log2(heads)))
    want = np.concatenate([2.0 ** (-8.0 * (np.arange(n) + 1) / n), 2.0 ** (-4.0 * (2 * np.arange(heads - n) + 1) / n)]).astype(np.float32)
    got = np.empty(heads, dtype=np.float32)
    assert load_pplhip().lib().pplhip_op_alibi_slopes(heads, got.ctypes.data) == 0 and (got == want).all()
