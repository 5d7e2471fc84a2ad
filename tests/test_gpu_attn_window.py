"""Sliding-window attention as an operator (pplhip_op_attention_window: the band prefill kernel and the windowed decode rows of
csrc/k_attn_window.hip) against float64 attention over the dequantised cache under the band mask max(0, p - W + 1) <= j <= p.
Bound: the one tests/test_gpu_attn_shared.py holds this comparison to, 1.5e-3 + 1.5e-3 |want| elementwise.  The needle cases are exact."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

D, PS = 128, 16
KV = {"fp16": (0, 1), "int8": (8, 8), "fp8": (8, 128), "int4": (4, 32)}   # (cache_quant_bit, cache_quant_group)
GEOM = [(4, 4), (8, 2)]


class Case:
    """requests with seqlens / start_pos, the first `nd` of them decode rows; needle = (request, key position): q = 1, every K = 0 and V = 1
    but that key's K = 8 and V = -3 (exact in fp16 and as int8 x scale 0.5): its score leads by 128 x 8 / sqrt(128) = 90 nats"""

    def __init__(self, fmt, paged, H, Hkv, seqlens, start_pos, nd, needle=None, D=D):
        rng = np.random.RandomState(H + 3 * len(seqlens) + int(sum(seqlens)))
        self.fmt, self.paged, self.H, self.Hkv, self.D, self.nd = fmt, paged, H, Hkv, D, nd
        self.seqlens, self.start_pos = np.asarray(seqlens, dtype=np.int64), np.asarray(start_pos, dtype=np.int64)
        self.B, self.T = len(seqlens), int(sum(seqlens))
        self.kv_len = self.start_pos + self.seqlens
        npg = (self.kv_len + PS - 1) // PS
        self.max_pages = int(npg.max())
        self.N = int(npg.sum() + 3) * PS
        if paged:   # shuffled pages; entries past a request's own stay at the padding value
            free = list(rng.permutation(self.N // PS))
            self.table = np.full((self.B, self.max_pages), np.iinfo(np.int64).max, dtype=np.int64)
            for b in range(self.B):
                self.table[b, :npg[b]] = [free.pop() for _ in range(npg[b])]
        else:
            self.table = (np.concatenate([[0], np.cumsum(npg[:-1])]) * PS + 5).astype(np.int64)
        shape = (2, 2, Hkv, self.N, D)   # layout 3: [layer, k / v, head, slot, channel]; layer 1 is used
        quant = fmt == "int8"
        if quant:
            self.cache = rng.randint(-127, 128, size=shape).astype(np.int8)
            self.scale = (0.02 * (0.5 + rng.rand(*shape[:-1], D // 8))).astype(np.float16)
        else:
            self.cache = rng.randn(*shape).astype(np.float16)
            self.scale = None
        q = rng.randn(self.T, H + 2 * Hkv, D)
        if needle:
            q[:] = 1.0
            self.cache[1, 0], self.cache[1, 1] = 0, (2 if quant else 1)
            if quant:
                self.scale[1] = 0.5
            s = self.slots(needle[0], np.array([needle[1]]))[0]
            self.cache[1, 0, :, s], self.cache[1, 1, :, s] = (16, -6) if quant else (8, -3)
        self.qkv = q.astype(np.float16).reshape(self.T, -1)

    def slots(self, b, pos):
        return self.table[b, pos // PS] * PS + pos % PS if self.paged else self.table[b] + pos

    def reference(self, W):
        kv = self.cache[1].astype(np.float64)
        if self.scale is not None:
            kv = kv * np.repeat(self.scale[1].astype(np.float64), 8, axis=-1)
        q = self.qkv.astype(np.float64).reshape(self.T, -1, self.D)[:, :self.H]
        grp, want, t = self.H // self.Hkv, np.empty((self.T, self.H, self.D)), 0
        for b in range(self.B):
            for i in range(self.seqlens[b]):
                p = self.start_pos[b] + i
                sl = self.slots(b, np.arange(max(0, p - W + 1), p + 1))
                for hk in range(self.Hkv):
                    s = q[t, hk * grp:(hk + 1) * grp] @ kv[0, hk, sl].T / np.sqrt(self.D)
                    e = np.exp(s - s.max(axis=1, keepdims=True))
                    want[t, hk * grp:(hk + 1) * grp] = (e / e.sum(axis=1, keepdims=True)) @ kv[1, hk, sl]
                t += 1
        return want.reshape(self.T, -1)

    def run(self, m, W, split=1, entry="window"):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dq, dcache = dev(self.qkv), dev(self.cache)
        dscale = dev(self.scale) if self.scale is not None else None
        dseq, dsp, dtab = dev(np.concatenate([[0], np.cumsum(self.seqlens)])), dev(self.start_pos), dev(self.table)
        v = m.KvView()
        v.cache, v.scale = dcache.data_ptr(), (dscale.data_ptr() if dscale is not None else None)
        v.max_tokens, v.num_layers, v.kv_heads, v.head_dim = self.N, 2, self.Hkv, self.D
        v.quant_bit, v.quant_group = KV[self.fmt]
        v.layout, v.mode, v.page_size, v.layer = 3, int(self.paged), (PS if self.paged else 0), 1
        ws = torch.empty(self.nd * self.H * split * (self.D + 2) * 4 + 512 + self.nd * (16 + 8 * self.max_pages) + 256, dtype=torch.uint8, device="cuda")
        out = torch.full((self.T, self.H * self.D), 7.0, dtype=torch.float16, device="cuda")
        args = [None, dq.data_ptr(), C.byref(v), dseq.data_ptr(), dsp.data_ptr(), dtab.data_ptr(), self.max_pages, self.B, self.T, self.nd,
                int(self.seqlens.max()), int(self.kv_len.max()), self.H, split, ws.data_ptr(), ws.numel(), out.data_ptr()]
        rc = m.lib().pplhip_op_attention_window(*args, W) if entry == "window" else m.lib().pplhip_op_attention(*args)
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()


def check(case, m, W, split=1):
    rc, got = case.run(m, W, split)
    assert rc == 0
    want = case.reference(W)
    err = np.abs(got.astype(np.float64) - want)
    print(f"window {W} split {split}: max err {err.max():.3e}, max |want| {np.abs(want).max():.3f}")
    assert np.isfinite(got).all() and (err <= 1.5e-3 + 1.5e-3 * np.abs(want)).all()


def decode_positions(W):
    return [W - 1, W, W + 1, W + 15, W + 16, 3 * W + 5]


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("W", [40, 64])
@pytest.mark.parametrize("H,Hkv", GEOM)
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("fmt", ["fp16", "int8"])
def test_window_decode(fmt, paged, H, Hkv, W, split):
    pos = decode_positions(W)
    check(Case(fmt, paged, H, Hkv, [1] * len(pos), pos, len(pos)), load_pplhip(), W, split)


# (W, seqlen, start_pos): W below a wave's 32 rows plus a 64-key tile -- wholly masked tiles at both ends, a tile that is both edges;
# a band that straddles tile and query-block boundaries; one row past the window; a cache-prefill whose band starts inside history
PREFILL = [(40, 300, 0), (100, 300, 0), (128, 129, 0), (96, 70, 130)]


@pytest.mark.parametrize("W,seqlen,sp", PREFILL)
@pytest.mark.parametrize("H,Hkv", GEOM)
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("fmt", ["fp16", "int8"])
def test_window_prefill(fmt, paged, H, Hkv, W, seqlen, sp):
    """Measured on an MI355X: max error 2.7e-4 .. 9.8e-4 in every case, fp16 and int8 alike -- half an fp16 ulp of the largest outputs
    (|want| up to 3.7).  int8 K / V enter the band kernel's MFMAs as exact hi + lo pairs; with int8 x scale rounded to fp16 once (the causal
    32-row kernel's form) two int8 cases sat at 2.6e-3, outside the bound."""
    check(Case(fmt, paged, H, Hkv, [seqlen], [sp], 0), load_pplhip(), W)


@pytest.mark.parametrize("H,Hkv", GEOM)
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("fmt", ["fp16", "int8"])
def test_window_never_binds_is_op_attention(fmt, paged, H, Hkv):
    """window 4096 over 200 tokens: the same launches as pplhip_op_attention, so the same bits"""
    case, m = Case(fmt, paged, H, Hkv, [200], [0], 0), load_pplhip()
    (rc0, a), (rc1, b) = case.run(m, 4096), case.run(m, 0, entry="plain")
    assert rc0 == 0 and rc1 == 0 and (a.view(np.uint16) == b.view(np.uint16)).all()


@pytest.mark.parametrize("H,Hkv", GEOM)
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("fmt", ["fp16", "int8"])
def test_window_mixed_step(fmt, paged, H, Hkv):
    """three decode rows, a cache-prefill and a prefill request in one call"""
    check(Case(fmt, paged, H, Hkv, [1, 1, 1, 70, 150], [39, 57, 200, 130, 0], 3), load_pplhip(), 40, split=2)


@pytest.mark.parametrize("inside", [False, True])
@pytest.mark.parametrize("kind", ["decode", "prefill"])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("fmt", ["fp16", "int8"])
def test_window_needle(fmt, paged, kind, inside):
    """a key that would take the whole softmax sits at p - W (just outside: the output is the other keys' V = 1 exactly) or at p - W + 1
    (just inside: the output is its V = -3 exactly); either window bound moved by one swaps the two"""
    W, p = 40, 157
    key = p - W + 1 if inside else p - W
    case = Case(fmt, paged, 8, 2, [1], [p], 1, needle=(0, key)) if kind == "decode" else Case(fmt, paged, 8, 2, [100], [100], 0, needle=(0, key))
    rc, got = case.run(load_pplhip(), W)
    assert rc == 0
    row = got[0] if kind == "decode" else got[p - 100]
    assert (row == (-3.0 if inside else 1.0)).all(), row[:8]
    if kind == "prefill":   # the rows around it: the needle is inside the window of rows p - W + 1 .. key + W - 1, and a row sees keys <= itself
        sees = (np.arange(100, 200) >= key) & (np.arange(100, 200) - W + 1 <= key)
        assert (got[sees] == -3.0).all() and (got[~sees] == 1.0).all()


@pytest.mark.parametrize("fmt,dim", [("fp16", 64), ("fp8", 128), ("int4", 128)])
def test_window_refusals(fmt, dim):
    case = Case("fp16", True, 4, 4, [1, 60], [80, 0], 1, D=dim)
    case.fmt = fmt
    if fmt != "fp16":   # (the bytes are never read: the call refuses before any launch)
        case.cache, case.scale = np.zeros(case.cache.size // 2, dtype=np.uint8), np.zeros((2, 2, 4, case.N, 4), dtype=np.float16)
    rc, got = case.run(load_pplhip(), 40)
    assert rc == -7 and (got == 7.0).all()
