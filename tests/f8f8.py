"""Test-side specification of online_f8f8 (act_quant_bit PPLHIP_ACT_QUANT_FP8; DESIGN.md "numerics").

Activations (per token row, in front of every layer linear) and weights (per output row, quantised from fp16 at load) follow the
fp8 KV row rule of tests/kv_fp8.py: e = the smallest integer with 448 * 2^e >= max|x| (clamped to [-15, 8]), q = e4m3fn_RNE(x 2^-e),
scale 2^e.  The product is y[m,n] = fp16(2^(ex[m] + ew[n]) * sum_k qx * qw) with fp32 sums.  Every dequantised value q 2^e is an fp16
number and every product of two of them is exact in fp32, so the fp8 linear IS the oracle's fp16 linear on Q(x) and Q(w), up to the
fp32 summation order: `ComposedOracle` below is tests/kv_fp8.py's composed forward with that replacement in front of the four layer
linears (the lm_head stays fp16), optionally together with the fp8 KV cache.
"""
import ctypes as C

import numpy as np

from oracle import ref
from tests import kv_fp8
from tests.kv_fp8 import dequantize, exp_of, quantize_rows, scale_of  # noqa: F401

ACT_QUANT_I8 = 8
ACT_QUANT_FP8 = 0x108
LAYER_LINEARS = ("attention.wqkv", "attention.wo", "feed_forward.w13", "feed_forward.w2")


def qdq(x, K=None):
    """Q(rows): fp16-valued rows [..., K] -> the fp16 values (as fp32) an fp8 row stands for"""
    x = np.asarray(x)
    shape = x.shape
    rows = x.reshape(-1, K if K is not None else shape[-1])
    return dequantize(*quantize_rows(rows)).astype(np.float32).reshape(shape)


def e4m3_values():
    """fp32 value of every finite e4m3fn code (index = code; NaN codes 0x7f / 0xff as nan), from the format's definition"""
    v = np.empty(256, dtype=np.float64)
    for c in range(256):
        s, ex, m = c >> 7, (c >> 3) & 15, c & 7
        if ex == 15 and m == 7:
            v[c] = np.nan
        elif ex == 0:
            v[c] = m / 8.0 * 2.0 ** -6
        else:
            v[c] = (1 + m / 8.0) * 2.0 ** (ex - 7)
        if s:
            v[c] = -v[c]
    return v


def rne_code(y):
    """e4m3fn code of the scalar |y| <= 448 by exhaustive search: the nearest value, ties to the even code (the one whose mantissa
    LSB is 0); the sign of y is kept for zero too"""
    v = e4m3_values()
    pos = np.arange(128)[:127]                # +0 .. +448
    d = np.abs(v[pos] - abs(float(y)))
    best = np.flatnonzero(d == d.min())
    c = int(best[0]) if len(best) == 1 else int(best[(best & 1) == 0][0])
    return c | (0x80 if np.signbit(y) else 0)


class ComposedOracle(kv_fp8.ComposedOracle):
    """tests/kv_fp8.py's composed TP-1 forward of `rm` (an FP16-weight, fp16-KV `ref.RefModel`) with every layer linear
    multiplying Q(x) by Q(w): online_f8f8 when linears=True.  kv: "fp16", "fp8" (tests/kv_fp8.py: Q(row) after every KV write) or
    "int8" (the oracle's own int8-g8 cache: its KV write and attention run on the int8 desc and slabs).  With linears off and an
    fp16 cache it is ref.forward.

    tp > 1: the tensor-parallel split of wo / w2 (K sliced across ranks, pplhip.shard_weights): each rank quantises its own K-slice
    of the activation row and of every weight row, so Q applies per slice of K / tp columns."""

    def __init__(self, rm, tokens, kv="fp16", linears=True, tp=1):
        super().__init__(rm, tokens, quant=kv == "fp8")
        assert rm.desc.weight_quant_bit == 0 and kv in ("fp16", "fp8", "int8")
        self.linears, self.tp = linears, tp
        self.kvd, self.kv_scale = self.d, None
        if kv == "int8":
            self.kvd = kv_fp8.desc_with(self.d, cache_quant_bit=8, cache_quant_group=8)
            self.kv = np.zeros(self.kv.size, dtype=np.int8)
            self.kv_scale = np.zeros(self.kv.size // 8, dtype=np.float16)
        if linears:
            for name in list(self.w):
                lin = self._layer_linear(name)
                if lin and name.endswith(".weight"):
                    self.w[name] = qdq(self.w[name].astype(np.float32), self._slice(lin)).astype(np.float16)

    @staticmethod
    def _layer_linear(name):
        for lin in LAYER_LINEARS:
            if f".{lin}." in name:
                return lin
        return None

    def _slice(self, lin):
        """the row length one quantiser sees: the whole K, or a rank's K-slice of wo / w2"""
        if lin in ("attention.wo", "feed_forward.w2"):
            K = self.d.num_heads * (self.d.hidden_dim // self.d.num_heads) if lin == "attention.wo" else self.d.intermediate_dim
            return K // self.tp
        return self.d.hidden_dim

    def _linear(self, name, x, N, K, out_fp32=0, quantized=True):
        lin = self._layer_linear(name + ".weight")
        if self.linears and quantized and lin:
            x = np.ascontiguousarray(qdq(x, self._slice(lin)))
        return super()._linear(name, x, N, K, out_fp32, quantized)

    def forward(self, step):
        """tests/kv_fp8.py ComposedOracle.forward with the KV write and attention on self.kvd / self.kv_scale"""
        d, kd, H, Hkv, D = self.d, self.kvd, self.H, self.Hkv, self.D
        tok, ss, sp, ci = step._keep[:4]
        T, B, hd, inter = len(tok), len(sp), d.hidden_dim, d.intermediate_dim
        L = ref.lib()
        sc = None if self.kv_scale is None else self.kv_scale.ctypes.data
        h = np.empty((T, hd), dtype=np.float32)
        L.ref_embedding(tok.ctypes.data, self.w["tok_embeddings.weight"].ctypes.data, T, hd, h.ctypes.data)
        pending = None
        for l in range(d.num_layers):
            xn = self._norm(h, pending, self.w[f"layers.{l}.attention_norm.weight"], h)
            qkv = self._linear(f"layers.{l}.attention.wqkv", xn, (H + 2 * Hkv) * D, hd)
            L.ref_rope_kv_write(qkv.ctypes.data, self.rope.ctypes.data, C.byref(kd), H, Hkv, D, l, self.kv.ctypes.data, sc, self.N,
                                ss.ctypes.data, sp.ctypes.data, ci.ctypes.data, step.max_pages, B)
            if self.quant:
                self.kv[:] = kv_fp8.qdq_rows(self.kv.reshape(-1, D)).reshape(-1)
            att = np.empty((T, H * D), dtype=np.float32)
            L.ref_attention(qkv.ctypes.data, C.byref(kd), H, Hkv, D, l, self.kv.ctypes.data, sc, self.N, ss.ctypes.data,
                            sp.ctypes.data, ci.ctypes.data, step.max_pages, B, att.ctypes.data)
            part = self._linear(f"layers.{l}.attention.wo", att, hd, H * D)
            xn = self._norm(h, part, self.w[f"layers.{l}.ffn_norm.weight"], h)
            gu = self._linear(f"layers.{l}.feed_forward.w13", xn, 2 * inter, hd)
            act = np.empty((T, inter), dtype=np.float32)
            L.ref_silu_mul(gu.ctypes.data, T, inter, act.ctypes.data)
            pending = self._linear(f"layers.{l}.feed_forward.w2", act, hd, inter)
        last = ss[1:] - 1
        hn = self._norm(np.ascontiguousarray(h[last]), np.ascontiguousarray(pending[last]), self.w["norm.weight"], None)
        return self._linear("output", hn, d.vocab_size, hd, out_fp32=1, quantized=False)
