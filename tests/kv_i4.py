"""Test-side specification of the int4 KV cache (cache_quant_bit 4, cache_quant_group 32; DESIGN.md "numerics").

Per group of 32 consecutive channels of a head row of fp16 values x, in fp32:
    amax = max |x|;  t = amax / 7 (one correctly rounded division);  s = t rounded UP to 8 significant bits
    (u = (u + 0xFFFF) & ~0xFFFF on the fp32 bit pattern), clamped to [2^-14, 9344]: an fp16 number whose low three mantissa bits are zero;
    inv = 1 / s (correctly rounded);  q = clamp(rint(x * inv), -7, 7);  stored nibble q + 8 (1 .. 15).
Channel 2j of a group is the low nibble of byte j, channel 2j + 1 the high one; a head row is D / 2 bytes and D / 32 fp16 scales.
Every q * s is an fp16 number, so the int4 cache is the fp16 cache with every written group replaced by
Q(group) = dequantize(*quantize_groups(group)).  `ComposedOracle` is tests/kv_fp8.py's with exactly that replacement after each
layer's KV write.
"""
import ctypes as C

import numpy as np

from oracle import ref
from tests import kv_fp8 as F

GROUP = 32
S_MIN, S_MAX = np.float32(2.0 ** -14), np.float32(9344.0)
desc_with = F.desc_with


def scale_of_amax(amax):
    """fp32 scales (exactly fp16 numbers) of fp32 group maxima."""
    t = (np.asarray(amax, dtype=np.float32) / np.float32(7.0)).astype(np.float32)   # IEEE division: correctly rounded
    u = np.ascontiguousarray(t).view(np.uint32)
    u = (u + np.uint32(0xFFFF)) & np.uint32(0xFFFF0000)
    return np.clip(u.view(np.float32), S_MIN, S_MAX)


def quantize_groups(x):
    """fp16 rows [..., D] (D % 32 == 0) -> (q int8 in [-7, 7] [..., D], s fp16 [..., D / 32])."""
    x32 = np.asarray(x, dtype=np.float16).astype(np.float32)
    g = x32.reshape(x32.shape[:-1] + (x32.shape[-1] // GROUP, GROUP))
    s = scale_of_amax(np.abs(g).max(-1))
    inv = (np.float32(1.0) / s).astype(np.float32)
    q = np.clip(np.rint((g * inv[..., None]).astype(np.float32)), -7, 7).astype(np.int8)
    s16 = s.astype(np.float16)
    assert (s16.astype(np.float32) == s).all() and (s16.view(np.uint16) & 7 == 0).all(), "the scale is not an 8-bit fp16 number"
    return q.reshape(x32.shape), s16


def dequantize(q, s):
    """(q in [-7, 7] [..., D], fp16 scales [..., D / 32]) -> fp16 rows q * s (exact)."""
    q = np.asarray(q)
    s32 = np.asarray(s, dtype=np.float16).astype(np.float32)
    out = (q.reshape(s32.shape + (GROUP,)).astype(np.float32) * s32[..., None]).reshape(q.shape)
    h = out.astype(np.float16)
    assert (h.astype(np.float32) == out).all(), "q * s is not an fp16 number"
    return h


def qdq_rows(x):
    """Q(row): the fp16 rows an int4 cache holds for fp16 rows x."""
    return dequantize(*quantize_groups(x))


def pack_nibbles(q):
    """q in [-7, 7] [..., D] -> bytes [..., D / 2]: channel 2j the low nibble of byte j (q + 8), channel 2j + 1 the high one."""
    n = (np.asarray(q).astype(np.int16) + 8).astype(np.uint8)
    assert ((n >= 1) & (n <= 15)).all()
    return (n[..., 0::2] | (n[..., 1::2] << 4)).astype(np.uint8)


def unpack_nibbles(b):
    """bytes [..., D / 2] -> q int8 [..., D]."""
    b = np.asarray(b).view(np.uint8)
    q = np.empty(b.shape[:-1] + (2 * b.shape[-1],), dtype=np.int8)
    q[..., 0::2] = (b & 15).astype(np.int8) - 8
    q[..., 1::2] = (b >> 4).astype(np.int8) - 8
    return q


def slab_to_i4(slab16, D):
    """an fp16 KV slab (any layout: head rows are D-contiguous) -> (packed bytes as int8, fp16 scales), D / 32 scales per head row."""
    q, s = quantize_groups(np.asarray(slab16, dtype=np.float16).reshape(-1, D))
    return pack_nibbles(q).reshape(-1).view(np.int8), s.reshape(-1)


def i4_to_slab(cache_bytes, scales, D):
    """device int4 slab -> the fp16 slab it stands for."""
    q = unpack_nibbles(np.asarray(cache_bytes).view(np.uint8).reshape(-1, D // 2))
    return dequantize(q, np.asarray(scales, dtype=np.float16).reshape(-1, D // GROUP)).reshape(-1)


class ComposedOracle(F.ComposedOracle):
    """tests/kv_fp8.py's composed forward with the int4 Q: quant=True replaces every group of 32 channels of the slab by Q(group) after
    each layer's KV write, so that attention reads exactly what an int4 cache holds (Q is idempotent on groups already replaced)."""

    def forward(self, step):
        d, H, Hkv, D = self.d, self.H, self.Hkv, self.D
        tok, ss, sp, ci = step._keep[:4]
        T, B, hd, inter = len(tok), len(sp), d.hidden_dim, d.intermediate_dim
        L = ref.lib()
        h = np.empty((T, hd), dtype=np.float32)
        L.ref_embedding(tok.ctypes.data, self.w["tok_embeddings.weight"].ctypes.data, T, hd, h.ctypes.data)
        pending = None
        for l in range(d.num_layers):
            xn = self._norm(h, pending, self.w[f"layers.{l}.attention_norm.weight"], h)
            qkv = self._linear(f"layers.{l}.attention.wqkv", xn, (H + 2 * Hkv) * D, hd)
            L.ref_rope_kv_write(qkv.ctypes.data, self.rope.ctypes.data, C.byref(d), H, Hkv, D, l, self.kv.ctypes.data, None, self.N,
                                ss.ctypes.data, sp.ctypes.data, ci.ctypes.data, step.max_pages, B)
            if self.quant:
                self.kv[:] = qdq_rows(self.kv.reshape(-1, D)).reshape(-1)
            att = np.empty((T, H * D), dtype=np.float32)
            L.ref_attention(qkv.ctypes.data, C.byref(d), H, Hkv, D, l, self.kv.ctypes.data, None, self.N, ss.ctypes.data,
                            sp.ctypes.data, ci.ctypes.data, step.max_pages, B, att.ctypes.data)
            part = self._linear(f"layers.{l}.attention.wo", att, hd, H * D)
            xn = self._norm(h, part, self.w[f"layers.{l}.ffn_norm.weight"], h)
            gu = self._linear(f"layers.{l}.feed_forward.w13", xn, 2 * inter, hd)
            act = np.empty((T, inter), dtype=np.float32)
            L.ref_silu_mul(gu.ctypes.data, T, inter, act.ctypes.data)
            pending = self._linear(f"layers.{l}.feed_forward.w2", act, hd, inter)
        last = ss[1:] - 1
        hl = np.ascontiguousarray(h[last])
        pl = np.ascontiguousarray(pending[last])
        hn = self._norm(hl, pl, self.w["norm.weight"], None)
        return self._linear("output", hn, d.vocab_size, hd, out_fp32=1, quantized=False)
