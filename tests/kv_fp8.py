"""Test-side specification of the fp8 KV cache (cache_quant_bit 8, cache_quant_group = head_dim; DESIGN.md "numerics").

Per (token, layer, K|V, kv head) row of fp16 values x:
    amax = max |x|;  e = the smallest integer with 448 * 2^e >= amax, clamped to [-15, 8] (amax = 0: -15);
    q = e4m3fn_RNE(x * 2^-e) (OCP e4m3fn, torch's float8_e4m3fn), |q| <= 240 when e = 8;  scale slot = fp16(2^e).
Every dequantised element q * 2^e is an fp16 number, so the fp8 cache is the fp16 cache with every written row replaced by
Q(row) = dequantize(*quantize_rows(row)).  `composed_forward` is the oracle's forward assembled from its exported operators with
exactly that replacement after each layer's KV write.
"""
import ctypes as C

import numpy as np
import torch

from oracle import ref


def quantize_rows(x):
    """fp16 rows [..., D] -> (q uint8 e4m3fn codes [..., D], e int32 [...])."""
    x32 = np.asarray(x, dtype=np.float16).astype(np.float32)
    amax = np.abs(x32).max(-1)
    m, k = np.frexp(amax)                               # amax = m 2^k, m in [0.5, 1); 448 = 0.875 2^9
    e = np.where(m <= 0.875, k - 9, k - 8)
    e = np.where(amax == 0, -15, np.clip(e, -15, 8)).astype(np.int32)
    y = x32 * np.ldexp(np.float32(1.0), -e)[..., None].astype(np.float32)
    lim = np.where(e == 8, 240.0, 448.0).astype(np.float32)[..., None]
    y = np.clip(y, -lim, lim)
    q = torch.from_numpy(np.ascontiguousarray(y)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return q, e


def scale_of(e):
    """fp16 scale slot of exponent e: 2^e, exact."""
    return np.ldexp(np.float32(1.0), np.asarray(e)).astype(np.float16)


def exp_of(scale):
    """exponent e of fp16 scale slots (the inverse of scale_of)."""
    _, k = np.frexp(np.asarray(scale, dtype=np.float16).astype(np.float32))
    return (k - 1).astype(np.int32)


def dequantize(q, e):
    """(codes, exponents) -> fp16 rows q * 2^e (exact)."""
    v = torch.from_numpy(np.ascontiguousarray(q, dtype=np.uint8)).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    out = v * np.ldexp(np.float32(1.0), np.asarray(e))[..., None].astype(np.float32)
    h = out.astype(np.float16)
    assert (h.astype(np.float32) == out).all(), "q * 2^e is not an fp16 number"
    return h


def qdq_rows(x):
    """Q(row): the fp16 rows an fp8 cache holds for fp16 rows x."""
    return dequantize(*quantize_rows(x))


def slab_to_fp8(slab16, D):
    """an fp16 KV slab (any layout: head rows are D-contiguous) -> (e4m3 bytes as int8, fp16 scales), one scale per head row."""
    q, e = quantize_rows(np.asarray(slab16, dtype=np.float16).reshape(-1, D))
    return q.reshape(-1).view(np.int8), scale_of(e).reshape(-1)


def fp8_to_slab(cache_bytes, scales, D):
    """device fp8 slab -> the fp16 slab it stands for."""
    q = np.asarray(cache_bytes).view(np.uint8).reshape(-1, D)
    return dequantize(q, exp_of(scales).reshape(-1)).reshape(-1)


def desc_with(desc, **kw):
    d = ref.ModelDesc()
    for name, _ in ref.ModelDesc._fields_:
        setattr(d, name, getattr(desc, name))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


class ComposedOracle:
    """TP 1 forward of `ref.RefModel` `rm` (fp16 KV desc) assembled from the oracle's exported operators over an fp16 KV slab
    held here; quant=True replaces every head row of the slab by Q(row) after each layer's KV write, so that attention reads
    exactly what an fp8 cache holds (Q is idempotent on rows already replaced)."""

    def __init__(self, rm, tokens, quant=True):
        d = rm.desc
        assert d.cache_quant_bit == 0 and rm.tp_size == 1
        self.rm, self.d, self.quant, self.N = rm, d, quant, tokens
        self.H, self.Hkv = d.num_heads, d.num_kv_heads
        self.D = d.hidden_dim // d.num_heads
        self.kv = np.zeros(tokens * d.num_layers * 2 * self.Hkv * self.D, dtype=np.float16)
        self.rope = np.empty((d.max_position, self.D), dtype=np.float32)
        ref.lib().ref_build_rope_table(self.rope.ctypes.data, d.max_position, self.D, d.rope_theta)
        self.w = {n: self._get(n) for n in ref.tensor_names(d)}

    def _get(self, name):
        d = self.d
        if name.endswith(".scale"):
            return self.rm.get_tensor(name, np.float16)
        if name.endswith(".weight") and any(k in name for k in ("wqkv", "wo", "w13", "w2")) and d.weight_quant_bit:
            return self.rm.get_tensor(name, np.int8 if d.weight_quant_bit == 8 else np.uint8)
        return self.rm.get_tensor(name, np.float16)

    def _linear(self, name, x, N, K, out_fp32=0, quantized=True):
        d = self.d
        w = self.w[name + ".weight"]
        qbit = d.weight_quant_bit if quantized else 0
        sc = self.w[name + ".scale"] if qbit else None
        y = np.empty((x.shape[0], N), dtype=np.float32)
        ref.lib().ref_linear_raw(x.ctypes.data, w.ctypes.data, None if sc is None else sc.ctypes.data, qbit, d.weight_quant_group,
                                 x.shape[0], N, K, y.ctypes.data, out_fp32)
        return y

    def _norm(self, x, skip, w, residual):
        out = np.empty_like(x)
        ref.lib().ref_rmsnorm(x.ctypes.data, None if skip is None else skip.ctypes.data, w.ctypes.data, self.d.norm_eps, x.shape[0],
                              x.shape[1], out.ctypes.data, residual.ctypes.data if residual is not None else None)
        return out

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
