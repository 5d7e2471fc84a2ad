"""Sharp attention inputs for pplhip_op_attention (no GPU here): a KV-slab builder with poison, two input families and a float64
reference that takes named mutations.

F1 (exact needles): queries are rows of a +-1 Sylvester Hadamard matrix; the heads of one kv-head group use disjoint rows, so their
dot products are exactly 0.  Background K is zero.  A needle is a key whose K is m * ALPHA * (its direction) with a small integer
multiplier m; every needle beats all other visible keys of its (row, head) by >= GAP natural-log units after the softmax scale, so
every other probability is exactly 0 in fp32 and the expected output is ONE V row, bit for bit.  `expect_gather` scores every
visible key exactly (float64 over the dequantised slab) and asserts the gap; it never trusts the construction.

F2 (sharp but unsaturated): per (request, kv head) a score matrix sigma[head in group, key] is realised as K = sum sigma h_dir / sqrt(D)
(so q . K / sqrt(D) = sigma before quantisation), with families 'compete' (a few keys within 0.5-3 units over a tail far below),
'sink' (key 0 holds about half the mass over a flat tail whose V has a non-zero mean) and 'rising' (each 64-key tile raises the
maximum by >= 5 units, asserted on the dequantised slab by check_rising).  These are checked against the C oracle at the existing bars; `ref64(case, mut)` is the float64 reference and
its mutations (MUTANTS) show that the bars would catch the named bugs.

Poison: every slab row no request owns (other layer, gap slots, spare and padding pages) holds K = GAMMA e_0 -- it scores like a
needle against every query (every Sylvester row starts with +1) -- and V = POISON_V on every channel.

Slab addressing mirrors kv_strides_of / kv_slot (oracle/llama_ref.c); fp8 rows reuse tests/kv_fp8.py, int4 rows tests/kv_i4.py.

int4 ('i4': 32-channel groups, 15 levels, one fp16 scale per group): F1's K rows (and the poison rows) take a power-of-two scale per
group, so that a small integer multiple of the needle amplitude round-trips exactly -- asserted for every K row, and a prefill
needle whose key row would not round-trip is refused (see _f1_prefill); every V row and F2's K rows take the product's own scale rule
(8 significant bits, not a power of two).  Every code x scale is an fp16 number, so the oracle runs on the fp16 slab the int4 slab
stands for, with exact operands.
"""
import ctypes as C
import math

import numpy as np

from oracle import ref
from tests import kv_fp8 as F8
from tests import kv_i4 as I4

GAP = 160.0            # F1: the needle's scaled score beats every other visible key by at least this (e^-160 == 0 in fp32)
GAMMA = 32768.0        # poison K on channel 0
POISON_V = 2048.0      # poison V on every channel
MAX_MULT = 6           # F1 needle multipliers 1..6 (fp8: integers <= 16 are exact e4m3 numbers, int8: codes <= 127, int4: <= 7)
RISE_STEP, RISE_RAMP, RISE_MIN = 8.0, 2.0, 5.0   # F2 'rising': level step per 64-key tile, ramp inside a tile, asserted rise

# kernel parameters the needle positions must straddle (csrc)
P3_BN = 64             # k_attn_prefill32.hip: keys per tile
PF_BN = 128            # k_attn_prefill.hip: keys per tile
PF_BM = 64             # k_attn_prefill.hip: half the query rows of a block (16 x PF_NW = 128, itself in the edge set below)
GQ_SUB, GQ_PAIR, GQ_STRIP = 16, 32, 128   # k_attn_decode_gqa.hip: sub-tile, pair step, split strip
DEC_UNROLL = 4         # k_attn_decode_dev.h


def alpha_of(D):
    """needle amplitude: ALPHA * sqrt(D) >= GAP (q = +-1)"""
    return 16.0 if D == 128 else 32.0


def hadamard(D):
    h = np.ones((1, 1))
    while h.shape[0] < D:
        h = np.block([[h, h], [h, -h]])
    return h


def gqa_form(fmt, H, Hkv, D):
    """mirror of attn_decode_gqa_supported (k_attn_decode_gqa.hip)"""
    grp = H // Hkv
    if grp < 4 or grp > 16 or H % Hkv:
        return False
    if fmt == "i4":
        return D == 128
    return D in (64, 128) if fmt != "f16" else D in (32, 64, 128)


def dec_key_step(fmt, D, threads=256):
    """keys per wave step and per block step of the multi-head decode kernel (AttnCfg, k_attn_dev.h)"""
    lpt = D // (32 if fmt == "i4" else 16 // (1 if fmt != "f16" else 2))   # int4: a lane piece is one group of 32 channels
    tpw = 64 // lpt
    nw = max(threads, D) // 64
    return tpw * DEC_UNROLL, nw * tpw * DEC_UNROLL


def split_chunks(n, split, gqa):
    """[beg, end) key ranges of the decode K-splits of one request of n keys"""
    per = -(-n // split)
    if gqa:
        per = -(-per // GQ_STRIP) * GQ_STRIP
    return [(s * per, min(n, (s + 1) * per)) for s in range(split) if s * per < n]


def p32_nsplit(max_seq_len, nreq, H, max_kv_len, forced=0):
    """number of KV splits launch_attn_prefill32 picks when a workspace is given (k_attn_prefill32.hip)"""
    nqb4 = (max_seq_len + 127) // 128
    blocks4 = nqb4 * nreq * H
    if not (max_seq_len < 1024 and blocks4 < 256 and max_kv_len >= 1024):
        return 1
    ntiles = (max_kv_len + P3_BN - 1) // P3_BN
    ns = min((512 + blocks4 - 1) // blocks4, ntiles // 4, 32)
    return forced if forced > 1 else ns


def p32_chunks(start, seqlen, i, nsplit):
    """[beg, end) key ranges of the split-KV blocks of the 128-row query block holding row i"""
    q0 = i // 128 * 128
    kv_end = start + min(q0 + 127, seqlen - 1) + 1
    nt = (kv_end + P3_BN - 1) // P3_BN
    out = []
    for y in range(nsplit):
        tb, te = nt * y // nsplit, nt * (y + 1) // nsplit
        if tb < te:
            out.append((tb * P3_BN, te * P3_BN))
    return out


def view5(flat, layout, N, L, h, d):
    """the flat slab as a [L, 2, h, N, d] view (writes go through): the strides of kv_strides_of for layouts 0-3"""
    if layout == 0:
        return flat.reshape(N, L, 2, h, d).transpose(1, 2, 3, 0, 4)
    if layout == 1:
        return flat.reshape(L, N, 2, h, d).transpose(0, 2, 3, 1, 4)
    if layout == 2:
        return flat.reshape(L, 2, N, h, d).transpose(0, 1, 3, 2, 4)
    return flat.reshape(L, 2, h, N, d)


def encode(fmt, x, pow2=False):
    """float rows [..., D] -> (codes, scales): fp16 values; int8 codes with one power-of-two fp16 scale per 8 channels (code x scale is
    an fp16 number); fp8 e4m3 codes with the row's power-of-two scale (tests/kv_fp8.py); int4 nibbles packed into [..., D / 2] bytes
    with one fp16 scale per 32 channels: the product's rule (tests/kv_i4.py), or with pow2 the power of two 2^ceil(log2(amax / 7))"""
    x = np.asarray(x, dtype=np.float32)
    D = x.shape[-1]
    if fmt == "f16":
        return x.astype(np.float16), None
    if fmt == "i8":
        g = x.reshape(x.shape[:-1] + (D // 8, 8))
        amax = np.abs(g).max(-1)
        e = np.ceil(np.log2(np.maximum(amax, 1e-30) / 127.0))
        e = np.where(amax == 0, -12.0, np.clip(e, -24, 15))
        s = np.ldexp(np.float32(1.0), e.astype(np.int32))
        codes = np.clip(np.rint(g / s[..., None]), -127, 127).astype(np.int8)
        return codes.reshape(x.shape), s.astype(np.float16)
    if fmt == "i4":
        if not pow2:
            q, s = I4.quantize_groups(x.astype(np.float16))
            return I4.pack_nibbles(q).view(np.int8), s
        g = x.reshape(x.shape[:-1] + (D // I4.GROUP, I4.GROUP))
        amax = np.abs(g).max(-1)
        e = np.ceil(np.log2(np.maximum(amax, 1e-30) / 7.0))
        e = np.where(amax == 0, -14.0, np.clip(e, -14, 13))   # within the product's scale range [2^-14, 9344]
        s = np.ldexp(np.float32(1.0), e.astype(np.int32))
        q = np.clip(np.rint(g / s[..., None]), -7, 7).astype(np.int8)
        return I4.pack_nibbles(q.reshape(x.shape)).view(np.int8), s.astype(np.float16)
    q, e = F8.quantize_rows(x.astype(np.float16))
    return q.view(np.int8), F8.scale_of(e)[..., None]


def decode(fmt, codes, scales, i4_mut=None):
    """(codes, scales) -> float64 rows; i4_mut: an int4 slab read wrongly ('nibble_order': low and high nibble swapped, 'bias8': the
    + 8 of the stored nibble left in)"""
    if fmt == "f16":
        return codes.astype(np.float64)
    if fmt == "i4":
        q = I4.unpack_nibbles(codes).astype(np.float64)
        if i4_mut == "nibble_order":
            q = q.reshape(q.shape[:-1] + (-1, 2))[..., ::-1].reshape(q.shape)
        if i4_mut == "bias8":
            q = q + 8.0
        g = q.reshape(q.shape[:-1] + (scales.shape[-1], I4.GROUP))
        return (g * scales.astype(np.float64)[..., None]).reshape(q.shape)
    D = codes.shape[-1]
    if fmt == "i8":
        g = codes.astype(np.float64).reshape(codes.shape[:-1] + (D // 8, 8))
        return (g * scales.astype(np.float64)[..., None]).reshape(codes.shape)
    e = F8.exp_of(scales[..., 0])
    v = F8.dequantize(codes.view(np.uint8), e)
    return v.astype(np.float64)


class Case:
    """one pplhip_op_attention launch: requests (seqlens new rows at start_pos), the first `nb` of them decode rows (one row each).
    Builders fill self.K[b], self.V[b] ([Hkv, kvlen_b, D] floats) and self.Q ([T, H, D]); finish() writes the slab.  (f1_stream
    writes request by request instead and keeps no K / V.)"""

    def __init__(self, fmt, H, Hkv, D, seqlens, start_pos, nb=0, layout=3, mode=0, page_size=16, L=2, layer=1, split=1, seed=0,
                 p32_split=0, name=""):
        self.fmt, self.H, self.Hkv, self.D, self.L, self.layer = fmt, H, Hkv, D, L, layer
        self.layout, self.mode, self.page_size, self.split, self.nb = layout, mode, page_size if mode else 0, split, nb
        self.name = name
        self.grp = H // Hkv
        self.rng = np.random.RandomState(seed)
        self.seqlens = np.asarray(seqlens, dtype=np.int64)
        self.start_pos = np.asarray(start_pos, dtype=np.int64)
        self.B = len(self.seqlens)
        self.kvlen = self.start_pos + self.seqlens
        self.seq_starts = np.concatenate([[0], np.cumsum(self.seqlens)]).astype(np.int64)
        self.T = int(self.seqlens.sum())
        self.max_seq_len = int(self.seqlens[nb:].max()) if self.B > nb else 1
        self.max_kv_len = int(self.kvlen.max())
        rng = self.rng
        if mode == 0:
            gaps = 1 + rng.randint(0, 4, size=self.B)
            self.cache_idx = (np.concatenate([[0], np.cumsum(self.kvlen + gaps)[:-1]]) + 3).astype(np.int64)
            self.max_pages = 0
            self.N = int((self.kvlen + gaps).sum()) + 8
        else:
            P = page_size
            npg = (self.kvlen + P - 1) // P
            self.max_pages = int(npg.max())
            n_pages = int(npg.sum()) + 3
            order = rng.permutation(n_pages)
            # unused page-table entries name a spare (poison) page: a read through them shows instead of faulting
            self.spare_page = int(order[-1])
            self.cache_idx = np.full((self.B, self.max_pages), self.spare_page, dtype=np.int64)
            k = 0
            for i in range(self.B):
                self.cache_idx[i, :npg[i]] = order[k:k + npg[i]]
                k += npg[i]
            self.N = n_pages * P
        self.K = [np.zeros((Hkv, int(n), D), dtype=np.float32) for n in self.kvlen]
        self.V = [np.zeros((Hkv, int(n), D), dtype=np.float32) for n in self.kvlen]
        self.Q = np.zeros((self.T, H, D), dtype=np.float32)
        self.needles_b = [set() for _ in range(self.B)]   # F1: key positions that carry a needle, per request
        self.special = {}           # F2: key positions with designed scores (edges used), per request
        self.p32_split = p32_split  # split-KV prefill: number of splits the launcher will pick (0: unsplit)
        self.family = None

    # ---------------------------------------------------------------- addressing
    def slots(self, b, pos):
        pos = np.asarray(pos, dtype=np.int64)
        if self.mode == 0:
            return self.cache_idx[b] + pos
        P = self.page_size
        return self.cache_idx[b, pos // P] * P + pos % P

    def row_of(self, b, i):
        """(token row, position) of row i of request b"""
        return int(self.seq_starts[b] + i), int(self.start_pos[b] + i)

    # ---------------------------------------------------------------- the slab
    def _alloc(self):
        """the slab, all poison; the step's qkv rows (zero)"""
        D, Hkv, L, N, H = self.D, self.Hkv, self.L, self.N, self.H
        elems = N * L * 2 * Hkv * D
        gsz = 8 if self.fmt == "i8" else (I4.GROUP if self.fmt == "i4" else D)
        dw = D // 2 if self.fmt == "i4" else D   # slab elements per head row (int4: two channels per byte)
        self.cache = np.zeros(elems // D * dw, dtype=np.float16 if self.fmt == "f16" else np.int8)
        self.scale = None if self.fmt == "f16" else np.zeros(elems // gsz, dtype=np.float16)
        self.cv = view5(self.cache, self.layout, N, L, Hkv, dw)
        self.sv = None if self.scale is None else view5(self.scale, self.layout, N, L, Hkv, D // gsz)
        pk = np.zeros(D, dtype=np.float32)
        pk[0] = GAMMA
        for kv, row in ((0, pk), (1, np.full(D, POISON_V, dtype=np.float32))):
            c, sc = encode(self.fmt, row, pow2=True)   # (int4: GAMMA = 4 x 2^13 and POISON_V = 4 x 2^9 exactly)
            self.cv[:, kv] = c
            if self.sv is not None:
                self.sv[:, kv] = sc
        self.qkv = np.zeros((self.T, (H + 2 * Hkv) * D), dtype=np.float16)
        self.Kd, self.Vd = [], []

    def _put(self, b, K, V):
        """writes request b's rows into the slab; returns their dequantised values (float32: fp16 numbers in every format).
        int4: F1's K rows take power-of-two scales and must round-trip exactly; V and F2's K take the product's scale rule"""
        H, Hkv, D = self.H, self.Hkv, self.D
        sl = self.slots(b, np.arange(self.kvlen[b]))
        deq = []
        for kv, rows in ((0, K), (1, V)):
            exact = self.fmt == "i4" and kv == 0 and self.family is None
            c, sc = encode(self.fmt, rows, pow2=exact)
            if exact:
                bad = np.argwhere((decode(self.fmt, c, sc) != rows).any(-1))
                assert len(bad) == 0, f"{self.name}: request {b}: K rows (kv head, key) {bad[:4].tolist()} do not round-trip through int4"
            self.cv[self.layer, kv][:, sl] = c
            if self.sv is not None:
                self.sv[self.layer, kv][:, sl] = sc
            deq.append(decode(self.fmt, c, sc).astype(np.float32))
        r0, r1 = self.seq_starts[b], self.seq_starts[b + 1]
        pos = np.arange(self.start_pos[b], self.kvlen[b])
        # the step's own K / V rows equal the slab rows
        self.qkv[r0:r1, H * D:(H + Hkv) * D] = deq[0][:, pos].transpose(1, 0, 2).reshape(len(pos), -1)
        self.qkv[r0:r1, (H + Hkv) * D:] = deq[1][:, pos].transpose(1, 0, 2).reshape(len(pos), -1)
        return deq

    def _set_q(self):
        H, D = self.H, self.D
        self.qkv[:, :H * D] = self.Q.reshape(self.T, H * D).astype(np.float16)
        assert (self.qkv[:, :H * D].astype(np.float32) == self.Q.reshape(self.T, -1)).all(), "q is not fp16"

    def finish(self):
        self._alloc()
        for b in range(self.B):
            kd, vd = self._put(b, self.K[b], self.V[b])
            self.Kd.append(kd)
            self.Vd.append(vd)
        self.K = self.V = None
        self._set_q()
        return self

    def read(self, kv, hk, slots, scale_from=None, group_shift=False, i4_mut=None):
        """dequantised slab rows of layer self.layer (float64); scale_from: read the scales of K (0) instead; group_shift: each
        int8 / int4 group takes its neighbour's scale; i4_mut: see decode"""
        c = self.cv[self.layer, kv][hk, slots]
        if self.sv is None:
            return c.astype(np.float64)
        s = self.sv[self.layer, kv if scale_from is None else scale_from][hk, slots]
        if group_shift:
            s = s[..., np.arange(s.shape[-1]) ^ 1]
        return decode(self.fmt, c, s, i4_mut)

    # ---------------------------------------------------------------- the oracle
    def desc(self):
        q8 = self.fmt == "i8"
        return ref.make_desc(hidden_dim=self.H * self.D, intermediate_dim=64, num_layers=self.L, num_heads=self.H,
                             num_kv_heads=self.Hkv, vocab_size=64, cache_quant_bit=8 if q8 else 0, cache_quant_group=8 if q8 else 1,
                             cache_layout=self.layout, cache_mode=self.mode, page_size=self.page_size)

    def oracle(self):
        """ref_attention (fp32, oracle/llama_ref.c) on the slab; fp8 and int4: on the fp16 slab it stands for"""
        d = self.desc()
        if self.fmt == "f8":
            cache, scale = F8.fp8_to_slab(self.cache, self.scale, self.D), None
        elif self.fmt == "i4":
            cache, scale = I4.i4_to_slab(self.cache, self.scale, self.D), None
        else:
            cache, scale = self.cache, self.scale
        q32 = np.ascontiguousarray(self.qkv.astype(np.float32))
        out = np.zeros((self.T, self.H * self.D), dtype=np.float32)
        ref.lib().ref_attention(q32.ctypes.data, C.byref(d), self.H, self.Hkv, self.D, self.layer, cache.ctypes.data,
                                None if scale is None else scale.ctypes.data, self.N, self.seq_starts.ctypes.data,
                                self.start_pos.ctypes.data, self.cache_idx.ctypes.data, self.max_pages, self.B, out.ctypes.data)
        return out

    def view(self, m, dcache, dscale):
        v = m.KvView()
        v.cache, v.scale = dcache.data_ptr(), (dscale.data_ptr() if dscale is not None else None)
        v.max_tokens, v.num_layers, v.kv_heads, v.head_dim = self.N, self.L, self.Hkv, self.D
        qb = 0 if self.fmt == "f16" else 8
        v.quant_bit, v.quant_group = qb, (8 if self.fmt == "i8" else (self.D if self.fmt == "f8" else 1))
        if self.fmt == "i4":
            v.quant_bit, v.quant_group = 4, I4.GROUP
        v.layout, v.mode, v.page_size, v.layer = self.layout, self.mode, self.page_size, self.layer
        return v

    # ---------------------------------------------------------------- kernel-form facts
    def decode_chunks(self, b):
        return split_chunks(int(self.kvlen[b]), self.split, gqa_form(self.fmt, self.H, self.Hkv, self.D))

    def chunks(self, b, i):
        """the K-split key ranges row i of request b is computed in (one range when unsplit)"""
        if b < self.nb:
            return self.decode_chunks(b) if self.split > 1 else None
        if self.p32_split > 1:
            return p32_chunks(int(self.start_pos[b]), int(self.seqlens[b]), i, self.p32_split)
        return None

    def edge_strides(self):
        """key strides of the kernel forms this launch reaches, whose both sides the F1 needles must cover"""
        st = set()
        if self.mode == 1:
            st.add(self.page_size)
        if self.nb > 0:
            if gqa_form(self.fmt, self.H, self.Hkv, self.D):
                st.update({GQ_SUB, GQ_PAIR, GQ_STRIP})
            else:
                st.update(dec_key_step(self.fmt, self.D))
        if self.B > self.nb:
            st.add(P3_BN if self.D == 128 else PF_BN)
        return sorted(st)


# -------------------------------------------------------------------------------------------------------------------------------------
# positions
# -------------------------------------------------------------------------------------------------------------------------------------
def edge_positions(n, strides, chunks=(), rng=None, deep=True):
    """both sides of the first two edges of every stride, of every split chunk, key 0, the last key, and (n > 4096) a few deep ones"""
    pos = {0, n - 1}
    for s in strides:
        for k in (1, 2):
            if k * s < n:
                pos.update({k * s - 1, k * s})
        if rng is not None and n > 4 * s:
            k = int(rng.randint(3, n // s))
            if k * s < n:
                pos.update({k * s - 1, k * s})
    for beg, _ in chunks:
        if beg > 0:
            pos.update({beg - 1, beg})
    if deep and n > 4096 and rng is not None:
        pos.update(int(x) for x in rng.randint(4096, n, size=3))
    return sorted(p for p in pos if 0 <= p < n)


def dirs_of(case, hq):
    """Hadamard rows of head hq: a disjoint set per head of the kv-head group"""
    nd = case.D // case.grp
    gi = hq % case.grp
    return [gi * nd + k for k in range(nd)]


# -------------------------------------------------------------------------------------------------------------------------------------
# F1: exact needles
# -------------------------------------------------------------------------------------------------------------------------------------
def _group_factor(case):
    """per-channel magnitude of V: neighbouring quant groups (int8: 8 channels, int4: 32) differ, so a neighbour's scale shows"""
    gsz = {"i8": 8, "i4": I4.GROUP}.get(case.fmt)
    return np.where((np.arange(case.D) // gsz) % 2 == 1, 0.3, 1.0) if gsz else np.ones(case.D)


def _f1_values(case, n):
    """distinct V rows; int8: odd groups smaller, so that neighbouring groups take different power-of-two scales; int4: likewise
    per 32 channels (product-rule scales)"""
    f = _group_factor(case)
    return (case.rng.uniform(-3, 3, size=(case.Hkv, n, case.D)) * f).astype(np.float32)


def f1(case):
    """fill case with F1 rows: distinct V everywhere, needles for every (row, head); returns case.finish()"""
    Hd, a = hadamard(case.D), alpha_of(case.D)
    for b in range(case.B):
        case.V[b][:] = _f1_values(case, int(case.kvlen[b]))
    for b in range(case.B):
        if b < case.nb:
            _f1_decode(case, b, Hd, a)
        else:
            _f1_prefill(case, b, Hd, a)
    return case.finish()


def f1_stream(case):
    """F1 for decode launches too large to hold K / V per request (config 2: 1024 x 32 heads x ~525 keys): each request's rows go
    straight into the slab and its expected gather is taken at once; expect_gather returns the result"""
    assert case.nb == case.B, "decode rows only"
    Hd, a = hadamard(case.D), alpha_of(case.D)
    case._alloc()
    case.want = np.zeros((case.T, case.H * case.D), dtype=np.float16)
    case.top = np.zeros((case.T, case.H), dtype=np.int64)
    case.K, case.V = [None] * case.B, [None] * case.B
    for b in range(case.B):
        n = int(case.kvlen[b])
        case.K[b] = np.zeros((case.Hkv, n, case.D), dtype=np.float32)
        case.V[b] = _f1_values(case, n)
        _f1_decode(case, b, Hd, a)
        kd, vd = case._put(b, case.K[b], case.V[b])
        case.K[b] = case.V[b] = None
        _gather_request(case, b, kd, vd, case.Q, case.want, case.top)
    case.K = case.V = None
    case._set_q()
    case.streamed = True
    return case


def edge_pairs(n, strides, chunks=(), rng=None):
    """(e - 1, e) pairs in priority order: split chunk starts, the first edge of every stride, the second ones, a random one each"""
    cp = [(beg - 1, beg) for beg, _ in chunks if beg > 0]
    out = cp[:1] + [(s - 1, s) for s in strides if s < n] + cp[1:] + [(2 * s - 1, 2 * s) for s in strides if 2 * s < n]
    if rng is not None:
        for s in strides:
            if n > 4 * s:
                k = int(rng.randint(3, n // s))
                if k * s < n:
                    out.append((k * s - 1, k * s))
    return out


def _f1_decode(case, b, Hd, a):
    """head 0: the current token; head 1: key 0 (the first request of each length) or a deep key before the last one; the other
    heads: edge pairs, the requests of one length taking successive pairs"""
    n = int(case.kvlen[b])
    chunks = case.decode_chunks(b) if case.split > 1 else ()
    pairs = edge_pairs(n, case.edge_strides(), chunks, case.rng)
    rank = int((case.kvlen[:b] == n).sum())
    ppr = (case.H - 2) // 2
    flat = [p for k in range(ppr) for p in (pairs[(rank * ppr + k) % len(pairs)] if pairs else (0, n - 1))]
    t, _ = case.row_of(b, 0)
    for hq in range(case.H):
        hk = hq // case.grp
        ds = dirs_of(case, hq)
        d = ds[(b + hq) % len(ds)]
        if hq == 0:
            p = n - 1
        elif hq == 1:   # deep keys stay off the last one: n > 4096 -> a key in [4096, n - 2]
            p = 0 if rank == 0 or n < 64 else int(case.rng.randint(4096 if n > 4097 else n // 2, n - 1))
        else:
            p = flat[(hq - 2) % len(flat)] if hq - 2 < len(flat) else int(case.rng.randint(0, n))
        case.K[b][hk, p] += a * Hd[d]
        case.Q[t, hq] = Hd[d]
        case.needles_b[b].add(p)


def _i4_exact(row):
    """does a K row survive the int4 encoder with power-of-two scales unchanged?"""
    return bool((decode("i4", *encode("i4", row, pow2=True)) == row).all())


def _f1_prefill(case, b, Hd, a):
    """rows cycle through the head's directions; every direction gets a needle no later than its first row; rows at edge positions
    get a needle on their own diagonal key or a probe (a stronger needle one key past them) -- alternately -- while the direction
    has multipliers left.  int4: a needle whose key row would not round-trip is refused (put); a direction's first needle then
    moves on to the next prefix edge or the row's own key"""
    s0, S, n = int(case.start_pos[b]), int(case.seqlens[b]), int(case.kvlen[b])
    st = case.edge_strides()
    edges = set(edge_positions(n, st + [PF_BM, 128, 256], (), case.rng))
    if case.p32_split > 1:
        for i in range(0, S, 128):
            for beg, _ in p32_chunks(s0, S, i, case.p32_split):
                if beg > 0:
                    edges.update({beg - 1, beg})
    prefix = sorted(p for p in edges if p < s0)
    for hq in range(case.H):
        hk = hq // case.grp
        ds = dirs_of(case, hq)
        run = max(1, S // (4 * len(ds)) if S > 64 else 1)
        mult = {d: 0 for d in ds}
        used = {d: set() for d in ds}
        k_pref, flip = hq, hq % 2

        def put(d, p):
            if mult[d] >= MAX_MULT or p in used[d] or p >= n:
                return False
            # int4: the key row may already carry needles of other heads and directions; refuse a sum that 15 levels cannot hold
            if case.fmt == "i4" and not _i4_exact(case.K[b][hk, p] + (mult[d] + 1) * a * Hd[d]):
                return False
            mult[d] += 1
            used[d].add(p)
            case.K[b][hk, p] += mult[d] * a * Hd[d]
            case.needles_b[b].add(p)
            return True

        for i in range(S):
            t, p = case.row_of(b, i)
            d = ds[(i // run) % len(ds)]
            case.Q[t, hq] = Hd[d]
            if mult[d] == 0:     # first row of this direction: a needle in the cached prefix (at an edge) or on its own diagonal
                if case.fmt == "i4":   # a refused key falls through to the next prefix edges, then to the row's own diagonal key
                    cands = [prefix[(k_pref + j) % len(prefix)] for j in range(len(prefix))] if prefix and (k_pref % 3 != 2) else []
                    assert any(put(d, c) for c in cands + [p]), f"{case.name}: request {b} head {hq} row {i}: no needle fits int4"
                    k_pref += 1
                elif prefix and (k_pref % 3 != 2):
                    put(d, prefix[k_pref % len(prefix)])
                    k_pref += 1
                else:
                    put(d, p)
                    k_pref += 1
            elif p in edges or (p + 1) in edges or i == S - 1:
                flip ^= 1
                put(d, p + 1 if flip else p)


def _gather_request(case, b, Kd, Vd, Q, want, top):
    """request b of an F1 case: every visible key scored exactly (float64), the top one asserted >= GAP above the runner-up, its
    V row written into want (fp16) and its index into top"""
    D, H, grp = case.D, case.H, case.grp
    sm = 1.0 / math.sqrt(D)
    s0, S, n = int(case.start_pos[b]), int(case.seqlens[b]), int(case.kvlen[b])
    r0 = int(case.seq_starts[b])
    q = Q[r0:r0 + S].astype(np.float64)
    for hk in range(case.Hkv):
        K = Kd[hk].astype(np.float64)
        for c0 in range(0, S, 256):
            c1 = min(S, c0 + 256)
            qg = q[c0:c1, hk * grp:(hk + 1) * grp]                                   # [rows, grp, D]
            sc = np.einsum("rgd,kd->rgk", qg, K) * sm
            pos = s0 + np.arange(c0, c1)
            sc = np.where(np.arange(n)[None, None, :] > pos[:, None, None], -np.inf, sc)
            best = sc.argmax(-1)
            s1 = np.take_along_axis(sc, best[..., None], -1)[..., 0]
            np.put_along_axis(sc, best[..., None], -np.inf, -1)
            gap = s1 - sc.max(-1)
            if not (gap >= GAP).all():
                r, g = np.argwhere(~(gap >= GAP))[0]
                raise AssertionError(f"{case.name}: request {b} row {c0 + r} head {hk * grp + g}: top key {best[r, g]} "
                                     f"beats the runner-up by {gap[r, g]:.1f} < {GAP}")
            top[r0 + c0:r0 + c1, hk * grp:(hk + 1) * grp] = best
            want[r0 + c0:r0 + c1].reshape(c1 - c0, H, D)[:, hk * grp:(hk + 1) * grp] = Vd[hk][best].astype(np.float16)


def expect_gather(case):
    """F1: (expected fp16 output [T, H*D], top key per (row, head) [T, H]).  Scores every visible key exactly from the dequantised
    slab and asserts that the top one beats the runner-up by >= GAP."""
    if getattr(case, "streamed", False):
        return case.want, case.top
    want = np.zeros((case.T, case.H * case.D), dtype=np.float16)
    top = np.zeros((case.T, case.H), dtype=np.int64)
    q = case.qkv[:, :case.H * case.D].astype(np.float32).reshape(case.T, case.H, case.D)
    for b in range(case.B):
        _gather_request(case, b, case.Kd[b], case.Vd[b], q, want, top)
    return want, top


def explain_mismatch(case, got, want, top, limit=8):
    """failure text: row, head, expected key and the key whose V row was produced (looked up by V row)"""
    D, H = case.D, case.H
    g = got.reshape(case.T, H, D)
    w = want.reshape(case.T, H, D)
    bad = np.argwhere((g.view(np.uint16) != w.view(np.uint16)).any(-1))
    lines = [f"{case.name}: {len(bad)} (row, head) outputs differ from the gathered V row"]
    for t, hq in bad[:limit]:
        b = int(np.searchsorted(case.seq_starts, t, side="right") - 1)
        hk = hq // case.grp
        V = case.read(1, hk, case.slots(b, np.arange(case.kvlen[b]))).astype(np.float16)
        hit = np.where((V.view(np.uint16) == g[t, hq].view(np.uint16)).all(-1))[0]
        if len(hit):
            what = f"key {int(hit[0])}'s V"
        elif np.abs(g[t, hq].astype(np.float32) - POISON_V).max() < 1.0:
            what = "the POISON V row (a slot the request does not own)"
        else:
            err = float(np.abs(g[t, hq].astype(np.float32) - w[t, hq].astype(np.float32)).max())
            what = f"no single V row (max |err| {err:.3g})"
        lines.append(f"  request {b} row {t - case.seq_starts[b]} (pos {case.start_pos[b] + t - case.seq_starts[b]}) head {hq}: "
                     f"expected key {int(top[t, hq])}, got {what}")
    return "\n".join(lines)


# -------------------------------------------------------------------------------------------------------------------------------------
# F2: sharp but unsaturated
# -------------------------------------------------------------------------------------------------------------------------------------
def f2(case, family):
    """fill case with an F2 family ('compete', 'sink', 'rising'); one direction per head; returns case.finish()"""
    rng, D, grp = case.rng, case.D, case.grp
    Hd = hadamard(D)
    case.family = family
    for b in range(case.B):
        n = int(case.kvlen[b])
        s0, S = int(case.start_pos[b]), int(case.seqlens[b])
        sig = np.zeros((grp, n), dtype=np.float64)
        spec = set()
        chunks = case.decode_chunks(b) if (b < case.nb and case.split > 1) else ()
        if b >= case.nb and case.p32_split > 1:
            chunks = [c for i in range(0, S, 128) for c in p32_chunks(s0, S, i, case.p32_split)]
        edges = edge_positions(n, case.edge_strides(), chunks, rng, deep=False)
        diag = sorted({s0, s0 + S // 2, n - 1}) if b >= case.nb else [n - 1]   # rows that get a competing key on their own diagonal
        for gi in range(grp):
            if family == "compete":
                sig[gi] = -math.log(n) + 0.5 + 0.3 * rng.randn(n)
                picks = [0] + [edges[(gi * 5 + k * 3 + b) % len(edges)] for k in range(3)]
                offs = rng.permutation([0.0, -0.6, -1.4, -2.5])
                for p, o in zip(picks, offs):
                    sig[gi, p] = 2.0 + o
                    spec.add(p)
                for p in diag:
                    sig[gi, p] = 1.2 + 0.3 * rng.randn()
                    spec.add(p)
            elif family == "sink":
                sig[gi] = 0.5 * rng.randn(n)
                sig[gi, 0] = math.log(max(n - 1, 1))
                spec.add(0)
                for p in diag:
                    sig[gi, p] = math.log(max(n - 1, 1)) - 1.0
                    spec.add(p)
            else:   # rising: a level 8 units up per 64-key tile and a 2-unit ramp inside it -- the first key of a tile already
                j = np.arange(n)   # beats everything before it by ~6, so every tile, a partial last one included, raises the maximum
                sig[gi] = RISE_STEP * (j // P3_BN) + RISE_RAMP * (j % P3_BN) / P3_BN + 0.05 * rng.randn(n)
                spec.update(p for p in edges if p % P3_BN in (0, P3_BN - 1))
        ds = [dirs_of(case, gi)[b % (D // grp)] for gi in range(grp)]
        for hk in range(case.Hkv):
            case.K[b][hk] = (sig.T @ Hd[ds] / math.sqrt(D)).astype(np.float32)
        # V: |V| <= 3 with a non-zero mean; int8 / int4: odd groups smaller (different scales)
        f = _group_factor(case)
        V = np.clip(0.8 + 0.9 * rng.randn(case.Hkv, n, D), -3, 3) * f
        for p in spec:
            V[:, p] = np.clip(-1.0 + 1.2 * rng.randn(case.Hkv, D), -3, 3) * f
        case.V[b][:] = V.astype(np.float32)
        case.special[b] = sorted(spec)
        for i in range(S):
            t, _ = case.row_of(b, i)
            for hq in range(case.H):
                case.Q[t, hq] = Hd[ds[hq % grp]]
    case.finish()
    if family == "rising":
        check_rising(case)
    return case


def check_rising(case):
    """the family's defining property on the dequantised slab: for every request and head, each 64-key tile (a partial last one
    included) raises the running maximum of the scores by >= RISE_MIN"""
    for b in range(case.B):
        n = int(case.kvlen[b])
        r0 = int(case.seq_starts[b])
        for hq in range(case.H):
            hk = hq // case.grp
            sc = case.Kd[b][hk].astype(np.float64) @ case.qkv[r0, hq * case.D:(hq + 1) * case.D].astype(np.float64) / math.sqrt(case.D)
            tmax = np.array([sc[t:t + P3_BN].max() for t in range(0, n, P3_BN)])
            rise = tmax[1:] - np.maximum.accumulate(tmax)[:-1]
            assert len(rise) == 0 or rise.min() >= RISE_MIN, \
                f"{case.name}: request {b} head {hq}: tile {int(rise.argmin()) + 1} raises the maximum by {rise.min():.2f} < {RISE_MIN}"


# -------------------------------------------------------------------------------------------------------------------------------------
# the float64 reference and its mutations
# -------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ["scale*1.01", "scale*0.99", "drop_last", "drop_first", "future_key", "slot+1@edge", "slot-1@edge", "page_swap",
           "wrong_kv_head", "v_scale", "split_drop", "split_nomax", "nibble_order", "bias8"]
# the last two are int4's own: low and high nibble swapped in K and V; the + 8 of the stored nibble not taken out of K's score and
# out of V.  (v_scale under int4: every 32-channel group takes its neighbour's scale; not at head_dim 32, which has one group.)
# what each family is built to catch.  'rising' puts nearly all the mass on the newest tile by design (check_rising: every tile lifts
# the maximum by >= 5, which drives the rescale and the split merges); the scores inside that tile span only 2 units, so a 1 %
# scale error moves the output little, and key 0 and the edge slots far behind carry no weight.
APPLIES = {"compete": set(MUTANTS), "sink": set(MUTANTS),
           "rising": {"drop_last", "future_key", "page_swap", "wrong_kv_head", "v_scale", "split_drop", "split_nomax"}}


def _softmax_out(s, V, chunks=None, mut=None):
    """s [rows, keys] scores (-inf: masked), V [keys, D] -> [rows, D]; chunks: key ranges merged like the split kernels"""
    if not chunks:
        m = s.max(-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        p = np.exp(s - m)
        return (p @ V) / np.maximum(p.sum(-1, keepdims=True), 1e-300)   # (a row that sees no key: 0)
    parts = []
    for k, (beg, end) in enumerate(chunks):
        if mut == "split_drop" and k == len(chunks) - 1:   # the split holding the newest keys
            continue
        ss = s[:, beg:end]
        m = ss.max(-1, keepdims=True)
        ok = np.isfinite(m)
        m = np.where(ok, m, 0.0)
        p = np.exp(ss - m)
        parts.append((m, p.sum(-1, keepdims=True), p @ V[beg:end], ok))
    mm = np.max([np.where(ok, m, -np.inf) for m, _, _, ok in parts], axis=0)
    num = 0.0
    den = 0.0
    for m, l, o, ok in parts:
        w = np.where(ok, 1.0 if mut == "split_nomax" else np.exp(m - mm), 0.0)
        num = num + o * w
        den = den + l * w
    return num / np.maximum(den, 1e-300)


def ref64(case, mut=None, edge=None):
    """float64 attention over the slab as the kernels should read it; `mut` (one of MUTANTS) reads it wrongly, `edge` the key the
    slot mutants move.  Returns None when the mutation does not apply to this case."""
    D, H, grp = case.D, case.H, case.grp
    sm = 1.0 / math.sqrt(D) * (1.01 if mut == "scale*1.01" else 0.99 if mut == "scale*0.99" else 1.0)
    if mut == "wrong_kv_head" and case.Hkv == 1:
        return None
    if mut == "page_swap" and case.mode == 0:
        return None
    if mut == "v_scale" and (case.fmt == "f16" or (case.fmt == "i4" and D == I4.GROUP)):
        return None
    if mut in ("nibble_order", "bias8") and case.fmt != "i4":
        return None
    i4_mut = mut if mut in ("nibble_order", "bias8") else None
    if mut in ("split_drop", "split_nomax") and not any(case.chunks(b, 0) and len(case.chunks(b, 0)) > 1 for b in range(case.B)):
        return None
    q = case.qkv[:, :H * D].astype(np.float64).reshape(case.T, H, D)
    out = np.zeros((case.T, H, D))
    for b in range(case.B):
        s0, S, n = int(case.start_pos[b]), int(case.seqlens[b]), int(case.kvlen[b])
        r0 = int(case.seq_starts[b])
        nk = n + 1                                               # one key past the request: the future-key mutant's
        pos = np.arange(nk)
        if case.mode == 0:
            sl = case.cache_idx[b] + pos
        else:
            pg = np.minimum(pos // case.page_size, case.max_pages - 1)
            pages = case.cache_idx[b].copy()
            if mut == "page_swap":   # the entry of the page holding key 0 swapped with the next request's (or a spare page)
                pages[0] = case.cache_idx[(b + 1) % case.B, 0] if case.B > 1 else case.spare_page
            sl = pages[pg] * case.page_size + pos % case.page_size
        if mut in ("slot+1@edge", "slot-1@edge") and edge is not None and edge < n:
            sl = sl.copy()
            sl[edge] = max(0, min(case.N - 1, sl[edge] + (1 if mut == "slot+1@edge" else -1)))
        for hk in range(case.Hkv):
            hr = (hk + 1) % case.Hkv if mut == "wrong_kv_head" else hk
            K = case.read(0, hr, sl, i4_mut=i4_mut)
            V = case.read(1, hr, sl, scale_from=0 if (mut == "v_scale" and case.fmt == "f8") else None,
                          group_shift=(mut == "v_scale" and case.fmt in ("i8", "i4")), i4_mut=i4_mut)
            rows = np.arange(S)
            vis_hi = s0 + rows + (1 if mut == "future_key" else 0)            # last visible key
            kk = np.arange(nk)[None, :]
            mask = kk <= vis_hi[:, None]
            if mut == "drop_last":
                mask &= kk != (s0 + rows)[:, None]
            if mut == "drop_first":
                mask &= kk != 0
            for g in range(grp):
                hq = hk * grp + g
                s = (q[r0:r0 + S, hq] @ K.T) * sm
                s = np.where(mask, s, -np.inf)
                ch = case.chunks(b, 0)
                if ch and b < case.nb:    # the key past the request (future-key mutant) falls into the last split
                    ch = ch[:-1] + [(ch[-1][0], nk)]
                if ch and b >= case.nb:    # split-KV prefill: the chunks depend on the row's query block
                    res = np.zeros((S, D))
                    for i0 in range(0, S, 128):
                        i1 = min(S, i0 + 128)
                        res[i0:i1] = _softmax_out(s[i0:i1], V, case.chunks(b, i0), mut)
                    out[r0:r0 + S, hq] = res
                else:
                    out[r0:r0 + S, hq] = _softmax_out(s, V, ch, mut)
    return out.reshape(case.T, H * D)


def bar_of(case, out_ref):
    """the GPU test's bar per element: decode rel 1.5e-3 + abs 1.5e-3, prefill rel 1e-3 + abs 1e-3 |V|max (tests/test_gpu_ops.py)"""
    bar = np.empty_like(out_ref)
    nbr = int(case.seq_starts[case.nb])
    bar[:nbr] = 1.5e-3 + 1.5e-3 * np.abs(out_ref[:nbr])
    vmax = max(float(np.abs(v).max()) for v in case.Vd)
    bar[nbr:] = 1e-3 * vmax + 1e-3 * np.abs(out_ref[nbr:])
    return bar


def teeth(case, want=None):
    """{mutant: max |mutant - ref64| / bar} over the case (None: does not apply).  Slot mutants: the smallest over the edges used."""
    if want is None:
        want = ref64(case)
    bar = bar_of(case, want)
    res = {}
    for mname in MUTANTS:
        if mname.startswith("slot"):
            edges = sorted(set(p for b in range(case.B) for p in case.special.get(b, ())))
            vals = []
            for e in edges:
                got = ref64(case, mname, edge=e)
                vals.append(float((np.abs(got - want) / bar).max()))
            res[mname] = min(vals) if vals else None
            continue
        got = ref64(case, mname)
        res[mname] = None if got is None else float((np.abs(got - want) / bar).max())
    return res


# -------------------------------------------------------------------------------------------------------------------------------------
# the cases the CPU spec and the GPU test share (a case is built from its spec on demand: building is the costly part)
# -------------------------------------------------------------------------------------------------------------------------------------
LAYOUT_MODES = [(3, 1), (0, 0), (1, 1), (2, 0), (3, 0)]
DEC_KV = [1, 2, 17, 64, 65, 700, 2049, 2049, 8192, 8192, 8192, 8192]        # decode kv lengths (the current token included)
ODD_KV = [1, 2, 17, 64, 65, 300, 700, 700]                                  # ... of the specs on odd page sizes


def f1_decode_specs():
    """multi-head decode kernel (group 1 and 2) and the grouped-query kernel in both block forms"""
    specs = []
    k = 0
    for fmt in ("f16", "i8", "f8"):
        for H, Hkv, D in ((4, 4, 32), (4, 4, 64), (4, 4, 128), (8, 4, 128)):
            for split in (1, 3, 8):
                layout, mode = LAYOUT_MODES[k % len(LAYOUT_MODES)]
                ps = 64 if k % 3 == 2 else 16
                specs.append(dict(name=f"dec_{fmt}_{H}x{Hkv}x{D}_s{split}_l{layout}m{mode}p{ps}", fmt=fmt, H=H, Hkv=Hkv, D=D,
                                  seqlens=[1] * len(DEC_KV), start_pos=[n - 1 for n in DEC_KV], nb=len(DEC_KV), layout=layout,
                                  mode=mode, page_size=ps, split=split, seed=k))
                k += 1
        # grouped-query kernel: groups 4 / 6 / 8 / 16, big blocks (few requests) with splits 1 and 3
        for H, Hkv, D in ((8, 2, 128), (12, 2, 64), (8, 1, 128), (16, 1, 64)) + (((8, 2, 32),) if fmt == "f16" else ()):
            for split in (1, 3):
                layout, mode = LAYOUT_MODES[k % len(LAYOUT_MODES)]
                specs.append(dict(name=f"gqa_{fmt}_{H}x{Hkv}x{D}_s{split}_l{layout}m{mode}", fmt=fmt, H=H, Hkv=Hkv, D=D,
                                  seqlens=[1] * len(DEC_KV), start_pos=[n - 1 for n in DEC_KV], nb=len(DEC_KV), layout=layout,
                                  mode=mode, page_size=16, split=split, seed=k))
                k += 1
        # small blocks: Hkv * requests * split >= 512 (GQ_SMALL_BLOCK_MIN), split 2 so that the reduce kernel runs
        kv = [int(x) for x in np.random.RandomState(7).randint(1, 600, size=128)] + [1100, 2049]
        specs.append(dict(name=f"gqa_small_{fmt}", fmt=fmt, H=16, Hkv=2, D=128 if fmt != "f16" else 64, seqlens=[1] * len(kv),
                          start_pos=[n - 1 for n in kv], nb=len(kv), layout=3, mode=1, page_size=16, split=2, seed=k))
        k += 1
    # page sizes off the usual 16 / 64 (the addressing branches of the kernels): multi-head decode on pages of 2 (page ids no longer
    # held in a lane register: page_shift < 2) and of 12 (page_shift -1: the division path), grouped-query decode on pages of 8 and 12
    # (rows of a 16-key sub-tile no longer consecutive slots: every row through the page table)
    for fmt in ("f16", "i8", "f8"):
        for tag, H, Hkv, ps, split, kv in (("dec", 8, 8, 2, 1, ODD_KV), ("dec", 8, 8, 12, 3, ODD_KV),
                                           ("gqa", 8, 1, 8, 2, ODD_KV + [1100]), ("gqa", 8, 2, 12, 1, ODD_KV)):
            specs.append(dict(name=f"{tag}_{fmt}_{H}x{Hkv}x128_s{split}_l3m1p{ps}", fmt=fmt, H=H, Hkv=Hkv, D=128, seqlens=[1] * len(kv),
                              start_pos=[n - 1 for n in kv], nb=len(kv), layout=3, mode=1, page_size=ps, split=split, seed=k))
            k += 1
    return specs + _f1_decode_specs_i4()


def _f1_decode_specs_i4():
    """the int4 pass, with a counter of its own (the seeds and layouts of the specs above do not move).  int4 reaches the grouped-query
    kernel at head_dim 128 only: groups 6 and 16 at head_dim 64 run the multi-head kernel"""
    specs = []
    k = 200
    common = dict(fmt="i4", seqlens=[1] * len(DEC_KV), start_pos=[n - 1 for n in DEC_KV], nb=len(DEC_KV))
    for H, Hkv, D in ((4, 4, 32), (4, 4, 64), (4, 4, 128), (8, 4, 128)):
        for split in (1, 3, 8):
            layout, mode = LAYOUT_MODES[k % len(LAYOUT_MODES)]
            ps = 64 if k % 3 == 2 else 16
            specs.append(dict(name=f"dec_i4_{H}x{Hkv}x{D}_s{split}_l{layout}m{mode}p{ps}", H=H, Hkv=Hkv, D=D, layout=layout, mode=mode,
                              page_size=ps, split=split, seed=k, **common))
            k += 1
    for H, Hkv, D in ((8, 2, 128), (12, 2, 64), (8, 1, 128), (16, 1, 64)):
        tag = "gqa_i4" if gqa_form("i4", H, Hkv, D) else f"dec_i4_g{H // Hkv}"
        for split in (1, 3):
            layout, mode = LAYOUT_MODES[k % len(LAYOUT_MODES)]
            specs.append(dict(name=f"{tag}_{H}x{Hkv}x{D}_s{split}_l{layout}m{mode}", H=H, Hkv=Hkv, D=D, layout=layout, mode=mode,
                              page_size=16, split=split, seed=k, **common))
            k += 1
    kv = [int(x) for x in np.random.RandomState(7).randint(1, 600, size=128)] + [1100, 2049]
    specs.append(dict(name="gqa_small_i4", fmt="i4", H=16, Hkv=2, D=128, seqlens=[1] * len(kv), start_pos=[n - 1 for n in kv],
                      nb=len(kv), layout=3, mode=1, page_size=16, split=2, seed=k))
    k += 1
    for tag, H, Hkv, ps, split, kv in (("dec", 8, 8, 2, 1, ODD_KV), ("dec", 8, 8, 12, 3, ODD_KV),
                                       ("gqa", 8, 1, 8, 2, ODD_KV + [1100]), ("gqa", 8, 2, 12, 1, ODD_KV)):
        specs.append(dict(name=f"{tag}_i4_{H}x{Hkv}x128_s{split}_l3m1p{ps}", fmt="i4", H=H, Hkv=Hkv, D=128, seqlens=[1] * len(kv),
                          start_pos=[n - 1 for n in kv], nb=len(kv), layout=3, mode=1, page_size=ps, split=split, seed=k))
        k += 1
    return specs


def f1_prefill_specs():
    """16-row prefill (D 32 / 64), 32-row prefill (D 128, 4 and 8 waves, cold and cache-prefill), split-KV (with decode rows ahead)"""
    specs = []
    k = 0
    for fmt in ("f16", "i8", "f8"):
        specs += _f1_prefill_specs_of(fmt, k)
        k += 6
    return specs + _f1_prefill_specs_of("i4", 200)   # int4: a pass of its own, the counter above does not move


def _f1_prefill_specs_of(fmt, k):
    """the nine prefill specs of one format; k: the format's first seed / layout counter"""
    specs = []
    for H, Hkv, D in ((4, 4, 32), (8, 2, 64)):
        layout, mode = LAYOUT_MODES[k % len(LAYOUT_MODES)]
        specs.append(dict(name=f"pf16_{fmt}_{H}x{Hkv}x{D}_l{layout}m{mode}", fmt=fmt, H=H, Hkv=Hkv, D=D, seqlens=[1, 1, 130, 64, 300],
                          start_pos=[40, 5, 0, 64, 1000], nb=2, layout=layout, mode=mode, page_size=16, seed=k))
        k += 1
    # odd page sizes: 5 (the two keys of a staging item no longer share a page) and 12 (no shift addressing)
    for ps in (5, 12):
        specs.append(dict(name=f"pf16_{fmt}_8x2x64_l3m1p{ps}", fmt=fmt, H=8, Hkv=2, D=64, seqlens=[1, 1, 130, 64, 300],
                          start_pos=[40, 5, 0, 64, 500], nb=2, layout=3, mode=1, page_size=ps, seed=k + 10 + ps))
    specs.append(dict(name=f"p32_{fmt}_4x2x128_l3m1p12", fmt=fmt, H=4, Hkv=2, D=128, seqlens=[1, 1, 130, 64, 300],
                      start_pos=[40, 5, 0, 64, 500], nb=2, layout=3, mode=1, page_size=12, seed=k + 30))
    specs.append(dict(name=f"p32w4_{fmt}", fmt=fmt, H=4, Hkv=2, D=128, seqlens=[300, 129, 5, 200], start_pos=[0, 900, 70, 3000],
                      nb=0, layout=3, mode=1, page_size=16, seed=k))
    specs.append(dict(name=f"p32w8_{fmt}", fmt=fmt, H=4, Hkv=1, D=128, seqlens=[1100, 37], start_pos=[0, 2000], nb=0, layout=3,
                      mode=0, seed=k + 1))
    specs.append(dict(name=f"p32split_{fmt}", fmt=fmt, H=2, Hkv=2, D=128, seqlens=[300], start_pos=[1800], nb=0, layout=3,
                      mode=1, page_size=16, seed=k + 2, ws=True))
    specs.append(dict(name=f"p32split_behind_decode_{fmt}", fmt=fmt, H=4, Hkv=2, D=128, seqlens=[1, 1, 1, 100],
                      start_pos=[1500, 1200, 3000, 4000], nb=3, layout=3, mode=1, page_size=16, seed=k + 3, ws=True))
    return specs


F1_CONFIG4 = dict(name="config4_i8", fmt="i8", H=8, Hkv=1, D=128, seqlens=[1] * 256, start_pos=[1999] * 256, nb=256, layout=3,
                  mode=1, page_size=16, L=1, layer=0, seed=44)
F1_CONFIG4_I4 = dict(F1_CONFIG4, name="config4_i4", fmt="i4", seed=244)
# config 2's decode launch: 1024 requests x 32 heads x kv 512-537, int8, 16-token pages shuffled over a ~557k-token slab whose V half
# starts past 2^31 elements (64-bit slot arithmetic); built request by request (f1_stream)
_KV2 = np.random.RandomState(42).randint(512, 538, size=1024)
F1_CONFIG2 = dict(name="config2_i8", fmt="i8", H=32, Hkv=32, D=128, seqlens=[1] * 1024, start_pos=[int(k) - 1 for k in _KV2], nb=1024,
                  layout=3, mode=1, page_size=16, L=1, layer=0, seed=42, stream=True)

# 'rising' runs on fp16 K: its scores reach hundreds of units, which an e4m3 K row (3 mantissa bits) would move by tens
F2_SPECS = [
    ("compete", dict(name="f2_dec_compete_i8_mha", fmt="i8", H=4, Hkv=4, D=128, seqlens=[1] * 3, start_pos=[699, 2047, 4096], nb=3,
                     layout=3, mode=1, split=3, seed=3)),
    ("sink", dict(name="f2_dec_sink_f8_gqa", fmt="f8", H=8, Hkv=1, D=128, seqlens=[1] * 3, start_pos=[1023, 4095, 7999], nb=3,
                  layout=3, mode=1, split=8, seed=3)),
    ("rising", dict(name="f2_dec_rising_f16_g2", fmt="f16", H=4, Hkv=2, D=64, seqlens=[1] * 2, start_pos=[2999, 8191], nb=2, layout=0,
                    mode=0, split=8, seed=3)),
    ("compete", dict(name="f2_pf_compete_i8_splitkv", fmt="i8", H=2, Hkv=2, D=128, seqlens=[300], start_pos=[1800], nb=0, layout=3,
                     mode=1, seed=3, ws=True)),
    ("sink", dict(name="f2_pf_sink_f16_pf16", fmt="f16", H=4, Hkv=2, D=64, seqlens=[1, 200], start_pos=[900, 1000], nb=1, layout=3,
                  mode=0, seed=3)),
    ("rising", dict(name="f2_pf_rising_f16_p32", fmt="f16", H=2, Hkv=1, D=128, seqlens=[1100], start_pos=[0], nb=0, layout=3, mode=1,
                    seed=3)),
    # int4 (K by the product's scale rule): every family on decode and on prefill.  The rising cases keep one head per kv head: a K
    # row is then a single +-1 direction times its score, which 15 levels hold to the scale's 8 bits however large the score
    ("compete", dict(name="f2_dec_compete_i4_mha", fmt="i4", H=4, Hkv=4, D=128, seqlens=[1] * 3, start_pos=[699, 2047, 4096], nb=3,
                     layout=3, mode=1, split=3, seed=3)),
    ("sink", dict(name="f2_dec_sink_i4_gqa", fmt="i4", H=8, Hkv=1, D=128, seqlens=[1] * 3, start_pos=[1023, 4095, 7999], nb=3,
                  layout=3, mode=1, split=8, seed=3)),
    ("compete", dict(name="f2_dec_compete_i4_gqa", fmt="i4", H=8, Hkv=2, D=128, seqlens=[1] * 3, start_pos=[699, 2047, 4096], nb=3,
                     layout=3, mode=1, split=3, seed=3)),
    ("rising", dict(name="f2_dec_rising_i4_mha", fmt="i4", H=2, Hkv=2, D=64, seqlens=[1] * 2, start_pos=[2999, 8191], nb=2, layout=0,
                    mode=0, split=8, seed=3)),
    ("compete", dict(name="f2_pf_compete_i4_splitkv", fmt="i4", H=2, Hkv=2, D=128, seqlens=[300], start_pos=[1800], nb=0, layout=3,
                     mode=1, seed=3, ws=True)),
    ("sink", dict(name="f2_pf_sink_i4_pf16", fmt="i4", H=4, Hkv=2, D=64, seqlens=[1, 200], start_pos=[900, 1000], nb=1, layout=3,
                  mode=0, seed=3)),
    ("rising", dict(name="f2_pf_rising_i4_p32", fmt="i4", H=2, Hkv=2, D=128, seqlens=[1100], start_pos=[0], nb=0, layout=3, mode=1,
                    seed=3)),
]


def make(spec, family=None):
    """Case of a spec; ws=True: the launch gets a split-KV workspace (the number of splits the launcher picks is mirrored)"""
    kw = dict(spec)
    ws = kw.pop("ws", False)
    stream = kw.pop("stream", False)
    c = Case(**kw)
    if ws:
        # decode K-splits would share the workspace with the split-KV partials (pplhip_op_attention): keep its check unambiguous
        assert c.split == 1, "a workspace case runs its decode rows unsplit"
        if c.D == 128:
            c.p32_split = p32_nsplit(c.max_seq_len, c.B - c.nb, c.H, c.max_kv_len)
    c.ws = ws
    if stream:
        return f1_stream(c)
    return f1(c) if family is None else f2(c, family)
