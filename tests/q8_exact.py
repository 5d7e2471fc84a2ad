"""Exact operands for the quantised-activation linears (k_gemm_i8.hip: online_i8i8 and online_f8f8): every kernel instantiation that
launch_linear_i8 / launch_linear_f8 reach checked bit for bit against a plain numpy reference (int64 / float64, independent of
oracle/llama_ref.c), with canaries around the output and poison behind every input.

int8   y = fp16_RNE( (fp32(S) * sx[m]) * fp32(scale[n]) ),  S the exact integer sum; fp32(S) is RNE, both multiplies are fp32 in that
       order, the fp32 output skips the last rounding.  Operand classes:
         full   activation codes in [-127, 127], weight codes in [-128, 127] (some rows hold -128), arbitrary fp32 sx and fp16 scale;
         large  same-sign +-127 runs over >= 3/4 of K in 60 % of the activation and weight rows: |S| > 2^24 in >= 25 % of the outputs.
fp8    y = fp16_RNE( S_real 2^(ex + ew) ), one rounding.  Operands come from exact bands -- low: i 2^-9, |i| <= 15 (every subnormal
       code and the first normals); mid: integers |i| <= 16; high: 32 i, |i| <= 14 (up to +-448) -- so K max|i| max|j| <= 2^24 units
       and every fp32 partial sum is exact in any order.  Power-of-two scales per row; codes from the exhaustive rne_code table of
       tests/f8f8.py; never 0x7F / 0xFF / -0.
SwiGLU gate and up are the values above rounded to fp16, y = silu(g) u in float64, bound E3 of tests/gemm_exact.py (1 fp16 ulp).

Conditions on the inputs (asserted by Case.check_conditions, on the CPU; not tolerances):
  * every non-zero expected output is a normal fp16 number;
  * int8 with arbitrary scales: >= 1 % of the outputs differ between the specified order and (a) S * (sx * scale), (b) a single
    rounding from float64, and on the large-sum cases (c) a sum accumulated in fp32.  (SwiGLU: measured on the fp16 gate / up values,
    the only place where those forms can show under E3.)  fp16 outputs tell (a) and (b) apart only next to an fp16 rounding boundary:
    every eighth weight row (n % 8 == 3) is a +-2^j copy of row 3, and sx[m] -- an arbitrary fp32 number -- is moved by less than
    2^-9 of itself so that the product of row m with those columns lands within an fp32 ulp of such a boundary;
  * fp8: >= 1 % of the outputs differ from the same product with the operands decoded as e5m2.
Guards: y is a view into a canary-filled buffer (canary columns right of the width when ldy > width, canary rows after M, a canary
tail); xq and w sit at the start of allocations whose tails (>= 256 activation rows, >= 384 weight rows, plus one K tile) hold 0x7F
bytes -- an e4m3 NaN and the largest int8 --, sx and scale are followed by NaN.  The kernels clamp out-of-range rows to the last row,
so a read of a tail shows up as NaN or a wrong sum, never as a fault.

The routes: pplhip_op_linear_q8_ex records "kernel=<template<args>> grid= threads= lds= n_tiles= m_tiles=", and its dry run decides
that without a device.  tests/test_q8_exact_spec.py sweeps the dispatch thresholds +-1 through the dry run; the coverage key is the
full kernel instantiation.
"""
import numpy as np

from tests import f8f8 as F
from tests.gemm_exact import (CANARY16, CANARY32, EPI_F16, EPI_F32, EPI_NAMES, EPI_SWIGLU, POISON8, out_width, parse_route,  # noqa: F401
                              ulp16, within_ulp)

FMT_I8, FMT_F8 = 8, 0x108
FMT_NAMES = {FMT_I8: "i8", FMT_F8: "f8"}

# ---------------------------------------------------------------------------------------------------------------
# routes and the sweep: every threshold of launch_linear_q8, +-1
# ---------------------------------------------------------------------------------------------------------------
SWEEP_M = [1, 16, 17, 32, 33, 64, 128, 129, 256, 511, 512, 513, 1024, 4095, 4096, 4097]
SWEEP_N = [4, 12, 60, 124, 132, 1020, 1024, 1028, 1036, 8188, 8192, 8196, 16384, 16388, 22016, 32776]
SWEEP_K = [16, 32, 48, 64, 112, 128, 144, 256, 384, 640, 768, 1376, 4096, 4112, 11008, 49152]
LAYOUTS = ["dense", "ldy4", "misaligned"]     # ldy = width; ldy = width + 4; y 8 bytes off a 16-byte boundary (fp16 / SwiGLU only)

# compiled instantiations that no call reaches at the default switches (a tuning build's PPLHIP_GEMM_I8_PC=3 / PPLHIP_GEMM_I8_256_ST=3
# select them): no exact case runs them.  (pattern over the kernel token, reason)
UNREACHABLE = [
    (r"gemm_i8_pc_kernel<\w+,3,\w+>", "the producer / consumer ring takes 2 or 4 stages; 3 only in a tuning build"),
    (r"gemm_i8_256_kernel<\w+,3>", "the 256 x 256 ring takes 4 stages; 3 only in a tuning build"),
]


def layout_of(layout, N, epi):
    """(ldy, byte offset of y from a 16-byte boundary)"""
    w = out_width(N, epi)
    return (w + 4 if layout == "ldy4" else w), (8 if layout == "misaligned" else 0)


def dry_route(m, fmt, M, N, K, epi, ldy=None, y_addr=1 << 24):
    """(status, route) of a dry run at fake addresses (the dry run never dereferences them)"""
    ldy = out_width(N, epi) if ldy is None else ldy
    return m.linear_q8_route(1 << 20, 1 << 21, 1 << 22, 1 << 23, fmt, M, N, K, y_addr, ldy, epi, dry_run=True)


def coverage_key(route):
    """the full kernel instantiation of a route text"""
    return parse_route(route)[0]["kernel"]


def run_sweep(m):
    """{kernel instantiation: the cheapest [fmt, M, N, K, epi, layout] that reached it}; skips the shapes the launcher refuses"""
    reached = {}
    for fmt in (FMT_I8, FMT_F8):
        for epi in (EPI_F16, EPI_F32, EPI_SWIGLU):
            for layout in LAYOUTS:
                if layout == "misaligned" and epi == EPI_F32:
                    continue
                for K in SWEEP_K:
                    for N in SWEEP_N:
                        ldy, off = layout_of(layout, N, epi)
                        for M in SWEEP_M:
                            rc, route = dry_route(m, fmt, M, N, K, epi, ldy=ldy, y_addr=(1 << 24) + off)
                            assert rc in (0, -2), (fmt, M, N, K, epi, layout, rc)
                            if rc:      # refused (a SwiGLU row stride of N / 2 % 4 != 0): nothing launches
                                assert route == "" and epi == EPI_SWIGLU and ldy % 4, (fmt, M, N, K, epi, layout, route)
                                continue
                            key = coverage_key(route)
                            if key not in reached or M * N * K < reached[key][1] * reached[key][2] * reached[key][3]:
                                reached[key] = [fmt, M, N, K, epi, layout]
    return reached


def compiled_instantiations():
    """every __global__ instantiation launch_linear_q8 can launch (the dispatch of k_gemm_i8.hip)"""
    out = set()
    for e in ("f16", "f32", "swiglu"):
        for f in ("i8", "f8"):
            out.update({f"gemv_i8_kernel<2,{e},4,{f}>", f"gemv_i8_kernel<1,{e},8,{f}>", f"gemv_i8_kernel<1,{e},4,{f}>", f"gemm_i8_wide_kernel<{e},{f}>"})
            out.update({f"gemm_i8_pc_kernel<{e},{st},{f}>" for st in (2, 3, 4)})
        out.update({f"gemm_i8_256_kernel<{e},{st}>" for st in (3, 4)})
    return out


# ---------------------------------------------------------------------------------------------------------------
# fp8 codes
# ---------------------------------------------------------------------------------------------------------------
BANDS = {"l": (2.0 ** -9, 15), "m": (1.0, 16), "h": (32.0, 14)}      # (unit, largest |i|)
_E4M3 = F.e4m3_values()


def band_codes(band):
    """e4m3fn code of every i unit, -imax <= i <= imax (index i + imax), by the exhaustive search of tests/f8f8.py; 0 is +0"""
    unit, imax = BANDS[band]
    codes = np.array([F.rne_code(0.0 if i == 0 else i * unit) for i in range(-imax, imax + 1)], dtype=np.uint8)
    assert (_E4M3[codes] == np.arange(-imax, imax + 1) * unit).all(), band          # every band value IS an e4m3 number
    assert not np.isin(codes, [0x7F, 0xFF, 0x80]).any()
    return codes


def band_magnitude_codes(band):
    """the non-negative code magnitudes that belong to a band"""
    unit, imax = BANDS[band]
    return {int(c) for c in band_codes(band)[imax:]}


def e5m2_values():
    """value of every byte read as e5m2 (inf and NaN codes: nan)"""
    v = np.empty(256)
    for c in range(256):
        s, ex, mt = c >> 7, (c >> 2) & 31, c & 3
        v[c] = np.nan if ex == 31 else (mt / 4.0 * 2.0 ** -14 if ex == 0 else (1 + mt / 4.0) * 2.0 ** (ex - 15))
        if s:
            v[c] = -v[c]
    return v


# ---------------------------------------------------------------------------------------------------------------
# the exact reference
# ---------------------------------------------------------------------------------------------------------------
def exact_sums(a, b):
    """a [M, K] . b [N, K]^T for integer-valued arrays, exact (every partial sum of the float64 product stays below 2^53)"""
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape[1] * float(np.abs(a).max(initial=0)) * float(np.abs(b).max(initial=0)) < 2.0 ** 53
    return np.rint(a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)


def ref_i8(xq, sx, wq, scale):
    """fp32 values (fp32(S) * sx[m]) * fp32(scale[n]) of int8 codes xq [M, K], wq [N, K], fp32 sx, fp16 scale"""
    S = exact_sums(xq, wq)
    assert np.abs(S).max(initial=0) < 2 ** 31
    return (S.astype(np.float32) * np.asarray(sx, dtype=np.float32)[:, None]) * np.asarray(scale, dtype=np.float16).astype(np.float32)[None, :]


def ref_f8(xq, ex, wq, ew):
    """fp32 values S_real 2^(ex[m] + ew[n]) of e4m3 codes (exact: asserted)"""
    vx, vw = _E4M3[xq], _E4M3[wq]
    assert not (np.isnan(vx).any() or np.isnan(vw).any())
    # in units of 2^-18 every product is an integer
    S = exact_sums(vx * 2.0 ** 9, vw * 2.0 ** 9)
    v = S.astype(np.float64) * 2.0 ** -18 * np.ldexp(1.0, np.asarray(ex)[:, None] + np.asarray(ew)[None, :])
    assert (v.astype(np.float32).astype(np.float64) == v).all(), "an fp8 reference value is not an fp32 number"
    return v.astype(np.float32)


def finish(v32, epi):
    """expected output from the fp32 values: fp32 bits, fp16 bits (RNE), or the float64 SwiGLU values of the fp16 gate / up"""
    if epi == EPI_F32:
        return v32
    h = v32.astype(np.float16)
    if epi == EPI_F16:
        return h
    g = h[:, 0::2].astype(np.float64)
    u = h[:, 1::2].astype(np.float64)
    return g / (1.0 + np.exp(-g)) * u


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
PROTO = 3     # weight rows n % 8 == 3 are +-2^j copies of row 3 (int8, fp16 / SwiGLU outputs)


class Case:
    """kind: int8 'full' / 'large'; fp8 two band letters, activations then weights ('ll', 'hh', 'lh', 'mm', 'hl').  zero: a zero
    activation row (sx = 0 for int8, the quantiser's minimum scale 2^-15 for fp8) and a zero weight row.  key: the kernel it must take."""

    def __init__(self, fmt, M, N, K, epi, layout, kind, zero, key):
        self.fmt, self.M, self.N, self.K, self.epi, self.layout, self.kind, self.zero, self.key = fmt, M, N, K, epi, layout, kind, zero, key
        self.width = out_width(N, epi)
        self.ldy, self.y_off_bytes = layout_of(layout, N, epi)
        self.name = f"{FMT_NAMES[fmt]}-{kind}-M{M}-N{N}-K{K}-{EPI_NAMES[epi]}-{layout}" + ("-zero" if zero else "")
        self.built = False
        assert (fmt == FMT_I8) == (kind in ("full", "large")), self.name
        assert not (layout == "misaligned" and epi == EPI_F32), self.name

    # ---- operands ------------------------------------------------------------------------------------------
    def build(self):
        if self.built:
            return self
        M, N, K = self.M, self.N, self.K
        self.zm = M // 3 if self.zero else -1
        self.zn = (N // 2) | 1 if self.zero else -1          # (odd: an up row under SwiGLU; never a copy of row PROTO)
        if self.zn % 8 == PROTO:
            self.zn += 2
        assert self.zn < N
        for attempt in range(64):      # (a handful of int8 outputs can all be insensitive to the order by chance: draw again)
            rng = np.random.RandomState((M * 7919 + N * 31 + K * 3 + self.fmt * 101 + self.epi * 13 + len(self.kind) + ord(self.kind[0])
                                         + attempt * 7777) % (2 ** 31))
            if self.fmt == FMT_F8:
                self._build_f8(rng)
                break
            self._build_i8(rng)
            if (M * N > 4096 and M > 4) or min(v for k, v in self.shares(built=True).items()) >= 0.01:
                break
        self.built = True
        return self

    def _bias_gates(self, xi, wi):
        """SwiGLU: the gate sums are kept away from zero (silu(g) u must be a normal fp16 number): on the even k (every k up to K = 256)
        the activations are non-negative and gate row n carries one sign"""
        K = self.K
        P = np.arange(K) if K <= 256 else np.arange(0, K, 2)
        xi[:, P] = np.abs(xi[:, P])
        g = np.arange(0, self.N, 2)
        sign = np.where((g // 2) % 3 == 1, -1, 1)[:, None]
        wi[np.ix_(g, P)] = np.abs(wi[np.ix_(g, P)]) * sign

    def _build_i8(self, rng):
        M, N, K, epi = self.M, self.N, self.K, self.epi
        x = rng.randint(-127, 128, size=(M, K)).astype(np.int64)
        w = rng.randint(-128, 128, size=(N, K)).astype(np.int64)
        if self.kind == "large":
            assert epi == EPI_F32 and K * 3 // 4 >= 1041, self.name
            p = np.where(rng.rand(K) < 0.5, -1, 1)           # the common sign pattern of the runs
            for arr, R in ((x, M), (w, N)):
                hot = np.flatnonzero(rng.rand(R) < 0.6) if R > 2 else np.arange(R)
                for r in hot:
                    L = rng.randint(K * 3 // 4, K + 1)
                    arr[r, :L] = 127 * p[:L] * (1 if rng.rand() < 0.5 else -1)
        if epi == EPI_SWIGLU:
            w = np.maximum(w, -127)
            self._bias_gates(x, w)
        w[1::(10 if epi == EPI_SWIGLU else 5), rng.randint(0, K, size=max(1, K // 8))] = -128      # rows that hold -128 (SwiGLU: up rows)
        tuned = epi != EPI_F32 and self.kind == "full"
        jn = np.zeros(N, dtype=np.int64)
        if tuned:
            w[PROTO] = np.maximum(w[PROTO], -127)
            cp = np.arange(PROTO + 8, N, 8)
            sg = np.where(rng.rand(len(cp)) < 0.5, -1, 1)
            w[cp] = w[PROTO][None, :] * sg[:, None]
            jn[cp] = rng.randint(-1, 2, size=len(cp))
        if self.zero:
            w[self.zn] = 0
        S = exact_sums(x, w)
        assert np.abs(S).max() < 2 ** 31, self.name
        Sf = S.astype(np.float64)
        # arbitrary scales: fp32 sx with full mantissas, fp16 scales, neither a power of two
        sx = (1.0 + rng.rand(M)) * 2.0 ** rng.randint(0, 2, size=M)
        if self.zero:
            sx[self.zm] = 0.0
        if epi == EPI_SWIGLU:
            gmax = np.abs(Sf[:, 0::2] * sx[:, None]).max(axis=0)
            sx = sx * 2.0 ** np.round(np.log2(6.0 / np.median(gmax[gmax > 0])) + 4)
            sc = self._swiglu_scales(Sf * sx[:, None], lambda n: 0.75 + 0.25 * rng.rand(n), lambda n: 1.0 + 0.25 * rng.rand(n))
            if tuned:
                sc[cp] = sc[PROTO] * 2.0 ** jn[cp]
        else:
            sc = (1.0 + rng.rand(N)) * 2.0 ** (rng.randint(0, 3, size=N) - 9)
            if tuned:
                sc[cp] = sc[PROTO] * 2.0 ** jn[cp]
            v = np.abs(Sf * sx[:, None] * sc[None, :])
            sx = sx * 2.0 ** np.ceil(-13 - np.log2(v[v > 0].min()))          # the smallest non-zero output at 2^-13 .. 2^-12
        self.scale = sc.astype(np.float16)
        assert ((self.scale.astype(np.float64) >= 2.0 ** -14) & (self.scale.astype(np.float64) < 65504)).all(), self.name
        sx = sx.astype(np.float32)
        if tuned:
            sx = self._tune_sx(S[:, PROTO], sx, self.scale[PROTO])
        self.sx = sx
        self.xq, self.wq, self.S = x.astype(np.int8), w.astype(np.int8), S

    def _swiglu_scales(self, v0, gate_f, up_f):
        """per-column factors for v0 = S (row factor): the gates end at |g| <= 6, the smallest non-zero up at >= 2^-6"""
        N = self.N
        a = np.abs(v0)
        big = a.max(axis=0)
        small = np.where(a > 0, a, np.inf).min(axis=0)
        sc = np.ones(N)
        gate = np.arange(N) % 2 == 0
        nz = big > 0
        with np.errstate(divide="ignore"):
            sc[gate & nz] = (6.0 / big * gate_f(N))[gate & nz]
            sc[~gate & nz] = (2.0 ** -6 / small * up_f(N))[~gate & nz]
        return sc

    @staticmethod
    def _tune_sx(Sp, sx, scp):
        """sx[m] moved (by < 2^-9 of itself) so that fp32(Sp[m]) sx[m] scp lands within an fp32 ulp of an fp16 rounding boundary, on the
        candidate where the specified order differs from both wrong forms if one does"""
        S32, S64 = Sp.astype(np.float32)[:, None], Sp.astype(np.float64)[:, None]
        sc32, sc64 = np.float32(scp), float(scp)
        ok = (Sp != 0) & (sx != 0)
        p0 = np.abs(S64[:, 0] * sx.astype(np.float64) * sc64)
        u = ulp16(np.where(ok, p0, 1.0))
        h = (np.floor(np.where(ok, p0, 1.0) / u) + 0.5)[:, None] * u[:, None] + np.arange(-1, 2)[None, :] * u[:, None]      # [M, 3] boundaries
        base = (h / (np.abs(S64) * sc64 + (~ok)[:, None])).astype(np.float32)
        # (bit patterns of positive floats are ordered: +-d ulps)
        cand = np.concatenate([(base.view(np.int32) + np.int32(d)).view(np.float32) for d in range(-4, 5)], axis=1)            # [M, 27]
        spec = ((S32 * cand) * sc32).astype(np.float16)
        order = (S32 * (cand * sc32)).astype(np.float16)
        single = (S64 * cand.astype(np.float64) * sc64).astype(np.float16)
        score = (spec != order).astype(int) + (spec != single)
        best = cand[np.arange(len(Sp)), np.argmax(score, axis=1)]
        out = np.where(ok, best, sx).astype(np.float32)
        assert (np.abs(out.astype(np.float64) - sx) <= np.abs(sx) * 2.0 ** -9).all()
        return out

    def _build_f8(self, rng):
        M, N, K, epi = self.M, self.N, self.K, self.epi
        (ux, ix), (uw, iw) = BANDS[self.kind[0]], BANDS[self.kind[1]]
        assert K * ix * iw <= 1 << 24, self.name
        xi = rng.randint(-ix, ix + 1, size=(M, K)).astype(np.int64)
        wi = rng.randint(-iw, iw + 1, size=(N, K)).astype(np.int64)
        if epi == EPI_SWIGLU:
            self._bias_gates(xi, wi)
        if self.zero:
            xi[self.zm] = 0
            wi[self.zn] = 0
        S = exact_sums(xi, wi)
        unit = ux * uw
        Sf = np.abs(S).astype(np.float64) * unit
        if epi == EPI_SWIGLU:
            rx = rng.randint(0, 2, size=M)
            gmax = (Sf[:, 0::2] * 2.0 ** rx[:, None]).max(axis=0)
            ex = rx + int(np.round(np.log2(6.0 / np.median(gmax[gmax > 0])) + 4))
            sc = self._swiglu_scales(Sf * 2.0 ** ex[:, None], lambda n: 1.0, lambda n: 1.0)
            gate = np.arange(N) % 2 == 0
            ew = np.where(gate, np.floor(np.log2(sc)), np.ceil(np.log2(sc))).astype(np.int64)
        else:
            rx, ew = rng.randint(0, 4, size=M), rng.randint(0, 4, size=N) - 6
            v = Sf * 2.0 ** (rx[:, None] + ew[None, :])
            ex = rx + int(np.ceil(-14 - np.log2(v[v > 0].min())))          # the smallest non-zero output at 2^-14 .. 2^-13
        if self.zero:
            ex[self.zm], ew[self.zn] = -15, -15                            # what the quantisers write for an all-zero row
        assert (ew >= -15).all() and (ew <= 15).all() and (ew[np.arange(N) != self.zn] >= -14).all(), (self.name, ew.min(), ew.max())
        assert (ex >= -126).all() and (ex <= 127).all(), self.name
        self.ex, self.ew = ex.astype(np.int64), ew.astype(np.int64)
        self.sx = np.ldexp(np.float32(1.0), self.ex).astype(np.float32)
        self.scale = np.ldexp(1.0, self.ew).astype(np.float16)              # (2^-15: an fp16 subnormal, exact)
        assert (self.scale.astype(np.float64) == np.ldexp(1.0, self.ew)).all()
        self.xq = band_codes(self.kind[0])[xi + ix]
        self.wq = band_codes(self.kind[1])[wi + iw]
        self.xi, self.wi, self.S = xi, wi, S

    # ---- the exact outputs ---------------------------------------------------------------------------------
    def values(self, built=False):
        """fp32 values before the last rounding"""
        if not built:
            self.build()
        if self.fmt == FMT_I8:
            return ref_i8(self.xq, self.sx, self.wq, self.scale)
        return ref_f8(self.xq, self.ex, self.wq, self.ew)

    def expected(self):
        return finish(self.values(), self.epi)

    def _cmp(self, v32):
        """what a wrong form is compared in: the output, under SwiGLU the fp16 gate / up values"""
        return v32 if self.epi == EPI_F32 else np.asarray(v32, dtype=np.float32).astype(np.float16)

    def shares(self, built=False):
        """{input condition: the share of outputs that tells the wrong form apart}"""
        c = self if built else self.build()
        v = c.values(built=True)
        spec = c._cmp(v)
        bits = np.uint32 if c.epi == EPI_F32 else np.uint16
        out = {}

        def share(other):
            o = np.asarray(other).astype(spec.dtype)
            return float(np.mean((spec.view(bits) != o.view(bits)) | np.isnan(o.astype(np.float64))))
        if c.fmt == FMT_I8:
            S32 = c.S.astype(np.float32)
            sc32 = c.scale.astype(np.float32)
            out["order S*(sx*scale)"] = share(S32 * (c.sx[:, None] * sc32[None, :]))
            f64 = c.S.astype(np.float64) * c.sx.astype(np.float64)[:, None] * c.scale.astype(np.float64)[None, :]
            with np.errstate(over="ignore"):
                out["single rounding from float64"] = share(f64.astype(np.float32) if c.epi == EPI_F32 else f64.astype(np.float16))
            if c.kind == "large":
                acc = np.zeros((c.M, c.N), dtype=np.float32)
                for k0 in range(0, c.K, 512):          # sequential fp32 accumulation over k
                    pr = c.xq[:, None, k0:k0 + 512].astype(np.float32) * c.wq[None, :, k0:k0 + 512].astype(np.float32)
                    acc = np.add.accumulate(np.concatenate([acc[:, :, None], pr], axis=2), axis=2, dtype=np.float32)[:, :, -1]
                out["sum accumulated in fp32"] = share((acc * c.sx[:, None]) * sc32[None, :])
                out["|S| > 2^24"] = float(np.mean(np.abs(c.S) > 2 ** 24))
        else:
            e5 = e5m2_values()
            with np.errstate(invalid="ignore", over="ignore"):
                o = (e5[c.xq] @ e5[c.wq].T) * np.ldexp(1.0, c.ex[:, None] + c.ew[None, :])
                out["operands decoded as e5m2"] = share(o.astype(np.float32))
        return out

    def check_conditions(self):
        """the builder's conditions on the inputs (raises AssertionError); returns shares()"""
        c = self.build()
        v = np.abs(c.values().astype(np.float64))
        nz = v[v > 0]
        assert nz.size and nz.min() >= 2.0 ** -14 and nz.max() < 65504, (c.name, nz.min(), nz.max())
        if c.epi == EPI_SWIGLU:
            y = np.abs(c.expected())
            assert np.isfinite(y).all() and y[y > 0].min() >= 2.0 ** -14 and y.max() < 65504, (c.name, y[y > 0].min(), y.max())
        if c.fmt == FMT_F8:
            assert c.K * np.abs(c.xi).max() * np.abs(c.wi).max() <= 1 << 24, c.name
            assert not np.isin(c.xq, [0x7F, 0xFF, 0x80]).any() and not np.isin(c.wq, [0x7F, 0xFF, 0x80]).any(), c.name
        else:
            assert np.abs(c.S).max() < 2 ** 31 and (c.wq == -128).any() and c.xq.min() >= -127, c.name
            assert not (c.sx.view(np.uint32) & 0x7FFFFF == 0)[c.sx != 0].all(), c.name       # not powers of two
            assert (c.scale.view(np.uint16) & 0x3FF != 0).mean() > 0.5 or c.N < 16, c.name
        sh = c.shares()
        for name, s in sh.items():
            assert s >= (0.25 if name == "|S| > 2^24" else 0.01), (c.name, name, s)
        if c.zero:
            assert (c.values()[c.zm] == 0).all() and (c.values()[:, c.zn] == 0).all()
        return sh


# (fmt, M, N, K, epi, layout, kind, zero, kernel).  First one case per kernel instantiation the sweep reaches -- the cheapest shape of
# the sweep grid that reaches it --, then the edges.
I8, F8 = FMT_I8, FMT_F8
E16, E32, ESW = EPI_F16, EPI_F32, EPI_SWIGLU
CASE_TABLE = [
    # ---- skinny / generic kernel -------------------------------------------------------------------------------------------------
    (I8, 1, 4, 16, E16, "dense", "full", False, "gemv_i8_kernel<1,f16,8,i8>"),            # K = 16: only a quarter of the lanes loads
    (F8, 1, 4, 16, E16, "misaligned", "ll", False, "gemv_i8_kernel<1,f16,8,f8>"),
    (I8, 1, 4, 16, E32, "ldy4", "full", False, "gemv_i8_kernel<1,f32,8,i8>"),
    (F8, 1, 4, 16, E32, "dense", "hh", False, "gemv_i8_kernel<1,f32,8,f8>"),
    (I8, 1, 1024, 16, ESW, "ldy4", "full", False, "gemv_i8_kernel<1,swiglu,8,i8>"),
    (F8, 1, 1024, 16, ESW, "dense", "lh", False, "gemv_i8_kernel<1,swiglu,8,f8>"),
    (I8, 1, 16388, 16, E16, "ldy4", "full", False, "gemv_i8_kernel<1,f16,4,i8>"),         # more than 1024 blocks of 16 weight rows
    (F8, 1, 16388, 16, E16, "dense", "mm", False, "gemv_i8_kernel<1,f16,4,f8>"),
    (I8, 1, 16388, 16, E32, "dense", "full", False, "gemv_i8_kernel<1,f32,4,i8>"),
    (F8, 1, 16388, 16, E32, "ldy4", "hl", False, "gemv_i8_kernel<1,f32,4,f8>"),
    (I8, 1, 22016, 16, ESW, "misaligned", "full", False, "gemv_i8_kernel<1,swiglu,4,i8>"),
    (F8, 1, 22016, 16, ESW, "ldy4", "ll", False, "gemv_i8_kernel<1,swiglu,4,f8>"),
    (I8, 17, 4, 16, E16, "misaligned", "full", False, "gemv_i8_kernel<2,f16,4,i8>"),      # M = 17: the second row tile is nearly empty
    (F8, 17, 4, 16, E16, "ldy4", "hh", False, "gemv_i8_kernel<2,f16,4,f8>"),
    (I8, 17, 4, 16, E32, "dense", "full", False, "gemv_i8_kernel<2,f32,4,i8>"),
    (F8, 17, 4, 16, E32, "ldy4", "lh", False, "gemv_i8_kernel<2,f32,4,f8>"),
    (I8, 17, 1024, 16, ESW, "dense", "full", False, "gemv_i8_kernel<2,swiglu,4,i8>"),
    (F8, 17, 1024, 16, ESW, "misaligned", "mm", False, "gemv_i8_kernel<2,swiglu,4,f8>"),
    # edges: K = 48; K = 64 with 8 waves (seven idle); K = 768 with 4 waves (a slice of 3 loads: the fp8 pair half empty); K = 4112 with 8
    # waves (a slice crosses the 8-load unroll); M = 16 / 17 / 32; N = 12; SwiGLU with ldy > width; the largest swept K
    (I8, 16, 12, 48, E16, "misaligned", "full", False, "gemv_i8_kernel<1,f16,8,i8>"),
    (F8, 16, 12, 48, E16, "ldy4", "hl", False, "gemv_i8_kernel<1,f16,8,f8>"),
    (I8, 16, 60, 64, E32, "ldy4", "full", False, "gemv_i8_kernel<1,f32,8,i8>"),
    (F8, 16, 60, 64, E32, "dense", "mm", False, "gemv_i8_kernel<1,f32,8,f8>"),
    (I8, 17, 124, 768, E16, "ldy4", "full", False, "gemv_i8_kernel<2,f16,4,i8>"),
    (F8, 17, 124, 768, E16, "dense", "lh", False, "gemv_i8_kernel<2,f16,4,f8>"),
    (F8, 16, 16388, 768, E32, "dense", "hh", False, "gemv_i8_kernel<1,f32,4,f8>"),
    (I8, 16, 132, 4112, E16, "dense", "full", True, "gemv_i8_kernel<1,f16,8,i8>"),
    (F8, 16, 132, 4112, E16, "ldy4", "ll", True, "gemv_i8_kernel<1,f16,8,f8>"),
    (I8, 32, 1032, 256, ESW, "ldy4", "full", True, "gemv_i8_kernel<2,swiglu,4,i8>"),
    (F8, 32, 1032, 256, ESW, "ldy4", "hh", True, "gemv_i8_kernel<2,swiglu,4,f8>"),
    (I8, 17, 12, 49152, E32, "ldy4", "large", False, "gemv_i8_kernel<2,f32,4,i8>"),       # |S| up to 2^29.6
    (F8, 16, 12, 49152, E16, "dense", "lh", False, "gemv_i8_kernel<1,f16,8,f8>"),
    # ---- 128 x 128 producer / consumer blocks ------------------------------------------------------------------------------------
    (I8, 33, 4, 128, E16, "ldy4", "full", False, "gemm_i8_pc_kernel<f16,4,i8>"),          # one K tile in a 4-stage ring; M = 33: 95 repeated rows
    (F8, 33, 4, 128, E16, "dense", "hl", False, "gemm_i8_pc_kernel<f16,4,f8>"),
    (I8, 33, 4, 128, E32, "dense", "full", False, "gemm_i8_pc_kernel<f32,4,i8>"),
    (F8, 33, 4, 128, E32, "ldy4", "ll", False, "gemm_i8_pc_kernel<f32,4,f8>"),
    (I8, 33, 1024, 128, ESW, "misaligned", "full", False, "gemm_i8_pc_kernel<swiglu,4,i8>"),
    (F8, 33, 1024, 128, ESW, "dense", "hh", False, "gemm_i8_pc_kernel<swiglu,4,f8>"),
    (I8, 33, 32776, 128, E16, "ldy4", "full", False, "gemm_i8_pc_kernel<f16,2,i8>"),      # more than 256 tiles: two stages
    (F8, 33, 32776, 128, E16, "dense", "ll", False, "gemm_i8_pc_kernel<f16,2,f8>"),
    (I8, 33, 32776, 128, E32, "dense", "full", False, "gemm_i8_pc_kernel<f32,2,i8>"),
    (F8, 33, 32776, 128, E32, "ldy4", "hh", False, "gemm_i8_pc_kernel<f32,2,f8>"),
    (I8, 33, 32776, 128, ESW, "misaligned", "full", False, "gemm_i8_pc_kernel<swiglu,2,i8>"),
    (F8, 33, 32776, 128, ESW, "ldy4", "lh", False, "gemm_i8_pc_kernel<swiglu,2,f8>"),
    # edges: N = 132 / 1036 (4 / 12 valid columns in the last weight tile), M = 129 (127 repeated rows), 3 tiles in a 4-stage ring, 5
    # tiles (the ring wraps), SwiGLU with ldy > width, 3 tiles through two stages, large sums
    (I8, 33, 132, 128, E16, "misaligned", "full", True, "gemm_i8_pc_kernel<f16,4,i8>"),
    (F8, 33, 132, 128, E16, "ldy4", "lh", True, "gemm_i8_pc_kernel<f16,4,f8>"),
    (I8, 129, 1036, 384, E32, "ldy4", "full", False, "gemm_i8_pc_kernel<f32,4,i8>"),
    (F8, 129, 1036, 384, E32, "dense", "mm", False, "gemm_i8_pc_kernel<f32,4,f8>"),
    (I8, 129, 132, 640, E16, "dense", "full", False, "gemm_i8_pc_kernel<f16,4,i8>"),
    (F8, 129, 132, 640, E16, "misaligned", "hh", False, "gemm_i8_pc_kernel<f16,4,f8>"),
    (I8, 33, 1032, 640, ESW, "ldy4", "full", False, "gemm_i8_pc_kernel<swiglu,4,i8>"),
    (F8, 33, 1032, 640, ESW, "ldy4", "ll", False, "gemm_i8_pc_kernel<swiglu,4,f8>"),
    (I8, 33, 32776, 384, ESW, "ldy4", "full", False, "gemm_i8_pc_kernel<swiglu,2,i8>"),
    (F8, 33, 32776, 384, E16, "dense", "hl", False, "gemm_i8_pc_kernel<f16,2,f8>"),
    (I8, 40, 132, 1664, E32, "dense", "large", False, "gemm_i8_pc_kernel<f32,4,i8>"),     # |S| up to 2^24.7
    # ---- 128 x 384 blocks --------------------------------------------------------------------------------------------------------
    (I8, 512, 22016, 128, E16, "dense", "full", False, "gemm_i8_wide_kernel<f16,i8>"),
    (F8, 512, 22016, 128, E16, "ldy4", "hh", False, "gemm_i8_wide_kernel<f16,f8>"),
    (I8, 512, 22016, 128, E32, "ldy4", "full", False, "gemm_i8_wide_kernel<f32,i8>"),
    (F8, 512, 22016, 128, E32, "dense", "ll", False, "gemm_i8_wide_kernel<f32,f8>"),
    (I8, 512, 22016, 128, ESW, "ldy4", "full", False, "gemm_i8_wide_kernel<swiglu,i8>"),
    (F8, 512, 22016, 128, ESW, "misaligned", "mm", False, "gemm_i8_wide_kernel<swiglu,f8>"),
    # edges: the smallest shape ragged in M and N that takes this form (6 row tiles, the last of 67 rows; 40 weight tiles, the last of
    # 152 rows); 3 tiles through the two stages
    (I8, 707, 15128, 384, E16, "misaligned", "full", True, "gemm_i8_wide_kernel<f16,i8>"),
    (F8, 707, 15128, 128, ESW, "ldy4", "lh", True, "gemm_i8_wide_kernel<swiglu,f8>"),
    # ---- 256 x 256 blocks (int8) -------------------------------------------------------------------------------------------------
    (I8, 4096, 1024, 128, E16, "dense", "full", False, "gemm_i8_256_kernel<f16,4>"),      # two 64-deep tiles in a 4-stage ring
    (I8, 4096, 1024, 128, E32, "ldy4", "full", False, "gemm_i8_256_kernel<f32,4>"),
    (I8, 4096, 1024, 128, ESW, "misaligned", "full", False, "gemm_i8_256_kernel<swiglu,4>"),
    # edges: ragged M and N; 6 tiles (the ring wraps) with SwiGLU and ldy > width
    (I8, 4100, 1092, 128, E16, "ldy4", "full", True, "gemm_i8_256_kernel<f16,4>"),
    (I8, 4100, 1096, 384, ESW, "ldy4", "full", False, "gemm_i8_256_kernel<swiglu,4>"),
]


def all_cases():
    return [Case(*row) for row in CASE_TABLE]


# ---------------------------------------------------------------------------------------------------------------
# the device run (tests/test_gpu_q8_exact.py)
# ---------------------------------------------------------------------------------------------------------------
X_TAIL_ROWS, W_TAIL_ROWS, TAIL_KTILE_BYTES, Y_CANARY_ROWS = 256, 384, 128, 16


def _poisoned(torch, arr, tail_bytes, fill32=None, fill16=None, fill8=None):
    """device bytes: arr at the start of the allocation, tail_bytes of poison after it"""
    b = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    pad = (-b.size) % 4
    t = torch.empty(b.size + pad + tail_bytes, dtype=torch.uint8, device="cuda")
    if fill32 is not None:
        t.view(torch.int32).fill_(fill32)
    elif fill16 is not None:
        t.view(torch.int16).fill_(fill16)
    else:
        t.fill_(fill8)
    t[:b.size].copy_(torch.from_numpy(b.copy()).cuda())
    return t


def run_case_gpu(m, case):
    """runs one case on the device through pplhip_op_linear_q8_ex and returns a list of failures (empty: on its kernel, exact, guarded)"""
    import torch
    c = case.build()
    M, N, K, W, ldy, off = c.M, c.N, c.K, c.width, c.ldy, c.y_off_bytes
    fails = []
    dx = _poisoned(torch, c.xq, X_TAIL_ROWS * K + TAIL_KTILE_BYTES, fill8=POISON8)
    dw = _poisoned(torch, c.wq, W_TAIL_ROWS * K + TAIL_KTILE_BYTES, fill8=POISON8)
    dsx = _poisoned(torch, c.sx, X_TAIL_ROWS * 4, fill32=0x7FC00000)
    dsc = _poisoned(torch, c.scale, W_TAIL_ROWS * 2 + (2 if N % 2 else 0), fill16=0x7E00)
    esz = 4 if c.epi == EPI_F32 else 2
    n_el = (M + Y_CANARY_ROWS) * ldy + 64
    ybuf = torch.empty((n_el + off // esz + 8) * esz // 2, dtype=torch.int16, device="cuda")
    if esz == 4:
        ybuf.view(torch.int32).fill_(CANARY32)
    else:
        ybuf.fill_(CANARY16)
    assert ybuf.data_ptr() % 16 == 0
    yp = ybuf.data_ptr() + off
    torch.cuda.synchronize()
    args = (dx.data_ptr(), dsx.data_ptr(), dw.data_ptr(), dsc.data_ptr(), c.fmt, M, N, K, yp, ldy, c.epi)
    rc_d, r_d = m.linear_q8_route(*args, dry_run=True)
    rc, r_real = m.linear_q8_route(*args, dry_run=False)
    torch.cuda.synchronize()
    if rc_d != 0 or rc != 0:
        return [f"status dry {rc_d} launch {rc}"]
    if coverage_key(r_d) != c.key:
        fails.append(f"dry-run kernel {coverage_key(r_d)!r} != expected {c.key!r}")
    if r_real != r_d:
        fails.append(f"launch route {r_real!r} != dry-run route {r_d!r}")
    raw = ybuf.cpu().numpy().view(np.uint8)
    vals = raw[off:off + n_el * esz].view(np.uint32 if esz == 4 else np.uint16)
    can = CANARY32 if esz == 4 else CANARY16
    if off and not (raw[:off].view(np.uint16) == CANARY16).all():
        fails.append("canary in front of y overwritten")
    inside = np.zeros(vals.size, dtype=bool)
    idx = (np.arange(M)[:, None] * ldy + np.arange(W)[None, :]).reshape(-1)
    inside[idx] = True
    bad = np.nonzero((vals != can) & ~inside)[0]
    if bad.size:
        fails.append(f"{bad.size} canaries overwritten, first at element {bad[0]} (row {bad[0] // ldy}, column {bad[0] % ldy})")
    got = vals[idx].reshape(M, W)
    want = c.expected()
    if c.epi == EPI_SWIGLU:
        ok = within_ulp(got.view(np.float16).astype(np.float64), want)
    else:
        ok = got == want.view(np.uint32 if esz == 4 else np.uint16)
    if not ok.all():
        r, col = np.argwhere(~ok)[0]
        g = got.view(np.float32 if esz == 4 else np.float16)
        fails.append(f"{int((~ok).sum())} of {ok.size} outputs wrong, first [{r}, {col}]: got {g[r, col]!r} want {want[r, col]!r}")
    del dx, dw, dsx, dsc, ybuf
    return fails
