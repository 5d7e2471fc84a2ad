"""Exactly summable operands for the linear layers (k_gemm.hip, k_gemm_wide.hip, k_gemm_pc.hip, k_gemv.hip): every GEMM route of
launch_linear checked bit for bit, with canaries around the output and poison behind every input.

Every operand is an integer multiple of a power-of-two unit, x = i u_x and w_deq = j u_w:
  fp16 weights: integers |j| <= 2047;  W8: codes |j| <= 127 (the row scale is applied after the sum);  W4: (nibble - 8) 2^e[n, g] with
  power-of-two group scales that vary by row and group, u_w = 2^min e.
The builder asserts K max|i| max|j| <= 2^24, so every partial sum -- in any order, with any split -- is exact in fp32 and the integer
sum S (float64 here, exact below 2^53) defines every output bit for bit:
  E1  fp32 output y = S u;  fp16 output y = fp16_RNE(S u)  (fp16 / W4 weights, W8 with power-of-two row scales)
  E2  W8 with arbitrary fp16 row scales: y = fp16(fp32(S u_x) scale[n])  -- two roundings (Numerics); the scales are picked so
      that many outputs differ from the single rounding fp16_RNE(S u_x scale[n])
  E3  fused SwiGLU: gate and up are exact sums rounded to fp16 (after the W8 scale), y = silu(g) u in float64, within 1 fp16 ulp
Guards (a condition, not a tolerance): y is a view with row stride >= width + 8 into a canary-filled buffer with canary rows after M and a
canary tail; x, w and the scales sit at the start of allocations whose tails (>= 256 activation rows, >= 384 weight rows, plus one K tile
of bytes) hold poison -- fp16 NaN, 0x7F bytes for int8 / int4 -- and the workspace is NaN before every call.

The routes: pplhip_op_linear_ex records the kernel a call takes ("kernel=<template<args>> splits= kchunk= reduce= order= ..."), and its
dry run decides that route without a device.  Every case names the route it must take; tests/test_gemm_exact_spec.py sweeps a dense
grid of shapes through the dry run and requires every route it reaches to be among the cases.
"""
import re

import numpy as np

F16_NAN = 0x7E00              # poison behind fp16 inputs
CANARY16 = 0x7D5A             # output canaries (NaN payloads no kernel produces)
CANARY32 = 0x7FA5A5A5
POISON8 = 0x7F                # behind int8 / int4 weights
OP_WS = 64 << 20              # what pplhip_op_linear / _swiglu pass
EPI_F16, EPI_F32, EPI_SWIGLU = 0, 1, 2
EPI_NAMES = {EPI_F16: "f16", EPI_F32: "f32", EPI_SWIGLU: "swiglu"}


def model_ws_bytes(H, Hkv, D, hidden, inter, vocab_local):
    """the split-K workspace a model rank owns (pplhip.cc: 8 * 256 * the widest output * 4 B, at least 96 MiB)"""
    return max(8 * 256 * max(2 * inter, (H + 2 * Hkv) * D, hidden, vocab_local) * 4, 96 << 20)


# the BASELINE configurations' per-rank workspaces: 7B TP 1, 13B TP 2, 70B TP 8
WS_CFG1 = model_ws_bytes(32, 32, 128, 4096, 11008, 32000)
WS_CFG3 = model_ws_bytes(20, 20, 128, 5120, 6912, 16000)
WS_CFG4 = model_ws_bytes(8, 1, 128, 8192, 3584, 4000)
WS_SIZES = {"op": OP_WS, "cfg1": WS_CFG1, "cfg3": WS_CFG3, "cfg4": WS_CFG4, "none": 0}


# ---------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------
def parse_route(text):
    """'a=1 b=2 ; a=3' -> [{'a': '1', 'b': '2'}, {'a': '3'}]"""
    groups = []
    for g in text.split(" ; "):
        d = {}
        for tok in g.split():
            k, _, v = tok.partition("=")
            d[k] = v
        groups.append(d)
    return groups


def coverage_keys(text):
    """one key per launch group: the kernel instantiation plus {split, reduce epilogue, super-tile order, M-split main part} (and the
    256 x 256 kernel's epilogue form)"""
    groups = parse_route(text)
    keys = []
    for gi, g in enumerate(groups):
        order = g.get("order", "plain")
        order = "super" if order.startswith("super") else order
        p = [g["kernel"], "split" if int(g.get("splits", "1")) > 1 else "nosplit", "reduce=" + g.get("reduce", "none"), "order=" + order]
        if "epilogue" in g:
            p.append("epilogue=" + g["epilogue"])
        if len(groups) > 1 and gi == 0:
            p.append("msplit")   # (the rest of an M-split is an ordinary launch of <= 256 rows at offset pointers: its own key)
        keys.append(" ".join(p))
    return keys


def out_width(N, epi):
    return N // 2 if epi == EPI_SWIGLU else N


def dry_route(m, wq, group, M, N, K, epi, ws_bytes, ldy=None, y_addr=1 << 20, x_addr=1 << 21, w_addr=1 << 22, s_addr=1 << 23):
    """(status, route) of a dry run at fake, aligned addresses (the dry run never dereferences them)"""
    ldy = out_width(N, epi) if ldy is None else ldy
    return m.linear_route(x_addr, w_addr, s_addr if wq else None, wq, group, M, N, K, y_addr, ldy, epi,
                          ws=(1 << 24) if ws_bytes else None, ws_bytes=ws_bytes, dry_run=True)


# ---------------------------------------------------------------------------------------------------------------
# the sweep: every threshold of launch_linear and the launchers it calls, +-1
# ---------------------------------------------------------------------------------------------------------------
SWEEP_M = [1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 79, 80, 81, 96, 112, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1040,
           1279, 1280, 1281, 3583, 3584, 4095, 4096, 4097]
SWEEP_N = [4, 12, 60, 68, 124, 132, 252, 260, 380, 388, 1020, 1024, 1028, 8188, 8192, 8196, 22016, 32776]   # (32776: > 256 tiles of 128)
# K: minimums (8 / 16 / 32), non-multiples of 64 and of 128, multiples of 128, W4 K = 64 * 128 and past it, the streaming GEMV's piece
# limits (more than 4 pieces: 8 waves along K; 24 pieces and past them)
SWEEP_K = [8, 16, 32, 64, 96, 128, 192, 1376, 4096, 4112, 4160, 8192, 8320, 12288, 24576, 24592, 49152, 49280]
SWEEP_WQ = [(0, 128), (8, 128), (4, 32), (4, 64), (4, 128)]
SWEEP_WS = ["op", "cfg1", "cfg3", "cfg4", "none"]
SWEEP_LAYOUT = ["dense", "odd_ldy", "misaligned"]     # ldy = width; ldy % 8 == 4; y 8 bytes off a 16-byte boundary


def sweep_layout(layout, N, epi):
    """(ldy, y address) of a sweep layout"""
    w = out_width(N, epi)
    if layout == "dense":
        return w, 1 << 20
    if layout == "odd_ldy":
        return w + 4 if w % 8 == 0 else w, 1 << 20
    return w, (1 << 20) + 8


def run_sweep(m):
    """{coverage key: the cheapest (wq, group, M, N, K, epi, ws, layout) that reached it}; skips the shapes launch_linear refuses"""
    reached = {}
    for wq, group in SWEEP_WQ:
        for K in SWEEP_K:
            if (wq == 0 and K % 8) or (wq == 8 and K % 16) or (wq == 4 and (K % 32 or K % group)):
                continue
            for N in SWEEP_N:
                for epi in (EPI_F16, EPI_F32, EPI_SWIGLU):
                    for M in SWEEP_M:
                        # the workspaces on the dense layout; the layouts with the operators' workspace
                        for wsn, layout in [(w, "dense") for w in SWEEP_WS] + [("op", lay) for lay in SWEEP_LAYOUT[1:]]:
                                ldy, ya = sweep_layout(layout, N, epi)
                                rc, route = dry_route(m, wq, group, M, N, K, epi, WS_SIZES[wsn], ldy=ldy, y_addr=ya)
                                assert rc in (0, -2), (wq, group, M, N, K, epi, wsn, layout, rc)
                                if rc:      # refused (a SwiGLU output of N / 2 % 4 != 0 columns): nothing launches
                                    assert route == "", route
                                    continue
                                for key in coverage_keys(route):
                                    pt = (wq, group, M, N, K, epi, wsn, layout)
                                    # (the cheapest shape that reaches the key)
                                    if key not in reached or M * N * K < reached[key][2] * reached[key][3] * reached[key][4]:
                                        reached[key] = pt
    return reached


# ---------------------------------------------------------------------------------------------------------------
# operands and the exact reference
# ---------------------------------------------------------------------------------------------------------------
def f16_bits(a):
    return np.asarray(a, dtype=np.float16).view(np.uint16)


def sig_bits(S):
    """significant bits of the integers |S| (0 for 0)"""
    a = np.abs(np.asarray(S, dtype=np.int64))
    low = a & -a                                          # lowest set bit (a power of two, exact in float64)
    nz = a != 0
    hi = np.floor(np.log2(np.where(nz, a, 1).astype(np.float64)))
    # (log2 of an int64 near a power of two may round up: correct against the integer itself)
    hi = hi - ((np.int64(1) << hi.astype(np.int64)) > np.where(nz, a, 1))
    return np.where(nz, hi.astype(np.int64) - np.log2(np.where(nz, low, 1).astype(np.float64)).astype(np.int64) + 1, 0)


def ulp16(v):
    """the fp16 spacing at |v| (float64 in, float64 out; 2^-24 in the subnormal range)"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a >= 2.0 ** -14, 2.0 ** (e - 10), 2.0 ** -24)


class Case:
    """One exact case.  wq 0 / 8 / 4 with `group`; epi EPI_F16 / EPI_F32 / EPI_SWIGLU; ws a WS_SIZES key; layout 'dense' (ldy = width + 8),
    'odd_ldy' (ldy % 8 == 4), 'misaligned' (y 8 bytes past a 16-byte boundary); tiny: units that put part of the output in the fp16 subnormal
    range.  Built lazily (build())."""

    def __init__(self, wq, group, M, N, K, epi, ws, layout, route, tiny=False, seed=0):
        self.wq, self.group, self.M, self.N, self.K, self.epi, self.ws, self.layout = wq, group, M, N, K, epi, ws, layout
        self.route, self.tiny, self.seed = route, tiny, seed
        self.family = "E3" if epi == EPI_SWIGLU else ("E2" if wq == 8 and not tiny else "E1")
        self.name = f"{self.family}-w{wq}g{group}-M{M}-N{N}-K{K}-{EPI_NAMES[epi]}-{ws}-{layout}" + ("-tiny" if tiny else "")
        self.width = out_width(N, epi)
        if layout == "odd_ldy":
            self.ldy = self.width + (12 if self.width % 8 == 0 else 8)
        else:
            self.ldy = self.width + 8
        self.y_off_bytes = 8 if layout == "misaligned" else 0
        self.built = False

    # ---- operands ------------------------------------------------------------------------------------------
    def build(self):
        if self.built:
            return self
        wq, M, N, K = self.wq, self.M, self.N, self.K
        for attempt in range(64):   # (a few outputs can all be short sums by chance: draw again)
            rng = np.random.RandomState((self.seed * 1000003 + M * 7919 + N * 31 + K * 3 + wq * 101 + self.epi + attempt * 7777) % (2 ** 31))
            self._draw(rng)
            if np.mean(sig_bits(self.S.astype(np.int64)) > 11) >= 0.5:
                break
        self._units(rng)
        self.built = True
        return self

    def _draw(self, rng):
        wq, M, N, K = self.wq, self.M, self.N, self.K
        budget = (1 << 24) // K
        # weights: integer j and a power-of-two exponent per element (constant per row for fp16 weights, per (row, group) for W4)
        if wq == 0:
            jmax = int(min(2047, max(1, np.sqrt(budget))))
        elif wq == 8:
            jmax = 127
        else:
            jmax = 8
        espread = 0
        if wq == 4:   # group exponents spread over 0..espread, j_eff = (nib - 8) 2^(e - emin): |j_eff| <= 8 2^espread
            espread = int(min(3, max(0, np.floor(np.log2(max(1, budget // 8) / 8.0 + 1e-9))))) if budget >= 16 else 0
        jeff_max = jmax << espread
        imax = int(min(2047, budget // jeff_max))
        assert imax >= 1, (self.name, budget, jeff_max)
        i = rng.randint(-imax, imax + 1, size=(M, K)).astype(np.int64)
        if M >= 8:
            i[M // 3] = 0                                    # an all-zero row
            i[M // 2] = imax                                 # a row at the largest activation magnitude
            sp = np.zeros(K, dtype=np.int64)                 # a sparse row: small sums (subnormal outputs in the tiny cases)
            sp[rng.choice(K, size=min(K, 3), replace=False)] = rng.choice([-1, 1], size=min(K, 3))
            i[M - 2] = sp
        if wq == 0:
            j = rng.randint(-jmax, jmax + 1, size=(N, K)).astype(np.int64)
            ew = np.zeros((N, 1), dtype=np.int64)
        elif wq == 8:
            j = rng.randint(-127, 128, size=(N, K)).astype(np.int64)
            ew = np.zeros((N, 1), dtype=np.int64)
        else:
            G = K // self.group
            nib = rng.randint(0, 16, size=(N, K)).astype(np.int64)
            # (neighbouring groups and rows always differ when espread > 0)
            e = ((rng.randint(0, espread + 1) + np.arange(N)[:, None] + np.arange(G)[None, :]) % (espread + 1)).astype(np.int64)
            j = nib - 8
            ew = np.repeat(e, self.group, axis=1)            # exponent of every element, relative to the unit
            self.nib, self.gexp = nib, e
        jeff = j << ew if wq == 4 else j
        assert K * imax * int(np.abs(jeff).max()) <= 1 << 24, self.name
        S = i.astype(np.float64) @ jeff.astype(np.float64).T   # exact: every partial sum < 2^24 (< 2^53)
        self.i, self.j, self.jeff, self.S = i, j, jeff, S

    def _units(self, rng):
        """power-of-two units (and the W8 scales) that keep every output below 65504 and x / w fp16-exact"""
        wq, N, M = self.wq, self.N, self.M
        smax = max(1.0, float(np.abs(self.S).max()))
        xcap = 2.0 ** np.floor(np.log2(65504.0 / np.abs(self.i).max())) if np.abs(self.i).max() else 1.0   # |x| < 65504
        gate = np.arange(N) % 2 == 0
        cap = np.where(gate, 24.0, 2048.0)     # SwiGLU: |g| <= 24, |u| <= 2048, so |silu(g) u| < 65504
        if wq == 8:
            if self.tiny:        # power-of-two row scales 2^-24 .. 2^-21 (fp16 subnormal scales): sparse rows land in the subnormal range
                ux = 1.0
                sc = 2.0 ** rng.randint(-24, -20, size=N)
            elif self.epi == EPI_SWIGLU:
                # arbitrary scales: gates around |g| ~ 3 (silu neither 0 nor the identity), ups up to ~ 2^10
                ux = min(xcap, 2.0 ** np.floor(np.log2(65504.0 / smax)))
                med = np.maximum(1.0, np.mean(np.abs(self.S), axis=0) * ux)
                tgt = np.where(gate, 3.0, 2.0 ** rng.randint(-2, 10, size=N))
                sc = np.minimum(tgt / med, 2.0 ** -1)
                sc = np.maximum(np.minimum(sc, cap / np.maximum(1.0, np.abs(self.S).max(axis=0) * ux)), 2.0 ** -14)
                sc = sc.astype(np.float16).astype(np.float64)
            else:
                # E2: scales in [2^-12, 2^-10) picked so that output (n % M, n) rounds differently twice than once where one can
                ux = min(xcap, 2.0 ** np.floor(np.log2(65504.0 / (smax * 2.0 ** -10))))
                sc = self._pick_double_rounding_scales(ux, rng)
            self.ux = ux
            self.scale = sc.astype(np.float16)
            self.rowunit = np.ones(N)
        else:
            if self.tiny:
                ux, uw = 2.0 ** -14, 2.0 ** -14
                rowu = np.full(N, uw)
            elif self.epi == EPI_SWIGLU:
                ux = 2.0 ** -10
                med = np.maximum(1.0, np.mean(np.abs(self.S), axis=0) * ux)
                tgt = np.where(gate, 3.0, 2.0 ** rng.randint(-2, 10, size=N))
                rowu = 2.0 ** np.floor(np.log2(tgt / med))
                rowu = np.minimum(rowu, 2.0 ** np.floor(np.log2(cap / np.maximum(1.0, np.abs(self.S).max(axis=0) * ux))))
                rowu = np.maximum(rowu, 2.0 ** -14)                  # (normal fp16 weights and group scales)
            else:
                u = 2.0 ** np.floor(np.log2(65504.0 / smax))
                ux = min(xcap, u * 2.0 ** 8)
                rowu = np.full(N, u / ux)
            self.ux = ux
            self.rowunit = rowu                                      # 2^emin of row n
            if self.wq == 4:
                self.scale = (rowu[:, None] * 2.0 ** self.gexp).astype(np.float16)
                assert (self.scale.astype(np.float64) == rowu[:, None] * 2.0 ** self.gexp).all(), self.name
            else:
                self.scale = None
        x = self.i * self.ux
        self.x = x.astype(np.float16)
        assert (self.x.astype(np.float64) == x).all(), ("x not fp16-exact", self.name)
        if self.wq == 0:
            w = self.j * self.rowunit[:, None]
            self.w = w.astype(np.float16)
            assert (self.w.astype(np.float64) == w).all(), ("w not fp16-exact", self.name)
        elif self.wq == 8:
            self.w = self.j.astype(np.int8)
        else:
            nb = self.nib.astype(np.uint8)
            self.w = (nb[:, 0::2] | (nb[:, 1::2] << 4)).astype(np.uint8)

    def _pick_double_rounding_scales(self, ux, rng):
        """per weight row n the fp16 scale in [2^-12, 2^-10) that double-rounds the most of outputs (n + r) % M, r < 4 (random among
        equals; a random scale where none does)"""
        cand = np.arange(0x0C00, 0x1400, dtype=np.uint16).view(np.float16)
        c32 = cand.astype(np.float32)[None, None, :]
        c64 = cand.astype(np.float64)[None, None, :]
        R = min(self.M, 4)
        sc = np.empty(self.N)
        for n0 in range(0, self.N, 256):
            n = np.arange(n0, min(self.N, n0 + 256))
            rows = (n[:, None] + np.arange(R)[None, :]) % self.M
            v = (self.S[rows, n[:, None]] * ux)[:, :, None]
            hit = ((v.astype(np.float32) * c32).astype(np.float16) != (v * c64).astype(np.float16)).sum(axis=1)
            sc[n] = cand.astype(np.float64)[np.argmax(hit + rng.rand(*hit.shape), axis=1)]
        return sc

    # ---- the exact outputs ---------------------------------------------------------------------------------
    def values(self, S=None):
        """fp32 value of every sum S (before any fp16 rounding): S u, W8 fp32(S u_x) * scale in fp32"""
        S = self.S if S is None else S
        if self.wq == 8:
            return (S * self.ux).astype(np.float32) * self.scale.astype(np.float32)[None, :]
        v = S * self.ux * self.rowunit[None, :]
        assert (v.astype(np.float32).astype(np.float64) == v).all()
        return v.astype(np.float32)

    def expected(self, v=None):
        """fp16 / fp32 output bits (E1, E2) or float64 SwiGLU values (E3) from fp32 values v"""
        v = self.values() if v is None else v
        if self.epi == EPI_F32:
            return v
        h = v.astype(np.float16)
        if self.epi == EPI_F16:
            return h
        g = h[:, 0::2].astype(np.float64)
        u = h[:, 1::2].astype(np.float64)
        return g / (1.0 + np.exp(-g)) * u

    def check_assertions(self):
        """the builder's conditions on the inputs (raises AssertionError)"""
        self.build()
        assert self.K * np.abs(self.i).max() * np.abs(self.jeff).max() <= 1 << 24, self.name
        v = self.values().astype(np.float64)
        assert np.abs(v).max() < 65504, (self.name, np.abs(v).max())
        if self.epi == EPI_SWIGLU:
            g = v[:, 0::2].astype(np.float16).astype(np.float64)
            assert np.mean(np.abs(g) <= 8) >= 0.5, (self.name, "gates", np.mean(np.abs(g) <= 8))
            assert np.abs(self.expected()).max() < 65504, self.name
        # at least half the outputs need more than 11 significant bits: rounding a partial sum to fp16 loses something
        assert np.mean(sig_bits(self.S.astype(np.int64)) > 11) >= 0.5, (self.name, np.mean(sig_bits(self.S.astype(np.int64)) > 11))

    def double_roundings(self):
        """E2, fp16 epilogue: outputs where fp16(fp32(S u_x) scale) != fp16_RNE(S u_x scale)"""
        if self.family != "E2" or self.epi != EPI_F16:
            return 0
        two = self.expected()
        one = (self.S * self.ux * self.scale.astype(np.float64)[None, :]).astype(np.float16)
        return int((two.view(np.uint16) != one.view(np.uint16)).sum())


# ---------------------------------------------------------------------------------------------------------------
# mutants: what a subtly wrong kernel would write (host models; the device mutants are in DESIGN.md section 2)
# ---------------------------------------------------------------------------------------------------------------
def _row_groups(case):
    """[(row slice, route group)] -- an M-split runs rows [0, M & ~1023) and the rest as two launches"""
    groups = parse_route(case.route)
    if len(groups) == 1:
        return [(slice(0, case.M), groups[0])]
    m_main = case.M & ~1023
    return [(slice(0, m_main), groups[0]), (slice(m_main, case.M), groups[1])]


def _split_partials(case, sl, g):
    """fp32 values of every split's partial sum for rows sl (W8: before the scale), or None for an unsplit group"""
    if int(g.get("splits", "1")) <= 1:
        return None
    kc = int(g["kchunk"])
    parts = []
    for k0 in range(0, case.K, kc):
        P = case.i[sl, k0:k0 + kc].astype(np.float64) @ case.jeff[:, k0:k0 + kc].astype(np.float64).T
        unit = case.ux if case.wq == 8 else case.ux * case.rowunit[None, :]
        parts.append((P * unit).astype(np.float32))
    return parts


def mutant_outputs(case):
    """{mutant name: output (the form of case.expected())} for every mutant this case is built for"""
    c = case.build()
    out = {}
    K = c.K

    def from_S(S):
        return c.expected(c.values(S))

    def drop(cols):
        return from_S(c.S - c.i[:, cols].astype(np.float64) @ c.jeff[:, cols].astype(np.float64).T)

    out["drop last k"] = drop(slice(K - 1, K))
    out["drop first K tile"] = drop(slice(0, min(64, K)))
    out["drop last K tile"] = drop(slice((K - 1) // 64 * 64, K))
    v = c.values()
    if any(int(g.get("splits", "1")) > 1 for _, g in _row_groups(c)):
        vf16 = v.copy()
        vsc = v.copy()
        for sl, g in _row_groups(c):
            parts = _split_partials(c, sl, g)
            if parts is None:
                continue
            acc = np.zeros_like(parts[0])
            acc2 = np.zeros_like(parts[0])
            for p in parts:
                acc = acc + p.astype(np.float16).astype(np.float32)
                if c.wq == 8:
                    acc2 = acc2 + p * c.scale.astype(np.float32)[None, :]
            vf16[sl] = acc * c.scale.astype(np.float32)[None, :] if c.wq == 8 else acc
            if c.wq == 8:
                vsc[sl] = acc2
        out["split partials rounded to fp16"] = c.expected(vf16)
        if c.wq == 8 and c.family == "E2" and c.epi == EPI_F32:
            out["W8 scale applied per split"] = c.expected(vsc)
    if c.family == "E2" and c.epi == EPI_F16:
        out["single-rounding epilogue"] = (c.S * c.ux * c.scale.astype(np.float64)[None, :]).astype(np.float16)
    if c.wq == 8 and c.N > 1:
        nb = np.arange(c.N) + 1
        nb[-1] = c.N - 2
        out["neighbouring W8 row scale"] = c.expected((c.S * c.ux).astype(np.float32) * c.scale.astype(np.float32)[None, nb])
    if c.wq == 4:
        G = K // c.group
        sc = c.scale.astype(np.float64)
        if G > 1:
            gb = np.arange(G) + 1
            gb[-1] = G - 2
            sc2 = sc[:, gb]
        else:
            nb = np.arange(c.N) + 1
            nb[-1] = c.N - 2
            sc2 = sc[nb]
        wd = (c.j * np.repeat(sc2, c.group, axis=1))
        out["neighbouring W4 group scale"] = c.expected((c.x.astype(np.float64) @ wd.T).astype(np.float32))
    if c.M >= 2:
        t0 = (c.M - 1) // 16 * 16
        S2 = c.S.copy()
        S2[t0:c.M - 1] = c.S[t0 + 1:c.M]
        S2[c.M - 1] = 0
        if t0 == c.M - 1:
            S2[t0 - 1:c.M - 1] = c.S[t0:c.M]
        out["x row m+1 in the last row tile"] = from_S(S2)
    if c.epi == EPI_SWIGLU:
        h = v.astype(np.float16)
        g = h[:, 0::2].astype(np.float64)
        u = h[:, 1::2].astype(np.float64)
        out["gate and up swapped"] = u / (1.0 + np.exp(-u)) * g
        e = c.expected()
        nb = np.arange(e.shape[1]) + 1
        if e.shape[1] > 1:
            nb[-1] = e.shape[1] - 2
            out["neighbouring gate/up pair"] = e[:, nb]
    return out


def differs(case, got, want):
    """True when `got` is wrong against `want` somewhere: any bit (E1 / E2) or beyond 1 fp16 ulp (E3, +-0 equal)"""
    if case.epi == EPI_SWIGLU:
        return bool(np.any(~within_ulp(got, want)))
    g = np.asarray(got)
    w = np.asarray(want)
    bits = np.uint32 if case.epi == EPI_F32 else np.uint16
    return bool(np.any(g.astype(w.dtype).view(bits) != w.view(bits)))


def within_ulp(got, want):
    """E3 bar: |got - want| <= 1 fp16 ulp at want (want float64; +-0 equal; NaN never)"""
    g = np.asarray(got, dtype=np.float64)
    w = np.asarray(want, dtype=np.float64)
    return np.abs(g - w) <= ulp16(w)


def case_dry_route(m, case, y_addr=1 << 20):
    """dry-run route of a case's shape, row stride and output alignment (fake, otherwise aligned addresses)"""
    return dry_route(m, case.wq, case.group, case.M, case.N, case.K, case.epi, WS_SIZES[case.ws], ldy=case.ldy,
                     y_addr=y_addr + case.y_off_bytes)


# ---------------------------------------------------------------------------------------------------------------
# the cases: (wq, group, M, N, K, epi, workspace, layout, tiny, expected route).  One at least for every route the sweep reaches (the
# cheapest shape that reaches it; E2 routes with room for double roundings), plus tiny-unit cases with fp16-subnormal outputs.
# ---------------------------------------------------------------------------------------------------------------
CASE_TABLE = [
    (0, 128, 1, 4, 8, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 1, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,1,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 1, 4, 24576, 0, 'op', 'dense', False, 'kernel=gemv_kernel<0,1,f16,8> splits=1 reduce=none order=plain'),
    (0, 128, 1, 256, 256, 0, 'op', 'dense', True, 'kernel=gemv_stream_kernel<0,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 2, 4, 8, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,2,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 2, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,2,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 3, 4, 8, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,3,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 3, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,3,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 4, 4, 8, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,4,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 4, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,4,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 5, 4, 8, 0, 'op', 'dense', False, 'kernel=gemm_kernel<0,f16> splits=1 reduce=none order=plain'),
    (0, 128, 5, 4, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,3,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 5, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,3,1,64> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=plain'),
    (0, 128, 5, 8196, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,2,1,64> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=plain'),
    (0, 128, 5, 22016, 8, 0, 'none', 'dense', False, 'kernel=gemv_kernel<0,1,f16,4> splits=1 reduce=none order=plain'),
    (0, 128, 5, 32776, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,2,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 64, 256, 512, 0, 'op', 'dense', True, 'kernel=gemm_dma_kernel<0,f16,3,1,64> splits=1 kchunk=512 reduce=none order=plain'),
    (0, 128, 65, 4, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,3,5> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 65, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,3,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=plain'),
    (0, 128, 129, 8196, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,2,1> splits=2 kchunk=2048 reduce=splitk_reduce_kernel<f16> order=plain'),
    (0, 128, 511, 8196, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,2,1> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 1025, 4, 8, 0, 'op', 'dense', False, 'kernel=gemm_kernel<0,f16> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<0,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 1025, 4, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,3,5> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<0,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 1025, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,3,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=plain ; kernel=gemv_stream_kernel<0,1,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 1025, 1028, 8192, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,2,1> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f16> order=plain ; kernel=gemv_stream_kernel<0,1,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 1025, 8188, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,2,1> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<0,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 1030, 512, 192, 0, 'op', 'dense', True, 'kernel=gemm_dma_kernel<0,f16,3,5> splits=1 kchunk=192 reduce=none order=plain ; kernel=gemm_dma_kernel<0,f16,3,1,64> splits=1 kchunk=192 reduce=none order=plain'),
    (0, 128, 3583, 4, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,3,5> splits=1 kchunk=64 reduce=none order=super(7x1)'),
    (0, 128, 3583, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,3,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=super(7x1)'),
    (0, 128, 4097, 132, 8192, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,2,1> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f16> order=super(3x1)'),
    (0, 128, 4097, 1020, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f16,2,1> splits=1 kchunk=64 reduce=none order=super(3x1)'),
    (0, 128, 1, 4, 8, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 1, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,1,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 1, 4, 24576, 1, 'op', 'dense', False, 'kernel=gemv_kernel<0,1,f32,8> splits=1 reduce=none order=plain'),
    (0, 128, 2, 4, 8, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,2,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 2, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,2,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 3, 4, 8, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,3,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 3, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,3,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 4, 4, 8, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,4,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 4, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,4,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 5, 4, 8, 1, 'op', 'dense', False, 'kernel=gemm_kernel<0,f32> splits=1 reduce=none order=plain'),
    (0, 128, 5, 4, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,3,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 5, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,3,1,64> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=plain'),
    (0, 128, 5, 8196, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,2,1,64> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=plain'),
    (0, 128, 5, 22016, 8, 1, 'none', 'dense', False, 'kernel=gemv_kernel<0,1,f32,4> splits=1 reduce=none order=plain'),
    (0, 128, 5, 32776, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,2,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 65, 4, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,3,5> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 65, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,3,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=plain'),
    (0, 128, 129, 8196, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,2,1> splits=2 kchunk=2048 reduce=splitk_reduce_kernel<f32> order=plain'),
    (0, 128, 511, 8196, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,2,1> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 1025, 4, 8, 1, 'op', 'dense', False, 'kernel=gemm_kernel<0,f32> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<0,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 1025, 4, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,3,5> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<0,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 1025, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,3,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=plain ; kernel=gemv_stream_kernel<0,1,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 1025, 1028, 8192, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,2,1> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f32> order=plain ; kernel=gemv_stream_kernel<0,1,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 1025, 8188, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,2,1> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<0,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 3583, 4, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,3,5> splits=1 kchunk=64 reduce=none order=super(7x1)'),
    (0, 128, 3583, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,3,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=super(7x1)'),
    (0, 128, 4097, 132, 8192, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,2,1> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f32> order=super(3x1)'),
    (0, 128, 4097, 1020, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,f32,2,1> splits=1 kchunk=64 reduce=none order=super(3x1)'),
    (0, 128, 1, 1024, 8, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 1, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,1,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 2, 1024, 8, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,2,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 2, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,2,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 3, 1024, 8, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,3,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 3, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,3,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 4, 1024, 8, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,4,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 4, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<0,4,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 5, 1024, 8, 2, 'op', 'dense', False, 'kernel=gemm_kernel<0,swiglu> splits=1 reduce=none order=plain'),
    (0, 128, 5, 1024, 8, 2, 'none', 'dense', False, 'kernel=gemv_kernel<0,1,swiglu,8> splits=1 reduce=none order=plain'),
    (0, 128, 5, 1024, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,3,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 5, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,3,1,64> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (0, 128, 5, 8192, 8192, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,2,1,64> splits=8 kchunk=1024 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (0, 128, 5, 22016, 8, 2, 'none', 'dense', False, 'kernel=gemv_kernel<0,1,swiglu,4> splits=1 reduce=none order=plain'),
    (0, 128, 5, 32776, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,2,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 65, 1024, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,3,5> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 65, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,3,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (0, 128, 129, 8192, 8192, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,2,1> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (0, 128, 513, 8192, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,2,1> splits=1 kchunk=64 reduce=none order=plain'),
    (0, 128, 1025, 1024, 8, 2, 'op', 'dense', False, 'kernel=gemm_kernel<0,swiglu> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<0,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 1025, 1024, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,3,5> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<0,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 1025, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,3,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<swiglu> order=plain ; kernel=gemv_stream_kernel<0,1,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (0, 128, 1025, 8192, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,2,1> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<0,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (0, 128, 3583, 1024, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,3,5> splits=1 kchunk=64 reduce=none order=super(7x1)'),
    (0, 128, 4097, 1024, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<0,swiglu,2,1> splits=1 kchunk=64 reduce=none order=super(3x1)'),
    (4, 32, 1, 4, 32, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 1, 4, 8320, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,1,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 1, 4, 49280, 0, 'op', 'dense', False, 'kernel=gemv_kernel<4,1,f16,8> splits=1 reduce=none order=plain'),
    (4, 32, 2, 4, 32, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,2,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 2, 4, 8320, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,2,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 3, 4, 32, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,3,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 3, 4, 8320, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,3,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 3, 256, 256, 0, 'op', 'dense', True, 'kernel=gemv_stream_kernel<4,3,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 4, 4, 32, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,4,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 4, 4, 8320, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,4,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 5, 4, 32, 0, 'op', 'dense', False, 'kernel=gemm_kernel<4,f16> splits=1 reduce=none order=plain'),
    (4, 32, 5, 22016, 32, 0, 'none', 'dense', False, 'kernel=gemv_kernel<4,1,f16,4> splits=1 reduce=none order=plain'),
    (4, 32, 1025, 4, 32, 0, 'op', 'dense', False, 'kernel=gemm_kernel<4,f16> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<4,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 1, 4, 32, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 1, 4, 8320, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,1,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 1, 4, 49280, 1, 'op', 'dense', False, 'kernel=gemv_kernel<4,1,f32,8> splits=1 reduce=none order=plain'),
    (4, 32, 2, 4, 32, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,2,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 2, 4, 8320, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,2,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 3, 4, 32, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,3,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 3, 4, 8320, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,3,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 4, 4, 32, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,4,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 4, 4, 8320, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,4,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 5, 4, 32, 1, 'op', 'dense', False, 'kernel=gemm_kernel<4,f32> splits=1 reduce=none order=plain'),
    (4, 32, 5, 22016, 32, 1, 'none', 'dense', False, 'kernel=gemv_kernel<4,1,f32,4> splits=1 reduce=none order=plain'),
    (4, 32, 1025, 4, 32, 1, 'op', 'dense', False, 'kernel=gemm_kernel<4,f32> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<4,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 1, 1024, 32, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 1, 1024, 8320, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,1,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 2, 1024, 32, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,2,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 2, 1024, 8320, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,2,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 3, 1024, 32, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,3,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 3, 1024, 8320, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,3,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 4, 1024, 32, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,4,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 32, 4, 1024, 8320, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<4,4,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 32, 5, 1024, 32, 2, 'op', 'dense', False, 'kernel=gemm_kernel<4,swiglu> splits=1 reduce=none order=plain'),
    (4, 32, 5, 1024, 32, 2, 'none', 'dense', False, 'kernel=gemv_kernel<4,1,swiglu,8> splits=1 reduce=none order=plain'),
    (4, 32, 5, 22016, 32, 2, 'none', 'dense', False, 'kernel=gemv_kernel<4,1,swiglu,4> splits=1 reduce=none order=plain'),
    (4, 32, 1025, 1024, 32, 2, 'op', 'dense', False, 'kernel=gemm_kernel<4,swiglu> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<4,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 128, 5, 4, 128, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,4,1,64> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 5, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1,64> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=plain'),
    (4, 128, 5, 32776, 128, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1,64> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 40, 384, 1024, 0, 'op', 'dense', True, 'kernel=gemm_dma_kernel<4,f16,4,1,64> splits=1 kchunk=1024 reduce=none order=plain'),
    (4, 128, 65, 4, 128, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,4,5> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 65, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=plain'),
    (4, 128, 65, 8196, 8320, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1> splits=4 kchunk=2176 reduce=splitk_reduce_kernel<f16> order=plain'),
    (4, 128, 129, 8192, 128, 0, 'op', 'dense', False, 'kernel=gemm_w4_pc_kernel<f16> splits=1 reduce=none order=plain'),
    (4, 128, 129, 8196, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1,128,16> splits=2 kchunk=2048 reduce=splitk_reduce_kernel<f16> order=plain'),
    (4, 128, 511, 8196, 128, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 1025, 4, 128, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,4,5> splits=1 kchunk=128 reduce=none order=plain ; kernel=gemv_stream_kernel<4,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 128, 1025, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=plain ; kernel=gemv_stream_kernel<4,1,f16,4> splits=1 reduce=none order=plain nwk=2 nb=1'),
    (4, 128, 1025, 1028, 8192, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1,128,16> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f16> order=plain ; kernel=gemv_stream_kernel<4,1,f16,4> splits=1 reduce=none order=plain nwk=4 nb=1'),
    (4, 128, 1025, 1028, 8320, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1> splits=4 kchunk=2176 reduce=splitk_reduce_kernel<f16> order=plain ; kernel=gemv_stream_kernel<4,1,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 128, 1025, 8188, 128, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1> splits=1 kchunk=128 reduce=none order=plain ; kernel=gemv_stream_kernel<4,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 128, 3583, 4, 128, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,4,5> splits=1 kchunk=128 reduce=none order=super(7x1)'),
    (4, 128, 3583, 4, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=super(7x1)'),
    (4, 128, 4097, 132, 8192, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1,128,16> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f16> order=super(3x1)'),
    (4, 128, 4097, 132, 8320, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1> splits=4 kchunk=2176 reduce=splitk_reduce_kernel<f16> order=super(3x1)'),
    (4, 128, 4097, 1020, 128, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f16,2,1> splits=1 kchunk=128 reduce=none order=super(3x1)'),
    (4, 128, 5, 4, 128, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,4,1,64> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 5, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1,64> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=plain'),
    (4, 128, 5, 32776, 128, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1,64> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 65, 4, 128, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,4,5> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 65, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=plain'),
    (4, 128, 65, 8196, 8320, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1> splits=4 kchunk=2176 reduce=splitk_reduce_kernel<f32> order=plain'),
    (4, 128, 129, 8196, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1,128,16> splits=2 kchunk=2048 reduce=splitk_reduce_kernel<f32> order=plain'),
    (4, 128, 511, 8196, 128, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 1025, 4, 128, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,4,5> splits=1 kchunk=128 reduce=none order=plain ; kernel=gemv_stream_kernel<4,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 128, 1025, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=plain ; kernel=gemv_stream_kernel<4,1,f32,4> splits=1 reduce=none order=plain nwk=2 nb=1'),
    (4, 128, 1025, 1028, 8192, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1,128,16> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f32> order=plain ; kernel=gemv_stream_kernel<4,1,f32,4> splits=1 reduce=none order=plain nwk=4 nb=1'),
    (4, 128, 1025, 1028, 8320, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1> splits=4 kchunk=2176 reduce=splitk_reduce_kernel<f32> order=plain ; kernel=gemv_stream_kernel<4,1,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 128, 1025, 8188, 128, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1> splits=1 kchunk=128 reduce=none order=plain ; kernel=gemv_stream_kernel<4,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 128, 3583, 4, 128, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,4,5> splits=1 kchunk=128 reduce=none order=super(7x1)'),
    (4, 128, 3583, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=super(7x1)'),
    (4, 128, 4097, 132, 8192, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1,128,16> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f32> order=super(3x1)'),
    (4, 128, 4097, 132, 8320, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1> splits=4 kchunk=2176 reduce=splitk_reduce_kernel<f32> order=super(3x1)'),
    (4, 128, 4097, 1020, 128, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,f32,2,1> splits=1 kchunk=128 reduce=none order=super(3x1)'),
    (4, 128, 5, 1024, 128, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,4,1,64> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 5, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,2,1,64> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (4, 128, 5, 32776, 128, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,2,1,64> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 65, 1024, 128, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,4,5> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 65, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (4, 128, 129, 8192, 128, 2, 'op', 'dense', False, 'kernel=gemm_w4_pc_kernel<swiglu> splits=1 reduce=none order=plain'),
    (4, 128, 129, 8192, 8192, 2, 'op', 'odd_ldy', False, 'kernel=gemm_dma_kernel<4,swiglu,2,1,128,16> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (4, 128, 129, 8192, 8320, 2, 'op', 'odd_ldy', False, 'kernel=gemm_dma_kernel<4,swiglu,2,1> splits=4 kchunk=2176 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (4, 128, 513, 8192, 128, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,2,1> splits=1 kchunk=128 reduce=none order=plain'),
    (4, 128, 1025, 1024, 128, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,4,5> splits=1 kchunk=128 reduce=none order=plain ; kernel=gemv_stream_kernel<4,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 128, 1025, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<swiglu> order=plain ; kernel=gemv_stream_kernel<4,1,swiglu,4> splits=1 reduce=none order=plain nwk=2 nb=1'),
    (4, 128, 1025, 1024, 49152, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,2,1> splits=6 kchunk=8192 reduce=splitk_reduce_kernel<swiglu> order=plain ; kernel=gemv_stream_kernel<4,1,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (4, 128, 1025, 8192, 128, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,2,1> splits=1 kchunk=128 reduce=none order=plain ; kernel=gemv_stream_kernel<4,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (4, 128, 3583, 1024, 128, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,4,5> splits=1 kchunk=128 reduce=none order=super(7x1)'),
    (4, 128, 3583, 1024, 8320, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,2,1> splits=2 kchunk=4224 reduce=splitk_reduce_kernel<swiglu> order=super(7x1)'),
    (4, 128, 4097, 1024, 128, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<4,swiglu,2,1> splits=1 kchunk=128 reduce=none order=super(3x1)'),
    (8, 128, 1, 124, 16, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1, 124, 4112, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,1,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 2, 124, 16, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,2,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 2, 124, 4112, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,2,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 2, 256, 512, 0, 'op', 'dense', True, 'kernel=gemv_stream_kernel<8,2,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 3, 124, 16, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,3,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 3, 124, 128, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,16> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 3, 124, 128, 0, 'none', 'dense', False, 'kernel=gemv_kernel<8,1,f16,8> splits=1 reduce=none order=plain'),
    (8, 128, 3, 124, 4096, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,16> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 3, 124, 4112, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,3,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 4, 124, 16, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,4,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 4, 124, 4112, 0, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,4,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 5, 124, 16, 0, 'op', 'dense', False, 'kernel=gemm_kernel<8,f16> splits=1 reduce=none order=plain'),
    (8, 128, 5, 124, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,4,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 5, 124, 4160, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,4,1,64> splits=4 kchunk=1088 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 5, 8196, 4160, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,2,1,64> splits=4 kchunk=1088 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 5, 22016, 16, 0, 'none', 'dense', False, 'kernel=gemv_kernel<8,1,f16,4> splits=1 reduce=none order=plain'),
    (8, 128, 5, 32776, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,2,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 17, 124, 128, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,32> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 17, 124, 4096, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,32> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 63, 124, 128, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,64> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 63, 124, 4096, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,64> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 63, 32776, 128, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,2,64> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 65, 124, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,4,6> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 65, 124, 128, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,80> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 65, 124, 4096, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,80> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 65, 124, 4160, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,4,5> splits=4 kchunk=1088 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 81, 124, 4096, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,96> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 112, 124, 4096, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,112> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 127, 124, 4096, 0, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f16,3,128> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 129, 8196, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,2,1> splits=2 kchunk=2048 reduce=splitk_reduce_kernel<f16> order=plain'),
    (8, 128, 300, 1024, 1024, 0, 'op', 'dense', True, 'kernel=gemm_dma_kernel<8,f16,4,6> splits=1 kchunk=1024 reduce=none order=plain'),
    (8, 128, 511, 8196, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,2,1> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 512, 22016, 64, 0, 'op', 'dense', False, 'kernel=gemm_w8_wide_kernel<f16,3,12> splits=1 reduce=none order=plain'),
    (8, 128, 1025, 124, 16, 0, 'op', 'dense', False, 'kernel=gemm_kernel<8,f16> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1025, 124, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,4,6> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1025, 124, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=plain ; kernel=gemv_stream_kernel<8,1,f16,4> splits=1 reduce=none order=plain nwk=4 nb=1'),
    (8, 128, 1025, 1028, 8192, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,2,1> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f16> order=plain ; kernel=gemv_stream_kernel<8,1,f16,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 1025, 8188, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,2,1> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1025, 22016, 64, 0, 'op', 'dense', False, 'kernel=gemm_w8_wide_kernel<f16,3,12> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,f16,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 3583, 124, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,4,6> splits=1 kchunk=64 reduce=none order=super(7x1)'),
    (8, 128, 3583, 124, 4096, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f16> order=super(7x1)'),
    (8, 128, 3584, 1024, 64, 0, 'op', 'odd_ldy', False, 'kernel=gemm_w8_dma256_kernel<f16> splits=1 reduce=none order=super(2x1) epilogue=direct'),
    (8, 128, 3584, 1024, 64, 0, 'op', 'dense', False, 'kernel=gemm_w8_dma256_kernel<f16> splits=1 reduce=none order=super(2x1) epilogue=staged'),
    (8, 128, 4097, 132, 8192, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,2,1> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f16> order=super(3x1)'),
    (8, 128, 4097, 1020, 64, 0, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f16,2,1> splits=1 kchunk=64 reduce=none order=super(3x1)'),
    (8, 128, 1, 4, 16, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1, 4, 4112, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,1,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 1, 4, 24592, 1, 'op', 'dense', False, 'kernel=gemv_kernel<8,1,f32,8> splits=1 reduce=none order=plain'),
    (8, 128, 2, 4, 16, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,2,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 2, 4, 4112, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,2,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 3, 4, 16, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,3,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 3, 4, 128, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,16> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 3, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,16> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 3, 4, 4112, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,3,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 4, 4, 16, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,4,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 4, 4, 4112, 1, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,4,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 5, 4, 16, 1, 'op', 'dense', False, 'kernel=gemm_kernel<8,f32> splits=1 reduce=none order=plain'),
    (8, 128, 5, 4, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,4,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 5, 4, 4160, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,4,1,64> splits=4 kchunk=1088 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 5, 8196, 4160, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,2,1,64> splits=4 kchunk=1088 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 5, 22016, 16, 1, 'none', 'dense', False, 'kernel=gemv_kernel<8,1,f32,4> splits=1 reduce=none order=plain'),
    (8, 128, 5, 32776, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,2,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 17, 4, 128, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,32> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 17, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,32> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 63, 4, 128, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,64> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 63, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,64> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 63, 32776, 128, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,2,64> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 65, 4, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,4,6> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 65, 4, 128, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,80> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 65, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,80> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 65, 4, 4160, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,4,5> splits=4 kchunk=1088 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 81, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,96> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 112, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,112> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 127, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<f32,3,128> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 129, 8196, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,2,1> splits=2 kchunk=2048 reduce=splitk_reduce_kernel<f32> order=plain'),
    (8, 128, 511, 8196, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,2,1> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 512, 22016, 64, 1, 'op', 'dense', False, 'kernel=gemm_w8_wide_kernel<f32,3,12> splits=1 reduce=none order=plain'),
    (8, 128, 1025, 4, 16, 1, 'op', 'dense', False, 'kernel=gemm_kernel<8,f32> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1025, 4, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,4,6> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1025, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=plain ; kernel=gemv_stream_kernel<8,1,f32,4> splits=1 reduce=none order=plain nwk=4 nb=1'),
    (8, 128, 1025, 1028, 8192, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,2,1> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f32> order=plain ; kernel=gemv_stream_kernel<8,1,f32,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 1025, 8188, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,2,1> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1025, 22016, 64, 1, 'op', 'dense', False, 'kernel=gemm_w8_wide_kernel<f32,3,12> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,f32,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 3583, 4, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,4,6> splits=1 kchunk=64 reduce=none order=super(7x1)'),
    (8, 128, 3583, 4, 4096, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<f32> order=super(7x1)'),
    (8, 128, 3584, 1024, 64, 1, 'op', 'odd_ldy', False, 'kernel=gemm_w8_dma256_kernel<f32> splits=1 reduce=none order=super(2x1) epilogue=direct'),
    (8, 128, 3584, 1024, 64, 1, 'op', 'dense', False, 'kernel=gemm_w8_dma256_kernel<f32> splits=1 reduce=none order=super(2x1) epilogue=staged'),
    (8, 128, 4097, 132, 8192, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,2,1> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<f32> order=super(3x1)'),
    (8, 128, 4097, 1020, 64, 1, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,f32,2,1> splits=1 kchunk=64 reduce=none order=super(3x1)'),
    (8, 128, 1, 1024, 16, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1, 1024, 4112, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,1,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 2, 1024, 16, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,2,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 2, 1024, 4112, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,2,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 3, 1024, 16, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,3,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 3, 1024, 128, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,16> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 3, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,16> splits=8 kchunk=512 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 3, 1024, 4112, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,3,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 4, 1024, 16, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,4,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 4, 1024, 4112, 2, 'op', 'dense', False, 'kernel=gemv_stream_kernel<8,4,swiglu,8> splits=1 reduce=none order=plain nwk=8 nb=1'),
    (8, 128, 5, 1024, 16, 2, 'op', 'dense', False, 'kernel=gemm_kernel<8,swiglu> splits=1 reduce=none order=plain'),
    (8, 128, 5, 1024, 16, 2, 'none', 'dense', False, 'kernel=gemv_kernel<8,1,swiglu,8> splits=1 reduce=none order=plain'),
    (8, 128, 5, 1024, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,4,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 5, 1024, 4160, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,4,1,64> splits=4 kchunk=1088 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 5, 22016, 16, 2, 'none', 'dense', False, 'kernel=gemv_kernel<8,1,swiglu,4> splits=1 reduce=none order=plain'),
    (8, 128, 5, 22016, 4160, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,2,1,64> splits=4 kchunk=1088 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 5, 32776, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,2,1,64> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 17, 1024, 128, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,32> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 17, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,32> splits=8 kchunk=512 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 63, 1024, 128, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,64> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 63, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,64> splits=8 kchunk=512 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 63, 32776, 128, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,2,64> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 65, 1024, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,4,6> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 65, 1024, 128, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,80> splits=1 kchunk=128 reduce=none order=plain'),
    (8, 128, 65, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,80> splits=8 kchunk=512 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 65, 1024, 4160, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,4,5> splits=4 kchunk=1088 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 81, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,96> splits=8 kchunk=512 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 112, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,112> splits=8 kchunk=512 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 127, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_w8_half128_kernel<swiglu,3,128> splits=8 kchunk=512 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 129, 8192, 8192, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,2,1> splits=4 kchunk=2048 reduce=splitk_reduce_kernel<swiglu> order=plain'),
    (8, 128, 512, 22016, 64, 2, 'op', 'dense', False, 'kernel=gemm_w8_wide_kernel<swiglu,3,12> splits=1 reduce=none order=plain'),
    (8, 128, 513, 8192, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,2,1> splits=1 kchunk=64 reduce=none order=plain'),
    (8, 128, 1025, 1024, 16, 2, 'op', 'dense', False, 'kernel=gemm_kernel<8,swiglu> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1025, 1024, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,4,6> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1025, 1024, 4096, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,4,5> splits=4 kchunk=1024 reduce=splitk_reduce_kernel<swiglu> order=plain ; kernel=gemv_stream_kernel<8,1,swiglu,4> splits=1 reduce=none order=plain nwk=4 nb=1'),
    (8, 128, 1025, 8192, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,2,1> splits=1 kchunk=64 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 1025, 22016, 64, 2, 'op', 'dense', False, 'kernel=gemm_w8_wide_kernel<swiglu,3,12> splits=1 reduce=none order=plain ; kernel=gemv_stream_kernel<8,1,swiglu,4> splits=1 reduce=none order=plain nwk=1 nb=1'),
    (8, 128, 3583, 1024, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,4,6> splits=1 kchunk=64 reduce=none order=super(7x1)'),
    (8, 128, 3583, 8192, 64, 2, 'op', 'dense', False, 'kernel=gemm_dma_kernel<8,swiglu,2,1> splits=1 kchunk=64 reduce=none order=super(7x8)'),
    (8, 128, 3584, 1024, 64, 2, 'op', 'odd_ldy', False, 'kernel=gemm_w8_dma256_kernel<swiglu> splits=1 reduce=none order=super(2x1) epilogue=direct'),
    (8, 128, 3584, 1024, 64, 2, 'op', 'dense', False, 'kernel=gemm_w8_dma256_kernel<swiglu> splits=1 reduce=none order=super(2x1) epilogue=staged'),
]


def all_cases():
    return [Case(*row[:8], route=row[9], tiny=row[8]) for row in CASE_TABLE]


# compiled instantiations that no call reaches with the product defaults (no PPLHIP_* switch set): the sweep asserts that it reaches none
# of them.  (pattern over the kernel token, reason)
UNREACHABLE = [
    (r"gemm_dma_kernel<\d,\w+,2,5>", "the 5-wave layout runs only when tiles x splits <= 256, which always selects the deep ring"),
    (r"gemm_dma_kernel<0,\w+,4,", "fp16 weights never take 4 stages (4 x 32 KiB: lowered to 3)"),
    (r"gemm_dma_kernel<[48],\w+,3,", "int8 and int4 weights take 2 or 4 stages, never 3"),
    (r"gemm_dma_kernel<\d,\w+,[34],1>", "128-row 4-wave tiles run only when tiles x splits > 256, which always selects two stages"),
]


def compiled_instantiations():
    """every __global__ instantiation the linear launchers can launch (the launch macros of k_gemm.hip, k_gemv.hip, k_gemm_wide.hip,
    k_gemm_pc.hip)"""
    E = ["f16", "f32", "swiglu"]
    out = set()
    for wq in (8, 4, 0):
        for M in (1, 2, 3, 4):
            for e in E:
                for nw in (4, 8):
                    out.add(f"gemv_stream_kernel<{wq},{M},{e},{nw}>")
        for e in E:
            for nw in (4, 8):
                out.add(f"gemv_kernel<{wq},1,{e},{nw}>")
        for e in E:
            out.add(f"gemm_kernel<{wq},{e}>")
            for st in (2, 3, 4):
                if wq == 8 and st >= 3:
                    out.add(f"gemm_dma_kernel<8,{e},{st},6>")
                out.add(f"gemm_dma_kernel<{wq},{e},{st},5>")
                out.add(f"gemm_dma_kernel<{wq},{e},{st},1,64>")
                out.add(f"gemm_dma_kernel<{wq},{e},{st},1>")
                if wq == 4 and st == 2:
                    out.add(f"gemm_dma_kernel<4,{e},2,1,128,16>")
    for e in E:
        out.add(f"gemm_w8_wide_kernel<{e},3,12>")
        out.add(f"gemm_w8_dma256_kernel<{e}>")
        for st, bm in ((3, 16), (3, 32), (2, 64), (3, 64), (3, 80), (3, 96), (3, 112), (3, 128)):
            out.add(f"gemm_w8_half128_kernel<{e},{st},{bm}>")
        out.add(f"splitk_reduce_kernel<{e}>")
    out.add("gemm_w4_pc_kernel<f16>")
    out.add("gemm_w4_pc_kernel<swiglu>")
    return out


def reached_instantiations(keys):
    out = set()
    for k in keys:
        tok = k.split()
        out.add(tok[0])
        for t in tok:
            if t.startswith("reduce=splitk"):
                out.add(t[len("reduce="):])
    return out


# ---------------------------------------------------------------------------------------------------------------
# the device run (tests/test_gpu_gemm_exact.py and its child processes)
# ---------------------------------------------------------------------------------------------------------------
X_TAIL_ROWS, W_TAIL_ROWS, TAIL_KTILE_BYTES, Y_CANARY_ROWS = 256, 384, 128, 16


def _poisoned(torch, arr, tail_bytes, fill16=None, fill8=None):
    """device bytes: arr at the start of the allocation, tail_bytes of poison after it (fp16 pattern fill16, or the byte fill8)"""
    b = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    t = torch.empty(b.size + tail_bytes, dtype=torch.uint8, device="cuda")
    if fill16 is not None:
        t.view(torch.int16).fill_(fill16)
    else:
        t.fill_(fill8)
    t[:b.size].copy_(torch.from_numpy(b.copy()).cuda())
    return t


def run_case_gpu(m, case, expect_route=None, via_op=False):
    """runs one case on the device (pplhip_op_linear_ex; via_op: pplhip_op_linear / _swiglu with ldy = N and its own workspace) and returns
    a list of failures (empty: exact, guarded, on the expected route)"""
    import torch
    c = case.build()
    M, N, K, W = c.M, c.N, c.K, c.width
    expect_route = c.route if expect_route is None else expect_route
    fails = []
    dx = _poisoned(torch, c.x, X_TAIL_ROWS * K * 2 + TAIL_KTILE_BYTES, fill16=F16_NAN)
    wtail = W_TAIL_ROWS * K * (2 if c.wq == 0 else 1) // (2 if c.wq == 4 else 1) + TAIL_KTILE_BYTES
    if c.wq == 0:
        dw = _poisoned(torch, c.w, wtail, fill16=F16_NAN)
    else:
        dw = _poisoned(torch, c.w, wtail, fill8=POISON8)
    ds = None
    if c.scale is not None:
        per_row = 1 if c.wq == 8 else K // c.group
        ds = _poisoned(torch, c.scale, (W_TAIL_ROWS * per_row + 64) * 2, fill16=F16_NAN)
    ldy = W if via_op else c.ldy
    off = 0 if via_op else c.y_off_bytes
    esz = 4 if c.epi == EPI_F32 else 2
    total = (M + Y_CANARY_ROWS) * ldy + 64 + off // esz + 8
    ybuf = torch.empty(total * esz // 2, dtype=torch.int16, device="cuda")
    if esz == 4:
        ybuf.view(torch.int32).fill_(CANARY32)
    else:
        ybuf.fill_(CANARY16)
    yp = ybuf.data_ptr() + off
    wsb = WS_SIZES[c.ws]
    ws = torch.full((max(1, wsb // 4),), float("nan"), dtype=torch.float32, device="cuda") if wsb else None
    torch.cuda.synchronize()
    args = (dx.data_ptr(), dw.data_ptr(), ds.data_ptr() if ds is not None else None, c.wq, c.group, M, N, K, yp, ldy, c.epi)
    if via_op:
        rc_d, r_d = m.linear_route(*args, ws=ws.data_ptr() if ws is not None else None, ws_bytes=OP_WS, dry_run=True)
        if c.epi == EPI_SWIGLU:
            rc = m.lib().pplhip_op_linear_swiglu(None, args[0], args[1], args[2], c.wq, c.group, M, N, K, yp)
        else:
            rc = m.lib().pplhip_op_linear(None, args[0], args[1], args[2], c.wq, c.group, M, N, K, yp, int(c.epi == EPI_F32))
        r_real = r_d
    else:
        kw = dict(ws=ws.data_ptr() if ws is not None else None, ws_bytes=wsb)
        rc_d, r_d = m.linear_route(*args, dry_run=True, **kw)
        rc, r_real = m.linear_route(*args, dry_run=False, **kw)
    torch.cuda.synchronize()
    if rc_d != 0 or rc != 0:
        return [f"status dry {rc_d} launch {rc}"]
    if r_d != expect_route:
        fails.append(f"dry-run route {r_d!r} != expected {expect_route!r}")
    if r_real != r_d:
        fails.append(f"launch route {r_real!r} != dry-run route {r_d!r}")
    raw = ybuf.cpu().numpy().view(np.uint8)[off:off + ((M + Y_CANARY_ROWS) * ldy + 64) * esz]
    vals = raw.view(np.uint32 if esz == 4 else np.uint16)
    can = CANARY32 if esz == 4 else CANARY16
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
    del dx, dw, ds, ybuf, ws
    return fails


# cases whose route a product switch changes (tests/test_gpu_gemm_exact.py runs them in a child process with the switch set; the route
# here is the default one, which the switch must change)
SWITCH_CASES = {
    "PPLHIP_GEMV_STREAM_MAX_M=4": [
        (8, 128, 3, 124, 128, 0, "op", "dense", False, "kernel=gemm_w8_half128_kernel<f16,3,16> splits=1 kchunk=128 reduce=none order=plain"),
        (8, 128, 4, 256, 512, 2, "op", "dense", False,
         "kernel=gemm_w8_half128_kernel<swiglu,3,16> splits=4 kchunk=128 reduce=splitk_reduce_kernel<swiglu> order=plain"),
        (8, 128, 4, 132, 4096, 1, "op", "dense", False,
         "kernel=gemm_w8_half128_kernel<f32,3,16> splits=8 kchunk=512 reduce=splitk_reduce_kernel<f32> order=plain"),
    ],
    "PPLHIP_GEMM_PC=0": [
        (4, 128, 129, 8192, 128, 0, "op", "dense", False, "kernel=gemm_w4_pc_kernel<f16> splits=1 reduce=none order=plain"),
        (4, 128, 257, 4096, 1024, 2, "op", "dense", False, "kernel=gemm_w4_pc_kernel<swiglu> splits=1 reduce=none order=plain"),
    ],
}
