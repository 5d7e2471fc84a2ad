"""Exactly summable operands for the mixture-of-experts block (k_moe.hip): pplhip_op_moe_route and pplhip_op_moe_ffn checked bit for bit,
with canaries around the output, poison behind every input and a NaN workspace.  No tolerance anywhere.

Every operand is an integer code times a power-of-two unit (tests/gemm_exact.py's scheme), so the integer sums define every bit:
  router  x and the router matrix hold dense small integers with hidden max|x| max|g| <= 2^24: every logit is an exact integer in fp32 in
          any order.  The experts are partitioned into classes that share one gate row (members scattered over the indices), every class
          has at least k members, so a token's k winners are the k lowest indices of its top class with bit-equal logits and
          p_s = exp(0) / k = 1/k exactly (k in {1, 2, 4, 8}).  A class larger than k ties slot k with slot k + 1 on every token.
  w13     four reserved channels of x hold the code 2 in every token; the gate rows of w13 are nonzero only there and evaluate to
          g in {16, 0, 32, -64}, varying by column and expert; the up rows hold dense small codes on the other channels (|u| <= 2048
          codes) under power-of-two row units.  silu(16) and silu(32) differ from g by < 2^-22 relative and g u is an fp16 number, so any
          fp32 evaluation with relative error below 2^-13 rounds to exactly g u; g = 0 and g = -64 give +-0: h is exact however the device
          divides or exponentiates.  (Closed columns check the (gate_i, up_i) interleave: swapped, g = -64 opens the column.)
  w2      integer codes per expert (fp16 integers, or int8 under power-of-two row scales), K zero-padded to inter_p;
          inter max|h| max|w2| <= 2^24 and k max|slot| <= 2^24 in units, so y[t] = fp16_RNE((1/k) sum_s S2[t, e_s] unit) bit for bit.
  E2      k = 1 and W8 only: w2's row scales are arbitrary fp16 numbers, y = fp16(fp32(S2 unit) scale2[n]) -- two roundings (gemm_exact's
          rule E2), the scales picked so that at least 5 % of the outputs differ from the single rounding.
The builder asserts every bound and refuses a case that breaks one.  `distinct` is the one case whose winners differ: its logit gaps are
0 or >= 128, so exp underflows to exactly 0 in fp32 and the weights are 1 / (number of top logits) or 0 -- still exact.

Cases (each with wq 0 and 8); lo / hi: the largest T on short tiles and the next one (32 rows while T k <= 32 E):
  one_token     T 1, E 8, k 2, hidden 64, inter 32     one K tile, under the ring depth; N under one column tile in w2; the decode shape
  k1            37, 8, 1, 128, 64                      k = 1, p = 1; W8: arbitrary scale2 (two roundings)
  k_eq_e_odd3   9, 3, 1, 128, 64                       E not a power of two; classes {0, 2} and {1}; W8: arbitrary scale2 as well
  k_eq_e_odd5   20, 5, 4, 128, 64                      E = 5, k = 4: one class of five, slot 4 ties with slot 5 on every token
  tie_wide      50, 8, 2, 128, 64, classes of 4        the tie between slot k and k + 1 on every token; members scattered
  e64_k8        40, 64, 8, 128, 64, classes of 16      every lane holds a logit; 8 arg-max rounds, all tied
  ragged_n192   33, 8, 2, 192, 160                     ragged last column tile of w2; inter under inter_p; three K tiles
  ragged_n320   33, 8, 2, 320, 96                      the same with three column tiles of w2 and five K tiles of w13
  exact_short   70, 8, 2, 128, 64                      counts 32, 33, 0 on short tiles: no padding against one padded row; experts 2 and 5 empty
  exact_tall    513, 8, 2, 128, 64                     counts 128, 129, 256, 0 on tall tiles; experts 0 and E - 1 empty
  one_expert    300, 8, 2, 128, 64                     every token on experts {1, 4}: three tall tiles each, six experts empty, live 6 of 13
  spread        300, 8, 2, 128, 64                     one_expert's shape with free routing (more live tiles: the call before it, stale state)
  two_pass      547, 8, 2, 128, 64                     1094 pairs: the bucket's second pass, with a ragged last wave
  three_pass_k1 2049, 8, 1, 64, 32                     2049 pairs: the carry across two boundaries, one pair in the last pass (power-of-two scale2)
  three_pass_k8 300, 16, 8, 64, 32                     2400 pairs: experts in all three passes, and experts whose first pair is in the second
  threshold_lo  lo, 8, 2, 128, 64                      short tiles
  threshold_hi  hi, 8, 2, 128, 64                      tall tiles on the same data plus one appended token
  distinct      45, 8, 2, 128, 64, classes of 1        winners with different logits: slots by descending logit, weights 1 and 0
"""
import zlib

import numpy as np

from tests.gemm_exact import CANARY16, F16_NAN, POISON8, _poisoned

RES = (5, 21, 38, 59)            # reserved channels of x (below 64: every hidden has them), code XR in every token
XR = 2
G_VALUES = (16, 0, 32, -64)      # what a gate column evaluates to, by (column + expert) % 4
BUCKET_NT = 1024                 # pairs per pass of moe_bucket_kernel
X_TAIL_ROWS, W_TAIL_ROWS, TAIL_KTILE_BYTES, Y_CANARY_ROWS = 128, 128, 128, 4
COUNTS_SENTINEL = 12345


def tile_rows(T, k, E):
    """the header's formula (moe_tile_rows): 32 rows while T k <= 32 E"""
    return 32 if T * k <= 32 * E else 128


def threshold_T(E, k):
    return 32 * E // k


def scattered(E, size):
    """E experts in E / size classes whose members are spread over the indices"""
    C = E // size
    assert C * size == E
    cls = [[] for _ in range(C)]
    for e in range(E):
        cls[(e + e // C) % C].append(e)
    return cls


def select(r, k, tie_high=False):
    """k rounds of arg-max over integer logits r [T, E]; ties to the lower expert (tie_high: the mistake)"""
    r = np.array(r, dtype=np.int64)
    T, E = r.shape
    ids = np.empty((T, k), dtype=np.int64)
    for s in range(k):
        j = E - 1 - np.argmax(r[:, ::-1], axis=1) if tie_high else np.argmax(r, axis=1)
        ids[:, s] = j
        r[np.arange(T), j] = np.iinfo(np.int64).min
    return ids


def layout(T, E, k, hidden, inter):
    """the workspace of a call (k_moe.hip, moe_layout): byte offsets of its parts and the total"""
    inter_p = (inter + 63) // 64 * 64
    pairs = T * k
    rows_cap = pairs + (E + 1) * 128
    tiles_cap = (pairs + E * 31) // 32 + 1
    at = 0
    off = {}
    for name, nbytes in [("counts", 256), ("live", 4), ("ids", pairs * 4), ("weights", pairs * 4), ("sorted", rows_cap * 4), ("inv", pairs * 4),
                         ("tiles", tiles_cap * 16), ("h", rows_cap * inter_p * 2), ("y", pairs * hidden * 4)]:
        off[name] = at
        at += (nbytes + 255) // 256 * 256
    off["bytes"], off["rows_cap"], off["tiles_cap"] = at, rows_cap, tiles_cap
    return off


class Case:
    """One exact case.  classes: the partition of the experts; plan: the class of every token's winners (None: free routing);
    gate_max: the router codes' range; distinct: winners may differ by >= 128 (weights 1 / n_top and 0)."""

    def __init__(self, name, T, E, k, hidden, inter, wq, classes, plan=None, gate_max=7, distinct=False, claim=None, seed=0, head=None, pow2=False):
        self.name, self.T, self.E, self.k, self.hidden, self.inter, self.wq = f"{name}-w{wq}", T, E, k, hidden, inter, wq
        self.base, self.classes, self.plan, self.gate_max, self.distinct, self.claim, self.seed = name, classes, plan, gate_max, distinct, claim or {}, seed
        self.head = head                 # build T rows, keep the first `head` (threshold_lo)
        self.inter_p = (inter + 63) // 64 * 64
        self.e2 = k == 1 and wq == 8 and not pow2   # (pow2: too many tokens for one scale per row to double-round 5 % of them)
        self.built = False

    # ---- operands ----------------------------------------------------------------------------------------------
    def build(self):
        if self.built:
            return self
        T, E, k, hidden, inter, wq = self.T, self.E, self.k, self.hidden, self.inter, self.wq
        assert k in (1, 2, 4, 8) and k <= E <= 64 and hidden % 64 == 0 and inter % 2 == 0
        assert sorted(e for c in self.classes for e in c) == list(range(E))
        if not self.distinct:
            assert min(len(c) for c in self.classes) >= k, self.name
        rng = np.random.RandomState(zlib.crc32(f"{self.seed or self.base} {E} {k} {hidden} {inter} {wq}".encode()) % (2 ** 31))
        free = np.setdiff1d(np.arange(hidden), RES)
        xm = 3 if (hidden - len(RES)) * 9 <= 2048 else 2
        wm = min(3, 2048 // ((hidden - len(RES)) * xm))
        assert wm >= 1 and hidden * max(xm, XR) * self.gate_max <= 1 << 24, self.name
        self.xm, self.wm = xm, wm
        # router: one row per class
        rows = rng.randint(-self.gate_max, self.gate_max + 1, size=(len(self.classes), hidden)).astype(np.int64)
        self.class_of = np.empty(E, dtype=np.int64)
        for ci, c in enumerate(self.classes):
            self.class_of[c] = ci
        self.gcode = rows[self.class_of]
        # w13: gate rows on the reserved channels, up rows on the others; power-of-two row units that vary by row and expert
        gval = np.array(G_VALUES)[(np.arange(inter)[None, :] + np.arange(E)[:, None]) % 4]                 # [E, inter]
        sg = 2.0 ** -((np.arange(inter)[None, :] // 4 + np.arange(E)[:, None]) % 3)                         # 1, 1/2, 1/4
        su = 2.0 ** -(3 + (np.arange(inter)[None, :] + 2 * np.arange(E)[:, None]) % 3)                      # 1/8, 1/16, 1/32
        total = (gval / (XR * sg)).astype(np.int64)
        assert (total * XR * sg == gval).all()
        gc = np.zeros((E, inter, hidden), dtype=np.int64)
        j1, j2 = rng.randint(-20, 21, size=(2, E, inter))
        q = total // 4
        gc[:, :, RES[0]], gc[:, :, RES[1]], gc[:, :, RES[2]], gc[:, :, RES[3]] = q + j1, q - j1, q + j2, total - 3 * q - j2
        uc = np.zeros((E, inter, hidden), dtype=np.int64)
        uc[:, :, free] = rng.randint(-wm, wm + 1, size=(E, inter, len(free)))
        assert np.abs(gc).max() <= 127
        self.gval, self.sg, self.su, self.gc, self.uc = gval, sg, su, gc, uc
        # w2 codes are drawn after x (their range follows max|h|); x: free routing takes the rows as drawn, a plan filters them
        xc = self._draw_x(rng, free)
        self.xcode = xc
        self.logits = xc @ self.gcode.T
        self.ids = select(self.logits, k)
        sel = np.take_along_axis(self.logits, self.ids, 1)
        d = sel - sel[:, :1]
        ntop = (d == 0).sum(1)
        assert ((d == 0) | (d <= -128)).all() and np.isin(ntop, (1, 2, 4, 8)).all(), self.name
        if not self.distinct:
            assert (d == 0).all(), self.name
        self.p = np.where(d == 0, 1.0 / ntop[:, None], 0.0).astype(np.float32)
        # h in integer form: u codes, h = g u_int su
        uint = np.einsum("th,eih->tei", xc, uc)                                                            # [T, E, inter]
        assert np.abs(uint).max() <= 2048, self.name
        self.uint = uint
        self.uh = 16 * 2.0 ** -5
        hcode = np.where(gval[None] > 0, uint * (np.maximum(gval, 0)[None] // 16) * (su[None] * 32).astype(np.int64), 0)
        self.hcode = hcode                                                                                  # h = hcode uh
        assert np.abs(hcode).max() * self.uh < 65504 and self.uh >= 2.0 ** -14, self.name
        used = np.zeros((T, E), dtype=bool)
        used[np.arange(T)[:, None], self.ids] = True
        hmax = int(np.abs(hcode[used]).max()) if used.any() else 1
        w2max = int(min(127 if wq == 8 else 2047, (1 << 24) // (inter * max(1, hmax) * (1 if self.e2 else 4 * k))))   # (4: the row units' spread)
        assert w2max >= 1 and inter * hmax * w2max <= 1 << 24, self.name
        self.w2max = w2max
        w2c = np.zeros((E, hidden, self.inter_p), dtype=np.int64)
        w2c[:, :, :inter] = rng.randint(-w2max, w2max + 1, size=(E, hidden, inter))
        self.w2code = w2c
        S2 = np.zeros((T, k, hidden), dtype=np.int64)
        for s in range(k):
            for e in range(E):
                t = np.nonzero(self.ids[:, s] == e)[0]
                S2[t, s] = hcode[t, e] @ w2c[e, :, :inter].T
        self.S2 = S2
        assert np.abs(S2).max() <= 1 << 24
        self._units(rng)
        self._operands()
        if self.head is not None:
            self._truncate(self.head)
        self.built = True
        return self

    def _draw_x(self, rng, free):
        T, k, hidden, xm = self.T, self.k, self.hidden, self.xm

        def draw(n):
            xc = np.zeros((n, hidden), dtype=np.int64)
            xc[:, free] = rng.randint(-xm, xm + 1, size=(n, len(free)))
            xc[:, list(RES)] = XR
            return xc

        def gaps_ok(xc):
            r = np.sort(xc @ self.gcode.T, axis=1)[:, ::-1][:, :k]
            d = r - r[:, :1]
            return ((d == 0) | (d <= -128)).all(1) & np.isin((d == 0).sum(1), (1, 2, 4, 8))

        if self.plan is None and not self.distinct:
            return draw(T)
        out = np.zeros((T, hidden), dtype=np.int64)
        want = np.full(T, -1) if self.plan is None else np.asarray(self.plan)
        assert len(want) == T
        todo = list(range(T))
        lowest = [tuple(sorted(c)[:k]) for c in self.classes]
        for _ in range(200):
            if not todo:
                break
            pool = draw(4 * len(todo) + 64)
            ids = select(pool @ self.gcode.T, k)
            ok = gaps_ok(pool)
            if self.plan is None:
                rows = [i for i in range(len(pool)) if ok[i]]
                for t, i in zip(list(todo), rows):
                    out[t] = pool[i]
                    todo.remove(t)
                continue
            by_class = {}
            for i in range(len(pool)):
                key = tuple(ids[i])
                for ci, low in enumerate(lowest):
                    if ok[i] and key == low:
                        by_class.setdefault(ci, []).append(i)
            for t in list(todo):
                if by_class.get(want[t]):
                    out[t] = pool[by_class[want[t]].pop()]
                    todo.remove(t)
        assert not todo, (self.name, "could not draw the planned routing")
        return out

    def _units(self, rng):
        """w2's row scales: powers of two that vary by row and expert, or (E2) arbitrary fp16 numbers picked for double roundings"""
        T, E, k, hidden = self.T, self.E, self.k, self.hidden
        if self.e2:
            # one octave of fp16 scales holds every significand; a row takes the best of ALTS draws of its codes together with the scale
            # that double-rounds the most of its expert's first 8 tokens (a power of two times a scale rounds like the scale)
            ALTS, inter = 6, self.inter
            hsel = np.abs(np.take_along_axis(self.hcode, self.ids[:, :, None], 1))
            vbound = inter * max(1, int(hsel.max())) * self.w2max * self.uh
            b = int(np.floor(np.log2(32768.0 / vbound)))
            assert -14 <= b <= 14, self.name
            cand = np.arange((b + 15) << 10, (b + 16) << 10, dtype=np.uint16).view(np.float16)              # [2^b, 2^(b+1)): normal fp16
            c32, c64 = cand.astype(np.float32), cand.astype(np.float64)
            sc = np.empty((E, hidden))
            for e in range(E):
                t = np.nonzero(self.ids[:, 0] == e)[0]
                alts = rng.randint(-self.w2max, self.w2max + 1, size=(ALTS, hidden, inter)).astype(np.int64)
                alts[0] = self.w2code[e, :, :inter]
                v = np.einsum("ti,rni->rnt", self.hcode[t[:8], e], alts)[..., None] * self.uh               # fp32-exact
                hit = ((v.astype(np.float32) * c32).astype(np.float16) != (v * c64).astype(np.float16)).sum(2)   # [ALTS, hidden, cand]
                best = np.argmax((hit + rng.rand(*hit.shape)).transpose(1, 0, 2).reshape(hidden, -1), axis=1)
                self.w2code[e, :, :inter] = alts[best // len(cand), np.arange(hidden)]
                sc[e] = c64[best % len(cand)]
                self.S2[t, 0] = self.hcode[t, e] @ self.w2code[e, :, :inter].T
            assert np.abs(self.S2).max() <= 1 << 24
            self.s2 = sc
            return
        rel = 2.0 ** -((np.arange(hidden)[None, :] + np.arange(E)[:, None]) % 3)                            # 1, 1/2, 1/4
        slot = self.S2 * (rel[self.ids] * 4).astype(np.int64)                                               # in units of uh base / 4
        assert k * np.abs(slot).max() <= 1 << 24, self.name
        ymax = max(1.0, float(np.abs(slot.sum(1)).max()) / 4 / k * self.uh)
        base = 2.0 ** np.floor(np.log2(32768.0 / ymax))
        base = min(base, 1.0)
        assert base / 4 >= 2.0 ** -12, self.name
        self.s2 = rel * base

    def _operands(self):
        """the device arrays: x, gate (fp16), w13 (rows interleaved gate_i, up_i), w2 (K padded), the scales"""
        E, inter, hidden, wq = self.E, self.inter, self.hidden, self.wq

        def f16_exact(a):
            h = np.asarray(a, dtype=np.float64).astype(np.float16)
            assert (h.astype(np.float64) == a).all() and ((h == 0) | (np.abs(h.astype(np.float64)) >= 2.0 ** -14)).all(), self.name
            return h

        self.x, self.gate = f16_exact(self.xcode), f16_exact(self.gcode)
        c13 = np.empty((E, 2 * inter, hidden), dtype=np.int64)
        c13[:, 0::2], c13[:, 1::2] = self.gc, self.uc
        s13 = np.empty((E, 2 * inter))
        s13[:, 0::2], s13[:, 1::2] = self.sg, self.su
        self.c13, self.s13f = c13, s13
        if wq == 8:
            self.w13, self.s13 = c13.astype(np.int8), f16_exact(s13)
            self.w2, self.s2h = self.w2code.astype(np.int8), f16_exact(self.s2)
        else:
            self.w13, self.s13 = f16_exact(c13 * s13[:, :, None]), None
            self.w2, self.s2h = f16_exact(self.w2code * self.s2[:, :, None]), None

    def _truncate(self, T):
        for n in ("xcode", "logits", "ids", "p", "uint", "hcode", "S2", "x"):
            setattr(self, n, getattr(self, n)[:T])
        self.T = T

    # ---- the exact outputs -------------------------------------------------------------------------------------
    def expected(self):
        """y bits from the integer form: fp16_RNE(sum_s p_s S2 unit); E2: fp16(fp32(S2 uh) scale2)"""
        s2 = self.s2[self.ids]                                                                              # [T, k, hidden]
        if self.e2:
            return ((self.S2[:, 0] * self.uh).astype(np.float32) * s2[:, 0].astype(np.float32)).astype(np.float16)
        slots = self.S2 * self.uh * s2 * self.p.astype(np.float64)[:, :, None]
        assert (slots.astype(np.float32).astype(np.float64) == slots).all()
        y = slots.sum(1)
        assert (y.astype(np.float32).astype(np.float64) == y).all() and np.abs(y).max() < 65504, self.name
        return y.astype(np.float16)

    def single_rounding(self):
        return (self.S2[:, 0] * self.uh * self.s2[self.ids][:, 0]).astype(np.float16)

    def double_roundings(self):
        return int((self.expected().view(np.uint16) != self.single_rounding().view(np.uint16)).sum()) if self.e2 else 0

    def histogram(self):
        return np.bincount(self.ids.ravel(), minlength=64)

    def passes(self):
        return -(-self.T * self.k // BUCKET_NT)

    def tied_tokens(self):
        """tokens whose k-th and (k+1)-th logits are equal"""
        if self.k == self.E:
            return 0
        r = np.sort(self.logits, axis=1)[:, ::-1]
        return int((r[:, self.k - 1] == r[:, self.k]).sum())


def reference(case):
    """float64 restatement of DESIGN.md's numerics on the device operands: ids, weights (fp32), y (fp16).  silu is evaluated honestly."""
    c = case.build()
    T, E, k, inter = c.T, c.E, c.k, c.inter
    x = c.x.astype(np.float64)
    r = x @ c.gate.astype(np.float64).T
    ids = np.argsort(-r, axis=1, kind="stable")[:, :k]
    sel = np.take_along_axis(r, ids, 1)
    with np.errstate(under="ignore"):
        p = np.exp(sel - sel[:, :1])
        p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    s13 = np.ones((E, 2 * inter)) if c.s13 is None else c.s13.astype(np.float64)
    s2 = np.ones((E, c.hidden)) if c.s2h is None else c.s2h.astype(np.float64)
    slots = np.zeros((T, k, c.hidden))
    for e in range(E):
        t, s = np.nonzero(ids == e)
        gu = ((x[t] @ c.w13[e].astype(np.float64).T) * s13[e]).astype(np.float16).astype(np.float64)
        g, u = gu[:, 0::2], gu[:, 1::2]
        with np.errstate(over="ignore"):
            h = (g / (1.0 + np.exp(-g)) * u).astype(np.float16).astype(np.float64)
        acc = h @ c.w2[e].astype(np.float64)[:, :inter].T
        if c.e2:
            slots[t, s] = (acc.astype(np.float32) * s2[e].astype(np.float32)).astype(np.float64)
        else:
            slots[t, s] = acc * s2[e] * p[t, s, None].astype(np.float64)
    return ids, p, slots.sum(1).astype(np.float16)


# -------------------------------------------------------------------------------------------------------------------
# a model of the block, kernel by kernel, that can make one named mistake
# -------------------------------------------------------------------------------------------------------------------
FAULTS = {   # fault -> the case written for it
    "ties to the higher expert": "tie_wide",
    "slots in ascending logit order": "distinct",
    "run[e] not carried between passes": "three_pass_k8",
    "two pairs of one expert swapped within a pass": "two_pass",
    "routing weight read from slot s ^ 1": "distinct",
    "padding rows stored": "exact_short",
    "last K tile of w2 skipped": "ragged_n192",
    "last K tile of w13 read twice": "one_token",
    "w2 column tile clamp off by one row": "ragged_n320",
    "(gate_i, up_i) swapped": "k1",
    "expert e's weights taken from e + 1": "k_eq_e_odd3",
    "stale live from a previous, larger call": "one_expert",       # (after `spread` on the same workspace)
}


def bucket(ids, E, BM, fault=None):
    """moe_bucket_kernel: live, tiles [(expert, row0, valid)], sorted (padded rows name their tile's first pair), inv"""
    T, k = ids.shape
    flat = ids.ravel()
    n = flat.size
    cnt = np.bincount(flat, minlength=E)
    te = -(-cnt // BM)
    row0 = np.concatenate([[0], np.cumsum(te * BM)])[:-1]
    tiles = [(e, int(row0[e] + i * BM), int(min(BM, cnt[e] - i * BM))) for e in range(E) for i in range(te[e])]
    srt = np.full(int((te * BM).sum()), -1, dtype=np.int64)
    inv = np.full(n, -1, dtype=np.int64)
    run = np.zeros(E, dtype=np.int64)
    swapped = False
    for base in range(0, n, BUCKET_NT):
        seg = flat[base:base + BUCKET_NT]
        for e in np.unique(seg):
            idx = np.nonzero(seg == e)[0]
            if fault == "two pairs of one expert swapped within a pass" and not swapped and len(idx) >= 2:
                idx = np.concatenate([idx[1::-1], idx[2:]])
                swapped = True
            r = row0[e] + run[e] + np.arange(len(idx))
            srt[r] = base + idx
            inv[base + idx] = r
        if fault != "run[e] not carried between passes":
            run += np.bincount(seg, minlength=E)
    for e, r0, valid in tiles:
        srt[r0 + valid:r0 + BM] = srt[r0]
    return dict(live=len(tiles), tiles=tiles, sorted=srt, inv=inv)


def model(case, fault=None, prev=None):
    """the block as the kernels run it, in float64 on the device operands, on a NaN workspace: dict(ids, weights, y, live, tiles, sorted,
    inv).  fault: one of FAULTS; prev: the state a previous call of the same shape left (stale live reads it)."""
    c = case.build()
    T, E, k, hidden, inter, inter_p = c.T, c.E, c.k, c.hidden, c.inter, c.inter_p
    ids = select(c.logits, k, tie_high=fault == "ties to the higher expert")
    sel = np.take_along_axis(c.logits, ids, 1)
    if fault == "slots in ascending logit order":
        o = np.argsort(sel, axis=1, kind="stable")
        ids, sel = np.take_along_axis(ids, o, 1), np.take_along_axis(sel, o, 1)
    with np.errstate(under="ignore"):
        p = np.exp((sel - sel.max(1, keepdims=True)).astype(np.float64))
        p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    BM = tile_rows(T, k, E)
    st = bucket(ids, E, BM, fault)
    tiles, srt = list(st["tiles"]), st["sorted"]
    if fault == "stale live from a previous, larger call" and prev is not None and prev["live"] > st["live"]:
        full = prev["sorted"].copy()
        n = min(len(full), len(srt))
        full[:n] = srt[:n]
        srt = np.concatenate([full, srt[n:]])
        tiles = tiles + list(prev["tiles"][len(tiles):prev["live"]])
    x = c.x.astype(np.float64)
    s13 = np.ones((E, 2 * inter)) if c.s13 is None else c.s13.astype(np.float64)
    s2 = np.ones((E, hidden)) if c.s2h is None else c.s2h.astype(np.float64)
    shift = fault == "expert e's weights taken from e + 1"

    def weights_of(w, s, e):
        if shift and e + 1 >= E:
            return np.full(w[0].shape, np.nan), s[0]
        return w[e + shift].astype(np.float64), s[e + shift]

    h = np.full((max(len(srt), 1), inter_p), np.nan)
    for e, r0, valid in tiles:                                  # w13: gather through sorted, SwiGLU, h in sorted order
        w, sc = weights_of(c.w13, s13, e)
        rows = srt[r0:r0 + BM]
        xr = np.where((rows >= 0)[:, None], x[np.maximum(rows, 0) // k], np.nan)
        acc = xr @ w.T
        if fault == "last K tile of w13 read twice":
            acc = acc + xr[:, -64:] @ w[:, -64:].T
        gu = (acc * sc).astype(np.float16).astype(np.float64)
        g, u = gu[:, 0::2], gu[:, 1::2]
        if fault == "(gate_i, up_i) swapped":
            g, u = u, g
        with np.errstate(over="ignore", invalid="ignore"):
            hv = (g / (1.0 + np.exp(-g)) * u).astype(np.float16).astype(np.float64)
        h[r0:r0 + valid, :inter] = hv[:valid]
        h[r0:r0 + valid, inter:] = 0.0
    ys = np.full((T * k, hidden), np.nan)
    pw = p.ravel().astype(np.float64)
    for e, r0, valid in tiles:                                  # w2: h rows, the routing weight, scatter to y_slots[pair]
        w, sc = weights_of(c.w2, s2, e)
        if fault == "w2 column tile clamp off by one row" and hidden % 128:
            w, sc = w.copy(), np.array(sc, dtype=np.float64)
            w[hidden - 1], sc[hidden - 1] = w[hidden - 2], sc[hidden - 2]
        hr = h[r0:r0 + BM]
        kk = inter_p - 64 if fault == "last K tile of w2 skipped" else inter_p
        with np.errstate(invalid="ignore"):
            acc = hr[:, :kk] @ w[:, :kk].T
        v = (acc.astype(np.float32) * sc.astype(np.float32)).astype(np.float64) if c.e2 else acc * sc
        n_store = BM if fault == "padding rows stored" else valid
        for j in range(n_store):
            pair = srt[r0 + j]
            if pair >= 0:
                ys[pair] = v[j] * pw[pair ^ 1 if fault == "routing weight read from slot s ^ 1" and k > 1 else pair]
    with np.errstate(invalid="ignore", over="ignore"):
        y = ys.reshape(T, k, hidden).astype(np.float32).sum(1, dtype=np.float64).astype(np.float16)
    return dict(ids=ids, weights=p, y=y, live=st["live"], tiles=st["tiles"], sorted=st["sorted"], inv=st["inv"])


def same_outputs(a, b):
    """every bit of what a call leaves: ids, weights, y, and the bucket's live count, tile table and row lists"""
    return ((a["ids"] == b["ids"]).all() and (a["weights"].view(np.uint32) == b["weights"].view(np.uint32)).all()
            and (a["y"].view(np.uint16) == b["y"].view(np.uint16)).all() and a["live"] == b["live"] and a["tiles"] == b["tiles"]
            and np.array_equal(a["sorted"], b["sorted"]) and np.array_equal(a["inv"], b["inv"]))


# -------------------------------------------------------------------------------------------------------------------
# the cases
# -------------------------------------------------------------------------------------------------------------------
def _plan(counts, seed):
    """a shuffled token -> class plan with the given number of tokens per class"""
    seq = np.concatenate([np.full(n, c) for c, n in enumerate(counts)]).astype(np.int64)
    return np.random.RandomState(seed).permutation(seq)


def _three_pass_plan():
    rng = np.random.RandomState(5)
    return np.concatenate([np.zeros(136, dtype=np.int64), rng.randint(0, 2, size=162), [0, 1]])   # class 1 starts at pair 1088


def _table(wq):
    sing = lambda E: [[e] for e in range(E)]
    lo = threshold_T(8, 2)
    pairs2 = scattered(8, 2)      # {0, 7}, {1, 4}, {2, 5}, {3, 6}
    return [
        Case("one_token", 1, 8, 2, 64, 32, wq, pairs2, claim=dict(passes=1, tile=32)),
        Case("k1", 37, 8, 1, 128, 64, wq, sing(8), claim=dict(passes=1, tile=32)),
        Case("k_eq_e_odd3", 9, 3, 1, 128, 64, wq, [[0, 2], [1]], claim=dict(tied_is_hist=0, tile=32)),
        Case("k_eq_e_odd5", 20, 5, 4, 128, 64, wq, [[0, 1, 2, 3, 4]], claim=dict(tied=20, hist={4: 0, 0: 20}, tile=32)),
        Case("tie_wide", 50, 8, 2, 128, 64, wq, scattered(8, 4), claim=dict(tied=50, tile=32)),
        Case("e64_k8", 40, 64, 8, 128, 64, wq, scattered(64, 16), claim=dict(tied=40, tile=32)),
        Case("ragged_n192", 33, 8, 2, 192, 160, wq, pairs2, claim=dict(tile=32)),
        Case("ragged_n320", 33, 8, 2, 320, 96, wq, pairs2, claim=dict(tile=32)),
        Case("exact_short", 70, 8, 2, 128, 64, wq, pairs2, plan=_plan([32, 33, 0, 5], 1),
             claim=dict(hist={0: 32, 7: 32, 1: 33, 4: 33, 2: 0, 5: 0, 3: 5, 6: 5}, tile=32)),
        Case("exact_tall", 513, 8, 2, 128, 64, wq, pairs2, plan=_plan([0, 128, 129, 256], 2),
             claim=dict(hist={0: 0, 7: 0, 1: 128, 4: 128, 2: 129, 5: 129, 3: 256, 6: 256}, tile=128, passes=2)),
        Case("one_expert", 300, 8, 2, 128, 64, wq, pairs2, plan=_plan([0, 300, 0, 0], 3),
             claim=dict(hist={1: 300, 4: 300, 0: 0, 2: 0, 3: 0, 5: 0, 6: 0, 7: 0}, tile=128, live=6)),
        Case("spread", 300, 8, 2, 128, 64, wq, pairs2, claim=dict(tile=128, live=8)),
        Case("two_pass", 547, 8, 2, 128, 64, wq, pairs2, claim=dict(passes=2, tile=128)),
        Case("three_pass_k1", 2049, 8, 1, 64, 32, wq, sing(8), pow2=True, claim=dict(passes=3, tile=128)),
        Case("three_pass_k8", 300, 16, 8, 64, 32, wq, scattered(16, 8), plan=_three_pass_plan(), claim=dict(passes=3, tile=128)),
        Case("threshold_lo", lo + 1, 8, 2, 128, 64, wq, pairs2, seed=9, head=lo, claim=dict(tile=32)),
        Case("threshold_hi", lo + 1, 8, 2, 128, 64, wq, pairs2, seed=9, claim=dict(tile=128)),
        Case("distinct", 45, 8, 2, 128, 64, wq, sing(8), gate_max=255, distinct=True, claim=dict(tied=0, tile=32)),
    ]


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = [c for wq in (0, 8) for c in _table(wq)]
    return _CASES


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


# -------------------------------------------------------------------------------------------------------------------
# the device run (tests/test_gpu_moe_exact.py)
# -------------------------------------------------------------------------------------------------------------------
class DeviceCase:
    """a case's operands on the device, each at the start of an allocation with a poison tail, and a canary buffer around y"""

    def __init__(self, torch, case):
        c = self.c = case.build()
        self.torch = torch
        K13, K2 = c.hidden, c.inter_p
        self.x = _poisoned(torch, c.x, X_TAIL_ROWS * c.hidden * 2 + TAIL_KTILE_BYTES, fill16=F16_NAN)
        self.gate = _poisoned(torch, c.gate, W_TAIL_ROWS * c.hidden * 2 + TAIL_KTILE_BYTES, fill16=F16_NAN)
        if c.wq == 8:
            self.w13 = _poisoned(torch, c.w13, W_TAIL_ROWS * K13 + TAIL_KTILE_BYTES, fill8=POISON8)
            self.w2 = _poisoned(torch, c.w2, W_TAIL_ROWS * K2 + TAIL_KTILE_BYTES, fill8=POISON8)
            self.s13 = _poisoned(torch, c.s13, (W_TAIL_ROWS + 64) * 2, fill16=F16_NAN)
            self.s2 = _poisoned(torch, c.s2h, (W_TAIL_ROWS + 64) * 2, fill16=F16_NAN)
        else:
            self.w13 = _poisoned(torch, c.w13, W_TAIL_ROWS * K13 * 2 + TAIL_KTILE_BYTES, fill16=F16_NAN)
            self.w2 = _poisoned(torch, c.w2, W_TAIL_ROWS * K2 * 2 + TAIL_KTILE_BYTES, fill16=F16_NAN)
            self.s13 = self.s2 = None
        self.ldy = c.hidden + 8
        self.ws_bytes = layout(c.T, c.E, c.k, c.hidden, c.inter)["bytes"]
        self.fresh_y()

    def fresh_y(self):
        c = self.c
        self.ybuf = self.torch.full(((c.T + 2 * Y_CANARY_ROWS) * self.ldy + 64,), CANARY16, dtype=self.torch.int16, device="cuda")
        self.y_ptr = self.ybuf.data_ptr() + Y_CANARY_ROWS * self.ldy * 2

    def ptr(self, t):
        return None if t is None else t.data_ptr()

    def launch(self, L, ws_ptr, ws_bytes, stream=None):
        c = self.c
        return L.pplhip_op_moe_ffn(stream, self.x.data_ptr(), self.gate.data_ptr(), self.w13.data_ptr(), self.ptr(self.s13), self.w2.data_ptr(),
                                   self.ptr(self.s2), c.wq, c.T, c.E, c.k, c.hidden, c.inter, ws_ptr, ws_bytes, self.y_ptr, self.ldy)

    def y_bits(self):
        """(y bits [T, hidden], failures of the guards) after a synchronise"""
        c = self.c
        vals = self.ybuf.cpu().numpy().view(np.uint16)
        inside = np.zeros(vals.size, dtype=bool)
        idx = ((Y_CANARY_ROWS + np.arange(c.T))[:, None] * self.ldy + np.arange(c.hidden)[None, :]).reshape(-1)
        inside[idx] = True
        bad = np.nonzero((vals != CANARY16) & ~inside)[0]
        fails = []
        if bad.size:
            fails.append(f"{bad.size} canaries overwritten, first at element {bad[0]} (row {bad[0] // self.ldy - Y_CANARY_ROWS}, column {bad[0] % self.ldy})")
        got = vals[idx].reshape(c.T, c.hidden)
        if np.isnan(got.view(np.float16)).any():
            fails.append(f"{int(np.isnan(got.view(np.float16)).sum())} NaN in y")
        return got, fails

    def check(self, want=None, ws=None):
        """failures of one finished call: y bit for bit, the guards, and (ws: the call's workspace tensor, bytes) the bucket's state"""
        c = self.c
        got, fails = self.y_bits()
        want = c.expected().view(np.uint16) if want is None else want
        bad = got != want
        if bad.any():
            t, col = (int(v) for v in np.argwhere(bad)[0])
            st = bucket(c.ids, c.E, tile_rows(c.T, c.k, c.E))
            where = []
            for s in range(c.k):
                e, pair = int(c.ids[t, s]), t * c.k + s
                rows = [(r0, r0 + v) for ee, r0, v in st["tiles"] if ee == e]
                where.append(f"slot {s}: expert {e} rows [{rows[0][0]}, {rows[-1][1]}) row {int(st['inv'][pair])} pass {pair // BUCKET_NT}")
            fails.append(f"{int(bad.sum())} of {bad.size} outputs wrong, first (t {t}, column {col}): got {got.view(np.float16)[t, col]!r} want "
                         f"{want.view(np.float16)[t, col]!r}; ids {c.ids[t].tolist()}; " + "; ".join(where))
        if ws is not None:
            fails += self.check_bucket(ws)
        return fails

    def check_bucket(self, ws):
        """the bucket kernel's promises, read from the workspace: counts left zero, live, the tile table, stable placement, padding rows"""
        c = self.c
        lay = layout(c.T, c.E, c.k, c.hidden, c.inter)
        raw = ws.view(self.torch.uint8)[:lay["bytes"]].cpu().numpy()
        i32 = lambda name, n: raw[lay[name]:lay[name] + 4 * n].view(np.int32)
        st = bucket(c.ids, c.E, tile_rows(c.T, c.k, c.E))
        fails = []
        if i32("counts", 64).any():
            fails.append("counts not left zero")
        if int(i32("live", 1)[0]) != st["live"]:
            fails.append(f"live {int(i32('live', 1)[0])} != {st['live']}")
        tiles = i32("tiles", 4 * st["live"]).reshape(-1, 4)[:, :3]
        if tiles.tolist() != [list(t) for t in st["tiles"]]:
            fails.append("tile table differs")
        if not np.array_equal(i32("sorted", len(st["sorted"])), st["sorted"]):
            r = int(np.nonzero(i32("sorted", len(st["sorted"])) != st["sorted"])[0][0])
            fails.append(f"sorted differs first at row {r}: {int(i32('sorted', len(st['sorted']))[r])} != {int(st['sorted'][r])} (placement not stable?)")
        if not np.array_equal(i32("inv", c.T * c.k), st["inv"]):
            fails.append("inv is not the inverse of sorted")
        return fails


def nan_workspace(torch, nbytes):
    return torch.full((nbytes // 4 + 1,), float("nan"), dtype=torch.float32, device="cuda")


def run_route_gpu(m, torch, case):
    """pplhip_op_moe_route: ids with slot order, counts (zeros from E to 63), weights bit for bit"""
    c = case.build()
    d = DeviceCase(torch, c)
    ids = torch.full((c.T, c.k), -1, dtype=torch.int32, device="cuda")
    wts = torch.full((c.T, c.k), float("nan"), dtype=torch.float32, device="cuda")
    counts = torch.full((64,), COUNTS_SENTINEL, dtype=torch.int32, device="cuda")
    rc = m.lib().pplhip_op_moe_route(None, d.x.data_ptr(), d.gate.data_ptr(), c.T, c.hidden, c.E, c.k, ids.data_ptr(), wts.data_ptr(), counts.data_ptr())
    torch.cuda.synchronize()
    fails = [f"status {rc}"] if rc else []
    gi, gw, gc = ids.cpu().numpy(), wts.cpu().numpy(), counts.cpu().numpy()
    if not (gi == c.ids).all():
        t = int(np.argwhere(gi != c.ids)[0][0])
        fails.append(f"ids differ first at token {t}: got {gi[t].tolist()} want {c.ids[t].tolist()} (logits {c.logits[t].tolist()})")
    if not (gc == c.histogram()).all():
        fails.append(f"counts {gc[:c.E + 2].tolist()} != {c.histogram()[:c.E + 2].tolist()}")
    if not (gw.view(np.uint32) == c.p.view(np.uint32)).all():
        t = int(np.argwhere(gw.view(np.uint32) != c.p.view(np.uint32))[0][0])
        fails.append(f"weights differ first at token {t}: got {gw[t].tolist()} want {c.p[t].tolist()}")
    return fails
