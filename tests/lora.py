"""Multi-LoRA (csrc/k_lora.hip, pplhip_op_lora): the arithmetic of DESIGN.md section 2 restated in float64, operands on which it is exact,
a bound for random operands, mutants of the reference and the host's tile list.

An adapter gives a target linear y0 = linear(x) the factors A fp16 [r, K], B fp16 [N, r] and one fp32 scale.  For a row m on the adapter:
    t[m, j] = fp16_RNE( sum_k x[m, k] A[j, k] )                                   fp32 sums
    y[m, n] = fp16_RNE( fp32(y0[m, n]) + scale * sum_j fp32(t[m, j]) B[n, j] )    fp32 sums, one multiply by scale at the end
Rows without an adapter are neither read nor rewritten.

Exact cases (build_exact): x = i 2^-4, A = a 2^-3 with at most 16 non-zeros |a| <= 4 a row and |i| <= 15, so every t = S 2^-7 with an
integer |S| <= 960 < 2^11: exactly an fp16 number, whatever the summation order.  B = b 2^-6 with |b| <= 7, scale a power of two and
y0 = iy 2^6 U on the output grid U = 2^-13 scale: fp32(y0) + scale * sum = (iy 2^6 + sum_j S_j b_j) U with every partial sum below 2^24 in
magnitude -- exact in fp32 in any order.  Every output is then one fp16 rounding of a known number: compared bit for bit.

Random cases (build_random) are compared against the float64 value v before the last rounding within bound(): see there.
"""
import numpy as np

TILE = 16
MAX_SLOTS, MAX_RANK = 64, 128
F16_NAN = 0x7E00              # poison behind and between the inputs, and in the workspace
CANARY16 = 0x7D5A             # output canaries (a NaN payload no kernel produces)
U32 = 2.0 ** -24              # unit roundoff of fp32


def pad_rank(r):
    return (r + 15) // 16 * 16


def ulp16(v):
    """the fp16 spacing at |v| (2^-24 in the subnormal range)"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a >= 2.0 ** -14, 2.0 ** (e - 10), 2.0 ** -24)


# ---------------------------------------------------------------------------------------------------------------
# the tile list (rt_lora.cc lora_build_tiles restated)
# ---------------------------------------------------------------------------------------------------------------
def build_tiles(row_slots):
    """[(slot, [row, ...])]: slots ascending, a slot's rows ascending, 16 to a tile"""
    rs = np.asarray(row_slots)
    tiles = []
    for s in sorted(set(int(v) for v in rs if v >= 0)):
        rows = [int(m) for m in np.nonzero(rs == s)[0]]
        for i in range(0, len(rows), TILE):
            tiles.append((s, rows[i:i + TILE]))
    return tiles


def check_tiles(row_slots, tiles):
    """the tile list's properties (raises AssertionError)"""
    rs = np.asarray(row_slots)
    seen = np.zeros(len(rs), dtype=np.int64)
    for s, rows in tiles:
        assert 1 <= len(rows) <= TILE, (s, rows)
        for m in rows:
            assert 0 <= m < len(rs) and rs[m] == s, ("a tile mixes slots or names an unassigned row", s, m)
            seen[m] += 1
    assert (seen[rs >= 0] == 1).all(), "an assigned row is in no tile or in two"
    assert (seen[rs < 0] == 0).all(), "an unassigned row is in a tile"


# ---------------------------------------------------------------------------------------------------------------
# the reference and its mutants
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ["wrong slot for a tile", "last row of a tile dropped", "padding row written", "scale omitted", "rank truncated to 16",
           "t not rounded", "ldy taken as N"]


def reference(x, ybuf, T, N, row_slots, adapters, mutant=None, rounded=True):
    """x: float array [>= T, >= K] (only columns < K of assigned rows are read); ybuf: fp16 [rows, ldy], the whole output buffer with its
    canaries; adapters: {slot: (A fp16 [r, K], B fp16 [N, r], scale)}.  Returns the buffer after the call: fp16 bits as float64 when
    `rounded`, else the float64 values before the last rounding (untouched elements as they were).  mutant: one of MUTANTS."""
    out = np.asarray(ybuf, dtype=np.float16).astype(np.float64).copy()
    y0 = out.copy()
    ldy = out.shape[1]
    flat = out.reshape(-1)
    tiles = build_tiles(row_slots)
    slots_used = sorted(adapters)
    for ti, (s, rows) in enumerate(tiles):
        if mutant == "wrong slot for a tile" and ti == len(tiles) - 1:
            s = slots_used[(slots_used.index(s) + 1) % len(slots_used)]
        A, B, scale = adapters[s]
        A64, B64 = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        K = A64.shape[1]
        if mutant == "rank truncated to 16":
            A64, B64 = A64[:16], B64[:, :16]
        if mutant == "scale omitted":
            scale = 1.0
        upd = list(rows)
        if mutant == "last row of a tile dropped":
            upd = upd[:-1]
        if mutant == "padding row written" and len(rows) < TILE:
            upd = upd + [0]                                   # a padding entry taken for row 0
        for m in upd:
            t = np.asarray(x[m, :K], dtype=np.float64) @ A64.T
            if mutant != "t not rounded":
                t = t.astype(np.float16).astype(np.float64)
            v = y0[m, :N] + float(scale) * (B64 @ t)
            if rounded:
                with np.errstate(over="ignore"):
                    v = v.astype(np.float16).astype(np.float64)
            if mutant == "ldy taken as N":
                flat[m * N:m * N + N] = v
            else:
                flat[m * ldy:m * ldy + N] = v
    return out


def bound(x, ybuf, T, N, row_slots, adapters):
    """Elementwise bound on |device fp16 output - reference(rounded=False)| for the rows on an adapter (0 elsewhere), from the operand
    magnitudes.  With u = 2^-24:
      shrink: the fp32 sum over K carries at most e_t = K u sum_k |x A| in any order; the device's t is the fp16 rounding of some number
        within e_t of the exact sum, so it differs from the reference's t by dt = max |fp16(s +- e_t) - fp16(s)| (0 almost everywhere, one
        fp16 ulp where s sits next to a rounding boundary);
      expand: sum_j dt |B| from that, rp u sum_j |t B| for the fp32 sum over the padded rank, u |scale sum| for the multiply and u |v| for
        the add;
      the output is the fp16 rounding of a number within err of v: |y - v| <= err + ulp16(|v| + err) / 2."""
    out = np.zeros(np.asarray(ybuf).shape, dtype=np.float64)
    y0 = np.asarray(ybuf, dtype=np.float16).astype(np.float64)
    rs = np.asarray(row_slots)
    for s, (A, B, scale) in adapters.items():
        rows = np.nonzero(rs == s)[0]
        if not len(rows):
            continue
        A64, B64 = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
        K, rp = A64.shape[1], pad_rank(A64.shape[0])
        xr = np.asarray(x[rows, :K], dtype=np.float64)
        sx = xr @ A64.T
        e_t = K * U32 * (np.abs(xr) @ np.abs(A64).T)
        t = sx.astype(np.float16).astype(np.float64)
        dt = np.maximum(np.abs((sx + e_t).astype(np.float16).astype(np.float64) - t), np.abs((sx - e_t).astype(np.float16).astype(np.float64) - t))
        acc = t @ B64.T
        mag = (np.abs(t) + dt) @ np.abs(B64).T
        v = y0[rows, :N] + float(scale) * acc
        err = abs(float(scale)) * (dt @ np.abs(B64).T + rp * U32 * mag) + U32 * np.abs(float(scale) * acc) + U32 * (np.abs(v) + abs(float(scale)) * mag * rp * U32)
        out[rows, :N] = err + 0.5 * ulp16(np.abs(v) + err)
    return out


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
RANKS = [1, 8, 16, 24, 64, 128]
SHAPES = [(1, 256, 256), (17, 256, 768), (50, 320, 272), (130, 4096, 512)]
ROW_MAPS = ["none", "all", "runs", "mod3", "ids"]


def row_map(kind, T):
    if kind == "none":
        return np.full(T, -1, dtype=np.int32)
    if kind == "all":
        return np.full(T, 2, dtype=np.int32)
    if kind == "mod3":
        return (np.arange(T) % 3 - 1).astype(np.int32)
    if kind == "ids":                                         # slot ids 0, 5 and 63 (and rows without one)
        return np.array([0, 5, -1, 63, 63, 5], dtype=np.int32)[np.arange(T) % 6]
    # "runs": same-slot runs of 1 / 15 / 16 / 17 / 33 rows on alternating slots, an unassigned row between two runs
    out, s = [], 1
    for n in (1, 15, 16, 17, 33):
        out += [s] * n + [-1]
        s = 4 - s                                             # 1, 3, 1, ...
    out = (out * (T // len(out) + 1))[:T]
    return np.array(out, dtype=np.int32)


class Case:
    """One operator case.  kind 'exact' / 'random' / 'cancel'.  cancel: random operands with y0 = -fp16(the update), so what is left of an
    output is rounding residue and a t that was not rounded shows; x and A are positive there (sum |x A| = |t|: the fp32 sum over K then
    rarely carries t across an fp16 rounding boundary, and the bound stays far below that residue).  Half the cases have ldx > K and
    ldy > N; ldy % 4 != 0 takes the kernel's 2-byte path."""

    def __init__(self, idx, T, K, N, rmap, kind, ranks=None):
        self.T, self.K, self.N, self.rmap, self.kind = T, K, N, rmap, kind
        self.ldx = K + (8 if idx % 2 else 0)
        self.ldy = N + (0, 8, 0, 6)[idx % 4]
        self.row_slots = row_map(rmap, T)
        slots = sorted(set(int(s) for s in self.row_slots if s >= 0)) or [2]
        # two different ranks in one launch wherever two slots are in use
        self.ranks = {s: (ranks or RANKS)[(idx + 2 * i) % len(ranks or RANKS)] for i, s in enumerate(slots)}
        self.seed = idx
        self.name = f"{kind}-T{T}-K{K}-N{N}-{rmap}-r" + "_".join(str(self.ranks[s]) for s in slots) + f"-ldx{self.ldx}-ldy{self.ldy}"
        self.built = False

    def build(self):
        if self.built:
            return self
        rng = np.random.RandomState(1000 + self.seed)
        T, K, N = self.T, self.K, self.N
        self.rows_alloc = T + 3                                # canary rows past T
        self.adapters = {}
        if self.kind == "exact":
            xi = rng.randint(-15, 16, size=(T, K))
            self.x = (xi * 2.0 ** -4).astype(np.float16)
            sums = {}
            for s, r in self.ranks.items():
                a = np.zeros((r, K), dtype=np.int64)
                for j in range(r):
                    cols = rng.choice(K, size=min(K, 16), replace=False)
                    a[j, cols] = rng.randint(-4, 5, size=len(cols))
                a[0, K - 1] = 3                                # the last column of the last K step is in use
                b = rng.randint(-7, 8, size=(N, r))
                scale = 2.0 ** ((s % 3) - 1)                  # 0.5, 1, 2 by slot
                self.adapters[s] = ((a * 2.0 ** -3).astype(np.float16), (b * 2.0 ** -6).astype(np.float16), scale)
                S = xi @ a.T
                # every t is exactly an fp16 number
                assert np.abs(S).max() < 2 ** 11, ("t needs more than 11 bits", self.name)
                t = S * 2.0 ** -7
                assert (t.astype(np.float16).astype(np.float64) == t).all(), ("t not fp16-exact", self.name)
                sums[s] = (S, b, scale)
            iy = rng.randint(-2047, 2048, size=(T, N))
            y0 = np.zeros((T, N))
            self.exact_int = np.zeros((T, N), dtype=np.int64)
            self.unit = np.ones(T)
            for m in range(T):
                s = int(self.row_slots[m])
                scale = sums[s][2] if s >= 0 else 1.0
                U = 2.0 ** -13 * scale
                y0[m] = iy[m] * 64 * U
                if s >= 0:
                    S, b, _ = sums[s]
                    # fp32(y0) + scale * sum is exact in fp32 in any summation order: every partial sum is an integer below 2^24 on the grid U
                    assert np.abs(iy[m]).max() * 64 + (np.abs(S[m])[None, :] * np.abs(b)).sum(axis=1).max() < 2 ** 24, self.name
                    self.exact_int[m] = iy[m] * 64 + b @ S[m]
                    self.unit[m] = U
            self.y0 = y0.astype(np.float16)
            assert (self.y0.astype(np.float64) == y0).all(), ("y0 not fp16-exact", self.name)
        else:
            lo = 0.0 if self.kind == "cancel" else -1.0
            self.x = rng.uniform(lo, 1, size=(T, K)).astype(np.float16)
            for s, r in self.ranks.items():
                A = (rng.uniform(lo, 1, size=(r, K)) * (4.0 / np.sqrt(K))).astype(np.float16)
                B = rng.uniform(-1, 1, size=(N, r)).astype(np.float16)
                self.adapters[s] = (A, B, np.float32(0.37 + 0.21 * (s % 5)))
            self.y0 = rng.uniform(-2, 2, size=(T, N)).astype(np.float16)
            if self.kind == "cancel":
                upd = np.zeros((T, N))
                for s, (A, B, scale) in self.adapters.items():
                    rows = np.nonzero(self.row_slots == s)[0]
                    t = (self.x[rows].astype(np.float64) @ A.astype(np.float64).T).astype(np.float16).astype(np.float64)
                    upd[rows] = float(scale) * (t @ B.astype(np.float64).T)
                self.y0 = np.where((self.row_slots >= 0)[:, None], -upd, self.y0.astype(np.float64)).astype(np.float16)
        # buffers as the device gets them: poison in x's padding, behind it and on the rows without an adapter (never read); canaries around y
        xb = np.full((self.rows_alloc, self.ldx), F16_NAN, dtype=np.uint16)
        assigned = self.row_slots >= 0
        xb[:T, :K][assigned] = self.x.view(np.uint16)[assigned]
        self.xbuf = xb
        yb = np.full((self.rows_alloc, self.ldy), CANARY16, dtype=np.uint16)
        yb[:T, :N] = self.y0.view(np.uint16)
        self.ybuf = yb
        self.built = True
        return self

    def xval(self):
        """x with the poisoned rows as zeros (the reference never reads them)"""
        x = np.zeros((self.T, self.K), dtype=np.float64)
        a = self.row_slots >= 0
        x[a] = self.x.astype(np.float64)[a]
        return x

    def expected(self, mutant=None, rounded=True):
        c = self.build()
        x = c.xval()
        if mutant == "padding row written":
            x[c.row_slots < 0] = np.nan                       # such a kernel reads what the buffer holds on those rows: the poison
        ref = reference(x, c.ybuf.view(np.float16), c.T, c.N, c.row_slots, c.adapters, mutant=mutant, rounded=rounded)
        if c.kind == "exact" and mutant is None and rounded:
            # the integers define the same bits (a check of the reference by the builder's own arithmetic)
            a = c.row_slots >= 0
            want = (c.exact_int * c.unit[:, None]).astype(np.float16)
            assert (ref[:c.T, :c.N][a] == want.astype(np.float64)[a]).all(), c.name
        return ref

    def bound(self):
        c = self.build()
        return bound(c.xval(), c.ybuf.view(np.float16), c.T, c.N, c.row_slots, c.adapters)


def all_cases():
    cases, idx = [], 0
    for T, K, N in SHAPES:
        for rmap in ROW_MAPS:
            for kind in ("exact", "random"):
                cases.append(Case(idx, T, K, N, rmap, kind))
            idx += 1
    cases.append(Case(idx, 50, 320, 272, "runs", "cancel", ranks=[16, 8]))
    cases.append(Case(idx + 1, 17, 256, 768, "all", "cancel", ranks=[16]))
    return cases


def bits(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).view(np.uint16)


def judge(case, got_bits):
    """failures of a device (or mutant) output buffer uint16 [rows_alloc, ldy] against the case: exact cases and everything the call must
    not touch bit for bit, random cases within the bound"""
    c = case.build()
    fails = []
    got_bits = np.asarray(got_bits, dtype=np.uint16).reshape(c.ybuf.shape)
    touched = np.zeros(c.ybuf.shape, dtype=bool)
    touched[:c.T, :c.N] = (c.row_slots >= 0)[:, None]
    if (got_bits[~touched] != c.ybuf[~touched]).any():
        bad = np.argwhere((got_bits != c.ybuf) & ~touched)
        fails.append(f"{len(bad)} elements outside the adapter rows changed (canaries, rows without an adapter), first at {bad[0].tolist()}")
    if c.kind == "exact":
        want = bits(c.expected())
        neq = (got_bits != want) & touched
        if neq.any():
            i = np.argwhere(neq)[0]
            fails.append(f"{int(neq.sum())} of {int(touched.sum())} outputs differ in bits, first at {i.tolist()}: got {got_bits[tuple(i)]:#06x} want {want[tuple(i)]:#06x}")
    else:
        v = c.expected(rounded=False)
        got = got_bits.view(np.float16).astype(np.float64)
        with np.errstate(invalid="ignore"):
            over = touched & ~(np.abs(got - v) <= c.bound())
        if over.any():
            i = np.argwhere(over)[0]
            fails.append(f"{int(over.sum())} outputs beyond the bound, first at {i.tolist()}: got {got[tuple(i)]!r} want {v[tuple(i)]!r} bound {c.bound()[tuple(i)]!r}")
    return fails


def run_case_gpu(m, case):
    """the case through pplhip_op_lora on the device: list of failures"""
    import torch
    c = case.build()
    dev = "cuda"
    x = torch.from_numpy(c.xbuf.view(np.int16).copy()).to(dev)
    y = torch.from_numpy(c.ybuf.view(np.int16).copy()).to(dev)
    n_slots = max(c.adapters) + 1
    keep, A, B, ranks, scales = [], [None] * n_slots, [None] * n_slots, [0] * n_slots, [0.0] * n_slots
    for s, (a, b, scale) in c.adapters.items():
        r, rp = a.shape[0], pad_rank(a.shape[0])
        ap = np.zeros((rp, c.K), dtype=np.float16)
        ap[:r] = a
        bp = np.zeros((c.N, rp), dtype=np.float16)
        bp[:, :r] = b
        ta, tb = torch.from_numpy(ap.view(np.int16)).to(dev), torch.from_numpy(bp.view(np.int16)).to(dev)
        keep += [ta, tb]
        A[s], B[s], ranks[s], scales[s] = ta.data_ptr(), tb.data_ptr(), r, float(scale)
    wsb = m.lora_ws_bytes(c.T, n_slots)
    ws = torch.full((wsb // 2,), F16_NAN, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    rc = m.op_lora(x.data_ptr(), c.ldx, y.data_ptr(), c.ldy, c.T, c.N, c.K, c.row_slots, A, B, ranks, scales, ws.data_ptr(), wsb)
    torch.cuda.synchronize()
    if rc:
        return [f"pplhip_op_lora -> {m.STATUS.get(rc, rc)}"]
    fails = judge(c, y.cpu().numpy().view(np.uint16))
    if (x.cpu().numpy().view(np.uint16) != c.xbuf).any():
        fails.append("x was written")
    return fails
