"""Host references and case builders for the row kernels between the GEMMs: (Skip)RMSNorm in every kernel form, the split-K slab
consumers and the KV-cache write.  Pure numpy, no device: tests/test_gpu_row_ops.py runs the cases on the GPU, tests/test_row_ops_spec.py
checks on the CPU that the cases reach every kernel form and that the checker rejects a subtly wrong kernel.

RMSNorm reference (float64): x~ = RN16(x + skip), y = x~ w / sqrt(mean(x~^2) + eps); RN16 is one correct rounding to fp16 (the sum of two
fp16 numbers is exact in float64).

Checker: `got` must be an fp16 number in [RN16(y (1 - d)), RN16(y (1 + d))], d = DELTA = 2^-16.  Where d comes from (u = 2^-24, one fp32
rounding): every form sums at most 64 squares per thread (8 chunks of 8), then 6 shuffle steps and at most 16 per-wave partials -- each
partial sum of positive terms passes through fewer than 100 fp32 roundings (products included), so ss is within 100 u < 2^-17 of the exact
sum, relatively.  inv = 1 / sqrt(ss / hidden + eps) carries half of that (the square root halves a relative error) plus the roundings of
the division by hidden, the sum with eps, the root and the reciprocal (the root halves the first two): under 2^-18 + 3 u; the product
x~ * inv * w adds two more: under 2^-18 + 5 u = 2^-16 * 0.33.  A kernel that drops, doubles or misplaces a chunk, divides by another
count or forgets eps moves every output of a row by far more than d, and a shift of s > d moves about min(1, s / 2^-11) of a row's
outputs out of their intervals (needle rows below).
"""
import functools

import numpy as np

DELTA = 2.0 ** -16
EPS = 1e-5
EPS64 = float(np.float32(EPS))   # the kernel's `float eps`
BLOCK = 128                      # rows per float64 pass (a 2048 x 16384 case is never held in float64 whole)


def rn16(a):
    """float64 -> fp16, one correct rounding"""
    with np.errstate(over="ignore"):   # (a mutant's output may overflow to inf; the reference's never does)
        return np.asarray(a, dtype=np.float64).astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------
# (Skip)RMSNorm: the kernel forms and the cases that reach them
# ---------------------------------------------------------------------------------------------------------------
# (rows, hidden) of every launch shape tests/test_gpu_row_ops.py runs, by the form it must take
FORM_CASES = {
    "rmsnorm_kernel<1,256>": [(1, 8), (3, 2048), (37, 136)],
    "rmsnorm_kernel<2,256>": [(4, 4096), (513, 4096), (37, 2056), (37, 4088)],
    "rmsnorm_kernel<4,256>": [(4, 8192), (1024, 8192), (37, 4104), (4, 5120), (640, 5120)],   # (640 rows: above the wide forms' 512)
    "rmsnorm_kernel<8,256>": [(1, 16384), (37, 8200), (2048, 16384)],
    "rmsnorm_kernel<1,512>": [(5, 4096), (512, 4096)],
    "rmsnorm_kernel<1,1024>": [(5, 8192), (37, 4608)],
}
QUANT_TAGS = {0: "", 1: ",i8", 2: ",f8"}
ALL_FORM_CASES = [(r, h) for v in FORM_CASES.values() for (r, h) in v]


def form_text(form, quant):
    return form[:-1] + QUANT_TAGS[quant] + ">"


def form_args(form):
    """'rmsnorm_kernel<4,256,f8>' -> (4, 256)"""
    a = form[form.index("<") + 1:-1].split(",")
    return int(a[0]), int(a[1])


def expected_form(rows, hidden):
    for f, cases in FORM_CASES.items():
        if (rows, hidden) in cases:
            return f
    raise KeyError((rows, hidden))


NEEDLE_MAG = 1.0 + (2 * np.arange(8) + 1) / 16.0          # eight distinct magnitudes in [1, 2)
NEEDLE_SIGN = np.array([1, -1, -1, 1, -1, 1, 1, -1], dtype=np.float64)
NEEDLE = (NEEDLE_MAG * NEEDLE_SIGN).astype(np.float16)
SWAP_LANES = (2, 5)
EDGE_KINDS = ("zero", "big", "cancel", "tiny")


def norm_weights(hidden):
    """distinct within every chunk and against the same lane of the next chunk: a swap of two lanes or a shift by one chunk shows"""
    w = (0.5 + (np.arange(hidden) * 0.6180339887498949) % 1.0).astype(np.float16)
    c = w.reshape(-1, 8)
    assert all(len(set(r.tolist())) == 8 for r in c[:64]) and (hidden == 8 or (w[8:] != w[:-8]).all())
    return w


def needle_positions(chunks, seed=0):
    """needle chunks of a launch shape of at most 4 rows: chunk 0, the last one, both sides of every 64-lane wave boundary (every
    i * NT boundary of the register loops is one of them), and 16 seeded random chunks"""
    p = {0, chunks - 1}
    for b in range(64, chunks, 64):
        p.update((b - 1, b))
    p.update(int(c) for c in np.random.default_rng(1000 + seed + chunks).integers(0, chunks, size=16))
    return sorted(c for c in p if 0 <= c < chunks)


class NormCase:
    """The rows of one launch shape (rows, hidden): x, skip (or None), w, and per flat row its kind ('needle', an EDGE_KINDS name or
    'pad') and needle chunk (-1: none).  The flat rows are cut into launches of `rows` rows: the needle rows (padded with zero rows to
    whole launches), then the four edge rows (padded likewise).  Pad rows are never the first rows of a needle launch shape of more
    than 4 rows: rows [0, rows) are row r -> chunk r % chunks."""

    def __init__(self, rows, hidden, skip):
        self.rows, self.hidden, self.has_skip = rows, hidden, bool(skip)
        chunks = self.chunks = hidden // 8
        rng = np.random.default_rng(hidden * 131 + rows * 2 + int(skip))
        # more than 4 rows: row r carries chunk r % chunks (rows >= chunks: every chunk); fewer rows than chunks: further launches
        # with the boundary positions
        pos = [r % chunks for r in range(rows)] if rows > 4 else []
        if rows < chunks or rows <= 4:
            pos += [c for c in needle_positions(chunks) if c not in set(pos)]
        nn = len(pos)
        n_needle_rows = -(-nn // rows) * rows
        n_edge_rows = -(-len(EDGE_KINDS) // rows) * rows
        R = self.R = n_needle_rows + n_edge_rows
        self.kind = np.array(["pad"] * R, dtype=object)
        self.needle = np.full(R, -1, dtype=np.int64)
        x = np.zeros((R, hidden), dtype=np.float16)
        sk = np.zeros((R, hidden), dtype=np.float16)
        # needle rows: background uniform in +-2^-4, one chunk of NEEDLE (skip: a second background of +-2^-6 on every element, so that
        # x + skip needs its rounding everywhere, the needle chunk included)
        x[:nn] = ((rng.random((nn, hidden), dtype=np.float32) * 2 - 1) * np.float32(2.0 ** -4)).astype(np.float16)
        xc = x.reshape(R, chunks, 8)
        xc[np.arange(nn), pos] = NEEDLE
        if skip:
            sk[:nn] = ((rng.random((nn, hidden), dtype=np.float32) * 2 - 1) * np.float32(2.0 ** -6)).astype(np.float16)
            # (in the needle chunk just over half an ulp of the needle, alternately up and down: x + skip is rounded by the most there is)
            sk.reshape(R, chunks, 8)[np.arange(nn), pos] = ((2.0 ** -11 + 2.0 ** -15) * np.array([1, -1, 1, -1, 1, -1, 1, -1])).astype(np.float16)
        self.kind[:nn] = "needle"
        self.needle[:nn] = pos
        # edge rows
        e0 = n_needle_rows
        sign = np.where(rng.integers(0, 2, size=hidden) == 1, 1.0, -1.0)
        bg = (rng.uniform(-1, 1, size=hidden) * 2.0 ** -4).astype(np.float16)
        bg2 = (rng.uniform(-1, 1, size=hidden) * 2.0 ** -6).astype(np.float16)
        # zero: the output is 0 because of eps
        # big: +-60000, squares near 3.6e9, ss up to 5.9e13 -- finite in fp32 (the skip is absorbed by the rounding)
        x[e0 + 1] = (60000.0 * sign).astype(np.float16)
        sk[e0 + 1] = bg2 if skip else 0
        # cancel: x + skip is exactly zero in every even chunk (no skip: x is zero there)
        even = (np.arange(hidden) // 8) % 2 == 0
        x[e0 + 2] = bg
        x[e0 + 2].reshape(chunks, 8)[min(1, chunks - 1)] = NEEDLE
        if skip:
            sk[e0 + 2] = np.where(even, -x[e0 + 2].astype(np.float32), bg2.astype(np.float32)).astype(np.float16)
        else:
            x[e0 + 2][even] = 0
        # tiny: a needle row scaled by 2^-9 -- mean(x^2) is of the order of eps or far below it, eps decides the output
        x[e0 + 3] = (bg.astype(np.float32) * 2.0 ** -9).astype(np.float16)
        x[e0 + 3].reshape(chunks, 8)[chunks // 2] = (NEEDLE.astype(np.float32) * 2.0 ** -9).astype(np.float16)
        sk[e0 + 3] = (bg2.astype(np.float32) * 2.0 ** -9).astype(np.float16) if skip else 0
        self.needle[e0 + 3] = chunks // 2
        for i, k in enumerate(EDGE_KINDS):
            self.kind[e0 + i] = k
        self.x, self.skip, self.w = x, (sk if skip else None), norm_weights(hidden)
        self.launches = R // rows
        self.live = np.flatnonzero(self.kind != "pad")        # the rows a reference is computed for (pad rows: output 0)
        if hidden == 16384:   # the needle chunk carries over 40 % of a needle row's energy at the largest hidden
            v = self.residual(np.arange(min(nn, 8))).astype(np.float64).reshape(-1, chunks, 8)
            e = (v * v).sum(-1)
            assert (e[np.arange(len(e)), pos[:len(e)]] / e.sum(-1) > 0.4).all()

    def residual(self, idx=None):
        """x~ = RN16(x + skip) of the flat rows idx (all rows: block by block); x itself without a skip"""
        if self.skip is None:
            return self.x if idx is None else self.x[idx]
        if idx is None:
            out = np.zeros_like(self.x)                     # (pad rows: 0 + 0)
            for i in range(0, len(self.live), BLOCK):
                j = self.live[i:i + BLOCK]
                out[j] = rn16(self.x[j].astype(np.float64) + self.skip[j].astype(np.float64))
            return out
        return rn16(self.x[idx].astype(np.float64) + self.skip[idx].astype(np.float64))


@functools.lru_cache(maxsize=4)
def norm_case(rows, hidden, skip):
    return NormCase(rows, hidden, skip)


MUTANTS = ("drop_needle", "drop_other", "div_h8", "no_eps", "skip_unrounded", "swap_lanes", "w_shift")


def mutant_applies(mutant, case):
    if mutant in ("drop_other", "w_shift"):
        return case.chunks > 1          # one chunk: there is no other chunk, and a shift by a chunk is the identity
    if mutant == "skip_unrounded":
        return case.has_skip
    return True


def ref_rmsnorm_rows(case, rows_idx, mutant=None):
    """float64 y of the flat rows `rows_idx` of a NormCase (mutant: a subtly wrong kernel, see MUTANTS)"""
    idx = np.asarray(rows_idx)
    x = case.x[idx].astype(np.float64)
    if case.skip is not None:
        s = x + case.skip[idx].astype(np.float64)
        v = s if mutant == "skip_unrounded" else rn16(s).astype(np.float64)
    else:
        v = x
    h, chunks = case.hidden, case.chunks
    vc = v.reshape(len(idx), chunks, 8)
    ss = (vc * vc).sum(-1)                                   # per chunk
    tot = ss.sum(-1)
    nd = np.where(case.needle[idx] >= 0, case.needle[idx], 0)
    ar = np.arange(len(idx))
    if mutant == "drop_needle":
        tot = tot - ss[ar, nd]
    elif mutant == "drop_other":
        tot = tot - ss[ar, (nd + 1) % chunks]
    div = float(h - 8) if mutant == "div_h8" else float(h)
    w = case.w.astype(np.float64)
    if mutant == "w_shift":
        w = np.roll(w, 8)
    if mutant == "swap_lanes":
        vc = vc.copy()
        a, b = SWAP_LANES
        vc[ar, nd, a], vc[ar, nd, b] = vc[ar, nd, b].copy(), vc[ar, nd, a].copy()
        v = vc.reshape(len(idx), h)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v * w / np.sqrt(tot / div + (0.0 if mutant == "no_eps" else EPS64))[:, None]


def interval(y, delta=DELTA):
    a, b = rn16(y * (1 - delta)).astype(np.float32), rn16(y * (1 + delta)).astype(np.float32)
    return np.minimum(a, b), np.maximum(a, b)


def violations(got16, y, delta=DELTA):
    """boolean mask: got is not an fp16 number inside the interval of y (a NaN never is)"""
    lo, hi = interval(y, delta)
    g = np.asarray(got16, dtype=np.float16).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return ~((g >= lo) & (g <= hi))


def needed_delta(got16, y):
    """the smallest d for which `got` lies in the interval of y, in units of DELTA (0: got == RN16(y)): the distance from y to the set
    of reals that round to `got`, relative to |y|"""
    g16 = np.asarray(got16, dtype=np.float16)
    g = g16.astype(np.float64)
    up = np.nextafter(g16, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(g16, np.float16(-np.inf)).astype(np.float64)
    d = np.maximum(0.0, np.maximum((g + dn) / 2 - y, y - (g + up) / 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(y != 0, d / np.abs(y), np.where(g == 0, 0.0, np.inf))
    return np.where(np.isnan(g), np.inf, r) / DELTA


def check_norm_rows(case, rows_idx, got16, mutant=None):
    """(rows with a violation [bool per row], largest needed_delta) of device / emulated rows against the (mutated) reference.  An
    output equal to RN16(y) is inside the interval (rounding is monotonic) at distance 0: only the others are looked at more closely"""
    idx = np.asarray(rows_idx)
    bad = np.zeros(len(idx), dtype=bool)
    worst = 0.0
    for i in range(0, len(idx), BLOCK):
        y = ref_rmsnorm_rows(case, idx[i:i + BLOCK], mutant)
        g = np.asarray(got16[i:i + BLOCK], dtype=np.float16)
        with np.errstate(invalid="ignore"):
            r, c = np.nonzero(g.astype(np.float32) != rn16(y).astype(np.float32))      # (a NaN differs from everything)
        if len(r) == 0:
            continue
        v = violations(g[r, c], y[r, c])
        bad[i + np.unique(r[v])] = True
        if mutant is None:
            worst = max(worst, float(needed_delta(g[r, c], y[r, c]).max()))
    return bad, worst


def emulate_form(res16, w16, maxc, nt, hidden):
    """the kernel's arithmetic in numpy float32, in the form's own summation order: thread t sums chunks t, t + NT, ... lane by lane,
    a 64-lane xor butterfly, then the per-wave partials in order; out = fp16(v * inv * w)"""
    f32 = np.float32
    v = np.asarray(res16, dtype=np.float16).astype(f32)
    R, chunks = v.shape[0], hidden // 8
    vp = np.zeros((R, maxc * nt, 8), dtype=f32)
    vp[:, :chunks] = v.reshape(R, chunks, 8)
    vp = vp.reshape(R, maxc, nt, 8)
    ss = np.zeros((R, nt), dtype=f32)
    for i in range(maxc):
        for j in range(8):
            ss = ss + vp[:, i, :, j] * vp[:, i, :, j]
    ss = ss.reshape(R, nt // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[:, :, lane ^ o]
    red = ss[:, :, 0]
    tot = red[:, 0] + red[:, 1] + red[:, 2] + red[:, 3]
    for k in range(4, nt // 64):
        tot = tot + red[:, k]
    inv = f32(1.0) / np.sqrt(tot / f32(hidden) + f32(EPS))
    assert inv.dtype == np.float32
    return ((v * inv[:, None]) * np.asarray(w16, dtype=np.float16).astype(f32)[None, :]).astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------
# split-K slabs
# ---------------------------------------------------------------------------------------------------------------
MAX_SLABS = 8


def slab_reduce(ws, splits, scale=None):
    """fp16((sum z = 0, 1, ... of ws[z], float32, in that order) * float32(scale[n])): the IEEE operation sequence of the device (an add
    followed by a multiply cannot be contracted), hence bit-exact"""
    ws = np.asarray(ws)
    assert ws.dtype == np.float32
    acc = ws[0].copy()
    for z in range(1, splits):
        acc = acc + ws[z]
    if scale is not None:
        acc = acc * np.asarray(scale, dtype=np.float16).astype(np.float32)[None, :]
    assert acc.dtype == np.float32
    return acc.astype(np.float16)


def build_slabs(M, N, splits, with_scale, seed=0):
    """(ws float32 [MAX_SLABS, M, N], scale fp16 [N] or None): `splits` live slabs, the rest NaN.  Half of the elements carry +B in one
    slab and -B in another, B of 2^13 .. 2^17, beside terms of order 1: what is added between the two is rounded to ulp(B), so the
    result depends on the order of the sum (asserted for splits >= 3: a reversed order changes at least 1 % of the fp16 results)."""
    rng = np.random.default_rng(seed * 977 + M * 31 + N + splits * 7 + int(with_scale))
    ws = np.full((MAX_SLABS, M, N), np.nan, dtype=np.float32)
    live = rng.standard_normal((splits, M, N)).astype(np.float32)
    if splits >= 2:
        paired = rng.random((M, N)) < 0.5
        p = rng.integers(0, splits, size=(M, N))
        q = (p + rng.integers(1, splits, size=(M, N))) % splits
        B = (rng.uniform(1, 2, size=(M, N)) * 2.0 ** rng.integers(13, 17, size=(M, N))).astype(np.float32)
        mi, ni = np.nonzero(paired)
        live[p[mi, ni], mi, ni] = B[mi, ni]
        live[q[mi, ni], mi, ni] = -B[mi, ni]
    ws[:splits] = live
    scale = (0.5 + rng.random(N)).astype(np.float16) if with_scale else None
    if splits >= 3:
        fwd, rev = slab_reduce(live, splits, scale), slab_reduce(live[::-1], splits, scale)
        assert (fwd.view(np.uint16) != rev.view(np.uint16)).mean() >= 0.01
    return ws, scale


# ---------------------------------------------------------------------------------------------------------------
# KV-cache write: quantisation edge rows
# ---------------------------------------------------------------------------------------------------------------
def kv_edge_head_rows(D):
    """fp16 head rows [n, D] for the k / v heads of a token at position 0 (RoPE is the identity there): per cache format the groups
    where a writer goes wrong.  No inf, no NaN.
      0 zero            every format's all-zero group (int8: scale 0, codes 0; fp8: e = -15; int4: scale 2^-14, nibbles 8)
      1 denormal        k 2^-24, k <= 40: int8 max / 127 < 2^-25 rounds to an fp16 scale of 0, codes 0; fp8 (e = -15): x 2^15 = k 2^-9 is
                        every fp8 subnormal and, from k = 17 on, odd k are ties between two codes; int4: codes 0
      2 int8 ties       max 127 / 8 exactly: scale 2^-3, x * inv = k + 0.5 exactly (ties to even), +-127 exactly
      3 int4 floor ties (k + 0.5) 2^-14 under the scale floor 2^-14
      4 int4 ties       max 7 / 8 exactly: scale 2^-3, x * inv = k + 0.5, +-7 exactly
      5 fp8 ties        max 448 exactly (e = 0, code 0x7e), odd integers in [16, 32) and multiples of 2 in [32, 64): ties at e = 0
      6 big             up to +-60000 (fp8 e = 8: saturation at 240; int4 scale 60000 / 7 below the 9344 cap)
    """
    n8 = D // 8
    rows = np.zeros((7, D), dtype=np.float64)
    rows[1] = (np.arange(D) % 41) * 2.0 ** -24
    rows[1, 1::2] *= -1
    g = np.array([127, 0.5, 1.5, 2.5, -3.5, -0.5, 100.5, -126.5]) / 8.0
    rows[2] = np.tile(g, n8)
    rows[2, 8] = -127 / 8.0
    k7 = (np.arange(D) % 7) + 0.5
    sg = np.where(np.arange(D) % 3 == 0, -1.0, 1.0)
    rows[3] = k7 * sg * 2.0 ** -14
    rows[4] = k7 * sg / 8.0
    rows[4, 0::32] = 7 / 8.0
    rows[4, 5::32] = -7 / 8.0
    t = np.array([17, -19, 21, 23, -25, 27, 29, 31, 34, -38, 42, 46, -50, 54, 58, 62], dtype=np.float64)
    rows[5] = np.tile(t, D // 16)
    rows[5, 0], rows[5, 3] = 448, -448
    rng = np.random.default_rng(D)
    rows[6] = rng.uniform(-60000, 60000, size=D)
    rows[6, 7], rows[6, D - 1] = 60000, -60000
    h = rows.astype(np.float16)
    assert (h.astype(np.float64)[:6] == rows[:6]).all() and np.isfinite(h.astype(np.float32)).all()
    return h


def ragged_batch(n_decode, prefill_lens):
    """seq lens of a step: decode rows first (one token each), then prefill requests"""
    return [1] * n_decode + list(prefill_lens)


# ---------------------------------------------------------------------------------------------------------------
# the real producer: launch_linear with a non-null `defer`
# ---------------------------------------------------------------------------------------------------------------
DEFER_WS_BYTES = 64 << 20
DEFER_WQ = [(0, 128), (8, 128), (4, 128)]                 # (wq_bit, group): W16, W8 (the slab scale is set), W4
# (M, N, K) -> the split count of the deferred route per wq_bit, as the dispatcher decides them with DEFER_WS_BYTES of workspace (pinned by
# tests/test_row_ops_spec.py from the route text; 2, 5, 4 and 8 are all present)
DEFER_SHAPES = {
    (5, 1024, 4096): {0: 4, 8: 8, 4: 4},
    (65, 1024, 4096): {0: 4, 8: 8, 4: 4},
    (129, 2048, 8192): {0: 8, 8: 8, 4: 8},
    (33, 1024, 2048): {0: 2, 8: 8, 4: 2},
    (8, 5120, 5120): {0: 5, 8: 6, 4: 5},
}
ROPE_GEOMETRY = {1024: (4, 2, 128), 2048: (8, 4, 128)}    # N = (H + 2 Hkv) D -> (H, Hkv, D); other N feed the norm only


def route_splits(route):
    toks = dict(t.split("=", 1) for t in route.split() if "=" in t)
    return int(toks["splits"]), toks["reduce"]
