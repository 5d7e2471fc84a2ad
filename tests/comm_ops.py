"""Host references, case builders and the checker for the direct collectives of csrc/k_comm.hip as operators (pplhip_comm_op): the
all-reduce, the all-reduce fused with the residual add and the RMSNorm, and the all-gather.  Pure numpy, no device:
tests/test_gpu_comm_ops.py runs the cases on the GPU, tests/test_comm_ops_spec.py checks on the CPU that the cases reach every class named
below and that the checker rejects a subtly wrong kernel.

References (none of them shares code with the kernels):
  all-reduce   want = fp16(fp32 sum in rank order 0 .. n-1): sequential np.float32 additions from +0, one astype(np.float16).  Bit exact.
               exact = fp16(float64 sum) (a float64 sum of <= 8 fp16 numbers is exact) is what the value families are judged by, not the
               kernel.
  fused form   s as above; r = fp16(np.float32(h) + np.float32(s)), bit exact, in the residual rows h of the row's owner;
               y = r w / sqrt(mean(r^2) + eps) in float64, and the device's y must be an fp16 number in
               [RN16(y (1 - d)), RN16(y (1 + d))], d = row_ops.DELTA = 2^-16 (the interval checker of tests/row_ops.py on x~ = r).
               Where d comes from for THIS kernel (u = 2^-24, one fp32 rounding): a thread squares and adds at most 16 values (2 chunks of
               8: 16 products, 16 additions), the wave adds in 6 shuffle steps, 8 wave partials are added in 7 steps -- a sum of positive
               terms in which every term passes through at most 1 + 16 + 6 + 7 = 30 roundings, so ss is within 30 u of the exact sum,
               relatively.  inv = 1 / sqrt(ss / hidden + eps): the root halves the 30 u and the roundings of the division and of the sum
               with eps (15 u + u), the root and the reciprocal add one each: under 18 u.  The products r * inv * w add two: under 20 u =
               2^-16 * 0.08.  (row_ops derived the same d for up to 100 roundings in the sum; this kernel stays inside that count.)
  all-gather   a bit copy: columns [r cols, (r + 1) cols) of every target row are rank r's shard row.

Value families of the sum: "exact" (multiples of 1/4 in [-8, 8): every order and precision gives the same bits, want == exact),
"random" (every finite fp16 bit pattern, with subnormal inputs and results, -0.0, total cancellation and sums that overflow to +-inf
planted in the first and the last granule) and "needles": per rank count, element vectors on which the documented arithmetic and its
neighbours part -- want != exact (the fp32 sum lands on an fp16 tie that the float64 sum misses; for 8 ranks 32768, 16 and 2^-9 on the
other six give 32768 in rank order and 32800 exactly), want != the reverse rank order, != the adjacent-pairs tree, != fp16 accumulation.
What cannot exist: with TWO ranks a sum has one addition, so every order and the tree are the same function, and fp32 holds the sum of
two fp16 numbers exactly wherever the fp16 rounding could tell (the smaller one's last bit is 2^-21 of the larger at a tie, fp32 keeps
2^-23), so want == exact == fp16 accumulation for every input; with THREE ranks the adjacent-pairs tree (x0 + x1) + x2 IS the rank
order.  NEEDLE_KINDS says which needles a rank count has; test_comm_ops_spec.py checks the claims above by search.

The mirror of the kernels' slice and grid arithmetic (ar_geometry, fused_geometry, gather_granule) only CLASSIFIES cases (which ranks own
nothing, how many blocks, how many trips); no expected value comes from it except the owner of a residual row, which is the documented
contract (rank r owns rows [r per, (r + 1) per), per = ceil(rows / n)).
"""
import functools

import numpy as np

from tests import row_ops as R

RANKS = (2, 3, 4, 5, 6, 7, 8)
AR, FUSED, GATHER = 0, 1, 2                     # pplhip.COMM_ALLREDUCE, COMM_ALLREDUCE_NORM, COMM_ALLGATHER
BLOCK_CAP, THREADS, GRANULES_PER_BLOCK = 32, 512, 512 * 8
CANARY16 = np.uint16(0x5AC3)                    # a finite fp16 nothing computes
CANARY32 = np.uint32(0x7FC5A5A5)                # a NaN payload: a canary that was "copied" through a float would still be seen
PAD = 64                                        # canary elements behind every image
FUSED_WIDTHS = (8, 4096, 4104, 5120, 8184, 8192)
GATHER_COLS = (2, 4, 6, 1026)
EPS = R.EPS


def bits16(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---------------------------------------------------------------------------------------------------------------
# the arithmetic: the reference and its wrong neighbours
# ---------------------------------------------------------------------------------------------------------------
def _f16(a32):
    with np.errstate(over="ignore"):
        return a32.astype(np.float16)


def sum_rank_order(X, ranks=None):
    """X fp16 [n, ...] -> fp32 sum, rank 0 first, from +0 (ranks: the order, default 0 .. n-1)"""
    acc = np.zeros(X.shape[1:], dtype=np.float32)
    for r in (range(X.shape[0]) if ranks is None else ranks):
        acc = acc + X[r].astype(np.float32)
    return acc


def sum_tree(X):
    """adjacent pairs, level by level (an odd one out moves up unchanged), in fp32"""
    level = [X[r].astype(np.float32) for r in range(X.shape[0])]
    while len(level) > 1:
        level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
    return level[0]


def sum_f16(X):
    acc = np.zeros(X.shape[1:], dtype=np.float16)
    with np.errstate(over="ignore"):
        for r in range(X.shape[0]):
            acc = (acc + X[r]).astype(np.float16)
    return acc


SUM_MUTANTS = ("reverse", "tree", "f16acc", "drop_rank")


def reduce16(X, mutant=None):
    """the all-reduce's result fp16 [...] (mutant: a wrong kernel)"""
    n = X.shape[0]
    if mutant == "reverse":
        return _f16(sum_rank_order(X, range(n - 1, -1, -1)))
    if mutant == "tree":
        return _f16(sum_tree(X))
    if mutant == "f16acc":
        return sum_f16(X)
    if mutant == "drop_rank":
        return _f16(sum_rank_order(X, range(n - 1)))
    return _f16(sum_rank_order(X))


def exact16(X):
    return _f16(X.astype(np.float64).sum(0))


# ---------------------------------------------------------------------------------------------------------------
# needles
# ---------------------------------------------------------------------------------------------------------------
def NEEDLE_KINDS(n):
    """which of (exact, reverse, tree, f16acc) a needle of n ranks can part from `want` (module docstring)"""
    if n == 2:
        return ()
    return ("exact", "reverse", "f16acc") if n == 3 else ("exact", "reverse", "tree", "f16acc")


def _needle_pool(n, m, rng):
    """m candidate vectors fp16 [n, m]: signed powers of two (and 1.5 x) from 2^-14 to 2^15, a quarter of them zero.  All finite, so
    no order of additions makes a NaN"""
    k = rng.randint(-14, 16, size=(n, m))
    v = np.ldexp(np.where(rng.rand(n, m) < 0.3, 1.5, 1.0), k) * np.where(rng.rand(n, m) < 0.5, -1.0, 1.0)
    v[rng.rand(n, m) < 0.25] = 0.0
    return v.astype(np.float16)


@functools.lru_cache(maxsize=None)
def needles(n):
    """fp16 [n, k]: columns are element vectors; for every kind of NEEDLE_KINDS(n) at least four columns part `want` from it, and every
    column has a finite `want` of magnitude <= 40000 (the fused cases add a residual to it).  The first column, from 3 ranks on, is the
    example of the issue: 32768, 16, 2^-9 on the others."""
    if not NEEDLE_KINDS(n):
        return np.zeros((n, 0), dtype=np.float16)
    rng = np.random.RandomState(1000 + n)
    pool = _needle_pool(n, 40000, rng)
    first = np.full((n, 1), 2.0 ** -9, dtype=np.float16)
    first[0, 0], first[1, 0] = 32768.0, 16.0
    # fp16 accumulation loses every addend of half an ulp: 1, 2^-11, 2^-11, ...
    second = np.full((n, 1), 2.0 ** -11, dtype=np.float16)
    second[0, 0] = 1.0
    pool = np.concatenate([first, second, pool], axis=1)
    want = reduce16(pool)
    ok = np.isfinite(want) & (np.abs(want.astype(np.float32)) <= 40000)
    other = {"exact": exact16(pool), "reverse": reduce16(pool, "reverse"), "tree": reduce16(pool, "tree"), "f16acc": reduce16(pool, "f16acc")}
    cols = [0, 1]
    for kind in NEEDLE_KINDS(n):
        hit = np.nonzero(ok & (bits16(want) != bits16(other[kind])))[0]
        assert len(hit) >= 4, (n, kind)
        cols += list(hit[:4])
    cols = sorted(set(cols))
    assert ok[cols].all()
    return np.ascontiguousarray(pool[:, cols])


# ---------------------------------------------------------------------------------------------------------------
# the mirror: slices and grids (classification only)
# ---------------------------------------------------------------------------------------------------------------
def slices(n, units):
    """[(lo, hi)] per rank over `units` granules or rows; hi <= lo: the rank owns nothing"""
    per = -(-units // n)
    return per, [(per * r, min(per * r + per, units)) for r in range(n)]


def ar_geometry(n, granules):
    per, sl = slices(n, granules)
    blocks = min(BLOCK_CAP, max(1, -(-per // GRANULES_PER_BLOCK)))
    return dict(per=per, slices=sl, blocks=blocks, trips=-(-per // (blocks * THREADS)))


def fused_geometry(n, rows, hidden):
    per, sl = slices(n, rows)
    blocks = min(BLOCK_CAP, per)
    chunks = hidden // 8
    return dict(per=per, slices=sl, blocks=blocks, trips=-(-per // blocks), chunks=chunks,
                second_chunk=chunks > THREADS, clamped=chunks % THREADS != 0)


def gather_granule(cols, stride):
    return 16 if cols % 4 == 0 and stride % 4 == 0 else 8


def slice_classes(n, units):
    """names of the ragged-slice classes a shape of `units` granules / rows reaches"""
    per, sl = slices(n, units)
    out = set()
    if any(hi <= lo for lo, hi in sl):
        out.add("rank_owns_nothing")
    if any(0 < hi - lo < per for lo, hi in sl):
        out.add("short_last_slice")
    if per * n > units:
        out.add("past_the_end")
    if units == n * (per - 1) + 1 and per >= 2:
        out.add("one_in_last_row_of_slices")
    return out


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
class Case:
    """kind AR: granules, family; FUSED: rows, hidden, family; GATHER: rows, cols, stride.  build() -> the per-rank inputs (fresh
    arrays, deterministic)."""

    def __init__(self, kind, n, name, seed, **kw):
        self.kind, self.n, self.name, self.seed = kind, n, name, seed
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name

    # -- sizes --
    @property
    def count(self):
        return self.granules * 8

    def data_bytes(self):
        """of the collective's data buffer (gather: of the source)"""
        return {AR: lambda: (self.count + PAD) * 2, FUSED: lambda: self.rows * self.hidden * 2, GATHER: lambda: self.rows * self.cols * 4}[self.kind]()

    def image_elems(self):
        if self.kind == FUSED:
            return (self.rows + 2) * self.hidden + PAD
        return (self.rows - 1) * self.stride + self.n * self.cols + PAD

    def classes(self):
        if self.kind == AR:
            g = ar_geometry(self.n, self.granules)
            out = slice_classes(self.n, self.granules) | {"family_" + self.family}
            if g["blocks"] == 2:
                out.add("two_blocks")
            if g["blocks"] == BLOCK_CAP and g["trips"] > 1:
                out.add("block_cap_and_trips")
            return out
        if self.kind == FUSED:
            g = fused_geometry(self.n, self.rows, self.hidden)
            out = slice_classes(self.n, self.rows) | {"hidden_%d" % self.hidden, "rows_%s" % self.rows_tag}
            if g["per"] > BLOCK_CAP:
                out.add("per_above_block_cap")
            return out
        return {"granule_%d" % gather_granule(self.cols, self.stride), "cols_%d" % self.cols, "rows_%d" % self.rows,
                "stride_wide" if self.stride > self.n * self.cols else "stride_tight"}

    # -- inputs --
    def _sum_values(self, rng, shape_tail, family):
        """fp16 [n, *shape_tail] of a value family; the flat element index runs over shape_tail"""
        n = self.n
        size = int(np.prod(shape_tail))
        if family == "exact":
            X = (rng.randint(-32, 32, size=(n, size)) * 0.25).astype(np.float16)
        elif family == "needles":
            nd = needles(n)
            X = nd[:, np.arange(size) % nd.shape[1]].copy()
        else:
            b = rng.randint(0, 1 << 16, size=(n, size)).astype(np.uint16)
            inf_nan = (b & 0x7C00) == 0x7C00
            b[inf_nan] &= np.uint16(0xFBFF)                      # exponent 30: finite
            X = b.view(np.float16)
            if family == "moderate":                             # (the fused form: the residual must stay finite)
                X = (X.astype(np.float32) * np.float32(2.0 ** -6)).astype(np.float16)   # |x| < 1024, many subnormals
            sp = self._specials(family)
            for base in (0, size - 8):
                X[:, base:base + 8] = sp
            if family == "mixed":
                nd = needles(n)
                if nd.shape[1]:
                    idx = np.arange(8 + 3, size - 8, 5)
                    X[:, idx] = nd[:, idx % nd.shape[1]]
                idx = np.arange(8 + 1, size - 8, 11)
                X[:, idx] = (rng.randint(-32, 32, size=(n, len(idx))) * 0.25).astype(np.float16)
        return np.ascontiguousarray(X.reshape((n,) + tuple(shape_tail)))

    def _specials(self, family):
        """fp16 [n, 8]: subnormal inputs and result | -0.0 everywhere | total cancellation | overflow to +inf | to -inf | a subnormal
        result of normal inputs | 65504 + 16: the tie below infinity | -0.0 with +0.0.  (moderate: the overflows become large finite sums)"""
        n = self.n
        sp = np.zeros((n, 8), dtype=np.float16)
        sp[:, 0] = (np.arange(n) + 1) * 2.0 ** -24
        sp[:, 1] = -0.0
        sp[0, 2], sp[1, 2] = 1234.0, -1234.0
        big = 65504.0 if family != "moderate" else 8192.0
        sp[0, 3], sp[1, 3] = big, big
        sp[0, 4], sp[1, 4] = -big, -big
        sp[0, 5], sp[1, 5] = 1.5 * 2.0 ** -14, -(2.0 ** -14)
        sp[0, 6], sp[1, 6] = big, 16.0
        sp[::2, 7] = -0.0
        return sp

    def build(self):
        rng = np.random.RandomState(self.seed)
        n = self.n
        if self.kind == AR:
            data = np.full((n, self.count + PAD), 0, dtype=np.float16)
            data[:, :self.count] = self._sum_values(rng, (self.count,), self.family)
            bits16(data)[:, self.count:] = CANARY16
            return dict(data=data)
        if self.kind == FUSED:
            rows, hd = self.rows, self.hidden
            part = self._sum_values(rng, (rows, hd), self.family)
            h = (rng.standard_normal((n, rows, hd)) * 0.5).astype(np.float16)     # every rank its own residual rows
            # where fp16(h + sum) and fp16(h + fp16(sum)) part: sum = 1 + 2^-11 (rounds to 1), h = 2^-11
            cols = np.arange(0, hd, 24)
            part[:, :, cols] = 0
            part[0][:, cols], part[1][:, cols] = 1.0, 2.0 ** -11
            h[:, :, cols] = 2.0 ** -11
            w = np.broadcast_to(R.norm_weights(hd), (n, hd)).copy()
            ie = self.image_elems()
            himg = np.full((n, ie), 0, dtype=np.float16)
            bits16(himg)[:] = CANARY16
            himg[:, :rows * hd] = h.reshape(n, -1)
            ximg = np.full((n, ie), 0, dtype=np.float16)
            bits16(ximg)[:] = CANARY16
            return dict(data=part.reshape(n, -1), h=himg, xn=ximg, w=w)
        rows, cols = self.rows, self.cols
        shard = rng.randint(0, 1 << 32, size=(n, rows, cols), dtype=np.uint64).astype(np.uint32)
        shard[:, 0, 0] = 0x7FC00001 + np.arange(n)                               # NaN payloads
        shard[:, -1, -1] = 0xFFFFFFFF
        target = np.full((n, self.image_elems()), CANARY32, dtype=np.uint32)
        return dict(data=shard.reshape(n, -1), target=target)

    def item(self, inp, **kw):
        """the dict pplhip.Context.comm_op takes"""
        n = self.n
        d = dict(kind=self.kind, data=[inp["data"][r] for r in range(n)], **kw)
        if self.kind == AR:
            d.update(count=self.count)
        elif self.kind == FUSED:
            d.update(rows=self.rows, hidden=self.hidden, eps=EPS, h=[inp["h"][r] for r in range(n)], xn=[inp["xn"][r] for r in range(n)],
                     w=[inp["w"][r] for r in range(n)])
        else:
            d.update(rows=self.rows, cols=self.cols, dst_stride=self.stride, target=[inp["target"][r] for r in range(n)])
        return d


def ar_granules(n):
    """{name: granules}: the smallest shapes that reach each class"""
    g = {"one": 1, "n-1": n - 1, "n": n, "n+1": n + 1, "n(per-1)+1": 2 * n + 1, "n*per-1": 3 * n - 1, "two_blocks": n * GRANULES_PER_BLOCK + 1}
    if n == 2:
        del g["n-1"]                                # (1 again)
    if n in (2, 8):
        g["block_cap"] = n * (BLOCK_CAP - 1) * GRANULES_PER_BLOCK + 1
    return g


def fused_rows(n):
    rw = {"one": 1, "n-1": n - 1, "n": n, "n+1": n + 1, "33n-1": 33 * n - 1}
    if n == 2:
        del rw["n-1"]                               # (1 again)
    return rw


def fused_shapes(n):
    """[(rows tag, rows, hidden)]: every rows value at the widths 8 and 4104, every width at n and n + 1 rows"""
    rw = fused_rows(n)
    out = []
    for tag, rows in rw.items():
        for hd in (8, 4104):
            out.append((tag, rows, hd))
    for hd in FUSED_WIDTHS:
        for tag in ("n", "n+1"):
            if (tag, rw[tag], hd) not in out:
                out.append((tag, rw[tag], hd))
    return out


FUSED_FAMILIES = ("exact", "moderate", "needles")


@functools.lru_cache(maxsize=None)
def cases(n):
    out = []
    seed = n * 10000
    for tag, g in ar_granules(n).items():
        fams = ("mixed",) if tag in ("two_blocks", "block_cap") else ("exact", "random") + (("needles",) if NEEDLE_KINDS(n) else ())
        for fam in fams:
            seed += 1
            out.append(Case(AR, n, "ar_n%d_%s_%s" % (n, tag, fam), seed, granules=g, family=fam, tag=tag))
    for i, (tag, rows, hd) in enumerate(fused_shapes(n)):
        fam = FUSED_FAMILIES[i % 3]
        if fam == "needles" and not NEEDLE_KINDS(n):
            fam = "moderate"
        seed += 1
        out.append(Case(FUSED, n, "fused_n%d_rows_%s_h%d_%s" % (n, tag, hd, fam), seed, rows=rows, hidden=hd, family=fam, rows_tag=tag))
    for cols in GATHER_COLS:
        for rows in (1, 5):
            for pad in (0, 4):
                seed += 1
                out.append(Case(GATHER, n, "gather_n%d_r%d_c%d_pad%d" % (n, rows, cols, pad), seed, rows=rows, cols=cols, stride=n * cols + pad))
    seed += 1
    out.append(Case(GATHER, n, "gather_n%d_r5_c4_pad2" % n, seed, rows=5, cols=4, stride=n * 4 + 2))   # 16-byte rows on an 8-byte stride
    return out


def all_cases():
    return [c for n in RANKS for c in cases(n)]


def small(case):
    """cheap enough for the CPU tests to run every mutant on"""
    return case.data_bytes() <= (1 << 20)


# ---------------------------------------------------------------------------------------------------------------
# expected outputs (mutant: what a wrong kernel would leave) and the checker
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = SUM_MUTANTS + ("no_inner_rounding", "boundary_off_by_one", "skip_last_partial_slice", "h_rows_overwritten", "swap_8_in_16")


def mutant_applies(mutant, case):
    n = case.n
    if mutant in ("reverse", "tree", "f16acc"):
        return case.kind in (AR, FUSED) and case.family in ("needles", "mixed") and mutant in NEEDLE_KINDS(n)
    if mutant == "drop_rank":
        return case.kind in (AR, FUSED)
    if mutant == "no_inner_rounding" or mutant == "h_rows_overwritten":
        return case.kind == FUSED
    units = case.granules if case.kind == AR else case.rows
    if mutant == "boundary_off_by_one":
        return case.kind in (AR, FUSED) and units > slices(n, units)[0]          # a second slice exists
    if mutant == "skip_last_partial_slice":
        return case.kind in (AR, FUSED) and "short_last_slice" in slice_classes(n, units)
    if mutant == "swap_8_in_16":
        return case.kind == GATHER and case.cols % 4 == 0
    return False


def emulate(case, inp, mutant=None):
    """what the documented arithmetic (or a mutant of it) leaves on every rank, as pplhip.Context.comm_op returns it: AR: [data image per
    rank]; FUSED: [(h image, xn image) per rank], y rounded once from float64; GATHER: [target image per rank]"""
    n = case.n
    if case.kind == GATHER:
        rows, cols, stride = case.rows, case.cols, case.stride
        shard = inp["data"].reshape(n, rows, cols)
        if mutant == "swap_8_in_16":
            shard = shard.reshape(n, rows, cols // 4, 2, 2)[:, :, :, ::-1, :].reshape(n, rows, cols)
        outs = []
        for q in range(n):
            t = inp["target"][q].copy()
            for row in range(rows):
                t[row * stride:row * stride + n * cols] = shard[:, row, :].reshape(-1)
            outs.append(t)
        return outs
    sum_mut = mutant if mutant in SUM_MUTANTS else None
    if case.kind == AR:
        cnt = case.count
        X = inp["data"][:, :cnt]
        res = reduce16(X, sum_mut)
        per, sl = slices(n, case.granules)
        outs = []
        for q in range(n):
            o = inp["data"][q].copy()
            o[:cnt] = res
            if mutant == "boundary_off_by_one":      # the first granule of rank 1's slice is nobody's: the buffer keeps the rank's input
                o[per * 8:per * 8 + 8] = inp["data"][q][per * 8:per * 8 + 8]
            if mutant == "skip_last_partial_slice":
                lo, hi = [s for s in sl if s[1] > s[0]][-1]
                o[lo * 8:hi * 8] = inp["data"][q][lo * 8:hi * 8]
            outs.append(o)
        return outs
    rows, hd = case.rows, case.hidden
    X = inp["data"].reshape(n, rows, hd)
    h = inp["h"][:, :rows * hd].reshape(n, rows, hd)
    per, sl = slices(n, rows)
    owner = np.minimum(np.arange(rows) // per, n - 1)
    if mutant == "no_inner_rounding":
        s32 = sum_rank_order(X)
    else:
        s32 = reduce16(X, sum_mut).astype(np.float32)
    h_own = h[owner, np.arange(rows)]                                            # [rows, hd]: the owner's residual rows
    r16 = _f16(h_own.astype(np.float32) + s32)
    y16 = np.empty((rows, hd), dtype=np.float16)
    for i in range(0, rows, R.BLOCK):
        y16[i:i + R.BLOCK] = R.rn16(fused_y(r16[i:i + R.BLOCK], inp["w"][0]))
    skip = np.zeros(rows, dtype=bool)
    if mutant == "boundary_off_by_one":
        skip[per] = True
    if mutant == "skip_last_partial_slice":
        lo, hi = [s for s in sl if s[1] > s[0]][-1]
        skip[lo:hi] = True
    outs = []
    for q in range(n):
        ho, xo = inp["h"][q].copy(), inp["xn"][q].copy()
        hv, xv = ho[:rows * hd].reshape(rows, hd), xo[:rows * hd].reshape(rows, hd)
        mine = (owner == q) if mutant != "h_rows_overwritten" else np.ones(rows, dtype=bool)
        hv[mine & ~skip] = r16[mine & ~skip]
        xv[~skip] = y16[~skip]
        outs.append((ho, xo))
    return outs


def fused_y(r16, w16):
    """float64 y of residual rows r16 [rows, hidden]"""
    r = r16.astype(np.float64)
    return r * w16.astype(np.float64) / np.sqrt((r * r).mean(-1) + R.EPS64)[:, None]


def _diff(name, got, want, limit=3):
    """[] or one message: where the bits of two arrays differ"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    g, w = g.view(np.uint16 if g.itemsize == 2 else np.uint32).reshape(-1), w.view(np.uint16 if w.itemsize == 2 else np.uint32).reshape(-1)
    if g.shape != w.shape:
        return ["%s: shape %s against %s" % (name, g.shape, w.shape)]
    bad = np.nonzero(g != w)[0]
    if len(bad) == 0:
        return []
    return ["%s: %d of %d differ, first at %s (got %s, want %s)" % (name, len(bad), g.size, bad[:limit].tolist(),
                                                                   [hex(int(v)) for v in g[bad[:limit]]], [hex(int(v)) for v in w[bad[:limit]]])]


def check(case, inp, outs):
    """messages of everything that is wrong with what every rank holds after the collective (empty: all right)"""
    n = case.n
    fails = []
    if len(outs) != n:
        return ["%d outputs for %d ranks" % (len(outs), n)]
    if case.kind in (AR, GATHER):
        want = emulate(case, inp)
        for q in range(n):                                     # every rank, canaries included (they are part of the image)
            fails += _diff("%s rank %d" % (case.name, q), outs[q], want[q])
        for q in range(1, n):
            fails += _diff("%s rank %d against rank 0" % (case.name, q), outs[q][:len(outs[q]) - PAD], outs[0][:len(outs[0]) - PAD]) if case.kind == AR else []
        return fails
    rows, hd = case.rows, case.hidden
    want = emulate(case, inp)
    r16 = np.empty((rows, hd), dtype=np.float16)
    per, sl = slices(n, rows)
    for q in range(n):
        lo, hi = sl[q]
        if hi > lo:
            r16[lo:hi] = want[q][0][lo * hd:hi * hd].reshape(hi - lo, hd)
    assert np.isfinite(r16.astype(np.float32)).all(), case.name           # (the builder keeps the residual finite)
    for q in range(n):
        gh, gx = outs[q]
        # h: owned rows updated, every other row and the canaries as they were -- want[q][0] says exactly that
        fails += _diff("%s h of rank %d" % (case.name, q), gh, want[q][0])
        # xn: canaries and the rows past `rows` untouched, every rank the same bits as rank 0 ...
        fails += _diff("%s xn canaries of rank %d" % (case.name, q), gx[rows * hd:], inp["xn"][q][rows * hd:])
        if q:
            fails += _diff("%s xn of rank %d against rank 0" % (case.name, q), gx, outs[0][1])
    # ... and rank 0's rows inside the interval of the float64 y of the reference residual
    gx = np.asarray(outs[0][1][:rows * hd]).view(np.float16).reshape(rows, hd)
    nbad, first = 0, None
    for i in range(0, rows, R.BLOCK):
        y = fused_y(r16[i:i + R.BLOCK], inp["w"][0])
        g = gx[i:i + R.BLOCK]
        with np.errstate(invalid="ignore"):
            rr, cc = np.nonzero(g.astype(np.float32) != R.rn16(y).astype(np.float32))
        if len(rr):
            v = R.violations(g[rr, cc], y[rr, cc])
            nbad += int(v.sum())
            if v.any() and first is None:
                k = np.nonzero(v)[0][0]
                first = (i + int(rr[k]), int(cc[k]), float(g[rr[k], cc[k]]), float(y[rr[k], cc[k]]))
    if nbad:
        fails.append("%s xn: %d values outside the interval of y, first (row, col, got, y) = %s" % (case.name, nbad, first))
    return fails


# ---------------------------------------------------------------------------------------------------------------
# on the device (tests/test_gpu_comm_ops.py)
# ---------------------------------------------------------------------------------------------------------------
def run_sequence_gpu(ctx, seq, channel=0, skews=None, advances=None):
    """one pplhip_comm_op call for the cases `seq`, back to back -> (status, messages, counters)"""
    inputs = [c.build() for c in seq]
    items = []
    for i, (c, inp) in enumerate(zip(seq, inputs)):
        kw = dict(channel=channel if c.kind != GATHER else 0)
        if skews is not None and skews[i] is not None:
            kw["skew"] = skews[i]
        if advances is not None and advances[i]:
            kw["epoch_advance"] = advances[i]
        items.append(c.item(inp, **kw))
    rc, outs, counters = ctx.comm_op(items)
    if rc:
        return rc, ["status %d: %s" % (rc, ctx.last_error())], counters
    fails = []
    for i, (c, inp) in enumerate(zip(seq, inputs)):
        fails += ["item %d: %s" % (i, f) for f in check(c, inp, outs[i])]
    return 0, fails, counters
