"""Top-N logprobs (csrc/k_logprobs.hip; DESIGN.md "numerics", top-N logprobs row): the reference, the checker and the case builders, shared
by tests/test_top_logprobs_spec.py (no GPU) and the tests/test_gpu_top_logprobs*.py files.

Specification.  Row b with n = num_logprobs[b]: x = fp32(logit * fp32(1 / t)) (postproc.scaled: the sampler's one fp32 step); ranking = x
descending, ties by ascending token index (a float comparison: -0 ties with +0); entry j < min(n, V) = the token of rank j and
x_j - lse, lse = mx + log(sum exp(x - mx)); entries j >= V: token -1, logprob -inf.  The reference forms x in float32 and does everything
after it in float64.  Tokens are compared bit for bit in every entry of every row; there is no uncompared row.

The logprob bound, per entry (u = 2^-24, W = 256 threads of the block, V the vocabulary):

    bound_j = (ceil(V / W) + log2(W) + 2 ln V + C) u  +  2 u |ln S|  +  u |lse|  +  u |logprob_j|            S = sum exp(x - mx), C = 8

  * the mass S.  A thread adds its terms in sequence, at most ceil(V / W) + 2 roundings deep (a 16-byte piece is summed (x + y) + (z + w)
    before it joins the running sum: the + 2), then log2(W) tree steps follow (six in the wave, two across the four waves).  Every rounding
    multiplies a partial sum of positive terms by (1 + d), |d| <= u, so the relative error of S from the additions is at most their depth
    times u.  Every term is exp(a_i) with a_i = x_i - mx: the subtraction rounds (relative u of |a_i|) and the exponential multiplies its
    argument by a rounded log2(e) (another u |a_i|), so term i is off by a factor 1 + 2 u |a_i| and S by the mass-weighted mean of that,
    2 u sum p_i |a_i|.  That mean is at most the entropy: H = sum p_i (lse - x_i) = sum p_i (mx - x_i) + (lse - mx) and lse >= mx; and
    H <= ln V.  C collects what is left: 2 for the depth above, 2 for the exponential instruction (one ulp = at most 2 u), 3 for the
    fp32 constant log2(e) itself (off by 0.22 u relative, times |a_i|, weighted as above: 0.22 ln V <= 3 up to V = 2^19), 1 for the
    second-order terms of all the products.  A relative error e of S is an absolute error e of ln S.
  * logf: faithful, one ulp of |ln S|, at most 2 u |ln S|.
  * mx + ln S: one rounding, u |lse|.   x_j - lse: one rounding, u |logprob_j|.

The same formula with W = 1024 and the greedy kernel's tree (six steps in the wave, then its 16 waves in sequence: 21 steps) bounds
pplhip_op_sample's greedy logprob (greedy_bound), for the comparison of entry 0 against it.

Case construction: in every asked row the ranks 0 .. min(n, V - 1) are pairwise either exactly equal in x or >= 2^-6 apart
(check_assertions), so a swapped pair shows in the logprobs too, at hundreds of times the bound.

Guards, as in tests/postproc.py: rows `stride` >= V apart, +inf behind vocab, in front of a misaligned base and in a canary row behind
the batch; both outputs filled with canaries: the slots of a row behind its n and the rows behind the last asked row must come back
untouched.
"""
import math

import numpy as np

from tests import postproc as P

NMAX = 20                                                # PPLHIP_TOP_LOGPROBS_MAX
W = 256                                                  # TL_THREADS: the block of top_logprobs_row
U = 2.0 ** -24
C_REST = 8
GAP = 2.0 ** -6
TAIL_ROWS = 2                                            # canary rows behind the last asked row of both outputs


def mass_bound(V, width=W, tree_steps=None):
    tree = math.log2(width) if tree_steps is None else tree_steps
    return (math.ceil(V / width) + tree + 2.0 * math.log(V) + C_REST) * U


def entry_bound(V, log_s, lse, lp, width=W, tree_steps=None):
    return mass_bound(V, width, tree_steps) + 2 * U * abs(log_s) + U * abs(lse) + U * abs(lp)


def greedy_bound(V, log_s, lse, lp):
    """pplhip_op_sample with top_k = 1: 1024 threads, six tree steps in the wave and the 16 wave sums in sequence"""
    return entry_bound(V, log_s, lse, lp, width=P.SG_THREADS, tree_steps=6 + 15)


def ref_row(x, n):
    """x: the scaled row (float32) -> (tokens [n] int32, logprobs [n] float64, ln S, lse)"""
    V = x.size
    k = min(n, V)
    order = np.argsort(-x, kind="stable")[:k]            # descending, ties by ascending index; -0 == +0
    mx = float(x.max())
    log_s = float(np.log(np.exp(x.astype(np.float64) - mx).sum()))
    lse = mx + log_s
    tok = np.full(n, -1, dtype=np.int32)
    lp = np.full(n, -np.inf, dtype=np.float64)
    tok[:k] = order
    with np.errstate(invalid="ignore"):
        lp[:k] = x[order].astype(np.float64) - lse
    return tok, lp, log_s, lse


class TCase:
    """one launch of pplhip_op_top_logprobs: B rows of V logits, rows `stride` apart, the base `off` floats past a 16-byte boundary;
    per row num_logprobs (0: the row does not ask) and temperature (temps None: NULL)"""

    def __init__(self, name, family, logits, stride, off, nlp, temps=None):
        self.name, self.family = name, family
        self.logits = np.ascontiguousarray(logits, dtype=np.float32)
        self.B, self.V = self.logits.shape
        self.stride, self.off = stride, off
        self.nlp = np.ascontiguousarray(nlp, dtype=np.int32)
        self.temps = None if temps is None else np.ascontiguousarray(temps, dtype=np.float32)
        assert self.nlp.shape == (self.B,) and (self.temps is None or self.temps.shape == (self.B,))
        self.asked = [b for b in range(self.B) if self.nlp[b] > 0]
        self._ref = None

    def x(self, b):
        return P.scaled(self.logits[b], None if self.temps is None else self.temps[b])

    def uses_vector_path(self):
        return self.stride % 4 == 0 and self.off == 0

    def image(self):
        img = np.full(4 + (self.B + 1) * self.stride + 4, np.inf, dtype=np.float32)
        for b in range(self.B):
            img[self.off + b * self.stride:self.off + b * self.stride + self.V] = self.logits[b]
        return img

    def reference(self):
        """per asked row, in ascending batch row: (tokens [n], logprobs [n] float64, ln S, lse); computed once"""
        if self._ref is None:
            self._ref = [ref_row(self.x(b), int(self.nlp[b])) for b in self.asked]
        return self._ref

    def check_assertions(self):
        assert 0 <= self.off <= 3 and self.stride >= self.V >= 1
        assert ((self.nlp >= 0) & (self.nlp <= NMAX)).all(), self.name
        img = self.image()
        mask = np.ones(img.size, dtype=bool)
        for b in range(self.B):
            mask[self.off + b * self.stride:self.off + b * self.stride + self.V] = False
        assert np.isposinf(img[mask]).all() and mask.sum() == img.size - self.B * self.V, (self.name, "poison")
        assert not np.isnan(self.logits).any() and not np.isposinf(self.logits).any(), self.name
        assert (self.logits.max(axis=1) > -np.inf).all(), (self.name, "a row without a finite entry")
        for b in self.asked:
            x = self.x(b)
            top = x[np.argsort(-x, kind="stable")[:min(int(self.nlp[b]) + 1, self.V)]].astype(np.float64)
            for j in range(1, top.size):
                d = top[j - 1] - top[j] if np.isfinite(top[j]) else (0.0 if np.isneginf(top[j - 1]) else np.inf)
                assert d == 0.0 or d >= GAP, (self.name, b, j, top[j - 1], top[j])
        return self.reference()


def blank_outputs(asked):
    """both outputs as the launch receives them: [asked + TAIL_ROWS, NMAX] of canaries"""
    return (np.full((asked + TAIL_ROWS, NMAX), P.TOK_CANARY, dtype=np.int32), np.full((asked + TAIL_ROWS, NMAX), P.LP_CANARY, dtype=np.uint32))


def check(c, tok, lp_bits):
    """tok int32 / lp_bits uint32, both [asked + TAIL_ROWS, NMAX], as they came back -> (failures, largest |error| / bound over all entries)"""
    fails, frac = [], 0.0
    ref = c.reference()
    A = len(c.asked)
    if tok.shape != (A + TAIL_ROWS, NMAX) or lp_bits.shape != tok.shape:
        return [f"output shape {tok.shape}"], 0.0
    if not (tok[A:] == P.TOK_CANARY).all() or not (lp_bits[A:] == P.LP_CANARY).all():
        fails.append("rows behind the last asked row were written")
    lp = lp_bits.view(np.float32)
    for j, b in enumerate(c.asked):
        n = int(c.nlp[b])
        wtok, wlp, log_s, lse = ref[j]
        if not (tok[j, n:] == P.TOK_CANARY).all() or not (lp_bits[j, n:] == P.LP_CANARY).all():
            fails.append(f"row {b} (n {n}): slots behind n were written")
        bad = np.flatnonzero(tok[j, :n] != wtok)
        if bad.size:
            e = int(bad[0])
            fails.append(f"row {b} (n {n}): entry {e} token {int(tok[j, e])} want {int(wtok[e])} ({bad.size} entries differ)")
            continue
        for e in range(n):
            g, w = float(lp[j, e]), float(wlp[e])
            if np.isneginf(w):
                if not np.isneginf(g):
                    fails.append(f"row {b} (n {n}): entry {e} logprob {g!r} want -inf")
                continue
            bound = entry_bound(c.V, log_s, lse, w)
            err = abs(g - w)
            if not err <= bound:
                fails.append(f"row {b} (n {n}): entry {e} logprob {g!r} want {w!r}: off by {err:.3g}, bound {bound:.3g}")
            else:
                frac = max(frac, err / bound)
    return fails, frac


def launch(m, torch, c):
    """the case through pplhip_op_top_logprobs: (rc, tokens, logprob bits), both [asked + TAIL_ROWS, NMAX]"""
    d = torch.from_numpy(c.image()).cuda()
    assert d.data_ptr() % 16 == 0
    d_t = None if c.temps is None else torch.from_numpy(c.temps).cuda()
    d_n = torch.from_numpy(c.nlp).cuda()
    tok0, lp0 = blank_outputs(len(c.asked))
    d_tok, d_lp = torch.from_numpy(tok0).cuda(), torch.from_numpy(lp0.view(np.int32)).cuda()
    torch.cuda.synchronize()
    rc = m.lib().pplhip_op_top_logprobs(None, d.data_ptr() + 4 * c.off, None if d_t is None else d_t.data_ptr(), d_n.data_ptr(), c.B, c.V,
                                        c.stride, d_tok.data_ptr(), d_lp.data_ptr())
    torch.cuda.synchronize()
    return rc, d_tok.cpu().numpy(), d_lp.cpu().numpy().view(np.uint32)


def launch_greedy(m, torch, c):
    """pplhip_op_sample with top_k = 1 on the same image: (tokens [B], logprobs [B])"""
    d = torch.from_numpy(c.image()).cuda()
    d_t = None if c.temps is None else torch.from_numpy(c.temps).cuda()
    d_tok = torch.zeros(c.B, dtype=torch.int32, device="cuda")
    d_lp = torch.zeros(c.B, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = m.lib().pplhip_op_sample(None, d.data_ptr() + 4 * c.off, None if d_t is None else d_t.data_ptr(), None, None, c.B, c.V, c.stride, 1,
                                  0.0, d_tok.data_ptr(), d_lp.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (c.name, rc)
    return d_tok.cpu().numpy(), d_lp.cpu().numpy()


def as_outputs(c, rows):
    """per-asked-row (tokens [n], logprobs [n]) -> the two output arrays a launch would have left (logprobs rounded to float32)"""
    tok, lp = blank_outputs(len(c.asked))
    for j, b in enumerate(c.asked):
        n = int(c.nlp[b])
        tok[j, :n] = rows[j][0]
        lp[j, :n] = np.asarray(rows[j][1], dtype=np.float32).view(np.uint32)
    return tok, lp


# ---- mutated references (tests/test_top_logprobs_spec.py: the checker must reject each in every family it is built for) -----------------
def _mut_ties_high(x, n):
    V, k = x.size, min(n, x.size)
    order = (V - 1 - np.argsort(-x[::-1], kind="stable"))[:k]      # ties by DESCENDING index
    tok, lp, log_s, lse = ref_row(x, n)
    tok[:k] = order
    return tok, lp


def _mut_drop_last(x, n):
    if x.size == 1:
        return ref_row(x, n)[:2]
    with np.errstate(invalid="ignore"):                  # (a masked row whose one finite entry was the last)
        tok, lp, _, _ = ref_row(x[:-1], n)
    return tok, lp


def _mut_drop_first(x, n):
    if x.size == 1:
        return ref_row(x, n)[:2]
    with np.errstate(invalid="ignore"):
        tok, lp, _, _ = ref_row(x[1:], n)
    tok[tok >= 0] += 1
    return tok, lp


def _mut_no_shift(x, n):
    """lse = logf(sum expf(x)) in float32, without the maximum shift: overflows for x > 88.7"""
    tok, lp, _, _ = ref_row(x, n)
    with np.errstate(over="ignore", invalid="ignore"):
        lse = np.log(np.exp(x).astype(np.float32).sum(dtype=np.float32))
        k = min(n, x.size)
        lp[:k] = (x[tok[:k]] - lse).astype(np.float64)
    return tok, lp


def _mut_rank_n(x, n):
    """entry n - 1 holds rank n"""
    tok, lp, _, _ = ref_row(x, n)
    if x.size > n:
        t2, l2, _, _ = ref_row(x, n + 1)
        tok[n - 1], lp[n - 1] = t2[n], l2[n]
    return tok, lp


MUTANTS = {   # name: (mutated row reference, the families it must be caught in)
    "ties-to-higher-index": (_mut_ties_high, ("ties", "flat")),
    "last-element-dropped": (_mut_drop_last, ("gaps", "ties", "masked")),
    "first-element-dropped": (_mut_drop_first, ("gaps", "ties", "flat")),
    "lse-without-max-shift": (_mut_no_shift, ("needle",)),
    "rank-n-for-rank-n-1": (_mut_rank_n, ("gaps", "ties", "flat", "needle")),
}


def mutant_outputs(c, name):
    f = MUTANTS[name][0]
    return as_outputs(c, [f(c.x(b), int(c.nlp[b])) for b in c.asked])


# ---- case builders ---------------------------------------------------------------------------------------------------
GRID_V = [1, 2, 3, 19, 20, 21, 255, 256, 257, 1023, 1025, 4097, 32000, 32001, 128256]
GRID_B = [1, 2, 8, 64]
NS = [1, 2, 5, 19, 20]
TS = [1.0, 0.0, -1.0, 0.5, 0.7]                          # and NULL: every fourth case
PATTERNS = ("first", "last", "alternating", "all")       # "none": none_cases
FAMILIES = ("gaps", "ties", "masked", "flat", "needle")
PLANTED = 22                                             # >= NMAX + 2: the ranks the assertions look at are all planted
TIE_VALUES = [2.0, float(np.uint32(0x3FFFFFFF).view(np.float32)), -0.5, 0.0]   # 0.0: the block mixes +0 and -0


def pattern_rows(pattern, B):
    """True where the row asks"""
    h = (B + 1) // 2
    return {"first": [b < h for b in range(B)], "last": [b >= B - h for b in range(B)], "alternating": [b % 2 == 0 for b in range(B)],
            "all": [True] * B, "none": [False] * B}[pattern]


def _edges(V):
    """indices on both sides of what the kernel's loops break at: the row's ends, the 16-byte tail, a wave, a thread's stride, the
    1024-chunk step of the vector loop, a digit of the index rounds"""
    e = [0, V - 1, 4 * (V // 4) - 1, 4 * (V // 4), 63, 64, 255, 256, 1023, 1024, 4095, 4096, 65535, 65536]
    return sorted({i for i in e if 0 <= i < V})


def _positions(rng, V, m, first=()):
    """m distinct indices: `first`, then the edges in random order, then random others"""
    out = [i for i in first if 0 <= i < V]
    for i in rng.permutation(_edges(V)):
        if len(out) < m and i not in out:
            out.append(int(i))
    while len(out) < m:
        i = int(rng.randint(0, V))
        if i not in out:
            out.append(i)
    return out[:m]


def _base(rng, V, ceil):
    """the bulk of a row: everything <= ceil"""
    return np.minimum(rng.randn(V) * 1.5 + (ceil - 4.0), ceil).astype(np.float32)


def _gaps_row(rng, V, n, k, top=8.0):
    m = min(V, PLANTED)
    r = _base(rng, V, top - 0.25 * m - 1.0)
    pos = _positions(rng, V, m, first=(0, V - 1) if k % 2 else (V - 1, 0))
    r[pos] = (top - 0.25 * rng.permutation(m)).astype(np.float32)
    return r


def _ties_row(rng, V, n, k):
    tv = TIE_VALUES[k % len(TIE_VALUES)]
    a = min((0, n - 1, n // 2)[k % 3], V - 1)            # entries above the block
    T = min(V - a, max((2, 5, 40, 300)[(k // 3) % 4], n - a + 1))   # the block reaches past rank n (where the row has that many)
    r = _base(rng, V, tv - 1.0)
    pos = _positions(rng, V, a + T, first=(V - 1, 0) if k % 2 else (0,))
    above, block = pos[:a], pos[a:]
    r[above] = (np.float32(tv) + 0.25 * (1 + np.arange(a))).astype(np.float32)
    r[block] = np.float32(tv)
    if tv == 0.0:
        r[block[::2]] = np.float32(-0.0)
    return r


def _masked_row(rng, V, n, k):
    f = max(1, min(V, (1, n - 1, n, n + 1)[k % 4]))      # finite entries: fewer than n, n, more
    r = np.full(V, -np.inf, dtype=np.float32)
    pos = _positions(rng, V, f, first=(V - 1,) if k % 2 else ())
    r[pos] = (3.0 - 0.25 * rng.permutation(f)).astype(np.float32)
    return r


def _flat_row(rng, V, n, k):
    return np.full(V, (0.25, -3.0, 0.0)[k % 3], dtype=np.float32)


def _needle_row(rng, V, n, k):
    """one logit 60 above the rest (99.75 against a ladder whose next value is 39.75): logprobs of the ranks >= 1 near -60, the mass near 1"""
    r = _gaps_row(rng, V, n, k, top=40.0)
    r[int(np.argmax(r))] = np.float32(99.75)             # the ladder's second value is 39.75
    return r


ROW = {"gaps": _gaps_row, "ties": _ties_row, "masked": _masked_row, "flat": _flat_row, "needle": _needle_row}


def _case(name, family, V, B, pattern, stride, off, k, rows_of=None):
    rng = np.random.RandomState(9000 + V % 9973 + 37 * k)
    asks = pattern_rows(pattern, B)
    nlp = [NS[(b + k) % len(NS)] if asks[b] else 0 for b in range(B)]
    rows = [ROW[rows_of or family](rng, V, nlp[b] if nlp[b] else NS[(b + k) % len(NS)], b + k) for b in range(B)]
    temps = None if k % 4 == 3 else [TS[(b + k) % len(TS)] for b in range(B)]
    return TCase(name, family, np.stack(rows), stride, off, nlp, temps)


def grid_cases():
    """every V x every family; B, the pattern, the stride, the base offset and the per-row n / t walk through their lists"""
    out, k = [], 0
    for V in GRID_V:
        for family in FAMILIES:
            B = GRID_B[k % 4] if V < 100000 else GRID_B[k % 3]
            pattern = PATTERNS[(k // 2) % 4]
            # every second case may be read in 16-byte pieces (whatever V % 4 is), the others have every other stride and base
            stride, off = (4 * (V // 4) + 4, 0) if k % 2 == 0 else (V + (1, 2, 3, 7)[(k // 2) % 4], (k // 2) % 4)
            name = f"{family}-V{V}-{pattern}-B{B}-s{stride}-o{off}"
            out.append(P.Lazy(name, family, lambda name=name, family=family, V=V, B=B, pattern=pattern, stride=stride, off=off, k=k:
                              _case(name, family, V, B, pattern, stride, off, k)))
            k += 1
    return out


def none_cases():
    """nobody asks: success, no launch, both outputs untouched"""
    out = []
    for k, (V, B) in enumerate(((1, 1), (257, 8), (32000, 64))):
        name = f"gaps-V{V}-none-B{B}"
        out.append(P.Lazy(name, "none", lambda name=name, V=V, B=B, k=k: _case(name, "none", V, B, "none", V + 4, k % 4, k, rows_of="gaps")))
    return out


def all_cases():
    return grid_cases() + none_cases()
