"""min_p / typical_p truncation (csrc/k_sample_dev.h sample_trunc_row; DESIGN.md "numerics", min_p / typical_p row): a float64 reference
of the rule, its margins and the case builders, shared by tests/test_sample_trunc_spec.py (no GPU) and tests/test_gpu_sample_trunc.py.

The rule, on a scaled row x = logit * (1 / t):
  1. candidates: the k largest x (ties to the lower index), k = top_k clamped to [1, 1024], top_k <= 0: 1024 and the whole-vocabulary mass
     as the top-p denominator; sorted by (x descending, index ascending); e_i = exp(x_i - max); km = #{e_i > 0}; cum = scan(e)
  2. keep_p = 1 + first i < km with cum[i] / tot >= top_p (km if none)
  3. keep_m = #{i < km : e_i >= min_p} (min_p off: km); keep = min(keep_p, keep_m)
  4. typical_p on: over the `keep` survivors q = e / cum[keep - 1], H = -sum q ln q, s = |-ln q - H|; order by (s ascending, rank ascending);
     n_t = 1 + first j with scan(q)[j] >= typical_p (keep if none); T = the first n_t of that order.  Off: T = the first `keep` ranks
  5. pick: c = scan over ranks i < keep of e_i [i in T]; the first i in T with c[i] > u * c[keep - 1], else the last member of T
  logprob: x_token - logsumexp(x) over the whole vocabulary.
Defaults: min_p off when <= 0 or NaN, above 1 counts as 1; typical_p off when <= 0, >= 1 or NaN.

Margins.  A row's token is compared only where every decision of the float64 rule stands further from its edge than fp32 can move it:
  * cumulative-mass edges (top-p, typical-p, pick), as shares of the mass they are taken of: tests/postproc.py's MARGIN = 3e-6
  * edges in nats: |(x_i - x_0) - ln(min_p)| at the min_p boundary (entries with x_i == x_0 have e = 1 exactly and are no edge), and the gap
    in s between the last kept and the first dropped entry of the typical order (and between the last two kept entries where their swap
    would move the cut).  NATS_BAR = 1e-4, for builders that assert |x| <= 100:
      x * (1 / t) carries <= 2^-23 relative: <= 1.2e-5 on a difference of two x (the reference takes the same fp32 x, so this term is
      spare);
      H is a sum of <= 1024 terms with sum |q ln q| <= ln 1024 = 6.93; the kernel adds a thread's <= 4 terms in series, then the six
      shuffle steps of a wave, then (w0 + w1) + (w2 + w3): 12 roundings in series (< 20), each <= 2^-24 of a partial sum <= 6.93: < 1e-5;
      logf and expf are within a few ulp of values that matter at magnitude <= 10: < 2e-6.
    Together < 2.5e-5: 1e-4 leaves >= 4x.
Rows closer than that are counted and only checked to be candidates with mass; a family may leave out at most UNCOMPARED_CAP = 4 % of its
rows (tests/test_sample_trunc_spec.py asserts that on the committed seeds; the builders redraw a row on a fixed seed schedule).
"""
import math

import numpy as np

from tests import postproc as P
from tests import sample_rows as S

NATS_BAR = 1e-4
MUTANTS = ("minp-total-mass", "minp-strict", "typical-no-abs", "typical-descending", "typical-unnormalised", "nt-off-by-one",
           "pick-s-order", "keep-max")


def norm_min_p(v):
    v = float(v)
    return 0.0 if not v > 0 else min(v, 1.0)


def norm_typical_p(v):
    v = float(v)
    return v if 0 < v < 1 else 0.0


def truncating(top_k, min_p, typical_p):
    return top_k != 1 and (norm_min_p(min_p) > 0 or norm_typical_p(typical_p) > 0)


def trunc_ref(x, top_k, top_p, min_p, typical_p, u, mutant=None):
    """float64 rule on a scaled row: (token, (mass margin, nats margin), kept set as token ids in rank order, logsumexp).  mutant: one of
    MUTANTS, a named wrong reading of the rule (tests/test_sample_trunc_spec.py)"""
    V = x.size
    full = top_k <= 0
    k = min(P.TOPK_MAX if full else min(top_k, P.TOPK_MAX), V)
    order = np.argsort(-x, kind="stable")[:k]
    mx = float(x.max())
    xs = x[order].astype(np.float64)
    e = np.exp(xs - mx)
    km = max(int(np.count_nonzero(e)), 1)
    se = np.exp(x.astype(np.float64) - mx).sum()
    tot = se if full else e.sum()
    cum = np.cumsum(e)
    m_mass, m_nats = np.inf, np.inf
    # 2. top-p
    hit = np.flatnonzero(cum[:km] / tot >= float(top_p))
    keep_p = int(hit[0]) + 1 if hit.size else km
    n_edge = min(keep_p, km - 1)
    if n_edge > 0:
        m_mass = min(m_mass, float(np.abs(cum[:n_edge] / tot - float(top_p)).min()))
    # 3. min_p
    mp = norm_min_p(min_p)
    if mp > 0:
        if mutant == "minp-total-mass":
            keep_m = int(np.count_nonzero(e[:km] / e[:km].sum() >= mp))
        elif mutant == "minp-strict":
            keep_m = int(np.count_nonzero(e[:km] > mp))
        else:
            keep_m = int(np.count_nonzero(e[:km] >= mp))
        keep_m = max(keep_m, 1)
        below = xs[:km] < xs[0]
        if below.any():
            m_nats = min(m_nats, float(np.abs((xs[:km][below] - xs[0]) - math.log(mp)).min()))
    else:
        keep_m = km
    keep = max(keep_p, keep_m) if mutant == "keep-max" else min(keep_p, keep_m)
    # 4. typical_p
    ty = norm_typical_p(typical_p)
    member = np.ones(keep, dtype=bool)
    s_order = np.arange(keep)
    if ty > 0:
        S_ = cum[keep - 1]
        lq = (xs[:keep] - mx) - math.log(S_)
        q = e[:keep] / S_
        if mutant == "typical-unnormalised":
            lq, q = (xs[:keep] - mx) - math.log(se), e[:keep] / se
        H = -float((q * lq).sum())
        s = (-lq - H) if mutant == "typical-no-abs" else np.abs(-lq - H)
        s_order = np.lexsort((np.arange(keep), -s if mutant == "typical-descending" else s))
        cq = np.cumsum(q[s_order])
        hit = np.flatnonzero(cq >= ty)
        n_t = int(hit[0]) + 1 if hit.size else keep
        if mutant == "nt-off-by-one":
            n_t = max(n_t - 1, 1)
        if n_t > 1:
            m_mass = min(m_mass, float(np.abs(cq[:n_t - 1] - ty).min()))
        ss = s[s_order]
        if n_t < keep:
            m_nats = min(m_nats, float(ss[n_t] - ss[n_t - 1]))
        if n_t >= 2 and cq[n_t - 1] - q[s_order[n_t - 2]] >= ty:    # the last two kept ones swapped: the cut would come one earlier
            m_nats = min(m_nats, float(ss[n_t - 1] - ss[n_t - 2]))
        member[:] = False
        member[s_order[:n_t]] = True
        s_order = s_order[:n_t]
    # 5. pick
    ranks = s_order if mutant == "pick-s-order" else np.flatnonzero(member)
    c = np.cumsum(e[ranks])
    target = float(u) * c[-1]
    sel = min(int(np.searchsorted(c, target, side="right")), ranks.size - 1)
    if ranks.size > 1:
        m_mass = min(m_mass, float(np.abs(c[:-1] - target).min() / c[-1]))
    return int(order[ranks[sel]]), (m_mass, m_nats), order[np.flatnonzero(member)], mx + math.log(se)


def compared(margin):
    return margin[0] >= P.MARGIN and margin[1] >= NATS_BAR


def brute_ref(x, top_k, top_p, min_p, typical_p, u):
    """the same rule as a chain of filters on full-vocabulary arrays, each one masking to -inf and the next one taking the softmax of what
    is left: top_k, top_p, min_p, typical.  (token, kept set as sorted token ids)"""
    V = x.size
    z = x.astype(np.float64).copy()
    rank_of = np.empty(V, dtype=np.int64)
    rank_of[np.argsort(-x, kind="stable")] = np.arange(V)           # x descending, ties to the lower index

    def softmax(a):
        w = np.exp(a - a.max())
        return w / w.sum()

    full = top_k <= 0
    k = min(P.TOPK_MAX if full else min(top_k, P.TOPK_MAX), V)
    p_all = softmax(z)                                              # pure top-p mode: the nucleus is measured on the whole vocabulary
    z[rank_of >= k] = -np.inf
    p = p_all if full else softmax(z)
    alive = np.flatnonzero(p * (z > -np.inf) > 0)
    by_rank = alive[np.argsort(rank_of[alive])]
    cum = np.cumsum(p[by_rank])
    hit = np.flatnonzero(cum >= float(top_p))
    z_new = np.full(V, -np.inf)
    kept = by_rank[:int(hit[0]) + 1] if hit.size else by_rank
    z_new[kept] = z[kept]
    z = z_new
    mp = norm_min_p(min_p)
    if mp > 0:
        w = np.exp(z - z.max())                                     # p / p_max, whatever the normalisation
        z[w < mp] = -np.inf
    ty = norm_typical_p(typical_p)
    if ty > 0:
        alive = np.flatnonzero(z > -np.inf)
        p = softmax(z)[alive]
        lq = (z[alive] - z.max()) - math.log(np.exp(z[alive] - z.max()).sum())
        H = -float((p * lq).sum())
        s = np.abs(-lq - H)
        o = np.lexsort((rank_of[alive], s))
        cq = np.cumsum(p[o])
        hit = np.flatnonzero(cq >= ty)
        n_t = int(hit[0]) + 1 if hit.size else alive.size
        z_new = np.full(V, -np.inf)
        z_new[alive[o[:n_t]]] = z[alive[o[:n_t]]]
        z = z_new
    alive = np.flatnonzero(z > -np.inf)
    by_rank = alive[np.argsort(rank_of[alive])]
    c = np.cumsum(np.exp(z[by_rank] - float(x.max())))
    sel = min(int(np.searchsorted(c, float(u) * c[-1], side="right")), by_rank.size - 1)
    return int(by_rank[sel]), np.sort(alive)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
class TCase(S.RCase):
    """one launch of pplhip_op_sample_rows2: an RCase with a min_p and a typical_p per row (None: NULL)"""

    def __init__(self, name, family, logits, stride, off, top_k, top_p, min_p, typical_p, temps=None, seeds=None, draws=None, rnd=None):
        super().__init__(name, family, logits, stride, off, top_k, top_p, temps, seeds, draws, rnd)
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        self.min_p, self.typical_p = f(min_p), f(typical_p)

    def mp(self, b):
        return 0.0 if self.min_p is None else float(self.min_p[b])

    def ty(self, b):
        return 0.0 if self.typical_p is None else float(self.typical_p[b])

    def truncating(self, b):
        return truncating(int(self.top_k[b]), self.mp(b), self.ty(b))

    def reference(self):
        """per row (token, logprob, margin, candidates with mass or None, kind): greedy and sampling rows by tests/sample_rows.py's rules"""
        rows, r = [], self.numbers()
        for b in range(self.B):
            x = self.x(b)
            if self.greedy(b):
                tok, lp, gap = P.greedy_ref(x)
                rows.append((tok, lp, gap, None, "greedy"))
            elif not self.truncating(b):
                tok, margin, cand, lse = P.topk_ref(x, int(self.top_k[b]), float(self.top_p[b]), r[b])
                rows.append((tok, float(x[tok]) - lse, margin, cand, "sampling"))
            else:
                tok, margin, _, lse = trunc_ref(x, int(self.top_k[b]), float(self.top_p[b]), self.mp(b), self.ty(b), r[b])
                cand = P.topk_ref(x, int(self.top_k[b]), 2.0, 0.0)[2]
                rows.append((tok, float(x[tok]) - lse, margin, cand, "trunc"))
        return rows

    def check_assertions(self):
        """the builder's conditions; returns (reference rows, truncating rows, truncating rows that are not compared)"""
        img = self.image()
        assert 0 <= self.off <= 3 and self.stride >= self.V >= 1
        assert not np.isnan(self.logits).any() and not np.isposinf(self.logits).any(), self.name
        assert (self.logits.max(axis=1) > -np.inf).all(), self.name
        assert np.isposinf(img).sum() == img.size - self.B * self.V + int(np.isposinf(self.logits).sum()), (self.name, "poison")
        for b in range(self.B):
            x = self.x(b)
            fin = x[np.isfinite(x)]
            assert np.abs(fin).max() <= 100.0 and fin.max() - fin.min() <= 80.0, (self.name, b)   # NATS_BAR's premise; fp32 masses > 0
        r = self.numbers()
        assert (r >= 0).all() and (r < 1).all(), self.name
        rows = self.reference()
        n_t = sum(1 for row in rows if row[4] == "trunc")
        n_unc = sum(1 for row in rows if row[4] == "trunc" and not compared(row[2]))
        return rows, n_t, n_unc


def check_rows(c, rows, tok, lp, tok_tail, lp_tail):
    """failures of one launch: tokens where the margin allows, candidates with mass elsewhere, logprobs by postproc.LOGPROB_BAR, canaries"""
    fails = []
    if not (tok_tail == P.TOK_CANARY).all() or not (lp_tail == P.LP_CANARY).all():
        fails.append("canaries behind out_tok / out_logprob were written")
    for b, (wtok, wlp, margin, cand, kind) in enumerate(rows):
        t, x = int(tok[b]), c.x(b)
        if not 0 <= t < c.V:
            fails.append(f"row {b} ({kind}): token {t} is outside [0, {c.V})")
            continue
        sure = kind == "greedy" or (compared(margin) if kind == "trunc" else margin >= P.MARGIN)
        if sure and t != wtok:
            fails.append(f"row {b} ({kind}, k {int(c.top_k[b])} p {float(c.top_p[b])} min_p {c.mp(b)} typ {c.ty(b)}): token {t} (x {x[t]!r}) "
                         f"want {wtok} (x {x[wtok]!r}) margin {margin}")
            continue
        if not sure and t not in cand:
            fails.append(f"row {b} ({kind}): token {t} is no candidate that carries mass")
            continue
        want_lp = wlp if t == wtok else float(x[t]) - P._lse(x)
        if not abs(float(lp[b]) - want_lp) <= P.LOGPROB_BAR:
            fails.append(f"row {b} ({kind}): logprob {float(lp[b])!r} want {want_lp!r}")
    return fails


def launch_rows2(m, torch, c, entry="pplhip_op_sample_rows2"):
    """the case through pplhip_op_sample_rows2 (or, without the two arrays, pplhip_op_sample_rows): (rc, tokens [B], logprobs [B], token
    tail, logprob tail as uint32)"""
    d = torch.from_numpy(c.image()).cuda()
    assert d.data_ptr() % 16 == 0
    dev = lambda a: None if a is None else torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    d_t, d_k, d_p, d_s, d_n, d_r = (dev(a) for a in (c.temps, c.top_k, c.top_p, c.seeds, c.draws, c.rnd))
    d_m, d_y = dev(c.min_p), dev(c.typical_p)
    d_tok = torch.from_numpy(np.full(c.B + 8, P.TOK_CANARY, dtype=np.int32)).cuda()
    d_lp = torch.from_numpy(np.full(c.B + 8, P.LP_CANARY, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    if entry == "pplhip_op_sample_rows2":
        rc = m.lib().pplhip_op_sample_rows2(None, d.data_ptr() + 4 * c.off, ptr(d_t), ptr(d_k), ptr(d_p), ptr(d_m), ptr(d_y), ptr(d_s), ptr(d_n),
                                            ptr(d_r), c.B, c.V, c.stride, d_tok.data_ptr(), d_lp.data_ptr())
    else:
        rc = m.lib().pplhip_op_sample_rows(None, d.data_ptr() + 4 * c.off, ptr(d_t), ptr(d_k), ptr(d_p), ptr(d_s), ptr(d_n), ptr(d_r), c.B, c.V,
                                           c.stride, d_tok.data_ptr(), d_lp.data_ptr())
    torch.cuda.synchronize()
    tok, lp = d_tok.cpu().numpy(), d_lp.cpu().numpy()
    return rc, tok[:c.B], lp[:c.B].view(np.float32), tok[c.B:], lp[c.B:].view(np.uint32)


# ---- builders --------------------------------------------------------------------------------------------------------------------------
GRID_V = [1, 2, 33, 257, 1025, 32000, 128256]
TEMPS = [1.0, 0.7, 2.0, 4.0]
REDRAWS = 12                                               # a row is drawn again, seed + attempt, until every margin of it holds
SEED_BASE = 0x7C0FFEE5EED


def head_row(rng, V, n_head, span, masked=0):
    """a row with n_head entries spread evenly (jittered) over [-span, 0] at random places, the rest 30 .. 35 below the maximum; `masked`
    of the rest are -inf"""
    r = (-30.0 - 5.0 * rng.rand(V)).astype(np.float32)
    n_head = min(n_head, V)
    pos = rng.choice(V, size=n_head, replace=False)
    step = span / max(n_head, 1)
    r[pos] = (-(np.arange(n_head) + 0.8 * rng.rand(n_head)) * step).astype(np.float32)
    rest = np.setdiff1d(np.arange(V), pos)
    if masked:
        r[rng.choice(rest, size=min(masked, rest.size), replace=False)] = -np.inf
    return r


def _settle(make_row, params, seed):
    """the first draw of the row, on the schedule seed, seed + 1, ..., whose margins all hold (the last draw if none does)"""
    for a in range(REDRAWS):
        row = make_row(np.random.RandomState((seed + a) % (2 ** 32)))
        t, k, p, mp, ty, u = params
        x = P.scaled(row, t)
        if not truncating(k, mp, ty) or compared(trunc_ref(x, k, p, mp, ty, u)[1]):
            break
    return row


def _case(name, family, V, specs, n, temps=True):
    """specs: per row (make_row(rng), top_k, top_p, min_p, typical_p); the layout, temperatures and random numbers walk with n"""
    def make():
        B = len(specs)
        stride, off = V + (0, 2, 6, 3)[n % 4], (n // 2) % 4
        ts = [TEMPS[(b + n) % len(TEMPS)] for b in range(B)] if temps else None
        seeds = np.array([(SEED_BASE + 1000003 * n + 7919 * b) & ((1 << 64) - 1) for b in range(B)], dtype=np.uint64)
        draws = np.array([(0, 1, 2, 77, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5)[(b + n) % 7] for b in range(B)], dtype=np.uint64)
        us = S.uniform(seeds, draws)
        rows = [_settle(mk, (ts[b] if ts else None, k, p, mp, ty, us[b]), 9000 + 131 * n + 17 * b) for b, (mk, k, p, mp, ty) in enumerate(specs)]
        return TCase(name, family, np.stack(rows), stride, off, [s[1] for s in specs], [s[2] for s in specs], [s[3] for s in specs],
                     [s[4] for s in specs], ts, seeds, draws)
    return P.Lazy(name, family, make)


MODES = (("minp", 0.08, 0.0), ("typical", 0.0, 0.6), ("both", 0.03, 0.9))


def grid_cases():
    """every V x (min_p only, typical only, both): rows that walk through top_k (0, negative, > V, 50, 1024, 5000), top_p and the head size"""
    out, n = [], 0
    for V in GRID_V:
        for mode, mp, ty in MODES:
            B = 4 if V > 100000 else 8
            specs = []
            for b in range(B):
                k = (0, 50, 5000, -3, 1024, 300, 2, 40)[(b + n) % 8]
                # (no top_p of exactly 1 on these rows: their last candidates carry less than fp32 resolves of the whole mass, so the scan
                # reaches 1 early -- an edge of top-p's own that tests/test_gpu_sampler_exact.py covers on rows made for it)
                p = (2.0, 0.95, 0.0, 0.999, 0.8, 0.9, -1.0, 2.0)[(b + 3 * n) % 8]
                heads = (300, 40, 1100, 12)[(b + n) % 4]
                specs.append((lambda rng, V=V, heads=heads: head_row(rng, V, heads, 8.0 + 0.004 * heads), k, p, mp, ty))
            out.append(_case(f"trunc-V{V}-{mode}", "trunc-grid", V, specs, n))
            n += 1
    return out


KEEPS = [1, 2, 255, 256, 257, 1023, 1024]


def keep_cases():
    """`keep` at the block width's and the candidate limit's edges, reached two ways: top_k = keep with a min_p that is on and cuts nothing,
    and top_k <= 0 with a min_p that cuts a head of exactly `keep` entries off the rest; min_p alone, with typical_p, and typical_p alone"""
    out, n = [], 100
    for V in (1025, 4099):
        specs = []
        for keep in KEEPS:
            span = 2.0 + keep * 0.006
            mk = lambda rng, V=V, keep=keep, span=span: head_row(rng, V, keep, span)
            cut = float(np.exp(-(span + 5.0)))                                  # between the head and the rest, > 5 nats from either
            # (top_p 2: no nucleus cut.  At 1 the scan's last entries stand within fp32's reach of the whole mass, an edge of its own)
            specs += [(mk, keep, 2.0, 1e-30, 0.0), (mk, keep, 2.0, 1e-30, 0.7), (mk, 0, 2.0, cut, 0.0), (mk, -1, 2.0, cut, 0.85),
                      (mk, keep, 2.0, 0.0, 0.5)]
        out.append(_case(f"trunc-keep-V{V}", "trunc-keep", V, specs, n, temps=False))
        n += 1
    return out


def masked_cases():
    """fewer candidates with mass than k (km < k): masked logits, k > V, and every truncation over them"""
    out, n = [], 200
    for V, alive in ((257, 57), (1025, 300), (33, 1), (2, 1)):
        specs = []
        for j, (mode, mp, ty) in enumerate(MODES):
            for k in (100, 0, 5000):
                def mk(rng, V=V, alive=alive):
                    r = np.full(V, -np.inf, dtype=np.float32)
                    pos = rng.choice(V, size=alive, replace=False)
                    r[pos] = (-(np.arange(alive) + 0.8 * rng.rand(alive)) * (6.0 / alive)).astype(np.float32)
                    return r
                specs.append((mk, k, (1.0, 0.9)[j % 2], mp, ty))
        out.append(_case(f"trunc-masked-V{V}-alive{alive}", "trunc-masked", V, specs, n))
        n += 1
    return out


FAMILIES = ("trunc-grid", "trunc-keep", "trunc-masked")


def all_cases():
    return grid_cases() + keep_cases() + masked_cases()


# ---- exact cases: no margin --------------------------------------------------------------------------------------------------------------
def minp_one_case():
    """min_p = 1 at temperature 4: only the maximum's ties survive (e = 1 exactly), chosen in index order by u.  (case, ties per row)"""
    V, B = 4097, 16
    rng = np.random.RandomState(41)
    lg = (rng.randn(B, V) * 2.0).astype(np.float32)
    ties = []
    for b in range(B):
        pos = np.sort(rng.choice(V, size=1 + b % 4, replace=False))
        lg[b, pos] = np.float32(12.0)
        ties.append(pos)
    rnd = np.array([(0.0, 0.3, 0.6, float(P.RND_TOP))[b % 4] for b in range(B)], dtype=np.float32)
    c = TCase("trunc-minp-one", "trunc-exact", lg, V + 3, 1, [0, 50] * (B // 2), [2.0] * B, [1.0, 7.5] * (B // 2), None, [4.0] * B, None, None, rnd)
    return c, ties


def typical_head_case():
    """one token at p = 0.3 and 714 equal tokens that share 0.7 (714 * 0.3 / 0.7 = 306 exactly: the head stands ln 306 over the others),
    typical_p = 0.5: H = 5.15 nats, the head's -ln p = 1.20 is 3.9 from it and the others' 6.92 only 1.8, so the 714 come first in the
    typical order and half of them reach 0.5: the argmax is never in the set, whatever u.  Without the cut it is drawn for u < 0.3."""
    V, B, head = 715, 32, 123
    lg = np.zeros((B, V), dtype=np.float32)
    lg[:, head] = np.float32(math.log(306.0))
    rnd = (np.arange(B, dtype=np.float32) / np.float32(B)).astype(np.float32)
    rnd[-1] = P.RND_TOP
    return TCase("trunc-typical-head", "trunc-exact", lg, V + 1, 0, [0] * B, [2.0] * B, None, [0.5] * B, None, None, None, rnd), head


def mixed_case():
    """greedy, sampling and truncating rows in one launch: (case, the rows that do not ask)"""
    V, B = 32000, 24
    rng = np.random.RandomState(77)
    lg = (rng.randn(B, V) * 1.0).astype(np.float32)
    ks = [(1, 50, 0, 1024)[b % 4] for b in range(B)]
    mp = [(0.0, 0.1, -1.0, float("nan"), 0.0, 0.0)[b % 6] for b in range(B)]
    ty = [(1.0, 0.0, 0.0, 2.0, 0.5, float("nan"))[b % 6] for b in range(B)]
    seeds = np.arange(B, dtype=np.uint64) * np.uint64(7919) + np.uint64(SEED_BASE)
    draws = np.arange(B, dtype=np.uint64)
    c = TCase("trunc-mixed", "trunc-exact", lg, V + 2, 2, ks, [0.9] * B, mp, ty, [TEMPS[b % 4] for b in range(B)], seeds, draws)
    return c, [b for b in range(B) if not c.truncating(b)]
