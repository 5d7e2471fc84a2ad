"""The per-request sampler (csrc/k_sample_rows.hip; DESIGN.md "numerics", per-request sampler row): a numpy restatement of its generator,
a per-row reference and the case builders, shared by tests/test_sample_rows_spec.py (no GPU) and the tests/test_gpu_sample_rows*.py files.

Generator: u(seed, n) = fp32(w0 >> 8) * 2^-24 with w0 the first output word of Philox4x32-10 under key (seed lo, seed hi) and counter
(n lo, n hi, 0, 0) -- integers, compared bit for bit.

Sampler: row b is answered by the rules of tests/postproc.py with ITS parameters: x = scaled(logits[b], t[b]); top_k[b] == 1: greedy_ref;
anything else: topk_ref(x, top_k[b], top_p[b], rnd) with rnd = u(seeds[b], draws[b]) or the caller's number.  The checks are
postproc.check_sample's, one row at a time and with its constants (MARGIN, UNCOMPARED_CAP, LOGPROB_BAR): no tolerance of this file's own.
Greedy rows carry a planted gap >= 1 (or an exact tie) and are always compared.  The guards are SCase's: +inf behind vocab, in front of a
misaligned base and in a canary row behind the batch; token / logprob canaries behind `batch`.
"""
import numpy as np

from tests import postproc as P

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (python ints or equal-shaped uint64 arrays holding 32-bit values) -> the 4 output words"""
    c = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK32) for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & np.uint64(MASK32) for w in key]
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                        # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & m32, (p0 >> s32) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(W0)) & m32, (k[1] + np.uint64(W1)) & m32]
    return [w.astype(np.uint32) for w in c]


def word0(seeds, draws):
    s = np.asarray(seeds, dtype=np.uint64)
    n = np.asarray(draws, dtype=np.uint64)
    z = np.zeros_like(s)
    return philox4x32_10((n & np.uint64(MASK32), n >> np.uint64(32), z, z), (s & np.uint64(MASK32), s >> np.uint64(32)))[0]


def u_from_word(w):
    """fp32(w >> 8) * 2^-24: both steps are exact (24 bits, a power of two)"""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def uniform(seeds, draws):
    return u_from_word(word0(seeds, draws))


def splitmix64(x):
    """the seed of the n-th request that brings none: splitmix64(sampling_seed + n)"""
    m = (1 << 64) - 1
    z = (int(x) + 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


class RowView:
    """row b of a case with the face postproc.check_sample looks at: one row, its top_k"""

    def __init__(self, c, b):
        self.V, self.top_k, self._x = c.V, int(c.top_k[b]), c.x(b)

    def x(self, _):
        return self._x


class RCase:
    """one launch of pplhip_op_sample_rows: B rows of V logits, rows `stride` apart, the base `off` floats past a 16-byte boundary; per row
    top_k / top_p / temperature (temps None: NULL) and either (seeds, draws) or the caller's rnd"""

    def __init__(self, name, family, logits, stride, off, top_k, top_p, temps=None, seeds=None, draws=None, rnd=None, expect=None):
        self.name, self.family = name, family
        self.logits = np.ascontiguousarray(logits, dtype=np.float32)
        self.B, self.V = self.logits.shape
        self.stride, self.off = stride, off
        self.top_k = np.ascontiguousarray(top_k, dtype=np.int32)
        self.top_p = np.ascontiguousarray(top_p, dtype=np.float32)
        f = lambda a, t: None if a is None else np.ascontiguousarray(a, dtype=t)
        self.temps, self.rnd = f(temps, np.float32), f(rnd, np.float32)
        self.seeds, self.draws = f(seeds, np.uint64), f(draws, np.uint64)
        self.expect = expect                              # {row: planted answer} of the greedy rows
        assert self.top_k.shape == self.top_p.shape == (self.B,)
        assert (self.rnd is None) != (self.seeds is None) and (self.seeds is None) == (self.draws is None), name

    def greedy(self, b):
        return self.top_k[b] == 1

    def x(self, b):
        return P.scaled(self.logits[b], None if self.temps is None else self.temps[b])

    def numbers(self):
        """the random number of every row"""
        return self.rnd if self.rnd is not None else uniform(self.seeds, self.draws)

    def image(self):
        img = np.full(4 + (self.B + 1) * self.stride + 4, np.inf, dtype=np.float32)
        for b in range(self.B):
            img[self.off + b * self.stride:self.off + b * self.stride + self.V] = self.logits[b]
        return img

    def reference(self):
        """per row (token, logprob, margin or gap, candidates or None): postproc.SCase.reference with every row's own parameters"""
        rows, r = [], self.numbers()
        for b in range(self.B):
            x = self.x(b)
            if self.greedy(b):
                tok, lp, gap = P.greedy_ref(x)
                rows.append((tok, lp, gap, None))
            else:
                tok, margin, cand, lse = P.topk_ref(x, int(self.top_k[b]), float(self.top_p[b]), r[b])
                rows.append((tok, float(x[tok]) - lse, margin, cand))
        return rows

    def check_assertions(self):
        """the builder's conditions; returns (reference rows, sampling rows, sampling rows that are not compared)"""
        assert 0 <= self.off <= 3 and self.stride >= self.V and self.V >= 1
        img = self.image()
        mask = np.ones(img.size, dtype=bool)
        for b in range(self.B):
            mask[self.off + b * self.stride:self.off + b * self.stride + self.V] = False
        assert np.isposinf(img[mask]).all() and mask.sum() == img.size - self.B * self.V, (self.name, "poison")
        assert not np.isnan(self.logits).any() and not np.isposinf(self.logits).any(), self.name
        assert (self.logits.max(axis=1) > -np.inf).all(), (self.name, "a row without a finite entry")
        r = self.numbers()
        assert (r >= 0).all() and (r < 1).all(), self.name
        rows = self.reference()
        n_s = n_unc = 0
        for b, (tok, lp, m, _) in enumerate(rows):
            if self.greedy(b):
                assert m >= 1.0 or m == 0.0, (self.name, b, m)
                assert self.expect is None or b not in self.expect or tok == self.expect[b], (self.name, b, tok, self.expect[b])
            else:
                n_s += 1
                n_unc += m < P.MARGIN
        return rows, n_s, n_unc


def check_rows(c, rows, tok, lp, tok_tail, lp_tail):
    """postproc.check_sample, row by row"""
    fails = []
    for b in range(c.B):
        fails += [f.replace("row 0:", f"row {b} (top_k {int(c.top_k[b])}):") for f in
                  P.check_sample(RowView(c, b), [rows[b]], tok[b:b + 1], lp[b:b + 1], tok_tail, lp_tail)]
    return fails


def launch_rows(m, torch, c):
    """the case through pplhip_op_sample_rows: (rc, tokens [B], logprobs [B], token tail, logprob tail as uint32)"""
    d = torch.from_numpy(c.image()).cuda()
    assert d.data_ptr() % 16 == 0
    dev = lambda a: None if a is None else torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    d_t, d_k, d_p, d_s, d_n, d_r = (dev(a) for a in (c.temps, c.top_k, c.top_p, c.seeds, c.draws, c.rnd))
    d_tok = torch.from_numpy(np.full(c.B + 8, P.TOK_CANARY, dtype=np.int32)).cuda()
    d_lp = torch.from_numpy(np.full(c.B + 8, P.LP_CANARY, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    rc = m.lib().pplhip_op_sample_rows(None, d.data_ptr() + 4 * c.off, ptr(d_t), ptr(d_k), ptr(d_p), ptr(d_s), ptr(d_n), ptr(d_r), c.B, c.V,
                                       c.stride, d_tok.data_ptr(), d_lp.data_ptr())
    torch.cuda.synchronize()
    tok, lp = d_tok.cpu().numpy(), d_lp.cpu().numpy()
    return rc, tok[:c.B], lp[:c.B].view(np.float32), tok[c.B:], lp[c.B:].view(np.uint32)


def launch_rows_alone(m, torch, c):
    """every row of the case on its own through pplhip_op_sample (the uniform kernels) with the row's parameters and random number, at the
    row's place in the same image: (tokens [B], logprobs [B])"""
    d = torch.from_numpy(c.image()).cuda()
    r = torch.from_numpy(np.ascontiguousarray(c.numbers())).cuda()
    d_t = None if c.temps is None else torch.from_numpy(c.temps).cuda()
    d_p = torch.from_numpy(c.top_p).cuda()
    d_tok = torch.from_numpy(np.full(c.B, P.TOK_CANARY, dtype=np.int32)).cuda()
    d_lp = torch.from_numpy(np.full(c.B, P.LP_CANARY, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    for b in range(c.B):
        rc = m.lib().pplhip_op_sample(None, d.data_ptr() + 4 * (c.off + b * c.stride), None if d_t is None else d_t.data_ptr() + 4 * b,
                                      d_p.data_ptr() + 4 * b, r.data_ptr() + 4 * b, 1, c.V, c.stride, int(c.top_k[b]), 0.0,
                                      d_tok.data_ptr() + 4 * b, d_lp.data_ptr() + 4 * b)
        assert rc == 0, (c.name, b, rc)
    torch.cuda.synchronize()
    return d_tok.cpu().numpy(), d_lp.cpu().numpy().view(np.float32)


# ---- case builders ---------------------------------------------------------------------------------------------------
KS = [1, 2, 8, 50, 1024, 5000, 0, -3]
SAMPLING_KS = KS[1:]
PS = P.TOPK_PS                                           # -1, 0, 0.25, 0.9, 1, 2
TS = P.TEMPS                                             # 1, 0, -1, 0.5, 2, 0.7
GRID_V = [1, 2, 3, 5, 255, 1023, 1024, 1025, 4097, 32000, 32001, 128256]
GRID_B = [1, 2, 8, 64]
PATTERNS = ("sampling-greedy", "greedy-sampling", "alternating", "all-greedy", "all-sampling")
SEED_BASE = 0x5EED0000C0FFEE                             # fixed: tests/test_sample_rows_spec.py checks the uncompared cap on these


def pattern_rows(pattern, B):
    """True where the row is greedy"""
    h = (B + 1) // 2
    return {"sampling-greedy": [b >= h for b in range(B)], "greedy-sampling": [b < B - h for b in range(B)],
            "alternating": [b % 2 == 1 for b in range(B)], "all-greedy": [True] * B, "all-sampling": [False] * B}[pattern]


def _greedy_row(rng, V, b, kind):
    """a row with a planted answer: the maximum stands >= 1 over the rest at every temperature of TS (gap >= 6 before scaling)"""
    if kind == 0:
        r = (rng.randn(V) * 2.0).astype(np.float32)
        pos = (0, V - 1, V // 2, 4 * (V // 4) - 1 if V >= 4 else 0, 4 * (V // 4) if V % 4 else V // 3)[b % 5]
        r[pos] = np.float32(18.0)
    elif kind == 1:                                      # all negative: a zero that is not there would win
        r = (rng.randn(V) * 2.0 - 40.0).astype(np.float32)
        pos = (V - 1, 0)[b % 2]
        r[pos] = np.float32(-22.0)
    else:                                                # masked down to one entry
        r = np.full(V, -np.inf, dtype=np.float32)
        pos = (V // 2, V - 1)[b % 2]
        r[pos] = np.float32(-3.0)
    return r, pos


def _sampling_row(rng, V, k):
    keff = min(V, P.TOPK_MAX if k <= 0 else min(k, P.TOPK_MAX))
    scale = 2.5 if keff <= 64 else (1.0 if keff < V else 0.3)         # postproc.topk_grid_cases: the last candidate keeps a share above the margin
    return (rng.randn(V) * scale).astype(np.float32)


def grid_cases():
    """every V x every pattern; B, the stride, the base offset and the per-row k / p / t walk through their lists"""
    out, n = [], 0
    for V in GRID_V:
        for pattern in PATTERNS:
            B = GRID_B[n % 4] if V < 100000 else GRID_B[n % 3]
            stride, off = V + (0, 2, 6)[n % 3], (n // 3) % 4
            name = f"rows-V{V}-{pattern}-B{B}-s{stride}-o{off}"

            def make(V=V, pattern=pattern, B=B, stride=stride, off=off, n=n, name=name):
                rng = np.random.RandomState(7000 + V % 9973 + 31 * n)
                gr = pattern_rows(pattern, B)
                rows, ks, expect = [], [], {}
                for b in range(B):
                    if gr[b]:
                        r, pos = _greedy_row(rng, V, b + n, (b + n) % 3)
                        expect[b] = pos
                        ks.append(1)
                    else:
                        ks.append(SAMPLING_KS[(b + n) % len(SAMPLING_KS)])
                        r = _sampling_row(rng, V, ks[-1])
                    rows.append(r)
                tp = [PS[(b // 2 + n) % len(PS)] for b in range(B)]
                temps = None if n % 4 == 3 else [TS[(b + n) % len(TS)] for b in range(B)]
                seeds = [(SEED_BASE + 1000003 * n + 7919 * b) & ((1 << 64) - 1) for b in range(B)]
                draws = [(0, 1, 2, 77, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5)[(b + n) % 7] for b in range(B)]
                return RCase(name, "rows-grid", np.stack(rows), stride, off, ks, tp, temps, seeds, draws, None, expect)
            out.append(P.Lazy(name, "rows-grid", make))
            n += 1
    return out


def _interleave_greedy(c, family, name, rng):
    """an SCase of postproc's (uniform top_k, the caller's rnd) as a mixed launch: its rows keep their k, p, t and rnd, and a planted greedy
    row follows every second one"""
    rows, ks, tp, temps, rnd, expect = [], [], [], [], [], {}
    for b in range(c.B):
        rows.append(c.logits[b]); ks.append(c.top_k); tp.append(c.tp(b)); rnd.append(c.rnd[b])
        temps.append(1.0 if c.temps is None else c.temps[b])
        if b % 2 == 0:
            r, pos = _greedy_row(rng, c.V, b // 2, (b // 2) % 3)
            expect[len(rows)] = pos
            rows.append(r); ks.append(1); tp.append(0.5); rnd.append(P.RNDS[(b // 2) % 3]); temps.append(TS[(b // 2) % len(TS)])
    return RCase(name, family, np.stack(rows), c.stride, c.off, ks, tp, temps, None, None, rnd, expect)


def masked_cases():
    """postproc.topk_masked_cases (fewer finite entries than k) inside mixed launches, rnd in {0, 0.5, RND_TOP}"""
    out = []
    for lz in P.topk_masked_cases():
        if "-V32003-" in lz.name:
            continue
        name = "rows-" + lz.name
        out.append(P.Lazy(name, "rows-masked", lambda lz=lz, name=name: _interleave_greedy(lz.build(), "rows-masked", name, np.random.RandomState(len(name)))))
    return out


def tie_cases():
    """postproc.topk_tie_cases (the candidate cut falls into a plateau of equal values) inside mixed launches"""
    out = []
    for lz in P.topk_tie_cases():
        if "-V32003-" in lz.name:
            continue
        name = "rows-" + lz.name
        out.append(P.Lazy(name, "rows-ties", lambda lz=lz, name=name: _interleave_greedy(lz.build(), "rows-ties", name, np.random.RandomState(len(name)))))
    return out


FAMILIES = ("rows-grid", "rows-masked", "rows-ties")


def all_cases():
    return grid_cases() + masked_cases() + tie_cases()


def q3_case():
    """row 0 samples (top_k 50, rnd 0.999 on a flat-ish row), row 1 is greedy with a planted gap of 1.5.  Under ONE top_k of 50
    for the batch, row 1's arg-max holds under 10 % of its candidates' mass and rnd 0.999 picks another token."""
    rng = np.random.RandomState(3)
    V = 1024
    lg = (rng.randn(2, V) * 0.05).astype(np.float32)
    lg[1, 321] = np.float32(1.5 + lg[1].max())
    return RCase("rows-q3", "rows-q3", lg, V, 0, [50, 1], [1.0, 1.0], None, None, None, [0.999, 0.999], {1: 321})
