"""The post-processor kernels of csrc/k_sample.hip (penalty, greedy sampling, top-k / top-p sampling) at their edges: case builders, references
written from the specification and the checks, shared by tests/test_postproc_spec.py (no GPU) and tests/test_gpu_postproc.py.  The device is
reached through pplhip_op_penalty / pplhip_op_sample, which take the caller's count map, vocabulary, row stride and base pointer.

Penalty (specification: the comment over penalty_kernel and DESIGN.md "numerics", penalty row).  The count map is uint16 [slots, vocab]; batch
row b owns row batch_slots[b].  A step first clears the rows with start_pos[b] == 0 or b >= decoding_batches, then adds 1 per fed token,
stopping at 65535: integers, compared bit for bit over the WHOLE map after every step.  The logits of counted tokens become
x > 0 ? x / rep : x * rep, then - presence, then - frequency * count; every logit is divided by the temperature (NULL or <= 0: 1).  The
reference does this in float64.  The device rounds to fp32 at most after: the rep product / quotient (magnitude |x| R, R = max(rep, 1 / rep)),
the presence difference (<= |x| R + |p|), frequency * count (|f| c; the count itself converts exactly), their difference (<= M = |x| R + |p| +
|f| c) and the quotient by t (M / t): relative 2^-24 each, together at most (3 M + |x| R) 2^-24 / t <= 4 M 2^-24 / t.  So
    |got - want64| <= 4 * 2^-24 * (|x| R + |p| + |f| c) / t + 2^-126        (the last term: results in the denormal range)
and an uncounted element at t == 1 comes back bit for bit.  A count that is off by one moves a logit by |f| / t; check_penalty_scenario
asserts that this is more than the bounds at c and c + 1 together for every fed token of a row with |f| >= 0.01 and |x| <= 1000.

Samplers (specification: the comments in k_sample.hip and DESIGN.md "numerics", sampler row).  x = fp32(logit * fp32(1 / t)) is the one fp32
step the reference repeats (it fixes which values tie); from x on everything is float64: greedy = the first maximum and
logprob = -log(sum exp(x - max)); top-k / top-p as decision_margins of tests/test_gpu_sampler_exact.py, for any V, k > V and -inf entries.  A
row's margin is its distance from the two cumulative-mass decisions, taken over the edges that decide something: the edge at the last
candidate that carries mass decides nothing (target = rnd * kept mass lies below the kept mass for every rnd < 1, and a pick past the kept
prefix is clamped to its last candidate; the prefix reaches top_p there or ends there), and a candidate of zero mass (a masked, -inf logit)
adds no edge.  Tokens are compared where the margin is >= 3e-6, the other rows are counted, at most 4 % per case family (both numbers are
those of tests/test_gpu_sampler_exact.py); greedy rows are always compared (the cases plant a gap >= 1.0 or an exact tie).  Every row,
compared or not, must name a token in [0, V) that is one of the reference's candidates and carries mass -- never a masked one -- and a
logprob within 2e-4 of x[token] - logsumexp(x).

Guards (conditions, not tolerances): rows lie `stride` >= vocab floats apart; the columns [vocab, stride), the floats in front of a misaligned
base and a canary row after the last batch row hold poison (+inf for the samplers: a read past vocab wins the arg-max; a NaN pattern for the
penalty, which must come back bit for bit); out_tok / out_logprob carry canaries after `batch`; count-map rows no batch row names hold a
pseudo-random pattern.
"""
import numpy as np

U = 2.0 ** -24
DENORM = 2.0 ** -126
PEN_POISON = 0x7FD5A5A5       # NaN pattern behind vocab and in the canary row (penalty)
TOK_CANARY = 0x5A5A5A5A
LP_CANARY = 0x7FA5A5A5
MARGIN = 3e-6                 # tests/test_gpu_sampler_exact.py
UNCOMPARED_CAP = 0.04
LOGPROB_BAR = 2e-4
TOPK_MAX = 1024
RND_TOP = np.float32(1.0 - 2.0 ** -24)
DETECT_FREQ = 0.01
DETECT_X = 1000.0


class Lazy:
    """a case by name; build() makes it (the large ones are not kept)"""

    def __init__(self, name, family, make):
        self.name, self.family, self.make = name, family, make

    def build(self):
        c = self.make()
        assert c.name == self.name and c.family == self.family, (c.name, self.name)
        return c


# =====================================================================================================================
# penalty
# =====================================================================================================================
class PStep:
    """one launch: slots / start_pos [B], tokens [T] with seq_starts [B + 1], decoding_batches, per-row parameters (float32 [B] or None) and
    the logits [B, vocab] it is applied to"""

    def __init__(self, slots, seqs, start_pos, dec, logits, temps=None, rep=None, pres=None, freq=None):
        self.slots = np.asarray(slots, dtype=np.int64)
        self.B = len(self.slots)
        self.tokens = np.concatenate([np.asarray(s, dtype=np.int64) for s in seqs]) if seqs else np.zeros(0, dtype=np.int64)
        self.seq_starts = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
        self.start_pos = np.asarray(start_pos, dtype=np.int64)
        self.dec = int(dec)
        self.logits = np.ascontiguousarray(logits, dtype=np.float32)
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        self.temps, self.rep, self.pres, self.freq = f(temps), f(rep), f(pres), f(freq)

    def seq(self, b):
        return self.tokens[self.seq_starts[b]:self.seq_starts[b + 1]]


class PScenario:
    def __init__(self, name, family, vocab, stride, nslots, cm0, steps):
        self.name, self.family, self.vocab, self.stride, self.nslots, self.cm0, self.steps = name, family, vocab, stride, nslots, cm0, steps


def penalty_ref_step(cm, st, vocab):
    """the specification on one step: (count map after, float64 logits [B, vocab], bound [B, vocab], counts used [B, vocab])"""
    cm = cm.copy()
    want = np.empty((st.B, vocab), dtype=np.float64)
    bound = np.empty((st.B, vocab), dtype=np.float64)
    counts = np.empty((st.B, vocab), dtype=np.int64)
    for b in range(st.B):
        row = cm[st.slots[b]].astype(np.int64)
        if st.start_pos[b] == 0 or b >= st.dec:
            row[:] = 0
        row = np.minimum(row + np.bincount(st.seq(b), minlength=vocab), 65535)
        cm[st.slots[b]] = row.astype(np.uint16)
        x = st.logits[b].astype(np.float64)
        t = float(st.temps[b]) if st.temps is not None and st.temps[b] > 0 else 1.0
        r = float(st.rep[b]) if st.rep is not None else 1.0
        p = float(st.pres[b]) if st.pres is not None else 0.0
        f = float(st.freq[b]) if st.freq is not None else 0.0
        y = np.where(x > 0, x / r, x * r) - p - f * row
        want[b] = np.where(row > 0, y, x) / t
        bound[b] = 4 * U * (np.abs(x) * max(r, 1 / r) + abs(p) + abs(f) * row) / t + DENORM
        counts[b] = row
    return cm, want, bound, counts


def penalty_image(sc, st):
    """the logits buffer of a step as uint32 bit patterns: B rows of `stride` + one canary row, poison behind vocab"""
    img = np.full((st.B + 1, sc.stride), PEN_POISON, dtype=np.uint32)
    img[:st.B, :sc.vocab] = st.logits.view(np.uint32)
    return img


def check_penalty_scenario(sc):
    """the builder's conditions (AssertionError): ids and slots in range (the kernel trusts them), the poison placed, an off-by-one count
    detectable.  Returns the per-step reference results."""
    V = sc.vocab
    assert V % 2 == 0 and sc.stride >= V and sc.cm0.shape == (sc.nslots, V) and sc.cm0.dtype == np.uint16, sc.name
    cm, out = sc.cm0, []
    for si, st in enumerate(sc.steps):
        assert st.B >= 1 and st.logits.shape == (st.B, V), (sc.name, si)
        assert st.tokens.size == 0 or (st.tokens.min() >= 0 and st.tokens.max() < V), (sc.name, si, "token id out of range")
        assert st.slots.min() >= 0 and st.slots.max() < sc.nslots and len(set(st.slots.tolist())) == st.B, (sc.name, si, "slots")
        assert st.seq_starts[0] == 0 and (np.diff(st.seq_starts) >= 0).all() and st.seq_starts[-1] == st.tokens.size, (sc.name, si)
        assert 0 <= st.dec <= st.B and (st.start_pos >= 0).all(), (sc.name, si)
        assert np.isfinite(st.logits).all(), (sc.name, si)
        img = penalty_image(sc, st)
        assert (img[:, V:] == PEN_POISON).all() and (img[st.B] == PEN_POISON).all(), (sc.name, si, "poison")
        cm, want, bound, counts = penalty_ref_step(cm, st, V)
        assert np.isfinite(want).all(), (sc.name, si)
        for b in range(st.B):
            f = abs(float(st.freq[b])) if st.freq is not None else 0.0
            fed = np.unique(st.seq(b))
            if f < DETECT_FREQ or fed.size == 0:
                continue
            t = float(st.temps[b]) if st.temps is not None and st.temps[b] > 0 else 1.0
            fed = fed[np.abs(st.logits[b, fed]) <= DETECT_X]
            assert fed.size, (sc.name, si, b, "no fed token with a moderate logit")
            step_up = 4 * U * f / t                                    # bound(c + 1) - bound(c)
            assert (f / t > 2 * bound[b, fed] + step_up).all(), (sc.name, si, b, "an off-by-one count hides inside the bound")
        out.append((cm, want, bound, counts))
    return out


def check_penalty_step(sc, st, got_img, got_cm, ref):
    """device results of one step against the reference: list of failure texts"""
    cm, want, bound, counts = ref
    V, fails = sc.vocab, []
    if not (got_cm == cm).all():
        bad = np.argwhere(got_cm != cm)
        s, v = bad[0]
        fails.append(f"count map differs at {len(bad)} places, first slot {s} token {v}: got {got_cm[s, v]} want {cm[s, v]}")
    if not (got_img[:, V:] == PEN_POISON).all():
        fails.append("columns behind vocab were written")
    if not (got_img[st.B] == PEN_POISON).all():
        fails.append("the canary row was written")
    got = got_img[:st.B, :V].view(np.float32)
    err = np.abs(got.astype(np.float64) - want)
    over = ~(err <= bound)
    if over.any():
        b, v = np.argwhere(over)[0]
        fails.append(f"{int(over.sum())} logits over the bound, first row {b} token {v}: in {st.logits[b, v]!r} got {got[b, v]!r} want {want[b, v]!r} "
                     f"bound {bound[b, v]:.3g} count {counts[b, v]}")
    for b in range(st.B):
        if st.temps is None or not st.temps[b] > 0 or st.temps[b] == 1:
            same = counts[b] == 0
            if not (got_img[b, :V][same] == st.logits[b].view(np.uint32)[same]).all():
                fails.append(f"row {b}: uncounted logits at temperature 1 are not bit-identical")
    return fails


def _pattern(rng, shape):
    return rng.randint(0, 65536, size=shape).astype(np.uint16)


def _fresh_map(rng, nslots, vocab, used, preload=24):
    """pseudo-random pattern in the rows nobody names; the used rows hold a previous owner's sparse counts"""
    cm = _pattern(rng, (nslots, vocab))
    for s in used:
        cm[s] = 0
        idx = rng.choice(vocab, size=min(preload, vocab), replace=False)
        cm[s, idx] = rng.randint(1, 300, size=idx.size)
    return cm


def _params(rng, B, temps="mixed", rep=True, pres=True, freq=True):
    t = None
    if temps == "mixed":
        t = np.array([(1.0, 0.7, 0.0, -1.5, 2.0, 1.3)[b % 6] for b in range(B)])
    elif temps == "one":
        t = np.ones(B)
    r = np.array([(1.2, 0.8, 1.0, 2.0, 0.5)[b % 5] for b in range(B)]) if rep else None
    p = np.array([(0.5, -0.25, 0.0, 1.5)[b % 4] for b in range(B)]) if pres else None
    f = np.array([(0.3, 0.02, 0.11, -0.05)[b % 4] for b in range(B)]) if freq else None
    return dict(temps=t, rep=r, pres=p, freq=f)


def _logits(rng, B, V):
    return (rng.randn(B, V) * 3.0).astype(np.float32)


def _interleave(a, na, b, nb):
    out = []
    for i in range(max(na, nb)):
        if i < na:
            out.append(a)
        if i < nb:
            out.append(b)
    return out


def contention_scenarios():
    out = []
    for V in (1024,):
        for a in (0, V - 2):
            for na, nb in ((1, 3), (255, 256), (256, 255), (257, 4000), (4000, 257)):
                rng = np.random.RandomState(V + a + na)
                nsl = 4
                s0 = 1 if a == 0 else 2                  # the second row owns the slot on the side of the map this word touches
                s1 = 0 if a == 0 else 3
                nb_tok = (V - 2, V - 1) if a == 0 else (0, 1)
                other = _interleave(nb_tok[0], 37, nb_tok[1], 300)
                cm0 = _fresh_map(rng, nsl, V, [s0, s1])
                steps = [PStep([s0, s1], [_interleave(a, na, a ^ 1, nb), other], [0, 0], 0, _logits(rng, 2, V), **_params(rng, 2)),
                         PStep([s1, s0], [[nb_tok[1]], [a]], [337, na + nb], 2, _logits(rng, 2, V), **_params(rng, 2)),
                         PStep([s0, s1], [[a ^ 1], [nb_tok[0]]], [na + nb + 1, 338], 2, _logits(rng, 2, V), **_params(rng, 2))]
                out.append(PScenario(f"contend-V{V}-a{a}-n{na}x{nb}", "contention", V, V + 2 * (na % 2), nsl, cm0, steps))
    return out


SAT_PRELOADS = [(p, half, other) for p in (65533, 65534, 65535) for half in (0, 1) for other in (0, 65535)]


def saturation_scenarios():
    out = []
    V, nsl = 1024, 3
    for burst in (True, False):
        rng = np.random.RandomState(77 + burst)
        cm0 = _fresh_map(rng, nsl, V, [1], preload=0)
        toks = []
        for i, (p, half, other) in enumerate(SAT_PRELOADS):
            tok = 2 * (5 + 41 * i) + half
            cm0[1, tok], cm0[1, tok ^ 1] = p, other
            toks.append(tok)
        # (word 0 and the last word of the row as well: the neighbours are the adjacent slots' pattern)
        cm0[1, 0], cm0[1, 1], cm0[1, V - 2], cm0[1, V - 1] = 65534, 65535, 65535, 65534
        toks += [0, V - 1]
        kw = dict(temps=np.array([0.8]), rep=np.array([1.1]), pres=np.array([0.4]), freq=np.array([0.02]))
        if burst:
            seq = [t for _ in range(3) for t in toks]
            steps = [PStep([1], [seq], [9], 1, _logits(rng, 1, V), **kw)]
        else:
            steps = [PStep([1], [toks], [9 + i * len(toks)], 1, _logits(rng, 1, V), **kw) for i in range(3)]
        out.append(PScenario("saturate-" + ("burst" if burst else "steps"), "saturation", V, V + 6, nsl, cm0, steps))
    return out


def _req_tokens(rng, V, n, pool=6):
    """n tokens drawn from a small pool: counts above 1"""
    return rng.choice(rng.choice(V, size=min(pool, V), replace=False), size=n).tolist()


def clear_rule_scenarios():
    out = []
    V, nsl = 1024, 7
    rng = np.random.RandomState(5)
    # one launch with every rule: decode rows first (kept), a row b < decoding_batches at start_pos 0 (cleared), a fresh prefill
    # (cleared) and a prefix hit in a reused slot (b >= decoding_batches, start_pos > 0: cleared)
    slots = [6, 2, 4, 0, 3]
    cm0 = _fresh_map(rng, nsl, V, slots, preload=40)
    seqs = [[int(np.flatnonzero(cm0[6])[0])], [int(np.flatnonzero(cm0[2])[3])], [11], _req_tokens(rng, V, 9), _req_tokens(rng, V, 5)]
    steps = [PStep(slots, seqs, [17, 40, 0, 0, 16], 3, _logits(rng, 5, V), **_params(rng, 5)),
             PStep(slots[::-1], [[int(s[-1])] for s in seqs[::-1]], [21, 9, 1, 41, 18], 5, _logits(rng, 5, V), **_params(rng, 5))]
    out.append(PScenario("clear-every-rule", "clear", V, V + 2, nsl, cm0, steps))

    # requests come and go: B ends and D takes its slot with a prefix hit; A ends and E takes its slot from position 0
    rng = np.random.RandomState(6)
    A, B_, C, D, E = 3, 0, 6, 0, 3
    cm0 = _fresh_map(rng, nsl, V, [0, 3, 6], preload=40)
    pr = {k: _req_tokens(rng, V, n) for k, n in (("A", 12), ("B", 7), ("C", 20), ("D", 4), ("E", 9))}
    nxt = lambda k: [int(rng.choice(pr[k]))]
    L = lambda B: _logits(rng, B, V)
    P = lambda B: _params(rng, B)
    steps = [PStep([A, B_], [pr["A"], pr["B"]], [0, 0], 0, L(2), **P(2)),
             PStep([A, B_], [nxt("A"), nxt("B")], [12, 7], 2, L(2), **P(2)),
             PStep([A, B_, C], [nxt("A"), nxt("B"), pr["C"]], [13, 8, 0], 2, L(3), **P(3)),
             PStep([A, C, D], [nxt("A"), nxt("C"), pr["D"]], [14, 20, 8], 2, L(3), **P(3)),          # D: prefix hit in B's old slot
             PStep([A, C, D], [nxt("A"), nxt("C"), nxt("D")], [15, 21, 12], 3, L(3), **P(3)),
             PStep([C, D, E], [nxt("C"), nxt("D"), pr["E"]], [22, 13, 0], 2, L(3), **P(3)),          # E: A's old slot, from position 0
             PStep([C, D, E], [nxt("C"), nxt("D"), nxt("E")], [23, 14, 9], 3, L(3), **P(3))]
    out.append(PScenario("clear-lifecycle", "clear", V, V, nsl, cm0, steps))
    return out


SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 1.5e-38, -1.5e-38, 1e30, -1e30, 3.0, -3.0, 2.0 ** -20, -2.0 ** -20, 60000.0, -60000.0]


def logit_rule_scenarios():
    out = []
    V, B = 1024, 10
    variants = [("all", {}), ("no-presence", dict(pres=False)), ("no-frequency", dict(freq=False)), ("no-temperature", dict(temps=None)),
                ("no-rep", dict(rep=False)), ("temperature-one", dict(temps="one"))]
    for vi, (name, kw) in enumerate(variants):
        rng = np.random.RandomState(300 + vi)
        cm0 = _fresh_map(rng, B + 2, V, range(1, B + 1))
        steps = []
        for si in range(2):
            lg = _logits(rng, B, V)
            seqs = []
            for b in range(B):
                pos = rng.choice(V, size=len(SPECIALS) + 4, replace=False)
                lg[b, pos[:len(SPECIALS)]] = np.array(SPECIALS, dtype=np.float32)
                lg[b, pos[len(SPECIALS) - 2] ^ 1] = np.float32(SPECIALS[b % len(SPECIALS)])     # an uncounted neighbour holds one too
                seqs.append(np.repeat(pos, 1 + b % 3).tolist() if si == 0 else [int(pos[b % len(pos)]), int(pos[-1])])
            steps.append(PStep(np.arange(1, B + 1), seqs, [0] * B if si == 0 else [50] * B, 0 if si == 0 else B, lg, **_params(rng, B, **kw)))
        out.append(PScenario("logit-rule-" + name, "logit", V, V + 2 * (vi % 2), B + 2, cm0, steps))
    return out


SHAPE_GRID = [(V, V + ds, B) for V in (2, 1024, 32000) for ds in (0, 2, 6) for B in (1, 8, 64)] + \
             [(128256, 128256, 1), (128256, 128258, 8), (128256, 128262, 64)]


def shape_scenarios():
    out = []
    for V, stride, B in SHAPE_GRID:
      def make(V=V, stride=stride, B=B):
        rng = np.random.RandomState(V % 9973 + stride + B)
        nsl = B + 2
        slots = rng.permutation(nsl)[:B]
        if nsl - 1 not in slots:
            slots[0] = nsl - 1                           # the highest slot is in use
        cm0 = _fresh_map(rng, nsl, V, slots)
        lens = rng.randint(1, 48, size=B)
        seqs = [_req_tokens(rng, V, n, pool=5) + [0, V - 1] for n in lens]
        steps = [PStep(slots, seqs, [0] * B, 0, _logits(rng, B, V), **_params(rng, B)),
                 PStep(slots, [[int(s[b % len(s)])] for b, s in enumerate(seqs)], lens + 2, B, _logits(rng, B, V), **_params(rng, B))]
        return PScenario(f"shape-V{V}-s{stride}-B{B}", "shape", V, stride, nsl, cm0, steps)
      out.append(Lazy(f"shape-V{V}-s{stride}-B{B}", "shape", make))
    return out


def penalty_scenarios():
    """every penalty scenario, as Lazy"""
    small = [s for f in (contention_scenarios, saturation_scenarios, clear_rule_scenarios, logit_rule_scenarios) for s in f()]
    return [Lazy(s.name, s.family, lambda s=s: s) for s in small] + shape_scenarios()


def clears_only_at_position_zero(sc):
    """no row is cleared by the second rule alone (b >= decoding_batches at start_pos > 0)"""
    return all(not (st.start_pos[b] > 0 and b >= st.dec) for st in sc.steps for b in range(st.B))


def run_penalty_gpu(m, torch, sc):
    """every step of a scenario on the device, on one count map"""
    refs = check_penalty_scenario(sc)                    # (also: every id and slot is in range before anything is launched)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    d_cm = torch.from_numpy(sc.cm0.view(np.int16).copy()).cuda()
    fails = []
    for si, st in enumerate(sc.steps):
        d_lg = torch.from_numpy(penalty_image(sc, st).view(np.int32)).cuda()
        d = [dev(a) for a in (st.temps, st.rep, st.pres, st.freq, st.slots, st.tokens, st.seq_starts, st.start_pos)]
        torch.cuda.synchronize()
        rc = m.lib().pplhip_op_penalty(None, d_lg.data_ptr(), *[ptr(t) for t in d], st.B, sc.vocab, sc.stride, st.dec, d_cm.data_ptr())
        torch.cuda.synchronize()
        if rc:
            return [f"step {si}: pplhip_op_penalty -> {rc}"]
        got_img = d_lg.cpu().numpy().view(np.uint32)
        got_cm = d_cm.cpu().numpy().view(np.uint16)
        fails += [f"step {si}: {f}" for f in check_penalty_step(sc, st, got_img, got_cm, refs[si])]
        if fails:
            break
    return fails


# =====================================================================================================================
# samplers
# =====================================================================================================================
def scaled(row, t):
    """x = fp32(logit * fp32(1 / t)), t NULL or <= 0: 1"""
    t = np.float32(t) if t is not None and t > 0 else np.float32(1.0)
    return (row.astype(np.float32) * (np.float32(1.0) / t)).astype(np.float32)


def _lse(x):
    mx = float(x.max())
    return mx + float(np.log(np.exp(x.astype(np.float64) - mx).sum()))


def greedy_ref(x):
    """(token, logprob, gap to the best other entry) of a scaled row"""
    tok = int(np.argmax(x))
    if x.size == 1:
        return tok, 0.0, np.inf
    rest = x.copy()
    rest[tok] = -np.inf
    return tok, float(x[tok]) - _lse(x), float(x[tok]) - float(rest.max())


def topk_ref(x, top_k, top_p, rnd):
    """float64 pick rule on a scaled row: (token, margin, the candidates that carry mass, logsumexp)"""
    V = x.size
    full = top_k <= 0
    k = min(TOPK_MAX if full else min(top_k, TOPK_MAX), V)
    order = np.argsort(-x, kind="stable")[:k]
    mx = float(x.max())
    e = np.exp(x[order].astype(np.float64) - mx)
    n_eff = int(np.count_nonzero(e))                     # (sorted: the massless candidates are last)
    tot = np.exp(x.astype(np.float64) - mx).sum() if full else e.sum()
    cum = np.cumsum(e / tot)
    hit = np.flatnonzero(cum >= float(top_p))
    keep = int(hit[0]) + 1 if hit.size else k
    n_keep = min(keep, n_eff - 1)                        # the edges that decide something lie in front of the last candidate with mass ...
    m_keep = float(np.abs(cum[:n_keep] - float(top_p)).min()) if n_keep > 0 else np.inf
    c = np.cumsum(e[:keep])
    target = float(rnd) * c[-1]
    n_pick = min(keep, n_eff) - 1                        # ... and, for the pick, in front of the last kept one
    sel = min(int(np.searchsorted(c, target, side="right")), n_pick)
    m_pick = float(np.abs(c[:n_pick] - target).min() / c[-1]) if n_pick > 0 else np.inf
    return int(order[sel]), min(m_keep, m_pick), order[:n_eff], mx + float(np.log(np.exp(x.astype(np.float64) - mx).sum()))


class SCase:
    """one launch of pplhip_op_sample: B rows of V logits, rows `stride` apart, the base `off` floats past a 16-byte boundary"""

    def __init__(self, name, family, logits, stride, off, top_k, top_p=0.0, top_p_list=None, temps=None, rnd=None, expect=None):
        self.name, self.family = name, family
        self.logits = np.ascontiguousarray(logits, dtype=np.float32)
        self.B, self.V = self.logits.shape
        self.stride, self.off, self.top_k, self.top_p = stride, off, top_k, float(top_p)
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        self.top_p_list, self.temps, self.rnd = f(top_p_list), f(temps), f(rnd)
        self.expect = expect                              # greedy: the planted answer of every row

    def x(self, b):
        return scaled(self.logits[b], None if self.temps is None else self.temps[b])

    def tp(self, b):
        return self.top_p if self.top_p_list is None else float(self.top_p_list[b])

    def image(self):
        img = np.full(4 + (self.B + 1) * self.stride + 4, np.inf, dtype=np.float32)
        for b in range(self.B):
            img[self.off + b * self.stride:self.off + b * self.stride + self.V] = self.logits[b]
        return img

    def reference(self):
        """per row (token, logprob, margin or gap, candidates or None)"""
        rows = []
        for b in range(self.B):
            x = self.x(b)
            if self.top_k == 1:
                tok, lp, gap = greedy_ref(x)
                rows.append((tok, lp, gap, None))
            else:
                tok, margin, cand, lse = topk_ref(x, self.top_k, self.tp(b), self.rnd[b])
                rows.append((tok, float(x[tok]) - lse, margin, cand))
        return rows

    def check_assertions(self):
        """the builder's conditions; returns (reference rows, number of uncompared rows)"""
        assert 0 <= self.off <= 3 and self.stride >= self.V and self.V >= 1
        img = self.image()
        mask = np.ones(img.size, dtype=bool)
        for b in range(self.B):
            mask[self.off + b * self.stride:self.off + b * self.stride + self.V] = False
        assert np.isposinf(img[mask]).all() and mask.sum() == img.size - self.B * self.V, (self.name, "poison")
        assert not np.isnan(self.logits).any() and not np.isposinf(self.logits).any(), self.name
        assert (self.logits.max(axis=1) > -np.inf).all(), (self.name, "a row without a finite entry")
        rows = self.reference()
        if self.top_k == 1:
            for b, (tok, lp, gap, _) in enumerate(rows):
                assert gap >= 1.0 or gap == 0.0, (self.name, b, gap)
                assert self.expect is None or tok == self.expect[b], (self.name, b, tok, self.expect[b])
            return rows, 0
        assert self.rnd is not None and (self.rnd >= 0).all() and (self.rnd < 1).all(), self.name
        return rows, sum(1 for r in rows if r[2] < MARGIN)

    def uses_vector_path(self):
        return self.stride % 4 == 0 and self.off == 0


def check_sample(c, rows, tok, lp, tok_tail, lp_tail):
    fails = []
    if not (tok_tail == TOK_CANARY).all() or not (lp_tail == LP_CANARY).all():
        fails.append("canaries behind out_tok / out_logprob were written")
    for b, (wtok, wlp, margin, cand) in enumerate(rows):
        t = int(tok[b])
        if not 0 <= t < c.V:
            fails.append(f"row {b}: token {t} is outside [0, {c.V})")
            continue
        x = c.x(b)
        if c.top_k == 1 or margin >= MARGIN:
            if t != wtok:
                fails.append(f"row {b}: token {t} (x {x[t]!r}) want {wtok} (x {x[wtok]!r}) margin {margin:.3g}")
                continue
        elif t not in cand:
            fails.append(f"row {b}: token {t} (x {x[t]!r}) is no candidate that carries mass")
            continue
        want_lp = float(x[t]) - _lse(x) if t != wtok else wlp
        if not abs(float(lp[b]) - want_lp) <= LOGPROB_BAR:
            fails.append(f"row {b}: logprob {float(lp[b])!r} want {want_lp!r}")
    return fails


def run_sample_gpu(m, torch, c, rows=None):
    rows = c.check_assertions()[0] if rows is None else rows
    d = torch.from_numpy(c.image()).cuda()
    assert d.data_ptr() % 16 == 0
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    d_t, d_p, d_r = dev(c.temps), dev(c.top_p_list), dev(c.rnd)
    d_tok = torch.from_numpy(np.full(c.B + 8, TOK_CANARY, dtype=np.int32)).cuda()
    d_lp = torch.from_numpy(np.full(c.B + 8, LP_CANARY, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    rc = m.lib().pplhip_op_sample(None, d.data_ptr() + 4 * c.off, ptr(d_t), ptr(d_p), ptr(d_r), c.B, c.V, c.stride, c.top_k, c.top_p,
                                  d_tok.data_ptr(), d_lp.data_ptr())
    torch.cuda.synchronize()
    if rc:
        return [f"pplhip_op_sample -> {rc}"]
    tok = d_tok.cpu().numpy()
    lp = d_lp.cpu().numpy()
    return check_sample(c, rows, tok[:c.B], lp[:c.B].view(np.float32), tok[c.B:], lp[c.B:].view(np.uint32))


# ---- greedy ---------------------------------------------------------------------------------------------------------
GREEDY_V = [1, 2, 3, 5, 255, 1023, 1024, 1025, 4097, 16385, 32000, 32001, 32003, 128256]
SG_THREADS = 1024             # k_sample.hip: threads of the greedy kernel, each with four 16-byte loads in flight
TEMPS = [1.0, 0.0, -1.0, 0.5, 2.0, 0.7]


def next8(V):
    return (V // 8 + 1) * 8


def layouts(V, thin):
    """(stride, base offset in floats)"""
    if thin:
        return [(V, 0), (V + 1, 0), (V + 3, 2), (next8(V), 0), (next8(V), 3), (V, 1)]
    return [(s, o) for s in (V, V + 1, V + 3, next8(V)) for o in range(4)]


def u3_chunks(V):
    """float4 chunks that only the fourth unrolled load reaches (chunk % 4096 >= 3072): (the first, the last), or () when there is none"""
    nv = V // 4
    if nv <= 3 * SG_THREADS:
        return ()
    last = nv - 1
    if last % (4 * SG_THREADS) < 3 * SG_THREADS:
        last = last // (4 * SG_THREADS) * 4 * SG_THREADS - 1
    return (3 * SG_THREADS + 5, last)


def guard_entered(V):
    """the `c < nv` guard of the 4-deep unroll is false for some thread: the float4 chunks do not fill the last round of 4096"""
    return (V // 4) % (4 * SG_THREADS) != 0


def greedy_plants(V):
    """[(kind, positions holding the maximum)]: the first position is the answer"""
    nv = V // 4
    p = [("first", [0]), ("last", [V - 1])]
    if nv:
        p.append(("last-float4", [4 * (nv - 1)]))
    p += [(f"tail{i - 4 * nv}", [i]) for i in range(4 * nv, V)]
    for j, c in enumerate(u3_chunks(V)):
        p.append((f"u3-{j}", [4 * c + 1 + j]))
    if V > 4 * nv and nv:
        p.append(("tie-vec-tail", [4 * (nv // 2) + 1, 4 * nv]))
    if V >= 2:
        p.append(("tie-ends", [0, V - 1]))
    if V >= 8:
        p.append(("tie-mid", [V // 2, V // 2 + 3]))
    return p


def greedy_cases():
    out = []
    for V in GREEDY_V:
        for li, (stride, off) in enumerate(layouts(V, thin=V > 4097)):
            def make(V=V, li=li, stride=stride, off=off):
                rng = np.random.RandomState(V * 31 + stride * 7 + off)
                rows, expect = [], []
                for kind, pos in greedy_plants(V):
                    r = (rng.randn(V) * 2.0).astype(np.float32)
                    r[pos] = np.float32(18.0)
                    rows.append(r)
                    expect.append(pos[0])
                # all negative (a zero that is not there would win), and rows masked down to one entry
                for pos in sorted({0, V - 1, 4 * (V // 4) if V % 4 else V // 2}):
                    r = (rng.randn(V) * 2.0 - 40.0).astype(np.float32)
                    r[pos] = np.float32(-22.0)
                    rows.append(r)
                    expect.append(pos)
                    r = np.full(V, -np.inf, dtype=np.float32)
                    r[pos] = np.float32(-3.0)
                    rows.append(r)
                    expect.append(pos)
                B = len(rows)
                temps = None if li % 3 == 2 else np.array([TEMPS[(b + li) % len(TEMPS)] for b in range(B)], dtype=np.float32)
                return SCase(f"greedy-V{V}-s{stride}-o{off}", "greedy", np.stack(rows), stride, off, 1, temps=temps, expect=expect)
            out.append(Lazy(f"greedy-V{V}-s{stride}-o{off}", "greedy", make))
    return out


# ---- top-k / top-p --------------------------------------------------------------------------------------------------
TOPK_KS = [2, 8, 50, 1024, 5000, 0, -3]
TOPK_PS = [-1.0, 0.0, 0.25, 0.9, 1.0, 2.0]
RNDS = [0.0, 0.5, RND_TOP]


def _rnd(rng, B):
    r = rng.rand(B).astype(np.float32)
    r[r >= 1] = 0.5
    r[:9] = RNDS * 3
    return r


def _layout(V, i):
    return [(V, 0), (V + 1, 1), (V + 3, 2), (next8(V), 0), (next8(V), 3), (V, 3)][i % 6]


def topk_grid_cases():
    out = []
    n = 0
    for V in (3, 5, 255, 1023, 1024, 1025, 4097, 32000, 32003, 128256):
        for ki, k in enumerate(TOPK_KS):
            stride, off = _layout(V, n)

            def make(V=V, ki=ki, k=k, n=n, stride=stride, off=off):
                rng = np.random.RandomState(1000 + V + 17 * ki)
                B = 18
                keff = min(V, TOPK_MAX if k <= 0 else min(k, TOPK_MAX))
                scale = 2.5 if keff <= 64 else (1.0 if keff < V else 0.3)       # the last candidate keeps a share above the margin
                lg = (rng.randn(B, V) * scale).astype(np.float32)
                per_row = n % 2 == 0
                tpl = np.array([TOPK_PS[(b // 3 + n) % len(TOPK_PS)] for b in range(B)]) if per_row else None
                tp0 = 0.5 if per_row else TOPK_PS[n // 2 % len(TOPK_PS)]
                temps = None if n % 3 == 0 else np.array([TEMPS[(b + n) % len(TEMPS)] for b in range(B)])
                return SCase(f"topk-V{V}-k{k}-s{stride}-o{off}", "topk-grid", lg, stride, off, k, tp0, tpl, temps, _rnd(rng, B))
            out.append(Lazy(f"topk-V{V}-k{k}-s{stride}-o{off}", "topk-grid", make))
            n += 1
    return out


def topk_small_cases():
    """V < 256 with k > V, k == V and k < V"""
    out = []
    n = 0
    for V, ks in ((1, (2, 0)), (2, (2, 8, -3)), (3, (2, 50)), (5, (5, 1024, 0)), (100, (8, 100, 5000)), (255, (50, 255, 1024, 0))):
        for k in ks:
            stride, off = _layout(V, n + 1)

            def make(V=V, k=k, n=n, stride=stride, off=off):
                rng = np.random.RandomState(2000 + V * 13 + n)
                B = 18
                lg = (rng.randn(B, V) * (2.0 if V <= 5 else 0.5)).astype(np.float32)
                tpl = np.array([TOPK_PS[(b // 3 + n) % len(TOPK_PS)] for b in range(B)])
                return SCase(f"topk-small-V{V}-k{k}-s{stride}-o{off}", "topk-small", lg, stride, off, k, 0.9, tpl, None, _rnd(rng, B))
            out.append(Lazy(f"topk-small-V{V}-k{k}-s{stride}-o{off}", "topk-small", make))
            n += 1
    return out


def topk_masked_cases():
    """fewer finite entries than k: the masked ones are candidates (they fill the k) and must never be the answer"""
    out = []
    n = 0
    for V in (255, 1025, 32003):
        for k in (8, 50, 1024, 0):
            stride, off = _layout(V, n)

            def make(V=V, k=k, n=n, stride=stride, off=off):
                keff = min(V, TOPK_MAX if k <= 0 else k)
                rng = np.random.RandomState(3000 + V + k)
                rows, tps, rnds = [], [], []
                for nf in sorted({1, 2, 3, max(1, keff // 2), keff - 1}):
                    if nf >= keff:
                        continue
                    for tp in (0.9, 1.0, 2.0):
                        for r in RNDS:
                            row = np.full(V, -np.inf, dtype=np.float32)
                            row[rng.choice(V, size=nf, replace=False)] = (rng.randn(nf) * 0.5 + 2.0).astype(np.float32)
                            rows.append(row)
                            tps.append(tp)
                            rnds.append(r)
                as_list = n % 2 == 0
                if not as_list:      # one default top_p for the launch
                    sel = [i for i, t in enumerate(tps) if t == (1.0, 2.0)[n // 2 % 2]]
                    rows, tps, rnds = [rows[i] for i in sel], [tps[i] for i in sel], [rnds[i] for i in sel]
                return SCase(f"topk-masked-V{V}-k{k}-s{stride}-o{off}", "topk-masked", np.stack(rows), stride, off, k,
                             tps[0], np.array(tps) if as_list else None, None, np.array(rnds))
            out.append(Lazy(f"topk-masked-V{V}-k{k}-s{stride}-o{off}", "topk-masked", make))
            n += 1
    return out


def topk_tie_cases():
    """`above` entries over a plateau of equal values that the candidate cut falls into, V % 256 != 0, plateau members at the row's end"""
    out = []
    n = 0
    for V in (1279, 4097, 32003):
        for k, n_ties, above in ((50, 300, 19), (8, 600, 1), (1024, 200, 900), (0, 700, 500), (5000, 2000, 1)):
            stride, off = _layout(V, n)

            def make(V=V, k=k, n_ties=n_ties, above=above, n=n, stride=stride, off=off):
                if above + n_ties > V:
                    n_ties = V - above - 8
                rng = np.random.RandomState(4000 + V + k)
                B = 12
                lg = (rng.randn(B, V) * 0.5 - 6.0).astype(np.float32)
                for b in range(B):
                    idx = rng.permutation(V - 3)
                    lg[b, idx[:above]] = (2.0 + rng.rand(above)).astype(np.float32)
                    lg[b, idx[above:above + n_ties - 3]] = np.float32(1.25)
                    lg[b, V - 3:] = np.float32(1.25)
                rnd = _rnd(rng, B)
                rnd[3:6] = RND_TOP                              # the pick is the LAST candidate: the plateau member on the cut
                temps = None if n % 2 else np.array([TEMPS[b % len(TEMPS)] for b in range(B)])
                return SCase(f"topk-ties-V{V}-k{k}-s{stride}-o{off}", "topk-ties", lg, stride, off, k, (1.0, 2.0)[n % 2], None, temps, rnd)
            out.append(Lazy(f"topk-ties-V{V}-k{k}-s{stride}-o{off}", "topk-ties", make))
            n += 1
    return out


TOPK_FAMILIES = ("topk-grid", "topk-small", "topk-masked", "topk-ties")


def topk_cases():
    return topk_grid_cases() + topk_small_cases() + topk_masked_cases() + topk_tie_cases()
