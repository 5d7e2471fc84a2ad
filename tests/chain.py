"""The post-processing chain of one step as a specification (DESIGN.md "the chain"): the existing references of the single stages, applied
in the order of LLMEngine::Execute, and the generator's per-row bookkeeping between two steps.  No arithmetic of its own and no tolerance of
its own: every number comes from tests/guide.py, tests/logit_rules.py, tests/postproc.py, tests/sample_rows.py and tests/top_logprobs.py.
Shared by tests/test_chain_spec.py (no GPU) and tests/test_gpu_chain.py.

  1. guide.ref_edit               rows with guide_slots[b] >= 0, row states[b] of that slot's masks
  2. logit_rules.ref_edit         rows with flags[b] != 0, the rule of batch slot slots[b]
  3. postproc.penalty_ref_step    every row, only when the penalty is on; it divides by the temperature
  4. top_logprobs.ref_row         rows with nlp[b] > 0; the answers stand in LIST order (the j-th asking row), not by batch row
  5. the sampler of sample_rows   every row; top_k == 1 is greedy

The temperature goes to stages 4 and 5 only when the penalty is off: with the penalty on, stage 3 has divided already.

A ChainState is what the generator keeps per batch row between steps; `advance` restates llm_generator.cc's loop over the step's tokens:
the draw counts up, the stop-suppress bit (flag bit 1) leaves once min_new_tokens tokens are out, a guided row walks its automaton over the
token's bytes (an end token leaves the state alone), the prompt ask is -1 from the second step on, and the next step feeds the token.

MUTANTS names one ordering or indexing mistake each; tests/test_chain_spec.py shows that every one of them changes a compared output on the
cases below.  PATTERNS is the row table: over two batches of eight rows every subset of {guide, rule, top-N, sampled} occurs once.
"""
import copy

import numpy as np

from tests import guide as G
from tests import logit_rules as R
from tests import postproc as P
from tests import sample_rows as S
from tests import top_logprobs as T

GUIDE, RULE, TOPN, SAMPLED = 1, 2, 4, 8
# batch 0: none at row 1, the greedy rule row 3 right behind the sampling row 2, every feature at row 4, guide only at row 5
# batch 1: the greedy row 1 right behind the sampling row 0
PATTERNS = ((RULE | TOPN, 0, SAMPLED, RULE, GUIDE | RULE | TOPN | SAMPLED, GUIDE, GUIDE | TOPN | SAMPLED, TOPN),
            (GUIDE | SAMPLED, GUIDE | RULE, RULE | SAMPLED, GUIDE | TOPN, RULE | TOPN | SAMPLED, GUIDE | RULE | TOPN, TOPN | SAMPLED,
             GUIDE | RULE | SAMPLED))
ROW_NONE, ROW_GREEDY_BEHIND_SAMPLING, ROW_ALL, ROW_GUIDE_ONLY = 1, 3, 4, 5      # of batch 0
# the batch slot of every row (the rule table's and the count map's row): never the identity.  A guided row's rule has no mask (slot % 4
# in (1, 2): the kinds "bias" and "stops" of the rule table below), as the generator admits no allow list beside a guide; an unguided rule
# row of either batch has a rule of stops alone (slots 2 and 6), whose tokens nothing else kills: the stop-suppress bit shows there
SLOTS = ((2, 4, 7, 0, 5, 3, 6, 1), (3, 1, 6, 0, 7, 2, 4, 5))
CAP = 8                                                  # batch slots
V = 1024
GUIDE_SLOTS, GUIDE_STATES, N_TOK, END = (3, 9), 6, 600, 2
STEPS = 6
TEMPS = (0.7, 1.3, 2.0, 0.5)
REP, PRES, FREQ = (1.2, 0.8, 1.5, 1.1), (0.5, -0.25, 0.3, 0.1), (0.3, 0.02, 0.11, 0.05)
NLP = (1, 5, 20, 3)
TOP_K, TOP_P = (50, 0, 8, 1024), (0.9, 1.0, 0.95, 0.5)
MIN_NEW = (2, 1, 3, 2)
SEED_BASE = 0x5EED0000C0FFEE + 11                        # tests/test_chain_spec.py: with these seeds no sampling row of a case is left uncompared

MUTANTS = ("penalty_before_rules", "topn_before_penalty", "temperature_twice", "topn_by_batch_row", "flags_with_next_slot",
           "stop_bit_never_cleared", "draw_not_incremented", "guide_state_not_advanced")
STEP_MUTANTS = MUTANTS[:5]                               # mistakes inside one step (ref_chain)
ADVANCE_MUTANTS = MUTANTS[5:]                            # mistakes between two steps (advance)
NEEDS_PENALTY = ("penalty_before_rules", "topn_before_penalty", "temperature_twice")


class Tables:
    """what is loaded once: a rule in every batch slot, two guides over one vocabulary"""

    def __init__(self):
        self.rules = {}
        for s in range(CAP):                             # every kind among them (tests/test_gpu_staging.py builds the same table)
            self.rules[s] = R._rule(np.random.default_rng(600 + s), V, R.KINDS[s % 4], R.N_BIAS[1 + s % 4], [1, V - 1, V, 40][s % 4])
        rng = np.random.default_rng(41)
        self.toks = G.random_vocab(rng, N_TOK)
        self.ends = [END]
        self.masks = np.zeros((G.MAX_SLOTS, GUIDE_STATES, G.words(V)), dtype=np.uint32)
        self.trans, self.accept = {}, {}
        for g in GUIDE_SLOTS:
            while True:                                  # (pplhip_guide_load wants a token for every state)
                trans, accept = G.random_dfa(rng, GUIDE_STATES)
                mask, anyf = G.ref_build(trans, accept, self.toks, self.ends, V)
                if anyf.all():
                    break
            self.trans[g], self.accept[g], self.masks[g] = trans, accept, mask

    def guide_allowed(self, g, s):
        return np.unpackbits(self.masks[g, s].view(np.uint8), bitorder="little")[:V].astype(bool)

    def assert_live(self):
        """a condition of the cases, not of the code under test: whatever state a guided row of PATTERNS reaches, its guide and its rule
        together leave a token alive (a row without one has no defined answer)"""
        for bi, pats in enumerate(PATTERNS):
            for b, p in enumerate(pats):
                if p & GUIDE and p & RULE:
                    rule = self.rules[SLOTS[bi][b]]
                    assert rule.mask is None, (bi, b)
                    for g in GUIDE_SLOTS:
                        for s in range(GUIDE_STATES):
                            live = np.isfinite(R.ref_edit(np.where(self.guide_allowed(g, s), 0, G.NINF).astype(np.float32), rule, 3))
                            assert live.sum() >= 1, (bi, b, g, s)


class ChainStep:
    """one step: the logits image [B, stride] (columns at or behind `vocab` belong to nobody) and every per-row list of the chain; seqs /
    start_pos / dec are the step inputs the penalty counts from (postproc.PStep)"""

    def __init__(self, logits, vocab, guide_slots, guide_states, slots, flags, rep, pres, freq, temps, nlp, top_k, top_p, seeds, draws,
                 seqs, start_pos, dec):
        self.logits = np.ascontiguousarray(logits, dtype=np.float32)
        self.B, self.stride = self.logits.shape
        self.vocab = vocab
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        self.guide_slots, self.guide_states, self.nlp, self.top_k = i32(guide_slots), i32(guide_states), i32(nlp), i32(top_k)
        self.slots = np.ascontiguousarray(slots, dtype=np.int64)
        self.flags = np.ascontiguousarray(flags, dtype=np.uint32)
        self.rep, self.pres, self.freq, self.temps, self.top_p = f32(rep), f32(pres), f32(freq), f32(temps), f32(top_p)
        self.seeds, self.draws = np.ascontiguousarray(seeds, dtype=np.uint64), np.ascontiguousarray(draws, dtype=np.uint64)
        self.seqs = [np.asarray(s, dtype=np.int64) for s in seqs]
        self.start_pos = np.ascontiguousarray(start_pos, dtype=np.int64)
        self.dec = int(dec)


class ChainState:
    """the per-row lists the generator carries from step to step, the count map and the tables"""

    def __init__(self, tables, batch, asking=None, nslots=CAP):
        """batch: index into PATTERNS.  asking: None (the table), () (nobody asks) or the rows that ask while the others ask for nothing"""
        self.tables = tables
        pats = PATTERNS[batch]
        B = self.B = len(pats)
        self.batch = batch
        ask = [asking is None or b in asking for b in range(B)]
        self.patterns = [p if ask[b] else 0 for b, p in enumerate(pats)]
        self.slots = list(SLOTS[batch])
        self.cm = np.zeros((nslots, V), dtype=np.uint16)
        self.guide_slots, self.guide_states, self.flags, self.min_new, self.nlp = [], [], [], [], []
        self.top_k, self.top_p, self.temps, self.rep, self.pres, self.freq = [], [], [], [], [], []
        for b, p in enumerate(self.patterns):
            self.guide_slots.append(GUIDE_SLOTS[b % 2] if p & GUIDE else -1)
            self.guide_states.append(0)
            self.flags.append(3 if p & RULE else 0)
            self.min_new.append(MIN_NEW[b % 4] if p & RULE else 0)
            self.nlp.append(NLP[b % 4] if p & TOPN else 0)
            self.top_k.append(TOP_K[b % 4] if p & SAMPLED else 1)
            self.top_p.append(TOP_P[b % 4] if p & SAMPLED else 0.0)
            plain = p == 0                               # a row that asks for nothing: neutral penalties, temperature 1
            self.temps.append(1.0 if plain else TEMPS[b % 4])
            self.rep.append(1.0 if plain else REP[b % 4])
            self.pres.append(0.0 if plain else PRES[b % 4])
            self.freq.append(0.0 if plain else FREQ[b % 4])
        m64 = (1 << 64) - 1
        self.seeds = [(SEED_BASE + 1000003 * batch + 7919 * b) & m64 for b in range(B)]
        self.draws = [0] * B
        self.gen = [0] * B
        self.prompt_ask = [-1] * B
        self.seqs, self.start_pos, self.dec = [[] for _ in range(B)], [0] * B, 0

    def copy(self):
        c = copy.copy(self)
        for k, v in vars(self).items():
            if isinstance(v, list):
                setattr(c, k, [list(x) if isinstance(x, list) else x for x in v])
        c.cm = self.cm.copy()
        return c

    def feed(self, seqs, start_pos, dec, prompt_ask=None):
        """the inputs of the next step (the first one: afterwards `advance` feeds the tokens)"""
        self.seqs, self.start_pos, self.dec = [list(map(int, s)) for s in seqs], [int(p) for p in start_pos], int(dec)
        if prompt_ask is not None:
            self.prompt_ask = [int(a) for a in prompt_ask]

    def step(self, logits):
        return ChainStep(logits, V, self.guide_slots, self.guide_states, self.slots, self.flags, self.rep, self.pres, self.freq, self.temps,
                         self.nlp, self.top_k, self.top_p, self.seeds, self.draws, self.seqs, self.start_pos, self.dec)


class ChainResult:
    pass


def _pstep(st, rows_vocab):
    return P.PStep(st.slots, st.seqs, st.start_pos, st.dec, rows_vocab, temps=st.temps, rep=st.rep, pres=st.pres, freq=st.freq)


def _edit(st, tables, image, mutant=None, guide=True, rules=True):
    Vv = st.vocab
    out = image
    if guide:
        out = G.ref_edit(out.reshape(-1), 0, st.stride, Vv, st.guide_slots.tolist(), st.guide_states.tolist(), tables.masks).reshape(out.shape)
    else:
        out = out.copy()
    if rules:
        for b in range(st.B):
            f = int(st.flags[b])
            if f:
                s = int(st.slots[(b + 1) % st.B]) if mutant == "flags_with_next_slot" else int(st.slots[b])
                out[b, :Vv] = R.ref_edit(out[b, :Vv], tables.rules[s], f)
    return out


def _penalise(st, cm, rows_vocab):
    """postproc.penalty_ref_step and its float64 answer rounded once to float32 (what the stages behind it read in the reference)"""
    ref = P.penalty_ref_step(cm, _pstep(st, rows_vocab), st.vocab)
    with np.errstate(invalid="ignore", over="ignore"):
        return ref, ref[1].astype(np.float32)


def ref_chain(st, state, penalty_on, mutant=None, penalised=None):
    """the chain on step `st` with the tables and the count map of `state` (which is not changed).  penalised: float32 [B, vocab], the
    image behind the penalty as a device left it -- stages 4 and 5 then read it in place of the rounded reference, so that the penalty's
    rounding is judged once (check_penalty) and not again in every token behind it.  Returns a ChainResult:
      edited      float32 [B, stride]: the image behind guide and rules
      pen         None or postproc.penalty_ref_step's tuple (count map after, float64 logits, bound, counts) on `edited`
      front       float32 [B, vocab]: what top-N and the sampler read
      behind_t    None or the temperatures stages 4 and 5 are given
      asked, top  the asking batch rows in ascending order and ref_row's tuple of each, in LIST order
      top_of_row  {batch row: its tuple}, as the generator's cursor hands the list out
      cm_before, cm the count map in front of the step and behind it
      rcase, rows the sample_rows.RCase of stage 5 and its per-row reference; tokens int32 [B], logprobs float64 [B]
    """
    assert mutant is None or mutant in STEP_MUTANTS, mutant
    tables, Vv = state.tables, st.vocab
    r = ChainResult()
    r.cm_before = state.cm.copy()
    if mutant == "penalty_before_rules" and penalty_on:
        guided = _edit(st, tables, st.logits, rules=False)
        r.pen, pen32 = _penalise(st, state.cm, guided[:, :Vv])
        r.edited = guided                                # (the image in front of the penalty)
        full = guided.copy()
        full[:, :Vv] = pen32
        r.front = _edit(st, tables, full, guide=False)[:, :Vv].copy()
    else:
        r.edited = _edit(st, tables, st.logits, mutant)
        if penalty_on:
            r.pen, pen32 = _penalise(st, state.cm, r.edited[:, :Vv])
            r.front = pen32 if penalised is None else np.ascontiguousarray(penalised, dtype=np.float32)
        else:
            r.pen, r.front = None, r.edited[:, :Vv].copy()
    r.cm = r.pen[0] if r.pen is not None else state.cm
    r.behind_t = None if penalty_on else st.temps
    # 4. top-N
    top_src, top_t = r.front, r.behind_t
    if mutant == "topn_before_penalty" and penalty_on:
        top_src = r.edited[:, :Vv]
    if mutant == "temperature_twice" and penalty_on:
        top_t = st.temps
    r.asked = [b for b in range(st.B) if st.nlp[b] > 0]
    with np.errstate(invalid="ignore"):
        r.top = [T.ref_row(P.scaled(top_src[b], None if top_t is None else top_t[b]), int(st.nlp[b])) for b in r.asked]
    if mutant == "topn_by_batch_row":
        r.top_of_row = {b: (r.top[b] if b < len(r.top) else None) for b in r.asked}
    else:
        r.top_of_row = {b: r.top[j] for j, b in enumerate(r.asked)}
    # 5. the sampler
    samp_t = st.temps if (mutant == "temperature_twice" and penalty_on) else r.behind_t
    r.rcase = S.RCase("chain", "chain", r.front, Vv, 0, st.top_k, st.top_p, samp_t, st.seeds, st.draws)
    with np.errstate(invalid="ignore"):                  # (a mutant may leave a row without a live token)
        r.rows = r.rcase.reference()
    r.tokens = np.array([row[0] for row in r.rows], dtype=np.int32)
    r.logprobs = np.array([row[1] for row in r.rows], dtype=np.float64)
    return r


def advance(state, tokens, cm=None, mutant=None):
    """the generator's bookkeeping behind a step whose rows drew `tokens`; cm: the count map the step's penalty left (ChainResult.cm)"""
    assert mutant is None or mutant in ADVANCE_MUTANTS, mutant
    tb = state.tables
    if cm is not None:
        state.cm = cm.copy()
    for b in range(state.B):
        tok = int(tokens[b])
        state.gen[b] += 1
        if mutant != "draw_not_incremented":
            state.draws[b] += 1
        if state.gen[b] >= state.min_new[b] and mutant != "stop_bit_never_cleared":
            state.flags[b] &= ~2
        g = state.guide_slots[b]
        if g >= 0 and tok not in tb.ends and mutant != "guide_state_not_advanced":
            data = tb.toks[tok] if tok < len(tb.toks) else b""
            to = G.walk(tb.trans[g], state.guide_states[b], data) if data else G.DEAD
            assert to != G.DEAD, f"row {b}: token {tok} is not allowed in state {state.guide_states[b]} of guide {g}"
            state.guide_states[b] = to
        state.prompt_ask[b] = -1
        state.start_pos[b] += len(state.seqs[b])
        state.seqs[b] = [tok]
    state.dec = state.B


# ---------------------------------------------------------------------------------------------------------------- checks
def left_out(res):
    """the sampling rows that postproc.check_sample does not compare exactly (margin under postproc.MARGIN)"""
    return [b for b, row in enumerate(res.rows) if not res.rcase.greedy(b) and row[2] < P.MARGIN]


def check_penalty(st, res, got):
    """got: float32 [B, vocab] behind the penalty.  A token that is dead in front of the penalty (-inf) must be -inf behind it, bit for
    bit; everything else goes through postproc.check_penalty_step as it is (the dead elements stand as zeros in the input, the wanted
    and the given image there, where inf - inf would be no number).  The context keeps its count map to itself: it is judged through the logits (counts_show)."""
    cm, want, bound, counts = res.pen
    Vv = st.vocab
    x = res.edited[:, :Vv]
    dead = np.isneginf(x)
    fails = []
    if not R.same_bits(got[dead], x[dead]):
        fails.append(f"{int((got[dead].view(np.uint32) != x[dead].view(np.uint32)).sum())} dead tokens did not stay -inf")
    live_x, live_got = np.where(dead, np.float32(0), x), np.where(dead, np.float32(0), got).astype(np.float32)
    pst = _pstep(st, live_x)
    want, bound = np.where(dead, 0.0, want), np.where(dead, P.DENORM, bound)
    ref = (cm, want, bound, counts)
    sc = P.PScenario("chain", "chain", Vv, Vv, cm.shape[0], None, [pst])
    img = np.full((st.B + 1, Vv), P.PEN_POISON, dtype=np.uint32)
    img[:st.B] = live_got.view(np.uint32)
    return fails + P.check_penalty_step(sc, pst, img, cm, ref)


def counts_show(st, res):
    """the rows in which a count that is off by one would move a live fed token's logit by more than the bounds at both counts together
    (postproc.check_penalty_scenario's condition, on this step)"""
    cm, want, bound, counts = res.pen
    out = []
    for b in range(st.B):
        f = abs(float(st.freq[b]))
        fed = np.unique(st.seqs[b])
        if f < P.DETECT_FREQ or fed.size == 0:
            continue
        t = float(st.temps[b]) if st.temps[b] > 0 else 1.0
        x = res.edited[b, fed]
        fed = fed[np.isfinite(x) & (np.abs(x) <= P.DETECT_X)]
        if fed.size and (f / t > 2 * bound[b, fed] + 4 * P.U * f / t).all():
            out.append(b)
    return out


def check_tokens(res, tok, lp):
    """the existing sampler checks, row by row (sample_rows.check_rows); the context hands out no canaries, so none are looked at"""
    return S.check_rows(res.rcase, res.rows, np.asarray(tok), np.asarray(lp, dtype=np.float32), np.full(1, P.TOK_CANARY, dtype=np.int32),
                        np.full(1, P.LP_CANARY, dtype=np.uint32))


def check_greedy_logprobs(res, tok, lp):
    """greedy rows: the logprob within top_logprobs.greedy_bound of the reference"""
    fails = []
    for b in range(res.rcase.B):
        if res.rcase.greedy(b) and int(tok[b]) == res.rows[b][0]:
            wtok, wlp, log_s, lse = T.ref_row(res.rcase.x(b), 1)
            bound = T.greedy_bound(res.rcase.V, log_s, lse, wlp[0])
            if not abs(float(lp[b]) - float(wlp[0])) <= bound:
                fails.append(f"row {b}: greedy logprob {float(lp[b])!r} want {float(wlp[0])!r} bound {bound:.3g}")
    return fails


def check_top(st, res, tok, lp):
    """tok / lp: [asked, NMAX] in list order: tokens exact in the first n entries, logprobs within top_logprobs.entry_bound"""
    fails = []
    if tok.shape[0] != len(res.asked):
        return [f"{tok.shape[0]} top-N rows for {len(res.asked)} asking rows"]
    for j, b in enumerate(res.asked):
        n = int(st.nlp[b])
        wtok, wlp, log_s, lse = res.top[j]
        if not (tok[j, :n] == wtok).all():
            fails.append(f"row {b} (place {j}, n {n}): tokens {tok[j, :n].tolist()} want {wtok.tolist()}")
            continue
        for e in range(n):
            g, w = float(lp[j, e]), float(wlp[e])
            if np.isneginf(w):
                if not np.isneginf(g):
                    fails.append(f"row {b} entry {e}: logprob {g!r} want -inf")
            elif not abs(g - w) <= T.entry_bound(st.vocab, log_s, lse, w):
                fails.append(f"row {b} entry {e}: logprob {g!r} want {w!r} bound {T.entry_bound(st.vocab, log_s, lse, w):.3g}")
    return fails


# ---------------------------------------------------------------------------------------------------------------- cases
def case_logits(batch, penalty_on, step):
    """the synthetic logits of a CPU case: finite, a spread the samplers' candidates carry mass in"""
    rng = np.random.default_rng(20261020 + 100 * batch + 10 * int(penalty_on) + step)
    return (rng.standard_normal((len(PATTERNS[batch]), V)) * 3).astype(np.float32)


def case_prompts(batch):
    """two decode rows (their prompts went in before the case's first step) and six prefill rows of at most 12 tokens"""
    rng = np.random.RandomState(50 + batch)
    lens = [7, 4, 12, 1, 5, 9, 3, 12] if batch == 0 else [5, 9, 2, 12, 6, 1, 11, 4]
    return [rng.randint(3, V, size=n) for n in lens]


def start_state(tables, batch, asking=None):
    """the state in front of the mixed step: rows 0 and 1 decode (one fed token each, their prompts behind them), rows 2 .. 7 prefill"""
    st = ChainState(tables, batch, asking)
    pr = case_prompts(batch)
    rng = np.random.RandomState(70 + batch)
    seqs = [[int(rng.randint(3, V))], [int(rng.randint(3, V))]] + [p.tolist() for p in pr[2:]]
    st.feed(seqs, [len(pr[0]), len(pr[1])] + [0] * 6, 2, prompt_ask=[-1, -1] + [(0, -1, 2, -1, 20, 0)[i] for i in range(6)])
    for b in (0, 1):                                     # the step that prefilled the decode rows counted their prompts
        st.cm[st.slots[b]] = np.bincount(pr[b], minlength=V).astype(np.uint16)
    return st


def run_case(tables, batch, penalty_on, asking=None, step_mutant=None, advance_mutant=None):
    """STEPS steps of synthetic logits through ref_chain and advance: the list of (the state in front of the step, ChainStep, ChainResult)"""
    state = start_state(tables, batch, asking)
    out = []
    for s in range(STEPS):
        st = state.step(case_logits(batch, penalty_on, s))
        res = ref_chain(st, state, penalty_on, step_mutant)
        out.append((state.copy(), st, res))
        advance(state, res.tokens, res.cm, advance_mutant)
    return out
