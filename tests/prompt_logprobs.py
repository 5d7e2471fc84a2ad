"""Prompt logprobs (csrc/k_prompt_logprobs.hip; DESIGN.md "numerics", prompt logprobs row): the reference, the checker and the case builders,
shared by tests/test_prompt_logprobs_spec.py (no GPU) and the tests/test_gpu_prompt_logprobs*.py files.

Specification.  A step packs B requests, request b owning token rows s .. e-1 (s = seq[b], e = seq[b + 1]).  With ask[b] >= 0 it yields the
positions r = s .. e-2, in ascending row: row r's raw fp32 logits x scored against t = tokens[r + 1],

    logprob = x[t] - lse,  lse = mx + log(sum exp(x - mx));      rank = #{v : x[v] > x[t]} + #{v < t : x[v] == x[t]}

(float comparison: -0 equals +0; rank 0 is the greedy token).  The request's last row is no position; a request of one row yields none.
ask[b] = n >= 1 adds the first n entries of the row's ranking, tests/top_logprobs.py's ref_row at temperature 1 (entries behind the
vocabulary: token -1, logprob -inf).  The reference does everything in float64 on the float32 logits; rows, ranks and top tokens are
compared exactly, logprobs within tests/top_logprobs.py's entry_bound -- it applies unchanged because the kernel's two sweeps are
top_logprobs_row's: the same 256-thread block, the same order of the mass.  Where the target is among the position's own top entries the
two logprobs must be equal bit for bit (they are one expression of the same lse).

Guards of an operator case (tests/top_logprobs.py's): rows `stride` > V apart, +inf behind the vocabulary and in front of a misaligned base;
every output filled with canaries: TAIL_ROWS rows behind the last position, the top slots behind a position's n, and every top slot of an
n = 0 position must come back untouched.
"""
import numpy as np

from tests import postproc as P
from tests import top_logprobs as T

NMAX = T.NMAX
TAIL_ROWS = T.TAIL_ROWS
RANK_CANARY = 0x5A5A5A5A


def positions(seq, ask):
    """the listing: (rows [P] int32, n_top [P] int32), ascending"""
    rows, ntop = [], []
    for b in range(len(ask)):
        if ask[b] < 0:
            continue
        for r in range(int(seq[b]), int(seq[b + 1]) - 1):
            rows.append(r)
            ntop.append(int(ask[b]))
    return np.array(rows, dtype=np.int32), np.array(ntop, dtype=np.int32)


def clamp_ask(n):
    """Request::prompt_logprobs as the generator admits it: above 20 is 20, below -1 is -1"""
    return max(-1, min(int(n), NMAX))


def ref_position(x, target, n):
    """x: the row's raw logits (float32) -> (logprob float64, rank, top tokens [n], top logprobs [n] float64, ln S, lse)"""
    x = np.asarray(x, dtype=np.float32)
    xt = x[target]
    rank = int((x > xt).sum() + (x[:target] == xt).sum())
    tok, lp, log_s, lse = T.ref_row(x, n)
    with np.errstate(invalid="ignore"):
        logprob = float(np.float64(xt) - lse)
    return logprob, rank, tok, lp, log_s, lse


class PCase:
    """one step's ask: tokens [T] int64, seq [B + 1], ask [B]; `logits` maps every asked row r to its float32 logits [V].  As an operator
    case the listed rows are the launch's logits rows, `stride` apart, the base `off` floats past a 16-byte boundary."""

    def __init__(self, name, family, V, tokens, seq, ask, logits, stride, off, chunk=8):
        self.name, self.family, self.V = name, family, V
        self.tokens = np.ascontiguousarray(tokens, dtype=np.int64)
        self.seq = np.ascontiguousarray(seq, dtype=np.int64)
        self.ask = np.ascontiguousarray(ask, dtype=np.int32)
        self.rows, self.ntop = positions(self.seq, self.ask)
        self.P = len(self.rows)
        self.logits = logits
        self.stride, self.off, self.chunk = stride, off, chunk
        self._ref = None

    def uses_vector_path(self):
        return self.stride % 4 == 0 and self.off == 0

    def image(self):
        img = np.full(4 + (self.P + 1) * self.stride + 4, np.inf, dtype=np.float32)
        for j, r in enumerate(self.rows):
            img[self.off + j * self.stride:self.off + j * self.stride + self.V] = self.logits[int(r)]
        return img

    def targets(self):
        return self.tokens[self.rows + 1]

    def reference(self):
        """per position: ref_position's tuple; computed once"""
        if self._ref is None:
            self._ref = [ref_position(self.logits[int(r)], int(self.tokens[r + 1]), int(n)) for r, n in zip(self.rows, self.ntop)]
        return self._ref

    def check_assertions(self):
        assert 0 <= self.off <= 3 and self.stride > self.V >= 1 and self.seq[0] == 0 and self.seq[-1] == len(self.tokens)
        assert ((self.ask >= -1) & (self.ask <= NMAX)).all() and ((self.tokens >= 0) & (self.tokens < self.V)).all(), self.name
        assert sorted(self.logits) == sorted(set(int(r) for r in self.rows)), (self.name, "a logits row per asked row")
        for x in self.logits.values():
            assert x.dtype == np.float32 and x.shape == (self.V,) and not np.isnan(x).any() and not np.isposinf(x).any() and x.max() > -np.inf
        return self.reference()


def blank_outputs(Pn):
    """the four outputs as a launch receives them: logprob bits [P + TAIL], rank [P + TAIL], top tokens / top logprob bits [P + TAIL, NMAX]"""
    n = Pn + TAIL_ROWS
    return {"lp": np.full(n, P.LP_CANARY, dtype=np.uint32), "rank": np.full(n, RANK_CANARY, dtype=np.int32),
            "top_tok": np.full((n, NMAX), P.TOK_CANARY, dtype=np.int32), "top_lp": np.full((n, NMAX), P.LP_CANARY, dtype=np.uint32)}


def as_outputs(c, ref=None, rows=None):
    """the reference (or a mutated one: a list of ref_position tuples, for the listing `rows`) as the arrays a launch would have left"""
    ref = c.reference() if ref is None else ref
    out = blank_outputs(len(ref))
    out["rows"] = c.rows.copy() if rows is None else np.asarray(rows, dtype=np.int32)
    for j, (lp, rank, tok, tlp, _, _) in enumerate(ref):
        out["lp"][j] = np.float32(lp).view(np.uint32)
        out["rank"][j] = rank
        n = len(tok)
        out["top_tok"][j, :n] = tok
        out["top_lp"][j, :n] = np.asarray(tlp, dtype=np.float32).view(np.uint32)
        hit = np.flatnonzero(tok == c.tokens[out["rows"][j] + 1]) if out["rows"][j] + 1 < len(c.tokens) else []
        if len(hit):                                     # one expression on the device: the same float32
            out["lp"][j] = out["top_lp"][j, hit[0]]
    return out


def check(c, got, canaries=True):
    """got: {"rows" [P'], "lp" bits, "rank", "top_tok", "top_lp" bits}, the last four with TAIL_ROWS canary rows when `canaries` (an operator
    launch; the product's pinned block has none, and leaves the top slots of an n = 0 position unspecified)
    -> (failures, largest |logprob error| / bound over all positions and entries)"""
    fails, frac = [], 0.0
    ref = c.reference()
    if len(got["rows"]) != c.P or (np.asarray(got["rows"]) != c.rows).any():
        return [f"positions {list(got['rows'][:8])}.. ({len(got['rows'])}), want {list(c.rows[:8])}.. ({c.P})"], 0.0
    tail = TAIL_ROWS if canaries else 0
    for k in ("lp", "rank", "top_tok", "top_lp"):
        if len(got[k]) != c.P + tail:
            return [f"output {k} has {len(got[k])} rows"], 0.0
    if canaries:
        if not ((got["lp"][c.P:] == P.LP_CANARY).all() and (got["rank"][c.P:] == RANK_CANARY).all() and
                (got["top_tok"][c.P:] == P.TOK_CANARY).all() and (got["top_lp"][c.P:] == P.LP_CANARY).all()):
            fails.append("rows behind the last position were written")
    lpf, tlpf = got["lp"].view(np.float32), got["top_lp"].view(np.float32)
    for j in range(c.P):
        r, n, t = int(c.rows[j]), int(c.ntop[j]), int(c.tokens[c.rows[j] + 1])
        wlp, wrank, wtok, wtlp, log_s, lse = ref[j]
        if canaries and not ((got["top_tok"][j, n:] == P.TOK_CANARY).all() and (got["top_lp"][j, n:] == P.LP_CANARY).all()):
            fails.append(f"row {r} (n {n}): top slots behind n were written")
        if int(got["rank"][j]) != wrank:
            fails.append(f"row {r} target {t}: rank {int(got['rank'][j])} want {wrank}")
        pairs = [("logprob", float(lpf[j]), wlp)]
        bad = np.flatnonzero(got["top_tok"][j, :n] != wtok)
        if bad.size:
            e = int(bad[0])
            fails.append(f"row {r} (n {n}): entry {e} token {int(got['top_tok'][j, e])} want {int(wtok[e])} ({bad.size} entries differ)")
        else:
            pairs += [(f"entry {e}", float(tlpf[j, e]), float(wtlp[e])) for e in range(n)]
            hit = np.flatnonzero(wtok == t)
            if hit.size and got["lp"][j] != got["top_lp"][j, hit[0]]:
                fails.append(f"row {r} target {t}: logprob bits {int(got['lp'][j]):#x} differ from its own entry {int(hit[0])} {int(got['top_lp'][j, hit[0]]):#x}")
        for what, g, w in pairs:
            if np.isneginf(w):
                if not np.isneginf(g):
                    fails.append(f"row {r}: {what} {g!r} want -inf")
                continue
            bound = T.entry_bound(c.V, log_s, lse, w)
            err = abs(g - w)
            if not err <= bound:
                fails.append(f"row {r}: {what} {g!r} want {w!r}: off by {err:.3g}, bound {bound:.3g}")
            else:
                frac = max(frac, err / bound)
    return fails, frac


def launch(m, torch, c):
    """the case through pplhip_op_prompt_logprobs: (rc, outputs as blank_outputs plus "rows")"""
    d = torch.from_numpy(c.image()).cuda()
    assert d.data_ptr() % 16 == 0
    out = blank_outputs(c.P)
    dev = {k: torch.from_numpy(v.view(np.int32)).cuda() for k, v in out.items()}
    d_rows, d_ntop, d_tok = torch.from_numpy(c.rows).cuda(), torch.from_numpy(c.ntop).cuda(), torch.from_numpy(c.tokens).cuda()
    torch.cuda.synchronize()
    rc = m.lib().pplhip_op_prompt_logprobs(None, d.data_ptr() + 4 * c.off, c.stride, c.V, d_rows.data_ptr(), c.P, d_tok.data_ptr(), len(c.tokens),
                                           d_ntop.data_ptr(), dev["lp"].data_ptr(), dev["rank"].data_ptr(), dev["top_tok"].data_ptr(),
                                           dev["top_lp"].data_ptr())
    torch.cuda.synchronize()
    got = {k: dev[k].cpu().numpy().view(out[k].dtype) for k in out}
    got["rows"] = c.rows.copy()
    return rc, got


# ---- mutated references (tests/test_prompt_logprobs_spec.py: the checker must reject each in every family it is built for) ---------------
def _row_logits(c, r):
    """a mutant may score a row nobody asked for: it sees the nearest asked row's logits (only the listing is wrong then)"""
    return c.logits[r] if r in c.logits else c.logits[min(c.logits, key=lambda q: abs(q - r))]


def _mut_target_from_row(c):
    return [ref_position(c.logits[int(r)], int(c.tokens[r]), int(n)) for r, n in zip(c.rows, c.ntop)], c.rows


def _mut_listing(c, last_of_every_request):
    rows, ref = [], []
    T_ = len(c.tokens)
    for b in range(len(c.ask)):
        if c.ask[b] < 0:
            continue
        s, e = int(c.seq[b]), int(c.seq[b + 1])
        end = e if (last_of_every_request or e < T_) else e - 1      # the last row too (scored against whatever token follows it)
        for r in range(s, end):
            rows.append(r)
            ref.append(ref_position(_row_logits(c, r), int(c.tokens[min(r + 1, T_ - 1)]), int(c.ask[b])))
    return ref, rows


def _mut_next_request(c):
    """a request's last row scored against the NEXT request's first token (where there is a next request)"""
    return _mut_listing(c, False)


def _mut_last_included(c):
    """L positions for a prompt of L tokens"""
    return _mut_listing(c, True)


def _mut_rank(c, f):
    out = []
    for (lp, rank, tok, tlp, log_s, lse), r in zip(c.reference(), c.rows):
        x, t = c.logits[int(r)], int(c.tokens[r + 1])
        out.append((lp, f(x, t), tok, tlp, log_s, lse))
    return out, c.rows


def _mut_rank_ge(c):
    return _mut_rank(c, lambda x, t: int((x >= x[t]).sum()))


def _mut_rank_ties_high(c):
    return _mut_rank(c, lambda x, t: int((x > x[t]).sum() + (x[t + 1:] == x[t]).sum()))


def _mut_no_shift(c):
    """lse = logf(sum expf(x)) in float32, without the maximum shift: overflows for x > 88.7"""
    out = []
    for (lp, rank, tok, tlp, log_s, lse), r in zip(c.reference(), c.rows):
        x, t = c.logits[int(r)], int(c.tokens[r + 1])
        with np.errstate(over="ignore", invalid="ignore"):
            bad = np.log(np.exp(x).astype(np.float32).sum(dtype=np.float32))
            out.append((float(x[t] - bad), rank, tok, (x[np.maximum(tok, 0)] - bad).astype(np.float64), log_s, lse))
    return out, c.rows


MUTANTS = {   # name: (mutated reference -> (per-position tuples, listing), the families it must be caught in)
    "target-from-row": (_mut_target_from_row, ("gaps", "ties", "masked", "flat", "needle")),
    "last-row-against-next-request": (_mut_next_request, ("gaps", "ties", "masked", "flat", "needle")),
    "last-position-included": (_mut_last_included, ("gaps", "ties", "masked", "flat", "needle", "last-request")),
    "rank-counts-ge": (_mut_rank_ge, ("gaps", "ties", "flat", "needle")),
    "rank-ties-to-higher-index": (_mut_rank_ties_high, ("ties", "flat")),
    "logprob-without-max-shift": (_mut_no_shift, ("needle",)),
}


CHUNK_MUTANT = "chunk-last-row-dropped"
ALL_MUTANTS = sorted(MUTANTS) + [CHUNK_MUTANT]


def mutant_families(name):
    return CHUNK_MUTANT_FAMILIES if name == CHUNK_MUTANT else MUTANTS[name][1]


def mutant_outputs(c, name):
    if name == CHUNK_MUTANT:                             # the last position of every chunk of c.chunk positions is never written
        out = as_outputs(c)
        for j in list(range(c.chunk - 1, c.P, c.chunk)) + [c.P - 1]:
            out["lp"][j], out["rank"][j] = P.LP_CANARY, RANK_CANARY
            out["top_tok"][j], out["top_lp"][j] = P.TOK_CANARY, P.LP_CANARY
        return out
    ref, rows = MUTANTS[name][0](c)
    return as_outputs(c, ref, rows)


CHUNK_MUTANT_FAMILIES = ("gaps", "ties", "masked", "flat", "needle")


# ---- case builders ---------------------------------------------------------------------------------------------------------------------
GRID_V = [1, 2, 3, 255, 256, 257, 1023, 1025, 4097, 32000, 32001, 128256]
GRID_R = [1, 2, 64]                                      # positions of a case
FAMILIES = T.FAMILIES
ASKS = [0, 1, 20, 5]
# requests (length, asks) by the number of positions they add up to; an asking request of one token and a request that does not ask in each
SHAPES = {1: ((1, True), (2, True), (3, False)), 2: ((3, True), (1, True), (2, False)),
          64: ((1, True), (20, True), (5, False), (40, True), (7, True))}
TARGET_KINDS = ("token0", "last", "tie", "masked", "top")


def _target(rng, x, kind, n):
    """an index of the row by kind; the row may be edited so that the kind exists"""
    V = x.size
    order = np.argsort(-x, kind="stable")
    if kind == "token0":
        return 0
    if kind == "last":
        return V - 1
    if kind == "tie":                                    # inside a block of equal values where the row has one (the middle of the block)
        vals, first, counts = np.unique(x, return_index=True, return_counts=True)
        if counts.max() > 1:
            v = vals[np.argmax(counts)]
            idx = np.flatnonzero(x == v)
            return int(idx[len(idx) // 2])
        return int(order[min(1, V - 1)])
    if kind == "masked":                                 # a -inf logit (planted where the row has none and can spare an entry)
        inf = np.flatnonzero(np.isneginf(x))
        if inf.size:
            return int(inf[inf.size // 2])
        if V >= 4:
            i = int(order[-1])
            x[i] = -np.inf
            return i
        return int(order[-1])
    return int(order[min(int(rng.randint(0, max(n, 1) + 1)), V - 1)])   # among the first n + 1 of the ranking: mostly inside the top-n


def _case(name, family, V, R, stride, off, k, shape=None):
    rng = np.random.RandomState(7000 + V % 9973 + 41 * k)
    shape = SHAPES[R] if shape is None else shape
    lens = [L for L, _ in shape]
    seq = np.concatenate([[0], np.cumsum(lens)])
    ask, a = [], k
    for L, asks in shape:
        ask.append(ASKS[a % len(ASKS)] if asks else -1)
        a += asks
    tokens = rng.randint(0, V, size=int(seq[-1])).astype(np.int64)
    logits, j = {}, 0
    for b, (L, asks) in enumerate(shape):
        for r in range(int(seq[b]), int(seq[b + 1]) - 1):
            if not asks:
                continue
            n = ask[b] if ask[b] > 0 else T.NS[(j + k) % len(T.NS)]
            x = T.ROW[family if family in T.ROW else "gaps"](rng, V, n, j + k)
            t = _target(rng, x, TARGET_KINDS[(j + k) % len(TARGET_KINDS)], ask[b])
            tokens[r + 1] = t
            if r == int(seq[b]) and V > 1:               # the row's own token differs from its target
                tokens[r] = (t + 1 + int(rng.randint(0, V - 1))) % V
            logits[r] = x
            j += 1
        if b + 1 < len(shape) and V > 1 and L >= 2:      # the next request's first token differs from this one's last
            tokens[int(seq[b + 1])] = (tokens[int(seq[b + 1]) - 1] + 1 + int(rng.randint(0, V - 1))) % V
    return PCase(name, family, V, tokens, seq, ask, logits, stride, off)


def grid_cases():
    """every V x every family; the positions, the stride, the base offset, the asks and the target kinds walk through their lists"""
    out, k = [], 0
    for V in GRID_V:
        for family in FAMILIES:
            R = GRID_R[k % 3] if V < 100000 else GRID_R[k % 2]
            stride, off = (4 * (V // 4) + 4, 0) if k % 2 == 0 else (V + (1, 2, 3, 7)[(k // 2) % 4], (k // 2) % 4)
            name = f"{family}-V{V}-R{R}-s{stride}-o{off}"
            out.append(P.Lazy(name, family, lambda name=name, family=family, V=V, R=R, stride=stride, off=off, k=k:
                              _case(name, family, V, R, stride, off, k)))
            k += 1
    return out


def last_request_cases():
    """the only asking request is the step's last one: nothing follows its last row"""
    out = []
    for k, V in enumerate((3, 257, 4097)):
        name = f"last-request-V{V}"
        out.append(P.Lazy(name, "last-request", lambda name=name, V=V, k=k:
                          _case(name, "last-request", V, 0, V + 5, k % 4, k, shape=((2, False), (1, False), (4 + k, True)))))
    return out


def all_cases():
    return grid_cases() + last_request_cases()
