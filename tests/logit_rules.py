"""Logit rules (DESIGN.md "numerics", logit rules row): the reference the device is held against, bit for bit.

A request's rule is: bias pairs (token, value; -inf bans), an optional set of allowed tokens held as a bit mask (token v is bit v & 31 of
word v >> 5, bits at or behind V mean nothing) and the stop tokens that min_new_tokens suppresses.  A row is edited with a flag word:
bit 0 applies mask and bias, bit 1 suppresses the stops, 0 leaves the row alone.  With x the logit as the model wrote it:

    y = -inf              if bit 0 and the rule has a mask and v's bit is clear
      = -inf              else if bit 1 and v is in stops
      = fp32(x + bias)    else if bit 0 and v has a bias
      = x, bit for bit    otherwise

The arithmetic is one float32 addition or a store, so there is no tolerance anywhere: `image()` is the memory a launch receives (rows
`stride` apart behind a base `off` floats past a 16-byte boundary, +inf poison everywhere else, a canary row behind the batch),
`want_image()` what it must leave, and they are compared as uint32 over every element.  The rule table a case hands the kernel has a
HOSTILE record (mask all clear, 512 biases, 64 stops) in every slot that no asking row names, the slots of the rows with flags 0 included:
applying a rule to the wrong row, or through the row index instead of the slot, shows.

`validate` is the admission check of the host stack and of pplhip_logit_rule_set; `merge` what they then hand the device.
"""
import itertools

import numpy as np

BIAS_MAX = 512   # PPLHIP_LOGIT_BIAS_MAX
STOP_MAX = 64    # PPLHIP_LOGIT_STOP_MAX
NINF = np.float32(-np.inf)


def words(V):
    return (V + 31) // 32


def pack_mask(allowed, V, tail_bits=0):
    """allowed: iterable of tokens in [0, V) -> uint32 [ceil(V / 32)]; tail_bits: what the bits at or behind V are set to (they mean nothing)"""
    m = np.zeros(words(V), dtype=np.uint32)
    for v in allowed:
        assert 0 <= v < V
        m[v >> 5] |= np.uint32(1) << np.uint32(v & 31)
    if V & 31:
        tail = np.uint32((0xFFFFFFFF << (V & 31)) & 0xFFFFFFFF)
        m[-1] |= np.uint32(tail_bits) & tail
    return m


class Rule:
    """bias: [(token, value)] with unique tokens; mask: None or uint32 [words(V)]; stops: [token]"""

    def __init__(self, bias=(), mask=None, stops=()):
        self.bias = [(int(t), np.float32(v)) for t, v in bias]
        self.mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint32)
        self.stops = [int(t) for t in stops]
        assert len(self.bias) <= BIAS_MAX and len(self.stops) <= STOP_MAX

    def allowed(self, v):
        return self.mask is None or bool((int(self.mask[v >> 5]) >> (v & 31)) & 1)


def ref_edit(x, rule, flags):
    """x: float32 [V] as the model wrote it -> the edited row (a copy)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    V = x.size
    y = x.copy()
    if flags == 0:
        return y
    dead = np.zeros(V, dtype=bool)
    if (flags & 1) and rule.mask is not None:
        bits = np.unpackbits(rule.mask.view(np.uint8), bitorder="little")[:V].astype(bool)
        dead |= ~bits
    if flags & 2:
        for t in rule.stops:
            dead[t] = True
    if flags & 1:
        with np.errstate(invalid="ignore"):
            for t, b in rule.bias:
                y[t] = np.float32(x[t] + b)      # one float32 addition
    y[dead] = NINF
    return y


# ---------------------------------------------------------------------------------------------------------------- validation

def validate(V, logit_bias=(), allowed=None, banned=(), stops=(), min_new_tokens=0):
    """the admission check: None when the rule is accepted, else the name of the field at fault.  logit_bias: pairs (token, value);
    allowed: None or tokens; banned: tokens; stops: the request's effective stop tokens (suppressed while min_new_tokens > 0)."""
    finite = set()
    bans = set()
    for t, v in logit_bias:
        if not 0 <= t < V:
            return "logit_bias"
        v = float(v)
        if v != v or v == np.inf:
            return "logit_bias"
        if v == -np.inf:
            bans.add(t)
            continue
        if t in finite:
            return "logit_bias"
        finite.add(t)
    for t in banned:
        if not 0 <= t < V:
            return "banned_tokens"
        bans.add(t)
    if allowed is not None:
        for t in allowed:
            if not 0 <= t < V:
                return "allowed_tokens"
    if len(bans | finite) > BIAS_MAX:
        return "logit_bias"
    sup = set()
    if min_new_tokens > 0:
        for t in stops:
            if not 0 <= t < V:
                return "stop_tokens"
            sup.add(t)
        if len(sup) > STOP_MAX:
            return "stop_tokens"
    live = (set(range(V)) if allowed is None else set(allowed)) - bans - sup
    if not live:
        return "allowed_tokens" if allowed is not None else ("banned_tokens" if bans else "min_new_tokens")
    return None


def merge(V, logit_bias=(), allowed=None, banned=(), stops=(), min_new_tokens=0):
    """an accepted request -> the Rule the device gets: the ban wins over a bias, the stops travel only when they will be suppressed"""
    assert validate(V, logit_bias, allowed, banned, stops, min_new_tokens) is None
    bans = set(banned) | {t for t, v in logit_bias if float(v) == -np.inf}
    bias = [(t, v) for t, v in logit_bias if t not in bans] + [(t, -np.inf) for t in sorted(bans)]
    return Rule(bias, None if allowed is None else pack_mask(allowed, V), sorted(set(stops)) if min_new_tokens > 0 else ())


# ---------------------------------------------------------------------------------------------------------------- cases

class ECase:
    """one launch of pplhip_op_logit_edit: B rows of V logits `stride` apart, the base `off` floats past a 16-byte boundary; slots [B]
    (distinct, in [0, S)), flags [B], rules {slot: Rule} for the rows that ask"""

    def __init__(self, name, logits, stride, off, slots, flags, rules, S, given_rows=False):
        self.name = name
        self.logits = np.ascontiguousarray(logits, dtype=np.float32)
        self.B, self.V = self.logits.shape
        self.stride, self.off, self.S = stride, off, S
        self.slots = np.ascontiguousarray(slots, dtype=np.int32)
        self.flags = np.ascontiguousarray(flags, dtype=np.uint32)
        self.rules = rules
        self.given_rows = given_rows     # hand the kernel a device row list instead of letting the operator make it
        self.asking = [b for b in range(self.B) if self.flags[b]]
        assert 0 <= off <= 3 and stride >= self.V >= 1 and len(set(self.slots.tolist())) == self.B
        assert all(0 <= s < S for s in self.slots) and all(int(self.slots[b]) in rules for b in self.asking)
        assert not np.isnan(self.logits).any() and not np.isposinf(self.logits).any()

    def uses_vector_path(self):
        return self.stride % 4 == 0 and self.off == 0

    def image(self):
        img = np.full(4 + (self.B + 1) * self.stride + 4, np.inf, dtype=np.float32)
        for b in range(self.B):
            img[self.off + b * self.stride:self.off + b * self.stride + self.V] = self.logits[b]
        return img

    def table(self):
        """(head [S, 4], bias_tok [S, 512], bias_val [S, 512], stops [S, 64], mask [S, W]): hostile records wherever no asking row points"""
        S, V, W = self.S, self.V, words(self.V)
        head = np.zeros((S, 4), dtype=np.int32)
        bt = np.zeros((S, BIAS_MAX), dtype=np.int32)
        bv = np.zeros((S, BIAS_MAX), dtype=np.float32)
        st = np.zeros((S, STOP_MAX), dtype=np.int32)
        mk = np.zeros((S, W), dtype=np.uint32)
        head[:] = (BIAS_MAX, STOP_MAX, 1, 0)
        bt[:] = np.arange(BIAS_MAX) % V
        bv[:] = 1000.0
        st[:] = (np.arange(STOP_MAX) * 7) % V
        asking_slots = {int(self.slots[b]) for b in self.asking}
        for s in asking_slots:
            r = self.rules[s]
            head[s] = (len(r.bias), len(r.stops), 0 if r.mask is None else 1, 0)
            # behind the counts the record keeps hostile entries: they must not be read
            for i, (t, v) in enumerate(r.bias):
                bt[s, i], bv[s, i] = t, v
            st[s, :len(r.stops)] = r.stops
            if r.mask is not None:
                mk[s] = r.mask
            else:
                mk[s] = 0                 # has_mask = 0: an all-clear mask that must be ignored
        return head, bt, bv, st, mk

    def want_image(self):
        return edited_image(self)


def edited_image(c, mutant=None):
    """the image the launch must leave; `mutant` names one deliberate mistake (MUTANTS) for the spec test"""
    img = c.image()
    head, bt, bv, st, mk = c.table()
    V = c.V
    for b in range(c.B):
        f = int(c.flags[b])
        if f == 0:
            continue
        s = b if mutant == "row_for_slot" and b < c.S else int(c.slots[b])
        n_bias, n_stop, has_mask = int(head[s, 0]), int(head[s, 1]), int(head[s, 2])
        if mutant == "drop_last_bias":
            n_bias = max(n_bias - 1, 0)
        base = c.off + b * c.stride
        x = img[base:base + V].copy()
        bit0 = bool(f & 1)
        dead = {}
        if bit0 and has_mask:
            hi = 32 * words(V) if mutant == "tail_bits" else V
            for v in range(hi):
                w = v >> 5
                if mutant == "word_off_by_one" and v and v % 32 == 0:
                    w -= 1
                if not (int(mk[s, w]) >> (v & 31)) & 1 and base + v < img.size:
                    dead[v] = True
        if (f & 2) or mutant == "stops_without_bit1":
            for t in st[s, :n_stop]:
                dead[int(t)] = True
        if bit0 or mutant == "bias_without_bit0":
            with np.errstate(invalid="ignore"):
                for i in range(n_bias):
                    t = int(bt[s, i])
                    if mutant == "bias_resurrects":
                        dead.pop(t, None)
                    if t not in dead:
                        img[base + t] = np.float32(x[t] + bv[s, i])
        for v in dead:
            img[base + v] = NINF
    return img


MUTANTS = ("tail_bits", "bias_resurrects", "stops_without_bit1", "bias_without_bit0", "row_for_slot", "drop_last_bias", "word_off_by_one")


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def diff(c, got):
    """got: the image as it came back -> list of messages (empty: bit for bit the wanted image)"""
    want = c.want_image()
    if got.shape != want.shape:
        return [f"image of {got.shape}"]
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    out = []
    for i in bad[:6]:
        j = int(i) - c.off
        b, v = (j // c.stride, j % c.stride) if j >= 0 else (-1, j)
        where = f"row {b} token {v}" if 0 <= b < c.B and v < c.V else f"element {int(i)} outside every row (row {b}, column {v})"
        out.append(f"{where}: got {got[i]!r} want {want[i]!r}" + (f" (flags {int(c.flags[b])})" if 0 <= b < c.B else ""))
    if bad.size > 6:
        out.append(f"{bad.size} elements differ")
    return out


GRID_V = [1, 2, 31, 32, 33, 63, 64, 65, 127, 1000, 4099]
N_BIAS = [0, 1, 2, 511, 512]
KINDS = ("mask", "bias", "stops", "all")


def strides(V):
    return [V, V + 1, V + 3, (V + 3) // 4 * 4 + 4]


def _logits(rng, B, V):
    x = (rng.standard_normal((B, V)) * 4).astype(np.float32)
    x[rng.random((B, V)) < 0.02] = NINF          # a logit may be -inf already
    x[rng.random((B, V)) < 0.02] = np.float32(-0.0)
    return x


def _rule(rng, V, kind, n_bias, n_allowed):
    """a rule of the kind with n_bias entries (capped by V) and n_allowed allowed tokens; tail bits of the mask random"""
    mask = None
    if kind in ("mask", "all"):
        allowed = rng.choice(V, size=min(max(n_allowed, 1), V), replace=False)
        mask = pack_mask(allowed.tolist(), V, tail_bits=int(rng.integers(0, 1 << 32)))
    bias = []
    if kind in ("bias", "all"):
        toks = rng.choice(V, size=min(n_bias, V), replace=False)
        for t in toks:
            r = rng.random()
            v = -np.inf if r < 0.15 else (0.0 if r < 0.2 else float(np.float32(rng.uniform(-8, 8))))
            bias.append((int(t), v))
    stops = []
    if kind in ("stops", "all"):
        stops = rng.choice(V, size=min(int(rng.integers(1, 5)), V), replace=False).tolist()
    return Rule(bias, mask, stops)


def _perm_slots(rng, B, S):
    """distinct slots, never the identity on the rows"""
    while True:
        s = rng.permutation(S)[:B]
        if B == 1 and S > 1:
            if s[0] != 0:
                return s
        elif (s != np.arange(B)).any():
            return s


def grid_cases():
    out = []
    k = 0
    for V in GRID_V:
        for si, (stride, off) in enumerate(zip(strides(V) + [strides(V)[3]], [0, 1, 2, 0, 3])):
            rng = np.random.default_rng(1000 * V + si)
            B = [4, 5, 6, 6, 3][si] if V > 2 else [4, 2, 6, 5, 1][si]
            S = B + 2
            slots = _perm_slots(rng, B, S)
            flags = [(k + b) % 4 for b in range(B)]        # 0, 1, 2, 3 side by side
            if B < 4:
                flags[-1] = 3
            rules = {}
            for b in range(B):
                kind = KINDS[(k + b + si) % 4]
                n_bias = N_BIAS[(k + b) % 5] if kind != "all" or b % 2 else N_BIAS[(k + 3 + b) % 5]
                n_allowed = [1, V - 1, V, max(V // 2, 1)][(k + b) % 4]
                rules[int(slots[b])] = _rule(rng, V, kind, n_bias, n_allowed)
            out.append(ECase(f"V{V}-s{stride}-o{off}-B{B}", _logits(rng, B, V), stride, off, slots, flags, rules, S, given_rows=(k % 3 == 0)))
            k += 1
    # V = 32000, all four flag words, every kind, 512 biases
    rng = np.random.default_rng(32000)
    B, V = 6, 32000
    slots = _perm_slots(rng, B, 8)
    rules = {int(slots[b]): _rule(rng, V, KINDS[b % 4] if b < 4 else "all", [512, 511, 2, 512, 1, 512][b], [1000, V - 1, V, 1, 5, 16000][b])
             for b in range(B)}
    out.append(ECase("V32000-B6", _logits(rng, B, V), V, 0, slots, [3, 1, 2, 3, 0, 1], rules, 8))
    out.append(ECase("V32000-B6-unaligned", _logits(rng, B, V), V + 3, 1, slots, [1, 3, 0, 2, 3, 3], rules, 8, given_rows=True))
    return out


def hazard_cases():
    """in one 16-byte piece (tokens 4 .. 7) and across a mask word boundary (tokens 30 .. 33), every permutation of: a masked token, a
    biased and allowed one, a biased and masked one, a stop (allowed, suppressed by bit 1); on and off the 16-byte path"""
    out = []
    perms = list(itertools.permutations(range(4)))
    V = 67
    for base in (4, 30):
        for stride, off in ((68, 0), (67, 1)):
            for g in range(4):
                rng = np.random.default_rng(base * 100 + g * 10 + off)
                B, S = 6, 9
                slots = _perm_slots(rng, B, S)
                rules = {}
                for b in range(B):
                    p = perms[g * 6 + b]
                    masked, biased, biased_masked, stop = (base + p[i] for i in range(4))
                    allowed = [v for v in range(V) if v not in (masked, biased_masked) and (v < base - 2 or v >= base + 4 or v in (biased, stop))]
                    # (the two tokens in front of the piece are masked as well, so the neighbouring piece is mixed too)
                    rules[int(slots[b])] = Rule([(biased, 1.5), (biased_masked, 2.5)], pack_mask(allowed, V, tail_bits=0xFFFFFFFF), [stop])
                x = rng.standard_normal((B, V)).astype(np.float32)   # finite everywhere: a resurrected token would show
                out.append(ECase(f"hazard-t{base}-o{off}-g{g}", x, stride, off, slots, [3] * B, rules, S, given_rows=(g % 2 == 1)))
    return out


def big_case():
    """B = 64, V = 32000, every row asking"""
    rng = np.random.default_rng(64)
    B, V, S = 64, 32000, 66
    slots = _perm_slots(rng, B, S)
    rules = {int(slots[b]): _rule(rng, V, KINDS[b % 4], N_BIAS[b % 5], [1000, V - 1, V, 1][b % 4]) for b in range(B)}
    return ECase("V32000-B64-all-asking", _logits(rng, B, V), V, 0, slots, [1 + b % 3 for b in range(B)], rules, S)


def all_cases():
    return grid_cases() + hazard_cases() + [big_case()]


def launch(m, torch, c):
    """the case through pplhip_op_logit_edit: (rc, the image as it came back)"""
    d = torch.from_numpy(c.image()).cuda()
    assert d.data_ptr() % 16 == 0
    parts = [torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda() for a in c.table()]
    d_flags = torch.from_numpy(c.flags.view(np.int32)).cuda()
    d_slots = torch.from_numpy(c.slots).cuda()
    d_rows = torch.from_numpy(np.asarray(c.asking + [0], dtype=np.int32)).cuda() if c.given_rows else None
    torch.cuda.synchronize()
    rc = m.lib().pplhip_op_logit_edit(None, d.data_ptr() + 4 * c.off, c.stride, c.V, c.B, d_flags.data_ptr(), d_slots.data_ptr(),
                                      *[p.data_ptr() for p in parts], None if d_rows is None else d_rows.data_ptr(),
                                      len(c.asking) if c.given_rows else 0)
    torch.cuda.synchronize()
    return rc, d.cpu().numpy()
