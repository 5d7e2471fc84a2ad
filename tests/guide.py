"""Numpy reference of guided decoding's two kernels (csrc/k_guide.hip; DESIGN.md "numerics", guided decoding row), the cases of the
operator test and the named mutants that tests/test_guide_spec.py tells apart on those cases.

A guide is a byte-level DFA: trans uint8 [S, 256] (255 = the dead state, which has no row), accept uint8 [S].  The vocabulary is a list of
bytes objects, one per token id < n_tok; ids at or behind n_tok are empty.

  build   mask[s] bit t = accept[s]                                        if t is an end token
                        = 0                                                if token t is empty
                        = walking its bytes from s never meets the dead state   otherwise
          token t is bit t & 31 of word t >> 5; bits at or behind `vocab` are 0; any[s] = 1 iff row s has a bit set
  edit    logits[b, v] = -inf for v < vocab whose bit is clear in row states[b] of slot guide_slots[b]; guide_slots[b] = -1: untouched
"""
import numpy as np

DEAD = 255
MAX_STATES = 255
MAX_SLOTS = 16
NINF = np.float32(-np.inf)

MUTANTS = ("skip_last_byte", "swap_ballot_words", "end_in_non_accepting", "allow_empty", "state_stride", "tail_bits", "dead_is_row_255")


def words(V):
    return (V + 31) // 32


def walk(trans, state, data):
    """the state after `data` from `state`, DEAD as soon as the dead state is met (GuideDfa::Step)"""
    for b in data:
        if state == DEAD:
            return DEAD
        state = int(trans[state, b])
    return state


def brute_build(trans, accept, toks, ends, vocab):
    """the definition, token by token and state by state: bool [S, vocab]"""
    S = len(trans)
    out = np.zeros((S, vocab), dtype=bool)
    for s in range(S):
        for t in range(vocab):
            if t in ends:
                out[s, t] = bool(accept[s])
            elif t < len(toks) and len(toks[t]) > 0:
                out[s, t] = walk(trans, s, toks[t]) != DEAD
    return out


def ref_allowed(trans, accept, toks, ends, vocab, mutant=None):
    """bool [S, vocab], vectorised over the tokens of one length at a time"""
    trans = np.asarray(trans, dtype=np.uint8)
    S = len(trans)
    ext = np.full((256, 256), DEAD, dtype=np.uint8)   # row 255: the dead state stays dead
    ext[:S] = trans
    if mutant == "dead_is_row_255":
        ext[255] = trans[S - 1]
    out = np.zeros((S, vocab), dtype=bool)
    n_tok = min(len(toks), vocab)
    lens = np.array([len(toks[t]) for t in range(n_tok)], dtype=np.int64)
    start = np.arange(S, dtype=np.int64)[:, None]
    for L in np.unique(lens):
        ids = np.nonzero(lens == L)[0]
        if L == 0:
            if mutant == "allow_empty":
                out[:, ids] = True
            continue
        data = np.frombuffer(b"".join(toks[t] for t in ids), dtype=np.uint8).reshape(len(ids), L)
        cur = np.broadcast_to(start, (S, len(ids))).copy()
        steps = L - 1 if mutant == "skip_last_byte" else L
        for i in range(steps):
            cur = ext[cur, data[None, :, i]].astype(np.int64)
        out[:, ids] = cur != DEAD
    acc = np.asarray(accept).astype(bool)
    for t in ends:
        if 0 <= t < vocab:
            out[:, t] = True if mutant == "end_in_non_accepting" else acc
    return out


def pack(allowed, stride, fill=0, mutant=None):
    """bool [S, V] -> uint32 [S, stride]; words at or behind ceil(V / 32) keep `fill` (the kernel stores none of them)"""
    S, V = allowed.shape
    W = words(V)
    bits = np.zeros((S, W * 32), dtype=np.uint8)
    bits[:, :V] = allowed
    if mutant == "tail_bits":
        bits[:, V:] = 1
    w = np.packbits(bits.reshape(S, W, 32), axis=-1, bitorder="little").view(np.uint32).reshape(S, W)
    if mutant == "swap_ballot_words":
        w = w.copy()
        pairs = W // 2
        sw = w[:, :pairs * 2].reshape(S, pairs, 2)[:, :, ::-1].reshape(S, pairs * 2)
        w[:, :pairs * 2] = sw
    out = np.full((S, stride), fill, dtype=np.uint32)
    out[:, :W] = w
    return out


def ref_build(trans, accept, toks, ends, vocab, stride=None, fill=0, mutant=None):
    """(mask uint32 [S, stride], any uint32 [S])"""
    stride = words(vocab) if stride is None else stride
    allowed = ref_allowed(trans, accept, toks, ends, vocab, mutant)
    mask = pack(allowed, stride, fill, mutant)
    anyf = (mask[:, :words(vocab)] != 0).any(axis=1).astype(np.uint32)
    return mask, anyf


def ref_edit(image, off, stride, vocab, guide_slots, states, masks, mutant=None):
    """image: float32 flat; row b starts at off + b * stride.  masks uint32 [n_slots, S, mask_stride].  Returns the edited copy."""
    out = image.copy()
    n_slots, S, ms = masks.shape
    flat = masks.reshape(-1)
    for b, (g, s) in enumerate(zip(guide_slots, states)):
        if g < 0:
            continue
        row_words = ((g * S + s) * ms) if mutant != "state_stride" else ((g * S) * ms + s * words(vocab))
        w = flat[row_words:row_words + words(vocab)]
        bits = np.unpackbits(w.view(np.uint8), bitorder="little")[:vocab].astype(bool)
        row = out[off + b * stride: off + b * stride + vocab]
        row[~bits] = NINF
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------- cases

ALPHABET = b"abcdefgh"


def random_dfa(rng, S, p_dead=0.35, p_accept=0.3):
    """over ALPHABET, every other byte dead; a state without a live byte becomes accepting (what pplhip_guide_load demands)"""
    trans = np.full((S, 256), DEAD, dtype=np.uint8)
    for ch in ALPHABET:
        to = rng.integers(0, S, size=S)
        dead = rng.random(S) < p_dead
        trans[:, ch] = np.where(dead, DEAD, to)
    accept = (rng.random(S) < p_accept).astype(np.uint8)
    accept[(trans == DEAD).all(axis=1)] = 1
    accept[S - 1] = 0 if (trans[S - 1] != DEAD).any() else 1   # a non-accepting last state where it can be
    return trans, accept


def random_vocab(rng, n_tok, lens=(0, 1, 2, 3, 5), long_every=0):
    """token lengths drawn from `lens` (every long_every-th token 64 bytes); mostly the alphabet, one token in ten ends in a foreign byte"""
    L = np.asarray(lens)[rng.integers(0, len(lens), size=n_tok)]
    if long_every:
        L[1::long_every] = 64
    off = np.concatenate([[0], np.cumsum(L)])
    data = np.frombuffer(ALPHABET, dtype=np.uint8)[rng.integers(0, len(ALPHABET), size=int(off[-1]))].copy()
    foreign = (rng.random(n_tok) < 0.1) & (L > 0)
    data[off[1:][foreign] - 1] = ord("Z")
    blob = data.tobytes()
    return [blob[off[t]:off[t + 1]] for t in range(n_tok)]


class BCase:
    """one build: canary words behind every mask row (stride > words) and behind the table"""

    def __init__(self, name, trans, accept, toks, ends, vocab, pad=3):
        self.name, self.trans, self.accept, self.toks, self.ends, self.vocab = name, trans, accept, toks, list(ends), vocab
        self.S = len(trans)
        self.stride = words(vocab) + pad
        self.canary = np.uint32(0xC0FFEE11)

    def expect(self, mutant=None):
        """(mask image uint32 [S + 1, stride] with the canary row behind the table, any uint32 [S + 1] with a canary)"""
        mask, anyf = ref_build(self.trans, self.accept, self.toks, self.ends, self.vocab, self.stride, self.canary, mutant)
        img = np.full((self.S + 1, self.stride), self.canary, dtype=np.uint32)
        img[:self.S] = mask
        return img, np.concatenate([anyf, np.array([self.canary], dtype=np.uint32)])


SMALL_V = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257]


def build_specs(spm_pieces=None):
    """(name, thunk that makes the BCase) of every build case, so that the names cost nothing.
    spm_pieces: the 420 token byte strings of tests/golden/spm_bpe.model (None: those two cases are left out)"""
    out = []

    def small(i, V):
        rng = np.random.default_rng(20261019 + i)
        S = (1, 2, 255)[i % 3]
        trans, accept = random_dfa(rng, S)
        n_tok = V if i % 2 == 0 else max(1, V - 2)     # ids behind n_tok are empty
        return BCase(f"v{V}_s{S}", trans, accept, random_vocab(rng, n_tok), {0, V - 1}, V)

    def spm(V, ends):
        rng = np.random.default_rng(4201024)
        trans, accept = random_dfa(rng, 7)
        # the model test's vocabulary: 420 pieces, also inside a model vocabulary of 1024; the DFA reads lower-case letters and the space
        for ch in b"aeinorst ":
            trans[:, ch] = rng.integers(0, 7, size=7)
        return BCase(f"spm420_v{V}", trans, accept, list(spm_pieces), ends, V)

    def big(V, S):
        rng = np.random.default_rng(V + S)
        trans, accept = random_dfa(rng, S, p_dead=0.02 if S > 2 else 0.1)
        toks = random_vocab(rng, V - 5, lens=(0, 1, 1, 1), long_every=997)
        return BCase(f"v{V}_s{S}", trans, accept, toks, {0, V - 1}, V)

    for i, V in enumerate(SMALL_V):
        out.append((f"v{V}_s{(1, 2, 255)[i % 3]}", lambda i=i, V=V: small(i, V)))
    if spm_pieces is not None:
        out.append(("spm420_v1024", lambda: spm(1024, {2, 1023})))
        out.append(("spm420_v420", lambda: spm(420, {0, 419})))
    for V, S in ((32000, 255), (32000, 1), (128256, 2), (128256, 64)):
        out.append((f"v{V}_s{S}", lambda V=V, S=S: big(V, S)))
    return out


def build_cases(spm_pieces=None):
    return [make() for _, make in build_specs(spm_pieces)]


class MCase:
    """one mask edit: the whole logits image with a gap in front (off), canary columns behind every row's vocab and a canary row behind"""

    def __init__(self, name, B, V, stride, off, guide_slots, states, n_slots, S, seed, given_rows=False):
        rng = np.random.default_rng(seed)
        self.name, self.B, self.V, self.stride, self.off = name, B, V, stride, off
        self.guide_slots = np.asarray(guide_slots, dtype=np.int32)
        self.states = np.asarray(states, dtype=np.int32)
        self.n_slots, self.S, self.given_rows = n_slots, S, given_rows
        self.mask_stride = words(V) + 2
        self.masks = rng.integers(0, 2 ** 32, size=(n_slots, S, self.mask_stride), dtype=np.uint64).astype(np.uint32)
        # whole nibbles of ones and zeros too, so that all three forms of the 16-byte path are taken
        self.masks[:, :, ::3] = rng.choice(np.array([0, 0xFFFFFFFF, 0x0F0FF0F0, 0xFFFF0000], dtype=np.uint32), size=self.masks[:, :, ::3].shape)
        self.logits = rng.standard_normal(off + (B + 1) * stride).astype(np.float32)

    def image(self):
        return self.logits.copy()

    def expect(self, mutant=None):
        return ref_edit(self.logits, self.off, self.stride, self.V, self.guide_slots, self.states, self.masks, mutant)


def mask_cases():
    out = []
    seed = 77
    for V in (33, 32000):
        wide = (V + 3) // 4 * 4 + 4    # a multiple of 4 above V: the 16-byte path, with canary columns behind every row
        # tight: stride == V; off4: the rows' base off 16 bytes; odd: stride % 4 != 0
        for stride, off, tag in ((V, 0, "tight"), (wide, 0, "wide"), (wide, 1, "off4"), (wide - 1, 0, "odd")):
            B = 6
            seed += 1
            # asking and non-asking rows, two slots, states 0 and 254
            out.append(MCase(f"v{V}_{tag}", B, V, stride, off, [0, -1, 1, 1, -1, 0], [0, 9, 254, 0, 7, 254], 2, 255, seed,
                             given_rows=(seed % 2 == 0)))
    return out


def dev(torch, a):
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


def launch_build(m, torch, c):
    """runs pplhip_op_guide_build on case c; returns (rc, mask image, any image)"""
    img = np.full((c.S + 1, c.stride), c.canary, dtype=np.uint32)
    anyf = np.zeros(c.S + 1, dtype=np.uint32)
    anyf[c.S] = c.canary
    off = np.zeros(len(c.toks) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for t in c.toks])
    blob = np.frombuffer(b"".join(c.toks) + b"\0", dtype=np.uint8)
    d_tr, d_ac, d_blob, d_off = dev(torch, c.trans), dev(torch, c.accept), dev(torch, blob), dev(torch, off)
    d_end = dev(torch, np.asarray(c.ends, dtype=np.int32))
    d_mask, d_any = dev(torch, img), dev(torch, anyf)
    torch.cuda.synchronize()
    rc = m.lib().pplhip_op_guide_build(None, d_tr.data_ptr(), d_ac.data_ptr(), c.S, d_blob.data_ptr(), d_off.data_ptr(), len(c.toks),
                                       d_end.data_ptr(), len(c.ends), c.vocab, d_mask.data_ptr(), c.stride, d_any.data_ptr())
    torch.cuda.synchronize()
    return rc, d_mask.cpu().numpy().view(np.uint32), d_any.cpu().numpy().view(np.uint32)


def launch_mask(m, torch, c):
    """runs pplhip_op_guide_mask on case c; returns (rc, logits image)"""
    # the image starts 16-byte aligned (a fresh allocation), so off = 1 puts the rows' base off 16 bytes
    d = dev(torch, c.image())
    d_gs, d_st, d_masks = dev(torch, c.guide_slots), dev(torch, c.states), dev(torch, c.masks)
    rows, n_rows, d_rows = None, 0, None
    if c.given_rows:
        lst = np.nonzero(c.guide_slots >= 0)[0].astype(np.int32)
        d_rows = dev(torch, lst)
        rows, n_rows = d_rows.data_ptr(), len(lst)
    torch.cuda.synchronize()
    rc = m.lib().pplhip_op_guide_mask(None, d.data_ptr() + 4 * c.off, c.stride, c.V, c.B, d_gs.data_ptr(), d_st.data_ptr(), d_masks.data_ptr(),
                                      c.n_slots, c.S, c.mask_stride, rows, n_rows)
    torch.cuda.synchronize()
    return rc, d.cpu().numpy()


def spm_vocab(model="spm_bpe.model"):
    """(token bytes of every piece plus two empty ids behind them, piece count, EOS id) of a golden SentencePiece model, as the project's own
    tokenizer sees it (build/guide_trace vocab: Tokenizer::TokenBytes)"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "ppl.llm.serving_amd", "build", "guide_trace")
    assert os.path.exists(tool), f"{tool} is missing: build it with __graft_entry__.build()"
    out = subprocess.run([tool, "vocab", os.path.join(root, "tests", "golden", model)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(next(line for line in out.stdout.splitlines() if line.startswith("{")))
    assert rec["ok"] == 1
    return [bytes.fromhex(h) for h in rec["bytes"]], rec["pieces"], rec["eos"]


def compile_regex(pattern):
    """(trans uint8 [S, 256], accept uint8 [S]) of a pattern through the project's own compiler (build/guide_trace dfa); raises on a refusal"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "ppl.llm.serving_amd", "build", "guide_trace")
    assert os.path.exists(tool), f"{tool} is missing: build it with __graft_entry__.build()"
    out = subprocess.run([tool, "dfa"], input=pattern.encode("utf-8").hex() + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(next(line for line in out.stdout.splitlines() if line.startswith("{")))
    assert rec["ok"] == 1, rec
    S = rec["n_states"]
    return np.array(rec["trans"], dtype=np.uint8).reshape(S, 256), np.array(rec["accept"], dtype=np.uint8)
