"""Numpy reference of the wide guide build (guide_build16_kernel of csrc/k_guide.hip; DESIGN.md "numerics", guided decoding row), the cases of
its operator test and the named mutants that tests/test_guide16_spec.py tells apart on those cases.

A wide guide is a byte-level DFA of up to 4096 live states: trans uint16 [S, 256] (0xFFFF = the dead state, which has no row; state 255 is
an ordinary live state), accept uint8 [S].  The vocabulary, the bit layout, the end tokens and `any` are those of tests/guide.py:

  build   mask[s] bit t = accept[s]                                        if t is an end token
                        = 0                                                if token t is empty (also every id at or behind n_tok)
                        = walking its bytes from s never meets the dead state   otherwise

The device's grid is (token block, chunk of CHUNK states); the two chunk mutants model a chunk that is lost or lands at the wrong rows.
"""
import numpy as np

from tests import guide

DEAD = 0xFFFF
MAX_STATES = 4096
CHUNK = 64          # the mutants' chunk; the GPU test takes the kernel's from pplhip_guide16_state_chunk() and compares
words = guide.words
same_bits = guide.same_bits

MUTANTS = ("state_low_byte", "dead_is_255", "dead_row_indexed", "last_chunk_dropped", "chunk_stride", "skip_last_byte", "end_in_non_accepting",
           "tail_bits")


def walk(trans, state, data):
    """the state after `data` from `state`, DEAD as soon as the dead state is met (GuideDfa16::Step)"""
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
    """bool [S, vocab], vectorised over the tokens of one length at a time.  The dead state is index S of the extended table."""
    trans = np.asarray(trans, dtype=np.uint16)
    S = len(trans)
    ext = np.full((S + 1, 256), S, dtype=np.int64)     # row S: the dead state stays dead
    ext[:S] = np.where(trans == DEAD, S, trans.astype(np.int64))
    if mutant == "dead_is_255" and S > 255:
        ext[ext == 255] = S
    if mutant == "dead_row_indexed":
        ext[S] = ext[DEAD % S]
    out = np.zeros((S, vocab), dtype=bool)
    n_tok = min(len(toks), vocab)
    lens = np.array([len(toks[t]) for t in range(n_tok)], dtype=np.int64)
    start = np.arange(S, dtype=np.int64)[:, None]
    for L in np.unique(lens):
        ids = np.nonzero(lens == L)[0]
        if L == 0:
            continue
        data = np.frombuffer(b"".join(toks[t] for t in ids), dtype=np.uint8).reshape(len(ids), L)
        cur = np.broadcast_to(start, (S, len(ids))).copy()
        steps = L - 1 if mutant == "skip_last_byte" else L
        for i in range(steps):
            cur = ext[cur, data[None, :, i]]
            if mutant == "state_low_byte":
                cur = np.where(cur == S, S, np.minimum(cur & 255, S - 1))
        out[:, ids] = cur != S
    acc = np.asarray(accept).astype(bool)
    for t in ends:
        if 0 <= t < vocab:
            out[:, t] = True if mutant == "end_in_non_accepting" else acc
    return out


def ref_build(trans, accept, toks, ends, vocab, stride=None, fill=0, mutant=None, chunk=CHUNK):
    """(mask uint32 [S, stride], any uint32 [S]); rows that a chunk mutant never writes keep `fill` (and any 0)"""
    stride = words(vocab) if stride is None else stride
    allowed = ref_allowed(trans, accept, toks, ends, vocab, mutant)
    mask = guide.pack(allowed, stride, fill, "tail_bits" if mutant == "tail_bits" else None)
    anyf = (mask[:, :words(vocab)] != 0).any(axis=1).astype(np.uint32)
    S = len(mask)
    if mutant == "last_chunk_dropped" and S % chunk:
        keep = S // chunk * chunk
        mask[keep:] = fill
        anyf[keep:] = 0
    if mutant == "chunk_stride":
        moved = np.full_like(mask, fill)
        moved_any = np.zeros_like(anyf)
        for s in range(S):   # chunk c lands at rows c * (chunk / 2) ..: later chunks overwrite earlier ones
            to = (s // chunk) * (chunk // 2) + s % chunk
            moved[to] = mask[s]
            moved_any[to] = anyf[s]
        mask, anyf = moved, moved_any
    return mask, anyf


# ---------------------------------------------------------------------------------------------------------------- cases

ALPHABET = guide.ALPHABET


def random_dfa(rng, S, p_dead=0.35, p_accept=0.3):
    """guide.random_dfa on 16 bits.  Beyond 256 states the mutants are made visible by construction: state 255 is reached from the start and
    is live, the walk crosses 255 / 256 in both directions, and state 256 differs from state 0 in acceptance and in its row."""
    trans = np.full((S, 256), DEAD, dtype=np.uint16)
    for ch in ALPHABET:
        to = rng.integers(0, S, size=S)
        dead = rng.random(S) < p_dead
        trans[:, ch] = np.where(dead, DEAD, to)
    accept = (rng.random(S) < p_accept).astype(np.uint8)
    pin_wide(trans, accept)
    return trans, accept


def pin_wide(trans, accept):
    """what random_dfa promises beyond 256 states, written into the table (again, where a case has redrawn whole columns since)"""
    S = len(trans)
    if S > 256:
        a, b, c = ALPHABET[0], ALPHABET[1], ALPHABET[2]
        trans[0, a] = 255           # start -> 255
        trans[255, a] = 256         # 255 -> 256: upwards across the byte
        trans[256, a] = 3 % S       # 256 -> a low state: downwards across it
        trans[256, b] = S - 1       # and to the last state
        trans[0, b] = DEAD          # state 0 and state 256 differ in byte b ...
        trans[0, c] = 256
        accept[0], accept[256] = 1, 0   # ... and in acceptance
    accept[(trans == DEAD).all(axis=1)] = 1
    if S > 1 and (trans[S - 1] != DEAD).any():
        accept[S - 1] = 0           # a non-accepting last state where it can be


def widen(trans8):
    """a narrow table (uint8, dead 255) as a wide one"""
    t = np.asarray(trans8, dtype=np.uint8)
    return np.where(t == guide.DEAD, DEAD, t.astype(np.uint16)).astype(np.uint16)


class BCase(guide.BCase):
    """guide.BCase with the wide reference"""

    def expect(self, mutant=None, chunk=CHUNK):
        mask, anyf = ref_build(self.trans, self.accept, self.toks, self.ends, self.vocab, self.stride, self.canary, mutant, chunk)
        img = np.full((self.S + 1, self.stride), self.canary, dtype=np.uint32)
        img[:self.S] = mask
        return img, np.concatenate([anyf, np.array([self.canary], dtype=np.uint32)])


SMALL_S = [1, 255, 256, 257]
SMALL_V = [1, 31, 32, 33, 63, 64, 65, 257]


def build_specs(spm_pieces=None, chunk=CHUNK):
    """(name, thunk that makes the BCase) of every build case.  spm_pieces: the 420 token byte strings of tests/golden/spm_bpe.model (None:
    that case is left out); chunk: the grid's state chunk, whose edges get a case each"""
    out = []

    def small(S, V):
        rng = np.random.default_rng(20261020 + 1000 * S + V)
        trans, accept = random_dfa(rng, S)
        n_tok = V if (S + V) % 2 == 0 else max(1, V - 2)     # ids behind n_tok are empty
        return BCase(f"s{S}_v{V}", trans, accept, guide.random_vocab(rng, n_tok), {0, V - 1}, V)

    def big(S, V, p_dead, tag=""):
        rng = np.random.default_rng(V + S)
        trans, accept = random_dfa(rng, S, p_dead=p_dead)
        toks = guide.random_vocab(rng, V - 5, lens=(0, 1, 2, 3, 9), long_every=997)   # 9 and 64: past the eight bytes a lane keeps
        return BCase(f"{tag}s{S}_v{V}", trans, accept, toks, {0, V - 1}, V)

    def spm(S):
        rng = np.random.default_rng(4204096)
        trans, accept = random_dfa(rng, S)
        for ch in b"aeinorst ":     # the pieces' own letters and the space
            trans[:, ch] = rng.integers(0, S, size=S)
        pin_wide(trans, accept)     # "a" and "e" were redrawn
        return BCase(f"s{S}_spm420", trans, accept, list(spm_pieces), {0, 419}, 420)

    for S in SMALL_S:
        for V in SMALL_V:
            out.append((f"s{S}_v{V}", lambda S=S, V=V: small(S, V)))
    out.append(("s4096_v2048", lambda: big(4096, 2048, 0.35)))       # the cap
    out.append(("s257_v128256", lambda: big(257, 128256, 0.1)))      # row stride past one block's tokens and past 2^16 bits
    out.append(("s1000_v32000", lambda: big(1000, 32000, 0.1)))      # the L2-resident table at a real vocabulary
    if spm_pieces is not None:
        out.append(("s4096_spm420", lambda: spm(4096)))
    for S in sorted({chunk - 1, chunk, chunk + 1, 2 * chunk + 1}):
        if S >= 1:
            out.append((f"chunk_s{S}_v300", lambda S=S: big(S, 300, 0.35, "chunk_")))
    return out


def dev(torch, a):
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def launch_build(m, torch, c, narrow=False):
    """runs pplhip_op_guide_build16 on case c (narrow: pplhip_op_guide_build on its uint8 table); returns (rc, mask image, any image)"""
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
    fn = m.lib().pplhip_op_guide_build if narrow else m.lib().pplhip_op_guide_build16
    rc = fn(None, d_tr.data_ptr(), d_ac.data_ptr(), c.S, d_blob.data_ptr(), d_off.data_ptr(), len(c.toks), d_end.data_ptr(), len(c.ends), c.vocab,
            d_mask.data_ptr(), c.stride, d_any.data_ptr())
    torch.cuda.synchronize()
    return rc, d_mask.cpu().numpy().view(np.uint32), d_any.cpu().numpy().view(np.uint32)


def launch_mask(m, torch, c):
    """runs pplhip_op_guide_mask16 on a guide.MCase; returns (rc, logits image)"""
    d = dev(torch, c.image())
    d_gs, d_st, d_masks = dev(torch, c.guide_slots), dev(torch, c.states), dev(torch, c.masks)
    rows, n_rows, d_rows = None, 0, None
    if c.given_rows:
        lst = np.nonzero(c.guide_slots >= 0)[0].astype(np.int32)
        d_rows = dev(torch, lst)
        rows, n_rows = d_rows.data_ptr(), len(lst)
    torch.cuda.synchronize()
    rc = m.lib().pplhip_op_guide_mask16(None, d.data_ptr() + 4 * c.off, c.stride, c.V, c.B, d_gs.data_ptr(), d_st.data_ptr(), d_masks.data_ptr(),
                                        c.n_slots, c.S, c.mask_stride, rows, n_rows)
    torch.cuda.synchronize()
    return rc, d.cpu().numpy()


def compile_schemas(schemas):
    """every schema (a dict, or its text) through the project's own compiler (build/guide_json_trace dfa): a list of records, {"ok": 0, "err"}
    or {"ok": 1, "n_states", "trans" uint16 [S, 256], "accept" uint8 [S]}"""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "ppl.llm.serving_amd", "build", "guide_json_trace")
    assert os.path.exists(tool), f"{tool} is missing: build it with __graft_entry__.build()"
    texts = [s if isinstance(s, str) else json.dumps(s, ensure_ascii=False) for s in schemas]
    out = subprocess.run([tool, "dfa"], input="".join(t.encode("utf-8").hex() + "\n" for t in texts), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    recs = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert len(recs) == len(texts)
    for r in recs:
        if r["ok"]:
            r["trans"] = np.frombuffer(bytes.fromhex(r["trans"]), dtype="<u2").reshape(r["n_states"], 256)
            r["accept"] = np.array(r["accept"], dtype=np.uint8)
    return recs


def compile_schema(schema):
    """(trans, accept) of one schema; raises on a refusal"""
    rec = compile_schemas([schema])[0]
    assert rec["ok"] == 1, rec
    return rec["trans"], rec["accept"]


def accepts(trans, accept, data):
    """(accepted, the number of bytes read before the dead state or the end)"""
    s = 0
    for i, b in enumerate(data):
        s = int(trans[s, b])
        if s == DEAD:
            return False, i
    return bool(accept[s]), len(data)


def longest(trans, accept):
    """the bytes of the longest accepted string, None when the language is infinite (the trimmed automaton has a cycle)"""
    S = len(trans)
    succ = [sorted(set(trans[s].tolist()) - {DEAD}) for s in range(S)]
    depth, state = {}, {}     # memo; state: 1 = on the stack

    def visit(s):
        stack = [(s, iter(succ[s]))]
        state[s] = 1
        best = {s: 0}
        while stack:
            cur, it = stack[-1]
            nxt = next(it, None)
            if nxt is None:
                stack.pop()
                state[cur] = 2
                depth[cur] = best[cur]
                if stack:
                    best[stack[-1][0]] = max(best[stack[-1][0]], depth[cur] + 1)
                continue
            if state.get(nxt) == 1:
                return False
            if state.get(nxt) == 2:
                best[cur] = max(best[cur], depth[nxt] + 1)
                continue
            state[nxt] = 1
            best[nxt] = 0
            stack.append((nxt, iter(succ[nxt])))
        return True

    return depth[0] if visit(0) else None
