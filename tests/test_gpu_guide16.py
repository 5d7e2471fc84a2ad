"""The wide guide on the device, operator level (pplhip_op_guide_build16 / pplhip_op_guide_mask16) against tests/guide16.py, bit for bit.

Build kernel: the mask with canary words behind every mask row and a canary row behind the table, the per-state any-flags with a canary
behind them.  States 1, 255, 256 and 257 at vocabularies 1 .. 257; the cap of 4096 states at 2048 tokens and at the 420 pieces of
tests/golden/spm_bpe.model; 257 states at 128256 tokens; 1000 states at 32000 tokens; one case at every edge of the grid's state chunk
(chunk - 1, chunk, chunk + 1, 2 chunk + 1), the chunk taken from pplhip_guide16_state_chunk().  A narrow automaton widened to 16 bits gives
the bytes of pplhip_op_guide_build.
Mask kernel under its wide symbol: states 0, 255, 256 and 4095 in two slots, the whole logits image bit for bit.
The refused arguments of both launch nothing."""
import faulthandler

import numpy as np
import pytest

from tests import guide as G8
from tests import guide16 as G
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STEP_SECONDS = 300     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run
_CASES = {}
# the names cost nothing; the chunk cases are named after the reference's chunk, which test_chunk_constant holds equal to the kernel's
BUILD_NAMES = [name for name, _ in G.build_specs(spm_pieces=())]


def chunk():
    return int(load_pplhip().lib().pplhip_guide16_state_chunk())


def build_case(idx):
    """made on first use and kept: the golden model's pieces are read once"""
    if "specs" not in _CASES:
        pieces, n, _ = G8.spm_vocab()
        assert n == 420
        _CASES["specs"] = G.build_specs(pieces[:n], chunk=chunk())
    if idx not in _CASES:
        _CASES[idx] = _CASES["specs"][idx][1]()
    return _CASES[idx]


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.cuda.synchronize()


def check(c, rc, mask, anyf, want_mask, want_any, what):
    assert rc == 0, f"{c.name}: {what} -> {rc}"
    if not G.same_bits(mask, want_mask):
        bad = np.argwhere(mask != want_mask)
        s, w = bad[0]
        pytest.fail(f"{c.name}: {len(bad)} mask words differ; first at state {s} word {w}: got {int(mask[s, w]):#010x} want {int(want_mask[s, w]):#010x}")
    assert G.same_bits(anyf, want_any), f"{c.name}: any-flags differ first at state {int(np.argmax(anyf != want_any))}"


def test_chunk_constant():
    c = chunk()
    assert 1 <= c <= G.MAX_STATES
    assert c == G.CHUNK, "tests/guide16.py's chunk mutants are written for another chunk size than the kernel's"
    assert [n for n, _ in G.build_specs(spm_pieces=(), chunk=c)] == BUILD_NAMES


@pytest.mark.parametrize("idx", range(len(BUILD_NAMES)), ids=BUILD_NAMES)
def test_build(idx):
    m = load_pplhip()
    c = build_case(idx)
    assert c.name == BUILD_NAMES[idx]
    want_mask, want_any = c.expect()
    rc, mask, anyf = G.launch_build(m, torch, c)
    check(c, rc, mask, anyf, want_mask, want_any, "pplhip_op_guide_build16")


@pytest.mark.parametrize("S,V", [(255, 257), (64, 32000)])
def test_widened_narrow_automaton_gives_the_narrow_kernels_bytes(S, V):
    m = load_pplhip()
    rng = np.random.default_rng(S + V)
    trans, accept = G8.random_dfa(rng, S)
    toks = G8.random_vocab(rng, V - 3, long_every=97)
    narrow = G8.BCase(f"narrow_s{S}_v{V}", trans, accept, toks, {0, V - 1}, V)
    wide = G.BCase(f"wide_s{S}_v{V}", G.widen(trans), accept, toks, {0, V - 1}, V)
    rc8, mask8, any8 = G.launch_build(m, torch, narrow, narrow=True)
    assert rc8 == 0
    rc, mask, anyf = G.launch_build(m, torch, wide)
    check(wide, rc, mask, anyf, mask8, any8, "pplhip_op_guide_build16 against pplhip_op_guide_build")
    want_mask, want_any = wide.expect()
    check(wide, rc, mask, anyf, want_mask, want_any, "pplhip_op_guide_build16")


def test_build_refused_arguments_write_nothing():
    m = load_pplhip()
    c = build_case(BUILD_NAMES.index("s257_v33"))
    img = np.full((c.S + 1, c.stride), c.canary, dtype=np.uint32)
    d = {k: G.dev(torch, v) for k, v in dict(tr=c.trans, ac=c.accept, blob=np.zeros(4096, dtype=np.uint8), off=np.zeros(c.vocab + 1, dtype=np.int64),
                                               end=np.asarray(c.ends, dtype=np.int32), mask=img, any=np.zeros(c.S + 1, dtype=np.uint32)).items()}
    torch.cuda.synchronize()

    def call(S=c.S, n_tok=len(c.toks), n_end=len(c.ends), vocab=c.vocab, stride=c.stride, **null):
        p = {k: (None if k in null else t.data_ptr()) for k, t in d.items()}
        return m.lib().pplhip_op_guide_build16(None, p["tr"], p["ac"], S, p["blob"], p["off"], n_tok, p["end"], n_end, vocab, p["mask"], stride, p["any"])
    assert call(S=0) == -2 and call(S=4097) == -2 and call(S=-1) == -2
    assert call(vocab=0) == -2
    assert call(n_tok=c.vocab + 1) == -2 and call(n_tok=-1) == -2
    assert call(n_end=65) == -2 and call(n_end=-1) == -2
    assert call(stride=G.words(c.vocab) - 1) == -2
    for k in ("tr", "ac", "blob", "off", "end", "mask", "any"):
        assert call(**{k: True}) == -2, k
    torch.cuda.synchronize()
    assert G.same_bits(d["mask"].cpu().numpy().view(np.uint32), img)
    assert not d["any"].cpu().numpy().any()


# (vocab, stride, off, seed): a stride equal to vocab, the 16-byte path with a base off 16 bytes, a stride off the 16-byte path
MASK_SPECS = [(33, 33, 0, 1), (32000, 32004, 1, 2), (32000, 32003, 0, 3)]


@pytest.mark.parametrize("V,stride,off,seed", MASK_SPECS, ids=[f"v{s[0]}_stride{s[1]}_off{s[2]}" for s in MASK_SPECS])
def test_mask(V, stride, off, seed):
    m = load_pplhip()
    # asking and non-asking rows, two slots, states on both sides of 8 bits and the last one.  The operator takes ONE n_states for all its
    # slots; slots of different sizes and kinds side by side are compared with the reference through the context calls
    # (tests/test_gpu_guide_json_model.py: a wide slot of more than 300 states, a narrow one and a wide one of 29)
    c = G8.MCase(f"v{V}_stride{stride}_off{off}", 6, V, stride, off, [0, -1, 1, 1, -1, 0], [0, 9, 255, 256, 7, 4095], 2, 4096, seed,
                 given_rows=(seed % 2 == 0))
    rc, got = G.launch_mask(m, torch, c)
    assert rc == 0, f"{c.name}: pplhip_op_guide_mask16 -> {rc}"
    want = c.expect()
    if not G.same_bits(got, want):
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        i = int(bad[0]) - c.off
        pytest.fail(f"{c.name}: {len(bad)} floats differ; first at row {i // c.stride} column {i % c.stride}: got {got[bad[0]]} want {want[bad[0]]}")


def test_mask_refused_arguments_write_nothing():
    m = load_pplhip()
    c = G8.MCase("refused", 6, 33, 36, 0, [0, -1, 1, 1, -1, 0], [0, 9, 255, 256, 7, 299], 2, 300, 9)
    img = c.image()
    d = G.dev(torch, img)
    gs, st, mk = G.dev(torch, c.guide_slots), G.dev(torch, c.states), G.dev(torch, c.masks)
    bad_state = G.dev(torch, np.where(c.guide_slots >= 0, 300, 0).astype(np.int32))
    bad_slot = G.dev(torch, np.where(c.guide_slots >= 0, 2, -1).astype(np.int32))
    torch.cuda.synchronize()

    def call(fn=m.lib().pplhip_op_guide_mask16, stride=c.stride, vocab=c.V, batch=c.B, slots=gs.data_ptr(), states=st.data_ptr(), masks=mk.data_ptr(),
             n_slots=c.n_slots, S=c.S, ms=c.mask_stride, n_rows=0):
        return fn(None, d.data_ptr(), stride, vocab, batch, slots, states, masks, n_slots, S, ms, None, n_rows)
    assert call(batch=0) == 0
    assert call(stride=c.V - 1) == -2
    assert call(vocab=0) == -2
    assert call(batch=-1) == -2
    assert call(slots=None) == -2 and call(states=None) == -2 and call(masks=None) == -2
    assert call(n_slots=0) == -2 and call(n_slots=17) == -2
    assert call(S=0) == -2 and call(S=4097) == -2
    assert call(ms=G.words(c.V) - 1) == -2
    assert call(n_rows=c.B + 1) == -2
    assert call(states=bad_state.data_ptr()) == -2      # a state behind the slot's rows
    assert call(slots=bad_slot.data_ptr()) == -2        # a slot behind `masks`
    assert call(fn=m.lib().pplhip_op_guide_mask) == -2  # 300 states: the narrow symbol keeps its bound
    torch.cuda.synchronize()
    assert G.same_bits(d.cpu().numpy(), img)
