"""Guided decoding on the device, operator level (pplhip_op_guide_build / pplhip_op_guide_mask) against tests/guide.py.

Build kernel: the mask, bit for bit, with canary words behind every mask row and a canary row behind the table, and the per-state
any-flags with a canary behind them; vocabularies 1 .. 257, the 420 pieces of tests/golden/spm_bpe.model, synthetic vocabularies of 32000
and 128256 tokens with token lengths 0, 1 and 64; 1, 2, 64 and 255 states; end tokens at id 0 and id vocab - 1.
Mask kernel: the whole logits image bit for bit -- the asking rows, the others, the canary columns behind every row's vocab, the floats in
front of a base off 16 bytes and the canary row -- for a stride equal to vocab, above it, off the 16-byte path, vocab 33 and 32000, two
slots, states 0 and 254.  The refused arguments launch nothing."""
import faulthandler

import numpy as np
import pytest

from tests import guide as G
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STEP_SECONDS = 300     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run
_CASES = {}
BUILD_NAMES = [name for name, _ in G.build_specs(spm_pieces=())]


def build_case(idx):
    """made on first use and kept: the golden model's pieces are read once"""
    if "specs" not in _CASES:
        pieces, n, _ = G.spm_vocab()
        assert n == 420
        _CASES["specs"] = G.build_specs(pieces[:n])
    if idx not in _CASES:
        _CASES[idx] = _CASES["specs"][idx][1]()
    return _CASES[idx]


MASK = G.mask_cases()


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.cuda.synchronize()


@pytest.mark.parametrize("idx", range(len(BUILD_NAMES)), ids=BUILD_NAMES)
def test_build(idx):
    m = load_pplhip()
    c = build_case(idx)
    assert c.name == BUILD_NAMES[idx]
    want_mask, want_any = c.expect()
    rc, mask, anyf = G.launch_build(m, torch, c)
    assert rc == 0, f"{c.name}: pplhip_op_guide_build -> {rc}"
    if not G.same_bits(mask, want_mask):
        bad = np.argwhere(mask != want_mask)
        s, w = bad[0]
        pytest.fail(f"{c.name}: {len(bad)} mask words differ; first at state {s} word {w}: got {int(mask[s, w]):#010x} want {int(want_mask[s, w]):#010x}")
    assert G.same_bits(anyf, want_any), f"{c.name}: any-flags {anyf.tolist()[:16]} want {want_any.tolist()[:16]}"


def test_build_refused_arguments_write_nothing():
    m = load_pplhip()
    c = build_case(3)
    img = np.full((c.S + 1, c.stride), c.canary, dtype=np.uint32)
    d = {k: G.dev(torch, v) for k, v in dict(tr=c.trans, ac=c.accept, blob=np.zeros(4096, dtype=np.uint8), off=np.zeros(c.vocab + 1, dtype=np.int64),
                                               end=np.asarray(c.ends, dtype=np.int32), mask=img, any=np.zeros(c.S + 1, dtype=np.uint32)).items()}
    torch.cuda.synchronize()

    def call(S=c.S, n_tok=len(c.toks), n_end=len(c.ends), vocab=c.vocab, stride=c.stride, **null):
        p = {k: (None if k in null else t.data_ptr()) for k, t in d.items()}
        return m.lib().pplhip_op_guide_build(None, p["tr"], p["ac"], S, p["blob"], p["off"], n_tok, p["end"], n_end, vocab, p["mask"], stride, p["any"])
    assert call(S=0) == -2 and call(S=256) == -2
    assert call(vocab=0) == -2
    assert call(n_tok=c.vocab + 1) == -2 and call(n_tok=-1) == -2
    assert call(n_end=65) == -2 and call(n_end=-1) == -2
    assert call(stride=G.words(c.vocab) - 1) == -2
    for k in ("tr", "ac", "blob", "off", "end", "mask", "any"):
        assert call(**{k: True}) == -2, k
    torch.cuda.synchronize()
    assert G.same_bits(d["mask"].cpu().numpy().view(np.uint32), img)
    assert not d["any"].cpu().numpy().any()


@pytest.mark.parametrize("idx", range(len(MASK)), ids=[c.name for c in MASK])
def test_mask(idx):
    m = load_pplhip()
    c = MASK[idx]
    rc, got = G.launch_mask(m, torch, c)
    assert rc == 0, f"{c.name}: pplhip_op_guide_mask -> {rc}"
    want = c.expect()
    if not G.same_bits(got, want):
        bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        i = int(bad[0]) - c.off
        pytest.fail(f"{c.name}: {len(bad)} floats differ; first at row {i // c.stride} column {i % c.stride}: got {got[bad[0]]} want {want[bad[0]]}")


@pytest.mark.parametrize("given_rows", [False, True])
def test_mask_nobody_asks(given_rows):
    m = load_pplhip()
    src = MASK[1]
    c = G.MCase("nobody", src.B, src.V, src.stride, src.off, [-1] * src.B, [0] * src.B, 2, 255, 5, given_rows=given_rows)
    rc, got = G.launch_mask(m, torch, c)
    assert rc == 0
    assert G.same_bits(got, c.image())


def test_mask_refused_arguments_write_nothing():
    m = load_pplhip()
    c = MASK[1]
    img = c.image()
    d = G.dev(torch, img)
    gs, st, mk = G.dev(torch, c.guide_slots), G.dev(torch, c.states), G.dev(torch, c.masks)
    bad_state = G.dev(torch, np.where(c.guide_slots >= 0, 255, 0).astype(np.int32))
    bad_slot = G.dev(torch, np.where(c.guide_slots >= 0, 2, -1).astype(np.int32))
    torch.cuda.synchronize()

    def call(stride=c.stride, vocab=c.V, batch=c.B, slots=gs.data_ptr(), states=st.data_ptr(), masks=mk.data_ptr(), n_slots=c.n_slots, S=c.S,
             ms=c.mask_stride, n_rows=0):
        return m.lib().pplhip_op_guide_mask(None, d.data_ptr(), stride, vocab, batch, slots, states, masks, n_slots, S, ms, None, n_rows)
    assert call(batch=0) == 0
    assert call(stride=c.V - 1) == -2
    assert call(vocab=0) == -2
    assert call(batch=-1) == -2
    assert call(slots=None) == -2 and call(states=None) == -2 and call(masks=None) == -2
    assert call(n_slots=0) == -2 and call(n_slots=17) == -2
    assert call(S=0) == -2 and call(S=256) == -2
    assert call(ms=G.words(c.V) - 1) == -2
    assert call(n_rows=c.B + 1) == -2
    assert call(states=bad_state.data_ptr()) == -2      # a state behind the slot's rows
    assert call(slots=bad_slot.data_ptr()) == -2        # a slot behind `masks`
    torch.cuda.synchronize()
    assert G.same_bits(d.cpu().numpy(), img)
