"""The post-processing chain on the device, through the context API, on configs/tiny_w8a16_kv8_paged.json (2 layers, V = 1024),
max_running_batch 8: a rule in every batch slot, two guides, three adapters; one mixed step (two decode rows, six prefill rows of at most 12
tokens) and five decode steps.  After every ctx.run the logits are read (the "before" image) and guide_edit, logit_edit, penalty,
top_logprobs and sample_rows run on the context's own logits in the engine's order with no synchronisation in between; the results are held
against tests/chain.py's ref_chain on the device's own "before" image, so the model's arithmetic is no part of the comparison.  The rows of
one batch ask for different subsets of the features (chain.PATTERNS), once in a context with the penalty and once without, where the
temperatures go to top-N and the sampler instead.

  image behind guide and rules   bit for bit (read in a pass of its own, then the "before" image is written back and the whole chain runs)
  image behind the penalty       chain.check_penalty: postproc.check_penalty_step, dead tokens exactly -inf.  The context keeps its count
                                 map to itself; a count shows in the logits (chain.counts_show names the rows where one off by one would)
  tokens                         sample_rows.check_rows (postproc.check_sample), greedy logprobs within top_logprobs.greedy_bound
  top-N                          tokens exact, logprobs within top_logprobs.entry_bound, by list place
No tolerance of this file's own.  Then, bit for bit: a row gets alone what it got in the mixed batch; rows that ask for nothing are
untouched and draw what they draw when nobody asks; rows without an adapter do not see their neighbours' adapters."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import ref
from tests import chain as C
from tests import logit_rules as R
from tests import lora_model as LM
from tests import prompt_logprobs as PL
from tests.conftest import ROOT, load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CFG = os.path.join(ROOT, "ppl.llm.serving_amd", "configs", "tiny_w8a16_kv8_paged.json")
B, PAGES = 8, 8                                          # the batch of every step; pages per request (page_size 4: 32 KV tokens)
ADAPTERS = (0, 1, 2)                                     # adapter id = adapter slot (tests/lora_model.py ADAPTERS)
ADAPTER_ROWS = np.array([0, -1, 1, -1, 2, -1, 0, -1], dtype=np.int32)       # half the rows, more than one row on adapter 0


class Box:
    pass


@pytest.fixture(scope="module", params=[True, False], ids=["penalty", "plain"])
def model(request):
    m = load_pplhip()
    cfg = json.load(open(CFG))
    keys = ("num_heads", "num_kv_heads", "num_layers", "hidden_dim", "intermediate_dim", "vocab_size", "cache_quant_bit", "cache_quant_group",
            "cache_layout", "cache_mode", "page_size", "weight_quant_bit", "max_position")
    desc = ref.make_desc(**{k: cfg[k] for k in keys})
    assert desc.cache_mode == 1 and desc.page_size == 4 and desc.vocab_size == C.V and desc.num_layers == 2
    ctx = m.Context(m.copy_desc(desc), max_running_batch=C.CAP, max_tokens_per_step=64, enable_penalty=request.param)
    ctx.init_synthetic(0, 3)
    ctx.kv_alloc(0, B * PAGES * desc.page_size)
    tb = C.Tables()
    tb.assert_live()
    for s, rule in tb.rules.items():
        ctx.logit_rule_set(s, rule.bias, rule.mask, rule.stops)
    ctx.guide_set_vocab(tb.toks)
    for g in C.GUIDE_SLOTS:
        ctx.guide_load(g, tb.trans[g], tb.accept[g], tb.ends)
    for a in ADAPTERS:
        tensors, scale = LM.make_adapter(desc, a)
        ctx.lora_set(0, a, tensors, scale)
    ctx.sync(0)
    box = Box()
    box.m, box.ctx, box.tables, box.pen, box.runs = m, ctx, tb, request.param, {}
    yield box
    ctx.close()


def _pages():
    return np.arange(B * PAGES, dtype=np.int64).reshape(B, PAGES)


def _restore(box, image):
    """writes a saved image back into the context's logits buffer"""
    ptr, stride = box.ctx.logits_ptr(0)
    assert stride == C.V
    img = np.ascontiguousarray(image, dtype=np.float32)
    box.ctx.sync(0)
    copy = box.m.lib().hipMemcpy
    copy.argtypes, copy.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int], ctypes.c_int
    assert copy(ptr, img.ctypes.data, img.nbytes, 1) == 0            # host to device
    box.ctx.sync(0)


def _model_step(box, state, first, adapters):
    """feeds the state's step to the model and returns the "before" image"""
    m, ctx = box.m, box.ctx
    tok = np.concatenate([np.asarray(s, dtype=np.int64) for s in state.seqs])
    seq = np.concatenate([[0], np.cumsum([len(s) for s in state.seqs])])
    ctx.set_inputs(0, m.make_step(tok, seq, np.asarray(state.start_pos), _pages(), state.dec, max_pages=PAGES, req_list_changed=int(first)))
    if adapters is not None:
        ctx.set_adapters(0, adapters)
    if first:
        ctx.set_prompt_logprobs(0, np.asarray(state.prompt_ask, dtype=np.int32))
    ctx.run(0)
    return ctx.copy_logits(B), seq


def _edits(box, st):
    box.ctx.guide_edit(st.guide_slots, st.guide_states)
    box.ctx.logit_edit(st.slots, st.flags)


def _chain(box, st):
    """the five calls in the engine's order, nothing synchronised in between: (final image, tokens, logprobs, top-N tokens, top-N logprobs)"""
    ctx, t = box.ctx, (None if box.pen else st.temps)
    _edits(box, st)
    if box.pen:
        ctx.penalty(st.temps, st.rep, st.pres, st.freq, st.slots, req_list_changed=True)
    read = ctx.top_logprobs(st.nlp, temperatures=t)
    tok, lp = ctx.sample_rows(st.top_k, st.top_p, st.seeds, st.draws, temperatures=t)
    top_tok, top_lp = read()
    return ctx.copy_logits(B), tok, lp, top_tok, top_lp


def _start(box, batch, asking):
    """the two decode rows' prompts go in (and are counted, where the penalty is on); returns the state in front of the mixed step"""
    m, ctx = box.m, box.ctx
    pr = C.case_prompts(batch)[:2]
    lens = [len(p) for p in pr]
    ctx.set_inputs(0, m.make_step(np.concatenate(pr), np.concatenate([[0], np.cumsum(lens)]), np.zeros(2, dtype=np.int64), _pages()[:2], 0,
                                  max_pages=PAGES, req_list_changed=1))
    ctx.run(0)
    state = C.start_state(box.tables, batch, asking)
    if box.pen:
        ctx.penalty(np.ones(2), np.ones(2), np.zeros(2), np.zeros(2), np.asarray(state.slots[:2], dtype=np.int64), req_list_changed=True)
    ctx.sync(0)
    return state


def _run(box, batch, asking=None, adapters=None, check=False):
    """chain.STEPS steps, every row fed its own token: per step a Box of the device's images and results (and, check, every comparison)"""
    state = _start(box, batch, asking)
    out = []
    for s in range(C.STEPS):
        d = Box()
        d.before, seq = _model_step(box, state, s == 0, adapters)
        st = d.st = state.step(d.before)
        _edits(box, st)
        d.edited = box.ctx.copy_logits(B)
        _restore(box, d.before)
        d.final, d.tok, d.lp, d.top_tok, d.top_lp = _chain(box, st)
        res = d.res = C.ref_chain(st, state, box.pen, penalised=d.final if box.pen else None)
        d.top_of_row = {b: (d.top_tok[j, :st.nlp[b]].copy(), d.top_lp[j, :st.nlp[b]].copy()) for j, b in enumerate(res.asked)}
        if s == 0:
            d.prompt = box.ctx.prompt_logprobs(0)
            rows, _ = PL.positions(seq, np.asarray(state.prompt_ask, dtype=np.int32))
            assert R.same_bits(d.prompt[0], rows) and np.isfinite(d.prompt[1]).all()      # the prompt ask has a position list of its own
        if check:
            tag = (batch, s)
            bad = np.flatnonzero((d.edited.view(np.uint32) != res.edited.view(np.uint32)).any(axis=1))
            assert bad.size == 0, (tag, "rows whose image behind guide and rules differs", bad.tolist())
            assert not R.same_bits(d.edited, d.before)
            if box.pen:
                fails = C.check_penalty(st, res, d.final)
                assert not fails, (tag, fails[:4])
                shown = C.counts_show(st, res)
                print(f"batch {batch} step {s}: a count off by one would show in rows {shown}")
                assert set(shown) >= {b for b in range(B) if state.patterns[b] and not state.patterns[b] & (C.GUIDE | C.RULE)}, (tag, shown)
            else:
                assert R.same_bits(d.final, res.edited), tag          # top-N and the sampler write nothing
            fails = C.check_tokens(res, d.tok, d.lp) + C.check_greedy_logprobs(res, d.tok, d.lp) + C.check_top(st, res, d.top_tok, d.top_lp)
            print(f"batch {batch} step {s}: tokens {d.tok.tolist()}; sampling rows not compared exactly: {C.left_out(res)}")
            assert not fails, (tag, fails[:6])
        C.advance(state, d.tok, res.cm)
        out.append(d)
    return out


def _cached(box, batch):
    """the mixed run of a batch, checked against the reference, once per context"""
    if batch not in box.runs:
        box.runs[batch] = _run(box, batch, check=True)
    return box.runs[batch]


@pytest.mark.parametrize("batch", [0, 1])
def test_mixed_batch_against_the_reference_chain(model, batch):
    run = _cached(model, batch)
    assert len(run) == C.STEPS
    states = np.array([d.st.guide_states for d in run])
    assert (states[1:] != states[:-1]).any()             # the guides moved
    flags = np.array([d.st.flags for d in run])
    assert (flags == 3).any() and (flags[-1] != 3).all() # the stop-suppress bit was there and left


def _same_row(a, b, row, what):
    """row `row` of two steps' results, bit for bit"""
    for k in ("before", "edited", "final"):
        assert R.same_bits(getattr(a, k)[row], getattr(b, k)[row]), (what, row, k)
    assert a.tok[row] == b.tok[row] and R.same_bits(a.lp[row:row + 1], b.lp[row:row + 1]), (what, row, a.tok[row], b.tok[row])
    assert (row in a.top_of_row) == (row in b.top_of_row)
    if row in a.top_of_row:
        assert (a.top_of_row[row][0] == b.top_of_row[row][0]).all() and R.same_bits(a.top_of_row[row][1], b.top_of_row[row][1]), (what, row)


def test_a_row_alone_gets_what_it_got_in_the_mixed_batch(model):
    """on the mixed step: the saved "before" image goes back into the context's buffer and the chain runs with one row asking"""
    box = model
    mixed = _cached(box, 0)[0]
    state = _start(box, 0, None)
    before, _ = _model_step(box, state, True, None)
    assert R.same_bits(before, mixed.before)
    for b in (C.ROW_ALL, C.ROW_GUIDE_ONLY, C.ROW_GREEDY_BEHIND_SAMPLING):
        assert state.start_pos[b] == 0                   # a prefill row: the penalty counts its prompt afresh on every call
        alone = C.start_state(box.tables, 0, asking=(b,))
        st = alone.step(mixed.before)
        d = Box()
        d.before = mixed.before
        _restore(box, mixed.before)
        _edits(box, st)
        d.edited = box.ctx.copy_logits(B)
        _restore(box, mixed.before)
        d.final, d.tok, d.lp, top_tok, top_lp = _chain(box, st)
        asked = [r for r in range(B) if st.nlp[r] > 0]
        assert asked == ([b] if mixed.st.nlp[b] > 0 else []) and top_tok.shape[0] == len(asked)
        d.top_of_row = {r: (top_tok[j, :st.nlp[r]], top_lp[j, :st.nlp[r]]) for j, r in enumerate(asked)}
        _same_row(d, mixed, b, "alone")
        for r in range(B):                               # and nobody else was touched by guide or rules
            if r != b:
                assert R.same_bits(d.edited[r], mixed.before[r]), (b, r)


def test_plain_rows_are_untouched_and_draw_what_they_draw_when_nobody_asks(model):
    box = model
    mixed = _cached(box, 0)
    nobody = _run(box, 0, asking=())
    b = C.ROW_NONE
    for s, (dm, dn) in enumerate(zip(mixed, nobody)):
        assert R.same_bits(dm.edited[b], dm.before[b]) and R.same_bits(dm.final[b], dm.before[b]), s       # neutral penalties at temperature 1
        assert R.same_bits(dn.edited, dn.before) and dn.top_tok.shape[0] == 0, s
        _same_row(dm, dn, b, f"nobody asks, step {s}")
    assert any((dm.tok != dn.tok).any() for dm, dn in zip(mixed, nobody))     # the others did ask for something


def test_rows_without_an_adapter_do_not_see_their_neighbours_adapters(model):
    box = model
    mixed = _cached(box, 0)
    with_adapters = _run(box, 0, adapters=ADAPTER_ROWS)
    for s, (dm, da) in enumerate(zip(mixed, with_adapters)):
        for b in range(B):
            if ADAPTER_ROWS[b] < 0:
                _same_row(dm, da, b, f"adapters, step {s}")
    assert all(any(not R.same_bits(dm.before[b], da.before[b]) for dm, da in zip(mixed, with_adapters)) for b in range(B) if ADAPTER_ROWS[b] >= 0)
