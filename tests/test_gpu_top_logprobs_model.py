"""pplhip_top_logprobs, the product entry point, on the logits of a mixed prefill + decode step of configs/tiny_w8a16_kv8_paged.json: queued
in front of pplhip_sample_rows and read after it, against the reference on the copied logits of the same step (also behind the penalty
kernel with NULL temperatures); a step nobody asks in leaves the sampler's answers bit-identical; invalid arguments are refused."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import ref
from tests import top_logprobs as T
from tests.conftest import ROOT, load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CFG = os.path.join(ROOT, "ppl.llm.serving_amd", "configs", "tiny_w8a16_kv8_paged.json")
ND, NP = 3, 3                                            # decode rows (first), prefill rows of the mixed step
B = ND + NP
NLP = np.array([5, 0, 20, 1, 0, 19], dtype=np.int32)    # asking rows among the decode rows and among the prefill rows
TEMPS = np.array([0.7, 1.3, 1.0, 0.0, 2.0, 0.5], dtype=np.float32)
K = np.array([1, 50, 0, 1, 8, 1], dtype=np.int32)
TP = np.array([0.0, 0.9, 0.95, 1.0, 0.5, 0.0], dtype=np.float32)
SEEDS = np.array([11, 2 ** 40 + 3, 2 ** 64 - 5, 1, 2, 3], dtype=np.uint64)
DRAWS = np.array([1, 1, 1, 0, 0, 0], dtype=np.uint64)
PAGES = 8


@pytest.fixture(scope="module")
def model():
    """a context after a prefill step of ND requests; yields (binding, context, the mixed step that follows, vocab)"""
    m = load_pplhip()
    cfg = json.load(open(CFG))
    keys = ("num_heads", "num_kv_heads", "num_layers", "hidden_dim", "intermediate_dim", "vocab_size", "cache_quant_bit", "cache_quant_group",
            "cache_layout", "cache_mode", "page_size", "weight_quant_bit", "max_position")
    desc = ref.make_desc(**{k: cfg[k] for k in keys})
    assert desc.cache_mode == 1 and desc.page_size == 4
    ctx = m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=64, enable_penalty=True)
    ctx.init_synthetic(0, 3)
    ctx.kv_alloc(0, B * PAGES * desc.page_size)
    rng = np.random.RandomState(5)
    V = desc.vocab_size
    pages = np.arange(B * PAGES, dtype=np.int64).reshape(B, PAGES)
    first = [rng.randint(3, V, size=n) for n in (6, 3, 9)]
    lens = np.array([len(p) for p in first])
    ctx.set_inputs(0, m.make_step(np.concatenate(first), np.concatenate([[0], np.cumsum(lens)]), np.zeros(ND, dtype=np.int64), pages[:ND], 0,
                                  max_pages=PAGES, req_list_changed=1))
    ctx.run(0)
    ctx.sync(0)
    # the mixed step: one new token for each of the ND running requests, then NP prompts
    new = [rng.randint(3, V, size=n) for n in (7, 4, 11)]
    tok = np.concatenate([rng.randint(3, V, size=ND)] + new)
    seq = np.concatenate([[0], np.cumsum([1] * ND + [len(p) for p in new])])
    sp = np.concatenate([lens, np.zeros(NP, dtype=np.int64)])
    yield m, ctx, (tok, seq, sp, pages, ND), V
    ctx.close()


def _run(m, ctx, step):
    tok, seq, sp, pages, nd = step
    ctx.set_inputs(0, m.make_step(tok, seq, sp, pages, nd, max_pages=PAGES, req_list_changed=1))
    ctx.run(0)
    return ctx.copy_logits(B)


def _check(logits, V, nlp, temps, got):
    c = T.TCase("model", "model", logits, V, 0, nlp, temps)
    tok, lp = T.blank_outputs(len(c.asked))              # (the product's block has no canaries: the slots behind n are not compared)
    for j, b in enumerate(c.asked):
        n = int(nlp[b])
        tok[j, :n] = got[0][j, :n]
        lp[j, :n] = got[1][j, :n].view(np.uint32)
    fails, frac = T.check(c, tok, lp)
    print(f"largest logprob error {frac:.3f} of the bound")
    assert not fails, "; ".join(fails[:6])
    return c


def test_mixed_step_in_front_of_the_sampler(model):
    m, ctx, step, V = model
    logits = _run(m, ctx, step)
    read = ctx.top_logprobs(NLP, temperatures=TEMPS)
    assert read.rows == int((NLP > 0).sum())
    s_tok, s_lp = ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=TEMPS)      # the step's one synchronisation
    got = read()
    c = _check(logits, V, NLP, TEMPS, got)
    # entry 0 is the greedy rows' sampled token, and its logprob the sampler's within the two bounds
    for j, b in enumerate(c.asked):
        if K[b] == 1:
            _, wlp, log_s, lse = c.reference()[j]
            assert got[0][j, 0] == s_tok[b]
            assert abs(float(got[1][j, 0]) - float(s_lp[b])) <= T.entry_bound(V, log_s, lse, wlp[0]) + T.greedy_bound(V, log_s, lse, wlp[0])
    # pplhip_sync makes them readable as well, and the operator gives the same bits on the copied logits
    read2 = ctx.top_logprobs(NLP, temperatures=TEMPS)
    ctx.sync(0)
    got2 = read2()
    rc, o_tok, o_lp = T.launch(m, torch, c)
    assert rc == 0
    for j, b in enumerate(c.asked):
        n = int(NLP[b])
        assert (got2[0][j, :n] == got[0][j, :n]).all() and (got2[1][j, :n].view(np.uint32) == got[1][j, :n].view(np.uint32)).all()
        assert (o_tok[j, :n] == got[0][j, :n]).all() and (o_lp[j, :n] == got[1][j, :n].view(np.uint32)).all()


def test_behind_the_penalty_kernel_with_null_temperatures(model):
    m, ctx, step, V = model
    _run(m, ctx, step)
    rep = np.array([1.2, 1.0, 1.5, 0.8, 1.1, 1.0], dtype=np.float32)
    pres = np.array([0.1, 0.0, 0.3, 0.2, 0.0, 0.4], dtype=np.float32)
    freq = np.array([0.05, 0.2, 0.0, 0.1, 0.3, 0.0], dtype=np.float32)
    ctx.penalty(TEMPS, rep, pres, freq, np.array([5, 0, 2, 7, 1, 3], dtype=np.int64), req_list_changed=True)
    penalised = ctx.copy_logits(B)                       # already divided by the temperatures
    read = ctx.top_logprobs(NLP, temperatures=None)
    s_tok, _ = ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=None)
    c = _check(penalised, V, NLP, None, read())
    for j, b in enumerate(c.asked):
        if K[b] == 1:
            assert read()[0][j, 0] == s_tok[b]


def test_nobody_asks_and_the_sampler_is_untouched(model):
    m, ctx, step, V = model
    _run(m, ctx, step)
    alone = ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=TEMPS)
    _run(m, ctx, step)
    read = ctx.top_logprobs(np.zeros(B, dtype=np.int32), temperatures=TEMPS)
    assert read.rows == 0
    with_call = ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=TEMPS)
    assert (alone[0] == with_call[0]).all() and (alone[1].view(np.uint32) == with_call[1].view(np.uint32)).all()
    assert read()[0].shape == (0, T.NMAX)
    # ... and with somebody asking, too: the call reads the logits only
    _run(m, ctx, step)
    ctx.top_logprobs(NLP, temperatures=TEMPS)
    asked = ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=TEMPS)
    assert (alone[0] == asked[0]).all() and (alone[1].view(np.uint32) == asked[1].view(np.uint32)).all()


def test_invalid_arguments(model):
    m, ctx, step, V = model
    _run(m, ctx, step)
    lg = ctx.logits_ptr(0)[0]
    ok = np.array([1, 0, 20, 0, 0, 0, 0, 0, 0], dtype=np.int32)
    p_tok, p_lp, rows = C.c_void_p(), C.c_void_p(), C.c_int32(-1)

    def call(nlp=ok, batch=B, stride=V, logits=lg, args=True):
        a = m.TopLogprobsArgs()
        a.num_logprobs = None if nlp is None else nlp.ctypes.data
        a.batch, a.vocab_size, a.batch_stride = batch, V, stride
        return m.lib().pplhip_top_logprobs(ctx.h, logits, C.byref(a) if args else None, C.byref(p_tok), C.byref(p_lp), C.byref(rows))

    assert call(nlp=None) == -2
    assert call(nlp=np.array([1, 21, 0, 0, 0, 0], dtype=np.int32)) == -2
    assert call(nlp=np.array([1, -1, 0, 0, 0, 0], dtype=np.int32)) == -2
    assert call(batch=-1) == -2 and call(batch=9) == -2          # max_running_batch is 8
    assert call(stride=V - 1) == -2
    assert call(logits=None) == -2 and call(args=False) == -2
    assert rows.value == -1                                      # nothing was answered
    assert call(batch=0) == 0 and rows.value == 0
    assert call() == 0 and rows.value == 2
    ctx.sync(0)
