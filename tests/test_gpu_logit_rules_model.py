"""pplhip_logit_rule_set / pplhip_logit_edit, the product entry points, on the logits of a mixed prefill + decode step of
configs/tiny_w8a16_kv8_paged.json (V = 1024): sixteen rules set back to back, then a step and one edit, the logits before and after
against the reference bit for bit; then the existing consumers on edited rows -- the greedy sampler, the top-k / top-p sampler with
replayed random numbers, top-N logprobs and the penalty kernel -- which have never seen a -inf logit before; and every refusal."""
import json
import os

import numpy as np
import pytest

from oracle import ref
from tests import logit_rules as R
from tests import postproc as P
from tests import top_logprobs as T
from tests.conftest import ROOT, load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CFG = os.path.join(ROOT, "ppl.llm.serving_amd", "configs", "tiny_w8a16_kv8_paged.json")
ND, NP = 3, 3                                            # decode rows (first), prefill rows of the mixed step
B = ND + NP
PAGES = 8
CAP = 16                                                 # max_running_batch: the slots of the rule table
SLOTS = np.array([15, 3, 8, 0, 11, 6], dtype=np.int64)   # the rows' batch slots: not the identity
FLAGS = np.array([3, 1, 0, 2, 3, 1], dtype=np.uint32)
GAP = 2.0 ** -6


@pytest.fixture(scope="module")
def model():
    """a context after a prefill step of ND requests; yields (binding, context, the mixed step that follows, its prompts, vocab)"""
    m = load_pplhip()
    cfg = json.load(open(CFG))
    keys = ("num_heads", "num_kv_heads", "num_layers", "hidden_dim", "intermediate_dim", "vocab_size", "cache_quant_bit", "cache_quant_group",
            "cache_layout", "cache_mode", "page_size", "weight_quant_bit", "max_position")
    desc = ref.make_desc(**{k: cfg[k] for k in keys})
    assert desc.cache_mode == 1 and desc.page_size == 4 and desc.vocab_size == 1024
    ctx = m.Context(m.copy_desc(desc), max_running_batch=CAP, max_tokens_per_step=64, enable_penalty=True)
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
    new = [rng.randint(3, V, size=n) for n in (7, 4, 11)]
    tok = np.concatenate([rng.randint(3, V, size=ND)] + new)
    seq = np.concatenate([[0], np.cumsum([1] * ND + [len(p) for p in new])])
    sp = np.concatenate([lens, np.zeros(NP, dtype=np.int64)])
    yield m, ctx, (tok, seq, sp, pages, ND), new, V
    ctx.close()


def _run(m, ctx, step, copy=True):
    tok, seq, sp, pages, nd = step
    ctx.set_inputs(0, m.make_step(tok, seq, sp, pages, nd, max_pages=PAGES, req_list_changed=1))
    ctx.run(0)
    return ctx.copy_logits(B) if copy else None


def _set(ctx, slot, rule, check=True):
    return ctx.logit_rule_set(slot, rule.bias, rule.mask, rule.stops, check=check)


def _spread(x, n, rng, among=None):
    """n tokens of the row whose logits are pairwise at least GAP apart (so no 1-ulp matter decides a winner among them)"""
    out = []
    for t in rng.permutation(x.size if among is None else among):
        if np.isfinite(x[t]) and all(abs(float(x[t]) - float(x[u])) >= GAP for u in out):
            out.append(int(t))
            if len(out) == n:
                return out
    raise AssertionError("the row has no such tokens")


def _sixteen_rules(V):
    """one rule per slot, every kind among them; independent of any logits"""
    rules = {}
    for s in range(CAP):
        rng = np.random.default_rng(900 + s)
        rules[s] = R._rule(rng, V, R.KINDS[s % 4], R.N_BIAS[s % 5], [1, V - 1, V, 40][s % 4])
    return rules


def test_sixteen_rules_back_to_back_then_one_edit(model):
    m, ctx, step, _, V = model
    rules = _sixteen_rules(V)
    for s in range(CAP):                                 # nothing synchronises in between: the staging ring has four records
        _set(ctx, s, rules[s])
    before = _run(m, ctx, step)
    ctx.logit_edit(SLOTS, FLAGS)
    after = ctx.copy_logits(B)
    for b in range(B):
        want = R.ref_edit(before[b], rules[int(SLOTS[b])], int(FLAGS[b]))
        assert R.same_bits(after[b], want), f"row {b} (slot {SLOTS[b]}, flags {FLAGS[b]}): {np.flatnonzero(after[b].view(np.uint32) != want.view(np.uint32))[:8]}"
    assert R.same_bits(after[2], before[2])              # flags 0
    assert any(not R.same_bits(after[b], before[b]) for b in range(B))
    # all flags 0: no device call, the logits stay bit for bit
    before2 = _run(m, ctx, step)
    assert R.same_bits(before2, before)
    ctx.logit_edit(SLOTS, np.zeros(B, dtype=np.uint32))
    assert R.same_bits(ctx.copy_logits(B), before2)
    # a later rule of a slot replaces the earlier one
    _set(ctx, int(SLOTS[0]), R.Rule(bias=[(7, -np.inf)]))
    ctx.logit_edit(SLOTS, np.array([1, 0, 0, 0, 0, 0], dtype=np.uint32))
    again = ctx.copy_logits(B)
    assert R.same_bits(again[0], R.ref_edit(before2[0], R.Rule(bias=[(7, -np.inf)]), 1)) and R.same_bits(again[1:], before2[1:])


def _three_live(m, ctx, step, V):
    """runs the step, gives every row a rule with three live tokens (a mask of five, one of them banned, one a suppressed stop) and edits:
    (the logits before, the edited logits as the reference has them, the live tokens per row)"""
    before = _run(m, ctx, step)
    rng = np.random.default_rng(77)
    live, want = [], []
    for b in range(B):
        five = _spread(before[b], 5, rng)
        rule = R.Rule(bias=[(five[3], -np.inf), (five[0], 0.25)], mask=R.pack_mask(five, V), stops=[five[4]])
        _set(ctx, int(SLOTS[b]), rule)
        want.append(R.ref_edit(before[b], rule, 3))
        live.append(five[:3])
        assert len({float(want[-1][t]) for t in five[:3]}) == 3      # no ties among the live: their order is the float order
    ctx.logit_edit(SLOTS, np.full(B, 3, dtype=np.uint32))
    return before, np.stack(want), live


def _margin_ok(row):
    top = np.sort(row[np.isfinite(row)].astype(np.float64))[::-1]
    return top.size >= 2 and top[0] - top[1] >= GAP


def test_greedy_sampler_on_edited_rows(model):
    m, ctx, step, _, V = model
    before = _run(m, ctx, step)
    rng = np.random.default_rng(78)
    want = []
    for b in range(B):
        # five allowed tokens; after the bias of +0.25 on the first the best two live ones must still be 2^-6 apart: pick until they are
        for _ in range(50):
            five = _spread(before[b], 5, rng)
            rule = R.Rule(bias=[(five[3], -np.inf), (five[0], 0.25)], mask=R.pack_mask(five, V), stops=[five[4]])
            row = R.ref_edit(before[b], rule, 3)
            if _margin_ok(row):
                break
        assert _margin_ok(row), b                        # asserted on the host before the device runs
        assert int(np.isfinite(row).sum()) == 3
        _set(ctx, int(SLOTS[b]), rule)
        want.append(row)
    want = np.stack(want)
    ctx.logit_edit(SLOTS, np.full(B, 3, dtype=np.uint32))
    tok, lp = ctx.sample(B, top_k=1)
    assert R.same_bits(ctx.copy_logits(B), want)
    for b in range(B):
        wtok, wlp, log_s, lse = T.ref_row(want[b], 1)
        assert int(tok[b]) == int(wtok[0]) == int(np.argmax(want[b])), (b, tok[b], wtok[0])
        bound = T.greedy_bound(V, log_s, lse, wlp[0])
        print(f"row {b}: logprob {lp[b]!r} want {wlp[0]!r} bound {bound:.3g}")
        assert abs(float(lp[b]) - float(wlp[0])) <= bound, (b, lp[b], wlp[0], bound)


def test_sampler_never_draws_a_dead_token(model):
    m, ctx, step, _, V = model
    _, want, live = _three_live(m, ctx, step, V)
    after = ctx.copy_logits(B)
    assert R.same_bits(after, want)
    us = np.array([0.0, 0.2, 0.5, 0.75, 0.999, float(P.RND_TOP)], dtype=np.float32)
    for b in (0, 4):
        rows = np.repeat(after[b][None, :], us.size, axis=0)
        d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        k = torch.full((us.size,), 50, dtype=torch.int32, device="cuda")
        p = torch.full((us.size,), 1.0, dtype=torch.float32, device="cuda")
        z = torch.zeros(us.size, dtype=torch.int64, device="cuda")
        u = torch.from_numpy(us).cuda()
        o_tok = torch.full((us.size,), -5, dtype=torch.int32, device="cuda")
        o_lp = torch.zeros(us.size, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc = m.lib().pplhip_op_sample_rows(None, d.data_ptr(), None, k.data_ptr(), p.data_ptr(), z.data_ptr(), z.data_ptr(), u.data_ptr(),
                                           us.size, V, V, o_tok.data_ptr(), o_lp.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        got = o_tok.cpu().numpy().tolist()
        print(f"row {b}: live {live[b]} drawn {got}")
        assert all(t in live[b] for t in got), (b, got, live[b])
        order = sorted(live[b], key=lambda t: -float(want[b][t]))
        assert got[0] == order[0] and got[-1] == order[-1]      # u = 0: the most probable; u just under 1: the least probable LIVE token
        assert np.isfinite(o_lp.cpu().numpy()).all()


def test_top_logprobs_on_an_edited_row(model):
    m, ctx, step, _, V = model
    _, want, live = _three_live(m, ctx, step, V)
    nlp = np.array([20, 0, 0, 0, 20, 0], dtype=np.int32)
    read = ctx.top_logprobs(nlp)
    ctx.sync(0)
    tok, lp = read()
    for j, b in enumerate((0, 4)):
        order = sorted(live[b], key=lambda t: -float(want[b][t]))
        dead = [t for t in range(V) if t not in live[b]][:17]
        assert tok[j].tolist() == order + dead, (b, tok[j].tolist(), order)       # the live tokens first, then -inf entries by token
        assert np.isfinite(lp[j, :3]).all() and np.isneginf(lp[j, 3:]).all(), lp[j]
        wtok, wlp, log_s, lse = T.ref_row(want[b], 20)
        assert wtok.tolist() == tok[j].tolist()
        for e in range(3):
            assert abs(float(lp[j, e]) - float(wlp[e])) <= T.entry_bound(V, log_s, lse, wlp[e])


def test_penalty_chain_keeps_dead_tokens_dead(model):
    m, ctx, step, prompts, V = model
    before = _run(m, ctx, step)
    rng = np.random.default_rng(79)
    rep, pres, temp = np.float32(1.3), np.float32(0.5), np.float32(0.7)

    def penalised(row, counted):
        y = row.copy()
        for t in set(int(t) for t in counted):
            x = y[t]
            x = np.float32(x / rep) if x > 0 else np.float32(x * rep)
            y[t] = np.float32(x - pres)
        return (y / temp).astype(np.float32)

    want = {}
    rules = {}
    for b in range(B):
        among = None
        for _ in range(50):
            forty = _spread(before[b], 40, rng, among)
            # a counted token among the allowed ones where the row has one (prefill rows: their prompt is counted at this step)
            if b >= ND:
                forty[0] = int(prompts[b - ND][0])
            rule = R.Rule(bias=[(forty[1], 0.5), (forty[2], -np.inf)], mask=R.pack_mask(forty, V), stops=[forty[3]])
            edited = R.ref_edit(before[b], rule, 3)
            if b < ND or _margin_ok(penalised(edited, prompts[b - ND])):
                break
        rules[b] = (rule, edited)
        _set(ctx, int(SLOTS[b]), rule)
        if b >= ND:
            want[b] = penalised(edited, prompts[b - ND])
            assert _margin_ok(want[b]), b
    ctx.logit_edit(SLOTS, np.full(B, 3, dtype=np.uint32))
    ctx.penalty(np.full(B, temp), np.full(B, rep), np.full(B, pres), None, SLOTS, req_list_changed=True)
    tok, _ = ctx.sample(B, top_k=1, enable_penalty=True)
    after = ctx.copy_logits(B)
    for b in range(B):
        dead = np.isneginf(rules[b][1])
        assert dead.sum() >= V - 40 and np.isneginf(after[b][dead]).all(), b     # exactly -inf still
        assert np.isfinite(after[b][~dead]).all()
        assert not dead[int(tok[b])]
    for b in range(ND, B):                               # rows whose count map is this step's prompt: the whole arithmetic is known
        assert int(tok[b]) == int(np.argmax(want[b])), (b, tok[b], int(np.argmax(want[b])))
        live = ~np.isneginf(want[b])
        assert np.allclose(after[b][live], want[b][live], rtol=1e-6, atol=0)


def test_refusals(model):
    m, ctx, step, _, V = model
    _run(m, ctx, step, copy=False)
    ctx.sync(0)
    nan, inf = float("nan"), float("inf")

    def refused(what, **kw):
        slot = kw.pop("slot", 1)
        rc = ctx.logit_rule_set(slot, kw.get("bias", ()), kw.get("mask"), kw.get("stops", ()), check=False)
        msg = m.lib().pplhip_last_error(ctx.h, 0).decode()
        assert rc == -2 and msg.startswith("logit rule") and what in msg, (what, rc, msg)

    refused("slot", slot=CAP)
    refused("slot", slot=-1)
    refused("bias_tokens", bias=[(V, 1.0)])
    refused("bias_tokens", bias=[(-1, 1.0)])
    refused("stop_tokens", stops=[V])
    refused("NaN", bias=[(1, nan)])
    refused("+inf", bias=[(1, inf)])
    refused("has an entry already", bias=[(1, 1.0), (2, 1.0), (1, 2.0)])
    refused("n_bias", bias=[(t % V, 1.0) for t in range(513)])
    refused("n_stop", stops=list(range(65)))
    refused("no token", mask=R.pack_mask([], V))
    refused("no token", mask=R.pack_mask([4, 5, 6], V), bias=[(4, -inf), (5, -inf)], stops=[6])
    refused("no token", bias=[(t, -inf) for t in range(512)], stops=list(range(512, 576)), mask=R.pack_mask(range(576), V))
    # the boundaries that pass: one live token, 512 biases, 64 stops
    assert ctx.logit_rule_set(1, [(t, -inf) for t in range(512)], R.pack_mask(range(577), V), list(range(512, 576)), check=False) == 0
    # the edit's own refusals
    ok = np.array([1, 0, 0, 0, 0, 0], dtype=np.uint32)
    assert ctx.logit_edit(SLOTS, np.array([4, 0, 0, 0, 0, 0], dtype=np.uint32), check=False) == -2
    assert ctx.logit_edit(np.array([CAP, 0, 0, 0, 0, 0], dtype=np.int64), ok, check=False) == -2
    assert ctx.logit_edit(np.array([-1, 0, 0, 0, 0, 0], dtype=np.int64), ok, check=False) == -2
    assert ctx.logit_edit(np.full(B, 2 ** 63 - 1, dtype=np.int64), np.zeros(B, dtype=np.uint32), check=False) == 0   # nobody asks: slots unread
    ctx.sync(0)


def test_a_slot_without_a_rule_cannot_ask():
    m = load_pplhip()
    cfg = json.load(open(CFG))
    keys = ("num_heads", "num_kv_heads", "num_layers", "hidden_dim", "intermediate_dim", "vocab_size", "cache_quant_bit", "cache_quant_group",
            "cache_layout", "cache_mode", "page_size", "weight_quant_bit", "max_position")
    desc = ref.make_desc(**{k: cfg[k] for k in keys})
    ctx = m.Context(m.copy_desc(desc), max_running_batch=4, max_tokens_per_step=16, enable_penalty=False)
    try:
        one = np.array([1], dtype=np.uint32)
        assert ctx.logit_edit(np.array([0], dtype=np.int64), np.zeros(1, dtype=np.uint32), check=False) == 0
        assert ctx.logit_edit(np.array([0], dtype=np.int64), one, check=False) == -2          # no rule was ever set: no table
        ctx.logit_rule_set(2, [(3, 1.0)])
        assert ctx.logit_edit(np.array([0], dtype=np.int64), one, check=False) == -2          # slot 0 holds none
        ctx.sync(0)
    finally:
        ctx.close()
