"""Restaging a pinned block while its previous upload is still queued, on configs/tiny_w8a16_kv8_paged.json (2 layers, V = 1024),
max_running_batch 8, batch 4.  Every entry point that stages per-call arrays in a pinned block (the step inputs, the adapter tile list, the
prompt-logprobs ask, the logit-edit and guide-edit rows) waits for the copy that last read the block before it writes it again.  On an idle
stream that copy is long done when the next call comes, so each test first queues a few dozen decode steps with no synchronisation and
then calls the entry point twice in a row: the second call's staging can meet the first call's upload still waiting behind real work.

The steps keep the page list of the first one (req_list_changed = 0): a changed page list synchronises the stream and would drain it.
Results only, never timing: what the second call staged must not reach the first call's kernel.  These tests pin the results the guard
has to keep; they are no proof of the guard -- on an MI355X a build whose guard did not wait passed them too (the tiny model's queue
drains about as fast as the host fills it)."""
import json
import os

import numpy as np
import pytest

from oracle import ref
from tests import guide as G
from tests import logit_rules as R
from tests import lora_model as LM
from tests import prompt_logprobs as PL
from tests.conftest import ROOT, load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CFG = os.path.join(ROOT, "ppl.llm.serving_amd", "configs", "tiny_w8a16_kv8_paged.json")
CAP, B = 8, 4                                            # max_running_batch, the batch of every step
PAGES = 8                                                # pages per request (page_size 4: 32 KV tokens)
PRE = 8                                                  # tokens of the prefill that every test starts from
BUSY = 48                                                # decode steps queued in front of what a test is about
RULE_SLOTS = range(CAP)
GUIDE_SLOTS, GUIDE_STATES = (3, 9), 6
ADAPTERS = (0, 1, 2)                                     # adapter id = adapter slot (tests/lora_model.py ADAPTERS)


@pytest.fixture(scope="module")
def model():
    m = load_pplhip()
    cfg = json.load(open(CFG))
    keys = ("num_heads", "num_kv_heads", "num_layers", "hidden_dim", "intermediate_dim", "vocab_size", "cache_quant_bit", "cache_quant_group",
            "cache_layout", "cache_mode", "page_size", "weight_quant_bit", "max_position")
    desc = ref.make_desc(**{k: cfg[k] for k in keys})
    assert desc.cache_mode == 1 and desc.page_size == 4 and desc.vocab_size == 1024 and desc.num_layers == 2
    V = desc.vocab_size
    ctx = m.Context(m.copy_desc(desc), max_running_batch=CAP, max_tokens_per_step=64, enable_penalty=False)
    ctx.init_synthetic(0, 3)
    ctx.kv_alloc(0, B * PAGES * desc.page_size)
    # one logit rule per slot, every kind among them
    rules = {}
    for s in RULE_SLOTS:
        rules[s] = R._rule(np.random.default_rng(600 + s), V, R.KINDS[s % 4], R.N_BIAS[1 + s % 4], [1, V - 1, V, 40][s % 4])
        ctx.logit_rule_set(s, rules[s].bias, rules[s].mask, rules[s].stops)
    # two guides over a random vocabulary; the masks as the host reference builds them, by guide slot
    rng = np.random.default_rng(41)
    toks = G.random_vocab(rng, 600)
    ctx.guide_set_vocab(toks)
    masks = np.zeros((G.MAX_SLOTS, GUIDE_STATES, G.words(V)), dtype=np.uint32)
    for g in GUIDE_SLOTS:
        while True:                                      # (pplhip_guide_load wants a token for every state)
            trans, accept = G.random_dfa(rng, GUIDE_STATES)
            mask, anyf = G.ref_build(trans, accept, toks, [2], V)
            if anyf.all():
                break
        ctx.guide_load(g, trans, accept, [2])
        masks[g] = mask
    for a in ADAPTERS:
        tensors, scale = LM.make_adapter(desc, a)
        ctx.lora_set(0, a, tensors, scale)
    ctx.sync(0)
    yield m, ctx, desc, rules, masks
    ctx.close()


def _pages():
    return np.arange(B * PAGES, dtype=np.int64).reshape(B, PAGES)


def _start(m, ctx, V):
    """the state every pass starts from: PRE prompt tokens per request in the cache, the page list on the device, an idle stream"""
    rng = np.random.RandomState(2)
    ctx.set_inputs(0, m.make_step(rng.randint(3, V, size=B * PRE), np.arange(B + 1) * PRE, np.zeros(B, dtype=np.int64), _pages(), 0,
                                  max_pages=PAGES, req_list_changed=1))
    ctx.run(0)
    ctx.sync(0)


def _decode(m, ctx, tokens, pos):
    ctx.set_inputs(0, m.make_step(tokens, np.arange(B + 1), np.full(B, pos, dtype=np.int64), _pages(), B, max_pages=PAGES, req_list_changed=0))


def _busy(m, ctx, V):
    """BUSY decode steps of the same requests at position PRE, queued with no synchronisation"""
    for i in range(BUSY):
        _decode(m, ctx, (np.arange(B) * 37 + 11 * i + 5) % V, PRE)
        ctx.run(0)


def _buffers(seed):
    """two fp32 [B, V] device buffers and their host copies, made and synchronised before anything is queued"""
    g = np.random.default_rng(seed)
    host = [g.standard_normal((B, 1024)).astype(np.float32) * 4 for _ in range(2)]
    dev = [torch.from_numpy(h).cuda() for h in host]
    torch.cuda.synchronize()
    return host, dev


def test_logit_edit_twice_behind_a_busy_stream(model):
    m, ctx, desc, rules, _ = model
    V = desc.vocab_size
    (x0, y0), (X, Y) = _buffers(1)
    calls = [(np.array([5, 2, 7, 0], dtype=np.int64), np.array([3, 0, 1, 2], dtype=np.uint32), X, x0),      # rows 0, 2, 3 ask
             (np.array([1, 6, 3, 4], dtype=np.int64), np.array([0, 2, 3, 0], dtype=np.uint32), Y, y0)]      # rows 1, 2 ask, other slots
    _start(m, ctx, V)
    _busy(m, ctx, V)
    for slots, flags, buf, _ in calls:
        ctx.logit_edit(slots, flags, logits_ptr=buf.data_ptr())
    ctx.sync(0)
    for slots, flags, buf, before in calls:
        got = buf.cpu().numpy()
        for b in range(B):
            want = R.ref_edit(before[b], rules[int(slots[b])], int(flags[b]))
            assert R.same_bits(got[b], want), (b, int(slots[b]), int(flags[b]))
        assert not R.same_bits(got, before)


def test_guide_edit_twice_behind_a_busy_stream(model):
    m, ctx, desc, _, masks = model
    V = desc.vocab_size
    (x0, y0), (X, Y) = _buffers(2)
    calls = [(np.array([3, -1, 9, 3], dtype=np.int32), np.array([0, 0, 5, 2], dtype=np.int32), X, x0),      # rows 0, 2, 3 ask
             (np.array([-1, 9, -1, 9], dtype=np.int32), np.array([0, 1, 0, 4], dtype=np.int32), Y, y0)]     # rows 1, 3 ask, other guides
    _start(m, ctx, V)
    _busy(m, ctx, V)
    for slots, states, buf, _ in calls:
        ctx.guide_edit(slots, states, logits_ptr=buf.data_ptr())
    ctx.sync(0)
    for slots, states, buf, before in calls:
        want = G.ref_edit(before.reshape(-1), 0, V, V, slots.tolist(), states.tolist(), masks).reshape(B, V)
        got = buf.cpu().numpy()
        assert G.same_bits(got, want), np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        assert not G.same_bits(got, before)


STEP_TOKENS = [np.array([17, 901, 5, 333]), np.array([640, 3, 77, 1000]), np.array([8, 8, 512, 41]), np.array([999, 250, 6, 123])]
STEP_ADAPTERS = [np.array([0, -1, 1, 2]), np.array([1, 1, -1, 0]), np.array([-1, 2, 0, -1]), np.array([2, 0, 2, 1])]


@pytest.mark.parametrize("adapters", [False, True], ids=["plain", "adapters"])
def test_four_steps_without_synchronisation(model, adapters):
    """four decode steps with different tokens (and, `adapters`, a different adapter assignment each): synchronised after every step, then
    queued back to back behind a busy stream -- the step inputs' two staging blocks take turns, so the third step restages the first's, and
    the tile list has one block that every step restages.  Same final logits and the same cache, bit for bit."""
    m, ctx, desc, _, _ = model
    V = desc.vocab_size

    def four(sync):
        _start(m, ctx, V)
        _busy(m, ctx, V)
        for i, tok in enumerate(STEP_TOKENS):
            _decode(m, ctx, tok, PRE + 1 + i)
            if adapters:
                ctx.set_adapters(0, STEP_ADAPTERS[i])
            ctx.run(0)
            if sync:
                ctx.sync(0)
        return ctx.copy_logits(B), ctx.kv_read(0, 0), ctx.kv_read(0, 1)

    want = four(True)
    got = four(False)
    for g, w, what in zip(got, want, ("logits", "cache", "cache scales")):
        assert R.same_bits(g, w), what
    if adapters:                                         # the adapters do act on these steps
        _start(m, ctx, V)
        for i, tok in enumerate(STEP_TOKENS):
            _decode(m, ctx, tok, PRE + 1 + i)
            ctx.run(0)
        assert not R.same_bits(ctx.copy_logits(B), got[0])


def test_two_asking_prefill_steps_back_to_back(model):
    m, ctx, desc, _, _ = model
    V = desc.vocab_size
    rng = np.random.RandomState(9)
    steps = []
    for lens, ask in (((5, 3, 6, 2), (0, 2, -1, 20)), ((4, 7, 2, 5), (20, -1, 0, 1))):
        seq = np.concatenate([[0], np.cumsum(lens)])
        steps.append((rng.randint(3, V, size=int(seq[-1])), seq, np.array(ask, dtype=np.int32)))

    def ask_step(tok, seq, ask):
        ctx.set_inputs(0, m.make_step(tok, seq, np.zeros(B, dtype=np.int64), _pages(), 0, max_pages=PAGES, req_list_changed=0))
        ctx.set_prompt_logprobs(0, ask)
        ctx.run(0)

    _start(m, ctx, V)
    _busy(m, ctx, V)
    ask_step(*steps[1])                                  # the second step alone
    ctx.sync(0)
    want = ctx.prompt_logprobs(0)
    _start(m, ctx, V)
    _busy(m, ctx, V)
    ask_step(*steps[0])
    ask_step(*steps[1])
    ctx.sync(0)
    got = ctx.prompt_logprobs(0)
    rows, ntop = PL.positions(steps[1][1], steps[1][2])
    assert len(rows) == 3 + 1 + 4 and R.same_bits(got[0], rows) and R.same_bits(want[0], rows)
    assert R.same_bits(got[1], want[1]) and R.same_bits(got[2], want[2])
    for j, n in enumerate(ntop):                         # (the slots behind a position's n are unspecified)
        assert R.same_bits(got[3][j, :n], want[3][j, :n]) and R.same_bits(got[4][j, :n], want[4][j, :n]), j
    assert np.isfinite(got[1]).all() and (got[2] >= 0).all()
