"""pplhip_guide_set_vocab / _load / _unload / _edit, the product entry points, in a decode loop on configs/tiny_w8a16_kv8_paged.json
(V = 1024) with the vocabulary of tests/golden/spm_bpe.model (420 pieces, all 256 byte pieces among them): three guided rows with
finite-language patterns beside three plain rows, greedy and sampled.  Every guided row must end on the end token within the longest match
+ 1 steps with bytes that re.fullmatch its pattern; the plain rows' logits and tokens are bit for bit those of the same batch run without
any guide.  Then the refusals, among them a pattern whose automaton needs a byte no piece of a tokenizer without byte fallback has."""
import json
import os
import re

import numpy as np
import pytest

from oracle import ref
from tests import guide as G
from tests.conftest import ROOT, load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CFG = os.path.join(ROOT, "ppl.llm.serving_amd", "configs", "tiny_w8a16_kv8_paged.json")
PATTERNS = ["(yes|no|maybe)", "[0-9]{3}-[0-9]{4}", '\\{"ok": (true|false), "n": [1-9][0-9]{0,2}\\}']
LONGEST = [len("maybe"), len("000-0000"), len('{"ok": false, "n": 123}')]   # bytes of each pattern's longest match
B = 6
GUIDED = [0, 2, 4]                                       # batch rows of the three patterns; 1, 3, 5 are plain
PAGES = 16
STEPS = max(LONGEST) + 1                                 # generation_length = the longest match in bytes + 1


@pytest.fixture(scope="module")
def setup():
    m = load_pplhip()
    cfg = json.load(open(CFG))
    keys = ("num_heads", "num_kv_heads", "num_layers", "hidden_dim", "intermediate_dim", "vocab_size", "cache_quant_bit", "cache_quant_group",
            "cache_layout", "cache_mode", "page_size", "weight_quant_bit", "max_position")
    desc = ref.make_desc(**{k: cfg[k] for k in keys})
    assert desc.cache_mode == 1 and desc.page_size == 4 and desc.vocab_size == 1024
    pieces, n, eos = G.spm_vocab()
    assert n == 420 and eos == 2
    assert {p for p in pieces if len(p) == 1} == {bytes([b]) for b in range(256)}   # every byte has a piece: every live state has a token
    ctx = m.Context(m.copy_desc(desc), max_running_batch=16, max_tokens_per_step=64, enable_penalty=False)
    ctx.init_synthetic(0, 3)
    ctx.kv_alloc(0, B * PAGES * desc.page_size)
    ctx.guide_set_vocab(pieces[:n])
    dfas = [G.compile_regex(p) for p in PATTERNS]
    yield m, ctx, desc, pieces[:n], eos, dfas
    ctx.close()


def _decode(m, ctx, desc, pieces, eos, dfas, guided, sampled):
    """STEPS steps of B requests (a prefill step, then decode steps); returns (the tokens [STEPS, B], the plain rows' logits per step, the
    step at which each guided row drew the end token)"""
    rng = np.random.RandomState(11)
    V = desc.vocab_size
    pages = np.arange(B * PAGES, dtype=np.int64).reshape(B, PAGES)
    prompts = [rng.randint(3, 420, size=n) for n in (5, 3, 7, 4, 6, 2)]
    lens = np.array([len(p) for p in prompts])
    slots = np.full(B, -1, dtype=np.int32)
    states = np.zeros(B, dtype=np.int32)
    if guided:
        for k, b in enumerate(GUIDED):
            slots[b] = k + 3                                 # guide slots 3, 4, 5: not the rows' own numbers
    tokens, plain_logits, done = [], [], {}
    seeds = np.arange(1, B + 1, dtype=np.uint64) * np.uint64(7919)
    last = None
    for step in range(STEPS):
        if step == 0:
            st = m.make_step(np.concatenate(prompts), np.concatenate([[0], np.cumsum(lens)]), np.zeros(B, dtype=np.int64), pages, 0,
                             max_pages=PAGES, req_list_changed=1)
        else:
            st = m.make_step(last, np.arange(B + 1), lens + step - 1, pages, B, max_pages=PAGES, req_list_changed=0)
        ctx.set_inputs(0, st)
        ctx.run(0)
        ctx.guide_edit(slots, states)
        logits = ctx.copy_logits(B)
        plain_logits.append(logits[[b for b in range(B) if b not in GUIDED]].copy())
        if guided:   # what the guided rows may draw is exactly what their automaton allows
            for k, b in enumerate(GUIDED):
                if slots[b] < 0:
                    continue
                trans, accept = dfas[k]
                alive = np.isfinite(logits[b])
                for t in range(V):
                    want = bool(accept[states[b]]) if t == eos else (t < len(pieces) and len(pieces[t]) > 0 and
                                                                       G.walk(trans, int(states[b]), pieces[t]) != G.DEAD)
                    assert alive[t] == want, (step, b, t)
        if sampled:
            tok, _ = ctx.sample_rows(np.full(B, 40), np.full(B, 0.95), seeds, np.full(B, step, dtype=np.uint64), temperatures=np.full(B, 1.5))
        else:
            tok, _ = ctx.sample(B, top_k=1, req_list_changed=(step == 0))
        tok = tok.astype(np.int64)
        tokens.append(tok.copy())
        for k, b in enumerate(GUIDED):
            if slots[b] < 0:
                continue
            if tok[b] == eos:
                done[b] = step
                slots[b] = -1                                # the request has finished: its row stays in the batch, unguided, to keep the shape
            else:
                states[b] = G.walk(dfas[k][0], int(states[b]), pieces[tok[b]])
                assert states[b] != G.DEAD
        last = tok % 420
    return np.stack(tokens), plain_logits, done


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_guided_rows_match_and_plain_rows_are_untouched(setup, sampled):
    m, ctx, desc, pieces, eos, dfas = setup
    base_tokens, base_logits, _ = _decode(m, ctx, desc, pieces, eos, dfas, guided=False, sampled=sampled)
    for k, (tr, ac) in enumerate(dfas):
        ctx.guide_load(k + 3, tr, ac, [eos])
    try:
        tokens, logits, done = _decode(m, ctx, desc, pieces, eos, dfas, guided=True, sampled=sampled)
    finally:
        for k in range(len(dfas)):
            ctx.guide_unload(k + 3)
    for k, b in enumerate(GUIDED):
        assert b in done, f"row {b} ({PATTERNS[k]}) never drew the end token"
        assert done[b] <= LONGEST[k], (b, done[b])           # within generation_length = the longest match + 1
        text = b"".join(pieces[t] for t in tokens[:done[b], b])
        assert re.fullmatch(PATTERNS[k].encode(), text), (PATTERNS[k], text)
    plain = [b for b in range(B) if b not in GUIDED]
    first_done = min(done.values())
    # the plain rows: the same tokens, and logits bit for bit, as in the batch without any guide, as long as the batch feeds the same tokens
    # (a finished guided row goes on unguided and may feed other tokens than in the unguided run; no row reads another row's tokens)
    assert (tokens[:, plain] == base_tokens[:, plain]).all()
    for step in range(STEPS):
        assert G.same_bits(logits[step], base_logits[step]), step
    assert first_done >= 1


def test_refusals(setup):
    m, ctx, desc, pieces, eos, dfas = setup
    tr, ac = dfas[0]
    L = m.lib()
    assert ctx.guide_load(0, tr, ac, [eos]) == 0
    assert ctx.guide_load(0, tr, ac, [eos], check=False) == -2                   # the slot is loaded
    assert ctx.guide_load(16, tr, ac, [eos], check=False) == -2 and ctx.guide_load(-1, tr, ac, [eos], check=False) == -2
    assert ctx.guide_load(1, tr, ac, [desc.vocab_size], check=False) == -2       # an end token outside the vocabulary
    assert ctx.guide_load(1, tr, ac, list(range(65)), check=False) == -2
    bad = tr.copy()
    bad[0, ord("y")] = len(tr)                                                   # a transition to a state >= n_states other than 255
    assert ctx.guide_load(1, bad, ac, [eos], check=False) == -2
    stuck = tr.copy()
    live = int(np.flatnonzero(ac == 0)[-1])
    stuck[live, :] = G.DEAD                                                      # a live state with neither a live byte nor acceptance
    assert ctx.guide_load(1, stuck, ac, [eos], check=False) == -2
    assert b"neither" in L.pplhip_last_error(ctx.h, 0)
    assert ctx.guide_set_vocab(pieces, check=False) == -2                        # the vocabulary is set once
    slots = np.full(B, -1, dtype=np.int32)
    states = np.zeros(B, dtype=np.int32)
    assert ctx.guide_edit(slots, states) == 0                                    # nobody asks
    slots[1] = 7
    assert ctx.guide_edit(slots, states, check=False) == -2                      # a slot that holds no guide
    slots[1], states[1] = 0, len(tr)
    assert ctx.guide_edit(slots, states, check=False) == -2                      # a state outside the guide
    states[1] = -1
    assert ctx.guide_edit(slots, states, check=False) == -2
    assert ctx.guide_unload(5, check=False) == -2                                # not loaded
    assert ctx.guide_unload(0) == 0
    assert ctx.guide_unload(0, check=False) == -2


def test_tokenizer_without_byte_fallback_refuses_a_pattern_it_cannot_spell(setup):
    m, _, desc, _, _, _ = setup
    pieces, n, eos = G.spm_vocab("spm_unigram_nofb.model")
    assert not any(p[:1] in (b"7", b"9", b"Q", b"{") for p in pieces)
    ctx = m.Context(m.copy_desc(desc), max_running_batch=4, max_tokens_per_step=16, enable_penalty=False)
    try:
        ctx.init_synthetic(0, 3)
        tr, ac = G.compile_regex("a7")
        assert ctx.guide_load(0, tr, ac, [eos], check=False) == -2               # no vocabulary yet
        assert b"vocabulary" in m.lib().pplhip_last_error(ctx.h, 0)
        ctx.guide_set_vocab(pieces[:n])
        assert ctx.guide_load(0, tr, ac, [eos], check=False) == -2               # the state behind "a" allows no token
        msg = m.lib().pplhip_last_error(ctx.h, 0)
        assert b"state 1" in msg and b"no token" in msg, msg
        tr2, ac2 = G.compile_regex("a8")                                         # the slot was freed: it takes a pattern it can spell
        assert ctx.guide_load(0, tr2, ac2, [eos]) == 0
    finally:
        ctx.close()
