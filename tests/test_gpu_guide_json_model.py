"""pplhip_guide_load16, the product entry point for a JSON schema's automaton, in a decode loop on configs/tiny_w8a16_kv8_paged.json
(V = 1024) with the vocabulary of tests/golden/spm_bpe.model (420 pieces with byte fallback, so every JSON byte has a piece): a row
guided by a compiled schema of more than 255 states, a row guided by a regular expression (a narrow slot) and a row guided by a small
schema (a wide slot of few states) beside three plain rows, greedy and sampled.  At every step the tokens left alive in a guided row are
exactly those the numpy reference allows in the host-tracked state; every guided row ends on the end token within the longest document
+ 1 steps with a document that parses and fits its schema; the big schema's row passes through states beyond 255; the plain rows'
logits are bit for bit those of the same batch without any guide.  Then pplhip_guide_edit's state bound by the slot's own kind, a slot
reloaded with the other kind, and pplhip_guide_load16's refusals."""
import json
import os
import re

import numpy as np
import pytest

from oracle import ref
from tests import guide as G8
from tests import guide16 as G
from tests.conftest import ROOT, load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CFG = os.path.join(ROOT, "ppl.llm.serving_amd", "configs", "tiny_w8a16_kv8_paged.json")
_rng = np.random.default_rng(3)
CITIES = ["".join(chr(97 + int(c)) for c in _rng.integers(0, 26, size=8)) for _ in range(48)]
BIG = {"type": "object", "properties": {"city": {"enum": CITIES}, "n": {"type": "integer"}, "ok": {"type": "boolean"}},
       "required": ["city", "n", "ok"]}                   # the trie of 48 names: more than 300 states, a finite language
SMALL = {"type": "array", "items": {"type": "boolean"}, "maxItems": 3}
PATTERN = "[0-9]{3}-[0-9]{4}"
B = 6
GUIDED = [0, 2, 4]                                        # batch rows of BIG (wide), PATTERN (narrow), SMALL (wide); 1, 3, 5 are plain
SLOTS = [3, 4, 5]
PAGES = 20


@pytest.fixture(scope="module")
def setup():
    m = load_pplhip()
    cfg = json.load(open(CFG))
    keys = ("num_heads", "num_kv_heads", "num_layers", "hidden_dim", "intermediate_dim", "vocab_size", "cache_quant_bit", "cache_quant_group",
            "cache_layout", "cache_mode", "page_size", "weight_quant_bit", "max_position")
    desc = ref.make_desc(**{k: cfg[k] for k in keys})
    assert desc.cache_mode == 1 and desc.page_size == 4 and desc.vocab_size == 1024
    pieces, n, eos = G8.spm_vocab()
    assert n == 420 and eos == 2
    assert {p for p in pieces if len(p) == 1} == {bytes([b]) for b in range(256)}   # every byte has a piece: every live state has a token
    pieces = pieces[:n]
    big, small = G.compile_schema(BIG), G.compile_schema(SMALL)
    tr8, ac8 = G8.compile_regex(PATTERN)
    assert 300 < len(big[0]) <= 4096 and len(small[0]) < 255
    guides = [big, (G.widen(tr8), ac8), small]            # the narrow one widened: one reference and one walk for all three
    longest = [G.longest(*g) for g in guides]
    assert longest[0] is not None and longest[2] is not None and longest[1] == 8
    V = desc.vocab_size
    allowed = [G.ref_allowed(tr, ac, pieces, [eos], V) for tr, ac in guides]         # computed once, shared, left unchanged
    ctx = m.Context(m.copy_desc(desc), max_running_batch=16, max_tokens_per_step=64, enable_penalty=False)
    ctx.init_synthetic(0, 3)
    ctx.kv_alloc(0, B * PAGES * desc.page_size)
    ctx.guide_set_vocab(pieces)
    yield dict(m=m, ctx=ctx, desc=desc, pieces=pieces, eos=eos, guides=guides, narrow=(tr8, ac8), longest=longest, allowed=allowed,
               steps=max(longest) + 1)
    ctx.close()


def load_all(s):
    ctx, eos = s["ctx"], s["eos"]
    ctx.guide_load16(SLOTS[0], *s["guides"][0], [eos])
    ctx.guide_load(SLOTS[1], *s["narrow"], [eos])
    ctx.guide_load16(SLOTS[2], *s["guides"][2], [eos])


def unload_all(s):
    for g in SLOTS:
        s["ctx"].guide_unload(g)


def _decode(s, guided, sampled):
    """`steps` steps of B requests (a prefill step, then decode steps); returns (the tokens [steps, B], the plain rows' logits per step, the
    step at which each guided row drew the end token, the highest state each guided row was in)"""
    m, ctx, desc, pieces, eos = s["m"], s["ctx"], s["desc"], s["pieces"], s["eos"]
    assert (s["steps"] + 8 <= PAGES * desc.page_size)
    rng = np.random.RandomState(11)
    pages = np.arange(B * PAGES, dtype=np.int64).reshape(B, PAGES)
    prompts = [rng.randint(3, 420, size=n) for n in (5, 3, 7, 4, 6, 2)]
    lens = np.array([len(p) for p in prompts])
    slots = np.full(B, -1, dtype=np.int32)
    states = np.zeros(B, dtype=np.int32)
    if guided:
        for k, b in enumerate(GUIDED):
            slots[b] = SLOTS[k]
    tokens, plain_logits, done, top = [], [], {}, {b: 0 for b in GUIDED}
    seeds = np.arange(1, B + 1, dtype=np.uint64) * np.uint64(7919)
    last = None
    for step in range(s["steps"]):
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
        if guided:   # what a guided row may draw is exactly what the reference allows in the state the host tracks
            for k, b in enumerate(GUIDED):
                if slots[b] >= 0:
                    assert (np.isfinite(logits[b]) == s["allowed"][k][states[b]]).all(), (step, b, int(states[b]))
        if sampled:
            tok, _ = ctx.sample_rows(np.full(B, 40), np.full(B, 0.95), seeds, np.full(B, step, dtype=np.uint64), temperatures=np.full(B, 1.5))
        else:
            tok, _ = ctx.sample(B, top_k=1, req_list_changed=(step == 0))
        tok = tok.astype(np.int64)
        tokens.append(tok.copy())
        for k, b in enumerate(GUIDED):
            if slots[b] < 0:
                continue
            assert s["allowed"][k][states[b], tok[b]], (step, b, int(tok[b]))
            if tok[b] == eos:
                done[b] = step
                slots[b] = -1                                # the request has finished: its row stays in the batch, unguided, to keep the shape
            else:
                states[b] = G.walk(s["guides"][k][0], int(states[b]), pieces[tok[b]])
                assert states[b] != G.DEAD
                top[b] = max(top[b], int(states[b]))
        last = tok % 420
    return np.stack(tokens), plain_logits, done, top


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_guided_rows_fit_their_schemas_and_plain_rows_are_untouched(setup, sampled):
    s = setup
    pieces = s["pieces"]
    base_tokens, base_logits, _, _ = _decode(s, guided=False, sampled=sampled)
    load_all(s)
    try:
        tokens, logits, done, top = _decode(s, guided=True, sampled=sampled)
    finally:
        unload_all(s)
    for k, b in enumerate(GUIDED):
        assert b in done, f"row {b} never drew the end token"
        assert done[b] <= s["longest"][k], (b, done[b])      # within generation_length = the longest document + 1
    text = [b"".join(pieces[t] for t in tokens[:done[b], b]) for b in GUIDED]
    doc = json.loads(text[0].decode("utf-8"))
    assert list(doc) == ["city", "n", "ok"] and doc["city"] in CITIES and isinstance(doc["ok"], bool)
    assert isinstance(doc["n"], int) and not isinstance(doc["n"], bool)
    assert top[GUIDED[0]] >= 256, "the big schema's row never went beyond state 255"
    assert re.fullmatch(PATTERN.encode(), text[1]), text[1]
    arr = json.loads(text[2].decode("utf-8"))
    assert isinstance(arr, list) and len(arr) <= 3 and all(isinstance(x, bool) for x in arr)
    plain = [b for b in range(B) if b not in GUIDED]
    assert (tokens[:, plain] == base_tokens[:, plain]).all()
    for step in range(s["steps"]):
        assert G.same_bits(logits[step], base_logits[step]), step
    assert min(done.values()) >= 1


def test_state_bound_is_the_slots_own_and_a_slot_takes_either_kind(setup):
    s = setup
    ctx, eos, L = s["ctx"], s["eos"], s["m"].lib()
    (big_tr, big_ac), (tr8, ac8) = s["guides"][0], s["narrow"]
    assert len(big_tr) > 300 >= len(tr8)
    ctx.guide_load16(0, big_tr, big_ac, [eos])
    ctx.guide_load(1, tr8, ac8, [eos])
    slots = np.full(B, -1, dtype=np.int32)
    states = np.zeros(B, dtype=np.int32)
    try:
        for state in (256, 300, len(big_tr) - 1):
            slots[1], states[1] = 0, state
            assert ctx.guide_edit(slots, states, check=False) == 0, state            # legal in the wide slot
        states[1] = len(big_tr)
        assert ctx.guide_edit(slots, states, check=False) == -2                      # behind the wide slot's states
        for state in (256, 300):
            slots[1], states[1] = 1, state
            assert ctx.guide_edit(slots, states, check=False) == -2, state           # the same states in the narrow slot
            assert b"outside its guide" in L.pplhip_last_error(ctx.h, 0)
        states[1] = len(tr8) - 1
        assert ctx.guide_edit(slots, states, check=False) == 0
        # each slot reloaded with the other kind: the bound follows
        ctx.guide_unload(0)
        ctx.guide_unload(1)
        ctx.guide_load(0, tr8, ac8, [eos])
        ctx.guide_load16(1, big_tr, big_ac, [eos])
        slots[1], states[1] = 0, 300
        assert ctx.guide_edit(slots, states, check=False) == -2
        slots[1] = 1
        assert ctx.guide_edit(slots, states, check=False) == 0
        ctx.sync()
    finally:
        ctx.guide_unload(0)
        ctx.guide_unload(1)


def test_load16_refusals(setup):
    s = setup
    ctx, eos, desc, L = s["ctx"], s["eos"], s["desc"], s["m"].lib()
    tr, ac = s["guides"][0]
    S = len(tr)
    assert ctx.guide_load16(0, tr, ac, [eos]) == 0
    try:
        assert ctx.guide_load16(0, tr, ac, [eos], check=False) == -2                 # the slot is loaded
        assert ctx.guide_load(0, *s["narrow"], [eos], check=False) == -2             # ... for either kind
        assert ctx.guide_load16(16, tr, ac, [eos], check=False) == -2 and ctx.guide_load16(-1, tr, ac, [eos], check=False) == -2
        assert ctx.guide_load16(1, tr, ac, [desc.vocab_size], check=False) == -2     # an end token outside the vocabulary
        assert ctx.guide_load16(1, tr, ac, list(range(65)), check=False) == -2
        wide = np.full((4097, 256), 0, dtype=np.uint16)
        assert ctx.guide_load16(1, wide, np.ones(4097, dtype=np.uint8), [eos], check=False) == -2
        assert b"PPLHIP_GUIDE16_MAX_STATES" in L.pplhip_last_error(ctx.h, 0)
        bad = tr.copy()
        bad[0, ord("{")] = S                                                         # a transition to a state >= n_states other than 0xFFFF
        assert ctx.guide_load16(1, bad, ac, [eos], check=False) == -2
        assert b">= n_states" in L.pplhip_last_error(ctx.h, 0)
        bad[0, ord("{")] = 255 if S <= 255 else 0xFFFE
        assert ctx.guide_load16(1, bad, ac, [eos], check=False) == -2                # 255 is no dead state here, and 0xFFFE is none either
        stuck = tr.copy()
        live = int(np.flatnonzero(ac == 0)[-1])
        stuck[live, :] = G.DEAD                                                      # a live state with neither a live byte nor acceptance
        assert ctx.guide_load16(1, stuck, ac, [eos], check=False) == -2
        assert b"neither" in L.pplhip_last_error(ctx.h, 0)
    finally:
        ctx.guide_unload(0)
    assert ctx.guide_unload(0, check=False) == -2


def test_tokenizer_without_byte_fallback_refuses_a_schema_it_cannot_spell(setup):
    """the check after the build: a state in which no token of the vocabulary is allowed frees the slot"""
    m, desc = setup["m"], setup["desc"]
    pieces, n, eos = G8.spm_vocab("spm_unigram_nofb.model")
    assert not any(p[:1] in (b"7", b"9", b"Q", b"{") for p in pieces)
    ctx = m.Context(m.copy_desc(desc), max_running_batch=4, max_tokens_per_step=16, enable_penalty=False)
    try:
        ctx.init_synthetic(0, 3)
        tr, ac = G.compile_schema({"type": "boolean"})
        assert ctx.guide_load16(0, tr, ac, [eos], check=False) == -2             # no vocabulary yet
        assert b"vocabulary" in m.lib().pplhip_last_error(ctx.h, 0)
        ctx.guide_set_vocab(pieces[:n])
        tr7, ac7 = G.compile_schema({"const": 7})
        assert ctx.guide_load16(0, tr7, ac7, [eos], check=False) == -2           # no piece begins with "7"
        msg = m.lib().pplhip_last_error(ctx.h, 0)
        assert b"allows no token" in msg, msg
        assert ctx.guide_load16(0, tr, ac, [eos]) == 0                           # the slot was freed: it takes a schema it can spell
    finally:
        ctx.close()
