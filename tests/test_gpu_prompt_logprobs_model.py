"""Prompt logprobs, the product path (pplhip_set_prompt_logprobs / pplhip_run / pplhip_prompt_logprobs), on one mixed step of
configs/tiny_w8a16_kv8_paged.json and of the same model over a contiguous cache, max_running_batch = 8 so that a chunk is 8 rows: decode
rows, a prompt that does not ask and asking prompts of 1 token (no position), 2, 9 (exactly one chunk), 10 and 20 tokens (three chunks)
with n in {0, 1, 20}.

Reference: the ORACLE's logits of every position -- the oracle answers the last row of a request, so prompt position j of a prompt is its
answer to the request prompt[:j + 1] (K/V are read back from the slab, so the prefix alone gives the row the whole prompt gives) -- then
log-softmax and rank in float64 (tests/prompt_logprobs.py).  Logprobs within TWICE the logit tolerance tests/test_gpu_model.py derives for
such a step, max(1e-3, NOISE_RATIO x oracle_noise) of max(1, |logit|max): |d(x_t - lse)| <= |dx_t| + |d lse| <= 2 max|dx|.  Ranks and top
tokens exactly at the positions where no other oracle logit lies within twice that tolerance of a deciding one (the target's logit for the
rank; the first n + 1 logits of the ranking for the entries); at least half of the positions qualify, which SEED was chosen for on the
oracle alone (the asking prompts are likely text under the oracle: step_tokens says why).  The step's own logits and sampled tokens are bit-identical with and without the ask."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import ref
from tests import prompt_logprobs as PL
from tests.conftest import ROOT, load_pplhip
from tests.parity import oracle_noise, record_err

CFG = os.path.join(ROOT, "ppl.llm.serving_amd", "configs", "tiny_w8a16_kv8_paged.json")
NOISE_RATIO = 2.5                                        # tests/test_gpu_model.py
SEED = 7                                                 # 23 of the 37 positions qualify on the oracle alone (seeds 0 .. 7: 15 .. 23)
FIRST = (5, 3)                                           # prompts of the two requests that are decode rows in the mixed step
PROMPTS = (6, 1, 2, 9, 10, 20)                           # lengths of the mixed step's prompts ...
ASK = np.array([5, -1, -1, 0, 1, 20, 0, 1], dtype=np.int32)   # ... behind the two decode rows: a decode row asks too (no position)
ND, B = len(FIRST), len(FIRST) + len(PROMPTS)
SLOT = 32                                                # KV tokens per request
MIN_QUALIFY = 0.5


def make_desc(mode):
    cfg = json.load(open(CFG))
    keys = ("num_heads", "num_kv_heads", "num_layers", "hidden_dim", "intermediate_dim", "vocab_size", "cache_quant_bit", "cache_quant_group",
            "cache_layout", "weight_quant_bit", "max_position")
    return ref.make_desc(cache_mode=mode, page_size=cfg["page_size"] if mode else 0, **{k: cfg[k] for k in keys})


def cache_plan(desc, n):
    """request i owns KV tokens [i * SLOT, (i + 1) * SLOT): (cache_indices, max_pages)"""
    if desc.cache_mode == 0:
        return np.arange(n, dtype=np.int64) * SLOT, 0
    mp = SLOT // desc.page_size
    return np.arange(n * mp, dtype=np.int64).reshape(n, mp), mp


RANKS = (0, 0, 1, 0, 2, 1, 4, 0, 7, 12)                  # the oracle rank a likely next token takes, drawn per position


def _last_row(rm, desc, prefix):
    """the oracle's logits behind `prefix`, a request of its own"""
    rm.kv_alloc(SLOT)
    idx, mp = cache_plan(desc, 1)
    return ref.forward([rm], ref.make_step(prefix, [0, len(prefix)], np.zeros(1, dtype=np.int64), idx, 0, mp))[0]


def step_tokens(desc, rm):
    """the mixed step's tokens.  The asking prompts are LIKELY text under the oracle, which is what scoring is used on: every fourth token
    uniformly random, the others the oracle's token of a rank drawn from RANKS behind the prompt so far.  (Uniformly random prompts cannot
    qualify at any seed: the tiny model's 1024 logits have a standard deviation of 0.32, so about seven of them lie within twice the
    tolerance, 2.6e-3 .. 3.2e-3, of a random target's -- seeds 0 .. 11 gave 0 .. 5 rank-safe positions of 37 on the oracle alone.)"""
    V = desc.vocab_size
    rng = np.random.RandomState(SEED)
    first = [rng.randint(3, V, size=n) for n in FIRST]
    new = []
    for n, a in zip(PROMPTS, ASK[ND:]):
        p = rng.randint(3, V, size=n).astype(np.int64)
        for j in range(1, n if (a >= 0 and n > 1) else 0):
            k = RANKS[rng.randint(0, len(RANKS))]
            if j % 4 != 3:
                p[j] = np.argsort(-_last_row(rm, desc, p[:j]), kind="stable")[k]
        new.append(p)
    tok = np.concatenate([rng.randint(3, V, size=ND)] + new).astype(np.int64)
    seq = np.concatenate([[0], np.cumsum([1] * ND + list(PROMPTS))])
    return first, tok, seq


def oracle_positions(desc):
    """the step's tokens, the oracle's logits of every asked position {row: [V]} and the logit tolerance of the comparison"""
    rm = ref.RefModel(desc)
    rm.init_synthetic(3)
    first, tok, seq = step_tokens(desc, rm)
    rows, _ = PL.positions(seq, ASK)
    logits, noise, top = {}, 0.0, 1.0
    for b in range(B):
        s, e = int(seq[b]), int(seq[b + 1])
        if ASK[b] < 0 or e - s < 2:
            continue
        n = e - s - 1                                    # request j of the oracle's batch is prompt[:j + 1]
        rm.kv_alloc(n * SLOT)
        idx, mp = cache_plan(desc, n)
        lens = np.arange(1, n + 1)
        st = ref.make_step(np.concatenate([tok[s:s + j + 1] for j in range(n)]), np.concatenate([[0], np.cumsum(lens)]),
                           np.zeros(n, dtype=np.int64), idx, 0, mp)
        want = ref.forward([rm], st)
        alt = oracle_noise([rm], st)
        noise = max(noise, float(np.abs(alt - want).max() / max(1.0, np.abs(want).max())))
        top = max(top, float(np.abs(want).max()))
        for j in range(n):
            logits[s + j] = want[j].astype(np.float32)
    rm.close()
    assert sorted(logits) == rows.tolist()
    rel = max(1e-3, NOISE_RATIO * noise)
    return first, tok, seq, logits, rel * top, rel, noise


def qualifying(c, tol):
    """per position (rank_safe, top_safe): no other logit within 2 tol of the target's; the first n + 1 of the ranking 2 tol apart"""
    out = []
    for r, n in zip(c.rows, c.ntop):
        x = c.logits[int(r)].astype(np.float64)
        t = int(c.tokens[r + 1])
        d = np.abs(x - x[t])
        d[t] = np.inf
        srt = np.sort(x)[::-1][:int(n) + 1]
        out.append((bool(d.min() > 2 * tol), bool(n == 0 or (srt[:-1] - srt[1:]).min() > 2 * tol)))
    return out


@pytest.fixture(scope="module", params=[1, 0], ids=["paged", "contiguous"])
def setup(request):
    desc = make_desc(request.param)
    first, tok, seq, logits, tol, rel, noise = oracle_positions(desc)
    c = PL.PCase("model", "model", desc.vocab_size, tok, seq, ASK, logits, desc.vocab_size + 4, 0)
    return desc, first, c, tol, rel, noise


def test_oracle_alone_qualifies_half_of_the_positions(setup):
    desc, first, c, tol, rel, noise = setup
    q = qualifying(c, tol)
    assert c.P == sum(n - 1 for n, a in zip(PROMPTS, ASK[ND:]) if a >= 0 and n > 1) == 37
    assert sum(a and b for a, b in q) >= MIN_QUALIFY * c.P, (sum(a and b for a, b in q), c.P, tol)


# ---- on the device ---------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(setup):
    torch = pytest.importorskip("torch")   # noqa: F841  (the conftest's device guard)
    desc, first, c, tol, rel, noise = setup
    m = load_pplhip()
    ctx = m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=64)
    ctx.init_synthetic(0, 3)
    ctx.kv_alloc(0, B * SLOT)
    idx, mp = cache_plan(desc, B)
    lens = np.array(FIRST)
    ctx.set_inputs(0, m.make_step(np.concatenate(first), np.concatenate([[0], np.cumsum(lens)]), np.zeros(ND, dtype=np.int64), idx[:ND], 0,
                                  max_pages=mp, req_list_changed=1))
    ctx.run(0)
    ctx.sync(0)
    sp = np.concatenate([lens, np.zeros(len(PROMPTS), dtype=np.int64)])
    step = lambda: m.make_step(c.tokens, c.seq, sp, idx, ND, max_pages=mp, req_list_changed=1)
    yield m, ctx, step
    ctx.close()


def _run(ctx, step, ask):
    ctx.set_inputs(0, step())
    if ask is not None:
        ctx.set_prompt_logprobs(0, ask)
    ctx.run(0)
    logits = ctx.copy_logits(B)                          # the synchronisation
    return logits, ctx.prompt_logprobs(0), ctx.sample(B, top_k=1)


@gpu
def test_mixed_step_against_the_oracle(setup, device):
    desc, first, c, tol, rel, noise = setup
    m, ctx, step = device
    logits, (rows, lp, rank, ttok, tlp), _ = _run(ctx, step, ASK)
    assert rows.tolist() == c.rows.tolist()
    ref_ = c.reference()
    q = qualifying(c, tol)
    worst = 0.0
    for j in range(c.P):
        wlp, wrank, wtok, wtlp, _, _ = ref_[j]
        n = int(c.ntop[j])
        errs = [abs(float(lp[j]) - wlp)] + ([] if not q[j][1] else [abs(float(tlp[j, e]) - float(wtlp[e])) for e in range(n)])
        worst = max(worst, max(errs))
        print(f"row {int(rows[j])} n {n}: logprob {float(lp[j]):.6f} oracle {wlp:.6f}, rank {int(rank[j])} oracle {wrank}, "
              f"safe {q[j]}, largest error {max(errs):.3g} (bound {2 * tol:.3g})")
        assert max(errs) <= 2 * tol, (int(rows[j]), errs, 2 * tol)
        if q[j][0]:
            assert int(rank[j]) == wrank, (int(rows[j]), int(rank[j]), wrank)
        if q[j][1]:
            assert ttok[j, :n].tolist() == wtok.tolist(), (int(rows[j]), ttok[j, :n], wtok)
        hit = np.flatnonzero(ttok[j, :n] == c.tokens[rows[j] + 1])
        if hit.size:                                     # the target inside its own ranking: one number
            assert lp[j].view(np.uint32) == tlp[j, hit[0]].view(np.uint32) and int(rank[j]) == int(hit[0])
    scale = 2 * tol / (2 * rel)                          # max(1, |logit|max)
    record_err(f"prompt_logprobs_model[{'paged' if desc.cache_mode else 'contiguous'}]", worst / scale, 2 * rel, noise=noise)
    # the device's numbers are its own logits' numbers: the operator on what the product's norm and lm_head give for the same rows is
    # exercised by tests/test_gpu_prompt_logprobs.py; here the greedy rank-0 positions agree with the top entry
    for j in range(c.P):
        if c.ntop[j] > 0 and rank[j] == 0:
            assert ttok[j, 0] == c.tokens[rows[j] + 1]


@gpu
def test_step_is_bit_identical_with_and_without_the_ask(setup, device):
    m, ctx, step = device
    plain, none, (tok0, lp0) = _run(ctx, step, None)
    assert none[0].size == 0
    asked, got, (tok1, lp1) = _run(ctx, step, ASK)
    assert got[0].size == 37
    assert (plain.view(np.uint32) == asked.view(np.uint32)).all()
    assert (tok0 == tok1).all() and (lp0.view(np.uint32) == lp1.view(np.uint32)).all()
    again, got2, _ = _run(ctx, step, ASK)               # and the results do not depend on what ran before
    for a, b in zip(got, got2):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()
    off, none, _ = _run(ctx, step, np.full(B, -1, dtype=np.int32))
    assert none[0].size == 0 and (off.view(np.uint32) == plain.view(np.uint32)).all()
    # the second run clears the results; one-token prompts alone ask for nothing
    _run(ctx, step, ASK)
    _, none, _ = _run(ctx, step, None)
    assert none[0].size == 0
    only_short = np.where(np.diff(setup[2].seq) == 1, 7, -1).astype(np.int32)
    _, none, _ = _run(ctx, step, only_short)
    assert none[0].size == 0


@gpu
def test_invalid_arguments_are_refused(setup, device):
    m, ctx, step = device
    ctx.set_inputs(0, step())
    call = lambda ask, batch: m.lib().pplhip_set_prompt_logprobs(ctx.h, 0, None if ask is None else ask.ctypes.data, batch)
    ok = ASK.copy()
    assert call(None, B) == -2
    assert call(ok, B - 1) == -2 and call(ok, B + 1) == -2
    for bad in (-2, 21):
        a = ok.copy()
        a[3] = bad
        assert call(a, B) == -2
    assert m.lib().pplhip_set_prompt_logprobs(None, 0, ok.ctypes.data, B) == -2
    assert m.lib().pplhip_set_prompt_logprobs(ctx.h, 1, ok.ctypes.data, B) == -2
    assert m.lib().pplhip_prompt_logprobs(ctx.h, 0, None) == -2
    ctx.run(0)                                           # a refused ask is no ask
    ctx.sync(0)
    assert ctx.prompt_logprobs(0)[0].size == 0


@gpu
def test_tensor_parallel_context_refuses(setup):
    desc = setup[0]
    m = load_pplhip()
    tp = m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=64, n_local_ranks=2, device_ids=[0, 0])   # world_size 2
    try:
        for rank in (0, 1):
            assert m.lib().pplhip_set_prompt_logprobs(tp.h, rank, ASK.ctypes.data, B) == -7            # PPLHIP_UNSUPPORTED
            assert b"tensor parallelism" in m.lib().pplhip_last_error(tp.h, rank)
        assert m.lib().pplhip_set_prompt_logprobs(tp.h, 0, None, B) == -7                              # in front of every other check
    finally:
        tp.close()
