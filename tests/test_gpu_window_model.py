"""Sliding-window attention inside the step (pplhip_sliding_window): a tiny paged W8A16 / int8-KV model with head_dim 128.  A window no
request reaches changes no bit; a window of 24 leaves every step up to 24 tokens bit-identical and moves the logits from the first step
that passes it, in a prefill and in decode steps; keys poisoned below every row's window change no bit and a poisoned first key inside it
does; shared-prefix detection and the window refuse each other."""
import numpy as np
import pytest

from oracle import ref
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def make_ctx(m):
    desc = ref.make_desc(hidden_dim=256, intermediate_dim=512, num_layers=2, num_heads=2, num_kv_heads=2, vocab_size=1024, max_position=512,
                         cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=1, page_size=16, weight_quant_bit=8,
                         weight_quant_group=128)
    ctx = m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=256)
    ctx.init_synthetic(0, 1234)
    ctx.kv_alloc(0, 1024)
    return ctx


def poison(ctx, pages, positions):
    """V of the given (request, key position) pairs, every layer and head, becomes 127 x scale 1 (ordinary values stay below 4): a row that
    reads such a key with any weight moves its logits; K stays, so the scores stay plausible"""
    N, D = ctx.kv_tokens, 128
    cache, scale = ctx.kv_read(0, 0).reshape(2, 2, 2, N, D), ctx.kv_read(0, 1).reshape(2, 2, 2, N, D // 8)   # layout 3: [layer, k / v, head, slot, .]
    for b, p in positions:
        slot = pages[b, p // 16] * 16 + p % 16
        cache[:, 1, :, slot], scale[:, 1, :, slot] = 127, 1.0
    ctx.kv_write(0, 0, cache)
    ctx.kv_write(0, 1, scale)


def run_trace(m, window, prompts, steps, poison_outside=None, poison_edge=None):
    """prefill of the prompts, then greedy decode steps; the logits of every step.  poison_outside = W: in front of every decode step all
    keys below each row's window of W are poisoned; poison_edge = (W, step): in front of that step each row's first key inside it"""
    ctx = make_ctx(m)
    if window is not None:
        ctx.sliding_window(window)
    B = len(prompts)
    pages = (np.arange(B * 8, dtype=np.int64).reshape(B, 8) * 7) % (B * 8)   # every request 8 pages of its own, out of order
    lens = np.array([len(p) for p in prompts])
    tok, seq, sp, out = np.concatenate(prompts).astype(np.int64), np.concatenate([[0], np.cumsum(lens)]), np.zeros(B, dtype=np.int64), []
    for s in range(steps + 1):
        if s > 0 and poison_outside:
            poison(ctx, pages, [(b, p) for b in range(B) for p in range(max(0, sp[b] - poison_outside + 1))])
        if poison_edge and s == poison_edge[1]:
            poison(ctx, pages, [(b, sp[b] - poison_edge[0] + 1) for b in range(B)])
        ctx.set_inputs(0, m.make_step(tok, seq, sp, pages, 0 if s == 0 else B, 8, req_list_changed=int(s < 2)))
        ctx.run(0, cache_prefill=0)
        out.append(ctx.copy_logits(B).copy())
        tok, sp, seq = out[-1].argmax(axis=1).astype(np.int64), sp + (seq[1:] - seq[:-1]), np.arange(B + 1)
    ctx.close()
    return out


def test_window_beyond_every_request_changes_no_bit():
    m, rng = load_pplhip(), np.random.RandomState(5)
    prompts = [rng.randint(3, 1024, size=n) for n in (9, 30)]
    a, b = run_trace(m, 64, prompts, 6), run_trace(m, None, prompts, 6)
    assert all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(a, b))


def test_window_binds_in_prefill_and_decode():
    m, rng = load_pplhip(), np.random.RandomState(6)
    prompts = [rng.randint(3, 1024, size=n) for n in (50, 10)]   # request 0 passes W = 24 in its prefill, request 1 in decode step 15
    a, b = run_trace(m, 24, prompts, 40), run_trace(m, None, prompts, 40)
    same = [[(x[r].view(np.uint32) == y[r].view(np.uint32)).all() for x, y in zip(a, b)] for r in range(2)]
    assert not same[0][0] and not any(same[0])            # its last prompt row already attends 24 of 50 keys
    # request 1: kv lengths 10 .. 24 fit the window (same keys; the decode split may differ, so close rather than equal), the step at
    # position 24 is the first past it
    assert all(np.abs(x[1] - y[1]).max() <= 2e-3 * np.abs(y[1]).max() for x, y in zip(a[:15], b[:15])) and not same[1][15]
    assert all(np.isfinite(x).all() for x in a)
    assert any((x[0].argmax() != y[0].argmax()) for x, y in zip(a, b))   # the greedy tokens part from the unwindowed run's


def test_context_reads_each_rows_window_and_nothing_else():
    """What the context path itself reads (window_plan's shifted table, the chunk's offsets into it, the skips): with W = 24, prompts of 50
    and 10 tokens and 40 decode steps, every key BELOW a row's window is poisoned in front of every decode step -- no bit of any step may
    move (a table one page early, a skip one short, another row's table would read poison) --, and, in a second run, each row's FIRST
    key inside its window in front of step 20 -- both rows' logits must move (a window one key short would not read it).  The arithmetic
    on the keys in between is pplhip_op_attention_window's, held to float64 by tests/test_gpu_attn_window.py.  (The unwindowed context
    does read the poisoned keys: the poison is seen.)"""
    m, rng = load_pplhip(), np.random.RandomState(6)
    prompts = [rng.randint(3, 1024, size=n) for n in (50, 10)]
    clean, outside = run_trace(m, 24, prompts, 40), run_trace(m, 24, prompts, 40, poison_outside=24)
    assert all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(clean, outside))
    edge = run_trace(m, 24, prompts, 20, poison_edge=(24, 20))
    assert all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(clean[:20], edge[:20]))
    assert all((edge[20][r].view(np.uint32) != clean[20][r].view(np.uint32)).any() for r in range(2))
    plain, seen = run_trace(m, None, prompts, 2), run_trace(m, None, prompts, 2, poison_outside=24)
    assert (seen[1][0].view(np.uint32) != plain[1][0].view(np.uint32)).any()


def test_window_and_shared_prefix_refuse_each_other():
    m = load_pplhip()
    ctx = make_ctx(m)
    ctx.shared_prefix(2, 16)
    assert m.lib().pplhip_sliding_window(ctx.h, 24) == -7
    ctx.shared_prefix(0, 0)
    ctx.sliding_window(24)
    assert m.lib().pplhip_shared_prefix(ctx.h, 2, 16) == -7
    ctx.close()
