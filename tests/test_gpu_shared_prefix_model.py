"""Shared-prefix decode attention inside the step: six requests behind one cached prefix, the logits of every step against the oracle
exactly as tests/test_gpu_model.py holds the tiny paged W8A16 / int8-KV model (test_synthetic_model: the geometry of
configs/tiny_w8a16_kv8_paged.json at 16-token pages -- the kernel's sub-tile is 16 keys), with the feature on and off, on one lane and
as a two-lane step, whose halves each see the part of the group that lies inside them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref
from tests.conftest import load_pplhip
from tests.test_gpu_model import check_steps
from tests.parity import oracle_noise

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
I64MAX = np.iinfo(np.int64).max


def run_trace(enabled, want_info, name):
    m = load_pplhip()
    desc = ref.make_desc(hidden_dim=256, intermediate_dim=512, num_layers=2, num_heads=4, num_kv_heads=4, vocab_size=1024, max_position=512,
                         cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=1, page_size=16, weight_quant_bit=8,
                         weight_quant_group=128)
    rm = ref.RefModel(desc)
    rm.init_synthetic(1234)
    rm.kv_alloc(1024)
    ctx = m.Context(m.copy_desc(desc), max_running_batch=16, max_tokens_per_step=256)
    ctx.init_synthetic(0, 1234)
    ctx.kv_alloc(0, 1024)
    if enabled:
        ctx.shared_prefix(2, 16)
    rng = np.random.RandomState(11)
    first = rng.randint(3, 1024, size=40)                                  # request 0: pages 0, 1 full, 2 begun
    tails = [rng.randint(3, 1024, size=n) for n in (1, 5, 14, 17, 20)]     # five more behind its first 32 tokens
    all_pages = np.array([[0, 1, 2, 3]] + [[0, 1, 4 + 2 * i, 5 + 2 * i] for i in range(5)], dtype=np.int64)
    res, infos, last = [], [], [None]

    def step(tok, seq_starts, start_pos, rows, dec):
        # a row's table holds the pages it has reached; the list counts as changed when a row takes a new page or turns into a decode row
        end = np.asarray(start_pos) + np.diff(seq_starts)
        pages = np.where(np.arange(4)[None, :] * 16 < end[:, None], all_pages[rows], I64MAX)
        changed = int(last[0] is None or last[0][1] != dec or last[0][0].shape != pages.shape or (last[0][0] != pages).any())
        last[0] = (pages, dec)
        st_r = ref.make_step(tok, seq_starts, start_pos, pages, dec, 4)
        want, alt = ref.forward([rm], st_r), oracle_noise([rm], st_r)
        ctx.set_inputs(0, m.make_step(tok, seq_starts, start_pos, pages, dec, 4, req_list_changed=changed))
        ctx.run(0, cache_prefill=1)
        gtok, glp = ctx.sample(len(rows), top_k=1)
        wtok, wlp = ref.sample(want, top_k=1)
        res.append((ctx.copy_logits(len(rows)), want, gtok, wtok, glp, wlp, alt))
        infos.append((ctx.shared_prefix_info(0), changed))
        return wtok.astype(np.int64)

    nxt = step(first, [0, 40], [0], [0], 0)
    # request 0 decodes; the five arrive as cache-prefill rows on its two full pages, the way a prefix hit arrives
    lens = np.array([1] + [len(t) for t in tails])
    nxt = step(np.concatenate([nxt] + tails), np.concatenate([[0], np.cumsum(lens)]), [40] + [32] * 5, list(range(6)), 1)
    start_pos = np.array([41] + [32 + len(t) for t in tails])
    for s in range(4):
        nxt = step(nxt, np.arange(7), start_pos + s, list(range(6)), 6)
    assert [i for i, _ in infos[:2]] == [(0, 0, 0)] * 2                    # one decode row: no group
    assert [i for i, _ in infos[2:]] == [want_info if enabled else (0, 0, 0)] * 4
    assert [ch for _, ch in infos[2:]] == [1, 0, 1, 0]                     # the row at position 47 takes page 3 in the third decode step
    check_steps(res, k=1, name=name)
    ctx.close()


@pytest.mark.parametrize("enabled", [True, False])
def test_shared_prefix_decode_steps(enabled):
    run_trace(enabled, (1, 6, 32), f"shared_prefix_model_{int(enabled)}")


def test_shared_prefix_two_lane_step():
    """PPLHIP_DUAL_STREAM=1 (read at context creation: a child process): the six decode rows run as two halves of three on two streams,
    and the group, cut by the halves, counts as two groups of three rows"""
    code = ("from tests.test_gpu_shared_prefix_model import run_trace\n"
            "run_trace(True, (2, 6, 64), 'shared_prefix_model_two_lanes')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PPLHIP_DUAL_STREAM="1", PPLHIP_DUAL_MIN_ROWS="4", PPLHIP_VERBOSE="1"),
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "two-stream decode (rows 3 + 3)" in r.stderr, r.stderr[-2000:]   # the path under test did run
