"""The post-processor kernels (csrc/k_sample.hip) on the device through pplhip_op_penalty / pplhip_op_sample, against the references, bounds
and guards of tests/postproc.py: the count map bit for bit after every step, logits within the derived bound, tokens equal to the float64
reference, poison and canaries untouched."""
import faulthandler

import numpy as np
import pytest

from tests import postproc as P
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PENALTY = P.penalty_scenarios()
GREEDY = P.greedy_cases()
TOPK = P.topk_cases()
STEP_SECONDS = 300     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.cuda.synchronize()


@pytest.mark.parametrize("idx", range(len(PENALTY)), ids=[s.name for s in PENALTY])
def test_penalty_scenario(idx):
    m = load_pplhip()
    sc = PENALTY[idx].build()
    fails = P.run_penalty_gpu(m, torch, sc)
    assert not fails, f"{sc.name}: " + "; ".join(fails[:6])


def test_penalty_batch_zero_and_odd_vocab_write_nothing():
    m = load_pplhip()
    V, B = 1024, 4
    lg = torch.from_numpy(np.full((B + 1) * V, P.PEN_POISON, dtype=np.uint32).view(np.int32)).cuda()
    cm = torch.from_numpy(np.full((B + 1) * V, 0x5A5A, dtype=np.uint16).view(np.int16)).cuda()
    f = torch.ones(B, dtype=torch.float32, device="cuda")
    slots = torch.arange(B, dtype=torch.int64, device="cuda")
    toks = torch.zeros(B, dtype=torch.int64, device="cuda")
    seq = torch.arange(B + 1, dtype=torch.int64, device="cuda")
    sp = torch.zeros(B, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    call = lambda batch, vocab, stride: m.lib().pplhip_op_penalty(None, lg.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(),
                                                                  slots.data_ptr(), toks.data_ptr(), seq.data_ptr(), sp.data_ptr(), batch, vocab,
                                                                  stride, 0, cm.data_ptr())
    assert call(0, V, V) == 0
    assert call(0, V - 1, V) == 0                        # nothing to do comes first
    assert call(B, V - 1, V) == -2                       # PPLHIP_INVALID_VALUE: the rows of the count map would not be 4-byte aligned
    assert call(B, 1023, 1023) == -2
    assert call(B, V, V - 2) == -2                       # rows that overlap
    torch.cuda.synchronize()
    assert (lg.cpu().numpy().view(np.uint32) == P.PEN_POISON).all()
    assert (cm.cpu().numpy().view(np.uint16) == 0x5A5A).all()


@pytest.mark.parametrize("idx", range(len(GREEDY)), ids=[c.name for c in GREEDY])
def test_greedy_case(idx):
    m = load_pplhip()
    c = GREEDY[idx].build()
    fails = P.run_sample_gpu(m, torch, c)
    assert not fails, f"{c.name}: " + "; ".join(fails[:6])


@pytest.mark.parametrize("idx", range(len(TOPK)), ids=[c.name for c in TOPK])
def test_topk_topp_case(idx):
    m = load_pplhip()
    c = TOPK[idx].build()
    fails = P.run_sample_gpu(m, torch, c)
    assert not fails, f"{c.name}: " + "; ".join(fails[:6])


def test_sample_batch_zero_writes_nothing():
    m = load_pplhip()
    lg = torch.full((64,), float("inf"), dtype=torch.float32, device="cuda")
    tok = torch.from_numpy(np.full(8, P.TOK_CANARY, dtype=np.int32)).cuda()
    lp = torch.from_numpy(np.full(8, P.LP_CANARY, dtype=np.uint32).view(np.int32)).cuda()
    rnd = torch.zeros(8, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for top_k in (1, 8, 0):
        assert m.lib().pplhip_op_sample(None, lg.data_ptr(), None, None, rnd.data_ptr(), 0, 16, 16, top_k, 0.9, tok.data_ptr(), lp.data_ptr()) == 0
    assert m.lib().pplhip_op_sample(None, lg.data_ptr(), None, None, rnd.data_ptr(), 2, 16, 12, 1, 0.9, tok.data_ptr(), lp.data_ptr()) == -2
    torch.cuda.synchronize()
    assert (tok.cpu().numpy() == P.TOK_CANARY).all() and (lp.cpu().numpy().view(np.uint32) == P.LP_CANARY).all()
