"""Top-N logprobs on the device, operator level (pplhip_op_top_logprobs), against tests/top_logprobs.py: every entry of every asked row --
token bit for bit, logprob inside the derived bound -- with the guards of that module; entry 0 against the greedy kernel on the same row;
the batches in which nobody asks; the refused arguments."""
import faulthandler

import numpy as np
import pytest

from tests import postproc as P
from tests import top_logprobs as T
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = T.grid_cases()
NONE = T.none_cases()
STEP_SECONDS = 300     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run
WORST = {"frac": 0.0, "case": None}


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.cuda.synchronize()


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name for c in CASES])
def test_case(idx):
    m = load_pplhip()
    c = CASES[idx].build()
    ref = c.check_assertions()
    rc, tok, lp = T.launch(m, torch, c)
    assert rc == 0, f"{c.name}: pplhip_op_top_logprobs -> {rc}"
    fails, frac = T.check(c, tok, lp)
    if frac > WORST["frac"]:
        WORST.update(frac=frac, case=c.name)
    print(f"{c.name}: largest logprob error {frac:.3f} of the bound (so far {WORST['frac']:.3f} in {WORST['case']})")
    assert not fails, f"{c.name}: " + "; ".join(fails[:6])
    # entry 0 is the greedy kernel's answer on the same row: token exact, logprob within the two bounds added
    g_tok, g_lp = T.launch_greedy(m, torch, c)
    lpf = lp.view(np.float32)
    for j, b in enumerate(c.asked):
        _, wlp, log_s, lse = ref[j]
        assert int(tok[j, 0]) == int(g_tok[b]), f"{c.name}: row {b} entry 0 token {int(tok[j, 0])}, greedy {int(g_tok[b])}"
        both = T.entry_bound(c.V, log_s, lse, wlp[0]) + T.greedy_bound(c.V, log_s, lse, wlp[0])
        assert abs(float(lpf[j, 0]) - float(g_lp[b])) <= both, f"{c.name}: row {b} entry 0 logprob {lpf[j, 0]!r}, greedy {g_lp[b]!r}, bound {both:.3g}"


@pytest.mark.parametrize("idx", range(len(NONE)), ids=[c.name for c in NONE])
def test_nobody_asks(idx):
    m = load_pplhip()
    c = NONE[idx].build()
    c.check_assertions()
    assert not c.asked
    rc, tok, lp = T.launch(m, torch, c)
    assert rc == 0
    assert (tok == P.TOK_CANARY).all() and (lp == P.LP_CANARY).all()


def test_refused_arguments_write_nothing():
    m = load_pplhip()
    lg = torch.full((64,), float("inf"), dtype=torch.float32, device="cuda")
    tok0, lp0 = T.blank_outputs(2)
    tok, lp = torch.from_numpy(tok0).cuda(), torch.from_numpy(lp0.view(np.int32)).cuda()
    n = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    ok, over, under = n(1, 20), n(1, 21), n(-1, 1)
    torch.cuda.synchronize()
    call = lambda nlp, batch, vocab, stride: m.lib().pplhip_op_top_logprobs(None, lg.data_ptr(), None, nlp, batch, vocab, stride, tok.data_ptr(),
                                                                            lp.data_ptr())
    assert call(ok.data_ptr(), 0, 16, 16) == 0
    assert call(ok.data_ptr(), 2, 16, 12) == -2                       # rows that overlap
    assert call(ok.data_ptr(), 2, 0, 16) == -2
    assert call(None, 2, 16, 16) == -2
    assert call(over.data_ptr(), 2, 16, 16) == -2
    assert call(under.data_ptr(), 2, 16, 16) == -2
    torch.cuda.synchronize()
    assert (tok.cpu().numpy() == P.TOK_CANARY).all() and (lp.cpu().numpy().view(np.uint32) == P.LP_CANARY).all()
