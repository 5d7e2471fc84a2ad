"""Prompt logprobs on the device, operator level (pplhip_op_prompt_logprobs), against tests/prompt_logprobs.py: every position of every case --
rank exact, logprob inside tests/top_logprobs.py's derived bound, the top entries token for token, the target's logprob bit-identical to
its own top entry -- with the guards of that module; the refused arguments."""
import faulthandler

import numpy as np
import pytest

from tests import postproc as P
from tests import prompt_logprobs as PL
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = PL.all_cases()
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
    c.check_assertions()
    rc, got = PL.launch(m, torch, c)
    assert rc == 0, f"{c.name}: pplhip_op_prompt_logprobs -> {rc}"
    fails, frac = PL.check(c, got)
    if frac > WORST["frac"]:
        WORST.update(frac=frac, case=c.name)
    print(f"{c.name}: largest logprob error {frac:.3f} of the bound (so far {WORST['frac']:.3f} in {WORST['case']})")
    assert not fails, f"{c.name}: " + "; ".join(fails[:6])


def test_refused_arguments_write_nothing():
    m = load_pplhip()
    lg = torch.full((64,), float("inf"), dtype=torch.float32, device="cuda")
    out = PL.blank_outputs(2)
    dev = {k: torch.from_numpy(v.view(np.int32)).cuda() for k, v in out.items()}
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    tokens = torch.tensor([1, 2, 3], dtype=torch.int64, device="cuda")
    rows, n_ok, n_over, n_under, rows_past, rows_before = i32(0, 1), i32(0, 20), i32(0, 21), i32(-1, 0), i32(0, 2), i32(-2, 0)
    torch.cuda.synchronize()

    def call(rows=rows, n=n_ok, n_rows=2, vocab=16, stride=16, n_targets=3, lp=dev["lp"], top=dev["top_tok"]):
        return m.lib().pplhip_op_prompt_logprobs(None, lg.data_ptr(), stride, vocab, None if rows is None else rows.data_ptr(), n_rows,
                                                 tokens.data_ptr(), n_targets, None if n is None else n.data_ptr(),
                                                 None if lp is None else lp.data_ptr(), dev["rank"].data_ptr(),
                                                 None if top is None else top.data_ptr(), dev["top_lp"].data_ptr())
    assert call(n_rows=0) == 0
    assert call(stride=12) == -2 and call(vocab=0) == -2 and call(n_rows=-1) == -2
    assert call(rows=None) == -2 and call(n=None) == -2 and call(lp=None) == -2
    assert call(n=n_over) == -2 and call(n=n_under) == -2
    assert call(rows=rows_past) == -2 and call(rows=rows_before) == -2 and call(n_targets=2) == -2      # rows[j] + 1 outside the targets
    assert call(top=None) == -2                                                                           # a position asks for the ranking
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (dev[k].cpu().numpy().view(v.dtype) == v).all(), k
