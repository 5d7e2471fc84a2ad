"""Logit rules on the device, operator level (pplhip_op_logit_edit), against tests/logit_rules.py: the whole memory image of every case bit
for bit -- the edited rows, the rows with flags 0, the floats behind every row's V, in front of a misaligned base and in the canary row --
with hostile records in every table slot no asking row names; batches in which nobody asks; the refused arguments."""
import faulthandler

import numpy as np
import pytest

from tests import logit_rules as R
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = R.all_cases()
STEP_SECONDS = 300     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.cuda.synchronize()


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name for c in CASES])
def test_case(idx):
    m = load_pplhip()
    c = CASES[idx]
    rc, got = R.launch(m, torch, c)
    assert rc == 0, f"{c.name}: pplhip_op_logit_edit -> {rc}"
    fails = R.diff(c, got)
    assert not fails, f"{c.name}: " + "; ".join(fails)


@pytest.mark.parametrize("given_rows", [False, True])
def test_nobody_asks(given_rows):
    m = load_pplhip()
    src = CASES[3]
    c = R.ECase("nobody", src.logits, src.stride, src.off, src.slots, [0] * src.B, {}, src.S, given_rows=given_rows)
    rc, got = R.launch(m, torch, c)
    assert rc == 0
    assert R.same_bits(got, c.image())


def test_refused_arguments_write_nothing():
    m = load_pplhip()
    c = CASES[3]
    img = c.image()
    d = torch.from_numpy(img).cuda()
    parts = [torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda() for a in c.table()]
    fl, sl = torch.from_numpy(c.flags.view(np.int32)).cuda(), torch.from_numpy(c.slots).cuda()
    torch.cuda.synchronize()
    p = [t.data_ptr() for t in parts]

    def call(stride, vocab, batch, flags=fl.data_ptr(), slots=sl.data_ptr(), parts=p, n_rows=0):
        return m.lib().pplhip_op_logit_edit(None, d.data_ptr(), stride, vocab, batch, flags, slots, *parts, None, n_rows)
    assert call(c.stride, c.V, 0) == 0
    assert call(c.V - 1, c.V, c.B) == -2                      # rows that overlap
    assert call(c.stride, 0, c.B) == -2
    assert call(c.stride, c.V, -1) == -2
    assert call(c.stride, c.V, c.B, flags=None) == -2
    assert call(c.stride, c.V, c.B, slots=None) == -2
    for i in range(5):
        assert call(c.stride, c.V, c.B, parts=p[:i] + [None] + p[i + 1:]) == -2
    assert call(c.stride, c.V, c.B, n_rows=c.B + 1) == -2
    torch.cuda.synchronize()
    assert R.same_bits(d.cpu().numpy(), img)
