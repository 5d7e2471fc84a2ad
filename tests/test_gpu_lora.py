"""The two multi-LoRA kernels on the device through pplhip_op_lora (tests/lora.py): exact cases bit for bit, random cases within the
helper's bound, rows without an adapter and every canary bit-identical to before the call."""
import faulthandler

import numpy as np
import pytest

from tests import lora as L
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = L.all_cases()
STEP_SECONDS = 120     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.cuda.synchronize()


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name for c in CASES])
def test_case(idx):
    m = load_pplhip()
    fails = L.run_case_gpu(m, CASES[idx])
    assert not fails, f"{CASES[idx].name}: " + "; ".join(fails)


def test_refusals_leave_every_canary():
    m = load_pplhip()
    c = next(c for c in CASES if c.kind == "exact" and c.T == 17 and c.rmap == "all").build()
    x = torch.from_numpy(c.xbuf.view(np.int16).copy()).to("cuda")
    y = torch.from_numpy(c.ybuf.view(np.int16).copy()).to("cuda")
    a = torch.zeros((16, c.K), dtype=torch.float16, device="cuda")
    b = torch.zeros((c.N, 16), dtype=torch.float16, device="cuda")
    wsb = m.lora_ws_bytes(c.T, 3)
    ws = torch.full((wsb // 2,), L.F16_NAN, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    A, B = [None, None, a.data_ptr()], [None, None, b.data_ptr()]

    def call(rs=c.row_slots, K=c.K, N=c.N, ranks=(0, 0, 8), wsb=wsb):
        return m.op_lora(x.data_ptr(), c.ldx, y.data_ptr(), c.ldy, c.T, N, K, rs, A, B, list(ranks), [0.0, 0.0, 1.0], ws.data_ptr(), wsb)

    assert call(K=c.K - 8) == -2 and call(N=c.N - 8) == -2
    assert call(rs=np.full(c.T, 1, dtype=np.int32)) == -2        # slot 1 is not loaded
    assert call(rs=np.full(c.T, 3, dtype=np.int32)) == -2        # slot 3 is out of range
    assert call(ranks=(0, 0, 129)) == -2
    assert call(wsb=256) == -2
    torch.cuda.synchronize()
    assert (y.cpu().numpy().view(np.uint16) == c.ybuf).all()
    assert call() == 0                                             # (a zero B: the update adds nothing)
    torch.cuda.synchronize()
    assert (y.cpu().numpy().view(np.uint16) == c.ybuf).all()
