"""Every kernel instantiation of launch_linear_i8 / launch_linear_f8 on the device, bit for bit (SwiGLU: 1 fp16 ulp, E3 of
tests/gemm_exact.py) on the exact operands of tests/q8_exact.py, with canaries around the output and poison behind every input; the
route a launch records equals its dry run's and names the case's kernel."""
import faulthandler

import numpy as np
import pytest

from tests import q8_exact as Q
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = Q.all_cases()
STEP_SECONDS = 300     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.cuda.synchronize()


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name for c in CASES])
def test_case_exact_and_guarded(idx):
    m = load_pplhip()
    fails = Q.run_case_gpu(m, CASES[idx])
    assert not fails, f"{CASES[idx].name}: " + "; ".join(fails)


# the operator entry points (ldy = the width): the same kernel as pplhip_op_linear_q8_ex with that stride, the same bits
OP_CASES = [c for c in CASES if c.layout == "dense" and c.M * c.N <= 1 << 20]


@pytest.mark.parametrize("idx", range(len(OP_CASES)), ids=[c.name for c in OP_CASES])
def test_operator_entry_points_give_the_same_bits(idx):
    m = load_pplhip()
    c = OP_CASES[idx].build()
    dx, dw = torch.from_numpy(c.xq.view(np.uint8)).cuda(), torch.from_numpy(c.wq.view(np.uint8)).cuda()
    dsx, dsc = torch.from_numpy(c.sx).cuda(), torch.from_numpy(c.scale.view(np.int16)).cuda()
    ys = []
    for via_op in (False, True):
        y = torch.zeros((c.M, c.width), dtype=torch.float32 if c.epi == Q.EPI_F32 else torch.float16, device="cuda")
        if via_op:
            op = m.lib().pplhip_op_linear_i8 if c.fmt == Q.FMT_I8 else m.lib().pplhip_op_linear_f8
            rc = op(None, dx.data_ptr(), dsx.data_ptr(), dw.data_ptr(), dsc.data_ptr(), c.M, c.N, c.K, y.data_ptr(), int(c.epi == Q.EPI_F32),
                    int(c.epi == Q.EPI_SWIGLU))
        else:
            rc, route = m.linear_q8_route(dx.data_ptr(), dsx.data_ptr(), dw.data_ptr(), dsc.data_ptr(), c.fmt, c.M, c.N, c.K, y.data_ptr(), c.width,
                                          c.epi, dry_run=False)
            assert Q.coverage_key(route) == c.key
        torch.cuda.synchronize()
        assert rc == 0
        ys.append(y.cpu().numpy())
    assert (ys[0].view(np.uint8) == ys[1].view(np.uint8)).all()


def test_m0_and_argument_errors_leave_every_canary():
    m = load_pplhip()
    y = torch.full((4096,), Q.CANARY16, dtype=torch.int16, device="cuda")
    x = torch.zeros((64 * 256,), dtype=torch.uint8, device="cuda")
    w = torch.zeros((256 * 256,), dtype=torch.uint8, device="cuda")
    sx = torch.ones((64,), dtype=torch.float32, device="cuda")
    s = torch.ones((4096,), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    for fmt, M, N, K, epi, ldy, want in [(8, 0, 64, 64, 0, 64, 0), (0x108, 0, 64, 64, 2, 32, 0),              # M = 0: nothing to do
                                         (8, 8, 6, 64, 0, 8, -2), (0x108, 8, 66, 64, 1, 68, -2),              # N % 4
                                         (8, 8, 64, 24, 0, 64, -2), (0x108, 8, 64, 8, 0, 64, -2),             # K % 16
                                         (8, 8, 64, 64, 0, 66, -2), (0x108, 8, 60, 64, 2, 30, -2),            # ldy % 4
                                         (8, 8, 64, 64, 3, 64, -2), (0x100, 8, 64, 64, 0, 64, -2)]:           # epilogue, format
        for dry in (True, False):
            rc, route = m.linear_q8_route(x.data_ptr(), sx.data_ptr(), w.data_ptr(), s.data_ptr(), fmt, M, N, K, y.data_ptr(), ldy, epi, dry_run=dry)
            torch.cuda.synchronize()
            assert rc == want and route == "", (fmt, M, N, K, epi, ldy, dry, rc, route)
    assert (y.cpu().numpy() == Q.CANARY16).all()
