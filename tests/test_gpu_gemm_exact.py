"""Every route of launch_linear on the device, bit for bit (E3: 1 fp16 ulp) on exactly summable operands (tests/gemm_exact.py), with
canaries around the output and poison behind every input; the route a launch records equals its dry run's and the case's."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gemm_exact as G
from tests.conftest import ROOT, load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = G.all_cases()
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
    fails = G.run_case_gpu(m, CASES[idx])
    assert not fails, f"{CASES[idx].name}: " + "; ".join(fails)


# the operator entry points (64 MiB workspace, ldy = N): the same route as pplhip_op_linear_ex with those, the same outputs
OP_CASES = [c for c in CASES if c.ws == "op" and c.layout == "dense"][::7]


@pytest.mark.parametrize("idx", range(len(OP_CASES)), ids=[c.name for c in OP_CASES])
def test_operator_entry_points_take_the_same_route(idx):
    m = load_pplhip()
    c = OP_CASES[idx]
    rc, route = G.dry_route(m, c.wq, c.group, c.M, c.N, c.K, c.epi, G.OP_WS)
    assert rc == 0
    assert G.coverage_keys(route) == G.coverage_keys(c.route), (route, c.route)
    fails = G.run_case_gpu(m, c, expect_route=route, via_op=True)
    assert not fails, f"{c.name} via pplhip_op_linear: " + "; ".join(fails)


def test_m0_and_argument_errors_leave_every_canary():
    m = load_pplhip()
    y = torch.full((4096,), G.CANARY16, dtype=torch.int16, device="cuda")
    x = torch.zeros((64 * 256,), dtype=torch.float16, device="cuda")
    w = torch.zeros((256 * 256,), dtype=torch.float16, device="cuda")
    s = torch.ones((4096,), dtype=torch.float16, device="cuda")
    ws = torch.full((1 << 20,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for wq, group, M, N, K, epi, want in [(8, 128, 0, 64, 64, 0, 0), (0, 128, 0, 64, 64, 2, 0),          # M = 0: nothing to do
                                          (8, 128, 8, 6, 64, 0, -2), (0, 128, 8, 66, 64, 1, -2),         # N % 4
                                          (0, 128, 8, 64, 12, 0, -2), (8, 128, 8, 64, 24, 0, -2),        # K not allowed for the format
                                          (4, 32, 8, 64, 48, 0, -2), (4, 128, 8, 64, 192, 2, -2), (4, 48, 8, 64, 96, 0, -2)]:
        for dry in (True, False):
            rc, route = m.linear_route(x.data_ptr(), w.data_ptr(), s.data_ptr() if wq else None, wq, group, M, N, K, y.data_ptr(),
                                       G.out_width(N, epi), epi, ws=ws.data_ptr(), ws_bytes=4 << 20, dry_run=dry)
            torch.cuda.synchronize()
            assert rc == want and route == "", (wq, group, M, N, K, epi, dry, rc, route)
    assert (y.cpu().numpy() == G.CANARY16).all()


# (torch is imported before the library is loaded, as in every test module: the library then binds to the HIP runtime torch brought)
_CHILD = """
import sys
import torch
sys.path.insert(0, sys.argv[1])
from tests import gemm_exact as G
from tests.conftest import load_pplhip
m = load_pplhip()
bad = []
for row in G.SWITCH_CASES[sys.argv[2]]:
    c = G.Case(*row[:8], route=row[9], tiny=row[8])
    rc, route = G.case_dry_route(m, c)
    assert rc == 0
    if route == c.route:
        bad.append(c.name + ": the switch did not change the route " + route)
        continue
    f = G.run_case_gpu(m, c, expect_route=route)
    if f:
        bad.append(c.name + " on " + route + ": " + "; ".join(f))
    print(c.name, "->", route)
assert not bad, bad
print("OK")
"""


@pytest.mark.parametrize("switch", sorted(G.SWITCH_CASES))
def test_product_switches_in_a_child_process(switch):
    """PPLHIP_GEMV_STREAM_MAX_M=4 (W8 with K % 128 == 0 at 3-4 rows on the streaming GEMV) and PPLHIP_GEMM_PC=0 (W4 at a few hundred rows
    on the ring kernel): read once per process, so each runs in a child of its own"""
    name, value = switch.split("=")
    env = dict(os.environ, **{name: value})
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, switch], env=env, cwd=ROOT, capture_output=True, text=True, timeout=STEP_SECONDS)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
