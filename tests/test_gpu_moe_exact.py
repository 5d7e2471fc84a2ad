"""The mixture-of-experts block on the device, bit for bit on exactly summable operands (tests/moe_exact.py: the cases, what each is for, and
the reference): the router alone, the whole block twice on a NaN workspace with canaries around y and poison behind every input, the
bucket kernel's promises read back from the workspace (y does not depend on the placement, so stability shows only there), stale workspace
state across calls of different sizes, and two calls back to back on one stream.  No tolerance in this file."""
import faulthandler

import numpy as np
import pytest

from tests import moe_exact as X
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = X.all_cases()
IDS = [c.name for c in CASES]
STEP_SECONDS = 120     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.cuda.synchronize()


def _ws_bytes(L, c):
    n = L.pplhip_op_moe_ffn_workspace_bytes(c.T, c.E, c.k, c.hidden, c.inter)
    assert n == X.layout(c.T, c.E, c.k, c.hidden, c.inter)["bytes"], "moe_exact.layout no longer mirrors moe_layout"
    return n


def test_tile_heights_are_the_formula():
    L = load_pplhip().lib()
    rows = [L.pplhip_op_moe_tile_rows(T, 2, 8) for T in range(1, 2049)]
    assert rows == sorted(rows) and rows.index(128) == X.threshold_T(8, 2)     # rows[i] belongs to T = i + 1: lo = index, hi = lo + 1
    for c in CASES:
        c.build()
        assert L.pplhip_op_moe_tile_rows(c.T, c.k, c.E) == X.tile_rows(c.T, c.k, c.E) == c.claim["tile"], c.name


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_route_exact(idx):
    fails = X.run_route_gpu(load_pplhip(), torch, CASES[idx])
    assert not fails, f"{CASES[idx].name}: " + "; ".join(fails)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_ffn_exact_and_guarded(idx):
    L = load_pplhip().lib()
    d = X.DeviceCase(torch, CASES[idx])
    n = _ws_bytes(L, d.c)
    ws = X.nan_workspace(torch, n)
    torch.cuda.synchronize()
    assert d.launch(L, ws.data_ptr(), n) == 0
    torch.cuda.synchronize()
    first, _ = d.y_bits()
    fails = d.check(ws=ws)
    assert not fails, f"{d.c.name}: " + "; ".join(fails)
    d.fresh_y()                                   # the same call on the workspace as it was left
    assert d.launch(L, ws.data_ptr(), n) == 0
    torch.cuda.synchronize()
    again, _ = d.y_bits()
    fails = d.check(ws=ws)
    assert not fails, f"{d.c.name}, second call: " + "; ".join(fails)
    assert (again == first).all()


SEQUENCES = [["three_pass_k8", "one_token", "k1"], ["k1", "one_token", "three_pass_k8"], ["spread", "one_expert", "one_token", "exact_tall"]]


@pytest.mark.parametrize("wq", [0, 8])
@pytest.mark.parametrize("seq", SEQUENCES, ids=["-".join(s) for s in SEQUENCES])
def test_stale_workspace_state(seq, wq):
    """a prefill-sized call, then decode-sized ones (and the reverse) on ONE workspace allocation that is NaN only before the first call"""
    L = load_pplhip().lib()
    runs = [X.DeviceCase(torch, X.by_name(f"{n}-w{wq}")) for n in seq]
    n = max(_ws_bytes(L, d.c) for d in runs)
    ws = X.nan_workspace(torch, n)
    at = ws.data_ptr()
    torch.cuda.synchronize()
    for d in runs:
        assert ws.data_ptr() == at
        assert d.launch(L, at, n) == 0
        torch.cuda.synchronize()
        fails = d.check(ws=ws)
        assert not fails, f"{d.c.name} after {[r.c.name for r in runs[:runs.index(d)]]}: " + "; ".join(fails)


@pytest.mark.parametrize("wq", [0, 8])
def test_two_calls_back_to_back_on_one_stream(wq):
    """nothing in the block relies on a host-side wait: two different cases on a non-default stream, one synchronise at the end"""
    L = load_pplhip().lib()
    runs = [X.DeviceCase(torch, X.by_name(f"{n}-w{wq}")) for n in ("two_pass", "exact_short")]
    wss = [X.nan_workspace(torch, _ws_bytes(L, d.c)) for d in runs]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()                      # the operands and the NaN fill are on the device
    for d, ws in zip(runs, wss):
        assert d.launch(L, ws.data_ptr(), d.ws_bytes, stream=stream.cuda_stream) == 0
    stream.synchronize()
    for d, ws in zip(runs, wss):
        fails = d.check(ws=ws)
        assert not fails, f"{d.c.name}: " + "; ".join(fails)
