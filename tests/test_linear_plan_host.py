"""The launch plan of the weight-only linear layers on the host (tests/host/linear_plan_trace.cc: csrc/linear_plan.cc built with the host
compiler alone, no HIP, no device).

* every plan of the sweep grid of tests/gemm_exact.py keeps the conditions the kernels rely on -- the grid covers every tile exactly once,
  no empty K split, W4 scale groups within the block's LDS area, slabs within the workspace, deferred slabs only where a consumer can take
  them, dynamic LDS by the family's formula and within a CU, block sizes equal to the launch bounds, M-split parts disjoint and complete
  (the program checks them and exits non-zero, naming the line);
* the program's route text equals the library's dry-run route for every exact case and for 2000 fixed pseudo-random grid points;
* the quantised-activation linears (plan_linear_q8, `linear_plan_trace q8`): every plan of the sweep grid of tests/q8_exact.py keeps the
  conditions of the comment block at the top of k_gemm_i8.hip -- the grid covers n_tiles x m_tiles exactly once after the round-up to the 8
  XCDs, dynamic LDS = stages x stage size within a CU, tile kernels only for M > 32 and K % 128 == 0, 256 x 256 blocks only for int8, 128 x
  384 blocks only where linear_w8_wide_waves(M, N) == 12 -- and its route text equals the library's dry run.
"""
import os
import random
import subprocess

import pytest

from tests import gemm_exact as G
from tests import q8_exact as Q
from tests.conftest import ROOT, load_pplhip

BIN = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "linear_plan_trace")
Y_ADDR = 1 << 20


def _line(wq, group, M, N, K, epi, ws_bytes, ldy, y_addr=Y_ADDR, defer=0):
    return f"{wq} {group} {M} {N} {K} {epi} {ws_bytes} {defer} {ldy} {y_addr}"


def _grid():
    """(wq, group, M, N, K, epi, workspace name) of SWEEP_M x SWEEP_N x SWEEP_K x SWEEP_WQ x the three epilogues, workspaces op / none"""
    return [(wq, group, M, N, K, epi, wsn)
            for wq, group in G.SWEEP_WQ for K in G.SWEEP_K for N in G.SWEEP_N for epi in (G.EPI_F16, G.EPI_F32, G.EPI_SWIGLU)
            for M in G.SWEEP_M for wsn in ("op", "none")]


def _grid_line(pt):
    wq, group, M, N, K, epi, wsn = pt
    return _line(wq, group, M, N, K, epi, G.WS_SIZES[wsn], G.out_width(N, epi))


def _trace(lines, env, mode=()):
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} is missing: build it with __graft_entry__.build()")
    out = subprocess.run([BIN, *mode], input="\n".join(lines) + "\n", env=env, capture_output=True, text=True, timeout=600)
    rows = [ln.split("\t") for ln in out.stdout.split("\n") if ln]
    return out, rows


def test_every_plan_of_the_grid_keeps_the_invariants():
    env = {k: v for k, v in os.environ.items() if not k.startswith("PPLHIP_")}
    grid = _grid()
    out, rows = _trace([_grid_line(pt) for pt in grid], env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len(rows) == len(grid)
    assert all(r[0] in ("0", "-2") and (r[0] == "0") == bool(r[1]) for r in rows)
    planned = sum(r[0] == "0" for r in rows)
    print(f"\n{len(grid)} problems, {planned} planned, {len(grid) - planned} refused")
    assert planned > len(grid) // 2


def test_routes_equal_the_library_dry_run():
    m = load_pplhip()
    probs = [(c.wq, c.group, c.M, c.N, c.K, c.epi, G.WS_SIZES[c.ws], c.ldy, Y_ADDR + c.y_off_bytes) for c in G.all_cases()]
    rnd = random.Random(20261020)
    probs += [(wq, group, M, N, K, epi, G.WS_SIZES[wsn], G.out_width(N, epi), Y_ADDR) for wq, group, M, N, K, epi, wsn in rnd.sample(_grid(), 2000)]
    out, rows = _trace([_line(*p) for p in probs], dict(os.environ))
    assert out.returncode == 0, out.stderr[-2000:]
    assert len(rows) == len(probs)
    wrong = []
    for (wq, group, M, N, K, epi, ws_bytes, ldy, ya), r in zip(probs, rows):
        rc, route = G.dry_route(m, wq, group, M, N, K, epi, ws_bytes, ldy=ldy, y_addr=ya)
        if (str(rc), route) != (r[0], r[1]):
            wrong.append(((wq, group, M, N, K, epi, ws_bytes, ldy, ya), (rc, route), r[:2]))
    assert not wrong, wrong[:5]


def _q8_grid():
    """(fmt, M, N, K, epi, ldy) of the q8 sweep: both formats, the three epilogues, ldy = width and width + 4, plus every exact case"""
    grid = [(fmt, M, N, K, epi, G.out_width(N, epi) + pad)
            for fmt in (Q.FMT_I8, Q.FMT_F8) for epi in (G.EPI_F16, G.EPI_F32, G.EPI_SWIGLU) for pad in (0, 4)
            for K in Q.SWEEP_K for N in Q.SWEEP_N for M in Q.SWEEP_M]
    return grid + [(c.fmt, c.M, c.N, c.K, c.epi, c.ldy) for c in Q.all_cases()]


def test_q8_plans_keep_the_invariants_and_equal_the_library_dry_run():
    m = load_pplhip()
    env = {k: v for k, v in os.environ.items() if not k.startswith("PPLHIP_")}
    grid = _q8_grid()
    out, rows = _trace([" ".join(str(v) for v in pt) for pt in grid], env, mode=("q8",))
    assert out.returncode == 0, out.stderr[-2000:]
    assert len(rows) == len(grid)
    wrong = []
    families = set()
    for (fmt, M, N, K, epi, ldy), r in zip(grid, rows):
        rc, route = Q.dry_route(m, fmt, M, N, K, epi, ldy=ldy)
        if (str(rc), route) != (r[0], r[1]):
            wrong.append(((fmt, M, N, K, epi, ldy), (rc, route), r[:2]))
        if r[0] == "0":
            families.add(r[2].split()[0])
    assert not wrong, wrong[:5]
    planned = sum(r[0] == "0" for r in rows)
    print(f"\n{len(grid)} problems, {planned} planned, {len(grid) - planned} refused; families {sorted(families)}")
    assert families == {"family=gemv", "family=pc", "family=wide", "family=256"} and planned > len(grid) // 2


def test_q8_trace_refuses_a_malformed_line():
    """a line that is not 'act_fmt M N K epi ldy' ends the program with status 2"""
    out, rows = _trace(["8 33 132"], dict(os.environ), mode=("q8",))
    assert out.returncode == 2 and "expected" in out.stderr
