"""CPU side of tests/gemm_exact.py (no device: the library's dry-run routes and the CPU oracle).

* every case is built under the builder's conditions and ref_linear_raw (+ ref_silu_mul for E3) reproduces its exact reference;
* the mutation table: every case differs from every mutant it is built for in at least one valid output (E3: beyond 1 fp16 ulp);
* every case takes the route it names (dry run of pplhip_op_linear_ex);
* the coverage sweep: a dense grid of shapes, workspaces and output layouts through the dry run (in a child process with no PPLHIP_*
  switch set) reaches only routes that some exact case takes, and none of the instantiations listed as unreachable.
"""
import collections
import json
import os
import re
import subprocess
import sys

import numpy as np

from oracle import ref
from tests import gemm_exact as G
from tests.conftest import ROOT, load_pplhip


def test_every_case_takes_its_route():
    m = load_pplhip()
    wrong = []
    for c in G.all_cases():
        rc, route = G.case_dry_route(m, c)
        if rc != 0 or route != c.route:
            wrong.append((c.name, rc, route, c.route))
    assert not wrong, wrong[:5]


def test_cases_exact_against_oracle_and_mutation_table():
    """the builder's conditions, the oracle bit for bit (E3: gate / up bit for bit, ref_silu_mul within the 1-ulp bar), the E2 double
    roundings per route, and the mutation table"""
    L = ref.lib()
    failures = []
    table = collections.defaultdict(lambda: [0, 0])          # mutant -> [cases built for it, cases that tell it apart]
    dr_per_key = collections.Counter()
    seen = {"subnormal": 0, "zero row": 0, "max |y| >= 2^15": 0}
    for c in G.all_cases():
        try:
            c.check_assertions()
        except AssertionError as e:
            failures.append(f"{c.name}: builder condition {e}")
            continue
        want = c.expected()
        raw = np.empty((c.M, c.N), dtype=np.float32)
        xs = np.ascontiguousarray(c.x.astype(np.float32))    # (kept alive across the call)
        L.ref_linear_raw(xs.ctypes.data, c.w.ctypes.data, None if c.scale is None else c.scale.ctypes.data, c.wq,
                         c.group, c.M, c.N, c.K, raw.ctypes.data, int(c.epi == G.EPI_F32))
        if c.epi == G.EPI_SWIGLU:
            v16 = c.values().astype(np.float16).astype(np.float32)
            if not (raw.view(np.uint32) == v16.view(np.uint32)).all():
                failures.append(f"{c.name}: oracle gate / up differ from the exact fp16 values")
            inter = c.N // 2
            gu = np.ascontiguousarray(np.concatenate([raw[:, 0::2], raw[:, 1::2]], axis=1))
            act = np.empty((c.M, inter), dtype=np.float32)
            L.ref_silu_mul(gu.ctypes.data, c.M, inter, act.ctypes.data)
            if not G.within_ulp(act, want).all():
                failures.append(f"{c.name}: ref_silu_mul outside 1 fp16 ulp of silu(g) u")
        else:
            got = raw if c.epi == G.EPI_F32 else raw.astype(np.float16)
            if G.differs(c, got, want):
                failures.append(f"{c.name}: ref_linear_raw differs from the exact reference")
            y = want.astype(np.float64)
            seen["subnormal"] += int(c.epi == G.EPI_F16 and ((y != 0) & (np.abs(y) < 2.0 ** -14)).any())
            seen["max |y| >= 2^15"] += int(c.epi == G.EPI_F16 and np.abs(y).max() >= 2.0 ** 15)
        seen["zero row"] += int((c.i == 0).all(axis=1).any())
        if c.family == "E2" and c.epi == G.EPI_F16:
            for k in G.coverage_keys(c.route):
                dr_per_key[k] += c.double_roundings()
        for name, mut in G.mutant_outputs(c).items():
            table[name][0] += 1
            if G.differs(c, mut, want):
                table[name][1] += 1
            else:
                failures.append(f"{c.name}: no valid output tells the mutant '{name}' apart")
    print("\nmutation table (cases built for the mutant / cases that tell it apart):")
    for name, (n, k) in sorted(table.items()):
        print(f"  {name:38s} {n:4d} {k:4d}")
    print("E2 outputs that two roundings and one tell apart, per fp16 route:")
    for k, v in sorted(dr_per_key.items()):
        print(f"  {v:6d}  {k}")
    print("cases with:", seen)
    low = {k: v for k, v in dr_per_key.items() if v < 8}
    assert not low, f"E2 routes with fewer than 8 double-rounding outputs: {low}"
    assert all(v > 0 for v in seen.values()), seen
    assert not failures, "\n".join(failures[:20])


_SWEEP_CHILD = """
import json, os, sys
sys.path.insert(0, sys.argv[1])
assert not [k for k in os.environ if k.startswith("PPLHIP_")], "a PPLHIP_* switch is set"
from tests.conftest import load_pplhip
from tests import gemm_exact as G
print(json.dumps(G.run_sweep(load_pplhip())))
"""


def test_coverage_sweep_reaches_only_covered_routes():
    env = {k: v for k, v in os.environ.items() if not k.startswith("PPLHIP_")}
    r = subprocess.run([sys.executable, "-c", _SWEEP_CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    reached = json.loads(r.stdout.strip().splitlines()[-1])
    cover = collections.defaultdict(list)
    for c in G.all_cases():
        for k in G.coverage_keys(c.route):
            cover[k].append(c.name)
    print(f"\ncoverage: {len(reached)} routes reached by the sweep, {len(G.all_cases())} exact cases")
    for k in sorted(reached):
        names = cover.get(k, [])
        print(f"  {k}\n      <- {', '.join(names[:3])}{' ...' if len(names) > 3 else ''}")
    missing = sorted(set(reached) - set(cover))
    assert not missing, f"routes the sweep reaches without an exact case: {missing[:10]} (first shapes: {[reached[k] for k in missing[:10]]})"
    inst = G.reached_instantiations(reached)
    opened = [(u, why) for u in sorted(inst) for p, why in G.UNREACHABLE if re.match(p, u)]
    assert not opened, f"instantiations listed as unreachable are reached now -- give them exact cases: {opened}"
    compiled = G.compiled_instantiations()
    assert inst <= compiled, inst - compiled
    unexplained = [u for u in sorted(compiled - inst) if not any(re.match(p, u) for p, _ in G.UNREACHABLE)]
    assert not unexplained, f"compiled instantiations neither reached nor listed as unreachable: {unexplained}"


def test_dry_run_refusals_match_the_launch_rules():
    """argument errors are decided by the dry run as by a launch: N % 4, K not allowed for the format, a bad epilogue; M = 0 is a no-op"""
    m = load_pplhip()
    for wq, group, M, N, K, epi in [(8, 128, 8, 6, 64, 0), (0, 128, 8, 64, 12, 0), (8, 128, 8, 64, 24, 0), (4, 32, 8, 64, 48, 0),
                                    (4, 48, 8, 64, 96, 0), (4, 128, 8, 64, 192, 0), (8, 128, 8, 64, 64, 3)]:
        rc, route = G.dry_route(m, wq, group, M, N, K, epi, G.OP_WS, ldy=64)
        assert rc == -2 and route == "", (wq, group, M, N, K, epi, rc, route)
    rc, route = G.dry_route(m, 8, 128, 0, 64, 64, 0, G.OP_WS)
    assert rc == 0 and route == ""
