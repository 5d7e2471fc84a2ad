"""CPU side of tests/q8_exact.py (no device: the library's dry-run routes and the numpy reference).

* the reference reproduces a 3 x 4 x 16 problem worked out by hand, for both formats and the SwiGLU epilogue;
* every case is built under the builder's conditions (tests/q8_exact.py: normal fp16 outputs, the order / single-rounding / fp32-sum /
  e5m2 shares, the fp8 bands' code coverage) and takes the kernel it names;
* the coverage sweep: the dispatch thresholds of launch_linear_q8 +-1 through the dry run (in a child process with no PPLHIP_* switch
  set).  Every kernel instantiation it reaches has an exact case and every case's kernel is reached; the set of reached instantiations
  is pinned below, so a change of the dispatch is a visible diff.  Not reachable at the default switches, and therefore without a
  case: gemm_i8_pc_kernel<E,3,*> and gemm_i8_256_kernel<E,3> (the ring depths a tuning build's PPLHIP_GEMM_I8_PC=3 /
  PPLHIP_GEMM_I8_256_ST=3 select) -- q8_exact.UNREACHABLE.
"""
import collections
import json
import math
import os
import re
import subprocess
import sys

import numpy as np

from tests import q8_exact as Q
from tests.conftest import ROOT, load_pplhip

# the kernel instantiations launch_linear_i8 / launch_linear_f8 reach at the default switches
REACHED = sorted(
    [f"gemv_i8_kernel<{a},{e},{f}>" for a in ("1", "2") for e in ("f16,4", "f32,4", "swiglu,4") for f in ("i8", "f8")]
    + [f"gemv_i8_kernel<1,{e},8,{f}>" for e in ("f16", "f32", "swiglu") for f in ("i8", "f8")]
    + [f"gemm_i8_pc_kernel<{e},{st},{f}>" for e in ("f16", "f32", "swiglu") for st in (2, 4) for f in ("i8", "f8")]
    + [f"gemm_i8_wide_kernel<{e},{f}>" for e in ("f16", "f32", "swiglu") for f in ("i8", "f8")]
    + [f"gemm_i8_256_kernel<{e},4>" for e in ("f16", "f32", "swiglu")])


def test_reference_by_hand_int8():
    """3 x 4 x 16: sums, both fp32 multiplies and the fp16 rounding worked out by hand"""
    alt = np.array([127, -127] * 8)
    x = np.array([[1] * 16, list(range(1, 17)), alt])
    w = np.array([[2] * 16, [-128] * 16, [1] + [0] * 15, alt])
    assert (Q.exact_sums(x, w) == [[32, -2048, 1, 0], [272, -17408, 1, -1016], [0, 0, 127, 258064]]).all()
    sx = np.array([0.5, 0.75, 1.5], dtype=np.float32)
    scale = np.array([0.5, 0.25, 1.5, 0.125], dtype=np.float16)
    v = Q.ref_i8(x.astype(np.int8), sx, w.astype(np.int8), scale)
    assert v.dtype == np.float32
    assert (v == [[8, -256, 0.75, 0], [102, -3264, 1.125, -95.25], [0, 0, 285.75, 48387]]).all()
    h = Q.finish(v, Q.EPI_F16)
    assert h.dtype == np.float16 and h[2, 3] == 48384 and (h.astype(np.float32)[:2] == v[:2]).all()    # 48387 -> the fp16 grid of 32
    assert Q.finish(v, Q.EPI_F32) is v
    y = Q.finish(v, Q.EPI_SWIGLU)
    assert y.shape == (3, 2) and y[2, 0] == 0 and y[0, 1] == 0
    assert math.isclose(y[0, 0], 8 / (1 + math.exp(-8)) * -256, rel_tol=1e-15) and math.isclose(y[2, 1], 285.75 / (1 + math.exp(-285.75)) * 48384)
    # fp32(S) is round-to-nearest-even, the order of the multiplies is (S sx) scale, and the fp16 rounding follows two fp32 ones
    assert (np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 25 + 6)], dtype=np.int64).astype(np.float32) == [2 ** 24, 2 ** 24 + 4, -(2 ** 25 + 8)]).all()
    one = Q.ref_i8(np.array([[3] + [0] * 15], dtype=np.int8), np.array([1 / 3], dtype=np.float32), np.array([[1] + [0] * 15], dtype=np.int8),
                   np.array([7], dtype=np.float16))
    # fp32(1/3) = 11184811 2^-25: 3 fp32(1/3) = 1 + 2^-25 rounds to 1, then 1 * 7 = 7; the other order gives fl(7 fp32(1/3)) * 3 = 7 + 2^-21
    assert one[0, 0] == 7.0 and np.float32(3) * np.float32(np.float32(1 / 3) * np.float32(7)) == np.float32(7.000000476837158)


def test_reference_by_hand_fp8():
    """3 x 4 x 16 of e4m3 codes: 1.0, the smallest subnormal 2^-9, +-448, 2^-6 -- sums and power-of-two scales by hand"""
    z = [0] * 15
    x = np.array([[0x38] * 16, [0x01] * 16, [0x7E] + z], dtype=np.uint8)
    w = np.array([[0x40] * 16, [0xB8] * 16, [0x7E] + z, [0x08] * 16], dtype=np.uint8)
    v = Q.ref_f8(x, np.array([0, 3, -4]), w, np.array([1, 0, -2, 2]))
    assert v.dtype == np.float32
    assert (v == [[64, -16, 112, 1], [1, -0.25, 1.75, 2.0 ** -6], [112, -28, 3136, 1.75]]).all()
    assert (Q.finish(v, Q.EPI_F16).astype(np.float32) == v).all()
    e5 = Q.e5m2_values()
    assert e5[0x3C] == 1.0 and e5[0x01] == 2.0 ** -16 and e5[0x7B] == 57344 and np.isnan(e5[0x7C]) and e5[0xC0] == -2.0


def test_fp8_band_codes():
    """the bands hold what they claim: every subnormal code and the first normals; the integers up to 16; multiples of 32 up to 448"""
    assert Q.band_magnitude_codes("l") == set(range(0x00, 0x10))
    assert [float(F) for F in Q._E4M3[sorted(Q.band_magnitude_codes("m"))]] == [float(i) for i in range(17)]
    assert max(Q._E4M3[sorted(Q.band_magnitude_codes("h"))]) == 448 and 0x7E in Q.band_magnitude_codes("h")


def test_every_case_keeps_the_input_conditions():
    used = {"x": set(), "w": set()}
    table = collections.defaultdict(list)
    kinds = collections.Counter()
    lines = []
    for c in Q.all_cases():
        sh = c.check_conditions()          # raises with the case's name
        lines.append(f"  {c.name:52s} " + "  ".join(f"{k}: {100 * v:.1f} %" for k, v in sh.items()))
        for k, v in sh.items():
            table[k].append(v)
        kinds[c.kind] += 1
        if c.fmt == Q.FMT_F8:
            used["x"] |= {int(b) & 0x7F for b in np.unique(c.xq)}
            used["w"] |= {int(b) & 0x7F for b in np.unique(c.wq)}
    print("\nshare of outputs that tells each wrong form apart:")
    print("\n".join(lines))
    print("smallest share per condition:", {k: round(min(v), 4) for k, v in table.items()})
    # every finite non-negative e4m3fn code magnitude that belongs to a band, at least once per operand side
    want = Q.band_magnitude_codes("l") | Q.band_magnitude_codes("m") | Q.band_magnitude_codes("h")
    assert want <= used["x"] and want <= used["w"], (sorted(want - used["x"]), sorted(want - used["w"]))
    assert all(kinds[k] for k in ("ll", "hh", "lh", "full", "large")), kinds


def _family(key):
    return key.split("<")[0]


def test_case_table_holds_the_edges():
    """what the table must hold beyond one case per kernel (a structural check, so that a later edit cannot drop an edge silently)"""
    cases = Q.all_cases()
    fams = {"gemv_i8_kernel", "gemm_i8_pc_kernel", "gemm_i8_wide_kernel", "gemm_i8_256_kernel"}
    assert {_family(c.key) for c in cases if c.epi == Q.EPI_SWIGLU and c.ldy > c.width} == fams       # the w13 -> w2 hand-off
    assert {_family(c.key) for c in cases if c.zero} == fams
    large = [c for c in cases if c.kind == "large"]
    assert any(_family(c.key) == "gemv_i8_kernel" and c.K == max(Q.SWEEP_K) for c in large) and any(_family(c.key) != "gemv_i8_kernel" for c in large)
    for fmt in (Q.FMT_I8, Q.FMT_F8):
        sk = [(c.M, c.N, c.K) for c in cases if c.fmt == fmt and _family(c.key) == "gemv_i8_kernel"]
        assert {16, 48, 64, 768, 4112} <= {k for _, _, k in sk} and {1, 16, 17, 32} <= {m for m, _, _ in sk} and {4, 12} <= {n for _, n, _ in sk}
        pc = [(c.M, c.N, c.K) for c in cases if c.fmt == fmt and _family(c.key) == "gemm_i8_pc_kernel"]
        assert {128, 384, 640} <= {k for _, _, k in pc} and {33, 129} <= {m for m, _, _ in pc} and {132, 1036} <= {n for _, n, _ in pc}
    assert any(c.M == 4100 and c.N == 1092 for c in cases if _family(c.key) == "gemm_i8_256_kernel")
    assert any(c.M % 128 and c.N % 384 for c in cases if _family(c.key) == "gemm_i8_wide_kernel")
    assert all(not (c.layout == "misaligned" and c.epi == Q.EPI_F32) for c in cases)


def test_every_case_takes_its_kernel():
    m = load_pplhip()
    wrong = []
    for c in Q.all_cases():
        rc, route = Q.dry_route(m, c.fmt, c.M, c.N, c.K, c.epi, ldy=c.ldy, y_addr=(1 << 24) + c.y_off_bytes)
        if rc != 0 or Q.coverage_key(route) != c.key:
            wrong.append((c.name, rc, route, c.key))
    assert not wrong, wrong[:5]


_SWEEP_CHILD = """
import json, os, sys
sys.path.insert(0, sys.argv[1])
assert not [k for k in os.environ if k.startswith("PPLHIP_")], "a PPLHIP_* switch is set"
from tests.conftest import load_pplhip
from tests import q8_exact as Q
print(json.dumps(Q.run_sweep(load_pplhip())))
"""


def _sweep():
    env = {k: v for k, v in os.environ.items() if not k.startswith("PPLHIP_")}
    r = subprocess.run([sys.executable, "-c", _SWEEP_CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_coverage_sweep_and_cases_name_the_same_kernels():
    reached = _sweep()
    cover = collections.defaultdict(list)
    for c in Q.all_cases():
        cover[c.key].append(c.name)
    print(f"\ncoverage: {len(reached)} kernel instantiations reached by the sweep, {len(Q.all_cases())} exact cases")
    for k in sorted(reached):
        print(f"  {k:36s} cheapest {reached[k]}  <- {len(cover.get(k, []))} cases")
    missing = sorted(set(reached) - set(cover))
    assert not missing, f"kernels the sweep reaches without an exact case: {missing} (first shapes: {[reached[k] for k in missing]})"
    gone = sorted(set(cover) - set(reached))
    assert not gone, f"cases whose kernel the sweep no longer reaches: {[(k, cover[k]) for k in gone]}"
    # each kernel's first case is the cheapest shape of the grid that reaches it
    first = {}
    for c in Q.all_cases():
        first.setdefault(c.key, (c.M, c.N, c.K))
    dearer = {k: (first[k], reached[k][1:4]) for k in reached if first[k][0] * first[k][1] * first[k][2] != reached[k][1] * reached[k][2] * reached[k][3]}
    assert not dearer, dearer


def test_reached_kernels_are_pinned():
    reached = _sweep()
    assert sorted(reached) == REACHED, (sorted(set(reached) - set(REACHED)), sorted(set(REACHED) - set(reached)))
    assert len(REACHED) == 39
    compiled = Q.compiled_instantiations()
    assert set(REACHED) <= compiled
    opened = [(u, why) for u in REACHED for p, why in Q.UNREACHABLE if re.fullmatch(p, u)]
    assert not opened, f"instantiations listed as unreachable are reached now -- give them exact cases: {opened}"
    unexplained = [u for u in sorted(compiled - set(REACHED)) if not any(re.fullmatch(p, u) for p, _ in Q.UNREACHABLE)]
    assert not unexplained, f"compiled instantiations neither reached nor listed as unreachable: {unexplained}"


def test_dry_run_refusals_match_the_launch_rules():
    """N % 4, K % 16, ldy % 4, a bad epilogue or format are refused before any plan; M = 0 is a no-op; the route text of a plan"""
    m = load_pplhip()
    for fmt, M, N, K, epi, ldy in [(8, 8, 6, 64, 0, 8), (0x108, 8, 64, 24, 0, 64), (8, 8, 64, 64, 0, 66), (0x108, 8, 60, 64, 2, 30),
                                   (8, 8, 64, 64, 3, 64), (4, 8, 64, 64, 0, 64), (0x100, 8, 64, 64, 0, 64)]:
        rc, route = Q.dry_route(m, fmt, M, N, K, epi, ldy=ldy)
        assert rc == -2 and route == "", (fmt, M, N, K, epi, ldy, rc, route)
    for fmt in (Q.FMT_I8, Q.FMT_F8):
        assert Q.dry_route(m, fmt, 0, 64, 64, 0) == (0, "")
    assert Q.dry_route(m, Q.FMT_F8, 1024, 4096, 4096, 0)[1] == "kernel=gemm_i8_pc_kernel<f16,4,f8> grid=256x1 threads=512 lds=131072 n_tiles=32 m_tiles=8"
    assert Q.dry_route(m, Q.FMT_I8, 4096, 22016, 4096, 2, ldy=11008)[1] == ("kernel=gemm_i8_256_kernel<swiglu,4> grid=2048x1 threads=512 lds=131072 "
                                                                          "n_tiles=86 m_tiles=16 order=super(4x8)")
