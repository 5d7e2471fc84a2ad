#!/usr/bin/env python3
"""Device-assembly comparison of the five GEMM sources between two trees (no GPU needed: hipcc cross-compiles).

    python profiles/gemm_asm_compare.py OLD/ppl.llm.serving_amd/csrc NEW/ppl.llm.serving_amd/csrc [--keep DIR]

Each source is compiled with the Makefile's flags plus --cuda-device-only -S.  Per source the script prints the kernel symbols only
one side has, and for every common kernel whether its instructions are byte-identical (comments dropped, and the function index inside local
labels, .LBB<index>_<block>, which only follows the order in which the templates are instantiated); where they are not, the figures that decide whether
the kernel still does the same work at the same occupancy: counts of v_mfma*, LDS reads (ds_read* / ds_load*), LDS-DMA
(global_load_lds* / buffer_load*lds), s_barrier and global_store*, scratch bytes, static LDS bytes, and the VGPR count with its
allocation granule of 8.  A kernel MISSES the bar when any count differs, scratch is not zero, the LDS size differs or the VGPR
count leaves its granule.  Exit status 1 when a kernel misses the bar."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

SOURCES = ["k_gemm.hip", "k_gemm_wide.hip", "k_gemm_pc.hip", "k_gemv.hip", "k_gemm_i8.hip"]
VGPR_FORM = {"k_gemm.hip", "k_gemm_wide.hip", "k_gemm_i8.hip"}   # csrc/Makefile: -mllvm -amdgpu-mfma-vgpr-form=1
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fvisibility=hidden -Wall -Wno-unused-result -Wno-unused-value".split()
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
COUNTED = [("mfma", r"v_mfma"), ("lds_read", r"ds_(read|load)"), ("lds_dma", r"(global_load_lds|buffer_load\w*lds)"),
           ("barrier", r"s_barrier"), ("gstore", r"global_store")]


def compile_asm(csrc, src, out):
    cmd = [HIPCC] + FLAGS + (["-mllvm", "-amdgpu-mfma-vgpr-form=1"] if src in VGPR_FORM else []) + \
          ["--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)


def parse(path):
    """-> {symbol: {"text": body, counts..., "scratch", "lds", "vgpr", "sgpr"}}"""
    lines = open(path).read().split("\n")
    kernels, cur, body = {}, None, []
    for ln in lines:
        m = re.match(r"^(\w+):\s*; @\1\s*$", ln)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:", ln):
                # comments dropped; local labels carry the function's index in the module (.LBB<index>_<block>), which follows the
                # order of instantiation
                code = "\n".join(ln.split(";")[0].rstrip() for ln in body)
                kernels[cur] = {"text": re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", code)}
                cur = None
            else:
                body.append(ln)
    meta, entry = [], None
    for ln in lines:
        if re.match(r"^  - \.\w+:", ln):
            entry = {}
            meta.append(entry)
            ln = "    " + ln[4:]
        m = re.match(r"^    \.(\w+):\s+(.*)$", ln)
        if m and entry is not None:
            entry[m.group(1)] = m.group(2).strip()
    for e in meta:
        k = kernels.get(e.get("name"))
        if k is not None:
            k.update(scratch=int(e["private_segment_fixed_size"]), lds=int(e["group_segment_fixed_size"]), vgpr=int(e["vgpr_count"]),
                     sgpr=int(e["sgpr_count"]))
    kernels = {s: k for s, k in kernels.items() if "vgpr" in k}   # kernels only, not device functions
    for k in kernels.values():
        code = [ln.strip() for ln in k["text"].split("\n")]
        for name, rx in COUNTED:
            k[name] = sum(1 for c in code if re.match(rx, c))
    return kernels


def demangle(syms):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not syms or not filt:
        return {s: s for s in syms}
    out = subprocess.run([filt] + list(syms), capture_output=True, text=True).stdout.split("\n")
    return {s: re.sub(r"^(void )?pplhip::(\(anonymous namespace\)::)?|\(.*$", "", d) for s, d in zip(syms, out)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_dir")
    ap.add_argument("new_dir")
    ap.add_argument("--keep", help="directory that keeps the .s files")
    a = ap.parse_args()
    old_dir, new_dir, keep = a.old_dir, a.new_dir, a.keep
    work = keep or tempfile.mkdtemp(prefix="gemm_asm_")
    os.makedirs(work, exist_ok=True)
    jobs = [(d, src, os.path.join(work, f"{tag}_{src}.s")) for src in SOURCES for tag, d in (("old", old_dir), ("new", new_dir))]
    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1, 10)) as pool:
        list(pool.map(lambda j: compile_asm(*j), jobs))
    missed = 0
    for src in SOURCES:
        sides = [parse(os.path.join(work, f"{tag}_{src}.s")) for tag in ("old", "new")]
        old, new = sides
        names = demangle(sorted(set(old) | set(new)))
        common = sorted(set(old) & set(new), key=lambda s: names[s])
        same = [s for s in common if old[s]["text"] == new[s]["text"]]
        print(f"== {src}: {len(old)} kernels old, {len(new)} new, {len(same)} of {len(common)} common kernels byte-identical")
        for s in sorted(set(old) - set(new)):
            print(f"   only old: {names[s]}")
        for s in sorted(set(new) - set(old)):
            print(f"   only new: {names[s]}")
        for s in common:
            if s in same:
                continue
            a, b = old[s], new[s]
            bad = [n for n, _ in COUNTED if a[n] != b[n]]
            if a["scratch"] or b["scratch"]:
                bad.append("scratch")
            if a["lds"] != b["lds"]:
                bad.append("lds")
            if (a["vgpr"] + 7) // 8 != (b["vgpr"] + 7) // 8:
                bad.append("vgpr granule")
            missed += bool(bad)
            counts = " ".join(f"{n} {a[n]}/{b[n]}" for n, _ in COUNTED)
            print(f"   {'MISS' if bad else 'ok  '} {names[s]}: {counts} scratch {a['scratch']}/{b['scratch']} lds {a['lds']}/{b['lds']} "
                  f"vgpr {a['vgpr']}/{b['vgpr']} sgpr {a['sgpr']}/{b['sgpr']}" + (f"  <- {', '.join(bad)}" if bad else ""))
    print(f"kernels that miss the bar: {missed}")
    sys.exit(1 if missed else 0)


if __name__ == "__main__":
    main()
