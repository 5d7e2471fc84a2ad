#!/usr/bin/env python3
"""Device-assembly comparison of the kernel sources between two trees (no GPU needed: hipcc cross-compiles).

    python profiles/asm_compare.py OLD/ppl.llm.serving_amd/csrc NEW/ppl.llm.serving_amd/csrc [--sources k_a.hip,k_b.hip] [--keep DIR]
                                   [--map 'REGEX=REPLACEMENT']

Each source is compiled with the command its tree's Makefile uses for it (make -n), with --cuda-device-only -S in place of -c.  Per
source the script prints the kernel symbols only one side has, and classes every common kernel:
  identical  the instructions are byte-identical (comments dropped, and the function index inside local labels, .LBB<index>_<block>,
             which only follows the order in which the templates are instantiated);
  reordered  the same multiset of mnemonics: only the order of instructions or the names of registers differ.  (A conditional
             branch and the scalar compare in front of it count the same in either sense -- s_cmp_eq / s_cmp_lg, s_cbranch_scc0 /
             scc1, vccz / vccnz, execz / execnz: which sense a loop's back edge takes follows the order of the basic blocks.
             s_nop and s_waitcnt are left out of the multiset: the hazard and wait-count passes insert them after scheduling,
             as the order requires.  The total instruction count printed beside the class includes them.)
  differs    anything else.
For a kernel that is not identical it prints the total instruction count and the figures that decide whether it still does the same
work at the same occupancy: counts of v_mfma*, LDS reads (ds_read* / ds_load*), LDS-DMA (global_load_lds* / buffer_load*lds),
s_barrier and global_store*, scratch bytes, static LDS bytes, and the VGPR count with its allocation granule of 8.  A kernel MISSES the
bar when it differs, when its instruction count rises (whatever its class), when any count differs, scratch is above the old tree's,
the LDS size differs or the VGPR count leaves its granule.  A source of which no kernel exists on both sides under the same name
misses too: nothing was compared.  Exit status 1 when anything misses the bar.  The first line of the output is the command line.
--map renames OLD kernels (demangled names) before matching, for a kernel whose template parameter list changed.  Against commit
badc41a and earlier, whose 16-row prefill kernel had a fourth parameter RG (1 in every kernel that is left):
    --map 'attn_prefill_kernel<(.*), 1>=attn_prefill_kernel<\\1>'"""
import argparse
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

SOURCES = ["k_gemm.hip", "k_gemm_wide.hip", "k_gemm_pc.hip", "k_gemv.hip", "k_gemm_i8.hip",
           "k_attn_decode.hip", "k_attn_decode_gqa.hip", "k_attn_prefill.hip", "k_attn_prefill32.hip"]
SENSE = re.compile(r"^(s_cmp_|s_cbranch_(?:scc|vcc|exec))(?:eq|lg|0|1|z|nz)(?=_|$)")   # a compare / branch in either sense
COUNTED = [("mfma", r"v_mfma"), ("lds_read", r"ds_(read|load)"), ("lds_dma", r"(global_load_lds|buffer_load\w*lds)"),
           ("barrier", r"s_barrier"), ("gstore", r"global_store")]


def compile_asm(csrc, src, out):
    """the Makefile's own command for this object (per-file flags included), turned into a device-only assembly run"""
    obj = src[:-4] + ".o"
    plan = subprocess.run(["make", "-n", "-B", "-C", csrc, obj], capture_output=True, text=True, check=True).stdout.split("\n")
    cmd = shlex.split([ln for ln in plan if f" -c {src} " in ln][-1])
    i = cmd.index("-c")
    cmd = cmd[:i] + ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.check_call(cmd, cwd=csrc, stderr=subprocess.DEVNULL)


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
        # instructions: not blank, not a label, not a directive
        insts = [SENSE.sub(r"\1", c.split()[0]) for c in code if c and not c.endswith(":") and not c.startswith(".")]
        k["insts"] = len(insts)
        k["mnemonics"] = sorted(m for m in insts if m not in ("s_nop", "s_waitcnt"))
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
    ap.add_argument("--sources", help="comma-separated source files (default: all nine kernel sources)")
    ap.add_argument("--map", action="append", default=[], help="REGEX=REPLACEMENT applied to the old tree's demangled kernel names")
    ap.add_argument("--keep", help="directory that keeps the .s files")
    a = ap.parse_args()
    old_dir, new_dir, keep = os.path.abspath(a.old_dir), os.path.abspath(a.new_dir), a.keep and os.path.abspath(a.keep)
    sources = a.sources.split(",") if a.sources else SOURCES
    work = keep or tempfile.mkdtemp(prefix="asm_compare_")
    os.makedirs(work, exist_ok=True)
    jobs = [(d, src, os.path.join(work, f"{tag}_{src}.s")) for src in sources for tag, d in (("old", old_dir), ("new", new_dir))]
    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1, 10)) as pool:
        list(pool.map(lambda j: compile_asm(*j), jobs))
    print("command: python profiles/asm_compare.py " + " ".join(shlex.quote(x) for x in sys.argv[1:]))
    missed = 0
    for src in sources:
        sides = []
        for tag in ("old", "new"):   # kernels by demangled name; the old side's after --map
            k = parse(os.path.join(work, f"{tag}_{src}.s"))
            names = demangle(sorted(k))
            for rule in (a.map if tag == "old" else []):
                rx, repl = rule.split("=", 1)
                names = {s: re.sub(rx, repl, n) for s, n in names.items()}
            sides.append({names[s]: v for s, v in k.items()})
        old, new = sides
        common = sorted(set(old) & set(new))
        same = [s for s in common if old[s]["text"] == new[s]["text"]]
        moved = [s for s in common if s not in same and old[s]["mnemonics"] == new[s]["mnemonics"]]
        print(f"== {src}: {len(old)} kernels old, {len(new)} new; of {len(common)} common kernels {len(same)} identical, "
              f"{len(moved)} reordered, {len(common) - len(same) - len(moved)} differ")
        for s in sorted(set(old) - set(new)):
            print(f"   only old: {s}")
        for s in sorted(set(new) - set(old)):
            print(f"   only new: {s}")
        if not common:   # nothing was compared: a changed template parameter list needs --map, or the source is new
            missed += 1
            print("   MISS no kernel of this source exists on both sides under the same name (see --map)")
        for s in common:
            if s in same:
                continue
            a_, b = old[s], new[s]
            bad = [] if s in moved else ["differs"]
            if b["insts"] > a_["insts"]:
                bad.append("instruction count")
            bad += [n for n, _ in COUNTED if a_[n] != b[n]]
            if b["scratch"] > a_["scratch"]:
                bad.append("scratch")
            if a_["lds"] != b["lds"]:
                bad.append("lds")
            if (a_["vgpr"] + 7) // 8 != (b["vgpr"] + 7) // 8:
                bad.append("vgpr granule")
            missed += bool(bad)
            counts = " ".join(f"{n} {a_[n]}/{b[n]}" for n, _ in COUNTED)
            print(f"   {'MISS' if bad else 'ok  '} {'reordered' if s in moved else 'differs  '} {s}: insts {a_['insts']}/{b['insts']} {counts} "
                  f"scratch {a_['scratch']}/{b['scratch']} lds {a_['lds']}/{b['lds']} vgpr {a_['vgpr']}/{b['vgpr']} sgpr {a_['sgpr']}/{b['sgpr']}"
                  + (f"  <- {', '.join(bad)}" if bad else ""))
    print(f"kernels that miss the bar: {missed}")
    sys.exit(1 if missed else 0)


if __name__ == "__main__":
    main()
