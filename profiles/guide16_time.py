#!/usr/bin/env python3
"""What loading a wide guide costs (pplhip_guide_load16; guide_build16_kernel of csrc/k_guide.hip).  Every shape runs in a process of its
own under its own time limit; a shape that fails or runs out of time ends the script.  Every leg is warmed up; the median over all timed
calls and the spread (max - min) of the per-round medians.

    load S V      pplhip_guide_load16 on a context of vocabulary V, S states: WALL time of the whole synchronous call (validation, two
                  allocations, the uploads, the build kernel, the read-back of the any-flags), the slot unloaded between calls; and the
                  build kernel alone (pplhip_op_guide_build16, device time between two events).  For S <= 255 the same automaton through
                  pplhip_guide_load / pplhip_op_guide_build, alternated with the wide legs in rounds: the existing kernel as the reference.
                  The automaton and the tokens follow the distribution of build/guide_json_trace hostbuild (eight letters, one transition
                  in fifty dead, tokens of 1 .. 9 bytes), which draws its own data and times walks of the same kind as a single-thread C++
                  loop on the CPU: the `host` line.  Like data, not the same data: the byte totals of the two differ slightly.
Writes one JSON line per leg to profiles/guide16_time.jsonl.
usage: python profiles/guide16_time.py                       (everything, one child process per shape)
       python profiles/guide16_time.py --shape 4096 128256"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "guide16_time.jsonl")
SHAPES = [(4096, 128256), (289, 32000), (255, 32000)]
STEP_SECONDS = 240
ROUNDS, CALLS, WARM = 4, 10, 3


def emit(rec):
    print(json.dumps(rec), flush=True)


def shape(S, V):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from oracle import ref
    from tests.conftest import load_pplhip
    m = load_pplhip()
    L = m.lib()
    rng = np.random.default_rng(S * 1000003 + V)
    trans = np.full((S, 256), 0xFFFF, dtype=np.uint16)
    for ch in b"abcdefgh":
        trans[:, ch] = np.where(rng.random(S) < 0.02, 0xFFFF, rng.integers(0, S, size=S))
    accept = np.ones(S, dtype=np.uint8)
    lens = rng.integers(1, 10, size=V)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    blob = np.frombuffer(b"abcdefgh", dtype=np.uint8)[rng.integers(0, 8, size=int(off[-1]))].copy()
    toks = [blob[off[t]:off[t + 1]].tobytes() for t in range(V)]
    narrow = S <= 255
    trans8 = np.where(trans == 0xFFFF, 255, trans).astype(np.uint8) if narrow else None

    desc = ref.make_desc(hidden_dim=256, intermediate_dim=512, num_layers=1, num_heads=4, num_kv_heads=4, vocab_size=V, max_position=512,
                         cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=0, weight_quant_bit=8)
    ctx = m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=64)
    ctx.init_synthetic(0, 7)
    ctx.guide_set_vocab(toks)

    W = (V + 31) // 32
    d = [torch.from_numpy(a).cuda() for a in (trans.view(np.int16), accept, blob, off, np.array([2], dtype=np.int32))]
    d8 = torch.from_numpy(trans8).cuda() if narrow else None
    mask = torch.zeros((S, W), dtype=torch.int32, device="cuda")
    anyf = torch.zeros(S, dtype=torch.int32, device="cuda")

    def wall_us(load):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        load()
        us = (time.perf_counter() - t0) * 1e6
        ctx.guide_unload(0)
        return us

    def device_us(fn, table):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        rc = fn(None, table.data_ptr(), d[1].data_ptr(), S, d[2].data_ptr(), d[3].data_ptr(), V, d[4].data_ptr(), 1, V, mask.data_ptr(), W,
                anyf.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        return e0.elapsed_time(e1) * 1e3

    legs = {"load16_wall": lambda: wall_us(lambda: ctx.guide_load16(0, trans, accept, [2])),
            "build16_kernel": lambda: device_us(L.pplhip_op_guide_build16, d[0])}
    if narrow:
        legs["load_wall"] = lambda: wall_us(lambda: ctx.guide_load(0, trans8, accept, [2]))
        legs["build_kernel"] = lambda: device_us(L.pplhip_op_guide_build, d8)
        # the two kernels write the same mask
        device_us(L.pplhip_op_guide_build, d8)
        first = mask.clone()
        mask.zero_()
        device_us(L.pplhip_op_guide_build16, d[0])
        assert torch.equal(first, mask)
    calls, meds = {}, {}
    for _ in range(ROUNDS):
        for name, f in legs.items():
            for _ in range(WARM):
                f()
            us = [f() for _ in range(CALLS)]
            calls.setdefault(name, []).extend(us)
            meds.setdefault(name, []).append(float(np.median(us)))
    for name in legs:
        emit(dict(leg=name, states=S, tokens=V, bytes=int(off[-1]), us=round(float(np.median(calls[name])), 1),
                  spread_us=round(max(meds[name]) - min(meds[name]), 1), calls=len(calls[name])))
    ctx.close()


def main():
    if "--shape" in sys.argv:
        k = sys.argv.index("--shape")
        shape(int(sys.argv[k + 1]), int(sys.argv[k + 2]))
        return 0
    tool = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "guide_json_trace")
    steps = []
    for S, V in SHAPES:
        steps.append([sys.executable, os.path.abspath(__file__), "--shape", str(S), str(V)])
        steps.append([tool, "hostbuild", str(S), str(V)])
    lines = []
    for cmd in steps:
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            print("timed out: " + " ".join(cmd), file=sys.stderr)
            return 1
        if out.returncode != 0:   # nothing more is started after a step that failed
            print(f"exit {out.returncode}: {' '.join(cmd)}\n{out.stderr[-2000:]}", file=sys.stderr)
            return 1
        for line in out.stdout.splitlines():
            if line.startswith("{"):
                rec = json.loads(line)
                if "host_build_ms" in rec:
                    rec = dict(leg="host", states=rec["states"], tokens=rec["tokens"], bytes=rec["bytes"], ms=round(rec["host_build_ms"], 2))
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    with open(OUT, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
