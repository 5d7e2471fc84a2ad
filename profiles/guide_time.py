#!/usr/bin/env python3
"""What guided decoding costs (csrc/k_guide.hip) at the operator level.  Every shape runs in a process of its own under its own time limit;
a shape that fails or runs out of time ends the script.  Device time between two events on the stream around ONE call that is followed by
a synchronise; every leg is warmed up; the median over all timed calls and the spread (max - min) of the per-round medians.

    build S V     pplhip_op_guide_build, S states x V tokens, for S in (64, 255) and V in (32000, 128256): a synthetic automaton over eight
                  letters in which a walk rarely dies (one transition in fifty is dead) and tokens of 1 .. 9 bytes, 5 on average -- the
                  shape of build/guide_trace hostbuild, which times the same (state, token) walks as a single-thread C++ loop on this
                  machine's CPU: the `host` line of the same shape
    mask          pplhip_op_guide_mask, 1024 asking rows of 32000 logits, 16 slots x 64 states, 1000 allowed tokens per mask row, against
                  pplhip_op_logit_edit with a mask of 1000 allowed tokens per row and nothing else, alternated in rounds in the same process.
                  The two do the same stores, so parity is expected; above 1.2x wants an explanation
Writes one JSON line per leg to profiles/guide_time.jsonl.
usage: python profiles/guide_time.py                       (everything, one child process per shape)
       python profiles/guide_time.py --shape build 64 32000  |  --shape mask"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "guide_time.jsonl")
BUILD_SHAPES = [(64, 32000), (64, 128256), (255, 32000), (255, 128256)]
STEP_SECONDS = 240


def emit(rec):
    print(json.dumps(rec), flush=True)


def shape_build(S, V):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from tests.conftest import load_pplhip
    L = load_pplhip().lib()
    rng = np.random.default_rng(S * 1000003 + V)
    trans = np.full((S, 256), 255, dtype=np.uint8)
    for ch in b"abcdefgh":
        trans[:, ch] = np.where(rng.random(S) < 0.02, 255, rng.integers(0, S, size=S))
    accept = np.ones(S, dtype=np.uint8)
    lens = rng.integers(1, 10, size=V)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    blob = np.frombuffer(b"abcdefgh", dtype=np.uint8)[rng.integers(0, 8, size=int(off[-1]))].copy()
    W = (V + 31) // 32
    d = [torch.from_numpy(a).cuda() for a in (trans, accept, blob, off, np.array([2], dtype=np.int32))]
    mask = torch.zeros((S, W), dtype=torch.int32, device="cuda")
    anyf = torch.zeros(S, dtype=torch.int32, device="cuda")

    def call():
        return L.pplhip_op_guide_build(None, d[0].data_ptr(), d[1].data_ptr(), S, d[2].data_ptr(), d[3].data_ptr(), V, d[4].data_ptr(), 1, V,
                                       mask.data_ptr(), W, anyf.data_ptr())

    def device_us():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        rc = call()
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        return e0.elapsed_time(e1) * 1e3

    for _ in range(5):
        device_us()
    meds = []
    for _ in range(4):
        meds.append(float(np.median([device_us() for _ in range(25)])))
    bits = int(sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in mask[0].cpu().numpy()))
    emit(dict(leg="build", states=S, tokens=V, bytes=int(off[-1]), us=round(float(np.median(meds)), 2), spread_us=round(max(meds) - min(meds), 2),
              calls=100, allowed_in_state_0=bits))


def shape_mask():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from tests import logit_rules as R
    from tests.conftest import load_pplhip
    L = load_pplhip().lib()
    B, V, SLOTS, S, ROUNDS, CALLS, WARM = 1024, 32000, 16, 64, 4, 50, 3
    W = R.words(V)
    rng = np.random.default_rng(0)
    pristine = torch.from_numpy((rng.standard_normal((B, V)) * 2.0).astype(np.float32)).cuda()
    work = torch.empty_like(pristine)
    mk = np.stack([R.pack_mask(rng.choice(V, size=1000, replace=False).tolist(), V) for _ in range(B)]).astype(np.uint32)
    masks = torch.from_numpy(mk.view(np.int32)).cuda()            # [B, W]: the rule table's masks, and the guides' [16, 64, W]
    head = np.zeros((B, 4), dtype=np.int32)
    head[:, 2] = 1                                                 # a mask and nothing else
    tab = [torch.from_numpy(a).cuda() for a in (head, np.zeros((B, R.BIAS_MAX), dtype=np.int32), np.zeros((B, R.BIAS_MAX), dtype=np.float32),
                                                 np.zeros((B, R.STOP_MAX), dtype=np.int32))] + [masks]
    perm = rng.permutation(B).astype(np.int32)
    slots = torch.from_numpy(perm).cuda()                          # the rule of row b: record perm[b]
    g_slots = torch.from_numpy((perm // S).astype(np.int32)).cuda()   # the same mask row through (slot, state)
    g_states = torch.from_numpy((perm % S).astype(np.int32)).cuda()
    rows = torch.arange(B, dtype=torch.int32, device="cuda")
    flags = torch.ones(B, dtype=torch.int32, device="cuda")
    legs = {
        "logit_edit_mask_only": lambda: L.pplhip_op_logit_edit(None, work.data_ptr(), V, V, B, flags.data_ptr(), slots.data_ptr(),
                                                               *[t.data_ptr() for t in tab], rows.data_ptr(), B),
        "guide_mask": lambda: L.pplhip_op_guide_mask(None, work.data_ptr(), V, V, B, g_slots.data_ptr(), g_states.data_ptr(), masks.data_ptr(),
                                                     SLOTS, S, W, rows.data_ptr(), B),
    }

    def device_us(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        work.copy_(pristine)
        torch.cuda.synchronize()
        e0.record()
        rc = f()
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0, rc
        return e0.elapsed_time(e1) * 1e3

    images = {}
    for name, f in legs.items():                                   # the two legs write the same image
        device_us(f)
        images[name] = work.clone()
    assert torch.equal(images["guide_mask"].view(torch.int32), images["logit_edit_mask_only"].view(torch.int32))
    calls, meds = {}, {}
    for _ in range(ROUNDS):
        for name, f in legs.items():
            for _ in range(WARM):
                device_us(f)
            us = [device_us(f) for _ in range(CALLS)]
            calls.setdefault(name, []).extend(us)
            meds.setdefault(name, []).append(float(np.median(us)))
    res = {n: float(np.median(v)) for n, v in calls.items()}
    for n in legs:
        emit(dict(leg=n, B=B, V=V, us=round(res[n], 2), spread_us=round(max(meds[n]) - min(meds[n]), 2), calls=len(calls[n])))
    ratio = res["guide_mask"] / res["logit_edit_mask_only"]
    emit(dict(expectation="guide_mask <= 1.2 x logit_edit_mask_only", ratio=round(ratio, 3), met=bool(ratio <= 1.2)))


def main():
    if "--shape" in sys.argv:
        k = sys.argv.index("--shape")
        if sys.argv[k + 1] == "build":
            shape_build(int(sys.argv[k + 2]), int(sys.argv[k + 3]))
        else:
            shape_mask()
        return 0
    tool = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "guide_trace")
    steps = []
    for S, V in BUILD_SHAPES:
        steps.append([sys.executable, os.path.abspath(__file__), "--shape", "build", str(S), str(V)])
        steps.append([tool, "hostbuild", str(S), str(V)])
    steps.append([sys.executable, os.path.abspath(__file__), "--shape", "mask"])
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
