#!/usr/bin/env python3
"""A/B of two builds of libpplhip.so on the step schedule: the same bits from every schedule.

    PPLHIP_LIB=<lib> python profiles/step_ab.py --case NAME     one build, one case: a JSON line (SHA-256 of every step's logits and of
                                                               rank 0's KV slab at the end); the case's switches come from the caller
    python profiles/step_ab.py --ab PARENT_LIB HEAD_LIB [--log FILE] [--cases NAME,...]
    python profiles/step_ab.py --timing PARENT_LIB HEAD_LIB [--log FILE] [--rounds 3] [--legs bench,small,dual]

--ab runs every case once per library, a fresh process each with the case's switches and a time limit, and stops at the first child
that fails: nothing more is started on the device.  Every hash must be equal between the two libraries.
The model is the tiny synthetic one of tests/test_gpu_tp.py (hidden 512, 3 layers, vocab 2048, W8, int8 KV, pages of 16), all ranks
of a group on device 0: a packed prefill, then four decode steps on the library's own greedy tokens.  The two-lane case at tp 1
alternates prefill -> two-lane decode -> a mixed step with one new request -> two-lane decode in one context.
--timing runs the two libraries alternately (P H P H ..., a fresh process each) on bench.py's headline, on
profiles/small_batch_latency.py at batch 1 / 8 / 64 and on one two-stream step (PPLHIP_DUAL_STREAM=1, tp 1, 256 rows), and judges each
figure by the parent's own spread (max - min of its rounds): the head's median must lie within that of the parent's median."""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHORT = (40, 3, 129, 1, 16, 77)
WIDE = (40, 3, 29, 1, 16, 77, 5, 9, 2, 33, 12)    # eleven decode rows: halves of 5 + 6
OV1 = {"PPLHIP_TP_OVERLAP": "1", "PPLHIP_TP_OVERLAP_MIN_TOKENS": "2"}
# name: (tp, act_quant_bit, prompt lengths, a new request joins after the first decode step, switches)
CASES = {
    "tp1_plain": (1, 0, SHORT, False, {}),
    "tp1_two_lane_mixed": (1, 0, WIDE, True, {"PPLHIP_DUAL_STREAM": "1", "PPLHIP_DUAL_MIN_ROWS": "8"}),
    "tp1_graph": (1, 0, SHORT, False, {"PPLHIP_DECODE_GRAPH": "1"}),
    "tp1_comm_ov0": (1, 0, SHORT, False, {"PPLHIP_FORCE_COMM": "1", "PPLHIP_TP_OVERLAP": "0"}),
    "tp1_comm_ov1_flags": (1, 0, SHORT, False, dict(OV1, PPLHIP_FORCE_COMM="1")),
    "tp1_comm_ov1_events": (1, 0, SHORT, False, dict(OV1, PPLHIP_FORCE_COMM="1", PPLHIP_TP_HANDOFF="events")),
    "tp2_ov0": (2, 0, SHORT, False, {"PPLHIP_TP_OVERLAP": "0"}),
    "tp2_ov1": (2, 0, SHORT, False, OV1),
    "tp2_no_fused_norm": (2, 0, SHORT, False, {"PPLHIP_TP_OVERLAP": "0", "PPLHIP_TP_FUSE_NORM": "0"}),
    "tp2_two_lane": (2, 0, WIDE, False, {"PPLHIP_DUAL_STREAM": "1", "PPLHIP_DUAL_MIN_ROWS": "2", "PPLHIP_TP_OVERLAP": "0"}),
    "tp2_i8_ov1": (2, 8, SHORT, False, OV1),
}
SWITCHES = sorted({k for c in CASES.values() for k in c[4]})
PG, KV_TOKENS, DECODE_STEPS, CHILD_SECONDS = 16, 2048, 4, 300


def run_case(name):
    import numpy as np
    from tests.conftest import load_pplhip
    m = load_pplhip()
    tp, act, lens, joins, _ = CASES[name]
    desc = m.make_desc(hidden_dim=512, intermediate_dim=1024, num_layers=3, num_heads=8, num_kv_heads=8, vocab_size=2048, max_position=512,
                       cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=1, page_size=PG, weight_quant_bit=8, act_quant_bit=act)
    ctx = m.Context(desc, max_running_batch=16, max_tokens_per_step=512, n_local_ranks=tp, device_ids=[0] * tp)
    for r in range(tp):
        ctx.init_synthetic(r, 31 + tp)
        ctx.kv_alloc(r, KV_TOKENS)
    rng = np.random.RandomState(tp)
    prompts = [rng.randint(3, 2048, size=n) for n in lens]
    late = rng.randint(3, 2048, size=7)                      # the request that joins (its pages are planned from the start)
    total = np.array([len(p) for p in prompts] + [len(late)]) + DECODE_STEPS + 1
    npg = (total + PG - 1) // PG
    mp = int(npg.max())
    pages = np.full((len(total), mp), np.iinfo(np.int64).max, dtype=np.int64)
    order, k = np.random.RandomState(0).permutation(KV_TOKENS // PG), 0
    for i in range(len(total)):
        pages[i, :npg[i]] = order[k:k + npg[i]]
        k += npg[i]

    def step(tok, seq, start_pos, dec, changed):
        n = len(start_pos)
        st = m.make_step(tok, seq, start_pos, pages[:n], dec, mp, req_list_changed=changed)
        for r in range(tp):      # one host thread enqueues every rank's step; the streams run side by side
            ctx.set_inputs(r, st)
            ctx.run(r)
        logits = ctx.copy_logits(n)
        for r in range(1, tp):
            ctx.sync(r)
        return logits

    n = len(prompts)
    lens_a = np.array([len(p) for p in prompts])
    logits = step(np.concatenate(prompts).astype(np.int64), np.concatenate([[0], np.cumsum(lens_a)]), np.zeros(n, dtype=np.int64), 0, 1)
    hashes = [hashlib.sha256(logits.tobytes()).hexdigest()]
    start_pos = lens_a.astype(np.int64)
    for s in range(DECODE_STEPS):
        tok = logits.argmax(-1).astype(np.int64)
        if joins and s == 1:     # n decode rows, then the new request's prompt
            logits = step(np.concatenate([tok, late]), np.concatenate([np.arange(n + 1), [n + len(late)]]), np.concatenate([start_pos, [0]]), n, 1)
            start_pos = np.concatenate([start_pos + 1, [len(late)]])
            n += 1
        else:
            logits = step(tok, np.arange(n + 1), start_pos, n, 0)
            start_pos = start_pos + 1
        hashes.append(hashlib.sha256(logits.tobytes()).hexdigest())
    kv = hashlib.sha256(ctx.kv_read(0, 0).tobytes() + ctx.kv_read(0, 1).tobytes()).hexdigest()
    info = ctx.comm_info(n)
    ctx.close()
    print(json.dumps({"case": name, "logits": hashes, "kv": kv, "schedule": info["schedule"], "collectives": info["mode"]}), flush=True)


def child(cmd, env, seconds):
    """(status, stdout, stderr) of one child under its time limit; a child that runs out of time counts as failed like any other"""
    try:
        r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=seconds)
        return r.returncode, r.stdout, r.stderr
    except subprocess.TimeoutExpired as e:
        out, err = [x.decode(errors="replace") if isinstance(x, bytes) else (x or "") for x in (e.stdout, e.stderr)]
        return f"none: killed at its time limit of {seconds} s", out, err


def stop(lines, what, out, err, log):
    """a failed child ends the run: nothing more is started on the device; the log says which child it was"""
    text = "\n".join(lines + [what, out[-2000:], err[-4000:]])
    if log:
        open(log, "w").write(text + "\n")
    sys.exit(text)


def ab(parent, head, only, log):
    lines, ok = ["command: " + " ".join(sys.argv)], True
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    for name in [c for c in CASES if not only or c in only]:
        got = {}
        for tag, lib in (("parent", parent), ("head", head)):
            print(f"{name}: {tag}", file=sys.stderr, flush=True)
            rc, out, err = child([os.path.abspath(__file__), "--case", name], dict(base, PPLHIP_LIB=os.path.abspath(lib), **CASES[name][4]), CHILD_SECONDS)
            if rc != 0:
                stop(lines, f"{name}: {tag} run failed with status {rc}", out, err, log)
            got[tag] = [json.loads(ln) for ln in out.split("\n") if ln.startswith("{")][-1]
        same = got["parent"]["logits"] == got["head"]["logits"] and got["parent"]["kv"] == got["head"]["kv"]
        ok &= same
        lines.append(f"{name}: {len(got['head']['logits'])} steps, logits {' '.join(h[:12] for h in got['head']['logits'])} | kv {got['head']['kv'][:12]} | "
                     f"schedule of the last step: {got['head']['schedule']} (parent reports: {got['parent']['schedule']}) | "
                     f"{'equal' if same else 'DIFFER: parent ' + json.dumps(got['parent'])}")
    lines.append("verdict: " + ("every hash equal between parent and head" if ok else "MISS"))
    text = "\n".join(lines)
    print(text)
    if log:
        open(log, "w").write(text + "\n")
    sys.exit(0 if ok else 1)


# leg: (command, switches, time limit of one child in seconds)
LEGS = {
    "bench": (["bench.py", "--gpus", "1", "--steps", "16", "--warmup", "3", "--no-cpu-baseline", "--no-serving-leg", "--no-i8i8-leg"], {}, 420),
    "small": (["profiles/small_batch_latency.py", "1", "8", "64"], {}, 300),
    "dual": (["profiles/small_batch_latency.py", "256"], {"PPLHIP_DUAL_STREAM": "1", "PPLHIP_VERBOSE": "1"}, 300),
}


def figures(leg, out, err):
    if leg == "bench":
        return {"bench.py tokens/s": float([json.loads(ln) for ln in out.split("\n") if ln.startswith("{")][-1]["value"])}
    if leg == "dual" and "two-stream decode" not in err:
        return None   # the schedule under test did not run
    label = "two-stream step" if leg == "dual" else "decode step"
    return {f"{label}, batch {b}, ms": float(ms) for b, ms in re.findall(r"batch (\d+): ([\d.]+) ms/step", out)}


def timing(parent, head, rounds, legs, log):
    lines, ok = ["command: " + " ".join(sys.argv)], True
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    for leg in legs:
        cmd, env, seconds = LEGS[leg]
        lines.append(f"{leg}: python {' '.join(cmd)}" + "".join(f" {k}={v}" for k, v in env.items() if k != "PPLHIP_VERBOSE"))
        series = {"parent": [], "head": []}
        for i in range(rounds):
            for tag, lib in (("parent", parent), ("head", head)):
                print(f"{leg} round {i + 1} of {rounds}: {tag}", file=sys.stderr, flush=True)
                rc, out, err = child(cmd, dict(base, PPLHIP_LIB=os.path.abspath(lib), **env), seconds)
                got = figures(leg, out, err) if rc == 0 else None
                if not got:
                    stop(lines, f"{leg}: {tag} run failed with status {rc}", out, err, log)
                series[tag].append(got)
        for key in series["parent"][0]:
            tp, th = [x[key] for x in series["parent"]], [x[key] for x in series["head"]]
            spread, dm = max(tp) - min(tp), statistics.median(th) - statistics.median(tp)
            ok &= abs(dm) <= spread
            lines.append(f"  {key}: parent {tp} head {th} | parent median {statistics.median(tp)} spread {spread:.3f} head - parent {dm:+.3f} | "
                         f"{'ok' if abs(dm) <= spread else 'MISS'}")
        if log:   # (kept up to date leg by leg)
            open(log, "w").write("\n".join(lines) + "\n")
    lines.append("verdict: " + ("every head median within the parent's spread" if ok else "MISS"))
    text = "\n".join(lines)
    print(text)
    if log:
        open(log, "w").write(text + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ab", nargs=2, metavar=("PARENT_LIB", "HEAD_LIB"))
    ap.add_argument("--timing", nargs=2, metavar=("PARENT_LIB", "HEAD_LIB"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="bench,small,dual", help="--timing: which of " + ", ".join(LEGS))
    ap.add_argument("--log")
    ap.add_argument("--cases", help="comma-separated case names (default: all)")
    ap.add_argument("--case", choices=sorted(CASES), help="one build, one case (the switches are the caller's)")
    a = ap.parse_args()
    if a.ab:
        ab(a.ab[0], a.ab[1], a.cases.split(",") if a.cases else None, a.log)
    elif a.timing:
        timing(a.timing[0], a.timing[1], a.rounds, a.legs.split(","), a.log)
    elif a.case:
        run_case(a.case)
    else:
        ap.error("--ab, --timing or --case")
