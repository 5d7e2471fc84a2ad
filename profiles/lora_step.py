#!/usr/bin/env python3
"""What per-request LoRA adapters cost a step: one process, LLaMA-2-7B geometry, W8A16 weights, int8-g8 KV, synthetic weights and a
synthetic slab (pplhip_kv_fill_synthetic), the cases alternated over three rounds:
  none          no slot loaded                                   (today's step)
  loaded        64 slots loaded, none assigned                   (must equal `none`)
  one_r16       batch 1024, every row on one adapter, q / k / v rank 16 fused to 48, wo / w2 rank 16
  rr8 / rr64    batch 1024, 8 / 64 such adapters round-robin over the rows
  b64_rr8       batch 64, 8 adapters round-robin
  prefill8192   one 8192-token prompt on one adapter
Per case: the step in ms (host clock around set_inputs + set_adapters + run + sync, profiling off), the summed time of the two adapter
kernels per step (a second pass with the runtime profiler's event pairs around every launch_lora: PPLHIP_PROF_LORA), the byte floor of
those launches at 8 TB/s -- per tile the slot's A and B once, 16 rows of x read, 16 rows of y read and written -- and the spread
(max - min) between the rounds.  Prints one JSON line per (case, round) and one summary line per case.
--bench-parent LIB: instead, the headline path against the parent commit: bench.py --gpus 1 --steps 16 --warmup 3 as child processes,
this tree's library and LIB (the parent's libpplhip.so, built in a scratch directory; PPLHIP_LIB) alternated over three rounds, in both
orders of a pair (the chip runs at its power limit: the order of a pair is not neutral); one JSON line per run and one summary line.
usage: python profiles/lora_step.py [case ...] | --bench-parent LIB"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref  # noqa: E402
from tests.conftest import load_pplhip  # noqa: E402

m = load_pplhip()
MODEL = dict(hidden_dim=4096, intermediate_dim=11008, num_layers=32, num_heads=32, num_kv_heads=32, vocab_size=32000)
PEAK = 8e12
CASES = {
    "none": dict(B=1024, load=0, assign=0),
    "loaded": dict(B=1024, load=64, assign=0),
    "one_r16": dict(B=1024, load=1, assign=1),
    "rr8": dict(B=1024, load=8, assign=8),
    "rr64": dict(B=1024, load=64, assign=64),
    "b64_rr8": dict(B=64, load=8, assign=8),
    "prefill8192": dict(B=1, T=8192, load=1, assign=1),
}
R_QKV, R_WO, R_W2 = 48, 16, 16


def adapter(rng):
    hd, inter, L = MODEL["hidden_dim"], MODEL["intermediate_dim"], MODEL["num_layers"]
    t = {}
    for l in range(L):
        for name, r, n, k in (("attention.wqkv", R_QKV, 3 * hd, hd), ("attention.wo", R_WO, hd, hd), ("feed_forward.w2", R_W2, hd, inter)):
            t[f"layers.{l}.{name}.lora_a"] = (rng.standard_normal((r, k)) * 0.01).astype(np.float16)
            t[f"layers.{l}.{name}.lora_b"] = (rng.standard_normal((n, r)) * 0.01).astype(np.float16)
    return t


def floor_bytes(row_slots):
    """bytes the adapter launches of ONE step must move: per tile A and B of its slot once, x read, y read and written"""
    hd, inter, L = MODEL["hidden_dim"], MODEL["intermediate_dim"], MODEL["num_layers"]
    kp = (inter + 63) // 64 * 64
    tiles = sum(((row_slots == s).sum() + 15) // 16 for s in set(row_slots[row_slots >= 0].tolist()))
    rows = int((row_slots >= 0).sum())
    per_layer = 0
    for r, n, k in ((R_QKV, 3 * hd, hd), (R_WO, hd, hd), (R_W2, hd, kp)):
        per_layer += tiles * (r * k * 2 + n * r * 2) + rows * (k * 2 + 2 * n * 2)
    return per_layer * L


def one(case, rnd, tensors, warm=2, steps=5):
    c = CASES[case]
    B, T = c["B"], c.get("T", c["B"])
    prefill = T != B
    out = {}
    for profiling in (0, 1):
        desc = ref.make_desc(max_position=16384 if prefill else 4096, cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=0,
                             weight_quant_bit=8, **MODEL)
        ctx = m.Context(m.copy_desc(desc), max_running_batch=max(B, 8), max_tokens_per_step=T, profiling=profiling)
        ctx.init_synthetic(0, 1)
        kv = 0 if prefill else 512
        per = T + 8 if prefill else kv + warm + steps + 2
        ctx.kv_alloc(0, B * per)
        ctx.kv_fill_synthetic(0, 3)
        for s in range(c["load"]):
            ctx.lora_set(0, s, tensors, 2.0)
        slots = (np.arange(B) % c["assign"]).astype(np.int32) if c["assign"] else None
        ci = np.arange(B, dtype=np.int64) * per
        tok = np.random.RandomState(0).randint(3, 32000, size=T).astype(np.int64)
        ss = np.array([0, T], dtype=np.int64) if prefill else np.arange(B + 1, dtype=np.int64)
        ms, lora_ms = [], []
        for i in range(warm + steps):
            sp = np.zeros(B, np.int64) if prefill else np.full(B, kv + i, np.int64)
            st = m.make_step(tok, ss, sp, ci, 0 if prefill else B, req_list_changed=int(i == 0))
            if profiling:
                ctx.profile_reset(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.set_inputs(0, st)
            if slots is not None:
                ctx.set_adapters(0, slots)
            ctx.run(0)
            ctx.sync(0)
            t1 = time.perf_counter()
            if i >= warm:
                ms.append((t1 - t0) * 1e3)
                if profiling:
                    lora_ms.append(ctx.profile_get(m.PROF_LORA, 0))
        ctx.close()
        torch.cuda.empty_cache()
        if profiling:
            out["lora_launch_pairs"] = int(lora_ms[0][0])
            out["lora_ms"] = round(float(np.median([x[1] for x in lora_ms])), 4)
        else:
            out["step_ms"] = round(float(np.median(ms)), 3)
    row_slots = np.full(T, -1, dtype=np.int32) if slots is None else np.repeat(slots, T // B)
    fb = floor_bytes(row_slots)
    row = {"what": "round", "case": case, "round": rnd, "B": B, "T": T, **out, "floor_bytes": int(fb), "floor_ms_at_8TBps": round(fb / PEAK * 1e3, 4)}
    print(json.dumps(row), flush=True)
    return row


def bench_parent(parent_lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = []
    for order in (("head", "parent"), ("parent", "head")):
        for rnd in range(3):
            for build in order:
                env = dict(os.environ)
                env.pop("PPLHIP_LIB", None)
                if build == "parent":
                    env["PPLHIP_LIB"] = os.path.abspath(parent_lib)
                out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "16", "--warmup", "3", "--no-cpu-baseline",
                                      "--no-serving-leg", "--no-i8i8-leg"], env=env, cwd=root, capture_output=True, text=True, timeout=600, check=True).stdout
                r = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
                rows.append({"what": "bench.py --gpus 1 --steps 16 --warmup 3 (headline decode step, no adapters)", "build": build,
                             "order": order[0] + " first", "round": rnd, "ms_per_step": r["ms_per_step"], "tokens_per_s": r["value"]})
                print(json.dumps(rows[-1]), flush=True)
    ms = {b: np.array([r["ms_per_step"] for r in rows if r["build"] == b]) for b in ("head", "parent")}
    print(json.dumps({"what": "bench summary", "head_ms_per_step_median": round(float(np.median(ms["head"])), 3),
                      "parent_ms_per_step_median": round(float(np.median(ms["parent"])), 3),
                      "head_spread": round(float(ms["head"].max() - ms["head"].min()), 3),
                      "parent_spread": round(float(ms["parent"].max() - ms["parent"].min()), 3),
                      "difference_within_spread": bool(abs(np.median(ms["head"]) - np.median(ms["parent"])) <=
                                                       max(ms["head"].max() - ms["head"].min(), ms["parent"].max() - ms["parent"].min()))}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--bench-parent":
        bench_parent(sys.argv[2])
        sys.exit(0)
    cases = sys.argv[1:] or list(CASES)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "time": time.strftime("%Y-%m-%dT%H:%M:%S")}), flush=True)
    tensors = adapter(np.random.RandomState(0))
    rows = {c: [] for c in cases}
    for rnd in range(3):
        for c in cases:
            rows[c].append(one(c, rnd, tensors))
    for c, rr in rows.items():
        t = np.array([r["step_ms"] for r in rr])
        k = np.array([r["lora_ms"] for r in rr])
        print(json.dumps({"what": "summary", "case": c, "step_ms": round(float(np.median(t)), 3), "step_ms_spread": round(float(t.max() - t.min()), 3),
                          "lora_ms": round(float(np.median(k)), 4), "lora_ms_spread": round(float(k.max() - k.min()), 4),
                          "floor_ms_at_8TBps": rr[0]["floor_ms_at_8TBps"],
                          "lora_over_floor": None if not rr[0]["floor_bytes"] else round(float(np.median(k)) / rr[0]["floor_ms_at_8TBps"], 2)}), flush=True)
