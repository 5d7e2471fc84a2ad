#!/usr/bin/env python3
"""int8-g8 vs fp8 vs int4-g32 KV cache on the same device, in ONE process and one build, the formats alternated in three rounds:
the decode-attention launch time (profiling mode 2: start / stop stamps of the kernel's own dispatch packet) and the whole decode step
(host clock around set_inputs + run + sync), synthetic weights and a synthetic slab, at
  * 7b_b1024: bench.py's own shape -- LLaMA-2-7B W8A16, batch 1024, 24 timed steps from position 514 on (kv 515 .. 538; multi-head decode kernel);
  * gqa_b256_kv2048: LLaMA-2-70B's attention geometry per rank of TP 8 (8 query heads on 1 KV head of 128) in a stand-in model (hidden
    1024, 80 layers: the STEP time is that stand-in's, only the attention launch is the 70B rank's), batch 256, kv 2048 .. (grouped-query kernel);
  * 7b_b64: LLaMA-2-7B, batch 64, kv 512 ..
Per format: the median over the timed steps of each round, then the median and the spread (max - min) over the rounds; the algorithmic
bytes per launch  sum(kv) * 2 * Hkv * row_bytes + B * H * D * 4  with row_bytes 160 / 130 / 72 per 128 channels, and the fraction of 8 TB/s.
Prints one JSON line per (shape, format, round), one summary line per (shape, format) and one ratio line per shape.
usage: python profiles/kv_i4_step.py [shape ...]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref  # noqa: E402
from tests.conftest import load_pplhip  # noqa: E402

m = load_pplhip()
FORMATS = {"int8-g8": (8, 8, 160), "fp8": (8, 128, 130), "int4-g32": (4, 32, 72)}   # (bit, group, bytes per 128-channel row)
SHAPES = {
    "7b_b1024": dict(model=dict(hidden_dim=4096, intermediate_dim=11008, num_layers=32, num_heads=32, num_kv_heads=32, vocab_size=32000),
                     B=1024, kv=512, warm=2, steps=24),
    "gqa_b256_kv2048": dict(model=dict(hidden_dim=1024, intermediate_dim=3584, num_layers=80, num_heads=8, num_kv_heads=1, vocab_size=32000),
                            B=256, kv=2048, warm=2, steps=12),
    "7b_b64": dict(model=dict(hidden_dim=4096, intermediate_dim=11008, num_layers=32, num_heads=32, num_kv_heads=32, vocab_size=32000),
                   B=64, kv=512, warm=2, steps=12),
}
PEAK = 8e12


def one(shape, fmt, rnd):
    s = SHAPES[shape]
    bit, group, rowb = FORMATS[fmt]
    B, kv, warm, steps = s["B"], s["kv"], s["warm"], s["steps"]
    mk = s["model"]
    H, Hkv, D, layers = mk["num_heads"], mk["num_kv_heads"], mk["hidden_dim"] // mk["num_heads"], mk["num_layers"]
    desc = ref.make_desc(max_position=4096, cache_quant_bit=bit, cache_quant_group=group, cache_layout=3, cache_mode=0, weight_quant_bit=8, **mk)
    ctx = m.Context(m.copy_desc(desc), max_running_batch=B, max_tokens_per_step=B, profiling=2)
    ctx.init_synthetic(0, 1)
    per = kv + warm + steps + 2
    ctx.kv_alloc(0, B * per)
    ctx.kv_fill_synthetic(0, 3)
    ci = np.arange(B, dtype=np.int64) * per
    tok = np.random.RandomState(0).randint(3, 32000, size=B).astype(np.int64)
    step_ms, attn_us, frac = [], [], []
    for i in range(warm + steps):
        st = m.make_step(tok, np.arange(B + 1, dtype=np.int64), np.full(B, kv + i, np.int64), ci, B, req_list_changed=int(i == 0))
        ctx.profile_reset(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.set_inputs(0, st)
        ctx.run(0)
        ctx.sync(0)
        t1 = time.perf_counter()
        if i >= warm:
            n, ms = ctx.profile_get(m.PROF_ATTN_DECODE, 0)
            assert n == layers, (n, layers)
            us = ms * 1e3 / n
            nbytes = B * (kv + i + 1) * 2 * Hkv * rowb * D // 128 + B * H * D * 4
            step_ms.append((t1 - t0) * 1e3)
            attn_us.append(us)
            frac.append(nbytes / (us * 1e-6) / PEAK)
    ctx.close()
    torch.cuda.empty_cache()
    row = {"what": "round", "shape": shape, "kv_format": fmt, "round": rnd, "B": B, "kv_first": kv + warm + 1, "kv_last": kv + warm + steps,
           "attn_us_per_launch": round(float(np.median(attn_us)), 2), "step_ms": round(float(np.median(step_ms)), 3),
           "bytes_per_launch_at_kv_last": int(nbytes), "fraction_of_8TBps": round(float(np.median(frac)), 3)}
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    shapes = sys.argv[1:] or list(SHAPES)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "time": time.strftime("%Y-%m-%dT%H:%M:%S")}), flush=True)
    for shape in shapes:
        rows = {f: [] for f in FORMATS}
        for rnd in range(3):
            for fmt in FORMATS:
                rows[fmt].append(one(shape, fmt, rnd))
        summ = {}
        for fmt, rr in rows.items():
            a = np.array([r["attn_us_per_launch"] for r in rr])
            t = np.array([r["step_ms"] for r in rr])
            summ[fmt] = {"what": "summary", "shape": shape, "kv_format": fmt, "attn_us_per_launch": round(float(np.median(a)), 2),
                         "attn_us_spread": round(float(a.max() - a.min()), 2), "step_ms": round(float(np.median(t)), 3),
                         "step_ms_spread": round(float(t.max() - t.min()), 3),
                         "fraction_of_8TBps": round(float(np.median([r["fraction_of_8TBps"] for r in rr])), 3)}
            print(json.dumps(summ[fmt]), flush=True)
        base = summ["int8-g8"]
        for fmt in ("fp8", "int4-g32"):
            print(json.dumps({"what": "ratio_to_int8-g8", "shape": shape, "kv_format": fmt,
                              "attn": round(summ[fmt]["attn_us_per_launch"] / base["attn_us_per_launch"], 3),
                              "step": round(summ[fmt]["step_ms"] / base["step_ms"], 3),
                              "bytes": round(FORMATS[fmt][2] / 160, 3),
                              "attn_faster_by_more_than_spread": bool(base["attn_us_per_launch"] - summ[fmt]["attn_us_per_launch"] >
                                                                      max(base["attn_us_spread"], summ[fmt]["attn_us_spread"]))}), flush=True)
