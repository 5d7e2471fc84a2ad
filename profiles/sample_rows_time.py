#!/usr/bin/env python3
"""What the per-request sampler costs (csrc/k_sample_rows.hip), in ONE process and one build, the forms alternated in three rounds:
B = 1024 rows of V = 32000 logits, stride 32000.  Device time between two events on the stream around ONE call, median of CALLS calls per
round, then the median and the spread (max - min) over the rounds.
  operator level (the issue's bars):
    rows_greedy / rows_topk50 / rows_half   pplhip_op_sample_rows, all top_k 1 / all top_k 50 / rows alternating 1 and 50
    old_greedy / old_topk50                 pplhip_op_sample of the same build (top_k 1 / 50, per-row top_p and rnd)
    old_greedy_b512 / old_topk50_b512       the same on 512 rows: what the two launches of rows_half are made of (a row kernel that is bound
                                            by its own latency does not take half the time for half the rows)
    launch                                  the smallest launch the library has (pplhip_op_sample_uniform on one row) as the empty kernel
    bars: rows_greedy <= old_greedy + margin, rows_topk50 <= old_topk50 + margin, rows_half <= (old_greedy + old_topk50) / 2 + margin,
          margin = max(largest spread of the forms in the bar, launch).  pplhip_op_sample_rows takes DEVICE arrays and has to read top_k
          back to make its row list, so its event span holds two host round trips that the kernels themselves do not need;
  product level (for information: the entry points a backend calls, host arrays, one synchronisation each, host clock around the call):
    product_rows_*  pplhip_sample_rows,  product_old_*  pplhip_sample.
Writes one JSON line per (form, round), one summary line per form and one line per bar to profiles/sample_rows_time.jsonl.
usage: python profiles/sample_rows_time.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref  # noqa: E402
from tests.conftest import load_pplhip  # noqa: E402

m = load_pplhip()
L = m.lib()
B, V, ROUNDS, CALLS, WARM = 1024, 32000, 3, 20, 3
OUT = os.path.join(ROOT, "profiles", "sample_rows_time.jsonl")

rng = np.random.RandomState(0)
logits = torch.from_numpy((rng.randn(B, V) * 2.0).astype(np.float32)).cuda()
K = {"greedy": np.ones(B, np.int32), "topk50": np.full(B, 50, np.int32), "half": np.where(np.arange(B) % 2 == 0, 1, 50).astype(np.int32)}
d_k = {n: torch.from_numpy(k).cuda() for n, k in K.items()}
top_p = np.full(B, 0.9, np.float32)
temps = np.full(B, 0.8, np.float32)
seeds = rng.randint(1, 2 ** 62, size=B).astype(np.uint64)
draws = rng.randint(0, 4096, size=B).astype(np.uint64)
d_p, d_t = torch.from_numpy(top_p).cuda(), torch.from_numpy(temps).cuda()
d_s, d_n = torch.from_numpy(seeds.view(np.int64)).cuda(), torch.from_numpy(draws.view(np.int64)).cuda()
d_r = torch.rand(B, device="cuda") * 0.999
d_tok = torch.zeros(B, dtype=torch.int32, device="cuda")
d_lp = torch.zeros(B, dtype=torch.float32, device="cuda")
d_u = torch.zeros(8, dtype=torch.float32, device="cuda")

desc = ref.make_desc(hidden_dim=256, intermediate_dim=512, num_layers=1, num_heads=4, num_kv_heads=4, vocab_size=V, max_position=256,
                     cache_quant_bit=0, cache_quant_group=1, cache_layout=3, cache_mode=0)
ctx = m.Context(m.copy_desc(desc), max_running_batch=B, max_tokens_per_step=B)


def op_rows(name):
    return lambda: L.pplhip_op_sample_rows(None, logits.data_ptr(), d_t.data_ptr(), d_k[name].data_ptr(), d_p.data_ptr(), d_s.data_ptr(),
                                           d_n.data_ptr(), None, B, V, V, d_tok.data_ptr(), d_lp.data_ptr())


def op_old(top_k, batch=B):
    return lambda: L.pplhip_op_sample(None, logits.data_ptr(), d_t.data_ptr(), d_p.data_ptr(), d_r.data_ptr(), batch, V, V, top_k, 0.9,
                                      d_tok.data_ptr(), d_lp.data_ptr())


DEVICE_FORMS = {"rows_greedy": op_rows("greedy"), "rows_topk50": op_rows("topk50"), "rows_half": op_rows("half"),
                "old_greedy": op_old(1), "old_topk50": op_old(50), "old_greedy_b512": op_old(1, B // 2), "old_topk50_b512": op_old(50, B // 2),
                "launch": lambda: L.pplhip_op_sample_uniform(None, d_s.data_ptr(), d_n.data_ptr(), 1, d_u.data_ptr())}
HOST_FORMS = {"product_rows_greedy": lambda: ctx.sample_rows(K["greedy"], top_p, seeds, draws, temps, logits_ptr=logits.data_ptr()),
              "product_rows_topk50": lambda: ctx.sample_rows(K["topk50"], top_p, seeds, draws, temps, logits_ptr=logits.data_ptr()),
              "product_rows_half": lambda: ctx.sample_rows(K["half"], top_p, seeds, draws, temps, logits_ptr=logits.data_ptr()),
              "product_old_greedy": lambda: ctx.sample(B, top_k=1, temperatures=temps, top_p_list=top_p, logits_ptr=logits.data_ptr()),
              "product_old_topk50": lambda: ctx.sample(B, top_k=50, top_p=0.9, temperatures=temps, top_p_list=top_p, logits_ptr=logits.data_ptr())}


def device_us(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    rc = f()
    e1.record()
    torch.cuda.synchronize()
    assert rc == 0, rc
    return e0.elapsed_time(e1) * 1e3


def host_us(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e6


lines, per_form = [], {}
for rnd in range(ROUNDS):
    for forms, timer in ((DEVICE_FORMS, device_us), (HOST_FORMS, host_us)):
        for name, f in forms.items():
            for _ in range(WARM):
                timer(f)
            us = float(np.median([timer(f) for _ in range(CALLS)]))
            per_form.setdefault(name, []).append(us)
            lines.append(dict(form=name, round=rnd, us=round(us, 2)))
summary = {n: dict(us=float(np.median(v)), spread=float(max(v) - min(v))) for n, v in per_form.items()}
for n, s in summary.items():
    lines.append(dict(form=n, summary=True, us=round(s["us"], 2), spread_us=round(s["spread"], 2), B=B, V=V))


def bar(name, new, olds, weights):
    margin = max([summary[n]["spread"] for n in [new] + olds] + [summary["launch"]["us"]])
    limit = sum(w * summary[o]["us"] for o, w in zip(olds, weights)) + margin
    lines.append(dict(bar=name, us=round(summary[new]["us"], 2), limit_us=round(limit, 2), margin_us=round(margin, 2),
                      met=bool(summary[new]["us"] <= limit)))


bar("rows_greedy <= old_greedy + margin", "rows_greedy", ["old_greedy"], [1.0])
bar("rows_topk50 <= old_topk50 + margin", "rows_topk50", ["old_topk50"], [1.0])
bar("rows_half <= (old_greedy + old_topk50) / 2 + margin", "rows_half", ["old_greedy", "old_topk50"], [0.5, 0.5])
with open(OUT, "w") as fh:
    for ln in lines:
        fh.write(json.dumps(ln) + "\n")
        if "round" not in ln:
            print(json.dumps(ln))
ctx.close()
