#!/usr/bin/env python3
"""What top-N logprobs cost (csrc/k_logprobs.hip), in ONE process and one build, the forms alternated in three rounds: B = 1024 rows of
V = 32000 logits, stride 32000, n = 20.  Device time between two events on the stream around ONE call, median of CALLS calls per round,
then the median and the spread (max - min) over the rounds.
  operator level:
    tl_all / tl_512 / tl_1   pplhip_op_top_logprobs with n = 20 on all rows / on every second row / on row 0 alone (the others n = 0)
    old_topk50               the yardstick: pplhip_op_sample with top_k = 50 on the same logits (the sampler's kernel, untouched)
    bar: tl_all <= old_topk50 + max(spread of tl_all, spread of old_topk50).  pplhip_op_top_logprobs takes a DEVICE num_logprobs and has to
         read it back to make its row list, so its event span holds two host round trips that the kernel itself does not need
         (pplhip_op_sample has none); the product entry point has the array on the host.
  product level (host clock around the calls a step makes, which end in the sampler's synchronisation):
    product_rows             pplhip_sample_rows alone (top_k 50)
    product_tl_all_rows / product_tl_1_rows    pplhip_top_logprobs (all rows / row 0 asking) and then pplhip_sample_rows: the asynchronous
                             form adds its device work to the one synchronisation, not a synchronisation of its own
    product_tl_none_rows     nobody asks: pplhip_top_logprobs makes no device call
Writes one JSON line per (form, round), one summary line per form and one line for the bar to profiles/top_logprobs_time.jsonl.
usage: python profiles/top_logprobs_time.py"""
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
B, V, N, ROUNDS, CALLS, WARM = 1024, 32000, 20, 3, 20, 3
OUT = os.path.join(ROOT, "profiles", "top_logprobs_time.jsonl")

rng = np.random.RandomState(0)
logits = torch.from_numpy((rng.randn(B, V) * 2.0).astype(np.float32)).cuda()
NLP = {"all": np.full(B, N, np.int32), "512": np.where(np.arange(B) % 2 == 0, N, 0).astype(np.int32),
       "1": np.where(np.arange(B) == 0, N, 0).astype(np.int32), "none": np.zeros(B, np.int32)}
d_nlp = {n: torch.from_numpy(v).cuda() for n, v in NLP.items()}
top_k = np.full(B, 50, np.int32)
top_p = np.full(B, 0.9, np.float32)
temps = np.full(B, 0.8, np.float32)
seeds = rng.randint(1, 2 ** 62, size=B).astype(np.uint64)
draws = rng.randint(0, 4096, size=B).astype(np.uint64)
d_p, d_t = torch.from_numpy(top_p).cuda(), torch.from_numpy(temps).cuda()
d_r = torch.rand(B, device="cuda") * 0.999
d_tok = torch.zeros(B, dtype=torch.int32, device="cuda")
d_lp = torch.zeros(B, dtype=torch.float32, device="cuda")
d_ttok = torch.zeros(B * m.TOP_LOGPROBS_MAX, dtype=torch.int32, device="cuda")
d_tlp = torch.zeros(B * m.TOP_LOGPROBS_MAX, dtype=torch.float32, device="cuda")

desc = ref.make_desc(hidden_dim=256, intermediate_dim=512, num_layers=1, num_heads=4, num_kv_heads=4, vocab_size=V, max_position=256,
                     cache_quant_bit=0, cache_quant_group=1, cache_layout=3, cache_mode=0)
ctx = m.Context(m.copy_desc(desc), max_running_batch=B, max_tokens_per_step=B)


def op_tl(name):
    return lambda: L.pplhip_op_top_logprobs(None, logits.data_ptr(), d_t.data_ptr(), d_nlp[name].data_ptr(), B, V, V, d_ttok.data_ptr(),
                                            d_tlp.data_ptr())


def product(name):
    def f():
        if name:
            ctx.top_logprobs(NLP[name], temps, logits_ptr=logits.data_ptr())
        ctx.sample_rows(top_k, top_p, seeds, draws, temps, logits_ptr=logits.data_ptr())
    return f


DEVICE_FORMS = {"tl_all": op_tl("all"), "tl_512": op_tl("512"), "tl_1": op_tl("1"),
                "old_topk50": lambda: L.pplhip_op_sample(None, logits.data_ptr(), d_t.data_ptr(), d_p.data_ptr(), d_r.data_ptr(), B, V, V, 50, 0.9,
                                                         d_tok.data_ptr(), d_lp.data_ptr())}
HOST_FORMS = {"product_rows": product(None), "product_tl_all_rows": product("all"), "product_tl_1_rows": product("1"),
              "product_tl_none_rows": product("none")}


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
    lines.append(dict(form=n, summary=True, us=round(s["us"], 2), spread_us=round(s["spread"], 2), B=B, V=V, n=N))
margin = max(summary["tl_all"]["spread"], summary["old_topk50"]["spread"])
limit = summary["old_topk50"]["us"] + margin
lines.append(dict(bar="tl_all <= old_topk50 + larger spread", us=round(summary["tl_all"]["us"], 2), limit_us=round(limit, 2),
                  margin_us=round(margin, 2), met=bool(summary["tl_all"]["us"] <= limit)))
with open(OUT, "w") as fh:
    for ln in lines:
        fh.write(json.dumps(ln) + "\n")
        if "round" not in ln:
            print(json.dumps(ln))
ctx.close()
