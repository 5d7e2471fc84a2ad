#!/usr/bin/env python3
"""What prompt logprobs cost (csrc/k_prompt_logprobs.hip), in ONE process and one build, the legs alternated in rounds.

Kernel, operator level: 1024 rows of V = 32000 logits, stride 32000.  Device time between two events on the stream around ONE call that is
followed by a synchronise; every leg is warmed up in every round; ROUNDS x CALLS timed calls per leg; the median over all of them and the
spread (max - min) of the per-round medians.
    top_logprobs_n1   the yardstick: pplhip_op_top_logprobs, n = 1 on every row (two row passes for maximum and mass, four radix rounds,
                      one gather); the operator reads num_logprobs back and sends a row list up: two host round trips inside the span
    prompt_n0         pplhip_op_prompt_logprobs, n = 0 on every row (two row passes); the operator reads rows and n_top back: one host
                      round trip inside the span
    prompt_n1         the same with n = 1: both row functions on every row
  expectation: prompt_n0 <= top_logprobs_n1.

Step: a synthetic fp16 model (hidden 4096, 2 layers, V = 32000: the feature's cost does not depend on the depth), max_running_batch 1024,
one prefill step of 4 prompts of 512 tokens, host clock around set_inputs .. copy_logits (the synchronisation):
    step_plain        nobody asks: today's step
    step_ask_n0       every prompt asks, n = 0: 2044 positions in two chunks of 1024 and 1020 rows
    step_ask_n20      the same, n = 20
    lm_head_1024      pplhip_op_linear alone, M = 1024, K = 4096, N = 32000, fp32 out (device time): the GEMM a chunk adds
  reported: step_ask - step_plain and the share of it that two such GEMMs are.  No bar: the GEMM over the 2044 extra rows is inherent.

Writes one JSON line per (leg, round), one summary line per leg and the derived lines to profiles/prompt_logprobs_time.jsonl.
usage: python profiles/prompt_logprobs_time.py"""
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
B, V, ROUNDS, CALLS, WARM = 1024, 32000, 4, 50, 3
OUT = os.path.join(ROOT, "profiles", "prompt_logprobs_time.jsonl")

rng = np.random.default_rng(0)
logits = torch.from_numpy((rng.standard_normal((B, V)) * 2.0).astype(np.float32)).cuda()
tokens = torch.from_numpy(rng.integers(0, V, size=B + 1).astype(np.int64)).cuda()
rows = torch.arange(B, dtype=torch.int32, device="cuda")
n0 = torch.zeros(B, dtype=torch.int32, device="cuda")
n1 = torch.ones(B, dtype=torch.int32, device="cuda")
o_lp = torch.empty(B, dtype=torch.float32, device="cuda")
o_rank = torch.empty(B, dtype=torch.int32, device="cuda")
o_tok = torch.empty((B, 20), dtype=torch.int32, device="cuda")
o_tlp = torch.empty((B, 20), dtype=torch.float32, device="cuda")

HID = 4096
x = torch.from_numpy((rng.standard_normal((B, HID)) * 0.5).astype(np.float16)).cuda()
w = torch.from_numpy((rng.standard_normal((V, HID)) * 0.02).astype(np.float16)).cuda()
y = torch.empty((B, V), dtype=torch.float32, device="cuda")


def prompt_op(n):
    return lambda: L.pplhip_op_prompt_logprobs(None, logits.data_ptr(), V, V, rows.data_ptr(), B, tokens.data_ptr(), B + 1, n.data_ptr(),
                                               o_lp.data_ptr(), o_rank.data_ptr(), o_tok.data_ptr(), o_tlp.data_ptr())


KERNEL_LEGS = {
    "top_logprobs_n1": lambda: L.pplhip_op_top_logprobs(None, logits.data_ptr(), None, n1.data_ptr(), B, V, V, o_tok.data_ptr(), o_tlp.data_ptr()),
    "prompt_n0": prompt_op(n0),
    "prompt_n1": prompt_op(n1),
    "lm_head_1024": lambda: L.pplhip_op_linear(None, x.data_ptr(), w.data_ptr(), None, 0, 0, B, V, HID, y.data_ptr(), 1),
}


def device_us(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    rc = f()
    e1.record()
    torch.cuda.synchronize()
    assert rc == 0, rc
    return e0.elapsed_time(e1) * 1e3


# ---- the step
NP, PL = 4, 512
desc = ref.make_desc(hidden_dim=HID, intermediate_dim=11008, num_layers=2, num_heads=32, num_kv_heads=32, vocab_size=V, max_position=2048,
                     cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=0, weight_quant_bit=0)
ctx = m.Context(m.copy_desc(desc), max_running_batch=1024, max_tokens_per_step=4096)
ctx.init_synthetic(0, 11)
ctx.kv_alloc(0, NP * 1024)
s_tok = rng.integers(3, V, size=NP * PL).astype(np.int64)
s_seq = np.arange(NP + 1, dtype=np.int64) * PL
s_idx = np.arange(NP, dtype=np.int64) * 1024


def step(ask):
    def f():
        t0 = time.perf_counter()
        ctx.set_inputs(0, m.make_step(s_tok, s_seq, np.zeros(NP, dtype=np.int64), s_idx, 0, req_list_changed=1))
        if ask is not None:
            ctx.set_prompt_logprobs(0, np.full(NP, ask, dtype=np.int32))
        ctx.run(0)
        ctx.copy_logits(NP)
        us = (time.perf_counter() - t0) * 1e6
        assert ctx.prompt_logprobs(0)[0].size == (0 if ask is None else NP * (PL - 1))
        return us
    return f


STEP_LEGS = {"step_plain": step(None), "step_ask_n0": step(0), "step_ask_n20": step(20)}

lines, calls, medians = [], {}, {}
for rnd in range(ROUNDS):
    for name, f in KERNEL_LEGS.items():
        for _ in range(WARM):
            device_us(f)
        us = [device_us(f) for _ in range(CALLS)]
        calls.setdefault(name, []).extend(us)
        medians.setdefault(name, []).append(float(np.median(us)))
        lines.append(dict(leg=name, round=rnd, us=round(medians[name][-1], 2)))
    for name, f in STEP_LEGS.items():
        for _ in range(WARM):
            f()
        us = [f() for _ in range(CALLS // 2)]
        calls.setdefault(name, []).extend(us)
        medians.setdefault(name, []).append(float(np.median(us)))
        lines.append(dict(leg=name, round=rnd, us=round(medians[name][-1], 2)))
summary = {n: dict(us=float(np.median(v)), spread=float(max(medians[n]) - min(medians[n]))) for n, v in calls.items()}
for n, s in summary.items():
    lines.append(dict(leg=n, summary=True, us=round(s["us"], 2), spread_us=round(s["spread"], 2), calls=len(calls[n])))
lines.append(dict(expectation="prompt_n0 <= top_logprobs_n1", us=round(summary["prompt_n0"]["us"], 2),
                  limit_us=round(summary["top_logprobs_n1"]["us"], 2), met=bool(summary["prompt_n0"]["us"] <= summary["top_logprobs_n1"]["us"])))
for leg in ("step_ask_n0", "step_ask_n20"):
    extra = summary[leg]["us"] - summary["step_plain"]["us"]
    lines.append(dict(derived=f"{leg} - step_plain", extra_us=round(extra, 1), positions=NP * (PL - 1), chunks=2,
                      lm_head_share=round(2 * summary["lm_head_1024"]["us"] / extra, 3)))
with open(OUT, "w") as fh:
    for ln in lines:
        fh.write(json.dumps(ln) + "\n")
        if "round" not in ln:
            print(json.dumps(ln))
ctx.close()
