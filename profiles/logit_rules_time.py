#!/usr/bin/env python3
"""What the logit rules edit costs (csrc/k_logit_rules.hip) at the operator level, in ONE process and one build, the legs alternated in
rounds: B = 1024 rows of V = 32000 logits, stride 32000.  Device time between two events on the stream around ONE call that is followed
by a synchronise; the logits are restored from a pristine copy in front of the first event, so every call edits the same values.  Every
leg is warmed up in every round; ROUNDS x CALLS = 200 timed calls per leg; the median over all of them, and the spread (max - min) of the
per-round medians.
    penalty       the yardstick: pplhip_op_penalty on a decode step of the same batch (reads and writes every row, reads a 64 KB count map
                  row per request)
    edit_a        pplhip_op_logit_edit, every row with a mask of 1000 allowed tokens and 300 biases, flags 1, a device row list
    edit_b        the same with 300 biases and no mask
    edit_c        one asking row of the 1024 (the rule of leg a)
    edit_a_readback   leg a without a row list: the operator reads the flags back and sends the list up, two host round trips
  expectation: edit_a and edit_b at or below penalty.
Writes one JSON line per (leg, round), one summary line per leg and one line per expectation to profiles/logit_rules_time.jsonl.
usage: python profiles/logit_rules_time.py            (the timing)
       python profiles/logit_rules_time.py --trace    (20 untimed calls per leg, for a kernel trace taken in a run of its own)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import logit_rules as R  # noqa: E402
from tests.conftest import load_pplhip  # noqa: E402

m = load_pplhip()
L = m.lib()
B, V, ROUNDS, CALLS, WARM = 1024, 32000, 4, 50, 3
OUT = os.path.join(ROOT, "profiles", "logit_rules_time.jsonl")
TRACE = "--trace" in sys.argv

rng = np.random.default_rng(0)
pristine = torch.from_numpy((rng.standard_normal((B, V)) * 2.0).astype(np.float32)).cuda()
work = torch.empty_like(pristine)
W = R.words(V)


def table(with_mask):
    head = np.zeros((B, 4), dtype=np.int32)
    bt = np.zeros((B, R.BIAS_MAX), dtype=np.int32)
    bv = np.zeros((B, R.BIAS_MAX), dtype=np.float32)
    st = np.zeros((B, R.STOP_MAX), dtype=np.int32)
    mk = np.zeros((B, W), dtype=np.uint32)
    for s in range(B):
        head[s] = (300, 0, int(with_mask), 0)
        bt[s, :300] = rng.choice(V, size=300, replace=False)
        bv[s, :300] = rng.uniform(-4, 4, size=300)
        if with_mask:
            mk[s] = R.pack_mask(rng.choice(V, size=1000, replace=False).tolist(), V)
    return [torch.from_numpy(a.view(np.int32)).cuda() for a in (head, bt, bv, st, mk)]


TAB = {True: table(True), False: table(False)}
slots = torch.from_numpy(rng.permutation(B).astype(np.int32)).cuda()
all_rows = torch.arange(B, dtype=torch.int32, device="cuda")
flags_all = torch.ones(B, dtype=torch.int32, device="cuda")
flags_one = torch.zeros(B, dtype=torch.int32, device="cuda")
flags_one[517] = 1
row_one = torch.tensor([517], dtype=torch.int32, device="cuda")

# the penalty's decode step: one token per row, nothing cleared
p_slots = torch.from_numpy(rng.permutation(B).astype(np.int64)).cuda()
p_tok = torch.from_numpy(rng.integers(0, V, size=B).astype(np.int64)).cuda()
p_seq = torch.arange(B + 1, dtype=torch.int64, device="cuda")
p_sp = torch.full((B,), 17, dtype=torch.int64, device="cuda")
p_t = torch.full((B,), 0.8, dtype=torch.float32, device="cuda")
p_rep = torch.full((B,), 1.2, dtype=torch.float32, device="cuda")
p_pres = torch.full((B,), 0.1, dtype=torch.float32, device="cuda")
p_freq = torch.full((B,), 0.05, dtype=torch.float32, device="cuda")
count_map = torch.from_numpy((rng.random((B, V)) < 0.02).astype(np.int16)).cuda()   # 2 % of the tokens counted once


def edit(with_mask, flags, rows, n_rows):
    t = TAB[with_mask]
    return lambda: L.pplhip_op_logit_edit(None, work.data_ptr(), V, V, B, flags.data_ptr(), slots.data_ptr(), *[p.data_ptr() for p in t],
                                          None if rows is None else rows.data_ptr(), n_rows)


LEGS = {
    "penalty": lambda: L.pplhip_op_penalty(None, work.data_ptr(), p_t.data_ptr(), p_rep.data_ptr(), p_pres.data_ptr(), p_freq.data_ptr(),
                                           p_slots.data_ptr(), p_tok.data_ptr(), p_seq.data_ptr(), p_sp.data_ptr(), B, V, V, B,
                                           count_map.data_ptr()),
    "edit_a": edit(True, flags_all, all_rows, B),
    "edit_b": edit(False, flags_all, all_rows, B),
    "edit_c": edit(True, flags_one, row_one, 1),
    "edit_a_readback": edit(True, flags_all, None, 0),
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


if TRACE:
    for name, f in LEGS.items():
        for _ in range(20):
            work.copy_(pristine)
            assert f() == 0
        torch.cuda.synchronize()
    sys.exit(0)

lines, calls, medians = [], {}, {}
for rnd in range(ROUNDS):
    for name, f in LEGS.items():
        for _ in range(WARM):
            device_us(f)
        us = [device_us(f) for _ in range(CALLS)]
        calls.setdefault(name, []).extend(us)
        medians.setdefault(name, []).append(float(np.median(us)))
        lines.append(dict(leg=name, round=rnd, us=round(medians[name][-1], 2)))
summary = {n: dict(us=float(np.median(v)), spread=float(max(medians[n]) - min(medians[n]))) for n, v in calls.items()}
for n, s in summary.items():
    lines.append(dict(leg=n, summary=True, us=round(s["us"], 2), spread_us=round(s["spread"], 2), calls=len(calls[n]), B=B, V=V))
for leg in ("edit_a", "edit_b"):
    lines.append(dict(expectation=f"{leg} <= penalty", us=round(summary[leg]["us"], 2), limit_us=round(summary["penalty"]["us"], 2),
                      met=bool(summary[leg]["us"] <= summary["penalty"]["us"])))
with open(OUT, "w") as fh:
    for ln in lines:
        fh.write(json.dumps(ln) + "\n")
        if "round" not in ln:
            print(json.dumps(ln))
