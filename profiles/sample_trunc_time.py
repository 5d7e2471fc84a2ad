#!/usr/bin/env python3
"""What a truncating row costs (csrc/k_sample_dev.h sample_trunc_row) against sample_rows_topk_topp_kernel on the same 64 rows, in ONE
process and one build, the forms alternated in three rounds: B = 64 rows of V = 32000 and of V = 128256 logits.  Device time between two
events on the stream around ONE call after WARM warm-up calls, median of CALLS calls per round, then the median and the spread
(max - min) over the rounds.  Both entry points read top_k back to make their row list, so every span holds the same two host round trips;
the difference of two forms is the kernels'.
  topk_topp_k50 / topk_topp_full    pplhip_op_sample_rows, top_k 50 / top_k 0 (1024 candidates), top_p 0.9
  minp_* / typical_* / both_*       pplhip_op_sample_rows2 on the same rows with min_p 0.05 / typical_p 0.9 / both
A record, not a bar.  Writes one JSON line per (form, round) and one summary line per form.
usage: python profiles/sample_trunc_time.py [out.jsonl]   (default profiles/sample_trunc.jsonl)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.conftest import load_pplhip  # noqa: E402

m = load_pplhip()
L = m.lib()
B, ROUNDS, CALLS, WARM = 64, 3, 20, 3
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sample_trunc.jsonl")


def device_us(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    rc = f()
    e1.record()
    torch.cuda.synchronize()
    assert rc == 0, rc
    return e0.elapsed_time(e1) * 1e3


lines = []
for V in (32000, 128256):
    rng = np.random.RandomState(V)
    logits = torch.from_numpy((rng.randn(B, V) * 2.0).astype(np.float32)).cuda()
    f32 = lambda v: torch.full((B,), v, dtype=torch.float32, device="cuda")
    d_k = {"k50": torch.full((B,), 50, dtype=torch.int32, device="cuda"), "full": torch.zeros(B, dtype=torch.int32, device="cuda")}
    d_p, d_t, d_mp, d_ty = f32(0.9), f32(0.8), f32(0.05), f32(0.9)
    d_s = torch.from_numpy(rng.randint(1, 2 ** 62, size=B).astype(np.int64)).cuda()
    d_n = torch.from_numpy(rng.randint(0, 4096, size=B).astype(np.int64)).cuda()
    d_tok = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_lp = torch.zeros(B, dtype=torch.float32, device="cuda")

    def rows(k):
        return lambda: L.pplhip_op_sample_rows(None, logits.data_ptr(), d_t.data_ptr(), d_k[k].data_ptr(), d_p.data_ptr(), d_s.data_ptr(),
                                               d_n.data_ptr(), None, B, V, V, d_tok.data_ptr(), d_lp.data_ptr())

    def rows2(k, mp, ty):
        return lambda: L.pplhip_op_sample_rows2(None, logits.data_ptr(), d_t.data_ptr(), d_k[k].data_ptr(), d_p.data_ptr(),
                                                mp.data_ptr() if mp is not None else None, ty.data_ptr() if ty is not None else None,
                                                d_s.data_ptr(), d_n.data_ptr(), None, B, V, V, d_tok.data_ptr(), d_lp.data_ptr())

    forms = {}
    for k in ("k50", "full"):
        forms[f"topk_topp_{k}"] = rows(k)
        forms[f"minp_{k}"] = rows2(k, d_mp, None)
        forms[f"typical_{k}"] = rows2(k, None, d_ty)
        forms[f"both_{k}"] = rows2(k, d_mp, d_ty)
    per_form = {}
    for rnd in range(ROUNDS):
        for name, f in forms.items():
            for _ in range(WARM):
                device_us(f)
            us = float(np.median([device_us(f) for _ in range(CALLS)]))
            per_form.setdefault(name, []).append(us)
            lines.append(dict(form=name, V=V, B=B, round=rnd, us=round(us, 2)))
    for n, v in per_form.items():
        lines.append(dict(form=n, V=V, B=B, summary=True, us=round(float(np.median(v)), 2), spread_us=round(float(max(v) - min(v)), 2)))

with open(OUT, "w") as fh:
    for ln in lines:
        fh.write(json.dumps(ln) + "\n")
        if "round" not in ln:
            print(json.dumps(ln))
