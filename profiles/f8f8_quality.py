#!/usr/bin/env python3
"""Quality note for online_f8f8 (no bar): the HF tiny fixtures (tests/golden/hf_tiny_{mha,gqa}.npz) loaded as fp16 tensors into an
fp16, an online_i8i8 and an online_f8f8 context (the W8A8 modes quantise them on the device), one packed prefill of the fixture's
prompts; max |logit - fp16 logits| of the last token of every prompt, absolute and relative to the largest fp16 logit.
usage: python profiles/f8f8_quality.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.conftest import load_pplhip  # noqa: E402
from tests.test_oracle_hf import desc_from_meta, load_fixture  # noqa: E402

m = load_pplhip()
for name in ("mha", "gqa"):
    meta, weights, prompts, _, _, _ = load_fixture(os.path.join(ROOT, "tests", "golden", f"hf_tiny_{name}.npz"))
    lens = np.array([len(p) for p in prompts])
    tok = np.concatenate(prompts).astype(np.int64)
    ss = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ci = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    out = {}
    for mode, wq, act in (("fp16", 0, 0), ("online_i8i8", 8, 8), ("online_f8f8", 8, 0x108)):
        desc = desc_from_meta(meta, cache_layout=3, cache_mode=0, cache_quant_bit=0, cache_quant_group=1, weight_quant_bit=wq,
                              act_quant_bit=act)
        ctx = m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=256)
        for k, v in weights.items():
            ctx.set_tensor(0, k, v)
        ctx.kv_alloc(0, 512)
        ctx.set_inputs(0, m.make_step(tok, ss, np.zeros(len(prompts), np.int64), ci, 0, req_list_changed=1))
        ctx.run(0)
        out[mode] = ctx.copy_logits(len(prompts))
        ctx.close()
    sc = float(np.abs(out["fp16"]).max())
    for mode in ("online_i8i8", "online_f8f8"):
        d = float(np.abs(out[mode] - out["fp16"]).max())
        print(json.dumps({"fixture": f"hf_tiny_{name}", "mode": mode, "max_abs_logit_diff_vs_fp16": round(d, 5),
                          "relative_to_max_logit": round(d / sc, 5),
                          "greedy_equal_rows": int((out[mode].argmax(-1) == out["fp16"].argmax(-1)).sum()), "rows": len(prompts)}),
              flush=True)
