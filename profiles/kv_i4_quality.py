#!/usr/bin/env python3
"""Quality note for the KV cache formats (no bar): int8-g8, fp8 and int4-g32 against the fp16 KV cache of the same library (which the
test suite holds to the oracle), same weights, same tokens: one packed prefill and 8 decode steps fed with the fp16 run's greedy tokens.
Per format: max |logit - fp16 logits| over all rows (the last token of every prompt and every decode row) relative to the largest |fp16
logit|, and the share of rows whose greedy token equals the fp16 run's.
Models: the HF tiny fixtures (tests/golden/hf_tiny_{mha,gqa}.npz, fp16 weights) and the 32-layer LLaMA-2-7B geometry with synthetic W8A16
weights (8 prompts of 64 random tokens; synthetic logits have small top-2 margins, so the greedy figure there is a harsh one).
usage: python profiles/kv_i4_quality.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref  # noqa: E402
from tests.conftest import load_pplhip  # noqa: E402
from tests.test_oracle_hf import desc_from_meta, load_fixture  # noqa: E402

m = load_pplhip()
DECODE = 8


def run(make_ctx, prompts, forced=None):
    """-> (logits [(1 + DECODE) * B, vocab], greedy tokens per step); forced: the tokens to feed instead of the run's own"""
    B = len(prompts)
    lens = np.array([len(p) for p in prompts])
    per = int(lens.max()) + DECODE + 2
    ctx = make_ctx()
    ctx.kv_alloc(0, B * per)
    ci = np.arange(B, dtype=np.int64) * per
    tok = np.concatenate(prompts).astype(np.int64)
    ss = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    sp = np.zeros(B, np.int64)
    logits, toks = [], []
    for s in range(1 + DECODE):
        ctx.set_inputs(0, m.make_step(tok, ss, sp, ci, 0 if s == 0 else B, req_list_changed=int(s == 0)))
        ctx.run(0)
        lg = ctx.copy_logits(B)
        logits.append(lg)
        toks.append(lg.argmax(-1).astype(np.int64))
        sp = sp + (ss[1:] - ss[:-1])
        tok = forced[s] if forced is not None else toks[-1]
        ss = np.arange(B + 1, dtype=np.int64)
    ctx.close()
    return np.concatenate(logits), toks


def compare(name, make_ctx_of, prompts, D):
    base, toks = run(lambda: make_ctx_of(0, 1), prompts)
    sc = float(np.abs(base).max())
    for fmt, (bit, group) in (("int8-g8", (8, 8)), ("fp8", (8, D)), ("int4-g32", (4, 32))):
        got, _ = run(lambda: make_ctx_of(bit, group), prompts, forced=toks)
        d = float(np.abs(got - base).max())
        print(json.dumps({"model": name, "kv_format": fmt, "rows": int(base.shape[0]), "max_abs_logit_diff_vs_fp16_kv": round(d, 5),
                          "relative_to_max_logit": round(d / sc, 5),
                          "greedy_agreement": round(float((got.argmax(-1) == base.argmax(-1)).mean()), 4)}), flush=True)


for name in ("mha", "gqa"):
    meta, weights, prompts, _, _, _ = load_fixture(os.path.join(ROOT, "tests", "golden", f"hf_tiny_{name}.npz"))

    def make(bit, group, meta=meta, weights=weights):
        desc = desc_from_meta(meta, cache_layout=3, cache_mode=0, cache_quant_bit=bit, cache_quant_group=group, weight_quant_bit=0)
        ctx = m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=256)
        for k, v in weights.items():
            ctx.set_tensor(0, k, v)
        return ctx
    d0 = desc_from_meta(meta, cache_layout=3, cache_mode=0, cache_quant_bit=0, cache_quant_group=1, weight_quant_bit=0)
    compare(f"hf_tiny_{name}", make, prompts, d0.hidden_dim // d0.num_heads)


def make7b(bit, group):
    desc = ref.make_desc(hidden_dim=4096, intermediate_dim=11008, num_layers=32, num_heads=32, num_kv_heads=32, vocab_size=32000,
                         max_position=4096, cache_quant_bit=bit, cache_quant_group=group, cache_layout=3, cache_mode=0, weight_quant_bit=8)
    ctx = m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=512)
    ctx.init_synthetic(0, 1)
    return ctx


rng = np.random.RandomState(0)
compare("synthetic_7b_32_layers", make7b, [rng.randint(3, 32000, size=64).astype(np.int64) for _ in range(8)], 128)
