"""Qwen2 / Qwen3 through the context (pplhip_qkv_prologue): the HF fixtures of tools/make_qwen_golden.py -- whose script asserts that an HF
model without the biases / the head norms misses them by 10 x the cap used here -- fp16 weights, tensors uploaded by name, a prompt and
four greedy decode steps."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu

CAP = 2e-2            # test_distinct_experts_match_hf_mixtral's (test_hf_fixture_model's) cap for HF vectors, x max(1, |logit|max)
INT8_KV_RATIO = 2.25  # test_hf_fixture_model grants its grouped-query fixture k = 4.5 over int8 KV and k = 2 over fp16 KV
TP_CAP = 1.5e-3       # test_tensor_parallel_group_on_one_device's cap for its tiny model, x max(1, |logit|max)


def fixture(golden_dir, name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_qwen_golden", os.path.join(root, "ppl.llm.serving_amd", "tools", "make_qwen_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = np.load(os.path.join(golden_dir, f"hf_tiny_{name}.npz"))
    cfg = json.loads(str(fx["config"]))
    weights = gen.draw_weights(cfg, int(fx["seed"]))
    bias, norm = cfg.pop("qkv_bias"), cfg.pop("qk_norm")
    return cfg, (bias, norm, cfg["norm_eps"]), weights, fx["tokens"], fx["logits"]


def rank_slice(name, arr, cfg, tp, r):
    """a tensor of the model directory as rank r of tp holds it (the exporter's slicing)"""
    D = cfg["hidden_dim"] // cfg["num_heads"]
    h, hk = cfg["num_heads"] * D // tp, cfg["num_kv_heads"] * D // tp
    rows = lambda a, n: a[r * n:(r + 1) * n]
    if ".wqkv." in name:
        q, k, v = arr[:h * tp], arr[h * tp:(h + hk) * tp], arr[(h + hk) * tp:]
        return np.concatenate([rows(q, h), rows(k, hk), rows(v, hk)])
    if ".w13." in name:
        return np.concatenate([rows(a, len(a) // tp) for a in np.split(arr, 2)])
    if name == "output.weight":
        return rows(arr, len(arr) // tp)
    if ".wo." in name or ".w2." in name:
        return np.ascontiguousarray(rows(arr.T, arr.shape[1] // tp).T)
    return arr


def run_fixture(m, cfg, prologue, weights, tokens, steps, tp=1, **desc_kw):
    """-> logits [steps, V] of the prompt and the decode steps (request 0, pages 0 .. of a paged cache or slot 0)"""
    two = dict(n_local_ranks=tp, device_ids=[0] * tp) if tp > 1 else {}
    ctx = m.Context(m.make_desc(**dict(cfg, **desc_kw)), max_running_batch=4, max_tokens_per_step=64, **two)
    if prologue:
        ctx.qkv_prologue(*prologue)
    for r in range(tp):
        for name, arr in weights.items():
            ctx.set_tensor(r, name, rank_slice(name, arr, cfg, tp, r))
        ctx.kv_alloc(r, 64)
    paged = desc_kw.get("cache_mode", 0) == 1
    cache_idx, max_pages = (np.arange(4, dtype=np.int64)[None], 4) if paged else (np.zeros(1, dtype=np.int64), 0)
    n0, out = len(tokens) - (steps - 1), []
    for s in range(steps):
        tok, pos = (tokens[:n0], 0) if s == 0 else (tokens[n0 + s - 1:n0 + s], n0 + s - 1)
        for r in range(tp):
            ctx.set_inputs(r, m.make_step(tok, [0, len(tok)], [pos], cache_idx, int(s > 0), max_pages, req_list_changed=int(s == 0)))
            ctx.run(r)
        out.append(ctx.copy_logits(1)[0])
        for r in range(1, tp):
            ctx.sync(r)
    ctx.close()
    return np.stack(out)


def check(name, got, want, cap):
    for s in range(len(want)):
        err = float(np.abs(got[s] - want[s]).max())
        print(f"{name} step {s}: max |logit error| {err:.3e}, cap {cap:.3e}")
        assert err < cap, (s, err, cap)
        assert got[s].argmax() == want[s].argmax() or np.sort(want[s])[-1] - np.sort(want[s])[-2] < 2 * cap


@pytest.mark.parametrize("name,kv", [("qwen2", "fp16"), ("qwen3", "fp16"), ("qwen3", "int8_paged")])
def test_hf_qwen_fixture(golden_dir, name, kv):
    """fp16 KV at the cap for HF vectors; the Qwen3 fixture also over int8-g8 KV on a paged cache, at that cap times INT8_KV_RATIO"""
    m = load_pplhip()
    cfg, prologue, weights, tokens, want = fixture(golden_dir, name)
    kw = dict(cache_quant_bit=8, cache_quant_group=8, cache_mode=1, page_size=16) if kv == "int8_paged" else {}
    cap = CAP * max(1.0, float(np.abs(want).max())) * (INT8_KV_RATIO if kv == "int8_paged" else 1.0)
    check(f"hf_tiny_{name} {kv}", run_fixture(m, cfg, prologue, weights, tokens, len(want), **kw), want, cap)


def test_tensor_parallel_bias_slices(golden_dir):
    """a TP-2 group on one device, the bias sliced with wqkv's rows, against the single rank's logits"""
    m = load_pplhip()
    cfg, prologue, weights, tokens, want = fixture(golden_dir, "qwen2")
    one = run_fixture(m, cfg, prologue, weights, tokens, len(want))
    two = run_fixture(m, cfg, prologue, weights, tokens, len(want), tp=2)
    check("hf_tiny_qwen2 tp2 against tp1", two, one, TP_CAP * max(1.0, float(np.abs(one).max())))


def test_zero_bias_is_the_llama_context(golden_dir):
    """the call made and the zeros left in place: the bits of a context without the call, prefill and decode (x + 0 is x; the head norm
    with its ones in place still divides by the row's rms, so it has no such identity)"""
    m = load_pplhip()
    cfg, _, weights, tokens, want = fixture(golden_dir, "qwen2")
    weights = {k: v for k, v in weights.items() if not k.endswith(".bias")}
    plain = run_fixture(m, cfg, None, weights, tokens, 3)
    zeros = run_fixture(m, cfg, (True, False, 0.0), weights, tokens, 3)
    assert (plain.view(np.uint32) == zeros.view(np.uint32)).all()


def test_the_call_after_a_weight_is_refused(golden_dir):
    m = load_pplhip()
    cfg, _, weights, _, _ = fixture(golden_dir, "qwen3")
    ctx = m.Context(m.make_desc(**cfg), max_running_batch=4, max_tokens_per_step=64)
    ctx.set_tensor(0, "norm.weight", weights["norm.weight"])
    assert m.lib().pplhip_qkv_prologue(ctx.h, 0, 1, 1e-6) == m.lib().pplhip_qkv_prologue(None, 1, 1, 1e-6) != 0   # PPLHIP_INVALID_VALUE
    with pytest.raises(m.PplHipError, match="INVALID_VALUE: pplhip_qkv_prologue: call it before any weight is loaded"):
        ctx.qkv_prologue(qk_norm=True)
    ctx.close()
