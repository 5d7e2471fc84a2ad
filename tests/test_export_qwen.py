"""The exporter on Qwen2 / Qwen3 checkpoints (tools/export_hf_llama.py): the two params.json keys, the fused bias in wqkv's row order, its
per-rank slices, the replicated norm weights, the refusal of a head_dim the model description cannot derive -- and LLaMA as it was."""
import argparse

import numpy as np
import pytest

from tests.test_export_hf import exp

ARGS = argparse.Namespace(kv_cache="fp16", cache_quant_bit=0, cache_layout=3, cache_mode=0, page_size=16, quant="none", quant_group=128)
H, HKV, D, HD, L = 4, 2, 32, 128, 2


def checkpoint(model_type, **extra):
    cfg = dict(hidden_size=HD, num_attention_heads=H, num_key_value_heads=HKV, num_hidden_layers=L, intermediate_size=64, vocab_size=96,
               model_type=model_type, sliding_window=4096, use_sliding_window=False, **extra)
    rng = np.random.RandomState(0)
    sd = {"model.embed_tokens.weight": rng.randn(96, HD), "model.norm.weight": rng.randn(HD), "lm_head.weight": rng.randn(96, HD)}
    for l in range(L):
        p = f"model.layers.{l}."
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = rng.randn(HD), rng.randn(HD)
        for name, rows in (("q", H * D), ("k", HKV * D), ("v", HKV * D)):
            sd[p + f"self_attn.{name}_proj.weight"], sd[p + f"self_attn.{name}_proj.bias"] = rng.randn(rows, HD), rng.randn(rows)
        sd[p + "self_attn.q_norm.weight"], sd[p + "self_attn.k_norm.weight"] = rng.randn(D), rng.randn(D)
        sd[p + "self_attn.o_proj.weight"] = rng.randn(HD, H * D)
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"], sd[p + "mlp.down_proj.weight"] = rng.randn(64, HD), rng.randn(64, HD), rng.randn(HD, 64)
    return cfg, sd


@pytest.mark.parametrize("model_type,bias,norm", [("qwen2", True, False), ("qwen3", False, True), ("llama", False, False)])
@pytest.mark.parametrize("tp", [1, 2])
def test_export(model_type, bias, norm, tp):
    cfg, sd = checkpoint(model_type)
    p = exp.params_json(cfg, ARGS)
    assert p.get("qkv_bias") == (True if bias else None) and p.get("qk_norm") == (True if norm else None)
    assert ("sliding_window" in p) == (model_type == "llama")   # (Qwen configs name a window that use_sliding_window leaves off)
    slices = exp.convert(sd, cfg, tp, "none", 128)
    h, hk = H // tp, HKV // tp
    f16 = lambda a: np.asarray(a, np.float32).astype(np.float16)
    for r, out in enumerate(slices):
        for l in range(L):
            a, q = f"layers.{l}.attention.", f"model.layers.{l}.self_attn."
            assert (a + "wqkv.bias" in out) == bias and (a + "q_norm.weight" in out) == (a + "k_norm.weight" in out) == norm
            if bias:   # the rank's q, k, v pieces, in the order of its wqkv rows
                want = np.concatenate([sd[q + "q_proj.bias"][r * h * D:(r + 1) * h * D], sd[q + "k_proj.bias"][r * hk * D:(r + 1) * hk * D],
                                       sd[q + "v_proj.bias"][r * hk * D:(r + 1) * hk * D]])
                assert (out[a + "wqkv.bias"] == f16(want)).all() and len(want) == len(out[a + "wqkv.weight"])
            if norm:
                assert (out[a + "q_norm.weight"] == f16(sd[q + "q_norm.weight"])).all() and (out[a + "k_norm.weight"] == f16(sd[q + "k_norm.weight"])).all()


def test_head_dim_the_description_cannot_derive_is_refused():
    cfg, sd = checkpoint("qwen3", head_dim=64)
    with pytest.raises(ValueError, match=f"head_dim 64 x num_attention_heads {H} is not hidden_size {HD}"):
        exp.convert(sd, cfg, 1, "none", 128)
