"""The exporter on Baichuan checkpoints (tools/export_hf_llama.py): W_pack split into wqkv's q | k | v rows, Baichuan2's normalised head,
max_position from model_max_length, the "alibi" key with its default and its flag override -- and LLaMA's params.json as it was."""
import argparse
import json

import numpy as np
import pytest

from tests.test_export_hf import exp
from tests.test_export_qwen import ARGS, checkpoint as llama_checkpoint

H, D, HD, L = 4, 32, 128, 2


def checkpoint(vocab=96, **extra):
    cfg = dict(hidden_size=HD, num_attention_heads=H, num_hidden_layers=L, intermediate_size=64, vocab_size=vocab, model_type="baichuan", **extra)
    rng = np.random.RandomState(1)
    sd = {"model.embed_tokens.weight": rng.randn(vocab, HD).astype(np.float32), "model.norm.weight": rng.randn(HD),
          "lm_head.weight": rng.randn(vocab, HD).astype(np.float32)}
    for l in range(L):
        p = f"model.layers.{l}."
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = rng.randn(HD), rng.randn(HD)
        sd[p + "self_attn.W_pack.weight"], sd[p + "self_attn.o_proj.weight"] = rng.randn(3 * HD, HD), rng.randn(HD, HD)
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"], sd[p + "mlp.down_proj.weight"] = rng.randn(64, HD), rng.randn(64, HD), rng.randn(HD, 64)
    return cfg, sd


@pytest.mark.parametrize("tp", [1, 2])
def test_w_pack_becomes_wqkv_rows(tp):
    cfg, sd = checkpoint(model_max_length=4096)
    slices, h = exp.convert(sd, cfg, tp, "none", 128), H // tp
    llama_cfg, llama_sd = llama_checkpoint("llama")
    assert set(slices[0]) == set(exp.convert(llama_sd, llama_cfg, tp, "none", 128)[0])   # LLaMA's tensor names
    f16 = lambda a: np.asarray(a, np.float32).astype(np.float16)
    for r, out in enumerate(slices):
        for l in range(L):
            q, k, v = np.split(sd[f"model.layers.{l}.self_attn.W_pack.weight"], 3, axis=0)
            assert (out[f"layers.{l}.attention.wqkv.weight"] == f16(np.concatenate([x[r * h * D:(r + 1) * h * D] for x in (q, k, v)], 0))).all()
        assert (out["output.weight"] == f16(sd["lm_head.weight"][r * 96 // tp:(r + 1) * 96 // tp])).all()   # Baichuan (1): the head as it is


@pytest.mark.parametrize("flag,normalised", [(None, True), (False, False)])
def test_baichuan2_head_is_normalised(flag, normalised):
    cfg, sd = checkpoint(vocab=125696, model_max_length=4096)   # (Baichuan2's vocabulary: the default's cue)
    head = sd["lm_head.weight"]
    want = head / np.linalg.norm(head, axis=1, keepdims=True) if normalised else head
    assert (exp.convert(sd, cfg, 1, "none", 128, flag)[0]["output.weight"] == want.astype(np.float16)).all()


@pytest.mark.parametrize("extra,flag,alibi,max_position", [
    (dict(model_max_length=4096), None, True, 4096),                                   # the 13B form: no max_position_embeddings
    (dict(max_position_embeddings=2048, model_max_length=4096), None, False, 2048),    # the 7B form: rotary
    (dict(max_position_embeddings=2048), True, True, 2048),                            # the flags win, both ways
    (dict(model_max_length=4096), False, False, 4096)])
def test_alibi_and_max_position_keys(extra, flag, alibi, max_position):
    p = exp.params_json(checkpoint(**extra)[0], argparse.Namespace(alibi=flag, **vars(ARGS)))
    assert p.get("alibi") == (1 if alibi else None) and p["max_position"] == max_position


def test_llama_params_json_is_byte_for_byte_what_it_was():
    """the keys, their order and their values written out: what the exporter wrote for this config before it knew ALiBi"""
    text = json.dumps(exp.params_json(llama_checkpoint("llama")[0], ARGS), indent=1)
    assert text == json.dumps({"num_heads": 4, "num_kv_heads": 2, "num_layers": 2, "hidden_dim": 128, "intermediate_dim": 64, "vocab_size": 96,
                               "cache_quant_bit": 0, "cache_quant_group": 1, "cache_layout": 3, "cache_mode": 0, "dynamic_batching": True,
                               "auto_causal": True, "norm_eps": 1e-5, "rope_theta": 10000.0, "max_position": 4096, "weight_quant_bit": 0,
                               "weight_quant_group": 128, "sliding_window": 4096}, indent=1)
