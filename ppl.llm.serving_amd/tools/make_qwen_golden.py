#!/usr/bin/env python3
"""Writes tests/golden/hf_tiny_qwen2.npz and hf_tiny_qwen3.npz: independent answers for the two Qwen forms of the RoPE / KV-write prologue.

    qwen2: a bias on the q / k / v projections, grouped-query attention, head_dim 64   (transformers' Qwen2ForCausalLM)
    qwen3: an RMSNorm over every q and k head row with non-trivial weights, head_dim 128 (transformers' Qwen3ForCausalLM)

Each fixture holds the config, a numpy seed from which both sides draw the weights (draw_weights below: fp16 values under the model
directory's tensor names -- no weight arrays are stored), the token ids and the fp32 last-token logits of a prefill and four greedy decode
steps.  The HF models are built from a config on the CPU (nothing is fetched) and run in fp32 on the fp16-valued weights.

The script asserts that each fixture discriminates: with the biases zeroed (qwen2) or the head norms skipped (qwen3) the HF model's own
logits move, at every step, by at least 10 x the cap the device test grants (CAP x max(1, |logit|max); qwen3: x INT8_KV_RATIO, the cap
of its int8-KV run), so a device that ignores the feature cannot pass.

    python make_qwen_golden.py [--out-dir tests/golden]
"""
import argparse
import json
import os

import numpy as np

CONFIGS = {
    "qwen2": dict(hidden_dim=256, intermediate_dim=192, num_layers=2, num_heads=4, num_kv_heads=2, vocab_size=320, max_position=64,
                  norm_eps=1e-6, rope_theta=10000.0, qkv_bias=True, qk_norm=False),
    "qwen3": dict(hidden_dim=256, intermediate_dim=192, num_layers=2, num_heads=2, num_kv_heads=1, vocab_size=320, max_position=64,
                  norm_eps=1e-6, rope_theta=10000.0, qkv_bias=False, qk_norm=True),
}
SEEDS = {"qwen2": 200, "qwen3": 300}
PROMPT_LEN, DECODE_STEPS = 19, 4
CAP = 2e-2            # tests/test_gpu_model.py's cap for HF vectors, relative to max(1, |logit|max)
INT8_KV_RATIO = 2.25  # what test_hf_fixture_model grants a grouped-query fixture over int8 KV (k 4.5) against fp16 KV (k 2)


def draw_weights(cfg, seed):
    """name -> fp16 array, in the model directory's naming and layout (wqkv = q rows, k rows, v rows; w13 = gate rows, then up rows).
    The biases are as large as the projections' outputs and the norm weights spread over 0.5 .. 3.5: what the discrimination assert needs"""
    rng = np.random.RandomState(seed)
    hd, inter, V = cfg["hidden_dim"], cfg["intermediate_dim"], cfg["vocab_size"]
    D = hd // cfg["num_heads"]
    nqkv = (cfg["num_heads"] + 2 * cfg["num_kv_heads"]) * D
    mat = lambda n, k, amp=0.06: (rng.randn(n, k) * amp).astype(np.float16)
    norm = lambda: (1.0 + 0.1 * rng.randn(hd)).astype(np.float16)
    w = {"tok_embeddings.weight": mat(V, hd, 1.0), "norm.weight": norm(), "output.weight": mat(V, hd)}
    for l in range(cfg["num_layers"]):
        p = f"layers.{l}."
        w[p + "attention_norm.weight"], w[p + "ffn_norm.weight"] = norm(), norm()
        w[p + "attention.wqkv.weight"] = mat(nqkv, hd)
        if cfg["qkv_bias"]:
            w[p + "attention.wqkv.bias"] = (rng.randn(nqkv) * 1.0).astype(np.float16)
        if cfg["qk_norm"]:
            w[p + "attention.q_norm.weight"] = (0.5 + 3.0 * rng.rand(D)).astype(np.float16)
            w[p + "attention.k_norm.weight"] = (0.5 + 3.0 * rng.rand(D)).astype(np.float16)
        w[p + "attention.wo.weight"] = mat(hd, hd, 0.12)
        w[p + "feed_forward.w13.weight"] = mat(2 * inter, hd)
        w[p + "feed_forward.w2.weight"] = mat(hd, inter)
    return w


def hf_model(cfg, w, ablate=False):
    """the HF model on the drawn weights; ablate: the same model with the biases zeroed / the head norms skipped"""
    import torch
    import transformers
    H, Hkv, D, inter = cfg["num_heads"], cfg["num_kv_heads"], cfg["hidden_dim"] // cfg["num_heads"], cfg["intermediate_dim"]
    kw = dict(hidden_size=cfg["hidden_dim"], intermediate_size=inter, num_hidden_layers=cfg["num_layers"], num_attention_heads=H,
              num_key_value_heads=Hkv, vocab_size=cfg["vocab_size"], max_position_embeddings=cfg["max_position"], rms_norm_eps=cfg["norm_eps"],
              tie_word_embeddings=False, use_sliding_window=False, rope_parameters={"rope_type": "default", "rope_theta": cfg["rope_theta"]})
    if cfg["qk_norm"]:
        hc = transformers.Qwen3Config(head_dim=D, attention_bias=False, **kw)
        model = transformers.Qwen3ForCausalLM(hc)
    else:
        hc = transformers.Qwen2Config(**kw)
        model = transformers.Qwen2ForCausalLM(hc)
    model.config._attn_implementation = "eager"
    model = model.float().eval()
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    sd = {"model.embed_tokens.weight": t(w["tok_embeddings.weight"]), "model.norm.weight": t(w["norm.weight"]), "lm_head.weight": t(w["output.weight"])}
    for l in range(cfg["num_layers"]):
        p, q = f"layers.{l}.", f"model.layers.{l}."
        qkv = w[p + "attention.wqkv.weight"]
        sd[q + "input_layernorm.weight"], sd[q + "post_attention_layernorm.weight"] = t(w[p + "attention_norm.weight"]), t(w[p + "ffn_norm.weight"])
        cuts = {"q_proj": slice(0, H * D), "k_proj": slice(H * D, (H + Hkv) * D), "v_proj": slice((H + Hkv) * D, None)}
        for name, cut in cuts.items():
            sd[q + f"self_attn.{name}.weight"] = t(qkv[cut])
            if cfg["qkv_bias"]:
                sd[q + f"self_attn.{name}.bias"] = t(w[p + "attention.wqkv.bias"][cut]) * (0.0 if ablate else 1.0)
        if cfg["qk_norm"]:
            sd[q + "self_attn.q_norm.weight"], sd[q + "self_attn.k_norm.weight"] = t(w[p + "attention.q_norm.weight"]), t(w[p + "attention.k_norm.weight"])
        sd[q + "self_attn.o_proj.weight"] = t(w[p + "attention.wo.weight"])
        w13 = w[p + "feed_forward.w13.weight"]
        sd[q + "mlp.gate_proj.weight"], sd[q + "mlp.up_proj.weight"] = t(w13[:inter]), t(w13[inter:])
        sd[q + "mlp.down_proj.weight"] = t(w[p + "feed_forward.w2.weight"])
    missing = model.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    if ablate and cfg["qk_norm"]:
        for layer in model.model.layers:
            layer.self_attn.q_norm, layer.self_attn.k_norm = torch.nn.Identity(), torch.nn.Identity()
    return model


def trace(cfg, seed):
    """-> (tokens, logits [steps, V], the ablated model's logits on the same tokens)"""
    import torch
    w = draw_weights(cfg, seed)
    model, ablated = hf_model(cfg, w), hf_model(cfg, w, ablate=True)
    tokens = list(np.random.RandomState(seed + 1).randint(3, cfg["vocab_size"], size=PROMPT_LEN))
    logits, other = [], []
    with torch.no_grad():
        for _ in range(1 + DECODE_STEPS):
            logits.append(model(torch.tensor([tokens])).logits[0, -1].numpy().astype(np.float32))
            other.append(ablated(torch.tensor([tokens])).logits[0, -1].numpy().astype(np.float32))
            tokens.append(int(logits[-1].argmax()))
    return np.array(tokens[:-1], dtype=np.int64), np.stack(logits), np.stack(other)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out-dir", default=os.path.join(root, "tests", "golden"))
    args = ap.parse_args()
    for name, cfg in CONFIGS.items():
        tokens, logits, other = trace(cfg, SEEDS[name])
        cap = CAP * max(1.0, float(np.abs(logits).max())) * (INT8_KV_RATIO if cfg["qk_norm"] else 1.0)
        moved = np.abs(other - logits).max(1)
        assert (moved >= 10 * cap).all(), (name, moved, 10 * cap)
        out = os.path.join(args.out_dir, f"hf_tiny_{name}.npz")
        np.savez(out, config=json.dumps(cfg), seed=SEEDS[name], tokens=tokens, logits=logits)
        print(f"wrote {out}: {len(tokens)} tokens, logits {logits.shape}, max |logit| {np.abs(logits).max():.3f}; without the feature "
              f"the logits move by {moved.min():.3f} .. {moved.max():.3f} (10 x cap = {10 * cap:.3f})")


if __name__ == "__main__":
    main()
