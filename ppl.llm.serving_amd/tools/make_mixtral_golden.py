#!/usr/bin/env python3
"""Writes tests/golden/hf_tiny_mixtral.npz: an independent answer for a tiny mixture-of-experts model with DISTINCT experts.

The fixture holds the config, a numpy seed from which both sides draw the weights (draw_weights below: fp16 values under the model
directory's tensor names -- no weight arrays are stored), the token ids, the fp32 last-token logits of a prefill and four greedy decode
steps, and layer 0's expert choice per token.  The answer comes from transformers' own MixtralForCausalLM, built from a config on the CPU
(nothing is fetched) and run in fp32 on the fp16-valued weights.  The script asserts that every routing decision of the trace, in every
layer, is safe under fp32 accumulation: the gap between the k-th and (k+1)-th router logits is at least 8 x hidden x 2^-24 x sum |x_i g_i|
(DESIGN.md "numerics", mixture of experts); a seed that fails is skipped.

    python make_mixtral_golden.py [--out tests/golden/hf_tiny_mixtral.npz]
"""
import argparse
import json
import os

import numpy as np

CONFIG = dict(hidden_dim=128, intermediate_dim=192, num_layers=2, num_heads=4, num_kv_heads=2, vocab_size=320, max_position=64,
              norm_eps=1e-5, rope_theta=10000.0, num_experts=4, experts_per_token=2)
PROMPT_LEN, DECODE_STEPS = 19, 4


def draw_weights(cfg, seed):
    """name -> fp16 array, in the model directory's naming and layout (w13 = gate rows, then up rows)"""
    rng = np.random.RandomState(seed)
    hd, inter, V, E = cfg["hidden_dim"], cfg["intermediate_dim"], cfg["vocab_size"], cfg["num_experts"]
    D = hd // cfg["num_heads"]
    mat = lambda n, k, amp=0.06: (rng.randn(n, k) * amp).astype(np.float16)
    norm = lambda: (1.0 + 0.1 * rng.randn(hd)).astype(np.float16)
    w = {"tok_embeddings.weight": mat(V, hd, 1.0), "norm.weight": norm(), "output.weight": mat(V, hd)}
    for l in range(cfg["num_layers"]):
        p = f"layers.{l}."
        w[p + "attention_norm.weight"], w[p + "ffn_norm.weight"] = norm(), norm()
        w[p + "attention.wqkv.weight"] = mat((cfg["num_heads"] + 2 * cfg["num_kv_heads"]) * D, hd)
        w[p + "attention.wo.weight"] = mat(hd, hd)
        w[p + "feed_forward.gate.weight"] = mat(E, hd, 0.3)
        for j in range(E):
            w[p + f"feed_forward.experts.{j}.w13.weight"] = mat(2 * inter, hd)
            w[p + f"feed_forward.experts.{j}.w2.weight"] = mat(hd, inter)
    return w


def hf_model(cfg, w):
    import torch
    from transformers import MixtralConfig, MixtralForCausalLM
    hc = MixtralConfig(hidden_size=cfg["hidden_dim"], intermediate_size=cfg["intermediate_dim"], num_hidden_layers=cfg["num_layers"],
                       num_attention_heads=cfg["num_heads"], num_key_value_heads=cfg["num_kv_heads"], vocab_size=cfg["vocab_size"],
                       max_position_embeddings=cfg["max_position"], rms_norm_eps=cfg["norm_eps"], num_local_experts=cfg["num_experts"],
                       num_experts_per_tok=cfg["experts_per_token"], sliding_window=None, tie_word_embeddings=False,
                       rope_parameters={"rope_type": "default", "rope_theta": cfg["rope_theta"]})
    hc._attn_implementation = "eager"
    model = MixtralForCausalLM(hc).float().eval()
    H, Hkv, D, E = cfg["num_heads"], cfg["num_kv_heads"], cfg["hidden_dim"] // cfg["num_heads"], cfg["num_experts"]
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    sd = {"model.embed_tokens.weight": t(w["tok_embeddings.weight"]), "model.norm.weight": t(w["norm.weight"]), "lm_head.weight": t(w["output.weight"])}
    for l in range(cfg["num_layers"]):
        p, q = f"layers.{l}.", f"model.layers.{l}."
        qkv = w[p + "attention.wqkv.weight"]
        sd[q + "input_layernorm.weight"], sd[q + "post_attention_layernorm.weight"] = t(w[p + "attention_norm.weight"]), t(w[p + "ffn_norm.weight"])
        sd[q + "self_attn.q_proj.weight"], sd[q + "self_attn.k_proj.weight"] = t(qkv[:H * D]), t(qkv[H * D:(H + Hkv) * D])
        sd[q + "self_attn.v_proj.weight"], sd[q + "self_attn.o_proj.weight"] = t(qkv[(H + Hkv) * D:]), t(w[p + "attention.wo.weight"])
        sd[q + "mlp.gate.weight"] = t(w[p + "feed_forward.gate.weight"])
        sd[q + "mlp.experts.gate_up_proj"] = t(np.stack([w[p + f"feed_forward.experts.{j}.w13.weight"] for j in range(E)]))
        sd[q + "mlp.experts.down_proj"] = t(np.stack([w[p + f"feed_forward.experts.{j}.w2.weight"] for j in range(E)]))
    missing = model.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return model


def trace(cfg, seed):
    """-> (tokens, logits [steps, V], layer-0 experts [tokens, k]) or None when a routing gap of the trace is not safe"""
    import torch
    w = draw_weights(cfg, seed)
    model = hf_model(cfg, w)
    k, hd = cfg["experts_per_token"], cfg["hidden_dim"]
    seen = []   # (layer order) router inputs of the last forward
    hooks = [layer.mlp.gate.register_forward_hook(lambda mod, inp, out: seen.append((mod.weight.detach().double().numpy(), inp[0].detach().double().numpy().reshape(-1, hd))))
             for layer in model.model.layers]
    tokens = list(np.random.RandomState(seed + 1).randint(3, cfg["vocab_size"], size=PROMPT_LEN))
    logits = []
    with torch.no_grad():
        for _ in range(1 + DECODE_STEPS):   # causal: the last forward's states are every earlier forward's
            seen.clear()
            logits.append(model(torch.tensor([tokens])).logits[0, -1].numpy().astype(np.float32))
            tokens.append(int(logits[-1].argmax()))
    for h in hooks:
        h.remove()
    choice = None
    for g, x in seen:   # every layer, every token of the trace
        r = x @ g.T
        order = np.argsort(-r, axis=1, kind="stable")
        top = np.take_along_axis(r, order[:, :k + 1], 1)
        bound = 8 * hd * 2.0 ** -24 * np.abs(x[:, None, :] * g[None]).sum(-1).max(1)
        if ((top[:, :-1] - top[:, 1:]).min(1) < bound).any():
            return None
        if choice is None:
            choice = order[:, :k].astype(np.int32)
    return np.array(tokens[:-1], dtype=np.int64), np.stack(logits), choice


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=os.path.join(root, "tests", "golden", "hf_tiny_mixtral.npz"))
    args = ap.parse_args()
    for seed in range(100, 120):
        res = trace(CONFIG, seed)
        if res is not None:
            break
    assert res is not None, "no seed with safe routing gaps"
    tokens, logits, choice = res
    assert len(np.unique(choice)) == CONFIG["num_experts"]   # layer 0 uses every expert
    np.savez(args.out, config=json.dumps(CONFIG), seed=seed, tokens=tokens, logits=logits, layer0_experts=choice)
    print(f"wrote {args.out}: seed {seed}, {len(tokens)} tokens, logits {logits.shape}, max |logit| {np.abs(logits).max():.3f}")


if __name__ == "__main__":
    main()
