#!/usr/bin/env python3
"""export_peft_lora.py <adapter_dir> <out_dir> --params params.json

Converts a PEFT LoRA adapter of a LLaMA-family model (adapter_config.json + adapter_model.safetensors, read directly: peft is not
needed) into <out_dir>/lora.pplhip for pplhip_lora_load / offline_inference --lora-dirs (include/pplhip.h "multi-LoRA"):

    layers.{l}.attention.wqkv.lora_a [r_q + r_k + r_v, hidden]   the q / k / v factors A stacked
    layers.{l}.attention.wqkv.lora_b [(H + 2 Hkv) D, r_q + r_k + r_v]   block diagonal, rows in the order export_hf_llama.py gives
                                                                 wqkv: q rows, k rows, v rows
    layers.{l}.attention.wo.lora_a / .lora_b, layers.{l}.feed_forward.w2.lora_a / .lora_b   (o_proj, down_proj) as they are
    lora.scale fp32 [1] = lora_alpha / r  (lora_alpha / sqrt(r) with use_rslora)

so that W_q|W_k|W_v + scale B A is the fused matrix of the merged model.  The zero blocks of the fused B cost nothing that matters
beside the base GEMM.  Refused, with the reason: rank_pattern, alpha_pattern, use_dora, bias other than "none", modules_to_save, gate /
up (or any other) target modules, a fused rank above 128.  Tensor parallelism is not supported by the adapter kernels: one slice.
"""
import argparse
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from export_hf_llama import write_container  # noqa: E402

MAX_RANK = 128
ATTN = ("q_proj", "k_proj", "v_proj")
PLAIN = {"o_proj": "attention.wo", "down_proj": "feed_forward.w2"}


class Refused(ValueError):
    pass


def load_tensors(path):
    try:
        from safetensors.numpy import load_file
        return {k: np.asarray(v) for k, v in load_file(path).items()}
    except TypeError:          # bfloat16 has no numpy type: go through torch
        from safetensors.torch import load_file as load_torch
        return {k: v.float().numpy() for k, v in load_torch(path).items()}


def check_config(cfg):
    if cfg.get("peft_type", "LORA") != "LORA":
        raise Refused(f"peft_type {cfg.get('peft_type')!r}: only LORA adapters are supported")
    if cfg.get("rank_pattern"):
        raise Refused("rank_pattern is set: an adapter has one rank per target here")
    if cfg.get("alpha_pattern"):
        raise Refused("alpha_pattern is set: an adapter has one scale here (lora.scale)")
    if cfg.get("use_dora"):
        raise Refused("use_dora: DoRA rescales the merged weight's columns, which is not a low-rank update")
    if cfg.get("bias", "none") != "none":
        raise Refused(f"bias {cfg.get('bias')!r}: adapters with trained biases are not supported (bias must be \"none\")")
    if cfg.get("modules_to_save"):
        raise Refused(f"modules_to_save {cfg.get('modules_to_save')}: fully trained modules are not part of an adapter here")
    r = int(cfg["r"])
    if r < 1:
        raise Refused(f"rank {r}")
    return r, float(cfg.get("lora_alpha", r)) / (np.sqrt(r) if cfg.get("use_rslora") else r)


def convert(tensors, cfg, params):
    """-> ({container name: fp16 array}, scale)"""
    r, scale = check_config(cfg)
    H, Hkv, hd, L = params["num_heads"], params.get("num_kv_heads", params["num_heads"]), params["hidden_dim"], params["num_layers"]
    D = hd // H
    rows = {"q_proj": H * D, "k_proj": Hkv * D, "v_proj": Hkv * D}
    found = {}
    for key, w in tensors.items():
        m = re.search(r"layers\.(\d+)\.(?:self_attn|mlp)\.(\w+)\.lora_([AB])(?:\.\w+)?\.weight$", key)
        if not m:
            raise Refused(f"tensor {key}: not a LoRA factor of a decoder layer linear")
        l, mod, ab = int(m.group(1)), m.group(2), m.group(3)
        if mod in ("gate_proj", "up_proj"):
            raise Refused(f"tensor {key}: gate / up (w13) targets are not supported, the fused SwiGLU epilogue never materialises them")
        if mod not in ATTN and mod not in PLAIN:
            raise Refused(f"tensor {key}: unknown target module {mod}")
        if l >= L:
            raise Refused(f"tensor {key}: the model has {L} layers")
        found[(l, mod, ab)] = np.asarray(w, dtype=np.float32)
    out = {}
    for l in range(L):
        mods = [m for m in ATTN if (l, m, "A") in found or (l, m, "B") in found]
        for m in mods + [m for m in PLAIN if (l, m, "A") in found or (l, m, "B") in found]:
            if (l, m, "A") not in found or (l, m, "B") not in found:
                raise Refused(f"layer {l} {m}: one factor of two")
            a, b = found[(l, m, "A")], found[(l, m, "B")]
            if a.shape[0] != r or b.shape[1] != r:
                raise Refused(f"layer {l} {m}: factors of rank {a.shape[0]} / {b.shape[1]}, adapter_config.json says {r}")
        if mods:
            fused = r * len(mods)
            if fused > MAX_RANK:
                raise Refused(f"layer {l}: fused q / k / v rank {fused} is above {MAX_RANK}")
            A = np.concatenate([found[(l, m, "A")] for m in mods], 0)
            B = np.zeros((sum(rows.values()), fused), dtype=np.float32)
            n0 = 0
            for m in ATTN:
                if m in mods:
                    j = mods.index(m) * r
                    if found[(l, m, "B")].shape[0] != rows[m] or found[(l, m, "A")].shape[1] != hd:
                        raise Refused(f"layer {l} {m}: factor shapes do not fit params.json")
                    B[n0:n0 + rows[m], j:j + r] = found[(l, m, "B")]
                n0 += rows[m]
            out[f"layers.{l}.attention.wqkv.lora_a"], out[f"layers.{l}.attention.wqkv.lora_b"] = A, B
        for m, name in PLAIN.items():
            if (l, m, "A") in found:
                if r > MAX_RANK:
                    raise Refused(f"rank {r} is above {MAX_RANK}")
                out[f"layers.{l}.{name}.lora_a"], out[f"layers.{l}.{name}.lora_b"] = found[(l, m, "A")], found[(l, m, "B")]
    if not out:
        raise Refused("the adapter holds no factors")
    return {k: v.astype(np.float16) for k, v in out.items()}, scale


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("adapter_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--params", required=True, help="params.json of the exported base model (export_hf_llama.py)")
    args = ap.parse_args(argv)
    cfg = json.load(open(os.path.join(args.adapter_dir, "adapter_config.json")))
    params = json.load(open(args.params))
    try:
        tensors, scale = convert(load_tensors(os.path.join(args.adapter_dir, "adapter_model.safetensors")), cfg, params)
    except Refused as e:
        print(f"export_peft_lora: refused: {e}", file=sys.stderr)
        return 2
    os.makedirs(args.out_dir, exist_ok=True)
    tensors["lora.scale"] = np.array([scale], dtype=np.float32)
    write_container(os.path.join(args.out_dir, "lora.pplhip"), tensors)
    print(f"wrote {args.out_dir}/lora.pplhip: {len(tensors) - 1} factors, scale {scale}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
