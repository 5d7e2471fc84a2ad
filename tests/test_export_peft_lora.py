"""tools/export_peft_lora.py on a fixture adapter written here with safetensors: the fused tensors reproduce W_q|W_k|W_v + scale B A of
the separate PEFT factors in float64, the container loads back, and every refusal names its reason."""
import importlib.util
import json
import os
import struct

import numpy as np
import pytest
import safetensors.numpy as st

from tests.conftest import ROOT

PARAMS = dict(num_heads=8, num_kv_heads=2, num_layers=2, hidden_dim=64, intermediate_dim=96, vocab_size=128)
R, ALPHA = 4, 8.0


def _tool():
    path = os.path.join(ROOT, "ppl.llm.serving_amd", "tools", "export_peft_lora.py")
    spec = importlib.util.spec_from_file_location("export_peft_lora", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _shapes():
    D = PARAMS["hidden_dim"] // PARAMS["num_heads"]
    hd, inter = PARAMS["hidden_dim"], PARAMS["intermediate_dim"]
    return {"self_attn.q_proj": (PARAMS["num_heads"] * D, hd), "self_attn.k_proj": (PARAMS["num_kv_heads"] * D, hd),
            "self_attn.v_proj": (PARAMS["num_kv_heads"] * D, hd), "self_attn.o_proj": (hd, PARAMS["num_heads"] * D),
            "mlp.down_proj": (hd, inter), "mlp.gate_proj": (inter, hd), "mlp.up_proj": (inter, hd)}


def write_adapter(d, modules=("q_proj", "k_proj", "v_proj", "o_proj", "down_proj"), r=R, cfg_extra=None, seed=0):
    rng = np.random.RandomState(seed)
    tensors = {}
    for l in range(PARAMS["num_layers"]):
        for full, (n, k) in _shapes().items():
            if full.split(".")[1] not in modules:
                continue
            pre = f"base_model.model.model.layers.{l}.{full}"
            # (values on a power-of-two grid: exactly fp16, so the fp16 container holds what was written)
            tensors[pre + ".lora_A.weight"] = (rng.randint(-8, 9, size=(r, k)) / 64.0).astype(np.float32)
            tensors[pre + ".lora_B.weight"] = (rng.randint(-8, 9, size=(n, r)) / 64.0).astype(np.float32)
    os.makedirs(d, exist_ok=True)
    st.save_file(tensors, os.path.join(d, "adapter_model.safetensors"))
    cfg = dict(peft_type="LORA", r=r, lora_alpha=ALPHA, bias="none", target_modules=list(modules), use_dora=False, rank_pattern={},
               alpha_pattern={}, modules_to_save=None)
    cfg.update(cfg_extra or {})
    json.dump(cfg, open(os.path.join(d, "adapter_config.json"), "w"))
    json.dump(PARAMS, open(os.path.join(d, "params.json"), "w"))
    return tensors


def read_container(path):
    out = {}
    with open(path, "rb") as f:
        assert f.read(8) == b"PPLHIPW1"
        (n,) = struct.unpack("<I", f.read(4))
        for _ in range(n):
            (nl,) = struct.unpack("<I", f.read(4))
            name = f.read(nl).decode()
            (nb,) = struct.unpack("<Q", f.read(8))
            f.seek((64 - f.tell() % 64) % 64, 1)
            out[name] = f.read(nb)
    return out


def test_fused_tensors_reproduce_the_separate_factors(tmp_path):
    tool = _tool()
    src, out = str(tmp_path / "adapter"), str(tmp_path / "out")
    t = write_adapter(src)
    assert tool.main([src, out, "--params", os.path.join(src, "params.json")]) == 0
    c = read_container(os.path.join(out, "lora.pplhip"))
    scale = float(np.frombuffer(c["lora.scale"], dtype=np.float32)[0])
    assert scale == ALPHA / R
    sh = _shapes()
    nqkv = sh["self_attn.q_proj"][0] + 2 * sh["self_attn.k_proj"][0]
    rng = np.random.RandomState(1)
    for l in range(PARAMS["num_layers"]):
        pre = f"base_model.model.model.layers.{l}."
        A = np.frombuffer(c[f"layers.{l}.attention.wqkv.lora_a"], dtype=np.float16).reshape(3 * R, -1).astype(np.float64)
        B = np.frombuffer(c[f"layers.{l}.attention.wqkv.lora_b"], dtype=np.float16).reshape(nqkv, 3 * R).astype(np.float64)
        W = {m: rng.standard_normal(sh["self_attn." + m]) for m in ("q_proj", "k_proj", "v_proj")}
        want = np.concatenate([W[m] + scale * t[pre + f"self_attn.{m}.lora_B.weight"].astype(np.float64) @ t[pre + f"self_attn.{m}.lora_A.weight"].astype(np.float64)
                               for m in ("q_proj", "k_proj", "v_proj")], 0)       # the row order export_hf_llama.py gives wqkv
        got = np.concatenate([W[m] for m in ("q_proj", "k_proj", "v_proj")], 0) + scale * B @ A
        assert np.array_equal(got, want)
        for mod, name in (("self_attn.o_proj", "attention.wo"), ("mlp.down_proj", "feed_forward.w2")):
            a = np.frombuffer(c[f"layers.{l}.{name}.lora_a"], dtype=np.float16).reshape(R, -1)
            b = np.frombuffer(c[f"layers.{l}.{name}.lora_b"], dtype=np.float16).reshape(-1, R)
            assert np.array_equal(a.astype(np.float32), t[pre + mod + ".lora_A.weight"]) and np.array_equal(b.astype(np.float32), t[pre + mod + ".lora_B.weight"])
    assert not any("w13" in k for k in c)


def test_q_and_v_only_fuse_to_twice_the_rank(tmp_path):
    tool = _tool()
    src, out = str(tmp_path / "adapter"), str(tmp_path / "out")
    t = write_adapter(src, modules=("q_proj", "v_proj"))
    assert tool.main([src, out, "--params", os.path.join(src, "params.json")]) == 0
    c = read_container(os.path.join(out, "lora.pplhip"))
    sh = _shapes()
    nq, nkv = sh["self_attn.q_proj"][0], sh["self_attn.k_proj"][0]
    B = np.frombuffer(c["layers.0.attention.wqkv.lora_b"], dtype=np.float16).reshape(nq + 2 * nkv, 2 * R)
    assert not B[nq:nq + nkv].any() and not B[:nq, R:].any() and not B[nq + nkv:, :R].any()       # k rows untouched, blocks apart
    assert np.array_equal(B[nq + nkv:, R:].astype(np.float32), t["base_model.model.model.layers.0.self_attn.v_proj.lora_B.weight"])
    assert set(c) == {f"layers.{l}.attention.wqkv.lora_{x}" for l in range(2) for x in "ab"} | {"lora.scale"}


@pytest.mark.parametrize("kw,reason", [
    (dict(cfg_extra={"rank_pattern": {"q_proj": 8}}), "rank_pattern"),
    (dict(cfg_extra={"alpha_pattern": {"q_proj": 4}}), "alpha_pattern"),
    (dict(cfg_extra={"use_dora": True}), "use_dora"),
    (dict(cfg_extra={"bias": "all"}), "bias"),
    (dict(cfg_extra={"modules_to_save": ["lm_head"]}), "modules_to_save"),
    (dict(modules=("q_proj", "gate_proj")), "gate / up"),
    (dict(modules=("up_proj",)), "gate / up"),
    (dict(r=48), "fused q / k / v rank 144 is above 128"),
])
def test_refusals_name_their_reason(tmp_path, capsys, kw, reason):
    tool = _tool()
    src, out = str(tmp_path / "adapter"), str(tmp_path / "out")
    write_adapter(src, **kw)
    assert tool.main([src, out, "--params", os.path.join(src, "params.json")]) == 2
    assert reason in capsys.readouterr().err
    assert not os.path.exists(os.path.join(out, "lora.pplhip"))
