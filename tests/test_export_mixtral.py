"""The exporter on a Mixtral-type checkpoint (tools/export_hf_llama.py): a tiny random MixtralForCausalLM is saved, exported at fp16 and
W8A16, and the container's gate and expert tensors and the two params.json keys are checked against the state dict."""
import json
import os

import numpy as np
import pytest

from tests.test_export_hf import exp, read_container

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")


@pytest.mark.parametrize("quant", ["none", "w8a16"])
def test_mixtral_export_names_layout_and_params(tmp_path, quant):
    from transformers import MixtralConfig, MixtralForCausalLM
    torch.manual_seed(5)
    E, k, hd, inter, L = 4, 2, 128, 96, 2
    cfg = MixtralConfig(hidden_size=hd, intermediate_size=inter, num_hidden_layers=L, num_attention_heads=4, num_key_value_heads=2, vocab_size=256,
                        max_position_embeddings=64, num_local_experts=E, num_experts_per_tok=k, tie_word_embeddings=False)
    model = MixtralForCausalLM(cfg).float().eval()
    model.save_pretrained(str(tmp_path / "hf"), safe_serialization=True)
    sd = {n: v.numpy() for n, v in model.state_dict().items()}
    out = str(tmp_path / "out")
    exp.main(["--model-dir", str(tmp_path / "hf"), "--out", out, "--tensor-parallel-size", "1", "--quant", quant])
    params = json.load(open(os.path.join(out, "params.json")))
    assert (params["num_experts"], params["experts_per_token"], params["intermediate_dim"]) == (E, k, inter)
    t = read_container(os.path.join(out, "model_slice_0", "weights.pplhip"))
    assert not any(".feed_forward.w13" in n or ".feed_forward.w2" in n for n in t)   # no dense FFN tensors
    for l in range(L):
        p = f"model.layers.{l}.mlp."
        assert (t[f"layers.{l}.feed_forward.gate.weight"].view(np.float16).reshape(E, hd) == sd[p + "gate.weight"].astype(np.float16)).all()
        for j in range(E):
            for name, w in ((f"layers.{l}.feed_forward.experts.{j}.w13", sd[p + "experts.gate_up_proj"][j]),   # [gate rows | up rows]
                            (f"layers.{l}.feed_forward.experts.{j}.w2", sd[p + "experts.down_proj"][j])):
                if quant == "none":
                    assert (t[name + ".weight"].view(np.float16).reshape(w.shape) == w.astype(np.float16)).all()
                else:
                    q, s = exp.quant_w8(w)
                    assert (t[name + ".weight"].view(np.int8).reshape(w.shape) == q).all() and (t[name + ".scale"].view(np.float16) == s).all()
    with pytest.raises(ValueError, match="tensor-parallel size 1"):
        exp.convert(sd, json.load(open(tmp_path / "hf" / "config.json")), 2, quant, 128)
