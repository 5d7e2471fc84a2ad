"""The exporter's params.json (tools/export_hf_llama.py params_json): `sliding_window` is written only for a checkpoint whose config.json
has a non-null one, so every other export stays as it was."""
import argparse

import pytest

from tests.test_export_hf import exp

CFG = dict(hidden_size=256, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512, vocab_size=1024, model_type="mistral")
ARGS = argparse.Namespace(kv_cache="int8", cache_quant_bit=8, cache_layout=3, cache_mode=1, page_size=16, quant="w8a16", quant_group=128)


@pytest.mark.parametrize("extra,want", [({}, None), ({"sliding_window": None}, None), ({"sliding_window": 4096}, 4096)])
def test_params_json_sliding_window(extra, want):
    p, base = exp.params_json(dict(CFG, **extra), ARGS), exp.params_json(CFG, ARGS)
    assert p.get("sliding_window") == want and {k: v for k, v in p.items() if k != "sliding_window"} == base
    assert ("sliding_window" in p) == (want is not None)
