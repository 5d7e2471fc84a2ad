"""tools/offline_inference --lora-dirs / --lora-map on the tiny model of tests/lora_model.py: every request's tokens equal the greedy
continuation of the oracle on ITS adapter's exactly merged weights, on the rows outside the near-tie margin (as tests/test_gpu_tools.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import ref
from tests import lora_model as LM
from tests.conftest import load_pplhip
from tests.test_gpu_tools import tool

pytestmark = pytest.mark.gpu


def oracle_greedy(desc, weights, prompt, n):
    rm = LM.oracle(desc, weights, 64)
    toks, margins = [], []
    tok, start = np.asarray(prompt, dtype=np.int64), 0
    pages = np.arange(64 // desc.page_size, dtype=np.int64)[None, :]
    for s in range(n):
        st = ref.make_step(tok, [0, len(tok)], [start], pages, 0 if s == 0 else 1, max_pages=pages.shape[1])
        logits = ref.forward([rm], st)[0]
        srt = np.sort(logits)
        margins.append(float(srt[-1] - srt[-2]))
        toks.append(int(logits.argmax()))
        start += len(tok)
        tok = np.array([toks[-1]], dtype=np.int64)
    rm.close()
    return toks, margins


def test_offline_inference_serves_per_request_adapters(tmp_path):
    m = load_pplhip()
    desc = LM.make_desc("mha", "i8paged")
    w = LM.base_weights(desc, seed=77)
    os.makedirs(tmp_path / "model_slice_0")
    m.write_container(str(tmp_path / "model_slice_0" / "weights.pplhip"), w)
    params = dict(num_heads=desc.num_heads, num_kv_heads=desc.num_kv_heads, num_layers=desc.num_layers, hidden_dim=desc.hidden_dim,
                  intermediate_dim=desc.intermediate_dim, vocab_size=desc.vocab_size, cache_quant_bit=8, cache_quant_group=8, cache_layout=3,
                  cache_mode=1, page_size=desc.page_size, dynamic_batching=True, auto_causal=True, weight_quant_bit=0, max_position=512)
    json.dump(params, open(tmp_path / "params.json", "w"))
    adapters = [LM.make_adapter(desc, a, amp=6) for a in (0, 1)]     # (strong enough to change greedy continuations)
    for i, (t, s) in enumerate(adapters):
        os.makedirs(tmp_path / f"adapter{i}")
        m.write_lora_container(str(tmp_path / f"adapter{i}" / "lora.pplhip"), t, s)
    lora_map = [0, -1, 1, 0]
    out = subprocess.check_output([tool("offline_inference"), "--model-param-path", str(tmp_path / "params.json"), "--model-dir", str(tmp_path),
                                   "--kv-cache-max-tokens", "512", "--max-running-batch", "8", "--max-tokens-per-step", "64",
                                   "--workload", "prompts4", "--lora-dirs", f"{tmp_path}/adapter0,{tmp_path}/adapter1",
                                   "--lora-map", ",".join(map(str, lora_map))], timeout=300).decode()
    prompts, answers = [], []
    for line in out.splitlines():
        if line.startswith("Prompt tokens:"):
            prompts.append([int(x) for x in line.split(":")[1].split()])
        if line.startswith("Answer tokens:"):
            answers.append([int(x) for x in line.split(":")[1].split()])
    assert len(prompts) == 4 and [len(a) for a in answers] == [8, 9, 10, 11]
    compared = differs_from_base = 0
    for p, a, slot in zip(prompts, answers, lora_map):
        weights = w if slot < 0 else LM.merged(w, *adapters[slot])
        want, margins = oracle_greedy(desc, weights, p, len(a))
        base, _ = oracle_greedy(desc, w, p, len(a))
        differs_from_base += int(slot >= 0 and want != base)
        for i, (g, x) in enumerate(zip(a, want)):
            if margins[i] < 8e-3:      # near-tie: either choice is legitimate, and the continuations diverge
                break
            assert g == x, (slot, p, i, a, want)
            compared += 1
    assert compared >= 12
    assert differs_from_base >= 1, "the adapters never change a greedy continuation: the comparison shows nothing"
    # a map that names a slot nobody loaded is refused before anything runs
    r = subprocess.run([tool("offline_inference"), "--model-param-path", str(tmp_path / "params.json"), "--model-dir", str(tmp_path),
                        "--kv-cache-max-tokens", "512", "--workload", "prompts4", "--lora-dirs", f"{tmp_path}/adapter0", "--lora-map", "1"],
                       capture_output=True, timeout=300)
    assert r.returncode != 0 and b"--lora-map names slot 1" in r.stderr
