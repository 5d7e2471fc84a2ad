#!/usr/bin/env python3
"""CPU probe behind the online_f8f8 whole-model bar (tests/test_gpu_f8f8.py, K_F8): on the two-layer models of that test (cold
ragged prefill of 9 + 4 + 30 tokens), how far the composed oracle moves (a) against itself when 5 % of the embedding entries move
by one fp16 ulp -- the class of input difference the device's fp32 summation order produces --, and (b) from fp8 to fp16 linears.
Both relative to the largest logit.  usage: python profiles/probes/f8f8_noise.py"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import ref  # noqa: E402
from tests import f8f8 as F  # noqa: E402


def model(H, Hkv, seed=7):
    d = ref.make_desc(hidden_dim=H * 64, intermediate_dim=512, num_layers=2, num_heads=H, num_kv_heads=Hkv, vocab_size=1024,
                      max_position=1024, cache_quant_bit=0, cache_quant_group=1, cache_layout=3, cache_mode=0)
    rm = ref.RefModel(d)
    rm.init_synthetic(seed)
    return rm


for H, Hkv in ((4, 4), (8, 2)):
    for kv in ("fp16", "int8", "fp8"):
        rm = model(H, Hkv)
        rng = np.random.RandomState(1)
        tok = rng.randint(3, 1024, size=43).astype(np.int64)
        st = ref.make_step(tok, np.array([0, 9, 13, 43]), np.zeros(3, np.int64), np.arange(3, dtype=np.int64) * 256, 0)
        a = F.ComposedOracle(rm, 1024, kv=kv).forward(st)
        sc = max(1.0, float(np.abs(a).max()))
        noise = []
        for s in range(3):
            o = F.ComposedOracle(rm, 1024, kv=kv)
            e = o.w["tok_embeddings.weight"].copy()
            r = np.random.RandomState(5 + s)
            idx = r.rand(e.size) < 0.05
            e[idx] = np.nextafter(e[idx], (np.sign(r.randn(int(idx.sum()))) * np.inf).astype(np.float16))
            o.w["tok_embeddings.weight"] = e
            noise.append(float(np.abs(o.forward(st) - a).max()) / sc)
        fp = F.ComposedOracle(rm, 1024, kv=kv, linears=False).forward(st)
        print(json.dumps({"H": H, "Hkv": Hkv, "kv": kv, "self_noise_5pct_1ulp": [round(x, 5) for x in noise],
                          "fp8_vs_fp16_linears": round(float(np.abs(fp - a).max()) / sc, 5)}), flush=True)
        rm.close()
