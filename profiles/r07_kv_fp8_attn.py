#!/usr/bin/env python3
"""Decode attention (pplhip_op_attention) with int8-g8 and fp8 KV on the same synthetic slab geometry, same process, layout 3, contiguous:
config 2 (7B: H 32, Hkv 32, B 1024, kv 512), config 3 per rank (13B / TP2: H 20, Hkv 20, B 1024, kv 512), config 4 per rank
(70B / TP8: H 8, Hkv 1, B 256, kv 2048).  Prints one JSON line per (config, format): kernel us (torch events over 20 launches) and TB/s
on the format's own algorithmic bytes (K + V rows + their scales of every request, q and out).
usage: python profiles/r07_kv_fp8_attn.py"""
import ctypes as C, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.conftest import load_pplhip

m = load_pplhip()
D = 128
CONFIGS = [("config2", 32, 32, 1024, 512), ("config3_tp2_rank", 20, 20, 1024, 512), ("config4_tp8_rank", 8, 1, 256, 2048)]


def run(name, H, Hkv, B, KV, fmt):
    N = B * KV
    g = 8 if fmt == "int8" else D
    cache = torch.randint(-127, 128, (2 * Hkv * N * D,), dtype=torch.int8, device="cuda")
    if fmt == "fp8":
        cache &= 0x3f   # finite e4m3 codes of magnitude < 1
        scale = torch.full((2 * Hkv * N,), 2.0 ** -5, dtype=torch.float16, device="cuda")
    else:
        scale = (torch.rand(2 * Hkv * N * D // 8, device="cuda") * 0.02 + 0.01).half()
    qkv = torch.randn(B, (H + 2 * Hkv) * D, device="cuda").half()
    out = torch.empty(B, H * D, device="cuda", dtype=torch.float16)
    seq = torch.arange(B + 1, device="cuda", dtype=torch.int64)
    sp = torch.full((B,), KV - 1, device="cuda", dtype=torch.int64)
    ci = torch.arange(B, device="cuda", dtype=torch.int64) * KV
    v = m.KvView()
    v.cache, v.scale, v.max_tokens, v.num_layers, v.kv_heads, v.head_dim = cache.data_ptr(), scale.data_ptr(), N, 1, Hkv, D
    v.quant_bit, v.quant_group, v.layout, v.mode, v.page_size, v.layer = 8, g, 3, 0, 0, 0
    call = lambda: m.lib().pplhip_op_attention(None, qkv.data_ptr(), C.byref(v), seq.data_ptr(), sp.data_ptr(), ci.data_ptr(), 0, B, B, B,
                                               1, KV, H, 1, None, 0, out.data_ptr())
    for _ in range(3):
        assert call() == 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        call()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1000 / 20
    row = D + 2 * (D // g)
    nbytes = 2 * Hkv * B * KV * row + B * (H + 2 * Hkv) * D * 2 + B * H * D * 2
    print(json.dumps({"config": name, "kv": fmt, "H": H, "Hkv": Hkv, "B": B, "kv_len": KV, "attn_us": round(us, 2),
                      "bytes": nbytes, "TBps": round(nbytes / us / 1e6, 3)}), flush=True)
    return us


for name, H, Hkv, B, KV in CONFIGS:
    t8 = run(name, H, Hkv, B, KV, "int8")
    tf = run(name, H, Hkv, B, KV, "fp8")
    print(json.dumps({"config": name, "fp8_over_int8": round(tf / t8, 3)}), flush=True)
