#!/usr/bin/env python3
"""W8A16 vs online_i8i8 vs online_f8f8 on the same device, in one process:
  * the 7B layer's four linears (wqkv, wo, w13 with fused SwiGLU, w2) at M = 1, 8, 64, 256, 1024, 8192, quantisers included
    (pplhip_op_quant_act[_f8] + pplhip_op_linear_{i8,f8}; W8A16: pplhip_op_linear[_swiglu]), torch events over 10 launches;
  * the whole decode step at config 2's shape (7B, 32 layers, batch 1024, kv 512, int8-g8 KV, synthetic weights) and at batch 1, with
    the per-step GEMM time of the runtime's own profiler (PPLHIP_PROF_GEMM: the linears and, for the W8A8 modes, their quantisers).
Prints one JSON line per measurement.
usage: python profiles/f8f8_step.py [--layers-only | --step MODE BATCH]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ref  # noqa: E402
from tests.conftest import load_pplhip  # noqa: E402

m = load_pplhip()
L = m.lib()
HD, INTER, NQKV = 4096, 11008, 12288
LINEARS = [("wqkv", NQKV, HD, False), ("wo", HD, HD, False), ("w13", 2 * INTER, HD, True), ("w2", HD, INTER, False)]
MODES = ["w8a16", "online_i8i8", "online_f8f8"]


def timed(call, reps=10):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / reps


def layer_gemms(M):
    res = {}
    for mode in MODES:
        total = 0.0
        for name, N, K, swiglu in LINEARS:
            x = (torch.randn(M, K, device="cuda") * 0.5).half()
            y = torch.empty(M, N // 2 if swiglu else N, device="cuda", dtype=torch.float16)
            sc = (torch.rand(N, device="cuda") * 1e-3 + 1e-4).half()
            if mode == "w8a16":
                w = torch.randint(-127, 128, (N, K), dtype=torch.int8, device="cuda")
                if swiglu:
                    call = lambda: L.pplhip_op_linear_swiglu(None, x.data_ptr(), w.data_ptr(), sc.data_ptr(), 8, 128, M, N, K, y.data_ptr())
                else:
                    call = lambda: L.pplhip_op_linear(None, x.data_ptr(), w.data_ptr(), sc.data_ptr(), 8, 128, M, N, K, y.data_ptr(), 0)
            else:
                f8 = mode == "online_f8f8"
                w = torch.randint(-127, 128, (N, K), dtype=torch.int8, device="cuda")
                if f8:
                    w &= 0x3f    # finite e4m3 codes of magnitude < 1
                    sc = torch.full((N,), 2.0 ** -6, device="cuda", dtype=torch.float16)
                xq = torch.empty(M, K, dtype=torch.int8, device="cuda")
                sx = torch.empty(M, dtype=torch.float32, device="cuda")
                qa = L.pplhip_op_quant_act_f8 if f8 else L.pplhip_op_quant_act
                lin = L.pplhip_op_linear_f8 if f8 else L.pplhip_op_linear_i8

                def call(qa=qa, lin=lin, x=x, xq=xq, sx=sx, w=w, sc=sc, y=y, N=N, K=K, swiglu=swiglu):
                    qa(None, x.data_ptr(), M, K, xq.data_ptr(), sx.data_ptr())
                    return lin(None, xq.data_ptr(), sx.data_ptr(), w.data_ptr(), sc.data_ptr(), M, N, K, y.data_ptr(), 0, int(swiglu))
            assert call() == 0, (mode, name, M)
            us = timed(call)
            total += us
            print(json.dumps({"what": "layer_linear", "mode": mode, "linear": name, "M": M, "N": N, "K": K, "us": round(us, 2)}), flush=True)
            del w, x, y
        res[mode] = total
        print(json.dumps({"what": "layer_gemms", "mode": mode, "M": M, "us": round(total, 2)}), flush=True)
    print(json.dumps({"what": "layer_gemms_ratio", "M": M, "f8f8_over_i8i8": round(res["online_f8f8"] / res["online_i8i8"], 3),
                      "f8f8_over_w8a16": round(res["online_f8f8"] / res["w8a16"], 3)}), flush=True)
    torch.cuda.empty_cache()


def step(mode, B, kv_len, steps=5):
    act = {"w8a16": 0, "online_i8i8": 8, "online_f8f8": 0x108}[mode]
    desc = ref.make_desc(hidden_dim=HD, intermediate_dim=INTER, num_layers=32, num_heads=32, num_kv_heads=32, vocab_size=32000,
                         max_position=4096, cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=0, weight_quant_bit=8,
                         act_quant_bit=act)
    ctx = m.Context(m.copy_desc(desc), max_running_batch=B, max_tokens_per_step=B, profiling=True)
    ctx.init_synthetic(0, 1)
    ctx.kv_alloc(0, B * (kv_len + steps + 2))
    ctx.kv_fill_synthetic(0, 3)
    ci = np.arange(B, dtype=np.int64) * (kv_len + steps + 2)
    tok = np.random.RandomState(0).randint(3, 32000, size=B).astype(np.int64)
    times, gemm = [], []
    for s in range(steps + 2):
        st = m.make_step(tok, np.arange(B + 1, dtype=np.int64), np.full(B, kv_len + s, np.int64), ci, B, req_list_changed=int(s == 0))
        ctx.profile_reset(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.set_inputs(0, st)
        ctx.run(0)
        ctx.sync(0)
        t1 = time.perf_counter()
        if s >= 2:
            times.append((t1 - t0) * 1e3)
            gemm.append(ctx.profile_get(m.PROF_GEMM, 0)[1])
    ctx.close()
    row = {"what": "decode_step", "mode": mode, "B": B, "kv_len": kv_len, "kv": "int8-g8", "ms_per_step": round(float(np.median(times)), 3),
           "gemm_ms_per_step": round(float(np.median(gemm)), 3)}
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    if "--step" in sys.argv:   # one mode's steps alone (for a kernel trace): --step MODE BATCH
        i = sys.argv.index("--step")
        step(sys.argv[i + 1], int(sys.argv[i + 2]), 512)
        sys.exit(0)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "time": time.strftime("%Y-%m-%dT%H:%M:%S")}), flush=True)
    for M in (1, 8, 64, 256, 1024, 8192):
        layer_gemms(M)
    if "--layers-only" not in sys.argv:
        for B in (1024, 1):
            r = {mode: step(mode, B, 512) for mode in MODES}
            print(json.dumps({"what": "decode_step_ratio", "B": B,
                              "gemm_f8f8_over_i8i8": round(r["online_f8f8"]["gemm_ms_per_step"] / r["online_i8i8"]["gemm_ms_per_step"], 3),
                              "step_f8f8_over_w8a16": round(r["online_f8f8"]["ms_per_step"] / r["w8a16"]["ms_per_step"], 3)}), flush=True)
