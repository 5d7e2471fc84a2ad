"""ALiBi attention, operator timings on one device in one session (profiles/attn_alibi.md has the results): pplhip_op_attention_alibi
against pplhip_op_attention on the same inputs, Baichuan-13B geometry (40 heads, head_dim 128), the standard slopes.
  prefill  one 4096-token prompt
  decode   128 rows at kv 4096, every row with slots of its own, so the reads come from HBM
Warm-up launches first, then the median of `--iters` event-timed launches, the variants interleaved (plain, ALiBi, plain again: the spread
of the two plain columns is the noise of the comparison).
    python profiles/time_attn_alibi.py [--iters 30] [--kv fp16|int8]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from __graft_entry__ import _load_pplhip  # noqa: E402

H, D = 40, 128


def view(m, cache, scale, N, quant):
    v = m.KvView()
    v.cache, v.scale = cache.data_ptr(), (scale.data_ptr() if quant else None)
    v.max_tokens, v.num_layers, v.kv_heads, v.head_dim = N, 1, H, D
    v.quant_bit, v.quant_group = (8, 8) if quant else (0, 1)
    v.layout, v.mode, v.page_size, v.layer = 3, 0, 0, 0
    return v


def slab(N, quant):
    """[1, k / v, head, slot, channel]: small random values, scales near 0.02"""
    if quant:
        return (torch.randint(-127, 128, (1, 2, H, N, D), dtype=torch.int8, device="cuda"),
                torch.full((1, 2, H, N, D // 8), 0.02, dtype=torch.float16, device="cuda"))
    return torch.randn((1, 2, H, N, D), dtype=torch.float16, device="cuda"), None


def timed(calls, iters):
    """median microseconds of every call in `calls`, interleaved"""
    for f in calls:
        for _ in range(3):
            assert f() == 0
    torch.cuda.synchronize()
    us = [[] for _ in calls]
    for _ in range(iters):
        for i, f in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert f() == 0
            b.record()
            b.synchronize()
            us[i].append(a.elapsed_time(b) * 1e3)
    return [float(np.median(u)) for u in us]


def ops(m, slopes, qkv, v, seq, sp, ci, B, T, nd, max_seq, max_kv, ws, out):
    """(plain, ALiBi, plain) on the same arguments"""
    args = [None, qkv.data_ptr(), C.byref(v), seq.data_ptr(), sp.data_ptr(), ci.data_ptr(), 1, B, T, nd, max_seq, max_kv, H, 1, ws.data_ptr(),
            ws.numel(), out.data_ptr()]
    plain = lambda: m.lib().pplhip_op_attention(*args)
    return [plain, lambda: m.lib().pplhip_op_attention_alibi(*args, slopes.data_ptr()), plain]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--kv", choices=["fp16", "int8"], default="int8")
    a = ap.parse_args()
    m, quant = _load_pplhip(), a.kv == "int8"
    dev = lambda x: torch.from_numpy(np.asarray(x, dtype=np.int64)).cuda()
    host_slopes = np.empty(H, dtype=np.float32)
    assert m.lib().pplhip_op_alibi_slopes(H, host_slopes.ctypes.data) == 0
    slopes = torch.from_numpy(host_slopes).cuda()
    res = {"kv": a.kv, "iters": a.iters, "heads": H}
    names = ("plain", "alibi", "plain_again")
    # ---- prefill: one request of L tokens
    L = 4096
    cache, scale = slab(L, quant)
    qkv = torch.randn((L, 3 * H * D), dtype=torch.float16, device="cuda")
    out, ws = torch.empty((L, H * D), dtype=torch.float16, device="cuda"), torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    v, seq, sp, ci = view(m, cache, scale, L, quant), dev([0, L]), dev([0]), dev([0])
    us = timed(ops(m, slopes, qkv, v, seq, sp, ci, 1, L, 0, L, L, ws, out), a.iters)
    res["prefill_4096_us"] = dict(zip(names, us))
    res["prefill_ratio"] = us[1] / (0.5 * (us[0] + us[2]))
    del cache, scale, qkv, out
    # ---- decode: B rows at kv 4096, row b's slots start at 4096 b
    B, KV = 128, 4096
    cache, scale = slab(B * KV, quant)
    qkv = torch.randn((B, 3 * H * D), dtype=torch.float16, device="cuda")
    out = torch.empty((B, H * D), dtype=torch.float16, device="cuda")
    v, seq, sp, ci = view(m, cache, scale, B * KV, quant), dev(np.arange(B + 1)), dev([KV - 1] * B), dev(np.arange(B) * KV)
    us = timed(ops(m, slopes, qkv, v, seq, sp, ci, B, B, B, 1, KV, ws, out), a.iters)
    res["decode_128x4096_us"] = dict(zip(names, us))
    res["decode_ratio"] = us[1] / (0.5 * (us[0] + us[2]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
