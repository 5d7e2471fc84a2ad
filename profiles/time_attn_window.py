"""Sliding-window attention, operator timings on one device in one session (profiles/attn_window.md has the results):
  prefill  the band kernel on an 8192-token prompt (7B geometry: 32 heads, head_dim 128, int8 KV) at W 4096 and W 1024 against the causal
           prefill of the same prompt; beside the measured ratio the counted one, (W L - W^2 / 2) / (L^2 / 2) score pairs
  decode   1024 windowed rows at kv 8192, W 4096, against 1024 ordinary rows at kv 4096: the same bytes read.  Every row has slots of its
           own for the keys it reads, so the reads come from HBM
Warm-up launches first, then the median of `--iters` event-timed launches, the variants interleaved.
    python profiles/time_attn_window.py [--iters 20] [--kv fp16|int8]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from __graft_entry__ import _load_pplhip  # noqa: E402

H = HKV = 32
D = 128


def view(m, cache, scale, N, quant):
    v = m.KvView()
    v.cache, v.scale = cache.data_ptr(), (scale.data_ptr() if quant else None)
    v.max_tokens, v.num_layers, v.kv_heads, v.head_dim = N, 1, HKV, D
    v.quant_bit, v.quant_group = (8, 8) if quant else (0, 1)
    v.layout, v.mode, v.page_size, v.layer = 3, 0, 0, 0
    return v


def slab(N, quant):
    """[1, k / v, head, slot, channel]: small random values, scales near 0.02"""
    if quant:
        return (torch.randint(-127, 128, (1, 2, HKV, N, D), dtype=torch.int8, device="cuda"),
                torch.full((1, 2, HKV, N, D // 8), 0.02, dtype=torch.float16, device="cuda"))
    return torch.randn((1, 2, HKV, N, D), dtype=torch.float16, device="cuda"), None


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


def op(m, window, qkv, v, seq, sp, ci, B, T, nd, max_seq, max_kv, ws, out):
    args = [None, qkv.data_ptr(), C.byref(v), seq.data_ptr(), sp.data_ptr(), ci.data_ptr(), 1, B, T, nd, max_seq, max_kv, H, 1, ws.data_ptr(),
            ws.numel(), out.data_ptr()]
    if window:
        return lambda: m.lib().pplhip_op_attention_window(*args, window)
    return lambda: m.lib().pplhip_op_attention(*args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kv", choices=["fp16", "int8"], default="int8")
    a = ap.parse_args()
    m, quant = _load_pplhip(), a.kv == "int8"
    dev = lambda x: torch.from_numpy(np.asarray(x, dtype=np.int64)).cuda()
    res = {"kv": a.kv, "iters": a.iters}
    # ---- prefill: one request of L tokens
    L = 8192
    cache, scale = slab(L, quant)
    qkv = torch.randn((L, (H + 2 * HKV) * D), dtype=torch.float16, device="cuda")
    out, ws = torch.empty((L, H * D), dtype=torch.float16, device="cuda"), torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    v, seq, sp, ci = view(m, cache, scale, L, quant), dev([0, L]), dev([0]), dev([0])
    us = timed([op(m, w, qkv, v, seq, sp, ci, 1, L, 0, L, L, ws, out) for w in (0, 4096, 1024)], a.iters)
    res["prefill_us"] = {"causal": us[0], "W4096": us[1], "W1024": us[2]}
    res["prefill_ratio"] = {f"W{w}": {"measured": u / us[0], "counted": (w * L - w * w / 2) / (L * L / 2)} for w, u in ((4096, us[1]), (1024, us[2]))}
    del cache, scale, qkv, out
    # ---- decode: B rows, each with 4096 slots of its own for the keys it reads (row b's slots start at 4096 b)
    B, W = 1024, 4096
    N = (B + 1) * W
    cache, scale = slab(N, quant)
    qkv = torch.randn((B, (H + 2 * HKV) * D), dtype=torch.float16, device="cuda")
    out = torch.empty((B, H * D), dtype=torch.float16, device="cuda")
    ws = torch.empty(4096 + B * 32, dtype=torch.uint8, device="cuda")
    v, seq, ci = view(m, cache, scale, N, quant), dev(np.arange(B + 1)), dev(np.arange(B) * W)
    # the launch a windowed context makes on a contiguous cache: the ordinary decode kernel on the arrays pplhip_op_window_shift gives
    # (pplhip_op_attention_window itself would add its host round trip for the positions to the interval); reads slots 4096 b + 4096 .. + 8191
    rc, pos, tab, _, max_kv = m.window_shift(np.full(B, 2 * W - 1), np.arange(B) * W, 0, 0, W)
    assert rc == 0 and max_kv == W
    wpos, wtab, opos = dev(pos), dev(tab[:, 0]), dev([W - 1] * B)   # (named: the launches hold raw pointers)
    windowed = op(m, 0, qkv, v, seq, wpos, wtab, B, B, B, 1, W, ws, out)
    ordinary = op(m, 0, qkv, v, seq, opos, ci, B, B, B, 1, W, ws, out)             # reads slots 4096 b .. + 4095
    us = timed([ordinary, windowed, ordinary], a.iters)
    res["decode_us"] = {"ordinary_kv4096": us[0], "windowed_kv8192_W4096": us[1], "ordinary_kv4096_again": us[2]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
