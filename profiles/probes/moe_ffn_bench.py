"""Times pplhip_op_moe_ffn at Mixtral 8x7B's layer (hidden 4096, inter 14336, E 8, k 2, W8A16) against the dense yardstick: pplhip_op_linear_swiglu +
pplhip_op_linear on T k rows of ONE expert's weights (the same FLOPs, 1 / E of the weight bytes).  Device events around `iters` back-to-back
calls, the two alternating, median of `reps` windows; warm-up per shape.  Writes profiles/moe_ffn.md's table rows to stdout."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
spec = importlib.util.spec_from_file_location("pplhip_binding", os.path.join(ROOT, "ppl.llm.serving_amd", "pplhip.py"))
m = importlib.util.module_from_spec(spec)
spec.loader.exec_module(m)
L = m.lib()
hidden, inter, E, k = 4096, 14336, 8, 2
g = torch.Generator(device="cuda").manual_seed(0)
w13 = torch.randint(-127, 128, (E, 2 * inter, hidden), dtype=torch.int8, device="cuda", generator=g)
w2 = torch.randint(-127, 128, (E, hidden, inter), dtype=torch.int8, device="cuda", generator=g)
s13 = (torch.rand((E, 2 * inter), device="cuda", generator=g) * 4e-4 + 2e-4).half()
s2 = (torch.rand((E, hidden), device="cuda", generator=g) * 4e-4 + 2e-4).half()
gate = (torch.randn((E, hidden), device="cuda", generator=g) * 0.1).half()


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us per call


for T in [int(a) for a in sys.argv[1:]] or [64, 1024, 4096]:
    x = (torch.randn((T, hidden), device="cuda", generator=g) * 0.5).half()
    xd = (torch.randn((T * k, hidden), device="cuda", generator=g) * 0.5).half()
    ws_bytes = L.pplhip_op_moe_ffn_workspace_bytes(T, E, k, hidden, inter)
    ws = torch.zeros(ws_bytes // 4 + 1, dtype=torch.float32, device="cuda")
    y = torch.empty((T, hidden), dtype=torch.float16, device="cuda")
    h = torch.empty((T * k, inter), dtype=torch.float16, device="cuda")
    yd = torch.empty((T * k, hidden), dtype=torch.float16, device="cuda")

    def moe():
        assert L.pplhip_op_moe_ffn(None, x.data_ptr(), gate.data_ptr(), w13.data_ptr(), s13.data_ptr(), w2.data_ptr(), s2.data_ptr(), 8, T, E, k, hidden,
                                   inter, ws.data_ptr(), ws_bytes, y.data_ptr(), hidden) == 0

    def dense():
        assert L.pplhip_op_linear_swiglu(None, xd.data_ptr(), w13.data_ptr(), s13.data_ptr(), 8, 128, T * k, 2 * inter, hidden, h.data_ptr()) == 0
        assert L.pplhip_op_linear(None, h.data_ptr(), w2.data_ptr(), s2.data_ptr(), 8, 128, T * k, hidden, inter, yd.data_ptr(), 0) == 0

    iters = 20 if T >= 1024 else 100
    for fn in (moe, dense, moe, dense):
        window(fn, 5)
    tm, td = [], []
    for _ in range(7):
        tm.append(window(moe, iters))
        td.append(window(dense, iters))
    flops = 2.0 * T * k * hidden * inter * 3
    wbytes = E * 3 * hidden * inter
    a, b = float(np.median(tm)), float(np.median(td))
    print(f"| {T} | {L.pplhip_op_moe_tile_rows(T, k, E)} | {a:.0f} ({min(tm):.0f} .. {max(tm):.0f}) | {b:.0f} ({min(td):.0f} .. {max(td):.0f}) | {a / b:.2f} | "
          f"{flops / a / 1e6:.0f} | {wbytes / a / 1e6:.2f} |", flush=True)
