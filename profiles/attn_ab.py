#!/usr/bin/env python3
"""A/B of two builds of libpplhip.so on the attention operator: same outputs, same speed.

    PPLHIP_LIB=<lib> python profiles/attn_ab.py [--shapes NAME,...]      one build: a JSON line per shape (median us, SHA-256 of the output)
    python profiles/attn_ab.py --ab PARENT_LIB HEAD_LIB [--rounds 3] [--log FILE]

--ab runs the two libraries alternately (P H P H ..., a fresh process each) and judges per shape: the hashes must be equal in every
round; the allowed time difference is the parent's own spread (max - min of its rounds' medians) -- the head's median must lie within
that of the parent's median.  Inputs are seeded (torch's Philox generator): every process sees the same bytes.
Shapes: the decode launches the sources' comments quote (B 1024 x kv 512 / 1024, 32 heads), config 4's (B 256, kv 2000, 8 query heads
on 1 KV head: the grouped-query kernel), a split-K launch; prefill 1 x 8192, 16 x 512, 1 x 2048 behind a 6144-token cache, 1 x 16
behind 8176 tokens with a workspace (split-KV), and a head_dim-64 launch for the 16-row kernel.  int8-g8 KV, layout 3, pages of 16."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, decode rows, requests, new tokens per request, tokens already cached, H, Hkv, D, decode splits, workspace
SHAPES = [
    ("dec_b1024_kv512_h32", True, 1024, 1, 511, 32, 32, 128, 1, False),
    ("dec_b1024_kv1024_h32", True, 1024, 1, 1023, 32, 32, 128, 1, False),
    ("dec_b256_kv2000_h8x1", True, 256, 1, 1999, 8, 1, 128, 1, False),
    ("dec_b8_kv8192_h32_split8", True, 8, 1, 8191, 32, 32, 128, 8, True),
    ("pf_1x8192", False, 1, 8192, 0, 32, 32, 128, 1, False),
    ("pf_16x512", False, 16, 512, 0, 32, 32, 128, 1, False),
    ("pf_1x2048_behind_6144", False, 1, 2048, 6144, 32, 32, 128, 1, False),
    ("pf_1x16_behind_8176_splitkv", False, 1, 16, 8176, 32, 32, 128, 1, True),
    ("pf_4x1024_d64", False, 4, 1024, 0, 32, 32, 64, 1, False),
]
PG, ITERS, WARMUP = 16, 20, 3


def run_shapes(only):
    import numpy as np
    import torch
    from tests.conftest import load_pplhip
    m = load_pplhip()
    for name, dec, R, S, P, H, HKV, D, split, want_ws in [s for s in SHAPES if not only or s[0] in only]:
        torch.manual_seed(1234)
        per = (P + S + PG - 1) // PG * PG
        N = R * per
        cache = torch.randint(-127, 128, (2 * HKV * N * D,), dtype=torch.int8, device="cuda")
        scale = (torch.rand(2 * HKV * N * D // 8, device="cuda") * 0.02 + 0.01).half()
        qkv = torch.randn(R * S, (H + 2 * HKV) * D, device="cuda").half()
        out = torch.zeros(R * S, H * D, device="cuda", dtype=torch.float16)
        seq = torch.arange(R + 1, device="cuda", dtype=torch.int64) * S
        sp = torch.full((R,), P, device="cuda", dtype=torch.int64)
        mp = per // PG
        ci = torch.from_numpy(np.random.RandomState(0).permutation(N // PG).astype(np.int64).reshape(R, mp)).cuda()
        v = m.KvView()
        v.cache, v.scale, v.max_tokens, v.num_layers, v.kv_heads, v.head_dim = cache.data_ptr(), scale.data_ptr(), N, 1, HKV, D
        v.quant_bit, v.quant_group, v.layout, v.mode, v.page_size, v.layer = 8, 8, 3, 1, PG, 0
        n_ws = R * S * H * (split if dec else 32) * (D + 2) if want_ws else 0
        ws = torch.zeros(n_ws, device="cuda", dtype=torch.float32) if n_ws else None

        def call():
            return m.lib().pplhip_op_attention(None, qkv.data_ptr(), C.byref(v), seq.data_ptr(), sp.data_ptr(), ci.data_ptr(), mp, R, R * S,
                                               R if dec else 0, S, P + S, H, split, ws.data_ptr() if ws is not None else None, n_ws * 4,
                                               out.data_ptr())
        for _ in range(WARMUP):
            assert call() == 0, name
        torch.cuda.synchronize()
        times = []
        for _ in range(ITERS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        digest = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
        print(json.dumps({"shape": name, "median_us": round(statistics.median(times), 2), "sha256": digest}), flush=True)
        del cache, scale, qkv, out, ws
        torch.cuda.empty_cache()


def ab(parent, head, rounds, log):
    series = {"parent": [], "head": []}   # per round: {shape: (median_us, sha256)}
    for i in range(rounds):
        for tag, lib in (("parent", parent), ("head", head)):
            print(f"round {i + 1} of {rounds}: {tag}", file=sys.stderr, flush=True)
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, PPLHIP_LIB=os.path.abspath(lib)),
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:   # a failed run ends the comparison: nothing more is started on the device
                sys.exit(f"{tag} run failed with status {r.returncode}:\n{r.stdout}\n{r.stderr}")
            rows = [json.loads(ln) for ln in r.stdout.split("\n") if ln.startswith("{")]
            series[tag].append({x["shape"]: (x["median_us"], x["sha256"]) for x in rows})
    lines, ok = [], True
    for name in [s[0] for s in SHAPES]:
        tp = [rd[name][0] for rd in series["parent"]]
        th = [rd[name][0] for rd in series["head"]]
        hashes = {rd[name][1] for tag in series for rd in series[tag]}
        spread, dm = max(tp) - min(tp), statistics.median(th) - statistics.median(tp)
        good = len(hashes) == 1 and abs(dm) <= spread
        ok &= good
        lines.append(f"{name}: parent us {tp} head us {th} | parent spread {spread:.2f} head - parent {dm:+.2f} | "
                     f"hashes {'equal' if len(hashes) == 1 else 'DIFFER'} {sorted(hashes)[0][:16]} | {'ok' if good else 'MISS'}")
    lines.append("verdict: " + ("every shape: equal outputs, head median within the parent's spread" if ok else "MISS"))
    text = "\n".join(lines)
    print(text)
    if log:
        open(log, "w").write(text + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ab", nargs=2, metavar=("PARENT_LIB", "HEAD_LIB"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log")
    ap.add_argument("--shapes", help="one build only: comma-separated shape names (default: all), e.g. under a profiler")
    a = ap.parse_args()
    if a.ab:
        ab(a.ab[0], a.ab[1], a.rounds, a.log)
    else:
        run_shapes(a.shapes.split(",") if a.shapes else None)
