"""Prompt logprobs through the whole host stack on the GPU: offline_inference --prompt-logprobs on the four fixed prompts, a scenario with
mixed asks (the generated tokens of every request equal the run without asks), the prefix cache (an asking request gives bit for bit the
per-position numbers of a cold cache although an identical prompt is cached, and a request that does not ask hits what an asking one
published), and the serving C API variants pplsrv_submit_prompt_logprobs / pplsrv_poll_prompt_logprobs."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import pytest

from tests.test_gpu_tools import CFG, PKG

pytestmark = pytest.mark.gpu
VOCAB = 1024
TOOL = os.path.join(PKG, "build", "offline_inference")


def _scenario(tmp_path, name, gen, reqs):
    path = str(tmp_path / name)
    json.dump({"generator": gen, "kv_cache_max_tokens": 1024, "requests": reqs}, open(path, "w"))
    assert os.path.exists(TOOL), f"{TOOL} missing: run __graft_entry__.build()"
    out = subprocess.check_output([TOOL, "--model-param-path", CFG, "--synthetic-weights", "--workload", "scenario", "--scenario-file", path],
                                  timeout=300, stderr=subprocess.DEVNULL).decode()
    return json.loads(out.strip().splitlines()[-1])


def _check_request(res, rid, prompt, n):
    """the shape and the inner consistency of one asking request's lists"""
    lp, rk = res["prompt_logprobs"][rid], res["prompt_ranks"][rid]
    tt, tl = res["prompt_top_tokens"][rid], res["prompt_top_logprobs"][rid]
    P = len(prompt) - 1
    assert len(lp) == len(rk) == len(tt) == len(tl) == P
    for i in range(P):
        assert lp[i] < 0 and 0 <= rk[i] < VOCAB and len(tt[i]) == len(tl[i]) == n
        assert len(set(tt[i])) == n and all(a >= b for a, b in zip(tl[i], tl[i][1:]))
        if rk[i] < n:                                    # the target inside its own ranking: one number, at its rank
            assert tt[i][rk[i]] == prompt[i + 1] and tl[i][rk[i]] == lp[i]
        else:
            assert prompt[i + 1] not in tt[i] and (n == 0 or lp[i] <= tl[i][-1])


def test_flag_on_the_fixed_prompts():
    args = [TOOL, "--model-param-path", CFG, "--synthetic-weights", "--synthetic-seed", "77", "--kv-cache-max-tokens", "512",
            "--max-running-batch", "8", "--max-tokens-per-step", "64", "--workload", "prompts4"]
    out = subprocess.check_output(args + ["--prompt-logprobs", "2"], timeout=300, stderr=subprocess.DEVNULL).decode().splitlines()
    plain = subprocess.check_output(args, timeout=300, stderr=subprocess.DEVNULL).decode().splitlines()
    prompts = [[int(x) % VOCAB for x in l.split(":")[1].split()] for l in out if l.startswith("Prompt tokens:")]
    assert [l for l in out if l.startswith("Answer tokens:")] == [l for l in plain if l.startswith("Answer tokens:")]
    assert not [l for l in plain if l.startswith("Prompt logprob")]
    lines = [l[len("Prompt logprobs:"):] for l in out if l.startswith("Prompt logprobs:")]
    sums = [float(l.split(":")[1]) for l in out if l.startswith("Prompt logprob sum:")]
    assert len(prompts) == len(lines) == len(sums) == 4
    for p, line, total in zip(prompts, lines, sums):
        pos = [s.strip() for s in line.split("|")]
        assert len(pos) == len(p) - 1
        acc = 0.0
        for i, s in enumerate(pos):
            head, alts = s.split(" [")
            tok, lp, rank = head.split(":")
            assert int(tok) == p[i + 1] and float(lp) < 0 and 0 <= int(rank) < VOCAB
            alts = [(int(a.split(":")[0]), float(a.split(":")[1])) for a in alts.rstrip("]").split()]
            assert len(alts) == 2 and alts[0][1] >= alts[1][1]
            if int(rank) < 2:
                assert alts[int(rank)] == (int(tok), float(lp))
            acc += float(lp)
        assert abs(acc - total) <= 1e-5 * max(1.0, abs(total))


def test_scenario_with_mixed_asks(tmp_path):
    prompts = {i: [10 * i + 11 + j for j in range(n)] for i, n in enumerate((4, 1, 2, 9, 6, 3))}
    ask = {0: -1, 1: 0, 2: 3, 3: 0, 4: 25, 5: -7}        # 25: clamped to 20; -7: off
    reqs = [dict(id=i, tokens=p, top_k=1, generation_length=4, early_stopping=False, prompt_logprobs=ask[i]) for i, p in prompts.items()]
    gen = {"max_running_batch": 4, "max_tokens_per_step": 64, "max_prefill_batch": 2}
    res = _scenario(tmp_path, "asks.json", gen, reqs)
    assert res["failed"] == [] and all(len(res["tokens"][str(i)]) == 4 for i in prompts)
    asking = sorted(str(i) for i, n in ask.items() if n >= 0)
    for key in ("prompt_logprobs", "prompt_ranks", "prompt_top_tokens", "prompt_top_logprobs"):
        assert sorted(res[key]) == asking
    for i in asking:
        _check_request(res, i, prompts[int(i)], min(ask[int(i)], 20))
    assert res["prompt_logprobs"]["1"] == []             # a prompt of one token has no position
    for r in reqs:
        del r["prompt_logprobs"]
    plain = _scenario(tmp_path, "plain.json", gen, reqs)
    assert sorted(plain) == ["failed", "tokens"] and plain["tokens"] == res["tokens"]


def test_prefix_cache_changes_nothing_for_an_asking_request(tmp_path):
    """every request generates one token and max_prefill_batch is 1 under the prefix cache, so a step is one prompt alone: the asking
    request's step is the same launch on a cold cache and behind an identical cached prompt"""
    shared = [100 + j for j in range(11)]                # two full pages of four tokens and a tail
    other = [300 + j for j in range(6)]
    req = lambda i, tokens, n: dict(id=i, tokens=tokens, top_k=1, generation_length=1, early_stopping=False, prompt_logprobs=n)
    gen = {"max_running_batch": 4, "max_tokens_per_step": 64, "enable_prefix_cache": True}
    cold = _scenario(tmp_path, "cold.json", gen, [req(0, shared, 5)])
    warm = _scenario(tmp_path, "warm.json", gen, [req(0, shared, -1), req(1, shared, 5), req(2, other, 0), req(3, shared, -1), req(4, shared, 20)])
    assert cold["failed"] == warm["failed"] == []
    _check_request(cold, "0", shared, 5)
    for key in ("prompt_logprobs", "prompt_ranks", "prompt_top_tokens", "prompt_top_logprobs"):
        assert sorted(warm[key]) == ["1", "2", "4"]
        assert warm[key]["1"] == cold[key]["0"], key                                   # as printed: nine digits name a float32
    assert warm["prompt_logprobs"]["4"] == cold["prompt_logprobs"]["0"] and warm["prompt_ranks"]["4"] == cold["prompt_ranks"]["0"]
    assert [t[:5] for t in warm["prompt_top_tokens"]["4"]] == cold["prompt_top_tokens"]["0"]
    assert warm["tokens"]["0"] == warm["tokens"]["1"] == warm["tokens"]["4"] == cold["tokens"]["0"] and len(warm["tokens"]["3"]) == 1
    # without the prefix cache the same numbers again
    off = _scenario(tmp_path, "off.json", {"max_running_batch": 4, "max_tokens_per_step": 64, "max_prefill_batch": 1}, [req(0, shared, 5)])
    assert off["prompt_logprobs"] == cold["prompt_logprobs"] and off["prompt_top_tokens"] == cold["prompt_top_tokens"]


class CPrompt(C.Structure):
    _fields_ = [("positions", C.c_int32), ("n_top", C.c_int32), ("off", C.c_int64), ("top_off", C.c_int64)]


def test_serving_c_api():
    pytest.importorskip("grpc")
    sys.path.insert(0, os.path.join(PKG, "serving"))
    import argparse
    import grpc_server as gs
    ap = argparse.ArgumentParser()
    gs.add_flags(ap)
    a = ap.parse_args(["--model-param-path", CFG, "--synthetic-weights", "--synthetic-seed", "77", "--kv-cache-max-tokens", "2048",
                       "--max-running-batch", "16", "--max-tokens-per-step", "256"])
    lib = gs.load_lib()
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    lib.pplsrv_submit_prompt_logprobs.argtypes = [C.c_void_p, C.POINTER(gs.CRequest), i32p, C.POINTER(C.c_uint64), i32p, C.c_void_p, i32p, C.c_int32]
    lib.pplsrv_poll_prompt_logprobs.argtypes = [C.c_void_p, C.POINTER(gs.CResponse), C.c_int32, C.c_int32, C.c_char_p, C.c_int64, C.c_void_p,
                                                C.POINTER(CPrompt), f32p, i32p, C.c_int64, i32p, f32p, C.c_int64]
    h = C.c_void_p()
    assert lib.pplsrv_create_ex(C.byref(gs.make_config(a)), 0, 0, C.byref(h)) == 0
    prompts = [[5, 6, 7, 8, 9], [5, 6, 7, 8, 9], [21], [31, 32, 33]]
    GEN = 3

    def run(asks, cap=64, top_cap=1024):
        n = len(prompts)
        keep, reqs = [], (gs.CRequest * n)()
        for i, p in enumerate(prompts):
            toks = (C.c_int32 * len(p))(*p)
            keep.append(toks)
            q = reqs[i]
            q.id, q.tokens, q.n_tokens = i, toks, len(p)
            q.temperature, q.top_p, q.top_k, q.repetition_penalty, q.generation_length, q.early_stopping = 1.0, 0.0, 1, 1.0, GEN, 0
        assert lib.pplsrv_submit_prompt_logprobs(h, reqs, None, None, None, None, None if asks is None else (C.c_int32 * n)(*asks), n) == 0
        tokens, lists, done = {i: [] for i in range(n)}, {i: [] for i in range(n)}, 0
        buf, recs = (gs.CResponse * 64)(), (CPrompt * 64)()
        lp, rk = (C.c_float * cap)(), (C.c_int32 * cap)()
        tt, tl = (C.c_int32 * top_cap)(), (C.c_float * top_cap)()
        t0 = time.time()
        while done < n and time.time() - t0 < 120:
            for k in range(lib.pplsrv_poll_prompt_logprobs(h, buf, 64, 50, None, 0, None, recs, lp, rk, cap, tt, tl, top_cap)):
                r, pr = buf[k], recs[k]
                assert r.status != gs.P.FAILED
                tokens[r.id].append(r.token)
                P, nt = pr.positions, pr.n_top
                assert (pr.off >= 0) == (P > 0) and (pr.top_off >= 0) == (P > 0 and nt > 0)
                lists[r.id].append((list(lp[pr.off:pr.off + P]), list(rk[pr.off:pr.off + P]),
                                    [list(tt[pr.top_off + j * nt:pr.top_off + (j + 1) * nt]) for j in range(P)] if nt else [],
                                    [list(tl[pr.top_off + j * nt:pr.top_off + (j + 1) * nt]) for j in range(P)] if nt else []) if P else None)
                done += r.status != gs.P.PROCESSING
        assert done == n
        return tokens, lists

    try:
        plain_tokens, plain = run(None)
        assert all(v == [None] * GEN for v in plain.values())
        tokens, lists = run([0, 20, 4, -1])
        assert tokens == plain_tokens                    # the ask changes nobody's answer
        assert lists[2] == [None] * GEN and lists[3] == [None] * GEN               # one token: no position; -1: off
        for i, n in ((0, 0), (1, 20)):
            first, rest = lists[i][0], lists[i][1:]
            assert rest == [None] * (GEN - 1)            # with the first token only
            lp, rk, tt, tl = first
            assert len(lp) == len(rk) == 4 and all(v < 0 for v in lp) and all(0 <= r < VOCAB for r in rk)
            assert (tt, tl) == ([], []) if n == 0 else (len(tt) == 4 and all(len(t) == n for t in tt))
        assert lists[0][0][:2] == lists[1][0][:2]        # the same prompt in one step: the same numbers whatever n is
        for j, r in enumerate(lists[1][0][1]):
            if r < 20:
                assert lists[1][0][2][j][r] == prompts[1][j + 1] and lists[1][0][3][j][r] == lists[1][0][0][j]
    finally:
        lib.pplsrv_destroy(h)
