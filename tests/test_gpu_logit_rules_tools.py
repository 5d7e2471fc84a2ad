"""Logit rules through the whole host stack on the GPU: a scenario through tools/offline_inference with "allowed_tokens", "banned_tokens",
"logit_bias" and "min_new_tokens" on some requests and an invalid rule on one, with and without the penalty step; the same scenario
without the keys gives today's output; then rules beside plain requests through pplsrv_submit_rules of the serving C API."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import pytest

from tests.test_gpu_tools import CFG, PKG

pytestmark = pytest.mark.gpu
GEN = 12
VOCAB = 1024


def _offline(path):
    tool = os.path.join(PKG, "build", "offline_inference")
    assert os.path.exists(tool), f"{tool} missing: run __graft_entry__.build()"
    out = subprocess.check_output([tool, "--model-param-path", CFG, "--synthetic-weights", "--workload", "scenario", "--scenario-file", path],
                                  timeout=300, stderr=subprocess.DEVNULL).decode()
    line = out.strip().splitlines()[-1]
    return line, json.loads(line)


@pytest.mark.parametrize("penalty", [False, True])
def test_scenario_through_offline_inference(tmp_path, penalty):
    reqs = [dict(id=i, tokens=[10 * i + 11 + j for j in range(2 + i)], top_k=1, generation_length=GEN, early_stopping=True,
                 repetition_penalty=1.2 if penalty else 1.0) for i in range(6)]
    sc = {"generator": {"max_running_batch": 4, "max_tokens_per_step": 64, "max_prefill_batch": 2, "enable_penalty": penalty},
          "kv_cache_max_tokens": 1024, "requests": reqs}
    path = str(tmp_path / "scenario.json")
    json.dump(sc, open(path, "w"))
    plain_line, plain = _offline(path)                   # the plain scenario first: it names the tokens the rules are built around
    assert plain["failed"] == [] and sorted(plain) == ["failed", "tokens"]
    first = {i: plain["tokens"][str(i)][0] for i in range(6)}
    allowed = [17, 300, 301, 640, 1023]
    stop = 777
    assert all(stop not in plain["tokens"][str(i)] for i in range(6))
    ruled = json.loads(json.dumps(sc))
    r = ruled["requests"]
    r[0]["allowed_tokens"] = allowed
    r[1]["banned_tokens"] = [first[1]]
    r[2].update(min_new_tokens=4, stop_tokens=[stop], logit_bias=[[stop, 30.0]])
    r[3]["logit_bias"] = [[VOCAB, 1.0]]                  # outside the vocabulary: this request fails, alone
    r[4]["logit_bias"] = [[first[4], "-inf"]]            # a ban written as a bias
    json.dump(ruled, open(path, "w"))
    _, res = _offline(path)
    assert res["failed"] == [3] and sorted(res["tokens"]) == ["0", "1", "2", "4", "5"]
    assert len(res["tokens"]["0"]) == GEN and set(res["tokens"]["0"]) <= set(allowed)
    assert len(res["tokens"]["1"]) == GEN and res["tokens"]["1"][0] != first[1] and first[1] not in res["tokens"]["1"]
    # four tokens that are not the stop, then the stop (its +30 wins as soon as it may), and the request is over long before GEN tokens
    assert res["tokens"]["2"][4] == stop and stop not in res["tokens"]["2"][:4] and len(res["tokens"]["2"]) == 5
    assert res["tokens"]["4"][0] != first[4] and first[4] not in res["tokens"]["4"]
    assert res["tokens"]["5"] == plain["tokens"]["5"]    # the neighbour without a rule answers as before
    # without the keys: today's output line
    json.dump(sc, open(path, "w"))
    again_line, _ = _offline(path)
    assert again_line == plain_line


class CRule(C.Structure):   # pplsrv_rule of src/capi/serving_c.h
    _fields_ = [("bias_tokens", C.POINTER(C.c_int32)), ("bias_values", C.POINTER(C.c_float)), ("n_bias", C.c_int32),
                ("allowed_tokens", C.POINTER(C.c_int32)), ("n_allowed", C.c_int32), ("has_allowed", C.c_int32),
                ("banned_tokens", C.POINTER(C.c_int32)), ("n_banned", C.c_int32), ("min_new_tokens", C.c_int32)]


def _rule(keep, bias=(), allowed=None, banned=(), min_new_tokens=0):
    i32 = lambda v: (C.c_int32 * max(len(v), 1))(*v)
    arrs = (i32([t for t, _ in bias]), (C.c_float * max(len(bias), 1))(*[v for _, v in bias]), i32(allowed or []), i32(list(banned)))
    r = CRule(arrs[0], arrs[1], len(bias), arrs[2], len(allowed or []), int(allowed is not None), arrs[3], len(banned), min_new_tokens)
    keep.extend([arrs, r])
    return C.pointer(r)


def test_ctypes_mirror_of_pplsrv_rule(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "capi/serving_c.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(pplsrv_rule), offsetof(pplsrv_rule, allowed_tokens), '
                   'offsetof(pplsrv_rule, has_allowed), offsetof(pplsrv_rule, banned_tokens), offsetof(pplsrv_rule, min_new_tokens)); '
                   'return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-I", os.path.join(PKG, "src"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(CRule), CRule.allowed_tokens.offset, CRule.has_allowed.offset, CRule.banned_tokens.offset,
                   CRule.min_new_tokens.offset]


def test_rules_through_the_serving_c_api():
    """pplsrv_submit_rules, the entry point under the gRPC front end, without the penalty (only the asking requests take a slot): an
    allowed list, an invalid rule and two plain requests in one call; then a ban and a decisive bias"""
    pytest.importorskip("grpc")
    sys.path.insert(0, os.path.join(PKG, "serving"))
    import argparse
    import grpc_server as gs
    ap = argparse.ArgumentParser()
    gs.add_flags(ap)
    a = ap.parse_args(["--model-param-path", CFG, "--synthetic-weights", "--synthetic-seed", "77", "--kv-cache-max-tokens", "2048",
                       "--max-running-batch", "16", "--max-tokens-per-step", "256"])
    lib = gs.load_lib()
    lib.pplsrv_submit_rules.argtypes = [C.c_void_p, C.POINTER(gs.CRequest), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                        C.POINTER(C.POINTER(CRule)), C.c_int32]
    h = C.c_void_p()
    assert lib.pplsrv_create_ex(C.byref(gs.make_config(a)), 0, 0, C.byref(h)) == 0
    allowed = [9, 512, 513, 1000]
    next_id = [0]

    def ask(rules):
        n = len(rules)
        keep, reqs, ptrs = [], (gs.CRequest * n)(), (C.POINTER(CRule) * n)()
        base = next_id[0]
        next_id[0] += n
        for i, kw in enumerate(rules):
            toks = (C.c_int32 * 3)(5, 6, 7 + i % 2)                 # 0 and 2, 1 and 3 share a prompt
            keep.append(toks)
            q = reqs[i]
            q.id, q.tokens, q.n_tokens = base + i, toks, 3
            q.temperature, q.top_p, q.top_k, q.repetition_penalty, q.generation_length, q.early_stopping = 1.0, 0.0, 1, 1.0, 6, 0
            if kw is not None:
                ptrs[i] = _rule(keep, **kw)
        assert lib.pplsrv_submit_rules(h, reqs, None, None, None, ptrs, n) == 0
        seen, failed, done = {base + i: [] for i in range(n)}, [], 0
        buf = (gs.CResponse * 64)()
        t0 = time.time()
        while done < n and time.time() - t0 < 120:
            for k in range(lib.pplsrv_poll(h, buf, 64, 50)):
                r = buf[k]
                if r.status == gs.P.FAILED:
                    failed.append(r.id - base)
                else:
                    seen[r.id].append(r.token)
                done += r.status != gs.P.PROCESSING
        assert done == n
        return [seen[base + i] for i in range(n)], failed

    try:
        seen, failed = ask([dict(allowed=allowed), dict(bias=[(VOCAB, 1.0)]), None, None])
        assert failed == [1] and seen[1] == []
        assert len(seen[0]) == 6 and set(seen[0]) <= set(allowed)
        assert len(seen[2]) == len(seen[3]) == 6 and not set(seen[2]) <= set(allowed)
        first = seen[2][0]
        again, failed = ask([dict(banned=[first]), dict(bias=[(allowed[2], 60.0)]), None, None])
        assert failed == [] and again[2] == seen[2] and again[3] == seen[3]
        assert len(again[0]) == 6 and first not in again[0]
        assert again[1] == [allowed[2]] * 6
    finally:
        lib.pplsrv_destroy(h)
