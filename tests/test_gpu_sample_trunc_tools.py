"""min_p / typical_p through the whole host stack on the GPU (tiny config): a scenario through tools/offline_inference and the same requests
through pplsrv_submit_sampling of the serving C API.  With top_k 0, temperature 3 and min_p = 1 only the most probable token survives the
cut, so every answer equals the greedy run's token for token; the same requests without the key are sampled and differ; and a request
answers alike in a batch of four and alone."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "ppl.llm.serving_amd")
CFG = os.path.join(PKG, "configs", "tiny_w8a16_kv8_paged.json")
GEN = 8
PROMPTS = [[11, 12, 13, 14, 15], [21, 22, 23], [31, 32, 33, 34], [41], [51, 52, 53, 54, 55, 56, 57], [61, 62]]
SAMPLED = dict(top_k=0, top_p=1.0, temperature=3.0)
GREEDY = dict(top_k=1, top_p=0.0, temperature=3.0)


def scenario(params, batch=4, **extra):
    reqs = [dict(id=i, tokens=p, seed=100 + i, generation_length=GEN, early_stopping=False, **params, **extra) for i, p in enumerate(PROMPTS)]
    return {"generator": {"max_running_batch": batch, "max_tokens_per_step": 64, "max_prefill_batch": 2}, "kv_cache_max_tokens": 1024,
            "requests": reqs}


def run(tmp_path, name, sc, flags=("--per-request-sampling", "--sampling-seed", "5")):
    path = str(tmp_path / (name + ".json"))
    json.dump(sc, open(path, "w"))
    tool = os.path.join(PKG, "build", "offline_inference")
    assert os.path.exists(tool), f"{tool} missing: run __graft_entry__.build()"
    out = subprocess.check_output([tool, "--model-param-path", CFG, "--synthetic-weights", "--workload", "scenario", "--scenario-file", path,
                                   *flags], timeout=300, stderr=subprocess.DEVNULL).decode()
    res = json.loads(out.strip().splitlines()[-1])
    return {int(k): v for k, v in res["tokens"].items()}, res["failed"]


@pytest.fixture(scope="module")
def greedy(tmp_path_factory):
    tokens, failed = run(tmp_path_factory.mktemp("trunc_tools"), "greedy", scenario(GREEDY))
    assert failed == [] and all(len(t) == GEN for t in tokens.values())
    return tokens


def test_min_p_one_is_the_greedy_run(greedy, tmp_path):
    tokens, failed = run(tmp_path, "minp", scenario(SAMPLED, min_p=1.0))
    assert failed == [] and tokens == greedy
    # the same requests without the key are sampled at temperature 3
    plain, failed = run(tmp_path, "plain", scenario(SAMPLED))
    assert failed == [] and any(plain[i] != greedy[i] for i in greedy)
    # typical_p is read too: the typical set of a sampled request is not the whole distribution (a fixed outcome of the fixed seeds)
    typical, failed = run(tmp_path, "typical", scenario(SAMPLED, typical_p=0.2))
    assert failed == [] and any(typical[i] != plain[i] for i in plain)


def test_batch_of_four_equals_batch_of_one(tmp_path):
    sc = scenario(SAMPLED, min_p=0.3, typical_p=0.9)
    four, failed = run(tmp_path, "four", sc)
    assert failed == []
    one, failed = run(tmp_path, "one", scenario(SAMPLED, batch=1, min_p=0.3, typical_p=0.9))
    assert failed == [] and one == four


def test_a_request_that_asks_fails_alone_without_per_request_sampling(tmp_path):
    sc = scenario(GREEDY)
    sc["requests"][2]["min_p"] = 0.1
    sc["requests"][4]["typical_p"] = 0.5
    tokens, failed = run(tmp_path, "switch_off", sc, flags=())
    assert failed == [2, 4] and sorted(tokens) == [0, 1, 3, 5]


def test_submit_sampling_through_the_serving_c_api():
    pytest.importorskip("grpc")
    sys.path.insert(0, os.path.join(PKG, "serving"))
    import argparse
    import grpc_server as gs
    ap = argparse.ArgumentParser()
    gs.add_flags(ap)
    a = ap.parse_args(["--model-param-path", CFG, "--synthetic-weights", "--kv-cache-max-tokens", "1024", "--max-running-batch", "4",
                       "--max-tokens-per-step", "64"])
    lib = gs.load_lib()
    assert hasattr(lib, "pplsrv_submit_sampling")
    lib.pplsrv_submit_sampling.argtypes = [C.c_void_p, C.POINTER(gs.CRequest), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                           C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                           C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32]
    h = C.c_void_p()
    assert lib.pplsrv_create_ex(C.byref(gs.make_config(a)), 1, 5, C.byref(h)) == 0
    next_id = [0]

    def ask(params, min_p=None, typical_p=None):
        cnt = len(PROMPTS)
        keep, reqs, seeds = [], (gs.CRequest * cnt)(), (C.c_uint64 * cnt)(*[100 + i for i in range(cnt)])
        base = next_id[0]
        next_id[0] += cnt
        for i, p in enumerate(PROMPTS):
            toks = (C.c_int32 * len(p))(*p)
            keep.append(toks)
            q = reqs[i]
            q.id, q.tokens, q.n_tokens = base + i, toks, len(p)
            q.temperature, q.top_p, q.top_k = params["temperature"], params["top_p"], params["top_k"]
            q.repetition_penalty, q.generation_length, q.early_stopping = 1.0, GEN, 0
        mp = None if min_p is None else (C.c_float * cnt)(*[min_p] * cnt)
        ty = None if typical_p is None else (C.c_float * cnt)(*[typical_p] * cnt)
        assert lib.pplsrv_submit_sampling(h, reqs, None, seeds, None, None, None, None, None, mp, ty, cnt) == 0
        seen, failed, done = {i: [] for i in range(cnt)}, [], 0
        buf = (gs.CResponse * 64)()
        t0 = time.time()
        while done < cnt and time.time() - t0 < 120:
            for k in range(lib.pplsrv_poll(h, buf, 64, 50)):
                r = buf[k]
                if r.status == gs.P.FAILED:
                    failed.append(r.id - base)
                else:
                    seen[r.id - base].append(r.token)
                done += r.status != gs.P.PROCESSING
        assert done == cnt and failed == []
        return seen

    try:
        greedy = ask(GREEDY)
        assert all(len(t) == GEN for t in greedy.values())
        assert ask(SAMPLED, min_p=1.0) == greedy
        plain = ask(SAMPLED)
        assert any(plain[i] != greedy[i] for i in greedy)
        assert ask(SAMPLED, min_p=-1.0, typical_p=1.0) == plain       # both off: the requests of a call without the arrays
    finally:
        lib.pplsrv_destroy(h)
