"""choosing_parameters.seed over the wire: serving/grpc_server.py --per-request-sampling in a subprocess, a raw grpc client in the test.
With do_sample the same seed gives the same token stream, two seeds give two streams, and a do_sample = false request in the same
BatchedRequest behind a sampling one is answered greedily."""
import os
import subprocess
import sys
import time

import pytest

from tests.test_gpu_grpc import free_port
from tests.test_gpu_tools import CFG, PKG

pytestmark = pytest.mark.gpu
grpc = pytest.importorskip("grpc")
sys.path.insert(0, os.path.join(PKG, "serving"))
import llm_proto as P  # noqa: E402

PROMPT = [11, 12, 13, 14, 15]
N = 8
SEED_A, SEED_B = 1234567890123, 77                       # fixed: their streams differ (verified once on the device, kept)


@pytest.fixture(scope="module")
def server():
    assert os.path.exists(os.path.join(PKG, "build", "libpplserving_c.so")), "run __graft_entry__.build()"
    port = free_port()
    proc = subprocess.Popen([sys.executable, os.path.join(PKG, "serving", "grpc_server.py"), "--model-param-path", CFG,
                             "--synthetic-weights", "--synthetic-seed", "77", "--kv-cache-max-tokens", "2048", "--max-running-batch", "16",
                             "--max-tokens-per-step", "256", "--host", "127.0.0.1", "--port", str(port), "--per-request-sampling",
                             "--sampling-seed", "9"], stderr=subprocess.PIPE, text=True)
    t0 = time.time()
    line = ""
    while time.time() - t0 < 120:
        line = proc.stderr.readline()
        if "listening" in line or proc.poll() is not None:
            break
    assert "listening" in line, f"server did not start: {line}"
    yield f"127.0.0.1:{port}"
    proc.terminate()
    try:
        proc.wait(timeout=20)
    except subprocess.TimeoutExpired:
        proc.kill()


def call(target, reqs):
    """reqs: list of (id, tokens, seed or None for do_sample = false); returns {id: tokens}"""
    out = {}
    with grpc.insecure_channel(target) as ch:
        stub = ch.unary_stream(P.METHOD, request_serializer=P.BatchedRequest.SerializeToString,
                               response_deserializer=P.BatchedResponse.FromString)
        br = P.BatchedRequest()
        for rid, toks, seed in reqs:
            r = br.req.add()
            r.id = rid
            r.tokens.ids.extend(toks)
            r.stopping_parameters.max_new_tokens = N
            r.stopping_parameters.ignore_eos_token = True
            if seed is not None:
                cp = r.choosing_parameters
                cp.do_sample, cp.top_k, cp.top_p, cp.temperature, cp.seed = True, 0, 1.0, 200.0, seed
        for batch in stub(br, timeout=120):
            for rsp in batch.rsp:
                assert rsp.status != P.FAILED, rsp.id
                out.setdefault(rsp.id, []).extend(rsp.tokens.ids)
    assert all(len(t) == N for t in out.values()) and len(out) == len(reqs)
    return out


def test_same_seed_same_stream_and_other_seed_other_stream(server):
    a1 = call(server, [(1, PROMPT, SEED_A)])[1]
    b = call(server, [(2, PROMPT, SEED_B)])[2]
    both = call(server, [(3, PROMPT, SEED_B), (4, PROMPT, SEED_A), (5, PROMPT, SEED_A)])       # and in one batch, in another order
    assert both[4] == a1 and both[5] == a1 and both[3] == b
    assert a1 != b


def test_greedy_request_behind_a_sampling_one(server):
    # the same three prompts all greedy: the steps have the same shapes, so request 12's logits are the same numbers in both calls
    greedy = call(server, [(11, PROMPT, None), (12, PROMPT, None), (13, [21, 22, 23], None)])
    mixed = call(server, [(11, PROMPT, SEED_A), (12, PROMPT, None), (13, [21, 22, 23], SEED_B)])
    assert greedy[11] == greedy[12]
    assert mixed[12] == greedy[12]
    assert mixed[11] != greedy[11] and mixed[13] != greedy[13]        # the others were sampled (fixed outcome of the fixed seeds)
