"""Top-N logprobs through the whole host stack on the GPU: a scenario through tools/offline_inference with "num_logprobs" on some requests,
and a request through the gRPC server.  In both the lists are present exactly where they were asked for and entry 0 is the streamed token
under greedy sampling.  On the wire, messages that leave the new fields unset are byte for byte what they were."""
import json
import math
import os
import socket
import subprocess
import sys
import time

import pytest

from tests import top_logprobs as T
from tests.test_gpu_tools import CFG, PKG

pytestmark = pytest.mark.gpu
GEN = 5
ASK = {0: 0, 1: 3, 2: 20, 3: 0, 4: 1, 5: 25}              # 25: clamped to 20


def test_scenario_through_offline_inference(tmp_path):
    reqs = [dict(id=i, tokens=[10 * i + 11 + j for j in range(2 + i)], top_k=1, generation_length=GEN, early_stopping=False, num_logprobs=n)
            for i, n in ASK.items()]
    sc = {"generator": {"max_running_batch": 4, "max_tokens_per_step": 64, "max_prefill_batch": 2}, "kv_cache_max_tokens": 1024, "requests": reqs}
    path = str(tmp_path / "scenario.json")
    json.dump(sc, open(path, "w"))
    tool = os.path.join(PKG, "build", "offline_inference")
    assert os.path.exists(tool), f"{tool} missing: run __graft_entry__.build()"
    out = subprocess.check_output([tool, "--model-param-path", CFG, "--synthetic-weights", "--workload", "scenario", "--scenario-file", path],
                                  timeout=300, stderr=subprocess.DEVNULL).decode()
    res = json.loads(out.strip().splitlines()[-1])
    assert res["failed"] == [] and all(len(res["tokens"][str(i)]) == GEN for i in ASK)
    asking = sorted(str(i) for i, n in ASK.items() if n)
    assert sorted(res["top_tokens"]) == sorted(res["top_logprobs"]) == asking
    for i in asking:
        n = min(ASK[int(i)], 20)
        toks, lps = res["top_tokens"][i], res["top_logprobs"][i]
        assert len(toks) == len(lps) == GEN
        for step in range(GEN):
            assert len(toks[step]) == len(lps[step]) == n
            assert toks[step][0] == res["tokens"][i][step]                      # greedy: the best alternative is the answer
            assert len(set(toks[step])) == n and all(0 <= t < 1024 for t in toks[step])
            assert all(a >= b for a, b in zip(lps[step], lps[step][1:])) and lps[step][0] <= 0
    # the same scenario with nobody asking: the same answers, and today's output line
    for r in reqs:
        del r["num_logprobs"]
    json.dump(sc, open(path, "w"))
    out = subprocess.check_output([tool, "--model-param-path", CFG, "--synthetic-weights", "--workload", "scenario", "--scenario-file", path],
                                  timeout=300, stderr=subprocess.DEVNULL).decode()
    plain = json.loads(out.strip().splitlines()[-1])
    assert sorted(plain) == ["failed", "tokens"] and plain["tokens"] == res["tokens"]


@pytest.fixture
def server():
    """serving/grpc_server.py on the tiny model, as tests/test_gpu_grpc.py starts it"""
    pytest.importorskip("grpc")
    assert os.path.exists(os.path.join(PKG, "build", "libpplserving_c.so")), "run __graft_entry__.build()"
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    proc = subprocess.Popen([sys.executable, os.path.join(PKG, "serving", "grpc_server.py"), "--model-param-path", CFG, "--synthetic-weights",
                             "--synthetic-seed", "77", "--kv-cache-max-tokens", "2048", "--max-running-batch", "16", "--max-tokens-per-step",
                             "256", "--host", "127.0.0.1", "--port", str(port)], stderr=subprocess.PIPE, text=True)
    line = ""
    t0 = time.time()
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


def test_request_through_the_grpc_server(server):
    import grpc
    sys.path.insert(0, os.path.join(PKG, "serving"))
    import llm_proto as P
    asks = ((1, 0), (2, 4), (3, 20))
    with grpc.insecure_channel(server) as ch:
        stub = ch.unary_stream(P.METHOD, request_serializer=P.BatchedRequest.SerializeToString, response_deserializer=P.BatchedResponse.FromString)
        br = P.BatchedRequest()
        for rid, n in asks:
            r = br.req.add()
            r.id = rid
            r.tokens.ids.extend([5, 6, 7 + rid])
            r.stopping_parameters.max_new_tokens = GEN
            r.stopping_parameters.ignore_eos_token = True
            if n:
                r.choosing_parameters.top_logprobs = n
        seen = {rid: [] for rid, _ in asks}
        for batch in stub(br, timeout=120):
            for rsp in batch.rsp:
                assert rsp.status != P.FAILED
                seen[rsp.id].append((list(rsp.tokens.ids), list(rsp.detail.top_tokens), list(rsp.detail.top_logprobs), rsp.detail.logprobs))
    # the sampler's own logprob of the same token: the two kernels' bounds added, for a vocabulary of 1024 and |lse|, |logprob| <= 64
    both = T.entry_bound(1024, math.log(1024), 64.0, 64.0) + T.greedy_bound(1024, math.log(1024), 64.0, 64.0)
    for rid, n in asks:
        assert len(seen[rid]) == GEN
        for ids, top, lps, lp in seen[rid]:
            assert len(top) == len(lps) == n
            if n:
                assert top[0] == ids[0] and abs(lp) <= 64 and abs(lps[0] - lp) <= both
                assert len(set(top)) == n and all(a >= b for a, b in zip(lps, lps[1:]))


def test_wire_bytes_without_the_new_fields_are_todays():
    """the same messages through descriptors without fields 16 / 17: equal bytes; and the new fields travel past them as unknown fields"""
    sys.path.insert(0, os.path.join(PKG, "serving"))
    import llm_proto as P
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    fdp = descriptor_pb2.FileDescriptorProto()
    P._POOL.FindFileByName("ppl_llm.proto").CopyToProto(fdp)
    dropped = 0
    for msg in fdp.message_type:
        for f in [f for f in msg.field if f.number >= 16]:
            msg.field.remove(f)
            dropped += 1
    assert dropped == 3
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    old = lambda name: message_factory.GetMessageClass(pool.FindMessageTypeByName(f"{P.PKG}.{name}"))

    def fill_request(br):
        r = br.req.add()
        r.id, r.prompt = 7, "hi"
        r.tokens.ids.extend([1, 2, 300])
        cp = r.choosing_parameters
        cp.temperature, cp.top_k, cp.top_p, cp.do_sample, cp.seed, cp.repetition_penalty = 0.7, 50, 0.9, True, 12345, 1.1
        r.stopping_parameters.max_new_tokens = 9
        return br

    def fill_response(b):
        r = b.rsp.add()
        r.status, r.id = P.FINISHED, 7
        r.tokens.ids.append(42)
        r.detail.logprobs, r.detail.is_special, r.detail.finish_reason = -0.25, True, 1
        return b

    assert fill_request(P.BatchedRequest()).SerializeToString() == fill_request(old("BatchedRequest")()).SerializeToString()
    assert fill_response(P.BatchedResponse()).SerializeToString() == fill_response(old("BatchedResponse")()).SerializeToString()
    new = fill_response(P.BatchedResponse())
    new.rsp[0].detail.top_tokens.extend([42, 7])
    new.rsp[0].detail.top_logprobs.extend([-0.25, -2.0])
    seen_by_old = old("BatchedResponse").FromString(new.SerializeToString())
    assert seen_by_old.rsp[0].tokens.ids == [42] and seen_by_old.rsp[0].detail.finish_reason == 1
    assert len(new.SerializeToString()) > len(fill_response(P.BatchedResponse()).SerializeToString())
