"""The per-request sampler through the whole C++ host stack on the GPU: tools/offline_inference --per-request-sampling on a scenario that
mixes greedy and sampling requests.  Answers are a function of (prompt, parameters, seed) alone: two runs agree, equal requests answer
alike, swapping two seeds swaps two answers, and a greedy request is answered greedily whatever shares its batch."""
import copy
import json
import os
import subprocess

import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "ppl.llm.serving_amd")
CFG = os.path.join(PKG, "configs", "tiny_w8a16_kv8_paged.json")
GEN = 6
# a flat distribution over the whole vocabulary: the decisive synthetic head gives wide margins, the temperature takes them away again
SAMPLING = dict(top_k=0, top_p=1.0, temperature=200.0)
GREEDY = dict(top_k=1, top_p=0.0, temperature=0.7)
P1, P2 = [11, 12, 13, 14, 15], [21, 22, 23]


def scenario():
    reqs = [dict(id=0, tokens=P1, seed=101, **SAMPLING), dict(id=1, tokens=P1, seed=101, **SAMPLING),       # equal in everything
            dict(id=2, tokens=P2, seed=201, **SAMPLING), dict(id=3, tokens=P2, seed=202, **SAMPLING),       # equal but for the seed
            dict(id=4, tokens=[31, 32, 33, 34], **GREEDY), dict(id=5, tokens=[41], **GREEDY), dict(id=6, tokens=[51, 52, 53, 54, 55, 56, 57], **GREEDY),
            dict(id=7, tokens=[61, 62], seed=7, **SAMPLING), dict(id=8, tokens=[71, 72, 73], seed=8, top_k=50, top_p=0.9, temperature=150.0),
            dict(id=9, tokens=[81, 82, 83, 84], **SAMPLING)]                                                 # no seed: --sampling-seed's first
    for r in reqs:
        r.update(generation_length=GEN, early_stopping=False)
    return {"generator": {"max_running_batch": 4, "max_tokens_per_step": 64, "max_prefill_batch": 2}, "kv_cache_max_tokens": 1024,
            "requests": reqs}


def run(tmp_path, name, sc):
    path = str(tmp_path / (name + ".json"))
    json.dump(sc, open(path, "w"))
    tool = os.path.join(PKG, "build", "offline_inference")
    assert os.path.exists(tool), f"{tool} missing: run __graft_entry__.build()"
    out = subprocess.check_output([tool, "--model-param-path", CFG, "--synthetic-weights", "--synthetic-decisive-head", "7", "--workload", "scenario",
                                   "--scenario-file", path, "--per-request-sampling", "--sampling-seed", "5"], timeout=300,
                                  stderr=subprocess.DEVNULL).decode()
    res = json.loads(out.strip().splitlines()[-1])
    assert res["failed"] == [] and len(res["tokens"]) == len(sc["requests"])
    assert all(len(t) == GEN for t in res["tokens"].values())
    return {int(k): v for k, v in res["tokens"].items()}


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return run(tmp_path_factory.mktemp("rows_tools"), "base", scenario())


def test_two_runs_agree_and_equal_requests_answer_alike(base, tmp_path):
    assert run(tmp_path, "again", scenario()) == base
    assert base[0] == base[1]
    assert base[2] != base[3]                            # (a fixed outcome of the fixed seeds: the case below has teeth)


def test_swapping_two_seeds_swaps_two_answers(base, tmp_path):
    sc = scenario()
    sc["requests"][2]["seed"], sc["requests"][3]["seed"] = 202, 201
    got = run(tmp_path, "swapped", sc)
    assert got[2] == base[3] and got[3] == base[2]
    assert {k: v for k, v in got.items() if k not in (2, 3)} == {k: v for k, v in base.items() if k not in (2, 3)}


def test_greedy_requests_are_answered_greedily_among_sampling_ones(base, tmp_path):
    sc = copy.deepcopy(scenario())
    for r in sc["requests"]:
        r.update(GREEDY)
    greedy = run(tmp_path, "all_greedy", sc)
    for i in (4, 5, 6):
        assert base[i] == greedy[i], i
    assert any(base[i] != greedy[i] for i in (0, 2, 3, 7, 8, 9))       # and the sampling requests were sampled
