"""Every per-request feature at once through the whole host stack on the GPU: ONE scenario through tools/offline_inference with every key
of tools/scenario.h in use -- seeds, top-N logprobs, prompt logprobs, allow and ban lists, a bias, min_new_tokens, two guides, adapters, the
penalty step and the prefix cache -- on ten requests of at most eight tokens through four batch rows, and the same scenario with one batch
row, where every request runs alone.

What a request asks for decides what it gets, whatever shares its batch: the failed lists are equal, the greedy requests answer token for
token alike in both runs (--synthetic-decisive-head keeps their margins wide), guided answers match their patterns, allow list, ban list
and min_new_tokens hold, every asking request has one top-N list of its own length per generated token and exactly len(prompt) - 1 prompt
positions, and a second run of the same scenario prints the same line.  No logprob VALUE is compared between the two batch sizes: the
GEMM route depends on a step's row count, so they differ in their low bits by design."""
import json
import os
import re
import subprocess

import pytest

from oracle import ref
from tests import guide as G
from tests import lora_model as LM
from tests.conftest import ROOT, load_pplhip
from tests.test_gpu_tools import CFG, PKG

pytestmark = pytest.mark.gpu
SPM = os.path.join(ROOT, "tests", "golden", "spm_bpe.model")
VOCAB = 1024
SHARED = [301, 302, 303, 304, 305, 306, 307, 308]        # two full pages that requests 0, 4 and 9 share: the prefix cache has something to hit
ALLOWED = [17, 300, 301, 640, 1023]
BANNED = list(range(0, 1024, 3))
STOP = 777
GEN_STOP = 1000                                          # the generator's own stop token
LORA_MAP = [-1, 0, 1, -1, 0, -1, 1, 0, -1, -1]
GREEDY = (0, 1, 3, 4, 7, 8, 9)


def scenario(max_running_batch):
    g = dict(top_k=1, top_p=0.0)
    s = dict(top_k=0, top_p=1.0, temperature=200.0)      # a flat distribution: the temperature takes the decisive head's margins away
    reqs = [
        dict(id=0, tokens=SHARED + [11, 12], generation_length=8, early_stopping=False, temperature=0.7, repetition_penalty=1.2, **g),
        dict(id=1, tokens=[21, 22, 23], generation_length=6, early_stopping=False, allowed_tokens=ALLOWED, num_logprobs=3, **g),
        dict(id=2, tokens=[31, 32, 33, 34, 35], generation_length=8, early_stopping=False, seed=11, banned_tokens=BANNED, prompt_logprobs=2,
             presence_penalty=0.5, **s),
        dict(id=3, tokens=[41, 42], generation_length=8, early_stopping=True, guide_regex="(yes|no|maybe)", num_logprobs=2, **g),
        dict(id=4, tokens=SHARED + [51], generation_length=8, early_stopping=True, min_new_tokens=3, stop_tokens=[STOP],
             logit_bias=[[STOP, 10000.0]], **g),
        dict(id=5, tokens=[61, 62, 63], generation_length=4, early_stopping=False, logit_bias=[[VOCAB, 1.0]], num_logprobs=4, prompt_logprobs=1,
             **g),                                       # outside the vocabulary: this request fails, alone
        dict(id=6, tokens=[71, 72, 73, 74, 75, 76], generation_length=5, early_stopping=False, seed=12, top_k=50, top_p=0.9, temperature=150.0,
             num_logprobs=20, prompt_logprobs=0, frequency_penalty=0.25),
        dict(id=7, tokens=[81, 82, 83, 84], generation_length=8, early_stopping=True, guide_regex="[0-9]{3}", logit_bias=[[5, 0.5]],
             prompt_logprobs=1, **g),
        dict(id=8, tokens=[91, 92, 93], generation_length=7, early_stopping=False, banned_tokens=BANNED, logit_bias=[[7, "-inf"]],
             repetition_penalty=0.9, **g),
        dict(id=9, tokens=SHARED + [11, 12, 13], generation_length=7, early_stopping=False, num_logprobs=1, **g),
    ]
    return {"generator": {"max_running_batch": max_running_batch, "max_tokens_per_step": 64, "max_prefill_batch": 2, "max_cooldown_request": 2,
                          "enable_prefix_cache": True, "enable_penalty": True, "stop_tokens": [GEN_STOP]},
            "kv_cache_max_tokens": 1024, "requests": reqs}


@pytest.fixture(scope="module")
def adapters(tmp_path_factory):
    m = load_pplhip()
    cfg = json.load(open(CFG))
    keys = ("num_heads", "num_kv_heads", "num_layers", "hidden_dim", "intermediate_dim", "vocab_size", "cache_quant_bit", "cache_quant_group",
            "cache_layout", "cache_mode", "page_size", "weight_quant_bit", "max_position")
    desc = ref.make_desc(**{k: cfg[k] for k in keys})
    root = tmp_path_factory.mktemp("chain_adapters")
    dirs = []
    for a in (0, 1):
        tensors, scale = LM.make_adapter(desc, a)
        os.makedirs(root / f"adapter{a}")
        m.write_lora_container(str(root / f"adapter{a}" / "lora.pplhip"), tensors, scale)
        dirs.append(str(root / f"adapter{a}"))
    return dirs


def _offline(path, adapters):
    tool = os.path.join(PKG, "build", "offline_inference")
    assert os.path.exists(tool), f"{tool} missing: run __graft_entry__.build()"
    out = subprocess.check_output([tool, "--model-param-path", CFG, "--synthetic-weights", "--synthetic-decisive-head", "7", "--workload", "scenario",
                                   "--scenario-file", path, "--per-request-sampling", "--sampling-seed", "5", "--tokenizer-path", SPM,
                                   "--lora-dirs", ",".join(adapters), "--lora-map", ",".join(map(str, LORA_MAP))],
                                  timeout=300, stderr=subprocess.DEVNULL).decode()
    line = out.strip().splitlines()[-1]
    return line, json.loads(line)


def _properties(sc, res):
    """what must hold in any run of the scenario"""
    pieces, n_pieces, eos = G.spm_vocab()
    reqs = {r["id"]: r for r in sc["requests"]}
    assert res["failed"] == [5] and sorted(res["tokens"]) == [str(i) for i in range(10) if i != 5]
    tok = {int(k): v for k, v in res["tokens"].items()}
    for i, t in tok.items():
        assert 1 <= len(t) <= reqs[i]["generation_length"] and all(0 <= x < VOCAB for x in t), (i, t)
    for i in (0, 1, 2, 6, 8, 9):                         # nothing ends these before their length
        assert len(tok[i]) == reqs[i]["generation_length"], (i, tok[i])
    # guided outputs match their pattern, in full, and end on the end token
    for i in (3, 7):
        pattern = reqs[i]["guide_regex"]
        trans, accept = G.compile_regex(pattern)
        assert tok[i][-1] in (eos, GEN_STOP), (i, tok[i])  # an end token: allowed only where the pattern is matched in full
        text = b"".join(pieces[t] for t in tok[i][:-1])
        assert re.fullmatch(pattern.encode(), text), (pattern, text)
        assert accept[G.walk(trans, 0, text)] == 1       # (the project's own automaton says so too)
    # allow list, ban lists, min_new_tokens
    assert set(tok[1]) <= set(ALLOWED)
    assert not set(tok[2]) & set(BANNED) and not set(tok[8]) & (set(BANNED) | {7})
    assert tok[4][3] == STOP and STOP not in tok[4][:3] and len(tok[4]) == 4      # the stop's bias wins as soon as it may, and ends the request
    # one top-N list of the request's own length per generated token; greedy: its first entry is the answer
    asking = {i: min(r["num_logprobs"], 20) for i, r in reqs.items() if r.get("num_logprobs") and i != 5}
    assert sorted(res["top_tokens"]) == sorted(res["top_logprobs"]) == sorted(str(i) for i in asking)
    for i, n in asking.items():
        tt, tl = res["top_tokens"][str(i)], res["top_logprobs"][str(i)]
        assert len(tt) == len(tl) == len(tok[i]), (i, len(tt), len(tok[i]))
        for s in range(len(tt)):
            assert len(tt[s]) == len(tl[s]) == n and len(set(tt[s])) == n, (i, s, tt[s])
            assert all(a >= b for a, b in zip(tl[s], tl[s][1:])), (i, s, tl[s])
            if reqs[i]["top_k"] == 1:
                assert tt[s][0] == tok[i][s], (i, s)
    assert set(res["top_tokens"]["1"][0]) <= set(ALLOWED)                         # top-N saw the edited row: its three best are allowed ones
    # exactly len(prompt) - 1 prompt positions, with the request's own number of alternatives
    pasking = {i: r["prompt_logprobs"] for i, r in reqs.items() if r.get("prompt_logprobs", -1) >= 0 and i != 5}
    for key in ("prompt_logprobs", "prompt_ranks", "prompt_top_tokens", "prompt_top_logprobs"):
        assert sorted(res[key]) == sorted(str(i) for i in pasking), key
    for i, n in pasking.items():
        P = len(reqs[i]["tokens"]) - 1
        assert len(res["prompt_logprobs"][str(i)]) == len(res["prompt_ranks"][str(i)]) == P, i
        assert all(lp <= 0 for lp in res["prompt_logprobs"][str(i)]) and all(0 <= r < VOCAB for r in res["prompt_ranks"][str(i)])
        assert [len(x) for x in res["prompt_top_tokens"][str(i)]] == [n] * P and [len(x) for x in res["prompt_top_logprobs"][str(i)]] == [n] * P
    return tok


def test_one_scenario_with_everything_in_it(tmp_path, adapters):
    sc4, sc1 = scenario(4), scenario(1)
    p4, p1 = str(tmp_path / "batch4.json"), str(tmp_path / "batch1.json")
    json.dump(sc4, open(p4, "w"))
    json.dump(sc1, open(p1, "w"))
    line4, res4 = _offline(p4, adapters)
    tok4 = _properties(sc4, res4)
    line1, res1 = _offline(p1, adapters)
    tok1 = _properties(sc1, res1)
    assert res4["failed"] == res1["failed"]
    for i in GREEDY:                                     # a greedy request answers alike whatever shares its batch
        assert sc4["requests"][i]["top_k"] == 1
        assert tok4[i] == tok1[i], (i, tok4[i], tok1[i])
    print("sampled:", {i: (tok4[i], tok1[i]) for i in (2, 6)})
    again, _ = _offline(p4, adapters)
    assert again == line4                                # the same scenario, the same line
