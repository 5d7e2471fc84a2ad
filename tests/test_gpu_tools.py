"""The C++ host stack on the GPU: tools/offline_inference (LLMGenerator -> LLMEngine -> src/backends/hip -> libpplhip)
against the oracle's greedy continuation of the same prompts, and the prefix-cache benchmark driver."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import ref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "ppl.llm.serving_amd")
CFG = os.path.join(PKG, "configs", "tiny_w8a16_kv8_paged.json")


def tool(name):
    path = os.path.join(PKG, "build", name)
    assert os.path.exists(path), f"{path} missing: run __graft_entry__.build()"
    return path


def oracle_greedy(desc, seed, prompt, n):
    """greedy continuation of one prompt; also returns the top-2 margin of every step"""
    m = ref.RefModel(desc)
    m.init_synthetic(seed)
    total = len(prompt) + n
    m.kv_alloc(((total + 3) // 4) * 4)
    pages = np.arange((total + 3) // 4, dtype=np.int64)[None, :]
    toks, margins = [], []
    tok, start = np.asarray(prompt, dtype=np.int64), 0
    for s in range(n):
        st = ref.make_step(tok, [0, len(tok)], [start], pages, 0 if s == 0 else 1, max_pages=pages.shape[1])
        logits = ref.forward([m], st)[0]
        srt = np.sort(logits)
        margins.append(float(srt[-1] - srt[-2]))
        nxt = int(logits.argmax())
        toks.append(nxt)
        start += len(tok)
        tok = np.array([nxt], dtype=np.int64)
    return toks, margins


@pytest.mark.parametrize("quant_method", ["none", "online_i8i8"])
def test_offline_inference_prompts4_matches_oracle(quant_method):
    """--quant-method is the reference's flag (tools/llm_server.cc:62, offline_inference.cc; resource_manager.cc:49-56: none | online_i8i8)"""
    out = subprocess.check_output([tool("offline_inference"), "--model-param-path", CFG, "--synthetic-weights", "--synthetic-seed", "77",
                                   "--kv-cache-max-tokens", "512", "--max-running-batch", "8", "--max-tokens-per-step", "64",
                                   "--workload", "prompts4", "--quant-method", quant_method], timeout=300).decode()
    prompts, answers = [], []
    for line in out.splitlines():
        if line.startswith("Prompt tokens:"):
            prompts.append([int(x) for x in line.split(":")[1].split()])
        if line.startswith("Answer tokens:"):
            answers.append([int(x) for x in line.split(":")[1].split()])
    assert len(prompts) == 4 and [len(a) for a in answers] == [8, 9, 10, 11]     # generation_length = 8 + i
    assert "generation time:" in out
    cfg = json.load(open(CFG))
    desc = ref.make_desc(hidden_dim=cfg["hidden_dim"], intermediate_dim=cfg["intermediate_dim"], num_layers=cfg["num_layers"],
                         num_heads=cfg["num_heads"], num_kv_heads=cfg["num_kv_heads"], vocab_size=cfg["vocab_size"],
                         max_position=cfg["max_position"], cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=1,
                         page_size=4, weight_quant_bit=8, act_quant_bit=8 if quant_method == "online_i8i8" else 0)
    compared = 0
    for p, a in zip(prompts, answers):
        want, margins = oracle_greedy(desc, 77, p, len(a))
        for i, (g, w) in enumerate(zip(a, want)):
            if margins[i] < (2e-2 if quant_method == "online_i8i8" else 8e-3):      # near-tie: either choice is legitimate, and the continuations diverge
                break
            assert g == w, (p, i, a, want)
            compared += 1
    assert compared >= 12


def test_offline_inference_samples_workload_and_prefix_benchmark():
    out = subprocess.check_output([tool("offline_inference"), "--model-param-path", CFG, "--synthetic-weights",
                                   "--kv-cache-max-tokens", "2048", "--max-running-batch", "16", "--max-tokens-per-step", "256",
                                   "--workload", "samples1024", "--num-requests", "48", "--max-seq-len", "128"], timeout=300).decode()
    res = json.loads(out.strip().splitlines()[-1])
    assert res["failed"] == 0 and res["requests"] == 48 and res["output_tokens"] > 48
    assert res["max_running"] <= 16 and res["ttft_ms"]["p50"] > 0 and res["tokens_out_per_s"] > 0
    out = subprocess.check_output([tool("benchmark_prefix_cache_offline"), "--model-param-path", CFG, "--synthetic-weights",
                                   "--kv-cache-max-tokens", "2048", "--max-running-batch", "4", "--max-tokens-per-step", "512",
                                   "--max-input-tokens-per-request", "512", "--enable-prefix-cache", "--prompt-len", "200",
                                   "--shared-len", "160", "--generation-length", "8"], timeout=300).decode()
    res = json.loads(out.strip().splitlines()[-1])
    assert res["first_ttft_ms"] > 0 and res["prefix_ttft_ms"] > 0
    assert "first ttft:" in out and "prefix ttft:" in out


def test_reference_engine_and_generator_drive_the_hip_backend_unmodified():
    """SURVEY.md 8(b) B1/B2 on the device: oracle/_ref/ref_backend_driver is the REFERENCE'S OWN llm_generator.cc + llm_engine.cc
    (compiled in place from the reference's src/ by `make -C oracle ref` in build(), no line changed) over
    src/backends/hip_nn -- ppl::nn::Runtime / Tensor / Engine objects on top of libpplhip.  Same synthetic model, same four
    prompts as offline_inference --workload prompts4 (the repo's generator + engine): the generated tokens must be identical,
    at tensor-parallel size 1 and 2 (both ranks on device 0)."""
    drv = os.path.join(ROOT, "oracle", "_ref", "ref_backend_driver")
    if not os.path.exists(drv):
        pytest.skip("oracle/_ref/ref_backend_driver is built by build() only where the reference tree exists (oracle/Makefile ref)")

    def answers(out):
        return [[int(x) for x in l.split(":")[1].split()] for l in out.splitlines() if l.startswith("Answer tokens:")]

    for tp in (1, 2):
        env = dict(os.environ, GPU_MAX_HW_QUEUES="24", PPLHIP_DEVICE_IDS=",".join(["0"] * tp))
        mine = subprocess.check_output([tool("offline_inference"), "--model-param-path", CFG, "--synthetic-weights", "--kv-cache-max-tokens",
                                        "8192", "--workload", "prompts4", "--tensor-parallel-size", str(tp)], timeout=300, env=env).decode()
        theirs = subprocess.check_output([drv, CFG, str(tp)], timeout=300, env=env).decode()
        a, b = answers(mine), answers(theirs)
        assert [len(x) for x in a] == [8, 9, 10, 11] and a == b, (tp, a, b)


def test_offline_inference_text_prompts_through_the_cpp_tokenizer():
    """--tokenizer-path: the reference's four TEXT prompts (tools/offline_inference.cc:304-309) are tokenised by src/tokenizer (BOS
    first, models/llama/llama_tokenizer.h:35-38), run through generator + engine + libpplhip, and every generated token is
    detokenised and streamed back; prompt ids must equal the sentencepiece module's (tests/golden/spm_cases.json)."""
    spm = os.path.join(ROOT, "tests", "golden", "spm_bpe.model")
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "spm_cases.json")))["spm_bpe.model"]
    out = subprocess.check_output([tool("offline_inference"), "--model-param-path", CFG, "--synthetic-weights", "--kv-cache-max-tokens", "2048",
                                   "--workload", "prompts4", "--tokenizer-path", spm], timeout=300).decode()
    prompts = [l[len("Prompt: "):] for l in out.splitlines() if l.startswith("Prompt: ")]
    answers = [l[len("Answer: "):] for l in out.splitlines() if l.startswith("Answer: ")]
    ptoks = [[int(x) for x in l.split(":")[1].split()] for l in out.splitlines() if l.startswith("Prompt tokens:")]
    atoks = [[int(x) for x in l.split(":")[1].split()] for l in out.splitlines() if l.startswith("Answer tokens:")]
    assert prompts[:2] == ["Hello, my name is", "The president of the United States is"] and len(answers) == 4
    by_text = {t["text"]: t["ids"] for t in cases["texts"]}
    assert ptoks[0] == [cases["bos"]] + by_text["Hello, my name is"] and ptoks[1] == [cases["bos"]] + by_text["The president of the United States is"]
    assert [len(a) for a in atoks] == [8, 9, 10, 11]


def _random_scenario(rng, vocab, prefix, penalty, stochastic=False):
    shared = rng.randint(3, vocab, size=int(rng.randint(8, 30))).tolist()
    reqs = []
    for i in range(int(rng.randint(6, 20))):
        toks = rng.randint(3, vocab, size=int(rng.randint(1, 24))).tolist()
        if rng.rand() < 0.6:
            toks = shared[:int(rng.randint(1, len(shared) + 1))] + toks
        # greedy: both tools start their generator thread before the requests arrive, so WHICH requests share a step is a race,
        # and a stochastic sampler draws per (step, row) from one rand() sequence -- only greedy answers are a function of the
        # request alone.  (The per-request temperature still reaches the kernel and must not change an argmax.)
        r = {"id": i, "tokens": toks, "generation_length": int(rng.randint(1, 14)),
             "temperature": float(rng.choice([1.0, 0.7, 1.3])), "top_k": 1, "top_p": float(rng.choice([0.0, 0.9])),
             "early_stopping": bool(rng.rand() < 0.8)}
        if penalty:
            r.update(repetition_penalty=float(rng.choice([1.0, 1.2])), presence_penalty=float(rng.choice([0.0, 0.5])),
                     frequency_penalty=float(rng.choice([0.0, 0.3])))
        if rng.rand() < 0.3:
            r["stop_tokens"] = rng.randint(3, vocab, size=40).tolist()
        reqs.append(r)
    gen = {"max_running_batch": int(rng.randint(2, 9)), "max_tokens_per_step": int(rng.choice([64, 128, 512])),
           "max_prefill_batch": int(rng.randint(1, 5)), "max_cooldown_request": int(rng.randint(1, 4)),
           "enable_prefix_cache": prefix, "enable_penalty": penalty, "stop_tokens": rng.randint(3, vocab, size=6).tolist()}
    if stochastic:
        # one request at a time: the step composition is then fixed (FIFO), and so is the position of every draw in the sampler's
        # unseeded rand() sequence (post_processor.cc:179-183) -- per-request temperature / top-p and top_k_list[0] (Q3) must agree
        gen["max_running_batch"] = 1
        for r in reqs:
            r["top_k"] = int(rng.choice([1, 8, 40]))
    return {"generator": gen, "kv_cache_max_tokens": int(rng.choice([256, 1024])), "requests": reqs}


@pytest.mark.parametrize("seed,prefix,penalty,stochastic", [(0, False, False, False), (1, True, False, False), (2, False, True, False),
                                                            (3, True, True, False), (4, False, False, False), (5, True, True, False),
                                                            (6, False, False, True), (7, False, True, True), (8, True, False, True)])
def test_reference_stack_and_this_tree_agree_on_random_scenarios(tmp_path, seed, prefix, penalty, stochastic):
    """the reference's generator + engine (compiled in place) over hip_nn::Backend against this tree's generator + engine over
    src/backends/hip, same libpplhip: random prompts with shared prefixes, KV pressure, global and per-request stop tokens,
    early stopping on and off, per-request temperature, penalties, prefix cache -- every token of every request must be identical,
    and so must the set of rejected requests"""
    drv = os.path.join(ROOT, "oracle", "_ref", "ref_backend_driver")
    if not os.path.exists(drv):
        pytest.skip("oracle/_ref/ref_backend_driver is built by build() only where the reference tree exists (oracle/Makefile ref)")
    cfg = json.load(open(CFG))
    sc = _random_scenario(np.random.RandomState(seed), cfg["vocab_size"], prefix, penalty, stochastic)
    path = str(tmp_path / "scenario.json")
    json.dump(sc, open(path, "w"))
    tp = 2 if seed in (3, 7) else 1          # two of the cases tensor-parallel (both ranks on device 0, direct collectives)
    env = dict(os.environ, GPU_MAX_HW_QUEUES="24", PPLHIP_DEVICE_IDS=",".join(["0"] * tp))
    mine = subprocess.check_output([tool("offline_inference"), "--model-param-path", CFG, "--synthetic-weights", "--workload", "scenario",
                                    "--scenario-file", path, "--tensor-parallel-size", str(tp)], timeout=300, stderr=subprocess.DEVNULL,
                                   env=env).decode()
    theirs = subprocess.check_output([drv, CFG, str(tp), path], timeout=300, stderr=subprocess.DEVNULL, env=env).decode()
    a, b = json.loads(mine.strip().splitlines()[-1]), json.loads(theirs.strip().splitlines()[-1])
    assert sorted(a["failed"]) == sorted(b["failed"])
    assert a["tokens"] == b["tokens"]
    assert len(a["tokens"]) + len(a["failed"]) == len(sc["requests"]) and len(a["tokens"]) >= 1


def test_prefix_cache_benchmark_config5_shape_7b(tmp_path):
    """BASELINE config 5 at its own shape: LLaMA-2-7B W8A16, int8-g8 paged KV (page 16),
    prefix cache on, --max-prefill-batch 1, 8192-token prompts sharing their first 6144 tokens, the same prompt list submitted
    twice (reference tools/benchmark_prefix_cache_offline.cc:442-508).  Three prompts keep it to a few seconds.
      * the cached run answers what the cold run answered: greedy tokens equal up to the first near-tie (the cached run recomputes
        only the last page through the cache-prefill path -- a different summation order, tests/test_gpu_fulldepth.py);
      * the cache works: `prefix ttft` (first Send of run 2) is a small fraction of `first ttft`, and inside run 1 the second and
        third prompts (partial hits of 6144 tokens) start faster than the cold first one would."""
    dump = tmp_path / "answers.txt"
    cfg = os.path.join(PKG, "configs", "llama2_7b_w8a16_kv8_paged.json")
    out = subprocess.check_output([tool("benchmark_prefix_cache_offline"), "--model-param-path", cfg, "--synthetic-weights",
                                   "--enable-prefix-cache", "--max-prefill-batch", "1", "--max-input-tokens-per-request", "8192",
                                   "--max-total-tokens-per-request", "16384", "--kv-cache-max-tokens", "65536", "--batch", "3",
                                   "--generation-length", "6", "--dump-answers", str(dump)], timeout=600).decode()
    res = json.loads(out.strip().splitlines()[-1])
    assert res["prompt_len"] == 8192 and res["shared_len"] == 6144 and res["batch"] == 3 and res["second_run"] == "same"
    assert res["prefix_ttft_ms"] < 0.35 * res["first_ttft_ms"], res        # observed (r03): 19 ms against 165 ms
    assert res["prefix_generate_ms"] < res["first_generate_ms"], res
    lines = [[int(x) for x in l.split()] for l in open(dump).read().splitlines()]
    assert len(lines) == 6 and all(len(l) == 6 for l in lines)
    cold, cached = lines[:3], lines[3:]
    agree = [next((i for i in range(6) if a[i] != b[i]), 6) for a, b in zip(cold, cached)]   # tokens in common before the first difference
    assert sum(agree) >= 9 and min(agree) >= 1, (agree, cold, cached)


def test_prefix_cache_benchmark_answers_identical_with_a_decisive_head(tmp_path):
    """the same harness with a DECISIVE synthetic model (--synthetic-decisive-head 7: lm_head row v = embedding row v - 7, so every token t
    is answered by t + 7 with a top-2 margin of a third of the logit scale; pplhip_rank_tie_output): the cached run -- prefix-cache hits,
    cache-prefill of the last page, its own decode steps -- must answer EVERY request exactly like the cold run (VERDICT r4 item 5:
    `identical_answers` == batch; with the plain synthetic head 51 of 64 did, the rest being near-ties).  What this pins is the hit path's
    bookkeeping (pages, start positions, token hand-over); its arithmetic is pinned in tests/test_gpu_config5_tokens.py and
    tests/test_gpu_config34_shape.py."""
    dump = tmp_path / "answers.txt"
    cfg = os.path.join(PKG, "configs", "llama2_7b_w8a16_kv8_paged.json")
    out = subprocess.check_output([tool("benchmark_prefix_cache_offline"), "--model-param-path", cfg, "--synthetic-weights",
                                   "--synthetic-decisive-head", "7", "--enable-prefix-cache", "--max-prefill-batch", "1",
                                   "--max-input-tokens-per-request", "8192", "--max-total-tokens-per-request", "16384",
                                   "--kv-cache-max-tokens", "98304", "--batch", "8", "--generation-length", "12", "--dump-answers", str(dump)],
                                  timeout=900).decode()
    res = json.loads(out.strip().splitlines()[-1])
    assert res["batch"] == 8 and res["identical_answers"] == 8, res
    lines = [[int(x) for x in l.split()] for l in open(dump).read().splitlines()]
    assert len(lines) == 16 and lines[:8] == lines[8:]
    # the model is the decisive one: every answer continues its prompt's last token in steps of 7 (mod vocab)
    for l in lines[:8]:
        assert all((b - a) % 32000 == 7 for a, b in zip(l, l[1:])), l
