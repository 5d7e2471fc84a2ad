"""Mixture-of-experts models through the context (pplhip_moe): identical experts against the dense oracle -- the routing weights sum to 1,
so every step must meet the oracle as the dense model does --, distinct fp16 experts against transformers' MixtralForCausalLM
(tests/golden/hf_tiny_mixtral.npz, written by tools/make_mixtral_golden.py), and the refusals."""
import importlib.util
import json
import os

import numpy as np
import pytest

from oracle import ref
from tests.conftest import load_pplhip
from tests.test_gpu_model import check_steps
from tests.parity import oracle_noise

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GEOMETRY = dict(hidden_dim=256, intermediate_dim=512, num_layers=2, num_heads=4, num_kv_heads=4, vocab_size=1024, max_position=512,
                cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=1, page_size=16, weight_quant_bit=8, weight_quant_group=128)


@pytest.mark.parametrize("E,k", [(1, 1), (8, 2)])
def test_identical_experts_match_dense_oracle(E, k):
    """every expert of layer l holds the oracle's w13 / w2 of layer l, the gate is random: a prefill step, a mixed step and three decode
    steps at test_synthetic_model's cap (layer indexing, chunk offsets, gather and scatter through the whole step)"""
    m = load_pplhip()
    desc = ref.make_desc(**GEOMETRY)
    rm = ref.RefModel(desc)
    rm.init_synthetic(99)
    rm.kv_alloc(256)
    ctx = m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=128)
    ctx.moe(E, k)
    ctx.init_synthetic(0, 99)
    ctx.kv_alloc(0, 256)
    rng = np.random.RandomState(E)
    for l in range(desc.num_layers):
        ctx.set_tensor(0, f"layers.{l}.feed_forward.gate.weight", (rng.randn(E, desc.hidden_dim) * 0.1).astype(np.float16))
        for lin in ("w13", "w2"):
            w, s = rm.get_tensor(f"layers.{l}.feed_forward.{lin}.weight", np.int8), rm.get_tensor(f"layers.{l}.feed_forward.{lin}.scale", np.float16)
            for j in range(E):
                ctx.set_tensor(0, f"layers.{l}.feed_forward.experts.{j}.{lin}.weight", w)
                ctx.set_tensor(0, f"layers.{l}.feed_forward.experts.{j}.{lin}.scale", s)
    pages = np.arange(12, dtype=np.int64).reshape(3, 4)   # request i owns pages 4 i .. 4 i + 3
    res = []

    def step(tok, lens, start_pos, rows, dec):
        seq_starts = np.concatenate([[0], np.cumsum(lens)])
        st_r = ref.make_step(tok, seq_starts, start_pos, pages[rows], dec, 4)
        want, alt = ref.forward([rm], st_r), oracle_noise([rm], st_r)
        ctx.set_inputs(0, m.make_step(tok, seq_starts, start_pos, pages[rows], dec, 4, req_list_changed=1))
        ctx.run(0)
        gtok, glp = ctx.sample(len(rows), top_k=1)
        wtok, wlp = ref.sample(want, top_k=1)
        res.append((ctx.copy_logits(len(rows)), want, gtok, wtok, glp, wlp, alt))
        return wtok.astype(np.int64)

    nxt = step(rng.randint(3, 1024, size=42), [37, 5], [0, 0], [0, 1], 0)
    nxt = step(np.concatenate([nxt, rng.randint(3, 1024, size=20)]), [1, 1, 20], [37, 5, 0], [0, 1, 2], 2)
    for s in range(3):
        nxt = step(nxt, [1, 1, 1], np.array([38, 6, 20]) + s, [0, 1, 2], 3)
    check_steps(res, k=1, name=f"moe_identical_experts_{E}_{k}")
    ctx.close()
    rm.close()


def test_distinct_experts_match_hf_mixtral(golden_dir):
    """fp16 weights, fp16 KV: gate and expert tensors uploaded by name, a prefill and four greedy decode steps against the HF model's fp32
    logits at test_hf_fixture_model's cap for HF vectors.  The fixture's routing gaps are safe in every layer (asserted by its script), and
    its layer-0 choice uses every expert: a gate stored wrongly or an expert mistaken for another moves the logits far beyond the cap."""
    m = load_pplhip()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_mixtral_golden", os.path.join(root, "ppl.llm.serving_amd", "tools", "make_mixtral_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    fx = np.load(os.path.join(golden_dir, "hf_tiny_mixtral.npz"))
    cfg = json.loads(str(fx["config"]))
    E, k = cfg.pop("num_experts"), cfg.pop("experts_per_token")
    assert len(np.unique(fx["layer0_experts"])) == E and fx["layer0_experts"].shape == (len(fx["tokens"]), k)
    ctx = m.Context(m.make_desc(**cfg), max_running_batch=4, max_tokens_per_step=64)
    ctx.moe(E, k)
    for name, arr in gen.draw_weights(dict(cfg, num_experts=E, experts_per_token=k), int(fx["seed"])).items():
        ctx.set_tensor(0, name, arr)
    ctx.kv_alloc(0, 64)
    tokens, want = fx["tokens"], fx["logits"]
    n0 = len(tokens) - (len(want) - 1)   # the prompt; then one fixture token per decode step
    cap = 2e-2 * max(1.0, float(np.abs(want).max()))
    for s in range(len(want)):
        tok, pos = (tokens[:n0], 0) if s == 0 else (tokens[n0 + s - 1:n0 + s], n0 + s - 1)
        ctx.set_inputs(0, m.make_step(tok, [0, len(tok)], [pos], np.zeros(1, dtype=np.int64), int(s > 0), req_list_changed=int(s == 0)))
        ctx.run(0)
        got = ctx.copy_logits(1)[0]
        err = float(np.abs(got - want[s]).max())
        print(f"hf_tiny_mixtral step {s}: max |logit error| {err:.3e}, cap {cap:.3e}")
        assert err < cap, (s, err, cap)
        assert got.argmax() == want[s].argmax() or np.sort(want[s])[-1] - np.sort(want[s])[-2] < 2 * cap
    ctx.close()


@pytest.mark.parametrize("case", ["experts", "top_k", "top_k_over_experts", "w4a16", "online_i8i8", "online_f8f8", "world_size", "lora_w2", "dense"])
def test_refusals_and_untouched_dense_path(case):
    m = load_pplhip()
    kw = dict(GEOMETRY)
    if case == "w4a16":
        kw["weight_quant_bit"] = 4
    if case in ("online_i8i8", "online_f8f8"):
        kw["act_quant_bit"] = m.ACT_QUANT_I8 if case == "online_i8i8" else m.ACT_QUANT_FP8
    two = dict(n_local_ranks=2, world_size=2, device_ids=[0, 0]) if case == "world_size" else {}
    make = lambda: m.Context(m.make_desc(**kw), max_running_batch=8, max_tokens_per_step=4096, **two)
    ctx = make()
    if case == "dense":
        # what is shown: the routing buffers are allocated BY pplhip_moe, not by pplhip_init -- with one expert the stacked weights are the
        # dense ones' size, so the call takes the workspace (and the gate) and nothing else.  And it comes too late behind a weight
        free_dense = ctx.mem_info(0)[0]
        ctx.moe(1, 1)
        ws = m.lib().pplhip_op_moe_ffn_workspace_bytes(4096, 1, 1, kw["hidden_dim"], kw["intermediate_dim"])
        assert free_dense - ctx.mem_info(0)[0] >= 0.9 * ws
        ctx.close()
        ctx = make()
        ctx.init_synthetic(0, 1)
        with pytest.raises(m.PplHipError, match="INVALID_VALUE.*before any weight"):
            ctx.moe(1, 1)
    elif case == "lora_w2":
        ctx.moe(8, 2)
        with pytest.raises(m.PplHipError, match="UNSUPPORTED.*feed_forward.w2"):
            ctx.lora_set_tensor(0, 0, "layers.0.feed_forward.w2.lora_a", np.zeros((8, 512), dtype=np.float16))
        ctx.lora_set_tensor(0, 0, "layers.0.attention.wo.lora_a", np.zeros((8, 256), dtype=np.float16))   # the other targets stay
    else:
        E, k = {"experts": (65, 2), "top_k": (16, 9), "top_k_over_experts": (4, 5)}.get(case, (8, 2))
        with pytest.raises(m.PplHipError, match="UNSUPPORTED: pplhip_moe: "):
            ctx.moe(E, k)
        assert not m.lib().pplhip_last_error(ctx.h, -1).decode().endswith(": ")   # a reason is given
    ctx.close()
