"""Tensor parallelism of the HIP path itself (pplhip.cc's step schedule + the direct collectives of csrc/k_comm.hip) against
the oracle sharded the same way -- on ONE GPU: all ranks of the group are created on device 0, each with its own stream,
weights slice, KV slab and exchange region, so the collectives' flag protocol, the chunked overlap schedule and the
per-rank kernels run exactly as on an 8-GPU node except that a "peer" pointer is local.  (What a single GPU cannot show
is xGMI visibility; the runtime's start-up self-test checks that on the real node and falls back to RCCL otherwise.)

Also the BASELINE per-rank geometries the round-1 suite never touched:
  config 3  LLaMA-2-13B W8A16, TP 2: hidden 5120, 20 heads / rank, inter 6912 / rank
  config 4  LLaMA-2-70B W4A16-g128, TP 8: hidden 8192, 8 query heads + 1 KV head / rank, inter 3584 / rank, kv 2048
(2 layers each: the oracle is a plain CPU program)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import ref
from tests.conftest import load_pplhip
from tests.parity import oracle_noise, record_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

I64MAX = np.iinfo(np.int64).max


def f16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


def load_exporter():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ppl.llm.serving_amd", "tools", "export_hf_llama.py")
    spec = importlib.util.spec_from_file_location("export_hf_llama_for_tests", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Group:
    """tp ranks of the HIP path on device 0 + the oracle's tp slices."""

    def __init__(self, m, desc, tp, max_batch, max_tokens, kv_tokens):
        self.m, self.desc, self.tp, self.kv_tokens = m, desc, tp, kv_tokens
        self.ctx = m.Context(m.copy_desc(desc), max_running_batch=max_batch, max_tokens_per_step=max_tokens, n_local_ranks=tp,
                             device_ids=[0] * tp)
        assert self.ctx.comm_mode() == m.COMM_P2P
        self.models = [ref.RefModel(desc, tp, r) for r in range(tp)]
        for r in range(tp):
            self.models[r].kv_alloc(kv_tokens)
            self.ctx.kv_alloc(r, kv_tokens)

    def synthetic(self, seed):
        for r in range(self.tp):
            self.models[r].init_synthetic(seed)
            self.ctx.init_synthetic(r, seed)

    def set_tensors(self, rank, tensors):
        for k, v in tensors.items():
            self.models[rank].set_tensor(k, v)
            self.ctx.set_tensor(rank, k, v)

    def kv_history(self, seed):
        """the same pseudo-random int8 history (+ scales) in every rank's slab on both sides"""
        for r in range(self.tp):
            rng = np.random.RandomState(seed + r)
            kc, ks = self.models[r].kv_array(0), self.models[r].kv_array(1)
            kc[:] = rng.randint(-127, 128, size=kc.size).astype(np.int8)
            ks[:] = f16(0.01 + 0.02 * rng.rand(ks.size))
            self.ctx.kv_write(r, 0, kc)
            self.ctx.kv_write(r, 1, ks)

    def step(self, tok, seq_starts, start_pos, cache_idx, dec, max_pages, changed):
        st_r = ref.make_step(tok, seq_starts, start_pos, cache_idx, dec, max_pages)
        want = ref.forward(self.models, st_r)
        self.last_alt = oracle_noise(self.models, st_r)
        st = self.m.make_step(tok, seq_starts, start_pos, cache_idx, dec, max_pages, req_list_changed=changed)
        for r in range(self.tp):      # one host thread enqueues every rank's step; the streams run side by side
            self.ctx.set_inputs(r, st)
            self.ctx.run(r)
        n = len(start_pos)
        gtok, _ = self.ctx.sample(n, top_k=1)
        got = self.ctx.copy_logits(n)
        for r in range(1, self.tp):
            self.ctx.sync(r)
        return got, want, gtok

    def close(self):
        self.ctx.close()
        for mm in self.models:
            mm.close()


def plan(desc, lens_total, kv_tokens, seed=0):
    n = len(lens_total)
    lens_total = np.asarray(lens_total)
    if desc.cache_mode == 0:
        return np.concatenate([[0], np.cumsum(lens_total)[:-1]]).astype(np.int64), 0
    P = desc.page_size
    npg = (lens_total + P - 1) // P
    mp = int(npg.max())
    idx = np.full((n, mp), I64MAX, dtype=np.int64)
    order = np.random.RandomState(seed).permutation(kv_tokens // P)
    k = 0
    for i in range(n):
        idx[i, :npg[i]] = order[k:k + npg[i]]
        k += npg[i]
    return idx, mp


def generate(g, prompts, steps, start=None):
    """packed prefill (or cache-prefill from `start`), then decode steps driven by the ORACLE's greedy tokens"""
    n = len(prompts)
    lens = np.array([len(p) for p in prompts])
    start_pos = np.zeros(n, dtype=np.int64) if start is None else np.asarray(start, dtype=np.int64)
    cache_idx, mp = plan(g.desc, start_pos + lens + steps, g.kv_tokens)
    tok = np.concatenate(prompts).astype(np.int64)
    seq = np.concatenate([[0], np.cumsum(lens)])
    out = []
    for s in range(steps):
        got, want, gtok = g.step(tok, seq, start_pos, cache_idx, 0 if s == 0 else n, mp, 1 if s == 0 else 0)
        out.append((got, want, gtok, g.last_alt))
        start_pos = start_pos + (seq[1:] - seq[:-1])
        tok = want.argmax(-1).astype(np.int64)
        seq = np.arange(n + 1)
    return out


def check(name, res, k):
    worst, noise = 0.0, 0.0
    for s, (got, want, gtok, alt) in enumerate(res):
        scale = max(1.0, float(np.abs(want).max()))
        err = float(np.abs(got - want).max()) / scale
        worst = max(worst, err)
        noise = max(noise, float(np.abs(alt - want).max()) / scale)
        assert err <= 1e-3 * k, (name, s, err)
        n_s = float(np.abs(alt - want).max()) / scale
        # ... and within 2.5 x the oracle's own summation-order noise (online_i8i8 models: the integer GEMMs have none, n_s ~ 1e-7)
        assert n_s < 1e-5 or err <= max(1e-3, 2.5 * n_s), (name, s, err, n_s)
        srt = np.sort(want, -1)
        safe = (srt[:, -1] - srt[:, -2]) > 2e-3 * k * scale
        assert (gtok[safe] == want.argmax(-1)[safe]).all(), (name, s)
    record_err(name, worst, 1e-3 * k, noise=noise)


@pytest.mark.parametrize("tp", [2, 4, 8])
@pytest.mark.parametrize("mode,overlap", [(1, False), (0, True), (0, False), (1, True)])
def test_tensor_parallel_group_on_one_device(monkeypatch, tp, mode, overlap):
    """tiny model, every tp: prefill + decode through all-reduce after wo / w2 and the logits all-gather, with the
    collectives on the compute stream and with the two-chunk schedule that puts them on the communication stream."""
    m = load_pplhip()
    monkeypatch.setenv("PPLHIP_TP_OVERLAP", "1" if overlap else "0")
    monkeypatch.setenv("PPLHIP_TP_OVERLAP_MIN_TOKENS", "2")
    desc = ref.make_desc(hidden_dim=512, intermediate_dim=1024, num_layers=3, num_heads=8, num_kv_heads=8, vocab_size=2048,
                         max_position=512, cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=mode,
                         page_size=16 if mode else 0, weight_quant_bit=8)
    g = Group(m, desc, tp, max_batch=16, max_tokens=512, kv_tokens=2048)
    g.synthetic(31 + tp)
    rng = np.random.RandomState(tp)
    prompts = [rng.randint(3, 2048, size=n) for n in (40, 3, 129, 1, 16, 77)]
    check(f"tp{tp}_tiny_mode{mode}_ov{int(overlap)}", generate(g, prompts, 4), k=1.5)   # observed (r02) <= 0.98e-3, int8 KV
    # what the context reports for the decode steps it just ran (one plan behind the step and the report)
    assert g.ctx.comm_info(len(prompts))["schedule"] == m.COMM_SCHEDULES[m.SCHED_TWO_CHUNKS if overlap else m.SCHED_ONE_LANE]
    g.close()


@pytest.mark.parametrize("tp,mode", [(2, 0), (2, 1), (4, 0)])
def test_tensor_parallel_two_stream_decode(monkeypatch, tp, mode):
    """PPLHIP_DUAL_STREAM=1 under tensor parallelism: the decode steps run as two half-batches on two streams, each half issuing its
    all-reduces on its own stream and its own CHANNEL of the direct collectives (flag set, scratch pair, epoch counter: k_comm.hip) -- the
    all-reduce of one half runs beside the other half's matmuls.  Contiguous and paged cache; against the oracle's tp slices."""
    m = load_pplhip()
    monkeypatch.setenv("PPLHIP_DUAL_STREAM", "1")
    monkeypatch.setenv("PPLHIP_DUAL_MIN_ROWS", "2")
    monkeypatch.setenv("PPLHIP_TP_OVERLAP", "0")
    desc = ref.make_desc(hidden_dim=512, intermediate_dim=1024, num_layers=3, num_heads=8, num_kv_heads=8, vocab_size=2048,
                         max_position=512, cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=mode,
                         page_size=16 if mode else 0, weight_quant_bit=8)
    g = Group(m, desc, tp, max_batch=16, max_tokens=512, kv_tokens=2048)
    g.synthetic(31 + tp)
    rng = np.random.RandomState(tp)
    prompts = [rng.randint(3, 2048, size=n) for n in (40, 3, 29, 1, 16, 77, 5, 9, 2, 33, 12)]
    check(f"tp{tp}_tiny_mode{mode}_two_stream", generate(g, prompts, 5), k=1.5)
    assert g.ctx.comm_info(len(prompts))["schedule"] == m.COMM_SCHEDULES[m.SCHED_TWO_LANES]
    g.close()


@pytest.mark.parametrize("tp,overlap", [(2, False), (4, True)])
def test_tensor_parallel_online_i8i8(monkeypatch, tp, overlap):
    """--quant-method online_i8i8 under tensor parallelism: every rank quantises ITS activation slice rows (the per-token scale of the
    wo / w2 inputs is a per-rank quantity, exactly as in the oracle's sharded forward), partial sums are all-reduced in fp16"""
    m = load_pplhip()
    monkeypatch.setenv("PPLHIP_TP_OVERLAP", "1" if overlap else "0")
    monkeypatch.setenv("PPLHIP_TP_OVERLAP_MIN_TOKENS", "2")
    desc = ref.make_desc(hidden_dim=512, intermediate_dim=1024, num_layers=3, num_heads=8, num_kv_heads=8, vocab_size=2048,
                         max_position=512, cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=1, page_size=16,
                         weight_quant_bit=8, act_quant_bit=8)
    g = Group(m, desc, tp, max_batch=16, max_tokens=512, kv_tokens=2048)
    g.synthetic(77 + tp)
    rng = np.random.RandomState(tp)
    prompts = [rng.randint(3, 2048, size=n) for n in (40, 3, 129, 1, 16, 77)]
    # observed (r02): 3.1e-3 .. 5.4e-3 -- the SAME level as this model without tensor parallelism (4.2e-3 .. 4.4e-3,
    # profiles/probes/tp_a8_noise*.py) against 0.7e-3 with fp16 activations: every linear sits behind a discontinuous quantiser, so
    # an input that differs from the oracle's by one fp16 rounding can move an int8 by one step (16x that rounding); the quantisers
    # and the int8 GEMM themselves are bit-exact (tests/test_gpu_w8a8.py) and the greedy tokens agree on every row
    check(f"tp{tp}_online_i8i8_ov{int(overlap)}", generate(g, prompts, 4), k=7)
    g.close()


def test_every_rank_holds_the_same_logits_and_the_group_is_deterministic():
    """invariants that need no oracle: after the all-gather every rank of the group holds bit-identical logits, and a
    repeat from the same state reproduces them bit for bit (fixed reduction order 0..N-1 in the all-reduce kernel)."""
    m = load_pplhip()
    desc = ref.make_desc(hidden_dim=512, intermediate_dim=1024, num_layers=2, num_heads=8, num_kv_heads=4, vocab_size=2048,
                         max_position=256, cache_quant_bit=0, cache_quant_group=1, cache_layout=3, cache_mode=0, weight_quant_bit=8)
    g = Group(m, desc, 4, max_batch=8, max_tokens=256, kv_tokens=1024)
    g.synthetic(5)
    rng = np.random.RandomState(1)
    prompts = [rng.randint(3, 2048, size=n) for n in (33, 7, 64)]
    a = generate(g, prompts, 3)
    per_rank = [g.ctx.copy_logits(3, rank=r) for r in range(4)]
    for r in range(1, 4):
        assert (per_rank[r] == per_rank[0]).all()
    for r in range(4):                       # wipe the slabs so that the repeat starts from the same state
        kb, sb = g.ctx.kv_block_bytes()
        g.ctx.kv_write(r, 0, np.zeros(kb * g.kv_tokens, dtype=np.uint8))
        g.models[r].kv_array(0)[:] = 0
    b = generate(g, prompts, 3)
    for x, y in zip(a, b):
        assert (x[0] == y[0]).all()
    g.close()


def test_llama13b_tp2_rank_slices_w8a16():
    """BASELINE config 3 geometry: unsharded fp16 weights -> pplhip.shard_weights -> per-slice W8A16 quantisation ->
    pplhip_rank_set_tensor on both ranks; packed prefill + decode steps against the oracle sharded 2 ways."""
    m = load_pplhip()
    exp = load_exporter()
    dims = dict(hidden_dim=5120, intermediate_dim=13824, num_layers=2, num_heads=40, num_kv_heads=40, vocab_size=32000)
    desc = ref.make_desc(max_position=2048, cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=0,
                         weight_quant_bit=8, **dims)
    hd, inter, V, H, D = 5120, 13824, 32000, 40, 128
    rng = np.random.RandomState(13)
    gen = np.random.default_rng(13)

    def w(n, k, amp):
        return (gen.standard_normal((n, k), dtype=np.float32) * amp).astype(np.float16)

    weights = {"tok_embeddings.weight": w(V, hd, 1.0), "norm.weight": f16(1 + 0.1 * rng.randn(hd)), "output.weight": w(V, hd, 0.02)}
    for l in range(2):
        weights[f"layers.{l}.attention_norm.weight"] = f16(1 + 0.1 * rng.randn(hd))
        weights[f"layers.{l}.ffn_norm.weight"] = f16(1 + 0.1 * rng.randn(hd))
        weights[f"layers.{l}.attention.wqkv.weight"] = w(3 * H * D, hd, 0.02)
        weights[f"layers.{l}.attention.wo.weight"] = w(hd, H * D, 0.02)
        weights[f"layers.{l}.feed_forward.w13.weight"] = w(2 * inter, hd, 0.02)
        weights[f"layers.{l}.feed_forward.w2.weight"] = w(hd, inter, 0.02)
    g = Group(m, desc, 2, max_batch=16, max_tokens=512, kv_tokens=2048)
    for r in range(2):
        sh = m.shard_weights(weights, desc, 2, r)
        tensors = {}
        for name, arr in sh.items():
            if any(t in name for t in ("wqkv", ".wo.", "w13", ".w2.")):
                q, sc = exp.quant_w8(arr)
                tensors[name] = q
                tensors[name.replace(".weight", ".scale")] = sc
            else:
                tensors[name] = arr
        g.set_tensors(r, tensors)
    del weights
    prompts = [rng.randint(3, V, size=n) for n in (70, 3, 129, 1, 16)]
    check("llama13b_tp2_w8a16_int8kv", generate(g, prompts, 3), k=3.5)   # observed 2.4e-3, 1.4 x the oracle's own noise floor of 1.7e-3 (int8 KV, 40 heads, K up to 6912)
    g.close()


def test_llama70b_tp8_rank_slices_w4a16_decode_at_kv2048():
    """BASELINE config 4 geometry per rank: hidden 8192, 8 query heads sharing ONE KV head, inter 3584, W4A16-g128,
    int8 KV, paged; decode rows at kv 1..2048 over a synthetic history (the grouped-query MFMA decode kernel with
    split-K, the W4 tile GEMM at K = 8192 and K = 3584) and a small cache-prefill step."""
    m = load_pplhip()
    dims = dict(hidden_dim=8192, intermediate_dim=28672, num_layers=2, num_heads=64, num_kv_heads=8, vocab_size=32000)
    desc = ref.make_desc(max_position=4096, cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=1, page_size=16,
                         weight_quant_bit=4, weight_quant_group=128, **dims)
    kv_tokens = 16384
    g = Group(m, desc, 8, max_batch=16, max_tokens=256, kv_tokens=kv_tokens)
    g.synthetic(70)
    g.kv_history(7)
    rng = np.random.RandomState(70)
    # decode: 9 requests whose caches already hold kv_len - 1 tokens
    kv = np.array([2048, 2047, 1500, 1, 300, 17, 1025, 64, 2000])
    n = len(kv)
    cache_idx, mp = plan(desc, kv + 2, kv_tokens, seed=3)
    tok = rng.randint(3, 32000, size=n).astype(np.int64)
    res = []
    start = kv - 1
    for s in range(2):
        got, want, gtok = g.step(tok, np.arange(n + 1), start, cache_idx, n, mp, 1 if s == 0 else 0)
        res.append((got, want, gtok, g.last_alt))
        tok = want.argmax(-1).astype(np.int64)
        start = start + 1
    check("llama70b_tp8_w4a16_decode_kv2048", res, k=1.5)   # observed (r03) < 0.8e-3 with the exact hi + lo operands of the grouped-query kernel (r02: 4.1e-3)
    # cache-prefill: 40 and 17 new tokens on top of 512 and 33 cached ones (history from the synthetic slab)
    prompts = [rng.randint(3, 32000, size=40), rng.randint(3, 32000, size=17)]
    check("llama70b_tp8_w4a16_cache_prefill", generate(g, prompts, 2, start=[512, 33]), k=1.5)   # observed 5.4e-4
    g.close()


def test_one_process_per_rank_over_ipc_handles():
    """the driver's multi-GPU launch mode (one process per rank, exchange regions shared through hipIpc handles gathered
    by the launcher, collective self-test, direct collectives) with both processes on device 0: bench.py --gpus 2 self-
    launches, runs a 2-layer 7B-shaped tensor-parallel decode and must report the direct collectives in use."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PPLHIP_COMM="p2p", PPLHIP_BENCH_ONE_DEVICE="1", OMP_NUM_THREADS="1", PPLHIP_P2P_TIMEOUT_MS="30000")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--layers", "2",
                          "--batch", "64", "--kv-len", "64", "--no-cpu-baseline", "--prefill-sample", "0", "--full"], env=env, timeout=900,
                         capture_output=True)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(line) == 1, out.stdout.decode()[-2000:]
    res = json.loads(line[0])
    assert res["n_gpus"] == 2 and res["value"] > 0 and res["config"]["collectives"].startswith("direct")


def test_bench_retries_on_another_path_when_the_warm_up_fails_on_the_direct_collectives():
    """round 6: first contact with real links may pass the collectives' self-test and still fail in the first real steps (a spin that times
    out, a device error).  bench.py --gpus N then takes ONE retry: every rank agrees (gloo MIN) that the warm-up failed, closes its context and
    re-initialises on RCCL -- here, with both ranks on one device where RCCL cannot run, on the direct collectives again (test hook
    PPLHIP_BENCH_FALLBACK_TO=p2p), after rank 1's first warm-up was made to fail (PPLHIP_BENCH_FAIL_WARMUP_ONCE=1: rank 0 then really times out
    in its all-reduce).  The run must complete and say what happened in collectives.fallbacks."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PPLHIP_COMM="p2p", PPLHIP_BENCH_ONE_DEVICE="1", OMP_NUM_THREADS="1", PPLHIP_P2P_TIMEOUT_MS="4000", PPLHIP_BENCH_FAIL_WARMUP_ONCE="1",
               PPLHIP_BENCH_FALLBACK_TO="p2p")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--layers", "2",
                          "--batch", "64", "--kv-len", "64", "--no-cpu-baseline", "--prefill-sample", "0", "--ragged-steps", "0", "--full"], env=env,
                         timeout=900, capture_output=True)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    line = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(line) == 1, out.stdout.decode()[-2000:]
    res = json.loads(line[0])
    assert res["n_gpus"] == 2 and res["value"] > 0 and "error" not in res
    assert "warm-up steps failed on the direct collectives" in res["collectives"]["fallbacks"] and "re-initialised on p2p" in res["collectives"]["fallbacks"]
