"""int4 KV cache (cache_quant_bit 4, cache_quant_group 32) on the device, against the test-side specification of tests/kv_i4.py:
the cache write bit for bit, attention against the oracle run on the exactly dequantised fp16 slab with the fp16 tolerances of
tests/test_gpu_ops.py (the operands are exact, as with fp8), and whole models against the composed oracle.  Case for case
tests/test_gpu_kv_fp8.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import ref
from tests.conftest import ROOT, load_pplhip
from tests import kv_i4 as I
from tests.test_gpu_kv_fp8 import MODEL_STEPS, _run_steps
from tests.test_gpu_ops import ATT_SHAPES, LONG_CASES, KvCase, ck, close_f16, dev, _drop_device_tensors  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class I4Case(KvCase):
    """KvCase over an fp16 slab (the oracle's view) plus the int4 slab the device sees: the same rows, quantised."""

    def __init__(self, *a, **kw):
        kw["quant"] = 0
        super().__init__(*a, **kw)

    def view4(self, dcache, dscale):
        v = self.view(dcache, dscale)
        v.quant_bit, v.quant_group = 4, 32
        return v

    def randomise_history(self, rng):
        """random fp16 history, replaced by Q(group) -- what an int4 cache can hold -- and its int4 image"""
        self.cache[:] = I.qdq_rows((rng.randn(self.cache.size) * np.exp(0.5 * rng.randn(self.cache.size // self.D)).repeat(self.D))
                                   .astype(np.float16).reshape(-1, self.D)).reshape(-1)


def _write_i4(m, case):
    """the device writes the step's rows into the int4 image of case.cache (history as it stands)"""
    q4, s4 = I.slab_to_i4(case.cache, case.D)
    dcache, dscale = dev(q4), dev(s4)
    dq = dev(case.qkv)
    v = case.view4(dcache, dscale)
    ck(m.lib().pplhip_op_rope_kv_write(None, dq.data_ptr(), dev(case.rope).data_ptr(), C.byref(v), dev(case.seq_starts).data_ptr(),
                                       dev(case.start_pos).data_ptr(), dev(case.cache_idx).data_ptr(), case.max_pages, case.B,
                                       case.T, case.H))
    return dq, dcache, dscale, v


@pytest.mark.parametrize("layout,mode", [(0, 0), (1, 1), (2, 0), (3, 1), (3, 0)])
@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 32), (8, 2, 64), (4, 4, 128), (32, 8, 128), (8, 1, 128), (12, 2, 64)])
def test_i4_write_bit_exact(layout, mode, H, Hkv, D):
    """pplhip_op_rope_kv_write into an int4 slab: codes and scales equal slab_to_i4 of the oracle's fp16 write, rotated q equal"""
    m = load_pplhip()
    case = I4Case(m, H, Hkv, D, L=3, layer=1, layout=layout, mode=mode, seqlens=[5, 1, 9, 1], start_pos=[0, 7, 3, 0],
                  seed=layout * 10 + mode)
    # a row scaled up until a group's scale hits the 9344 cap (|RoPE'd k| stays finite in fp16; v is stored as it is), a row scaled
    # by 1e-5 for the 2^-14 floor, and a group of zeros
    case.qkv[2] = np.clip(case.qkv[2].astype(np.float32) * 15000, -45000, 45000).astype(np.float16)
    case.qkv[2, (H + Hkv) * D + 5] = 65504
    case.qkv[3] = (case.qkv[3].astype(np.float32) * 1e-5).astype(np.float16)
    case.qkv[4, (H + Hkv) * D:(H + Hkv) * D + 32] = 0
    dq, dcache, dscale, _ = _write_i4(m, case)
    want_q = case.ref_write()
    hq = H * D
    assert (dq.cpu().numpy().astype(np.float32)[:, :hq] == want_q[:, :hq]).all()
    q4, s4 = I.slab_to_i4(case.cache, D)
    got_s = dscale.cpu().numpy()
    assert (got_s.view(np.uint16) == s4.view(np.uint16)).all(), int((got_s.view(np.uint16) != s4.view(np.uint16)).sum())
    got_c = dcache.cpu().numpy()
    assert (got_c == q4).all(), int((got_c != q4).sum())
    # the cap and the floor were reached by WRITTEN groups (never-written slots are zero groups at the floor as well), and a written
    # group of zeros is all nibble 8
    written = np.abs(case.cache.astype(np.float32)).reshape(-1, 32).max(-1) > 0
    s32 = s4.astype(np.float32)
    assert (s32[written] == 9344.0).any() and (s32[written] == 2.0 ** -14).any()
    assert (np.abs(I.i4_to_slab(q4, s4, D).astype(np.float32)) > 0).any()
    assert (q4.view(np.uint8).reshape(-1, 16)[~written] == 0x88).all()


def _attention(m, case, nb, max_len, split=1, ws=None, ws_bytes=0):
    dq, dcache, dscale, v = _write_i4(m, case)
    q32 = case.ref_write()
    case.cache[:] = I.qdq_rows(case.cache.reshape(-1, case.D)).reshape(-1)  # the rows written this step, as the int4 cache holds them
    want = case.ref_attention(q32)
    out = torch.zeros((case.T, case.H * case.D), dtype=torch.float16, device="cuda")
    ck(m.lib().pplhip_op_attention(None, dq.data_ptr(), C.byref(v), dev(case.seq_starts).data_ptr(), dev(case.start_pos).data_ptr(),
                                   dev(case.cache_idx).data_ptr(), case.max_pages, case.B, case.T, nb, max_len, case.max_kv_len,
                                   case.H, split, ws, ws_bytes, out.data_ptr()))
    # the device's own write is the int4 image of the oracle's fp16 write: the slab the oracle read
    assert (I.i4_to_slab(dcache.cpu().numpy(), dscale.cpu().numpy(), case.D).view(np.uint16) == case.cache.view(np.uint16)).all()
    return out.cpu().numpy().astype(np.float32), want


# 16, 32 or 64 rows per wave-load (head_dim 128, 64, 32) and an unroll of 4: a wave's first group ends at 64, 128 and 256 keys -- the
# smallest lengths that cross each; 1030 moves the paged kernel's 64-page window
KV_LENS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 700, 1030]


@pytest.mark.parametrize("layout,mode", [(3, 0), (0, 0), (2, 1), (3, 1)])
@pytest.mark.parametrize("H,Hkv,D", ATT_SHAPES)
@pytest.mark.parametrize("split", [1, 3])
def test_i4_attention_decode(layout, mode, H, Hkv, D, split):
    m = load_pplhip()
    case = I4Case(m, H, Hkv, D, L=2, layer=1, layout=layout, mode=mode, seqlens=[1] * len(KV_LENS),
                  start_pos=[k - 1 for k in KV_LENS], seed=D + 1, page_size=16, decoding_batches=len(KV_LENS))
    case.randomise_history(np.random.RandomState(5))
    ws = torch.empty(case.B * H * split * (D + 2) + 16, dtype=torch.float32, device="cuda")
    got, want = _attention(m, case, case.B, 1, split, ws.data_ptr(), ws.numel() * 4)
    close_f16(got, want, rel=1.5e-3, abs_=1.5e-3)


@pytest.mark.parametrize("H,Hkv,D,mode", [(8, 1, 128, 1), (8, 2, 128, 0)])
def test_i4_attention_decode_gqa_small_blocks(H, Hkv, D, mode):
    """>= 512 blocks in one grouped-query launch: the 4-wave block form"""
    m = load_pplhip()
    rng = np.random.RandomState(11)
    nb = 520 // Hkv + 3
    kvlen = list(rng.randint(1, 90, size=nb))
    case = I4Case(m, H, Hkv, D, L=1, layer=0, layout=3, mode=mode, seqlens=[1] * nb, start_pos=[k - 1 for k in kvlen], seed=3,
                  page_size=16, decoding_batches=nb)
    case.randomise_history(rng)
    got, want = _attention(m, case, nb, 1)
    close_f16(got, want, rel=1.5e-3, abs_=1.5e-3)


@pytest.mark.parametrize("layout,mode", [(3, 0), (1, 0), (3, 1)])
@pytest.mark.parametrize("H,Hkv,D", ATT_SHAPES)
def test_i4_attention_prefill_and_mixed(layout, mode, H, Hkv, D):
    m = load_pplhip()
    seqlens = [1, 1, 130, 1, 64, 17, 200]
    start = [40, 5, 0, 0, 64, 30, 70]
    case = I4Case(m, H, Hkv, D, L=2, layer=0, layout=layout, mode=mode, seqlens=seqlens, start_pos=start, seed=D * 3,
                  page_size=16, decoding_batches=2)
    case.randomise_history(np.random.RandomState(9))
    got, want = _attention(m, case, 2, case.max_seq_len)
    vmax = float(np.abs(case.cache.astype(np.float32)).max())
    close_f16(got, want, rel=1e-3, abs_=1e-3 * vmax)


@pytest.mark.parametrize("seqlens,start,heads,mode", [c if len(c) == 4 else c + (1,) for c in LONG_CASES])
def test_i4_attention_long_prefill_and_cache_prefill(seqlens, start, heads, mode):
    m = load_pplhip()
    H, Hkv = heads
    case = I4Case(m, H, Hkv, 128, L=1, layer=0, layout=3, mode=mode, seqlens=seqlens, start_pos=start, seed=len(seqlens) + H,
                  page_size=16, decoding_batches=0)
    case.randomise_history(np.random.RandomState(17))
    got, want = _attention(m, case, 0, case.max_seq_len)
    vmax = float(np.abs(case.cache.astype(np.float32)).max())
    close_f16(got, want, rel=1e-3, abs_=1e-3 * vmax)


@pytest.mark.parametrize("seqlens,start,heads,mode,nb", [([16], [8176], (8, 1), 1, 0), ([300, 129], [2500, 900], (4, 4), 1, 0),
                                                           ([1, 1, 1, 16, 9], [1500, 1200, 3000, 4000, 2050], (4, 4), 1, 3)])
def test_i4_attention_short_suffix_split_kv(seqlens, start, heads, mode, nb):
    """short suffix behind a long cached prefix: the split-KV form (workspace given) and the unsplit one, both against the oracle"""
    m = load_pplhip()
    H, Hkv = heads
    D = 128
    outs = []
    for with_ws in (True, False):
        case = I4Case(m, H, Hkv, D, L=1, layer=0, layout=3, mode=mode, seqlens=seqlens, start_pos=start, seed=len(seqlens) + H,
                      page_size=16, decoding_batches=nb)
        case.randomise_history(np.random.RandomState(23))
        n_ws = (case.T - nb) * H * 32 * (D + 2)
        ws = torch.zeros(n_ws, dtype=torch.float32, device="cuda")
        got, want = _attention(m, case, nb, case.max_seq_len, 1, ws.data_ptr() if with_ws else None, n_ws * 4 if with_ws else 0)
        if with_ws:
            assert float(ws.abs().max()) > 0, "the split-KV path did not run"
        vmax = float(np.abs(case.cache.astype(np.float32)).max())
        close_f16(got, want, rel=1e-3, abs_=1e-3 * vmax)
        outs.append(got)
    close_f16(outs[0], outs[1], rel=2e-3, abs_=2e-4 * vmax)


# ---------------------------------------------------------------------------------------------------------------
# whole models
# ---------------------------------------------------------------------------------------------------------------
def _model(m, H, Hkv, layout, mode, page_size=16, kv_tokens=1024):
    desc = ref.make_desc(hidden_dim=H * 64, intermediate_dim=512, num_layers=2, num_heads=H, num_kv_heads=Hkv, vocab_size=1024,
                         max_position=1024, cache_quant_bit=0, cache_quant_group=1, cache_layout=layout, cache_mode=mode,
                         page_size=page_size if mode else 0, weight_quant_bit=8)
    rm = ref.RefModel(desc)
    rm.init_synthetic(7)
    d4 = I.desc_with(desc, cache_quant_bit=4, cache_quant_group=32)
    ctx = m.Context(m.copy_desc(d4), max_running_batch=16, max_tokens_per_step=512)
    ctx.init_synthetic(0, 7)
    ctx.kv_alloc(0, kv_tokens)
    return rm, ctx


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("layout,mode", [(3, 0), (3, 1), (1, 1)])
def test_i4_model_matches_composed_oracle(H, Hkv, layout, mode):
    """tiny MHA / GQA models, several steps (cold prefill, decodes, a new request, a partial prefix hit), contiguous and paged:
    device logits against the composed oracle (fp16 forward with Q(group) after every KV write), at the bar of the fp8 model test.
    The device's slab is the int4 image of the oracle's at the end."""
    m = load_pplhip()
    rm, ctx = _model(m, H, Hkv, layout, mode)
    orc = I.ComposedOracle(rm, 1024)
    for s, (got, want) in enumerate(_run_steps(m, ctx, orc, MODEL_STEPS, mode)):
        tol = 1.5e-3 * max(1.0, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        print(f"step {s}: max |dlogit| {err:.3e} (bar {tol:.3e})")
        assert err <= tol, f"step {s}: {err} > {tol}"
    ctx.close()


def test_i4_model_full_prefix_hit_and_permutation_invariance():
    """a full prefix hit (a request whose cached rows are read without being rewritten) and a batch permutation: bit-identical
    logits per request"""
    m = load_pplhip()
    rm, ctx = _model(m, 8, 2, 3, 1)
    rng = np.random.RandomState(4)
    maxp = 16
    pages = rng.permutation(4 * maxp).astype(np.int64).reshape(4, maxp)
    prompts = [rng.randint(3, 1024, size=n).astype(np.int64) for n in (17, 33, 5, 64)]
    ss = np.concatenate([[0], np.cumsum([len(p) for p in prompts])]).astype(np.int64)
    ctx.set_inputs(0, m.make_step(np.concatenate(prompts), ss, np.zeros(4, np.int64), pages, 0, max_pages=maxp, req_list_changed=1))
    ctx.run(0)
    first = ctx.copy_logits(4)
    # full prefix hit: recompute only the last token of every prompt over the cached rows
    last = np.array([p[-1] for p in prompts], dtype=np.int64)
    sp = np.array([len(p) - 1 for p in prompts], dtype=np.int64)
    outs = []
    for perm in (np.arange(4), np.array([2, 0, 3, 1])):
        ctx.set_inputs(0, m.make_step(last[perm], np.arange(5, dtype=np.int64), sp[perm], pages[perm], 4, max_pages=maxp,
                                      req_list_changed=1))
        ctx.run(0)
        g = ctx.copy_logits(4)
        o = np.empty_like(g)
        o[perm] = g
        outs.append(o)
    assert (outs[0] == outs[1]).all()
    # the single-token recompute over the int4 rows equals the prefill's own last-row logits up to the decode kernel's order
    tol = 1.5e-3 * max(1.0, float(np.abs(first).max()))
    assert float(np.abs(outs[0] - first).max()) <= tol
    ctx.close()


def test_i4_model_layout_mode_invariance():
    """the same steps on every cache layout and mode: bit-identical logits"""
    m = load_pplhip()
    res = []
    for layout, mode in ((0, 0), (2, 0), (3, 0)):
        rm, ctx = _model(m, 8, 2, layout, mode)
        rng = np.random.RandomState(2)
        tok = rng.randint(3, 1024, size=40).astype(np.int64)
        ss = np.array([0, 25, 40], dtype=np.int64)
        ci = np.array([0, 300], dtype=np.int64)
        ctx.set_inputs(0, m.make_step(tok, ss, np.zeros(2, np.int64), ci, 0, req_list_changed=1))
        ctx.run(0)
        a = ctx.copy_logits(2)
        ctx.set_inputs(0, m.make_step(tok[:2], np.arange(3, dtype=np.int64), np.array([25, 15], np.int64), ci, 2, req_list_changed=1))
        ctx.run(0)
        res.append((a, ctx.copy_logits(2)))
        ctx.close()
    for a, b in res[1:]:
        assert (a == res[0][0]).all() and (b == res[0][1]).all()


def test_i4_synthetic_fill_is_in_format():
    """pplhip_kv_fill_synthetic: nibbles 1..15 only and scales the rule can produce (8 significant bits, inside [2^-14, 9344])"""
    m = load_pplhip()
    rm, ctx = _model(m, 8, 2, 3, 0, kv_tokens=64)
    ctx.kv_fill_synthetic(0, 3)
    c, s = ctx.kv_read(0, 0).view(np.uint8), ctx.kv_read(0, 1)
    assert (c & 15 != 0).all() and (c >> 4 != 0).all()
    assert (s.view(np.uint16) & 7 == 0).all() and (s.astype(np.float32) >= 2.0 ** -14).all() and (s.astype(np.float32) <= 9344).all()
    assert len(np.unique(c)) > 100 and len(np.unique(s)) > 100
    I.i4_to_slab(c, s, 64)   # asserts that every q * s is an fp16 number
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# sizes and rejections
# ---------------------------------------------------------------------------------------------------------------
def test_i4_sizes_capacity_and_rejections(tmp_path):
    m = load_pplhip()
    L = m.lib()

    def ctx_of(bit, group, heads=8):   # 4 layers, 8 heads of 128 (2 KV heads)
        desc = ref.make_desc(hidden_dim=1024, intermediate_dim=2048, num_layers=4, num_heads=heads, num_kv_heads=2, vocab_size=1024,
                             cache_quant_bit=bit, cache_quant_group=group, weight_quant_bit=8)
        return m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=64)

    c4, ci8 = ctx_of(4, 32), ctx_of(8, 8)
    assert tuple(c4.kv_block_bytes()) == (4 * 2 * 2 * 128 // 2, 4 * 2 * 2 * (128 // 32) * 2)
    cap4, capi8 = c4.kv_capacity(0.5), ci8.kv_capacity(0.5)
    assert cap4 >= 2.2 * capi8, (cap4, capi8)
    c4.close()
    ci8.close()
    for bit, group in ((4, 8), (4, 64), (4, 128)):
        with pytest.raises(Exception):
            ctx_of(bit, group)
    with pytest.raises(Exception):
        ctx_of(4, 32, heads=64)   # head_dim 16
    # an operator view with a non-format pair is rejected as well
    case = I4Case(m, 4, 4, 128, L=1, layer=0, layout=3, mode=0, seqlens=[3], start_pos=[0])
    q4, s4 = I.slab_to_i4(case.cache, 128)
    v = case.view4(dev(q4), dev(s4))
    v.quant_group = 64
    rc = L.pplhip_op_rope_kv_write(None, dev(case.qkv).data_ptr(), dev(case.rope).data_ptr(), C.byref(v),
                                   dev(case.seq_starts).data_ptr(), dev(case.start_pos).data_ptr(), dev(case.cache_idx).data_ptr(), 0,
                                   case.B, case.T, 4)
    assert rc != 0
    # ... and by the generator's parameter check: offline_inference refuses such a params.json before it generates
    tool = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "offline_inference")
    assert os.path.exists(tool), f"{tool} missing: run __graft_entry__.build()"
    cfg = json.load(open(os.path.join(ROOT, "ppl.llm.serving_amd", "configs", "tiny_w8a16_kv4_paged.json")))
    for group, hidden in ((8, 256), (64, 256), (128, 256), (32, 64)):   # (32, 64): head_dim 16
        bad = dict(cfg, cache_quant_group=group, hidden_dim=hidden)
        path = tmp_path / f"bad_{group}_{hidden}.json"
        path.write_text(json.dumps(bad))
        r = subprocess.run([tool, "--model-param-path", str(path), "--synthetic-weights", "--kv-cache-max-tokens", "512",
                            "--max-running-batch", "8", "--max-tokens-per-step", "64", "--workload", "prompts4"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Answer tokens:" not in r.stdout, (group, hidden)


@pytest.mark.parametrize("cache_mode", [0, 1])
def test_i4_offline_inference_generates(tmp_path, cache_mode):
    """the C++ host stack (generator -> engine -> backend -> library) generates with the int4 pair in both cache modes"""
    tool = os.path.join(ROOT, "ppl.llm.serving_amd", "build", "offline_inference")
    assert os.path.exists(tool), f"{tool} missing: run __graft_entry__.build()"
    cfg = json.load(open(os.path.join(ROOT, "ppl.llm.serving_amd", "configs", "tiny_w8a16_kv4_paged.json")))
    assert (cfg["cache_quant_bit"], cfg["cache_quant_group"]) == (4, 32)
    cfg["cache_mode"] = cache_mode
    path = tmp_path / "params.json"
    path.write_text(json.dumps(cfg))
    out = subprocess.check_output([tool, "--model-param-path", str(path), "--synthetic-weights", "--synthetic-seed", "77",
                                   "--kv-cache-max-tokens", "512", "--max-running-batch", "8", "--max-tokens-per-step", "64",
                                   "--workload", "prompts4"], timeout=300).decode()
    answers = [[int(x) for x in line.split(":")[1].split()] for line in out.splitlines() if line.startswith("Answer tokens:")]
    assert [len(a) for a in answers] == [8, 9, 10, 11]
