"""fp8 e4m3 KV cache (cache_quant_bit 8, cache_quant_group = head_dim) on the device, against the test-side specification of
tests/kv_fp8.py: the cache write bit for bit, attention against the oracle run on the exactly dequantised fp16 slab with the fp16
tolerances of tests/test_gpu_ops.py, and whole models against the composed oracle."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref
from tests.conftest import load_pplhip
from tests import kv_fp8 as F
from tests.test_gpu_ops import ATT_SHAPES, LONG_CASES, KvCase, ck, close_f16, dev, _drop_device_tensors  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class Fp8Case(KvCase):
    """KvCase over an fp16 slab (the oracle's view) plus the fp8 slab the device sees: the same rows, quantised."""

    def __init__(self, *a, **kw):
        kw["quant"] = 0
        super().__init__(*a, **kw)

    def view8(self, dcache, dscale):
        v = self.view(dcache, dscale)
        v.quant_bit, v.quant_group = 8, self.D
        return v

    def randomise_history(self, rng):
        """random fp16 history, replaced by Q(row) -- what an fp8 cache can hold -- and its fp8 image"""
        self.cache[:] = F.qdq_rows((rng.randn(self.cache.size) * np.exp(0.5 * rng.randn(self.cache.size // self.D)).repeat(self.D))
                                   .astype(np.float16).reshape(-1, self.D)).reshape(-1)


def _write_fp8(m, case):
    """the device writes the step's rows into the fp8 image of case.cache (history as it stands); returns (device q rows)"""
    q8, s8 = F.slab_to_fp8(case.cache, case.D)
    dcache, dscale = dev(q8), dev(s8)
    dq = dev(case.qkv)
    v = case.view8(dcache, dscale)
    ck(m.lib().pplhip_op_rope_kv_write(None, dq.data_ptr(), dev(case.rope).data_ptr(), C.byref(v), dev(case.seq_starts).data_ptr(),
                                       dev(case.start_pos).data_ptr(), dev(case.cache_idx).data_ptr(), case.max_pages, case.B,
                                       case.T, case.H))
    return dq, dcache, dscale, v


@pytest.mark.parametrize("layout,mode", [(0, 0), (1, 1), (2, 0), (3, 1), (3, 0)])
@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 32), (8, 2, 64), (4, 4, 128), (32, 8, 128), (32, 32, 128), (8, 1, 128), (12, 2, 64)])
def test_fp8_write_bit_exact(layout, mode, H, Hkv, D):
    """pplhip_op_rope_kv_write into an fp8 slab: codes and scales equal quantize_rows of the oracle's fp16 write, rotated q equal"""
    m = load_pplhip()
    case = Fp8Case(m, H, Hkv, D, L=3, layer=1, layout=layout, mode=mode, seqlens=[5, 1, 9, 1], start_pos=[0, 7, 3, 0],
                   seed=layout * 10 + mode)
    # a row large enough for e = 8 (saturation; |RoPE'd k| stays finite in fp16) and a tiny one (fp8 subnormals)
    case.qkv[2] = np.clip(case.qkv[2].astype(np.float32) * 15000, -45000, 45000).astype(np.float16)
    case.qkv[2, (H + Hkv) * D] = 60000
    case.qkv[3] = (case.qkv[3].astype(np.float32) * 1e-5).astype(np.float16)
    dq, dcache, dscale, _ = _write_fp8(m, case)
    want_q = case.ref_write()
    hq = H * D
    assert (dq.cpu().numpy().astype(np.float32)[:, :hq] == want_q[:, :hq]).all()
    q8, s8 = F.slab_to_fp8(case.cache, D)
    got_s = dscale.cpu().numpy()
    assert (got_s.view(np.uint16) == s8.view(np.uint16)).all(), int((got_s.view(np.uint16) != s8.view(np.uint16)).sum())
    got_c = dcache.cpu().numpy()
    assert (got_c == q8).all(), int((got_c != q8).sum())
    assert (F.exp_of(s8) == 8).any() and (np.abs(F.fp8_to_slab(q8, s8, D).astype(np.float32)) > 0).any()


def _attention(m, case, nb, max_len, split=1, ws=None, ws_bytes=0):
    dq, dcache, dscale, v = _write_fp8(m, case)
    q32 = case.ref_write()
    case.cache[:] = F.qdq_rows(case.cache.reshape(-1, case.D)).reshape(-1)  # the rows written this step, as the fp8 cache holds them
    want = case.ref_attention(q32)
    out = torch.zeros((case.T, case.H * case.D), dtype=torch.float16, device="cuda")
    ck(m.lib().pplhip_op_attention(None, dq.data_ptr(), C.byref(v), dev(case.seq_starts).data_ptr(), dev(case.start_pos).data_ptr(),
                                   dev(case.cache_idx).data_ptr(), case.max_pages, case.B, case.T, nb, max_len, case.max_kv_len,
                                   case.H, split, ws, ws_bytes, out.data_ptr()))
    # the device's own write is the fp8 image of the oracle's fp16 write: the slab the oracle read
    assert (F.fp8_to_slab(dcache.cpu().numpy(), dscale.cpu().numpy(), case.D).view(np.uint16) == case.cache.view(np.uint16)).all()
    return out.cpu().numpy().astype(np.float32), want


@pytest.mark.parametrize("layout,mode", [(3, 0), (0, 0), (2, 1), (3, 1)])
@pytest.mark.parametrize("H,Hkv,D", ATT_SHAPES)
@pytest.mark.parametrize("split", [1, 3])
def test_fp8_attention_decode(layout, mode, H, Hkv, D, split):
    m = load_pplhip()
    kvlen = [1, 2, 63, 64, 65, 257, 700, 33]
    case = Fp8Case(m, H, Hkv, D, L=2, layer=1, layout=layout, mode=mode, seqlens=[1] * len(kvlen),
                   start_pos=[k - 1 for k in kvlen], seed=D + 1, page_size=16, decoding_batches=len(kvlen))
    case.randomise_history(np.random.RandomState(5))
    ws = torch.empty(case.B * H * split * (D + 2) + 16, dtype=torch.float32, device="cuda")
    got, want = _attention(m, case, case.B, 1, split, ws.data_ptr(), ws.numel() * 4)
    close_f16(got, want, rel=1.5e-3, abs_=1.5e-3)


@pytest.mark.parametrize("H,Hkv,D,mode", [(8, 1, 128, 1), (16, 2, 64, 0), (8, 2, 128, 0)])
def test_fp8_attention_decode_gqa_small_blocks(H, Hkv, D, mode):
    """>= 512 blocks in one grouped-query launch: the 4-wave block form"""
    m = load_pplhip()
    rng = np.random.RandomState(11)
    nb = 520 // Hkv + 3
    kvlen = list(rng.randint(1, 90, size=nb))
    case = Fp8Case(m, H, Hkv, D, L=1, layer=0, layout=3, mode=mode, seqlens=[1] * nb, start_pos=[k - 1 for k in kvlen], seed=3,
                   page_size=16, decoding_batches=nb)
    case.randomise_history(rng)
    got, want = _attention(m, case, nb, 1)
    close_f16(got, want, rel=1.5e-3, abs_=1.5e-3)


@pytest.mark.parametrize("layout,mode", [(3, 0), (1, 0), (3, 1)])
@pytest.mark.parametrize("H,Hkv,D", ATT_SHAPES)
def test_fp8_attention_prefill_and_mixed(layout, mode, H, Hkv, D):
    m = load_pplhip()
    seqlens = [1, 1, 130, 1, 64, 17, 200]
    start = [40, 5, 0, 0, 64, 30, 70]
    case = Fp8Case(m, H, Hkv, D, L=2, layer=0, layout=layout, mode=mode, seqlens=seqlens, start_pos=start, seed=D * 3,
                   page_size=16, decoding_batches=2)
    case.randomise_history(np.random.RandomState(9))
    got, want = _attention(m, case, 2, case.max_seq_len)
    vmax = float(np.abs(case.cache.astype(np.float32)).max())
    close_f16(got, want, rel=1e-3, abs_=1e-3 * vmax)


@pytest.mark.parametrize("seqlens,start,heads,mode", [c if len(c) == 4 else c + (1,) for c in LONG_CASES])
def test_fp8_attention_long_prefill_and_cache_prefill(seqlens, start, heads, mode):
    m = load_pplhip()
    H, Hkv = heads
    case = Fp8Case(m, H, Hkv, 128, L=1, layer=0, layout=3, mode=mode, seqlens=seqlens, start_pos=start, seed=len(seqlens) + H,
                   page_size=16, decoding_batches=0)
    case.randomise_history(np.random.RandomState(17))
    got, want = _attention(m, case, 0, case.max_seq_len)
    vmax = float(np.abs(case.cache.astype(np.float32)).max())
    close_f16(got, want, rel=1e-3, abs_=1e-3 * vmax)


@pytest.mark.parametrize("seqlens,start,heads,mode,nb", [([16], [8176], (8, 1), 1, 0), ([300, 129], [2500, 900], (4, 4), 1, 0),
                                                           ([1, 1, 1, 16, 9], [1500, 1200, 3000, 4000, 2050], (4, 4), 1, 3)])
def test_fp8_attention_short_suffix_split_kv(seqlens, start, heads, mode, nb):
    """short suffix behind a long cached prefix: the split-KV form (workspace given) and the unsplit one, both against the oracle"""
    m = load_pplhip()
    H, Hkv = heads
    D = 128
    outs = []
    for with_ws in (True, False):
        case = Fp8Case(m, H, Hkv, D, L=1, layer=0, layout=3, mode=mode, seqlens=seqlens, start_pos=start, seed=len(seqlens) + H,
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
    d8 = F.desc_with(desc, cache_quant_bit=8, cache_quant_group=64)
    ctx = m.Context(m.copy_desc(d8), max_running_batch=16, max_tokens_per_step=512)
    ctx.init_synthetic(0, 7)
    ctx.kv_alloc(0, kv_tokens)
    return rm, ctx


def _run_steps(m, ctx, orc, steps, mode, page_size=16):
    """steps: list of (tokens per request, start_pos per request, decoding_batches); cache indices: contiguous blocks of 256 slots, or
    shuffled pages.  Returns [(device logits, oracle logits)]."""
    rng = np.random.RandomState(1)
    B = max(len(s[0]) for s in steps)
    if mode == 0:
        ci_all = np.arange(B, dtype=np.int64) * 256
        maxp = 0
    else:
        maxp = 256 // page_size
        ci_all = rng.permutation(B * maxp).astype(np.int64).reshape(B, maxp)
    res = []
    for s, (lens, sp, nd) in enumerate(steps):
        Bs = len(lens)
        tok = rng.randint(3, 1024, size=int(sum(lens))).astype(np.int64)
        ss = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        sp = np.asarray(sp, dtype=np.int64)
        ci = ci_all[:Bs].copy()
        want = orc.forward(ref.make_step(tok, ss, sp, ci, nd, max_pages=maxp))
        ctx.set_inputs(0, m.make_step(tok, ss, sp, ci, nd, max_pages=maxp, req_list_changed=1))
        ctx.run(0)
        res.append((ctx.copy_logits(Bs), want))
    return res


MODEL_STEPS = [
    ([9, 4, 30], [0, 0, 0], 0),                 # cold prefill, ragged
    ([1, 1, 1], [9, 4, 30], 3),                 # decode
    ([1, 1, 1, 20], [10, 5, 31, 0], 3),         # decode + a new request
    ([1, 1, 1, 1], [11, 6, 32, 20], 4),         # decode
    ([1, 1, 5], [12, 7, 10], 2),                # a partial prefix hit: request 2 recomputes from position 10
]


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("layout,mode", [(3, 0), (3, 1), (1, 1)])
def test_fp8_model_matches_composed_oracle(H, Hkv, layout, mode):
    """tiny MHA / GQA models, several steps (cold prefill, decodes, a new request, a partial prefix hit), contiguous and paged:
    device logits against the composed oracle (fp16 forward with Q(row) after every KV write), at the smoke bar of the fp16 model"""
    m = load_pplhip()
    rm, ctx = _model(m, H, Hkv, layout, mode)
    orc = F.ComposedOracle(rm, 1024)
    for s, (got, want) in enumerate(_run_steps(m, ctx, orc, MODEL_STEPS, mode)):
        tol = 1.5e-3 * max(1.0, float(np.abs(want).max()))
        err = float(np.abs(got - want).max())
        assert err <= tol, f"step {s}: {err} > {tol}"
    ctx.close()


def test_fp8_model_full_prefix_hit_and_permutation_invariance():
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
    # the single-token recompute over the fp8 rows equals the prefill's own last-row logits up to the decode kernel's order
    tol = 1.5e-3 * max(1.0, float(np.abs(first).max()))
    assert float(np.abs(outs[0] - first).max()) <= tol
    ctx.close()


def test_fp8_model_layout_mode_invariance():
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


# ---------------------------------------------------------------------------------------------------------------
# sizes and rejections
# ---------------------------------------------------------------------------------------------------------------
def test_fp8_sizes_capacity_and_rejections():
    m = load_pplhip()
    L = m.lib()
    assert L.pplhip_version() == (1 << 16) | 2

    def ctx_of(bit, group):   # 4 layers, 8 heads of 128 (2 KV heads)
        desc = ref.make_desc(hidden_dim=1024, intermediate_dim=2048, num_layers=4, num_heads=8, num_kv_heads=2, vocab_size=1024,
                             cache_quant_bit=bit, cache_quant_group=group, weight_quant_bit=8)
        return m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=64)

    c8, ci8 = ctx_of(8, 128), ctx_of(8, 8)
    assert tuple(c8.kv_block_bytes()) == (4 * 2 * 2 * 128, 4 * 2 * 2 * 2)
    cap8, capi8 = c8.kv_capacity(0.5), ci8.kv_capacity(0.5)
    assert cap8 >= 1.2 * capi8, (cap8, capi8)
    c8.close()
    ci8.close()
    for bit, group in ((8, 16), (8, 64), (0, 128), (4, 128)):
        with pytest.raises(Exception):
            ctx_of(bit, group)
    # an operator view with a non-format pair is rejected as well
    case = Fp8Case(m, 4, 4, 128, L=1, layer=0, layout=3, mode=0, seqlens=[3], start_pos=[0])
    q8, s8 = F.slab_to_fp8(case.cache, 128)
    v = case.view8(dev(q8), dev(s8))
    v.quant_group = 64
    rc = L.pplhip_op_rope_kv_write(None, dev(case.qkv).data_ptr(), dev(case.rope).data_ptr(), C.byref(v),
                                   dev(case.seq_starts).data_ptr(), dev(case.start_pos).data_ptr(), dev(case.cache_idx).data_ptr(), 0,
                                   case.B, case.T, 4)
    assert rc != 0
