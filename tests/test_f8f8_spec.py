"""online_f8f8 specification (tests/f8f8.py) on the CPU: the row quantiser against the e4m3fn format's own definition, the exactness
facts the composed oracle rests on, the composed oracle itself, and the library's new entry points."""
import ctypes
import os

import numpy as np
import pytest

from oracle import ref
from tests import f8f8 as F
from tests.conftest import ROOT, load_pplhip

torch = pytest.importorskip("torch")


def _rows(seed, n=64, k=96):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, k)) * np.exp(3 * rng.standard_normal((n, 1)))
    x[0] = 0                                              # all-zero row: e = -15
    x[1] = np.linspace(-65504, 65504, k)                  # amax at the fp16 limit: e = 8, codes saturate at +-240
    x[2] = rng.standard_normal(k) * 2.0 ** -20            # fp8 subnormals under e = -15
    x[3, :4] = [448 * 2.0 ** -3, 0.5 * 2.0 ** -9, 1.5 * 2.0 ** -9, 9.5]   # exact ties at the subnormal and normal ranges
    return np.clip(x, -65504, 65504).astype(np.float16)


@pytest.mark.parametrize("seed", range(3))
def test_quantiser_matches_the_format_definition(seed):
    """codes of quantize_rows = the nearest e4m3fn value of x 2^-e with ties to even, searched over all 256 codes; e is the smallest
    integer with 448 2^e >= amax; torch.float8_e4m3fn decodes them to the same values"""
    x = _rows(seed)
    q, e = F.quantize_rows(x)
    x32 = x.astype(np.float64)
    amax = np.abs(x32).max(1)
    for r in range(x.shape[0]):
        want_e = -15 if amax[r] == 0 else int(np.clip(np.ceil(np.log2(amax[r] / 448)), -15, 8))
        assert e[r] == want_e, (r, amax[r], e[r])
        lim = 240.0 if e[r] == 8 else 448.0
        for k in range(0, x.shape[1], 7):
            y = float(np.clip(x32[r, k] * 2.0 ** -int(e[r]), -lim, lim))
            assert int(q[r, k]) == F.rne_code(y) or (y == 0 and int(q[r, k]) & 0x7f == 0), (r, k, y, q[r, k])
    vals = F.e4m3_values()
    dec = torch.from_numpy(q).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert (dec == vals[q]).all()
    assert e[0] == -15 and (q[0] & 0x7f == 0).all()
    assert e[1] == 8 and np.abs(vals[q[1]]).max() == 240
    assert (np.abs(vals[q[2]]) < 2.0 ** -6).any()       # subnormal codes in use


def test_dequantised_values_are_fp16_exact():
    x = _rows(7, n=256, k=128)
    q, e = F.quantize_rows(x)
    v = F.e4m3_values()[q] * np.ldexp(1.0, e)[:, None]
    assert (v.astype(np.float16).astype(np.float64) == v).all()
    assert (F.dequantize(q, e).astype(np.float64) == v).all()
    # Q is idempotent: the rows an fp8 operand stands for quantise to themselves
    assert (F.qdq(F.dequantize(q, e)) == F.dequantize(q, e).astype(np.float32)).all()


def test_scaled_integer_product_equals_the_product_of_dequantised_values():
    """2^(ex + ew) * sum qx qw (fp64) = sum (qx 2^ex)(qw 2^ew): the scale may sit in the epilogue, in the MFMA's E8M0 operands or both"""
    rng = np.random.default_rng(3)
    M, N, K = 9, 11, 1376
    qx, ex = F.quantize_rows(_rows(11, n=M, k=K))
    qw, ew = F.quantize_rows((rng.standard_normal((N, K)) * 0.02).astype(np.float16))
    vx, vw = F.e4m3_values()[qx], F.e4m3_values()[qw]
    a = (vx @ vw.T) * np.ldexp(1.0, ex[:, None] + ew[None, :])
    b = (vx * np.ldexp(1.0, ex)[:, None]) @ (vw * np.ldexp(1.0, ew)[:, None]).T
    assert (a == b).all()
    # every product of two dequantised values is exact in fp32 (>= 2^-48 in magnitude when nonzero, < 2^24 significand bits)
    p = (vx[:, :64, None] * np.ldexp(1.0, ex)[:, None, None]) * (vw.T[None, :64, :] * np.ldexp(1.0, ew)[None, None, :])
    assert (p.astype(np.float32).astype(np.float64) == p).all()


def _tiny(**kw):
    return ref.make_desc(hidden_dim=256, intermediate_dim=176, num_layers=2, num_heads=4, num_kv_heads=2, vocab_size=512,
                         max_position=256, cache_quant_bit=0, cache_quant_group=1, cache_layout=3, cache_mode=0, **kw)


def test_composed_oracle_without_quantisation_is_ref_forward():
    desc = _tiny()
    rm = ref.RefModel(desc)
    rm.init_synthetic(3)
    rm.kv_alloc(512)
    orc = F.ComposedOracle(rm, 512, kv="fp16", linears=False)
    rng = np.random.RandomState(2)
    tok = rng.randint(3, 512, size=30).astype(np.int64)
    ss = np.array([0, 21, 30], dtype=np.int64)
    ci = np.array([0, 256], dtype=np.int64)
    steps = [(tok, ss, np.zeros(2, np.int64), 0), (tok[[5, 7]], np.arange(3, dtype=np.int64), np.array([21, 9], np.int64), 2)]
    for t, s, sp, nd in steps:
        st = ref.make_step(t, s, sp, ci, nd)
        assert (orc.forward(st) == ref.forward([rm], st)).all()
    # with the fp8 linears on, the forward moves (by the quantisation noise, not more)
    st = ref.make_step(rng.randint(3, 512, size=8).astype(np.int64), np.array([0, 8]), np.zeros(1, np.int64), np.array([0]), 0)
    rm2 = ref.RefModel(desc)
    rm2.init_synthetic(3)
    rm2.kv_alloc(512)
    a = ref.forward([rm2], st)
    b = F.ComposedOracle(rm, 512, linears=True).forward(st)
    assert not (a == b).all() and np.abs(a - b).max() < 0.1 * np.abs(a).max()


def test_composed_oracle_int8_kv_without_quantisation_is_ref_forward():
    """the int8-g8 KV variant of the composed oracle: with the fp8 linears off it is the oracle's own int8-KV forward, bit for bit"""
    desc = _tiny()
    d8 = F.kv_fp8.desc_with(desc, cache_quant_bit=8, cache_quant_group=8)
    rm, rm8 = ref.RefModel(desc), ref.RefModel(d8)
    rm.init_synthetic(3)
    rm8.init_synthetic(3)
    rm8.kv_alloc(512)
    orc = F.ComposedOracle(rm, 512, kv="int8", linears=False)
    rng = np.random.RandomState(4)
    tok = rng.randint(3, 512, size=30).astype(np.int64)
    ci = np.array([0, 256], dtype=np.int64)
    steps = [(tok, np.array([0, 21, 30]), np.zeros(2, np.int64), 0), (tok[[3, 8]], np.arange(3), np.array([21, 9], np.int64), 2)]
    for t, s, sp, nd in steps:
        st = ref.make_step(t, np.asarray(s, np.int64), sp, ci, nd)
        assert (orc.forward(st) == ref.forward([rm8], st)).all()


def test_abi_declares_and_exports_the_fp8_entry_points():
    m = load_pplhip()
    lib = ctypes.CDLL(m.LIB_PATH)
    for s in ("pplhip_op_quant_act_f8", "pplhip_op_rmsnorm_quant_f8", "pplhip_op_quant_weight_f8", "pplhip_op_linear_f8"):
        assert s in m.SYMBOLS and hasattr(lib, s), s
    # 1.2: the version an existing test pins; online_f8f8 is detected by its symbols and by pplhip_init accepting 0x108 (pplhip.h)
    assert lib.pplhip_version() == (1 << 16) | 2
    assert (m.ACT_QUANT_I8, m.ACT_QUANT_FP8) == (F.ACT_QUANT_I8, F.ACT_QUANT_FP8) == (8, 0x108)
    text = open(os.path.join(ROOT, "include", "pplhip.h")).read()
    assert "#define PPLHIP_ACT_QUANT_I8 8" in text and "#define PPLHIP_ACT_QUANT_FP8 0x108" in text
