"""The fp8 KV cache's test-side specification (tests/kv_fp8.py) on the CPU: the quantiser's edge cases, the composed oracle against
ref.forward with the quantisation switched off, and the exporter's --kv-cache fp8."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref
from tests import kv_fp8 as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _e4m3_table():
    """value of every finite e4m3fn code (0x7f / 0xff are NaN)"""
    v = []
    for c in range(256):
        s, ex, mt = c >> 7, (c >> 3) & 15, c & 7
        if ex == 15 and mt == 7:
            v.append(np.nan)
            continue
        mag = (mt / 8.0) * 2.0 ** -6 if ex == 0 else (1 + mt / 8.0) * 2.0 ** (ex - 7)
        v.append(-mag if s else mag)
    return np.array(v)


def _rne_reference(y):
    """nearest finite e4m3 code by brute force, ties to the even code"""
    tab = _e4m3_table()
    out = np.empty(y.shape, dtype=np.uint8)
    for i, x in np.ndenumerate(y):
        d = np.abs(tab - x)
        d[np.isnan(d)] = np.inf
        best = np.flatnonzero(d == d.min())
        if len(best) > 1:
            best = [b for b in best if (b & 1) == 0] or best
        c = int(best[0])
        if x == 0:
            c = 0x80 if np.signbit(x) else 0
        out[i] = c
    return out


def test_quantiser_matches_brute_force_rne():
    rng = np.random.RandomState(0)
    rows = (rng.randn(64, 128) * np.exp(3 * rng.randn(64, 1))).astype(np.float16)
    q, e = F.quantize_rows(rows)
    y = rows.astype(np.float64) * np.ldexp(1.0, -e)[:, None]
    y = np.clip(y, -np.where(e == 8, 240, 448)[:, None], np.where(e == 8, 240, 448)[:, None])
    assert (q == _rne_reference(y)).all()


def test_quantiser_edges():
    D = 64
    # amax = 0: e = -15, all codes zero, dequantised zero
    q, e = F.quantize_rows(np.zeros((1, D), np.float16))
    assert e[0] == -15 and (q == 0).all() and (F.dequantize(q, e) == 0).all()
    # amax exactly 448 * 2^k: e = k (the row max is code 0x7e); one fp16 ulp above: e = k + 1
    for k in (-10, -3, 0, 4, 7):
        r = np.zeros((1, D), np.float16)
        r[0, 5] = np.float16(448 * 2.0 ** k)
        q, e = F.quantize_rows(r)
        assert e[0] == k and q[0, 5] == 0x7e
        r[0, 5] = np.nextafter(np.float16(448 * 2.0 ** k), np.float16(np.inf))
        q, e = F.quantize_rows(r)
        assert e[0] == k + 1
    # fp8 subnormals: values far below the row max keep their subnormal codes
    r = np.zeros((1, D), np.float16)
    r[0, 0] = 448.0
    r[0, 1:9] = (np.arange(1, 9) * 2.0 ** -9).astype(np.float16)
    q, e = F.quantize_rows(r)
    assert e[0] == 0 and list(q[0, 1:9]) == list(range(1, 9))
    # e = 8 saturation at 240: the dequantised value stays finite in fp16
    r = np.zeros((1, D), np.float16)
    r[0, 0], r[0, 1] = 65504.0, -60000.0
    q, e = F.quantize_rows(r)
    assert e[0] == 8
    dq = F.dequantize(q, e)
    assert np.isfinite(dq.astype(np.float32)).all() and float(dq[0, 0]) == 240 * 256 and float(dq[0, 1]) == -240 * 256
    # tiny rows: e clamps at -15, results still exact fp16 (subnormals included)
    r = (np.random.RandomState(1).randn(4, D) * 1e-6).astype(np.float16)
    q, e = F.quantize_rows(r)
    assert (e == -15).all()
    F.dequantize(q, e)


def test_dequantised_values_are_exact_fp16_and_idempotent():
    rng = np.random.RandomState(2)
    rows = (rng.randn(500, 32) * np.exp(4 * rng.randn(500, 1))).clip(-65504, 65504).astype(np.float16)
    q, e = F.quantize_rows(rows)
    assert ((e >= -15) & (e <= 8)).all()
    dq = F.dequantize(q, e)           # asserts q * 2^e is an fp16 number
    assert np.isfinite(dq.astype(np.float32)).all()
    assert (F.scale_of(e).astype(np.float32) == np.ldexp(1.0, e)).all() and (F.exp_of(F.scale_of(e)) == e).all()
    assert (F.qdq_rows(dq).view(np.uint16) == dq.view(np.uint16)).all()   # Q o deQ is idempotent
    err = np.abs(dq.astype(np.float32) - rows.astype(np.float32)).max(-1) / np.abs(rows.astype(np.float32)).max(-1)
    assert (err <= 2.0 ** -4 + 1e-6).all()   # 3 mantissa bits: half an ulp of the row max at most (saturated rows excluded above)


@pytest.mark.parametrize("H,Hkv,layout,mode", [(4, 4, 3, 0), (8, 2, 3, 1), (8, 2, 0, 0), (4, 4, 1, 1)])
def test_composed_oracle_without_quantisation_is_ref_forward(H, Hkv, layout, mode):
    """the composition itself, pinned: with Q switched off it equals ref.forward bit for bit over a cold prefill, decodes and a
    prefix-hit recompute, MHA and GQA, contiguous and paged"""
    desc = ref.make_desc(hidden_dim=H * 32, intermediate_dim=256, num_layers=2, num_heads=H, num_kv_heads=Hkv, vocab_size=512,
                         max_position=512, cache_layout=layout, cache_mode=mode, page_size=16 if mode else 0, weight_quant_bit=8)
    rm = ref.RefModel(desc)
    rm.init_synthetic(5)
    rm.kv_alloc(512)
    orc = F.ComposedOracle(rm, 512, quant=False)
    rng = np.random.RandomState(3)
    if mode == 0:
        ci, maxp = np.array([0, 200, 400], dtype=np.int64), 0
    else:
        maxp = 8
        ci = rng.permutation(3 * maxp).astype(np.int64).reshape(3, maxp)
    steps = [([7, 20, 3], [0, 0, 0], 0), ([1, 1, 1], [7, 20, 3], 3), ([1, 1, 4], [8, 21, 1], 2)]
    for lens, sp, nd in steps:
        tok = rng.randint(3, 512, size=sum(lens)).astype(np.int64)
        ss = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        want = ref.forward([rm], ref.make_step(tok, ss, np.array(sp, np.int64), ci, nd, max_pages=maxp))
        got = orc.forward(ref.make_step(tok, ss, np.array(sp, np.int64), ci, nd, max_pages=maxp))
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (orc.kv.view(np.uint16) == rm.kv_array(0).view(np.uint16)).all()


def test_composed_oracle_with_quantisation_reads_fp8_rows():
    """with Q on, the slab holds only rows an fp8 cache can hold, and the logits move off the fp16-KV forward by a little"""
    desc = ref.make_desc(hidden_dim=128, intermediate_dim=256, num_layers=2, num_heads=4, num_kv_heads=2, vocab_size=512,
                         max_position=512, weight_quant_bit=8)
    rm = ref.RefModel(desc)
    rm.init_synthetic(5)
    rm.kv_alloc(256)
    orc = F.ComposedOracle(rm, 256)
    tok = np.random.RandomState(4).randint(3, 512, size=30).astype(np.int64)
    st = (tok, np.array([0, 30], np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64), 0)
    want = ref.forward([rm], ref.make_step(*st))
    got = orc.forward(ref.make_step(*st))
    assert (F.qdq_rows(orc.kv.reshape(-1, 32)).view(np.uint16) == orc.kv.reshape(-1, 32).view(np.uint16)).all()
    d = float(np.abs(got - want).max())
    assert 0 < d < 0.1 * float(np.abs(want).max())


def test_export_kv_cache_fp8_params(tmp_path):
    pytest.importorskip("torch")
    pytest.importorskip("transformers")
    spec = importlib.util.spec_from_file_location("export_hf_llama", os.path.join(ROOT, "ppl.llm.serving_amd", "tools", "export_hf_llama.py"))
    exp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(exp)
    from tests.test_export_hf import make_hf_checkpoint
    hf, _, _ = make_hf_checkpoint(tmp_path / "hf")
    for kv, want in (("fp8", (8, 64)), ("int8", (8, 8)), ("fp16", (0, 1))):
        out = tmp_path / kv
        r = subprocess.run([sys.executable, os.path.join(ROOT, "ppl.llm.serving_amd", "tools", "export_hf_llama.py"), "--model-dir", hf,
                            "--out", str(out), "--kv-cache", kv], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        p = json.load(open(out / "params.json"))
        assert (p["cache_quant_bit"], p["cache_quant_group"]) == want
    # --cache-quant-bit keeps working as it did
    r = subprocess.run([sys.executable, os.path.join(ROOT, "ppl.llm.serving_amd", "tools", "export_hf_llama.py"), "--model-dir", hf,
                        "--out", str(tmp_path / "cqb0"), "--cache-quant-bit", "0"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0
    p = json.load(open(tmp_path / "cqb0" / "params.json"))
    assert (p["cache_quant_bit"], p["cache_quant_group"]) == (0, 1)
