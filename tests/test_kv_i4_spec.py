"""The int4 KV cache's test-side specification (tests/kv_i4.py) on the CPU: the scale rule over every finite fp16 group maximum, the
nibble packing, idempotence of Q, the composed oracle against ref.forward with the quantisation switched off, and the exporter's
--kv-cache int4."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref
from tests import kv_i4 as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_amax():
    """every non-negative finite fp16 value (31 744 of them)"""
    a = np.arange(0x7c00, dtype=np.uint16).view(np.float16)
    assert len(a) == 31744 and np.isfinite(a.astype(np.float32)).all()
    return a


def test_scale_rule_over_every_fp16_amax():
    amax = _all_amax().astype(np.float32)
    s = I.scale_of_amax(amax)
    s16 = s.astype(np.float16)
    assert (s16.astype(np.float32) == s).all(), "the scale is not an fp16 number"
    assert (s16.view(np.uint16) & 7 == 0).all(), "low three mantissa bits of the scale"
    assert s.min() == 2.0 ** -14 and s.max() == 9344.0
    for q in range(1, 8):
        p = (np.float32(q) * s).astype(np.float32)
        assert (p.astype(np.float64) == q * s.astype(np.float64)).all()                    # exact in fp32
        ph = p.astype(np.float16)
        assert np.isfinite(ph.astype(np.float32)).all() and (ph.astype(np.float32) == p).all(), q   # and exactly a finite fp16 number
        assert (np.abs(p) >= 2.0 ** -14).all()                                             # normal
    # the scale never falls below amax / 7 except at the cap, so amax itself codes to +-7 from 7 * 2^-14 on
    big = amax >= 7 * 2.0 ** -14
    inv = (np.float32(1.0) / s).astype(np.float32)
    qa = np.clip(np.rint((amax * inv).astype(np.float32)), -7, 7)
    assert (qa[big] == 7).all()
    rows = np.zeros((len(amax), 32), np.float16)
    rows[:, 3] = _all_amax()
    rows[:, 17] = -_all_amax()
    q, s2 = I.quantize_groups(rows)
    assert (s2[:, 0].view(np.uint16) == s16.view(np.uint16)).all()
    assert (q[big, 3] == 7).all() and (q[big, 17] == -7).all()
    I.dequantize(q, s2)   # asserts q * s is an fp16 number


def test_nibble_packing_round_trip():
    rng = np.random.RandomState(0)
    q = rng.randint(-7, 8, size=(50, 128)).astype(np.int8)
    b = I.pack_nibbles(q)
    assert b.shape == (50, 64) and b.dtype == np.uint8
    assert (b & 15 != 0).all() and (b >> 4 != 0).all()           # nibble 0 is never written
    qi = q.astype(np.int32)
    assert (b[:, 0] == (qi[:, 0] + 8) | ((qi[:, 1] + 8) << 4)).all()   # channel 2j low, 2j + 1 high
    assert (I.unpack_nibbles(b) == q).all()
    rows = (rng.randn(20, 64) * 3).astype(np.float16)
    c, s = I.slab_to_i4(rows.reshape(-1), 64)
    assert c.dtype == np.int8 and c.size == rows.size // 2 and s.size == rows.size // 32
    assert (I.i4_to_slab(c, s, 64).view(np.uint16) == I.qdq_rows(rows).reshape(-1).view(np.uint16)).all()


def test_q_is_idempotent():
    rng = np.random.RandomState(2)
    rows = (rng.randn(600, 128) * np.exp(4 * rng.randn(600, 1))).clip(-65504, 65504).astype(np.float16)
    rows[0] = 65504
    rows[1] = -65504
    rows[2, ::2] = 65504
    rows[2, 1::2] = -65504
    rows[3] = (rng.randn(128) * 1e-5).astype(np.float16)
    rows[4] = (rows[5].astype(np.float32) * 1e-5).astype(np.float16)
    rows[6] = 0
    rows[7, :32] = 0
    dq = I.qdq_rows(rows)
    assert np.isfinite(dq.astype(np.float32)).all()
    assert (I.qdq_rows(dq).view(np.uint16) == dq.view(np.uint16)).all()
    q, s = I.quantize_groups(dq)
    q0, s0 = I.quantize_groups(rows)
    assert (q == q0).all()
    assert (s0[0] == 9344).all() and (s0[3] == 2.0 ** -14).all() and (s0[6] == 2.0 ** -14).all() and (q0[6] == 0).all()
    # 4 bits: half a step of the group's scale, the scale at most 1 / 128 above amax / 7 (groups at the cap or the floor excluded)
    g = rows.astype(np.float32).reshape(600, 4, 32)
    err = np.abs(dq.astype(np.float32).reshape(600, 4, 32) - g).max(-1)
    s32 = s0.astype(np.float32)
    free = (s32 > 2.0 ** -14) & (s32 < 9344)
    assert (err[free] <= 0.5 * s32[free] * (1 + 1e-6)).all()
    assert (s32[free] <= np.abs(g).max(-1)[free] / 7 * (1 + 2.0 ** -7) * (1 + 1e-6)).all()


@pytest.mark.parametrize("H,Hkv,layout,mode", [(4, 4, 3, 0), (8, 2, 3, 1), (8, 2, 0, 0), (4, 4, 1, 1)])
def test_composed_oracle_without_quantisation_is_ref_forward(H, Hkv, layout, mode):
    """the composition itself, pinned: with Q switched off it equals ref.forward bit for bit over a cold prefill, decodes and a
    prefix-hit recompute, MHA and GQA, contiguous and paged"""
    desc = ref.make_desc(hidden_dim=H * 32, intermediate_dim=256, num_layers=2, num_heads=H, num_kv_heads=Hkv, vocab_size=512,
                         max_position=512, cache_layout=layout, cache_mode=mode, page_size=16 if mode else 0, weight_quant_bit=8)
    rm = ref.RefModel(desc)
    rm.init_synthetic(5)
    rm.kv_alloc(512)
    orc = I.ComposedOracle(rm, 512, quant=False)
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


def test_composed_oracle_with_quantisation_reads_int4_rows():
    """with Q on, the slab holds only rows an int4 cache can hold, and the logits move off the fp16-KV forward (4 bits: by more than fp8)"""
    desc = ref.make_desc(hidden_dim=128, intermediate_dim=256, num_layers=2, num_heads=4, num_kv_heads=2, vocab_size=512,
                         max_position=512, weight_quant_bit=8)
    rm = ref.RefModel(desc)
    rm.init_synthetic(5)
    rm.kv_alloc(256)
    orc = I.ComposedOracle(rm, 256)
    tok = np.random.RandomState(4).randint(3, 512, size=30).astype(np.int64)
    st = (tok, np.array([0, 30], np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64), 0)
    want = ref.forward([rm], ref.make_step(*st))
    got = orc.forward(ref.make_step(*st))
    assert (I.qdq_rows(orc.kv.reshape(-1, 32)).view(np.uint16) == orc.kv.reshape(-1, 32).view(np.uint16)).all()
    c, s = I.slab_to_i4(orc.kv, 32)
    assert (I.i4_to_slab(c, s, 32).view(np.uint16) == orc.kv.view(np.uint16)).all()
    d = float(np.abs(got - want).max())
    assert 0 < d < 0.5 * float(np.abs(want).max())


def test_export_kv_cache_int4_params(tmp_path):
    pytest.importorskip("torch")
    pytest.importorskip("transformers")
    spec = importlib.util.spec_from_file_location("export_hf_llama", os.path.join(ROOT, "ppl.llm.serving_amd", "tools", "export_hf_llama.py"))
    exp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(exp)
    from tests.test_export_hf import make_hf_checkpoint
    hf, _, _ = make_hf_checkpoint(tmp_path / "hf")
    out = tmp_path / "int4"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "ppl.llm.serving_amd", "tools", "export_hf_llama.py"), "--model-dir", hf,
                        "--out", str(out), "--kv-cache", "int4"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    p = json.load(open(out / "params.json"))
    assert (p["cache_quant_bit"], p["cache_quant_group"]) == (4, 32)
