"""Sharp attention inputs on the device (tests/attn_sharp.py), all through pplhip_op_attention: F1 exact needles must come out as ONE
V row, bit for bit, on every kernel form (multi-head and grouped-query decode in both block forms with their reduce, the 16-row and
32-row prefill kernels, split-KV prefill) x fp16 / int8-g8 / fp8 / int4-g32 x contiguous / paged x the four slab layouts; F2 sharp but
unsaturated inputs against the oracle at the bars of tests/test_gpu_ops.py.  Every slot no request owns holds poison.
(int4 reaches the grouped-query kernel at head_dim 128 only; its groups 6 and 16 at head_dim 64 run the multi-head kernel.)"""
import ctypes as C

import numpy as np
import pytest

from tests import attn_sharp as A
from tests.conftest import load_pplhip
from tests.test_gpu_ops import ck, dev, _drop_device_tensors  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _run(m, c):
    """one pplhip_op_attention launch of case c; returns the fp16 output [T, H*D]"""
    dq = dev(c.qkv)
    dcache = dev(c.cache)
    dscale = dev(c.scale) if c.scale is not None else None
    v = c.view(m, dcache, dscale)
    n_ws = c.nb * c.H * c.split * (c.D + 2) if c.split > 1 else 0
    if getattr(c, "ws", False):
        n_ws = max(n_ws, (c.T - c.nb) * c.H * 32 * (c.D + 2))
    ws = torch.zeros(n_ws + 16, dtype=torch.float32, device="cuda") if n_ws else None
    out = torch.zeros((c.T, c.H * c.D), dtype=torch.float16, device="cuda")
    ck(m.lib().pplhip_op_attention(None, dq.data_ptr(), C.byref(v), dev(c.seq_starts).data_ptr(), dev(c.start_pos).data_ptr(),
                                   dev(c.cache_idx).data_ptr(), c.max_pages, c.B, c.T, c.nb, c.max_seq_len, c.max_kv_len, c.H,
                                   c.split, ws.data_ptr() if ws is not None else None, n_ws * 4, out.data_ptr()))
    if getattr(c, "ws", False) and c.p32_split > 1:   # (workspace cases run their decode rows unsplit: A.make)
        n_part = (c.T - c.nb) * c.H * c.p32_split * (c.D + 2)
        assert float(ws[:n_part].abs().max()) > 0, "the split-KV path did not run"
    return out.cpu().numpy()


def _f1(spec):
    m = load_pplhip()
    c = A.make(spec)
    want, top = A.expect_gather(c)
    got = _run(m, c)
    assert (got.view(np.uint16) == want.view(np.uint16)).all(), A.explain_mismatch(c, got, want, top)


@pytest.mark.parametrize("spec", A.f1_decode_specs(), ids=lambda s: s["name"])
def test_f1_decode(spec):
    """decode rows up to 8192 keys: splits 1 / 3 / 8 (2 in the small-block grouped-query form), every layout, pages of 16 and 64, and the
    addressing branches behind pages of 2, 8 and 12"""
    _f1(spec)


@pytest.mark.parametrize("spec", A.f1_prefill_specs(), ids=lambda s: s["name"])
def test_f1_prefill(spec):
    """prefill and cache-prefill rows: needles on the diagonal, probes one key past it, tile / page / split edges, pages of 5 and 12"""
    _f1(spec)


def test_f1_config4_launch_shape():
    """config 4's decode launch: 256 requests x 8 query heads per KV head x 2000 keys, int8, pages of 16"""
    _f1(A.F1_CONFIG4)


def test_f1_config4_i4_launch_shape():
    """config 4's decode launch on the int4 cache: 256 requests x 8 query heads per KV head x 2000 keys, pages of 16"""
    spec = A.F1_CONFIG4_I4
    assert (spec["fmt"], spec["H"], spec["Hkv"], spec["D"], spec["nb"], spec["page_size"]) == ("i4", 8, 1, 128, 256, 16)
    assert set(spec["start_pos"]) == {1999}
    _f1(spec)


def test_f1_config2_launch_shape():
    """config 2's decode launch: 1024 requests x 32 heads x kv 512-537, int8, pages of 16 shuffled over a slab whose V half starts
    past 2^31 elements"""
    spec = A.F1_CONFIG2
    assert max(spec["start_pos"]) + 1 <= 537 and spec["H"] == spec["Hkv"] == 32
    m = load_pplhip()
    c = A.make(spec)
    assert c.N * c.Hkv * c.D > 2 ** 31
    want, top = A.expect_gather(c)
    got = _run(m, c)
    assert (got.view(np.uint16) == want.view(np.uint16)).all(), A.explain_mismatch(c, got, want, top)


@pytest.mark.parametrize("i", range(len(A.F2_SPECS)), ids=lambda i: A.F2_SPECS[i][1]["name"])
def test_f2_against_oracle(i):
    """sharp but unsaturated: competing keys, a sink over a long tail, a maximum rising on every tile -- at the existing bars
    (int4 too: its operands are exact fp16 numbers, so it is held to the fp16 bars)"""
    m = load_pplhip()
    family, spec = A.F2_SPECS[i]
    c = A.make(spec, family)
    want = c.oracle()
    got = _run(m, c).astype(np.float32)
    assert np.isfinite(got).all()
    bar = A.bar_of(c, want.astype(np.float64))
    err = np.abs(got - want)
    assert (err <= bar).all(), (float((err / bar).max()), int((err > bar).sum()))
