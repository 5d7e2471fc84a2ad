"""Sharp inputs through pplhip_op_attention_shared (own launch on the shifted page table + attn_decode_shared_kernel + merge), with a
workspace of exactly pplhip_op_attention_shared_workspace_bytes: F1 exact needles must come out as ONE V row, bit for bit -- winners in
the shared part with a weaker needle of the same direction in the row's own part, and the other way round, on every edge of the shared
splits, wave strides and register buffers and of the own chunks; F2 sharp but unsaturated inputs against the C oracle (ordinary page
table) at the decode bar of tests/test_gpu_ops.py.  Every slot no request owns holds poison.  The cases and what they cover are
specified on the CPU by tests/test_attn_shared_sharp_spec.py."""
import ctypes as C

import numpy as np
import pytest

from tests import attn_sharp as A
from tests.conftest import load_pplhip
from tests.test_gpu_attn_sharp import _run as run_ordinary
from tests.test_gpu_ops import dev, _drop_device_tensors  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F1_SPECS = A.f1_shared_specs()


def _run(m, c):
    """one pplhip_op_attention_shared call on case c; returns the fp16 output [B, H*D]"""
    dq, dcache, dseq = dev(c.qkv), dev(c.cache), dev(c.seq_starts)
    dscale = dev(c.scale) if c.scale is not None else None
    v = c.view(m, dcache, dscale)
    need = m.lib().pplhip_op_attention_shared_workspace_bytes(c.B, c.H, c.D, c.max_pages, c.own_split, c.shared_split)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.zeros((c.B, c.H * c.D), dtype=torch.float16, device="cuda")
    sp, pages = np.ascontiguousarray(c.start_pos), np.ascontiguousarray(c.cache_idx)
    group, tokens = np.ascontiguousarray(c.group, dtype=np.int32), np.ascontiguousarray(c.group_tokens, dtype=np.int64)
    rc = m.lib().pplhip_op_attention_shared(None, dq.data_ptr(), C.byref(v), dseq.data_ptr(), sp.ctypes.data, pages.ctypes.data, c.max_pages,
                                            c.B, c.H, group.ctypes.data, tokens.ctypes.data, len(tokens), c.own_split, c.shared_split,
                                            ws.data_ptr(), ws.numel(), out.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out.cpu().numpy()


@pytest.mark.parametrize("i", range(len(F1_SPECS)), ids=lambda i: F1_SPECS[i]["name"])
def test_f1_shared(i):
    """the operator's fp16 output equals the gathered V row, bit for bit; on every third spec the ordinary operator on the same slab
    and the ordinary page table gives the identical bits"""
    m = load_pplhip()
    c = A.make_shared(F1_SPECS[i])
    want, top = A.expect_gather(c)
    got = _run(m, c)
    assert (got.view(np.uint16) == want.view(np.uint16)).all(), A.explain_mismatch(c, got, want, top)
    if i % 3 == 0:
        plain = run_ordinary(m, c)
        assert (plain.view(np.uint16) == got.view(np.uint16)).all(), A.explain_mismatch(c, plain, want, top)


@pytest.mark.parametrize("i", range(len(A.F2_SHARED_SPECS)), ids=lambda i: A.F2_SHARED_SPECS[i][2]["name"])
def test_f2_shared_against_oracle(i):
    """competing keys, a sink, a maximum rising on every tile -- with the mass in the shared part, in the own part and on both sides of
    P -- at the existing decode bar, 1.5e-3 + 1.5e-3 |ref|"""
    m = load_pplhip()
    family, where, spec = A.F2_SHARED_SPECS[i]
    c = A.make_shared(spec, family, where)
    want = c.oracle()
    got = _run(m, c).astype(np.float32)
    assert np.isfinite(got).all()
    bar = A.bar_of(c, want.astype(np.float64))
    err = np.abs(got - want)
    print(f"{spec['name']}: max err / bar {float((err / bar).max()):.3f}")
    assert (err <= bar).all(), (float((err / bar).max()), int((err > bar).sum()))
