"""Shared-prefix decode attention (pplhip_op_attention_shared: own part + attn_decode_shared_kernel + merge) against a float64 numpy
reference: dequantise the cache, softmax(q K^T / sqrt(D)) V per row and head.  Bound: test_attention_decode's (tests/test_gpu_ops.py).
Pages of 16 in every case, and the same rows on pages of 32, 48 and 64 (test_attention_shared_page_sizes).  Exact needles and sharp
softmax inputs on this path: tests/test_gpu_attn_shared_sharp.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PS = 16
# 24 decode rows: group A 19 rows x 48 shared tokens (3 sub-tiles: fewer than a block has waves; grp 1: a short second tile, grp 4: five
# tiles, the last with three requests), group B 2 rows x 272 (17 sub-tiles: odd, more than the waves, uneven over 3 splits), 3 loose rows
KIND = ["L" if b in (2, 8, 17) else ("B" if b in (4, 12) else "A") for b in range(24)]
OWN = {"A": [1, 15, 16, 17, 130, 33, 2], "B": [17, 1], "L": [1, 50, 300]}   # keys of a row's own (loose rows: all its keys)
SHARED = {"A": 48, "B": 272, "L": 0}
# shared tokens of groups A and B on the other page sizes (multiples of the page; B keeps an odd number of sub-tiles or of pages)
SHARED_OF = {16: SHARED, 32: {"A": 64, "B": 288, "L": 0}, 48: {"A": 48, "B": 240, "L": 0}, 64: {"A": 64, "B": 320, "L": 0}}


class Case:
    def __init__(self, H, Hkv, D, quant, layout, dominant=None, PS=PS):
        rng = np.random.RandomState(H * 7 + D + quant + layout)
        self.H, self.Hkv, self.D, self.quant, self.layout, self.PS = H, Hkv, D, quant, layout, PS
        SHARED = SHARED_OF[PS]
        seen = {"A": 0, "B": 0, "L": 0}
        own = []
        for k in KIND:
            own.append(OWN[k][seen[k] % len(OWN[k])])
            seen[k] += 1
        self.P = np.array([SHARED[k] for k in KIND], dtype=np.int64)
        self.kv_len = self.P + np.array(own)
        self.start_pos = (self.kv_len - 1).astype(np.int64)
        self.B = len(KIND)
        npg = (self.kv_len + PS - 1) // PS
        self.max_pages = int(npg.max())
        own_pg = npg - self.P // PS
        n_sh = {k: SHARED[k] // PS for k in "AB"}   # (pages of 16: 3 and 17)
        free = list(rng.permutation(int(own_pg.sum()) + n_sh["A"] + n_sh["B"] + 4))
        shared_pages = {"A": [free.pop() for _ in range(n_sh["A"])], "B": [free.pop() for _ in range(n_sh["B"])], "L": []}   # written once, every member points at them
        self.pages = np.full((self.B, self.max_pages), np.iinfo(np.int64).max, dtype=np.int64)
        for b, k in enumerate(KIND):
            self.pages[b, :npg[b]] = shared_pages[k] + [free.pop() for _ in range(own_pg[b])]
        self.group = np.array([{"A": 0, "B": 1, "L": -1}[k] for k in KIND], dtype=np.int32)
        self.group_tokens = np.array([SHARED["A"], SHARED["B"]], dtype=np.int64)
        self.N = (len(free) + int(own_pg.sum()) + 20) * PS
        # the slab of 2 layers as [layer, k/v, (slot, head | head, slot), channel]; layer 1 is used
        shape = (2, 2, self.N, Hkv, D) if layout == 2 else (2, 2, Hkv, self.N, D)
        if quant:
            self.cache = rng.randint(-127, 128, size=shape).astype(np.int8)
            self.scale = (0.02 * (0.5 + rng.rand(*shape[:-1], D // 8))).astype(np.float16)
        else:
            self.cache = rng.randn(*shape).astype(np.float16)
            self.scale = None
        q = rng.randn(self.B, H + 2 * Hkv, D)
        if dominant:   # |q| . |k| x 30 on one part's keys: its scores lead the other part's by > 100 nats
            q = np.abs(q)
            is_shared = np.zeros(self.N, dtype=bool)
            for k in "AB":
                for pg in shared_pages[k]:
                    is_shared[pg * PS:(pg + 1) * PS] = True
            rows = is_shared if dominant == "shared" else ~is_shared
            sl = (1, 0, rows) if layout == 2 else (1, 0, slice(None), rows)
            self.cache[sl] = np.abs(self.cache[sl])
            if quant:
                self.scale[sl] = (self.scale[sl].astype(np.float32) * 30).astype(np.float16)
            else:
                self.cache[sl] = (self.cache[sl].astype(np.float32) * 30).astype(np.float16)
        self.qkv = q.astype(np.float16).reshape(self.B, -1)
        self.want, self.margin = self.reference(dominant)

    def reference(self, dominant):
        PS = self.PS
        kv = self.cache[1].astype(np.float64)
        if self.quant:
            kv = kv * np.repeat(self.scale[1].astype(np.float64), 8, axis=-1)
        if self.layout == 2:
            kv = kv.transpose(0, 2, 1, 3)   # -> [k/v, head, slot, channel]
        q = self.qkv.astype(np.float64).reshape(self.B, -1, self.D)[:, :self.H]
        grp = self.H // self.Hkv
        want = np.empty((self.B, self.Hkv, grp, self.D))
        margin = np.inf
        for b in range(self.B):
            pos = np.arange(self.kv_len[b])
            slots = self.pages[b, pos // PS] * PS + pos % PS
            for hk in range(self.Hkv):
                s = q[b, hk * grp:(hk + 1) * grp] @ kv[0, hk, slots].T / np.sqrt(self.D)   # [grp, kv_len]
                p = np.exp(s - s.max(axis=1, keepdims=True))
                want[b, hk] = (p / p.sum(axis=1, keepdims=True)) @ kv[1, hk, slots]
                if dominant and self.P[b]:
                    sh, ow = s[:, :self.P[b]].max(axis=1), s[:, self.P[b]:].max(axis=1)
                    margin = min(margin, float(((sh - ow) if dominant == "shared" else (ow - sh)).min()))
        return want.reshape(self.B, -1), margin

    def run(self, m, shared_split, own_split=2, ws_short=0, group_tokens=None, start_pos=None, quant_group=None, out=None):
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dq, dcache, dseq = dev(self.qkv), dev(self.cache), dev(np.arange(self.B + 1, dtype=np.int64))
        dscale = dev(self.scale) if self.quant else None
        v = m.KvView()
        v.cache, v.scale = dcache.data_ptr(), (dscale.data_ptr() if self.quant else None)
        v.max_tokens, v.num_layers, v.kv_heads, v.head_dim = self.N, 2, self.Hkv, self.D
        v.quant_bit, v.quant_group = self.quant, (quant_group or (8 if self.quant else 1))
        v.layout, v.mode, v.page_size, v.layer = self.layout, 1, self.PS, 1
        need = m.lib().pplhip_op_attention_shared_workspace_bytes(self.B, self.H, self.D, self.max_pages, own_split, shared_split)
        ws = torch.empty(need - ws_short, dtype=torch.uint8, device="cuda")
        out = torch.zeros((self.B, self.H * self.D), dtype=torch.float16, device="cuda") if out is None else out
        gt = self.group_tokens if group_tokens is None else np.asarray(group_tokens, dtype=np.int64)
        sp = self.start_pos if start_pos is None else np.asarray(start_pos, dtype=np.int64)
        rc = m.lib().pplhip_op_attention_shared(None, dq.data_ptr(), C.byref(v), dseq.data_ptr(), sp.ctypes.data, self.pages.ctypes.data,
                                                self.max_pages, self.B, self.H, self.group.ctypes.data, gt.ctypes.data, 2, own_split, shared_split,
                                                ws.data_ptr(), ws.numel(), out.data_ptr())
        torch.cuda.synchronize()
        return rc, out.cpu().numpy().astype(np.float64)


def check(got, want):
    err, tol = np.abs(got - want), 1.5e-3 + 1.5e-3 * np.abs(want)
    assert (err <= tol).all(), (err.max(), np.abs(want).max(), int((err > tol).sum()))


@functools.lru_cache(maxsize=None)
def shape_case(H, Hkv, D, quant, layout, PS=PS):
    """one case (and its reference) per shape, shared by the two splits"""
    return Case(H, Hkv, D, quant, layout, PS=PS)


@pytest.mark.parametrize("shared_split", [1, 3])
@pytest.mark.parametrize("quant", [0, 8])
@pytest.mark.parametrize("layout", [2, 3])
@pytest.mark.parametrize("H,Hkv,D", [(4, 4, 128), (8, 2, 64), (16, 1, 128), (12, 2, 128)])   # head groups 1, 4, 16, 6 (four padding columns)
def test_attention_shared(quant, layout, H, Hkv, D, shared_split):
    m = load_pplhip()
    case = shape_case(H, Hkv, D, quant, layout)
    rc, got = case.run(m, shared_split)
    assert rc == 0, rc
    check(got, case.want)


@pytest.mark.parametrize("shared_split", [1, 3])
@pytest.mark.parametrize("quant", [0, 8])
@pytest.mark.parametrize("page_size,layout,H,Hkv,D", [(ps, 2 + (k + j) % 2, *shape) for k, ps in enumerate((32, 48, 64)) for j, shape in
                                                      enumerate([(4, 4, 128), (8, 2, 64), (16, 1, 128), (12, 2, 128)])])
def test_attention_shared_page_sizes(page_size, layout, H, Hkv, D, quant, shared_split):
    """the same rows, shapes, splits and bound on pages of 32, 48 (no shift: the division path) and 64"""
    m = load_pplhip()
    case = shape_case(H, Hkv, D, quant, layout, page_size)
    rc, got = case.run(m, shared_split)
    assert rc == 0, rc
    check(got, case.want)


@pytest.mark.parametrize("quant", [0, 8])
@pytest.mark.parametrize("dominant", ["shared", "own"])
def test_attention_shared_one_part_dominates(dominant, quant):
    """one part's scores lead by > 100 nats: the other part's weight underflows to zero in the merge, the result is the leader's"""
    m = load_pplhip()
    case = Case(8, 2, 128, quant, 3, dominant=dominant)
    assert case.margin > 100, case.margin
    rc, got = case.run(m, 3)
    assert rc == 0, rc
    check(got, case.want)


def test_attention_shared_argument_checks():
    """refused before any launch: `out` keeps its sentinel"""
    m = load_pplhip()
    case = Case(4, 4, 128, 8, 3)
    short_row = case.start_pos.copy()
    short_row[4] = 271   # a member of group B with P = 272 > start_pos
    for want_rc, kw in [(-2, dict(group_tokens=[40, 272])), (-2, dict(start_pos=short_row)), (-2, dict(ws_short=1)), (-7, dict(quant_group=128))]:   # (8, head_dim): the fp8 cache, not built
        out = torch.full((case.B, case.H * case.D), 7.0, dtype=torch.float16, device="cuda")
        rc, got = case.run(m, 2, out=out, **kw)
        assert rc == want_rc, (rc, kw)
        assert (got == 7.0).all(), kw
