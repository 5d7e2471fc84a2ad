"""Mixture-of-experts block as operators (csrc/k_moe.hip): pplhip_op_moe_route and pplhip_op_moe_ffn against a float64 restatement of
DESIGN.md "numerics" (mixture of experts), and against the dense operators composed per expert."""
import numpy as np
import pytest

from tests.conftest import load_pplhip
from tests.test_gpu_ops import ck, close_f16, dev, f16, _drop_device_tensors  # noqa: F401  (the fixture frees what dev() keeps)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (T, E, k, hidden, inter, biased gate); T "lo" / "hi": either side of the short / tall tile threshold pplhip_op_moe_tile_rows reports
# (tied logits, k = 1, the bucket kernel's second and third pass, hidden 64 / 192 / 320, row counts on a tile boundary and stale workspace
# state are in tests/test_gpu_moe_exact.py, bit for bit on the exactly summable operands of tests/moe_exact.py)
SHAPES = [(1, 8, 2, 128, 64, False), (5, 4, 4, 128, 160, False), (37, 8, 2, 256, 192, False), (200, 4, 2, 128, 64, True),
          (64, 64, 8, 128, 64, False), ("lo", 8, 2, 128, 64, False), ("hi", 8, 2, 128, 64, False)]


def threshold_T(m, E, k):
    rows = [m.lib().pplhip_op_moe_tile_rows(T, k, E) for T in range(1, 2049)]
    assert rows[0] <= 32 and rows[-1] == 128 and rows == sorted(rows)
    return rows.index(128)   # the largest T on short tiles (rows[i] belongs to T = i + 1)


def build(T, E, k, hidden, inter, wq, biased):
    """inputs and the float64 reference: ids / weights [T, k], y [T, hidden] behind the two fp16 roundings (h, output)"""
    rng = np.random.RandomState(T * 7 + E * 3 + k + wq)
    gate = f16(rng.randn(E, hidden) * 0.1)
    draw = lambda n: rng.randn(n, hidden) * 0.5 + (1.0 if biased else 0.0)
    if biased:   # every row's mean pulls expert 0 up and the last expert down
        gate[0] = f16(gate[0] + 0.05)
        gate[E - 1] = f16(gate[E - 1] - 0.05)
    x = f16(draw(T))
    for t in range(T):   # exact routing: every gap down to the (k+1)-th logit clears 8 x the fp32 accumulation bound; redraw until it does
        while True:
            prod = x[t].astype(np.float64) * gate.astype(np.float64)
            top = np.sort(prod.sum(1))[::-1][:k + 1]
            if len(top) < 2 or (top[:-1] - top[1:]).min() >= 8 * hidden * 2.0 ** -24 * np.abs(prod).sum(1).max():
                break
            x[t] = f16(draw(1))[0]
    if wq == 8:
        q13, s13 = rng.randint(-127, 128, size=(E, 2 * inter, hidden)).astype(np.int8), f16(0.0008 * (0.5 + rng.rand(E, 2 * inter)))
        q2, s2 = rng.randint(-127, 128, size=(E, hidden, inter)).astype(np.int8), f16(0.0008 * (0.5 + rng.rand(E, hidden)))
        W13, W2 = q13 * s13.astype(np.float64)[..., None], q2 * s2.astype(np.float64)[..., None]
    else:
        q13, q2, s13, s2 = f16(rng.randn(E, 2 * inter, hidden) * 0.08), f16(rng.randn(E, hidden, inter) * 0.08), None, None
        W13, W2 = q13.astype(np.float64), q2.astype(np.float64)
    r = x.astype(np.float64) @ gate.astype(np.float64).T
    ids = np.argsort(-r, axis=1, kind="stable")[:, :k]   # ties to the lower expert
    sel = np.take_along_axis(r, ids, 1)
    p = np.exp(sel - sel[:, :1])
    p /= p.sum(1, keepdims=True)
    slots = np.zeros((T, k, hidden))
    for e in range(E):
        t, s = np.nonzero(ids == e)
        gu = (x[t].astype(np.float64) @ W13[e].T).astype(np.float16).astype(np.float64)   # container order: gate rows | up rows
        g, u = gu[:, :inter], gu[:, inter:]
        h = (g / (1.0 + np.exp(-g)) * u).astype(np.float16).astype(np.float64)
        slots[t, s] = p[t, s, None] * (h @ W2[e].T)
    perm = np.empty(2 * inter, dtype=np.int64)   # device layout: rows interleaved (gate_i, up_i); w2's K zero-padded to a multiple of 64
    perm[0::2], perm[1::2] = np.arange(inter), inter + np.arange(inter)
    q2p = np.zeros((E, hidden, (inter + 63) // 64 * 64), dtype=q2.dtype)
    q2p[:, :, :inter] = q2
    return dict(x=x, gate=gate, w13=q13[:, perm], s13=None if s13 is None else s13[:, perm], w2=q2p, s2=s2, ids=ids, p=p,
                want=slots.sum(1).astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("wq", [0, 8])
@pytest.mark.parametrize("T,E,k,hidden,inter,biased", SHAPES)
def test_moe_ffn(wq, T, E, k, hidden, inter, biased):
    m = load_pplhip()
    L = m.lib()
    if isinstance(T, str):
        T = threshold_T(m, E, k) + (T == "hi")
        assert L.pplhip_op_moe_tile_rows(T, k, E) == (128 if T > threshold_T(m, E, k) else 32)
    c = build(T, E, k, hidden, inter, wq, biased)
    inter_p = c["w2"].shape[2]
    ptr = lambda a: None if a is None else dev(a).data_ptr()
    dx, dg, dw13, ds13, dw2, ds2 = (ptr(c[n]) for n in ("x", "gate", "w13", "s13", "w2", "s2"))

    # routing: exact ids and slot order, counts = the histogram, weights to 1e-5
    ids = torch.full((T, k), -1, dtype=torch.int32, device="cuda")
    wts = torch.zeros((T, k), dtype=torch.float32, device="cuda")
    counts = torch.full((64,), 12345, dtype=torch.int32, device="cuda")
    ck(L.pplhip_op_moe_route(None, dx, dg, T, hidden, E, k, ids.data_ptr(), wts.data_ptr(), counts.data_ptr()))
    assert (ids.cpu().numpy() == c["ids"]).all()
    hist = np.bincount(c["ids"].ravel(), minlength=64)
    assert (counts.cpu().numpy() == hist).all()
    if biased:
        assert hist[0] > 128 and hist[E - 1] == 0   # two tall tiles of one expert, one of them ragged; an expert nobody chose
    np.testing.assert_allclose(wts.cpu().numpy(), c["p"], rtol=1e-5, atol=0)

    # the whole block: NaN workspace, canaries around y, twice the same bits
    ws_bytes = L.pplhip_op_moe_ffn_workspace_bytes(T, E, k, hidden, inter)
    ws = torch.full((ws_bytes // 4 + 1,), float("nan"), dtype=torch.float32, device="cuda")
    ldy = hidden + 8
    runs = []
    for _ in range(2):
        y = torch.full((T + 2, ldy), 777.0, dtype=torch.float16, device="cuda")
        ck(L.pplhip_op_moe_ffn(None, dx, dg, dw13, ds13, dw2, ds2, wq, T, E, k, hidden, inter, ws.data_ptr(), ws_bytes, y[1].data_ptr(), ldy))
        runs.append(y.cpu().numpy())
    got = runs[0]
    assert (runs[1].view(np.uint16) == got.view(np.uint16)).all()
    assert (got[0] == 777.0).all() and (got[-1] == 777.0).all() and (got[:, hidden:] == 777.0).all()
    got = got[1:-1, :hidden].astype(np.float32)

    # the dense composition: pplhip_op_linear_swiglu + pplhip_op_linear per expert on its rows, weighted and summed here in float64
    comp = np.zeros((T, k, hidden))
    for e in range(E):
        t, s = np.nonzero(c["ids"] == e)
        if len(t) == 0:
            continue
        M = len(t)
        h = torch.zeros((M, inter_p), dtype=torch.float16, device="cuda")
        hc = torch.empty((M, inter), dtype=torch.float16, device="cuda")
        ye = torch.empty((M, hidden), dtype=torch.float32, device="cuda")
        sc = lambda a: None if a is None else dev(a[e]).data_ptr()
        ck(L.pplhip_op_linear_swiglu(None, dev(c["x"][t]).data_ptr(), dev(c["w13"][e]).data_ptr(), sc(c["s13"]), wq, 128, M, 2 * inter, hidden, hc.data_ptr()))
        h[:, :inter] = hc
        ck(L.pplhip_op_linear(None, h.data_ptr(), dev(c["w2"][e]).data_ptr(), sc(c["s2"]), wq, 128, M, hidden, inter_p, ye.data_ptr(), 1))
        comp[t, s] = c["p"][t, s, None] * ye.cpu().numpy().astype(np.float64)
    comp = comp.sum(1).astype(np.float16).astype(np.float32)

    want = c["want"]
    rel = 3e-3   # test_linear_swiglu_fused's numbers: a product behind two fp16 roundings
    abs_ = rel * np.abs(want).max() * 0.05 + 1e-5
    comp_err = np.abs(comp - want)
    # the grouped kernels take the dense ones' operands and roundings; what may differ is the fp32 summation order and the routing weight
    # (fp32 here, float64 in the composition): 2^-24-relative terms of sums of at most inter products, below 2^-12 of the case's largest
    # output, and behind them the final rounding may fall one fp16 ulp apart
    ulp = np.spacing(np.abs(comp).astype(np.float16)).astype(np.float32)
    assert (np.abs(got - comp) <= ulp + 2.0 ** -12 * np.abs(comp).max()).all()
    widened = bool((comp_err > abs_ + rel * np.abs(want)).any())
    print(f"moe_ffn wq={wq} T={T} E={E} k={k}: max err {np.abs(got - want).max():.3e}, composition {comp_err.max():.3e}, abs term {abs_:.3e}, "
          f"composition breaks the bound: {widened}")
    if widened:   # the issue's rule: the case's bound becomes 1.5 x the composition's worst error (the cases: profiles/moe_ffn.md)
        abs_ = max(abs_, 1.5 * float(comp_err.max()))
    close_f16(got, want, rel=rel, abs_=abs_)
