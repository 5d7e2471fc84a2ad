"""pplhip_op_window_shift (csrc/rt_window.cc: the shifted positions, slots / page table and skips of sliding-window decode rows) against a
numpy restatement.  Host arrays only: no device."""
import numpy as np
import pytest

from tests.conftest import load_pplhip


def shift_ref(pos, table, mode, ps, W):
    """f = max(0, pos - W + 1); contiguous: slot + f; paged: the table from page f // ps on, as wide as the neediest row"""
    f = np.maximum(pos - W + 1, 0)
    base = f // ps * ps if mode == 1 else f
    npos, skip = pos - base, f - base
    if mode == 0:
        return npos, (table + f)[:, None], skip
    width = int((npos // ps + 1).max())
    first = base // ps
    out = np.array([[table[b, first[b] + j] if first[b] + j < table.shape[1] else 0 for j in range(width)] for b in range(len(pos))])
    return npos, out, skip


@pytest.mark.parametrize("W", [1, 16, 40, 64])
@pytest.mark.parametrize("ps", [16, 48])
@pytest.mark.parametrize("mode", [0, 1])
def test_window_shift(mode, ps, W):
    m = load_pplhip()
    pos = np.array([p for p in (W - 2, W - 1, W, W + 1, W + ps - 1, W + ps, 3 * W + 5) if p >= 0], dtype=np.int64)
    nb, mp = len(pos), int(pos.max()) // ps + 1
    rng = np.random.RandomState(W + ps + mode)
    table = rng.permutation(nb * mp).reshape(nb, mp).astype(np.int64) if mode == 1 else rng.randint(0, 1 << 20, size=nb).astype(np.int64)
    rc, gpos, gtab, gskip, max_kv = m.window_shift(pos, table, mode, ps, W)
    assert rc == 0
    wpos, wtab, wskip = shift_ref(pos, table, mode, ps, W)
    assert (gpos == wpos).all() and (gskip == wskip).all() and gtab.shape == wtab.shape and (gtab == wtab).all()
    assert max_kv == wpos.max() + 1 and (gskip < (ps if mode == 1 else 1)).all()
    assert max_kv <= W + (ps - 1 if mode == 1 else 0)                      # a row reads at most W keys plus its first page's skip
    unshifted = pos < W                                                  # f == 0: the row comes back as it went in
    assert unshifted.any() and (gpos[unshifted] == pos[unshifted]).all() and (gskip[unshifted] == 0).all()
    src = table[:, :gtab.shape[1]] if mode == 1 else table[:, None]
    assert (gtab[unshifted] == src[unshifted]).all()
