"""min_p / typical_p truncation on the device, operator level (pplhip_op_sample_rows2) against tests/sample_trunc.py: every case family by
the margins' rules, the exact cases that need no margin, and the rows that do not ask bit for bit against pplhip_op_sample_rows."""
import faulthandler

import numpy as np
import pytest

from tests import postproc as P
from tests import sample_trunc as T
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = T.all_cases()
STEP_SECONDS = 300     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.cuda.synchronize()


def _lib():
    m = load_pplhip()
    assert hasattr(m.lib(), "pplhip_op_sample_rows2"), "the library has no pplhip_op_sample_rows2"
    return m


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name for c in CASES])
def test_cases(idx):
    m = _lib()
    c = CASES[idx].build()
    rows, n_t, n_unc = c.check_assertions()
    assert n_unc <= P.UNCOMPARED_CAP * n_t, (c.name, n_unc, n_t)
    rc, tok, lp, tok_tail, lp_tail = T.launch_rows2(m, torch, c)
    assert rc == 0, f"{c.name}: pplhip_op_sample_rows2 -> {rc}"
    fails = T.check_rows(c, rows, tok, lp, tok_tail, lp_tail)
    assert not fails, f"{c.name}: {len(fails)} rows; " + "; ".join(fails[:6])


def test_min_p_one_picks_among_the_ties_of_the_maximum():
    """min_p = 1 (and above) at temperature 4: e = 1 exactly for the maximum's ties and for nothing else; u walks them in index order"""
    m = _lib()
    c, ties = T.minp_one_case()
    rc, tok, lp, tok_tail, lp_tail = T.launch_rows2(m, torch, c)
    assert rc == 0 and (tok_tail == P.TOK_CANARY).all() and (lp_tail == P.LP_CANARY).all()
    for b in range(c.B):
        n = len(ties[b])
        # the scan of n ones is exact and u * n is compared with integers: only u * n itself rounds, and no u of the case stands at an integer
        assert tok[b] == ties[b][min(int(float(c.rnd[b]) * n), n - 1)], (b, tok[b], ties[b], c.rnd[b])
        x = c.x(b)
        assert abs(float(lp[b]) - (float(x[tok[b]]) - P._lse(x))) <= P.LOGPROB_BAR


def test_typical_never_draws_the_head():
    """p = 0.3 for one token, 0.7 shared by 714 equal ones, typical_p = 0.5: the head is never in the typical set, so no u draws the argmax;
    the same rows without the cut draw it whenever u < 0.3"""
    m = _lib()
    c, head = T.typical_head_case()
    rc, tok, lp, tok_tail, lp_tail = T.launch_rows2(m, torch, c)
    assert rc == 0 and (tok_tail == P.TOK_CANARY).all() and (lp_tail == P.LP_CANARY).all()
    assert ((tok >= 0) & (tok < c.V)).all()
    assert (tok != head).all(), np.flatnonzero(tok == head)
    others = np.setdiff1d(np.arange(c.V), [head])
    # the members are a prefix of the equal tokens in index order (ties of s go by rank), and the pick walks them with u
    assert (np.diff(tok) >= 0).all() and tok[0] == others[0] and tok[-1] <= others[520]
    x = c.x(0)
    assert np.abs(lp - (x[tok] - P._lse(x))).max() <= P.LOGPROB_BAR
    rc, tok0, _, _, _ = T.launch_rows2(m, torch, c, entry="pplhip_op_sample_rows")
    assert rc == 0 and (tok0[c.rnd < 0.29] == head).all() and (tok0[c.rnd > 0.31] != head).all()


def test_rows_that_do_not_ask_keep_their_bits():
    """a mixed launch: the greedy and the sampling rows (min_p / typical_p off by every default: 0, negative, NaN, >= 1) carry the token and
    logprob bits of pplhip_op_sample_rows on the same inputs; the truncating rows are checked against the reference"""
    m = _lib()
    c, plain = T.mixed_case()
    rows = c.check_assertions()[0]
    rc, tok, lp, tok_tail, lp_tail = T.launch_rows2(m, torch, c)
    assert rc == 0
    fails = T.check_rows(c, rows, tok, lp, tok_tail, lp_tail)
    assert not fails, "; ".join(fails[:6])
    rc, tok0, lp0, _, _ = T.launch_rows2(m, torch, c, entry="pplhip_op_sample_rows")
    assert rc == 0
    assert (tok[plain] == tok0[plain]).all() and (lp[plain].view(np.uint32) == lp0[plain].view(np.uint32)).all()
    asking = [b for b in range(c.B) if b not in plain]
    assert any(tok[b] != tok0[b] for b in asking)         # (a fixed outcome of the fixed seeds: the cut changes some draw)


@pytest.mark.parametrize("arrays", ["null", "off"])
def test_all_off_equals_sample_rows(arrays):
    """both arrays NULL, or every row off: pplhip_op_sample_rows everywhere, bit for bit"""
    m = _lib()
    lz = [l for l in T.S.grid_cases() if l.name.startswith("rows-V4097-alternating")][0]
    r = lz.build()
    off = arrays == "off"
    mp = [(0.0, -2.0, float("nan"))[b % 3] for b in range(r.B)] if off else None
    ty = [(1.0, 0.0, 1.5, float("nan"))[b % 4] for b in range(r.B)] if off else None
    c = T.TCase(r.name, "trunc-off", r.logits, r.stride, r.off, r.top_k, r.top_p, mp, ty, r.temps, r.seeds, r.draws)
    rc, tok, lp, tok_tail, lp_tail = T.launch_rows2(m, torch, c)
    assert rc == 0 and (tok_tail == P.TOK_CANARY).all() and (lp_tail == P.LP_CANARY).all()
    rc, tok0, lp0, _, _ = T.launch_rows2(m, torch, c, entry="pplhip_op_sample_rows")
    assert rc == 0
    assert (tok == tok0).all() and (lp.view(np.uint32) == lp0.view(np.uint32)).all()


def test_invalid_arguments_write_nothing():
    m = _lib()
    lg = torch.full((64,), float("inf"), dtype=torch.float32, device="cuda")
    tok = torch.from_numpy(np.full(8, P.TOK_CANARY, dtype=np.int32)).cuda()
    lp = torch.from_numpy(np.full(8, P.LP_CANARY, dtype=np.uint32).view(np.int32)).cuda()
    k = torch.ones(8, dtype=torch.int32, device="cuda")
    f = torch.full((8,), 0.5, dtype=torch.float32, device="cuda")
    u = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    call = lambda top_k, top_p, seeds, rnd, batch, vocab, stride: m.lib().pplhip_op_sample_rows2(
        None, lg.data_ptr(), None, top_k, top_p, f.data_ptr(), f.data_ptr(), seeds, seeds, rnd, batch, vocab, stride, tok.data_ptr(), lp.data_ptr())
    assert call(k.data_ptr(), f.data_ptr(), u.data_ptr(), None, 0, 16, 16) == 0
    assert call(k.data_ptr(), f.data_ptr(), u.data_ptr(), None, 2, 16, 12) == -2
    assert call(None, f.data_ptr(), u.data_ptr(), None, 2, 16, 16) == -2
    assert call(k.data_ptr(), None, u.data_ptr(), None, 2, 16, 16) == -2
    assert call(k.data_ptr(), f.data_ptr(), None, None, 2, 16, 16) == -2
    torch.cuda.synchronize()
    assert (tok.cpu().numpy() == P.TOK_CANARY).all() and (lp.cpu().numpy().view(np.uint32) == P.LP_CANARY).all()
