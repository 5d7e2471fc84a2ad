"""The per-request sampler on the device, operator level (pplhip_op_sample_rows / pplhip_op_sample_uniform), against tests/sample_rows.py:
the generator bit for bit, mixed batches by postproc.check_sample's rules, every row bit for bit against the uniform kernels launched on
that row alone, the SURVEY.md Q3 case, and a row's independence of its neighbours."""
import faulthandler

import numpy as np
import pytest

from tests import postproc as P
from tests import sample_rows as S
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CASES = S.all_cases()
STEP_SECONDS = 300     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.cuda.synchronize()


def _u64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _device_uniform(m, seeds, draws):
    B = len(seeds)
    d_s, d_n = _u64(seeds), _u64(draws)
    out = torch.from_numpy(np.full(B + 8, P.LP_CANARY, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    assert m.lib().pplhip_op_sample_uniform(None, d_s.data_ptr(), d_n.data_ptr(), B, out.data_ptr()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[B:] == P.LP_CANARY).all(), "pplhip_op_sample_uniform wrote behind batch"
    return got[:B]


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1024])
def test_uniform_bit_for_bit(B):
    m = load_pplhip()
    rng = np.random.RandomState(B)
    rnd64 = lambda n: (rng.randint(0, 2 ** 32, size=n).astype(np.uint64) << np.uint64(32)) | rng.randint(0, 2 ** 32, size=n).astype(np.uint64)
    s_edge = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1], dtype=np.uint64)
    n_edge = np.array([0, 1, 2 ** 32 - 1, 2 ** 32], dtype=np.uint64)
    # every edge seed with every edge draw, edges against random partners, then random pairs; B of them per launch, all launches of one size
    s, n = np.meshgrid(s_edge, n_edge, indexing="ij")
    seeds = np.concatenate([s.ravel(), s_edge, rnd64(len(n_edge)), rnd64(40)])
    draws = np.concatenate([n.ravel(), rnd64(len(s_edge)), n_edge, rnd64(40)])
    reps = -(-max(B, len(seeds)) // len(seeds))
    seeds, draws = np.tile(seeds, reps), np.tile(draws, reps)
    draws[len(draws) // reps:] += np.uint64(3)          # the repeats are new pairs
    for lo in range(0, len(seeds) - B + 1, B):
        sd, dr = seeds[lo:lo + B], draws[lo:lo + B]
        got = _device_uniform(m, sd, dr)
        want = S.uniform(sd, dr).view(np.uint32)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"row {bad[0]}: seed {int(sd[bad[0]]):#x} draw {int(dr[bad[0]]):#x} got {got[bad[0]]:#x} want {want[bad[0]]:#x}"


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c.name for c in CASES])
def test_mixed_batch(idx):
    """check_sample's rules per row, then every row against pplhip_op_sample on that row alone: token and logprob bits equal"""
    m = load_pplhip()
    c = CASES[idx].build()
    rows = c.check_assertions()[0]
    rc, tok, lp, tok_tail, lp_tail = S.launch_rows(m, torch, c)
    assert rc == 0, f"{c.name}: pplhip_op_sample_rows -> {rc}"
    fails = S.check_rows(c, rows, tok, lp, tok_tail, lp_tail)
    assert not fails, f"{c.name}: " + "; ".join(fails[:6])
    a_tok, a_lp = S.launch_rows_alone(m, torch, c)
    bad = np.flatnonzero((a_tok != tok) | (a_lp.view(np.uint32) != lp.view(np.uint32)))
    assert bad.size == 0, (f"{c.name}: {bad.size} rows differ from the uniform kernels, first row {bad[0]} (top_k {c.top_k[bad[0]]}): "
                           f"token {tok[bad[0]]} logprob {lp[bad[0]]!r}, alone token {a_tok[bad[0]]} logprob {a_lp[bad[0]]!r}")


def test_q3_greedy_row_behind_a_sampling_row():
    m = load_pplhip()
    c = S.q3_case()
    rows = c.check_assertions()[0]
    rc, tok, lp, tok_tail, lp_tail = S.launch_rows(m, torch, c)
    assert rc == 0
    assert not S.check_rows(c, rows, tok, lp, tok_tail, lp_tail)
    assert tok[1] == 321
    # the batch as today's call sees it: the first row's top_k for every row
    old = P.SCase("q3-uniform", "q3", c.logits, c.stride, c.off, 50, 1.0, None, None, c.rnd)
    d = torch.from_numpy(old.image()).cuda()
    d_r = torch.from_numpy(old.rnd).cuda()
    d_tok = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_lp = torch.zeros(2, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert m.lib().pplhip_op_sample(None, d.data_ptr(), None, None, d_r.data_ptr(), 2, c.V, c.stride, 50, 1.0, d_tok.data_ptr(), d_lp.data_ptr()) == 0
    torch.cuda.synchronize()
    o_tok = d_tok.cpu().numpy()
    assert o_tok[0] == tok[0]                            # the sampling row is answered alike
    assert o_tok[1] != 321                               # the greedy request behind it is sampled


def test_row_is_independent_of_its_neighbours():
    """one row, one (seed, draw): the same answer at batch positions 0, 1, 7 and 63, among other neighbours, in other batch sizes"""
    m = load_pplhip()
    V = 4097
    rng = np.random.RandomState(11)
    me = (rng.randn(V) * 1.0).astype(np.float32)
    seed, draw, k, p, t = 0xC0FFEE123456789, 5, 50, 0.9, 0.7
    want = None
    for pos, B in ((0, 1), (1, 2), (7, 8), (63, 64), (0, 64), (7, 64)):
        lg = (rng.randn(B, V) * 2.0).astype(np.float32)
        lg[pos] = me
        ks = np.array([S.KS[(b + pos) % len(S.KS)] for b in range(B)], dtype=np.int32)
        tp = np.array([S.PS[(b + pos) % len(S.PS)] for b in range(B)], dtype=np.float32)
        ts = np.array([S.TS[(b + pos) % len(S.TS)] for b in range(B)], dtype=np.float32)
        seeds = rng.randint(1, 2 ** 62, size=B).astype(np.uint64)
        draws = rng.randint(0, 1000, size=B).astype(np.uint64)
        ks[pos], tp[pos], ts[pos], seeds[pos], draws[pos] = k, p, t, seed, draw
        c = S.RCase(f"neighbours-{pos}-{B}", "rows-neighbours", lg, V + 2, pos % 4, ks, tp, ts, seeds, draws)
        rc, tok, lp, tok_tail, lp_tail = S.launch_rows(m, torch, c)
        assert rc == 0 and (tok_tail == P.TOK_CANARY).all() and (lp_tail == P.LP_CANARY).all()
        if want is None:
            x = c.x(pos)
            wtok, margin, _, lse = P.topk_ref(x, k, p, S.uniform([seed], [draw])[0])
            assert margin >= P.MARGIN                    # (a fixed outcome of the fixed seeds above)
            assert tok[pos] == wtok
            want = (int(tok[pos]), lp[pos:pos + 1].view(np.uint32)[0])
        # the row function is the same whatever the slot, so even the logprob bits are equal
        assert (int(tok[pos]), lp[pos:pos + 1].view(np.uint32)[0]) == want, (pos, B)


def test_batch_zero_and_invalid_arguments_write_nothing():
    m = load_pplhip()
    lg = torch.full((64,), float("inf"), dtype=torch.float32, device="cuda")
    tok = torch.from_numpy(np.full(8, P.TOK_CANARY, dtype=np.int32)).cuda()
    lp = torch.from_numpy(np.full(8, P.LP_CANARY, dtype=np.uint32).view(np.int32)).cuda()
    k = torch.ones(8, dtype=torch.int32, device="cuda")
    f = torch.zeros(8, dtype=torch.float32, device="cuda")
    u = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    call = lambda top_k, top_p, seeds, draws, rnd, batch, vocab, stride: m.lib().pplhip_op_sample_rows(
        None, lg.data_ptr(), None, top_k, top_p, seeds, draws, rnd, batch, vocab, stride, tok.data_ptr(), lp.data_ptr())
    assert call(k.data_ptr(), f.data_ptr(), u.data_ptr(), u.data_ptr(), None, 0, 16, 16) == 0
    assert call(k.data_ptr(), f.data_ptr(), u.data_ptr(), u.data_ptr(), None, 2, 16, 12) == -2      # rows that overlap
    assert call(None, f.data_ptr(), u.data_ptr(), u.data_ptr(), None, 2, 16, 16) == -2
    assert call(k.data_ptr(), None, u.data_ptr(), u.data_ptr(), None, 2, 16, 16) == -2
    assert call(k.data_ptr(), f.data_ptr(), None, u.data_ptr(), None, 2, 16, 16) == -2              # no generator input and no rnd
    assert call(k.data_ptr(), f.data_ptr(), u.data_ptr(), None, None, 2, 16, 16) == -2
    assert m.lib().pplhip_op_sample_uniform(None, u.data_ptr(), u.data_ptr(), 0, f.data_ptr()) == 0
    assert m.lib().pplhip_op_sample_uniform(None, None, u.data_ptr(), 2, f.data_ptr()) == -2
    torch.cuda.synchronize()
    assert (tok.cpu().numpy() == P.TOK_CANARY).all() and (lp.cpu().numpy().view(np.uint32) == P.LP_CANARY).all()
