"""pplhip_sample_rows, the product entry point of the per-request sampler, on the logits of a real step of a tiny model: equal to the
operator on the copied logits, parameters taken on every call (no req_list_changed rule), free of rand() and so of pplhip_sample's sequence,
NULL temperatures behind the penalty kernel, invalid arguments refused."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref
from tests import postproc as P
from tests import sample_rows as S
from tests.conftest import load_pplhip

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, N = 1024, 4
K = np.array([1, 50, 0, 1], dtype=np.int32)
TP = np.array([0.0, 0.9, 0.95, 1.0], dtype=np.float32)
T = np.array([0.7, 1.3, 2.0, 0.0], dtype=np.float32)
SEEDS = np.array([11, 2 ** 40 + 3, 2 ** 64 - 5, 0], dtype=np.uint64)
DRAWS = np.array([0, 1, 2 ** 32, 7], dtype=np.uint64)


@pytest.fixture(scope="module")
def model():
    """a context after one prefill step of N requests; yields (binding, context, step inputs)"""
    m = load_pplhip()
    desc = ref.make_desc(hidden_dim=256, intermediate_dim=512, num_layers=1, num_heads=4, num_kv_heads=4, vocab_size=V,
                         max_position=256, cache_quant_bit=0, cache_quant_group=1, cache_layout=3, cache_mode=0)
    ctx = m.Context(m.copy_desc(desc), max_running_batch=8, max_tokens_per_step=64, enable_penalty=True)
    ctx.init_synthetic(0, 3)
    ctx.kv_alloc(0, 256)
    rng = np.random.RandomState(2)
    prompts = [rng.randint(3, V, size=n) for n in (12, 5, 9, 7)]
    lens = np.array([len(p) for p in prompts])
    tok = np.concatenate(prompts).astype(np.int64)
    seq = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    step = (tok, seq, np.zeros(N, dtype=np.int64), np.array([0, 64, 128, 192], dtype=np.int64))
    yield m, ctx, step
    ctx.close()


def _run(m, ctx, step):
    ctx.set_inputs(0, m.make_step(*step, 0, req_list_changed=1))
    ctx.run(0)
    return ctx.copy_logits(N)


def _case(logits, k, tp, t, seeds, draws):
    return S.RCase("model", "rows-model", logits, V, 0, k, tp, t, seeds, draws)


def _same(a, b):
    return (a[0] == b[0]).all() and (a[1].view(np.uint32) == b[1].view(np.uint32)).all()


def _check(m, logits, got, k, tp, t, seeds, draws):
    """the product's answer against the operator on the copied logits (bit for bit) and against the per-row reference"""
    c = _case(logits, k, tp, t, seeds, draws)
    rc, tok, lp, tok_tail, lp_tail = S.launch_rows(m, torch, c)
    assert rc == 0
    assert _same(got, (tok, lp)), (got, tok, lp)
    rows = c.reference()                                 # (real logits: no planted gaps; x is exact, so the arg-max is compared at any gap)
    fails = S.check_rows(c, rows, got[0], got[1], tok_tail, lp_tail)
    assert not fails, "; ".join(fails[:6])
    return rows


def test_equals_the_operator_and_takes_parameters_on_every_call(model):
    m, ctx, step = model
    logits = _run(m, ctx, step)
    got = ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=T)
    rows_a = _check(m, logits, got, K, TP, T, SEEDS, DRAWS)
    # the same step, no request-list change: the greedy rows now sample a flattened row, the sampling rows turn greedy
    k2 = np.array([0, 1, 1, 0], dtype=np.int32)
    tp2 = np.array([1.0, 0.5, 0.5, 1.0], dtype=np.float32)
    t2 = np.array([40.0, 1.0, 1.0, 40.0], dtype=np.float32)
    sd2 = SEEDS + np.uint64(17)
    got2 = ctx.sample_rows(k2, tp2, sd2, DRAWS, temperatures=t2)
    rows_b = _check(m, logits, got2, k2, tp2, t2, sd2, DRAWS)
    # teeth: the two parameter sets ask for different tokens in the rows that stopped being greedy, decided by a wide margin
    for b in (0, 3):
        assert rows_b[b][2] >= P.MARGIN and rows_b[b][0] != rows_a[b][0], (b, rows_a[b][:3], rows_b[b][:3])
        assert got2[0][b] != got[0][b]
    # and back
    assert _same(ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=T), got)


def test_does_not_share_a_random_sequence_with_pplhip_sample(model):
    m, ctx, step = model
    _run(m, ctx, step)
    libc = C.CDLL(None)
    a1 = ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=T)
    libc.srand(12345)
    s1 = ctx.sample(N, top_k=50, top_p=0.9, temperatures=T)
    a2 = ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=T)
    assert _same(a1, a2)
    # pplhip_sample again from the same point of rand()'s sequence, this time with per-request calls in between
    libc.srand(12345)
    ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=T)
    ctx.sample_rows(K, TP, SEEDS + np.uint64(1), DRAWS, temperatures=T)
    s2 = ctx.sample(N, top_k=50, top_p=0.9, temperatures=T)
    assert _same(s1, s2)
    g1 = ctx.sample(N, top_k=1, temperatures=T)
    ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=T)
    assert _same(g1, ctx.sample(N, top_k=1, temperatures=T))


def test_null_temperatures_behind_the_penalty_kernel(model):
    m, ctx, step = model
    _run(m, ctx, step)
    rep = np.array([1.2, 1.0, 1.5, 0.8], dtype=np.float32)
    pres = np.array([0.1, 0.0, 0.3, 0.2], dtype=np.float32)
    freq = np.array([0.05, 0.2, 0.0, 0.1], dtype=np.float32)
    ctx.penalty(T, rep, pres, freq, np.array([5, 0, 2, 7], dtype=np.int64), req_list_changed=True)
    penalised = ctx.copy_logits(N)                       # already divided by the temperatures
    got = ctx.sample_rows(K, TP, SEEDS, DRAWS, temperatures=None)
    _check(m, penalised, got, K, TP, None, SEEDS, DRAWS)


def test_invalid_arguments(model):
    m, ctx, step = model
    _run(m, ctx, step)
    lg = ctx.logits_ptr(0)[0]
    tok = np.full(16, P.TOK_CANARY, dtype=np.int32)
    lp = np.full(16, P.LP_CANARY, dtype=np.uint32)
    k, p, s, n = (np.ascontiguousarray(a) for a in (np.ones(16, np.int32), np.ones(16, np.float32), np.ones(16, np.uint64), np.ones(16, np.uint64)))

    def call(batch=N, top_k=k.ctypes.data, top_p=p.ctypes.data, seeds=s.ctypes.data, draws=n.ctypes.data, logits=lg, args=True, out=tok.ctypes.data):
        a = m.SampleRowsArgs()
        a.top_k, a.top_p, a.seeds, a.draws = top_k, top_p, seeds, draws
        a.batch, a.vocab_size, a.batch_stride = batch, V, V
        return m.lib().pplhip_sample_rows(ctx.h, logits, C.byref(a) if args else None, out, lp.ctypes.data)

    assert call(top_k=None) == -2 and call(top_p=None) == -2 and call(seeds=None) == -2 and call(draws=None) == -2
    assert call(batch=-1) == -2 and call(batch=9) == -2          # max_running_batch is 8
    assert call(logits=None) == -2 and call(args=False) == -2 and call(out=None) == -2
    assert (tok == P.TOK_CANARY).all() and (lp == P.LP_CANARY).all()
    assert call(batch=0) == 0
    assert (tok == P.TOK_CANARY).all() and (lp == P.LP_CANARY).all()
    assert call() == 0 and (tok[N:] == P.TOK_CANARY).all() and (tok[:N] >= 0).all() and (tok[:N] < V).all()
