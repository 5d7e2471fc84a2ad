"""The direct collectives of csrc/k_comm.hip on the device through pplhip_comm_op (tests/comm_ops.py): every case of every rank count
bit for bit (the fused form's y within the helper's interval), on every rank, canaries included; sequences with ranks that arrive late;
the epoch counter across 2^31 and 2^32; flag words of blocks that were idle for 2^31 epochs; two channels at once; the refusals; and a
model step on the same context afterwards.  All ranks of a group live on device 0 (tests/test_gpu_tp.py says what that can show)."""
import faulthandler
import os

import numpy as np
import pytest

from oracle import ref
from tests import comm_ops as Cm
from tests.conftest import load_pplhip
from tests.test_gpu_tp import Group, check, generate

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STEP_SECONDS = 120     # a step that hangs ends the process (a dump of every thread's stack) instead of the whole run
P2P_TIMEOUT_MS = 5000  # a protocol error ends as a reported status word, not as a wait
HEADS = {2: 8, 3: 6, 4: 8, 5: 10, 6: 6, 7: 14, 8: 8}     # x 64 = the model's hidden size: tp divides heads, kv heads, intermediate, vocab
CAP_B = 32
KV_TOKENS = 1024
ONE, DUAL = 0, 1
GROUPS = [(n, ONE) for n in Cm.RANKS] + [(2, DUAL), (4, DUAL)]
GROUP_IDS = ["tp%d%s" % (n, "_two_streams" if d else "") for n, d in GROUPS]


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def make_desc(n):
    return ref.make_desc(hidden_dim=64 * HEADS[n], intermediate_dim=256 * n, num_layers=2, num_heads=HEADS[n], num_kv_heads=HEADS[n],
                         vocab_size=512 * n, max_position=256, cache_quant_bit=8, cache_quant_group=8, cache_layout=3, cache_mode=0,
                         weight_quant_bit=8)


def cap_tokens(n, dual):
    """max_tokens_per_step: the data buffer (cap_T x hidden fp16) holds the largest case, h and xn the largest fused image (a two-stream
    context gives a channel half of them and runs no block-cap shape)"""
    hd = 64 * HEADS[n]
    cs = [c for c in Cm.cases(n) if not (dual and c.kind == Cm.AR and c.tag == "block_cap")]
    need = max(max(c.data_bytes() for c in cs), (2 if dual else 1) * max(c.image_elems() * 2 for c in cs if c.kind == Cm.FUSED))
    if n == 2 and not dual:
        k = -(-need // 16384) | 1       # an odd number of 8192-wide rows: test_refusals finds a shape that fits the data buffer, not the scratch slice
        assert (16 * k * hd * 2) == k * 16384
        return 16 * k
    return -(-need // (hd * 2)) + 8


class CommGroup:
    def __init__(self, n, dual):
        self.m = m = load_pplhip()
        self.n, self.dual, self.desc = n, dual, make_desc(n)
        self.cap_T = cap_tokens(n, dual)
        env = {"PPLHIP_P2P_TIMEOUT_MS": str(P2P_TIMEOUT_MS), "PPLHIP_DUAL_STREAM": "1" if dual else "0", "PPLHIP_DUAL_MIN_ROWS": "2",
               "PPLHIP_TP_OVERLAP": "0"}
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            self.ctx = m.Context(m.copy_desc(self.desc), max_running_batch=CAP_B, max_tokens_per_step=self.cap_T, n_local_ranks=n,
                                 device_ids=[0] * n)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        assert self.ctx.comm_mode() == m.COMM_P2P
        self.models = None

    def counters(self):
        """(epoch of channel 0, of channel 1, all-reduces of channel 0, of channel 1): an empty call is refused and reports them"""
        rc, _, cnt = self.ctx.comm_op([])
        assert rc == -2
        return cnt

    def run(self, seq, **kw):
        rc, fails, cnt = Cm.run_sequence_gpu(self.ctx, seq, **kw)
        return fails, cnt

    def close(self):
        self.ctx.close()
        for mm in self.models or []:
            mm.close()


_LIVE = {}     # at most one group at a time: 8 ranks are 16 streams of the 24 hardware queues tests/conftest.py asks for


def live_group(key):
    """the group (ranks, two streams or one) -- one context per group for the whole module when the tests run in file order, in which
    every group's tests stand together"""
    if key not in _LIVE:
        for g in _LIVE.values():
            torch.cuda.synchronize()
            g.close()
        _LIVE.clear()
        _LIVE[key] = CommGroup(*key)
    return _LIVE[key]


@pytest.fixture(scope="module", autouse=True)
def _close_groups():
    yield
    for g in _LIVE.values():
        torch.cuda.synchronize()
        g.close()
    _LIVE.clear()


def by(n, kind, **kw):
    return next(c for c in Cm.cases(n) if c.kind == kind and all(getattr(c, k) == v for k, v in kw.items()))


def check_case(group, idx):
    """one case of tests/comm_ops.py: every rank's result, canaries included, and the counters one collective further"""
    c = Cm.cases(group.n)[idx]
    before = group.counters()
    fails, after = group.run([c])
    assert not fails, "; ".join(fails[:6])
    ch0 = (before[0] + 1) & 0xFFFFFFFF
    assert after == (ch0, before[1], before[2] + (c.kind != Cm.GATHER), before[3])


def ar_sizes(n):
    """six all-reduces of different sizes: one granule, ragged ones, two blocks, and small again"""
    return [by(n, Cm.AR, tag=t, family=f) for t, f in (("n+1", "random"), ("two_blocks", "mixed"), ("one", "exact"), ("n*per-1", "random"),
                                                       ("n(per-1)+1", "exact"), ("n", "random"))]


def check_sequences_with_late_ranks(group):
    """back to back on the streams with no host synchronisation: the scratch double buffer (rewritten two collectives later, no end
    barrier) and the flag epochs with ranks that arrive at different times"""
    n = group.n
    seq = ar_sizes(n)
    late_first = [[12 if r == 0 else 0 for r in range(n)]] * len(seq)
    late_last = [[12 if r == n - 1 else 0 for r in range(n)]] * len(seq)
    alternating = [[(8 if (r + i) % 2 else 0) for r in range(n)] for i in range(len(seq))]
    for skews in (None, late_first, late_last, alternating):
        fails, _ = group.run(seq, skews=skews)
        assert not fails, "; ".join(fails[:6])
    # the shape of a step: all-reduce, fused, all-reduce, fused, all-gather -- twice (the second all-gather behind two more all-reduces)
    step = [by(n, Cm.AR, tag="n+1", family="random"), by(n, Cm.FUSED, rows_tag="n+1", hidden=4104), by(n, Cm.AR, tag="n*per-1", family="exact"),
            by(n, Cm.FUSED, rows_tag="33n-1", hidden=8), by(n, Cm.GATHER, rows=5, cols=1026, stride=n * 1026 + 4)]
    for skews in (None, late_first[:5] * 2, late_last[:5] * 2):
        fails, _ = group.run(step + step, skews=skews)
        assert not fails, "; ".join(fails[:6])


def wrap_sequence(n, channel):
    """8 collectives; the all-gather (channel 0) sits right in front of the boundary and right behind it"""
    a, b = by(n, Cm.AR, tag="n+1", family="random"), by(n, Cm.AR, tag="n*per-1", family="exact")
    f = by(n, Cm.FUSED, rows_tag="n+1", hidden=8)
    g = by(n, Cm.GATHER, rows=5, cols=4, stride=n * 4 + 4) if channel == 0 else a
    return [a, f, g, b, g, f, a, b]


def check_epoch_wrap(group):
    """flags are 32-bit epochs compared with (int32)(flag - epoch) < 0: the 4th collective of a sequence of 8 gets epoch 0x80000000, then
    the 4th of another gets epoch 0 (each advance below 2^31)"""
    n = group.n
    for channel in ((0, 1) if group.dual else (0,)):
        seq = wrap_sequence(n, channel)
        for boundary in ((0x80000000, 0) if group.counters()[channel] < 0x7FFFFFF0 else (0, 0x80000000)):
            cur = group.counters()[channel]
            adv = (boundary - 4 - cur) & 0xFFFFFFFF
            assert adv < 0x80000000, (hex(cur), hex(boundary))
            fails, after = group.run(seq, channel=channel, advances=[adv] + [0] * 7, skews=[[3 * ((r + i) % 2) for r in range(n)] for i in range(8)])
            assert not fails, "; ".join(fails[:6])
            assert after[channel] == (boundary + 4) & 0xFFFFFFFF
        fails, _ = group.run(seq, channel=channel)
        assert not fails, "; ".join(fails[:6])


def check_blocks_that_were_idle_for_2_31_epochs(group):
    """a flag word belongs to one block index: small collectives never touch the words of block 1 and up, and after 2^31 of them a word
    left at epoch e compares as AHEAD of e + 2^31 + 1 -- the barrier of a larger collective would let that block through without its
    peers.  A two-block all-reduce, 2^31 epochs of one-block ones (one advance below 2^31 and the collectives themselves), then the
    two-block one again, with the last rank late: its partial sums are not yet in place when an unguarded block 1 of rank 0 reads them."""
    n = group.n
    big, one = by(n, Cm.AR, tag="two_blocks", family="mixed"), by(n, Cm.AR, tag="one", family="exact")
    late_last = [12 if r == n - 1 else 0 for r in range(n)]
    for channel in ((0, 1) if group.dual else (0,)):
        fails, _ = group.run([big], channel=channel)
        assert not fails, "; ".join(fails[:6])
        fails, _ = group.run([one, one, big, one, big], channel=channel, advances=[0x7FFFFFFF, 0, 0, 0, 0], skews=[None, None, late_last, None, late_last])
        assert not fails, "; ".join(fails[:6])


def check_two_channels_at_once(group):
    """channel 0 on the rank's stream and channel 1 on its second stream, an all-reduce sequence each with different data, interleaved
    in one call: flag sets, scratch pairs and epoch counters of their own"""
    n = group.n
    s0 = ar_sizes(n)
    s1 = [by(n, Cm.AR, tag=t, family=f) for t, f in (("two_blocks", "mixed"), ("n", "exact"), ("n+1", "exact"), ("one", "random"),
                                                     ("n*per-1", "random"), ("n(per-1)+1", "random"))]
    inputs, items, seq = [], [], []
    for i in range(len(s0)):
        for ch, c in ((0, s0[i]), (1, s1[i])):
            inp = c.build()
            seq.append(c)
            inputs.append(inp)
            items.append(c.item(inp, channel=ch, skew=[(4 if (r + i + ch) % 2 else 0) for r in range(n)]))
    before = group.counters()
    rc, outs, after = group.ctx.comm_op(items)
    assert rc == 0, group.ctx.last_error()
    for c, inp, out in zip(seq, inputs, outs):
        fails = Cm.check(c, inp, out)
        assert not fails, "; ".join(fails[:6])
    assert after == tuple((before[i] + len(s0)) & 0xFFFFFFFF for i in range(4))


def check_refusals(group):
    """PPLHIP_INVALID_VALUE before anything is enqueued: no outputs, the epoch counters and all-reduce counts as they were, and the valid
    cases that ran before pass again afterwards, canaries included"""
    n, m, ctx = group.n, group.m, group.ctx
    hd = group.desc.hidden_dim
    data_cap, image_cap = group.cap_T * hd * 2, group.cap_T * hd * 2 // (2 if group.dual else 1)
    ok_ar, ok_f, ok_g = by(n, Cm.AR, tag="n+1", family="exact"), by(n, Cm.FUSED, rows_tag="n+1", hidden=8), by(n, Cm.GATHER, rows=5, cols=4, stride=n * 4 + 4)
    fails, _ = group.run([ok_ar, ok_f, ok_g])
    assert not fails, "; ".join(fails[:6])
    before = group.counters()

    def refused(items):
        rc, outs, cnt = ctx.comm_op(items)
        assert rc == -2 and outs is None and cnt == before, (rc, ctx.last_error())
        return ctx.last_error()

    def ar(count, elems=None, **kw):
        z = [np.zeros(elems or count + Cm.PAD, dtype=np.float16) for _ in range(n)]
        return dict(kind=m.COMM_ALLREDUCE, count=count, data=z, **kw)

    def fused(rows, hidden, image=None, **kw):
        return dict(kind=m.COMM_ALLREDUCE_NORM, rows=rows, hidden=hidden, eps=Cm.EPS, data=[np.zeros(rows * hidden, dtype=np.float16) for _ in range(n)],
                    h=[np.zeros(image or rows * hidden, dtype=np.float16) for _ in range(n)],
                    xn=[np.zeros(image or rows * hidden, dtype=np.float16) for _ in range(n)], w=[np.ones(hidden, dtype=np.float16) for _ in range(n)], **kw)

    def gather(rows, cols, stride, image=None, **kw):
        return dict(kind=m.COMM_ALLGATHER, rows=rows, cols=cols, dst_stride=stride, data=[np.zeros(rows * cols, dtype=np.uint32) for _ in range(n)],
                    target=[np.zeros(image or rows * stride, dtype=np.uint32) for _ in range(n)], **kw)

    valid = ok_ar.item(ok_ar.build())
    assert "count" in refused([valid, ar(12)])                                   # count % 8 (behind a valid item: nothing of it runs either)
    assert "hidden" in refused([fused(3, 12)])                                    # hidden % 8
    assert "hidden" in refused([fused(1, 8200)])                                  # hidden > 8192
    assert "channel" in refused([ar(8, channel=2)])
    if not group.dual:
        assert "two-stream" in refused([ar(8, channel=1)])                       # channel 1 on a one-stream context
    assert "data buffer" in refused([ar(data_cap // 2 + 8, elems=data_cap // 2 + 8)])
    assert "data buffer" in refused([ar(8, elems=data_cap // 2 + 8)])            # the image past the end of the buffer
    assert "data buffer" in refused([fused(data_cap // 16 + 1, 8)])
    assert "h / xn" in refused([fused(1, 8, image=image_cap // 2 + 8)])
    if not group.dual:
        rows = data_cap // 16384                                                  # odd (cap_tokens): the first rank's slice is half a row larger than half
        assert rows % 2 == 1 and rows * 16384 == data_cap
        assert "scratch" in refused([fused(rows, 8192)])
    vl, V = group.desc.vocab_size // n, group.desc.vocab_size
    assert "gather source" in refused([gather(CAP_B + 1, vl, V)])
    assert "gather target" in refused([gather(CAP_B, vl, V + 2)])
    assert "dst_stride" in refused([gather(1, 4, 4 * n - 2, image=64)])
    assert "even" in refused([gather(1, 3, 4 * n)])                              # a row of 12 bytes: the launcher wants 8-byte granules
    if group.dual:
        assert "channel 0" in refused([gather(1, 4, 4 * n, channel=1)])
    g1 = ok_g.item(ok_g.build())
    assert "second all-gather" in refused([g1, ok_g.item(ok_g.build())])          # the illegal sequence
    if group.dual:
        assert "second all-gather" in refused([g1, ok_ar.item(ok_ar.build(), channel=1), ok_g.item(ok_g.build())])   # (channel 1 orders nothing on channel 0)
    assert "epoch_advance" in refused([ar(8, epoch_advance=0x80000000)])
    assert "skew" in refused([ar(8, skew=[65] * n)])
    assert group.counters() == before
    fails, _ = group.run([ok_ar, ok_f, ok_g])
    assert not fails, "; ".join(fails[:6])


def check_model_steps_still_work(group):
    """after everything above (the tests of a group run together, this one last): a prefill and decode steps on the same context against
    the oracle, within tests/test_gpu_tp.py's bound -- the op left the epochs and the scratch parity of every rank consistent.  (The
    two-stream groups decode as two half-batches: channel 1 as well.)"""
    n = group.n
    g = Group.__new__(Group)
    g.m, g.desc, g.tp, g.kv_tokens, g.ctx = group.m, group.desc, n, KV_TOKENS, group.ctx
    g.models = group.models = [ref.RefModel(group.desc, n, r) for r in range(n)]
    for r in range(n):
        g.models[r].kv_alloc(KV_TOKENS)
        g.ctx.kv_alloc(r, KV_TOKENS)
    g.synthetic(31 + n)
    rng = np.random.RandomState(n)
    prompts = [rng.randint(3, group.desc.vocab_size, size=k) for k in (40, 3, 29, 1, 16, 77, 5, 9, 2, 33, 12)]
    before = group.counters()
    check("comm_ops_tp%d%s_steps" % (n, "_two_streams" if group.dual else ""), generate(g, prompts, 3), k=1.5)
    after = group.counters()
    assert after[0] != before[0] and (not group.dual or after[1] != before[1])
    sched = group.m.SCHED_TWO_LANES if group.dual else group.m.SCHED_ONE_LANE
    assert g.ctx.comm_info(len(prompts))["schedule"] == group.m.COMM_SCHEDULES[sched]
    fails, _ = group.run([by(n, Cm.AR, tag="n+1", family="random"), by(n, Cm.FUSED, rows_tag="n+1", hidden=8)])   # ... and the op after the steps
    assert not fails, "; ".join(fails[:6])


# ---- the tests: group by group, so that a group's context is created once and its model steps come after everything else ----
PLAN = {
    (2, ONE): (check_case, check_sequences_with_late_ranks, check_epoch_wrap, check_blocks_that_were_idle_for_2_31_epochs, check_refusals),
    (3, ONE): (check_case, check_sequences_with_late_ranks, check_epoch_wrap, check_blocks_that_were_idle_for_2_31_epochs),
    (4, ONE): (check_case,), (5, ONE): (check_case,), (6, ONE): (check_case,), (7, ONE): (check_case,),
    (8, ONE): (check_case, check_sequences_with_late_ranks),
    (2, DUAL): (check_epoch_wrap, check_blocks_that_were_idle_for_2_31_epochs, check_two_channels_at_once, check_refusals),
    (4, DUAL): (check_epoch_wrap, check_two_channels_at_once),
}


def _define(key, gid, body):
    name = "test_%s_%s" % (gid, body.__name__[len("check_"):])
    if body is check_case:
        def test(idx):
            body(live_group(key), idx)
        names = [c.name for c in Cm.cases(key[0])]
        test = pytest.mark.parametrize("idx", range(len(names)), ids=names)(test)
    else:
        def test():
            body(live_group(key))
    test.__name__ = test.__qualname__ = name
    test.__doc__ = body.__doc__
    globals()[name] = test


for _key, _gid in zip(GROUPS, GROUP_IDS):
    for _body in PLAN[_key] + (check_model_steps_still_work,):
        _define(_key, _gid, _body)
