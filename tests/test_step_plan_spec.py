"""The step schedule as a pure function (pplhip.cc plan_step, through pplhip_op_step_plan): no device, no context.

Every expectation here is written from the rules themselves -- literal chunks, or `want_*` below, a second statement of the rules in
Python -- never taken from the library:
* two chunks on the communication stream: tensor parallel, PPLHIP_TP_OVERLAP, a host copy of seq_starts, T >= the token threshold and
  B >= 2; the cut is the first request boundary at or after row T / 2 (never the last request), for pure decode whole 128-row tiles
  ((T / 2 rounded up to 128) when that is < B, else B / 2);
* two lanes: asked for, a second stream, not two chunks, pure decode, B in the row window and >= 2, collectives that have a second
  channel (none, identity, direct, or RCCL with a second communicator outside the automatic rule), fp16 activations, no residual
  dump, no graph capture; the first half is B / 2 rows, from 64 rows on rounded up to 16; lane 1's attention workspace starts
  b0 * H * 32 * (D + 2) floats in;
* the decode split of a chunk is decode_split of its decode rows; the fused norm and the two defer flags."""
import itertools

import pytest

from tests.conftest import load_pplhip

ONE, LANES, CHUNKS = 0, 1, 2
FP16, I8, FP8 = 0, 1, 2


def settings(**kw):
    s = dict(tp=1, tp_on=0, comm_mode=0, has_comm=0, has_comm2=0, emulate_tp=0, tp_overlap=1, dual_mode=0, dual_auto=0, has_stream2=0,
             tp_overlap_min_tokens=2048, dual_min_rows=96, dual_max_rows=512, fuse_norm_want=1, defer_on=1, act_fmt=FP16, hidden_dim=512,
             heads=8, kv_heads=8, head_dim=64, cache_quant_bit=8, cache_quant_group=8, decoding_attn_split_k=1)
    assert set(kw) <= set(s), set(kw) - set(s)
    s.update(kw)
    return s


def tp_direct(**kw):   # a tensor-parallel group on the direct collectives
    return settings(**dict(dict(tp=2, tp_on=1, comm_mode=2), **kw))


def dual(**kw):        # two-lane decode asked for, rows 2..512
    return dict(dict(dual_mode=1, has_stream2=1, dual_min_rows=2, tp_overlap=0), **kw)


def decode(m, s, B, **kw):
    return m.step_plan(s, B, B, B, list(range(B + 1)), **kw)


# ---- two chunks ---------------------------------------------------------------------------------------------------------------

def test_two_chunks_prefill_cut_at_the_request_boundary_behind_half_the_rows():
    m = load_pplhip()
    p = m.step_plan(tp_direct(tp_overlap_min_tokens=2), 6, 266, 0, [0, 40, 43, 172, 173, 189, 266])
    assert p["schedule"] == CHUNKS
    assert p["chunks"] == [(0, 3, 0, 172, 0), (3, 3, 172, 94, 0)]


def test_two_chunks_decode_rows_first():
    m = load_pplhip()
    p = m.step_plan(tp_direct(tp_overlap_min_tokens=2), 4, 100, 2, [0, 1, 2, 50, 100])
    assert p["schedule"] == CHUNKS
    assert p["chunks"] == [(0, 3, 0, 50, 2), (3, 1, 50, 50, 0)]


def test_two_chunks_never_leave_the_second_chunk_empty():
    m = load_pplhip()   # the boundary at or after T / 2 would be the step's end: the last request stays a chunk of its own
    p = m.step_plan(tp_direct(tp_overlap_min_tokens=2), 3, 100, 0, [0, 10, 20, 100])
    assert p["chunks"] == [(0, 2, 0, 20, 0), (2, 1, 20, 80, 0)]


@pytest.mark.parametrize("B,want", [(6, [(0, 3, 0, 3, 3), (3, 3, 3, 3, 3)]),                  # 128-row rounding does not fit: B / 2
                                    (300, [(0, 256, 0, 256, 256), (256, 44, 256, 44, 44)]),   # whole 128-row tiles in the first chunk
                                    (2, [(0, 1, 0, 1, 1), (1, 1, 1, 1, 1)]),
                                    (257, [(0, 128, 0, 128, 128), (128, 129, 128, 129, 129)]),
                                    (256, [(0, 128, 0, 128, 128), (128, 128, 128, 128, 128)])])
def test_two_chunks_pure_decode(B, want):
    m = load_pplhip()
    p = decode(m, tp_direct(tp_overlap_min_tokens=2), B)
    assert p["schedule"] == CHUNKS and p["chunks"] == want


@pytest.mark.parametrize("why,s,B,T,dec,seq", [
    ("below tp_overlap_min_tokens", tp_direct(tp_overlap_min_tokens=2048), 6, 266, 0, [0, 40, 43, 172, 173, 189, 266]),
    ("B = 1", tp_direct(tp_overlap_min_tokens=2), 1, 266, 0, [0, 266]),
    ("no host seq_starts", tp_direct(tp_overlap_min_tokens=2), 6, 266, 0, None),
    ("overlap off", tp_direct(tp_overlap_min_tokens=2, tp_overlap=0), 6, 266, 0, [0, 40, 43, 172, 173, 189, 266]),
    ("no tensor parallelism", settings(tp_overlap_min_tokens=2), 6, 266, 0, [0, 40, 43, 172, 173, 189, 266]),
])
def test_one_chunk(why, s, B, T, dec, seq):
    m = load_pplhip()
    p = m.step_plan(s, B, T, dec, seq)
    assert p["schedule"] == ONE and p["chunks"] == [(0, B, 0, T, dec)] and p["lane1_ws_off"] == 0, why


def test_the_threshold_itself_is_chunked():
    m = load_pplhip()
    assert decode(m, tp_direct(), 2048)["schedule"] == CHUNKS
    assert decode(m, tp_direct(), 2047)["schedule"] == ONE


# ---- two lanes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [settings(**dual()), tp_direct(**dual()), tp_direct(**dual(heads=4, kv_heads=1, head_dim=128))],
                         ids=["tp1", "direct", "direct_gqa"])
@pytest.mark.parametrize("B,b0", [(11, 5), (64, 32), (100, 64), (63, 31), (2, 1), (512, 256), (96, 48), (98, 64)])
def test_two_lanes_halves_and_workspace_offset(s, B, b0):
    m = load_pplhip()
    p = decode(m, s, B)
    assert p["schedule"] == LANES
    assert p["chunks"] == [(0, b0, 0, b0, b0), (b0, B - b0, b0, B - b0, B - b0)]
    assert p["lane1_ws_off"] == b0 * s["heads"] * 32 * (s["head_dim"] + 2)


def test_two_lanes_on_the_other_collectives():
    m = load_pplhip()
    rccl2 = settings(tp=2, tp_on=1, comm_mode=1, has_comm=1, has_comm2=1, **dual())       # RCCL, a communicator per lane, asked for explicitly
    identity = settings(tp=2, tp_on=1, comm_mode=0, has_comm=0, **dual())                 # no collective at all behind the schedule
    auto_direct = tp_direct(**dual(dual_auto=1, dual_min_rows=512, dual_max_rows=1024))   # the automatic rule on the direct collectives
    assert decode(m, rccl2, 11)["schedule"] == LANES
    assert decode(m, identity, 11)["schedule"] == LANES
    assert decode(m, auto_direct, 512)["schedule"] == LANES and decode(m, auto_direct, 1024)["schedule"] == LANES
    assert decode(m, auto_direct, 511)["schedule"] == ONE and decode(m, auto_direct, 1025)["schedule"] == ONE


@pytest.mark.parametrize("why,s,kw", [
    ("stream is capturing", tp_direct(**dual()), dict(capturing=True)),
    ("residual dump", tp_direct(**dual()), dict(dump=True)),
    ("int8 activations", tp_direct(**dual(act_fmt=I8)), {}),
    ("fp8 activations", tp_direct(**dual(act_fmt=FP8)), {}),
    ("B below the window", tp_direct(**dual(dual_min_rows=12)), {}),
    ("B above the window", tp_direct(**dual(dual_max_rows=10)), {}),
    ("RCCL without a second communicator", settings(tp=2, tp_on=1, comm_mode=1, has_comm=1, has_comm2=0, **dual()), {}),
    ("RCCL under the automatic rule", settings(tp=2, tp_on=1, comm_mode=1, has_comm=1, has_comm2=1, **dual(dual_auto=1)), {}),
    ("no second stream", tp_direct(**dual(has_stream2=0)), {}),
    ("not asked for", tp_direct(**dual(dual_mode=0)), {}),
])
def test_not_two_lanes(why, s, kw):
    m = load_pplhip()
    p = decode(m, s, 11, **kw)
    assert p["schedule"] == ONE and p["chunks"] == [(0, 11, 0, 11, 11)] and p["lane1_ws_off"] == 0, why
    control = dict(kw)   # the same step is two-lane once the obstacle is gone (so each case tests what it names)
    fixed = dict(s, act_fmt=FP16, dual_min_rows=2, dual_max_rows=512, has_comm2=s["has_comm"], dual_auto=0, has_stream2=1, dual_mode=1)
    control.pop("capturing", None)
    control.pop("dump", None)
    assert decode(m, fixed, 11, **control)["schedule"] == LANES, why


def test_not_two_lanes_with_a_prefill_row_or_under_the_chunked_schedule():
    m = load_pplhip()
    s = tp_direct(**dual())
    p = m.step_plan(s, 11, 12, 10, list(range(11)) + [12])      # ten decode rows and a two-token prefill
    assert p["schedule"] == ONE and p["chunks"] == [(0, 11, 0, 12, 10)]
    p = decode(m, tp_direct(**dual(tp_overlap=1, tp_overlap_min_tokens=2)), 11)   # the two-chunk schedule applies: it wins
    assert p["schedule"] == CHUNKS and p["lane1_ws_off"] == 0
    assert p["chunks"] == [(0, 5, 0, 5, 5), (5, 6, 5, 6, 6)]


# ---- flags and decode split: a second statement of the rules --------------------------------------------------------------------

def want_schedule(s, B, T, dec, has_seq, capturing, dump):
    if s["tp_on"] and s["tp_overlap"] and has_seq and T >= s["tp_overlap_min_tokens"] and B >= 2:
        return CHUNKS
    channel2 = (not s["tp_on"] or s["comm_mode"] == 2 or not s["has_comm"] or (s["has_comm2"] and not s["dual_auto"]))
    if (s["dual_mode"] and s["has_stream2"] and dec == B and T == B and s["dual_min_rows"] <= B <= s["dual_max_rows"] and B >= 2 and channel2
            and s["act_fmt"] == FP16 and not dump and not capturing):
        return LANES
    return ONE


def want_flags(s, schedule, dump):
    fuse = bool(s["fuse_norm_want"] and s["tp_on"] and s["tp"] > 1 and s["act_fmt"] == FP16 and not dump and s["hidden_dim"] % 8 == 0
                and s["hidden_dim"] <= 8192 and (s["comm_mode"] == 2 or s["emulate_tp"]))
    whole = schedule != CHUNKS     # one chunk, or two lanes
    defer_qkv = bool(s["defer_on"] and s["act_fmt"] == FP16 and not dump and whole)
    return fuse, bool(defer_qkv and not s["tp_on"]), defer_qkv


def want_split(s, nb, max_kv_len):
    mode, H, Hkv, D = s["decoding_attn_split_k"], s["heads"], s["kv_heads"], s["head_dim"]
    if mode == 0 or nb <= 0:
        return 1
    grp = H // Hkv
    gqa = H % Hkv == 0 and 4 <= grp <= 16 and (D in (64, 128) if s["cache_quant_bit"] == 8 else D in (32, 64, 128))
    blocks = nb * (Hkv if gqa else H)
    split = 1
    if mode == 2 or (blocks < 256 and max_kv_len >= 512):
        want = (512 + blocks - 1) // blocks
        cap = max(1, max_kv_len // 256, min(max_kv_len // 128, 8) if blocks <= 128 else 0)
        split = max(1, min(want, cap, 32))
        if mode == 2 and split < 2 and max_kv_len >= 64:
            split = 2
    return split


def test_fused_norm_and_defer_flags_over_the_cross_product():
    m = load_pplhip()
    comms = [dict(tp=1, tp_on=0, comm_mode=0), dict(tp=1, tp_on=1, comm_mode=1, has_comm=1),            # off; forced communicator at tp 1
             dict(tp=2, tp_on=1, comm_mode=1, has_comm=1, has_comm2=1), dict(tp=2, tp_on=1, comm_mode=2),
             dict(tp=4, tp_on=1, comm_mode=1, has_comm=1, emulate_tp=1)]
    shapes = [dict(tp_overlap=0), dict(tp_overlap=1, tp_overlap_min_tokens=2), dual()]                   # one chunk, two chunks, two lanes
    seen = set()
    for comm, shape, act, dump, fuse_want, defer_on, hd in itertools.product(comms, shapes, (FP16, I8, FP8), (False, True), (0, 1), (0, 1),
                                                                              (512, 516, 8192, 8200)):
        s = settings(**dict(comm, **shape), act_fmt=act, fuse_norm_want=fuse_want, defer_on=defer_on, hidden_dim=hd)
        sched = want_schedule(s, 11, 11, 11, True, False, dump)
        p = decode(m, s, 11, dump=dump)
        assert p["schedule"] == sched, (s, dump)
        assert (p["fuse_norm"], p["defer_reduce"], p["defer_qkv"]) == want_flags(s, sched, dump), (s, dump)
        seen.add((sched, p["fuse_norm"], p["defer_reduce"], p["defer_qkv"]))
    assert {x[0] for x in seen} == {ONE, LANES, CHUNKS}
    assert {x[1:] for x in seen} >= {(True, False, True), (True, False, False), (False, True, True), (False, False, True), (False, False, False)}


@pytest.mark.parametrize("heads,kv_heads,D,bit,group", [(32, 32, 128, 8, 8), (8, 1, 128, 8, 8), (8, 1, 128, 0, 1), (8, 2, 32, 8, 8), (8, 2, 32, 0, 1),
                                                         (4, 4, 64, 8, 64)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_decode_split_of_every_chunk(heads, kv_heads, D, bit, group, mode):
    m = load_pplhip()
    geo = dict(heads=heads, kv_heads=kv_heads, head_dim=D, cache_quant_bit=bit, cache_quant_group=group, decoding_attn_split_k=mode)
    for B, kv in itertools.product((1, 2, 3, 4, 8, 11, 16, 17, 33, 64, 100, 128, 129, 255, 256, 300), (1, 63, 64, 127, 128, 511, 512, 1024, 2048, 8192)):
        for s in (settings(**geo), tp_direct(tp_overlap_min_tokens=2, **geo), settings(**dual(**geo))):
            p = decode(m, s, B, max_kv_len=kv)
            assert p["decode_split"] == [want_split(s, c[4], kv) for c in p["chunks"]], (s, B, kv, p)
    p = m.step_plan(tp_direct(tp_overlap_min_tokens=2, **geo), 4, 100, 2, [0, 1, 2, 50, 100], max_kv_len=4096)   # a chunk without decode rows
    assert p["decode_split"] == [want_split(geo, 2, 4096), 1]


def test_bad_arguments():
    m = load_pplhip()
    with pytest.raises(m.PplHipError):
        m.step_plan(settings(), -1, 0, 0)
    assert m.lib().pplhip_op_step_plan(None, None, None) == -2
