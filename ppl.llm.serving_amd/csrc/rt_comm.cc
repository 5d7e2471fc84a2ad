// The direct collectives (k_comm.hip) as the runtime sets them up: mapping the peers' exchange regions (in this process or over IPC
// handles), the start-up self-test that decides between them and RCCL, and the pplhip_comm_* entry points.  What a step does with them
// (chunk_allreduce, the stream hand-offs of the two-chunk schedule) is in pplhip.cc.
#include "rt_internal.h"

static int p2p_refresh_if_due(pplhip_ctx* c, int rank, Channel& ch, hipStream_t s) {
    if ((uint32_t)(ch.p2p_epoch - ch.refreshed_at) >= P2P_FLAG_REFRESH_EPOCHS) {
        HIPCK(c, rank, launch_p2p_flag_refresh(s, c->ranks[rank].xbase, ch.id, ch.p2p_epoch));
        ch.refreshed_at = ch.p2p_epoch;
    }
    return 0;
}

int p2p_next_epoch(pplhip_ctx* c, int rank, Channel& ch, hipStream_t s, uint32_t* epoch) {
    if (int rc = p2p_refresh_if_due(c, rank, ch, s)) return rc;
    *epoch = ++ch.p2p_epoch;
    return 0;
}

namespace {

// the direct path cannot be used: an error when it was demanded (or no RCCL communicator exists), else RCCL stays in charge
int p2p_unavailable(pplhip_ctx* c, int rank, const std::string& why) {
    if (c->comm_want == 2 || c->comm_mode != 1) return fail(c, rank, PPLHIP_DEVICE_RUNTIME_ERROR, "direct collectives unavailable: " + why);
    c->selftest = -1;
    comm_note(c, "direct collectives unavailable (" + why + "): RCCL takes over");
    return 0;
}

// Runs both collectives four times on changing patterns on every local rank (all ranks of the group do this at the same time,
// in this process or in others) and compares with the exact answer.  Every rank then learns whether ALL ranks passed
// (one RCCL all-reduce when a communicator exists); only then comm_mode becomes 2.
// `local_failure`: this process could not even map its peers -- it skips the kernels but still takes part in the agreement, so that
// the other processes (whose self-test kernels give up waiting for it after the bounded spin) do not wait in the all-reduce forever.
int p2p_selftest(pplhip_ctx* c, const std::string* local_failure = nullptr) {
    const int n = (int)c->ranks.size(), tp = c->tp, hd = c->d.hidden_dim;
    // granules of the direct kernels (k_comm.hip): 16-byte pieces of the fp16 partial sums, 8- or 16-byte pieces of a shard's fp32
    // logits rows; a model that does not fit them keeps RCCL instead of failing at its first real step
    std::string shape_failure;
    if (!local_failure && (c->vocab_local % 2 != 0 || hd % 8 != 0)) {
        shape_failure = "vocab/tp must be even and hidden a multiple of 8 (vocab_local " + std::to_string(c->vocab_local) + ", hidden " + std::to_string(hd) + ")";
        local_failure = &shape_failure;
    }
    const int64_t cnt = std::min<int64_t>((int64_t)1 << 20, c->ranks[0].cap_T * (int64_t)hd) / 8 * 8;
    // the gather test: every rank's [grows, gcols] fp32 block -> [grows, gcols * tp]
    const int64_t gcols = c->vocab_local / 2 * 2, grows = std::min<int64_t>(c->ranks[0].cap_B, std::max<int64_t>(1, ((int64_t)1 << 18) / gcols));
    const int64_t gcnt = grows * gcols;
    const char* e = getenv("PPLHIP_P2P_SELFTEST_MS");
    const uint64_t ticks = (uint64_t)(e ? std::max(1, atoi(e)) : 10000) * 100000ull;
    auto pat = [](int64_t i, int g, int round) { return p2p_pattern_value(i, g, round); };
    bool ok = local_failure == nullptr;
    std::string why = local_failure ? *local_failure : std::string();
    std::vector<uint16_t> hbuf(cnt);
    std::vector<float> gbuf(gcnt), gall;
    for (int round = 0; round < 4 && ok; ++round) {
        for (int r = 0; r < n; ++r) {
            Rank& R = c->ranks[r];
            HIPCK(c, r, hipSetDevice(R.device));
            // inputs are written by a kernel on the rank's stream, like the partial sums and logits shards of a real step
            HIPCK(c, r, launch_p2p_pattern(R.stream, R.part, cnt, R.logits_local, gcnt, R.global_rank, round));
        }
        for (int r = 0; r < n; ++r) {
            Rank& R = c->ranks[r];
            Channel& ch = R.ch[0];
            HIPCK(c, r, hipSetDevice(R.device));
            uint32_t ep = 0;
            if (int rc = p2p_next_epoch(c, r, ch, R.stream, &ep)) return rc;
            HIPCK(c, r, launch_p2p_allreduce(R.stream, R.peers, R.global_rank, tp, R.x_part, ch.x_scratch[ch.ar_count++ & 1], cnt, ep,
                                             ticks, R.p2p_status));
            if (int rc = p2p_next_epoch(c, r, ch, R.stream, &ep)) return rc;
            HIPCK(c, r, launch_p2p_allgather(R.stream, R.peers, R.global_rank, tp, R.x_local, R.logits, grows, gcols * 4, (int64_t)gcols * 4 * tp,
                                             ep, ticks, R.p2p_status));
        }
        for (int r = 0; r < n && ok; ++r) {
            Rank& R = c->ranks[r];
            HIPCK(c, r, hipSetDevice(R.device));
            HIPCK(c, r, hipStreamSynchronize(R.stream));
            if (*R.p2p_status) { ok = false; why = "spin timed out (status " + std::to_string(*R.p2p_status) + ")"; *R.p2p_status = 0; break; }
            HIPCK(c, r, hipMemcpy(hbuf.data(), R.part, cnt * 2, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < cnt && ok; ++i) {
                float want = 0.f;
                for (int g = 0; g < tp; ++g) want += pat(i, g, round);
                if ((float)__builtin_bit_cast(_Float16, hbuf[i]) != want) {
                    ok = false;
                    int64_t nbad = 0, last = i;
                    for (int64_t j = i; j < cnt; ++j) {
                        float w2 = 0.f;
                        for (int g = 0; g < tp; ++g) w2 += pat(j, g, round);
                        if ((float)__builtin_bit_cast(_Float16, hbuf[j]) != w2) { ++nbad; last = j; }
                    }
                    why = "all-reduce mismatch: round " + std::to_string(round) + " rank " + std::to_string(R.global_rank) + " first " + std::to_string(i) +
                          " last " + std::to_string(last) + " bad " + std::to_string(nbad) + "/" + std::to_string(cnt) + " got " +
                          std::to_string((float)__builtin_bit_cast(_Float16, hbuf[i])) + " want " + std::to_string(want);
                }
            }
            gall.resize((size_t)gcnt * tp);
            HIPCK(c, r, hipMemcpy(gall.data(), R.logits, gall.size() * 4, hipMemcpyDeviceToHost));
            for (int g = 0; g < tp && ok; ++g)
                for (int64_t i = 0; i < gcnt && ok; ++i)
                    if (gall[(size_t)(i / gcols) * gcols * tp + (size_t)g * gcols + i % gcols] != pat(i, g, round + 2)) {
                        ok = false;
                        int64_t nbad = 0, last = i;
                        for (int64_t j = i; j < gcnt; ++j)
                            if (gall[(size_t)(j / gcols) * gcols * tp + (size_t)g * gcols + j % gcols] != pat(j, g, round + 2)) { ++nbad; last = j; }
                        why = "all-gather mismatch: round " + std::to_string(round) + " rank " + std::to_string(R.global_rank) + " block " + std::to_string(g) +
                              " first " + std::to_string(i) + " last " + std::to_string(last) + " bad " + std::to_string(nbad) + "/" + std::to_string(gcnt) +
                              " got " + std::to_string(gall[(size_t)(i / gcols) * gcols * tp + (size_t)g * gcols + i % gcols]) + " want " + std::to_string(pat(i, g, round + 2)) +
                              " prev-round " + std::to_string(pat(i, g, round + 1));
                    }
        }
    }
    // the fused all-reduce + residual add + RMSNorm (p2p_allreduce_norm_kernel, what a step issues when fuse_norm_active): against a LOCAL
    // reference built from parts that are already verified -- the plain all-reduce above leaves the exact sums on every rank, the kernel's
    // own one-rank form ("solo": same arithmetic, no peers) turns them into the expected residual and normed rows; the real kernel, run on
    // the unreduced patterns, must then give the same bits in every row it gathered and in the residual rows it owns
    const int64_t frows = hd > 0 ? cnt / hd : 0;
    if (ok && c->fuse_norm_want && c->act_fmt == ACT_FP16 && hd % 8 == 0 && hd <= P2P_NORM_MAX_HIDDEN && frows >= 1 &&
        c->ranks[0].gemm_ws_bytes >= (size_t)frows * hd * 4 + (size_t)hd * 2) {
        const int64_t fcnt = frows * hd;
        std::vector<uint16_t> want_x(fcnt), want_h(fcnt);
        for (int round = 0; round < 2 && ok; ++round) {
            for (int r = 0; r < n; ++r) {
                Rank& R = c->ranks[r];
                Channel& ch = R.ch[0];
                HIPCK(c, r, hipSetDevice(R.device));
                uint16_t* xref = (uint16_t*)R.gemm_ws, *href = xref + fcnt, *w = href + fcnt;
                HIPCK(c, r, launch_p2p_pattern(R.stream, R.part, fcnt, nullptr, 0, R.global_rank, round + 4));
                uint32_t ep = 0;
                if (int rc = p2p_next_epoch(c, r, ch, R.stream, &ep)) return rc;
                HIPCK(c, r, launch_p2p_allreduce(R.stream, R.peers, R.global_rank, tp, R.x_part, ch.x_scratch[ch.ar_count++ & 1], fcnt, ep, ticks, R.p2p_status));
                HIPCK(c, r, launch_p2p_pattern(R.stream, R.h, fcnt, nullptr, 0, 17, round + 4));    // the residual stream: the same on every rank
                HIPCK(c, r, launch_p2p_pattern(R.stream, w, hd, nullptr, 0, 23, round + 4));
                HIPCK(c, r, hipMemcpyAsync(href, R.h, (size_t)fcnt * 2, hipMemcpyDeviceToDevice, R.stream));
                HIPCK(c, r, launch_p2p_allreduce_norm(R.stream, R.peers, R.global_rank, 1, R.x_part, 0, frows, hd, href, w, c->d.norm_eps, xref, 0, ticks, R.p2p_status));
                HIPCK(c, r, launch_p2p_pattern(R.stream, R.part, fcnt, nullptr, 0, R.global_rank, round + 4));
                if (int rc = p2p_next_epoch(c, r, ch, R.stream, &ep)) return rc;
                HIPCK(c, r, launch_p2p_allreduce_norm(R.stream, R.peers, R.global_rank, tp, R.x_part, ch.x_scratch[ch.ar_count++ & 1], frows, hd, R.h, w, c->d.norm_eps,
                                                      R.xn, ep, ticks, R.p2p_status));
            }
            for (int r = 0; r < n && ok; ++r) {
                Rank& R = c->ranks[r];
                HIPCK(c, r, hipSetDevice(R.device));
                HIPCK(c, r, hipStreamSynchronize(R.stream));
                if (*R.p2p_status) { ok = false; why = "fused all-reduce + norm: spin timed out (status " + std::to_string(*R.p2p_status) + ")"; *R.p2p_status = 0; break; }
                HIPCK(c, r, hipMemcpy(want_x.data(), R.gemm_ws, (size_t)fcnt * 2, hipMemcpyDeviceToHost));
                HIPCK(c, r, hipMemcpy(want_h.data(), (uint16_t*)R.gemm_ws + fcnt, (size_t)fcnt * 2, hipMemcpyDeviceToHost));
                HIPCK(c, r, hipMemcpy(hbuf.data(), R.xn, (size_t)fcnt * 2, hipMemcpyDeviceToHost));
                int64_t bad = 0, first = -1;
                for (int64_t i = 0; i < fcnt; ++i) if (hbuf[i] != want_x[i]) { if (!bad) first = i; ++bad; }
                if (bad) { ok = false; why = "fused all-reduce + norm: " + std::to_string(bad) + "/" + std::to_string(fcnt) + " normed values differ on rank " + std::to_string(R.global_rank) + " (first: row " + std::to_string(first / hd) + ")"; break; }
                const int64_t per = (frows + tp - 1) / tp, lo = std::min<int64_t>(per * R.global_rank, frows), hi = std::min<int64_t>(lo + per, frows);
                HIPCK(c, r, hipMemcpy(hbuf.data(), R.h, (size_t)fcnt * 2, hipMemcpyDeviceToHost));
                for (int64_t i = lo * hd; i < hi * hd; ++i) if (hbuf[i] != want_h[i]) { ++bad; }
                if (bad) { ok = false; why = "fused all-reduce + norm: " + std::to_string(bad) + " residual values of the owned rows differ on rank " + std::to_string(R.global_rank); break; }
            }
        }
    }
    // agreement: min over all ranks of the group
    if (c->comm_mode == 1) {
        for (int r = 0; r < n; ++r) {
            Rank& R = c->ranks[r];
            HIPCK(c, r, hipSetDevice(R.device));
            const int32_t v = ok ? 1 : 0;
            HIPCK(c, r, hipMemcpy(R.d_flag, &v, 4, hipMemcpyHostToDevice));
        }
        NCCLCK(c, -1, ncclGroupStart());
        for (int r = 0; r < n; ++r) NCCLCK(c, r, ncclAllReduce(c->ranks[r].d_flag, c->ranks[r].d_flag, 1, ncclInt32, ncclMin, c->ranks[r].ch[0].comm, c->ranks[r].stream));
        NCCLCK(c, -1, ncclGroupEnd());
        for (int r = 0; r < n; ++r) {
            Rank& R = c->ranks[r];
            HIPCK(c, r, hipSetDevice(R.device));
            HIPCK(c, r, hipStreamSynchronize(R.stream));
            int32_t v = 0;
            HIPCK(c, r, hipMemcpy(&v, R.d_flag, 4, hipMemcpyDeviceToHost));
            if (!v && ok) { ok = false; why = "another rank failed its self-test"; }
        }
    }
    if (!ok) {
        // the check loop stopped at the first rank that showed a failure: drain EVERY local rank (the others normally time out on
        // the same dead peer) and clear every status word, or the RCCL steps that follow would report a stale "timed out"
        for (int r = 0; r < n; ++r) {
            Rank& R = c->ranks[r];
            (void)hipSetDevice(R.device);
            (void)hipStreamSynchronize(R.stream);
            if (R.p2p_status) *R.p2p_status = 0;
        }
        return p2p_unavailable(c, 0, "self-test: " + why);
    }
    c->comm_mode = 2;
    c->selftest = 1;
    if (verbose()) fprintf(stderr, "[pplhip] direct collectives over peer-mapped memory: self-test passed on %d local rank(s) of %d\n", n, tp);
    return 0;
}

}  // namespace

// all ranks of the group are in this process (the reference's mode, resource_manager.cc:392-422)
int p2p_connect_local(pplhip_ctx* c) {
    const int n = (int)c->ranks.size();
    for (int r = 0; r < n; ++r) {
        Rank& R = c->ranks[r];
        HIPCK(c, r, hipSetDevice(R.device));
        for (int g = 0; g < n; ++g) {
            Rank& Q = c->ranks[g];
            if (Q.device != R.device) {
                hipError_t e = hipDeviceEnablePeerAccess(Q.device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); return p2p_unavailable(c, r, std::string("peer access: ") + hipGetErrorString(e)); }
                (void)hipGetLastError();
            }
            R.peers.base[g] = Q.xbase;
        }
    }
    c->p2p_connected = true;
    return p2p_selftest(c);
}

// a kernel of the direct path gave up waiting for a peer: surfaced at the step's synchronisation points
int p2p_check(pplhip_ctx* c, int rank) {
    Rank& R = c->ranks[rank];
    if (R.p2p_status && *R.p2p_status == 64)
        return fail(c, rank, PPLHIP_DEVICE_RUNTIME_ERROR, "stream hand-off timed out (compute / communication stream of a tensor-parallel step)");
    if (c->comm_mode == 2 && R.p2p_status && *R.p2p_status) {
        const uint32_t v = *R.p2p_status;
        return fail(c, rank, PPLHIP_DEVICE_RUNTIME_ERROR, "direct collective timed out waiting for rank " + std::to_string((v - 1) & 15) +
                    ((v - 1) & 16 ? " (end barrier)" : " (start barrier)"));
    }
    return 0;
}

int pplhip_comm_export(pplhip_ctx* c, int rank, void* handle_out) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size() || !handle_out) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    memset(handle_out, 0, PPLHIP_IPC_HANDLE_BYTES);
    if (!R.xbase) return fail(c, rank, PPLHIP_INVALID_VALUE, "no exchange region (tensor parallelism is off)");
    static_assert(sizeof(hipIpcMemHandle_t) <= PPLHIP_IPC_HANDLE_BYTES, "ipc handle size");
    HIPCK(c, rank, hipSetDevice(R.device));
    hipIpcMemHandle_t h;
    HIPCK(c, rank, hipIpcGetMemHandle(&h, R.xbase));
    memcpy(handle_out, &h, sizeof(h));
    return 0;
}

int pplhip_comm_connect(pplhip_ctx* c, const void* all_handles) {
    if (!c || !all_handles) return PPLHIP_INVALID_VALUE;
    if (!c->tp_on || c->tp > P2P_MAX_RANKS) return fail(c, -1, PPLHIP_INVALID_VALUE, "nothing to connect");
    if (c->comm_want == 1) return 0;  // PPLHIP_COMM=rccl
    if (c->p2p_connected) return fail(c, -1, PPLHIP_INVALID_VALUE, "already connected");
    const int n = (int)c->ranks.size(), base = c->o.rank_base;
    for (int r = 0; r < n; ++r) {
        Rank& R = c->ranks[r];
        HIPCK(c, r, hipSetDevice(R.device));
        for (int g = 0; g < c->tp; ++g) {
            if (g >= base && g < base + n) {  // a rank of this process
                Rank& Q = c->ranks[g - base];
                if (Q.device != R.device) {
                    hipError_t e = hipDeviceEnablePeerAccess(Q.device, 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
                        (void)hipGetLastError();
                        const std::string why = std::string("peer access: ") + hipGetErrorString(e);
                        return p2p_selftest(c, &why);
                    }
                    (void)hipGetLastError();
                }
                R.peers.base[g] = Q.xbase;
                continue;
            }
            hipIpcMemHandle_t h;
            memcpy(&h, (const char*)all_handles + (size_t)g * PPLHIP_IPC_HANDLE_BYTES, sizeof(h));
            void* ptr = nullptr;
            hipError_t e = hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                const std::string why = std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e);
                return p2p_selftest(c, &why);
            }
            R.peers.base[g] = (char*)ptr;
            R.peer_ipc[g] = true;
        }
    }
    c->p2p_connected = true;
    return p2p_selftest(c);
}

int pplhip_comm_mode(pplhip_ctx* c) { return c ? c->comm_mode : PPLHIP_INVALID_VALUE; }
int pplhip_comm_fused_norm(pplhip_ctx* c) {
    if (!c || c->ranks.empty()) return PPLHIP_INVALID_VALUE;
    return fuse_norm_active(plan_settings(c, c->ranks[0]), c->ranks[0].dump_dev != nullptr) ? 1 : 0;
}

int pplhip_comm_info(pplhip_ctx* c, int64_t rows, pplhip_comm_info_t* out) {
    if (!c || !out) return PPLHIP_INVALID_VALUE;
    memset(out, 0, sizeof(*out));
    out->mode = c->comm_mode;
    out->selftest = c->selftest;
    out->has_rccl = !c->ranks.empty() && c->ranks[0].ch[0].comm != nullptr;
    out->dual_min_rows = c->dual_mode ? c->dual_min_rows : 0;
    out->dual_max_rows = c->dual_mode ? c->dual_max_rows : 0;
    // the schedule plan_step picks for a pure-decode step of `rows` rows (one token per request; no residual dump, no graph capture)
    static const int64_t held[1] = {0};   // "the rank holds a host copy of seq_starts": a pure-decode plan never reads it
    const pplhip_step_shape shape{rows, rows, rows, 0, held, 0, 0, 0};
    out->schedule = plan_step(plan_settings(c, c->ranks[0]), shape).schedule;
    snprintf(out->notes, sizeof(out->notes), "%s", c->comm_notes.c_str());
    return 0;
}

// one all-reduce of fp16 [rows, hidden], `iters` times back to back on the rank's stream, between two events.  Collective: every rank
// of the group calls it with the same arguments.  path 0: the collectives in use; 1: RCCL (when a communicator exists).
// The call enqueues AND synchronises: a context that holds several local ranks must call it from one thread per rank at the same time (like
// pplhip_run under ParallelExecute) -- rank by rank from one thread would wait for peers that were never enqueued.
int pplhip_comm_allreduce_us(pplhip_ctx* c, int rank, int64_t rows, int32_t iters, int32_t path, float* us) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size() || !us || iters < 1 || rows < 1) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    *us = -1.f;
    if (!c->tp_on || rows > R.cap_T) return PPLHIP_INVALID_VALUE;
    ncclComm_t rccl = R.ch[0].comm;
    if (path == 1 && !rccl) return 0;                // no RCCL communicator: nothing to compare with
    if (path == 0 && c->comm_mode != 2 && !rccl) return 0;
    HIPCK(c, rank, hipSetDevice(R.device));
    struct Ev {   // destroyed on every return path
        hipEvent_t e = nullptr;
        ~Ev() { if (e) (void)hipEventDestroy(e); }
    } ev0, ev1;
    HIPCK(c, rank, hipEventCreate(&ev0.e));
    HIPCK(c, rank, hipEventCreate(&ev1.e));
    hipEvent_t e0 = ev0.e, e1 = ev1.e;
    const int hd = c->d.hidden_dim;
    const Chunk k{0, rows, 0, rows, rows};
    Lane lane = make_lane(R, 0, 0);
    const uint16_t* norm_w = fuse_norm_active(plan_settings(c, R), R.dump_dev != nullptr) ? R.norm : nullptr;
    for (int it = -2; it < iters; ++it) {            // two warm-up rounds
        if (it == 0) HIPCK(c, rank, hipEventRecord(e0, R.stream));
        if (path == 1) NCCLCK(c, rank, ncclAllReduce(R.part, R.part, (size_t)rows * hd, ncclFloat16, ncclSum, rccl, R.stream));
        else if (int rc = chunk_allreduce(c, rank, lane, R.part, k, 0, false, norm_w)) return rc;   // what a step issues
    }
    HIPCK(c, rank, hipEventRecord(e1, R.stream));
    HIPCK(c, rank, hipStreamSynchronize(R.stream));
    float ms = 0.f;
    HIPCK(c, rank, hipEventElapsedTime(&ms, e0, e1));
    *us = ms * 1e3f / (float)iters;
    if (R.p2p_status && *R.p2p_status) return fail(c, rank, PPLHIP_DEVICE_RUNTIME_ERROR, "a direct collective timed out during pplhip_comm_allreduce_us");
    return 0;
}

// ---- pplhip_comm_op: the direct collectives as operators (include/pplhip.h) --------------------------------------------------------------
namespace {

constexpr size_t COMM_OP_SKEW_BYTES = (size_t)2 << 20;   // one skew copy moves this much inside the call's staging

// where an item's arrays sit in a rank's staging block (the same on every rank) and how large they are
struct CommOpPlace {
    size_t data = 0, image0 = 0, image1 = 0, w = 0, out0 = 0, out1 = 0;            // byte offsets
    size_t data_b = 0, image0_b = 0, image1_b = 0, w_b = 0;                       // bytes (out0 / out1: as image0 / image1; all-reduce: as data)
};

// the staging blocks of one call: freed, behind a synchronisation of every stream that may still use them, on every return path
struct CommOpStaging {
    pplhip_ctx* c;
    std::vector<char*> base;
    explicit CommOpStaging(pplhip_ctx* ctx) : c(ctx), base(ctx->ranks.size(), nullptr) {}
    ~CommOpStaging() {
        for (size_t r = 0; r < base.size(); ++r) {
            Rank& R = c->ranks[r];
            (void)hipSetDevice(R.device);
            (void)hipStreamSynchronize(R.stream);
            if (R.stream2) (void)hipStreamSynchronize(R.stream2);
            if (base[r]) (void)hipFree(base[r]);
        }
    }
};

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// the buffers of the fused form on a channel: a two-stream context gives each channel half of h and xn (its steps give each half-batch its rows)
size_t comm_op_image_cap(const pplhip_ctx* c, const Rank& R) {
    const size_t all = (size_t)R.cap_T * c->d.hidden_dim * 2;
    return R.stream2 ? all / 2 / 16 * 16 : all;
}

// PPLHIP_INVALID_VALUE with the reason, or 0 and the item's sizes
int comm_op_check(pplhip_ctx* c, const pplhip_comm_item& it, int idx, CommOpPlace& p) {
    const int n = c->tp;
    const Rank& R = c->ranks[0];
    auto bad = [&](const std::string& why) { return fail(c, -1, PPLHIP_INVALID_VALUE, "pplhip_comm_op: item " + std::to_string(idx) + ": " + why); };
    if (it.kind < PPLHIP_COMM_ALLREDUCE || it.kind > PPLHIP_COMM_ALLGATHER) return bad("kind");
    if (it.channel < 0 || it.channel >= P2P_CHANNELS) return bad("channel");
    if (it.channel == 1 && !R.stream2) return bad("channel 1 needs a context with two-stream decode");
    if (it.epoch_advance >= 0x80000000u) return bad("epoch_advance must stay below 2^31");
    if (!it.data || !it.out0) return bad("null array");
    const size_t data_cap = (size_t)R.cap_T * c->d.hidden_dim * 2, slice = R.x_slice_bytes;
    if (it.kind == PPLHIP_COMM_ALLREDUCE) {
        if (it.count < 8 || it.count % 8) return bad("count must be a positive multiple of 8");
        if (it.data_elems < it.count || (uint64_t)it.data_elems > data_cap / 2) return bad("the data buffer cannot hold it");
        const int64_t per = (it.count / 8 + n - 1) / n;
        if ((uint64_t)per * 16 > slice) return bad("the scratch slice cannot hold it");
        p.data_b = (size_t)it.data_elems * 2;
    } else if (it.kind == PPLHIP_COMM_ALLREDUCE_NORM) {
        if (it.rows < 1 || it.hidden < 8 || it.hidden % 8 || it.hidden > P2P_NORM_MAX_HIDDEN) return bad("rows >= 1, hidden a multiple of 8 up to 8192");
        if (it.rows > (int64_t)(data_cap / 2 / it.hidden)) return bad("the data buffer cannot hold it");
        const int64_t need = it.rows * it.hidden;
        if (it.data_elems != need) return bad("data_elems must be rows x hidden");
        if (it.image_elems < need || (uint64_t)it.image_elems > comm_op_image_cap(c, R) / 2) return bad("h / xn cannot hold it");
        const int64_t per = (it.rows + n - 1) / n;
        if ((uint64_t)per * it.hidden * 2 > slice) return bad("the scratch slice cannot hold it");
        if (!it.image0 || !it.image1 || !it.w || !it.out1) return bad("null array");
        p.data_b = (size_t)need * 2;
        p.image0_b = p.image1_b = (size_t)it.image_elems * 2;
        p.w_b = (size_t)it.hidden * 2;
    } else {
        if (it.channel != 0) return bad("the all-gather runs on channel 0");
        if (it.rows < 1 || it.cols < 2 || it.cols % 2 || it.dst_stride % 2) return bad("rows >= 1, cols and dst_stride even");
        if (it.cols > (int64_t)1 << 40 || it.dst_stride > (int64_t)1 << 40 || it.rows > (int64_t)1 << 20) return bad("shape");
        if (it.dst_stride < it.cols * n) return bad("dst_stride below ranks x cols");
        const int64_t need = it.rows * it.cols;
        if (it.data_elems != need || (uint64_t)need > (uint64_t)R.cap_B * c->vocab_local) return bad("the gather source cannot hold it");
        if (it.image_elems < (it.rows - 1) * it.dst_stride + it.cols * n || (uint64_t)it.image_elems > (uint64_t)R.cap_B * c->d.vocab_size)
            return bad("the gather target cannot hold it");
        if (!it.image0) return bad("null array");
        p.data_b = (size_t)need * 4;
        p.image0_b = (size_t)it.image_elems * 4;
    }
    for (int r = 0; r < n; ++r) {
        if (!it.data[r] || !it.out0[r] || (it.image0 && !it.image0[r])) return bad("null array");
        if (it.kind == PPLHIP_COMM_ALLREDUCE_NORM && (!it.image1[r] || !it.w[r] || !it.out1[r])) return bad("null array");
        if (it.skew && (it.skew[r] < 0 || it.skew[r] > 64)) return bad("skew must be 0 .. 64");
    }
    return 0;
}

void comm_op_counters(const pplhip_ctx* c, uint32_t* out) {
    if (!out || c->ranks.empty()) return;
    for (int ch = 0; ch < 2; ++ch) { out[ch] = c->ranks[0].ch[ch].p2p_epoch; out[2 + ch] = c->ranks[0].ch[ch].ar_count; }
}

}  // namespace

int pplhip_comm_op(pplhip_ctx* c, const pplhip_comm_op_args* a) {
    if (!c || !a) return PPLHIP_INVALID_VALUE;
    comm_op_counters(c, a->counters);
    const int n = (int)c->ranks.size();
    if (c->comm_mode != 2 || n != c->tp || n < 2) return fail(c, -1, PPLHIP_INVALID_VALUE, "pplhip_comm_op: needs the direct collectives with every rank in this process");
    if (a->n_items < 1 || a->n_items > 4096 || !a->items) return fail(c, -1, PPLHIP_INVALID_VALUE, "pplhip_comm_op: 1 .. 4096 items");
    // ---- everything that can be refused is refused here: nothing is enqueued, no counter has moved ----
    std::vector<CommOpPlace> place(a->n_items);
    size_t total = 2 * COMM_OP_SKEW_BYTES;
    bool gather_open = false;   // an all-gather that no all-reduce on channel 0 has followed yet (kernels.h, launch_p2p_allgather)
    for (int i = 0; i < a->n_items; ++i) {
        const pplhip_comm_item& it = a->items[i];
        CommOpPlace& p = place[i];
        if (int rc = comm_op_check(c, it, i, p)) return rc;
        if (it.kind == PPLHIP_COMM_ALLGATHER) {
            if (gather_open) return fail(c, -1, PPLHIP_INVALID_VALUE, "pplhip_comm_op: item " + std::to_string(i) +
                                         ": a second all-gather with no all-reduce on channel 0 since the first (its inputs would overwrite a source a peer may still read)");
            gather_open = true;
        } else if (it.channel == 0) {
            gather_open = false;
        }
        const size_t out0_b = it.kind == PPLHIP_COMM_ALLREDUCE ? p.data_b : p.image0_b;
        p.data = total;   total += up256(p.data_b);
        p.image0 = total; total += up256(p.image0_b);
        p.image1 = total; total += up256(p.image1_b);
        p.w = total;      total += up256(p.w_b);
        p.out0 = total;   total += up256(out0_b);
        p.out1 = total;   total += up256(p.image1_b);
    }
    // ---- staging: host -> device with synchronous copies, before any collective is enqueued (a copy that waited for a stream on which a
    //      collective waits for a peer that is not enqueued yet would wait with it) ----
    CommOpStaging st(c);
    for (int r = 0; r < n; ++r) {
        Rank& R = c->ranks[r];
        HIPCK(c, r, hipSetDevice(R.device));
        HIPCK(c, r, hipStreamSynchronize(R.stream));
        if (R.stream2) HIPCK(c, r, hipStreamSynchronize(R.stream2));
        HIPCK(c, r, hipMalloc((void**)&st.base[r], total));
        HIPCK(c, r, hipMemset(st.base[r], 0, 2 * COMM_OP_SKEW_BYTES));
        for (int i = 0; i < a->n_items; ++i) {
            const pplhip_comm_item& it = a->items[i];
            const CommOpPlace& p = place[i];
            HIPCK(c, r, hipMemcpy(st.base[r] + p.data, it.data[r], p.data_b, hipMemcpyHostToDevice));
            if (p.image0_b) HIPCK(c, r, hipMemcpy(st.base[r] + p.image0, it.image0[r], p.image0_b, hipMemcpyHostToDevice));
            if (p.image1_b) HIPCK(c, r, hipMemcpy(st.base[r] + p.image1, it.image1[r], p.image1_b, hipMemcpyHostToDevice));
            if (p.w_b) HIPCK(c, r, hipMemcpy(st.base[r] + p.w, it.w[r], p.w_b, hipMemcpyHostToDevice));
        }
        HIPCK(c, r, hipDeviceSynchronize());
    }
    // ---- the sequence: item by item, rank by rank, from this thread; device copies and kernels only ----
    for (int i = 0; i < a->n_items; ++i) {
        const pplhip_comm_item& it = a->items[i];
        const CommOpPlace& p = place[i];
        for (int r = 0; r < n; ++r) {
            Rank& R = c->ranks[r];
            Channel& ch = R.ch[it.channel];
            hipStream_t s = it.channel ? R.stream2 : R.stream;
            char* sb = st.base[r];
            HIPCK(c, r, hipSetDevice(R.device));
            for (int k = 0; it.skew && k < it.skew[r]; ++k)
                HIPCK(c, r, hipMemcpyAsync(sb + COMM_OP_SKEW_BYTES, sb, COMM_OP_SKEW_BYTES, hipMemcpyDeviceToDevice, s));
            // epoch_advance in steps of at most P2P_FLAG_REFRESH_EPOCHS: the counter gets there the way counting would take it, the
            // refresh of idle blocks' flag words included
            for (uint32_t left = it.epoch_advance; left;) {
                const uint32_t step = std::min(left, P2P_FLAG_REFRESH_EPOCHS);
                ch.p2p_epoch += step;
                left -= step;
                if (int rc = p2p_refresh_if_due(c, r, ch, s)) return rc;
            }
            uint32_t ep = 0;
            if (int rc = p2p_next_epoch(c, r, ch, s, &ep)) return rc;
            const size_t data_off = it.channel ? R.x_part2 : R.x_part;
            if (it.kind == PPLHIP_COMM_ALLGATHER) {
                HIPCK(c, r, hipMemcpyAsync(R.xbase + R.x_local, sb + p.data, p.data_b, hipMemcpyDeviceToDevice, s));
                HIPCK(c, r, hipMemcpyAsync(R.logits, sb + p.image0, p.image0_b, hipMemcpyDeviceToDevice, s));
                HIPCK(c, r, launch_p2p_allgather(s, R.peers, R.global_rank, n, R.x_local, R.logits, it.rows, it.cols * 4, it.dst_stride * 4, ep,
                                                 c->p2p_timeout_ticks, R.p2p_status));
                HIPCK(c, r, hipMemcpyAsync(sb + p.out0, R.logits, p.image0_b, hipMemcpyDeviceToDevice, s));
            } else if (it.kind == PPLHIP_COMM_ALLREDUCE) {
                HIPCK(c, r, hipMemcpyAsync(R.xbase + data_off, sb + p.data, p.data_b, hipMemcpyDeviceToDevice, s));
                HIPCK(c, r, launch_p2p_allreduce(s, R.peers, R.global_rank, n, data_off, ch.x_scratch[ch.ar_count++ & 1], it.count, ep,
                                                 c->p2p_timeout_ticks, R.p2p_status, ch.id));
                HIPCK(c, r, hipMemcpyAsync(sb + p.out0, R.xbase + data_off, p.data_b, hipMemcpyDeviceToDevice, s));
            } else {
                const size_t img_off = it.channel ? comm_op_image_cap(c, R) : 0;
                uint16_t* h = (uint16_t*)((char*)R.h + img_off);
                uint16_t* xn = (uint16_t*)((char*)R.xn + img_off);
                HIPCK(c, r, hipMemcpyAsync(R.xbase + data_off, sb + p.data, p.data_b, hipMemcpyDeviceToDevice, s));
                HIPCK(c, r, hipMemcpyAsync(h, sb + p.image0, p.image0_b, hipMemcpyDeviceToDevice, s));
                HIPCK(c, r, hipMemcpyAsync(xn, sb + p.image1, p.image1_b, hipMemcpyDeviceToDevice, s));
                HIPCK(c, r, launch_p2p_allreduce_norm(s, R.peers, R.global_rank, n, data_off, ch.x_scratch[ch.ar_count++ & 1], it.rows, (int)it.hidden, h,
                                                      (const uint16_t*)(sb + p.w), it.eps, xn, ep, c->p2p_timeout_ticks, R.p2p_status, ch.id));
                HIPCK(c, r, hipMemcpyAsync(sb + p.out0, h, p.image0_b, hipMemcpyDeviceToDevice, s));
                HIPCK(c, r, hipMemcpyAsync(sb + p.out1, xn, p.image1_b, hipMemcpyDeviceToDevice, s));
            }
        }
    }
    comm_op_counters(c, a->counters);
    // ---- every rank, then the status words: all of them are cleared, the first one raised is reported ----
    for (int r = 0; r < n; ++r) {
        Rank& R = c->ranks[r];
        HIPCK(c, r, hipSetDevice(R.device));
        HIPCK(c, r, hipStreamSynchronize(R.stream));
        if (R.stream2) HIPCK(c, r, hipStreamSynchronize(R.stream2));
    }
    int bad_rank = -1;
    uint32_t bad_word = 0;
    for (int r = 0; r < n; ++r) {
        Rank& R = c->ranks[r];
        if (*R.p2p_status && bad_rank < 0) { bad_rank = r; bad_word = *R.p2p_status; }
        *R.p2p_status = 0;
    }
    if (bad_rank >= 0)
        return fail(c, -1, PPLHIP_DEVICE_RUNTIME_ERROR, "pplhip_comm_op: rank " + std::to_string(bad_rank) + " raised status word " + std::to_string(bad_word) +
                    " (a wait for rank " + std::to_string((bad_word - 1) & 15) + ((bad_word - 1) & 16 ? ", end barrier," : ", start barrier,") + " ran out)");
    for (int r = 0; r < n; ++r) {
        Rank& R = c->ranks[r];
        HIPCK(c, r, hipSetDevice(R.device));
        for (int i = 0; i < a->n_items; ++i) {
            const pplhip_comm_item& it = a->items[i];
            const CommOpPlace& p = place[i];
            HIPCK(c, r, hipMemcpy(it.out0[r], st.base[r] + p.out0, it.kind == PPLHIP_COMM_ALLREDUCE ? p.data_b : p.image0_b, hipMemcpyDeviceToHost));
            if (p.image1_b) HIPCK(c, r, hipMemcpy(it.out1[r], st.base[r] + p.out1, p.image1_b, hipMemcpyDeviceToHost));
        }
    }
    return 0;
}
