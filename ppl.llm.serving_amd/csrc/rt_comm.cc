// The direct collectives (k_comm.hip) as the runtime sets them up: mapping the peers' exchange regions (in this process or over IPC
// handles), the start-up self-test that decides between them and RCCL, and the pplhip_comm_* entry points.  What a step does with them
// (chunk_allreduce, the stream hand-offs of the two-chunk schedule) is in pplhip.cc.
#include "rt_internal.h"

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
            HIPCK(c, r, launch_p2p_allreduce(R.stream, R.peers, R.global_rank, tp, R.x_part, ch.x_scratch[ch.ar_count++ & 1], cnt, ++ch.p2p_epoch,
                                             ticks, R.p2p_status));
            HIPCK(c, r, launch_p2p_allgather(R.stream, R.peers, R.global_rank, tp, R.x_local, R.logits, grows, gcols * 4, (int64_t)gcols * 4 * tp,
                                             ++ch.p2p_epoch, ticks, R.p2p_status));
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
                HIPCK(c, r, launch_p2p_allreduce(R.stream, R.peers, R.global_rank, tp, R.x_part, ch.x_scratch[ch.ar_count++ & 1], fcnt, ++ch.p2p_epoch, ticks, R.p2p_status));
                HIPCK(c, r, launch_p2p_pattern(R.stream, R.h, fcnt, nullptr, 0, 17, round + 4));    // the residual stream: the same on every rank
                HIPCK(c, r, launch_p2p_pattern(R.stream, w, hd, nullptr, 0, 23, round + 4));
                HIPCK(c, r, hipMemcpyAsync(href, R.h, (size_t)fcnt * 2, hipMemcpyDeviceToDevice, R.stream));
                HIPCK(c, r, launch_p2p_allreduce_norm(R.stream, R.peers, R.global_rank, 1, R.x_part, 0, frows, hd, href, w, c->d.norm_eps, xref, 0, ticks, R.p2p_status));
                HIPCK(c, r, launch_p2p_pattern(R.stream, R.part, fcnt, nullptr, 0, R.global_rank, round + 4));
                HIPCK(c, r, launch_p2p_allreduce_norm(R.stream, R.peers, R.global_rank, tp, R.x_part, ch.x_scratch[ch.ar_count++ & 1], frows, hd, R.h, w, c->d.norm_eps,
                                                      R.xn, ++ch.p2p_epoch, ticks, R.p2p_status));
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
