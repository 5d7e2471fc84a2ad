// Host-callable launchers of the hand-written gfx950 kernels.  All pointers are device pointers, all
// launches are asynchronous on `stream`.  Return value: hipError_t of the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_common.h"
#include "linear_plan.h"

namespace pplhip {

// A split-K GEMM result that has NOT been reduced yet: y[m][n] = fp16( (sum_z ws[(z M + m) N + n]) * scale[n] ) (scale NULL: 1).  The tile
// kernels hand it to the kernel that consumes y anyway -- (Skip)RMSNorm for wo / w2, RoPE + KV write for wqkv -- instead of launching
// splitk_reduce_kernel: one ~5 us kernel and one kernel boundary less per linear of a small-batch step (round 4).  Same arithmetic, same
// summation order, same fp16 rounding as the reduce kernel: bit-identical results.
struct SplitSlabs {
    const float* ws = nullptr;
    int splits = 0;              // 0: nothing deferred (y was written)
    const uint16_t* scale = nullptr;
    int N = 0;
    int64_t M = 0;
};
// Route record of the linear launchers (pplhip_op_linear_ex, for the tests): the path a launch_linear call takes, as "key=value" tokens
// -- the first names the __global__ template and its template arguments; an M-split gives two groups separated by " ; ".  dry: decide the
// route exactly as a launch would and return the same status, but make no HIP call at all (no launch, no hipGetDevice, no attribute set).
struct LinearRoute {
    char* buf = nullptr;   // NUL-terminated text (may be null: only `dry` is used)
    int cap = 0;
    int len = 0;
    bool dry = false;
    void add(const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // one token, space-separated from the previous one
};
#ifdef __HIPCC__
// 8 consecutive outputs n .. n + 7 of row m, as fp16-rounded floats
__device__ __forceinline__ void slab_load8(const SplitSlabs& sl, int64_t m, int n, float* o) {
    // every slab's 32 bytes are requested before the first sum (one memory latency, not `splits` of them: a consumer row is one
    // workgroup); slabs past `splits` re-read slab 0 and are not added.  Summation order z = 0, 1, ... like splitk_reduce_kernel.
    const float* p = sl.ws + m * sl.N + n;
    const int64_t zs = sl.M * sl.N;
    float4 c[8], d[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) {
        const float* q = p + (z < sl.splits ? z : 0) * zs;
        c[z] = *reinterpret_cast<const float4*>(q);
        d[z] = *reinterpret_cast<const float4*>(q + 4);
    }
    float4 a = c[0], b = d[0];
#pragma unroll
    for (int z = 1; z < 8; ++z) {
        if (z < sl.splits) {
            a.x += c[z].x; a.y += c[z].y; a.z += c[z].z; a.w += c[z].w;
            b.x += d[z].x; b.y += d[z].y; b.z += d[z].z; b.w += d[z].w;
        }
    }
    if (sl.scale) {
        const h8 sh = __builtin_bit_cast(h8, *reinterpret_cast<const uint4*>(sl.scale + n));
        a.x *= (float)sh[0]; a.y *= (float)sh[1]; a.z *= (float)sh[2]; a.w *= (float)sh[3];
        b.x *= (float)sh[4]; b.y *= (float)sh[5]; b.z *= (float)sh[6]; b.w *= (float)sh[7];
    }
    o[0] = round_h(a.x); o[1] = round_h(a.y); o[2] = round_h(a.z); o[3] = round_h(a.w);
    o[4] = round_h(b.x); o[5] = round_h(b.y); o[6] = round_h(b.z); o[7] = round_h(b.w);
}
#endif

// ---- k_elem.hip -------------------------------------------------------------------------------
hipError_t launch_embedding(hipStream_t s, const int64_t* token_ids, const uint16_t* table, int64_t T, int hidden,
                            uint16_t* out);
// out[r] = rmsnorm(x[src(r)] (+ skip[src(r)])) * w.  gather_seq_starts != NULL: src(r) = seq_starts[r+1]-1
// (last-token gather of K11), else src(r) = r.  residual_out (optional) receives fp16(x + skip) at row r.
hipError_t launch_rmsnorm(hipStream_t s, const uint16_t* x, const uint16_t* skip, const uint16_t* w, float eps,
                          int64_t rows, int hidden, const int64_t* gather_seq_starts, uint16_t* out,
                          uint16_t* residual_out, int8_t* qout = nullptr, float* sx = nullptr,
                          const SplitSlabs* skip_slabs = nullptr,   // skip_slabs: the skip operand as unreduced split-K slabs
                          bool q_fp8 = false);  // qout / sx: int8 rows and max|y| / 127 (online_i8i8), or e4m3fn rows and 2^e (online_f8f8)
// the instantiation rmsnorm_kernel<maxc, nt> a launch of (rows, hidden) takes and the status it returns (rows == 0: success, no launch,
// maxc 0): a pure function, no HIP call.  wide_max_rows: rmsnorm_wide_max_rows() in the product (PPLHIP_RMSNORM_WIDE_MAX_ROWS, read once)
struct RmsnormForm {
    int maxc = 0, nt = 0;
};
hipError_t rmsnorm_form(int64_t rows, int hidden, int wide_max_rows, RmsnormForm* f);
int rmsnorm_wide_max_rows();
hipError_t launch_silu_mul(hipStream_t s, const uint16_t* gate_up, int64_t T, int inter, uint16_t* out);
// out[r] = x[seq_starts[r + 1] - 1] (last-token gather of K11 when the final norm already ran on every row: fused tensor-parallel norm)
hipError_t launch_gather_last_rows(hipStream_t s, const uint16_t* x, const int64_t* seq_starts, int64_t B, int hidden, uint16_t* out);

// The KV-cache kernels take the cache format kv_fmt (KV_FP16 / KV_I8G8 / KV_FP8 / KV_I4G32, k_common.h).
// ---- k_rope_kv.hip ----------------------------------------------------------------------------
hipError_t launch_rope_kv_write(hipStream_t s, uint16_t* qkv, const float* cos_sin, const KvAddr& kv, int kv_fmt,
                                const int64_t* seq_starts, const int64_t* start_pos,
                                const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t t0, int64_t T, int H,
                                int Hkv, int D, const SplitSlabs* qkv_slabs = nullptr);  // token rows [t0, t0 + T) of the step's B requests;
                                                   // qkv_slabs: the rows come from unreduced split-K slabs of a [T, N] launch (slab row = token row - t0); rotated q -> qkv

// ---- k_attn_decode.hip ------------------------------------------------------------------------
// rows [0, nb) of the batch are single-token queries; q row of request b is qkv row seq_starts[b].
// split > 1 uses `workspace` (fp32 [nb, H, split, D+2]).
size_t attn_decode_workspace_bytes(int64_t nb, int H, int D, int split);
hipError_t launch_attn_decode(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt,
                              const int64_t* seq_starts, const int64_t* start_pos, const int64_t* cache_indices,
                              int64_t max_pages, int64_t nb, int H, int Hkv, int D, int64_t max_kv_len, int split,
                              int threads, float* workspace, uint16_t* out, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);
// merges the `nsplit` partial rows of each of n_row_heads (row, head) pairs of `ws` ([row][head][split][D + 2] floats) into out
// ([row][head][D] fp16): the end of every split launch -- both decode kernels and the split-KV prefill
hipError_t launch_attn_reduce(hipStream_t s, const float* ws, int nsplit, int64_t n_row_heads, int D, uint16_t* out);

// ---- k_attn_prefill.hip -----------------------------------------------------------------------
// requests [b0, B): causal attention of their new tokens over the cache [0, start_pos + seqlen).
hipError_t launch_attn_prefill(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt,
                               const int64_t* seq_starts, const int64_t* start_pos, const int64_t* cache_indices,
                               int64_t max_pages, int64_t b0, int64_t B, int H, int Hkv, int D, int64_t max_seq_len,
                               uint16_t* out, int64_t max_kv_len = 0, float* ws = nullptr, size_t ws_bytes = 0, int64_t row0 = 0,
                               int64_t nrows = 0);  // max_kv_len .. nrows: optional, enable the split-KV form for short suffixes (k_attn_prefill32.hip)

// ---- k_attn_prefill32.hip ---------------------------------------------------------------------
// the same operation for head_dim 128 on the 32-row wave tile (mfma_f32_32x32x16_f16, 64-key tiles, one barrier per tile)
hipError_t launch_attn_prefill32(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt, const int64_t* seq_starts,
                                 const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t b0, int64_t B,
                                 int H, int Hkv, int D, int64_t max_seq_len, uint16_t* out, int64_t max_kv_len = 0, float* ws = nullptr,
                                 size_t ws_bytes = 0, int64_t row0 = 0, int64_t nrows = 0);

// ---- k_attn_decode_gqa.hip --------------------------------------------------------------------
// grouped-query decode (4 <= H/Hkv <= 16): MFMA kernel, one block per (request, KV head[, split]); same workspace layout
// and reduce (launch_attn_reduce, run by the caller) as launch_attn_decode.  t0 / t1: optional start / stop events of the kernel's own dispatch packet.
bool attn_decode_gqa_supported(int kv_fmt, int H, int Hkv, int D);
hipError_t launch_attn_decode_gqa(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt,
                                  const int64_t* seq_starts, const int64_t* start_pos, const int64_t* cache_indices,
                                  int64_t max_pages, int64_t nb, int H, int Hkv, int D, int split, float* workspace,
                                  uint16_t* out, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr);

// ---- k_gemm.hip -------------------------------------------------------------------------------
// y[M,N] = x[M,K] . W[N,K]^T (+ per-channel / per-group scales).  wq_bit 0/8/4.  out_fp32: y is float.
// ldy = row stride of y in elements.  ws (optional, fp32 scratch) enables split-K at small M.
// swiglu: the weight rows are interleaved (gate_i, up_i) and y[M, N/2] = silu(gate) * up (fused K10).
// W8A16 128 (m) x 384 (n) tile kernel (k_gemm_wide.hip); K % 64 == 0, N % 4 == 0; epi 0 fp16 / 1 fp32 / 2 fused SwiGLU
hipError_t launch_linear_w8_wide(hipStream_t s, const uint16_t* x, const int8_t* w, const uint16_t* scale, int64_t M, int N, int K, void* y,
                                 int64_t ldy, int epi, int nc, LinearRoute* route = nullptr);
// W4A16 (group 128) on 128 (m) x 64 (n) tiles, no K slabs (k_gemm_pc.hip): a few hundred rows; epi 0 fp16 / 2 fused SwiGLU
hipError_t launch_linear_w4_pc(hipStream_t s, const uint16_t* x, const void* w, const uint16_t* scale, int64_t M, int N, int K, void* y,
                               int64_t ldy, int epi, LinearRoute* route = nullptr);
// (which of them takes a problem: plan_linear, linear_plan.h -- with gemv_stream_max_m, linear_w8_wide_waves and linear_w4_pc_supported)
hipError_t launch_linear(hipStream_t s, const uint16_t* x, const void* w, const uint16_t* scale, int wq_bit, int group,
                         int64_t M, int N, int K, void* y, int64_t ldy, bool out_fp32, float* ws = nullptr, size_t ws_bytes = 0,
                         bool swiglu = false, SplitSlabs* defer = nullptr,   // defer: a split-K launch leaves its slabs unreduced there
                         LinearRoute* route = nullptr);                      // route: the path taken (tests); null: no record
// y = (sum of `splits` fp32 slabs [M][N] at ws) * scale (NULL: 1), epilogue epi (0 fp16 / 1 fp32 / 2 fused SwiGLU)
hipError_t launch_splitk_reduce(hipStream_t s, const float* ws, int splits, int64_t M, int N, const uint16_t* scale, void* y, int64_t ldy, int epi);
// ---- k_gemv.hip: streaming GEMV, 1 <= M <= 4 (whole 1-KiB row pieces per wave-load; VALU dot products) ----------------------------
hipError_t launch_gemv_stream(hipStream_t s, const uint16_t* x, const void* w, const uint16_t* scale, int wq_bit, int group, int64_t M, int N,
                              int K, void* y, int64_t ldy, int epi, LinearRoute* route = nullptr);
// ---- k_gemm_i8.hip: online_i8i8 (W8A8) ------------------------------------------------------------
// per-token int8 activations: q [M, ldq] (columns K..ldq-1 zeroed), sx [M] = max|x| / 127
hipError_t launch_quant_act(hipStream_t s, const uint16_t* x, int64_t M, int K, int64_t ldx, int8_t* q, int64_t ldq, float* sx);
// per-output-row int8 weights from an fp16 [N, K] matrix: q [N, ldq], scale [N] fp16
hipError_t launch_quant_weight(hipStream_t s, const uint16_t* w, int N, int K, int8_t* q, int64_t ldq, uint16_t* scale);
// y[M,N] = fp16/fp32( (sum_k xq * w) * sx[m] * scale[n] ); K = row stride of xq and w (K % 16 == 0)
// (which kernel takes a problem: plan_linear_q8, linear_plan.h; route: the path taken (tests), null: no record)
hipError_t launch_linear_i8(hipStream_t s, const int8_t* xq, const float* sx, const int8_t* w, const uint16_t* scale, int64_t M, int N,
                            int K, void* y, int64_t ldy, bool out_fp32, bool swiglu, LinearRoute* route = nullptr);
// online_f8f8 (fp8 e4m3fn W8A8): per-row codes under one power-of-two scale (the fp8 KV row rule, k_common.h fp8_row_exp / fp8_quant)
// activations: q [M, ldq] (columns K..ldq-1 zeroed), sx [M] = 2^e (fp32)
hipError_t launch_quant_act_f8(hipStream_t s, const uint16_t* x, int64_t M, int K, int64_t ldx, uint8_t* q, int64_t ldq, float* sx);
// weights from an fp16 [N, K] matrix: q [N, ldq], scale [N] = fp16(2^e)
hipError_t launch_quant_weight_f8(hipStream_t s, const uint16_t* w, int N, int K, uint8_t* q, int64_t ldq, uint16_t* scale);
// y[M,N] = fp16/fp32( (sum_k xq * w) * sx[m] * scale[n] ), fp32 sums; K = row stride of xq and w (K % 16 == 0)
hipError_t launch_linear_f8(hipStream_t s, const uint8_t* xq, const float* sx, const uint8_t* w, const uint16_t* scale, int64_t M, int N,
                            int K, void* y, int64_t ldy, bool out_fp32, bool swiglu, LinearRoute* route = nullptr);
// dst row r = src row perm(r): r even -> r/2 (gate), r odd -> half + r/2 (up).  row_bytes % 4 == 0.
hipError_t launch_interleave_rows(hipStream_t s, const void* src, void* dst, int rows, int64_t row_bytes);

// ---- k_lora.hip: multi-LoRA, the low-rank update of a layer linear on the rows whose request carries an adapter --------------------
constexpr int LORA_MAX_SLOTS = 64, LORA_MAX_RANK = 128;   // PPLHIP_LORA_MAX_SLOTS / PPLHIP_LORA_MAX_RANK
// up to 16 token rows that share adapter slot `slot`; row[i] = -1 marks padding.  Built on the host (rt_lora.cc lora_build_tiles).
struct LoraTile {
    int32_t slot;
    int32_t n;          // rows in use (the first n of row[])
    int32_t row[16];
};
// one slot's factors for ONE target linear: a [rp, K] and b [N, rp] fp16 with the rank zero-padded to rp (a multiple of 16);
// a == NULL: the adapter leaves this linear alone
struct LoraSlot {
    const uint16_t* a;
    const uint16_t* b;
    int32_t rp;
    float scale;
};
// t[tile][16][LORA_MAX_RANK] = fp16(x rows . a^T), then y rows += scale * t . b^T in place (fp16(fp32(y) + scale * sum)); slots: device
// LoraSlot [LORA_MAX_SLOTS]; t: device scratch of ntiles * 16 * LORA_MAX_RANK fp16.  K % 32 == 0, N % 16 == 0, ldx % 8 == 0, x 16-byte aligned
hipError_t launch_lora(hipStream_t s, const LoraTile* tiles, int ntiles, const LoraSlot* slots, const uint16_t* x, int64_t ldx, uint16_t* y,
                       int64_t ldy, int N, int K, uint16_t* t);

// ---- k_comm.hip ------------------------------------------------------------------------------
// direct (all-links) tensor-parallel collectives over peer-mapped exchange regions; see the file header.
constexpr int P2P_MAX_RANKS = 8;
constexpr int P2P_MAX_BLOCKS = 64;
// exchange-region layout (bytes, identical on every rank): flag words first, data buffers after P2P_DATA_START
constexpr size_t P2P_FLAGS_START = 0;                                         // uint32 [P2P_MAX_BLOCKS][P2P_MAX_RANKS]
constexpr size_t P2P_FLAGS_MID = (size_t)P2P_MAX_BLOCKS * P2P_MAX_RANKS * 4;  // uint32 [P2P_MAX_BLOCKS][P2P_MAX_RANKS]
// two channels (flag sets): collectives of different channels may be in flight at the same time (the two half-batches of a two-stream
// decode step, pplhip.cc run_launches); channel c's words sit P2P_CHANNEL_FLAG_BYTES x c further on
constexpr int P2P_CHANNELS = 2;
constexpr size_t P2P_CHANNEL_FLAG_BYTES = (size_t)2 * P2P_MAX_BLOCKS * P2P_MAX_RANKS * 4;
constexpr size_t P2P_DATA_START = 8192;
static_assert(P2P_CHANNELS * P2P_CHANNEL_FLAG_BYTES <= P2P_DATA_START, "flag words of every channel in front of the data");
// A flag word belongs to ONE block index, and a collective of b blocks only raises the words of blocks 0 .. b-1: the words of higher
// blocks stay where the last large collective left them.  Epochs are compared with (int32_t)(flag - epoch) < 0, which is right only
// while a word lags its channel's counter by at most 2^31 -- a word that small collectives leave behind for longer compares as AHEAD,
// and the block of the next large collective would pass its barriers without its peers.  So every P2P_FLAG_REFRESH_EPOCHS epochs of
// a channel the runtime (p2p_next_epoch, rt_comm.cc) launches launch_p2p_flag_refresh on the stream in front of the next collective: it
// lifts every word of the rank's OWN region (the words its own blocks wait on) that is behind the counter's value `epoch` to it.  Every
// collective up to `epoch` of this rank is complete by then (stream order), so no block still waits for such a value, and every later
// one waits for more.  A word that is ahead -- a peer has already entered a later collective -- is kept, also when the peer's store lands
// between the load and the store here (compare-and-swap).  Behind and ahead are told apart by the same signed comparison: between two
// refreshes the counter moves by less than 2^31 (pplhip_comm_op, which can move it in jumps, jumps by at most the refresh period).
constexpr uint32_t P2P_FLAG_REFRESH_EPOCHS = 1u << 30;
struct P2pPeers {
    char* base[P2P_MAX_RANKS];  // exchange region of every rank as mapped in this process (base[me] is the local one)
};
hipError_t launch_p2p_flag_refresh(hipStream_t s, char* my_base, int channel, uint32_t epoch);
// all-reduce(sum) of fp16[count] at byte offset data_off of every rank's region (count % 4 == 0); scratch_off: a region
// offset with room for ceil(count / n) fp16 that no other collective in flight uses
hipError_t launch_p2p_allreduce(hipStream_t s, const P2pPeers& peers, int me, int n, size_t data_off, size_t scratch_off, int64_t count,
                                uint32_t epoch, uint64_t timeout_ticks, uint32_t* status, int channel = 0);   // epochs count per channel
// The same all-reduce fused with the residual add + RMSNorm that consumes it (sequence-parallel residual stream, k_comm.hip): `rows` rows of
// fp16 [rows, hidden] partial sums at data_off of every rank's region; rank `me` owns rows [me per, (me + 1) per), per = ceil(rows / n): on those
// it computes s = fp16(sum over ranks), h = fp16(h + s) (h: LOCAL residual rows, only the owned ones are read or written) and
// y = rmsnorm(h) * w; every rank ends with all rows of y in the local matrix xn.  scratch_off: room for per rows.  n == 1: local reference
// form (no peers, no barriers, every row owned; reads data_off of the own region).  hidden <= P2P_NORM_MAX_HIDDEN, hidden % 8 == 0
constexpr int P2P_NORM_MAX_HIDDEN = 8192;
hipError_t launch_p2p_allreduce_norm(hipStream_t s, const P2pPeers& peers, int me, int n, size_t data_off, size_t scratch_off, int64_t rows,
                                     int hidden, uint16_t* h, const uint16_t* w, float eps, uint16_t* xn, uint32_t epoch, uint64_t timeout_ticks,
                                     uint32_t* status, int channel = 0);
// rows x row_bytes at src_off of every rank's region (rank r's column block) -> columns [r * row_bytes, ...) of the local
// [rows, dst_row_bytes] matrix dst (ordinary memory)
// Sequence rule: the all-gather has a start barrier and NO end barrier -- a rank that leaves the kernel knows nothing about its peers'
// reads of ITS shard.  So nothing may rewrite the source at src_off before a later all-reduce (plain or fused) of channel 0 on the same
// stream: passing that one's start barrier means every peer has left the all-gather.  A step keeps the rule by itself (the next lm_head
// writes the shards behind a whole step's all-reduces); pplhip_comm_op refuses a sequence that breaks it.
hipError_t launch_p2p_allgather(hipStream_t s, const P2pPeers& peers, int me, int n, size_t src_off, void* dst, int64_t rows,
                                int64_t row_bytes, int64_t dst_row_bytes, uint32_t epoch, uint64_t timeout_ticks, uint32_t* status);

// stream hand-off through a device-memory epoch (k_comm.hip): signal = one-thread kernel after the producer; wait = one-wave kernel
// in front of the consumer (bounded spin; optionally raises a second flag when the wait is over)
hipError_t launch_handoff_signal(hipStream_t s, uint32_t* flag, uint32_t epoch);
hipError_t launch_handoff_wait(hipStream_t s, const uint32_t* wait_flag, uint32_t wait_epoch, uint32_t* done_flag, uint32_t done_epoch,
                               uint64_t timeout_ticks, uint32_t* status);

// self-test patterns: halfs[i] = value(i, g, round), floats[i] = value(i, g, round + 2)
float p2p_pattern_value(int64_t i, int g, int round);
hipError_t launch_p2p_pattern(hipStream_t s, uint16_t* halfs, int64_t cnt, float* floats, int64_t gcnt, int g, int round);

// ---- k_sample.hip -----------------------------------------------------------------------------
hipError_t launch_sample_greedy(hipStream_t s, const float* logits, const float* temperatures, int batch, int vocab,
                                int stride, int32_t* out_tok, float* out_logprob);
size_t sample_topk_workspace_bytes(int batch, int vocab, int top_k);
hipError_t launch_sample_topk_topp(hipStream_t s, const float* logits, const float* temperatures, const float* top_p,
                                   const float* rnd, int batch, int vocab, int stride, int top_k, float default_top_p,
                                   void* workspace, int32_t* out_tok, float* out_logprob);
hipError_t launch_penalty(hipStream_t s, float* logits, const float* temperatures, const float* rep,
                          const float* presence, const float* frequency, const int64_t* batch_slots,
                          const int64_t* token_inputs, const int64_t* seq_starts, const int64_t* start_pos, int batch,
                          int vocab, int stride, int decoding_batches, uint16_t* count_map);

// ---- k_sample_rows.hip: the per-request sampler ---------------------------------------------------
// rows: device list of batch rows, the n_greedy rows with top_k == 1 first, then the n_sampling others; every other array is indexed by
// the batch row.  temperatures may be NULL; rnd != NULL replaces u(seeds, draws).  One launch per non-empty kind.
// Behind the n_sampling rows the list holds the n_trunc truncating rows (top_k != 1 with min_p or typical_p on, row_min_p / row_typical_p below); min_p /
// typical_p may be NULL (off for every row).
hipError_t launch_sample_rows(hipStream_t s, const float* logits, const float* temperatures, const int32_t* top_k, const float* top_p,
                              const uint64_t* seeds, const uint64_t* draws, const float* rnd, const int32_t* rows, int n_greedy,
                              int n_sampling, int vocab, int stride, int32_t* out_tok, float* out_logprob, const float* min_p = nullptr,
                              const float* typical_p = nullptr, int n_trunc = 0);
// The defaults of the two truncations, one rule for the host's row list and the kernel: min_p is off (0) when it is <= 0 or NaN and counts
// as 1 above 1; typical_p is off (0) when it is <= 0, >= 1 or NaN.  A row with top_k == 1 is greedy whatever else it carries; a row with
// both off is a sampling row (sample_topk_topp_row answers it); every other row is a truncating row (sample_trunc_row).
__host__ __device__ inline float row_min_p(float v) { return v > 0.f ? (v < 1.f ? v : 1.f) : 0.f; }
__host__ __device__ inline float row_typical_p(float v) { return (v > 0.f && v < 1.f) ? v : 0.f; }
// out_u[b] = u(seeds[b], draws[b]): Philox4x32-10, word 0, 24 bits
hipError_t launch_sample_uniform(hipStream_t s, const uint64_t* seeds, const uint64_t* draws, int batch, float* out_u);

// ---- k_logprobs.hip: top-N logprobs ---------------------------------------------------------------
// rows: device list of the n_rows batch rows with num_logprobs[b] in 1 .. 20, ascending; num_logprobs and temperatures (may be NULL) are
// indexed by the batch row, out_tok / out_logprob [n_rows, 20] by the place in the list.  No rows: no launch.
constexpr int TOP_LOGPROBS_MAX = 20;   // slots per asked row (PPLHIP_TOP_LOGPROBS_MAX)
hipError_t launch_top_logprobs(hipStream_t s, const float* logits, const float* temperatures, const int32_t* num_logprobs,
                               const int32_t* rows, int n_rows, int vocab, int stride, int32_t* out_tok, float* out_logprob);

// ---- k_logit_rules.hip: per-request logit rules ------------------------------------------------------
// The rule table, one record per batch slot, as five device arrays with their own strides (in elements) from one slot to the next:
// head [slot] = {n_bias, n_stop, has_mask, 0}; bias_tok / bias_val [slot, <= 512]; stops [slot, <= 64]; mask [slot, ceil(V / 32)] with
// token v at bit v & 31 of word v >> 5.
constexpr int LOGIT_BIAS_MAX = 512;   // PPLHIP_LOGIT_BIAS_MAX
constexpr int LOGIT_STOP_MAX = 64;    // PPLHIP_LOGIT_STOP_MAX
struct LogitRuleTable {
    const int32_t* head;
    const int32_t* bias_tok;
    const float* bias_val;
    const int32_t* stops;
    const uint32_t* mask;
    int64_t head_stride, bias_stride, stop_stride, mask_stride;
};
// rows: device list of the n_rows batch rows with flags[b] != 0; slots and flags (bit 0: mask and bias, bit 1: suppress the stops) are
// indexed by the batch row.  Edits logits[b * stride + 0 .. vocab) of the listed rows in place.  No rows: no launch.
hipError_t launch_logit_edit(hipStream_t s, float* logits, int stride, int vocab, const int32_t* rows, int n_rows, const int32_t* slots,
                             const uint32_t* flags, const LogitRuleTable& table);

// ---- k_guide.hip: guided decoding ------------------------------------------------------------------
// A guide is a byte-level DFA: trans [n_states, 256] names the next state, GUIDE_DEAD the dead one (it has no row); accept [n_states].
// Its mask [n_states, mask_stride] words holds one allowed-token row per state, token v at bit v & 31 of word v >> 5.
constexpr int GUIDE_MAX_SLOTS = 16;     // PPLHIP_GUIDE_MAX_SLOTS
constexpr int GUIDE_MAX_STATES = 255;   // PPLHIP_GUIDE_MAX_STATES: live states 0 .. 254
constexpr int GUIDE_DEAD = 255;
struct GuideTable {
    const uint32_t* mask[GUIDE_MAX_SLOTS];   // NULL: the slot is empty
    int64_t mask_stride;                     // words from one state's row to the next, the same in every slot
};
// The vocabulary is tok_bytes with token t at [tok_off[t], tok_off[t + 1]), t < n_tok <= vocab; end_tokens [n_end] are allowed exactly in
// accepting states.  Writes words 0 .. ceil(vocab / 32) - 1 of every state's mask row and ORs 1 into any[s] (zeroed by the caller) when
// state s allows some token.  n_states <= GUIDE_MAX_STATES.
hipError_t launch_guide_build(hipStream_t s, const uint8_t* trans, const uint8_t* accept, int n_states, const uint8_t* tok_bytes,
                              const int64_t* tok_off, int n_tok, const int32_t* end_tokens, int n_end, int vocab, uint32_t* mask,
                              int64_t mask_stride, uint32_t* any);
// The wide guide: trans is uint16 [n_states, 256], GUIDE16_DEAD the dead state, n_states <= GUIDE16_MAX_STATES; everything else as above.
// The grid is (token block, chunk of GUIDE16_STATE_CHUNK states); a next state at or behind n_states counts as dead.
constexpr int GUIDE16_MAX_STATES = 4096;   // PPLHIP_GUIDE16_MAX_STATES: live states 0 .. 4095
constexpr int GUIDE16_DEAD = 0xFFFF;
constexpr int GUIDE16_STATE_CHUNK = 64;
hipError_t launch_guide_build16(hipStream_t s, const uint16_t* trans, const uint8_t* accept, int n_states, const uint8_t* tok_bytes,
                                const int64_t* tok_off, int n_tok, const int32_t* end_tokens, int n_end, int vocab, uint32_t* mask,
                                int64_t mask_stride, uint32_t* any);
// rows: device list of the n_rows batch rows with guide_slots[b] >= 0; guide_slots and states are indexed by the batch row.  Sets
// logits[b * stride + v] to -inf for every v < vocab whose bit is clear in row states[b] of slot guide_slots[b].  No rows: no launch.
hipError_t launch_guide_mask(hipStream_t s, float* logits, int stride, int vocab, const int32_t* rows, int n_rows, const int32_t* guide_slots,
                             const int32_t* states, const GuideTable& table);

// ---- k_prompt_logprobs.hip: prompt logprobs -------------------------------------------------------
// One workgroup per listed position j < n_rows: logits row j ([n_rows, stride], raw), target tokens[rows[j] + 1] (the step's packed token
// ids), n_top[j] in 0 .. 20.  out_lp / out_rank [n_rows]; out_top_tok / out_top_lp [n_rows, 20], written for n_top[j] >= 1 only (the first
// n_top[j] slots).  A target outside [0, vocab) gives NaN / rank -1 and reads nothing.  No rows: no launch.
hipError_t launch_prompt_logprobs(hipStream_t s, const float* logits, int stride, int vocab, const int32_t* rows, int n_rows,
                                  const int64_t* tokens, const int32_t* n_top, float* out_lp, int32_t* out_rank, int32_t* out_top_tok,
                                  float* out_top_lp);

// ---- synth.hip --------------------------------------------------------------------------------
// kinds as in oracle/llama_ref.c: 0 fp16 uniform(-amp,amp), 1 int8, 2 packed int4 (n bytes), 3 scale, 4 norm; and for the fp8 KV
// slab only (no oracle counterpart): 5 e4m3 codes, 6 power-of-two fp16 scales; for the int4 KV slab: 7 nibble pairs 1..15, 8 scales of its rule
hipError_t launch_synth_fill(hipStream_t s, int kind, uint64_t seed, uint32_t tensor_id, uint32_t stream_id, float amp,
                             uint64_t n, void* out);

}  // namespace pplhip
