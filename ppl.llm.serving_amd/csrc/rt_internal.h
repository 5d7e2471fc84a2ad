// What the units of the runtime (pplhip.cc, rt_comm.cc, rt_lora.cc, rt_postproc.cc, rt_ops.cc) share: the per-rank state and the context,
// error reporting, the guarded staging block (Stage), the layouts of the packed blocks that travel between host and device, and the few
// functions that more than one unit calls.  Nothing here is exported: the library is built with -fvisibility=hidden, and the functions
// of include/pplhip.h take their C linkage and their visibility from their declarations there.
#pragma once
#include "../../include/pplhip.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <unordered_map>
#include <memory>
#include <string>
#include <vector>

#include "kernels.h"

using namespace pplhip;

// activation format of the layer linears, from pplhip_model_desc.act_quant_bit (act_format, derived once at init):
// fp16, int8 per token (online_i8i8), or e4m3fn per token under a power-of-two scale (online_f8f8)
enum { ACT_FP16 = 0, ACT_I8 = 1, ACT_FP8 = 2 };

struct Linear {
    int N = 0, K = 0, qbit = 0, group = 0;
    int Kp = 0;  // row stride on the device: K rounded up to the GEMM k-tile (64) with zero columns, so that a tensor-
                 // parallel slice like 11008 / 8 = 1376 still runs on the DMA tile kernels (the activation operand is
                 // padded with zeros to the same stride)
    void* w = nullptr;
    uint16_t* scale = nullptr;
    uint64_t elt_bytes(uint64_t n) const { return qbit == 0 ? n * 2 : qbit == 8 ? n : n / 2; }
    uint64_t w_bytes() const { return elt_bytes((uint64_t)N * K); }       // container (unpadded) size
    uint64_t alloc_bytes() const { return elt_bytes((uint64_t)N * Kp); }  // device size
    uint64_t s_bytes() const { return qbit == 0 ? 0 : qbit == 8 ? (uint64_t)N * 2 : (uint64_t)N * (K / group) * 2; }
};

struct GraphEntry { hipGraphExec_t exec; uint64_t tick; };

struct Layer {
    uint16_t* attn_norm = nullptr;
    uint16_t* ffn_norm = nullptr;
    Linear wqkv, wo, w13, w2;
};

// One adapter slot of a rank: per (layer, target) the two factors on the device, zero-padded to rank rp (a multiple of 16) and, for w2's
// A, to the padded row stride Kp of the activation it multiplies.  Targets: 0 attention.wqkv, 1 attention.wo, 2 feed_forward.w2.
enum { LORA_WQKV = 0, LORA_WO = 1, LORA_W2 = 2, LORA_TARGETS = 3 };
struct LoraFactor {
    uint16_t *a = nullptr, *b = nullptr;
    int ra = 0, rb = 0;   // ranks the two arrived with
};
struct LoraAdapter {
    bool committed = false;
    float scale = 0.f;
    std::vector<LoraFactor> f;   // [layer][target]; empty: nothing loaded
};

struct ProfEvent {
    int cls;
    hipEvent_t a, b;
};

// One collective channel of a rank: what two all-reduces need of their own to run side by side.  Channel 0 carries every collective
// of a one-lane or two-chunk step, the self-test and the logits all-gather; channel 1 the second half-batch of a two-lane decode step.
struct Channel {
    int id = 0;                      // flag set of the direct collectives (k_comm.hip)
    ncclComm_t comm = nullptr;       // RCCL communicator (a communicator serialises its streams, so each channel has one)
    size_t x_scratch[2] = {0, 0};    // scratch double buffer: byte offsets inside the exchange region
    uint32_t ar_count = 0;           // all-reduces issued (which scratch buffer is next)
    uint32_t p2p_epoch = 0;          // epoch of the channel's flag words (taken through p2p_next_epoch)
    uint32_t refreshed_at = 0;       // the counter's value when the flag words of idle blocks were last lifted (kernels.h)
};

// What the launches of one half-batch go out with.  run_launches builds a Lane per half on its stack for every step: lane 0 = the rank's
// stream, workspaces and channel 0; lane 1 (two-lane decode only) = stream2, gemm_ws2, the attention workspace past the first half's
// rows and channel 1.  Nothing in Rank is swapped while a step is issued, so an error return leaves nothing to restore.
struct Lane {
    hipStream_t stream = nullptr;
    float* gemm_ws = nullptr;        // split-K partial slabs
    float* attn_ws = nullptr;
    size_t attn_ws_bytes = 0;
    // split-K results left unreduced for the kernel that consumes them (kernels.h SplitSlabs): wqkv -> RoPE + KV write, wo -> FFN norm,
    // w2 -> the next layer's attention norm (or the final norm)
    SplitSlabs sl_qkv, sl_part, sl_part2;
    Channel* ch = nullptr;
};

// ---- the guarded staging block ---------------------------------------------------------------------------------------------------------
// A pinned host block that one call fills and uploads with one copy and the next call fills again, with the event behind the last copy out
// of it.  The interface is the rule that makes such a block safe: the host pointer comes from begin() alone, which has waited for that
// copy, and upload() records the event behind the new one.  (An event that was never recorded counts as passed.)
class Stage {
public:
    // the block and its event, all or nothing; a stage that has its block keeps it
    hipError_t allocate(size_t bytes) {
        if (host_) return hipSuccess;
        void* p = nullptr;
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        if ((e = hipEventCreateWithFlags(&done_, hipEventDisableTiming)) != hipSuccess) {
            (void)hipHostFree(p);
            done_ = nullptr;
            return e;
        }
        host_ = (char*)p;
        return hipSuccess;
    }
    // the copy that last read the block is done: it may be written
    hipError_t begin(char** host) {
        *host = nullptr;
        const hipError_t e = hipEventSynchronize(done_);
        if (e == hipSuccess) *host = host_;
        return e;
    }
    hipError_t upload(void* dst_device, size_t bytes, hipStream_t stream) {
        const hipError_t e = hipMemcpyAsync(dst_device, host_, bytes, hipMemcpyHostToDevice, stream);
        return e != hipSuccess ? e : hipEventRecord(done_, stream);
    }
    void release() {   // (also of a stage that was never allocated)
        if (host_) (void)hipHostFree(host_);
        if (done_) (void)hipEventDestroy(done_);
        host_ = nullptr;
        done_ = nullptr;
    }

private:
    char* host_ = nullptr;
    hipEvent_t done_ = nullptr;
};

// ---- the packed blocks -----------------------------------------------------------------------------------------------------------------
// A packed block is columns one behind the other.  Each block below is described once, by the col<>() calls of its constructor: the same
// struct is built over the pinned base for the host pointers and over the device base for the device pointers, and over no base at all
// for the size (block_bytes).
struct Packed {
    char* base;
    int64_t bytes = 0;   // of the columns taken so far; once constructed: of the whole block
    explicit Packed(void* b) : base((char*)b) {}
    template <class T> T* col(int64_t n) {
        T* p = (T*)((uintptr_t)base + (uintptr_t)bytes);
        bytes += n * (int64_t)sizeof(T);
        return p;
    }
    size_t upto(const void* p) const { return (size_t)((const char*)p - base); }   // bytes in front of p: a copy that ends there
};
template <class Block> size_t block_bytes(int64_t n) { return (size_t)Block(nullptr, n).bytes; }

static_assert(PPLHIP_TOP_LOGPROBS_MAX == TOP_LOGPROBS_MAX, "header and kernel disagree");

// pplhip_sample_rows / pplhip_sample_rows2: one step's per-row arrays, for capacity cap_B; the copy ends behind the rows of the list that
// are in use.  min_p / typical_p stand behind the list, so a call without a truncating row copies exactly the bytes it copied before
// the two columns existed; a call with one copies them too (the list in full, cap_B entries)
struct SampleRowsBlock : Packed {
    uint64_t *seeds, *draws;
    float *temperatures, *top_p;
    int32_t *top_k, *rows;
    float *min_p, *typical_p;
    SampleRowsBlock(void* b, int64_t cap) : Packed(b) {
        seeds = col<uint64_t>(cap); draws = col<uint64_t>(cap);
        temperatures = col<float>(cap); top_p = col<float>(cap);
        top_k = col<int32_t>(cap); rows = col<int32_t>(cap);
        min_p = col<float>(cap); typical_p = col<float>(cap);
    }
};
// pplhip_top_logprobs, going up (a block of its own: the step's sampler call restages the sampler's while this one's copy may still be in
// flight), for capacity cap_B ...
struct TopLogprobsIn : Packed {
    float* temperatures;
    int32_t *num_logprobs, *rows;
    TopLogprobsIn(void* b, int64_t cap) : Packed(b) { temperatures = col<float>(cap); num_logprobs = col<int32_t>(cap); rows = col<int32_t>(cap); }
};
// ... and coming down, for `asked` rows
struct TopLogprobsOut : Packed {
    int32_t* tokens;   // [asked, 20]
    float* logprobs;   // [asked, 20]
    TopLogprobsOut(void* b, int64_t asked) : Packed(b) {
        tokens = col<int32_t>(asked * PPLHIP_TOP_LOGPROBS_MAX);
        logprobs = col<float>(asked * PPLHIP_TOP_LOGPROBS_MAX);
    }
};
// pplhip_logit_edit and pplhip_guide_edit, for capacity cap_B: a slot per row, its argument (the rule's flags u32 / the guide's state) and
// the list of the rows that ask
struct RowEditBlock : Packed {
    int32_t *slots, *arg, *rows;
    RowEditBlock(void* b, int64_t cap) : Packed(b) { slots = col<int32_t>(cap); arg = col<int32_t>(cap); rows = col<int32_t>(cap); }
};
// prompt logprobs (k_prompt_logprobs.hip) for P positions, going up: entry j + 1 of gather is row_j + 1 (the final norm's gathering form
// reads row gather[j + 1] - 1; entry 0 is never read) ...
struct PromptLogprobsIn : Packed {
    int64_t* gather;   // [P + 1]
    int32_t *rows, *n_top;
    PromptLogprobsIn(void* b, int64_t P) : Packed(b) { gather = col<int64_t>(P + 1); rows = col<int32_t>(P); n_top = col<int32_t>(P); }
};
// ... and coming down (the last two only when a position asked for the ranking: else the copy ends at top_tokens)
struct PromptLogprobsOut : Packed {
    float* logprobs;
    int32_t *ranks, *top_tokens;   // top_tokens [P, 20]
    float* top_logprobs;           // [P, 20]
    PromptLogprobsOut(void* b, int64_t P) : Packed(b) {
        logprobs = col<float>(P); ranks = col<int32_t>(P);
        top_tokens = col<int32_t>(P * PPLHIP_TOP_LOGPROBS_MAX);
        top_logprobs = col<float>(P * PPLHIP_TOP_LOGPROBS_MAX);
    }
};
// the pinned block the download lands in, for capacity cap_T: behind the room for the columns, the packed rows of the last run
struct PromptLogprobsHost : Packed {
    char* out;   // PromptLogprobsOut of the last run's positions
    int32_t* rows;
    PromptLogprobsHost(void* b, int64_t cap) : Packed(b) { out = col<char>((int64_t)block_bytes<PromptLogprobsOut>(cap)); rows = col<int32_t>(cap); }
};
// the step inputs of pplhip_set_inputs for T tokens of B requests; cache_indices only with a contiguous cache (mode 0: the paged cache has
// its page lists in a block of their own)
struct StepInputsBlock : Packed {
    int64_t *token_ids, *seq_starts, *kv_starts, *start_pos, *cache_indices;
    StepInputsBlock(void* b, int64_t T, int64_t B, bool contiguous_cache) : Packed(b) {
        token_ids = col<int64_t>(T); seq_starts = col<int64_t>(B + 1); kv_starts = col<int64_t>(B + 1); start_pos = col<int64_t>(B);
        cache_indices = contiguous_cache ? col<int64_t>(B) : nullptr;
    }
};

// logit rules: a slot's record in the device table and in the pinned staging ring is
// head i32 [4] = {n_bias, n_stop, has_mask, 0} | bias tokens i32 [512] | bias values f32 [512] | stops i32 [64] | mask u32 [words, padded to 4]
// so one copy carries a rule.
static_assert(PPLHIP_LOGIT_BIAS_MAX == LOGIT_BIAS_MAX && PPLHIP_LOGIT_STOP_MAX == LOGIT_STOP_MAX, "header and kernel disagree");
static_assert(PPLHIP_GUIDE_MAX_SLOTS == GUIDE_MAX_SLOTS && PPLHIP_GUIDE_MAX_STATES == GUIDE_MAX_STATES && GUIDE_DEAD == 255, "header and kernel disagree");
static_assert(PPLHIP_GUIDE16_MAX_STATES == GUIDE16_MAX_STATES && PPLHIP_GUIDE16_DEAD == GUIDE16_DEAD, "header and kernel disagree");
constexpr int64_t LR_HEAD = 16, LR_BIAS_TOK = LR_HEAD, LR_BIAS_VAL = LR_BIAS_TOK + 4 * LOGIT_BIAS_MAX,
                  LR_STOPS = LR_BIAS_VAL + 4 * LOGIT_BIAS_MAX, LR_MASK = LR_STOPS + 4 * LOGIT_STOP_MAX;
constexpr int LR_RING = 4;   // staging records; a record is reused once the copy out of it is done

struct Rank {
    int device = 0;
    int global_rank = 0;
    hipStream_t stream = nullptr;
    Channel ch[2];                      // ch[1]: scratch pair when two-stream decode is on, communicator when it was asked for explicitly
    hipStream_t comm_stream = nullptr;  // collectives of a two-chunk step (pplhip_run)
    // two-lane decode (plan_step): the second half of a mid-size pure-decode step runs its layers on stream2, beside the first half on
    // `stream`, with split-K / attention workspaces of its own (Lane); ev_fork / ev_join order the two around the step
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    float* gemm_ws2 = nullptr;
    bool dual_seen = false;
    hipEvent_t ev_compute[2] = {nullptr, nullptr}, ev_comm[2] = {nullptr, nullptr};
    const int64_t* h_seq = nullptr;     // host copy of this step's seq_starts (lives in the staging buffer)
    std::string err;

    // weights
    uint16_t* embed = nullptr;
    uint16_t* norm = nullptr;
    Linear output;
    std::vector<Layer> layers;
    float* rope = nullptr;
    std::vector<void*> allocs;

    // KV slab
    uint64_t kv_tokens = 0;
    void* kv_cache = nullptr;
    uint16_t* kv_scale = nullptr;

    // step inputs
    Stage st_step[2];             // two staging blocks take turns (st_step_cur: the next one) over one device image
    int st_step_cur = 0;
    int64_t* step_dev = nullptr;  // StepInputsBlock of the staged step
    int64_t cap_T = 0, cap_B = 0;
    int64_t *d_tok = nullptr, *d_seq = nullptr, *d_kvs = nullptr, *d_sp = nullptr, *d_ci = nullptr;
    int64_t* pages_dev = nullptr;   // mode 1: [B, max_pages]
    int64_t* pages_host = nullptr;  // pinned
    uint64_t pages_cap = 0;
    int64_t B = 0, T = 0, decoding_batches = 0, max_seq_len = 0, max_kv_len = 0, max_pages = 0;

    // activations
    uint16_t *h = nullptr, *xn = nullptr, *qkv = nullptr, *att = nullptr, *part = nullptr, *part2 = nullptr, *gu = nullptr,
             *act = nullptr, *hn = nullptr;
    std::unordered_map<uint64_t, GraphEntry> graphs;  // captured pure-decode steps by shape (run_decode_graph)
    uint64_t graph_tick = 0;
    int8_t* xq = nullptr;  // online_i8i8: int8 activations [cap_T, max row] and per-token scales
    float* sx = nullptr;
    float* logits_local = nullptr;  // [B, V/tp] (tp > 1)
    float* logits_gather = nullptr; // [tp, B, V/tp]
    float* logits = nullptr;        // [B, V]
    float* attn_ws = nullptr;
    size_t attn_ws_bytes = 0;
    float* gemm_ws = nullptr;  // split-K partial slabs (gemm_ws2: as many bytes)
    size_t gemm_ws_bytes = 0;

    // sampler (local rank 0)
    float *d_temp = nullptr, *d_topp = nullptr, *d_rand = nullptr, *d_lp = nullptr;
    int32_t* d_tokout = nullptr;
    uint16_t* count_map = nullptr;
    int64_t* d_slots = nullptr;
    float *d_rep = nullptr, *d_pres = nullptr, *d_freq = nullptr, *d_ptemp = nullptr;
    float* h_rand = nullptr;  // pinned
    // The sampler's two staging blocks are plain pinned blocks, not Stages: pplhip_sample_rows ends in a synchronisation of the stream,
    // and two pplhip_top_logprobs calls need one between them (include/pplhip.h), so nothing restages them under a copy in flight.  As
    // Stages they measured slower on an MI355X, B = 1024, V = 32000, medians of three alternated runs against the unguarded blocks (whose
    // own spread was 1 .. 2 us): pplhip_sample_rows 85.1 -> 90.1 us (greedy) and 372.8 -> 377.5 us (top-k 50); pplhip_top_logprobs +
    // pplhip_sample_rows 505.9 -> 522.6 us (one row asking) and 766.5 -> 781.8 us (all rows) -- an event record per call.
    char *h_srows = nullptr, *d_srows = nullptr;      // pplhip_sample_rows: SampleRowsBlock for cap_B rows (pinned / device)
    char *h_tlp_in = nullptr, *d_tlp_in = nullptr;    // pplhip_top_logprobs: TopLogprobsIn for cap_B rows going up ...
    char *h_tlp_out = nullptr, *d_tlp_out = nullptr;  // ... TopLogprobsOut coming down
    // logit rules, all allocated by the first pplhip_logit_rule_set: the device table (cap_B records of lr_rec bytes), the ring of
    // staging records, which slots hold a rule, and pplhip_logit_edit's RowEditBlock for cap_B rows (staged / device)
    char* lr_table = nullptr;
    Stage st_rule[LR_RING];
    int64_t lr_rec = 0;
    int lr_next = 0;
    std::vector<uint8_t> lr_has;
    Stage st_lre;
    char* d_lre = nullptr;
    // guided decoding: the vocabulary (pplhip_guide_set_vocab; gd_n_tok < 0: none yet), the loaded slots' masks and state counts, and
    // pplhip_guide_edit's RowEditBlock for cap_B rows (staged / device)
    uint8_t* gd_bytes = nullptr;
    int64_t* gd_off = nullptr;
    int gd_n_tok = -1;
    uint32_t* gd_mask[GUIDE_MAX_SLOTS] = {};
    int gd_states[GUIDE_MAX_SLOTS] = {};
    Stage st_gde;
    char* d_gde = nullptr;
    // prompt logprobs (k_prompt_logprobs.hip), all allocated by the first pplhip_set_prompt_logprobs that asks, for cap_T positions:
    // PromptLogprobsIn going up in one copy (staged / device), PromptLogprobsOut coming down in one copy (device / pinned:
    // PromptLogprobsHost, which also keeps the rows of the last run -- the staging block cannot, the next step restages it before its run).
    Stage st_plp;
    char *d_plp_in = nullptr, *h_plp_out = nullptr, *d_plp_out = nullptr;
    std::vector<int32_t> plp_rows;          // the rows of the staged ask, as they went into the staging block
    int64_t plp_n = 0;                      // positions of the staged step (pplhip_set_inputs clears it)
    bool plp_top = false;                   // one of them asked for the ranking
    int64_t plp_done = 0;                   // positions of the last pplhip_run

    // exchange region of the direct collectives (k_comm.hip): fine-grained, peer-mapped; holds the flag words and the buffers
    // the collectives work in place on (part, part2) or push into (logits_gather)
    char* xbase = nullptr;
    size_t xbytes = 0, x_part = 0, x_part2 = 0, x_local = 0;  // byte offsets inside the region (the scratch pairs: Channel)
    size_t x_slice_bytes = 0;           // room of each scratch buffer of a channel
    P2pPeers peers{};
    bool peer_ipc[P2P_MAX_RANKS] = {};  // peers.base[g] came from hipIpcOpenMemHandle (closed on destroy)
    uint32_t* p2p_status = nullptr;     // pinned host word a kernel raises when one of its bounded spins timed out
    int32_t* d_flag = nullptr;          // one int for the cross-process agreement on the self-test
    // stream hand-offs of the two-chunk schedule through device-memory epochs (k_comm.hip handoff_*): words 0..1 = "chunk i's
    // partial sums are complete" (compute -> communication stream), 2..3 = "chunk i is reduced" (communication -> compute)
    uint32_t* hflags = nullptr;
    uint32_t h_ready_ep[2] = {0, 0}, h_done_ep[2] = {0, 0};

    // multi-LoRA (k_lora.hip): adapters by slot, allocated when a slot is loaded
    LoraAdapter lora[LORA_MAX_SLOTS];
    int lora_committed = 0;                 // slots in use
    std::vector<LoraSlot> lora_tab_host;    // [layer][target][slot]: what the kernels read, mirrored on the device (lora_tab)
    LoraSlot* lora_tab = nullptr;
    LoraTile* lora_tiles = nullptr;         // the staged step's tile list (device) and its staging block
    Stage st_lora_tiles;
    int64_t lora_tile_cap = 0;
    uint16_t* lora_t = nullptr;             // shrink output [lora_tile_cap][16][LORA_MAX_RANK] fp16
    int lora_ntiles = 0;                    // > 0: the staged step has rows on adapters (pplhip_set_adapters; pplhip_set_inputs clears it)
    std::vector<uint8_t> lora_touch;        // [layer][target]: some adapter of the staged assignment changes this linear
    bool lora_stale = false;                // a slot was unloaded under a staged assignment: pplhip_run wants new inputs first

    // diagnosis (pplhip_debug_run_dump): residual stream h and the pending row-parallel FFN output after every layer
    uint16_t* dump_dev = nullptr;  // [L+1][2][T, hidden] fp16 (slot 0 = h, slot 1 = pending), allocated for one run

    // profiling
    std::vector<ProfEvent> prof;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_free;
};

struct pplhip_ctx {
    pplhip_model_desc d;
    pplhip_opts o;
    int kv_fmt = KV_FP16;  // KV cache format of (d.cache_quant_bit, d.cache_quant_group): kv_format(), derived once at init
    int act_fmt = ACT_FP16;  // activation format of d.act_quant_bit: act_format(), derived once at init
    int tp = 1;
    bool tp_overlap = true;              // PPLHIP_TP_OVERLAP=0 keeps the collectives on the compute stream
    // PPLHIP_TP_OVERLAP_MIN_TOKENS.  Measured on one MI355X with identity collectives (bench.py --emulate-tp 2/4/8,
    // profiles/r01_tp_emulation.txt): the two-chunk schedule costs a 1024-row decode step +6..7 ms (27 us per
    // cross-stream hand-off x 128, plus two half-size GEMM launches instead of one) -- about what the 64 all-reduces
    // of 8 MB it hides are worth -- so it is used for steps that carry prefill tokens (T >= 2048: 16+ MB per
    // all-reduce, chunks of >= 1024 rows keep the GEMM tiles full), not for pure decode steps of <= 1024 rows.
    int64_t tp_overlap_min_tokens = 2048;
    bool handoff_flags = true;  // PPLHIP_TP_HANDOFF=events: HIP events instead of device-memory epochs between the two streams
    int tp_debug = 0;           // PPLHIP_TP_DEBUG (diagnosis): bit 0 = hand-off events are created anew instead of re-recorded inside a step,
                                // bit 1 = chunks, but their collectives stay on the compute stream
    bool defer_on = true;       // PPLHIP_DEFER_REDUCE=0: every split-K linear reduces its own slabs
    bool tp_on = false;     // the tensor-parallel step schedule (collectives after wo / w2, logits gather) is active
    // collectives: 2 = direct kernels over peer-mapped memory (k_comm.hip), 1 = RCCL, 0 = none.  PPLHIP_COMM=auto (default:
    // direct when the self-test passes on every rank, else RCCL) | p2p (direct or fail) | rccl
    int comm_mode = 0;
    int comm_want = 0;      // 0 auto, 1 rccl only, 2 p2p only
    bool p2p_connected = false;
    uint64_t p2p_timeout_ticks = 0;  // s_memrealtime ticks (100 MHz)
    // PPLHIP_DUAL_STREAM=1: pure-decode steps of dual_min_rows..dual_max_rows rows as two half-batches on two streams (run_launches)
    // -1 (default): automatic -- under real tensor parallelism (a communicator over >= 2 ranks) pure-decode steps of 512..1024 rows run as
    // two half-batches on two streams, so that each half's all-reduces overlap the other half's matmuls (the north star's schedule;
    // +0.25 ms of compute per 1024-row 7B / TP8 step against ~2.2 ms of link time, profiles/r04_late_experiments.md 1); config 4's 256
    // rows stay on one stream (halves of 128 rows measured -8 %).  Automatic only on the direct collectives (two channels, validated on
    // one device at tp 2 / 4): two RCCL communicators running concurrently on one device have never run on >= 2 devices, so a
    // group that fell back to RCCL keeps one stream unless PPLHIP_DUAL_STREAM=1 asks for it.  1: rows dual_min_rows..dual_max_rows at any tp; 0: never
    int dual_mode = -1;
    bool dual_auto = false;          // the automatic rule is in force (row window 512..1024)
    int64_t dual_min_rows = 96, dual_max_rows = 512;
    // Sequence-parallel residual stream (round 6): on the direct collectives the all-reduce behind wo / w2 also does the residual add and the
    // RMSNorm that consumes it, on the rows the rank owns after the first shot, and the second shot gathers NORMED rows (k_comm.hip
    // p2p_allreduce_norm_kernel): 1 / tp of the norm work per rank and one launch less per half-layer.  Each rank then keeps only its own
    // rows of the residual stream h.  Not with int8 activations (the norm writes the quantised operand there), residual dumps, RCCL
    // (plain all-reduce + replicated norm as before) or hidden > 8192.  PPLHIP_TP_FUSE_NORM=0: off (A/B runs)
    bool fuse_norm_want = true;
    bool emulate_tp = false;         // PPLHIP_EMULATE_TP (bench.py --emulate-tp): one rank's slice, collectives are local identities
    int selftest = 0;                // direct collectives' start-up self-test: 0 not run, 1 passed on every rank, -1 failed (RCCL in charge)
    std::string comm_notes;          // every fallback taken at start-up, in order (never silent: also on stderr)
    bool graph_on = false;           // PPLHIP_DECODE_GRAPH=1: replay pure-decode steps as HIP graphs (opt-in, see run_decode_graph)
    int64_t graph_max_batch = 64;    // above this a step is seconds of GPU work per thousand launches: nothing to gain
    int H = 0, Hkv = 0, D = 0, inter = 0, vocab_local = 0;
    std::vector<Rank> ranks;
    std::string err;
};

#define HIPCK(c, r, expr)                                                                                            \
    do {                                                                                                             \
        hipError_t e__ = (expr);                                                                                     \
        if (e__ != hipSuccess)                                                                                       \
            return fail(c, r, e__ == hipErrorOutOfMemory ? PPLHIP_OUT_OF_MEMORY : PPLHIP_DEVICE_RUNTIME_ERROR,       \
                        std::string(#expr) + ": " + hipGetErrorString(e__));                                         \
    } while (0)

#define NCCLCK(c, r, expr)                                                                                           \
    do {                                                                                                             \
        ncclResult_t e__ = (expr);                                                                                   \
        if (e__ != ncclSuccess)                                                                                      \
            return fail(c, r, PPLHIP_DEVICE_RUNTIME_ERROR, std::string(#expr) + ": " + ncclGetErrorString(e__));     \
    } while (0)

// ---- functions more than one unit calls ------------------------------------------------------------------------------------------------
// pplhip.cc
bool verbose();
void comm_note(pplhip_ctx* c, const std::string& msg);
int fail(pplhip_ctx* c, int rank, int code, const std::string& msg);
int dev_alloc(pplhip_ctx* c, int r, void** p, uint64_t bytes);
int kv_format(int quant_bit, int quant_group, int D);
KvAddr make_kv_addr(const pplhip_model_desc& d, int Hkv, int D, uint64_t tokens, void* cache, uint16_t* scale, int layer);
// A chunk of a step: requests [b0, b0 + bn) = token rows [t0, t0 + tn); the first nd requests of the chunk are
// decode rows.  A step runs as ONE chunk or as two (plan_step).
using Chunk = pplhip_chunk;
using StepPlan = pplhip_step_plan;
pplhip_plan_settings plan_settings(const pplhip_ctx* c, const Rank& R);
bool fuse_norm_active(const pplhip_plan_settings& s, bool dump);
StepPlan plan_step(const pplhip_plan_settings& s, const pplhip_step_shape& sh);
Lane make_lane(Rank& R, int i, int64_t attn_ws_off);
int chunk_allreduce(pplhip_ctx* c, int rank, Lane& lane, uint16_t* buf, const Chunk& k, int ci, bool overlapped, const uint16_t* norm_w = nullptr);
// rt_comm.cc
int p2p_connect_local(pplhip_ctx* c);
int p2p_check(pplhip_ctx* c, int rank);
// the epoch of the channel's next collective, which the caller launches on `s` right away (in front of it, every P2P_FLAG_REFRESH_EPOCHS
// epochs, the refresh of the flag words that idle blocks left behind)
int p2p_next_epoch(pplhip_ctx* c, int rank, Channel& ch, hipStream_t s, uint32_t* epoch);
// rt_lora.cc
void lora_build_tiles(const int32_t* row_slots, int64_t T, std::vector<LoraTile>& out);
// rt_postproc.cc
int sample_row_list(const int32_t* top_k, const float* min_p, const float* typical_p, int B, int32_t* rows, int* n_trunc);
int top_logprobs_row_list(const int32_t* num_logprobs, int B, int32_t* rows);
int run_prompt_logprobs(pplhip_ctx* c, int rank, hipStream_t s, const uint16_t* pending, const SplitSlabs& sl_part2);
