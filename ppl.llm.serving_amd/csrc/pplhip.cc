// libpplhip.so -- the C ABI of include/pplhip.h: per-rank runtime (streams, weights, KV slab, step inputs,
// activations), the decoder forward as a sequence of hand-written gfx950 kernels, RCCL collectives for tensor
// parallelism, the sampler and per-request LoRA adapters (slots loaded at run time, a tile list per
// step: "multi-LoRA").  The runtime replaces what the reference reaches through ppl.nn
// (Engine/Runtime/Tensor, src/backends/cuda/resource_manager.cc:43-211) and ppl.llm.kernel.cuda.
// What lives where:
//   pplhip.cc       (this file) init and destroy, weights, the KV slab, pplhip_set_inputs, the step plan and its launches (plan_step,
//                   run_launches, the stream hand-offs of the two-chunk schedule, the decode graph), pplhip_run / sync / logits, profiling
//   rt_comm.cc      the direct collectives' connection and self-test, pplhip_comm_*
//   rt_lora.cc      multi-LoRA: adapter slots and the step's tile list
//   rt_postproc.cc  what happens to the logits: samplers, penalty, top-N logprobs, logit rules, guided decoding, prompt logprobs
//   rt_ops.cc       pplhip_op_*: single kernels and pure functions on caller-owned memory, for the tests (no context)
//   rt_internal.h   what they share: Rank and pplhip_ctx, error reporting, the guarded staging block, the packed blocks' layouts
#include "rt_internal.h"

bool verbose() {   // PPLHIP_VERBOSE: messages on stderr (errors, the collectives' choice, graph capture)
    static const bool on = getenv("PPLHIP_VERBOSE") != nullptr;
    return on;
}

// a fallback was taken (direct collectives -> RCCL, two streams -> one): always on stderr, and kept for pplhip_comm_info
void comm_note(pplhip_ctx* c, const std::string& msg) {
    fprintf(stderr, "[pplhip] %s\n", msg.c_str());
    if (c) { if (!c->comm_notes.empty()) c->comm_notes += "; "; c->comm_notes += msg; }
}

int fail(pplhip_ctx* c, int rank, int code, const std::string& msg) {
    if (c) {
        if (rank >= 0 && rank < (int)c->ranks.size()) c->ranks[rank].err = msg; else c->err = msg;
    }
    if (verbose()) fprintf(stderr, "[pplhip] error %d (rank %d): %s\n", code, rank, msg.c_str());
    return code;
}

static inline float h2f_host(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
static inline uint16_t f2h_host(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }

// ACT_* of an act_quant_bit value (-1: none); the quantised forms need weight_quant_bit 8
static int act_format(int act_quant_bit, int weight_quant_bit) {
    if (act_quant_bit == 0) return ACT_FP16;
    if (weight_quant_bit != 8) return -1;
    if (act_quant_bit == PPLHIP_ACT_QUANT_I8) return ACT_I8;
    if (act_quant_bit == PPLHIP_ACT_QUANT_FP8) return ACT_FP8;
    return -1;
}

// k-tile the padded row stride of w2 / the SwiGLU output is rounded to: 64 (fp16-activation tile GEMM), 128 (int8 / fp8 operands)
static int k_tile(const pplhip_ctx* c) { return c->act_fmt != ACT_FP16 ? 128 : 64; }

int dev_alloc(pplhip_ctx* c, int r, void** p, uint64_t bytes) {
    *p = nullptr;
    if (bytes == 0) return 0;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(c, r, PPLHIP_OUT_OF_MEMORY, "hipMalloc(" + std::to_string(bytes) + "): " + hipGetErrorString(e));
    c->ranks[r].allocs.push_back(*p);
    return 0;
}

namespace {

int linear_alloc(pplhip_ctx* c, int r, Linear* l, int N, int K, int qbit, int group, bool pad_k = false) {
    l->N = N; l->K = K; l->qbit = qbit; l->group = group;
    const int kt = k_tile(c);
    l->Kp = (pad_k && qbit != 4) ? (K + kt - 1) / kt * kt : K;
    int rc = dev_alloc(c, r, &l->w, l->alloc_bytes());
    if (rc) return rc;
    if (l->Kp != K) {
        hipError_t e = hipMemset(l->w, 0, l->alloc_bytes());
        if (e != hipSuccess) return fail(c, r, PPLHIP_DEVICE_RUNTIME_ERROR, std::string("hipMemset: ") + hipGetErrorString(e));
    }
    return dev_alloc(c, r, (void**)&l->scale, l->s_bytes());
}

// name -> device buffer of a rank's slice; names: DESIGN.md "weight container"
bool find_tensor(pplhip_ctx* c, Rank& R, const char* name, void** ptr, uint64_t* bytes, Linear** lin_out = nullptr) {
    if (lin_out) *lin_out = nullptr;
    const int hd = c->d.hidden_dim;
    if (!strcmp(name, "tok_embeddings.weight")) { *ptr = R.embed; *bytes = (uint64_t)c->d.vocab_size * hd * 2; return true; }
    if (!strcmp(name, "norm.weight")) { *ptr = R.norm; *bytes = (uint64_t)hd * 2; return true; }
    if (!strcmp(name, "output.weight")) { *ptr = R.output.w; *bytes = R.output.w_bytes(); if (lin_out) *lin_out = &R.output; return true; }
    int l = -1;
    char rest[128];
    if (sscanf(name, "layers.%d.%127s", &l, rest) != 2 || l < 0 || l >= c->d.num_layers) return false;
    Layer& L = R.layers[l];
    if (!strcmp(rest, "attention_norm.weight")) { *ptr = L.attn_norm; *bytes = (uint64_t)hd * 2; return true; }
    if (!strcmp(rest, "ffn_norm.weight")) { *ptr = L.ffn_norm; *bytes = (uint64_t)hd * 2; return true; }
    struct { const char* n; Linear* lin; } tab[] = {{"attention.wqkv", &L.wqkv}, {"attention.wo", &L.wo},
                                                      {"feed_forward.w13", &L.w13}, {"feed_forward.w2", &L.w2}};
    for (auto& t : tab) {
        const size_t nl = strlen(t.n);
        if (strncmp(rest, t.n, nl)) continue;
        if (!strcmp(rest + nl, ".weight")) { *ptr = t.lin->w; *bytes = t.lin->w_bytes(); if (lin_out) *lin_out = t.lin; return true; }
        if (!strcmp(rest + nl, ".scale") && t.lin->qbit) { *ptr = t.lin->scale; *bytes = t.lin->s_bytes(); return true; }
    }
    return false;
}

}  // namespace

// KV cache format of a (cache_quant_bit, cache_quant_group) pair at head_dim D, -1 when the pair is not one of the four:
// (0, 1) fp16, (8, 8) int8 group 8, (8, D) fp8 e4m3 with one power-of-two scale per head row, (4, 32) int4 with one fp16 scale per 32
// channels (the last two at D = 32, 64, 128).  Everything behind the sizes (make_kv_addr, pplhip_kv_block_bytes) works from the pair
// itself: kv_row_bytes() bytes of codes and D / group scales per row.
int kv_format(int quant_bit, int quant_group, int D) {
    if (quant_bit == 0 && quant_group == 1) return KV_FP16;
    if (quant_bit == 8 && quant_group == 8) return KV_I8G8;
    if (quant_bit == 8 && quant_group == D && (D == 32 || D == 64 || D == 128)) return KV_FP8;
    if (quant_bit == 4 && quant_group == 32 && (D == 32 || D == 64 || D == 128)) return KV_I4G32;
    return -1;
}
// bytes of one head row of D channels in the slab: fp16 2 D, int8 / fp8 D, int4 D / 2 (two channels per byte)
static int64_t kv_row_bytes(int quant_bit, int D) { return quant_bit == 4 ? D / 2 : (quant_bit == 8 ? D : 2 * D); }

KvAddr make_kv_addr(const pplhip_model_desc& d, int Hkv, int D, uint64_t tokens, void* cache, uint16_t* scale, int layer) {
    const int elt = d.cache_quant_bit == 0 ? 2 : 1;
    const int g = d.cache_quant_group > 0 ? d.cache_quant_group : 1;
    // (int4: the slab is addressed like the int8 slab with a row of D / 2 one-byte elements)
    const KvStrides cs = kv_strides(d.cache_layout, (int64_t)tokens, d.num_layers, Hkv, kv_row_bytes(d.cache_quant_bit, D) / elt);
    const KvStrides ss = kv_strides(d.cache_layout, (int64_t)tokens, d.num_layers, Hkv, D / g);
    KvAddr a;
    a.cache = (char*)cache + (int64_t)layer * cs.sL * elt;
    a.scale = scale ? scale + (int64_t)layer * ss.sL : nullptr;
    a.sKV = cs.sKV; a.sH = cs.sH; a.sN = cs.sN;
    a.ssKV = ss.sKV; a.ssH = ss.sH; a.ssN = ss.sN;
    a.mode = d.cache_mode;
    a.page_size = d.page_size > 0 ? d.page_size : 1;
    a.page_shift = (a.page_size & (a.page_size - 1)) == 0 ? __builtin_ctz((unsigned)a.page_size) : -1;
    return a;
}

namespace {

void prof_begin(pplhip_ctx* c, Rank& R, const Lane& lane, int cls, ProfEvent* ev) {
    ev->cls = -1;
    if (!c->o.enable_profiling) return;
    // 2 = light: only the decode-attention launches (through hipExtLaunchKernel's start / stop events) and the whole run.  An event record is a barrier packet on the
    // stream: the full set (10 per layer) costs a batch-1024 decode step 1.3 ms of 43.9 (profiles/probes/prof_overhead.py)
    if (c->o.enable_profiling == 2 && cls != PPLHIP_PROF_RUN) return;   // (decode attention: timed through its own launch)
    std::pair<hipEvent_t, hipEvent_t> p;
    if (!R.prof_free.empty()) { p = R.prof_free.back(); R.prof_free.pop_back(); }
    else { hipEventCreate(&p.first); hipEventCreate(&p.second); }
    ev->cls = cls; ev->a = p.first; ev->b = p.second;
    hipEventRecord(ev->a, lane.stream);
}
void prof_end(Rank& R, const Lane& lane, ProfEvent* ev) {
    if (ev->cls < 0) return;
    hipEventRecord(ev->b, lane.stream);
    R.prof.push_back(*ev);
}

int decode_split(const pplhip_plan_settings& s, int64_t nb, int64_t max_kv_len) {
    const int mode = s.decoding_attn_split_k;
    if (mode == 0) return 1;
    const bool gqa = attn_decode_gqa_supported(kv_format(s.cache_quant_bit, s.cache_quant_group, s.head_dim), s.heads, s.kv_heads, s.head_dim);
    const int64_t blocks = nb * (gqa ? s.kv_heads : s.heads);  // GQA kernel: one block per KV head
    int split = 1;
    // measured (profiles/attn_microbench.py): 512 workgroups already stream at 5.3 TB/s; split only below ~256.  (The grouped-query
    // kernel at 256 blocks -- 70B / TP8, 256 requests x 1 KV head -- is faster unsplit: 37 us against 46 us with split 2, the reduce
    // launch costs more than the second block per CU brings, profiles/r03_roofline_sweep.json)
    if (mode == 2 || (blocks < 256 && max_kv_len >= 512)) {
        int64_t want = (512 + blocks - 1) / blocks;            // aim for >= 512 workgroups
        // >= 256 tokens per split; >= 128 when there are very few blocks (batch 1-4 of a multi-head model: kv 512 split 4 8.6 us against 10.3 us
        // with split 2, kv 2048 split 8 11.0 against 13.8 with 4 -- one memory round trip per wave instead of two, round 4)
        // (never below the >= 256-tokens rule: at kv 8192 a single stream keeps split 16 / 32 -- ADVICE r4: the 8-way limit of the
        // 128-token rule had lowered it to 8 from kv 2048 on)
        int64_t cap = std::max<int64_t>(1, std::max<int64_t>(max_kv_len / 256, blocks <= 128 ? std::min<int64_t>(max_kv_len / 128, 8) : 0));
        split = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(want, cap), 32));
        if (mode == 2 && split < 2 && max_kv_len >= 64) split = 2;
    }
    return split;
}

// ---- the hand-off between a compute stream and the communication stream (two-chunk schedule), once: device-memory epochs
// (k_comm.hip handoff_*, Rank::hflags) or, PPLHIP_TP_HANDOFF=events, HIP events

// "the work issued on `from` so far is complete for slot i": the communication stream waits for that, runs `work` and marks slot i done.
// identity: no collective exists (ranks emulated on one device) -- the wait kernel itself raises the done flag and nothing else is launched
// fresh_events: PPLHIP_TP_DEBUG bit 0 asks for new events instead of re-recorded ones (the all-reduces; the logits all-gather never did)
template <class Work>
int comm_handoff(pplhip_ctx* c, int rank, hipStream_t from, int i, bool identity, bool fresh_events, Work&& work) {
    Rank& R = c->ranks[rank];
    if (c->handoff_flags) {
        HIPCK(c, rank, launch_handoff_signal(from, R.hflags + i, ++R.h_ready_ep[i]));
        HIPCK(c, rank, launch_handoff_wait(R.comm_stream, R.hflags + i, R.h_ready_ep[i], identity ? R.hflags + 2 + i : nullptr,
                                           identity ? R.h_done_ep[i] + 1 : 0, c->p2p_timeout_ticks, R.p2p_status));
        ++R.h_done_ep[i];
        if (identity) return 0;
        if (int rc = work(R.comm_stream)) return rc;
        HIPCK(c, rank, launch_handoff_signal(R.comm_stream, R.hflags + 2 + i, R.h_done_ep[i]));
        return 0;
    }
    if (fresh_events) {  // diagnosis: never re-record an event inside a step (the old ones are not destroyed)
        hipEventCreateWithFlags(&R.ev_compute[i], hipEventDisableTiming);
        hipEventCreateWithFlags(&R.ev_comm[i], hipEventDisableTiming);
    }
    HIPCK(c, rank, hipEventRecord(R.ev_compute[i], from));
    HIPCK(c, rank, hipStreamWaitEvent(R.comm_stream, R.ev_compute[i], 0));
    if (int rc = work(R.comm_stream)) return rc;
    HIPCK(c, rank, hipEventRecord(R.ev_comm[i], R.comm_stream));
    return 0;
}

// the compute stream `to` picks up slot i: what the communication stream did for it is complete
int comm_pickup(pplhip_ctx* c, int rank, hipStream_t to, int i) {
    Rank& R = c->ranks[rank];
    if (c->handoff_flags)
        HIPCK(c, rank, launch_handoff_wait(to, R.hflags + 2 + i, R.h_done_ep[i], nullptr, 0, c->p2p_timeout_ticks, R.p2p_status));
    else
        HIPCK(c, rank, hipStreamWaitEvent(to, R.ev_comm[i], 0));
    return 0;
}

}  // namespace

int pplhip_version(void) { return (1 << 16) | 2; }  // 1.1: pplhip_model_desc.act_quant_bit, comm_* and W8A8 operator entry points;
                                                    // 1.2: fp8 e4m3 KV cache (cache_quant_bit 8, cache_quant_group = head_dim),
                                                    //      online_f8f8 (act_quant_bit PPLHIP_ACT_QUANT_FP8) and pplhip_op_*_f8
                                                    //      (later additions keep 1.2 and are detected by pplhip_init accepting them:
                                                    //      the int4 KV cache, cache_quant_bit 4 / cache_quant_group 32)

int pplhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return PPLHIP_DEVICE_RUNTIME_ERROR;
    return n;
}

int pplhip_get_unique_id(void* out) {
    static_assert(sizeof(ncclUniqueId) <= PPLHIP_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return PPLHIP_DEVICE_RUNTIME_ERROR;
    memset(out, 0, PPLHIP_UNIQUE_ID_BYTES);
    memcpy(out, &id, sizeof(id));
    return 0;
}

int pplhip_build_rope_table(float* out, int32_t max_position, int32_t head_dim, float theta) {
    const int half = head_dim / 2;
    for (int p = 0; p < max_position; ++p)
        for (int i = 0; i < half; ++i) {
            const double freq = pow((double)theta, -2.0 * (double)i / (double)head_dim);
            const double a = (double)p * freq;
            out[(size_t)p * head_dim + i] = (float)cos(a);
            out[(size_t)p * head_dim + half + i] = (float)sin(a);
        }
    return 0;
}

void pplhip_destroy(pplhip_ctx* c) {
    if (!c) return;
    for (auto& R : c->ranks) {
        hipSetDevice(R.device);
        if (R.stream) hipStreamSynchronize(R.stream);
        if (R.comm_stream) hipStreamSynchronize(R.comm_stream);
        if (R.stream2) { hipStreamSynchronize(R.stream2); hipStreamDestroy(R.stream2); }
        if (R.ev_fork) hipEventDestroy(R.ev_fork);
        if (R.ev_join) hipEventDestroy(R.ev_join);
        if (R.ch[1].comm) ncclCommDestroy(R.ch[1].comm);
        if (R.ch[0].comm) ncclCommDestroy(R.ch[0].comm);
        if (R.comm_stream) hipStreamDestroy(R.comm_stream);
        for (int i = 0; i < 2; ++i) {
            if (R.ev_compute[i]) hipEventDestroy(R.ev_compute[i]);
            if (R.ev_comm[i]) hipEventDestroy(R.ev_comm[i]);
        }
        for (auto& g : R.graphs) if (g.second.exec) hipGraphExecDestroy(g.second.exec);
        for (auto& e : R.prof) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
        for (auto& p : R.prof_free) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
        for (void* p : R.allocs) hipFree(p);
        for (auto& ad : R.lora) for (auto& f : ad.f) { if (f.a) hipFree(f.a); if (f.b) hipFree(f.b); }
        if (R.lora_tab) hipFree(R.lora_tab);
        if (R.lora_tiles) hipFree(R.lora_tiles);
        if (R.lora_t) hipFree(R.lora_t);
        for (int g = 0; g < P2P_MAX_RANKS; ++g)
            if (R.peer_ipc[g] && R.peers.base[g]) hipIpcCloseMemHandle(R.peers.base[g]);
        if (R.xbase) hipFree(R.xbase);
        if (R.p2p_status) hipHostFree(R.p2p_status);
        if (R.kv_cache) hipFree(R.kv_cache);
        if (R.kv_scale) hipFree(R.kv_scale);
        for (Stage* st : {&R.st_step[0], &R.st_step[1], &R.st_lora_tiles, &R.st_lre, &R.st_gde, &R.st_plp}) st->release();
        for (Stage& st : R.st_rule) st.release();
        if (R.pages_host) hipHostFree(R.pages_host);
        if (R.pages_dev) hipFree(R.pages_dev);
        for (void* p : {(void*)R.h_rand, (void*)R.h_srows, (void*)R.h_tlp_in, (void*)R.h_tlp_out, (void*)R.h_plp_out}) if (p) hipHostFree(p);
        if (R.gd_bytes) hipFree(R.gd_bytes);
        if (R.gd_off) hipFree(R.gd_off);
        for (uint32_t* m : R.gd_mask) if (m) hipFree(m);
        if (R.stream) hipStreamDestroy(R.stream);
    }
    delete c;
}

const char* pplhip_last_error(pplhip_ctx* c, int rank) {
    if (!c) return "null context";
    if (rank >= 0 && rank < (int)c->ranks.size() && !c->ranks[rank].err.empty()) return c->ranks[rank].err.c_str();
    return c->err.c_str();
}

int pplhip_init(const pplhip_model_desc* desc, const pplhip_opts* opts, pplhip_ctx** out) {
    if (!desc || !opts || !out) return PPLHIP_INVALID_VALUE;
    *out = nullptr;
    std::unique_ptr<pplhip_ctx> c(new pplhip_ctx());
    c->d = *desc;
    c->o = *opts;
    c->o.device_ids = nullptr;
    c->o.nccl_unique_id = nullptr;
    const int n = opts->n_local_ranks;
    const int tp = opts->world_size > 0 ? opts->world_size : n;
    c->tp = tp;
    const pplhip_model_desc& d = c->d;
    auto bad = [&](const char* m) { if (verbose()) fprintf(stderr, "[pplhip] init: %s\n", m); return PPLHIP_INVALID_VALUE; };
    if (n < 1 || tp < n || opts->rank_base < 0 || opts->rank_base + n > tp) return bad("rank layout");
    if (d.num_heads <= 0 || d.hidden_dim % d.num_heads) return bad("heads");
    if (d.num_heads % tp || d.num_kv_heads % tp || d.intermediate_dim % tp || d.vocab_size % tp) return bad("tp divisibility");
    if (d.num_heads % d.num_kv_heads) return bad("gqa");
    // src/generator/llm_generator.cc:114-144 (CheckParameters)
    // (plus the fp8 pair (8, head_dim) and the int4 pair (4, 32) of this library: kv_format)
    if (kv_format(d.cache_quant_bit, d.cache_quant_group, d.hidden_dim / d.num_heads) < 0) return bad("cache quant");
    if (d.cache_layout < 0 || d.cache_layout > 3 || d.cache_mode < 0 || d.cache_mode > 1) return bad("cache layout/mode");
    if (d.cache_mode == 1 && d.page_size <= 0) return bad("page_size");
    if (d.weight_quant_bit != 0 && d.weight_quant_bit != 8 && d.weight_quant_bit != 4) return bad("weight quant");
    if (act_format(d.act_quant_bit, d.weight_quant_bit) < 0) return bad("act quant (8 / 0x108 need weight_quant_bit 8)");
    if (opts->max_running_batch <= 0 || opts->max_tokens_per_step <= 0 || d.max_position <= 0) return bad("limits");
    c->D = d.hidden_dim / d.num_heads;
    c->kv_fmt = kv_format(d.cache_quant_bit, d.cache_quant_group, c->D);
    c->act_fmt = act_format(d.act_quant_bit, d.weight_quant_bit);
    c->H = d.num_heads / tp;
    c->Hkv = d.num_kv_heads / tp;
    c->inter = d.intermediate_dim / tp;
    c->vocab_local = d.vocab_size / tp;
    if (c->D != 32 && c->D != 64 && c->D != 128) return bad("head_dim must be 32, 64 or 128");
    if (d.hidden_dim % 16 || c->inter % 16 || c->vocab_local % 4) return bad("dims alignment");
    if (d.weight_quant_bit == 4 && (d.weight_quant_group % 32 || d.hidden_dim % d.weight_quant_group ||
                                    (c->H * c->D) % d.weight_quant_group || c->inter % d.weight_quant_group)) return bad("w4 group");

    c->ranks.resize(n);
    pplhip_ctx* cp = c.get();
    std::vector<int> devs(n);
    for (int r = 0; r < n; ++r) devs[r] = opts->device_ids ? opts->device_ids[r] : r;
    if (!opts->device_ids) {  // PPLHIP_DEVICE_IDS=0,0,...: device of each local rank (tests: a whole group on one GPU)
        if (const char* e = getenv("PPLHIP_DEVICE_IDS")) {
            int r = 0;
            for (const char* q = e; *q && r < n; ++r) {
                devs[r] = atoi(q);
                while (*q && *q != ',') ++q;
                if (*q == ',') ++q;
            }
        }
    }

    // communicators (replaces ppl::common::InitNccl, resource_manager.cc:393)
    // PPLHIP_FORCE_COMM=1: create the communicator and run every collective even at world size 1 (an identity) --
    // lets a single-GPU box exercise the RCCL call sequence, the communication stream and its event wiring
    const bool want_comm = tp > 1 || getenv("PPLHIP_FORCE_COMM") != nullptr;
    c->tp_on = want_comm;
    if (const char* e = getenv("PPLHIP_DECODE_GRAPH")) c->graph_on = atoi(e) != 0;
    if (const char* e = getenv("PPLHIP_TP_FUSE_NORM")) c->fuse_norm_want = atoi(e) != 0;
    c->emulate_tp = getenv("PPLHIP_EMULATE_TP") != nullptr;
    if (const char* e = getenv("PPLHIP_DUAL_STREAM")) c->dual_mode = atoi(e);
    int dual_min_env = 0;
    if (const char* e = getenv("PPLHIP_DUAL_MIN_ROWS")) dual_min_env = std::max(2, atoi(e));
    if (c->dual_mode < 0) {   // automatic: only where there is link time to hide
        c->dual_auto = tp > 1 && !getenv("PPLHIP_EMULATE_TP");
        c->dual_mode = c->dual_auto ? 1 : 0;
        if (c->dual_auto) { c->dual_min_rows = dual_min_env ? dual_min_env : 512; c->dual_max_rows = 1024; }
        // (no second stream or workspace for a context whose steps can never reach the window: memory, not safety -- the safety check is
        // the stream count against the hardware queues below)
        if (c->dual_auto && opts->max_running_batch < c->dual_min_rows) { c->dual_auto = false; c->dual_mode = 0; }
    }
    if (dual_min_env) c->dual_min_rows = dual_min_env;
    if (const char* e = getenv("PPLHIP_DUAL_MAX_ROWS")) c->dual_max_rows = atoi(e);
    if (const char* e = getenv("PPLHIP_DECODE_GRAPH_MAX_BATCH")) c->graph_max_batch = std::max(1, atoi(e));
    if (const char* e = getenv("PPLHIP_COMM")) c->comm_want = !strcmp(e, "rccl") ? 1 : (!strcmp(e, "p2p") ? 2 : 0);
    {   // bounded spins of the direct collectives: s_memrealtime runs at 100 MHz
        const char* e = getenv("PPLHIP_P2P_TIMEOUT_MS");
        c->p2p_timeout_ticks = (uint64_t)(e ? std::max(1, atoi(e)) : 20000) * 100000ull;
    }
    // several ranks on ONE device (tests: a whole tensor-parallel group emulated on a single GPU): RCCL refuses duplicate
    // devices, the direct collectives do not care where a peer's region lives
    bool dup_dev = false;
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b) dup_dev |= devs[a] == devs[b];
    if (dup_dev && c->comm_want == 1) return fail(cp, -1, PPLHIP_INVALID_VALUE, "PPLHIP_COMM=rccl needs distinct devices");
    if (dup_dev) c->comm_want = 2;
    if (tp > P2P_MAX_RANKS || getenv("PPLHIP_EMULATE_TP") || tp < 2) {
        if (c->comm_want == 2 && want_comm) return fail(cp, -1, PPLHIP_INVALID_VALUE, "direct collectives need 2..8 connected ranks");
        c->comm_want = 1;
    }
    if (const char* e = getenv("PPLHIP_TP_OVERLAP")) c->tp_overlap = atoi(e) != 0;
    if (const char* e = getenv("PPLHIP_TP_HANDOFF")) c->handoff_flags = strcmp(e, "events") != 0;
    {   // read once per process, like every diagnosis switch
        static const int tp_debug = getenv("PPLHIP_TP_DEBUG") ? atoi(getenv("PPLHIP_TP_DEBUG")) : 0;
        static const int defer_on = getenv("PPLHIP_DEFER_REDUCE") ? atoi(getenv("PPLHIP_DEFER_REDUCE")) : 1;
        c->tp_debug = tp_debug;
        c->defer_on = defer_on != 0;
    }
    {   // Streams against hardware queues.  Kernels of this library WAIT for kernels on other streams of the same process (direct collectives
        // of ranks that share a device, the hand-off kernels of the two-chunk schedule, the halves of a two-stream step meeting in a
        // collective): the HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues per device (default 4), and a
        // spinning kernel queued IN FRONT of the kernel it waits for on the same hardware queue never sees it run.  That is what round 5's
        // "stream hand-off timed out" was (a tp-8 group on ONE device with automatic two-stream decode: 8 x 3 streams on 24 queues).
        // Checked here as a resource, per device: streams this context will create there against the queues the runtime will give it.
        const char* q = getenv("GPU_MAX_HW_QUEUES");
        const int hwq = q && atoi(q) > 0 ? atoi(q) : 4;
        auto streams_per_rank = [&]() { return 1 + (c->dual_mode ? 1 : 0) + (c->tp_on ? 1 : 0); };
        int worst = 0;
        for (int a = 0; a < n; ++a) {
            int same = 0;
            for (int b = 0; b < n; ++b) same += devs[a] == devs[b];
            worst = std::max(worst, same);
        }
        if (c->dual_auto && worst * streams_per_rank() > hwq) {
            comm_note(c.get(), "two-stream decode off: " + std::to_string(worst) + " local rank(s) per device x " + std::to_string(streams_per_rank()) +
                                   " streams exceed " + std::to_string(hwq) + " hardware queues (GPU_MAX_HW_QUEUES)");
            c->dual_auto = false;
            c->dual_mode = 0;
        }
        if (c->tp_on && worst * streams_per_rank() > hwq) {
            if (c->handoff_flags && !getenv("PPLHIP_TP_HANDOFF")) {
                c->handoff_flags = false;   // events never spin
                comm_note(c.get(), "stream hand-offs by events, not device flags: " + std::to_string(worst * streams_per_rank()) + " streams on one device exceed " +
                                       std::to_string(hwq) + " hardware queues");
            }
            if (worst > 1)
                comm_note(c.get(), "warning: " + std::to_string(worst) + " ranks share a device with " + std::to_string(worst * streams_per_rank()) + " streams on " +
                                       std::to_string(hwq) + " hardware queues -- direct collectives between them can time out (set GPU_MAX_HW_QUEUES)");
        }
    }
    if (const char* e = getenv("PPLHIP_TP_OVERLAP_MIN_TOKENS")) c->tp_overlap_min_tokens = std::max(2, atoi(e));
    if (want_comm && c->comm_want != 2) {
        std::vector<ncclComm_t> comms(n);
        // PPLHIP_EMULATE_TP=1 (measurement only): this process holds n of the tp slices but the communicator spans only
        // those n, so one GPU can time the per-rank work of a tp-way step (collectives become local identities and the
        // gathered logits are incomplete)
        if ((tp == n && !opts->nccl_unique_id) || getenv("PPLHIP_EMULATE_TP")) {
            NCCLCK(cp, -1, ncclCommInitAll(comms.data(), n, devs.data()));
        } else {
            if (!opts->nccl_unique_id) return fail(cp, -1, PPLHIP_INVALID_VALUE, "nccl_unique_id required when world_size > n_local_ranks");
            ncclUniqueId id;
            memcpy(&id, opts->nccl_unique_id, sizeof(id));
            NCCLCK(cp, -1, ncclGroupStart());
            for (int r = 0; r < n; ++r) {
                HIPCK(cp, -1, hipSetDevice(devs[r]));
                NCCLCK(cp, -1, ncclCommInitRank(&comms[r], tp, id, opts->rank_base + r));
            }
            NCCLCK(cp, -1, ncclGroupEnd());
        }
        for (int r = 0; r < n; ++r) c->ranks[r].ch[0].comm = comms[r];
        // a second communicator over the same ranks for the second stream of a two-stream decode step -- only when two-stream decode was
        // asked for explicitly (PPLHIP_DUAL_STREAM=1): the automatic mode runs on the direct collectives' second channel and never uses it
        // (plan_step), and two RCCL communicators on one device have never run on two devices
        if (c->dual_mode && !c->dual_auto) {
            std::vector<ncclComm_t> comms2(n, nullptr);
            ncclResult_t rc2 = ncclGroupStart();
            for (int r = 0; r < n && rc2 == ncclSuccess; ++r) rc2 = ncclCommSplit(comms[r], 0, opts->rank_base + r, &comms2[r], nullptr);
            const ncclResult_t rc3 = ncclGroupEnd();
            if (rc2 == ncclSuccess && rc3 == ncclSuccess) {
                for (int r = 0; r < n; ++r) c->ranks[r].ch[1].comm = comms2[r];
            } else {
                // ladder: without a second communicator a two-stream step can still run on the direct collectives (their second channel);
                // on RCCL it falls back to one stream (plan_step checks has_comm2)
                for (int r = 0; r < n; ++r) if (comms2[r]) (void)ncclCommAbort(comms2[r]);   // partially created group
                comm_note(c.get(), std::string("second RCCL communicator unavailable (") + ncclGetErrorString(rc2 != ncclSuccess ? rc2 : rc3) +
                                       "): two-stream decode only on the direct collectives, else one stream");
            }
        }
        c->comm_mode = 1;
    }

    const int64_t cap_B = opts->max_running_batch;
    const int64_t cap_T = std::max<int64_t>(opts->max_tokens_per_step, opts->max_running_batch);
    const int hd = d.hidden_dim, q = d.weight_quant_bit, g = d.weight_quant_group;
    std::vector<float> rope((size_t)d.max_position * c->D);
    pplhip_build_rope_table(rope.data(), d.max_position, c->D, d.rope_theta);

    for (int r = 0; r < n; ++r) {
        Rank& R = c->ranks[r];
        R.device = devs[r];
        R.global_rank = opts->rank_base + r;
        R.ch[1].id = 1;
        HIPCK(cp, r, hipSetDevice(R.device));
        HIPCK(cp, r, hipStreamCreateWithFlags(&R.stream, hipStreamNonBlocking));
        if (c->dual_mode) {
            HIPCK(cp, r, hipStreamCreateWithFlags(&R.stream2, hipStreamNonBlocking));
            HIPCK(cp, r, hipEventCreateWithFlags(&R.ev_fork, hipEventDisableTiming));
            HIPCK(cp, r, hipEventCreateWithFlags(&R.ev_join, hipEventDisableTiming));
        }
        if (c->tp_on) {
            HIPCK(cp, r, hipStreamCreateWithFlags(&R.comm_stream, hipStreamNonBlocking));
            for (int i = 0; i < 2; ++i) {
                HIPCK(cp, r, hipEventCreateWithFlags(&R.ev_compute[i], hipEventDisableTiming));
                HIPCK(cp, r, hipEventCreateWithFlags(&R.ev_comm[i], hipEventDisableTiming));
            }
        }
        int rc;
#define ALLOC(ptr, bytes) if ((rc = dev_alloc(cp, r, (void**)&(ptr), (uint64_t)(bytes)))) return rc
        ALLOC(R.embed, (uint64_t)d.vocab_size * hd * 2);
        ALLOC(R.norm, hd * 2);
        if ((rc = linear_alloc(cp, r, &R.output, c->vocab_local, hd, 0, 0))) return rc;
        R.layers.resize(d.num_layers);
        for (int l = 0; l < d.num_layers; ++l) {
            Layer& L = R.layers[l];
            ALLOC(L.attn_norm, hd * 2);
            ALLOC(L.ffn_norm, hd * 2);
            if ((rc = linear_alloc(cp, r, &L.wqkv, (c->H + 2 * c->Hkv) * c->D, hd, q, g))) return rc;
            if ((rc = linear_alloc(cp, r, &L.wo, hd, c->H * c->D, q, g))) return rc;
            if ((rc = linear_alloc(cp, r, &L.w13, 2 * c->inter, hd, q, g))) return rc;
            if ((rc = linear_alloc(cp, r, &L.w2, hd, c->inter, q, g, /*pad_k=*/true))) return rc;
        }
        ALLOC(R.rope, rope.size() * sizeof(float));
        HIPCK(cp, r, hipMemcpy(R.rope, rope.data(), rope.size() * sizeof(float), hipMemcpyHostToDevice));

        // step inputs
        R.cap_B = cap_B; R.cap_T = cap_T;
        const size_t step_bytes = (size_t)StepInputsBlock(nullptr, cap_T, cap_B, true).bytes;
        for (Stage& st : R.st_step) HIPCK(cp, r, st.allocate(step_bytes));
        ALLOC(R.step_dev, step_bytes);

        // activations
        ALLOC(R.h, (uint64_t)cap_T * hd * 2);
        ALLOC(R.xn, (uint64_t)cap_T * hd * 2);
        ALLOC(R.qkv, (uint64_t)cap_T * (c->H + 2 * c->Hkv) * c->D * 2);
        ALLOC(R.att, (uint64_t)cap_T * c->H * c->D * 2);
        if (!c->tp_on) {
            ALLOC(R.part, (uint64_t)cap_T * hd * 2);
            ALLOC(R.part2, (uint64_t)cap_T * hd * 2);
        } else {
            // the buffers collectives touch live in ONE fine-grained allocation that peers map (k_comm.hip); RCCL works on them too
            auto up = [](size_t v) { return (v + 4095) / 4096 * 4096; };
            R.x_part = P2P_DATA_START;
            R.x_part2 = R.x_part + up((size_t)cap_T * hd * 2);
            // a rank's reduced slice: <= half the buffer (n >= 2) -- as elements (plain all-reduce) or as whole rows (fused norm: ceil(T / 2) rows)
            const size_t slice_bytes = up(((size_t)cap_T / 2 + 1) * hd * 2 + 64);
            R.x_slice_bytes = slice_bytes;
            R.x_local = R.x_part2 + up((size_t)cap_T * hd * 2);
            for (int ch = 0; ch < (c->dual_mode ? 2 : 1); ++ch)
                for (int i = 0; i < 2; ++i) { R.ch[ch].x_scratch[i] = R.x_local; R.x_local += slice_bytes; }
            R.xbytes = R.x_local + up((size_t)cap_B * c->vocab_local * 4);
            // FINE-GRAINED device memory: the kind HIP defines as coherent between devices at system scope (what RCCL puts its
            // peer buffers in).  hipDeviceMallocUncached is NOT usable here: with several ranks on one MI355X a kernel reading
            // a buffer that the previous kernel of another stream had just written through an uncached mapping saw stale data
            // (profiles/probes/tp_matrix.sh: 8 bad steps of 36 and aborted runs, against 0 of 96 for fine-grained and plain
            // memory).  PPLHIP_P2P_XALLOC=0 (plain) / 1 (uncached) exist for that probe only.
            static const int xalloc = getenv("PPLHIP_P2P_XALLOC") ? atoi(getenv("PPLHIP_P2P_XALLOC")) : 2;
            hipError_t e = xalloc == 0 ? hipMalloc((void**)&R.xbase, R.xbytes)
                                       : hipExtMallocWithFlags((void**)&R.xbase, R.xbytes, xalloc == 1 ? hipDeviceMallocUncached : hipDeviceMallocFinegrained);
            if (e != hipSuccess) return fail(cp, r, PPLHIP_OUT_OF_MEMORY, std::string("exchange region: ") + hipGetErrorString(e));
            HIPCK(cp, r, hipMemset(R.xbase, 0, P2P_DATA_START));
            R.part = (uint16_t*)(R.xbase + R.x_part);
            R.part2 = (uint16_t*)(R.xbase + R.x_part2);
            R.logits_local = (float*)(R.xbase + R.x_local);
            if (R.ch[0].comm) ALLOC(R.logits_gather, (uint64_t)cap_B * d.vocab_size * 4);  // RCCL all-gather target
            HIPCK(cp, r, hipHostMalloc((void**)&R.p2p_status, 64, hipHostMallocMapped));
            *R.p2p_status = 0;
            ALLOC(R.d_flag, 64);
            ALLOC(R.hflags, 64);
            HIPCK(cp, r, hipMemset(R.hflags, 0, 64));
        }
        const int inter_p = (d.weight_quant_bit != 4) ? (c->inter + k_tile(cp) - 1) / k_tile(cp) * k_tile(cp) : c->inter;  // = layers[*].w2.Kp
        if (c->act_fmt != ACT_FP16) {  // online_i8i8 / f8f8: the 1-byte copy of whatever feeds the next linear + its per-token scales
            ALLOC(R.xq, (uint64_t)cap_T * std::max(std::max(hd, c->H * c->D), inter_p));
            ALLOC(R.sx, (uint64_t)cap_T * 4);
        }
        ALLOC(R.act, (uint64_t)cap_T * inter_p * 2);
        if (inter_p != c->inter) HIPCK(cp, r, hipMemset(R.act, 0, (uint64_t)cap_T * inter_p * 2));  // pad columns stay zero
        ALLOC(R.hn, (uint64_t)cap_B * hd * 2);
        ALLOC(R.logits, (uint64_t)cap_B * d.vocab_size * 4);
        R.attn_ws_bytes = attn_decode_workspace_bytes(cap_B, c->H, c->D, 32);
        ALLOC(R.attn_ws, R.attn_ws_bytes);
        R.gemm_ws_bytes = (size_t)8 * 256 * (size_t)std::max(std::max(2 * c->inter, (c->H + 2 * c->Hkv) * c->D), std::max(hd, c->vocab_local)) * sizeof(float);
        R.gemm_ws_bytes = std::max<size_t>(R.gemm_ws_bytes, (size_t)96 << 20);
        ALLOC(R.gemm_ws, R.gemm_ws_bytes);
        if (c->dual_mode) ALLOC(R.gemm_ws2, R.gemm_ws_bytes);

        if (r == 0) {  // sampler lives on local rank 0 (src/backends/cuda/resource_manager.cc:315-327)
            ALLOC(R.d_temp, cap_B * 4); ALLOC(R.d_topp, cap_B * 4); ALLOC(R.d_rand, cap_B * 4);
            ALLOC(R.d_lp, cap_B * 4); ALLOC(R.d_tokout, cap_B * 4);
            HIPCK(cp, r, hipHostMalloc((void**)&R.h_rand, cap_B * 4, hipHostMallocDefault));
            ALLOC(R.d_srows, block_bytes<SampleRowsBlock>(cap_B));
            HIPCK(cp, r, hipHostMalloc((void**)&R.h_srows, block_bytes<SampleRowsBlock>(cap_B), hipHostMallocDefault));
            ALLOC(R.d_tlp_in, block_bytes<TopLogprobsIn>(cap_B));
            HIPCK(cp, r, hipHostMalloc((void**)&R.h_tlp_in, block_bytes<TopLogprobsIn>(cap_B), hipHostMallocDefault));
            ALLOC(R.d_tlp_out, block_bytes<TopLogprobsOut>(cap_B));
            HIPCK(cp, r, hipHostMalloc((void**)&R.h_tlp_out, block_bytes<TopLogprobsOut>(cap_B), hipHostMallocDefault));
            if (opts->enable_penalty) {
                ALLOC(R.count_map, (uint64_t)cap_B * d.vocab_size * 2);
                ALLOC(R.d_slots, cap_B * 8);
                ALLOC(R.d_rep, cap_B * 4); ALLOC(R.d_pres, cap_B * 4); ALLOC(R.d_freq, cap_B * 4); ALLOC(R.d_ptemp, cap_B * 4);
                HIPCK(cp, r, hipMemsetAsync(R.count_map, 0, (uint64_t)cap_B * d.vocab_size * 2, R.stream));
            }
        }
#undef ALLOC
        HIPCK(cp, r, hipDeviceSynchronize());
    }
    // every rank of the group lives in this process: map the peers' regions now and try the direct collectives
    if (c->tp_on && c->comm_want != 1 && tp == n) {
        if (int rc = p2p_connect_local(cp)) return rc;
    }
    *out = c.release();
    return 0;
}

/* ------------------------------------------------------------------------------------------------ weights */

int pplhip_rank_set_tensor(pplhip_ctx* c, int rank, const char* name, const void* data, uint64_t bytes) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size() || !name || !data) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    void* p; uint64_t b;
    Linear* lin = nullptr;
    if (!find_tensor(c, R, name, &p, &b, &lin)) return fail(c, rank, PPLHIP_NOT_FOUND, std::string("unknown tensor ") + name);
    const char* w13 = strstr(name, "feed_forward.w13.");
    if (lin && lin->qbit == 8 && c->act_fmt != ACT_FP16 && bytes == (uint64_t)lin->N * lin->K * 2) {
        // online_i8i8 / f8f8 "online" half: an fp16 [N, K] matrix for a 1-byte linear is quantised per output row on the device
        HIPCK(c, rank, hipSetDevice(R.device));
        void *tmp = nullptr, *tmp2 = nullptr;
        HIPCK(c, rank, hipMalloc(&tmp, bytes));
        hipError_t e = hipMemcpy(tmp, data, bytes, hipMemcpyHostToDevice);
        const uint16_t* src = (const uint16_t*)tmp;
        if (e == hipSuccess && w13) {  // rows interleaved (gate_i, up_i) first: the per-row quantisation moves with the row
            e = hipMalloc(&tmp2, bytes);
            if (e == hipSuccess) e = launch_interleave_rows(R.stream, tmp, tmp2, lin->N, (int64_t)lin->K * 2);
            src = (const uint16_t*)tmp2;
        }
        if (e == hipSuccess)
            e = c->act_fmt == ACT_FP8 ? launch_quant_weight_f8(R.stream, src, lin->N, lin->K, (uint8_t*)lin->w, lin->Kp, lin->scale)
                                      : launch_quant_weight(R.stream, src, lin->N, lin->K, (int8_t*)lin->w, lin->Kp, lin->scale);
        if (e == hipSuccess) e = hipStreamSynchronize(R.stream);
        hipFree(tmp);
        if (tmp2) hipFree(tmp2);
        if (e != hipSuccess) return fail(c, rank, PPLHIP_DEVICE_RUNTIME_ERROR, std::string("online weight quantisation: ") + hipGetErrorString(e));
        return 0;
    }
    if (b != bytes) return fail(c, rank, PPLHIP_INVALID_VALUE, std::string("tensor ") + name + ": got " + std::to_string(bytes) + " bytes, want " + std::to_string(b));
    if (c->act_fmt == ACT_FP8 && !lin && strstr(name, ".scale")) {
        // online_f8f8 codes handed over as they are (N * K bytes + .scale): the row scales must be the powers of two 2^e, e in [-15, 8],
        // that the row rule produces -- a scale of any other value has no exact fp16 product with the codes
        const uint16_t* sc = (const uint16_t*)data;
        for (uint64_t i = 0; i < bytes / 2; ++i)
            if (sc[i] != 0x0200u && ((sc[i] & 0x83ffu) || sc[i] < 0x0400u || sc[i] > 0x5c00u))   // 2^-15 is the subnormal 0x0200
                return fail(c, rank, PPLHIP_INVALID_VALUE, std::string("tensor ") + name + ": online_f8f8 scales must be powers of two 2^-15 .. 2^8");
    }
    HIPCK(c, rank, hipSetDevice(R.device));
    if (w13) {
        // the container stores w13 as [gate rows | up rows]; on the device the rows are interleaved (gate_i, up_i) so
        // that the GEMM epilogue can apply SwiGLU (kernels.h: launch_linear swiglu)
        void* tmp = nullptr;
        HIPCK(c, rank, hipMalloc(&tmp, bytes));
        hipError_t e = hipMemcpy(tmp, data, bytes, hipMemcpyHostToDevice);
        const int rows = 2 * c->inter;
        if (e == hipSuccess) e = launch_interleave_rows(R.stream, tmp, p, rows, (int64_t)(bytes / rows));
        if (e == hipSuccess) e = hipStreamSynchronize(R.stream);
        hipFree(tmp);
        if (e != hipSuccess) return fail(c, rank, PPLHIP_DEVICE_RUNTIME_ERROR, std::string("interleave w13: ") + hipGetErrorString(e));
        return 0;
    }
    if (lin && lin->Kp != lin->K) {  // zero-padded rows (linear_alloc cleared the buffer)
        const size_t rb = (size_t)lin->elt_bytes(lin->K), rbp = (size_t)lin->elt_bytes(lin->Kp);
        HIPCK(c, rank, hipMemcpy2D(p, rbp, data, rb, rb, lin->N, hipMemcpyHostToDevice));
        return 0;
    }
    HIPCK(c, rank, hipMemcpy(p, data, bytes, hipMemcpyHostToDevice));
    return 0;
}

// container: "PPLHIPW1" | u32 count | count x { u32 name_len | name | u64 nbytes | pad to 64 | data }
int pplhip_rank_load(pplhip_ctx* c, int rank, const char* slice_dir) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size() || !slice_dir) return PPLHIP_INVALID_VALUE;
    const std::string path = std::string(slice_dir) + "/weights.pplhip";
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return fail(c, rank, PPLHIP_NOT_FOUND, "cannot open " + path);
    char magic[8];
    uint32_t count = 0;
    int rc = 0;
    std::vector<char> buf;
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "PPLHIPW1", 8) || fread(&count, 4, 1, f) != 1) {
        fclose(f);
        return fail(c, rank, PPLHIP_INVALID_VALUE, "bad header in " + path);
    }
    for (uint32_t i = 0; i < count && !rc; ++i) {
        uint32_t nl = 0; uint64_t nb = 0;
        char name[256];
        if (fread(&nl, 4, 1, f) != 1 || nl >= sizeof(name) || fread(name, 1, nl, f) != nl || fread(&nb, 8, 1, f) != 1) { rc = PPLHIP_INVALID_VALUE; break; }
        name[nl] = 0;
        long pos = ftell(f);
        long pad = (64 - pos % 64) % 64;
        fseek(f, pad, SEEK_CUR);
        buf.resize(nb);
        if (fread(buf.data(), 1, nb, f) != nb) { rc = PPLHIP_INVALID_VALUE; break; }
        rc = pplhip_rank_set_tensor(c, rank, name, buf.data(), nb);
    }
    fclose(f);
    if (rc == PPLHIP_INVALID_VALUE && c->ranks[rank].err.empty()) fail(c, rank, rc, "truncated container " + path);
    return rc;
}

int pplhip_rank_init_synthetic(pplhip_ctx* c, int rank, uint64_t seed) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    HIPCK(c, rank, hipSetDevice(R.device));
    const int hd = c->d.hidden_dim;
    const uint32_t st = 1u + (uint32_t)R.global_rank;
    const float AMP = 0.034641016f;
    auto tid = [](int layer, int slot) { return (uint32_t)((layer + 1) * 32 + slot); };
    hipStream_t s = R.stream;
    auto lin = [&](Linear& l, int layer, int wslot) -> hipError_t {
        hipError_t e;
        if (l.qbit == 0) return launch_synth_fill(s, 0, seed, tid(layer, wslot), st, AMP, (uint64_t)l.N * l.K, l.w);
        if (c->act_fmt == ACT_FP8) {   // online_f8f8: the fp16 weights of an fp16 desc with this seed, quantised on the device (rows of K)
            void* w16 = nullptr;
            if ((e = hipMalloc(&w16, (uint64_t)l.N * l.K * 2)) != hipSuccess) return e;
            e = launch_synth_fill(s, 0, seed, tid(layer, wslot), st, AMP, (uint64_t)l.N * l.K, w16);
            if (e == hipSuccess) e = launch_quant_weight_f8(s, (const uint16_t*)w16, l.N, l.K, (uint8_t*)l.w, l.K, l.scale);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            hipFree(w16);
            return e;
        }
        if (l.qbit == 8) {
            if ((e = launch_synth_fill(s, 1, seed, tid(layer, wslot), st, 0.f, (uint64_t)l.N * l.K, l.w)) != hipSuccess) return e;
            return launch_synth_fill(s, 3, seed, tid(layer, wslot + 1), st, AMP / 127.0f, (uint64_t)l.N, l.scale);
        }
        if ((e = launch_synth_fill(s, 2, seed, tid(layer, wslot), st, 0.f, (uint64_t)l.N * l.K / 2, l.w)) != hipSuccess) return e;
        return launch_synth_fill(s, 3, seed, tid(layer, wslot + 1), st, AMP / 7.0f, (uint64_t)l.N * (l.K / l.group), l.scale);
    };
    HIPCK(c, rank, launch_synth_fill(s, 0, seed, tid(-1, 0), 0, 1.0f, (uint64_t)c->d.vocab_size * hd, R.embed));
    HIPCK(c, rank, launch_synth_fill(s, 4, seed, tid(-1, 11), 0, 0.f, hd, R.norm));
    HIPCK(c, rank, launch_synth_fill(s, 0, seed, tid(-1, 12), st, AMP, (uint64_t)c->vocab_local * hd, R.output.w));
    for (int l = 0; l < c->d.num_layers; ++l) {
        Layer& L = R.layers[l];
        HIPCK(c, rank, launch_synth_fill(s, 4, seed, tid(l, 1), 0, 0.f, hd, L.attn_norm));
        HIPCK(c, rank, launch_synth_fill(s, 4, seed, tid(l, 6), 0, 0.f, hd, L.ffn_norm));
        HIPCK(c, rank, lin(L.wqkv, l, 2));
        HIPCK(c, rank, lin(L.wo, l, 4));
        {   // generated in container order, then row-interleaved like an uploaded tensor
            Linear tmp = L.w13;
            HIPCK(c, rank, hipMalloc(&tmp.w, L.w13.w_bytes()));
            if (L.w13.s_bytes()) HIPCK(c, rank, hipMalloc((void**)&tmp.scale, L.w13.s_bytes()));
            HIPCK(c, rank, lin(tmp, l, 7));
            HIPCK(c, rank, launch_interleave_rows(s, tmp.w, L.w13.w, L.w13.N, (int64_t)(L.w13.w_bytes() / L.w13.N)));
            if (L.w13.s_bytes()) HIPCK(c, rank, launch_interleave_rows(s, tmp.scale, L.w13.scale, L.w13.N, (int64_t)(L.w13.s_bytes() / L.w13.N)));
            HIPCK(c, rank, hipStreamSynchronize(s));
            hipFree(tmp.w);
            if (tmp.scale) hipFree(tmp.scale);
        }
        if (L.w2.Kp == L.w2.K) {
            HIPCK(c, rank, lin(L.w2, l, 9));
        } else {  // generated contiguous, then copied into the zero-padded rows
            Linear tmp = L.w2;
            HIPCK(c, rank, hipMalloc(&tmp.w, L.w2.w_bytes()));
            HIPCK(c, rank, lin(tmp, l, 9));  // scale goes straight to L.w2.scale (same pointer)
            const size_t rb = (size_t)L.w2.elt_bytes(L.w2.K), rbp = (size_t)L.w2.elt_bytes(L.w2.Kp);
            HIPCK(c, rank, hipMemcpy2DAsync(L.w2.w, rbp, tmp.w, rb, rb, L.w2.N, hipMemcpyDeviceToDevice, s));
            HIPCK(c, rank, hipStreamSynchronize(s));
            hipFree(tmp.w);
        }
    }
    HIPCK(c, rank, hipStreamSynchronize(s));
    return 0;
}

/* ------------------------------------------------------------------------------------------------ KV slab */

// A DECISIVE synthetic model: the embedding table is regenerated at amplitude `embed_amp` (the synthetic default is 1; behind 32 synthetic
// layers the residual stream has an rms of ~10, which buries a unit-amplitude embedding: profiles/r05_tie_probe.log) and
// output.weight[v] := tok_embeddings.weight[(v - shift) mod vocab] on this rank's vocabulary shard.  The final hidden state of a position
// then keeps a strong component along its own token's embedding, so token t is answered by t + shift with a top-2 margin of a third or more of the
// logit scale -- far above what two evaluation orders of the same arithmetic differ by.  For harness checks that compare ANSWERS of two
// runs (benchmark_prefix_cache_offline --synthetic-decisive-head: cold run vs prefix-cache hits); what such a check pins is the
// bookkeeping of the path (pages, start positions, hand-over of tokens), not its arithmetic.
int pplhip_rank_tie_output(pplhip_ctx* c, int rank, int64_t shift, uint64_t seed, float embed_amp) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    if (R.output.qbit != 0) return fail(c, rank, PPLHIP_INVALID_VALUE, "tie_output: the lm_head is fp16");
    HIPCK(c, rank, hipSetDevice(R.device));
    const int64_t V = c->d.vocab_size, hd = c->d.hidden_dim, v0 = (int64_t)R.global_rank * c->vocab_local;
    if (embed_amp > 0.f) HIPCK(c, rank, launch_synth_fill(R.stream, 0, seed, (uint32_t)(0 * 32 + 0), 0, embed_amp, (uint64_t)V * hd, R.embed));   // tensor id of pplhip_rank_init_synthetic's embedding
    shift = ((shift % V) + V) % V;
    for (int64_t v = 0; v < c->vocab_local;) {          // at most two contiguous runs
        const int64_t src = ((v0 + v - shift) % V + V) % V;
        const int64_t n = std::min<int64_t>(c->vocab_local - v, V - src);
        HIPCK(c, rank, hipMemcpyAsync((char*)R.output.w + v * hd * 2, (const char*)R.embed + src * hd * 2, (size_t)n * hd * 2, hipMemcpyDeviceToDevice, R.stream));
        v += n;
    }
    HIPCK(c, rank, hipStreamSynchronize(R.stream));
    return 0;
}

int pplhip_kv_block_bytes(pplhip_ctx* c, uint64_t* cache_bytes, uint64_t* scale_bytes) {
    if (!c) return PPLHIP_INVALID_VALUE;
    // src/backends/cuda/resource_manager.cc:381-387
    const uint64_t kb = (uint64_t)c->d.num_layers * 2 * c->Hkv * (uint64_t)kv_row_bytes(c->d.cache_quant_bit, c->D);
    const uint64_t sb = c->d.cache_quant_bit > 0 ? (uint64_t)c->d.num_layers * 2 * c->Hkv * (c->D / c->d.cache_quant_group) * 2 : 0;
    if (cache_bytes) *cache_bytes = kb;
    if (scale_bytes) *scale_bytes = sb;
    return 0;
}

int pplhip_kv_capacity(pplhip_ctx* c, float max_tokens_scale, uint64_t* tokens) {
    if (!c || !tokens) return PPLHIP_INVALID_VALUE;
    uint64_t kb, sb;
    pplhip_kv_block_bytes(c, &kb, &sb);
    HIPCK(c, 0, hipSetDevice(c->ranks[0].device));
    size_t free_b = 0, total = 0;
    HIPCK(c, 0, hipMemGetInfo(&free_b, &total));
    // resource_manager.cc:330-341
    const uint64_t kv_cache_max_bytes = (uint64_t)((double)max_tokens_scale * (double)free_b * (double)kb / (double)(kb + sb));
    *tokens = kv_cache_max_bytes / kb;
    return 0;
}

int pplhip_kv_alloc(pplhip_ctx* c, int rank, uint64_t tokens) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size() || tokens == 0) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    HIPCK(c, rank, hipSetDevice(R.device));
    uint64_t kb, sb;
    pplhip_kv_block_bytes(c, &kb, &sb);
    if (R.kv_cache) { hipFree(R.kv_cache); R.kv_cache = nullptr; }
    if (R.kv_scale) { hipFree(R.kv_scale); R.kv_scale = nullptr; }
    hipError_t e = hipMalloc(&R.kv_cache, tokens * kb);
    if (e != hipSuccess) return fail(c, rank, PPLHIP_OUT_OF_MEMORY, "alloc kv cache [" + std::to_string(tokens * kb) + "] failed: " + hipGetErrorString(e));
    if (sb) {
        e = hipMalloc((void**)&R.kv_scale, tokens * sb);
        if (e != hipSuccess) {
            hipFree(R.kv_cache); R.kv_cache = nullptr;
            return fail(c, rank, PPLHIP_OUT_OF_MEMORY, "alloc kv scale [" + std::to_string(tokens * sb) + "] failed: " + hipGetErrorString(e));
        }
    }
    // deterministic contents for never-written slots (the reference's cudaMalloc leaves them undefined)
    // stream-ordered on the rank's own (non-blocking) stream: a null-stream memset is NOT ordered against it and could
    // land after the first steps have written the slab
    HIPCK(c, rank, hipMemsetAsync(R.kv_cache, 0, tokens * kb, R.stream));
    if (sb) HIPCK(c, rank, hipMemsetAsync(R.kv_scale, 0, tokens * sb, R.stream));
    HIPCK(c, rank, hipStreamSynchronize(R.stream));
    R.kv_tokens = tokens;
    return 0;
}

int pplhip_kv_ptrs(pplhip_ctx* c, int rank, void** kv_cache_mem, void** kv_scale_mem) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    if (kv_cache_mem) *kv_cache_mem = c->ranks[rank].kv_cache;
    if (kv_scale_mem) *kv_scale_mem = c->ranks[rank].kv_scale;
    return 0;
}

static int kv_rw(pplhip_ctx* c, int rank, int which, uint64_t offset, void* host, uint64_t bytes, bool read) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size() || !host) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    uint64_t kb, sb;
    pplhip_kv_block_bytes(c, &kb, &sb);
    char* base = which ? (char*)R.kv_scale : (char*)R.kv_cache;
    const uint64_t total = R.kv_tokens * (which ? sb : kb);
    if (!base || offset + bytes > total) return fail(c, rank, PPLHIP_INVALID_VALUE, "kv read/write out of range");
    HIPCK(c, rank, hipSetDevice(R.device));
    HIPCK(c, rank, hipStreamSynchronize(R.stream));
    if (read) HIPCK(c, rank, hipMemcpy(host, base + offset, bytes, hipMemcpyDeviceToHost));
    else HIPCK(c, rank, hipMemcpy(base + offset, host, bytes, hipMemcpyHostToDevice));
    return 0;
}
int pplhip_kv_read(pplhip_ctx* c, int rank, int which, uint64_t offset, void* dst, uint64_t bytes) {
    return kv_rw(c, rank, which, offset, dst, bytes, true);
}
int pplhip_kv_write(pplhip_ctx* c, int rank, int which, uint64_t offset, const void* src, uint64_t bytes) {
    return kv_rw(c, rank, which, offset, const_cast<void*>(src), bytes, false);
}

int pplhip_kv_fill_synthetic(pplhip_ctx* c, int rank, uint64_t seed) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    if (!R.kv_cache) return fail(c, rank, PPLHIP_INVALID_VALUE, "kv slab not allocated");
    HIPCK(c, rank, hipSetDevice(R.device));
    uint64_t kb, sb;
    pplhip_kv_block_bytes(c, &kb, &sb);
    const uint32_t st = 100u + (uint32_t)R.global_rank;
    if (c->kv_fmt == KV_FP8) {   // finite e4m3 codes and power-of-two row scales
        HIPCK(c, rank, launch_synth_fill(R.stream, 5, seed, 1, st, 0.f, R.kv_tokens * kb, R.kv_cache));
        HIPCK(c, rank, launch_synth_fill(R.stream, 6, seed, 2, st, 0.f, R.kv_tokens * sb / 2, R.kv_scale));
    } else if (c->kv_fmt == KV_I4G32) {   // nibbles 1..15 and scales of the format's rule
        HIPCK(c, rank, launch_synth_fill(R.stream, 7, seed, 1, st, 0.f, R.kv_tokens * kb, R.kv_cache));
        HIPCK(c, rank, launch_synth_fill(R.stream, 8, seed, 2, st, 0.f, R.kv_tokens * sb / 2, R.kv_scale));
    } else if (c->kv_fmt == KV_I8G8) {
        HIPCK(c, rank, launch_synth_fill(R.stream, 1, seed, 1, st, 0.f, R.kv_tokens * kb, R.kv_cache));
        HIPCK(c, rank, launch_synth_fill(R.stream, 3, seed, 2, st, 0.02f, R.kv_tokens * sb / 2, R.kv_scale));
    } else {
        HIPCK(c, rank, launch_synth_fill(R.stream, 0, seed, 1, st, 1.5f, R.kv_tokens * kb / 2, R.kv_cache));
    }
    HIPCK(c, rank, hipStreamSynchronize(R.stream));
    return 0;
}

/* ------------------------------------------------------------------------------------------------ the step */

int pplhip_set_inputs(pplhip_ctx* c, int rank, const pplhip_step* st) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size() || !st) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    R.lora_ntiles = 0;   // the adapter assignment belongs to one step (pplhip_set_adapters)
    R.lora_stale = false;
    R.plp_n = 0;         // so does the prompt-logprobs ask (pplhip_set_prompt_logprobs)
    R.plp_top = false;
    const int64_t B = st->batch, T = st->num_tokens;
    if (B < 0 || T < 0 || B > R.cap_B || T > R.cap_T)
        return fail(c, rank, PPLHIP_INVALID_VALUE, "step exceeds max_running_batch / max_tokens_per_step");
    if (B == 0) {  // an empty step is legal (LLMGenerator never sends one, llm_generator.cc:658-660) and does nothing
        if (T != 0) return fail(c, rank, PPLHIP_INVALID_VALUE, "tokens without requests");
        R.B = 0; R.T = 0; R.decoding_batches = 0; R.h_seq = nullptr;
        return 0;
    }
    if (!st->token_inputs || !st->seq_starts || !st->kv_starts || !st->start_pos) return PPLHIP_INVALID_VALUE;
    if (st->max_kv_len > c->d.max_position) return fail(c, rank, PPLHIP_INVALID_VALUE, "max_kv_len exceeds max_position");
    {   // the kernels index the rope table, the embedding table and the KV slab with these values: reject anything that
        // would leave them (O(B + T) on the host; the reference trusts its generator, this boundary does not)
        const int64_t* ss = st->seq_starts;
        if (ss[0] != 0 || ss[B] != T) return fail(c, rank, PPLHIP_INVALID_VALUE, "seq_starts must run from 0 to num_tokens");
        if (st->decoding_batches < 0 || st->decoding_batches > B) return fail(c, rank, PPLHIP_INVALID_VALUE, "decoding_batches out of range");
        const int64_t P = c->d.page_size > 0 ? c->d.page_size : 1;
        for (int64_t b = 0; b < B; ++b) {
            const int64_t len = ss[b + 1] - ss[b], sp = st->start_pos[b];
            if (len <= 0) return fail(c, rank, PPLHIP_INVALID_VALUE, "request " + std::to_string(b) + " has no tokens");
            if (b < st->decoding_batches && len != 1) return fail(c, rank, PPLHIP_INVALID_VALUE, "decode request " + std::to_string(b) + " must have one token");
            if (sp < 0 || sp + len > c->d.max_position) return fail(c, rank, PPLHIP_INVALID_VALUE, "request " + std::to_string(b) + " exceeds max_position");
            if (c->d.cache_mode == 0) {
                const int64_t ci = st->cache_indices ? st->cache_indices[b] : -1;
                if (ci < 0 || (uint64_t)(ci + sp + len) > R.kv_tokens)
                    return fail(c, rank, PPLHIP_INVALID_VALUE, "request " + std::to_string(b) + ": KV range outside the slab");
            } else if (st->req_list_changed && st->cache_indices && st->max_pages > 0) {
                const int64_t need = (sp + len + P - 1) / P;
                if (need > st->max_pages) return fail(c, rank, PPLHIP_INVALID_VALUE, "request " + std::to_string(b) + ": page list too short");
                for (int64_t pg = 0; pg < need; ++pg) {
                    const int64_t id = st->cache_indices[b * st->max_pages + pg];
                    if (id < 0 || (uint64_t)id >= R.kv_tokens / (uint64_t)P)  // (also catches the INT64_MAX padding)
                        return fail(c, rank, PPLHIP_INVALID_VALUE, "request " + std::to_string(b) + ": page outside the slab");
                }
            }
        }
        for (int64_t t = 0; t < T; ++t)
            if (st->token_inputs[t] < 0 || st->token_inputs[t] >= c->d.vocab_size)
                return fail(c, rank, PPLHIP_INVALID_VALUE, "token id outside the vocabulary at row " + std::to_string(t));
    }
    HIPCK(c, rank, hipSetDevice(R.device));
    const bool contiguous = c->d.cache_mode == 0;   // (cache_indices != NULL then: the range check above refused a step without them)
    Stage& stage = R.st_step[R.st_step_cur];
    R.st_step_cur ^= 1;
    char* hbuf;
    HIPCK(c, rank, stage.begin(&hbuf));
    const StepInputsBlock h(hbuf, T, B, contiguous), dv(R.step_dev, T, B, contiguous);
    memcpy(h.token_ids, st->token_inputs, T * 8);
    memcpy(h.seq_starts, st->seq_starts, (B + 1) * 8);
    memcpy(h.kv_starts, st->kv_starts, (B + 1) * 8);
    memcpy(h.start_pos, st->start_pos, B * 8);
    if (contiguous) memcpy(h.cache_indices, st->cache_indices, B * 8);
    R.d_tok = dv.token_ids; R.d_seq = dv.seq_starts; R.d_kvs = dv.kv_starts; R.d_sp = dv.start_pos;
    if (contiguous) R.d_ci = dv.cache_indices;
    R.h_seq = h.seq_starts;
    HIPCK(c, rank, stage.upload(R.step_dev, (size_t)h.bytes, R.stream));
    if (c->d.cache_mode == 1 && st->req_list_changed) {  // src/engine/llm_engine.cc:67-71
        if (!st->cache_indices || st->max_pages <= 0) return fail(c, rank, PPLHIP_INVALID_VALUE, "page list missing");
        const uint64_t n = (uint64_t)B * st->max_pages;
        if (n > R.pages_cap) {
            HIPCK(c, rank, hipStreamSynchronize(R.stream));
            if (R.pages_dev) hipFree(R.pages_dev);
            if (R.pages_host) hipHostFree(R.pages_host);
            R.pages_cap = std::max<uint64_t>(n * 2, 4096);
            HIPCK(c, rank, hipMalloc((void**)&R.pages_dev, R.pages_cap * 8));
            HIPCK(c, rank, hipHostMalloc((void**)&R.pages_host, R.pages_cap * 8, hipHostMallocDefault));
        } else {
            HIPCK(c, rank, hipStreamSynchronize(R.stream));  // previous async copy from pages_host
        }
        memcpy(R.pages_host, st->cache_indices, n * 8);
        HIPCK(c, rank, hipMemcpyAsync(R.pages_dev, R.pages_host, n * 8, hipMemcpyHostToDevice, R.stream));
        R.max_pages = st->max_pages;
    }
    if (c->d.cache_mode == 1) R.d_ci = R.pages_dev;
    R.B = B; R.T = T;
    R.decoding_batches = st->decoding_batches;
    R.max_seq_len = st->max_seq_len;
    R.max_kv_len = st->max_kv_len;
    return 0;
}

enum { SCHED_ONE_LANE = 0, SCHED_TWO_LANES = 1, SCHED_TWO_CHUNKS = 2 };   // pplhip_comm_info_t.schedule

// what plan_step needs of the context and the rank, as they stand now (comm_mode changes when the ranks connect)
pplhip_plan_settings plan_settings(const pplhip_ctx* c, const Rank& R) {
    pplhip_plan_settings s;
    memset(&s, 0, sizeof(s));
    s.tp = c->tp; s.tp_on = c->tp_on; s.comm_mode = c->comm_mode;
    s.has_comm = R.ch[0].comm != nullptr; s.has_comm2 = R.ch[1].comm != nullptr;
    s.emulate_tp = c->emulate_tp;
    s.tp_overlap = c->tp_overlap; s.tp_overlap_min_tokens = c->tp_overlap_min_tokens;
    s.dual_mode = c->dual_mode; s.dual_auto = c->dual_auto; s.has_stream2 = R.stream2 != nullptr;
    s.dual_min_rows = c->dual_min_rows; s.dual_max_rows = c->dual_max_rows;
    s.fuse_norm_want = c->fuse_norm_want; s.defer_on = c->defer_on;
    s.act_fmt = c->act_fmt;
    s.hidden_dim = c->d.hidden_dim; s.heads = c->H; s.kv_heads = c->Hkv; s.head_dim = c->D;
    s.cache_quant_bit = c->d.cache_quant_bit; s.cache_quant_group = c->d.cache_quant_group;
    s.decoding_attn_split_k = c->o.decoding_attn_split_k;
    return s;
}

// the sequence-parallel residual stream is in force for this rank's steps (pplhip_ctx::fuse_norm_want)
bool fuse_norm_active(const pplhip_plan_settings& s, bool dump) {
    const int hd = s.hidden_dim;
    return s.fuse_norm_want && s.tp_on && s.tp > 1 && s.act_fmt == ACT_FP16 && !dump && hd % 8 == 0 && hd <= P2P_NORM_MAX_HIDDEN &&
           (s.comm_mode == 2 || s.emulate_tp);
}

// The schedule of one step: a pure function of the settings and the step's shape (no HIP call, no environment read), so that what a
// step runs (run_launches), what pplhip_comm_info reports and what the tests check (pplhip_op_step_plan) are one decision.
StepPlan plan_step(const pplhip_plan_settings& s, const pplhip_step_shape& sh) {
    StepPlan p;
    memset(&p, 0, sizeof(p));
    const int64_t B = sh.batch, T = sh.num_tokens;
    const int64_t nb_decode = std::min<int64_t>(std::max<int64_t>(sh.decoding_batches, 0), B);
    const bool comm = s.tp_on, dump = sh.dump != 0;
    p.schedule = SCHED_ONE_LANE;
    p.chunk[0] = Chunk{0, B, 0, T, nb_decode};
    // Tensor parallel: the step is cut at a request boundary into two chunks of about T/2 rows.  While the collective reduces
    // the partial sums of one chunk on the communication stream, the compute stream runs the other chunk's block
    // (attention part or FFN part), so the xGMI time hides under the matmuls instead of adding to them.
    // Two-lane decode (PPLHIP_DUAL_STREAM=1): a pure-decode step of dual_min_rows..dual_max_rows rows is cut into two half-batches that run
    // their layers on two streams, side by side.  At these sizes no kernel of the step fills the chip -- the linears are 20-256 tiles with
    // short K loops, the attention launch a few hundred blocks -- so the halves' kernels interleave on the CUs instead of queueing behind each
    // other's ramps and tails, and one half's HBM-bound attention runs beside the other's matrix work.  The halves share nothing but the
    // weights and the KV slab: rows [t0, t0 + tn) of every activation buffer, a split-K workspace and an attention workspace each (Lane).
    // Results are those of the same rows run as a step of their own.  Under tensor parallelism every half issues its all-reduces on its OWN
    // stream and channel (direct collectives: a second flag set / scratch pair / epoch counter, k_comm.hip; RCCL: a second communicator over
    // the same ranks) -- the all-reduce of one half runs beside the other half's matmuls with no hand-off kernels and no extra launches,
    // which is what the chunked schedule pays +3.5 ms per 1024-row step for.  Not with int8 / fp8 activations (shared operand buffer),
    // residual dumps or graph capture.
    const bool identity_comm = comm && s.comm_mode != 2 && !s.has_comm;   // ranks emulated on one device (bench.py --emulate-tp)
    const bool lanes_ok = !sh.lora;   // a step with adapter rows: one lane, one chunk (the tile list names rows of the whole step)
    if (lanes_ok && comm && s.tp_overlap && sh.seq_starts && T >= s.tp_overlap_min_tokens && B >= 2) {
        int64_t bm = 1, tm;
        if (nb_decode == B) {   // pure decode: whole 128-row GEMM tiles in the first chunk (row i is request i: seq_starts is not read)
            const int64_t r = (T / 2 + 127) / 128 * 128;
            tm = bm = r < B ? r : B / 2;
        } else {
            while (bm < B - 1 && sh.seq_starts[bm] < T / 2) ++bm;  // first request boundary at or after row T/2
            tm = sh.seq_starts[bm];
        }
        p.chunk[0] = Chunk{0, bm, 0, tm, std::min(nb_decode, bm)};
        p.chunk[1] = Chunk{bm, B - bm, tm, T - tm, std::max<int64_t>(0, nb_decode - bm)};
        p.schedule = SCHED_TWO_CHUNKS;
    } else if (lanes_ok && s.dual_mode && s.has_stream2 && nb_decode == B && T == B && B >= s.dual_min_rows && B <= s.dual_max_rows && B >= 2 &&
               (!comm || identity_comm || s.comm_mode == 2 || (s.has_comm && s.has_comm2 && !s.dual_auto)) && s.act_fmt == ACT_FP16 && !dump &&
               !sh.capturing) {
        const int64_t bm = B >= 64 ? (B / 2 + 15) / 16 * 16 : B / 2;   // whole 16-row activation sub-tiles in the first half
        p.chunk[0] = Chunk{0, bm, 0, bm, bm};
        p.chunk[1] = Chunk{bm, B - bm, bm, B - bm, B - bm};
        p.schedule = SCHED_TWO_LANES;
        p.lane1_ws_off = bm * (int64_t)s.heads * 32 * (s.head_dim + 2);   // floats: past every row the first half can use
    }
    p.num_chunks = p.schedule == SCHED_ONE_LANE ? 1 : 2;
    for (int i = 0; i < 2; ++i) p.decode_split[i] = i < p.num_chunks && p.chunk[i].nd > 0 ? decode_split(s, p.chunk[i].nd, sh.max_kv_len) : 1;
    p.fuse_norm = fuse_norm_active(s, dump);
    // split-K slabs stay unreduced for their consumer: at tensor-parallel size 1, weight-only quantisation, no residual dump, no chunks on the
    // communication stream; wqkv's slabs alone also under tensor parallelism (RoPE + KV write consumes them on the rank itself, while wo / w2
    // feed the all-reduce: their slabs are summed first)
    p.defer_qkv = s.defer_on && s.act_fmt == ACT_FP16 && !dump && p.schedule != SCHED_TWO_CHUNKS && !sh.lora;
    p.defer_reduce = p.defer_qkv && !comm;
    return p;
}

Lane make_lane(Rank& R, int i, int64_t attn_ws_off) {
    Lane ln;
    ln.stream = i ? R.stream2 : R.stream;
    ln.gemm_ws = i ? R.gemm_ws2 : R.gemm_ws;
    ln.attn_ws = R.attn_ws + attn_ws_off;
    ln.attn_ws_bytes = R.attn_ws_bytes - (size_t)attn_ws_off * 4;
    ln.ch = &R.ch[i];
    return ln;
}

// one layer linear over a chunk: fp16 activations straight into the (weight-only quantised) GEMM, or -- online_i8i8 / f8f8 -- quantised
// per token first and multiplied in int8 / e4m3.  x rows have stride l.Kp.
// pre_quantised: R.xq / R.sx already hold the rows (written by the RMSNorm in front of wqkv / w13).
// defer: where the launch may leave its split-K slabs unreduced (the plan's defer flags decide; NULL: it reduces them itself)
static int layer_linear(pplhip_ctx* c, int rank, Lane& lane, const Linear& l, const uint16_t* x, int64_t M, void* y, int64_t ldy, bool swiglu,
                        bool pre_quantised = false, SplitSlabs* defer = nullptr) {
    Rank& R = c->ranks[rank];
    hipStream_t s = lane.stream;
    if (c->act_fmt == ACT_FP8) {
        if (!pre_quantised) HIPCK(c, rank, launch_quant_act_f8(s, x, M, l.Kp, l.Kp, (uint8_t*)R.xq, l.Kp, R.sx));
        HIPCK(c, rank, launch_linear_f8(s, (const uint8_t*)R.xq, R.sx, (const uint8_t*)l.w, l.scale, M, l.N, l.Kp, y, ldy, false, swiglu));
        return 0;
    }
    if (c->act_fmt == ACT_I8) {
        if (!pre_quantised) HIPCK(c, rank, launch_quant_act(s, x, M, l.Kp, l.Kp, R.xq, l.Kp, R.sx));
        HIPCK(c, rank, launch_linear_i8(s, R.xq, R.sx, (const int8_t*)l.w, l.scale, M, l.N, l.Kp, y, ldy, false, swiglu));
        return 0;
    }
    HIPCK(c, rank, launch_linear(s, x, l.w, l.scale, l.qbit, l.group, M, l.N, l.Kp, y, ldy, false, lane.gemm_ws, R.gemm_ws_bytes, swiglu, defer));
    return 0;
}

// the low-rank update of one target linear of layer l on the step's adapter rows (k_lora.hip), right behind the linear that wrote y.  The
// tile list names absolute token rows: x and y are the whole step's matrices (a step with adapter rows is one chunk on one lane)
static int layer_lora(pplhip_ctx* c, int rank, Lane& lane, int l, int target, const uint16_t* x, int64_t ldx, uint16_t* y, int N, int K) {
    Rank& R = c->ranks[rank];
    if (R.lora_ntiles <= 0 || !R.lora_touch[(size_t)l * LORA_TARGETS + target]) return 0;
    ProfEvent ev;
    prof_begin(c, R, lane, PPLHIP_PROF_LORA, &ev);
    HIPCK(c, rank, launch_lora(lane.stream, R.lora_tiles, R.lora_ntiles, R.lora_tab + ((size_t)l * LORA_TARGETS + target) * LORA_MAX_SLOTS, x, ldx,
                               y, N, N, K, R.lora_t));
    prof_end(R, lane, &ev);
    return 0;
}

// attention block of layer l for one chunk: (Skip)RMSNorm -> wqkv -> RoPE + KV write -> attention -> wo (partial sums)
// xn_ready: the fused collective of the previous half-layer already left this block's normalised input in R.xn (and the residual in R.h)
static int layer_attention_part(pplhip_ctx* c, int rank, Lane& lane, const StepPlan& p, int l, const Chunk& k, const uint16_t* pending, int split,
                                int threads, bool xn_ready = false) {
    Rank& R = c->ranks[rank];
    const pplhip_model_desc& d = c->d;
    hipStream_t s = lane.stream;
    const int hd = d.hidden_dim, H = c->H, Hkv = c->Hkv, D = c->D;
    const int nqkv = (H + 2 * Hkv) * D;
    Layer& L = R.layers[l];
    ProfEvent ev;
    uint16_t* h = R.h + k.t0 * hd;
    uint16_t* xn = R.xn + k.t0 * hd;
    const bool a8 = c->act_fmt != ACT_FP16;  // the norm writes the 1-byte operand of the next linear directly (no fp16 xn, no separate pass)
    if (!xn_ready)
        HIPCK(c, rank, launch_rmsnorm(s, h, pending ? pending + k.t0 * hd : nullptr, L.attn_norm, d.norm_eps, k.tn, hd, nullptr, xn,
                                      pending ? h : nullptr, a8 ? R.xq : nullptr, a8 ? R.sx : nullptr, pending ? &lane.sl_part2 : nullptr,
                                      c->act_fmt == ACT_FP8));
    lane.sl_part2 = SplitSlabs{};
    prof_begin(c, R, lane, PPLHIP_PROF_GEMM, &ev);
    if (int rc = layer_linear(c, rank, lane, L.wqkv, xn, k.tn, R.qkv + k.t0 * nqkv, L.wqkv.N, false, a8, p.defer_qkv ? &lane.sl_qkv : nullptr)) return rc;
    prof_end(R, lane, &ev);
    if (int rc = layer_lora(c, rank, lane, l, LORA_WQKV, R.xn, hd, R.qkv, nqkv, hd)) return rc;
    const KvAddr kv = make_kv_addr(d, Hkv, D, R.kv_tokens, R.kv_cache, R.kv_scale, l);
    HIPCK(c, rank, launch_rope_kv_write(s, R.qkv, R.rope, kv, c->kv_fmt, R.d_seq, R.d_sp, R.d_ci,
                                        R.max_pages, R.B, k.t0, k.tn, H, Hkv, D, &lane.sl_qkv));
    lane.sl_qkv = SplitSlabs{};
    // decode rows of the chunk: per-request arrays shifted to the chunk (q rows stay absolute through seq_starts);
    // prefill requests: absolute request range
    const int64_t ci_stride = d.cache_mode == 1 ? R.max_pages : 1;
    if (k.nd > 0) {
        // light profiling: the launch carries its own start / stop events (timestamps of the dispatch packet, no barrier
        // packets on the stream; with split-K the reduce kernel is not included)
        const bool light = c->o.enable_profiling == 2;
        prof_begin(c, R, lane, PPLHIP_PROF_ATTN_DECODE, &ev);   // (light: does nothing)
        if (light) {
            std::pair<hipEvent_t, hipEvent_t> pr;
            if (!R.prof_free.empty()) { pr = R.prof_free.back(); R.prof_free.pop_back(); }
            else { hipEventCreate(&pr.first); hipEventCreate(&pr.second); }
            ev.cls = PPLHIP_PROF_ATTN_DECODE; ev.a = pr.first; ev.b = pr.second;
        }
        HIPCK(c, rank, launch_attn_decode(s, R.qkv, kv, c->kv_fmt, R.d_seq + k.b0, R.d_sp + k.b0, R.d_ci + k.b0 * ci_stride,
                                          R.max_pages, k.nd, H, Hkv, D, R.max_kv_len, split, threads, lane.attn_ws,
                                          R.att + k.b0 * (int64_t)H * D, light ? ev.a : nullptr, light ? ev.b : nullptr));
        if (light) R.prof.push_back(ev);
        else prof_end(R, lane, &ev);
    }
    if (k.bn > k.nd) {
        prof_begin(c, R, lane, PPLHIP_PROF_ATTN_PREFILL, &ev);
        // (decode requests own one token row each, so the prefill requests' rows are [t0 + nd, t0 + tn): the split-KV form for short suffixes)
        HIPCK(c, rank, launch_attn_prefill(s, R.qkv, kv, c->kv_fmt, R.d_seq, R.d_sp, R.d_ci, R.max_pages, k.b0 + k.nd,
                                           k.b0 + k.bn, H, Hkv, D, R.max_seq_len, R.att, R.max_kv_len, lane.attn_ws, lane.attn_ws_bytes,
                                           k.t0 + k.nd, k.tn - k.nd));
        prof_end(R, lane, &ev);
    }
    prof_begin(c, R, lane, PPLHIP_PROF_GEMM, &ev);
    if (int rc = layer_linear(c, rank, lane, L.wo, R.att + k.t0 * (int64_t)H * D, k.tn, R.part + k.t0 * hd, hd, false, false,
                              p.defer_reduce ? &lane.sl_part : nullptr))
        return rc;
    prof_end(R, lane, &ev);
    return layer_lora(c, rank, lane, l, LORA_WO, R.att, (int64_t)H * D, R.part, hd, H * D);
}

// feed-forward block of layer l for one chunk: SkipRMSNorm -> w13 with fused SwiGLU (K3 + K10) -> w2 (partial sums)
// keep_part2: this launch of w2 must write part2 (its consumer runs on the other lane's stream): no deferred slabs
static int layer_ffn_part(pplhip_ctx* c, int rank, Lane& lane, const StepPlan& p, int l, const Chunk& k, bool keep_part2, bool xn_ready = false) {
    Rank& R = c->ranks[rank];
    const pplhip_model_desc& d = c->d;
    hipStream_t s = lane.stream;
    const int hd = d.hidden_dim;
    Layer& L = R.layers[l];
    ProfEvent ev;
    uint16_t* h = R.h + k.t0 * hd;
    uint16_t* xn = R.xn + k.t0 * hd;
    uint16_t* act = R.act + k.t0 * (int64_t)L.w2.Kp;
    const bool a8 = c->act_fmt != ACT_FP16;
    if (!xn_ready)
        HIPCK(c, rank, launch_rmsnorm(s, h, R.part + k.t0 * hd, L.ffn_norm, d.norm_eps, k.tn, hd, nullptr, xn, h, a8 ? R.xq : nullptr,
                                      a8 ? R.sx : nullptr, &lane.sl_part, c->act_fmt == ACT_FP8));
    lane.sl_part = SplitSlabs{};
    prof_begin(c, R, lane, PPLHIP_PROF_GEMM, &ev);
    if (int rc = layer_linear(c, rank, lane, L.w13, xn, k.tn, act, L.w2.Kp, /*swiglu=*/true, a8)) return rc;
    prof_end(R, lane, &ev);
    prof_begin(c, R, lane, PPLHIP_PROF_GEMM, &ev);
    if (int rc = layer_linear(c, rank, lane, L.w2, act, k.tn, R.part2 + k.t0 * hd, hd, false, false,
                              p.defer_reduce && !keep_part2 ? &lane.sl_part2 : nullptr))
        return rc;
    prof_end(R, lane, &ev);
    return layer_lora(c, rank, lane, l, LORA_W2, R.act, L.w2.Kp, R.part2, hd, L.w2.Kp);
}

// all-reduce(sum) of the chunk's rows of `buf` ([T, hidden] fp16) on the lane's channel.  Overlapped mode: on the communication stream,
// after the lane's work so far; the compute stream picks the result up later (comm_pickup, slot ci).
// norm_w != NULL (fuse_norm_active): the collective also folds the reduced rows into the residual stream and normalises them with norm_w --
// afterwards R.xn holds rmsnorm(h + sum) * norm_w for every row of the chunk and R.h the new residual on the rows this rank owns.
int chunk_allreduce(pplhip_ctx* c, int rank, Lane& lane, uint16_t* buf, const Chunk& k, int ci, bool overlapped, const uint16_t* norm_w) {
    Rank& R = c->ranks[rank];
    Channel& ch = *lane.ch;
    const int hd = c->d.hidden_dim;
    uint16_t* p = buf + k.t0 * hd;
    auto reduce_on = [&](hipStream_t st) -> int {
        uint32_t ep = 0;
        if (c->comm_mode == 2)
            if (int rc = p2p_next_epoch(c, rank, ch, st, &ep)) return rc;
        if (norm_w && c->comm_mode == 2) {
            HIPCK(c, rank, launch_p2p_allreduce_norm(st, R.peers, R.global_rank, c->tp, (size_t)((char*)p - R.xbase), ch.x_scratch[ch.ar_count++ & 1], k.tn,
                                                     hd, R.h + k.t0 * hd, norm_w, c->d.norm_eps, R.xn + k.t0 * hd, ep, c->p2p_timeout_ticks,
                                                     R.p2p_status, ch.id));
            return 0;
        }
        if (norm_w) {
            // one rank's slice without its peers (bench.py --emulate-tp): the link part of the collective is skipped as before; what stays is
            // the rank's OWN share of the fused kernel's arithmetic -- residual add + norm of the rows it owns (the other rows of xn keep
            // whatever they held: the emulated step's values are meaningless anyway, its timing is the point)
            const int64_t per = (k.tn + c->tp - 1) / c->tp, lo = std::min<int64_t>(per * R.global_rank, k.tn), nown = std::min<int64_t>(per, k.tn - lo);
            uint16_t* h = R.h + (k.t0 + lo) * hd;
            if (nown > 0) HIPCK(c, rank, launch_rmsnorm(st, h, p + lo * hd, norm_w, c->d.norm_eps, nown, hd, nullptr, R.xn + (k.t0 + lo) * hd, h));
            return 0;
        }
        if (c->comm_mode == 2)
            HIPCK(c, rank, launch_p2p_allreduce(st, R.peers, R.global_rank, c->tp, (size_t)((char*)p - R.xbase), ch.x_scratch[ch.ar_count++ & 1], k.tn * hd,
                                                ep, c->p2p_timeout_ticks, R.p2p_status, ch.id));
        else if (ch.comm)
            NCCLCK(c, rank, ncclAllReduce(p, p, (size_t)k.tn * hd, ncclFloat16, ncclSum, ch.comm, st));
        return 0;
    };
    if (!overlapped || (c->tp_debug & 2)) return reduce_on(lane.stream);
    // (identity: ranks emulated on one device, bench.py --emulate-tp -- nothing to reduce)
    return comm_handoff(c, rank, lane.stream, ci, c->comm_mode != 2 && !ch.comm, (c->tp_debug & 1) != 0, reduce_on);
}

// the launches of one step on the rank's stream(s): executes the plan, decides nothing
static int run_launches(pplhip_ctx* c, int rank, const pplhip_plan_settings& settings) {
    Rank& R = c->ranks[rank];
    const pplhip_model_desc& d = c->d;
    hipStream_t s = R.stream;
    const int64_t T = R.T, B = R.B;
    const int hd = d.hidden_dim;
    // (round 4: 128-thread blocks for many short requests looked 3-6 % faster in the operator micro-benchmark and measured 2 % SLOWER inside
    // the model step, interleaved A/B: 0.885 vs 0.868 ms per launch at batch 1024 / kv 520 -- not adopted)
    const int threads = c->o.decoding_attn_tpb == 512 ? 512 : 256;
    const bool comm = c->tp_on;

    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    if (settings.dual_mode && settings.has_stream2) (void)hipStreamIsCapturing(s, &cst);   // (only a two-lane step depends on it)
    const pplhip_step_shape shape{B, T, R.decoding_batches, R.max_kv_len, R.h_seq, cst != hipStreamCaptureStatusNone, R.dump_dev != nullptr,
                                  R.lora_ntiles > 0};
    const StepPlan p = plan_step(settings, shape);
    const Chunk* ck = p.chunk;
    const int nck = p.num_chunks;
    const bool dual = p.schedule == SCHED_TWO_LANES, fuse = p.fuse_norm != 0;
    const bool ov = p.schedule == SCHED_TWO_CHUNKS;                // collectives alternate with the other chunk's block ...
    const bool on_comm = ov && !(c->tp_debug & 2);                 // ... on the communication stream (diagnosis: chunks, but collectives in stream)
    if (dual && !R.dual_seen && verbose()) {
        R.dual_seen = true;
        fprintf(stderr, "[pplhip] rank %d: two-stream decode (rows %lld + %lld)\n", rank, (long long)ck[0].bn, (long long)ck[1].bn);
    }
    // chunk i goes out on lane i of a two-lane step, else on lane 0
    Lane lane[2] = {make_lane(R, 0, 0), make_lane(R, 1, p.lane1_ws_off)};
    auto lane_of = [&](int i) -> Lane& { return lane[dual ? i : 0]; };

    ProfEvent ev_run, ev;
    prof_begin(c, R, lane[0], PPLHIP_PROF_RUN, &ev_run);
    HIPCK(c, rank, launch_embedding(s, R.d_tok, R.embed, T, hd, R.h));
    const uint16_t* pending = nullptr;
    int rc;
    const size_t dump_n = (size_t)T * hd;  // elements of one dumped matrix
    if (R.dump_dev) HIPCK(c, rank, hipMemcpyAsync(R.dump_dev, R.h, dump_n * 2, hipMemcpyDeviceToDevice, s));
    if (dual) {   // the second stream starts behind the embedding (and with it behind the step's inputs and the previous step)
        HIPCK(c, rank, hipEventRecord(R.ev_fork, s));
        HIPCK(c, rank, hipStreamWaitEvent(R.stream2, R.ev_fork, 0));
    }
    for (int l = 0; l < d.num_layers; ++l) {
        // (the last layer's w2 writes part2 in both halves: the final norm gathers rows of both on the first stream)
        const bool keep_part2 = dual && l == d.num_layers - 1;
        for (int i = 0; i < nck; ++i) {
            if (on_comm && l > 0 && (rc = comm_pickup(c, rank, s, i))) return rc;  // part2 rows of chunk i are reduced
            if ((rc = layer_attention_part(c, rank, lane_of(i), p, l, ck[i], pending, p.decode_split[i], threads, fuse && l > 0))) return rc;
            if (comm && (rc = chunk_allreduce(c, rank, lane_of(i), R.part, ck[i], i, ov, fuse ? R.layers[l].ffn_norm : nullptr))) return rc;
        }
        for (int i = 0; i < nck; ++i) {
            if (on_comm && (rc = comm_pickup(c, rank, s, i))) return rc;            // part rows of chunk i are reduced
            if ((rc = layer_ffn_part(c, rank, lane_of(i), p, l, ck[i], keep_part2, fuse))) return rc;
            // (fused: the collective behind w2 normalises for the NEXT consumer -- the next layer's attention norm, or the final norm)
            if (comm && (rc = chunk_allreduce(c, rank, lane_of(i), R.part2, ck[i], i, ov, !fuse ? nullptr : (l + 1 < d.num_layers ? R.layers[l + 1].attn_norm : R.norm)))) return rc;
        }
        pending = fuse ? nullptr : R.part2;
        if (R.dump_dev) {
            if (on_comm) for (int i = 0; i < nck; ++i) if ((rc = comm_pickup(c, rank, s, i))) return rc;
            HIPCK(c, rank, hipMemcpyAsync(R.dump_dev + (size_t)(l + 1) * 2 * dump_n, R.h, dump_n * 2, hipMemcpyDeviceToDevice, s));
            HIPCK(c, rank, hipMemcpyAsync(R.dump_dev + ((size_t)(l + 1) * 2 + 1) * dump_n, R.part2, dump_n * 2, hipMemcpyDeviceToDevice, s));
        }
    }
    if (on_comm) for (int i = 0; i < nck; ++i) if ((rc = comm_pickup(c, rank, s, i))) return rc;
    if (dual) {   // the first stream goes on behind the second half's last layer
        HIPCK(c, rank, hipEventRecord(R.ev_join, R.stream2));
        HIPCK(c, rank, hipStreamWaitEvent(s, R.ev_join, 0));
    }
    // prompt logprobs of the rows that asked (pplhip_set_prompt_logprobs), in front of K11 and through its buffers; a step nobody asks in
    // issues exactly the launches below.  (An asking step has T != B and no tensor parallelism: one lane, no fused norm, no decode graph.)
    R.plp_done = 0;
    if (R.plp_n > 0) {
        if (fuse || comm || dual) return fail(c, rank, PPLHIP_OTHER_ERROR, "prompt logprobs on a step with collectives or two lanes");
        if ((rc = run_prompt_logprobs(c, rank, s, pending, lane[0].sl_part2))) return rc;
    }
    // K11: last-token gather + final (Skip)RMSNorm (the last FFN output is folded into the residual of the gathered
    // rows only) + lm_head (+ all-gather of the vocab shards)
    const uint16_t* hn = R.hn;
    if (fuse && d.num_layers > 0) {
        // the last collective already applied the final norm to every row: only the last-token gather is left (a pure-decode step's rows
        // ARE the last tokens, in order)
        if (T == B) hn = R.xn;
        else HIPCK(c, rank, launch_gather_last_rows(s, R.xn, R.d_seq, B, hd, R.hn));
    } else {
        HIPCK(c, rank, launch_rmsnorm(s, R.h, pending, R.norm, d.norm_eps, B, hd, R.d_seq, R.hn, nullptr, nullptr, nullptr, pending ? &lane[0].sl_part2 : nullptr));
    }
    prof_begin(c, R, lane[0], PPLHIP_PROF_GEMM, &ev);
    if (!comm) {
        HIPCK(c, rank, launch_linear(s, hn, R.output.w, nullptr, 0, 0, B, R.output.N, hd, R.logits, d.vocab_size, true, R.gemm_ws, R.gemm_ws_bytes));
        prof_end(R, lane[0], &ev);
    } else {
        const int vl = c->vocab_local;
        HIPCK(c, rank, launch_linear(s, hn, R.output.w, nullptr, 0, 0, B, vl, hd, R.logits_local, vl, true, R.gemm_ws, R.gemm_ws_bytes));
        prof_end(R, lane[0], &ev);
        // every collective of this communicator is issued on ONE stream (the communication stream when overlapping)
        Channel& ch = R.ch[0];
        auto gather_on = [&](hipStream_t cs) -> int {
            if (c->comm_mode == 2) {  // every rank pulls every shard straight into its [B, V] logits
                uint32_t ep = 0;
                if (int rc = p2p_next_epoch(c, rank, ch, cs, &ep)) return rc;
                HIPCK(c, rank, launch_p2p_allgather(cs, R.peers, R.global_rank, c->tp, R.x_local, R.logits, B, (int64_t)vl * 4,
                                                    (int64_t)d.vocab_size * 4, ep, c->p2p_timeout_ticks, R.p2p_status));
            } else if (ch.comm) {
                NCCLCK(c, rank, ncclAllGather(R.logits_local, R.logits_gather, (size_t)B * vl, ncclFloat32, ch.comm, cs));
            } else {  // world size 1 without a communicator cannot happen (tp_on implies one of the two)
                return fail(c, rank, PPLHIP_OTHER_ERROR, "tensor-parallel step without collectives");
            }
            return 0;
        };
        if (!on_comm) {
            if ((rc = gather_on(s))) return rc;
        } else {
            if ((rc = comm_handoff(c, rank, s, 0, false, false, gather_on))) return rc;
            if ((rc = comm_pickup(c, rank, s, 0))) return rc;
        }
        for (int r = 0; r < c->tp && c->comm_mode != 2; ++r)
            HIPCK(c, rank, hipMemcpy2DAsync(R.logits + (size_t)r * vl, (size_t)d.vocab_size * 4, R.logits_gather + (size_t)r * B * vl,
                                            (size_t)vl * 4, (size_t)vl * 4, B, hipMemcpyDeviceToDevice, s));
    }
    prof_end(R, lane[0], &ev_run);
    return 0;
}

// HIP-graph replay of pure-decode steps.  Everything a decode step launches depends only on (batch, attention split, page-table
// width): token ids, positions, cache slots and page lists are read from the step buffer, whose layout is fixed by the batch size.
// So the ~290 launches of a step whose shape was seen before can be replayed as one graph launch (the second occurrence of a
// shape captures it).  Measured (profiles/small_batch_latency.py, 7B W8A16, kv 512): batch 1 3.30 ms replayed vs 3.26 ms eager,
// batch 64 6.08 vs 6.07 -- the step is GPU-bound (the kernels already run back to back; what a small batch loses is the ramp-up
// of 290 short kernels, which a graph does not remove), so the replay only saves host time and stays opt-in
// (PPLHIP_DECODE_GRAPH=1).  Round 4, with the step at 2.3 ms: batch 1 / 2 2.33 / 2.53 -> 2.28 / 2.48 ms replayed, nothing from batch 4 up;
// still opt-in (a paged cache changes the page-table width, hence the captured shape, every page_size steps).
// Never under tensor parallelism (collectives on a second stream) or profiling.
static int run_decode_graph(pplhip_ctx* c, int rank, const pplhip_plan_settings& settings, bool* done) {
    Rank& R = c->ranks[rank];
    *done = false;
    const int64_t B = R.B;
    const int64_t nb_decode = std::min<int64_t>(std::max<int64_t>(R.decoding_batches, 0), B);
    if (!c->graph_on || c->tp_on || c->o.enable_profiling || R.T != B || nb_decode != B || B > c->graph_max_batch) return 0;
    if (R.lora_ntiles > 0) return 0;   // the tile list is this step's own: neither captured nor replayed
    const uint64_t key = (uint64_t)B | ((uint64_t)decode_split(settings, B, R.max_kv_len) << 24) | ((uint64_t)R.max_pages << 32);
    auto it = R.graphs.find(key);
    if (it == R.graphs.end()) {  // first sight: run eagerly (one-time function attributes, lazily loaded code objects)
        if (R.graphs.size() >= 32) {  // drop the least recently used shape
            auto old = R.graphs.begin();
            for (auto j = R.graphs.begin(); j != R.graphs.end(); ++j) if (j->second.tick < old->second.tick) old = j;
            if (old->second.exec) hipGraphExecDestroy(old->second.exec);
            R.graphs.erase(old);
        }
        R.graphs[key] = GraphEntry{nullptr, ++R.graph_tick};
        return 0;
    }
    it->second.tick = ++R.graph_tick;
    if (!it->second.exec) {
        hipGraph_t g = nullptr;
        HIPCK(c, rank, hipStreamBeginCapture(R.stream, hipStreamCaptureModeThreadLocal));
        const int rc = run_launches(c, rank, settings);
        const hipError_t e = hipStreamEndCapture(R.stream, &g);
        if (rc) { if (g) hipGraphDestroy(g); return rc; }
        if (e != hipSuccess || !g) { (void)hipGetLastError(); c->graph_on = false; return 0; }  // capture unsupported here: eager from now on
        hipGraphExec_t ex = nullptr;
        const hipError_t e2 = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (e2 != hipSuccess || !ex) { (void)hipGetLastError(); c->graph_on = false; return 0; }
        it->second.exec = ex;
        if (verbose()) fprintf(stderr, "[pplhip] rank %d: decode step captured as a HIP graph (batch %lld, split %d, page-table width %lld)\n",
                                              rank, (long long)B, (int)((key >> 24) & 0xff), (long long)R.max_pages);
    }
    HIPCK(c, rank, hipGraphLaunch(it->second.exec, R.stream));
    *done = true;
    return 0;
}

int pplhip_run(pplhip_ctx* c, int rank, int cache_prefill) {
    (void)cache_prefill;  // K6 and K7 are one kernel here: attention always reads K/V back from the slab
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    if (!R.kv_cache) return fail(c, rank, PPLHIP_INVALID_VALUE, "kv slab not allocated");
    HIPCK(c, rank, hipSetDevice(R.device));
    R.plp_done = 0;   // the results of pplhip_prompt_logprobs belong to one run
    if (R.B == 0) return 0;
    if (R.lora_stale) return fail(c, rank, PPLHIP_INVALID_VALUE, "an adapter slot was unloaded after the step's adapters were set: set the inputs again");
    bool done = false;
    const pplhip_plan_settings settings = plan_settings(c, R);   // once per step
    if (int rc = run_decode_graph(c, rank, settings, &done)) return rc;
    return done ? 0 : run_launches(c, rank, settings);
}

// Diagnosis entry point (tests bisect a logits difference per layer with it): pplhip_run with the residual stream captured after
// every layer, in the oracle's hidden_dump convention (oracle/llama_ref.c ref_forward): out[0] = embeddings, out[l + 1] =
// fp16(h + row-parallel FFN output of layer l) as fp32, [L + 1, T, hidden].  Eager launches, synchronises.
int pplhip_debug_run_dump(pplhip_ctx* c, int rank, float* hidden_dump_host) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size() || !hidden_dump_host) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    if (!R.kv_cache) return fail(c, rank, PPLHIP_INVALID_VALUE, "kv slab not allocated");
    HIPCK(c, rank, hipSetDevice(R.device));
    if (R.B == 0) return 0;
    const int L = c->d.num_layers;
    const size_t n = (size_t)R.T * c->d.hidden_dim;
    HIPCK(c, rank, hipMalloc((void**)&R.dump_dev, (size_t)(L + 1) * 2 * n * 2));
    int rc = run_launches(c, rank, plan_settings(c, R));
    std::vector<uint16_t> host((size_t)(L + 1) * 2 * n);
    hipError_t e = hipStreamSynchronize(R.stream);
    if (e == hipSuccess) e = hipMemcpy(host.data(), R.dump_dev, host.size() * 2, hipMemcpyDeviceToHost);
    hipFree(R.dump_dev);
    R.dump_dev = nullptr;
    if (rc) return rc;
    HIPCK(c, rank, e);
    for (size_t i = 0; i < n; ++i) hidden_dump_host[i] = h2f_host(host[i]);
    for (int l = 1; l <= L; ++l) {
        const uint16_t* a = host.data() + (size_t)l * 2 * n;
        const uint16_t* b = a + n;
        float* o = hidden_dump_host + (size_t)l * n;
        for (size_t i = 0; i < n; ++i) o[i] = h2f_host(f2h_host(h2f_host(a[i]) + h2f_host(b[i])));
    }
    return p2p_check(c, rank);
}

int pplhip_logits(pplhip_ctx* c, int rank, float** logits_device, int64_t* stride) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    if (logits_device) *logits_device = c->ranks[rank].logits;
    if (stride) *stride = c->d.vocab_size;
    return 0;
}

int pplhip_sync(pplhip_ctx* c, int rank) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    HIPCK(c, rank, hipSetDevice(c->ranks[rank].device));
    HIPCK(c, rank, hipStreamSynchronize(c->ranks[rank].stream));
    return p2p_check(c, rank);
}

int pplhip_copy_logits(pplhip_ctx* c, int rank, float* dst, int64_t batch) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size() || !dst) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    HIPCK(c, rank, hipSetDevice(R.device));
    HIPCK(c, rank, hipStreamSynchronize(R.stream));
    if (int rc = p2p_check(c, rank)) return rc;
    HIPCK(c, rank, hipMemcpy(dst, R.logits, (size_t)batch * c->d.vocab_size * 4, hipMemcpyDeviceToHost));
    return 0;
}

/* ------------------------------------------------------------------------------------------------ measurement */

int pplhip_profile_reset(pplhip_ctx* c, int rank) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    HIPCK(c, rank, hipSetDevice(R.device));
    HIPCK(c, rank, hipStreamSynchronize(R.stream));
    for (auto& e : R.prof) R.prof_free.push_back({e.a, e.b});
    R.prof.clear();
    return 0;
}

int pplhip_profile_get(pplhip_ctx* c, int rank, int cls, int64_t* launches, double* total_ms) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    Rank& R = c->ranks[rank];
    HIPCK(c, rank, hipSetDevice(R.device));
    HIPCK(c, rank, hipStreamSynchronize(R.stream));
    int64_t n = 0;
    double ms = 0;
    for (auto& e : R.prof)
        if (e.cls == cls) {
            float t = 0;
            if (hipEventElapsedTime(&t, e.a, e.b) == hipSuccess) { ms += t; ++n; }
        }
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    return 0;
}

int pplhip_profile_mode(pplhip_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 2) return PPLHIP_INVALID_VALUE;
    c->o.enable_profiling = mode;
    return 0;
}

int pplhip_mem_info(pplhip_ctx* c, int rank, uint64_t* free_bytes, uint64_t* total_bytes) {
    if (!c || rank < 0 || rank >= (int)c->ranks.size()) return PPLHIP_INVALID_VALUE;
    HIPCK(c, rank, hipSetDevice(c->ranks[rank].device));
    size_t f = 0, t = 0;
    HIPCK(c, rank, hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return 0;
}
