/*
 * pplhip.h -- C ABI of the MI355X (gfx950) backend for ppl.llm.serving's batched decode hot path.
 *
 * This is the drop-in boundary.  Everything below the dashed line of the
 * reference's layer map (ppl.nn Runtime/Tensor/Engine, ppl.llm.kernel.cuda, NCCL) is replaced by this
 * library; everything above it (src/engine, src/generator, tools) calls it through `src/backends/hip`.
 * Plain C structs of ints / pointers; no C++ or torch types cross this boundary.
 *
 * Conventions
 *   - every entry point returns 0 on success or a negative pplhip_status; the text of the last error of
 *     a rank is available from pplhip_last_error().  The codes map 1:1 onto the ppl::common::RetCode
 *     values the reference uses in-tree (src/backends/cuda/resource_manager.cc, post_processor.cc).
 *   - the caller owns all host buffers; the library owns all device memory.
 *   - `rank` is the LOCAL rank index inside this context.  A rank's entry points are called from that
 *     rank's worker thread only -- exactly how utils::ParallelExecute drives ranks in the reference
 *     (src/utils/utils.h:37-52).  pplhip_sample/pplhip_penalty act on local rank 0's stream and may be
 *     called from the generator thread (src/engine/llm_engine.cc:204-224).
 *   - no global state: several contexts may coexist.
 *   - set_inputs/run are asynchronous (stream-ordered); pplhip_sample is the one synchronisation point
 *     of a step (src/backends/cuda/post_processor.cc:196).
 */
#ifndef PPLHIP_H_
#define PPLHIP_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PPLHIP_API __attribute__((visibility("default")))

/* ---- status codes (ppl::common::RetCode counterparts) ------------------------------------------- */
typedef enum pplhip_status {
    PPLHIP_SUCCESS = 0,
    PPLHIP_OTHER_ERROR = -1,          /* RC_OTHER_ERROR */
    PPLHIP_INVALID_VALUE = -2,        /* RC_INVALID_VALUE */
    PPLHIP_OUT_OF_MEMORY = -3,        /* RC_OUT_OF_MEMORY */
    PPLHIP_DEVICE_RUNTIME_ERROR = -4, /* RC_DEVICE_RUNTIME_ERROR */
    PPLHIP_DEVICE_MEMORY_ERROR = -5,  /* RC_DEVICE_MEMORY_ERROR */
    PPLHIP_NOT_FOUND = -6,            /* RC_NOT_FOUND */
    PPLHIP_UNSUPPORTED = -7           /* RC_UNSUPPORTED */
} pplhip_status;

/* ---- model description: params.json (src/common/config.cc:31-148) + what the exported graph encodes */
typedef struct pplhip_model_desc {
    int32_t hidden_dim;
    int32_t intermediate_dim;
    int32_t num_layers;
    int32_t num_heads;
    int32_t num_kv_heads;
    int32_t vocab_size;
    float norm_eps;          /* RMSNorm epsilon (graph attribute in the reference; 1e-5 for LLaMA-2) */
    float rope_theta;        /* 10000 for LLaMA-2 */
    int32_t max_position;    /* size of the host-built cos/sin table */
    int32_t cache_quant_bit;   /* 0 (fp16 KV), 8 (int8 / fp8 KV) or 4 (int4 KV)   src/generator/llm_generator.cc:131-136 */
    int32_t cache_quant_group; /* 1 with bit 0 (fp16); 8 with bit 8 (int8, one fp16 scale per 8 channels); head_dim (32, 64, 128)
                                  with bit 8: fp8 e4m3fn, one power-of-two fp16 scale per head row (library 1.2; DESIGN.md numerics);
                                  32 with bit 4: int4 (nibble = q + 8, two channels per byte, low nibble first), one fp16 scale of 8
                                  significant bits per 32 channels, head_dim 32, 64 or 128: a head row is head_dim / 2 bytes and
                                  head_dim / 32 scales.  The pair arrived without a version bump (pplhip_version() stays 1.2): a
                                  client tells a library that has it by pplhip_init accepting it (older 1.2 libraries return
                                  PPLHIP_INVALID_VALUE) */
    int32_t cache_layout;      /* 0..3                                  src/engine/llm_engine.cc:122-166 */
    int32_t cache_mode;        /* 0 contiguous ranges, 1 paged          src/generator/llm_generator.cc:486-560 */
    int32_t page_size;         /* tokens per page when cache_mode == 1 */
    int32_t weight_quant_bit;   /* 0 fp16 weights, 8 = W8A16 per-output-channel, 4 = W4A16 grouped */
    int32_t weight_quant_group; /* K-group of W4A16 (128); ignored otherwise */
    int32_t act_quant_bit;      /* 0 = fp16 activations; 8 (with weight_quant_bit 8) = online_i8i8, the W8A8 mode of
                                   src/backends/cuda/resource_manager.cc:51-52: per-token int8 activations in front of
                                   every layer linear, int8 x int8 -> int32 on the matrix cores.  In this mode an fp16
                                   [N,K] matrix handed to pplhip_rank_set_tensor for an int8 linear is quantised per
                                   output row on the device ("online").
                                   PPLHIP_ACT_QUANT_FP8 (with weight_quant_bit 8) = online_f8f8: the same places and
                                   rows, quantised to OCP e4m3fn codes under one power-of-two scale per row (the rule of
                                   the fp8 KV cache), e4m3 x e4m3 -> fp32 on the matrix cores; weights are quantised per
                                   output row on the device from fp16 (DESIGN.md "numerics"). */
} pplhip_model_desc;

/* values of pplhip_model_desc.act_quant_bit besides 0: low byte the code width, bit 8 marks e4m3fn */
#define PPLHIP_ACT_QUANT_I8 8      /* online_i8i8 */
#define PPLHIP_ACT_QUANT_FP8 0x108 /* online_f8f8 */
/* online_f8f8 arrived without a version bump (pplhip_version() stays 1.2): a client tells a library that has it by the symbol
 * pplhip_op_linear_f8 (dlsym) or by pplhip_init accepting act_quant_bit PPLHIP_ACT_QUANT_FP8 (older 1.2 libraries return
 * PPLHIP_INVALID_VALUE for it). */

/* ---- context options: what CudaResourceManager::Init/InitTask take (resource_manager.cc:213-428) */
typedef struct pplhip_opts {
    int32_t n_local_ranks;     /* ranks (GPUs) driven by THIS process: tensor_parallel_size in the
                                  reference's single-process mode, 1 in one-process-per-GPU mode */
    int32_t world_size;        /* total tensor-parallel degree across processes */
    int32_t rank_base;         /* global rank of local rank 0 */
    const int32_t* device_ids; /* n_local_ranks HIP device ordinals; NULL = 0..n-1 */
    const void* nccl_unique_id;/* PPLHIP_UNIQUE_ID_BYTES bytes, shared by all processes; NULL when
                                  world_size == n_local_ranks (single process: ncclCommInitAll) */
    int32_t max_running_batch; /* --max-running-batch */
    int32_t max_tokens_per_step; /* --max-tokens-per-step */
    int32_t enable_penalty;    /* --enable-penalty */
    int32_t decoding_attn_split_k; /* --configure-decoding-attn-split-k: 0 off, 1 heuristic, 2 always */
    int32_t decoding_attn_tpb;     /* --specify-decoding-attn-tpb: 0 heuristic, 256, 512 */
    int32_t enable_profiling;  /* record HIP events around the dominant kernels (see pplhip_profile_*): 1 = every class,
                                  2 = decode attention and the whole run only (an event record is a barrier packet) */
} pplhip_opts;

#define PPLHIP_UNIQUE_ID_BYTES 128

/* ---- one step's inputs: ModelInput (src/engine/llm_engine.h:40-60) as the 11-input contract
 *      of the runtime (src/engine/llm_engine.h:124-138, src/engine/llm_engine.cc:29-111) ------------ */
typedef struct pplhip_step {
    int64_t batch;               /* B = start_pos.size() */
    int64_t num_tokens;          /* T = token_inputs.size() */
    int64_t decoding_batches;    /* first rows with seqlen 1 */
    int64_t max_seq_len;
    int64_t max_kv_len;
    int64_t max_pages;           /* cache_mode 1 only */
    const int64_t* token_inputs; /* [T] */
    const int64_t* seq_starts;   /* [B+1] */
    const int64_t* kv_starts;    /* [B+1] */
    const int64_t* start_pos;    /* [B] */
    const int64_t* cache_indices;/* mode 0: [B] first KV slot of each request;
                                    mode 1: [B, max_pages] page ids (INT64_MAX padded), may be NULL when
                                    req_list_changed == 0 (src/engine/llm_engine.cc:67-71) */
    int32_t req_list_changed;
} pplhip_step;

/* ---- sampler arguments: PostProcessor::SampleTopKTopP (src/common/post_processor.h:31-35) ------- */
typedef struct pplhip_sample_args {
    const float* temperatures;   /* host [B] or NULL */
    const int32_t* top_k;        /* host [B] or NULL (unused by the reference kernel, Q3 in SURVEY.md) */
    const float* top_p;          /* host [B] or NULL */
    int32_t batch;
    int32_t vocab_size;
    int32_t batch_stride;        /* logits row stride in floats */
    int32_t default_top_k;
    float default_top_p;
    int32_t req_list_changed;
    int32_t enable_penalty;
} pplhip_sample_args;

/* ---- penalty arguments: PostProcessor::ApplyPenalty (src/common/post_processor.h:37-42) --------- */
typedef struct pplhip_penalty_args {
    const float* temperatures;          /* host [B] */
    const float* repetition_penalties;  /* host [B] */
    const float* presence_penalties;    /* host [B] or NULL */
    const float* frequency_penalties;   /* host [B] or NULL */
    const int64_t* batch_slots;         /* host [B] */
    int32_t batch;
    int32_t vocab_size;
    int32_t req_list_changed;
} pplhip_penalty_args;

typedef struct pplhip_ctx pplhip_ctx;

/* ================================================================================================
 * life cycle  -- replaces CudaResourceManager::Init / ~CudaResourceManager
 *               (src/backends/cuda/resource_manager.cc:373-428, resource_manager.h:86-109)
 * ============================================================================================== */

/* library/ABI version (major<<16 | minor) */
PPLHIP_API int pplhip_version(void);

/* number of visible HIP devices, or a negative status (replaces the cudaGetDeviceCount probe). */
PPLHIP_API int pplhip_device_count(void);

/* fills PPLHIP_UNIQUE_ID_BYTES bytes with an RCCL unique id (replaces ppl::common::InitNccl,
 * resource_manager.cc:393, for the one-process-per-GPU launch). */
PPLHIP_API int pplhip_get_unique_id(void* out);

/* creates streams, RCCL communicators, cos/sin table and per-rank scratch.  Device work of rank r
 * happens on opts->device_ids[r]. */
PPLHIP_API int pplhip_init(const pplhip_model_desc* desc, const pplhip_opts* opts, pplhip_ctx** out);

PPLHIP_API void pplhip_destroy(pplhip_ctx* ctx);

/* ---- tensor-parallel collectives (replaces the NCCL calls ppl.nn issues on the engine's stream,
 *      src/backends/cuda/resource_manager.cc:239,392-398) ------------------------------------------------
 * Two implementations behind the same step schedule: RCCL, and direct kernels over peer-mapped memory that use all
 * xGMI links of a rank at once (csrc/k_comm.hip).  The direct path is preferred whenever its start-up self-test passes
 * on EVERY rank (env PPLHIP_COMM=auto|p2p|rccl).  When all ranks live in one process (the reference's mode)
 * pplhip_init connects them itself.  With one process per GPU the launcher does, after pplhip_init on every process:
 *     pplhip_comm_export(ctx, 0, mine);  all-gather the handles by global rank;  pplhip_comm_connect(ctx, all);
 * pplhip_comm_connect is collective (every process calls it at about the same time); skipping it keeps RCCL. */
#define PPLHIP_IPC_HANDLE_BYTES 64
PPLHIP_API int pplhip_comm_export(pplhip_ctx* ctx, int rank, void* handle_out /* PPLHIP_IPC_HANDLE_BYTES */);
PPLHIP_API int pplhip_comm_connect(pplhip_ctx* ctx, const void* all_handles /* world_size x PPLHIP_IPC_HANDLE_BYTES */);
/* collectives in use: 0 none (single rank), 1 RCCL, 2 direct kernels over peer-mapped memory */
PPLHIP_API int pplhip_comm_mode(pplhip_ctx* ctx);
/* 1 when the all-reduces behind wo / w2 also do the residual add and the RMSNorm that consumes them, on the rows a rank owns between the two
 * shots of the direct all-reduce (sequence-parallel residual stream: 1 / world_size of the norm work per rank, one launch less per
 * half-layer; the same bytes on the links).  Direct collectives only; RCCL keeps all-reduce + replicated norm.  PPLHIP_TP_FUSE_NORM=0: off */
PPLHIP_API int pplhip_comm_fused_norm(pplhip_ctx* ctx);

/* What a multi-GPU run actually does, for the benchmark's report and for diagnosing a first run on real links (no counterpart in the
 * reference, whose NCCL set-up either works or aborts: src/backends/cuda/resource_manager.cc:392-422).  Fallbacks are never silent: each
 * one is printed on stderr when it is taken and kept in `notes` (direct collectives -> RCCL when the self-test fails on any rank;
 * two-stream decode -> one stream when the second RCCL communicator cannot be created). */
typedef struct pplhip_comm_info_t {
    int32_t mode;           /* pplhip_comm_mode */
    int32_t selftest;       /* direct collectives' start-up self-test: 0 not run, 1 passed on every rank, -1 failed */
    int32_t schedule;       /* of a pure-decode step of `rows` rows: 0 collectives in-stream, 1 two half-batches on two streams, 2 two chunks
                               with the collectives on the communication stream */
    int32_t has_rccl;       /* an RCCL communicator exists */
    int64_t dual_min_rows, dual_max_rows;   /* row window of the two-stream schedule (0, 0: off) */
    char notes[512];
} pplhip_comm_info_t;
PPLHIP_API int pplhip_comm_info(pplhip_ctx* ctx, int64_t rows, pplhip_comm_info_t* out);
/* average microseconds of one all-reduce of fp16 [rows, hidden_dim] (the step's own message) on `rank`'s stream over `iters` calls;
 * path 0: the collectives in use, 1: RCCL.  *us = -1 when that path does not exist.  Collective: every rank calls it alike -- the call
 * enqueues and synchronises, so a context holding several local ranks calls it from one thread per rank at the same time. */
PPLHIP_API int pplhip_comm_allreduce_us(pplhip_ctx* ctx, int rank, int64_t rows, int32_t iters, int32_t path, float* us);

PPLHIP_API const char* pplhip_last_error(pplhip_ctx* ctx, int rank);

/* ================================================================================================
 * weights -- replaces onnx::RuntimeBuilder::LoadModel of model_slice_<rank>/model.onnx
 *            (src/backends/cuda/resource_manager.cc:117-147,280-289)
 * ============================================================================================== */

/* loads `<slice_dir>/weights.pplhip` (format: DESIGN.md "weight container"). */
PPLHIP_API int pplhip_rank_load(pplhip_ctx* ctx, int rank, const char* slice_dir);

/* uploads one named tensor of this rank's slice from host memory (names: DESIGN.md). */
PPLHIP_API int pplhip_rank_set_tensor(pplhip_ctx* ctx, int rank, const char* name, const void* data,
                                      uint64_t bytes);

/* fills every weight of this rank's slice on the device from the counter-based generator that
 * oracle/llama_ref.c restates (synthetic weights for benchmarks and parity tests). */
PPLHIP_API int pplhip_rank_init_synthetic(pplhip_ctx* ctx, int rank, uint64_t seed);

/* ================================================================================================
 * KV cache slab -- replaces the cudaMemGetInfo/cudaMalloc block of InitTask
 *                  (src/backends/cuda/resource_manager.cc:329-362)
 * ============================================================================================== */

/* bytes one token occupies in the KV slab / the scale slab of one rank (resource_manager.cc:381-387). */
PPLHIP_API int pplhip_kv_block_bytes(pplhip_ctx* ctx, uint64_t* cache_bytes, uint64_t* scale_bytes);

/* kv_cache_max_tokens = max_tokens_scale * free_bytes(local rank 0) * kb/(kb+sb) / kb. */
PPLHIP_API int pplhip_kv_capacity(pplhip_ctx* ctx, float max_tokens_scale, uint64_t* tokens);

/* allocates the slab (+ scale slab) for `tokens` tokens on this rank. */
PPLHIP_API int pplhip_kv_alloc(pplhip_ctx* ctx, int rank, uint64_t tokens);

/* device pointers of the slabs (Resource::items[rank].kv_cache_mem / kv_scale_mem). */
PPLHIP_API int pplhip_kv_ptrs(pplhip_ctx* ctx, int rank, void** kv_cache_mem, void** kv_scale_mem);

/* test/debug: copies `bytes` from the slab (which = 0) or the scale slab (which = 1), starting at byte
 * `offset`, to/from host memory.  Synchronous. */
PPLHIP_API int pplhip_kv_read(pplhip_ctx* ctx, int rank, int which, uint64_t offset, void* dst, uint64_t bytes);
PPLHIP_API int pplhip_kv_write(pplhip_ctx* ctx, int rank, int which, uint64_t offset, const void* src,
                               uint64_t bytes);

/* test/benchmark: fills the whole slab with pseudo-random history (int8 bytes / fp16 values from the
 * counter-based generator, scales in [0.01, 0.03)) so that decode steps can be measured at a given context
 * length without running the prefill first. */
PPLHIP_API int pplhip_kv_fill_synthetic(pplhip_ctx* ctx, int rank, uint64_t seed);

/* ================================================================================================
 * multi-LoRA: per-request adapters on attention.wqkv, attention.wo and feed_forward.w2 (no counterpart in the reference; library
 * extension, DESIGN.md "numerics").  An adapter gives a target linear y0 = linear(x) the factors A fp16 [r, K], B fp16 [N, r] and one fp32
 * scale (lora_alpha / r); rows of a request that uses it become y = fp16(fp32(y0) + scale * fp16(x A^T) B^T), fp32 sums.  The update works
 * on the fp16 input and output of the linear, so it is the same over fp16, W8A16 and W4A16 base weights and over every KV format.
 * Arrived without a version bump (pplhip_version() stays 1.2): a client tells a library that has it by the symbol pplhip_lora_commit
 * (dlsym).  Every pplhip_lora_* entry point and pplhip_set_adapters return PPLHIP_UNSUPPORTED when world_size > 1 (tensor parallelism) or
 * act_quant_bit != 0 (online_i8i8 / online_f8f8: the norm writes only the 1-byte operand, there is no fp16 x).  gate / up (w13) targets are
 * refused by name: the fused SwiGLU epilogue never materialises gate and up.
 * Sequence: pplhip_lora_load (or set_tensor x n + commit) once per slot; then per step pplhip_set_inputs, pplhip_set_adapters, pplhip_run.
 * ============================================================================================== */
#define PPLHIP_LORA_MAX_SLOTS 64
#define PPLHIP_LORA_MAX_RANK 128

/* uploads one factor of adapter `slot` (0 .. PPLHIP_LORA_MAX_SLOTS - 1) with rank r (1 .. PPLHIP_LORA_MAX_RANK; zero-padded to a multiple
 * of 16 on the device).  name: layers.{l}.attention.wqkv.lora_a (fp16 [r, hidden]) / .lora_b (fp16 [N, r], rows in the container's wqkv
 * order), and the same under attention.wo and feed_forward.w2 (lora_a [r, intermediate_dim]).  A name under feed_forward.w13 returns
 * PPLHIP_UNSUPPORTED.  A committed slot must be unloaded first (PPLHIP_INVALID_VALUE). */
PPLHIP_API int pplhip_lora_set_tensor(pplhip_ctx* ctx, int rank, int slot, const char* name, const void* data, uint64_t bytes, int32_t r);
/* makes the slot usable: every (layer, target) must have both factors (of one rank) or neither, at least one pair present. */
PPLHIP_API int pplhip_lora_commit(pplhip_ctx* ctx, int rank, int slot, float scale);
/* reads `<dir>/lora.pplhip` -- the weight container's format with the names above and a one-element fp32 tensor lora.scale -- and commits. */
PPLHIP_API int pplhip_lora_load(pplhip_ctx* ctx, int rank, int slot, const char* dir);
/* synchronises the rank's stream, then frees the slot (committed or half loaded).  A staged adapter assignment is dropped with it: the
 * next pplhip_run wants a new pplhip_set_inputs (+ pplhip_set_adapters). */
PPLHIP_API int pplhip_lora_unload(pplhip_ctx* ctx, int rank, int slot);
/* the adapter of every request of the staged step: slots host [batch], -1 = none.  After pplhip_set_inputs (which clears the assignment:
 * callers that never call this get the step they always got) and before pplhip_run.  With every entry -1 the step issues exactly the
 * launches of a step without adapters.  A step with an assigned row runs on one lane, reduces its split-K linears at once and is never
 * captured into or replayed from a decode graph. */
PPLHIP_API int pplhip_set_adapters(pplhip_ctx* ctx, int rank, const int32_t* slots, int64_t batch);

/* ================================================================================================
 * the step -- replaces SetInputTask / RunModelTask (src/engine/llm_engine.cc:29-116)
 * ============================================================================================== */

/* stages the step's small integer arrays into pinned memory and issues ONE async H2D copy. */
PPLHIP_API int pplhip_set_inputs(pplhip_ctx* ctx, int rank, const pplhip_step* step);

/* the decoder forward for the packed ragged batch: Runtime::Run() (llm_engine.cc:115).
 * cache_prefill = ENGINE_CONF_CACHE_PREFILL (llm_engine.cc:114). */
PPLHIP_API int pplhip_run(pplhip_ctx* ctx, int rank, int cache_prefill);

/* Prompt logprobs (DESIGN.md "numerics", prompt logprobs row; no counterpart in the reference): a request of the staged step can have every
 * one of its own prompt tokens scored.  Request b with ask[b] >= 0 and token rows s .. e-1 of the step (s = seq_starts[b], e =
 * seq_starts[b + 1]) yields the e - s - 1 positions r = s .. e-2: position r is row r's distribution scored against token_inputs[r + 1],
 *   logprob = x[t] - max - log(sum exp(x - max)),   rank = #{v : x[v] > x[t]} + #{v < t : x[v] == x[t]}   (rank 0: the greedy token),
 * x the row's RAW fp32 logits over the whole vocabulary.  The request's last row predicts its first generated token and is not a position;
 * a request of one row (a decode row among them) yields none.  ask[b] = n in 1 .. PPLHIP_TOP_LOGPROBS_MAX also gives the first n entries
 * of every position's ranking (x descending, ties to the lower token id; entries behind the vocabulary are token -1, logprob -inf), entry
 * 0 the greedy token; where the target is among them its logprob equals that entry's bit for bit.
 * THE DISTRIBUTION IS THE MODEL'S OWN: no temperature, no penalty, no logit rule touches it.  pplhip_top_logprobs is the opposite: it
 * reports the row the step's sampler sees, after all of them.
 * pplhip_set_prompt_logprobs: ask is host [batch], -1 (off) .. 20.  After pplhip_set_inputs (which clears the ask: callers that never call
 * this get the step they always got) and before pplhip_run, like pplhip_set_adapters.  With no position asked the step issues exactly the
 * launches of a step without it and nothing is allocated; the buffers (device and pinned) are allocated by the first call that asks.
 * pplhip_run then scores the asked rows in front of its own last-token gather, in chunks of at most max_running_batch rows through the
 * buffers the step's own lm_head uses next (final norm of the rows, lm_head, one workgroup per position), and queues ONE download into
 * pinned memory; the step's logits are bit for bit those of the step without the ask.
 * PPLHIP_INVALID_VALUE before any device call: ask NULL, batch other than the staged step's, an entry outside [-1, 20].
 * PPLHIP_UNSUPPORTED when world_size > 1: the lm_head is vocabulary-sharded under tensor parallelism and the reduction over the vocabulary
 * would have to cross the shards; that is a later change.
 * pplhip_prompt_logprobs fills `out` for the rank's LAST pplhip_run: the pointers are library-owned pinned memory, valid after the next
 * synchronisation of the rank's stream (the step's sampler call, pplhip_copy_logits or pplhip_sync) and until the next pplhip_run;
 * positions = 0 when that run had no ask.  Position i is packed row rows[i] (ascending) of the step.
 * Arrived without a version bump (pplhip_version() stays 1.2): a client tells a library that has it by the symbol
 * pplhip_set_prompt_logprobs (dlsym). */
typedef struct pplhip_prompt_logprobs_out {
    int64_t positions;
    const int32_t* rows;         /* [positions] packed row of the step, ascending; scored against token_inputs[rows[i] + 1] */
    const float* logprobs;       /* [positions] */
    const int32_t* ranks;        /* [positions] */
    const int32_t* top_tokens;   /* [positions, PPLHIP_TOP_LOGPROBS_MAX]: the first n slots of a position whose request asked n >= 1, */
    const float* top_logprobs;   /* the rest (and every slot of an n = 0 position) unspecified */
} pplhip_prompt_logprobs_out;
PPLHIP_API int pplhip_set_prompt_logprobs(pplhip_ctx* ctx, int rank, const int32_t* ask, int64_t batch);
PPLHIP_API int pplhip_prompt_logprobs(pplhip_ctx* ctx, int rank, pplhip_prompt_logprobs_out* out);

/* device pointer + row stride (floats) of `logits fp32[B, vocab]` of the last run (llm_engine.cc:207-222). */
PPLHIP_API int pplhip_logits(pplhip_ctx* ctx, int rank, float** logits_device, int64_t* stride);

/* test/debug: synchronises the rank's stream and copies the logits [batch, vocab] to host. */
PPLHIP_API int pplhip_copy_logits(pplhip_ctx* ctx, int rank, float* dst, int64_t batch);

/* blocks until the rank's stream is idle. */
PPLHIP_API int pplhip_sync(pplhip_ctx* ctx, int rank);

/* ================================================================================================
 * sampler -- replaces CudaPostProcessor (src/backends/cuda/post_processor.cc:71-281)
 * ============================================================================================== */

PPLHIP_API int pplhip_sample(pplhip_ctx* ctx, const float* logits_device, const pplhip_sample_args* args,
                             int32_t* output_host, float* logprob_host);

/* The per-request sampler (DESIGN.md "numerics", per-request sampler row): row b is answered with ITS temperature, top_k, top_p and the
 * random number u(seeds[b], draws[b]) (Philox4x32-10, made on the device); top_k[b] == 1 is greedy, <= 0 pure top-p, > 1024 clamped.
 * draws[b] = the number of tokens the request has produced so far.  Every array is staged and uploaded on every call (there is no
 * req_list_changed rule), one synchronisation like pplhip_sample, no rand(): the two entry points may be mixed.  Acts on local rank 0's
 * logits at any tensor-parallel degree.  NULL top_k / top_p / seeds / draws or batch outside [0, max_running_batch]:
 * PPLHIP_INVALID_VALUE before any device call.
 * Arrived without a version bump (pplhip_version() stays 1.2): a client tells a library that has it by the symbol pplhip_sample_rows
 * (dlsym). */
typedef struct pplhip_sample_rows_args {
    const float* temperatures;   /* host [B] or NULL (NULL when the penalty kernel already divided by them) */
    const int32_t* top_k;        /* host [B] */
    const float* top_p;          /* host [B] */
    const uint64_t* seeds;       /* host [B] */
    const uint64_t* draws;       /* host [B] */
    int32_t batch, vocab_size, batch_stride;
} pplhip_sample_rows_args;
PPLHIP_API int pplhip_sample_rows(pplhip_ctx* ctx, const float* logits_device, const pplhip_sample_rows_args* args,
                                  int32_t* output_host, float* logprob_host);

/* pplhip_sample_rows with two more truncations per row (DESIGN.md "numerics", min_p / typical_p row).  min_p[b] keeps the candidates whose
 * probability is at least min_p[b] times the most probable one's: off when <= 0 or NaN, values above 1 count as 1.  typical_p[b] is
 * locally typical sampling over what top_k, top_p and min_p left, renormalised: the tokens are ordered by |-ln q - H| (H the entropy of q,
 * ties by rank), the shortest prefix whose mass reaches typical_p[b] is kept, and the pick walks the kept tokens in rank order; off when
 * <= 0, >= 1 or NaN.  Either pointer may be NULL: off for every row.  A row with top_k == 1 is greedy whatever else it carries; a row with
 * both off is answered by pplhip_sample_rows' rule, bit for bit in token and logprob, and a call in which every row is so issues exactly
 * the copies and launches of pplhip_sample_rows.  The reported logprob stays the full-vocabulary one: truncation does not renormalise it.
 * A per-request parameter never fails the batch.  Validation, staging and the one synchronisation are pplhip_sample_rows'.
 * Arrived without a version bump: a client tells a library that has it by the symbol pplhip_sample_rows2 (dlsym). */
typedef struct pplhip_sample_rows2_args {
    const float* temperatures;   /* the first eight fields: pplhip_sample_rows_args */
    const int32_t* top_k;
    const float* top_p;
    const uint64_t* seeds;
    const uint64_t* draws;
    int32_t batch, vocab_size, batch_stride;
    const float* min_p;          /* host [B] or NULL */
    const float* typical_p;      /* host [B] or NULL */
} pplhip_sample_rows2_args;
PPLHIP_API int pplhip_sample_rows2(pplhip_ctx* ctx, const float* logits_device, const pplhip_sample_rows2_args* args,
                                   int32_t* output_host, float* logprob_host);

/* Top-N logprobs (DESIGN.md "numerics", top-N logprobs row): for every batch row b with n = num_logprobs[b] > 0 the first n tokens of the
 * ranking "x = logit * (1 / temperature) descending, ties by ascending token index" and logprob = x - logsumexp(x) over the whole
 * vocabulary, the number the samplers report for their token.  Entry 0 is the row's greedy token.  Entries j >= vocab_size are token -1,
 * logprob -inf.  The logits are the ones the step's sampler sees: call it after pplhip_penalty when the penalty is on, with temperatures
 * NULL then.
 * The results are compact: the j-th asking row, in ascending batch row, owns tokens_out[j * 20 .. j * 20 + n) and the same of
 * logprobs_out; *rows_out is the number of asking rows.  The two pointers are library-owned pinned memory.
 * ASYNCHRONOUS: one upload, one launch and one download are queued on local rank 0's stream and the call returns.  The contents are valid
 * after the next synchronisation of that stream (pplhip_sample, pplhip_sample_rows or pplhip_sync) and until the next pplhip_top_logprobs;
 * a step that asks calls this in front of its sampler and still has one synchronisation.  Two calls need such a synchronisation between
 * them.  No asking row: no device call at all, *rows_out = 0.  Acts on local rank 0's logits at any tensor-parallel degree.
 * NULL num_logprobs, an entry outside [0, PPLHIP_TOP_LOGPROBS_MAX], batch outside [0, max_running_batch] or batch_stride < vocab_size:
 * PPLHIP_INVALID_VALUE before any device call.
 * Arrived without a version bump: a client tells a library that has it by the symbol pplhip_top_logprobs (dlsym). */
#define PPLHIP_TOP_LOGPROBS_MAX 20
typedef struct pplhip_top_logprobs_args {
    const float* temperatures;   /* host [B] or NULL, the convention of pplhip_sample_rows_args */
    const int32_t* num_logprobs; /* host [B], 0 .. PPLHIP_TOP_LOGPROBS_MAX */
    int32_t batch, vocab_size, batch_stride;
} pplhip_top_logprobs_args;
PPLHIP_API int pplhip_top_logprobs(pplhip_ctx* ctx, const float* logits_device, const pplhip_top_logprobs_args* args,
                                   const int32_t** tokens_out, const float** logprobs_out, int32_t* rows_out);

/* Logit rules (DESIGN.md "numerics", logit rules row): what a request may produce.  A batch slot (the batch_slots of pplhip_penalty_args)
 * holds one rule, fixed while its request lives: up to PPLHIP_LOGIT_BIAS_MAX pairs (token, bias value; -inf bans the token), an optional
 * mask of allowed tokens (token v is bit v & 31 of word v >> 5; bits at or behind vocab_size mean nothing) and up to
 * PPLHIP_LOGIT_STOP_MAX stop tokens that a row can have suppressed.  The edit of a row with flags f, in place, x the logit as written:
 *   y = -inf              if (f & 1) and allowed_bits is given and v's bit is clear
 *     = -inf              else if (f & 2) and v is in stop_tokens
 *     = fp32(x + bias)    else if (f & 1) and v is in bias_tokens
 *     = x, bit for bit    otherwise;  f == 0: the row is not touched.
 * All pointers of pplhip_logit_rule are HOST memory and are read before pplhip_logit_rule_set returns.
 * pplhip_logit_rule_set validates (PPLHIP_INVALID_VALUE with the reason in pplhip_last_error, nothing changed: slot outside
 * [0, max_running_batch), a count above its maximum or negative, a token outside [0, vocab_size), a bias value that is NaN or +inf, a
 * token with two bias entries, and a rule that leaves no token alive: allowed (or all) minus banned minus stop_tokens is empty -- pass the
 * stops only for a request that will have them suppressed), stages the record in pinned memory and queues its copy to the slot on local
 * rank 0's stream, in front of every later pplhip_logit_edit; any number of calls may follow one another without a synchronisation.
 * The table (max_running_batch records) is allocated on the first call, so a context that never sets a rule allocates nothing.
 * A slot's record stays until the next pplhip_logit_rule_set of that slot; it is read only by rows that ask with that slot.
 * pplhip_logit_edit: batch_slots and flags are host [batch]; one upload and one launch over the rows with flags != 0 are queued on local
 * rank 0's stream, with no synchronisation of the device work; all flags 0 is no device call at all.  Call it in front of pplhip_penalty:
 * a bias is in raw-logit units, and the penalty, pplhip_top_logprobs and the samplers then all see the edited row.  A flag above 3, a slot
 * outside the table or without a rule in a row that asks, vocab_size other than the model's, batch outside [0, max_running_batch] or
 * batch_stride < vocab_size: PPLHIP_INVALID_VALUE before any device call.  Acts on local rank 0's logits at any tensor-parallel degree.
 * Arrived without a version bump: a client tells a library that has it by the symbol pplhip_logit_edit (dlsym). */
#define PPLHIP_LOGIT_BIAS_MAX 512
#define PPLHIP_LOGIT_STOP_MAX 64
typedef struct pplhip_logit_rule {
    const int32_t* bias_tokens;   /* [n_bias], unique */
    const float* bias_values;     /* [n_bias], finite or -inf */
    int32_t n_bias;
    const uint32_t* allowed_bits; /* NULL (every token allowed) or ceil(vocab_size / 32) words */
    const int32_t* stop_tokens;   /* [n_stop] */
    int32_t n_stop;
} pplhip_logit_rule;
typedef struct pplhip_logit_edit_args {
    const int64_t* batch_slots;   /* host [B] */
    const uint32_t* flags;        /* host [B]: bit 0 apply mask and bias, bit 1 suppress the stops */
    int32_t batch, vocab_size, batch_stride;
} pplhip_logit_edit_args;
PPLHIP_API int pplhip_logit_rule_set(pplhip_ctx* ctx, int32_t slot, const pplhip_logit_rule* rule);
PPLHIP_API int pplhip_logit_edit(pplhip_ctx* ctx, float* logits_device, const pplhip_logit_edit_args* args);

/* Guided decoding (DESIGN.md "numerics", guided decoding row): the generated bytes of a request stay inside the language of a byte-level
 * DFA.  A guide is trans [n_states, 256] (the next state of (state, byte); 255 is the dead state, which has no row), accept [n_states] and
 * the end tokens, which are allowed exactly in accepting states whatever their bytes; a token without bytes is never allowed.  State 0
 * is the start.  All pointers of these calls but logits_device are HOST memory and are read before the call returns.
 * pplhip_guide_set_vocab, once per context (a second call, n_tok outside [1, vocab_size], offsets that do not start at 0 or decrease:
 * PPLHIP_INVALID_VALUE): token t < n_tok is bytes[offsets[t] .. offsets[t + 1]), ids at or behind n_tok are empty; uploaded to local rank 0.
 * pplhip_guide_load builds the slot's mask, one row of ceil(vocab_size / 32) words per state, with one kernel on local rank 0's stream and
 * SYNCHRONISES: it happens once per distinct pattern, not per step.  PPLHIP_INVALID_VALUE before any device call, reason in
 * pplhip_last_error: no vocabulary set, slot outside [0, PPLHIP_GUIDE_MAX_SLOTS) or loaded, n_states outside [1, PPLHIP_GUIDE_MAX_STATES],
 * n_end outside [0, PPLHIP_LOGIT_STOP_MAX], an end token outside [0, vocab_size), a transition to a state >= n_states other than 255, a
 * state with neither a live byte nor acceptance.  After the build, a state in which no token at all is allowed (a tokenizer without byte
 * fallback may have no piece for a byte the pattern needs) frees the slot and returns PPLHIP_INVALID_VALUE with the state named.  That
 * check is conservative: such a state might be reachable by bytes yet by no sequence of whole tokens, and the guide is refused all the same.
 * pplhip_guide_unload synchronises local rank 0's stream, then frees the slot (not loaded: PPLHIP_INVALID_VALUE).
 * pplhip_guide_edit: guide_slots (-1: the row does not ask) and states are host [batch]; one upload and one launch over the asking rows are
 * queued on local rank 0's stream with no synchronisation; no asking row is no device call and no allocation.  Row b gets -inf at every
 * token that row states[b] of its slot's mask does not allow.  Call it in front of pplhip_logit_edit and pplhip_penalty.  A slot that is
 * not loaded or a state outside the slot's [0, n_states) in an asking row, vocab_size other than the model's, batch outside
 * [0, max_running_batch] or batch_stride < vocab_size: PPLHIP_INVALID_VALUE before any device call.
 * Arrived without a version bump: a client tells a library that has it by the symbol pplhip_guide_load (dlsym). */
#define PPLHIP_GUIDE_MAX_SLOTS 16
#define PPLHIP_GUIDE_MAX_STATES 255
typedef struct pplhip_guide_desc {
    const uint8_t* trans;         /* [n_states, 256] */
    const uint8_t* accept;        /* [n_states] */
    int32_t n_states;
    const int32_t* end_tokens;    /* [n_end] */
    int32_t n_end;
} pplhip_guide_desc;
typedef struct pplhip_guide_edit_args {
    const int32_t* guide_slots;   /* host [B], -1: not asking */
    const int32_t* states;        /* host [B] */
    int32_t batch, vocab_size, batch_stride;
} pplhip_guide_edit_args;
PPLHIP_API int pplhip_guide_set_vocab(pplhip_ctx* ctx, const uint8_t* bytes, const int64_t* offsets, int32_t n_tok);
PPLHIP_API int pplhip_guide_load(pplhip_ctx* ctx, int32_t slot, const pplhip_guide_desc* desc);
PPLHIP_API int pplhip_guide_unload(pplhip_ctx* ctx, int32_t slot);
PPLHIP_API int pplhip_guide_edit(pplhip_ctx* ctx, float* logits_device, const pplhip_guide_edit_args* args);

/* Wide guides (a JSON schema's automaton): pplhip_guide_load16 is pplhip_guide_load with 16-bit transitions.  trans is uint16
 * [n_states, 256], the dead state is 0xFFFF (PPLHIP_GUIDE16_DEAD; it has no row) and n_states is in [1, PPLHIP_GUIDE16_MAX_STATES]: state
 * 255 is an ordinary live state here.  The slots are the same sixteen and a slot holds either kind; pplhip_guide_unload and
 * pplhip_guide_edit serve both, the latter with the slot's own n_states as the bound of a row's state.  Validation, its messages, the
 * check after the build and the return codes are those of pplhip_guide_load (an allocation that fails: PPLHIP_OUT_OF_MEMORY, the slot
 * stays empty).  A slot's mask takes n_states * ceil(vocab_size / 32) * 4 bytes of device memory: 62.6 MiB for 4096 states at a vocabulary
 * of 128,256, 15.6 MiB at 32,000.  The build is one launch over (token block, chunk of pplhip_guide16_state_chunk() states) that reads
 * the table from global memory.
 * Arrived without a version bump: a client tells a library that has it by the symbol pplhip_guide_load16 (dlsym). */
#define PPLHIP_GUIDE16_MAX_STATES 4096
#define PPLHIP_GUIDE16_DEAD 0xFFFF
typedef struct pplhip_guide_desc16 {
    const uint16_t* trans;        /* [n_states, 256] */
    const uint8_t* accept;        /* [n_states] */
    int32_t n_states;
    const int32_t* end_tokens;    /* [n_end] */
    int32_t n_end;
} pplhip_guide_desc16;
PPLHIP_API int pplhip_guide_load16(pplhip_ctx* ctx, int32_t slot, const pplhip_guide_desc16* desc);
PPLHIP_API int32_t pplhip_guide16_state_chunk(void);   /* states per workgroup of the wide build's grid (for the tests' edge cases) */

/* in-place penalty on the logits of the last run, using the step's device-resident token_inputs /
 * seq_starts / start_pos (llm_engine.cc:204-216). */
PPLHIP_API int pplhip_penalty(pplhip_ctx* ctx, float* logits_device, const pplhip_penalty_args* args);

/* ================================================================================================
 * measurement
 * ============================================================================================== */

/* kernel classes that are timed with HIP events when opts.enable_profiling != 0 */
enum { PPLHIP_PROF_ATTN_DECODE = 0, PPLHIP_PROF_ATTN_PREFILL = 1, PPLHIP_PROF_GEMM = 2,
       PPLHIP_PROF_RUN = 3, PPLHIP_PROF_LORA = 4 /* the two adapter kernels of a target linear */, PPLHIP_PROF_COUNT = 5 };

/* clears the event log of this rank. */
PPLHIP_API int pplhip_profile_reset(pplhip_ctx* ctx, int rank);

/* synchronises, then returns number of launches and summed duration (ms) of a kernel class since reset. */
PPLHIP_API int pplhip_profile_get(pplhip_ctx* ctx, int rank, int kernel_class, int64_t* launches, double* total_ms);

/* changes opts.enable_profiling (0, 1, 2) for the steps that follow: bench.py times its steps in mode 2 (decode attention
 * through its own dispatch packet, no barrier packets on the stream) and then brackets every kernel class on a few extra,
 * untimed steps to report the GEMM share. */
PPLHIP_API int pplhip_profile_mode(pplhip_ctx* ctx, int mode);

/* free / total device memory of the rank's device (cudaMemGetInfo in llm_generator.cc:777). */
PPLHIP_API int pplhip_mem_info(pplhip_ctx* ctx, int rank, uint64_t* free_bytes, uint64_t* total_bytes);

/* ================================================================================================
 * TEST AND HARNESS SUPPORT -- not part of the hot path, called by no backend's step (the product boundary is the
 * sections above).  Everything from here to the end of the header exists for the parity tests, the diagnosis tools and the
 * benchmark harnesses: the two entry points below and the single-operator entry points that follow.
 * ============================================================================================== */

/* a synthetic model whose greedy answers have a wide top-2 margin (token t is followed by t + shift): the embedding table regenerated
 * from `seed` at amplitude embed_amp (0: kept) and output.weight[v] := tok_embeddings.weight[(v - shift) mod vocab] on this rank's shard.
 * For harness checks that compare the answers of two runs token for token (tools/benchmark_prefix_cache_offline
 * --synthetic-decisive-head; the reference compares nothing: benchmark_prefix_cache_offline.cc:442-508). */
PPLHIP_API int pplhip_rank_tie_output(pplhip_ctx* ctx, int rank, int64_t shift, uint64_t seed, float embed_amp);

/* Diagnosis (tests bisect a logits difference per layer with it): pplhip_run with the residual stream captured after every
 * layer in the oracle's convention: out[0] = embeddings, out[l+1] = fp16(h + FFN output of layer l), fp32 [L+1, T, hidden].
 * Launches eagerly and synchronises the rank's stream.  Not used by any backend. */
PPLHIP_API int pplhip_debug_run_dump(pplhip_ctx* ctx, int rank, float* hidden_dump_host);

/* ================================================================================================
 * single-operator entry points (device pointers, caller-provided stream; used by the parity tests to
 * check each hand-written kernel against the oracle in isolation).  `stream` is a hipStream_t or NULL.
 * All fp16 buffers are IEEE binary16.  Semantics: DESIGN.md "numerics".
 * ============================================================================================== */

PPLHIP_API int pplhip_op_embedding(void* stream, const int64_t* token_ids, const void* table, int64_t T,
                                   int32_t hidden, void* out);

/* out = rmsnorm(x (+ skip)) * w ; if skip != NULL also writes residual_out = fp16(x + skip). */
PPLHIP_API int pplhip_op_rmsnorm(void* stream, const void* x, const void* skip, const void* w, float eps,
                                 int64_t T, int32_t hidden, void* out, void* residual_out);

/* y[M,N] = x[M,K] . W[N,K]^T ; wq_bit 0: W fp16; 8: W int8 + scale fp16[N]; 4: W int4 packed + scale
 * fp16[N, K/group].  out_fp32 != 0 writes float, else fp16. */
PPLHIP_API int pplhip_op_linear(void* stream, const void* x, const void* w, const void* scale, int32_t wq_bit,
                                int32_t group, int64_t M, int32_t N, int32_t K, void* y, int32_t out_fp32);

/* fused K3 + K10: W rows interleaved (gate_0, up_0, gate_1, up_1, ...), N = 2 * inter; y[M, N/2] = silu(gate) * up. */
PPLHIP_API int pplhip_op_linear_swiglu(void* stream, const void* x, const void* w, const void* scale, int32_t wq_bit,
                                       int32_t group, int64_t M, int32_t N, int32_t K, void* y);

/* pplhip_op_linear with the caller's row stride ldy (elements), split-K workspace ws / ws_bytes (device memory, may be NULL) and
 * epilogue epi (0 fp16, 1 fp32, 2 fused SwiGLU: y[M, N/2]).  route (route_len bytes, may be NULL) receives the path taken as
 * space-separated key=value tokens, the first naming the kernel template and its arguments, e.g.
 * "kernel=gemm_dma_kernel<8,f16,4,6> splits=1 kchunk=4096 reduce=none order=super(8x12)"; a launch split along M gives two groups
 * separated by " ; ".  dry_run != 0 decides the route and the status exactly as a launch would and makes no HIP call at all (no
 * device needed).  For the tests: not part of the product boundary. */
PPLHIP_API int pplhip_op_linear_ex(void* stream, const void* x, const void* w, const void* scale, int32_t wq_bit, int32_t group,
                                   int64_t M, int32_t N, int32_t K, void* y, int64_t ldy, int32_t epi, void* ws, uint64_t ws_bytes,
                                   int32_t dry_run, char* route, int32_t route_len);

/* pplhip_op_linear_i8 (act_fmt PPLHIP_ACT_QUANT_I8) / pplhip_op_linear_f8 (act_fmt PPLHIP_ACT_QUANT_FP8) with the caller's row stride
 * ldy (elements) and epilogue epi (0 fp16, 1 fp32, 2 fused SwiGLU: y[M, N/2]), and the route record and dry run of
 * pplhip_op_linear_ex: route receives e.g.
 * "kernel=gemm_i8_pc_kernel<f16,4,f8> grid=8x1 threads=512 lds=131072 n_tiles=1 m_tiles=1" -- the kernel template with all its
 * arguments, the grid, the block size, the dynamic LDS bytes and the tile counts.  dry_run != 0: the route and the status exactly
 * as a launch would give them, no HIP call at all (no device needed).  For the tests: not part of the product boundary. */
PPLHIP_API int pplhip_op_linear_q8_ex(void* stream, const void* xq, const float* sx, const void* w, const void* scale, int32_t act_fmt,
                                      int64_t M, int32_t N, int32_t K, void* y, int64_t ldy, int32_t epi, int32_t dry_run, char* route,
                                      int32_t route_len);

/* The step schedule as a pure function (pplhip.cc plan_step: no HIP call, no environment read, no context, no device): what
 * pplhip_run executes for a step of this shape under these settings, and what pplhip_comm_info reports.  For the tests: not part of
 * the product boundary.  A chunk is requests [b0, b0 + bn) = token rows [t0, t0 + tn), its first nd requests decode rows. */
typedef struct pplhip_chunk {
    int64_t b0, bn, t0, tn, nd;
} pplhip_chunk;
typedef struct pplhip_plan_settings {   /* what pplhip_init derived from the descriptor, the options and the switches */
    int32_t tp, tp_on;                  /* world size; collectives after wo / w2 and the logits gather are issued */
    int32_t comm_mode;                  /* pplhip_comm_mode */
    int32_t has_comm, has_comm2;        /* an RCCL communicator exists for channel 0 / channel 1 */
    int32_t emulate_tp;                 /* PPLHIP_EMULATE_TP */
    int32_t tp_overlap;                 /* PPLHIP_TP_OVERLAP */
    int32_t dual_mode, dual_auto;       /* PPLHIP_DUAL_STREAM: on at all; by the automatic rule */
    int32_t has_stream2;                /* the rank owns a second compute stream */
    int64_t tp_overlap_min_tokens;      /* PPLHIP_TP_OVERLAP_MIN_TOKENS */
    int64_t dual_min_rows, dual_max_rows;
    int32_t fuse_norm_want, defer_on;   /* PPLHIP_TP_FUSE_NORM, PPLHIP_DEFER_REDUCE */
    int32_t act_fmt;                    /* 0 fp16, 1 int8, 2 fp8 activations */
    int32_t hidden_dim;
    int32_t heads, kv_heads, head_dim;  /* per rank */
    int32_t cache_quant_bit, cache_quant_group;
    int32_t decoding_attn_split_k;      /* pplhip_opts */
} pplhip_plan_settings;
typedef struct pplhip_step_shape {
    int64_t batch, num_tokens, decoding_batches, max_kv_len;   /* pplhip_step */
    const int64_t* seq_starts;          /* host [batch + 1], or NULL: the rank holds no host copy (never read for a pure-decode step) */
    int32_t capturing, dump;            /* the stream is capturing a graph; a residual dump is on */
    int32_t lora;                       /* some row of the step carries an adapter (pplhip_set_adapters): every linear's output must exist
                                           in memory, so no slabs stay unreduced and the step runs on one lane.  0: the plan of every step so far */
} pplhip_step_shape;
typedef struct pplhip_step_plan {
    int32_t schedule;                   /* as pplhip_comm_info_t.schedule: 0 one lane, 1 two lanes, 2 two chunks on the communication stream */
    int32_t num_chunks;
    pplhip_chunk chunk[2];
    int32_t decode_split[2];            /* split-K of each chunk's decode attention */
    int32_t fuse_norm, defer_reduce, defer_qkv;
    int64_t lane1_ws_off;               /* floats: where lane 1's attention workspace starts */
} pplhip_step_plan;
PPLHIP_API int pplhip_op_step_plan(const pplhip_plan_settings* settings, const pplhip_step_shape* shape, pplhip_step_plan* out);

/* online_i8i8 (W8A8, src/backends/cuda/resource_manager.cc:51-52).  Per-token activation quantisation: q[M,K] int8,
 * sx[M] = max|x| / 127; per-output-row weight quantisation of an fp16 [N,K] matrix: q[N,K] int8, scale[N] fp16;
 * y[m,n] = (sum_k xq * w as int32) * sx[m] * scale[n], rounded to fp16 (or kept fp32); swiglu as in pplhip_op_linear_swiglu. */
/* (Skip)RMSNorm whose output goes straight to the int8 operand of the next linear (what the runtime launches in front of wqkv / w13
 * in online_i8i8 mode): q[T,hidden] / sx[T] = pplhip_op_quant_act(pplhip_op_rmsnorm(...)), bit for bit */
PPLHIP_API int pplhip_op_rmsnorm_quant(void* stream, const void* x, const void* skip, const void* w, float eps, int64_t T,
                                       int32_t hidden, void* residual_out, void* q, float* sx);
PPLHIP_API int pplhip_op_quant_act(void* stream, const void* x, int64_t M, int32_t K, void* q, float* sx);
PPLHIP_API int pplhip_op_quant_weight(void* stream, const void* w, int32_t N, int32_t K, void* q, void* scale);
PPLHIP_API int pplhip_op_linear_i8(void* stream, const void* xq, const float* sx, const void* w, const void* scale, int64_t M,
                                   int32_t N, int32_t K, void* y, int32_t out_fp32, int32_t swiglu);

/* online_f8f8 (fp8 e4m3fn W8A8).  Every row -- a token's activations, a weight matrix's output row -- is quantised by the fp8 KV
 * row rule: e = the smallest integer with 448 * 2^e >= max|x|, clamped to [-15, 8] (0 for an all-zero row: -15),
 * q = e4m3fn_rne(x * 2^-e) saturated to +-448 (+-240 at e = 8).  Activations: q[M,K] codes, sx[M] = 2^e (fp32); weights:
 * q[N,K] codes, scale[N] = fp16(2^e); y[m,n] = (sum_k xq * w in fp32) * sx[m] * scale[n], rounded to fp16 (or kept fp32);
 * K % 16 == 0; swiglu as in pplhip_op_linear_swiglu.  pplhip_op_rmsnorm_quant_f8 = pplhip_op_quant_act_f8(pplhip_op_rmsnorm(...)),
 * bit for bit. */
PPLHIP_API int pplhip_op_rmsnorm_quant_f8(void* stream, const void* x, const void* skip, const void* w, float eps, int64_t T,
                                          int32_t hidden, void* residual_out, void* q, float* sx);
PPLHIP_API int pplhip_op_quant_act_f8(void* stream, const void* x, int64_t M, int32_t K, void* q, float* sx);
PPLHIP_API int pplhip_op_quant_weight_f8(void* stream, const void* w, int32_t N, int32_t K, void* q, void* scale);
PPLHIP_API int pplhip_op_linear_f8(void* stream, const void* xq, const float* sx, const void* w, const void* scale, int64_t M,
                                   int32_t N, int32_t K, void* y, int32_t out_fp32, int32_t swiglu);

/* the two multi-LoRA kernels alone (csrc/k_lora.hip) on the caller's stream: rows m of y [T, ldy] with slot s = row_slots[m] >= 0 become
 * fp16(fp32(y[m, n]) + scales[s] * sum_j fp32(t[m, j]) B_s[n, j]), t[m, j] = fp16(sum_k x[m, k] A_s[j, k]); rows with -1 are neither read
 * nor written.  x [T, ldx], y: device fp16; row_slots: HOST [T]; A, B: HOST arrays [n_slots] of device pointers (NULL: slot not loaded),
 * A_s fp16 [rp, K], B_s fp16 [N, rp] with rp = ranks[s] rounded up to a multiple of 16 and the rows / columns past ranks[s] zero (what
 * pplhip_lora_set_tensor makes of a factor); ranks, scales: HOST [n_slots].  ws: device scratch for the tile list, the slot table and t,
 * 8192 + (T / 16 + n_slots + 1) * 4352 bytes always suffice.  K % 32 == 0, N % 16 == 0, ldx % 8 == 0, n_slots <= PPLHIP_LORA_MAX_SLOTS,
 * ranks 1 .. PPLHIP_LORA_MAX_RANK, every named slot loaded: else PPLHIP_INVALID_VALUE before any HIP call.  For the tests. */
PPLHIP_API int pplhip_op_lora(void* stream, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t T, int32_t N, int32_t K,
                              const int32_t* row_slots, int32_t n_slots, const void* const* A, const void* const* B, const int32_t* ranks,
                              const float* scales, void* ws, uint64_t ws_bytes);

PPLHIP_API int pplhip_op_silu_mul(void* stream, const void* gate_up, int64_t T, int32_t inter, void* out);

/* the penalty kernel alone (launch_penalty), for the tests: every pointer is a device pointer; temperatures, rep, presence and
 * frequency may be NULL.  count_map is the caller's: uint16 [slots, vocab], row batch_slots[b] belongs to batch row b.  Rows of
 * `logits` are `stride` floats apart (stride >= vocab; columns [vocab, stride) are never touched).  Row b's counts are cleared when
 * start_pos[b] == 0 or b >= decoding_batches; token ids must lie in [0, vocab) (pplhip_set_inputs validates them on the product path,
 * nothing does here).  batch == 0 does nothing; an odd vocab is PPLHIP_INVALID_VALUE. */
PPLHIP_API int pplhip_op_penalty(void* stream, float* logits, const float* temperatures, const float* rep, const float* presence,
                                 const float* frequency, const int64_t* batch_slots, const int64_t* token_inputs,
                                 const int64_t* seq_starts, const int64_t* start_pos, int32_t batch, int32_t vocab, int32_t stride,
                                 int32_t decoding_batches, uint16_t* count_map);

/* the sampling kernels alone, for the tests: top_k == 1 launches the greedy kernel (top_p, rnd, default_top_p unused), any other top_k
 * the top-k / top-p kernel with the caller's random numbers rnd[batch] in [0, 1) (pplhip_sample draws them from rand()).  Device
 * pointers; temperatures and top_p may be NULL; out_tok / out_logprob are device buffers of `batch` elements. */
PPLHIP_API int pplhip_op_sample(void* stream, const float* logits, const float* temperatures, const float* top_p, const float* rnd,
                                int32_t batch, int32_t vocab, int32_t stride, int32_t top_k, float default_top_p, int32_t* out_tok,
                                float* out_logprob);

/* the per-request sampling kernels alone (csrc/k_sample_rows.hip), for the tests: every pointer is a DEVICE pointer, arrays of `batch`
 * elements indexed by the batch row.  temperatures may be NULL.  rnd != NULL replaces the generator with the caller's numbers in [0, 1)
 * (seeds / draws may then be NULL).  The greedy / sampling row list is made on the host from a read-back of top_k, so the call
 * synchronises `stream` before it launches: one launch for the rows with top_k == 1, one for the others, none for an empty kind. */
PPLHIP_API int pplhip_op_sample_rows(void* stream, const float* logits, const float* temperatures, const int32_t* top_k, const float* top_p,
                                     const uint64_t* seeds, const uint64_t* draws, const float* rnd, int32_t batch, int32_t vocab,
                                     int32_t stride, int32_t* out_tok, float* out_logprob);
/* pplhip_op_sample_rows plus the two truncation arrays of pplhip_sample_rows2_args as DEVICE pointers [batch] (either may be NULL: off for
 * every row), read back with top_k for the row list: a third launch for the rows with top_k != 1 and min_p or typical_p on, none when
 * there is no such row -- the call then issues exactly the launches of pplhip_op_sample_rows. */
PPLHIP_API int pplhip_op_sample_rows2(void* stream, const float* logits, const float* temperatures, const int32_t* top_k, const float* top_p,
                                      const float* min_p, const float* typical_p, const uint64_t* seeds, const uint64_t* draws,
                                      const float* rnd, int32_t batch, int32_t vocab, int32_t stride, int32_t* out_tok,
                                      float* out_logprob);
/* the top-N logprobs kernel alone (csrc/k_logprobs.hip), for the tests: DEVICE pointers.  temperatures may be NULL; num_logprobs [batch] in
 * 0 .. PPLHIP_TOP_LOGPROBS_MAX (anything else: PPLHIP_INVALID_VALUE, nothing launched).  out_tok / out_logprob are [asked, 20], `asked` the
 * number of rows with num_logprobs > 0, in ascending batch row; row j's slots behind its n are not written.  The row list is made on the
 * host from a read-back of num_logprobs, so the call synchronises `stream` before it launches; no asking row: no launch. */
PPLHIP_API int pplhip_op_top_logprobs(void* stream, const float* logits, const float* temperatures, const int32_t* num_logprobs,
                                      int32_t batch, int32_t vocab, int32_t stride, int32_t* out_tok, float* out_logprob);
/* the logit rules kernel alone (csrc/k_logit_rules.hip), for the tests: caller-owned DEVICE memory only.  flags / slots are [batch], indexed
 * by the batch row; the table is five arrays indexed by slot: head [slots, 4] = {n_bias, n_stop, has_mask, 0}, bias_tokens / bias_values
 * [slots, PPLHIP_LOGIT_BIAS_MAX], stop_tokens [slots, PPLHIP_LOGIT_STOP_MAX], mask [slots, ceil(vocab / 32)].  Nothing is validated
 * but the shape (batch < 0, vocab <= 0, stride < vocab, a NULL array: PPLHIP_INVALID_VALUE, nothing launched): the kernel skips a token
 * outside [0, vocab) and clamps the counts.  rows NULL: the list of the rows with flags != 0 is made on the host from a read-back of
 * flags, so the call synchronises `stream` before it launches.  rows != NULL: a device list of n_rows asking rows, launched as it is
 * with no host round trip (the product's path; the timing script's).  No asking row: no launch. */
PPLHIP_API int pplhip_op_logit_edit(void* stream, float* logits, int32_t stride, int32_t vocab, int32_t batch, const uint32_t* flags,
                                    const int32_t* slots, const int32_t* head, const int32_t* bias_tokens, const float* bias_values,
                                    const int32_t* stop_tokens, const uint32_t* mask, const int32_t* rows, int32_t n_rows);
/* the prompt logprobs kernel alone (csrc/k_prompt_logprobs.hip), for the tests: DEVICE pointers.  Position j < n_rows reads logits row j
 * ([n_rows, stride] raw fp32, stride >= vocab) and is scored against targets[rows[j] + 1] (targets: int64 [n_targets], the layout of a
 * step's token_inputs; rows: int32 [n_rows]); n_top [n_rows] in 0 .. PPLHIP_TOP_LOGPROBS_MAX.  out_logprob / out_rank [n_rows]; out_top_tok
 * / out_top_logprob [n_rows, 20], row j's first n_top[j] slots written, may be NULL when every n_top is 0.  rows and n_top are read back and
 * checked on the host (an n_top outside its range or a rows[j] + 1 outside [0, n_targets): PPLHIP_INVALID_VALUE, nothing launched), so the
 * call synchronises `stream` before it launches; a target outside [0, vocab) gives NaN / rank -1.  n_rows = 0: no launch. */
PPLHIP_API int pplhip_op_prompt_logprobs(void* stream, const float* logits, int32_t stride, int32_t vocab, const int32_t* rows, int32_t n_rows,
                                         const int64_t* targets, int64_t n_targets, const int32_t* n_top, float* out_logprob,
                                         int32_t* out_rank, int32_t* out_top_tok, float* out_top_logprob);
/* the two guided-decoding kernels alone (csrc/k_guide.hip), for the tests and the timing script: caller-owned DEVICE memory only.
 * pplhip_op_guide_build: trans [n_states, 256], accept [n_states], the vocabulary as tok_bytes / tok_off [n_tok + 1], end_tokens [n_end];
 * writes words 0 .. ceil(vocab / 32) - 1 of mask [n_states, mask_stride] and ORs 1 into any [n_states] (the caller zeroes it) for every
 * state that allows a token.  Only the shape is validated (n_states outside [1, 255], vocab <= 0, n_tok outside [0, vocab], n_end outside
 * [0, 64], mask_stride < ceil(vocab / 32), a NULL array: PPLHIP_INVALID_VALUE, nothing launched).
 * pplhip_op_guide_mask: guide_slots / states are [batch]; masks is [n_slots, n_states, mask_stride], n_slots <= 16.  rows NULL: the list of
 * the rows with guide_slots[b] >= 0 is made on the host from a read-back, so the call synchronises `stream` before it launches; rows !=
 * NULL: a device list of n_rows asking rows, launched as it is.  No asking row: no launch. */
PPLHIP_API int pplhip_op_guide_build(void* stream, const uint8_t* trans, const uint8_t* accept, int32_t n_states, const uint8_t* tok_bytes,
                                     const int64_t* tok_off, int32_t n_tok, const int32_t* end_tokens, int32_t n_end, int32_t vocab,
                                     uint32_t* mask, int64_t mask_stride, uint32_t* any);
PPLHIP_API int pplhip_op_guide_mask(void* stream, float* logits, int32_t stride, int32_t vocab, int32_t batch, const int32_t* guide_slots,
                                    const int32_t* states, const uint32_t* masks, int32_t n_slots, int32_t n_states, int64_t mask_stride,
                                    const int32_t* rows, int32_t n_rows);
/* the same two for wide guides: trans is uint16 [n_states, 256] with the dead state 0xFFFF, and n_states of both is in [1, 4096].
 * pplhip_op_guide_mask16 is pplhip_op_guide_mask's kernel and validation with that bound. */
PPLHIP_API int pplhip_op_guide_build16(void* stream, const uint16_t* trans, const uint8_t* accept, int32_t n_states, const uint8_t* tok_bytes,
                                       const int64_t* tok_off, int32_t n_tok, const int32_t* end_tokens, int32_t n_end, int32_t vocab,
                                       uint32_t* mask, int64_t mask_stride, uint32_t* any);
PPLHIP_API int pplhip_op_guide_mask16(void* stream, float* logits, int32_t stride, int32_t vocab, int32_t batch, const int32_t* guide_slots,
                                      const int32_t* states, const uint32_t* masks, int32_t n_slots, int32_t n_states, int64_t mask_stride,
                                      const int32_t* rows, int32_t n_rows);
/* out_u[b] = u(seeds[b], draws[b]), the generator alone (device pointers) */
PPLHIP_API int pplhip_op_sample_uniform(void* stream, const uint64_t* seeds, const uint64_t* draws, int32_t batch, float* out_u);

/* description of a KV slab for the attention / cache-write operators */
typedef struct pplhip_kv_view {
    void* cache;          /* fp16 or int8 */
    void* scale;          /* fp16, NULL when quant_bit == 0 (quant_bit / quant_group: the pairs of pplhip_model_desc, (4, 32) included) */
    int64_t max_tokens;   /* N */
    int32_t num_layers;   /* L */
    int32_t kv_heads;     /* h (per rank) */
    int32_t head_dim;     /* d */
    int32_t quant_bit, quant_group, layout, mode, page_size;
    int32_t layer;        /* layer this call addresses */
} pplhip_kv_view;

/* RoPE on q,k of the fused qkv[T, (H+2Hkv)*D] (in place on q) + write of k,v into the cache. */
PPLHIP_API int pplhip_op_rope_kv_write(void* stream, void* qkv, const float* cos_sin, const pplhip_kv_view* kv,
                                       const int64_t* seq_starts, const int64_t* start_pos,
                                       const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t T,
                                       int32_t num_heads);

/* ---- the row kernels between the GEMMs with everything their launchers take.  For the tests: not part of the product boundary. ----
 * A split-K linear may leave its result as unreduced fp32 slabs for the kernel that consumes it:
 * y[m][n] = fp16((sum_{z < splits}, z = 0, 1, ... slab_ws[(z * slab_M + m) * N + n]) * slab_scale[n]) (slab_scale fp16 [N], NULL: 1).
 * A slab description is (slab_ws, slab_splits, slab_scale, slab_M); slab_splits == 0: none; 1 .. 8; anything else, a NULL or misaligned
 * (16 bytes) slab_ws / slab_scale or N % 8 != 0 is PPLHIP_INVALID_VALUE before any HIP call. */

/* The kernel form a (Skip)RMSNorm launch of (rows, hidden) takes, as text in buf (len bytes): "rmsnorm_kernel<MAXC,NT>", with ",i8" /
 * ",f8" appended for the quantising epilogues (quant 0 none, 1 int8, 2 fp8; int8 is the runtime branch of the same instantiation as
 * none).  wide_max_rows: the largest row count that takes the 512 / 1024-thread forms (the product: PPLHIP_RMSNORM_WIDE_MAX_ROWS,
 * default 512).  Returns the status a launch would (hidden % 8 != 0 or more than 2048 chunks of 8: PPLHIP_INVALID_VALUE; rows == 0:
 * success, empty text).  The launcher calls the same function; no HIP call, no device needed. */
PPLHIP_API int pplhip_op_rmsnorm_form(int64_t rows, int32_t hidden, int32_t quant, int32_t wide_max_rows, char* buf, int32_t len);

/* launch_rmsnorm whole: out[r] = rmsnorm(x[src(r)] + skip[src(r)]) * w with src(r) = gather_seq_starts[r + 1] - 1 (device int64, NULL:
 * src(r) = r); skip from `skip` or, when slab_splits > 0, from the slab description (slab row = src(r), N = hidden); residual_out[r]
 * (may be NULL) = fp16(x + skip).  q != NULL: instead of out, the int8 (q_fp8 != 0: e4m3fn) rows q [rows, hidden] and sx [rows]. */
PPLHIP_API int pplhip_op_rmsnorm_ex(void* stream, const void* x, const void* skip, const void* w, float eps, int64_t rows, int32_t hidden,
                                    const int64_t* gather_seq_starts, void* out, void* residual_out, void* q, float* sx, int32_t q_fp8,
                                    const float* slab_ws, int32_t slab_splits, const void* slab_scale, int64_t slab_M);

/* out[r] = x[seq_starts[r + 1] - 1], r < B: the last-token gather alone (hidden % 8 == 0) */
PPLHIP_API int pplhip_op_gather_last_rows(void* stream, const void* x, const int64_t* seq_starts, int64_t B, int32_t hidden, void* out);

/* pplhip_op_rope_kv_write on token rows [t0, t0 + T) of the step's B requests; slab_splits > 0: the rows come from the slab description
 * of a [T, (H + 2 Hkv) D] launch (slab row = token row - t0, slab_M == T) instead of qkv, which then only receives the rotated q. */
PPLHIP_API int pplhip_op_rope_kv_write_ex(void* stream, void* qkv, const float* cos_sin, const pplhip_kv_view* kv, const int64_t* seq_starts,
                                          const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t t0,
                                          int64_t T, int32_t num_heads, const float* slab_ws, int32_t slab_splits, const void* slab_scale,
                                          int64_t slab_M);

/* pplhip_op_linear_ex (fp16 epilogue) called the way the runtime calls wqkv / wo / w2: a split-K route may leave its slabs unreduced in
 * ws.  *splits receives the slab count (0: y was written as usual), *slab_scale the scale pointer of the slab description (slab_M = M);
 * the route text then holds "reduce=deferred".  dry_run: route and status only, no HIP call; *splits stays 0 (read splits= in the route). */
PPLHIP_API int pplhip_op_linear_defer(void* stream, const void* x, const void* w, const void* scale, int32_t wq_bit, int32_t group,
                                      int64_t M, int32_t N, int32_t K, void* y, int64_t ldy, void* ws, uint64_t ws_bytes, int32_t dry_run,
                                      int32_t* splits, const void** slab_scale, char* route, int32_t route_len);

/* attention over the cache for rows [row_begin, row_end) of the batch: decode rows (seqlen 1) go to
 * the decode kernel, others to the prefill kernel.  out[T, H*D] fp16. */
PPLHIP_API int pplhip_op_attention(void* stream, const void* qkv, const pplhip_kv_view* kv,
                                   const int64_t* seq_starts, const int64_t* start_pos,
                                   const int64_t* cache_indices, int64_t max_pages, int64_t B, int64_t T,
                                   int64_t decoding_batches, int64_t max_seq_len, int64_t max_kv_len,
                                   int32_t num_heads, int32_t split_k, void* workspace, uint64_t workspace_bytes,
                                   void* out);

/* The direct collectives (csrc/k_comm.hip) as operators, for a context whose ranks all live in this process and run the direct mode
 * (pplhip_comm_mode == 2).  One call runs a SEQUENCE of collectives: every item is enqueued on every local rank from the calling thread,
 * back to back on the ranks' streams with no host synchronisation in between, then every rank is synchronised.  Channel 0 runs on the
 * rank's stream, channel 1 (only in a context with two-stream decode) on its second stream, each with its own flag set, scratch pair and
 * epoch counter -- the context's own counters, which the call advances exactly as a step would, so that steps still work afterwards.
 *
 * Per rank r an item takes host arrays and returns host copies of everything the collective may write (the caller puts canaries
 * around the regions: the images are larger than the operands):
 *   PPLHIP_COMM_ALLREDUCE       data[r]  fp16 [data_elems]: the image of the channel's data buffer, the first `count` elements are the partial
 *                               sums; out0[r] fp16 [data_elems]: the buffer afterwards
 *   PPLHIP_COMM_ALLREDUCE_NORM  data[r]  fp16 [rows, hidden] partial sums; image0[r] / image1[r] fp16 [image_elems]: the images of the residual
 *                               rows h and of the normed matrix xn, rows first; w[r] fp16 [hidden]; out0[r] / out1[r] [image_elems]: h and xn
 *                               afterwards.  `hidden` is the item's own (% 8, <= 8192), not the model's
 *   PPLHIP_COMM_ALLGATHER       data[r]  fp32 [rows, cols]: the rank's shard; image0[r] fp32 [image_elems]: the image of the gather target, a
 *                               [rows, dst_stride] matrix (dst_stride >= ranks x cols); out0[r] [image_elems]: the target afterwards.  Channel 0
 * The inputs reach the collectives' buffers by device copies ordered on the rank's own stream in front of the item (staged on the device
 * before anything is enqueued), the outputs leave by stream-ordered device copies into separate staging.  skew (may be NULL): skew[r]
 * (0 .. 64) extra stream-ordered device copies in front of rank r's part of the item, so that the ranks arrive at different times.
 * epoch_advance (< 2^31) is added to the channel's epoch counter on every rank in front of the item.
 *
 * PPLHIP_INVALID_VALUE, before anything is enqueued on any rank and with every counter unchanged: a shape that the data buffer, the scratch
 * slice, the gather source or target cannot hold, or that the launcher refuses (count % 8, hidden % 8, hidden > 8192, odd cols or stride); a
 * channel that does not exist; a second all-gather with no all-reduce on channel 0 between the two (the all-gather has no end barrier:
 * the next one's inputs would overwrite a source that a peer may still read).  A status word that a kernel raised (a bounded wait ran
 * out) is PPLHIP_DEVICE_RUNTIME_ERROR: pplhip_last_error names the rank and the word, which is cleared.
 * counters receives local rank 0's epoch counters and all-reduce counts of both channels as the call leaves them (on every return with a
 * valid context; the ranks' counters move together). */
enum { PPLHIP_COMM_ALLREDUCE = 0, PPLHIP_COMM_ALLREDUCE_NORM = 1, PPLHIP_COMM_ALLGATHER = 2 };
typedef struct pplhip_comm_item {
    int32_t kind, channel;
    uint32_t epoch_advance;
    float eps;                      /* fused form */
    int64_t count;                  /* all-reduce: fp16 elements */
    int64_t rows, hidden;           /* fused form: rows x hidden; all-gather: rows */
    int64_t cols, dst_stride;       /* all-gather: fp32 per rank and row; row stride of the target in fp32 */
    int64_t data_elems, image_elems;
    const void* const* data;        /* [ranks] */
    const void* const* image0;      /* [ranks] */
    const void* const* image1;      /* [ranks] */
    const void* const* w;           /* [ranks] */
    const int32_t* skew;            /* [ranks] or NULL */
    void* const* out0;              /* [ranks] */
    void* const* out1;              /* [ranks] */
} pplhip_comm_item;
typedef struct pplhip_comm_op_args {
    const pplhip_comm_item* items;
    int32_t n_items;
    uint32_t* counters;             /* out [4] (may be NULL): epoch of channel 0, of channel 1, ar_count of channel 0, of channel 1 */
} pplhip_comm_op_args;
PPLHIP_API int pplhip_comm_op(pplhip_ctx* ctx, const pplhip_comm_op_args* args);

/* builds the fp32 cos/sin table [max_position, head_dim] (cos first half, sin second half per row). */
PPLHIP_API int pplhip_build_rope_table(float* host_out, int32_t max_position, int32_t head_dim, float theta);

#ifdef __cplusplus
}
#endif

#endif /* PPLHIP_H_ */
