/* C ABI of the serving core (LLMGenerator + engine + hip backend) for front ends that are not C++: the gRPC server of
 * ppl.llm.serving_amd/serving/grpc_server.py binds it with ctypes.  It plays the role of the reference's
 * GRPCConnection/GRPCServer pair towards the generator (src/serving/grpc/grpc_server.cc:88-341): requests go in through
 * LLMGenerator::Process, responses come back through a Connection whose Send() fills a queue that pplsrv_poll drains. */
#ifndef PPLSRV_SERVING_C_H_
#define PPLSRV_SERVING_C_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PPLSRV_API __attribute__((visibility("default")))

typedef struct pplsrv pplsrv;

/* the tool flags of tools/offline_inference.cc:40-90 that matter to a server (0 / NULL = the tool's default) */
typedef struct pplsrv_config {
    const char* model_param_path;  /* params.json */
    const char* model_dir;         /* model_slice_<rank>/weights.pplhip; ignored with synthetic_weights */
    int32_t tensor_parallel_size;
    int32_t synthetic_weights;
    uint64_t synthetic_seed;
    uint64_t kv_cache_max_tokens;  /* 0: max_tokens_scale x free memory */
    float max_tokens_scale;
    int32_t max_running_batch, max_tokens_per_step;
    int32_t max_input_tokens_per_request, max_output_tokens_per_request, max_total_tokens_per_request;
    int32_t max_prefill_batch, max_cooldown_request;
    int32_t enable_prefix_cache, enable_penalty;
    const int32_t* stop_tokens;    /* EOS-like tokens (GeneratorConfig::stop_tokens) */
    int32_t n_stop_tokens;
    const char* tokenizer_path;    /* --tokenizer-path: text requests are tokenised / detokenised inside the generator (src/tokenizer);
                                      NULL or "": token-in/token-out only, a text request fails */
    const char* tokenizer_type;    /* --tokenizer-type, NULL = "sentencepiece" */
    const char* model_type;        /* --model-type, NULL = "llama" (LlamaTokenizer: BOS first) */
    const char* quant_method;      /* --quant-method: NULL / "none" / "online_i8i8" / "online_f8f8" */
    float top_p;                   /* --top-p, --top-k: the generator's defaults (GeneratorConfig; 0 / 0 = the tools' 0.0 and 1) */
    int32_t top_k;
    int32_t decoding_attn_split_k; /* --configure-decoding-attn-split-k + 1 (0 = the default, heuristic) */
    int32_t decoding_attn_tpb;     /* --specify-decoding-attn-tpb */
} pplsrv_config;

/* ParseRequest of grpc_server.cc:218-252 already applied by the caller */
typedef struct pplsrv_request {
    uint64_t id;
    const int32_t* tokens;
    int32_t n_tokens;
    float temperature, top_p;
    int32_t top_k;
    float repetition_penalty, presence_penalty, frequency_penalty;
    int32_t generation_length;
    int32_t early_stopping;
    const char* prompt;            /* text request (proto Request.prompt) when tokens == NULL: n_prompt UTF-8 bytes */
    int32_t n_prompt;
} pplsrv_request;

enum { PPLSRV_PROCESSING = 0, PPLSRV_FINISHED = 1, PPLSRV_FAILED = 2 };          /* proto Status */
enum { PPLSRV_REASON_LENGTH = 0, PPLSRV_REASON_EOS = 1, PPLSRV_REASON_STOP = 2 }; /* proto FinishReason */

typedef struct pplsrv_response {
    uint64_t id;
    int32_t token;
    float logprob;
    int32_t status;
    int32_t finish_reason;
    int32_t is_special;
    int32_t text_len;              /* text requests: bytes of this response's `generated` text ... */
    int64_t text_off;              /* ... at this offset of the text buffer handed to pplsrv_poll_text (-1: none / did not fit) */
} pplsrv_response;

PPLSRV_API int pplsrv_create(const pplsrv_config* cfg, pplsrv** out);      /* 0 on success, a negated RetCode otherwise */
PPLSRV_API int pplsrv_submit(pplsrv* s, const pplsrv_request* reqs, int32_t n);
/* LoRA adapters (include/pplhip.h "multi-LoRA"; pplsrv_request keeps its layout, so a request's adapter travels beside it).
 * pplsrv_load_adapter reads <dir>/lora.pplhip into slot 0 .. 63 on every rank; pplsrv_unload_adapter refuses a slot that a pending or
 * running request names; pplsrv_submit_lora is pplsrv_submit with slots[i] the adapter of reqs[i] (-1 = none; slots NULL = none at all).
 * A request that names a slot nothing is loaded in fails (PPLSRV_FAILED).  K/V pages computed under an adapter are shared through the
 * prefix cache only among requests on the same load of that adapter. */
PPLSRV_API int pplsrv_load_adapter(pplsrv* s, int32_t slot, const char* dir);
PPLSRV_API int pplsrv_unload_adapter(pplsrv* s, int32_t slot);
PPLSRV_API int pplsrv_submit_lora(pplsrv* s, const pplsrv_request* reqs, const int32_t* slots, int32_t n);
/* The per-request sampler (both structs keep their layout, so its switch and a request's seed travel beside them).  pplsrv_create_ex is
 * pplsrv_create with GeneratorConfig::per_request_sampling and ::sampling_seed (0: a seed from std::random_device); with the switch on
 * every request is sampled with its own top_k / top_p / temperature and a random sequence of its own.  pplsrv_submit_ex is
 * pplsrv_submit_lora with seeds[i] the sampling seed of reqs[i] (0 = none: the generator gives it the next one of sampling_seed's
 * sequence); slots NULL = no adapters, seeds NULL = no seeds. */
PPLSRV_API int pplsrv_create_ex(const pplsrv_config* cfg, int32_t per_request_sampling, uint64_t sampling_seed, pplsrv** out);
PPLSRV_API int pplsrv_submit_ex(pplsrv* s, const pplsrv_request* reqs, const int32_t* slots, const uint64_t* seeds, int32_t n);
/* Top-N logprobs (both structs keep their layout, so a request's count and a response's lists travel beside them).
 * pplsrv_submit_logprobs is pplsrv_submit_ex with num_logprobs[i] the number of ranked alternatives reqs[i] wants with every generated
 * token (Request::num_logprobs: above PPLSRV_TOP_LOGPROBS_MAX counts as that, negative as 0; num_logprobs NULL = nobody asks).
 * pplsrv_poll_logprobs is pplsrv_poll_text (text_buf may be NULL) with tops[i] the lists of out[i]: n entries, best first, entry 0 the
 * greedy token; n = 0 when the request did not ask. */
#define PPLSRV_TOP_LOGPROBS_MAX 20
typedef struct pplsrv_top_logprobs {
    int32_t n;
    int32_t tokens[PPLSRV_TOP_LOGPROBS_MAX];
    float logprobs[PPLSRV_TOP_LOGPROBS_MAX];
} pplsrv_top_logprobs;
PPLSRV_API int pplsrv_submit_logprobs(pplsrv* s, const pplsrv_request* reqs, const int32_t* slots, const uint64_t* seeds,
                                      const int32_t* num_logprobs, int32_t n);
PPLSRV_API int pplsrv_poll_logprobs(pplsrv* s, pplsrv_response* out, int32_t max, int32_t timeout_ms, char* text_buf, int64_t text_buf_bytes,
                                    pplsrv_top_logprobs* tops);
/* Logit rules (pplsrv_request keeps its layout, so a request's rule travels beside it).  pplsrv_submit_rules is pplsrv_submit_logprobs with
 * rules[i] the rule of reqs[i]: Request::logit_bias (pairs bias_tokens[j], bias_values[j]; -inf bans), ::allowed_tokens (has_allowed != 0:
 * the only tokens the request may produce, n_allowed of them), ::banned_tokens and ::min_new_tokens.  rules NULL or rules[i] NULL: no rule.
 * The arrays are read before the call returns.  A rule is validated when its request is admitted; an invalid one fails that request alone
 * (PPLSRV_FAILED), as does any rule on a backend without logit rules. */
typedef struct pplsrv_rule {
    const int32_t* bias_tokens;
    const float* bias_values;
    int32_t n_bias;
    const int32_t* allowed_tokens;
    int32_t n_allowed;
    int32_t has_allowed;
    const int32_t* banned_tokens;
    int32_t n_banned;
    int32_t min_new_tokens;
} pplsrv_rule;
PPLSRV_API int pplsrv_submit_rules(pplsrv* s, const pplsrv_request* reqs, const int32_t* slots, const uint64_t* seeds,
                                   const int32_t* num_logprobs, const pplsrv_rule* const* rules, int32_t n);
/* Prompt logprobs (both structs keep their layout).  pplsrv_submit_prompt_logprobs is pplsrv_submit_rules with prompt_logprobs[i] =
 * Request::prompt_logprobs of reqs[i]: -1 off, 0 the logprob and rank of every prompt token but the first under the model's own
 * distribution, 1 .. 20 also that many entries of every position's ranking (above 20: 20, below -1: -1; NULL = nobody asks).  Such a
 * request takes no prefix-cache hit.  On a backend without prompt logprobs (tensor parallelism among them) it fails alone (PPLSRV_FAILED).
 * pplsrv_poll_prompt_logprobs is pplsrv_poll_logprobs (text_buf and tops may be NULL) with prompts[i] the record of out[i]: the response
 * that carries a request's first token has positions = prompt length - 1 numbers at logprob_buf[off ..) and rank_buf[off ..), position
 * t - 1 for prompt token t, and for n_top >= 1 positions x n_top entries at top_token_buf[top_off ..) / top_logprob_buf[top_off ..), n_top
 * per position, best first (token -1 / -inf behind the vocabulary); every other response has positions = 0.  The buffers hold
 * buf_positions and top_buf_entries numbers for the whole call, filled back to back; a response whose lists do not fit any more stays
 * queued for the next call, and one that alone does not fit is delivered with off = top_off = -1. */
typedef struct pplsrv_prompt_logprobs {
    int32_t positions;
    int32_t n_top;
    int64_t off;
    int64_t top_off;
} pplsrv_prompt_logprobs;
PPLSRV_API int pplsrv_submit_prompt_logprobs(pplsrv* s, const pplsrv_request* reqs, const int32_t* slots, const uint64_t* seeds,
                                             const int32_t* num_logprobs, const pplsrv_rule* const* rules, const int32_t* prompt_logprobs,
                                             int32_t n);
PPLSRV_API int pplsrv_poll_prompt_logprobs(pplsrv* s, pplsrv_response* out, int32_t max, int32_t timeout_ms, char* text_buf,
                                           int64_t text_buf_bytes, pplsrv_top_logprobs* tops, pplsrv_prompt_logprobs* prompts,
                                           float* logprob_buf, int32_t* rank_buf, int64_t buf_positions, int32_t* top_token_buf,
                                           float* top_logprob_buf, int64_t top_buf_entries);
/* Guided decoding.  pplsrv_submit_guided is pplsrv_submit_prompt_logprobs with guide_regex[i] = Request::guide_regex of reqs[i]: a
 * NUL-terminated regular expression (src/common/guide.h has the dialect) that the bytes of the request's generated tokens must match in
 * full; NULL or "" = no guide; guide_regex NULL: nobody is guided.  The strings are read before the call returns.  The guide is compiled
 * and checked when its request is admitted; a pattern outside the dialect or too large, a request that also carries allowed_tokens,
 * banned_tokens, min_new_tokens, a -inf bias or early_stopping == 0, a server without a tokenizer, a backend without guides and a 17th
 * pattern while 16 are in use each fail that request alone (PPLSRV_FAILED). */
PPLSRV_API int pplsrv_submit_guided(pplsrv* s, const pplsrv_request* reqs, const int32_t* slots, const uint64_t* seeds,
                                    const int32_t* num_logprobs, const pplsrv_rule* const* rules, const int32_t* prompt_logprobs,
                                    const char* const* guide_regex, int32_t n);
/* The same by a JSON schema.  pplsrv_submit_guided_json is pplsrv_submit_guided with guide_json_schema[i] = Request::guide_json_schema of
 * reqs[i]: the NUL-terminated text of a JSON schema (src/common/guide_json.h has the subset and the one layout of the answer's text);
 * NULL or "" = no schema; guide_json_schema NULL: nobody has one.  The answer of such a request is a JSON document that fits the schema.
 * What fails a request with guide_regex fails this one alone too, as do a schema outside the subset or of more than 4096 states, a
 * request that carries both a pattern and a schema, and a backend without wide guides. */
PPLSRV_API int pplsrv_submit_guided_json(pplsrv* s, const pplsrv_request* reqs, const int32_t* slots, const uint64_t* seeds,
                                         const int32_t* num_logprobs, const pplsrv_rule* const* rules, const int32_t* prompt_logprobs,
                                         const char* const* guide_regex, const char* const* guide_json_schema, int32_t n);
/* min_p / typical_p (DESIGN.md "numerics", min_p / typical_p row).  pplsrv_submit_sampling is pplsrv_submit_guided_json with
 * min_p[i] = Request::min_p and typical_p[i] = Request::typical_p of reqs[i]; either array NULL: nobody asks (min_p 0, typical_p 1).
 * min_p is off when <= 0 or NaN, typical_p when <= 0, >= 1 or NaN.  A request that turns one on on a server created without
 * per_request_sampling, or over a backend without the truncating sampler, fails alone (PPLSRV_FAILED).  pplsrv_request keeps its layout. */
PPLSRV_API int pplsrv_submit_sampling(pplsrv* s, const pplsrv_request* reqs, const int32_t* slots, const uint64_t* seeds,
                                      const int32_t* num_logprobs, const pplsrv_rule* const* rules, const int32_t* prompt_logprobs,
                                      const char* const* guide_regex, const char* const* guide_json_schema, const float* min_p,
                                      const float* typical_p, int32_t n);
/* waits up to timeout_ms for at least one response, then returns up to `max` of them (0 on timeout) */
PPLSRV_API int pplsrv_poll(pplsrv* s, pplsrv_response* out, int32_t max, int32_t timeout_ms);
/* the same, plus the generated text of text requests (what DecodeAndSendTask, llm_generator.cc:58-112, put into Response::generated:
 * possibly empty while a multi-byte character is still incomplete): copied back to back into text_buf */
PPLSRV_API int pplsrv_poll_text(pplsrv* s, pplsrv_response* out, int32_t max, int32_t timeout_ms, char* text_buf, int64_t text_buf_bytes);
PPLSRV_API int pplsrv_cancel(pplsrv* s, uint64_t id);                      /* client went away: LLMGenerator::ClearTask */
PPLSRV_API uint64_t pplsrv_kv_cache_max_tokens(pplsrv* s);
PPLSRV_API void pplsrv_destroy(pplsrv* s);

#ifdef __cplusplus
}
#endif
#endif
