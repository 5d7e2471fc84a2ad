// K12 apply_penalty and K13 sample_topk_topp: the sampler behind PostProcessor
// (src/common/post_processor.h:25-43; driver src/backends/cuda/post_processor.cc:121-281).  The reference
// kernels live in ppl.llm.kernel.cuda (not in the tree); semantics are fixed by DESIGN.md "sampler" and
// restated by ref_sample / ref_penalty (oracle/llama_ref.c).  HBM/L2-bound row kernels, one workgroup per row.
// The two sampling rules themselves are the row functions of k_sample_dev.h; the kernels here hand them one launch's uniform
// top_k / default top_p and the caller's random numbers (k_sample_rows.hip: every row's own).
#include "k_sample_dev.h"

namespace pplhip {

__global__ __launch_bounds__(SG_THREADS) void sample_greedy_kernel(const float* __restrict__ logits,
                                                                   const float* __restrict__ temperatures, int vocab, int stride,
                                                                   int32_t* __restrict__ out_tok, float* __restrict__ out_lp) {
    const int b = blockIdx.x;
    const bool vec = (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    sample_greedy_row(logits + (int64_t)b * stride, vec, row_temperature(temperatures, b), vocab, out_tok + b, out_lp + b);
}

hipError_t launch_sample_greedy(hipStream_t s, const float* logits, const float* temperatures, int batch, int vocab,
                                int stride, int32_t* out_tok, float* out_logprob) {
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(sample_greedy_kernel, dim3(batch), dim3(SG_THREADS), 0, s, logits, temperatures, vocab, stride, out_tok,
                       out_logprob);
    return hipGetLastError();
}

__global__ __launch_bounds__(ST_THREADS) void sample_topk_topp_kernel(const float* __restrict__ logits,
                                                                      const float* __restrict__ temperatures,
                                                                      const float* __restrict__ top_p, const float* __restrict__ rnd,
                                                                      int vocab, int stride, int top_k, float default_top_p,
                                                                      int32_t* __restrict__ out_tok, float* __restrict__ out_lp) {
    const int b = blockIdx.x;
    sample_topk_topp_row(logits + (int64_t)b * stride, row_temperature(temperatures, b), top_k, top_p ? top_p[b] : default_top_p, rnd[b],
                         vocab, out_tok + b, out_lp + b);
}

size_t sample_topk_workspace_bytes(int, int, int) { return 0; }

hipError_t launch_sample_topk_topp(hipStream_t s, const float* logits, const float* temperatures, const float* top_p,
                                   const float* rnd, int batch, int vocab, int stride, int top_k, float default_top_p,
                                   void*, int32_t* out_tok, float* out_logprob) {
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(sample_topk_topp_kernel, dim3(batch), dim3(ST_THREADS), 0, s, logits, temperatures, top_p, rnd, vocab,
                       stride, top_k, default_top_p, out_tok, out_logprob);
    return hipGetLastError();
}

// penalty: count map row batch_slots[b] (uint16, saturating) counts every token the request has fed the model;
// cleared on a request's first step: start_pos[b] == 0, or row b >= decoding_batches (a prefill row -- a prompt is always
// prefilled in ONE step, so this also catches a prefix-cache hit that starts at start_pos = hit > 0 in a reused batch slot;
// the cached prompt tokens themselves are never fed and stay uncounted, as in the reference).  For counted tokens: x = x > 0 ? x/rep : x*rep; x -= presence; x -= freq*count;
// finally every logit is divided by the temperature.
__global__ __launch_bounds__(256) void penalty_kernel(float* __restrict__ logits, const float* __restrict__ temperatures,
                                                      const float* __restrict__ rep, const float* __restrict__ presence,
                                                      const float* __restrict__ frequency,
                                                      const int64_t* __restrict__ batch_slots,
                                                      const int64_t* __restrict__ token_inputs,
                                                      const int64_t* __restrict__ seq_starts,
                                                      const int64_t* __restrict__ start_pos, int vocab, int stride,
                                                      int decoding_batches, uint16_t* __restrict__ count_map) {
    const int b = blockIdx.x;
    uint16_t* cm = count_map + batch_slots[b] * (int64_t)vocab;
    if (start_pos[b] == 0 || b >= decoding_batches) {
        for (int v = threadIdx.x; v < vocab; v += 256) cm[v] = 0;
    }
    __syncthreads();
    for (int64_t t = seq_starts[b] + threadIdx.x; t < seq_starts[b + 1]; t += 256) {
        const int64_t tok = token_inputs[t];
        uint32_t* word = reinterpret_cast<uint32_t*>(cm + (tok & ~(int64_t)1));  // rows are 4-byte aligned (vocab even)
        const int sh = (tok & 1) ? 16 : 0;
        uint32_t old = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (true) {
            const uint32_t cnt = (old >> sh) & 0xffffu;
            if (cnt == 0xffffu) break;
            const uint32_t nw = old + (1u << sh);
            const uint32_t prev = atomicCAS(word, old, nw);
            if (prev == old) break;
            old = prev;
        }
    }
    __threadfence_block();
    __syncthreads();
    float* row = logits + (int64_t)b * stride;
    const float t = (temperatures && temperatures[b] > 0.f) ? temperatures[b] : 1.0f;
    const float r = rep ? rep[b] : 1.0f;
    for (int v = threadIdx.x; v < vocab; v += 256) {
        float x = row[v];
        // agent-scope load: the counts were updated by L2 atomics, a plain load could hit a stale L1 line
        const uint32_t cw = __hip_atomic_load(reinterpret_cast<uint32_t*>(cm) + (v >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t c = (cw >> (16 * (v & 1))) & 0xffffu;
        if (c) {
            x = x > 0.f ? x / r : x * r;
            if (presence) x -= presence[b];
            if (frequency) x -= frequency[b] * (float)c;
        }
        row[v] = x / t;
    }
}

hipError_t launch_penalty(hipStream_t s, float* logits, const float* temperatures, const float* rep,
                          const float* presence, const float* frequency, const int64_t* batch_slots,
                          const int64_t* token_inputs, const int64_t* seq_starts, const int64_t* start_pos, int batch,
                          int vocab, int stride, int decoding_batches, uint16_t* count_map) {
    if (batch == 0) return hipSuccess;
    if (vocab & 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(penalty_kernel, dim3(batch), dim3(256), 0, s, logits, temperatures, rep, presence, frequency,
                       batch_slots, token_inputs, seq_starts, start_pos, vocab, stride, decoding_batches, count_map);
    return hipGetLastError();
}

}  // namespace pplhip
