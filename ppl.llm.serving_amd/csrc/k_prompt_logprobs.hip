// Prompt logprobs (DESIGN.md "numerics", prompt logprobs row): for the prompt positions that asked, the logprob and the rank of the prompt
// token that follows, under the model's own distribution (raw fp32 logits), and for positions with n >= 1 the first n entries of the
// position's ranking.  The arithmetic is k_sample_dev.h's prompt_logprob_row and, for the ranking, top_logprobs_row at temperature 1 (no
// second ranking); this file runs them through a host-compacted list of the asked positions, as k_logprobs.hip runs the top-N logprobs: one
// workgroup per asked position, a position nobody asked for is in no list and costs nothing, an empty list is no launch.
// Position j of the list reads logits row j (the lm_head ran on exactly the listed rows) and its target from the step's device-resident
// tokens: tokens[rows[j] + 1], rows[j] the packed row of the step.
#include "k_sample_dev.h"

namespace pplhip {

__global__ __launch_bounds__(TL_THREADS) void prompt_logprobs_kernel(const float* __restrict__ logits, int stride, int vocab,
                                                                     const int32_t* __restrict__ rows, const int64_t* __restrict__ tokens,
                                                                     const int32_t* __restrict__ n_top, float* __restrict__ out_lp,
                                                                     int32_t* __restrict__ out_rank, int32_t* __restrict__ out_top_tok,
                                                                     float* __restrict__ out_top_lp) {
    const int j = blockIdx.x;
    const float* row = logits + (int64_t)j * stride;
    const bool vec = (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    const int64_t tk = tokens[(int64_t)rows[j] + 1];
    if (tk < 0 || tk >= vocab) {   // (the product validates the step's tokens on the host; the operator's come from its caller) uniform
        if (threadIdx.x == 0) { out_lp[j] = NAN; out_rank[j] = -1; }
        return;
    }
    const int target = (int)tk;
    prompt_logprob_row(row, vec, target, vocab, out_lp + j, out_rank + j);
    const int n = n_top[j];   // uniform over the block
    if (n > 0) top_logprobs_row(row, vec, 1.0f, n, vocab, out_top_tok + (int64_t)j * TOP_LOGPROBS_MAX, out_top_lp + (int64_t)j * TOP_LOGPROBS_MAX);
}

hipError_t launch_prompt_logprobs(hipStream_t s, const float* logits, int stride, int vocab, const int32_t* rows, int n_rows,
                                  const int64_t* tokens, const int32_t* n_top, float* out_lp, int32_t* out_rank, int32_t* out_top_tok,
                                  float* out_top_lp) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(prompt_logprobs_kernel, dim3(n_rows), dim3(TL_THREADS), 0, s, logits, stride, vocab, rows, tokens, n_top, out_lp, out_rank,
                       out_top_tok, out_top_lp);
    return hipGetLastError();
}

}  // namespace pplhip
