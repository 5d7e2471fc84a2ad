// Top-N logprobs (DESIGN.md "numerics", top-N logprobs row): for the batch rows that asked, the n best tokens of the row's ranking and
// their full-vocabulary log-softmax.  The arithmetic is k_sample_dev.h's top_logprobs_row; this file runs it through a host-compacted list
// of the asking rows, as k_sample_rows.hip runs the samplers: one workgroup per asked row, a row with n = 0 is in no list and costs
// nothing, an empty list is no launch.  The outputs are compact: the j-th asked row (ascending batch row) owns [j, 0 .. 19] of both, and
// writes the first n of them.
#include "k_sample_dev.h"

namespace pplhip {

__global__ __launch_bounds__(TL_THREADS) void top_logprobs_kernel(const float* __restrict__ logits, const float* __restrict__ temperatures,
                                                                  const int32_t* __restrict__ num_logprobs, const int32_t* __restrict__ rows,
                                                                  int vocab, int stride, int32_t* __restrict__ out_tok,
                                                                  float* __restrict__ out_lp) {
    const int b = rows[blockIdx.x];
    const bool vec = (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    top_logprobs_row(logits + (int64_t)b * stride, vec, row_temperature(temperatures, b), num_logprobs[b], vocab,
                     out_tok + (int64_t)blockIdx.x * TOP_LOGPROBS_MAX, out_lp + (int64_t)blockIdx.x * TOP_LOGPROBS_MAX);
}

hipError_t launch_top_logprobs(hipStream_t s, const float* logits, const float* temperatures, const int32_t* num_logprobs,
                               const int32_t* rows, int n_rows, int vocab, int stride, int32_t* out_tok, float* out_logprob) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(top_logprobs_kernel, dim3(n_rows), dim3(TL_THREADS), 0, s, logits, temperatures, num_logprobs, rows, vocab, stride,
                       out_tok, out_logprob);
    return hipGetLastError();
}

}  // namespace pplhip
