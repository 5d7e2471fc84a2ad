// The per-request sampler (DESIGN.md "numerics", per-request sampler row): every batch row with its own temperature, top_k, top_p and
// random number, the random number made on the device from (seed, draw) by Philox4x32-10.  The arithmetic is k_sample_dev.h's -- the same
// two row functions K13 instantiates -- so a row's token and logprob bits equal those of sample_greedy_kernel / sample_topk_topp_kernel
// launched on that row with the row's parameters.
//
// Form taken: up to THREE launches over a host-compacted row list, greedy rows (top_k == 1) at SG_THREADS = 1024 threads, the other rows
// at ST_THREADS = 256, the ones that ask for a min_p or typical_p cut (sample_trunc_row) apart from the ones that do not; a launch with no
// rows is not issued, so an all-greedy and an all-sampling batch cost exactly one launch and a batch in which nobody asks for a cut takes
// the launches it took before the third kind existed.  Why not one
// launch whose blocks branch per row: the two row functions are written for different block widths (the width fixes the summation order,
// i.e. the logprob bits), so a common block would have to be 1024 threads wide with 768 of them idle through every barrier of a sampling
// row, and the kernel would carry the larger register and LDS footprint of the two for every row.  With the list each kind keeps exactly
// the launch shape, occupancy and code of its K13 kernel; the added work is one list load, the row's parameter loads and the ten-round
// integer hash.
#include "k_sample_dev.h"

namespace pplhip {

// Philox4x32-10 (Salmon et al., SC'11): counter (n lo, n hi, 0, 0), key (seed lo, seed hi); output word 0
__device__ __forceinline__ uint32_t philox_word0(uint64_t seed, uint64_t n) {
    uint32_t c0 = (uint32_t)n, c1 = (uint32_t)(n >> 32), c2 = 0, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
// u = fp32(w0 >> 8) * 2^-24 in [0, 1 - 2^-24]: 24 bits, exact
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t n) {
    return (float)(philox_word0(seed, n) >> 8) * 0x1p-24f;
}

__global__ __launch_bounds__(256) void sample_uniform_kernel(const uint64_t* __restrict__ seeds, const uint64_t* __restrict__ draws, int batch,
                                                             float* __restrict__ out_u) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < batch) out_u[b] = philox_uniform(seeds[b], draws[b]);
}

hipError_t launch_sample_uniform(hipStream_t s, const uint64_t* seeds, const uint64_t* draws, int batch, float* out_u) {
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(sample_uniform_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, seeds, draws, batch, out_u);
    return hipGetLastError();
}

__global__ __launch_bounds__(SG_THREADS) void sample_rows_greedy_kernel(const float* __restrict__ logits,
                                                                        const float* __restrict__ temperatures,
                                                                        const int32_t* __restrict__ rows, int vocab, int stride,
                                                                        int32_t* __restrict__ out_tok, float* __restrict__ out_lp) {
    const int b = rows[blockIdx.x];
    const bool vec = (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    sample_greedy_row(logits + (int64_t)b * stride, vec, row_temperature(temperatures, b), vocab, out_tok + b, out_lp + b);
}

__global__ __launch_bounds__(ST_THREADS) void sample_rows_topk_topp_kernel(const float* __restrict__ logits,
                                                                           const float* __restrict__ temperatures,
                                                                           const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                                           const uint64_t* __restrict__ seeds, const uint64_t* __restrict__ draws,
                                                                           const float* __restrict__ rnd, const int32_t* __restrict__ rows,
                                                                           int vocab, int stride, int32_t* __restrict__ out_tok,
                                                                           float* __restrict__ out_lp) {
    const int b = rows[blockIdx.x];
    const float u = rnd ? rnd[b] : philox_uniform(seeds[b], draws[b]);
    sample_topk_topp_row(logits + (int64_t)b * stride, row_temperature(temperatures, b), top_k[b], top_p[b], u, vocab, out_tok + b,
                         out_lp + b);
}

// the truncating rows (min_p or typical_p on): min_p / typical_p may be NULL (off for every row)
__global__ __launch_bounds__(ST_THREADS) void sample_rows_trunc_kernel(const float* __restrict__ logits, const float* __restrict__ temperatures,
                                                                       const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                                       const float* __restrict__ min_p, const float* __restrict__ typical_p,
                                                                       const uint64_t* __restrict__ seeds, const uint64_t* __restrict__ draws,
                                                                       const float* __restrict__ rnd, const int32_t* __restrict__ rows,
                                                                       int vocab, int stride, int32_t* __restrict__ out_tok,
                                                                       float* __restrict__ out_lp) {
    const int b = rows[blockIdx.x];
    const float u = rnd ? rnd[b] : philox_uniform(seeds[b], draws[b]);
    sample_trunc_row(logits + (int64_t)b * stride, row_temperature(temperatures, b), top_k[b], top_p[b], min_p ? min_p[b] : 0.f,
                     typical_p ? typical_p[b] : 0.f, u, vocab, out_tok + b, out_lp + b);
}

hipError_t launch_sample_rows(hipStream_t s, const float* logits, const float* temperatures, const int32_t* top_k, const float* top_p,
                              const uint64_t* seeds, const uint64_t* draws, const float* rnd, const int32_t* rows, int n_greedy,
                              int n_sampling, int vocab, int stride, int32_t* out_tok, float* out_logprob, const float* min_p,
                              const float* typical_p, int n_trunc) {
    if (n_greedy > 0) {
        hipLaunchKernelGGL(sample_rows_greedy_kernel, dim3(n_greedy), dim3(SG_THREADS), 0, s, logits, temperatures, rows, vocab, stride,
                           out_tok, out_logprob);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (n_sampling > 0) {
        hipLaunchKernelGGL(sample_rows_topk_topp_kernel, dim3(n_sampling), dim3(ST_THREADS), 0, s, logits, temperatures, top_k, top_p, seeds,
                           draws, rnd, rows + n_greedy, vocab, stride, out_tok, out_logprob);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (n_trunc > 0) {
        hipLaunchKernelGGL(sample_rows_trunc_kernel, dim3(n_trunc), dim3(ST_THREADS), 0, s, logits, temperatures, top_k, top_p, min_p, typical_p,
                           seeds, draws, rnd, rows + n_greedy + n_sampling, vocab, stride, out_tok, out_logprob);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace pplhip
