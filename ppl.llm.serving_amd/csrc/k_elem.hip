// K1 embedding gather, K2 (Skip)RMSNorm (+ last-token gather of K11), K10 SwiGLU -- HBM-bound row kernels.
// One 256-thread workgroup per row, 16-byte (8 x fp16) accesses per lane, fp32 arithmetic.
// Semantics: DESIGN.md "numerics"; oracle: ref_embedding / ref_rmsnorm / ref_silu_mul (oracle/llama_ref.c).
#include <stdlib.h>
#include "kernels.h"

namespace pplhip {

__global__ __launch_bounds__(256) void embedding_kernel(const int64_t* __restrict__ ids, const uint4* __restrict__ table,
                                                        int chunks /* hidden/8 */, uint4* __restrict__ out) {
    const int64_t t = blockIdx.x;
    const int64_t row = ids[t];
    for (int c = threadIdx.x; c < chunks; c += 256) out[t * chunks + c] = table[row * chunks + c];
}

hipError_t launch_embedding(hipStream_t s, const int64_t* token_ids, const uint16_t* table, int64_t T, int hidden,
                            uint16_t* out) {
    if (T == 0) return hipSuccess;
    hipLaunchKernelGGL(embedding_kernel, dim3((unsigned)T), dim3(256), 0, s, token_ids, (const uint4*)table, hidden / 8,
                       (uint4*)out);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void gather_last_rows_kernel(const int64_t* __restrict__ seq_starts, const uint4* __restrict__ x, int chunks,
                                                               uint4* __restrict__ out) {
    const int64_t r = blockIdx.x, src = seq_starts[r + 1] - 1;
    for (int c = threadIdx.x; c < chunks; c += 256) out[r * chunks + c] = x[src * chunks + c];
}

hipError_t launch_gather_last_rows(hipStream_t s, const uint16_t* x, const int64_t* seq_starts, int64_t B, int hidden, uint16_t* out) {
    if (B == 0) return hipSuccess;
    if (hidden % 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_last_rows_kernel, dim3((unsigned)B), dim3(256), 0, s, seq_starts, (const uint4*)x, hidden / 8, (uint4*)out);
    return hipGetLastError();
}

// Each thread keeps up to MAXC chunks of its row in registers (hidden <= 256*8*MAXC); larger rows re-read.
// NT threads per row: 256, or -- steps of a few hundred rows at most, where the launch is one block per CU or less and a row is a chain of
// latencies (load, reduce, barrier, store) rather than bandwidth -- 512 / 1024 with one chunk per thread (launch_rmsnorm)
template <int MAXC, int NT = 256, bool F8 = false>
__global__ __launch_bounds__(NT) void rmsnorm_kernel(const uint4* x /* may alias residual_out */, const uint4* __restrict__ skip,
                                                      const uint4* __restrict__ w, float eps, int chunks, int hidden,
                                                      const int64_t* __restrict__ gather, uint4* __restrict__ out,
                                                      uint4* residual_out, int8_t* __restrict__ qout, float* __restrict__ sx, SplitSlabs sl) {
    __shared__ float red[NT / 64];
    __shared__ float redq[NT / 64];
    const int64_t r = blockIdx.x;
    const int64_t src = gather ? gather[r + 1] - 1 : r;
    float v[MAXC][8];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c = threadIdx.x + i * NT;
        if (c < chunks) {
            unpack8(x[src * chunks + c], v[i]);
            if (skip || sl.splits) {
                float sk[8];
                if (sl.splits) slab_load8(sl, src, c * 8, sk);   // the skip operand straight from the producing GEMM's split-K slabs
                else unpack8(skip[src * chunks + c], sk);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i][j] = round_h(v[i][j] + sk[j]);
                if (residual_out) residual_out[r * chunks + c] = pack8(v[i]);
            } else if (residual_out) {
                residual_out[r * chunks + c] = pack8(v[i]);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
        }
    }
    // the norm weights are fetched before the reduction so that their latency hides under it
    uint4 wraw[MAXC];
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c = threadIdx.x + i * NT;
        wraw[i] = c < chunks ? w[c] : make_uint4(0, 0, 0, 0);
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    ss = red[0] + red[1] + red[2] + red[3];
#pragma unroll
    for (int wv = 4; wv < NT / 64; ++wv) ss += red[wv];
    const float inv = 1.0f / sqrtf(ss / (float)hidden + eps);
    if (!qout) {
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const int c = threadIdx.x + i * NT;
            if (c < chunks) {
                float wf[8], o[8];
                unpack8(wraw[i], wf);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = v[i][j] * inv * wf[j];
                out[r * chunks + c] = pack8(o);
            }
        }
        return;
    }
    // online_i8i8: the normalised row goes straight to the next linear's int8 operand (k_gemm_i8.hip, quant_act_kernel's
    // arithmetic on the fp16-rounded values: sx = max|y| / 127, q = clamp(rint(y * (127 / max|y|))))
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c = threadIdx.x + i * NT;
        if (c < chunks) {
            float wf[8];
            unpack8(wraw[i], wf);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                v[i][j] = round_h(v[i][j] * inv * wf[j]);
                amax = fmaxf(amax, fabsf(v[i][j]));
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if ((threadIdx.x & 63) == 0) redq[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(redq[0], redq[1]), fmaxf(redq[2], redq[3]));
#pragma unroll
    for (int wv = 4; wv < NT / 64; ++wv) amax = fmaxf(amax, redq[wv]);
    if constexpr (F8) {   // online_f8f8: the same rows as e4m3fn codes under 2^e (k_gemm_i8.hip, quant_act_f8_kernel)
        const int e = fp8_row_exp(amax);
        if (threadIdx.x == 0) sx[r] = pow2f(e);
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const int c = threadIdx.x + i * NT;
            if (c < chunks) {
                uint32_t lo = 0, hi = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lo |= fp8_quant(v[i][j], e) << (8 * j);
                    hi |= fp8_quant(v[i][4 + j], e) << (8 * j);
                }
                *reinterpret_cast<uint2*>(qout + r * (int64_t)hidden + c * 8) = make_uint2(lo, hi);
            }
        }
        return;
    }
    const float qinv = amax > 0.f ? 127.0f / amax : 0.f;
    if (threadIdx.x == 0) sx[r] = amax / 127.0f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c = threadIdx.x + i * NT;
        if (c < chunks) {
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = fminf(fmaxf(rintf(v[i][j] * qinv), -127.f), 127.f), b = fminf(fmaxf(rintf(v[i][4 + j] * qinv), -127.f), 127.f);
                lo |= (uint32_t)((int)a & 0xff) << (8 * j);
                hi |= (uint32_t)((int)b & 0xff) << (8 * j);
            }
            *reinterpret_cast<uint2*>(qout + r * (int64_t)hidden + c * 8) = make_uint2(lo, hi);
        }
    }
}

// The form a launch takes, decided by (rows, hidden) alone: the record of pplhip_op_rmsnorm_form and the launch below come from this one
// function (as Half128Kernel / DmaKernel in k_gemm.hip).  No HIP call.
//
// few rows of a wide model (decode steps of 5..512 rows at hidden >= 4096): one chunk per thread on 512 / 1024 threads -- every load of
// the row is in flight at once.  -1.9 % on config 4's per-rank step and -0.4..-1.7 % on 7B steps of 8-512 rows
// (profiles/r04_rmsnorm_wide_ab.log).  The two forms sum a row's squares in different orders, so a token's norm -- and in the last bits
// its logits -- depend on the step's row count class (<= 4, 5..512, > 512; the 512-row halves of a two-stream step): the same kind of
// dependence as the GEMM tile choice by M, inside the specification's noise floor, guarded by the greedy-token tests
// (tests/test_gpu_config5_tokens.py, test_gpu_model.py).  Up to 4 rows stay on the 256-thread form only because a block of 1024
// threads per row buys nothing there.  Round 4 kept the wide form opt-in: its summation order moved the 70B / TP8 W4A16 parity case
// over its fixed cap -- a case that the grouped-query decode kernel's rounded V had already brought to 0.90 of that cap; with V exact
// again (k_attn_decode_gqa.hip, round 5) the case sits at 0.89e-3 = 1.27 x the oracle's noise floor WITH this form
// (profiles/r05_w4_gqa_margin.log).
hipError_t rmsnorm_form(int64_t rows, int hidden, int wide_max_rows, RmsnormForm* f) {
    *f = RmsnormForm{};
    if (rows == 0) return hipSuccess;
    const int chunks = hidden / 8;
    if (hidden % 8 || chunks > 256 * 8) return hipErrorInvalidValue;
    if (rows > 4 && rows <= wide_max_rows && chunks >= 512 && chunks <= 1024 && chunks % 64 == 0) *f = RmsnormForm{1, chunks <= 512 ? 512 : 1024};
    else *f = RmsnormForm{chunks <= 256 ? 1 : (chunks <= 512 ? 2 : (chunks <= 1024 ? 4 : 8)), 256};
    return hipSuccess;
}

// PPLHIP_RMSNORM_WIDE_MAX_ROWS=0: the 256-thread form (A/B runs); read once
int rmsnorm_wide_max_rows() {
    static const int wide_rows = getenv("PPLHIP_RMSNORM_WIDE_MAX_ROWS") ? atoi(getenv("PPLHIP_RMSNORM_WIDE_MAX_ROWS")) : 512;
    return wide_rows;
}

hipError_t launch_rmsnorm(hipStream_t s, const uint16_t* x, const uint16_t* skip, const uint16_t* w, float eps,
                          int64_t rows, int hidden, const int64_t* gather_seq_starts, uint16_t* out,
                          uint16_t* residual_out, int8_t* qout, float* sx, const SplitSlabs* skip_slabs, bool q_fp8) {
    RmsnormForm f;
    const hipError_t fe = rmsnorm_form(rows, hidden, rmsnorm_wide_max_rows(), &f);
    if (fe != hipSuccess || rows == 0) return fe;
    const int chunks = hidden / 8;
    SplitSlabs sl;
    if (skip_slabs && skip_slabs->splits > 0) {
        sl = *skip_slabs;
        if (sl.N != hidden) return hipErrorInvalidValue;
    }
    if (q_fp8 && !qout) return hipErrorInvalidValue;
    const dim3 g((unsigned)rows), b((unsigned)f.nt);
#define RMS_LAUNCH(MC, NT)                                                                                                          \
    do {                                                                                                                            \
        if (q_fp8) hipLaunchKernelGGL((rmsnorm_kernel<MC, NT, true>), g, b, 0, s, (const uint4*)x, (const uint4*)skip, (const uint4*)w, \
                                      eps, chunks, hidden, gather_seq_starts, (uint4*)out, (uint4*)residual_out, qout, sx, sl);    \
        else hipLaunchKernelGGL((rmsnorm_kernel<MC, NT>), g, b, 0, s, (const uint4*)x, (const uint4*)skip, (const uint4*)w, eps,    \
                                chunks, hidden, gather_seq_starts, (uint4*)out, (uint4*)residual_out, qout, sx, sl);               \
    } while (0)
    if (f.nt == 512) RMS_LAUNCH(1, 512);
    else if (f.nt == 1024) RMS_LAUNCH(1, 1024);
    else if (f.maxc == 1) RMS_LAUNCH(1, 256);
    else if (f.maxc == 2) RMS_LAUNCH(2, 256);
    else if (f.maxc == 4) RMS_LAUNCH(4, 256);
    else RMS_LAUNCH(8, 256);
#undef RMS_LAUNCH
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void silu_mul_kernel(const uint4* __restrict__ gu, int64_t total_chunks, int ichunks,
                                                       uint4* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total_chunks; i += (int64_t)gridDim.x * 256) {
        const int64_t t = i / ichunks;
        const int c = (int)(i - t * ichunks);
        float g[8], u[8], o[8];
        unpack8(gu[t * 2 * ichunks + c], g);
        unpack8(gu[t * 2 * ichunks + ichunks + c], u);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = g[j] / (1.0f + __expf(-g[j])) * u[j];
        out[i] = pack8(o);
    }
}

hipError_t launch_silu_mul(hipStream_t s, const uint16_t* gate_up, int64_t T, int inter, uint16_t* out) {
    if (T == 0) return hipSuccess;
    if (inter % 8) return hipErrorInvalidValue;
    const int64_t total = T * (inter / 8);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(silu_mul_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const uint4*)gate_up, total, inter / 8,
                       (uint4*)out);
    return hipGetLastError();
}

// Row interleave used for the fused SwiGLU GEMM: dst row r = src row (r even ? r/2 : rows/2 + r/2), i.e. the
// container's [gate rows | up rows] order becomes (gate_0, up_0, gate_1, up_1, ...) on the device.
template <typename U>
__global__ __launch_bounds__(256) void interleave_rows_kernel(const U* __restrict__ src, U* __restrict__ dst, int rows,
                                                              int64_t units_per_row) {
    const int64_t total = (int64_t)rows * units_per_row;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / units_per_row, c = i - r * units_per_row;
        const int64_t sr = (r & 1) ? (rows / 2 + (r >> 1)) : (r >> 1);
        dst[i] = src[sr * units_per_row + c];
    }
}

hipError_t launch_interleave_rows(hipStream_t s, const void* src, void* dst, int rows, int64_t row_bytes) {
    if (rows == 0 || row_bytes == 0) return hipSuccess;
    if ((rows & 1) || (row_bytes & 1)) return hipErrorInvalidValue;
    const bool wide = (row_bytes % 16) == 0;
    const int64_t units = wide ? row_bytes / 16 : row_bytes / 2;
    int64_t blocks = ((int64_t)rows * units + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if (wide)
        hipLaunchKernelGGL(interleave_rows_kernel<uint4>, dim3((unsigned)blocks), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, rows, units);
    else
        hipLaunchKernelGGL(interleave_rows_kernel<uint16_t>, dim3((unsigned)blocks), dim3(256), 0, s, (const uint16_t*)src, (uint16_t*)dst, rows, units);
    return hipGetLastError();
}

}  // namespace pplhip
