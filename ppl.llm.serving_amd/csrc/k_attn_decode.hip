// K8 MultiHeadCacheAttention, decode phase: one query row per (request, head) against kv_len cached keys/values.
// THE roofline kernel of the hot path: ~1-3 flop/byte, bound by HBM bandwidth.
//
// Layout of the work (wave64, gfx950):
//   grid  = (H, nb, split)      one workgroup per (query head, request[, K-split])
//   block = NW waves            each wave owns an interleaved set of token groups
//   a KV row (D channels) is covered by LPT = D*elt/16 lanes with ONE 16-byte load each (coalesced:
//   consecutive lanes read consecutive 16-B pieces, consecutive token rows are adjacent in layout 3 / inside
//   a page), so a wave-instruction fetches TPW = 64/LPT complete rows (1 KiB).  UNROLL token groups are in
//   flight per wave before the first use (>= 8 x 16 B loads per lane outstanding: K, V, and the scales).
//   Every lane keeps q (its channels), a private online-softmax state (m, l) shared by the LPT lanes of its
//   token group, and fp32 accumulators for its channels; the TPW token groups of a wave and the NW waves of
//   a block are merged once at the end (log-sum-exp merge through shuffles, then LDS).
//   int8 KV: bytes are biased to unsigned (x ^ 0x80), converted with v_cvt_f32_ubyteN and the -128 bias is
//   folded out algebraically (sum(q) and sum(p*scale) corrections) -- the per-group fp16 scale multiplies the
//   8-channel partial dot product, not each element.
//   fp8 KV (KV_FP8): e4m3 bytes -> fp32 exactly (v_cvt_pk_f32_fp8); the row's power-of-two scale multiplies K's score and V's
//   probability -- both exact in fp32, so the kernel computes attention over the exactly dequantised rows.
//   int4 KV (KV_I4G32): a lane's 16-byte piece is one quant group of 32 channels (q and acc of 32 floats; 16 / 32 / 64 rows per wave-load at
//   head_dim 128 / 64 / 32).  The nibbles of a word are masked into bytes (even and odd channels) and converted with v_cvt_f32_ubyteN; the
//   + 8 is folded out like int8's 128 (8 sum(q) per group for the score, 8 sum(p s) for V); the group's scale multiplies the lane's
//   partial dot product and the probability.  (A whole piece per lane rather than an 8-byte half: one scale and one correction per lane, and
//   16-byte loads -- 128 bytes per lane in flight -- as in every other format.  The price is registers: q, acc, four K / V pieces and their
//   addresses fill the 128 VGPRs of four waves per SIMD; empty asm statements (k_attn_decode_dev.h) keep the scheduler from converting all
//   four keys' nibbles ahead of their use (~250 VGPRs otherwise), 11-16 dwords still go to scratch.  Build variants with room for 168 and 243
//   VGPRs (three and two waves per SIMD, no or less scratch) were slower at 7B, batch 1024: 805 and 822 us against 779 us per launch
//   (measured before the nibbles' byte form was pinned, which took the launch to 638 us).
//   The kernel is bound by its instruction count, not by HBM: DESIGN.md "numerics", profiles/kv_i4_step.jsonl.)
// Numerics: fp32 everywhere, output rounded to fp16 once.  Oracle: ref_attention (oracle/llama_ref.c).
#include <stdlib.h>
#include <hip/hip_ext.h>
#include "k_attn_decode_dev.h"

namespace pplhip {

template <int QBIT, int D>
__global__ void attn_decode_kernel(const uint16_t* __restrict__ qkv, KvAddr kv, const int64_t* __restrict__ seq_starts,
                                   const int64_t* __restrict__ start_pos, const int64_t* __restrict__ cache_indices,
                                   int64_t max_pages, int H, int Hkv, int split, float* __restrict__ workspace,
                                   uint16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [NW][D + 2]
    attn_decode_body<QBIT, D>(qkv, kv, seq_starts, start_pos, cache_indices, max_pages, H, Hkv, split, workspace, out, (int)blockIdx.x,
                              (int64_t)blockIdx.y, (int)blockIdx.z, (int)(blockDim.x >> 6), smem);
}

// split reduce: one block per (row, head) of the workspace ([row][head][split][D + 2] floats), one thread per channel
template <int D>
__global__ void attn_decode_reduce_kernel(const float* __restrict__ workspace, int split, uint16_t* __restrict__ out) {
    const int64_t bh = blockIdx.x;
    const float* ws = workspace + bh * (int64_t)split * (D + 2);
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        const LseRow r = lse_merge(ws, split, D + 2, D, d);
        out[bh * D + d] = f2h(r.o / r.l);
    }
}

hipError_t launch_attn_reduce(hipStream_t s, const float* ws, int nsplit, int64_t n_row_heads, int D, uint16_t* out) {
    if (D != 128 && D != 64 && D != 32) return hipErrorInvalidValue;
    dispatch_int<128, 64, 32>(D, [&](auto DD) {
        hipLaunchKernelGGL((attn_decode_reduce_kernel<DD>), dim3((unsigned)n_row_heads), dim3(DD < 64 ? 64 : DD), 0, s, ws, nsplit, out);
    });
    return hipGetLastError();
}

size_t attn_decode_workspace_bytes(int64_t nb, int H, int D, int split) {
    return split > 1 ? (size_t)nb * H * split * (D + 2) * sizeof(float) : 0;
}

template <int QBIT, int D>
static hipError_t launch_decode_t(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, const int64_t* seq_starts,
                                  const int64_t* start_pos, const int64_t* cache_indices, int64_t max_pages, int64_t nb,
                                  int H, int Hkv, int split, int threads, float* workspace, uint16_t* out, hipEvent_t t0,
                                  hipEvent_t t1) {
    const int nw = threads / 64;
    const size_t lds = (size_t)nw * (D + 2) * sizeof(float);
    // t0 / t1: start and stop timestamps taken from the kernel's own dispatch packet -- no extra barrier packets on the stream
    // (an hipEventRecord pair around the launch costs ~10 us of GPU time)
    if (t0 && t1)
        hipExtLaunchKernelGGL((attn_decode_kernel<QBIT, D>), dim3(H, (unsigned)nb, split), dim3(threads), lds, s, t0, t1, 0, qkv, kv,
                              seq_starts, start_pos, cache_indices, max_pages, H, Hkv, split, workspace, out);
    else
        hipLaunchKernelGGL((attn_decode_kernel<QBIT, D>), dim3(H, (unsigned)nb, split), dim3(threads), lds, s, qkv, kv,
                           seq_starts, start_pos, cache_indices, max_pages, H, Hkv, split, workspace, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || split == 1) return e;
    return launch_attn_reduce(s, workspace, split, nb * H, D, out);
}

hipError_t launch_attn_decode(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt,
                              const int64_t* seq_starts, const int64_t* start_pos, const int64_t* cache_indices,
                              int64_t max_pages, int64_t nb, int H, int Hkv, int D, int64_t max_kv_len, int split,
                              int threads, float* workspace, uint16_t* out, hipEvent_t t0, hipEvent_t t1) {
    if (nb == 0) return hipSuccess;
    static const int forced_tpb = tune_int("PPLHIP_ATTN_TPB", 0);  // tuning only
    if (forced_tpb) threads = forced_tpb;
    if (threads < 64 || threads > 64 * DEC_MAX_WAVES || threads % 64) return hipErrorInvalidValue;
    if (threads < D) threads = D;  // the final merge uses one thread per channel
    if (split < 1) split = 1;
    // grouped-query models: the MFMA kernel (k_attn_decode_gqa.hip) reads each KV row once for the whole head group
    static const bool no_gqa = tune_set("PPLHIP_ATTN_NOGQA");
    if (attn_decode_gqa_supported(kv_fmt, H, Hkv, D) && !no_gqa) {
        hipError_t e = launch_attn_decode_gqa(s, qkv, kv, kv_fmt, seq_starts, start_pos, cache_indices, max_pages, nb, H,
                                              Hkv, D, split, workspace, out, t0, t1);
        if (e != hipSuccess || split == 1) return e;
        return launch_attn_reduce(s, workspace, split, nb * H, D, out);
    }
    if ((kv_fmt != KV_FP16 && kv_fmt != KV_I8G8 && kv_fmt != KV_FP8 && kv_fmt != KV_I4G32) || (D != 128 && D != 64 && D != 32)) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    dispatch_int<KV_I8G8, KV_FP16, KV_FP8, KV_I4G32>(kv_fmt, [&](auto QB) {
        dispatch_int<128, 64, 32>(D, [&](auto DD) {
            e = launch_decode_t<QB, DD>(s, qkv, kv, seq_starts, start_pos, cache_indices, max_pages, nb, H, Hkv, split, threads, workspace,
                                        out, t0, t1);
        });
    });
    return e;
}

}  // namespace pplhip
