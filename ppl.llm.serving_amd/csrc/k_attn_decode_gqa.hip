// K8, grouped-query variant: the launch of attn_decode_gqa_kernel.  The kernel, its design notes and its build switches:
// k_attn_decode_gqa_dev.h.
#include "k_attn_decode_gqa_dev.h"

namespace pplhip {

bool attn_decode_gqa_supported(int kv_fmt, int H, int Hkv, int D) {
    if (Hkv <= 0 || H % Hkv) return false;
    const int grp = H / Hkv;
    if (grp < 4 || grp > 16) return false;
    if (kv_fmt == KV_I8G8 || kv_fmt == KV_FP8) return D == 128 || D == 64;  // a row must hold >= four 16-byte pieces
    if (kv_fmt == KV_I4G32) return D == 128;   // (64 bytes; head_dim 64 and 32 run on the multi-head kernel)
    return kv_fmt == KV_FP16 && (D == 128 || D == 64 || D == 32);
}

hipError_t launch_attn_decode_gqa(hipStream_t s, const uint16_t* qkv, const KvAddr& kv, int kv_fmt,
                                  const int64_t* seq_starts, const int64_t* start_pos, const int64_t* cache_indices,
                                  int64_t max_pages, int64_t nb, int H, int Hkv, int D, int split, float* workspace,
                                  uint16_t* out, hipEvent_t t0, hipEvent_t t1) {
    if (nb == 0) return hipSuccess;
    if (!attn_decode_gqa_supported(kv_fmt, H, Hkv, D)) return hipErrorInvalidValue;
    dim3 grid((unsigned)Hkv, (unsigned)nb, (unsigned)split);
    static const int small_min = getenv("PPLHIP_GQA_SMALL_BLOCK_MIN") ? atoi(getenv("PPLHIP_GQA_SMALL_BLOCK_MIN")) : GQ_SMALL_BLOCK_MIN;   // A/B runs
    const bool small = (int64_t)Hkv * nb * split >= small_min;
    hipError_t unbuilt = hipSuccess;   // a (format, head_dim) the supported set admits but no kernel is built for: an error, never a no-op
    dispatch_int<KV_I8G8, KV_FP16, KV_FP8, KV_I4G32>(kv_fmt, [&](auto QB) {
        dispatch_int<128, 64, 32>(D, [&](auto DD) {
            if constexpr (QB == KV_I4G32 ? DD == 128 : (QB == KV_FP16 || DD != 32)) {
                dispatch_int<0, 1>(kv.mode, [&](auto MD) {
                    dispatch_int<GQ_WAVES_SMALL, GQ_WAVES_BIG>(small ? GQ_WAVES_SMALL : GQ_WAVES_BIG, [&](auto NW) {
                        const auto kernel = attn_decode_gqa_kernel<QB, DD, MD, NW>;
                        constexpr int lds = gq_lds_bytes<QB, DD, NW>();
                        if constexpr (lds > 65536) {   // two sub-tiles' exact V images per wave; once per (instantiation, device)
                            static std::mutex mu;      // (host threads may launch the same instantiation for the first time together)
                            static LdsOptIn once;
                            std::lock_guard<std::mutex> g(mu);
                            if (once.first()) set_max_lds(lds, kernel);
                        }
                        if (t0 && t1)
                            hipExtLaunchKernelGGL(kernel, grid, dim3(NW * 64), lds, s, t0, t1, 0, qkv, kv, seq_starts, start_pos, cache_indices,
                                                  max_pages, H, Hkv, split, workspace, out);
                        else
                            hipLaunchKernelGGL(kernel, grid, dim3(NW * 64), lds, s, qkv, kv, seq_starts, start_pos, cache_indices, max_pages, H,
                                               Hkv, split, workspace, out);
                    });
                });
            } else {
                unbuilt = hipErrorInvalidValue;   // int8 / fp8 with head_dim 32, int4 below 128: a row holds fewer than four 16-byte pieces
            }
        });
    });
    return unbuilt != hipSuccess ? unbuilt : hipGetLastError();
}

}  // namespace pplhip
