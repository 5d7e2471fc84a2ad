// Tile sizes and LDS byte formulas of the weight-only linear kernels (k_gemm*.hip, k_gemv.hip), each written once: the kernels size their
// LDS from them and the launch plan (linear_plan.h) its grids.  Plain constexpr values -- no HIP header, so the plan builds with the host
// compiler alone.
#pragma once

namespace pplhip {

// Epilogues (store4, k_gemm_dev.h): fp16 output, fp32 output (logits), fused SwiGLU
enum { EPI_F16 = 0, EPI_F32 = 1, EPI_SWIGLU = 2 };
inline const char* epi_name(int epi) { return epi == EPI_F32 ? "f32" : (epi == EPI_SWIGLU ? "swiglu" : "f16"); }

// generic and ring kernels (gemm_kernel, gemm_dma_kernel): block tile 128 (n) x 128 (m) x 64 (k)
constexpr int G_BN = 128, G_BM = 128, G_BK = 64;
constexpr int W4_MAXG = 64;  // W4: quantisation groups (of 128 along K) whose scales one block keeps in LDS
// LDS bytes gemm_dma_body needs (static: at most 56 KiB).  MAXG (W4): W4_MAXG, or 16 for launches whose K slabs span at most 32 tiles
// (44 instead of 56 KiB with two stages: three blocks per CU instead of two)
constexpr int gemm_dma_lds_bytes(int wq, int stages, int bm = G_BM, int maxg = W4_MAXG) {
    return stages * (bm * G_BK * 2 + G_BN * G_BK * (wq == 8 ? 2 : (wq == 4 ? 1 : 4)) / 2) + (wq == 4 ? maxg * G_BN * 2 : 0);
}

// half-height 128-deep kernel (gemm_w8_half128_kernel)
constexpr int S_KS = 2;                                        // 64-deep sub-tiles per stage
constexpr int S_WB = G_BN * G_BK * S_KS;                       // weight bytes per stage: 16 KiB
constexpr int s_xb(int bm) { return S_KS * bm * G_BK * 2; }    // activation bytes per stage: 4 / 8 / 16 KiB
constexpr int half128_lds_bytes(int st, int bm) { return st * (s_xb(bm) + S_WB); }

// 256 x 256 kernel (gemm_w8_dma256_kernel): 3-stage ring of X 32 KiB + W 16 KiB
constexpr int H_BN = 256, H_BM = 256, H_ST = 3;
constexpr int H_LDS = H_ST * (H_BM * G_BK * 2 + H_BN * G_BK);

// 128 (m) x 32 NC (n) kernel (gemm_w8_wide_kernel): NC consumer waves + WD_NP producers, WD_ST stages
constexpr int WD_BM = 128, WD_NP = 4, WD_ST = 3;
constexpr int WD_XB = WD_BM * G_BK * 2;   // activation bytes per stage: 16 KiB
constexpr int wide_lds_bytes(int st, int nc) { return st * (WD_XB + 32 * nc * G_BK); }

// W4 producer / consumer kernel (gemm_w4_pc_kernel): 128 (m) x 64 (n) tiles, 4 ring slots of a 128-deep super-tile
constexpr int PC_BM = 128, PC_BN = 64;
constexpr int PC_XT = PC_BM * 64 * 2;   // one 64-deep activation tile: 16 KiB
constexpr int PC_XB = 2 * PC_XT;        // activation bytes per super-tile: 32 KiB
constexpr int PC_NS = 4;                // ring slots (activations, raw weights, scales), super-tiles
constexpr int PC_RAWB = PC_BN * 64;     // raw int4 bytes per super-tile: 4 KiB (1 KiB per producer wave)
constexpr int PC_SCB = 1024;            // scale slot: one dword per producer lane
constexpr int PC_LDS = PC_NS * (PC_XB + PC_RAWB + PC_SCB);

// streaming GEMV (gemv_stream_kernel): most waves per block, most weight rows per wave, rows in flight per wave
constexpr int GV_NW = 8, GV_RB = 16, GV_U = 8;

// quantised-activation kernels (k_gemm_i8.hip; int8 and fp8 alike): block tile 128 (n) x 128 (m) x 128 (k) of one-byte codes, ring stages of
// X 16 KiB + W 16 KiB (gemm_i8_pc_kernel); the 128 x 384 blocks (gemm_i8_wide_kernel): twelve consumer + four producer waves, two stages of
// X 16 KiB + W 48 KiB; the 256 x 256 x 64 blocks (gemm_i8_256_kernel, int8 only): stages of X 16 KiB + W 16 KiB; the skinny kernel
// (gemv_i8_kernel): 16 weight rows per block, 16-row activation tiles
constexpr int I_BN = 128, I_BM = 128, I_BK = 128;
constexpr int IW_BN = 384, IW_NC = 12, IW_NP = 4, IW_ST = 2;
constexpr int IW_XB = I_BM * I_BK, IW_WB = IW_BN * I_BK;       // 16 KiB + 48 KiB per stage
constexpr int I2_BN = 256, I2_BM = 256, I2_BK = 64;
constexpr int IV_BN = 16, IV_BM = 16;
constexpr int i8_pc_lds_bytes(int st) { return st * 2 * I_BM * I_BK; }
constexpr int i8_wide_lds_bytes() { return IW_ST * (IW_XB + IW_WB); }
constexpr int i8_256_lds_bytes(int st) { return st * 2 * I2_BM * I2_BK; }
// static LDS of the skinny kernel: the partial accumulators of its NW - 1 other K slices, MT row tiles of 64 lanes x 16 bytes
constexpr int i8_gemv_lds_bytes(int mt, int nw) { return (nw - 1) * mt * 64 * 16; }

constexpr int LDS_PER_CU = 160 * 1024;
static_assert(H_LDS <= LDS_PER_CU && PC_LDS <= LDS_PER_CU && wide_lds_bytes(WD_ST, 12) <= LDS_PER_CU, "one block per CU");

}  // namespace pplhip
