// The allowed-token mask pass shared by k_logit_rules.hip and k_guide.hip: every token of `row` whose bit is clear in `mask` (token v is bit
// v & 31 of word v >> 5) is set to -inf; no logit is ever read.
//
// 16-byte path (vec: stride % 4 == 0 and a 16-byte aligned logits base, the convention of the sampler kernels): a lane owns the four
// consecutive tokens of piece c = 4c .. 4c + 3, whose bits are one nibble of mask word c >> 3, so a word serves eight lanes.  Nibble 0xf:
// nothing at all.  Nibble 0: one 16-byte store of -inf.  Mixed: a 4-byte store per cleared bit.  The V % 4 tokens behind the last whole
// piece, and every token of a row off the 16-byte path, go element by element.  No float at or behind `vocab` is ever addressed, whatever
// the tail word's high bits say: the loops stop at vocab.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pplhip {

template <int THREADS>
__device__ __forceinline__ void mask_row_ninf(float* row, const uint32_t* __restrict__ mask, int vocab, bool vec, int tid) {
    const float ninf = -INFINITY;
    const int nv = vec ? vocab >> 2 : 0;
    for (int c = tid; c < nv; c += THREADS) {
        const uint32_t nib = (mask[c >> 3] >> ((c & 7) * 4)) & 15u;
        if (nib == 15u) continue;
        if (nib == 0u) {
            reinterpret_cast<float4*>(row)[c] = make_float4(ninf, ninf, ninf, ninf);
        } else {
            float* p = row + c * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!((nib >> j) & 1u)) p[j] = ninf;
        }
    }
    for (int v = nv * 4 + tid; v < vocab; v += THREADS)
        if (!((mask[v >> 5] >> (v & 31)) & 1u)) row[v] = ninf;
}

}  // namespace pplhip
