// Logit rules (DESIGN.md "numerics", logit rules row): per-request bias, allowed-token mask and suppressed stop tokens, applied in place to
// the fp32 logits in front of the penalty step.  One workgroup per ASKING row, through a host-compacted row list as k_logprobs.hip and
// k_sample_rows.hip have it; a row with flags 0 is in no list and is never touched, an empty list is no launch.  The rule of a row is the
// record of its batch SLOT (slots[b]), not of its row.
//
//   y = -inf              if bit 0 and the rule has a mask and v's bit is clear
//     = -inf              else if bit 1 and v is one of the stops
//     = fp32(x + bias)    else if bit 0 and v has a bias          (a ban is the bias -inf)
//     = x, bit for bit    otherwise
//
// ORDERING.  Three passes, separated by workgroup barriers that also order the global stores (__syncthreads: release / acquire fences at
// workgroup scope around s_barrier, so a pass's stores are visible to the loads of the next one; one workgroup owns the whole row):
//   1. mask   only stores -inf, never reads a logit
//   2. stops  only stores -inf
//   3. bias   reads x as passes 1 and 2 left it and stores x + bias: a masked or suppressed token is -inf already and -inf + bias stays
//             -inf for every value validation lets through (finite or -inf), so "the mask wins" and "the stop wins" need no look-up
// Bias tokens are unique (validated on the host), so pass 3 has no two writers of one element; two equal stops both store -inf.
//
// Mask pass (mask_row_ninf of k_mask_dev.h, shared with k_guide.hip), 16-byte path (stride % 4 == 0 and a 16-byte aligned base: the `vec`
// convention of the sampler kernels): a lane owns the four
// consecutive tokens of piece c = 4c .. 4c + 3, whose bits are one nibble of mask word c >> 3, so a word serves eight lanes.  Nibble 0xf:
// nothing at all.  Nibble 0: one 16-byte store of -inf.  Mixed: a 4-byte store per cleared bit.  The V % 4 tokens behind the last whole
// piece, and every token of a row off the 16-byte path, go element by element.  No float at or behind V is ever addressed, whatever the
// tail word's high bits say: the loops stop at V, and bias / stop tokens outside [0, V) are skipped.
#include "k_mask_dev.h"
#include "kernels.h"

namespace pplhip {

constexpr int LR_THREADS = 256;

__global__ __launch_bounds__(LR_THREADS) void logit_edit_kernel(float* logits, int stride, int vocab,
                                                                const int32_t* __restrict__ rows, const int32_t* __restrict__ slots,
                                                                const uint32_t* __restrict__ flags, LogitRuleTable tb) {
    const int b = rows[blockIdx.x];
    const uint32_t f = flags[b];
    if (f == 0) return;   // (uniform over the block; the host lists asking rows only)
    const int64_t slot = slots[b];
    const int tid = threadIdx.x;
    float* row = logits + (int64_t)b * stride;
    const int32_t* head = tb.head + slot * tb.head_stride;
    const bool edit = (f & 1u) != 0;
    const int n_bias = edit ? min(max(head[0], 0), LOGIT_BIAS_MAX) : 0;
    const int n_stop = (f & 2u) ? min(max(head[1], 0), LOGIT_STOP_MAX) : 0;
    const float ninf = -INFINITY;

    if (edit && head[2]) {
        const uint32_t* __restrict__ mask = tb.mask + slot * tb.mask_stride;
        const bool vec = (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
        mask_row_ninf<LR_THREADS>(row, mask, vocab, vec, tid);
    }
    __syncthreads();
    if (tid < n_stop) {
        const int32_t v = (tb.stops + slot * tb.stop_stride)[tid];
        if ((uint32_t)v < (uint32_t)vocab) row[v] = ninf;
    }
    __syncthreads();
    const int32_t* __restrict__ bt = tb.bias_tok + slot * tb.bias_stride;
    const float* __restrict__ bv = tb.bias_val + slot * tb.bias_stride;
    for (int i = tid; i < n_bias; i += LR_THREADS) {
        const int32_t v = bt[i];
        if ((uint32_t)v < (uint32_t)vocab) row[v] = row[v] + bv[i];
    }
}

hipError_t launch_logit_edit(hipStream_t s, float* logits, int stride, int vocab, const int32_t* rows, int n_rows, const int32_t* slots,
                             const uint32_t* flags, const LogitRuleTable& table) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(logit_edit_kernel, dim3(n_rows), dim3(LR_THREADS), 0, s, logits, stride, vocab, rows, slots, flags, table);
    return hipGetLastError();
}

}  // namespace pplhip
