// Guided decoding (DESIGN.md "numerics", guided decoding row): the output of a request is held inside the language of a byte-level DFA.
// Two kernels.
//
// guide_build_kernel, once per pattern: mask[s][t] = "token t may follow in state s", one bit per token (token t is bit t & 31 of word
// t >> 5 of row s), for every live state s of the automaton:
//   an end token          accept[s], whatever its bytes
//   a zero-length token   0 (also every id at or behind n_tok)
//   any other token       1 iff walking its bytes from s through trans[state][byte] never meets the dead state GUIDE_DEAD
// One workgroup owns GB_THREADS consecutive tokens, one per lane, and loops over the states; the whole transition table sits in static
// LDS (255 x 256 bytes = 65,280 of the 65,536 a workgroup may declare statically), copied once.  A lane leaves its walk at the first dead
// transition, so the dead state's row -- the table has none -- is never indexed.  The 64 verdicts of a wave become two mask words by
// __ballot, stored by lane 0; a token id covers exactly one lane of one workgroup, so no word has two writers.  Bits at or behind `vocab`
// are 0: those lanes vote 0.  Words at or behind ceil(vocab / 32) are not stored.  any[s] collects "some token is allowed in s" by a vector
// atomic OR, one per wave that has a set bit.
//
// guide_build16_kernel, once per wide guide (a JSON schema's automaton; up to GUIDE16_MAX_STATES live states): the same definition on
// trans uint16 [S, 256] with the dead state GUIDE16_DEAD.  The table (up to 2 MiB) is read from global memory, where it stays in L2; the
// grid is (token block, state chunk): workgroup (x, y) owns GB_THREADS consecutive tokens, one per lane, and the GUIDE16_STATE_CHUNK
// states behind y * GUIDE16_STATE_CHUNK, so the cap at a 128 K vocabulary is some 128,000 waves and no lane walks more than a chunk's
// states.  A lane keeps its token's first eight bytes in registers; for four states at a time it first reads the four independent
// trans[s][byte 0] -- most (state, token) pairs die right there -- and only then walks what is left.  Every next state at or behind
// n_states counts as dead, so no row outside the table is ever read.  A (row, word) pair has one writer: the wave of the block that
// owns the row's chunk and the word's tokens.  any[s] is ORed by a vector atomic only while it still reads 0.
//
// guide_mask_kernel, every step: one workgroup per ASKING row (host-compacted list, as k_logit_rules.hip); row b gets -inf wherever row
// states[b] of slot guide_slots[b]'s mask has a clear bit.  The pass is mask_row_ninf of k_mask_dev.h, the logit rules' own.
#include "k_mask_dev.h"
#include "kernels.h"

namespace pplhip {

constexpr int GB_THREADS = 256;
constexpr int GM_THREADS = 256;

__global__ __launch_bounds__(GB_THREADS) void guide_build_kernel(const uint8_t* __restrict__ trans, const uint8_t* __restrict__ accept,
                                                                 int n_states, const uint8_t* __restrict__ tok_bytes,
                                                                 const int64_t* __restrict__ tok_off, int n_tok,
                                                                 const int32_t* __restrict__ end_tokens, int n_end, int vocab,
                                                                 uint32_t* __restrict__ mask, int64_t mask_stride, uint32_t* any) {
    __shared__ __attribute__((aligned(16))) uint8_t tab[GUIDE_MAX_STATES * 256];
    const int tid = threadIdx.x;
    n_states = min(n_states, GUIDE_MAX_STATES);
    if ((reinterpret_cast<uintptr_t>(trans) & 15) == 0) {
        const uint4* src = reinterpret_cast<const uint4*>(trans);
        uint4* dst = reinterpret_cast<uint4*>(tab);
        for (int i = tid; i < n_states * 16; i += GB_THREADS) dst[i] = src[i];
    } else {
        for (int i = tid; i < n_states * 256; i += GB_THREADS) tab[i] = trans[i];
    }
    const int t = blockIdx.x * GB_THREADS + tid;
    const bool in_vocab = t < vocab;
    bool is_end = false;
    for (int i = 0; i < n_end; ++i) is_end = is_end || end_tokens[i] == t;
    int64_t begin = 0;
    int len = 0;
    if (in_vocab && t < n_tok && !is_end) {
        begin = tok_off[t];
        len = (int)(tok_off[t + 1] - begin);
    }
    const uint8_t* __restrict__ bytes = tok_bytes + begin;
    __syncthreads();

    const int lane = tid & 63;
    const int word = (blockIdx.x * GB_THREADS + (tid & ~63)) >> 5;   // the wave's first mask word
    const int words = (vocab + 31) >> 5;
    for (int s = 0; s < n_states; ++s) {
        bool ok;
        if (is_end) {
            ok = in_vocab && accept[s] != 0;
        } else {
            int cur = s;
            int i = 0;
            for (; i < len; ++i) {
                cur = tab[cur * 256 + bytes[i]];
                if (cur >= GUIDE_MAX_STATES) break;   // the dead state: it has no row
            }
            ok = len > 0 && i == len;
        }
        const unsigned long long votes = __ballot(ok);
        if (lane == 0) {
            uint32_t* row = mask + (int64_t)s * mask_stride;
            if (word < words) row[word] = (uint32_t)votes;
            if (word + 1 < words) row[word + 1] = (uint32_t)(votes >> 32);
            if (votes) atomicOr(&any[s], 1u);
        }
    }
}

__global__ __launch_bounds__(GB_THREADS) void guide_build16_kernel(const uint16_t* __restrict__ trans, const uint8_t* __restrict__ accept,
                                                                   int n_states, const uint8_t* __restrict__ tok_bytes,
                                                                   const int64_t* __restrict__ tok_off, int n_tok,
                                                                   const int32_t* __restrict__ end_tokens, int n_end, int vocab,
                                                                   uint32_t* __restrict__ mask, int64_t mask_stride, uint32_t* any) {
    constexpr int G = 4;   // states in flight per lane
    static_assert(GUIDE16_STATE_CHUNK % G == 0, "a chunk is whole groups");
    const int tid = threadIdx.x;
    const int t = blockIdx.x * GB_THREADS + tid;
    const bool in_vocab = t < vocab;
    bool is_end = false;
    for (int i = 0; i < n_end; ++i) is_end = is_end || end_tokens[i] == t;
    int64_t begin = 0;
    int len = 0;
    if (in_vocab && t < n_tok && !is_end) {
        begin = tok_off[t];
        len = (int)(tok_off[t + 1] - begin);
    }
    const uint8_t* __restrict__ bytes = tok_bytes + begin;
    uint64_t head = 0;   // bytes 0 .. 7 of the token, byte i at bits 8 i
    for (int i = 0; i < min(len, 8); ++i) head |= (uint64_t)bytes[i] << (8 * i);
    const int b0 = (int)(head & 255);

    const int lane = tid & 63;
    const int word = (blockIdx.x * GB_THREADS + (tid & ~63)) >> 5;   // the wave's first mask word
    const int words = (vocab + 31) >> 5;
    const int s_begin = blockIdx.y * GUIDE16_STATE_CHUNK;
    const int s_end = min(n_states, s_begin + GUIDE16_STATE_CHUNK);
    for (int s0 = s_begin; s0 < s_end; s0 += G) {
        int cur[G];
#pragma unroll
        for (int k = 0; k < G; ++k) {
            const int s = min(s0 + k, s_end - 1);   // (a group's states behind the chunk's end repeat its last one and store nothing)
            cur[k] = len > 0 ? (int)trans[(int64_t)s * 256 + b0] : n_states;
        }
#pragma unroll
        for (int k = 0; k < G; ++k) {
            const int s = s0 + k;
            if (s >= s_end) break;   // (uniform over the block)
            bool ok;
            if (is_end) {
                ok = in_vocab && accept[s] != 0;
            } else {
                int c = cur[k];
                int i = 1;
                for (; i < len && c < n_states; ++i) {
                    const int b = i < 8 ? (int)((head >> (8 * i)) & 255) : (int)bytes[i];
                    c = trans[(int64_t)c * 256 + b];
                }
                ok = c < n_states;   // the dead state, and anything else that has no row, ends the walk
            }
            const unsigned long long votes = __ballot(ok);
            if (lane == 0) {
                uint32_t* row = mask + (int64_t)s * mask_stride;
                if (word < words) row[word] = (uint32_t)votes;
                if (word + 1 < words) row[word + 1] = (uint32_t)(votes >> 32);
                if (votes && __hip_atomic_load(&any[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(&any[s], 1u);
            }
        }
    }
}

__global__ __launch_bounds__(GM_THREADS) void guide_mask_kernel(float* logits, int stride, int vocab, const int32_t* __restrict__ rows,
                                                                const int32_t* __restrict__ guide_slots, const int32_t* __restrict__ states,
                                                                GuideTable tb) {
    const int b = rows[blockIdx.x];
    const int slot = guide_slots[b];
    if (slot < 0 || slot >= GUIDE_MAX_SLOTS) return;   // (uniform over the block; the host lists asking rows only)
    const uint32_t* __restrict__ mask = tb.mask[slot] + (int64_t)states[b] * tb.mask_stride;
    const bool vec = (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    mask_row_ninf<GM_THREADS>(logits + (int64_t)b * stride, mask, vocab, vec, threadIdx.x);
}

hipError_t launch_guide_build(hipStream_t s, const uint8_t* trans, const uint8_t* accept, int n_states, const uint8_t* tok_bytes,
                              const int64_t* tok_off, int n_tok, const int32_t* end_tokens, int n_end, int vocab, uint32_t* mask,
                              int64_t mask_stride, uint32_t* any) {
    if (n_states <= 0 || vocab <= 0) return hipSuccess;
    const int blocks = (vocab + GB_THREADS - 1) / GB_THREADS;
    hipLaunchKernelGGL(guide_build_kernel, dim3(blocks), dim3(GB_THREADS), 0, s, trans, accept, n_states, tok_bytes, tok_off, n_tok, end_tokens,
                       n_end, vocab, mask, mask_stride, any);
    return hipGetLastError();
}

hipError_t launch_guide_build16(hipStream_t s, const uint16_t* trans, const uint8_t* accept, int n_states, const uint8_t* tok_bytes,
                                const int64_t* tok_off, int n_tok, const int32_t* end_tokens, int n_end, int vocab, uint32_t* mask,
                                int64_t mask_stride, uint32_t* any) {
    if (n_states <= 0 || vocab <= 0) return hipSuccess;
    if (n_states > GUIDE16_MAX_STATES) return hipErrorInvalidValue;
    const dim3 grid((vocab + GB_THREADS - 1) / GB_THREADS, (n_states + GUIDE16_STATE_CHUNK - 1) / GUIDE16_STATE_CHUNK);
    hipLaunchKernelGGL(guide_build16_kernel, grid, dim3(GB_THREADS), 0, s, trans, accept, n_states, tok_bytes, tok_off, n_tok, end_tokens,
                       n_end, vocab, mask, mask_stride, any);
    return hipGetLastError();
}

hipError_t launch_guide_mask(hipStream_t s, float* logits, int stride, int vocab, const int32_t* rows, int n_rows, const int32_t* guide_slots,
                             const int32_t* states, const GuideTable& table) {
    if (n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(guide_mask_kernel, dim3(n_rows), dim3(GM_THREADS), 0, s, logits, stride, vocab, rows, guide_slots, states, table);
    return hipGetLastError();
}

}  // namespace pplhip
