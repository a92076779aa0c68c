// ezrs_select.hip -- the device-side list of failed codewords (ezrs_select_failed, include/ezrs.h).
//
// An order-preserving compaction of { k : result[k] < 0 } in three kernels on the caller's stream:
//   k_select_count   a workgroup per chunk of 4096 results: how many are negative -> ws[chunk]
//   k_select_scan    one workgroup: exclusive scan of ws[] in place, the total -> *count
//   k_select_write   a workgroup per chunk: base + k of its negative results to sel[ws[chunk] ..],
//                    in ascending k, clamped to cap; the same workgroups fill sel[min(total, cap) ..
//                    cap) with EZRS_SEL_NONE
// The order between the phases comes from the kernel boundaries alone: no workgroup waits for
// another one (no ticket, no look-back), so nothing depends on which workgroups are resident.
//
// Lane map of both chunk kernels: wave w of the workgroup owns 1024 consecutive results, lane l
// takes result l of each of their 16 runs of 64, so every load is one coalesced run and one ballot
// per run ranks its lanes: ascending k is (wave, run, lane).  The result array is read twice (8
// bytes per codeword); nothing else scales with n.
#include "ezrs_internal.hpp"

namespace ezrs {
namespace sel {

constexpr unsigned kRuns = (unsigned)(kSelChunk / 256);   // runs of 64 results per wave
constexpr uint64_t kNone = ~(uint64_t)0;                  // EZRS_SEL_NONE

// The ballots of the 16 runs of this wave: bit l of m[r] = result of (wave, run r, lane l) is negative.
__device__ __forceinline__ unsigned wave_ballots(const int32_t *result, size_t n, size_t k0, unsigned lane,
                                                 uint64_t (&m)[kRuns]) {
    unsigned total = 0;
#pragma unroll
    for (unsigned r = 0; r < kRuns; ++r) {
        const size_t k = k0 + 64 * r + lane;
        m[r] = __ballot(k < n && result[k] < 0);
        total += (unsigned)__popcll(m[r]);
    }
    return total;
}

__global__ void __launch_bounds__(256) k_select_count(const int32_t *result, size_t n, uint64_t *ws) {
    __shared__ unsigned wsum[4];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t m[kRuns];
    const unsigned total = wave_ballots(result, n, (size_t)blockIdx.x * kSelChunk + 1024 * wave, lane, m);
    if (lane == 0) wsum[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) ws[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One workgroup of 256 over the chunk counts, 256 at a time with a running carry.  A count is at
// most 4096, so a strip's sums fit 32 bits; the carry is 64 bits.
__global__ void __launch_bounds__(256) k_select_scan(uint64_t *ws, size_t nchunks, uint64_t *count) {
    __shared__ unsigned wsum[4];
    const unsigned t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint64_t carry = 0;
    for (size_t c0 = 0; c0 < nchunks; c0 += 256) {
        const unsigned v = c0 + t < nchunks ? (unsigned)ws[c0 + t] : 0u;
        unsigned x = v;                             // inclusive scan over the wave
#pragma unroll
        for (unsigned d = 1; d < 64; d <<= 1) {
            const unsigned y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        unsigned before = 0, strip = 0;
#pragma unroll
        for (unsigned w = 0; w < 4; ++w) {
            if (w < wave) before += wsum[w];
            strip += wsum[w];
        }
        if (c0 + t < nchunks) ws[c0 + t] = carry + before + (x - v);
        carry += strip;
        __syncthreads();                            // wsum[] is written again
    }
    if (t == 0) *count = carry;
}

// grid: a workgroup per chunk of results and per 4096 entries of sel, whichever are more.
__global__ void __launch_bounds__(256) k_select_write(const int32_t *result, size_t n, size_t nchunks,
                                                      uint64_t base, const uint64_t *ws, const uint64_t *count,
                                                      uint64_t *sel, size_t cap) {
    __shared__ unsigned wsum[4];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t b = blockIdx.x;
    // the tail of the list: entries [min(total, cap), cap) of this workgroup's 4096
    const uint64_t total = *count;
    for (size_t i = b * kSelChunk + threadIdx.x; i < cap && i < (b + 1) * kSelChunk; i += 256)
        if (i >= total) sel[i] = kNone;
    if (b >= nchunks) return;                       // uniform over the workgroup
    const size_t k0 = b * kSelChunk + 1024 * wave;
    uint64_t m[kRuns];
    const unsigned mine = wave_ballots(result, n, k0, lane, m);
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    uint64_t at = ws[b];                            // where this wave's first entry goes
    for (unsigned w = 0; w < wave; ++w) at += wsum[w];
#pragma unroll
    for (unsigned r = 0; r < kRuns; ++r) {
        const unsigned below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m[r] >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)m[r], 0u));
        if (((m[r] >> lane) & 1) && at + below < cap) sel[at + below] = base + (k0 + 64 * r + lane);
        at += (unsigned)__popcll(m[r]);
    }
}

} // namespace sel

hipError_t launch_select_failed(const int32_t *result, size_t n, uint64_t base, uint64_t *sel, size_t cap,
                                uint64_t *count, void *ws, hipStream_t s) {
    const size_t nchunks = select_ws_bytes(n) / sizeof(uint64_t);
    const size_t fill = (cap + kSelChunk - 1) / kSelChunk, grid = nchunks > fill ? nchunks : fill;
    if (grid > 0x7FFFFFFFu) return hipErrorInvalidValue;
    uint64_t *w = static_cast<uint64_t *>(ws);
    if (nchunks) hipLaunchKernelGGL(sel::k_select_count, dim3((unsigned)nchunks), dim3(256), 0, s, result, n, w);
    hipLaunchKernelGGL(sel::k_select_scan, dim3(1), dim3(256), 0, s, w, nchunks, count);
    if (grid)
        hipLaunchKernelGGL(sel::k_select_write, dim3((unsigned)grid), dim3(256), 0, s, result, n, nchunks, base,
                           w, count, sel, cap);
    return hipGetLastError();
}

} // namespace ezrs
