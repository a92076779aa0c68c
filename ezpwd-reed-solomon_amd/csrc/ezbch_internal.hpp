// ezbch_internal.hpp -- shared declarations of the MI355X BCH engine (not part of the C ABI):
// what the host ABI (ezbch.hip) hands to the kernels' launchers (ezbch_lane.hip, ezbch_wave.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace ezbch {

constexpr int kBigT = 64;                    // runtime-t decode (k_bch_decode_big<NW>)
constexpr int kMaxNW = 16;                   // 64-bit words of the widest remainder
constexpr int kMaxM = 15;
constexpr int kThreads = 256;
constexpr int kEBADMSG = 74, kEINVAL = 22;   // Linux errno values, negated as decode_bch returns them

struct DevBch {
    int m, n, t, ecc_bits, ecc_bytes;
    int lds_tabs;             // exp/log tables staged in LDS (m <= 12)
    int nw;                   // 64-bit words of the remainder (1 .. 16; the wave path: 64 nwl)
    int nwl;                  // wave path (t > 64 or ecc_bits > 1024): remainder words per lane, else 0
    uint64_t emask[kMaxNW];   // the ecc_bits significant bits of a left-justified remainder
    const uint64_t *step;     // [256][nw] byte-step remainder table
    const uint16_t *ex;       // [2n] alpha^i
    const uint16_t *lg;       // [n+1] log_alpha (lg[0] unused)
    const uint64_t *syn_tab;  // ecc_bits <= 64, t <= 4: [8][256] the odd syndromes S1, S3, S5, S7
                              // (16 bits each) of remainder byte b (from the top) holding value v
    int bps;                  // plane-sliced remainder kernels (ezbch_ps.hip): codec id, or -1
    int ncu;                  // compute units of the device
};

struct BchArgs {
    const uint8_t *data;      // rows read by both kernels
    uint8_t *wdata;           // the same rows, written by decode (corrections); null for encode
    size_t dstride;
    unsigned len;
    uint8_t *ecc;
    size_t estride;
    int32_t *result;
    uint32_t *errloc;
    size_t lstride;
    size_t ncw;
    int staged;               // the block's data rows are copied to LDS with coalesced loads
    int lds_fix;              // decode, staged rows with their ECC inline: corrections go to the LDS
                              // image and only the 16-byte pieces holding them are written back
    int ecc_only;             // decode_bch's "ecc = recv XOR calc" form: no data, nothing corrected
    const uint32_t *syn;      // decode_bch's syndrome form: S_1..S_2t per codeword (ecc_only set)
    size_t sstride;
};

// Codewords [k0, k0 + n) of a batch as a batch of their own.
inline BchArgs slice(const BchArgs &a, size_t k0, size_t n) {
    BchArgs c = a;
    c.ncw = n;
    if (c.data) c.data += k0 * a.dstride;
    if (c.wdata) c.wdata += k0 * a.dstride;
    if (c.ecc) c.ecc += k0 * a.estride;
    if (c.result) c.result += k0;
    if (c.errloc) c.errloc += k0 * a.lstride;
    if (c.syn) c.syn += k0 * a.sstride;
    return c;
}

constexpr size_t kLdsLimit = 65536;

// LDS layout of the lane kernels: [0, 2048 nw) byte-step table | exp/log tables (decode, m <= 12) |
// staged rows
__host__ __device__ inline size_t tabs_offset(const DevBch &b) { return (size_t)2048 * b.nw; }
__host__ __device__ inline size_t rows_offset(const DevBch &b, bool tabs) {
    return tabs_offset(b) + (tabs && b.lds_tabs ? (((size_t)3 * b.n + 1) * 2 + 15) / 16 * 16 : 0);
}

// staged rows: kThreads rows at the batch pitch from a dword-aligned start (+ 3 + 3 slack; C5's
// 256 rows of 127 bytes then fit four blocks per CU)
__host__ __device__ inline size_t rows_bytes(const BchArgs &a) { return (size_t)kThreads * a.dstride + 8; }

// Per-wave LDS of the wave decode: S[0..2t] u16 | C[W] u16 | B[W] u16 | lgC[W] i32 | P[t] u32 | E[t] u32 | cnt
__host__ __device__ inline size_t wave_w(int t) { return ((size_t)2 * t + 2 + 63) / 64 * 64; }
__host__ __device__ inline size_t wave_lds_bytes(int t) {
    return ((size_t)2 * t + 2) * 2 + wave_w(t) * (2 + 2 + 4) + (size_t)t * 8 + 16;
}

// f(std::integral_constant<int, NW>) for the kernels' remainder-word template argument: nw = 1, 2,
// 4 .. MAX, a power of two (DevBch::nw up to 16 on the lane path, DevBch::nwl up to 8 on the wave path)
template <int MAX, class F>
void with_nw(int nw, F &&f) {
    if (nw == 1) f(std::integral_constant<int, 1>{});
    else if (nw == 2) f(std::integral_constant<int, 2>{});
    else if (nw == 4) f(std::integral_constant<int, 4>{});
    else if (MAX > 8 && nw == 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, MAX>{});
}

// Lane kernels and the fused plane-sliced decode (ezbch_lane.hip): every batch the C ABI accepts;
// a wave-path codec (b.nwl != 0) is passed on to the launchers below.
hipError_t launch_encode(const DevBch &b, BchArgs a, hipStream_t s);
hipError_t launch_decode(const DevBch &b, BchArgs a, hipStream_t s);
// One wavefront per codeword (ezbch_wave.hip): b.nwl != 0.
hipError_t launch_encode_wave(const DevBch &b, const BchArgs &a, hipStream_t s);
hipError_t launch_decode_wave(const DevBch &b, const BchArgs &a, hipStream_t s);

} // namespace ezbch
