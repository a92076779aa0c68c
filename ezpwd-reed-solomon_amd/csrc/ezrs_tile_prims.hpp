// ezrs_tile_prims.hpp -- primitives of the plane-sliced tile kernels, shared by the RS kernels
// (ezrs_ps.hip) and the BCH tile loop (ezbch_ps_tile.hpp): the lane id, buffer descriptors, LDS
// addresses, byte transposes and the row reads of a 16-position piece.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ezrs {
namespace tile {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef int rsrc_t __attribute__((ext_vector_type(4)));

// The lane id, recomputed (v_mbcnt) wherever it is used: values derived from it are then not
// hoisted out of a tile loop, where they would pin registers across the state.
__device__ __forceinline__ uint32_t lane_id() {
    uint32_t l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// Buffer descriptor of [base, base + span): raw (stride 0), out-of-range bytes read as zero.
__device__ __forceinline__ rsrc_t make_rsrc(const uint8_t *base, uint32_t span) {
    const uint64_t p = (uint64_t)(uintptr_t)base;
    rsrc_t r;
    r.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)p);
    r.y = __builtin_amdgcn_readfirstlane((int)((uint32_t)(p >> 32) & 0xFFFFu));
    r.z = __builtin_amdgcn_readfirstlane((int)span);
    r.w = 0x00020000;
    return r;
}

__device__ __forceinline__ uint32_t lds_addr(const uint8_t *p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t *)p;
}

// 4x4 byte transpose: out[t] byte k = in[k] byte t.
__device__ __forceinline__ void transpose4x4(const uint32_t (&a)[4], uint32_t *out) {
    const uint32_t t01 = __builtin_amdgcn_perm(a[1], a[0], 0x05010400u);
    const uint32_t t23 = __builtin_amdgcn_perm(a[3], a[2], 0x05010400u);
    const uint32_t u01 = __builtin_amdgcn_perm(a[1], a[0], 0x07030602u);
    const uint32_t u23 = __builtin_amdgcn_perm(a[3], a[2], 0x07030602u);
    out[0] = __builtin_amdgcn_perm(t23, t01, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(t23, t01, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(u23, u01, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(u23, u01, 0x07060302u);
}

// Bytes s of a0..a3 -> one dword (a0 in byte 0).
__device__ __forceinline__ uint32_t gather4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, int s) {
    const uint32_t sel = (uint32_t)s | ((uint32_t)(s + 4) << 8) | 0x0c0c0000u;   // 0x0c: zero byte
    const uint32_t x01 = __builtin_amdgcn_perm(a1, a0, sel), x23 = __builtin_amdgcn_perm(a3, a2, sel);
    return __builtin_amdgcn_perm(x23, x01, 0x05040100u);
}

// Raw dwords of rows 4l + k at one 16-position piece (4-byte aligned reads, aligned afterwards
// with v_alignbyte).
struct Raw {
    u32x2 e[4][2];
    uint32_t d4[4];
};

// the piece at byte offset OFF (a multiple of 8) from the rows' dword-aligned position-0 addresses
// at4[k]: the offset rides in the instructions' immediates
template <int OFF>
__device__ __forceinline__ void issue_at(Raw &r, const uint32_t (&at4)[4]) {
    static_assert(OFF % 4 == 0 && OFF / 4 + 4 < 256, "ds_read2 dword offsets");
#pragma unroll
    for (int k = 0; k < 4; ++k)
        asm volatile("ds_read2_b32 %0, %3 offset0:%4 offset1:%5\n\t"
                     "ds_read2_b32 %1, %3 offset0:%6 offset1:%7\n\t"
                     "ds_read_b32 %2, %3 offset:%8"
                     : "=&v"(r.e[k][0]), "=&v"(r.e[k][1]), "=&v"(r.d4[k])
                     : "v"(at4[k]), "n"(OFF / 4), "n"(OFF / 4 + 1), "n"(OFF / 4 + 2), "n"(OFF / 4 + 3), "n"(OFF + 16)
                     : "memory");
}
__device__ __forceinline__ void wait_raw(Raw &r) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(r.e[0][0]), "+v"(r.e[0][1]), "+v"(r.d4[0]), "+v"(r.e[1][0]), "+v"(r.e[1][1]), "+v"(r.d4[1]),
                   "+v"(r.e[2][0]), "+v"(r.e[2][1]), "+v"(r.d4[2]), "+v"(r.e[3][0]), "+v"(r.e[3][1]), "+v"(r.d4[3])
                 :: "memory");
}

} // namespace tile
} // namespace ezrs
