// ezbch_locate.hpp -- device-only pieces shared by the lane kernels, the fused plane-sliced decode
// (ezbch_lane.hip) and the wave kernels (ezbch_wave.hip): the field view, the closed-form roots of
// a locator of degree <= 4, the reported bit location of a root, and the correction of a located
// bit in the rows in global memory or in an LDS image with its 16-byte piece write-back.
#pragma once

#include "ezbch_internal.hpp"

namespace ezbch {

struct GF {
    const uint16_t *ex, *lg;
    int n;
    __device__ uint32_t mul(uint32_t a, uint32_t b) const { return (a && b) ? ex[lg[a] + lg[b]] : 0u; }
    __device__ uint32_t div(uint32_t a, uint32_t b) const { return a ? ex[lg[a] + n - lg[b]] : 0u; }
    __device__ uint32_t inv(uint32_t a) const { return ex[n - lg[a]]; }
    __device__ uint32_t sq(uint32_t a) const { return a ? ex[2 * lg[a]] : 0u; }
    __device__ uint32_t sqrt(uint32_t a) const {
        if (!a) return 0u;
        const uint32_t l = lg[a];
        return ex[(l & 1) ? (l + n) >> 1 : l >> 1];
    }
};

// The field of a lane kernel: the tables stage_tables copied behind the step table in LDS
// (b.lds_tabs), or the ones in global memory.
__device__ __forceinline__ GF field_view(const DevBch &b, const uint8_t *smem) {
    const uint16_t *sx = reinterpret_cast<const uint16_t *>(smem + tabs_offset(b));
    return GF{b.lds_tabs ? sx : b.ex, b.lds_tabs ? sx + 2 * b.n : b.lg, b.n};
}

// The reported location of the codeword bit whose locator root is alpha^P (P <= last = nbits - 1):
// bit e = last - P counted from the first data bit, as data[e / 8] bit 7 - e % 8.
__device__ __forceinline__ uint32_t bit_location(uint32_t last, uint32_t P) {
    const uint32_t e = last - P;
    return (e & ~7u) | (7u - (e & 7u));
}

// Flip the bit at location el of a codeword in global memory: data row d of len bytes, ECC e.
__device__ __forceinline__ void flip_global(uint8_t *d, uint8_t *e, unsigned len, uint32_t el) {
    if (el < 8u * len) d[el >> 3] ^= (uint8_t)(1u << (el & 7));
    else e[(el >> 3) - len] ^= (uint8_t)(1u << (el & 7));
}

// Flip the bit at location el of the row at byte offset row_off of an LDS image (data, then its
// inline ECC); rows may share a dword.
__device__ __forceinline__ void flip_lds(uint8_t *image, uint32_t row_off, uint32_t el) {
    const uint32_t o = row_off + (el >> 3);
    atomicXor(reinterpret_cast<uint32_t *>(image + (o & ~3u)), (1u << (el & 7)) << (8 * (o & 3)));
}

// Once every flip of the rows sharing it is in the image (the caller's barrier): the row at image
// offset row_off writes back the 16-byte pieces (on the global 16-byte grid) that hold its corrected
// bits loc[0 .. cnt), from the image -- a piece wholly inside the image bytes [lo, hi) as one store
// (a piece shared by two rows may be written by both, with the same bytes), a piece reaching past
// them byte by byte over [lo, hi) only (whoever owns the neighbouring bytes writes the rest).
// g: the global address of image byte 0; DWORDS: g is dword aligned, so a piece is too and is read
// from the image as aligned dwords (else as bytes).
template <bool DWORDS, int T>
__device__ __forceinline__ void write_back_pieces(const uint8_t *image, uint8_t *g, int lo, int hi, uint32_t row_off,
                                                  const uint32_t (&loc)[T], int cnt) {
    const uint32_t gmis = (uint32_t)((uintptr_t)g & 15u);                  // image offset -> piece grid
    int last = -1000;
#pragma unroll
    for (int i = 0; i < T; ++i) {
        if (i >= cnt) break;
        const uint32_t o = row_off + (loc[i] >> 3);
        const int p0 = (int)((o + gmis) & ~15u) - (int)gmis;              // image offset of the piece
        if (p0 == last) continue;
        last = p0;
        if (p0 >= lo && p0 + 16 <= hi) {
            uint4 v;
            if constexpr (DWORDS) {
                const uint32_t *s4 = reinterpret_cast<const uint32_t *>(image + p0);
                v = make_uint4(s4[0], s4[1], s4[2], s4[3]);
            } else {
                __builtin_memcpy(&v, image + p0, 16);
            }
            *reinterpret_cast<uint4 *>(g + p0) = v;
        } else if constexpr (DWORDS) {
            // at most 15 bytes, and in the lane kernels any row may end in such a piece: a plain
            // byte loop (vectorised into a block copy it cost BCH(12,5) 1.7 % of its decode)
#pragma clang loop vectorize(disable)
            for (int q = p0 < lo ? lo : p0; q < p0 + 16 && q < hi; ++q) g[q] = image[q];
        } else {                                    // a tile's two ends: the compiler's choice
            for (int q = p0 < lo ? lo : p0; q < p0 + 16 && q < hi; ++q) g[q] = image[q];
        }
    }
}

// y -> A4 y^4 + A2 y^2 + A1 y is GF(2)-linear.  With the images of the polynomial-basis vectors
// 1 << i (= alpha^i) in echelon form: returns the kernel dimension, or -1 if A(y) = delta has no
// solution; y0 = a particular solution, k1, k2 = the first two kernel basis vectors.
// MM: m known at compile time (the plane-sliced decode's codec), or 0
template <int MM = 0>
__device__ int solve_affine(const GF &f, int m, uint32_t A4, uint32_t A2, uint32_t A1,
                            uint32_t delta, uint32_t &y0, uint32_t &k1, uint32_t &k2) {
    constexpr int kM = MM ? MM : kMaxM;
    if constexpr (MM != 0) m = MM;
    const int l4 = A4 ? (int)f.lg[A4] : -1, l2 = A2 ? (int)f.lg[A2] : -1, l1 = A1 ? (int)f.lg[A1] : -1;
    uint32_t v[kM], c[kM];
    int pb[kM];
    int dim = 0;
    uint32_t q1 = 0, q2 = 0;                // k1, k2: selects, not a store indexed by dim (scratch)
#pragma unroll
    for (int i = 0; i < kM; ++i) {
        v[i] = 0;
        c[i] = 0;
        pb[i] = -1;
        if (i < m) {
            uint32_t w = 0;
            if (l4 >= 0) w ^= f.ex[l4 + 4 * i];
            if (l2 >= 0) w ^= f.ex[l2 + 2 * i];
            if (l1 >= 0) w ^= f.ex[l1 + i];
            uint32_t cc = 1u << i;
#pragma unroll
            for (int k = 0; k < i; ++k)
                if (pb[k] >= 0 && ((w >> pb[k]) & 1u)) {
                    w ^= v[k];
                    cc ^= c[k];
                }
            v[i] = w;
            c[i] = cc;
            pb[i] = w ? 31 - __clz(w) : -1;
            q1 = (!w && dim == 0) ? cc : q1;
            q2 = (!w && dim == 1) ? cc : q2;
            dim += !w;
        }
    }
    uint32_t y = 0, rem = delta;
#pragma unroll
    for (int k = 0; k < kM; ++k)
        if (pb[k] >= 0 && ((rem >> pb[k]) & 1u)) {
            rem ^= v[k];
            y ^= c[k];
        }
    y0 = y;
    k1 = q1;
    k2 = q2;
    return rem ? -1 : dim;
}

// Roots X of sigma(X) = X^L + a X^(L-1) + b X^(L-2) + c X^(L-3) + d for L = 2..4 (sigma(0) != 0);
// returns L if there are L distinct roots, else 0.
template <int MM = 0>
__device__ int small_roots(const GF &f, int m, int L, uint32_t a, uint32_t b, uint32_t c, uint32_t d,
                           uint32_t (&X)[4]) {
    uint32_t A4, A2, A1, delta, s = 0;
    int want;                               // kernel dimension of L distinct roots
    if (L == 2) {                           // y = X:         y^2 + a y = b
        A4 = 0; A2 = 1; A1 = a; delta = b; want = 1;
    } else if (L == 3) {                    // y = X + a:     y^4 + (a^2 + b) y^2 + (ab + c) y = 0, y != 0
        A4 = 1; A2 = f.sq(a) ^ b; A1 = f.mul(a, b) ^ c; delta = 0; want = 2; s = a;
    } else if (a == 0) {                    // y = X:         y^4 + b y^2 + c y = d
        A4 = 1; A2 = b; A1 = c; delta = d; want = 2;
    } else {                                // X = s + 1/y, s^2 = c/a:  y^4 + (as + b)/e y^2 + a/e y = 1/e
        s = f.sqrt(f.div(c, a));
        const uint32_t s2 = f.sq(s);
        const uint32_t e = f.sq(s2) ^ f.mul(a, f.mul(s2, s)) ^ f.mul(b, s2) ^ f.mul(c, s) ^ d;
        if (!e) return 0;                   // X = s is a double root
        const uint32_t ie = f.inv(e);
        A4 = 1; A2 = f.mul(f.mul(a, s) ^ b, ie); A1 = f.mul(a, ie); delta = ie; want = 2;
    }
    uint32_t y0, k1, k2;
    if (solve_affine<MM>(f, m, A4, A2, A1, delta, y0, k1, k2) != want) return 0;
    // L = 2: y0, y0 + k1; L = 3 (y0 = 0): the three nonzero kernel elements + s; L = 4: the four
    // solutions y, X = 1/y + s (a != 0) or y.  Selects, every X[i] written: a store per case
    // would be merged into one indexed by L, in scratch memory.
    const bool l3 = L == 3, inv = L == 4 && a;
    const uint32_t y[4] = {l3 ? k1 : y0, l3 ? k2 : y0 ^ k1, l3 ? k1 ^ k2 : y0 ^ k2, y0 ^ k1 ^ k2};
#pragma unroll
    for (int i = 0; i < 4; ++i) X[i] = inv ? f.inv(y[i] ? y[i] : 1u) ^ s : (l3 ? y[i] ^ s : y[i]);
    return L;
}

} // namespace ezbch
