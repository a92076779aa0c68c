// ezbch_lane.hip -- batched binary BCH on MI355X (gfx950): one lane per codeword, 256-codeword
// workgroups, and the fused decode of the plane-sliced codecs.  Semantics: ezbch.hip.
//   k_bch_encode    byte-at-a-time LFSR over the data with a left-justified remainder of NW 64-bit
//                   words (NW = 1, 2, 4: ecc_bits <= 64, 128, 256) and a 256-entry step table in LDS;
//                   each row is read as aligned dwords (v_alignbyte).
//   k_bch_decode<T> the same remainder XOR the received ECC; zero -> result 0.  Otherwise, in the
//                   same lane: syndromes S_1..S_2t from the set bits of the difference, binary
//                   Berlekamp-Massey (odd steps; static register arrays), and the locator's roots:
//                   degree 1 directly, degrees 2..4 as an affine GF(2)-linear equation
//                   A4 y^4 + A2 y^2 + A1 y = delta solved by elimination over the m basis bits,
//                   degree > 4 by a Chien search over the codeword's bit positions.
//   k_bch_decode_big t <= 64, ecc_bits <= 1024 with run-time t (per-lane arrays).
//   k_bch_ps_decode  packed rows of a plane-sliced codec (ezbch_ps.hip), ECC inline: see below.
// Every larger init_bch-valid codec: one wavefront per codeword, ezbch_wave.hip.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>

#include "ezbch_locate.hpp"
#include "ezbch_ps.hpp"
#include "ezbch_ps_tile.hpp"

namespace ezbch {

using ezrs::BpsArgs;
using ezrs::bps_frame;
using ezrs::launch_bps;

namespace {

size_t lds_bytes(const DevBch &b, bool tabs, const BchArgs &a) {
    return rows_offset(b, tabs) + (a.staged ? rows_bytes(a) : 0);
}

// Rows are staged when the batch has a row pitch the block's span can hold within 64 KiB of LDS.
int want_staging(const DevBch &b, bool tabs, const BchArgs &a) {
    return a.ncw > 1 && a.len > 0 && a.dstride >= a.len &&
           rows_offset(b, tabs) + rows_bytes(a) <= kLdsLimit;
}

// ECC bytes inline after each row's data, rows packed back to back (the rows form at pitch len +
// ecc_bytes): the staged image holds them too, and a written-back piece holds no byte outside the
// rows (a gap between rows is never rewritten)
int ecc_inline(const DevBch &b, const BchArgs &a) {
    return a.ecc == a.data + a.len && a.estride == a.dstride && a.dstride == a.len + (size_t)b.ecc_bytes;
}

// The bytes p[0..len) in order, read as the aligned dwords that hold them.
template <class F>
__device__ __forceinline__ void for_each_byte(const uint8_t *p, unsigned len, F &&f) {
    if (!len) return;
    const unsigned a = (unsigned)((uintptr_t)p & 3u);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - a);
    const unsigned nd = (a + len + 3) >> 2;
    uint32_t lo = q[0];
    unsigned i = 0, j = 1;
    for (; i + 4 <= len; i += 4, ++j) {
        const uint32_t hi = j < nd ? q[j] : 0u;
        const uint32_t w = __builtin_amdgcn_alignbyte(hi, lo, a);
        f(w & 0xffu);
        f((w >> 8) & 0xffu);
        f((w >> 16) & 0xffu);
        f(w >> 24);
        lo = hi;
    }
    if (i < len) {
        uint32_t w = __builtin_amdgcn_alignbyte(j < nd ? q[j] : 0u, lo, a);
        for (; i < len; ++i, w >>= 8) f(w & 0xffu);
    }
}

// A left-justified multiword remainder: w[0] holds the most significant 64 bits.
template <int NW> struct Rem {
    uint64_t w[NW];
};

template <int NW>
__device__ __forceinline__ Rem<NW> data_remainder(const uint64_t *step, const uint8_t *p,
                                                  unsigned len) {
    Rem<NW> r;
#pragma unroll
    for (int i = 0; i < NW; ++i) r.w[i] = 0;
    for_each_byte(p, len, [&](uint32_t byte) {
        const uint64_t *s = step + NW * ((uint32_t)(r.w[0] >> 56) ^ byte);
#pragma unroll
        for (int i = 0; i < NW; ++i)
            r.w[i] = ((r.w[i] << 8) | (i + 1 < NW ? r.w[i + 1 < NW ? i + 1 : i] >> 56 : 0)) ^ s[i];
    });
    return r;
}

__device__ __forceinline__ void stage_tables(const DevBch &b, uint8_t *smem, bool tabs) {
    uint64_t *step = reinterpret_cast<uint64_t *>(smem);
    for (int i = threadIdx.x; i < 256 * b.nw; i += kThreads) step[i] = b.step[i];
    if (tabs && b.lds_tabs) {
        uint16_t *ex = reinterpret_cast<uint16_t *>(smem + tabs_offset(b)), *lg = ex + 2 * b.n;
        for (int i = threadIdx.x; i < 2 * b.n; i += kThreads) ex[i] = b.ex[i];
        for (int i = threadIdx.x; i <= b.n; i += kThreads) lg[i] = b.lg[i];
    }
    __syncthreads();
}

// This lane's data row: staged -- the block's rows are one contiguous span of global memory, copied
// into LDS with coalesced dword loads (a lane-per-row read of 127-byte rows touches a new cache line
// per lane and load) -- or read in place.
__device__ __forceinline__ const uint8_t *block_rows(uint8_t *smem, const DevBch &b, bool tabs,
                                                     const BchArgs &a) {
    const size_t k0 = (size_t)blockIdx.x * kThreads;
    if (!a.staged) return a.data + (k0 + threadIdx.x) * a.dstride;
    const size_t nrows = a.ncw - k0 < (size_t)kThreads ? a.ncw - k0 : (size_t)kThreads;
    const uint8_t *base = a.data + k0 * a.dstride;
    const size_t span = (nrows - 1) * a.dstride + a.len + (a.lds_fix ? (size_t)b.ecc_bytes : 0);
    const unsigned off = (unsigned)((uintptr_t)base & 3u);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(base - off);
    uint8_t *rows = smem + rows_offset(b, tabs);
    uint32_t *dst = reinterpret_cast<uint32_t *>(rows);
    const unsigned nd = (unsigned)((off + span + 3) >> 2);
    for (unsigned i = threadIdx.x; i < nd; i += kThreads) dst[i] = src[i];
    __syncthreads();
    return rows + off + threadIdx.x * a.dstride;
}

template <int NW>
__global__ void __launch_bounds__(kThreads) k_bch_encode(DevBch b, BchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    stage_tables(b, smem, false);
    const uint8_t *row = block_rows(smem, b, false, a);
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= a.ncw) return;
    const Rem<NW> r = data_remainder<NW>(reinterpret_cast<const uint64_t *>(smem), row, a.len);
    uint8_t *e = a.ecc + k * a.estride;
    // ecc_bytes = ceil(m t / 8) may pass the NW words when ecc_bits < m t: those bytes are zero
    for (int i = 0; i < b.ecc_bytes; ++i)
        e[i] = (i >> 3) < NW ? (uint8_t)(r.w[(i >> 3) < NW ? i >> 3 : 0] >> (56 - 8 * (i & 7))) : (uint8_t)0;
}

// Chien search over the codeword's bit positions p < nbits: X = alpha^p is a root of
// sigma(X) = sum_j C_j X^(L-j).  Returns the number of roots (their p in P[0..min(cnt,T)).
template <int T>
__device__ int chien(const GF &f, const uint32_t (&C)[2 * T + 2], int L, uint32_t nbits,
                     uint32_t (&P)[T]) {
    int lt[T + 1];
#pragma unroll
    for (int j = 0; j <= T; ++j) lt[j] = (j <= L && C[j]) ? (int)f.lg[C[j]] : -1;
    int cnt = 0;
    for (uint32_t p = 0; p < nbits; ++p) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j <= T; ++j)
            if (lt[j] >= 0) {
                v ^= f.ex[lt[j]];
                lt[j] += L - j;
                if (lt[j] >= f.n) lt[j] -= f.n;
            }
        if (!v) {
#pragma unroll
            for (int i = 0; i < T; ++i)
                if (i == cnt) P[i] = p;
            ++cnt;
        }
    }
    return cnt;
}

template <int J, int W>
__device__ __forceinline__ uint32_t coef(const uint32_t (&C)[W]) {
    if constexpr (J < W) return C[J];
    else return 0u;
}

// decode_bch on the masked ECC difference r (left-justified): the count and the ascending error
// locations, or -EBADMSG.
template <int T, int NW, int MM = 0>
__device__ int locate(const DevBch &b, const GF &f, Rem<NW> r, uint32_t nbits,
                      uint32_t (&loc)[T], const uint32_t *sin = nullptr) {
    uint64_t any = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) any |= r.w[i];
    if (!any && !sin) return 0;             // only unused ECC bits differ
    const uint32_t n = (uint32_t)b.n;
    uint32_t S[2 * T + 1];
#pragma unroll
    for (int j = 0; j <= 2 * T; ++j) S[j] = (sin && j > 0) ? sin[j - 1] : 0u;
    if (sin) {                              // a caller's syndrome outside GF(2^m) indexes no table
        uint32_t bad = 0;
#pragma unroll
        for (int j = 1; j <= 2 * T; ++j) bad |= S[j] > n;
        if (bad) return -EINVAL;
    }
    bool tab = false;
    if constexpr (NW == 1 && T <= 4) {
        if (b.syn_tab && !sin) {            // the odd syndromes are GF(2)-linear in the remainder's
            tab = true;                     // bits: one table entry per remainder byte
            uint64_t acc = 0;
            for (int bb = 0; bb < b.ecc_bytes; ++bb)
                acc ^= b.syn_tab[bb * 256 + (uint32_t)((r.w[0] >> (56 - 8 * bb)) & 255u)];
#pragma unroll
            for (int j = 1; j < 2 * T; j += 2) S[j] = (uint32_t)(acc >> (8 * (j - 1))) & 0xFFFFu;
        }
    }
#pragma unroll
    for (int wi = 0; wi < NW && !sin && !tab; ++wi) {
        uint64_t x = r.w[wi];
        while (x) {                         // S_j = r(alpha^j), j odd
            const int lz = __clzll(x);
            x &= ~(0x8000000000000000ull >> lz);
            const uint32_t p = (uint32_t)(b.ecc_bits - 1 - (64 * wi + lz));
            uint32_t p2 = 2 * p;
            if (p2 >= n) p2 -= n;
            uint32_t e = p;
#pragma unroll
            for (int j = 1; j < 2 * T; j += 2) {
                S[j] ^= f.ex[e];
                e += p2;
                if (e >= n) e -= n;
            }
        }
    }
    if (!sin) {
#pragma unroll
        for (int j = 1; j <= T; ++j) S[2 * j] = f.sq(S[j]);
    }

    // Berlekamp-Massey; for a binary code the even-step discrepancies vanish.  B holds x^m B.
    constexpr int W = 2 * T + 2;
    uint32_t C[W], B[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
        C[j] = j == 0;
        B[j] = j == 1;
    }
    int L = 0;
    // Log domain: the syndromes' logs once (an even one is twice the log of its half), the
    // discrepancy's quotient by its log, and only the coefficients that can be nonzero: before odd
    // step rr, deg C <= rr - 1 and deg B <= rr (B = x at rr = 1; C + q B, x^2 C, x^2 B keep it),
    // so the update touches C[1..rr].
    constexpr uint32_t kNoLog = 0xFFFFu;
    uint32_t lS[2 * T + 1];
#pragma unroll
    for (int j = 1; j <= 2 * T; ++j) {
        if (j % 2 || sin) {                 // a caller's even syndromes are taken as given
            lS[j] = S[j] ? (uint32_t)f.lg[S[j]] : kNoLog;
        } else {
            const uint32_t h = lS[j / 2];
            lS[j] = h == kNoLog ? kNoLog : (2 * h >= n ? 2 * h - n : 2 * h);
        }
    }
    uint32_t lbd = 0;                       // log of the last nonzero discrepancy (bd = 1)
#pragma unroll
    for (int rr = 1; rr < 2 * T; rr += 2) {
        uint32_t d = S[rr];
#pragma unroll
        for (int i = 1; i < rr; ++i)
            if (C[i] && lS[rr - i] != kNoLog) d ^= f.ex[f.lg[C[i]] + lS[rr - i]];
        if (d) {
            const bool grow = 2 * L <= rr - 1;
            const uint32_t ld = f.lg[d];
            const uint32_t lq = ld >= lbd ? ld - lbd : ld + n - lbd;    // log (d / bd)
            uint32_t old[W];
#pragma unroll
            for (int j = 0; j < W; ++j) old[j] = C[j];
#pragma unroll
            for (int j = 1; j <= rr && j < W; ++j)
                if (B[j]) C[j] ^= f.ex[lq + f.lg[B[j]]];
            if (grow) {
                L = rr - L;
                lbd = ld;
            }
#pragma unroll
            for (int j = W - 1; j >= 0; --j) B[j] = j >= 2 ? (grow ? old[j - 2] : B[j - 2]) : 0u;
        } else {
#pragma unroll
            for (int j = W - 1; j >= 0; --j) B[j] = j >= 2 ? B[j - 2] : 0u;
        }
    }
    if (L > T) return -kEBADMSG;
    if (L == 0) return 0;
    uint32_t lead = 0;
#pragma unroll
    for (int j = 0; j <= T; ++j)
        if (j == L) lead = C[j];
    if (!lead) return -kEBADMSG;            // the length exceeds the locator's true degree

    uint32_t P[T];                          // root exponents: X = alpha^P
    int nr = 0;
    if (L == 1) {
        P[0] = f.lg[C[1]];
        nr = 1;
    } else if (L <= 4) {
        uint32_t X[4];
        nr = small_roots<MM>(f, b.m, L, C[1], C[2], coef<3>(C), coef<4>(C), X);
#pragma unroll
        for (int i = 0; i < T && i < 4; ++i)
            if (i < nr) P[i] = f.lg[X[i]];
    } else {
        if constexpr (T > 4) nr = chien<T>(f, C, L, nbits, P);
    }
    if (nr != L) return -kEBADMSG;

    uint32_t el[T];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < T; ++i) {
        el[i] = 0xFFFFFFFFu;
        if (i < L) {
            if (P[i] >= nbits) {
                ok = false;
            } else {
                el[i] = bit_location(nbits - 1, P[i]);
            }
        }
    }
    if (!ok) return -kEBADMSG;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j + 1 < T - i; ++j) {
            const uint32_t x = el[j], y = el[j + 1];
            el[j] = x < y ? x : y;
            el[j + 1] = x < y ? y : x;
        }
#pragma unroll
    for (int i = 0; i < T; ++i) loc[i] = el[i];
    return L;
}

// ---- t > 16 or ecc_bits > 256: the same decode with run-time t ------------------------------
// The working polynomials are per-lane arrays indexed at run time (scratch memory): slower than
// the register-resident k_bch_decode<T, NW>, for the codecs it does not instantiate.

// Chien search over p < nbits, run-time degree L (as chien<T>)
__device__ int chien_big(const GF &f, const uint32_t *C, int L, uint32_t nbits, uint32_t *P, int T) {
    int lt[kBigT + 1];
    for (int j = 0; j <= L; ++j) lt[j] = C[j] ? (int)f.lg[C[j]] : -1;
    int cnt = 0;
    for (uint32_t p = 0; p < nbits; ++p) {
        uint32_t v = 0;
        for (int j = 0; j <= L; ++j)
            if (lt[j] >= 0) {
                v ^= f.ex[lt[j]];
                lt[j] += L - j;
                if (lt[j] >= f.n) lt[j] -= f.n;
            }
        if (!v) {
            if (cnt < T) P[cnt] = p;
            ++cnt;
        }
    }
    return cnt;
}

// locate<T, NW> with run-time t <= kBigT
template <int NW>
__device__ int locate_big(const DevBch &b, const GF &f, Rem<NW> r, uint32_t nbits, uint32_t *loc,
                          const uint32_t *sin = nullptr) {
    uint64_t any = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) any |= r.w[i];
    if (!any && !sin) return 0;
    const int T = b.t;
    const uint32_t n = (uint32_t)b.n;
    uint32_t S[2 * kBigT + 1];
    for (int j = 0; j <= 2 * T; ++j) S[j] = (sin && j > 0) ? sin[j - 1] : 0u;
    if (sin) {                              // a caller's syndrome outside GF(2^m) indexes no table
        uint32_t bad = 0;
        for (int j = 1; j <= 2 * T; ++j) bad |= S[j] > n;
        if (bad) return -EINVAL;
    }
#pragma unroll
    for (int wi = 0; wi < NW && !sin; ++wi) {
        uint64_t x = r.w[wi];
        while (x) {                         // S_j = r(alpha^j), j odd
            const int lz = __clzll(x);
            x &= ~(0x8000000000000000ull >> lz);
            const uint32_t p = (uint32_t)(b.ecc_bits - 1 - (64 * wi + lz));
            uint32_t p2 = 2 * p;
            if (p2 >= n) p2 -= n;
            uint32_t e = p;
            for (int j = 1; j < 2 * T; j += 2) {
                S[j] ^= f.ex[e];
                e += p2;
                if (e >= n) e -= n;
            }
        }
    }
    if (!sin)
        for (int j = 1; j <= T; ++j) S[2 * j] = f.sq(S[j]);
    // Berlekamp-Massey as in locate<T, NW>
    const int W = 2 * T + 2;
    uint32_t C[2 * kBigT + 2], B[2 * kBigT + 2], old[2 * kBigT + 2];
    for (int j = 0; j < W; ++j) {
        C[j] = j == 0;
        B[j] = j == 1;
    }
    int L = 0;
    uint32_t bd = 1;
    for (int rr = 1; rr < 2 * T; rr += 2) {
        uint32_t d = S[rr];
        for (int i = 1; i < rr; ++i) d ^= f.mul(C[i], S[rr - i]);
        if (d) {
            const bool grow = 2 * L <= rr - 1;
            const uint32_t q = f.div(d, bd);
            for (int j = 0; j < W; ++j) {
                old[j] = C[j];
                C[j] ^= f.mul(q, B[j]);
            }
            if (grow) {
                L = rr - L;
                bd = d;
            }
            for (int j = W - 1; j >= 0; --j) B[j] = j >= 2 ? (grow ? old[j - 2] : B[j - 2]) : 0u;
        } else {
            for (int j = W - 1; j >= 0; --j) B[j] = j >= 2 ? B[j - 2] : 0u;
        }
    }
    if (L > T) return -kEBADMSG;
    if (L == 0) return 0;
    if (!C[L]) return -kEBADMSG;
    uint32_t P[kBigT];
    int nr;
    if (L == 1) {
        P[0] = f.lg[C[1]];
        nr = 1;
    } else if (L <= 4) {
        uint32_t X[4];
        nr = small_roots(f, b.m, L, C[1], C[2], C[3], L >= 4 ? C[4] : 0u, X);
        for (int i = 0; i < nr && i < 4; ++i) P[i] = f.lg[X[i]];
    } else {
        nr = chien_big(f, C, L, nbits, P, T);
    }
    if (nr != L) return -kEBADMSG;
    for (int i = 0; i < L; ++i) {
        if (P[i] >= nbits) return -kEBADMSG;
        const uint32_t el = bit_location(nbits - 1, P[i]);
        int j = i;                          // insertion into the ascending list
        while (j > 0 && loc[j - 1] > el) {
            loc[j] = loc[j - 1];
            --j;
        }
        loc[j] = el;
    }
    return L;
}

// ---- the per-codeword decode of both lane kernels -----------------------------------------------
// The locator is a compile-time choice.  T > 0: locate<T, NW, MM>, its T locations in registers
// (every loop over them is fully unrolled and predicated, so that none is indexed at run time).
// Whether it is inlined decides the registers and the scratch of k_bch_decode<T, NW> (DESIGN.md
// section 4), so it is said here and does not hang on the compiler's size estimate of unrelated
// code: inline up to T = INL, a function of its own above.  INL is 7, and 12 for the syndrome form,
// whose zero remainder folds the set-bits loop away.  T = 0: locate_big<NW>, kBigT locations in a
// per-lane array walked by plain run-time loops.
template <int T>
constexpr int kLocCap = T ? T : kBigT;

template <int T, int NW, int MM = 0, int INL = 7>
__device__ __forceinline__ int locate_call(const DevBch &b, const GF &f, const Rem<NW> &r, uint32_t nbits,
                                           uint32_t (&loc)[kLocCap<T>], const uint32_t *sin = nullptr) {
    if constexpr (T == 0) {
        return locate_big<NW>(b, f, r, nbits, loc, sin);
    } else if constexpr (T > INL) {
        [[clang::noinline]] return locate<T, NW, MM>(b, f, r, nbits, loc, sin);
    } else {
        [[clang::always_inline]] return locate<T, NW, MM>(b, f, r, nbits, loc, sin);
    }
}

// One codeword of k_bch_decode<T, NW> or (T = 0) k_bch_decode_big<NW>; with `fix` (lds_fix) its
// corrections go to the staged image (row: this lane's row in it) instead of the rows in global
// memory, and loc[0 .. cnt_out) are left for the write-back.
template <int T, int NW>
__device__ __forceinline__ void decode_one(const DevBch &b, const BchArgs &a, uint8_t *smem, const uint8_t *row,
                                           size_t k, uint8_t *rows, bool fix, uint32_t (&loc)[kLocCap<T>], int &cnt_out) {
    if (8ull * a.len > (unsigned long long)(b.n - b.ecc_bits)) {   // decode_bch's length check
        a.result[k] = -kEINVAL;
        return;
    }
    const uint32_t nbits = 8u * a.len + (uint32_t)b.ecc_bits;
    if (a.syn) {                                        // syndrome form: locations only
        const Rem<NW> z{};
        uint32_t loc[kLocCap<T>];
        const int cnt = locate_call<T, NW, 0, 12>(b, field_view(b, smem), z, nbits, loc, a.syn + k * a.sstride);
        a.result[k] = cnt;
        if (a.errloc)
            for (int i = 0; i < cnt; ++i) a.errloc[k * a.lstride + i] = loc[i];
        return;
    }
    uint8_t *d = a.ecc_only ? nullptr : a.wdata + k * a.dstride, *e = a.ecc + k * a.estride;
    const uint8_t *er = fix ? row + a.len : e;           // the received ECC (staged when inline)
    Rem<NW> r{};
    if (!a.ecc_only) r = data_remainder<NW>(reinterpret_cast<const uint64_t *>(smem), row, a.len);
    for (int i = 0; i < b.ecc_bytes && (i >> 3) < NW; ++i)    // bytes past NW words: unused bits
        r.w[i >> 3] ^= (uint64_t)er[i] << (56 - 8 * (i & 7));
    uint64_t any = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) any |= r.w[i];
    if (!any) {
        a.result[k] = 0;
        return;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) r.w[i] &= b.emask[i];
    const int cnt = locate_call<T, NW>(b, field_view(b, smem), r, nbits, loc);
    a.result[k] = cnt;
    if (fix && cnt > 0) cnt_out = cnt;
    const auto correct = [&](int i) {
        const uint32_t el = loc[i];
        if (a.errloc) a.errloc[k * a.lstride + i] = el;
        if (a.ecc_only) return;
        if (fix) flip_lds(rows, (uint32_t)(row - rows), el);
        else flip_global(d, e, a.len, el);
    };
    if constexpr (T != 0) {
#pragma unroll
        for (int i = 0; i < T; ++i)
            if (i < cnt) correct(i);
    } else {
        for (int i = 0; i < cnt; ++i) correct(i);
    }
}

template <int T, int NW>
__global__ void __launch_bounds__(kThreads) k_bch_decode(DevBch b, BchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    stage_tables(b, smem, true);
    const uint8_t *row = a.ecc_only ? nullptr : block_rows(smem, b, true, a);
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    uint8_t *rows = smem + rows_offset(b, true);
    uint32_t loc[T];
    int cnt = 0;
    if (k < a.ncw) decode_one<T, NW>(b, a, smem, row, k, rows, a.lds_fix != 0, loc, cnt);
    if (!a.lds_fix) return;                             // (uniform over the block)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // Every lane of the wave has flipped its bits in the image.  What the wave may write: the bytes
    // of its own 64 rows (the neighbouring waves and blocks write theirs); the image starts at the
    // dword that holds the block's first byte.
    const size_t k0 = (size_t)blockIdx.x * kThreads;
    const size_t nrows = a.ncw - k0 < (size_t)kThreads ? a.ncw - k0 : (size_t)kThreads;
    const unsigned w = threadIdx.x >> 6;
    const size_t wend = 64u * w + 64u < nrows ? 64u * w + 64u : nrows;     // the wave's rows [64 w, wend)
    uint8_t *base = a.wdata + k0 * a.dstride;
    const unsigned off = (unsigned)((uintptr_t)base & 3u);
    write_back_pieces<true>(rows, base - off, (int)(off + 64u * w * a.dstride),
                         (int)(off + (wend - 1) * a.dstride + a.len + (size_t)b.ecc_bytes), (uint32_t)(row - rows),
                         loc, cnt);
}

// t > 16 or ecc_bits > 256: locate_big's run-time t
template <int NW>
__global__ void __launch_bounds__(kThreads) k_bch_decode_big(DevBch b, BchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    stage_tables(b, smem, true);
    const uint8_t *row = a.ecc_only ? nullptr : block_rows(smem, b, true, a);
    const size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x;
    uint32_t loc[kBigT];
    int cnt = 0;
    if (k < a.ncw) decode_one<0, NW>(b, a, smem, row, k, nullptr, false, loc, cnt);
}

// ---- plane-sliced codecs, ECC inline (C5): the fused decode ------------------------------------
// The encode's tile loop (ezbch_ps_tile.hpp) leaves each row's remainder XOR its received ECC in
// registers; a nonzero one is located (locate<T, 1>, the GF tables staged in LDS), its bits are
// flipped in the tile's LDS image, and after a workgroup barrier each row writes back the 16-byte
// pieces of the global grid that hold its flips -- a piece reaching outside the tile's bytes only
// over the tile's own, byte by byte.  One pass over the rows: read once, corrected pieces written.
// One tile image per workgroup and three workgroups per CU: the per-row locate is a chain of
// dependent table reads, and a third wave per SIMD hides more of it than a second image hides of
// the DMA (8 M: 0.644 vs 0.780 ms with two images and two workgroups per CU, r06r)
constexpr int kDecSlots = 1;
constexpr int kDecLds = kDecSlots * ezrs::bps::kImgSlot + ezrs::bps::kTW * ezrs::bps::kXch;
constexpr int kDecPerCu = 3;                   // workgroups per CU (LDS)

template <class C>
__global__ void __launch_bounds__(64 * ezrs::bps::kTW, kDecPerCu) k_bch_ps_decode(DevBch b, BchArgs a, BpsArgs p) {
    namespace bp = ezrs::bps;
    constexpr int TW = bp::tile_waves<C>(), T = C::T, NR = 4 / TW;
    constexpr uint32_t n = (1u << C::M) - 1;
    static_assert(T <= 4, "odd syndromes S1 .. S7 from the nibble tables");
    constexpr uint32_t kTabs = ((3 * n + 1) * 2 + 15) / 16 * 16, kNib = 2 * C::EB * 16;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kDecLds + kTabs + 8 * kNib];
    uint16_t *ex = reinterpret_cast<uint16_t *>(lds + kDecLds), *lg = ex + 2 * n;
    // syndrome tables by nibble of the remainder (from the top): the byte tables are linear in the
    // byte, so nibble q's entry for v is the byte table's for v << 4 (q even) or v
    uint64_t *nib = reinterpret_cast<uint64_t *>(lds + kDecLds + kTabs);
    for (uint32_t i = threadIdx.x; i < 2 * n; i += blockDim.x) ex[i] = b.ex[i];
    for (uint32_t i = threadIdx.x; i <= n; i += blockDim.x) lg[i] = b.lg[i];
    for (uint32_t i = threadIdx.x; i < kNib; i += blockDim.x) {
        const uint32_t q = i >> 4, v = i & 15u;
        nib[i] = b.syn_tab[(q >> 1) * 256 + ((q & 1) ? v : v << 4)];
    }
    __syncthreads();
    const GF f{ex, lg, (int)n};
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = bp::lane_id();
    const uint32_t nbits = 8u * a.len + (uint32_t)b.ecc_bits, tb = bp::kRows * p.stride;
    // rows 4l + k, k = w (TW = 4) or 2w, 2w + 1
    bp::tile_loop<C, true, -1, kDecSlots>(p, lds, [&](uint32_t tile, uint8_t *image, const uint32_t (&out)[C::EB]) {
        uint32_t loc[NR][T];
        int cnt[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const uint32_t k = NR * w + j, r = 4u * l + k;
            const size_t row = (size_t)tile * bp::kRows + r;
            cnt[j] = 0;
            if (row >= a.ncw) continue;
            uint32_t wd[2];
            bp::row_bytes<C::EB>(out, k, wd);
            Rem<1> rm;
            rm.w[0] = (((uint64_t)__builtin_bswap32(wd[0]) << 32) | __builtin_bswap32(wd[1])) & b.emask[0];
            int c = 0;
            if (rm.w[0]) {
                uint64_t acc = 0;
#pragma unroll
                for (uint32_t q = 0; q < 2 * C::EB; ++q) acc ^= nib[q * 16 + (uint32_t)((rm.w[0] >> (60 - 4 * q)) & 15u)];
                uint32_t S[2 * T];                          // S_1 .. S_2T; S_2j = S_j^2
#pragma unroll
                for (int jj = 1; jj < 2 * T; jj += 2) S[jj - 1] = (uint32_t)(acc >> (8 * (jj - 1))) & 0xFFFFu;
#pragma unroll
                for (int jj = 1; jj <= T; ++jj) S[2 * jj - 1] = f.sq(S[jj - 1]);
                c = locate_call<T, 1, C::M>(b, f, rm, nbits, loc[j], S);
            }
            a.result[row] = c;
            if (c <= 0) continue;
            cnt[j] = c;
#pragma unroll
            for (int i = 0; i < T; ++i) {
                if (i >= c) break;
                if (a.errloc) a.errloc[row * a.lstride + i] = loc[j][i];
                flip_lds(image, r * p.stride, loc[j][i]);
            }
        }
        __syncthreads();                                    // every row's flips are in the image
        // the tile's bytes of the image [0, hi); the image follows the rows' own alignment
        const uint32_t toff = tile * tb, hi = p.span - toff < tb ? p.span - toff : tb;
#pragma unroll
        for (int j = 0; j < NR; ++j)
            write_back_pieces<false>(image, a.wdata + toff, 0, (int)hi, (4u * l + NR * w + j) * p.stride, loc[j], cnt[j]);
    });
}

// Launches of the plane-sliced kernels over a batch: 256-row tiles, every byte offset of a launch
// below 0xE0000000 (32-bit buffer offsets).
template <class F>
hipError_t bps_chunks(const BchArgs &a, F &&launch) {
    const size_t pitch = a.dstride > a.estride ? a.dstride : a.estride;
    size_t per = (size_t)0xE0000000u / (pitch ? pitch : 1) / 256 * 256;
    if (per > ((size_t)1 << 28)) per = (size_t)1 << 28;       // 8-byte remainders: 32-bit offsets
    if (per == 0) per = 256;
    for (size_t k0 = 0; k0 < a.ncw; k0 += per) {
        const size_t n = a.ncw - k0 < per ? a.ncw - k0 : per;
        const hipError_t e = launch(k0, n);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The plane-sliced path takes rows of its frame (encode: data <= F bytes, decode: data + ECC) at a
// pitch of at most 128 bytes; decode also needs the ECC right after the data (the row is one
// polynomial).
bool bps_ok(const DevBch &b, const BchArgs &a, bool dec) {
    if (b.bps < 0 || a.ecc_only || a.syn || a.len == 0 || a.dstride > 128 || a.ncw == 0) return false;
    if (8ull * a.len > (unsigned long long)(b.n - b.ecc_bits)) return false;
    if ((int)(a.len + (dec ? b.ecc_bytes : 0)) > bps_frame(b.bps)) return false;
    if (dec && !(a.ecc == a.data + a.len && a.estride == a.dstride)) return false;
    if (!dec && (a.estride < b.ecc_bytes || a.estride > 4096)) return false;
    return a.dstride >= a.len;
}

hipError_t launch_bps_decode(const DevBch &b, const BchArgs &a, const BpsArgs &p, hipStream_t s) {
    const unsigned cap = (unsigned)kDecPerCu * (unsigned)(b.ncu > 0 ? b.ncu : 256);
    const unsigned grid = p.ntiles < cap ? p.ntiles : cap;
    if (!grid) return hipSuccess;
    int k = 0;
#define EZBCH_PS_DECODE(N, M, T)                                                                     \
    if (k++ == b.bps)                                                                                \
        hipLaunchKernelGGL((k_bch_ps_decode<ezrs::bps::BPS_##N>), dim3(grid),                       \
                           dim3(64 * ezrs::bps::tile_waves<ezrs::bps::BPS_##N>()), 0, s, b, a, p);
    EZBCH_PS_CODEC_LIST(EZBCH_PS_DECODE)
#undef EZBCH_PS_DECODE
    return hipGetLastError();
}

} // namespace

hipError_t launch_encode(const DevBch &b, BchArgs a, hipStream_t s) {
    if (bps_ok(b, a, false)) {
        return bps_chunks(a, [&](size_t k0, size_t n) {
            const BpsArgs p{a.data + k0 * a.dstride, (uint32_t)((n - 1) * a.dstride + a.len), (uint32_t)a.dstride,
                            (uint32_t)n, (uint32_t)((n + 255) / 256), bps_frame(b.bps) - (int)a.len,
                            a.ecc + k0 * a.estride, a.estride,
                            (uint32_t)((n - 1) * a.estride + b.ecc_bytes)};
            return launch_bps(b.bps, p, b.ncu, s);
        });
    }
    if (b.nwl) return launch_encode_wave(b, a, s);
    const unsigned grid = (unsigned)((a.ncw + kThreads - 1) / kThreads);
    a.staged = want_staging(b, false, a);
    const size_t sh = lds_bytes(b, false, a);
    with_nw<16>(b.nw, [&](auto NW) {
        hipLaunchKernelGGL(k_bch_encode<decltype(NW)::value>, dim3(grid), dim3(kThreads), sh, s, b, a);
    });
    return hipGetLastError();
}

hipError_t launch_decode(const DevBch &b, BchArgs a, hipStream_t s) {
    if (bps_ok(b, a, true) && ecc_inline(b, a)) {            // packed rows, ECC inline: fused decode
        return bps_chunks(a, [&](size_t k0, size_t n) {
            const BchArgs c = slice(a, k0, n);
            const BpsArgs p{c.data, (uint32_t)((n - 1) * a.dstride + a.len + b.ecc_bytes), (uint32_t)a.dstride,
                            (uint32_t)n, (uint32_t)((n + 255) / 256), bps_frame(b.bps) - (int)(a.len + b.ecc_bytes),
                            nullptr, 0, 0};
            return launch_bps_decode(b, c, p, s);
        });
    }
    if (b.nwl) return launch_decode_wave(b, a, s);
    const unsigned grid = (unsigned)((a.ncw + kThreads - 1) / kThreads);
    a.lds_fix = !a.ecc_only && !a.syn && ecc_inline(b, a) && b.t <= 16 && b.nw <= 4;  // k_bch_decode<T, NW>
    a.staged = a.ecc_only ? 0 : want_staging(b, true, a);
    if (!a.staged) a.lds_fix = 0;
    const size_t sh = lds_bytes(b, true, a);
    // (T, NW) instantiations: NW = 1 for ecc_bits <= 64 (t <= 12 since m >= 5), NW = 2 for
    // ecc_bits <= 128 (m t > 64: t >= 5), NW = 4 for ecc_bits <= 256 (t >= 9)
#define EZBCH_CASE(T, NW)                                                                     \
    if (b.t == T && b.nw == NW) {                                                             \
        hipLaunchKernelGGL((k_bch_decode<T, NW>), dim3(grid), dim3(kThreads), sh, s, b, a);   \
        return hipGetLastError();                                                             \
    }
    EZBCH_CASE(1, 1) EZBCH_CASE(2, 1) EZBCH_CASE(3, 1) EZBCH_CASE(4, 1) EZBCH_CASE(5, 1)
    EZBCH_CASE(6, 1) EZBCH_CASE(7, 1) EZBCH_CASE(8, 1) EZBCH_CASE(9, 1) EZBCH_CASE(10, 1)
    EZBCH_CASE(11, 1) EZBCH_CASE(12, 1)
    EZBCH_CASE(5, 2) EZBCH_CASE(6, 2) EZBCH_CASE(7, 2) EZBCH_CASE(8, 2) EZBCH_CASE(9, 2)
    EZBCH_CASE(10, 2) EZBCH_CASE(11, 2) EZBCH_CASE(12, 2) EZBCH_CASE(13, 2) EZBCH_CASE(14, 2)
    EZBCH_CASE(15, 2) EZBCH_CASE(16, 2)
    EZBCH_CASE(9, 4) EZBCH_CASE(10, 4) EZBCH_CASE(11, 4) EZBCH_CASE(12, 4) EZBCH_CASE(13, 4)
    EZBCH_CASE(14, 4) EZBCH_CASE(15, 4) EZBCH_CASE(16, 4)
#undef EZBCH_CASE
    // everything else init_bch accepts up to t = 64, ecc_bits = 1024
    with_nw<16>(b.nw, [&](auto NW) {
        hipLaunchKernelGGL(k_bch_decode_big<decltype(NW)::value>, dim3(grid), dim3(kThreads), sh, s, b, a);
    });
    return hipGetLastError();
}

} // namespace ezbch
