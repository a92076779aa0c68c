// ezrs_interleave.hip -- interleaved frames <-> packed rows (ezrs_encode_interleaved /
// ezrs_decode_interleaved, include/ezrs.h).
//
// A frame carries `depth` codewords interleaved symbol by symbol (CCSDS depth I; striped shards:
// depth = shard length, symbol stride = shard pitch).  The row kernels want one codeword per row,
// so k_il_gather copies the frames' symbols into packed rows in a staging area and k_il_scatter
// copies rows back; the codec's own kernels run unchanged in between (ezrs_capi.hip).
//
// Shape of both kernels: a workgroup owns a tile of 256 consecutive codewords (k = f * depth + j),
// whose staged rows are one contiguous span, and streams over the symbols in chunks of 128 bytes
// per row through an LDS tile [256 rows][132 bytes].
//   frame side  lanes are split between consecutive codewords (contiguous along j in a frame) and
//               consecutive symbols (contiguous too when sym_stride == depth is small): 64 / LS
//               lanes along j, LS along s, LS chosen per call from the depth, so a wavefront's
//               accesses fall in few cache lines at every depth.
//               General path: one element per lane and access, any geometry.
//               Fast path (uint8_t; depth, sym_stride, frame_pitch and the base multiples of 4): a
//               lane moves dwords -- four codewords of one symbol -- for four symbols and does the
//               4x4 byte transpose in registers, so LDS sees dwords only.
//   row side    consecutive lanes take consecutive 16-byte aligned slots of the rows' span: one
//               16-byte global access each, aligned dword LDS accesses and a v_alignbyte funnel
//               shift in between (packed rows start at every byte alignment); the partial slots
//               at a row segment's two ends are stored from the same registers as dwords and
//               bytes.
// LDS pitch 132 bytes = 33 dwords (banks are (a/4) mod 32 for ds_write and ds_read_b32): a column
// of dwords over consecutive rows, and a row's consecutive dwords, both fall in distinct banks;
// fast-path frame-side accesses (row 4q + i, dword c) are conflict-free for LS = 4 and 32 and at
// most 2-way (free on ds_write_b32) for LS = 8 and 16; the row side's 4 rows x 8 slots per
// 32-lane group are distinct up to each row's alignment shift (at most 2-way).
// The only division is one per thread and tile (k -> frame, column), 32-bit when it fits.
//
// Addressing policy, chosen by the argument struct A of both kernels.  Strided (IlArgs): symbol s of
// codeword (f, j) is element f * frame_pitch + s * sym_stride + j of `frames`.  Pointers
// (IlPtrArgs; ezrs_decode_ptrs / ezrs_decode_ptrs_batch): it is element j of the buffer
// table[f * pitch + s], the table in device memory.  Only the frame side differs: lanes along s
// read consecutive table entries, lanes along j of one stripe the same entry.  A tile that lies in
// one stripe (every tile once shard_len >= 256 + 255) holds the pointers of the current symbol
// chunk in LDS (at most 128 entries, one coalesced table read per chunk), so the symbol accesses
// do not wait for a table load each; a tile that spans stripes reads its entries from the table,
// one per symbol access.  The pointer fast path needs shard_len and every pointer to be multiples
// of 4; tiles start at multiples of 256 codewords, so a quad of codewords never straddles stripes.
// Selection (IlSel<B> over either policy; ezrs_decode_ptrs_select / ezrs_decode_interleaved_select):
// staged row i is codeword sel[i], so a tile's 256 rows are 256 codewords anywhere in the batch.  A
// thread reads its row's entry once (coalesced) and does its one division; off[] and row[] then mean
// what they mean in the "tile spans stripes" path, and off[] = kSkip marks a skipped row, which the
// gather stages as zeros and the scatter leaves out of flag[].  Neighbouring rows are not
// neighbouring codewords, so there is no dword path and the lanes of a wave go along the symbols
// (LS from len + NROOTS): in the pointer form they read consecutive table entries of one stripe.
#include "ezrs_internal.hpp"

namespace ezrs {
namespace il {

constexpr unsigned kTile = (unsigned)kIlTile;
constexpr unsigned kChunkB = 128;             // bytes of a row per symbol chunk
constexpr unsigned kPitchB = 132;             // LDS row pitch
constexpr unsigned kSlots = kChunkB / 16 + 1; // 16-byte global slots a row segment can touch

// 4x4 byte transpose: out[t] byte k = in[k] byte t.
__device__ __forceinline__ void transpose4x4(const uint32_t (&a)[4], uint32_t (&out)[4]) {
    const uint32_t t01 = __builtin_amdgcn_perm(a[1], a[0], 0x05010400u);
    const uint32_t t23 = __builtin_amdgcn_perm(a[3], a[2], 0x05010400u);
    const uint32_t u01 = __builtin_amdgcn_perm(a[1], a[0], 0x07030602u);
    const uint32_t u23 = __builtin_amdgcn_perm(a[3], a[2], 0x07030602u);
    out[0] = __builtin_amdgcn_perm(t23, t01, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(t23, t01, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(u23, u01, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(u23, u01, 0x07060302u);
}

// Codeword k = f * depth + j.
__device__ __forceinline__ void frame_of(size_t depth, size_t k, size_t &f, size_t &j) {
    if (((k | depth) >> 32) == 0) {                 // 32-bit division (see shard_row)
        const uint32_t k32 = (uint32_t)k, d32 = (uint32_t)depth, f32 = k32 / d32;
        f = f32;
        j = k32 - f32 * d32;
    } else {
        f = k / depth;
        j = k - f * depth;
    }
}

// Element offset of codeword k's symbol 0 in the frames.
__device__ __forceinline__ size_t frame_off(const IlArgs &a, size_t k) {
    size_t f, j;
    frame_of(a.depth, k, f, j);
    return f * a.frame_pitch + j;
}

template <class A>
constexpr bool kPtrs = std::is_base_of_v<IlPtrArgs, A>;
template <class A>
constexpr bool kSel = false;
template <class B>
constexpr bool kSel<IlSel<B>> = true;

// What a tile of the pointer policy keeps in LDS besides off[] (which holds j): the first table
// entry of every codeword's stripe and, for a tile in one stripe, the buffers of the symbol chunk.
template <bool PTRS>
struct PtrTile {};
template <>
struct PtrTile<true> {
    size_t row[kTile];
    void *sym[kChunkB];
};

// Pointer policy: (stripe, element) of the tile's codewords k .. k + nk - 1 into off[] and row[].
// one: the tile lies in one stripe, whose first table entry is row0 (both uniform over the tile).
// One division per tile (uniform) where the tile lies in one stripe, else one per thread.
__device__ __forceinline__ void ptr_tile(const IlPtrArgs &a, size_t k, unsigned nk, unsigned t, size_t *off,
                                         PtrTile<true> &pt, bool &one, size_t &row0) {
    size_t f, j;
    frame_of(a.depth, k, f, j);
    one = j + nk <= a.depth;
    row0 = f * a.pitch;
    if (one) j += t;
    else frame_of(a.depth, k + t, f, j);            // t >= nk: an entry that is never used
    off[t] = j;
    pt.row[t] = f * a.pitch;
}

constexpr size_t kSkip = ~(size_t)0;              // off[] of a selected row that is skipped

// Selection: (stripe, element) or the frame offset of the codeword of row i of the call into off[]
// (and row[]), for thread t; want: the row is needed at all.  False: not wanted, or skipped.
template <class A>
__device__ __forceinline__ bool sel_tile(const A &a, size_t i, bool want, unsigned t, size_t *off,
                                         PtrTile<kPtrs<A>> &pt) {
    typedef __attribute__((address_space(1))) const uint64_t Mem;   // global memory, as the table is
    size_t k = 0, f = 0, j = 0;
    bool use = want && (!a.count || i < *(Mem *)a.count);
    if (use) {
        k = ((Mem *)a.sel)[i];
        use = k < a.ncw;
    }
    if (use) frame_of(a.depth, k, f, j);
    if constexpr (kPtrs<A>) {
        off[t] = use ? j : kSkip;
        pt.row[t] = f * a.pitch;
    } else {
        off[t] = use ? f * a.frame_pitch + j : kSkip;
    }
    return use;
}

// Entry e of the pointer table, read as the global memory it is (see At).
__device__ __forceinline__ void *table_at(const IlPtrArgs &a, size_t e) {
    typedef void *Ptr;
    return ((__attribute__((address_space(1))) const Ptr *)a.table)[e];
}

// The frame side of one symbol chunk (first symbol sa) under either policy.  cw(off[kk]): what is
// fixed for codeword kk of the tile, the address of its symbol sa (strided) or its element j
// (pointers); sym(that, kk, s): where its symbol sa + s is; as<U>: that address as a U.  The
// buffers of the pointer policy are global memory and typed so: a generic pointer would make every
// symbol access a flat one, which counts on the LDS counter too, so the wait for the next pointer
// out of LDS would wait for all the symbol loads before it.  ONE (pointers): the tile lies in one
// stripe and the chunk's pointers are in LDS; a template parameter, so that the choice is made once
// per chunk and not in a branch around every access, which would keep a lane's pointer reads apart.
template <typename T, class A, bool ONE>
struct At {
    static constexpr bool PTRS = kPtrs<A>;
    template <typename U>
    using Mem = std::conditional_t<PTRS, __attribute__((address_space(1))) U *, U *>;
    typedef std::conditional_t<PTRS, size_t, T *> Cw;
    typedef Mem<T> Sym;
    const A &a;
    T *frames;
    const PtrTile<PTRS> &pt;
    unsigned sa;
    __device__ __forceinline__ Cw cw(size_t off) const {
        if constexpr (PTRS) return off;
        else return frames + off + (size_t)sa * a.sym_stride;
    }
    __device__ __forceinline__ Sym sym(Cw p, unsigned kk, unsigned s) const {
        if constexpr (PTRS) return (Sym)static_cast<T *>(ONE ? pt.sym[s] : table_at(a, pt.row[kk] + sa + s)) + p;
        else return p + (size_t)s * a.sym_stride;
    }
    template <typename U>
    static __device__ __forceinline__ Mem<U> as(Sym q) {
        if constexpr (PTRS) return (Mem<U>)q;
        else return reinterpret_cast<U *>(q);
    }
};

// Frames -> rows.  lg = log2(LS).
template <typename T, bool FAST, class A>
__global__ void __launch_bounds__(256) k_il_gather(A a, unsigned lg) {
    constexpr bool PTRS = kPtrs<A>, SEL = kSel<A>;
    // 16 guard bytes on either side: a partial slot's aligned dword reads may start before row 0
    // and end after row 255 (those bytes are never stored)
    __shared__ __attribute__((aligned(16))) uint8_t lds[16 + kTile * kPitchB + 16];
    __shared__ size_t off[kTile];
    __shared__ PtrTile<PTRS> pt;
    uint8_t *const tile = lds + 16;
    constexpr unsigned SC = kChunkB / sizeof(T), PT = kPitchB / sizeof(T);
    const unsigned t = threadIdx.x;
    const size_t kt0 = (size_t)blockIdx.x * kTile;
    const unsigned nk = a.n - kt0 < kTile ? (unsigned)(a.n - kt0) : kTile;
    bool one = false;
    size_t row0 = 0;
    if constexpr (SEL) sel_tile(a, a.k0 + kt0 + t, t < nk, t, off, pt);
    else if constexpr (PTRS) ptr_tile(a, a.k0 + kt0, nk, t, off, pt, one, row0);
    else off[t] = t < nk ? frame_off(a, a.k0 + kt0 + t) : 0;
    const T *frames = static_cast<const T *>(a.frames);
    uint8_t *rb = static_cast<uint8_t *>(a.rows);
    const unsigned ls = 1u << lg, si = t & (ls - 1), ki = t >> lg, kstep = 256u >> lg;
    for (unsigned sa = a.s0; sa < a.s1; sa += SC) {
        const unsigned ns = a.s1 - sa < SC ? a.s1 - sa : SC;
        if constexpr (PTRS && !SEL)                 // the last chunk's frame side is behind a barrier
            if (one && t < ns) pt.sym[t] = table_at(a, row0 + sa + t);
        __syncthreads();                            // off[] written; the tile's last chunk stored
        const auto frame_side = [&](auto at) {
            if constexpr (FAST) {
#pragma unroll 4
                for (unsigned q = ki; 4 * q < nk; q += kstep) {
                    const auto p = at.cw(off[4 * q]);
                    for (unsigned s4 = 4 * si; s4 < ns; s4 += 4 * ls) {
                        uint32_t in[4], out[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            in[i] = s4 + i < ns ? *at.template as<const uint32_t>(at.sym(p, 4 * q, s4 + i)) : 0u;
                        transpose4x4(in, out);          // out[i]: symbols s4..s4+3 of codeword 4q + i
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            *reinterpret_cast<uint32_t *>(tile + (4 * q + i) * kPitchB + s4) = out[i];
                    }
                }
            } else {
                T *lt = reinterpret_cast<T *>(tile);
                for (unsigned kk = ki; kk < nk; kk += kstep) {
                    if constexpr (SEL)
                        if (off[kk] == kSkip) {     // a skipped row: the all-zero word, nothing read
                            for (unsigned s = si; s < ns; s += ls) lt[kk * PT + s] = 0;
                            continue;
                        }
                    const auto p = at.cw(off[kk]);
#pragma unroll 8
                    for (unsigned s = si; s < ns; s += ls) lt[kk * PT + s] = *at.sym(p, kk, s);
                }
            }
        };
        if (PTRS && !SEL && one) frame_side(At<const T, A, PTRS && !SEL>{a, frames, pt, sa});
        else frame_side(At<const T, A, false>{a, frames, pt, sa});
        __syncthreads();
        // rows: the 16-byte aligned slots of every row's segment [g, g + nb)
        const unsigned nb = ns * (unsigned)sizeof(T);
        for (unsigned e = t; e < nk * kSlots; e += 256) {
            const unsigned kk = e / kSlots, q = e - kk * kSlots;
            const size_t g = ((kt0 + kk) * a.row_pitch + sa) * sizeof(T);
            const size_t G = (g & ~(size_t)15) + 16 * q;
            const int d = (int)(ptrdiff_t)(G - g);                 // -15 .. 128
            if (d >= (int)nb) continue;
            // bytes d .. d + 15 of the row's LDS segment from aligned dwords (d < 0 or d + 16 > nb:
            // the out-of-segment bytes come from the neighbouring rows or the guards and are dropped)
            const uint32_t *lw = reinterpret_cast<const uint32_t *>(tile + kk * kPitchB + (d & ~3));
            const uint32_t r = (uint32_t)d & 3;
            const uint32_t w0 = lw[0], w1 = lw[1], w2 = lw[2], w3 = lw[3], w4 = lw[4];
            const uint32_t o[4] = {__builtin_amdgcn_alignbyte(w1, w0, r), __builtin_amdgcn_alignbyte(w2, w1, r),
                                   __builtin_amdgcn_alignbyte(w3, w2, r), __builtin_amdgcn_alignbyte(w4, w3, r)};
            if (d >= 0 && d + 16 <= (int)nb) {
                *reinterpret_cast<uint4 *>(rb + G) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {                                // a segment's first or last slot: dwords, then bytes
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int p0 = d + 4 * i;
                    if (p0 >= 0 && p0 + 4 <= (int)nb) {
                        *reinterpret_cast<uint32_t *>(rb + G + 4 * i) = o[i];
                    } else {
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            if (p0 + b >= 0 && p0 + b < (int)nb) rb[G + 4 * i + b] = (uint8_t)(o[i] >> (8 * b));
                    }
                }
            }
        }
    }
}

// Rows -> frames, for every codeword of the tile (result == null) or those with a nonzero result.
template <typename T, bool FAST, class A>
__global__ void __launch_bounds__(256) k_il_scatter(A a, unsigned lg) {
    constexpr bool PTRS = kPtrs<A>, SEL = kSel<A>;
    __shared__ __attribute__((aligned(16))) uint8_t tile[kTile * kPitchB];
    __shared__ size_t off[kTile];
    __shared__ PtrTile<PTRS> pt;
    __shared__ __attribute__((aligned(4))) uint8_t flag[kTile];   // 1: write this codeword back
    constexpr unsigned SC = kChunkB / sizeof(T), PT = kPitchB / sizeof(T);
    const unsigned t = threadIdx.x;
    const size_t kt0 = (size_t)blockIdx.x * kTile;
    const unsigned nk = a.n - kt0 < kTile ? (unsigned)(a.n - kt0) : kTile;
    bool mine = t < nk && (!a.result || a.result[kt0 + t] != 0);
    if constexpr (SEL) mine = sel_tile(a, a.k0 + kt0 + t, mine, t, off, pt);   // and not skipped
    flag[t] = mine;
    if (!__syncthreads_or(mine)) return;            // a tile of clean codewords: nothing to write
    bool one = false;
    size_t row0 = 0;
    if constexpr (PTRS && !SEL) ptr_tile(a, a.k0 + kt0, nk, t, off, pt, one, row0);
    else if constexpr (!SEL) off[t] = mine ? frame_off(a, a.k0 + kt0 + t) : 0;
    T *frames = static_cast<T *>(a.frames);
    const uint8_t *rb = static_cast<const uint8_t *>(a.rows);
    const unsigned ls = 1u << lg, si = t & (ls - 1), ki = t >> lg, kstep = 256u >> lg;
    for (unsigned sa = a.s0; sa < a.s1; sa += SC) {
        const unsigned ns = a.s1 - sa < SC ? a.s1 - sa : SC;
        const unsigned nb = ns * (unsigned)sizeof(T);
        __syncthreads();
        if constexpr (PTRS && !SEL)                 // read after the next barrier
            if (one && t < ns) pt.sym[t] = table_at(a, row0 + sa + t);
        // rows -> LDS: 16-byte LDS slots from aligned global dwords (reads may run up to 19 bytes
        // past the segment: inside the staging area, il_stage_bytes)
        for (unsigned e = t; e < nk * (kChunkB / 16); e += 256) {
            const unsigned kk = e >> 3, q = e & 7;
            if (16 * q >= nb || !flag[kk]) continue;
            const size_t g = ((kt0 + kk) * a.row_pitch + sa) * sizeof(T) + 16 * q;
            const uint32_t *gp = reinterpret_cast<const uint32_t *>(rb + (g & ~(size_t)3));
            const uint32_t r = (uint32_t)g & 3;
            const uint32_t w0 = gp[0], w1 = gp[1], w2 = gp[2], w3 = gp[3], w4 = r ? gp[4] : 0u;
            uint32_t *lw = reinterpret_cast<uint32_t *>(tile + kk * kPitchB + 16 * q);
            lw[0] = __builtin_amdgcn_alignbyte(w1, w0, r);
            lw[1] = __builtin_amdgcn_alignbyte(w2, w1, r);
            lw[2] = __builtin_amdgcn_alignbyte(w3, w2, r);
            lw[3] = __builtin_amdgcn_alignbyte(w4, w3, r);
        }
        __syncthreads();
        const auto frame_side = [&](auto at) {
            if constexpr (FAST) {
                for (unsigned q = ki; 4 * q < nk; q += kstep) {
                    const uint32_t fl = *reinterpret_cast<const uint32_t *>(flag + 4 * q);
                    if (!fl) continue;
                    // off[] of the quad's first flagged codeword gives the quad's base
                    const unsigned i0 = (fl & 0xFFu) ? 0 : (fl & 0xFF00u) ? 1 : (fl & 0xFF0000u) ? 2 : 3;
                    const auto p = at.cw(off[4 * q + i0] - i0);
                    for (unsigned s4 = 4 * si; s4 < ns; s4 += 4 * ls) {
                        uint32_t in[4], out[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            in[i] = *reinterpret_cast<const uint32_t *>(tile + (4 * q + i) * kPitchB + s4);
                        transpose4x4(in, out);          // out[m]: symbol s4 + m of codewords 4q..4q+3
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            if (s4 + m >= ns) continue;
                            const auto dst = at.sym(p, 4 * q, s4 + m);
                            if (fl == 0x01010101u) {
                                *at.template as<uint32_t>(dst) = out[m];
                            } else {
#pragma unroll
                                for (int b = 0; b < 4; ++b)
                                    if ((fl >> (8 * b)) & 0xFFu) dst[b] = (uint8_t)(out[m] >> (8 * b));
                            }
                        }
                    }
                }
            } else {
                const T *lt = reinterpret_cast<const T *>(tile);
                for (unsigned kk = ki; kk < nk; kk += kstep) {
                    if (!flag[kk]) continue;
                    const auto p = at.cw(off[kk]);
#pragma unroll 4
                    for (unsigned s = si; s < ns; s += ls) *at.sym(p, kk, s) = lt[kk * PT + s];
                }
            }
        };
        if (PTRS && !SEL && one) frame_side(At<T, A, PTRS && !SEL>{a, frames, pt, sa});
        else frame_side(At<T, A, false>{a, frames, pt, sa});
    }
}

// Fast path: uint8_t, every dword of four codewords aligned.
static bool fast_ok(const DevCodec &d, const IlArgs &a) {
    if (d.mm > 8) return false;
    return ((a.depth | a.sym_stride | a.frame_pitch | (size_t)(uintptr_t)a.frames) & 3) == 0;
}

// log2 of the lanes along the symbols: the others (64 / LS) go along j, as many as one frame has
// consecutive codewords (fast path: dwords of four) to give, rounded down to a power of two.
static unsigned lanes_log2(size_t depth, bool fast) {
    const size_t per = fast ? depth / 4 : depth;
    unsigned lj = 0;                                // log2 of the lanes along j
    while (lj < 6 && ((size_t)2 << lj) <= per) ++lj;
    unsigned lg = 6 - lj;
    if (fast) {                                     // 4..32: the LDS bank analysis above
        if (lg < 2) lg = 2;
        if (lg > 5) lg = 5;
    }
    return lg;
}

// Selection: the lanes go along the symbols, as many as a row has (at most a wave).
static unsigned sel_lanes_log2(size_t syms) {
    unsigned lg = 0;
    while (lg < 6 && ((size_t)1 << lg) < syms) ++lg;
    return lg;
}

template <bool GATHER, class A>
static hipError_t launch(const DevCodec &d, const A &a, bool fast, hipStream_t s) {
    if (!a.n || a.s0 >= a.s1) return hipSuccess;
    if (a.n > kIlMaxRows) return hipErrorInvalidValue;
    const unsigned lg = kSel<A> ? sel_lanes_log2(a.row_pitch) : lanes_log2(a.depth, fast);
    const dim3 grid((unsigned)((a.n + kTile - 1) / kTile)), block(256);
    if (d.mm > 8) {
        if (GATHER) hipLaunchKernelGGL((k_il_gather<uint16_t, false, A>), grid, block, 0, s, a, lg);
        else hipLaunchKernelGGL((k_il_scatter<uint16_t, false, A>), grid, block, 0, s, a, lg);
    } else if (!kSel<A> && fast) {
        if constexpr (!kSel<A>) {
            if (GATHER) hipLaunchKernelGGL((k_il_gather<uint8_t, true, A>), grid, block, 0, s, a, lg);
            else hipLaunchKernelGGL((k_il_scatter<uint8_t, true, A>), grid, block, 0, s, a, lg);
        }
    } else {
        if (GATHER) hipLaunchKernelGGL((k_il_gather<uint8_t, false, A>), grid, block, 0, s, a, lg);
        else hipLaunchKernelGGL((k_il_scatter<uint8_t, false, A>), grid, block, 0, s, a, lg);
    }
    return hipGetLastError();
}

// Pointer fast path: uint8_t, the shard length and every pointer multiples of 4.
static bool fast_ok(const DevCodec &d, const IlPtrArgs &a, size_t al) { return d.mm <= 8 && ((a.depth | al) & 3) == 0; }

// One stripe's pointers from the kernel arguments into device memory, one entry per thread.  The
// entry is read where the kernel arguments lie (`tab` is the first of them), as k_recon's table
// policy does: indexed as tab.p[threadIdx.x], a lane-varying index, the compiler would copy the
// whole table to scratch first.
__global__ void __launch_bounds__(kPtrsMax) k_il_table(PtrTable tab, unsigned n, void **out) {
    typedef void *Ptr;                              // a generic pointer that lies in the kernarg segment
    typedef __attribute__((address_space(4))) const Ptr Ent;
    Ent *const args = (Ent *)__builtin_amdgcn_kernarg_segment_ptr();
    if (threadIdx.x < n) out[threadIdx.x] = args[threadIdx.x];
}

} // namespace il

hipError_t launch_il_gather(const DevCodec &d, const IlArgs &a, hipStream_t s) {
    return il::launch<true>(d, a, il::fast_ok(d, a), s);
}
hipError_t launch_il_scatter(const DevCodec &d, const IlArgs &a, hipStream_t s) {
    return il::launch<false>(d, a, il::fast_ok(d, a), s);
}
hipError_t launch_il_gather(const DevCodec &d, const IlPtrArgs &a, size_t al, hipStream_t s) {
    return il::launch<true>(d, a, il::fast_ok(d, a, al), s);
}
hipError_t launch_il_scatter(const DevCodec &d, const IlPtrArgs &a, size_t al, hipStream_t s) {
    return il::launch<false>(d, a, il::fast_ok(d, a, al), s);
}
// Selection over the strided policy: the same arguments without the table.
static IlSel<IlArgs> sel_strided(const IlSel<IlPtrArgs> &a) { return {{(const IlArgs &)a}, a.sel, a.count, a.ncw}; }
hipError_t launch_il_gather(const DevCodec &d, const IlSel<IlPtrArgs> &a, bool ptrs, hipStream_t s) {
    return ptrs ? il::launch<true>(d, a, false, s) : il::launch<true>(d, sel_strided(a), false, s);
}
hipError_t launch_il_scatter(const DevCodec &d, const IlSel<IlPtrArgs> &a, bool ptrs, hipStream_t s) {
    return ptrs ? il::launch<false>(d, a, false, s) : il::launch<false>(d, sel_strided(a), false, s);
}
hipError_t launch_il_table(const PtrTable &tab, unsigned n, void **out, hipStream_t s) {
    hipLaunchKernelGGL(il::k_il_table, dim3(1), dim3(kPtrsMax), 0, s, tab, n, out);
    return hipGetLastError();
}

} // namespace ezrs
