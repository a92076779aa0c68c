// ezrs_recon.hip -- shared-erasure reconstruction of interleaved frames (ezrs_recon_create /
// ezrs_reconstruct_interleaved, include/ezrs.h).
//
// Striped shards lose whole shards: every codeword of the stripe has the same erasure positions and
// no other errors.  The erasure system is then solved once per loss pattern on the host
// (recon_build) and what is left for the device is one constant matrix over GF(2^m) applied to the
// surviving symbols of every codeword, in place in the frames: no gather, no staging, no
// per-codeword control flow.
//
// The matrix.  S = len + NROOTS symbols, position p relative to the first data symbol,
// X(i, p) = alpha^((fcr + i) * prim * (S - 1 - p)), so that syndrome i of a word c is
// sum_p X(i, p) c_p.  With A = X(i < nlost, lost[r]):
//   rebuild rows  r < nlost      R[r][c] = sum_i A^-1[r][i] X(i, surv[c])   -> the symbol at lost[r]
//   check rows    nlost <= i     R[i][c] = X(i, surv[c]) + sum_r X(i, lost[r]) R[r][c]
//                                                          -> syndrome i of the rebuilt word
// The kernel never multiplies in the field: a coefficient is kept as its m bit columns in the
// codec's stored representation, col[r][c][b] = rep(R[r][c] * unrep(1 << b)) (rep / unrep: the CCSDS
// dual-basis maps, or the identity), and an output symbol is the XOR of the columns of the set bits
// of the survivors.  That covers every m and the dual basis with no table of the field.
//
// The kernel.  A lane owns a run of consecutive codewords of one frame: 16 bytes (one dwordx4 per
// symbol row) when the base and the strides allow it, else a dword, else one element; consecutive
// lanes take consecutive runs, so every survivor load and every lost-symbol store is coalesced.
//   m > 8   bit-column form (apply): per survivor dword and bit b the SWAR mask of the codewords
//           whose bit b is set is formed once and shared by all rows: acc[row] ^= mask & K[row][c][b]
//           (one v_bitop3), K being the bit column replicated across the dword.
//   m <= 8  byte form (apply8, apply8x2): the columns of three bits are folded on the host into an
//           8-entry byte table per row, and v_perm_b32 looks up the four codewords of a dword at
//           once: three lookups per row and dword instead of eight mask-and-XOR steps.
// The tables are indexed with wave-uniform values only and come through the scalar cache.  Rows
// are taken RB at a time (RB accumulators per dword of the run); the blocks of a plan with more
// rows are looped inside the kernel, so the check rows of all blocks are OR-ed in registers and
// `result` is written once, whatever the order.
//
// The in-place parity update (ezrs_update_create / ezrs_update_interleaved, k_update) is the same
// machinery on the difference of a few data symbols: the columns of the all-parity matrix at the
// changed positions, applied to new ^ old and XOR-ed into the parity where it lies.
//
// Both kernels address their symbol rows through a compile-time policy (At): rows at one stride from
// one base (the interleaved calls), one pointer per row, carried by value in the kernel arguments
// (ezrs_reconstruct_ptrs / ezrs_update_ptrs: one stripe whose shards are buffers of their own), or
// one pointer per row and stripe in a table in device memory (ezrs_reconstruct_ptrs_batch /
// ezrs_update_ptrs_batch: many such stripes per call).  In the batch forms a wave never spans two
// stripes, so all a plan contributes is uniform over the wave; ezrs_reconstruct_ptrs_mixed
// (ReconMixedArgs) and ezrs_update_ptrs_mixed (UpdateMixedArgs) therefore choose the plan per
// stripe, from a set of plans in one allocation.
#include <algorithm>
#include <cerrno>
#include <new>
#include <utility>

#include "../../include/ezrs.h"
#include "ezrs_internal.hpp"

namespace ezrs {

namespace {

// alpha^((fcr + i) * prim * (S - 1 - p))
inline unsigned recon_x(const CodecMath &m, unsigned i, unsigned S, unsigned p) {
    const uint64_t root = ((uint64_t)m.spec.fcr + i) % m.nn * (m.spec.prim % m.nn) % m.nn;
    return m.gf.alpha_to[root * (S - 1 - p) % m.nn];
}

inline unsigned gf_inv(const Field &gf, unsigned a) { return gf.alpha_to[(gf.nn - gf.index_of[a]) % gf.nn]; }

// In-place Gauss-Jordan inverse of the n x n matrix a (row-major); false if singular.
bool gf_invert(const Field &gf, std::vector<uint16_t> &a, unsigned n) {
    std::vector<uint16_t> inv((size_t)n * n, 0);
    for (unsigned i = 0; i < n; ++i) inv[(size_t)i * n + i] = 1;
    for (unsigned col = 0; col < n; ++col) {
        unsigned piv = col;
        while (piv < n && !a[(size_t)piv * n + col]) ++piv;
        if (piv == n) return false;
        if (piv != col)
            for (unsigned j = 0; j < n; ++j) {
                std::swap(a[(size_t)piv * n + j], a[(size_t)col * n + j]);
                std::swap(inv[(size_t)piv * n + j], inv[(size_t)col * n + j]);
            }
        const unsigned s = gf_inv(gf, a[(size_t)col * n + col]);
        for (unsigned j = 0; j < n; ++j) {
            a[(size_t)col * n + j] = (uint16_t)gf.mul(a[(size_t)col * n + j], s);
            inv[(size_t)col * n + j] = (uint16_t)gf.mul(inv[(size_t)col * n + j], s);
        }
        for (unsigned r = 0; r < n; ++r) {
            const unsigned f = a[(size_t)r * n + col];
            if (r == col || !f) continue;
            for (unsigned j = 0; j < n; ++j) {
                a[(size_t)r * n + j] ^= (uint16_t)gf.mul(a[(size_t)col * n + j], f);
                inv[(size_t)r * n + j] ^= (uint16_t)gf.mul(inv[(size_t)col * n + j], f);
            }
        }
    }
    a.swap(inv);
    return true;
}

} // namespace

bool recon_check(const CodecMath &m, unsigned len, const uint32_t *lost, unsigned nlost) {
    if (len < 1 || len > m.load || nlost > m.spec.nroots || (nlost && !lost)) return false;
    const unsigned S = len + m.spec.nroots;
    std::vector<uint8_t> seen(S, 0);
    for (unsigned r = 0; r < nlost; ++r) {
        if (lost[r] >= S || seen[lost[r]]) return false;
        seen[lost[r]] = 1;
    }
    return true;
}

bool recon_build(const CodecMath &m, unsigned len, const uint32_t *lost, unsigned nlost,
                 std::vector<uint16_t> &cols, std::vector<uint32_t> &surv) {
    if (!recon_check(m, len, lost, nlost)) return false;
    const Field &gf = m.gf;
    const unsigned NR = m.spec.nroots, S = len + NR, mm = m.spec.mm, nsurv = S - nlost;
    std::vector<uint8_t> gone(S, 0);
    for (unsigned r = 0; r < nlost; ++r) gone[lost[r]] = 1;
    surv.clear();
    for (unsigned p = 0; p < S; ++p)
        if (!gone[p]) surv.push_back(p);
    std::vector<uint16_t> ainv((size_t)nlost * nlost), xl((size_t)NR * nlost);
    for (unsigned i = 0; i < NR; ++i)
        for (unsigned r = 0; r < nlost; ++r) xl[(size_t)i * nlost + r] = (uint16_t)recon_x(m, i, S, lost[r]);
    std::copy(xl.begin(), xl.begin() + (size_t)nlost * nlost, ainv.begin());   // A[i][r]
    if (nlost && !gf_invert(gf, ainv, nlost)) return false;                    // ainv[r][i]
    // R, one survivor column at a time
    cols.assign((size_t)NR * nsurv * mm, 0);
    std::vector<uint16_t> xs(NR), R(NR);
    for (unsigned c = 0; c < nsurv; ++c) {
        for (unsigned i = 0; i < NR; ++i) xs[i] = (uint16_t)recon_x(m, i, S, surv[c]);
        for (unsigned r = 0; r < nlost; ++r) {
            unsigned v = 0;
            for (unsigned i = 0; i < nlost; ++i) v ^= gf.mul(ainv[(size_t)r * nlost + i], xs[i]);
            R[r] = (uint16_t)v;
        }
        for (unsigned i = nlost; i < NR; ++i) {
            unsigned v = xs[i];
            for (unsigned r = 0; r < nlost; ++r) v ^= gf.mul(xl[(size_t)i * nlost + r], R[r]);
            R[i] = (uint16_t)v;
        }
        for (unsigned b = 0; b < mm; ++b) {
            const unsigned e = m.spec.dual ? m.from_dual[1u << b] : 1u << b;
            for (unsigned r = 0; r < NR; ++r) {
                const unsigned v = gf.mul(R[r], e);
                cols[((size_t)r * nsurv + c) * mm + b] = (uint16_t)(m.spec.dual ? m.into_dual[v] : v);
            }
        }
    }
    return true;
}

// Rows of the device table per (survivor, bit): NROOTS rounded up to the row block that serves it,
// so that a row block's scalar loads never leave the table; rows past NROOTS are zero.
unsigned recon_row_pad(unsigned nroots) {
    for (unsigned rb = 4; rb < 32; rb *= 2)
        if (nroots <= rb) return rb;
    return (nroots + 31) / 32 * 32;
}

// Dwords of the coefficient part of the table.  m <= 8: per survivor, group of three symbol bits and
// row, the 8 byte-wide images of the group's values (two dwords; apply8).  m > 8: per survivor, bit
// and row, the bit's column replicated across the dword (apply).
size_t recon_coef_words(unsigned mm, unsigned nroots, unsigned nsurv) {
    const size_t per = mm <= 8 ? (size_t)((mm + 2) / 3) * 2 : mm;
    return (size_t)nsurv * per * recon_row_pad(nroots);
}

size_t recon_table_words(unsigned mm, unsigned nroots, unsigned nsurv, unsigned nlost) {
    return recon_coef_words(mm, nroots, nsurv) + nsurv + nlost + recon_row_pad(nroots);
}

void recon_table(unsigned mm, unsigned nroots, const std::vector<uint16_t> &cols,
                 const std::vector<uint32_t> &surv, const uint32_t *lost, unsigned nlost,
                 std::vector<uint32_t> &tab) {
    const unsigned nsurv = (unsigned)surv.size(), nrp = recon_row_pad(nroots);
    tab.assign(recon_table_words(mm, nroots, nsurv, nlost), 0);
    const TableView<uint32_t> t = table_view(tab.data(), mm, nroots, nsurv, nlost);
    std::copy(surv.begin(), surv.end(), t.pos);
    std::copy(lost, lost + nlost, t.lost);
    if (mm <= 8) {
        const unsigned G = (mm + 2) / 3;
        for (unsigned r = 0; r < nroots; ++r)
            for (unsigned c = 0; c < nsurv; ++c)
                for (unsigned g = 0; g < G; ++g) {
                    uint32_t *e = &tab[(((size_t)c * G + g) * nrp + r) * 2];
                    for (unsigned v = 1; v < 8; ++v) {          // image of the group value v
                        uint32_t img = 0;
                        for (unsigned i = 0; i < 3 && 3 * g + i < mm; ++i)
                            if (v >> i & 1) img ^= cols[((size_t)r * nsurv + c) * mm + 3 * g + i];
                        e[v >> 2] |= img << 8 * (v & 3);
                    }
                }
        return;                                     // no constant to take out: `fix` stays zero
    }
    for (unsigned r = 0; r < nroots; ++r)
        for (unsigned c = 0; c < nsurv; ++c)
            for (unsigned b = 0; b < mm; ++b)
                tab[((size_t)c * mm + b) * nrp + r] = cols[((size_t)r * nsurv + c) * mm + b] * 0x00010001u;
    for (size_t i = 0; i < (size_t)nsurv * mm; ++i)   // see apply()
        for (unsigned r = 0; r < nrp; ++r) t.fix[r] ^= tab[i * nrp + r] & 0x7fff7fffu;
}

bool update_check(const CodecMath &m, unsigned len, const uint32_t *changed, unsigned nchanged) {
    if (len < 1 || len > m.load || !changed || nchanged < 1 || nchanged > len) return false;
    std::vector<uint8_t> seen(len, 0);
    for (unsigned r = 0; r < nchanged; ++r) {
        if (changed[r] >= len || seen[changed[r]]) return false;
        seen[changed[r]] = 1;
    }
    return true;
}

// The all-parity plan's survivors are the data positions 0 .. len - 1 in order, so survivor column
// c of its matrix is data position c.
bool update_build(const CodecMath &m, unsigned len, const uint32_t *changed, unsigned nchanged,
                  std::vector<uint16_t> &cols) {
    if (!update_check(m, len, changed, nchanged)) return false;
    const unsigned NR = m.spec.nroots, mm = m.spec.mm;
    std::vector<uint32_t> par(NR), surv;
    for (unsigned i = 0; i < NR; ++i) par[i] = len + i;
    std::vector<uint16_t> all;
    if (!recon_build(m, len, par.data(), NR, all, surv)) return false;
    cols.resize((size_t)NR * nchanged * mm);
    for (unsigned i = 0; i < NR; ++i)
        for (unsigned r = 0; r < nchanged; ++r)
            std::copy_n(&all[((size_t)i * len + changed[r]) * mm], mm, &cols[((size_t)i * nchanged + r) * mm]);
    return true;
}

namespace recon {

constexpr unsigned kUnroll = 4;                   // survivors whose loads are in flight together

// V dwords per lane (4: one dwordx4; 1: one dword) or V = 0: one element.
template <typename T, int V>
struct Run {
    static constexpr int ND = V ? V : 1;
    static constexpr unsigned EPL = V ? V * (4 / sizeof(T)) : 1;   // codewords per lane
    static __device__ __forceinline__ void load(const T *p, uint32_t (&x)[ND]) {
        if constexpr (V == 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else if constexpr (V == 1) {
            x[0] = *reinterpret_cast<const uint32_t *>(p);
        } else {
            x[0] = *p;
        }
    }
    static __device__ __forceinline__ void store(T *p, const uint32_t (&x)[ND]) {
        if constexpr (V == 4) *reinterpret_cast<uint4 *>(p) = make_uint4(x[0], x[1], x[2], x[3]);
        else if constexpr (V == 1) *reinterpret_cast<uint32_t *>(p) = x[0];
        else *p = (T)x[0];
    }
};

// The lane map of the frame-in-place kernels: thread t = lane_index() of a launch takes run
// t % runs (epl codewords from codeword j) of frame f = f0 + t / runs.  The threads at and past
// runs * nf have no run: the kernels return on them before they ask (with that test in here
// k_recon<uint8_t, 4, 4> compiles to other registers and another occupancy).
__device__ __forceinline__ size_t lane_index() { return (size_t)blockIdx.x * 256 + threadIdx.x; }
__device__ __forceinline__ void lane(const FrameSpan &a, size_t t, unsigned epl, size_t &f, size_t &j) {
    size_t q;
    if (((t | a.runs) >> 32) == 0) {                // 32-bit division (see shard_row)
        const uint32_t t32 = (uint32_t)t, r32 = (uint32_t)a.runs, f32 = t32 / r32;
        f = f32;
        q = t32 - f32 * r32;
    } else {
        f = t / a.runs;
        q = t - f * a.runs;
    }
    f += a.f0;
    j = a.j0 + q * epl;
}

// Where the symbol rows of a lane's run are: the addressing policy of both kernels, chosen by the
// argument struct A.  Strided (ReconArgs, UpdateArgs): the row at position p is p * sym_stride
// elements past `base`, codeword j of frame f.  Table (ReconPtrArgs, UpdatePtrArgs): one frame, and
// the row is entry e of the pointer table in the kernel arguments, plus j; e is wave-uniform, so
// the pointer comes through a scalar load of the kernarg segment.  Callers name a row both ways and
// the policy takes the one it uses: the position loads of the table form fall away unused.
// Batch (ReconBatchArgs, UpdateBatchArgs): the row at position p of stripe f is entry f * pitch + p
// of a pointer table in device memory, plus j.  The stripe is uniform over a wave (batch_lane), the
// position is a wave-uniform scalar load from the plan's table, and the table is read through the
// constant address space (nothing the call writes may overlap it), so the pointer is one more
// scalar load, dependent on the position's, and never a vector load.
template <class A>
constexpr bool kTable = std::is_same_v<A, ReconPtrArgs> || std::is_same_v<A, UpdatePtrArgs>;
template <class A>
constexpr bool kBatch = std::is_same_v<A, ReconBatchArgs> || std::is_same_v<A, UpdateBatchArgs> ||
                        std::is_same_v<A, ReconMixedArgs> || std::is_same_v<A, UpdateMixedArgs>;

// The lane map of the batch forms.  A stripe takes a.wruns threads, its runs rounded up to a wave,
// so a wave never spans two stripes: wave w of the launch works on stripe s = w / (wruns / 64) of
// the launch (f = f0 + s), and its lane l on run q = (w % (wruns / 64)) * 64 + l.  w is built from
// scalars only and s goes through readfirstlane, so the compiler knows what follows from s to be
// uniform: the stripe's table row and every pointer fetched from it.  false: no run for this
// thread, past the stripe's runs or past the launch's stripes (s stays below 2^32: launch_frames).
template <class A>
__device__ __forceinline__ bool batch_lane(const A &a, unsigned epl, size_t &f, size_t &j) {
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t w = (size_t)blockIdx.x * 4 + wid, wps = a.wruns >> 6;
    uint32_t s, r;                                  // stripe of the launch, wave of the stripe
    if (((w | wps) >> 32) == 0) {                   // 32-bit division, as in lane()
        s = (uint32_t)w / (uint32_t)wps;
        r = (uint32_t)w - s * (uint32_t)wps;
    } else {
        s = (uint32_t)(w / wps);
        r = (uint32_t)(w - (size_t)s * wps);
    }
    s = __builtin_amdgcn_readfirstlane(s);
    r = __builtin_amdgcn_readfirstlane(r);
    const size_t q = (size_t)r * 64 + (threadIdx.x & 63);
    f = a.span.f0 + s;
    j = a.span.j0 + q * epl;
    return s < a.span.nf && q < a.span.runs;
}

template <typename T, class A>
struct At {
    static constexpr bool TABLE = kTable<A>, BATCH = kBatch<A>;
    typedef T *Row;
    typedef __attribute__((address_space(4))) const Row Slot;  // a generic pointer in constant memory
    const A &a;
    size_t f, j;
    T *base;                                        // strided only
    Slot *trow, *nrow;                              // batch only: the stripe's rows of the two tables
    bool live;                                      // batch only: the thread has a run
    __device__ __forceinline__ At(const A &a, size_t t, unsigned epl) : a(a) {
        trow = nrow = nullptr;
        live = true;
        if constexpr (BATCH) {
            live = batch_lane(a, epl, f, j);
            base = nullptr;
            trow = (Slot *)a.table + f * a.pitch;
            if constexpr (std::is_same_v<A, UpdateBatchArgs> || std::is_same_v<A, UpdateMixedArgs>)
                nrow = (Slot *)a.new_table + f * a.new_pitch;
        } else if constexpr (TABLE) {
            f = 0;
            j = a.span.j0 + t * epl;
            base = nullptr;
        } else {
            lane(a.span, t, epl, f, j);
            base = static_cast<T *>(a.span.frames) + f * a.span.frame_pitch + j;
        }
    }
    // batch: the pointer at position pos of the lane's stripe
    __device__ __forceinline__ T *slot(size_t pos) const { return trow[pos]; }
    // Entry e of the table, read where the kernel arguments lie: `a` is the kernels' first argument
    // and the table its last member.  (Indexed as a.tab.p[e], the two largest k_update forms, u16
    // with 32 rows at V = 1 and 0, got a copy of the whole argument struct in scratch, 2680 bytes,
    // and read their pointers from there with vector addresses.)
    __device__ __forceinline__ T *entry(unsigned e) const {
        typedef __attribute__((address_space(4))) const char Arg;
        typedef T *Ptr;                             // a generic pointer that lies in the kernarg segment
        typedef __attribute__((address_space(4))) const Ptr Ent;
        static_assert(alignof(A) == alignof(PtrTable), "the table ends A with no padding after it");
        Arg *const args = (Arg *)__builtin_amdgcn_kernarg_segment_ptr();
        return ((Ent *)(args + (sizeof(A) - sizeof(PtrTable))))[e];
    }
    // the symbol row at position pos, table entry e
    __device__ __forceinline__ T *row(size_t pos, unsigned e) const {
        if constexpr (BATCH) return slot(pos) + j;
        else if constexpr (TABLE) return entry(e) + j;
        else return base + pos * a.span.sym_stride;
    }
    // k_update: the first parity row (strided), parity row r from there, the new symbols of changed[c]
    __device__ __forceinline__ T *parity0() const {
        if constexpr (TABLE || BATCH) return nullptr;
        else return base + (size_t)a.len * a.span.sym_stride;
    }
    __device__ __forceinline__ T *parity(T *par, unsigned r) const {
        if constexpr (BATCH) return slot(a.len + r) + j;
        else if constexpr (TABLE) return entry(a.nchg + r) + j;
        else return par + (size_t)r * a.span.sym_stride;
    }
    __device__ __forceinline__ const T *fresh0() const {
        if constexpr (TABLE || BATCH) return nullptr;
        else return static_cast<const T *>(a.newsyms) + f * a.new_frame_pitch + j;
    }
    __device__ __forceinline__ const T *fresh(const T *nbase, unsigned c) const {
        if constexpr (BATCH) return nrow[c] + j;
        else if constexpr (TABLE) return entry(a.nchg + a.nroots + c) + j;
        else return nbase + (size_t)c * a.new_sym_stride;
    }
};

// One survivor's dwords x into the accumulators of a row block; kp: its columns, bit b at
// kp + b * nrp (KP: a pointer to const uint32_t; in the constant address space for the mixed form).  MB: the symbol bits when known at compile time (the bit loop is then unrolled and
// the columns' scalar loads are issued ahead), else 0 and mm is used.
// bit + 0x7f.. is 0x80.. in the codewords whose bit is set and 0x7f.. in the others, i.e. the mask
// 0xff.. / 0x00.. XOR the constant 0x7f..: one add instead of a shift and a subtract (which the
// compiler turns into a quarter-rate multiply by 0xff).  What the constant adds to an accumulator,
// XOR over all survivors and bits of K & 0x7f.., does not depend on the data: the table carries it
// per row (`fix`) and the kernel takes it out once at the end.
template <int RB, int ND, int MB, class KP>
__device__ __forceinline__ void apply(const uint32_t (&x)[ND], KP __restrict__ kp, unsigned nrp,
                                      unsigned mm, uint32_t ones, uint32_t low, uint32_t (&acc)[RB][ND]) {
    auto bit = [&](unsigned b, KP __restrict__ kb) {
        uint32_t d[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) d[i] = ((x[i] >> b) & ones) + low;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const uint32_t k = kb[r];
#pragma unroll
            for (int i = 0; i < ND; ++i)            // acc ^= d & k as one v_bitop3
                acc[r][i] = __builtin_amdgcn_bitop3_b32(acc[r][i], d[i], k, 0x78);
        }
    };
    if constexpr (MB != 0) {
#pragma unroll
        for (unsigned b = 0; b < MB; ++b) bit(b, kp + (size_t)b * nrp);
    } else {
        for (unsigned b = 0; b < mm; ++b, kp += nrp) bit(b, kp);
    }
}

// The byte form (m <= 8): a GF(2)-linear map of a byte is the XOR of its images on groups of three
// bits, and v_perm_b32 is an 8-entry byte table lookup for the four codewords of a dword at once:
// selector = the group's value in each byte, table = the 8 images of a row (two dwords, kp[2 r] and
// kp[2 r + 1]; group g at kp + g * 2 * nrp).  Three lookups and two XORs (one of them a three-input
// v_bitop3) per row and dword for m = 8, against eight v_bitop3 in the bit-column form, and five
// shared instructions per dword instead of 24.  MB == 8: the three groups unrolled; else a loop
// over the groups of mm bits, bits at and above mm masked out of the selectors.
template <int RB, int ND, int MB, class KP>
__device__ __forceinline__ void apply8(const uint32_t (&x)[ND], KP __restrict__ kp, unsigned nrp,
                                       unsigned mm, uint32_t (&acc)[RB][ND]) {
    if constexpr (MB == 8) {
        uint32_t i0[ND], i1[ND], i2[ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            i0[i] = x[i] & 0x07070707u;
            i1[i] = (x[i] >> 3) & 0x07070707u;
            i2[i] = (x[i] >> 6) & 0x03030303u;
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const uint32_t a0 = kp[2 * r], a1 = kp[2 * r + 1];
            const uint32_t b0 = kp[2 * nrp + 2 * r], b1 = kp[2 * nrp + 2 * r + 1];
            const uint32_t c0 = kp[4 * nrp + 2 * r];
#pragma unroll
            for (int i = 0; i < ND; ++i) {
                const uint32_t p0 = __builtin_amdgcn_perm(a1, a0, i0[i]);
                const uint32_t p1 = __builtin_amdgcn_perm(b1, b0, i1[i]);
                const uint32_t p2 = __builtin_amdgcn_perm(c0, c0, i2[i]);
                acc[r][i] = __builtin_amdgcn_bitop3_b32(acc[r][i], p0, p1, 0x96) ^ p2;   // three-input XOR
            }
        }
    } else {
        for (unsigned g = 0; 3 * g < mm; ++g, kp += 2 * nrp) {
            const unsigned nb = mm - 3 * g < 3 ? mm - 3 * g : 3;
            const uint32_t msk = ((1u << nb) - 1u) * 0x01010101u;
            uint32_t idx[ND];
#pragma unroll
            for (int i = 0; i < ND; ++i) idx[i] = (x[i] >> 3 * g) & msk;
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const uint32_t t0 = kp[2 * r], t1 = kp[2 * r + 1];
#pragma unroll
                for (int i = 0; i < ND; ++i) acc[r][i] ^= __builtin_amdgcn_perm(t1, t0, idx[i]);
            }
        }
    }
}

// Two survivors of m = 8 symbols at once: their six lookups go into an accumulator with three
// three-input XORs (two and a half instructions less per row and dword than one by one).
template <int RB, int ND, class KP>
__device__ __forceinline__ void apply8x2(const uint32_t (&x)[ND], const uint32_t (&y)[ND],
                                         KP __restrict__ kx, KP __restrict__ ky,
                                         unsigned nrp, uint32_t (&acc)[RB][ND]) {
    uint32_t ix[3][ND], iy[3][ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        ix[0][i] = x[i] & 0x07070707u;
        ix[1][i] = (x[i] >> 3) & 0x07070707u;
        ix[2][i] = (x[i] >> 6) & 0x03030303u;
        iy[0][i] = y[i] & 0x07070707u;
        iy[1][i] = (y[i] >> 3) & 0x07070707u;
        iy[2][i] = (y[i] >> 6) & 0x03030303u;
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const uint32_t a0 = kx[2 * r], a1 = kx[2 * r + 1], b0 = kx[2 * nrp + 2 * r], b1 = kx[2 * nrp + 2 * r + 1],
                       c0 = kx[4 * nrp + 2 * r];
        const uint32_t d0 = ky[2 * r], d1 = ky[2 * r + 1], e0 = ky[2 * nrp + 2 * r], e1 = ky[2 * nrp + 2 * r + 1],
                       f0 = ky[4 * nrp + 2 * r];
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            uint32_t v = acc[r][i];
            v = __builtin_amdgcn_bitop3_b32(v, __builtin_amdgcn_perm(a1, a0, ix[0][i]),
                                            __builtin_amdgcn_perm(b1, b0, ix[1][i]), 0x96);
            v = __builtin_amdgcn_bitop3_b32(v, __builtin_amdgcn_perm(c0, c0, ix[2][i]),
                                            __builtin_amdgcn_perm(d1, d0, iy[0][i]), 0x96);
            acc[r][i] = __builtin_amdgcn_bitop3_b32(v, __builtin_amdgcn_perm(e1, e0, iy[1][i]),
                                                    __builtin_amdgcn_perm(f0, f0, iy[2][i]), 0x96);
        }
    }
}

// All nsurv survivors of the lane's run into the accumulators of the row block that starts at row
// r0: kUnroll survivors' loads are issued together, the ragged end goes one by one.
template <typename T, int RB, int V, int MB, class A, class KP>
__device__ __forceinline__ void sweep(const At<T, A> &at, KP __restrict__ K,
                                      unsigned r0, KP __restrict__ surv, unsigned nsurv,
                                      uint32_t (&acc)[RB][Run<T, V>::ND]) {
    using R = Run<T, V>;
    const A &a = at.a;
    constexpr int ND = R::ND;
    constexpr bool BYTES = sizeof(T) == 1;
    const unsigned mm = MB ? MB : a.mm;
    const size_t kstep = BYTES ? (size_t)((mm + 2) / 3) * 2 * a.nrp : (size_t)mm * a.nrp;
    K += BYTES ? 2 * r0 : r0;
    auto one = [&](const uint32_t (&x)[ND], unsigned c) {
        if constexpr (BYTES) apply8<RB, ND, MB>(x, K + c * kstep, a.nrp, mm, acc);
        else apply<RB, ND, MB>(x, K + c * kstep, a.nrp, mm, 0x00010001u, 0x7fff7fffu, acc);
    };
    unsigned c = 0;
    for (; c + kUnroll <= nsurv; c += kUnroll) {
        uint32_t x[kUnroll][ND];
#pragma unroll
        for (unsigned u = 0; u < kUnroll; ++u) R::load(at.row(surv[c + u], c + u), x[u]);
        if constexpr (BYTES && MB == 8) {
#pragma unroll
            for (unsigned u = 0; u < kUnroll; u += 2)
                apply8x2<RB, ND>(x[u], x[u + 1], K + (c + u) * kstep, K + (c + u + 1) * kstep, a.nrp, acc);
        } else {
#pragma unroll
            for (unsigned u = 0; u < kUnroll; ++u) one(x[u], c + u);
        }
    }
    for (; c < nsurv; ++c) {
        uint32_t x[ND];
        R::load(at.row(surv[c], c), x);
        one(x, c);
    }
}

// K: the coefficients; surv / lost: the positions; fix: [nrp] (recon_table).  The mixed form
// (ReconMixedArgs) gets four null pointers and takes all of that per stripe: the stripe f is uniform
// over the wave (batch_lane), so its plan index, the plan's directory entry and from there the four
// parts of the plan's image are dependent scalar loads at the top of the wave; they are read through
// the constant address space, as At::Slot is (nothing the call writes may overlap plan_of or the
// set), and what follows from them stays in scalar registers.  A stripe whose index names no plan
// returns before anything is asked of the pointer table.  RB serves the whole set; the block loop
// runs to the stripe's own rows.
template <typename T, int RB, int V, class A>
__global__ void __launch_bounds__(256) k_recon(A a, const uint32_t *__restrict__ K,
                                               const uint32_t *__restrict__ surv,
                                               const uint32_t *__restrict__ lost,
                                               const uint32_t *__restrict__ fix) {
    using R = Run<T, V>;
    constexpr int ND = R::ND;
    constexpr unsigned W = 8 * sizeof(T);
    const size_t t = lane_index();
    if constexpr (!kBatch<A>)
        if (t >= a.span.runs * a.span.nf) return;
    const At<T, A> at(a, t, R::EPL);
    if constexpr (kBatch<A>)                        // nothing has been asked for yet
        if (!at.live) return;
    unsigned nsurv = a.nsurv, nlost = a.nlost, nrows = a.nrows;
    constexpr bool MIXED = std::is_same_v<A, ReconMixedArgs>;
    typedef __attribute__((address_space(4))) const uint32_t Word;
    std::conditional_t<MIXED, Word *, const uint32_t *> Kt, st, lt, ft;   // the plan's table, by part
    if constexpr (MIXED) {
        const uint32_t pi = __builtin_amdgcn_readfirstlane(((Word *)a.plan_of)[at.f]);
        if (pi >= a.nplans) return;
        Word *const set = (Word *)a.set, *const ent = set + (size_t)pi * (sizeof(ReconSetEntry) / 4);
        nsurv = ent[1];
        nlost = ent[2];
        if (!a.result) nrows = nlost;
        if (!nrows) return;
        Kt = set + ent[0];
        st = set + ent[3];
        lt = st + nsurv;
        ft = lt + nlost;
    } else {
        Kt = K;
        st = surv;
        lt = lost;
        ft = fix;
    }
    uint32_t bad[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) bad[d] = 0;
    for (unsigned r0 = 0; r0 < nrows; r0 += RB) {
        uint32_t acc[RB][ND];
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int d = 0; d < ND; ++d) acc[r][d] = 0;
        if (a.mm == 8) sweep<T, RB, V, 8>(at, Kt, r0, st, nsurv, acc);
        else sweep<T, RB, V, 0>(at, Kt, r0, st, nsurv, acc);
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const unsigned row = r0 + r;
            const uint32_t fx = ft[row];
#pragma unroll
            for (int d = 0; d < ND; ++d) acc[r][d] ^= fx;
            if (row < nlost) {
                if constexpr (kTable<A>) {          // a null entry: that shard is not wanted
                    if (at.entry(nsurv + row)) R::store(at.row(0, nsurv + row), acc[r]);
                } else if constexpr (kBatch<A>) {   // ... by this stripe
                    if (at.slot(lt[row])) R::store(at.row(lt[row], 0), acc[r]);
                } else {
                    R::store(at.row(lt[row], 0), acc[r]);
                }
            } else {                                // check rows; the padding rows are zero
#pragma unroll
                for (int d = 0; d < ND; ++d) bad[d] |= acc[r][d];
            }
        }
    }
    if (a.result) {
        int32_t *res = a.result + at.f * a.span.depth + at.j;
        constexpr unsigned EPD = V ? 4 / sizeof(T) : 1;
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (unsigned e = 0; e < EPD; ++e) {
                const uint32_t v = V ? (bad[d] >> (W * e)) & ((1u << W) - 1u) : bad[d];
                res[d * EPD + e] = v ? -1 : (int32_t)nlost;
            }
    }
}

// ---- in-place parity update (ezrs_update_interleaved) ---------------------------------------------
// The delta form: parity ^= G[:, changed] * (new ^ old).  The plan table is recon_table with the
// changed positions as the survivors, so the deltas go through apply / apply8 / apply8x2 like
// survivors do.  Where the registers allow it the accumulators start as the old parity instead of
// zero, which puts the parity loads in flight with the data loads; else the old parity is read
// where it is stored.  Either way its bits above the symbol stay as they were (the columns are
// symbols, and so is `fix`).

// N changed positions from c0: the old and the new symbols, loaded together; d = old ^ new.  KP,
// here and below: the pointer type of the plan's table, as in sweep.
template <typename T, int V, int N, class A, class KP>
__device__ __forceinline__ void udelta(const At<T, A> &at, const T *nbase,
                                       KP __restrict__ chg, unsigned c0,
                                       uint32_t (&d)[N][Run<T, V>::ND], uint32_t (&nw)[N][Run<T, V>::ND]) {
    using R = Run<T, V>;
#pragma unroll
    for (int u = 0; u < N; ++u) {
        R::load(at.row(chg[c0 + u], c0 + u), d[u]);
        R::load(at.fresh(nbase, c0 + u), nw[u]);
    }
#pragma unroll
    for (int u = 0; u < N; ++u)
#pragma unroll
        for (int i = 0; i < R::ND; ++i) d[u][i] ^= nw[u][i];
}

// The N deltas of the positions from c0 into the accumulators of a row block; K: the coefficients,
// already at the block's first row.  m = 8 takes them in pairs.
template <typename T, int RB, int V, int MB, int N, class KP>
__device__ __forceinline__ void ufeed(const UpdateArgs &a, KP __restrict__ K, unsigned c0,
                                      const uint32_t (&d)[N][Run<T, V>::ND],
                                      uint32_t (&acc)[RB][Run<T, V>::ND]) {
    constexpr int ND = Run<T, V>::ND;
    constexpr bool BYTES = sizeof(T) == 1;
    const unsigned mm = MB ? MB : a.mm;
    const size_t kstep = BYTES ? (size_t)((mm + 2) / 3) * 2 * a.nrp : (size_t)mm * a.nrp;
    auto one = [&](const uint32_t (&x)[ND], unsigned c) {
        if constexpr (BYTES) apply8<RB, ND, MB>(x, K + c * kstep, a.nrp, mm, acc);
        else apply<RB, ND, MB>(x, K + c * kstep, a.nrp, mm, 0x00010001u, 0x7fff7fffu, acc);
    };
    if constexpr (BYTES && MB == 8) {
#pragma unroll
        for (int u = 0; u + 1 < N; u += 2)
            apply8x2<RB, ND>(d[u], d[u + 1], K + (c0 + u) * kstep, K + (c0 + u + 1) * kstep, a.nrp, acc);
        if constexpr (N & 1) one(d[N - 1], c0 + N - 1);
    } else {
#pragma unroll
        for (int u = 0; u < N; ++u) one(d[u], c0 + u);
    }
}

// The changed positions of the lane's stripe: the plan's, or in the mixed form the stripe's own plan's
// (nchg, from the directory).  The one-plan forms read a.nchg where they use it, as they did before
// there was a mixed form: with a copy handed down instead, seven of them compiled to other streams.
template <class A>
__device__ __forceinline__ unsigned changed_count(const A &a, unsigned nchg) {
    if constexpr (std::is_same_v<A, UpdateMixedArgs>) return nchg;
    else return a.nchg;
}

// By the accumulator registers of a row block (RB x dwords of the run), what keeps every
// instantiation clear of spills and all but the two largest at four or more waves per SIMD
// (resource report in DESIGN section 4): whether the old parity is loaded ahead of the arithmetic
// (else it is read where it is stored), how many changed positions' loads (old and new) are issued
// together, and at most how many deltas stay in registers.
constexpr bool uearly(int accs) { return accs < 64; }
constexpr int ugroup(int accs) { return accs >= 128 ? 2 : (int)kUnroll; }
constexpr unsigned ukeep(int accs) { return accs >= 128 ? 1 : accs >= 64 ? 2 : kUnroll; }

// One row block.  NC != 0: the plan's NC deltas are in d.  NC == 0: all nchg changed positions are
// read (again), a group's loads issued together, the ragged end one by one.
template <typename T, int RB, int V, int MB, int NC, class A, class KP>
__device__ __forceinline__ void usweep(const At<T, A> &at, const T *nbase,
                                       KP __restrict__ chg, unsigned nchg, KP __restrict__ K,
                                       const uint32_t (&d)[NC ? NC : 1][Run<T, V>::ND],
                                       uint32_t (&acc)[RB][Run<T, V>::ND]) {
    constexpr int ND = Run<T, V>::ND, G = ugroup(RB * ND);
    const A &a = at.a;
    if constexpr (NC != 0) {
        ufeed<T, RB, V, MB, NC>(a, K, 0, d, acc);
    } else {
        unsigned c = 0;
        for (; c + G <= changed_count(a, nchg); c += G) {
            uint32_t e[G][ND], w[G][ND];
            udelta<T, V, G>(at, nbase, chg, c, e, w);
            ufeed<T, RB, V, MB, G>(a, K, c, e, acc);
        }
        for (; c < changed_count(a, nchg); ++c) {
            uint32_t e[1][ND], w[1][ND];
            udelta<T, V, 1>(at, nbase, chg, c, e, w);
            ufeed<T, RB, V, MB, 1>(a, K, c, e, acc);
        }
    }
}

// A lane's codewords through every row block.  NC = 1 .. kUnroll changed positions of a plan of one
// row block: the new symbols stay in registers from the delta to the write-back.  NC = 0, any plan:
// every block reads old and new again (mostly from L2), and the new symbols once more at the end.
// (Deltas kept across several blocks are not built: the compiler then hoists every bit mask and
// selector of every delta out of the block loop and the kernels need 160 - 256 VGPRs.)  Either way
// the data is overwritten only after the last block.
template <typename T, int RB, int V, int NC, class A, class KP>
__device__ __forceinline__ void ubody(const At<T, A> &at, KP __restrict__ K, KP __restrict__ chg,
                                      unsigned nchg, KP __restrict__ fix, const T *nbase) {
    using R = Run<T, V>;
    constexpr int ND = R::ND;
    const A &a = at.a;
    T *const par = at.parity0();
    uint32_t d[NC ? NC : 1][ND], nw[NC ? NC : 1][ND];
    if constexpr (NC != 0) udelta<T, V, NC>(at, nbase, chg, 0, d, nw);
    auto block = [&](unsigned r0) {
        uint32_t acc[RB][ND];
        if constexpr (uearly(RB * ND)) {
            // The accumulators start as the old parity, whose loads are so in flight with the data
            // loads.  The rows of a last block's padding start as the last parity row once more (no
            // load leaves the stripe, and no control flow on the way to the arithmetic); they are
            // never stored.
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const unsigned row = r0 + r < a.nroots ? r0 + r : a.nroots - 1;
                R::load(at.parity(par, row), acc[r]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < RB; ++r)
#pragma unroll
                for (int i = 0; i < ND; ++i) acc[r][i] = 0;
        }
        const KP Kb = K + (sizeof(T) == 1 ? 2 * r0 : r0);
        if (a.mm == 8) usweep<T, RB, V, 8, NC>(at, nbase, chg, nchg, Kb, d, acc);
        else usweep<T, RB, V, 0, NC>(at, nbase, chg, nchg, Kb, d, acc);
#pragma unroll
        for (int r = 0; r < RB; ++r)
            if (r0 + r < a.nroots) {
                T *const p = at.parity(par, r0 + r);
                const uint32_t fx = fix[r0 + r];
                if constexpr (uearly(RB * ND)) {
#pragma unroll
                    for (int i = 0; i < ND; ++i) acc[r][i] ^= fx;
                } else {
                    uint32_t old[ND];
                    R::load(p, old);
#pragma unroll
                    for (int i = 0; i < ND; ++i) acc[r][i] ^= fx ^ old[i];
                }
                R::store(p, acc[r]);
            }
    };
    if constexpr (NC != 0) {
        block(0);
#pragma unroll
        for (int u = 0; u < NC; ++u) R::store(at.row(chg[u], u), nw[u]);
    } else {
        for (unsigned r0 = 0; r0 < a.nroots; r0 += RB) block(r0);
        for (unsigned c = 0; c < changed_count(a, nchg); ++c) {
            uint32_t x[ND];
            R::load(at.fresh(nbase, c), x);
            R::store(at.row(chg[c], c), x);
        }
    }
}

// K: the coefficients of the changed positions; chg: the positions; fix: [nrp] (recon_table).  The
// mixed form (UpdateMixedArgs) gets three null pointers and takes all of that, and the number of
// changed positions, per stripe, as k_recon's mixed form does: the plan index, the plan's directory
// entry and the parts of the plan's image are dependent scalar loads through the constant address
// space at the top of the wave (nothing the call writes may overlap plan_of or the set; the NC = 0
// body reads the image and the pointer tables again after its first parity stores).  A stripe whose
// index names no plan returns before anything is asked of either pointer table.  RB serves the whole
// set, NROOTS being the same for all its plans; whether the deltas stay in registers is decided per
// stripe, a wave-uniform branch to one of the bodies below.
template <typename T, int RB, int V, class A>
__global__ void __launch_bounds__(256) k_update(A a, const uint32_t *__restrict__ K,
                                                const uint32_t *__restrict__ chg,
                                                const uint32_t *__restrict__ fix) {
    using R = Run<T, V>;
    const size_t t = lane_index();
    if constexpr (!kBatch<A>)
        if (t >= a.span.runs * a.span.nf) return;
    const At<T, A> at(a, t, R::EPL);
    if constexpr (kBatch<A>)                        // nothing has been asked for yet
        if (!at.live) return;
    constexpr bool MIXED = std::is_same_v<A, UpdateMixedArgs>;
    // the mixed form's count (changed_count), set below.  Its initial value is never used; started
    // from 0 instead, five mixed forms took more registers (u8 RB = 4 at V = 1: 53 against 32; both
    // sets of figures are in profiles/recon/isa_stats_update_mixed.txt).  Only registers hang on it.
    unsigned nchg = MIXED ? a.nchg : 0;
    typedef __attribute__((address_space(4))) const uint32_t Word;
    std::conditional_t<MIXED, Word *, const uint32_t *> Kt, ct, ft;   // the plan's table, by part
    if constexpr (MIXED) {
        const uint32_t pi = __builtin_amdgcn_readfirstlane(((Word *)a.plan_of)[at.f]);
        if (pi >= a.nplans) return;
        // (off, nchg, nroots, pos): an update plan's image has survivors = changed, lost = the parity
        Word *const set = (Word *)a.set, *const ent = set + (size_t)pi * (sizeof(ReconSetEntry) / 4);
        nchg = ent[1];
        Kt = set + ent[0];
        ct = set + ent[3];
        ft = ct + nchg + a.nroots;
    } else {
        Kt = K;
        ct = chg;
        ft = fix;
    }
    const T *const nbase = at.fresh0();
    static_assert(kUnroll == 4, "one case per count of changed positions kept in registers");
    constexpr unsigned KEEP = ukeep(RB * R::ND);
    const unsigned nc = a.nroots <= RB && changed_count(a, nchg) <= KEEP ? changed_count(a, nchg) : 0;
    if (nc == 1) {
        ubody<T, RB, V, 1>(at, Kt, ct, nchg, ft, nbase);
    } else if (nc == 2) {
        if constexpr (KEEP >= 2) ubody<T, RB, V, 2>(at, Kt, ct, nchg, ft, nbase);
    } else if (nc == 3) {
        if constexpr (KEEP >= 4) ubody<T, RB, V, 3>(at, Kt, ct, nchg, ft, nbase);
    } else if (nc == 4) {
        if constexpr (KEEP >= 4) ubody<T, RB, V, 4>(at, Kt, ct, nchg, ft, nbase);
    } else {
        ubody<T, RB, V, 0>(at, Kt, ct, nchg, ft, nbase);
    }
}

// Rows per block of a plan of nrows rows: 4, 8, 16 and, for 16-bit symbols only, 32.  The byte form
// stops at 16 (at 32 its 192 table dwords per survivor no longer fit the scalar registers and the
// kernel ran 1.5 x slower than two passes of 16).
template <typename T>
static unsigned rows_per_block(unsigned nrows) {
    const unsigned cap = sizeof(T) == 1 ? 16 : 32;
    unsigned rb = 4;
    while (rb < cap && rb < nrows) rb *= 2;
    return rb;
}

// f(RB) with the row block rb as a compile-time constant.
template <typename T, class F>
static void with_rb(unsigned rb, F &&f) {
    switch (rb) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default:                                        // 32 rows: the bit-column form only (rows_per_block)
        if constexpr (sizeof(T) == 2) f(std::integral_constant<int, 32>{});
        break;
    }
}

// Every codeword of every frame through a frame-in-place kernel.  a: the kernel's arguments, its
// FrameSpan `span` filled in per launch here; al: what else than the frames has to be aligned for a
// vector access, OR-ed (addresses and byte strides; the batch forms: the alignment promised for the
// tables' pointers); kernel(RB, V, grid, a): launches the kernel's <T, RB, V> form.  A frame takes
// one thread per run, in the batch forms rounded up to a wave.
template <typename T, class A, class F>
static hipError_t launch_frames(A a, size_t nframes, unsigned rb, size_t al, F &&kernel) {
    FrameSpan &sp = a.span;
    // codewords [j0, j0 + n) of every frame, Run<T, V>::EPL per lane
    auto span = [&](auto V, size_t j0, size_t n) -> hipError_t {
        if (!n) return hipSuccess;
        sp.j0 = j0;
        sp.runs = n / Run<T, decltype(V)::value>::EPL;
        const size_t maxt = (size_t)1 << 38;        // threads per launch (2^30 workgroups)
        if (sp.runs > maxt) return hipErrorInvalidValue;
        size_t tpf = sp.runs;                       // threads per frame
        if constexpr (kBatch<A>) a.wruns = tpf = (sp.runs + 63) / 64 * 64;   // batch_lane
        size_t fstep = maxt / tpf;
        if constexpr (kBatch<A>)                    // a launch's stripe index and the few past it: 32 bits
            if (fstep > (size_t)1 << 31) fstep = (size_t)1 << 31;
        for (size_t f0 = 0; f0 < nframes; f0 += fstep) {
            sp.f0 = f0;
            sp.nf = nframes - f0 < fstep ? nframes - f0 : fstep;
            const dim3 grid((unsigned)((tpf * sp.nf + 255) / 256));
            with_rb<T>(rb, [&](auto RB) { kernel(RB, V, grid, a); });
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    // widest access every symbol row of every frame is aligned for
    const size_t w = sizeof(T);
    al |= (size_t)(uintptr_t)sp.frames | sp.sym_stride * w;
    if (nframes > 1) al |= sp.frame_pitch * w;
    const size_t e16 = 16 / w, e4 = 4 / w;
    size_t done = 0;
    hipError_t e = hipSuccess;
    if ((al & 15) == 0 && sp.depth >= e16) {
        done = sp.depth / e16 * e16;
        e = span(std::integral_constant<int, 4>{}, 0, done);
    } else if ((al & 3) == 0 && sp.depth >= e4) {
        done = sp.depth / e4 * e4;
        e = span(std::integral_constant<int, 1>{}, 0, done);
    }
    if (e == hipSuccess) e = span(std::integral_constant<int, 0>{}, done, sp.depth - done);   // ragged end
    return e;
}

// A: the addressing; al: the OR of the addresses the table form uses (0 for the strided form, whose
// frames and strides launch_frames looks at itself)
template <typename T, class A>
static hipError_t launch_recon(const A &a, size_t nframes, size_t al, const DevTable &t, hipStream_t s) {
    return launch_frames<T>(a, nframes, rows_per_block<T>(a.nrows), al,
                            [&](auto RB, auto V, dim3 grid, const A &b) {
        hipLaunchKernelGGL((k_recon<T, decltype(RB)::value, decltype(V)::value, A>), grid, dim3(256), 0, s, b,
                           t.K, t.pos, t.lost, t.fix);
    });
}

template <typename T, class A>
static hipError_t launch_update(const A &a, size_t nframes, size_t al, const DevTable &t, hipStream_t s) {
    // `newsyms` is accessed like the frames (null and 0 in the table form)
    al |= (size_t)(uintptr_t)a.newsyms | a.new_sym_stride * sizeof(T);
    if (nframes > 1) al |= a.new_frame_pitch * sizeof(T);
    return launch_frames<T>(a, nframes, rows_per_block<T>(a.nroots), al,
                            [&](auto RB, auto V, dim3 grid, const A &b) {
        hipLaunchKernelGGL((k_update<T, decltype(RB)::value, decltype(V)::value, A>), grid, dim3(256), 0, s, b,
                           t.K, t.pos, t.fix);
    });
}

} // namespace recon

namespace {

template <class A>
hipError_t recon_any(const A &a, size_t nframes, size_t al, const DevTable &t, hipStream_t s) {
    if (!a.nrows || !nframes) return hipSuccess;
    return a.mm <= 8 ? recon::launch_recon<uint8_t>(a, nframes, al, t, s)
                     : recon::launch_recon<uint16_t>(a, nframes, al, t, s);
}

template <class A>
hipError_t update_any(const A &a, size_t nframes, size_t al, const DevTable &t, hipStream_t s) {
    if (!a.nchg || !nframes) return hipSuccess;
    return a.mm <= 8 ? recon::launch_update<uint8_t>(a, nframes, al, t, s)
                     : recon::launch_update<uint16_t>(a, nframes, al, t, s);
}

} // namespace

hipError_t launch_recon(const ReconArgs &a, size_t nframes, const DevTable &t, hipStream_t s) {
    return recon_any(a, nframes, 0, t, s);
}
hipError_t launch_update(const UpdateArgs &a, size_t nframes, const DevTable &t, hipStream_t s) {
    return update_any(a, nframes, 0, t, s);
}
hipError_t launch_recon(const ReconPtrArgs &a, size_t al, const DevTable &t, hipStream_t s) {
    return recon_any(a, 1, al, t, s);
}
hipError_t launch_update(const UpdatePtrArgs &a, size_t al, const DevTable &t, hipStream_t s) {
    return update_any(a, 1, al, t, s);
}
hipError_t launch_recon(const ReconBatchArgs &a, size_t nstripes, size_t al, const DevTable &t, hipStream_t s) {
    return recon_any(a, nstripes, al, t, s);
}
hipError_t launch_update(const UpdateBatchArgs &a, size_t nstripes, size_t al, const DevTable &t, hipStream_t s) {
    return update_any(a, nstripes, al, t, s);
}
hipError_t launch_recon(const ReconMixedArgs &a, size_t nstripes, size_t al, hipStream_t s) {
    return recon_any(a, nstripes, al, DevTable{}, s);   // !a.nrows: no result and no plan that rebuilds
}
hipError_t launch_update(const UpdateMixedArgs &a, size_t nstripes, size_t al, hipStream_t s) {
    return update_any(a, nstripes, al, DevTable{}, s);  // a.nchg: the set's largest, never 0
}

} // namespace ezrs

extern "C" int ezrs_recon_bitmatrix(unsigned symbol_bits, unsigned poly, unsigned fcr, unsigned prim,
                                    unsigned nroots, int dual, unsigned len, const uint32_t *lost,
                                    unsigned nlost, uint16_t *cols, size_t cols_cap, uint32_t *survivors) {
    using namespace ezrs;
    if (!cols || !survivors) return -EINVAL;
    CodecMath m;
    if (!m.build(CodecSpec{symbol_bits, poly, fcr, prim, nroots, dual ? 1 : 0})) return -EINVAL;
    if (!recon_check(m, len, lost, nlost)) return -EINVAL;
    const size_t nsurv = (size_t)len + nroots - nlost;
    if (cols_cap < (size_t)nroots * nsurv * symbol_bits) return -EINVAL;
    try {
        std::vector<uint16_t> c;
        std::vector<uint32_t> sv;
        if (!recon_build(m, len, lost, nlost, c, sv)) return -EINVAL;
        std::copy(c.begin(), c.end(), cols);
        std::copy(sv.begin(), sv.end(), survivors);
    } catch (const std::bad_alloc &) {
        return -ENOMEM;
    }
    return 0;
}
