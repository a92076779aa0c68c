// ezrs_internal.hpp -- shared declarations of the MI355X RS engine (not part of the C ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/ezrs.h"
#include "ezrs_field.hpp"

namespace ezrs {

// hipMemcpy2DAsync moves each row separately; when both pitches equal the row width the region
// is contiguous and goes as one linear copy.
inline hipError_t copy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width,
                         size_t height, hipMemcpyKind kind, hipStream_t st) {
    if (height == 1 || (dpitch == width && spitch == width))
        return hipMemcpyAsync(dst, src, width * height, kind, st);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, st);
}

// Everything a kernel needs to know about a codec, passed by value at launch.
struct DevCodec {
    unsigned mm, nn, nroots, load, fcr, prim, iprim, poly;
    int dual;
    int masked;                   // symbol narrower than its datum (rs_base:1194)
    int ncu;                      // compute units of the device (persistent grids)
    size_t launch_rows;           // test hook (ezrs_set_launch_rows): codewords per plane-sliced
                                  // launch, 0 = the largest batch whose 32-bit offsets fit
    int karn;                     // decode with Phil Karn's libfec semantics (ezrs_set_semantics):
                                  // erasures and positions in the full NN frame, none of ezpwd's
                                  // extra failure checks (fec-3.0.1/decode_rs.h:71-298)
    const uint16_t *alpha_to;     // device, nn+1
    const uint16_t *index_of;     // device, nn+1
    const uint16_t *genpoly;      // device, nroots+1 (index form)
    const uint8_t *into_dual;     // device, 256
    const uint8_t *from_dual;     // device, 256
};

// Bytes of the codec's datum (uint8_t symbols up to 8 bits, uint16_t above).
inline unsigned sym_bytes(const DevCodec &d) { return d.mm <= 8 ? 1 : 2; }

// Shard batches (ezrs_encode_shards / ezrs_decode_shards): codeword k is row j = k mod rows of
// shard s = k / rows, at element offset s * pitch + j * stride; every row holds `len` data symbols
// and its parity, except the shard's last row, which holds `tail` data symbols (a shortened
// codeword) and its parity.  rows == 0: a plain batch (row k at k * stride).
struct Shards {
    uint32_t rows = 0;
    uint32_t tail = 0;
    size_t pitch = 0;
};

// Element offset and data length of row k.
__host__ __device__ __forceinline__ size_t shard_row(const Shards &g, size_t k, size_t stride, unsigned len,
                                                     unsigned &rlen) {
    if (!g.rows) {
        rlen = len;
        return k * stride;
    }
    size_t s, j;
    if ((k >> 32) == 0) {                           // 32-bit division (the device's 64-bit one is a
        const uint32_t k32 = (uint32_t)k, s32 = k32 / g.rows;     // long software sequence)
        s = s32;
        j = k32 - s32 * g.rows;
    } else {
        s = k / g.rows;
        j = k - s * g.rows;
    }
    rlen = j + 1 == g.rows ? g.tail : len;
    return s * g.pitch + j * stride;
}

// Arguments of one batch decode (strides in elements).
struct DecodeArgs {
    void *data;
    size_t data_stride;
    unsigned len;
    void *parity;                 // never null here: the C ABI resolves parity == NULL
    size_t parity_stride;
    const uint32_t *eras;
    size_t eras_stride;
    const uint32_t *neras;
    int32_t *result;
    uint32_t *positions;
    size_t pos_stride;
    void *corr;
    size_t corr_stride;
    size_t ncw;
    Shards sh{};                  // sh.rows != 0: shard rows, parity inline (data + row length)
    // plane-sliced path: the syndrome kernel stores flag_gen into *flag_word when it flags a
    // codeword, and the error path skips its screen when the word holds another value (and no
    // erasures are given): nothing was flagged by this call
    uint32_t *flag_word = nullptr;
    uint32_t flag_gen = 0;
};

struct EncodeArgs {
    const void *data;
    size_t data_stride;
    unsigned len;
    void *parity;
    size_t parity_stride;
    size_t ncw;
    Shards sh{};                  // sh.rows != 0: shard rows, parity inline (data + row length)
};

// Row k's data and parity pointers and data length (plain batches: the strided arrays; shard
// batches: the row, its parity right after its data).
template <typename T, typename P, class A>
__host__ __device__ __forceinline__ void row_ptrs(const A &a, size_t k, P *&data, T *&parity, unsigned &len) {
    if (!a.sh.rows) {
        len = a.len;
        data = static_cast<P *>(a.data) + k * a.data_stride;
        parity = static_cast<T *>(a.parity) + k * a.parity_stride;
        return;
    }
    const size_t off = shard_row(a.sh, k, a.data_stride, a.len, len);
    data = static_cast<P *>(a.data) + off;
    parity = const_cast<T *>(reinterpret_cast<const T *>(data)) + len;
}

// Generic per-codeword kernels (ezrs_generic.hip): every codec, every length.
hipError_t launch_encode_generic(const DevCodec &c, const EncodeArgs &a, hipStream_t s);
hipError_t launch_decode_generic(const DevCodec &c, const DecodeArgs &a, hipStream_t s);
// Syndrome workspace layouts the error path reads.  Rows: [ncw][32] bytes (bit-sliced kernels).
// Tiled (plane-sliced kernels): codeword k's syndrome j at (k / 256) * kSynTile + 256 j + k % 256,
// so the syndrome kernel stores four codewords' syndrome j as one dword and the error path's loads
// of one syndrome across a wavefront's codewords fall in one or two cache lines.
constexpr size_t kSynTile = 256 * 32;
enum class SynLayout { Rows, Tiled };
// Error path behind the sliced syndrome kernels: decodes the codewords whose result holds the
// sentinel, starting from the syndromes in syn_ws.
hipError_t launch_decode_flagged(const DevCodec &c, const DecodeArgs &a, const uint8_t *syn_ws,
                                 SynLayout layout, hipStream_t s);

// Bit-sliced GF(2^8) kernels (ezrs_bitslice.hip) for the codecs of gen/ezrs_bs_tables.inc.
int bitslice_codec_id(const DevCodec &d);   // -1 if the codec has no bit-sliced path
// Encode needs a workspace of bs_encode_ws_bytes(ncw) device bytes.
size_t bs_encode_ws_bytes(size_t ncw);
hipError_t launch_bs_encode(int id, const DevCodec &d, const EncodeArgs &a, void *ws, hipStream_t s);
hipError_t launch_bs_syndromes(int id, const DevCodec &d, const DecodeArgs &a, uint8_t *syn_ws,
                               hipStream_t s);

// Plane-sliced GF(2^8) kernels (ezrs_ps.hip) for the codecs of gen/ezrs_ps_tables.inc: row pitch
// <= 256 bytes; decode needs the parity inside the row.
int planeslice_codec_id(const DevCodec &d);   // -1 if the codec has no plane-sliced path
size_t ps_ws_bytes(size_t ncw);
bool ps_can_encode(const DevCodec &d, const EncodeArgs &a);
bool ps_can_decode(const DevCodec &d, const DecodeArgs &a);
hipError_t launch_ps_encode(int id, const DevCodec &d, const EncodeArgs &a, void *ws, hipStream_t s);
hipError_t launch_ps_syndromes(int id, const DevCodec &d, const DecodeArgs &a, uint8_t *syn_ws,
                               hipStream_t s);

// GF(2^16) kernels (ezrs_wide.hip) for the codecs of gen/ezrs_wide_tables.inc: remainder networks
// + syndrome/parity finish + wavefront-per-codeword error path.  Decode needs inline parity.
int wide_codec_id(const DevCodec &d);        // -1 if the codec has no wide fast path
size_t wide_ws_bytes(int id, size_t ncw);
// blob: syndrome leader slots [32] | log beta [32] | log Q [NR][NR] (host copy; the Q part is
// also uploaded to the device)
bool wide_build_consts(int id, const CodecMath &m, std::vector<uint16_t> &blob);
size_t wide_cols_count(unsigned nroots);   // u16 entries of the device column tables (blob + 64)
bool wide_can_encode(const DevCodec &d, const EncodeArgs &a);
bool wide_can_decode(const DevCodec &d, const DecodeArgs &a);
hipError_t launch_wide_encode(int id, const DevCodec &d, const EncodeArgs &a, const uint16_t *blob_host,
                              const uint16_t *cols_dev, void *ws, hipStream_t s);
hipError_t launch_wide_decode(int id, const DevCodec &d, const DecodeArgs &a, const uint16_t *blob_host,
                              const uint16_t *cols_dev, void *ws, hipStream_t s);

// Interleaved frames (ezrs_interleave.hip; ezrs_encode_interleaved / ezrs_decode_interleaved):
// symbol s of codeword k = f * depth + j is element f * frame_pitch + s * sym_stride + j of
// `frames`.  The kernels copy symbols [s0, s1) of codewords k0 .. k0 + n - 1 between the frames and
// packed rows (row k - k0 at rows + (k - k0) * row_pitch, symbol s at column s), so the row kernels
// run unchanged on the staged rows.  Elements are the codec's datum; strides in elements.
struct IlArgs {
    void *frames;
    size_t frame_pitch, sym_stride, depth;
    void *rows;                   // 16-byte aligned; il_stage_bytes() bytes
    size_t row_pitch;
    size_t k0;                    // first codeword (frame-major index over the whole batch)
    uint32_t n;                   // codewords (<= kIlMaxRows)
    uint32_t s0, s1;              // symbols to copy
    const int32_t *result;        // scatter: null = every codeword, else only those with
                                  // result[k - k0] != 0 (the others are never written)
};
constexpr size_t kIlTile = 256;                   // codewords per workgroup (the row kernels' tile)
constexpr size_t kIlMaxRows = (size_t)1 << 31;    // per launch
// Staging bytes of n rows (the scatter's aligned dword loads may read a few bytes past the last row).
inline size_t il_stage_bytes(size_t n, size_t row_pitch, size_t w) {
    return (n * row_pitch * w + 32 + 255) & ~(size_t)255;
}
hipError_t launch_il_gather(const DevCodec &d, const IlArgs &a, hipStream_t s);
hipError_t launch_il_scatter(const DevCodec &d, const IlArgs &a, hipStream_t s);
// The pointer policy of the same two kernels (ezrs_decode_ptrs / ezrs_decode_ptrs_batch): frames
// (stripes) whose symbol rows are buffers of their own, named by a pointer table in DEVICE memory
// that the kernels read while they run.  Symbol s of codeword k = f * depth + j is element j of the
// buffer table[f * pitch + s]; frames is null, frame_pitch and sym_stride are 0, depth is the shard
// length.  al: what every pointer of the table is a multiple of (the caller's promise, or the OR of
// the addresses).
struct IlPtrArgs : IlArgs {
    void *const *table;
    size_t pitch;
};
hipError_t launch_il_gather(const DevCodec &d, const IlPtrArgs &a, size_t al, hipStream_t s);
hipError_t launch_il_scatter(const DevCodec &d, const IlPtrArgs &a, size_t al, hipStream_t s);
// The selection policy of the same two kernels (ezrs_decode_ptrs_select /
// ezrs_decode_interleaved_select), over either of the policies B above: staged row i of the call is
// codeword sel[i] of the ncw = nframes * depth codewords that B addresses, so k0 and n count rows of
// `sel` (and of `result`), not codewords of the batch.  A row is skipped when i >= count[0] (count
// non-null) or sel[i] >= ncw: the gather stages it as zeros and reads nothing for it, the scatter
// never writes it.  sel and count are DEVICE memory, read while the kernels run.  Element path only:
// neighbouring rows are not neighbouring codewords.
template <class B>
struct IlSel : B {
    const uint64_t *sel;
    const uint64_t *count;
    size_t ncw;
};
hipError_t launch_il_gather(const DevCodec &d, const IlSel<IlPtrArgs> &a, bool ptrs, hipStream_t s);
hipError_t launch_il_scatter(const DevCodec &d, const IlSel<IlPtrArgs> &a, bool ptrs, hipStream_t s);

// Order-preserving compaction of the failed codewords of a result array (ezrs_select.hip;
// ezrs_select_failed): sel[0 .. min(total, cap) - 1] = base + k for the k < n with result[k] < 0,
// ascending, the rest of sel[0 .. cap - 1] = EZRS_SEL_NONE, *count = total.  Three kernels on the
// stream (counts per chunk of kSelChunk results, their scan, the write); ws: select_ws_bytes(n).
constexpr size_t kSelChunk = 4096;
inline size_t select_ws_bytes(size_t n) { return (n / kSelChunk + (n % kSelChunk != 0)) * sizeof(uint64_t); }
hipError_t launch_select_failed(const int32_t *result, size_t n, uint64_t base, uint64_t *sel, size_t cap,
                                uint64_t *count, void *ws, hipStream_t s);

// Shared-erasure reconstruction of interleaved frames (ezrs_recon.hip; ezrs_recon_create /
// ezrs_reconstruct_interleaved): one constant GF matrix per loss pattern, applied to the survivors
// in place.  recon_build: the matrix as bit columns, cols[row][survivor][bit] (rows 0..nlost-1
// rebuild lost[0..nlost-1], the others are check rows), and the surviving positions, ascending;
// false for a bad length or loss list (recon_check).  recon_table: the device table of a plan,
// coefficients | survivors | lost | the per-row constant the kernel takes out of its accumulators
// at the end (table_view: the four parts from the table's base); coefficients for m > 8:
// [survivor][bit][recon_row_pad(nroots)] columns replicated across a dword, for m <= 8:
// [survivor][group of 3 bits][recon_row_pad(nroots)][2] dwords, the images of the group's 8 values
// as bytes.
bool recon_check(const CodecMath &m, unsigned len, const uint32_t *lost, unsigned nlost);
bool recon_build(const CodecMath &m, unsigned len, const uint32_t *lost, unsigned nlost,
                 std::vector<uint16_t> &cols, std::vector<uint32_t> &surv);
unsigned recon_row_pad(unsigned nroots);
size_t recon_coef_words(unsigned mm, unsigned nroots, unsigned nsurv);
size_t recon_table_words(unsigned mm, unsigned nroots, unsigned nsurv, unsigned nlost);
void recon_table(unsigned mm, unsigned nroots, const std::vector<uint16_t> &cols,
                 const std::vector<uint32_t> &surv, const uint32_t *lost, unsigned nlost,
                 std::vector<uint32_t> &tab);
template <class W>
struct TableView {
    W *K, *pos, *lost, *fix;      // coefficients | survivors [nsurv] | lost [nlost] | fix [row pad]
};
template <class W>
inline TableView<W> table_view(W *tab, unsigned mm, unsigned nroots, unsigned nsurv, unsigned nlost) {
    W *const pos = tab + recon_coef_words(mm, nroots, nsurv);
    return {tab, pos, pos + nsurv, pos + nsurv + nlost};
}
using DevTable = TableView<const uint32_t>;

// In-place parity update of interleaved frames (ezrs_recon.hip; ezrs_update_create /
// ezrs_update_interleaved): the code is linear, so parity_new = parity_old ^ G[:, changed] *
// (data_new ^ data_old), G the rebuild rows of the all-parity reconstruction plan (recon_build with
// lost = len .. len + NROOTS - 1).  update_check: len in 1..load and nchanged (1..len) distinct
// positions below len.  update_build: the columns `changed` of G, cols[row][r][bit]; false where
// update_check fails.  The device table is recon_table with survivors = changed and lost = the
// parity positions.
bool update_check(const CodecMath &m, unsigned len, const uint32_t *changed, unsigned nchanged);
bool update_build(const CodecMath &m, unsigned len, const uint32_t *changed, unsigned nchanged,
                  std::vector<uint16_t> &cols);

// What the two frame-in-place kernels work on: the frames as in IlArgs (strides in elements) and,
// set per launch by the launcher, the part of them a launch covers.  First member of both argument
// structs.
struct FrameSpan {
    void *frames;
    size_t frame_pitch, sym_stride, depth;
    size_t j0, runs;              // first codeword of a frame, lanes per frame
    size_t f0, nf;                // frames
};
struct ReconArgs {
    FrameSpan span;
    int32_t *result;              // nullable
    unsigned nsurv, nlost, mm;
    unsigned nrp;                 // recon_row_pad(nroots)
    unsigned nrows;               // rows to apply: nroots, or nlost when result is null
};
struct UpdateArgs {
    FrameSpan span;
    const void *newsyms;          // [frame][changed position][codeword]
    size_t new_frame_pitch, new_sym_stride;
    unsigned nchg, len, nroots, mm;
    unsigned nrp;                 // recon_row_pad(nroots)
};
// The pointer forms (ezrs_reconstruct_ptrs / ezrs_update_ptrs): one frame whose symbol rows are
// buffers of their own.  The device pointers travel by value with the kernel arguments, compacted
// on the host in the order the kernels walk them, so that no position list is read on the device:
//   reconstruction  survivor c [nsurv] | lost[r] [nlost] (null: that rebuilt row is not stored)
//   update          changed[c] [nchg] | parity row i [nroots] | new symbols of changed[c] [nchg]
// span.frames is null and span.sym_stride 0; span.depth is the shard length.
constexpr unsigned kPtrsMax = EZRS_PTRS_MAX;
struct PtrTable {
    void *p[kPtrsMax];
};
// ezrs_decode_ptrs: the n pointers of one stripe, by position, written to out[0 .. n-1] in device
// memory (the head of the call's workspace), so that the call runs the table policy of IlPtrArgs.
hipError_t launch_il_table(const PtrTable &tab, unsigned n, void **out, hipStream_t s);
struct ReconPtrArgs : ReconArgs {
    PtrTable tab;
};
struct UpdatePtrArgs : UpdateArgs {
    PtrTable tab;
};
// The batched pointer forms (ezrs_reconstruct_ptrs_batch / ezrs_update_ptrs_batch): nstripes frames
// whose symbol rows are buffers of their own, named by a pointer table in DEVICE memory that the
// kernels read while they run: the row at position p of stripe s is table[s * pitch + p], by
// position and not compacted, and the new symbols of changed[r] are new_table[s * new_pitch + r].
// span.frames is null, span.sym_stride and span.frame_pitch 0; span.depth is the shard length.
// wruns: the threads a stripe takes, span.runs rounded up to a wave, set per launch by the launcher.
struct ReconBatchArgs : ReconArgs {
    void *const *table;
    size_t pitch, wruns;
};
struct UpdateBatchArgs : UpdateArgs {
    void *const *table;
    const void *const *new_table;
    size_t pitch, new_pitch, wruns;
};
// The mixed batched form (ezrs_reconstruct_ptrs_mixed): the batched form with a plan per stripe.
// The plans of a set (ezrs_recon_set_create) lie in ONE device allocation, `set`, in dwords:
//   directory [nplans] of ReconSetEntry | the plans' recon_table images, each at a multiple of
//   kReconSetAlign dwords (what a plan's own allocation gives its table)
// and stripe f of the call works under plan plan_of[f]; an index >= nplans skips the stripe.  What
// ReconArgs says of one plan holds here for the whole set: nsurv and nlost are unused, and nrows is
// nroots with a result, else the largest nlost of the set (the launcher's row block); a stripe
// applies nroots rows or its own plan's nlost.
struct ReconSetEntry {
    uint32_t off;                 // of the plan's image, in dwords from `set`
    uint32_t nsurv, nlost;
    uint32_t pos;                 // of its survivor list: off + recon_coef_words(mm, nroots, nsurv)
};
constexpr size_t kReconSetAlign = 64;
struct ReconMixedArgs : ReconBatchArgs {
    const uint32_t *plan_of;      // [nstripes], device
    const uint32_t *set;          // the directory is at its head
    unsigned nplans;
};
// The mixed batched update (ezrs_update_ptrs_mixed): UpdateBatchArgs with a change set per stripe,
// from a set of update plans (ezrs_update_set_create) laid out as above.  An update plan's table is
// a recon_table image with survivors = changed and lost = the parity positions, so its directory
// entry reads (off, nchanged, nroots, offset of the changed list).  nchg here is the largest
// nchanged of the set, which the kernel does not use (a stripe takes its own plan's); len, nroots,
// mm and nrp hold for every plan of the set.
struct UpdateMixedArgs : UpdateBatchArgs {
    const uint32_t *plan_of;      // [nstripes], device
    const uint32_t *set;          // the directory is at its head
    unsigned nplans;
};
// t: the plan's device table (table_view of its base).  The pointer forms: al is the OR of the
// addresses in a.tab that the call uses; the batched forms: the alignment the caller promises for
// every pointer of the tables.
hipError_t launch_recon(const ReconArgs &a, size_t nframes, const DevTable &t, hipStream_t s);
hipError_t launch_update(const UpdateArgs &a, size_t nframes, const DevTable &t, hipStream_t s);
hipError_t launch_recon(const ReconPtrArgs &a, size_t al, const DevTable &t, hipStream_t s);
hipError_t launch_update(const UpdatePtrArgs &a, size_t al, const DevTable &t, hipStream_t s);
hipError_t launch_recon(const ReconBatchArgs &a, size_t nstripes, size_t al, const DevTable &t, hipStream_t s);
hipError_t launch_update(const UpdateBatchArgs &a, size_t nstripes, size_t al, const DevTable &t, hipStream_t s);
hipError_t launch_recon(const ReconMixedArgs &a, size_t nstripes, size_t al, hipStream_t s);
hipError_t launch_update(const UpdateMixedArgs &a, size_t nstripes, size_t al, hipStream_t s);

} // namespace ezrs
