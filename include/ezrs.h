/*
 * ezrs.h -- C ABI of the MI355X Reed-Solomon engine (libezrs_hip.so).
 *
 * Drop-in boundary for the hot path of pjkundert/ezpwd-reed-solomon: batched RS(N,K) encode and
 * errors+erasures decode over GF(2^m), m = 2..16, bit-exact with the reference's
 *
 *   ezpwd::reed_solomon<...>::encode<INP>(data, len, parity)                 c++/ezpwd/rs_base:868-904
 *   ezpwd::reed_solomon<...>::decode<INP>(data, len, parity, eras_pos,
 *                                         no_eras, corr)                     c++/ezpwd/rs_base:1170-1242
 *
 * applied independently to every codeword of a batch.  The reference has no batch or C ABI for
 * RS; each entry point below replaces a loop of those per-codeword calls (the loops in
 * rsencode.C:93-163, exercise.H:121-199, rsvalidate.C:97-289).  Codec construction replaces the
 * template instantiations ezpwd::RS<N,K>, RS_CCSDS<255,K>, RS_CCSDS_CONV<255,K> (c++/ezpwd/rs:74-104).
 *
 * Conventions
 *   - All compute entry points take DEVICE pointers (hipMalloc'd, on the codec's device) and a
 *     hipStream_t passed as void*; they are asynchronous and never synchronise.  A codec is const
 *     after creation and may be shared by threads and streams, like the reference's codec objects
 *     (rs_base:602-605): each stream gets its own device workspace (grown on demand, never freed
 *     before ezrs_destroy), so calls on different streams never share scratch memory.  The *_ws
 *     forms take a caller-owned workspace of ezrs_workspace_bytes() instead (no allocation at all:
 *     the form to capture into a hipGraph); ezrs_reserve_stream pre-sizes a stream's workspace.
 *     ezrs_*_host take host pointers and run a chunked, double-buffered H2D/kernel/D2H pipeline.
 *   - A codeword's symbols are stored as its datum type: uint8_t for m <= 8, uint16_t for m > 8
 *     (the reference's TYP, rs:75-89).  Strides are in ELEMENTS of the respective array.
 *   - `len` is the number of data (non-parity) symbols per codeword, 1..N-NROOTS; shorter codewords
 *     are shortened codes with implicit leading zeros (rs_base:1302-1304, 1378).
 *   - Encode reads `data` and writes `parity` (encode(data, len, parity), rs_base:868-904); rows that
 *     carry their own parity after the data (the reference's pair/container forms, rs_base:778-790)
 *     go through ezrs_encode_rows.  Decode with parity == NULL: the parity follows the data in the
 *     row, at data + len (the reference's decode(data, len+NROOTS) form, rs_base:1183-1186).
 *   - Symbols narrower than their datum (e.g. RS(31,K) in uint8_t) follow the reference's masked
 *     path: data bits above the symbol are ignored on encode and preserved on decode; a parity datum
 *     with bits above the symbol fails that codeword's decode with -1 (rs_base:1194-1235).
 *   - Return value of every function: 0 on success or a negative errno (-EINVAL bad arguments,
 *     -ENODEV no usable HIP device, -ENOMEM, -EIO a HIP runtime error).  No C++ exception ever
 *     crosses this ABI.  Per-codeword decode outcomes go to `result` (see ezrs_decode).
 */
#ifndef EZRS_H
#define EZRS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EZRS_ABI_VERSION 5

typedef struct ezrs_codec ezrs_codec;

typedef struct ezrs_info {
    unsigned symbol_bits;  /* m                                    (rs_base:570 SYMBOL/MM) */
    unsigned size;         /* N = 2^m - 1                          (rs_base:571 SIZE/NN)   */
    unsigned nroots;       /* N - K parity symbols                 (rs_base:723 NROOTS)    */
    unsigned load;         /* K = N - NROOTS max data symbols      (rs_base:724 LOAD)      */
    unsigned poly;         /* field polynomial                     (rs_base:756 poly())    */
    unsigned fcr;          /* first consecutive root               (rs_base:762 fcr())     */
    unsigned prim;         /* primitive element                    (rs_base:767 prim())    */
    unsigned datum_bytes;  /* 1 (uint8_t) or 2 (uint16_t)          (rs_base:568 DATUM/8)   */
    int dual;              /* CCSDS Berlekamp dual basis           (rs_base:772 dual())    */
    int device;            /* HIP device the codec lives on */
} ezrs_info;

/* Library / device probe: returns the number of visible HIP devices (>= 0) or a negative errno. */
int ezrs_device_count(void);
/* ABI version of the loaded library (EZRS_ABI_VERSION). */
int ezrs_abi_version(void);

/* Generic codec over GF(2^m): replaces ezpwd::reed_solomon<TYP,SYM,RTS,FCR,PRM,gfpoly<SYM,PLY>,DUAL>
 * (rs_base:702-1719).  Fails with -EINVAL where the reference's constructor would raise:
 * non-primitive poly (rs_base:623-625), nroots == 0 or >= N (rs_base:1254-1256), dual with m != 8
 * (rs_base:1188-1190); -ENOTSUP for m > 8 with more than 256 parity symbols (engine limit). */
int ezrs_create(ezrs_codec **out, unsigned symbol_bits, unsigned poly, unsigned fcr,
                unsigned prim, unsigned nroots, int dual, int device);
/* ezpwd::RS<N,K> -- the standard polynomial per N, FCR = 1, PRIM = 1 (rs:74-89). */
int ezrs_create_rs(ezrs_codec **out, unsigned n, unsigned k, int device);
/* ezpwd::RS_CCSDS<255,K> (dual = 1) / RS_CCSDS_CONV<255,K> (dual = 0): poly 0x187,
 * FCR = 128 - (255-K)/2, PRIM = 11 (rs:101-104). */
int ezrs_create_ccsds(ezrs_codec **out, unsigned k, int dual, int device);
int ezrs_destroy(ezrs_codec *codec);
/* Which kernel family serves the codec's full-length batches: EZRS_PATH_* (diagnostics; every
 * family is bit-exact with the reference). */
#define EZRS_PATH_GENERIC 0     /* per-codeword kernels (lane or 32-lane group per codeword)        */
#define EZRS_PATH_BITSLICE 1    /* bit-sliced GF(2^8) kernels (CCSDS dual basis)                     */
#define EZRS_PATH_PLANESLICE 2  /* plane-sliced GF(2^8) tile kernels (RS(255,K), NROOTS <= 32)       */
#define EZRS_PATH_WIDE 3        /* GF(2^16) remainder-network kernels (RS(65535,65503/65519))        */
int ezrs_kernel_path(const ezrs_codec *codec);
/* Decode semantics of a codec (encode is the same under both):
 *   EZRS_SEM_EZPWD (default) -- decode_symbols of c++/ezpwd/rs_base:1335-1718: erasures and
 *     positions relative to the first supplied symbol; -1 for deg lambda = 0, a zero Forney
 *     denominator or a root in the pad (rs_base:1589-1648).
 *   EZRS_SEM_KARN -- decode_rs_char / decode_rs_int of Phil Karn's libfec
 *     (fec-3.0.1/decode_rs.h:71-298): erasures and positions in the full NN frame (a position
 *     p >= pad is row symbol p - pad), none of those three checks (a zero denominator applies
 *     num1 * num2, a root in the pad is counted and reported but not corrected), the datum is the
 *     symbol.  The Karn ABI (include/ezrs_fec.h) creates its codecs in this mode.  As in libfec,
 *     the syndromes are checked before the erasures: a word with zero syndromes returns 0 even
 *     with an erasure position >= NN (otherwise -1, where libfec's result is undefined); a root in
 *     the pad gets correction value 0 in `corr`.
 * Set the semantics once, after create and before the codec's first decode: the setter takes the
 * codec's lock (it waits for a host-memory call in progress), but a device decode already enqueued
 * on a stream runs with the semantics it was launched with, and decodes issued concurrently from
 * other threads may see either. */
#define EZRS_SEM_EZPWD 0
#define EZRS_SEM_KARN 1
int ezrs_set_semantics(ezrs_codec *codec, int semantics);
int ezrs_get_semantics(const ezrs_codec *codec);
/* Test hook: cap the codewords one plane-sliced kernel launch of `codec` takes (0 restores the
 * default, the largest batch whose 32-bit buffer offsets fit).  Results never depend on it:
 * lowering it only splits a batch over more launches (mid-tile for shard batches), which the tests
 * use to exercise those splits at small sizes.  Per codec; takes the codec's lock, so it waits for
 * a host-memory call in progress, but a device call already enqueued keeps the cap it was
 * launched with. */
int ezrs_set_launch_rows(ezrs_codec *codec, size_t rows);
int ezrs_get_info(const ezrs_codec *codec, ezrs_info *info);

/* Pre-size the workspace of `stream` (NULL: the null stream) for batches of up to `ncw` codewords,
 * so that later calls of that size on that stream do not allocate. */
int ezrs_reserve(ezrs_codec *codec, size_t ncw);
int ezrs_reserve_stream(const ezrs_codec *codec, size_t ncw, void *stream);
/* Device workspace bytes a batch of ncw codewords needs (encode and decode alike; may be 0). */
size_t ezrs_workspace_bytes(const ezrs_codec *codec, size_t ncw);

/* Batch encode -- for every codeword k < ncw:
 *   encode<TYP>(data + k*data_stride, len, parity + k*parity_stride)          rs_base:868-904
 * data and parity are device arrays of the datum type; data is only read, parity is required. */
int ezrs_encode(const ezrs_codec *codec, const void *data, size_t data_stride, unsigned len,
                void *parity, size_t parity_stride, size_t ncw, void *stream);
/* Row form: row k holds len data symbols followed by its NROOTS parity symbols (written):
 *   encode(std::pair(rows_k, rows_k + len + NROOTS))                          rs_base:778-790 */
int ezrs_encode_rows(const ezrs_codec *codec, void *rows, size_t stride, unsigned len, size_t ncw,
                     void *stream);
/* The same with a caller-owned device workspace of >= ezrs_workspace_bytes(codec, ncw) bytes. */
int ezrs_encode_ws(const ezrs_codec *codec, const void *data, size_t data_stride, unsigned len,
                   void *parity, size_t parity_stride, size_t ncw, void *ws, size_t ws_bytes,
                   void *stream);
int ezrs_encode_rows_ws(const ezrs_codec *codec, void *rows, size_t stride, unsigned len,
                        size_t ncw, void *ws, size_t ws_bytes, void *stream);

/* Batch decode -- for every codeword k < ncw, in place:
 *   result[k] = decode<TYP>(data + k*data_stride, len, parity + k*parity_stride,
 *                           eras_pos_k, neras[k], corr + k*corr_stride)      rs_base:1170-1242
 * eras       (nullable) uint32 rows of eras_stride entries: erasure positions relative to data[0]
 *            (parity positions follow at len..len+NROOTS-1); neras (nullable) their counts.
 * result     int32[ncw]: number of corrected symbols (erasures included, even when the erased
 *            symbol was already right), 0 for a valid codeword, -1 if uncorrectable or invalid
 *            (rs_base:1335-1718).  On -1 the direct (unmasked) path may leave partial
 *            corrections applied, exactly as the reference does (rs_base:1610-1690, 1238-1241).
 * positions  (nullable) uint32 rows of pos_stride >= NROOTS: entries 0..result[k]-1 receive the
 *            corrected positions relative to data[0], in the reference's Chien-search order
 *            (rs_base:1557-1576, 1713-1716); other entries are left untouched.
 * corr       (nullable) datum rows of corr_stride >= NROOTS: corr[j] receives the correction
 *            pattern of position j, for the j the reference writes (rs_base:1658-1687). */
int ezrs_decode(const ezrs_codec *codec, void *data, size_t data_stride, unsigned len,
                void *parity, size_t parity_stride, const uint32_t *eras, size_t eras_stride,
                const uint32_t *neras, int32_t *result, uint32_t *positions, size_t pos_stride,
                void *corr, size_t corr_stride, size_t ncw, void *stream);
int ezrs_decode_ws(const ezrs_codec *codec, void *data, size_t data_stride, unsigned len,
                   void *parity, size_t parity_stride, const uint32_t *eras, size_t eras_stride,
                   const uint32_t *neras, int32_t *result, uint32_t *positions, size_t pos_stride,
                   void *corr, size_t corr_stride, size_t ncw, void *ws, size_t ws_bytes,
                   void *stream);

/* Shard batches (device-resident).  A shard of `shard_len` data symbols is stored as the rsencode
 * wire format lays it out (rsencode.C:93-163, one encode/decode per chunk): R = ceil(shard_len /
 * chunk) codewords back to back, each `chunk` data symbols followed by its NROOTS parity symbols,
 * except the last, which carries the remaining shard_len - (R-1)*chunk data symbols (a shortened
 * codeword, rs_base:1302-1304) and its parity.  Shard i starts at shards + i*shard_pitch (elements,
 * >= ezrs_shard_encoded_len).  Codewords are numbered shard-major, k = i*R + j: result[k],
 * erasure / position / correction rows k are codeword j of shard i, positions relative to that
 * codeword's first data symbol.  The whole batch is one launch of the codec's kernels. */
size_t ezrs_shard_codewords(const ezrs_codec *codec, size_t shard_len, unsigned chunk);
size_t ezrs_shard_encoded_len(const ezrs_codec *codec, size_t shard_len, unsigned chunk);
/* Writes every codeword's parity (its data is only read). */
int ezrs_encode_shards(const ezrs_codec *codec, void *shards, size_t shard_pitch, size_t shard_len,
                       unsigned chunk, size_t nshards, void *stream);
/* Decodes every codeword in place: result[k] etc. as ezrs_decode, for nshards * R codewords. */
int ezrs_decode_shards(const ezrs_codec *codec, void *shards, size_t shard_pitch, size_t shard_len,
                       unsigned chunk, size_t nshards, const uint32_t *eras, size_t eras_stride,
                       const uint32_t *neras, int32_t *result, uint32_t *positions,
                       size_t pos_stride, void *corr, size_t corr_stride, void *stream);

/* Interleaved frames (device-resident).  A frame carries `depth` codewords interleaved symbol by
 * symbol: symbol s (0 <= s < len + NROOTS, data first, then parity) of codeword j (0 <= j < depth)
 * of frame f is element  frames[f*frame_pitch + s*sym_stride + j]  (strides in elements of the
 * datum).  The reference has no interleaving: each call replaces de-interleaving on the host, the
 * per-codeword loop of encode / decode calls (rs_base:868-904, 1170-1242) and re-interleaving.
 *   CCSDS depth I      sym_stride == depth == I, frame_pitch >= (len + NROOTS) * I; a 1275-byte
 *                      RS_CCSDS(255,223) I = 5 codeblock is one frame.
 *   striped shards     K data and NROOTS parity shards of shard_len symbols, byte j of every shard
 *                      forming codeword j: nframes = 1, depth = shard_len, sym_stride = shard pitch
 *                      (ezrs_*_shards above is the rsencode layout, codewords contiguous in a shard).
 * Codewords are numbered frame-major, k = f*depth + j: result[k] and the erasure / position /
 * correction rows k, and positions relative to the codeword's first data symbol, mean what they
 * mean in ezrs_decode, under both semantics.  len < load is a shortened code.
 * The frames are gathered into packed rows in the workspace, the codec's row kernels run on those,
 * and rows are scattered back, a bounded number of codewords per pass.  Encode writes only the
 * NROOTS parity symbols of every codeword; decode writes only the symbols of codewords whose
 * result is nonzero (a -1 row carries the reference's partial corrections, rs_base:1610-1690).  No
 * other element of `frames` is ever written: not the gaps of sym_stride > depth, not the padding
 * after a frame's last symbol row or between frames.
 * The *_ws forms take a caller-owned workspace of >= ezrs_interleaved_workspace_bytes() bytes
 * (which is exactly what a call uses; 0 for invalid arguments) and allocate nothing.
 * -EINVAL: null codec, frames or result; depth == 0; sym_stride < depth; len outside 1..load;
 * nframes > 1 with frame_pitch < (len + NROOTS - 1)*sym_stride + depth; the stride rules of
 * ezrs_decode for eras, positions and corr when the batch has more than one codeword; a workspace
 * that is too small.  nframes == 0 returns 0 and touches nothing. */
size_t ezrs_interleaved_workspace_bytes(const ezrs_codec *codec, unsigned len, size_t depth,
                                        size_t nframes);
int ezrs_encode_interleaved(const ezrs_codec *codec, void *frames, size_t frame_pitch,
                            size_t sym_stride, size_t depth, unsigned len, size_t nframes,
                            void *stream);
int ezrs_encode_interleaved_ws(const ezrs_codec *codec, void *frames, size_t frame_pitch,
                               size_t sym_stride, size_t depth, unsigned len, size_t nframes,
                               void *ws, size_t ws_bytes, void *stream);
int ezrs_decode_interleaved(const ezrs_codec *codec, void *frames, size_t frame_pitch,
                            size_t sym_stride, size_t depth, unsigned len, size_t nframes,
                            const uint32_t *eras, size_t eras_stride, const uint32_t *neras,
                            int32_t *result, uint32_t *positions, size_t pos_stride, void *corr,
                            size_t corr_stride, void *stream);
int ezrs_decode_interleaved_ws(const ezrs_codec *codec, void *frames, size_t frame_pitch,
                               size_t sym_stride, size_t depth, unsigned len, size_t nframes,
                               const uint32_t *eras, size_t eras_stride, const uint32_t *neras,
                               int32_t *result, uint32_t *positions, size_t pos_stride, void *corr,
                               size_t corr_stride, void *ws, size_t ws_bytes, void *stream);

/* Shared-erasure reconstruction of interleaved frames (device-resident).  Striped shards lose whole
 * shards: every codeword of the stripe has the same erasure positions and no other errors.  A plan
 * solves that erasure system once on the host; ezrs_reconstruct_interleaved then applies one
 * constant GF(2^m) matrix to the surviving symbols, in place in the frames, with no staging and no
 * workspace (the reference has no such call: it replaces decode() with the same eras_pos for every
 * codeword, rs_base:1170-1242).
 *   plan     `lost`: nlost (0..NROOTS) distinct HOST positions in 0..len+NROOTS-1, relative to the
 *            codeword's first data symbol (parity follows at len..), in that frame under both
 *            semantics of the codec.  ezrs_recon_create builds the matrix, uploads it to the
 *            codec's device and may synchronise; the plan copies what it needs, so it stays valid
 *            after ezrs_destroy(codec); it is const afterwards and may be shared by threads and
 *            streams.  -EINVAL: null out or codec, len outside 1..load, nlost > NROOTS, a position
 *            >= len + NROOTS or given twice; -ENOTSUP when the plan's device table would exceed
 *            64 MiB (engine limit): for symbols wider than 8 bits it takes 4 bytes x symbol_bits x
 *            survivors x NROOTS (rounded up to 4, 8, 16 or a multiple of 32), so full-length
 *            RS(65535,65503) is such a case; no codec of up to 8 bits comes near it.
 *   call     geometry as in ezrs_*_interleaved above; every frame of the call shares the plan's
 *            loss pattern.  Asynchronous; never allocates, never synchronises.  For every codeword
 *            k = f*depth + j the nlost lost symbols are overwritten with the values the first nlost
 *            syndrome equations determine from the survivors, in the order of `lost`; their old
 *            contents are never read.  No other element of `frames` is written.  Bits above the
 *            symbol are ignored in survivors and zero in rebuilt symbols.
 *   result   (nullable) int32[nframes*depth]: nlost if the remaining NROOTS - nlost syndromes of
 *            the rebuilt word are zero, i.e. some codeword agrees with every survivor, else -1 (the
 *            lost symbols are written all the same; fall back to ezrs_decode_interleaved for that
 *            stripe).  Up to NROOTS - nlost wrong survivor symbols always give -1; with nlost ==
 *            NROOTS nothing can be checked and the result is nlost.  With result == NULL the check
 *            is not computed.  nlost == 0 writes nothing to `frames`: a verify (0 or -1).
 * -EINVAL: null plan or frames; depth == 0; sym_stride < depth; nframes > 1 with frame_pitch <
 * (len + NROOTS - 1)*sym_stride + depth.  nframes == 0 returns 0 and touches nothing. */
typedef struct ezrs_recon ezrs_recon;
int ezrs_recon_create(ezrs_recon **out, const ezrs_codec *codec, unsigned len, const uint32_t *lost,
                      unsigned nlost);
int ezrs_recon_destroy(ezrs_recon *plan);   /* NULL: 0 */
int ezrs_reconstruct_interleaved(const ezrs_recon *plan, void *frames, size_t frame_pitch,
                                 size_t sym_stride, size_t depth, size_t nframes, int32_t *result,
                                 void *stream);
/* The plan's matrix on the host, from the codec parameters of ezrs_create (no device is touched).
 * cols: NROOTS * nsurv * symbol_bits uint16 (cols_cap: entries available), [row][survivor][bit]:
 * the image, in the stored representation (dual basis where the codec has it), of bit `bit` of
 * survivor `survivor` in output row `row`; an output symbol is the XOR of the entries of the set
 * bits of all survivors.  Rows 0..nlost-1 rebuild lost[0..nlost-1] in the order given, the others
 * are the check rows.  survivors: the nsurv = len + NROOTS - nlost surviving positions, ascending.
 * -EINVAL: invalid codec parameters, the plan rules above, null outputs, cols_cap too small. */
int ezrs_recon_bitmatrix(unsigned symbol_bits, unsigned poly, unsigned fcr, unsigned prim,
                         unsigned nroots, int dual, unsigned len, const uint32_t *lost,
                         unsigned nlost, uint16_t *cols, size_t cols_cap, uint32_t *survivors);

/* In-place parity update of interleaved frames (device-resident): the small write.  One or a few
 * data shards of a stripe change and the parity shards must follow.  The code is linear, so with G
 * the parity rows of the all-parity reconstruction plan (lost = len..len+NROOTS-1),
 *   parity_new = parity_old ^ G[:, changed] * (data_new ^ data_old):
 * only the changed symbols and the parity are read and written, whatever `len` is (the reference
 * has no such call: it replaces encode() of the whole codeword, rs_base:868-904).
 *   plan     `changed`: nchanged (1..len) distinct HOST positions of data symbols, 0 <= changed[r] <
 *            len, relative to the codeword's first data symbol under both semantics of the codec.
 *            ezrs_update_create takes those columns of the all-parity matrix, uploads them to the
 *            codec's device in the reconstruction plan's table format and may synchronise; the plan
 *            copies what it needs, so it stays valid after ezrs_destroy(codec); it is const
 *            afterwards and may be shared by threads and streams.  -EINVAL: null out, codec or
 *            changed; len outside 1..load; nchanged == 0 or > len; a position >= len or given
 *            twice; -ENOTSUP when the plan's device table would exceed 64 MiB (the limit and the
 *            formula of ezrs_recon_create with nchanged for the survivors); -ENOMEM.
 *   call     `frames`: geometry as in ezrs_*_interleaved above; every frame of the call shares the
 *            plan's positions.  `newsyms` holds the new contents of the changed symbols only:
 *            newsyms[f*new_frame_pitch + r*new_sym_stride + j] is the new value of symbol changed[r]
 *            of codeword j of frame f (strides in elements of the datum).  Asynchronous; no
 *            workspace; never allocates, never synchronises.  For every codeword, with d_r =
 *            newsyms ^ the old symbol in `frames`, parity symbol i gets ^= sum_r G[i][changed[r]] *
 *            d_r, and then the changed data symbols are overwritten with newsyms.  Only those
 *            nchanged data symbols and the NROOTS parity symbols of each codeword are written in
 *            `frames`, no other element; `newsyms` is only read.  Bits above the symbol do not
 *            enter the parity, for old and new values alike; the data symbols are stored as given;
 *            a parity symbol's bits above the symbol are left as they were.
 *            The old parity is read, not recomputed: a stripe whose parity was wrong by e before
 *            the call is wrong by the same e afterwards (verify with an nlost == 0 reconstruction
 *            plan where that matters).  `newsyms` must not overlap the written elements of
 *            `frames`; that is the caller's contract and is not checked.
 * -EINVAL: null plan, frames or newsyms; depth == 0; sym_stride < depth or new_sym_stride < depth;
 * nframes > 1 with frame_pitch < (len + NROOTS - 1)*sym_stride + depth or with new_frame_pitch <
 * (nchanged - 1)*new_sym_stride + depth; depth > SIZE_MAX / nframes.  nframes == 0 returns 0 and
 * touches nothing. */
typedef struct ezrs_update ezrs_update;
int ezrs_update_create(ezrs_update **out, const ezrs_codec *codec, unsigned len,
                       const uint32_t *changed, unsigned nchanged);
int ezrs_update_destroy(ezrs_update *plan);   /* NULL: 0 */
int ezrs_update_interleaved(const ezrs_update *plan, void *frames, size_t frame_pitch,
                            size_t sym_stride, size_t depth, size_t nframes, const void *newsyms,
                            size_t new_frame_pitch, size_t new_sym_stride, void *stream);
/* The plan's matrix on the host, from the codec parameters of ezrs_create (no device is touched).
 * cols: NROOTS * nchanged * symbol_bits uint16 (cols_cap: entries available), [row][r][bit]: the
 * image, in the stored representation, of bit `bit` of the difference at changed[r] in parity
 * symbol `row`; entries mean what ezrs_recon_bitmatrix's mean.
 * -EINVAL: invalid codec parameters, the plan rules above, null cols, cols_cap too small. */
int ezrs_update_bitmatrix(unsigned symbol_bits, unsigned poly, unsigned fcr, unsigned prim,
                          unsigned nroots, int dual, unsigned len, const uint32_t *changed,
                          unsigned nchanged, uint16_t *cols, size_t cols_cap);

/* Pointer-array forms of the two calls above (device-resident): one stripe whose shards are
 * buffers of their own, as erasure-coding callers have them (ISA-L's ec_encode_data(len, k, rows,
 * tbls, data**, coding**), jerasure), instead of one base pointer and one sym_stride.  shard_len is
 * what depth is in the strided calls: codeword j is symbol j of every shard, in elements of the
 * datum.  `shards` (and `newsyms`) are HOST arrays of DEVICE pointers; they are read during the call
 * and not kept: the pointers travel with the kernel arguments, so the caller may free or overwrite
 * the arrays as soon as the call returns, although the work is asynchronous.  One stripe per call;
 * never allocate, never synchronise, no workspace; capturable like the strided forms.  For every
 * valid input the bytes written and `result` equal what the strided call produces on the same
 * symbols.  Accesses are 16 bytes wide per lane when every pointer the call uses is a multiple of
 * 16, 4 bytes when of 4, else one element; any alignment of the datum is valid.
 *   ezrs_reconstruct_ptrs   shards[len + NROOTS], indexed by position.  The entry of a surviving
 *            position is that shard, shard_len symbols, only read.  The entry of a lost position is
 *            where that rebuilt shard goes; NULL there means "not wanted" (a degraded read that needs
 *            one shard): nothing is written for it (its row is computed with the others and
 *            dropped), and `result` is not affected, since the check rows depend on the survivors
 *            only.  result: nullable int32[shard_len], as in ezrs_reconstruct_interleaved.  An
 *            nlost == 0 plan is a verify that writes nothing to any shard; the all-parity plan
 *            (lost = len..len+NROOTS-1) is the pointer-form encode.
 *   ezrs_update_ptrs        shards[len + NROOTS], indexed by position; only the entries at the
 *            plan's changed positions and at the parity positions len..len+NROOTS-1 are used, every
 *            other entry is ignored and may be NULL: those shards need not be on the device.
 *            newsyms[nchanged], in the order of `changed`, each shard_len new symbols, only read.
 *            Per codeword exactly ezrs_update_interleaved: the old parity is read, not recomputed;
 *            the data is overwritten after the parity; bits above the symbol as there.
 * Checked on the host before any launch.  -EINVAL: null plan, `shards` or `newsyms`; a NULL entry
 * the call must read or write (a survivor; a changed, parity or newsyms buffer); shard_len *
 * datum bytes overflowing size_t; two written buffers that overlap over [p, p + shard_len * datum
 * bytes), or a written buffer that overlaps a read one.  -ENOTSUP: the call uses more than
 * EZRS_PTRS_MAX pointers: len + NROOTS for the reconstruction, 2*nchanged + NROOTS for the update
 * (every codec of up to 8 bits fits at any length, wider codecs when shortened).  shard_len == 0
 * returns 0 and touches nothing. */
#define EZRS_PTRS_MAX 320   /* device pointers one *_ptrs call can carry (they travel as kernel arguments) */
int ezrs_reconstruct_ptrs(const ezrs_recon *plan, void *const *shards, size_t shard_len,
                          int32_t *result, void *stream);
int ezrs_update_ptrs(const ezrs_update *plan, void *const *shards, const void *const *newsyms,
                     size_t shard_len, void *stream);

/* Batched pointer-table forms of the two calls above (device-resident): nstripes stripes per call,
 * every shard of every stripe a buffer of its own, all stripes under the one plan (a rebuild, a
 * scrub, a flush of small writes).  Per stripe exactly the one-stripe form on that stripe's
 * pointers: the same bytes written and the same `result`.  What differs is where the pointers are:
 *   table    a DEVICE array of DEVICE pointers on the plan's device.  table[s*table_pitch + p] is
 *            the shard at position p (0 .. len+NROOTS-1) of stripe s, shard_len symbols of the datum;
 *            indexed by position, as `shards` is, and not compacted.  table_pitch >= len + NROOTS;
 *            the entries from len + NROOTS up to table_pitch are never read.  One table, resident on
 *            the device, serves a reconstruction plan, a verify plan and an update plan of the same
 *            stripes with no host work between them.
 *   new_table   new_table[s*new_pitch + r]: the new symbols of changed[r] of stripe s, shard_len of
 *            them, only read.  new_pitch >= nchanged; the entries past nchanged are never read.
 * The kernels read the tables WHILE THEY RUN: unlike the host arrays of the one-stripe forms, the
 * tables must stay valid and unchanged until the work has completed on `stream`.  There is no limit
 * on the number of pointers (EZRS_PTRS_MAX does not apply: nothing travels as kernel arguments).
 * Asynchronous; no workspace; never allocate, never synchronise; capturable.
 *   ezrs_reconstruct_ptrs_batch   survivors are only read; the entry of a lost position is where
 *            that rebuilt shard goes, and NULL there means "not wanted" for that stripe only: nothing
 *            is written for it and `result` is not affected.  result: nullable
 *            int32[nstripes*shard_len], stripe-major (codeword j of stripe s at s*shard_len + j):
 *            nlost or -1, as in ezrs_reconstruct_interleaved.  An nlost == 0 plan is a verify that
 *            writes nothing to any shard; the all-parity plan is the batched pointer-form encode.
 *   ezrs_update_ptrs_batch        only the entries of `table` at the plan's changed positions and
 *            at the parity positions len..len+NROOTS-1, and new_table, are used; every other entry is
 *            ignored and may be NULL or garbage.  The old parity is read, not recomputed; the data is
 *            overwritten after the parity; bits above the symbol as in ezrs_update_interleaved.
 *   align    the caller's promise: every pointer the call uses (in both tables) is a multiple of
 *            `align` bytes.  16, 4 or the size of the datum; it selects the access width, 16 bytes
 *            per lane, 4 bytes or one element, exactly as the OR of the addresses does in the
 *            one-stripe forms.  The ragged end of shard_len (what is left after whole 16- or 4-byte
 *            runs) goes element by element, whatever `align` is.
 * NOT CHECKED, because the host cannot see the tables, and undefined behaviour when broken: a
 * pointer that is not a multiple of `align`; a NULL (or invalid) entry that the call must read or
 * write (a survivor; a changed, parity or new_table entry); any overlap between two buffers the
 * call writes, in the same stripe or in different stripes, or between a buffer it writes and one
 * it reads (a table included), each over [p, p + shard_len * datum bytes).
 * Checked on the host before any launch.  -EINVAL: null plan, `table` or `new_table`; table_pitch <
 * len + NROOTS; new_pitch < nchanged; align not 16, 4 or the datum size; shard_len * datum bytes or
 * nstripes * shard_len overflowing size_t.  Otherwise nstripes == 0 or shard_len == 0 returns 0
 * and touches nothing. */
int ezrs_reconstruct_ptrs_batch(const ezrs_recon *plan, void *const *table, size_t table_pitch,
                                size_t shard_len, size_t nstripes, unsigned align, int32_t *result,
                                void *stream);
int ezrs_update_ptrs_batch(const ezrs_update *plan, void *const *table, size_t table_pitch,
                           const void *const *new_table, size_t new_pitch, size_t shard_len,
                           size_t nstripes, unsigned align, void *stream);

/* Mixed-plan batched reconstruction (device-resident): ezrs_reconstruct_ptrs_batch with a loss
 * pattern per stripe, for the sweeps in which one plan does not fit all stripes: a rebuild under
 * rotated placement (the failed drive holds another position of every stripe), a scrub that meets
 * healthy stripes (nlost == 0: verify) next to degraded ones, new stripes that want the all-parity
 * plan (encode) among them.  One call on the resident table, with no bucketing by pattern on the
 * host, no compacted table per bucket and no launch per bucket.
 *   ezrs_recon_set_create   gathers nplans existing plans into one device allocation on the plans'
 *            device: a directory (per plan: where its table lies, nsurv, nlost) and copies of the
 *            plans' device tables back to back.  The set copies what it needs and may synchronise
 *            to do so; it stays valid after the plans and the codec are destroyed, is const
 *            afterwards and may be shared by threads and streams.  The same pattern may appear
 *            more than once.  -EINVAL, before any device is touched: null `out` or `plans`; nplans
 *            == 0; a NULL entry; plans that differ in symbol bits, NROOTS, len or device.  -ENOTSUP:
 *            the set's allocation would exceed 64 MiB (the limit of one plan's table, here for the
 *            directory and all tables together).  -ENOMEM; -EIO for a HIP failure.  Plans of
 *            different codecs with equal symbol bits, NROOTS and len are NOT detected: each stripe
 *            simply gets its plan's matrix.
 *   ezrs_reconstruct_ptrs_mixed   stripe s works under plan plan_of[s] of the set.  plan_of: a DEVICE
 *            array of nstripes indices on the set's device, read WHILE THE KERNELS RUN, like the
 *            table.  Per stripe the call is exactly ezrs_reconstruct_ptrs_batch under that stripe's
 *            plan: the same bytes are written; result[s*shard_len + j] is that plan's nlost, or -1;
 *            NULL at a lost position of that stripe's plan means "not wanted" for that stripe;
 *            table, table_pitch, align and the ragged end of shard_len mean what they mean there.
 *            An index >= nplans skips the stripe (EZRS_PLAN_SKIP is the named way to say so): none
 *            of its table entries are read, so they may be anything, no byte of any shard is
 *            written, and its `result` entries are left as they were.  With result == NULL only the
 *            rebuild rows of each stripe's own plan are applied; a stripe whose plan has nlost == 0
 *            then does nothing, and none of its table entries are read either.
 *            Asynchronous; no workspace; never allocates, never synchronises; capturable.
 * NOT CHECKED, and undefined behaviour when broken: what ezrs_reconstruct_ptrs_batch lists, for
 * every stripe that is not skipped under that stripe's plan, and any overlap between a buffer the
 * call writes (`result` included) and plan_of.
 * Checked on the host before any launch.  -EINVAL: null set, plan_of or `table`; table_pitch < len +
 * NROOTS; align not 16, 4 or the datum size; shard_len * datum bytes or nstripes * shard_len
 * overflowing size_t.  Otherwise nstripes == 0 or shard_len == 0 returns 0 and touches nothing.
 * The strided forms have no mixed variant: in the strided lane map a wave may span two frames, so
 * a plan per frame would not be uniform over a wave.  The batched update has one, below. */
typedef struct ezrs_recon_set ezrs_recon_set;
#define EZRS_PLAN_SKIP 0xFFFFFFFFu   /* in plan_of: leave this stripe alone */
int ezrs_recon_set_create(ezrs_recon_set **out, const ezrs_recon *const *plans, unsigned nplans);
int ezrs_recon_set_destroy(ezrs_recon_set *set);   /* NULL: 0 */
int ezrs_reconstruct_ptrs_mixed(const ezrs_recon_set *set, const uint32_t *plan_of,
                                void *const *table, size_t table_pitch, size_t shard_len,
                                size_t nstripes, unsigned align, int32_t *result, void *stream);

/* Mixed-plan batched parity update (device-resident): ezrs_update_ptrs_batch with a change set per
 * stripe, for a flush of small writes in which one stripe's write hit data shard 3, the next one's
 * shard 7 and a third touched two shards.  One call on the resident table, with no bucketing by
 * change set on the host, no compacted table pair per bucket and no launch per bucket.
 *   ezrs_update_set_create   gathers nplans existing update plans into one device allocation, in
 *            every rule as ezrs_recon_set_create does for reconstruction plans: a directory (per
 *            plan: where its table lies, nchanged) and copies of the plans' device tables; valid
 *            after the plans and the codec are destroyed, const afterwards, shareable; the same
 *            change set may appear more than once.  -EINVAL, before any device is touched: null
 *            `out` or `plans`; nplans == 0; a NULL entry; plans that differ in symbol bits, NROOTS,
 *            len or device.  -ENOTSUP: the allocation would exceed 64 MiB.  -ENOMEM; -EIO for a HIP
 *            failure.  Plans of different codecs with equal symbol bits, NROOTS and len are NOT
 *            detected: each stripe simply gets its plan's columns.
 *   ezrs_update_ptrs_mixed   stripe s works under plan plan_of[s] of the set.  plan_of: a DEVICE
 *            array of nstripes indices on the set's device, read WHILE THE KERNELS RUN, like the
 *            tables.  Per stripe the call is exactly ezrs_update_ptrs_batch under that stripe's
 *            plan: the same bytes are written to the parity shards and to the changed shards; the
 *            old parity is read, not recomputed; the data is overwritten after the parity; bits
 *            above the symbol as there.  Of table[s*table_pitch + .] only the entries at the changed
 *            positions of THAT STRIPE'S plan and at len..len+NROOTS-1 are used, and of
 *            new_table[s*new_pitch + r] only r < that plan's nchanged, in the order of that plan's
 *            `changed`; every other entry of either row may be NULL or garbage.  new_pitch >= the
 *            largest nchanged of the set.  An index >= nplans skips the stripe (EZRS_PLAN_SKIP): no
 *            entry of either of its table rows is read and no byte is written.
 *            Asynchronous; no workspace; never allocates, never synchronises; capturable.
 * NOT CHECKED, and undefined behaviour when broken: what ezrs_update_ptrs_batch lists, for every
 * stripe that is not skipped under that stripe's plan; any overlap between a buffer the call writes
 * and plan_of or the set; and two stripes of one call that name the same physical stripe (two
 * writes to one stripe in one flush): they race on its parity.  Merge those into one plan with the
 * union of the changed positions, or issue two calls.
 * Checked on the host before any launch.  -EINVAL: null set, plan_of, `table` or `new_table`;
 * table_pitch < len + NROOTS; new_pitch < the largest nchanged of the set; align not 16, 4 or the
 * datum size; shard_len * datum bytes or nstripes * shard_len overflowing size_t.  Otherwise
 * nstripes == 0 or shard_len == 0 returns 0 and touches nothing.
 * A change set that differs from codeword to codeword within a stripe is not built. */
typedef struct ezrs_update_set ezrs_update_set;
int ezrs_update_set_create(ezrs_update_set **out, const ezrs_update *const *plans, unsigned nplans);
int ezrs_update_set_destroy(ezrs_update_set *set);   /* NULL: 0 */
int ezrs_update_ptrs_mixed(const ezrs_update_set *set, const uint32_t *plan_of,
                           void *const *table, size_t table_pitch,
                           const void *const *new_table, size_t new_pitch,
                           size_t shard_len, size_t nstripes, unsigned align, void *stream);

/* Pointer forms of ezrs_decode_interleaved (device-resident): the error path of the pointer forms
 * above.  A stripe whose verify or rebuild reported -1 holds errors at unknown positions; these
 * calls decode it where it lies, errors and erasures, with no strided copy of the stripe.  Per
 * stripe the call is exactly ezrs_decode_interleaved on one frame with depth = shard_len whose
 * symbol row p is the buffer at position p (0 .. len+NROOTS-1, data first, then parity): codeword j
 * is symbol j of every shard, and codewords are numbered stripe-major, k = s*shard_len + j, for
 * result[k] and the rows k of eras / neras / positions / corr, which mean what they mean in
 * ezrs_decode under both semantics of the codec and follow the same stride rules.
 * Only the symbols of codewords whose result is nonzero are written (a -1 codeword carries the
 * reference's partial corrections, rs_base:1610-1690); no other byte of any shard is touched.  The
 * stripes are gathered into packed rows in the workspace, the codec's row kernels run on those and
 * the rows of nonzero result are scattered back, a bounded number of codewords per pass.
 *   ezrs_decode_ptrs         one stripe.  shards: a HOST array of len + NROOTS DEVICE pointers,
 *            indexed by position, each shard_len symbols of the datum; read during the call and
 *            not kept: the pointers travel by value as kernel arguments (into a table at the head of
 *            the workspace), so the array is the caller's again when the call returns.  Every entry
 *            is read and may be written, so none may be NULL: a lost shard still needs a buffer to be
 *            rebuilt into, with that position in the codewords' erasure lists.  Symbols move as
 *            dwords of four codewords when every pointer and shard_len are multiples of 4 (the OR of
 *            the addresses, as in ezrs_reconstruct_ptrs), else one element at a time; any alignment
 *            of the datum is valid.  Checked on the host before any launch.  -EINVAL: null codec,
 *            `shards` or result; len outside 1..load; a NULL entry; shard_len * datum bytes
 *            overflowing size_t; any two buffers overlapping over [p, p + shard_len * datum bytes);
 *            the stride rules of ezrs_decode for eras, positions and corr when shard_len > 1; a
 *            workspace that is too small.  -ENOTSUP: len + NROOTS above EZRS_PTRS_MAX.  shard_len
 *            == 0 returns 0 and touches nothing.
 *   ezrs_decode_ptrs_batch   nstripes stripes.  table: a DEVICE array of DEVICE pointers,
 *            table[s*table_pitch + p] the shard at position p of stripe s, table_pitch >= len +
 *            NROOTS, the entries from len + NROOTS up to table_pitch never read: the table of
 *            ezrs_reconstruct_ptrs_batch, so one resident table serves verify, rebuild, update and
 *            decode.  The kernels read it WHILE THEY RUN: it must stay valid and unchanged until the
 *            work has completed on `stream`.  EZRS_PTRS_MAX does not apply.  align: the caller's
 *            promise that every pointer of the table the call uses is a multiple of `align` bytes,
 *            16, 4 or the size of the datum; the dword path is taken for align >= 4 and shard_len a
 *            multiple of 4.  Checked on the host: -EINVAL for a null codec, `table` or result; len
 *            outside 1..load; table_pitch < len + NROOTS; align not 16, 4 or the datum size;
 *            shard_len * datum bytes or nstripes * shard_len overflowing size_t; the stride rules of
 *            ezrs_decode when the call has more than one codeword; a workspace that is too small.
 *            Otherwise nstripes == 0 or shard_len == 0 returns 0 and touches nothing.
 *            NOT CHECKED, because the host cannot see the table, and undefined behaviour when
 *            broken: a pointer that is not a multiple of `align`; a NULL (or invalid) entry at any
 *            position below len + NROOTS; any overlap between two buffers of the call, in the same
 *            stripe or in different stripes, or between a buffer and the table, each over [p, p +
 *            shard_len * datum bytes).
 * Asynchronous.  The forms without _ws use the calling stream's workspace (and may grow it, as
 * ezrs_decode_interleaved does); the _ws forms take a caller-owned workspace of >=
 * ezrs_decode_ptrs_workspace_bytes() bytes, allocate nothing and synchronise nothing.  That
 * figure is what a call of either form uses for the geometry (0 for invalid arguments): one
 * stripe's table, (len + NROOTS) pointers rounded up to 256 bytes, then
 * ezrs_interleaved_workspace_bytes(codec, len, shard_len, nstripes). */
size_t ezrs_decode_ptrs_workspace_bytes(const ezrs_codec *codec, unsigned len, size_t shard_len,
                                        size_t nstripes);
int ezrs_decode_ptrs(const ezrs_codec *codec, void *const *shards, unsigned len, size_t shard_len,
                     const uint32_t *eras, size_t eras_stride, const uint32_t *neras,
                     int32_t *result, uint32_t *positions, size_t pos_stride, void *corr,
                     size_t corr_stride, void *stream);
int ezrs_decode_ptrs_ws(const ezrs_codec *codec, void *const *shards, unsigned len,
                        size_t shard_len, const uint32_t *eras, size_t eras_stride,
                        const uint32_t *neras, int32_t *result, uint32_t *positions,
                        size_t pos_stride, void *corr, size_t corr_stride, void *ws,
                        size_t ws_bytes, void *stream);
int ezrs_decode_ptrs_batch(const ezrs_codec *codec, void *const *table, size_t table_pitch,
                           unsigned len, size_t shard_len, size_t nstripes, unsigned align,
                           const uint32_t *eras, size_t eras_stride, const uint32_t *neras,
                           int32_t *result, uint32_t *positions, size_t pos_stride, void *corr,
                           size_t corr_stride, void *stream);
int ezrs_decode_ptrs_batch_ws(const ezrs_codec *codec, void *const *table, size_t table_pitch,
                              unsigned len, size_t shard_len, size_t nstripes, unsigned align,
                              const uint32_t *eras, size_t eras_stride, const uint32_t *neras,
                              int32_t *result, uint32_t *positions, size_t pos_stride, void *corr,
                              size_t corr_stride, void *ws, size_t ws_bytes, void *stream);

/* Selection (device-resident): the end of a scrub.  A verify (ezrs_reconstruct_ptrs_batch or
 * ezrs_reconstruct_interleaved under an nlost == 0 plan) marks the codewords whose check failed with
 * result[k] == -1; the decodes above would gather and decode every codeword of every stripe they
 * name.  These calls list the failed codewords on the device and decode only those, with no host
 * read in between: verify, ezrs_select_failed and a *_select decode can sit in one stream or one
 * captured graph.
 *   ezrs_select_failed       everything is DEVICE memory on the codec's device.  sel[0 .. min(total,
 *            cap) - 1] receives base + k for every k < n with result[k] < 0, in ascending k (the
 *            order is deterministic; neighbouring k land in neighbouring rows of the decode, which is
 *            what gives its gather any coalescing); sel[min(total, cap) .. cap - 1] is set to
 *            EZRS_SEL_NONE; count[0] receives total, which may exceed cap: the caller sees the
 *            overflow when it reads count, the decode clamps.  `codec` supplies the device and, in
 *            the form without _ws, the stream's workspace; nothing else of it is used.  base lets a
 *            caller verify a batch in pieces and number the codewords over the whole.  Three
 *            kernels on `stream` (counts per chunk of results, their scan, the write): no workgroup
 *            ever waits for another one.  Asynchronous; the _ws form takes a caller-owned workspace
 *            of exactly ezrs_select_workspace_bytes(n) bytes or more, allocates nothing and
 *            synchronises nothing.  n == 0 or cap == 0 still writes count[0] (0 for n == 0) and
 *            returns 0.  -EINVAL: a null codec, sel or count; a null result with n != 0; base + n
 *            overflowing 64 bits; a workspace that is too small.
 *   ezrs_decode_ptrs_select / ezrs_decode_interleaved_select   the geometry (table .. nstripes,
 *            frames .. nframes) is that of ezrs_decode_ptrs_batch / ezrs_decode_interleaved and names
 *            the same codewords, k = s*shard_len + j or f*depth + j.  Row i (0 <= i < nsel) of the
 *            call is codeword k = sel[i]: result[i], neras[i] and the rows i of eras, positions and
 *            corr belong to it, so these arrays are compact, sized by nsel and not by the batch, and
 *            follow the stride rules of ezrs_decode over nsel codewords.  Per selected codeword the
 *            bytes left in the shards or frames, the result, the positions and the corrections equal
 *            what the full call produces for codeword k under the same erasures, under both
 *            semantics of the codec (a -1 row carries the reference's partial corrections).  No
 *            symbol of a codeword that is not selected is read for its own sake, and no byte outside
 *            the selected codewords' symbols is ever written: not a codeword that was left out, not
 *            a gap of sym_stride > depth, not a guard byte.
 *            count: nullable DEVICE pointer; the call uses the rows i < min(count[0], nsel).  sel
 *            and count are read by the kernels WHILE THEY RUN, never by the host, so both may be
 *            the outputs of an ezrs_select_failed queued before on the same stream.
 *            A row is skipped when it is past count[0] or its entry is >= nstripes*shard_len
 *            (nframes*depth); EZRS_SEL_NONE is the canonical skip value.  For a skipped row no table
 *            entry and no symbol is read and nothing is scattered; it is staged as the all-zero word,
 *            so result[i] / positions / corr are what ezrs_decode gives for an all-zero codeword of
 *            length len under row i's erasures (0 when there are none).  That keeps the launch shape
 *            a host constant (capturable); a caller who knows the count on the host passes it as
 *            nsel with count == NULL and stages nothing spare.
 *            Entries must be distinct (NOT CHECKED: a duplicate has two rows writing the same
 *            symbols); any order is valid.  Pointers need only the datum's alignment: there is no
 *            `align`, because a row's neighbours are not its codeword's neighbours and symbols move
 *            one element at a time, one memory sector per symbol.  The table is read while the
 *            kernels run; EZRS_PTRS_MAX does not apply; what ezrs_decode_ptrs_batch lists as not
 *            checked holds here for the stripes of the selected codewords.
 *            Checked on the host: what the corresponding full call checks (without align), over nsel
 *            rows for the outputs, and a null sel.  nsel == 0 returns 0 and touches nothing (after
 *            the null-codec check), and so do nstripes == 0, shard_len == 0 and nframes == 0.
 *            Asynchronous.  Rows are staged a bounded number per pass as in the full calls, over
 *            nsel; the forms without _ws use the calling stream's workspace, the _ws forms a
 *            caller-owned one of >= ezrs_decode_select_workspace_bytes(codec, len, nsel) bytes (what
 *            a call of either form uses; 0 for invalid arguments): they allocate nothing and
 *            synchronise nothing. */
#define EZRS_SEL_NONE UINT64_MAX   /* in sel: no codeword, skip this row */
size_t ezrs_select_workspace_bytes(size_t n);
int ezrs_select_failed(const ezrs_codec *codec, const int32_t *result, size_t n, uint64_t base,
                       uint64_t *sel, size_t cap, uint64_t *count, void *stream);
int ezrs_select_failed_ws(const ezrs_codec *codec, const int32_t *result, size_t n, uint64_t base,
                          uint64_t *sel, size_t cap, uint64_t *count, void *ws, size_t ws_bytes,
                          void *stream);
size_t ezrs_decode_select_workspace_bytes(const ezrs_codec *codec, unsigned len, size_t nsel);
int ezrs_decode_ptrs_select(const ezrs_codec *codec, void *const *table, size_t table_pitch,
                            unsigned len, size_t shard_len, size_t nstripes, const uint64_t *sel,
                            size_t nsel, const uint64_t *count, const uint32_t *eras,
                            size_t eras_stride, const uint32_t *neras, int32_t *result,
                            uint32_t *positions, size_t pos_stride, void *corr, size_t corr_stride,
                            void *stream);
int ezrs_decode_ptrs_select_ws(const ezrs_codec *codec, void *const *table, size_t table_pitch,
                               unsigned len, size_t shard_len, size_t nstripes, const uint64_t *sel,
                               size_t nsel, const uint64_t *count, const uint32_t *eras,
                               size_t eras_stride, const uint32_t *neras, int32_t *result,
                               uint32_t *positions, size_t pos_stride, void *corr,
                               size_t corr_stride, void *ws, size_t ws_bytes, void *stream);
int ezrs_decode_interleaved_select(const ezrs_codec *codec, void *frames, size_t frame_pitch,
                                   size_t sym_stride, size_t depth, unsigned len, size_t nframes,
                                   const uint64_t *sel, size_t nsel, const uint64_t *count,
                                   const uint32_t *eras, size_t eras_stride, const uint32_t *neras,
                                   int32_t *result, uint32_t *positions, size_t pos_stride,
                                   void *corr, size_t corr_stride, void *stream);
int ezrs_decode_interleaved_select_ws(const ezrs_codec *codec, void *frames, size_t frame_pitch,
                                      size_t sym_stride, size_t depth, unsigned len, size_t nframes,
                                      const uint64_t *sel, size_t nsel, const uint64_t *count,
                                      const uint32_t *eras, size_t eras_stride,
                                      const uint32_t *neras, int32_t *result, uint32_t *positions,
                                      size_t pos_stride, void *corr, size_t corr_stride, void *ws,
                                      size_t ws_bytes, void *stream);

/* Host-memory forms: the same contracts with HOST pointers.  The batch is streamed through the
 * device in chunks of `chunk` codewords (0 = library default) over two HIP streams with
 * asynchronous copies; pinned host memory (ezrs_host_alloc) gets full PCIe overlap.  Blocking:
 * they return when the results are back in host memory.
 * Encode sends each chunk's rows to the device (one linear copy of the rows' span when the row
 * pitch is at most about twice the row; otherwise the rows are gathered into pinned staging first)
 * and brings back only the parity, as one compact block that is then scattered into place: the
 * caller's data symbols are never written.  Decode sends inline-parity rows as one linear span;
 * back come the results and only the rows whose result is nonzero (compacted on the device, then
 * scattered into place): a clean codeword's row is never written. */
int ezrs_encode_host(ezrs_codec *codec, const void *data, size_t data_stride, unsigned len,
                     void *parity, size_t parity_stride, size_t ncw, size_t chunk);
int ezrs_encode_rows_host(ezrs_codec *codec, void *rows, size_t stride, unsigned len, size_t ncw,
                          size_t chunk);
int ezrs_decode_host(ezrs_codec *codec, void *data, size_t data_stride, unsigned len,
                     void *parity, size_t parity_stride, const uint32_t *eras,
                     size_t eras_stride, const uint32_t *neras, int32_t *result,
                     uint32_t *positions, size_t pos_stride, void *corr, size_t corr_stride,
                     size_t ncw, size_t chunk);

/* rsencode wire format (replaces the per-chunk loop of rsencode.C:93-163, whose encode/decode
 * helpers call RS_t::encode / RS_t::decode once per chunk).  The input is cut into chunks of
 * `chunk` data symbols (the last may be shorter); each chunk is written followed by its NROOTS
 * parity symbols; symbols wider than 8 bits are big-endian on the wire (rsencode.C:52-85).  All
 * chunks of a call are one batch on the device.
 *  - ezrs_stream_encode: out receives at most ezrs_stream_encoded_bound(in_bytes) bytes.
 *  - ezrs_stream_decode: out receives the corrected data without parity (<= in_bytes bytes); a
 *    chunk the decoder cannot correct is passed on as the decoder left it, as rsencode does, and
 *    counted in *n_failed (nullable).
 * A trailing piece that cannot form a chunk (an odd byte for 16-bit symbols; for decode, fewer
 * than NROOTS + 1 symbols -- rsencode.C:110-111, 140-141) returns -EMSGSIZE after the whole
 * chunks before it were written (*out_bytes counts them).  -EINVAL: chunk 0 or above the codec's
 * load; -ENOSPC: out_cap too small. */
size_t ezrs_stream_encoded_bound(const ezrs_codec *codec, size_t in_bytes, unsigned chunk);
int ezrs_stream_encode(ezrs_codec *codec, const void *in, size_t in_bytes, unsigned chunk,
                       void *out, size_t out_cap, size_t *out_bytes);
int ezrs_stream_decode(ezrs_codec *codec, const void *in, size_t in_bytes, unsigned chunk,
                       void *out, size_t out_cap, size_t *out_bytes, size_t *n_failed);

/* Pinned host memory for the host-memory forms (hipHostMalloc / hipHostFree). */
int ezrs_host_alloc(void **ptr, size_t bytes);
int ezrs_host_free(void *ptr);

/* Human-readable text of the last HIP error seen by this thread ("" if none). */
const char *ezrs_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* EZRS_H */
