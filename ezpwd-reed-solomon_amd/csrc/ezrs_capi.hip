// ezrs_capi.hip -- the C ABI of the MI355X RS engine (include/ezrs.h).
//
// Codec objects own their device-resident tables (built once, like the reference's static
// reed_solomon_tabs / genpoly, rs_base:599-635, 1248-1286) and a decode workspace.  Batch entry
// points validate arguments the way the reference's encode<INP>/decode<INP> do
// (rs_base:868-904, 1170-1242) and dispatch to the fastest kernel that is bit-exact for the codec:
// the bit-sliced GF(2^8) kernels where they apply, the generic per-codeword kernels otherwise.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/ezrs.h"
#include "ezrs_internal.hpp"
#include "ezrs_host.hpp"

using namespace ezrs;

struct ezrs_codec {
    CodecMath math;
    int device = 0;
    DevCodec dev{};
    uint16_t *d_tabs = nullptr;   // alpha_to | index_of | genpoly
    uint8_t *d_dual = nullptr;    // into_dual | from_dual
    std::mutex mu;                // guards the lazily grown host-pipeline buffers
    StageBufs<2> d_stage;         // one per pipeline stream
    StageBufs<2, hipHostMallocMapped> h_stage;   // device-visible: k_compact_rows writes here
    hipStream_t streams[2] = {nullptr, nullptr};
    int bs_id = -1;               // bit-sliced GF(2^8) kernel set, -1 if none
    int ps_id = -1;               // plane-sliced GF(2^8) kernel set, -1 if none
    int wide_id = -1;             // GF(2^16) remainder kernel set, -1 if none
    mutable std::atomic<uint32_t> decode_gen{0};   // plane-sliced decode calls (DecodeArgs::flag_gen)
    std::vector<uint16_t> wide_blob;   // host: leader slots | log beta | column tables
    uint16_t *d_wcols = nullptr;  // device copy of the column tables (constant multipliers)
    // Device workspaces of the batch entry points, one per HIP stream: calls on different streams
    // never share scratch memory, calls on one stream are ordered by the stream.  A workspace only
    // grows; the buffer it replaces is kept until ezrs_destroy, so work already queued (or a
    // captured graph) that still points at it stays valid.  No entry point synchronises the device.
    struct Ws {
        void *p = nullptr;
        size_t bytes = 0;
    };
    mutable std::mutex ws_mu;
    mutable std::unordered_map<void *, Ws> ws;
    mutable std::vector<void *> ws_retired;
};

// What the plans of the frame-in-place kernels share: copies of what they need from the codec, and
// the device table (recon_table).  A plan is const after its *_create.
struct FramePlan {
    int device = 0;
    unsigned mm = 0, nroots = 0, len = 0;
    uint32_t *d_tab = nullptr;
    virtual ~FramePlan() = default;   // destroy_plan deletes either plan through this type
};

// A reconstruction plan: one loss pattern of one codec and length.
struct ezrs_recon : FramePlan {
    unsigned nlost = 0, nsurv = 0;
    std::vector<uint32_t> surv, lost;   // host copies of the table's position lists (the pointer form)
};

// A parity-update plan: one set of changed data positions of one codec and length.  Its table has
// survivors = changed, lost = the parity positions.
struct ezrs_update : FramePlan {
    unsigned nchg = 0;
    std::vector<uint32_t> chg;          // host copy of the changed positions (the pointer form)
};

// A set of plans of one kind and one codec geometry in one device allocation (ReconMixedArgs,
// UpdateMixedArgs): copies of the plans' tables behind a directory.  Const after its *_set_create;
// it keeps nothing of the plans it was made from.
struct PlanSet {
    int device = 0;
    unsigned mm = 0, nroots = 0, len = 0;
    unsigned nplans = 0;
    unsigned most = 0;                  // the largest nlost (reconstruction), nchanged (update) of the plans
    uint32_t *d_set = nullptr;
};
struct ezrs_recon_set : PlanSet {};
struct ezrs_update_set : PlanSet {};

namespace {

constexpr size_t kReconMaxTable = (size_t)64 << 20;   // bytes of a plan's device table (engine limit)

thread_local std::string g_last_error;

int hip_fail(hipError_t e, const char *what) { return ezrs::hip_fail(g_last_error, e, what); }

// Standard field polynomial per symbol size (rs:75-89).
unsigned std_poly(unsigned mm) {
    static const unsigned p[17] = {0, 0, 0x7, 0xb, 0x13, 0x25, 0x43, 0x89, 0x11d, 0x211, 0x409,
                                   0x805, 0x1053, 0x201b, 0x4443, 0x8003, 0x1100b};
    return mm <= 16 ? p[mm] : 0;
}

template <class S>
int destroy_set(S *s) {
    if (!s) return 0;
    DeviceGuard g(s->device);
    if (s->d_set) (void)hipFree(s->d_set);
    delete s;
    return 0;
}

// What ezrs_recon_set_create and ezrs_update_set_create share: S the set, P the plan (a FramePlan),
// kind: the set's name in the error texts; counts(plan): the survivors and the lost positions of the
// plan's recon_table image, i.e. (nsurv, nlost) or (nchanged, NROOTS); most_lost: PlanSet::most is
// the largest of the second of them, else of the first.
template <class S, class P, class F>
int create_set(S **out, const P *const *plans, unsigned nplans, const char *kind, F &&counts, bool most_lost) {
    if (!out) return -EINVAL;
    *out = nullptr;
    auto bad = [kind](const char *what) {
        g_last_error = std::string(kind) + ": " + what;
        return -EINVAL;
    };
    if (!plans) return bad("null plans");
    if (!nplans) return bad("no plans");
    for (unsigned i = 0; i < nplans; ++i)
        if (!plans[i]) return bad("a NULL plan");
    const FramePlan *const p0 = plans[0];
    for (unsigned i = 1; i < nplans; ++i) {
        const FramePlan *const p = plans[i];
        if (p->mm != p0->mm || p->nroots != p0->nroots || p->len != p0->len || p->device != p0->device)
            return bad("plans that differ in symbol bits, NROOTS, len or device");
    }
    // directory | images, each at a multiple of kReconSetAlign dwords
    auto up = [](size_t w) { return (w + kReconSetAlign - 1) / kReconSetAlign * kReconSetAlign; };
    const size_t cap = kReconMaxTable / sizeof(uint32_t), ent = sizeof(ReconSetEntry) / sizeof(uint32_t);
    size_t words = nplans <= cap / ent ? up(nplans * ent) : cap + 1;
    std::vector<ReconSetEntry> dir;
    std::vector<size_t> image;                      // dwords of plan i's table
    unsigned most = 0;
    try {
        for (unsigned i = 0; i < nplans && words <= cap; ++i) {
            const std::pair<unsigned, unsigned> c = counts(*plans[i]);
            const unsigned nsurv = c.first, nlost = c.second;
            dir.push_back({(uint32_t)words, nsurv, nlost,
                           (uint32_t)(words + recon_coef_words(p0->mm, p0->nroots, nsurv))});
            image.push_back(recon_table_words(p0->mm, p0->nroots, nsurv, nlost));
            words += up(image.back());
            most = std::max(most, most_lost ? nlost : nsurv);
        }
    } catch (const std::bad_alloc &) {
        return -ENOMEM;
    }
    if (words > cap) {
        g_last_error = std::string(kind) + ": device tables above 64 MiB together";
        return -ENOTSUP;
    }
    S *s = new (std::nothrow) S;
    if (!s) return -ENOMEM;
    s->device = p0->device;
    s->mm = p0->mm;
    s->nroots = p0->nroots;
    s->len = p0->len;
    s->nplans = nplans;
    s->most = most;
    DeviceGuard g(s->device);
    hipError_t e;
    if ((e = hipMalloc(&s->d_set, words * sizeof(uint32_t))) != hipSuccess) {
        delete s;
        return hip_fail(e, ("hipMalloc(" + std::string(kind) + ")").c_str());
    }
    e = hipMemset(s->d_set, 0, words * sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemcpy(s->d_set, dir.data(), dir.size() * sizeof(ReconSetEntry), hipMemcpyHostToDevice);
    for (unsigned i = 0; i < nplans && e == hipSuccess; ++i)
        e = hipMemcpy(s->d_set + dir[i].off, plans[i]->d_tab, image[i] * sizeof(uint32_t),
                      hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // the plans may be destroyed at once
    if (e != hipSuccess) {
        destroy_set(s);
        return hip_fail(e, ("copy of the plans' tables (" + std::string(kind) + ")").c_str());
    }
    *out = s;
    return 0;
}

} // namespace

extern "C" {

int ezrs_abi_version(void) { return EZRS_ABI_VERSION; }

int ezrs_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    return n;
}

const char *ezrs_last_error(void) { return g_last_error.c_str(); }

int ezrs_create(ezrs_codec **out, unsigned symbol_bits, unsigned poly, unsigned fcr,
                unsigned prim, unsigned nroots, int dual, int device) {
    if (!out) return -EINVAL;
    *out = nullptr;
    CodecSpec spec{symbol_bits, poly, fcr, prim, nroots, dual ? 1 : 0};
    ezrs_codec *c = new (std::nothrow) ezrs_codec;
    if (!c) return -ENOMEM;
    if (!c->math.build(spec)) {
        delete c;
        g_last_error = "invalid RS codec parameters";
        return -EINVAL;
    }
    if (symbol_bits > 8 && nroots > 256) {
        // the wide-symbol kernels keep at most 256 parity symbols' working state per lane
        delete c;
        g_last_error = "RS codecs with symbols wider than 8 bits support at most 256 parity symbols";
        return -ENOTSUP;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0 || device < 0 || device >= ndev) {
        delete c;
        g_last_error = "no usable HIP device";
        return -ENODEV;
    }
    c->device = device;
    DeviceGuard g(device);
    const CodecMath &m = c->math;
    const size_t ntab = 2 * (size_t)(m.nn + 1) + (m.spec.nroots + 1);
    if ((e = hipMalloc(&c->d_tabs, ntab * sizeof(uint16_t))) != hipSuccess ||
        (e = hipMalloc(&c->d_dual, 512)) != hipSuccess) {
        ezrs_destroy(c);
        return hip_fail(e, "hipMalloc(tables)");
    }
    std::vector<uint16_t> h(ntab);
    std::copy(m.gf.alpha_to.begin(), m.gf.alpha_to.end(), h.begin());
    std::copy(m.gf.index_of.begin(), m.gf.index_of.end(), h.begin() + (m.nn + 1));
    std::copy(m.genpoly.begin(), m.genpoly.end(), h.begin() + 2 * (m.nn + 1));
    uint8_t dm[512];
    std::memcpy(dm, m.into_dual, 256);
    std::memcpy(dm + 256, m.from_dual, 256);
    if ((e = hipMemcpy(c->d_tabs, h.data(), ntab * sizeof(uint16_t), hipMemcpyHostToDevice)) !=
            hipSuccess ||
        (e = hipMemcpy(c->d_dual, dm, 512, hipMemcpyHostToDevice)) != hipSuccess) {
        ezrs_destroy(c);
        return hip_fail(e, "hipMemcpy(tables)");
    }
    DevCodec &d = c->dev;
    d.mm = m.spec.mm; d.nn = m.nn; d.nroots = m.spec.nroots; d.load = m.load;
    d.fcr = m.spec.fcr; d.prim = m.spec.prim; d.iprim = m.iprim; d.dual = m.spec.dual;
    d.poly = m.spec.poly;
    d.masked = m.spec.mm != (m.spec.mm <= 8 ? 8u : 16u);
    d.alpha_to = c->d_tabs;
    d.index_of = c->d_tabs + (m.nn + 1);
    d.genpoly = c->d_tabs + 2 * (m.nn + 1);
    d.into_dual = c->d_dual;
    d.from_dual = c->d_dual + 256;
    if (hipDeviceGetAttribute(&d.ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
        d.ncu = 0;
    c->bs_id = bitslice_codec_id(d);
    // EZRS_NO_PLANESLICE=1 keeps the per-symbol bit-sliced kernels (A/B measurements)
    const char *nops = getenv("EZRS_NO_PLANESLICE");
    c->ps_id = (nops && *nops == '1') ? -1 : planeslice_codec_id(d);
    // EZRS_NO_WIDE=1 keeps the lane-group GF(2^16) kernels (A/B measurements)
    const char *now = getenv("EZRS_NO_WIDE");
    c->wide_id = (now && *now == '1') ? -1 : wide_codec_id(d);
    if (c->wide_id >= 0) {
        if (!wide_build_consts(c->wide_id, m, c->wide_blob)) {
            c->wide_id = -1;
        } else {
            const size_t qn = wide_cols_count(m.spec.nroots);
            if ((e = hipMalloc(&c->d_wcols, qn * sizeof(uint16_t))) != hipSuccess ||
                (e = hipMemcpy(c->d_wcols, c->wide_blob.data() + 64, qn * sizeof(uint16_t),
                               hipMemcpyHostToDevice)) != hipSuccess) {
                ezrs_destroy(c);
                return hip_fail(e, "hipMalloc(wide tables)");
            }
        }
    }
    *out = c;
    return 0;
}

int ezrs_create_rs(ezrs_codec **out, unsigned n, unsigned k, int device) {
    unsigned mm = 0;
    while (mm < 17 && ((1u << mm) - 1) < n) ++mm;
    if (mm < 2 || mm > 16 || ((1u << mm) - 1) != n || k == 0 || k >= n) {
        if (out) *out = nullptr;
        g_last_error = "RS<N,K>: N must be 2^m-1 (m = 2..16) and 0 < K < N";
        return -EINVAL;
    }
    return ezrs_create(out, mm, std_poly(mm), 1, 1, n - k, 0, device);
}

int ezrs_create_ccsds(ezrs_codec **out, unsigned k, int dual, int device) {
    if (k == 0 || k >= 255 || ((255 - k) & 1)) {
        if (out) *out = nullptr;
        g_last_error = "RS_CCSDS<255,K>: K must leave an even number of parity symbols";
        return -EINVAL;
    }
    return ezrs_create(out, 8, 0x187, 128 - (255 - k) / 2, 11, 255 - k, dual ? 1 : 0, device);
}

int ezrs_destroy(ezrs_codec *c) {
    if (!c) return 0;
    DeviceGuard g(c->device);
    (void)hipFree(c->d_tabs);
    (void)hipFree(c->d_dual);
    if (c->d_wcols) (void)hipFree(c->d_wcols);
    for (auto &kv : c->ws) (void)hipFree(kv.second.p);
    for (void *p : c->ws_retired) (void)hipFree(p);
    c->d_stage.release();
    c->h_stage.release();
    for (int i = 0; i < 2; ++i)
        if (c->streams[i]) (void)hipStreamDestroy(c->streams[i]);
    delete c;
    return 0;
}

int ezrs_set_semantics(ezrs_codec *c, int semantics) {
    if (!c || (semantics != EZRS_SEM_EZPWD && semantics != EZRS_SEM_KARN)) return -EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->dev.karn = semantics == EZRS_SEM_KARN;
    return 0;
}

int ezrs_set_launch_rows(ezrs_codec *c, size_t rows) {
    if (!c) return -EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    c->dev.launch_rows = rows;
    return 0;
}

int ezrs_get_semantics(const ezrs_codec *c) {
    if (!c) return -EINVAL;
    return c->dev.karn ? EZRS_SEM_KARN : EZRS_SEM_EZPWD;
}

int ezrs_kernel_path(const ezrs_codec *c) {
    if (!c) return -EINVAL;
    if (c->ps_id >= 0) return EZRS_PATH_PLANESLICE;
    if (c->wide_id >= 0) return EZRS_PATH_WIDE;
    if (c->bs_id >= 0) return EZRS_PATH_BITSLICE;
    return EZRS_PATH_GENERIC;
}

int ezrs_get_info(const ezrs_codec *c, ezrs_info *info) {
    if (!c || !info) return -EINVAL;
    const CodecMath &m = c->math;
    info->symbol_bits = m.spec.mm;
    info->size = m.nn;
    info->nroots = m.spec.nroots;
    info->load = m.load;
    info->poly = m.spec.poly;
    info->fcr = m.spec.fcr;
    info->prim = m.spec.prim;
    info->datum_bytes = sym_bytes(c->dev);
    info->dual = m.spec.dual;
    info->device = c->device;
    return 0;
}

namespace {

// Device scratch bytes one batch call of ncw codewords needs (encode and decode alike).
size_t ws_bytes_for(const ezrs_codec *c, size_t ncw) {
    size_t b = 0;                                          // both >= ncw * 32 (decode's need)
    if (c->bs_id >= 0) b = bs_encode_ws_bytes(ncw);
    if (c->ps_id >= 0 && ps_ws_bytes(ncw) + 256 > b) b = ps_ws_bytes(ncw) + 256;   // + the flag word
    if (c->wide_id >= 0 && wide_ws_bytes(c->wide_id, ncw) > b) b = wide_ws_bytes(c->wide_id, ncw);
    return b;
}

// The calling stream's workspace, grown to at least `bytes` (see ezrs_codec::Ws).
int stream_ws(const ezrs_codec *c, void *stream, size_t bytes, void **out) {
    *out = nullptr;
    if (!bytes) return 0;
    std::lock_guard<std::mutex> lk(c->ws_mu);
    ezrs_codec::Ws &w = c->ws[stream];
    if (w.bytes < bytes) {
        const size_t grow = w.bytes + w.bytes / 2 > bytes ? w.bytes + w.bytes / 2 : bytes;
        void *p = nullptr;
        HIP_TRY(hipMalloc(&p, grow));
        if (w.p) c->ws_retired.push_back(w.p);
        w.p = p;
        w.bytes = grow;
    }
    *out = w.p;
    return 0;
}

} // namespace

namespace {

// The one place that picks kernels: every entry point (device or host-memory) goes through these.
// ws: bs_encode_ws_bytes(ncw) bytes (bit-sliced path only).
hipError_t dispatch_encode(const ezrs_codec *c, const EncodeArgs &a, void *ws, hipStream_t st) {
    if (c->ps_id >= 0 && ps_can_encode(c->dev, a)) return launch_ps_encode(c->ps_id, c->dev, a, ws, st);
    if (a.sh.rows) return launch_encode_generic(c->dev, a, st);     // shard rows: per-codeword kernels
    if (c->wide_id >= 0 && wide_can_encode(c->dev, a))
        return launch_wide_encode(c->wide_id, c->dev, a, c->wide_blob.data(), c->d_wcols, ws, st);
    return c->bs_id >= 0 ? launch_bs_encode(c->bs_id, c->dev, a, ws, st) : launch_encode_generic(c->dev, a, st);
}

// syn_ws: the sliced paths' syndrome workspace (ws_bytes_for).
hipError_t dispatch_decode(const ezrs_codec *c, const DecodeArgs &a, uint8_t *syn_ws,
                           hipStream_t st) {
    const unsigned w = sym_bytes(c->dev);
    const bool contiguous = a.parity == static_cast<char *>(a.data) + (size_t)a.len * w &&
                            a.parity_stride == a.data_stride;
    if (c->ps_id >= 0 && ps_can_decode(c->dev, a)) {
        // the call's flag word (after the tiled syndromes) and a value no earlier call stored there
        // (a stale match only costs the error path's full screen)
        DecodeArgs b = a;
        b.flag_word = reinterpret_cast<uint32_t *>(syn_ws + ps_ws_bytes(a.ncw));
        b.flag_gen = c->decode_gen.fetch_add(1, std::memory_order_relaxed) + 1;
        hipError_t e = launch_ps_syndromes(c->ps_id, c->dev, b, syn_ws, st);
        if (e == hipSuccess) e = launch_decode_flagged(c->dev, b, syn_ws, SynLayout::Tiled, st);
        return e;
    }
    if (a.sh.rows) return launch_decode_generic(c->dev, a, st);     // shard rows: per-codeword kernels
    // the GF(2^16) error path keeps ezpwd's semantics only: Karn-mode codecs decode on the
    // per-codeword kernels (same syndromes, Karn's frame and checks)
    if (c->wide_id >= 0 && !c->dev.karn && wide_can_decode(c->dev, a))
        return launch_wide_decode(c->wide_id, c->dev, a, c->wide_blob.data(), c->d_wcols, syn_ws, st);
    if (c->bs_id >= 0 && contiguous) {
        // Bit-sliced syndromes for the whole batch; the reference algorithm only for the codewords
        // that are not valid as received (or carry erasures to validate).
        hipError_t e = launch_bs_syndromes(c->bs_id, c->dev, a, syn_ws, st);
        if (e == hipSuccess) e = launch_decode_flagged(c->dev, a, syn_ws, SynLayout::Rows, st);
        return e;
    }
    return launch_decode_generic(c->dev, a, st);
}

} // namespace

int ezrs_reserve(ezrs_codec *c, size_t ncw) { return ezrs_reserve_stream(c, ncw, nullptr); }

int ezrs_reserve_stream(const ezrs_codec *c, size_t ncw, void *stream) {
    if (!c) return -EINVAL;
    DeviceGuard g(c->device);
    void *p;
    return stream_ws(c, stream, ws_bytes_for(c, ncw), &p);
}

size_t ezrs_workspace_bytes(const ezrs_codec *c, size_t ncw) {
    return c ? ws_bytes_for(c, ncw) : 0;
}

namespace {

// Row geometry of a batch: the argument checks of encode<INP> / decode<INP> (rs_base:868-904,
// 1170-1242).  parity == NULL is the row form (rs_base:778-790), legal where row_form is set: the
// parity follows the data in each row, and parity / parity_stride are resolved to it.  The stride
// rules hold for ncw > 1 only (one codeword may pass any stride, 0 included).
int check_rows(const ezrs_codec *c, const void *data, size_t data_stride, unsigned len,
               void *&parity, size_t &parity_stride, size_t ncw, bool row_form) {
    if (!data || (!parity && !row_form)) return -EINVAL;
    const unsigned NR = c->dev.nroots;
    if (len < 1 || len > c->dev.load) return -EINVAL;                 // rs_base:875-877
    if (!parity) {
        parity = static_cast<char *>(const_cast<void *>(data)) + (size_t)len * sym_bytes(c->dev);
        parity_stride = data_stride;
        if (ncw > 1 && data_stride < (size_t)len + NR) return -EINVAL;
    } else if (ncw > 1 && parity_stride < NR) {
        return -EINVAL;
    }
    if (ncw > 1 && data_stride < len) return -EINVAL;
    return 0;
}

// What a decode returns per codeword, and the erasures it takes (strides in elements; ezrs_decode).
struct DecodeOut {
    const uint32_t *eras;
    size_t eras_stride;
    const uint32_t *neras;
    int32_t *result;
    uint32_t *positions;
    size_t pos_stride;
    void *corr;
    size_t corr_stride;

    // Decode of n codewords whose rows are given as they lie (data, parity) and whose outputs are
    // entries k0 .. k0 + n - 1 of this.  One codeword: a zero stride is harmless (row 0 only).
    DecodeArgs args(const ezrs_codec *c, void *data, size_t data_stride, unsigned len, void *parity,
                    size_t parity_stride, size_t k0, size_t n, const Shards &sh = {}) const {
        return {data, data_stride, len, parity, parity_stride,
                eras ? eras + k0 * eras_stride : nullptr, eras_stride, neras ? neras + k0 : nullptr,
                result + k0, positions ? positions + k0 * pos_stride : nullptr, pos_stride,
                corr ? static_cast<char *>(corr) + k0 * corr_stride * sym_bytes(c->dev) : nullptr,
                corr_stride, n, sh};
    }
};

int check_decode_out(const ezrs_codec *c, size_t ncw, const DecodeOut &o) {
    const unsigned NR = c->dev.nroots;
    if (!o.result) return -EINVAL;
    if (o.neras && !o.eras) return -EINVAL;
    if (o.eras && ncw > 1 && o.eras_stride == 0) return -EINVAL;
    if (o.positions && ncw > 1 && o.pos_stride < NR) return -EINVAL;
    if (o.corr && ncw > 1 && o.corr_stride < NR) return -EINVAL;
    return 0;
}

// A workspace the caller owns (the _ws forms); the other forms use the calling stream's.
struct CallerWs {
    void *p;
    size_t bytes;
};

int take_ws(const ezrs_codec *c, const CallerWs *cw, size_t need, void *stream, void **ws) {
    if (!cw) return stream_ws(c, stream, need, ws);
    *ws = cw->p;
    return cw->bytes < need || (cw->bytes && !cw->p) ? -EINVAL : 0;
}

int run_encode(const ezrs_codec *c, const EncodeArgs &a, void *ws, void *stream) {
    hipError_t e = dispatch_encode(c, a, ws, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "encode launch");
}

int run_decode(const ezrs_codec *c, const DecodeArgs &a, void *ws, void *stream) {
    hipError_t e = dispatch_decode(c, a, static_cast<uint8_t *>(ws), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "decode launch");
}

// One checked batch on the device (the encode `ea`, or else the decode `da`): the codec's device,
// the workspace, the kernels.
int run_batch(const ezrs_codec *c, const EncodeArgs *ea, const DecodeArgs *da, const CallerWs *cw,
              void *stream) {
    DeviceGuard g(c->device);
    void *ws = nullptr;
    if (int r = take_ws(c, cw, ws_bytes_for(c, ea ? ea->ncw : da->ncw), stream, &ws)) return r;
    return ea ? run_encode(c, *ea, ws, stream) : run_decode(c, *da, ws, stream);
}

int encode_dev(const ezrs_codec *c, const void *data, size_t data_stride, unsigned len, void *parity,
               size_t parity_stride, size_t ncw, bool row_form, const CallerWs *cw, void *stream) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (int r = check_rows(c, data, data_stride, len, parity, parity_stride, ncw, row_form)) return r;
    const EncodeArgs a{data, data_stride, len, parity, parity_stride, ncw};
    return run_batch(c, &a, nullptr, cw, stream);
}

int decode_dev(const ezrs_codec *c, void *data, size_t data_stride, unsigned len, void *parity,
               size_t parity_stride, const DecodeOut &o, size_t ncw, const CallerWs *cw, void *stream) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (int r = check_rows(c, data, data_stride, len, parity, parity_stride, ncw, true)) return r;
    if (int r = check_decode_out(c, ncw, o)) return r;
    const DecodeArgs a = o.args(c, data, data_stride, len, parity, parity_stride, 0, ncw);
    return run_batch(c, nullptr, &a, cw, stream);
}

} // namespace

int ezrs_encode_ws(const ezrs_codec *c, const void *data, size_t data_stride, unsigned len,
                   void *parity, size_t parity_stride, size_t ncw, void *ws, size_t ws_bytes,
                   void *stream) {
    const CallerWs cw{ws, ws_bytes};
    return encode_dev(c, data, data_stride, len, parity, parity_stride, ncw, false, &cw, stream);
}

int ezrs_encode(const ezrs_codec *c, const void *data, size_t data_stride, unsigned len,
                void *parity, size_t parity_stride, size_t ncw, void *stream) {
    return encode_dev(c, data, data_stride, len, parity, parity_stride, ncw, false, nullptr, stream);
}

int ezrs_encode_rows_ws(const ezrs_codec *c, void *rows, size_t stride, unsigned len, size_t ncw,
                        void *ws, size_t ws_bytes, void *stream) {
    const CallerWs cw{ws, ws_bytes};
    return encode_dev(c, rows, stride, len, nullptr, 0, ncw, true, &cw, stream);
}

int ezrs_encode_rows(const ezrs_codec *c, void *rows, size_t stride, unsigned len, size_t ncw,
                     void *stream) {
    return encode_dev(c, rows, stride, len, nullptr, 0, ncw, true, nullptr, stream);
}

int ezrs_decode_ws(const ezrs_codec *c, void *data, size_t data_stride, unsigned len,
                   void *parity, size_t parity_stride, const uint32_t *eras, size_t eras_stride,
                   const uint32_t *neras, int32_t *result, uint32_t *positions, size_t pos_stride,
                   void *corr, size_t corr_stride, size_t ncw, void *ws, size_t ws_bytes,
                   void *stream) {
    const CallerWs cw{ws, ws_bytes};
    return decode_dev(c, data, data_stride, len, parity, parity_stride,
                      {eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride}, ncw,
                      &cw, stream);
}

int ezrs_decode(const ezrs_codec *c, void *data, size_t data_stride, unsigned len, void *parity,
                size_t parity_stride, const uint32_t *eras, size_t eras_stride,
                const uint32_t *neras, int32_t *result, uint32_t *positions, size_t pos_stride,
                void *corr, size_t corr_stride, size_t ncw, void *stream) {
    return decode_dev(c, data, data_stride, len, parity, parity_stride,
                      {eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride}, ncw,
                      nullptr, stream);
}

// ---- shard batches -----------------------------------------------------------------------------
namespace {

// Rows per shard and the geometry of a shard batch (rsencode layout); false on bad arguments.
bool shard_geom(const ezrs_codec *c, size_t shard_len, unsigned chunk, size_t shard_pitch, Shards &g) {
    if (!c || shard_len == 0 || chunk == 0 || chunk > c->dev.load) return false;
    const size_t R = (shard_len + chunk - 1) / chunk;
    if (R > 0xFFFFFFFFu) return false;
    const size_t enc = shard_len + R * c->dev.nroots;
    if (shard_pitch < enc) return false;
    g.rows = (uint32_t)R;
    g.tail = (uint32_t)(shard_len - (R - 1) * chunk);
    g.pitch = shard_pitch;
    return true;
}

} // namespace

size_t ezrs_shard_codewords(const ezrs_codec *c, size_t shard_len, unsigned chunk) {
    if (!c || shard_len == 0 || chunk == 0 || chunk > c->dev.load) return 0;
    return (shard_len + chunk - 1) / chunk;
}

size_t ezrs_shard_encoded_len(const ezrs_codec *c, size_t shard_len, unsigned chunk) {
    const size_t R = ezrs_shard_codewords(c, shard_len, chunk);
    return R ? shard_len + R * c->dev.nroots : 0;
}

int ezrs_encode_shards(const ezrs_codec *c, void *shards, size_t shard_pitch, size_t shard_len,
                       unsigned chunk, size_t nshards, void *stream) {
    Shards g;
    if (!c || !shards || !shard_geom(c, shard_len, chunk, shard_pitch, g)) return -EINVAL;
    if (nshards == 0) return 0;
    const size_t row = (size_t)chunk + c->dev.nroots;
    char *r0 = static_cast<char *>(shards);
    const EncodeArgs a{r0, row, chunk, r0 + (size_t)chunk * sym_bytes(c->dev), row, nshards * g.rows, g};
    return run_batch(c, &a, nullptr, nullptr, stream);
}

int ezrs_decode_shards(const ezrs_codec *c, void *shards, size_t shard_pitch, size_t shard_len,
                       unsigned chunk, size_t nshards, const uint32_t *eras, size_t eras_stride,
                       const uint32_t *neras, int32_t *result, uint32_t *positions,
                       size_t pos_stride, void *corr, size_t corr_stride, void *stream) {
    Shards g;
    if (!c || !shards || !result || !shard_geom(c, shard_len, chunk, shard_pitch, g)) return -EINVAL;
    if (nshards == 0) return 0;
    const DecodeOut o{eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride};
    const size_t row = (size_t)chunk + c->dev.nroots, ncw = nshards * g.rows;
    if (int r = check_decode_out(c, ncw, o)) return r;
    char *r0 = static_cast<char *>(shards);
    const DecodeArgs a = o.args(c, r0, row, chunk, r0 + (size_t)chunk * sym_bytes(c->dev), row, 0, ncw, g);
    return run_batch(c, nullptr, &a, nullptr, stream);
}

// ---- interleaved frames ------------------------------------------------------------------------
namespace {

// Codewords staged per pass: whole tiles whose staged rows stay well inside the 256 MiB Infinity
// Cache (EZRS_IL_STAGE_MB, default 64; 0 = the whole batch in one pass, for A/B measurements),
// capped by the launch_rows test hook rounded up to whole tiles.
size_t il_chunk_rows(const ezrs_codec *c, unsigned len, size_t ncw) {
    const size_t w = sym_bytes(c->dev), row = ((size_t)len + c->dev.nroots) * w;
    size_t n = ncw < kIlMaxRows ? ncw : kIlMaxRows;
    const char *e = getenv("EZRS_IL_STAGE_MB");
    const size_t mb = e ? (size_t)strtoull(e, nullptr, 10) : 64;
    if (mb) {
        size_t by = (mb << 20) / row / kIlTile * kIlTile;
        if (by < kIlTile) by = kIlTile;
        if (by < n) n = by;
    }
    if (c->dev.launch_rows) {
        const size_t lr = (c->dev.launch_rows + kIlTile - 1) / kIlTile * kIlTile;
        if (lr < n) n = lr;
    }
    if (n < ncw) {                                  // equal passes: no short last one
        const size_t passes = (ncw + n - 1) / n;
        n = ((ncw + passes - 1) / passes + kIlTile - 1) / kIlTile * kIlTile;
    }
    return n;
}

// Workspace of an interleaved call: the codec's own region for one pass, then the staged rows.
size_t il_ws_codec(const ezrs_codec *c, size_t chunk) { return (ws_bytes_for(c, chunk) + 255) & ~(size_t)255; }
size_t il_ws_bytes(const ezrs_codec *c, unsigned len, size_t ncw) {
    const size_t w = sym_bytes(c->dev), chunk = il_chunk_rows(c, len, ncw);
    return il_ws_codec(c, chunk) + il_stage_bytes(chunk, (size_t)len + c->dev.nroots, w);
}

// The geometry of nframes >= 1 frames of ns symbol rows (every call that takes frames): the rows
// of a frame and the frames must not overlap, and nframes * depth must fit.  The pitch of a single
// frame is not used and is set to 0.
int frames_check(const void *frames, size_t &frame_pitch, size_t sym_stride, size_t depth, size_t ns,
                 size_t nframes) {
    if (!frames || depth == 0 || sym_stride < depth) return -EINVAL;
    if (nframes > 1 && frame_pitch < (ns - 1) * sym_stride + depth) return -EINVAL;
    if (depth > SIZE_MAX / nframes) return -EINVAL;
    if (nframes == 1) frame_pitch = 0;
    return 0;
}

// Argument checks shared by the interleaved calls; ncw = nframes * depth.
int il_check(const ezrs_codec *c, const void *frames, size_t &frame_pitch, size_t sym_stride,
             size_t depth, unsigned len, size_t nframes, size_t &ncw) {
    if (!c || len < 1 || len > c->dev.load) return -EINVAL;
    if (int r = frames_check(frames, frame_pitch, sym_stride, depth, (size_t)len + c->dev.nroots, nframes))
        return r;
    ncw = depth * nframes;
    return 0;
}

// The frames of a pointer-form decode (ezrs_decode_ptrs / ezrs_decode_ptrs_batch): the table on the
// device (pitch entries per stripe, every pointer a multiple of al), or else one stripe's pointers
// by value, which the call first writes to the head of its workspace as a table of pitch entries.
struct IlPtrs {
    void *const *table;
    size_t pitch, al;
    const PtrTable *stripe;
};

// The head of a pointer-form decode's workspace: room for one stripe's table (ezrs_decode_ptrs).
size_t il_ptrs_head(size_t positions) { return (positions * sizeof(void *) + 255) & ~(size_t)255; }

// Both directions, pass by pass: gather, the codec's row kernels on the staged rows, scatter.
//   encode (dec == null): gather the data symbols, scatter the parity symbols of every codeword
//   decode: gather whole codewords, scatter whole rows of the codewords whose result is nonzero
// pt != null: the frames are named by pointers (`frames` is null, depth the shard length).
// sl != null (a decode): the selection policy.  ncw then counts the rows of sl->sel, which are what
// the passes, the workspace and the outputs follow; the codewords they name are sl->ncw.
struct IlSelect {
    const uint64_t *sel, *count;
    size_t ncw;
};

int il_run(const ezrs_codec *c, void *frames, size_t frame_pitch, size_t sym_stride, size_t depth,
           unsigned len, size_t ncw, const DecodeOut *dec, const CallerWs *cw, void *stream,
           const IlPtrs *pt = nullptr, const IlSelect *sl = nullptr) {
    DeviceGuard g(c->device);
    void *ws = nullptr;
    const unsigned NR = c->dev.nroots;
    const size_t w = sym_bytes(c->dev), P = (size_t)len + NR;
    const size_t head = pt && !sl ? il_ptrs_head(P) : 0;
    if (int r = take_ws(c, cw, head + il_ws_bytes(c, len, ncw), stream, &ws)) return r;
    hipStream_t st = static_cast<hipStream_t>(stream);
    void *const *table = pt ? pt->table : nullptr;
    if (pt && pt->stripe) {
        hipError_t e = launch_il_table(*pt->stripe, (unsigned)P, static_cast<void **>(ws), st);
        if (e != hipSuccess) return hip_fail(e, "pointer table launch");
        table = static_cast<void *const *>(ws);
    }
    ws = static_cast<char *>(ws) + head;
    const size_t chunk = il_chunk_rows(c, len, ncw);
    char *stage =static_cast<char *>(ws) + il_ws_codec(c, chunk);
    for (size_t k0 = 0; k0 < ncw; k0 += chunk) {
        const size_t n = ncw - k0 < chunk ? ncw - k0 : chunk;
        IlPtrArgs a{{frames, frame_pitch, sym_stride, depth, stage, P, k0, (uint32_t)n, 0, dec ? len + NR : len,
                     nullptr}, table, pt ? pt->pitch : 0};
        IlSel<IlPtrArgs> as{a, sl ? sl->sel : nullptr, sl ? sl->count : nullptr, sl ? sl->ncw : 0};
        hipError_t e = sl   ? launch_il_gather(c->dev, as, pt != nullptr, st)
                       : pt ? launch_il_gather(c->dev, a, pt->al, st)
                            : launch_il_gather(c->dev, (const IlArgs &)a, st);
        if (e != hipSuccess) return hip_fail(e, "interleaved gather launch");
        if (!dec) {
            if (int r = run_encode(c, EncodeArgs{stage, P, len, stage + (size_t)len * w, P, n}, ws, stream))
                return r;
            a.s0 = len;
            a.s1 = len + NR;
        } else {
            if (int r = run_decode(c, dec->args(c, stage, P, len, stage + (size_t)len * w, P, k0, n), ws, stream))
                return r;
            a.result = as.result = dec->result + k0;
        }
        e = sl   ? launch_il_scatter(c->dev, as, pt != nullptr, st)
            : pt ? launch_il_scatter(c->dev, a, pt->al, st)
                 : launch_il_scatter(c->dev, (const IlArgs &)a, st);
        if (e != hipSuccess) return hip_fail(e, "interleaved scatter launch");
    }
    return 0;
}

// The four interleaved entry points: dec == null encodes; cw == null uses the stream's workspace.
int il_call(const ezrs_codec *c, void *frames, size_t frame_pitch, size_t sym_stride, size_t depth,
            unsigned len, size_t nframes, const DecodeOut *dec, const CallerWs *cw, void *stream) {
    if (!c) return -EINVAL;
    if (nframes == 0) return 0;
    size_t ncw;
    if (int r = il_check(c, frames, frame_pitch, sym_stride, depth, len, nframes, ncw)) return r;
    if (dec)
        if (int r = check_decode_out(c, ncw, *dec)) return r;
    return il_run(c, frames, frame_pitch, sym_stride, depth, len, ncw, dec, cw, stream);
}

} // namespace

size_t ezrs_interleaved_workspace_bytes(const ezrs_codec *c, unsigned len, size_t depth, size_t nframes) {
    if (!c || len < 1 || len > c->dev.load || depth == 0 || nframes == 0 || depth > SIZE_MAX / nframes)
        return 0;
    return il_ws_bytes(c, len, depth * nframes);
}

int ezrs_encode_interleaved_ws(const ezrs_codec *c, void *frames, size_t frame_pitch, size_t sym_stride,
                               size_t depth, unsigned len, size_t nframes, void *ws, size_t ws_bytes,
                               void *stream) {
    const CallerWs cw{ws, ws_bytes};
    return il_call(c, frames, frame_pitch, sym_stride, depth, len, nframes, nullptr, &cw, stream);
}

int ezrs_encode_interleaved(const ezrs_codec *c, void *frames, size_t frame_pitch, size_t sym_stride,
                            size_t depth, unsigned len, size_t nframes, void *stream) {
    return il_call(c, frames, frame_pitch, sym_stride, depth, len, nframes, nullptr, nullptr, stream);
}

int ezrs_decode_interleaved_ws(const ezrs_codec *c, void *frames, size_t frame_pitch, size_t sym_stride,
                               size_t depth, unsigned len, size_t nframes, const uint32_t *eras,
                               size_t eras_stride, const uint32_t *neras, int32_t *result,
                               uint32_t *positions, size_t pos_stride, void *corr, size_t corr_stride,
                               void *ws, size_t ws_bytes, void *stream) {
    const DecodeOut o{eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride};
    const CallerWs cw{ws, ws_bytes};
    return il_call(c, frames, frame_pitch, sym_stride, depth, len, nframes, &o, &cw, stream);
}

int ezrs_decode_interleaved(const ezrs_codec *c, void *frames, size_t frame_pitch, size_t sym_stride,
                            size_t depth, unsigned len, size_t nframes, const uint32_t *eras,
                            size_t eras_stride, const uint32_t *neras, int32_t *result,
                            uint32_t *positions, size_t pos_stride, void *corr, size_t corr_stride,
                            void *stream) {
    const DecodeOut o{eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride};
    return il_call(c, frames, frame_pitch, sym_stride, depth, len, nframes, &o, nullptr, stream);
}

// ---- plans of the frame-in-place kernels: shared-erasure reconstruction, in-place parity update ----
namespace {

int upload_table(FramePlan *p, const std::vector<uint32_t> &tab, const char *what) {
    DeviceGuard g(p->device);
    const size_t bytes = tab.size() * sizeof(uint32_t);
    hipError_t e;
    if ((e = hipMalloc(&p->d_tab, bytes)) != hipSuccess ||
        (e = hipMemcpy(p->d_tab, tab.data(), bytes, hipMemcpyHostToDevice)) != hipSuccess)
        return hip_fail(e, what);
    return 0;
}

int destroy_plan(FramePlan *p) {
    if (!p) return 0;
    DeviceGuard g(p->device);
    if (p->d_tab) (void)hipFree(p->d_tab);
    delete p;
    return 0;
}

// What ezrs_recon_create and ezrs_update_create share once their arguments are checked.  p: the new
// plan (null: out of memory), destroyed here on failure; kind: its name in the error texts; ncols,
// nlost: the table's survivors and lost positions; table(tab): builds it, false for bad arguments.
int init_plan(FramePlan *p, const ezrs_codec *c, unsigned len, const char *kind, unsigned ncols,
              unsigned nlost, const std::function<bool(std::vector<uint32_t> &)> &table) {
    const CodecSpec &spec = c->math.spec;
    int r = p ? 0 : -ENOMEM;
    if (recon_table_words(spec.mm, spec.nroots, ncols, nlost) * sizeof(uint32_t) > kReconMaxTable) {
        g_last_error = std::string(kind) + " plan: device table above 64 MiB";
        r = -ENOTSUP;
    }
    std::vector<uint32_t> tab;
    try {
        if (!r && !table(tab)) r = -EINVAL;
    } catch (const std::bad_alloc &) {
        r = -ENOMEM;
    }
    if (!r) {
        p->device = c->device;
        p->mm = spec.mm;
        p->nroots = spec.nroots;
        p->len = len;
        r = upload_table(p, tab, ("hipMalloc(" + std::string(kind) + " table)").c_str());
    }
    if (r) destroy_plan(p);
    return r;
}

} // namespace

int ezrs_recon_create(ezrs_recon **out, const ezrs_codec *c, unsigned len, const uint32_t *lost,
                      unsigned nlost) {
    if (!out) return -EINVAL;
    *out = nullptr;
    if (!c) return -EINVAL;
    const CodecMath &m = c->math;
    if (!recon_check(m, len, lost, nlost)) {
        g_last_error = "reconstruction plan: len outside 1..load, or lost positions that are not "
                       "distinct, below len + NROOTS and at most NROOTS";
        return -EINVAL;
    }
    const unsigned NR = m.spec.nroots, nsurv = len + NR - nlost;
    ezrs_recon *p = new (std::nothrow) ezrs_recon;
    std::vector<uint32_t> surv;
    const int r = init_plan(p, c, len, "reconstruction", nsurv, nlost, [&](std::vector<uint32_t> &tab) {
        std::vector<uint16_t> cols;
        if (!recon_build(m, len, lost, nlost, cols, surv)) return false;
        recon_table(m.spec.mm, NR, cols, surv, lost, nlost, tab);
        p->lost.assign(lost, lost + nlost);
        return true;
    });
    if (r) return r;
    p->surv.swap(surv);
    p->nlost = nlost;
    p->nsurv = nsurv;
    *out = p;
    return 0;
}

int ezrs_recon_destroy(ezrs_recon *p) { return destroy_plan(p); }

int ezrs_reconstruct_interleaved(const ezrs_recon *p, void *frames, size_t frame_pitch, size_t sym_stride,
                                 size_t depth, size_t nframes, int32_t *result, void *stream) {
    if (!p) return -EINVAL;
    if (nframes == 0) return 0;
    if (int r = frames_check(frames, frame_pitch, sym_stride, depth, (size_t)p->len + p->nroots, nframes)) return r;
    DeviceGuard g(p->device);
    ReconArgs a{{frames, frame_pitch, sym_stride, depth, 0, 0, 0, 0}, result, p->nsurv, p->nlost, p->mm,
                recon_row_pad(p->nroots), result ? p->nroots : p->nlost};
    const DevTable t = table_view<const uint32_t>(p->d_tab, p->mm, p->nroots, p->nsurv, p->nlost);
    hipError_t e = launch_recon(a, nframes, t, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "reconstruction launch");
    return 0;
}

int ezrs_update_create(ezrs_update **out, const ezrs_codec *c, unsigned len, const uint32_t *changed,
                       unsigned nchanged) {
    if (!out) return -EINVAL;
    *out = nullptr;
    if (!c || !changed) return -EINVAL;
    const CodecMath &m = c->math;
    if (!update_check(m, len, changed, nchanged)) {
        g_last_error = "update plan: len outside 1..load, or changed positions that are not 1..len "
                       "distinct positions below len";
        return -EINVAL;
    }
    const unsigned NR = m.spec.nroots;
    ezrs_update *p = new (std::nothrow) ezrs_update;
    const int r = init_plan(p, c, len, "update", nchanged, NR, [&](std::vector<uint32_t> &tab) {
        std::vector<uint16_t> cols;
        if (!update_build(m, len, changed, nchanged, cols)) return false;
        std::vector<uint32_t> par(NR);
        for (unsigned i = 0; i < NR; ++i) par[i] = len + i;
        p->chg.assign(changed, changed + nchanged);
        recon_table(m.spec.mm, NR, cols, p->chg, par.data(), NR, tab);
        return true;
    });
    if (r) return r;
    p->nchg = nchanged;
    *out = p;
    return 0;
}

int ezrs_update_destroy(ezrs_update *p) { return destroy_plan(p); }

int ezrs_update_interleaved(const ezrs_update *p, void *frames, size_t frame_pitch, size_t sym_stride,
                            size_t depth, size_t nframes, const void *newsyms, size_t new_frame_pitch,
                            size_t new_sym_stride, void *stream) {
    if (!p) return -EINVAL;
    if (nframes == 0) return 0;
    if (int r = frames_check(frames, frame_pitch, sym_stride, depth, (size_t)p->len + p->nroots, nframes)) return r;
    if (int r = frames_check(newsyms, new_frame_pitch, new_sym_stride, depth, p->nchg, nframes)) return r;
    DeviceGuard g(p->device);
    UpdateArgs a{{frames, frame_pitch, sym_stride, depth, 0, 0, 0, 0}, newsyms, new_frame_pitch, new_sym_stride,
                 p->nchg, p->len, p->nroots, p->mm, recon_row_pad(p->nroots)};
    const DevTable t = table_view<const uint32_t>(p->d_tab, p->mm, p->nroots, p->nchg, p->nroots);
    hipError_t e = launch_update(a, nframes, t, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "update launch");
    return 0;
}

// ---- pointer-array forms: one stripe, every shard a buffer of its own -----------------------------
namespace {

// The buffers of one pointer-form call: [lo, hi) byte ranges, the written ones first.
struct PtrRanges {
    std::pair<uintptr_t, uintptr_t> r[kPtrsMax];
    unsigned n = 0, nwritten = 0;
    size_t al = 0;                                  // OR of the addresses
    void add(const void *p, size_t bytes) {
        r[n++] = {(uintptr_t)p, (uintptr_t)p + bytes};
        al |= (size_t)(uintptr_t)p;
    }
    // true if a written buffer overlaps any other buffer
    bool clash() const {
        for (unsigned i = 0; i < nwritten; ++i)
            for (unsigned k = i + 1; k < n; ++k)
                if (r[i].first < r[k].second && r[k].first < r[i].second) return true;
        return false;
    }
};

int ptrs_fail(const char *what) {
    g_last_error = what;
    return -EINVAL;
}

} // namespace

int ezrs_reconstruct_ptrs(const ezrs_recon *p, void *const *shards, size_t shard_len, int32_t *result,
                          void *stream) {
    if (!p || !shards) return -EINVAL;
    if (p->nsurv + p->nlost > kPtrsMax) {
        g_last_error = "reconstruct_ptrs: len + NROOTS above EZRS_PTRS_MAX pointers";
        return -ENOTSUP;
    }
    if (shard_len == 0) return 0;
    const size_t w = p->mm <= 8 ? 1 : 2;
    if (shard_len > SIZE_MAX / w) return -EINVAL;
    ReconPtrArgs a{{{nullptr, 0, 0, shard_len, 0, 0, 0, 0}, result, p->nsurv, p->nlost, p->mm,
                    recon_row_pad(p->nroots), result ? p->nroots : p->nlost}, {}};
    PtrRanges rg;
    for (unsigned r = 0; r < p->nlost; ++r)         // the written buffers first
        if ((a.tab.p[p->nsurv + r] = shards[p->lost[r]])) rg.add(shards[p->lost[r]], shard_len * w);
    rg.nwritten = rg.n;
    for (unsigned c = 0; c < p->nsurv; ++c) {
        if (!(a.tab.p[c] = shards[p->surv[c]])) return ptrs_fail("reconstruct_ptrs: a surviving shard is NULL");
        rg.add(shards[p->surv[c]], shard_len * w);
    }
    if (rg.clash()) return ptrs_fail("reconstruct_ptrs: a rebuilt shard's buffer overlaps another buffer");
    DeviceGuard g(p->device);
    const DevTable t = table_view<const uint32_t>(p->d_tab, p->mm, p->nroots, p->nsurv, p->nlost);
    hipError_t e = launch_recon(a, rg.al, t, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "reconstruction launch");
    return 0;
}

int ezrs_update_ptrs(const ezrs_update *p, void *const *shards, const void *const *newsyms, size_t shard_len,
                     void *stream) {
    if (!p || !shards || !newsyms) return -EINVAL;
    if ((size_t)2 * p->nchg + p->nroots > kPtrsMax) {
        g_last_error = "update_ptrs: 2*nchanged + NROOTS above EZRS_PTRS_MAX pointers";
        return -ENOTSUP;
    }
    if (shard_len == 0) return 0;
    const size_t w = p->mm <= 8 ? 1 : 2;
    if (shard_len > SIZE_MAX / w) return -EINVAL;
    UpdatePtrArgs a{{{nullptr, 0, 0, shard_len, 0, 0, 0, 0}, nullptr, 0, 0, p->nchg, p->len, p->nroots, p->mm,
                     recon_row_pad(p->nroots)}, {}};
    PtrRanges rg;
    for (unsigned c = 0; c < p->nchg; ++c) {        // written: the changed shards and the parity
        if (!(a.tab.p[c] = shards[p->chg[c]])) return ptrs_fail("update_ptrs: a changed shard is NULL");
        rg.add(shards[p->chg[c]], shard_len * w);
    }
    for (unsigned i = 0; i < p->nroots; ++i) {
        if (!(a.tab.p[p->nchg + i] = shards[p->len + i])) return ptrs_fail("update_ptrs: a parity shard is NULL");
        rg.add(shards[p->len + i], shard_len * w);
    }
    rg.nwritten = rg.n;
    for (unsigned c = 0; c < p->nchg; ++c) {
        if (!newsyms[c]) return ptrs_fail("update_ptrs: a newsyms buffer is NULL");
        a.tab.p[p->nchg + p->nroots + c] = const_cast<void *>(newsyms[c]);
        rg.add(newsyms[c], shard_len * w);
    }
    if (rg.clash()) return ptrs_fail("update_ptrs: a changed or parity shard's buffer overlaps another buffer");
    DeviceGuard g(p->device);
    const DevTable t = table_view<const uint32_t>(p->d_tab, p->mm, p->nroots, p->nchg, p->nroots);
    hipError_t e = launch_update(a, rg.al, t, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "update launch");
    return 0;
}

// ---- batched pointer forms: many stripes, the pointers in a table on the device --------------------
namespace {

// What the host can check of a batch call: the table is on the device.  w: bytes of the datum;
// 0: go on, 1: nothing to do, else the error.
int batch_check(const char *call, size_t pitch, size_t need, size_t shard_len, size_t nstripes,
                unsigned align, size_t w) {
    const char *bad = nullptr;
    if (pitch < need) bad = "table_pitch below len + NROOTS";
    else if (align != 16 && align != 4 && align != w) bad = "align is not 16, 4 or the datum size";
    else if (shard_len > SIZE_MAX / w) bad = "shard_len * datum bytes overflows size_t";
    else if (shard_len && nstripes > SIZE_MAX / shard_len) bad = "nstripes * shard_len overflows size_t";
    if (bad) {
        g_last_error = std::string(call) + ": " + bad;
        return -EINVAL;
    }
    return nstripes && shard_len ? 0 : 1;
}

} // namespace

int ezrs_reconstruct_ptrs_batch(const ezrs_recon *p, void *const *table, size_t table_pitch, size_t shard_len,
                                size_t nstripes, unsigned align, int32_t *result, void *stream) {
    if (!p || !table) return -EINVAL;
    const size_t w = p->mm <= 8 ? 1 : 2;
    if (int r = batch_check("reconstruct_ptrs_batch", table_pitch, (size_t)p->len + p->nroots, shard_len,
                            nstripes, align, w))
        return r < 0 ? r : 0;
    ReconBatchArgs a{{{nullptr, 0, 0, shard_len, 0, 0, 0, 0}, result, p->nsurv, p->nlost, p->mm,
                      recon_row_pad(p->nroots), result ? p->nroots : p->nlost}, table, table_pitch, 0};
    DeviceGuard g(p->device);
    const DevTable t = table_view<const uint32_t>(p->d_tab, p->mm, p->nroots, p->nsurv, p->nlost);
    hipError_t e = launch_recon(a, nstripes, align, t, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "reconstruction launch");
    return 0;
}

int ezrs_update_ptrs_batch(const ezrs_update *p, void *const *table, size_t table_pitch,
                           const void *const *new_table, size_t new_pitch, size_t shard_len, size_t nstripes,
                           unsigned align, void *stream) {
    if (!p || !table || !new_table) return -EINVAL;
    const size_t w = p->mm <= 8 ? 1 : 2;
    if (new_pitch < p->nchg) {
        g_last_error = "update_ptrs_batch: new_pitch below nchanged";
        return -EINVAL;
    }
    if (int r = batch_check("update_ptrs_batch", table_pitch, (size_t)p->len + p->nroots, shard_len,
                            nstripes, align, w))
        return r < 0 ? r : 0;
    UpdateBatchArgs a{{{nullptr, 0, 0, shard_len, 0, 0, 0, 0}, nullptr, 0, 0, p->nchg, p->len, p->nroots, p->mm,
                       recon_row_pad(p->nroots)}, table, new_table, table_pitch, new_pitch, 0};
    DeviceGuard g(p->device);
    const DevTable t = table_view<const uint32_t>(p->d_tab, p->mm, p->nroots, p->nchg, p->nroots);
    hipError_t e = launch_update(a, nstripes, align, t, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "update launch");
    return 0;
}

// ---- mixed batched forms: many stripes, a plan per stripe (create_set, destroy_set: above) ----------
int ezrs_recon_set_create(ezrs_recon_set **out, const ezrs_recon *const *plans, unsigned nplans) {
    return create_set(out, plans, nplans, "reconstruction set", [](const ezrs_recon &p) {
        return std::make_pair(p.nsurv, p.nlost);
    }, true);
}

int ezrs_recon_set_destroy(ezrs_recon_set *s) { return destroy_set(s); }

int ezrs_reconstruct_ptrs_mixed(const ezrs_recon_set *s, const uint32_t *plan_of, void *const *table,
                                size_t table_pitch, size_t shard_len, size_t nstripes, unsigned align,
                                int32_t *result, void *stream) {
    if (!s || !plan_of || !table) return -EINVAL;
    const size_t w = s->mm <= 8 ? 1 : 2;
    if (int r = batch_check("reconstruct_ptrs_mixed", table_pitch, (size_t)s->len + s->nroots, shard_len,
                            nstripes, align, w))
        return r < 0 ? r : 0;
    // nsurv, nlost: per stripe, from the directory
    ReconMixedArgs a{{{{nullptr, 0, 0, shard_len, 0, 0, 0, 0}, result, 0, 0, s->mm, recon_row_pad(s->nroots),
                       result ? s->nroots : s->most}, table, table_pitch, 0}, plan_of, s->d_set, s->nplans};
    DeviceGuard g(s->device);
    hipError_t e = launch_recon(a, nstripes, align, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "reconstruction launch");
    return 0;
}

// An update plan's table is the image of a reconstruction with survivors = changed and lost = the
// parity positions.
int ezrs_update_set_create(ezrs_update_set **out, const ezrs_update *const *plans, unsigned nplans) {
    return create_set(out, plans, nplans, "update set", [](const ezrs_update &p) {
        return std::make_pair(p.nchg, p.nroots);
    }, false);
}

int ezrs_update_set_destroy(ezrs_update_set *s) { return destroy_set(s); }

int ezrs_update_ptrs_mixed(const ezrs_update_set *s, const uint32_t *plan_of, void *const *table,
                           size_t table_pitch, const void *const *new_table, size_t new_pitch,
                           size_t shard_len, size_t nstripes, unsigned align, void *stream) {
    if (!s || !plan_of || !table || !new_table) return -EINVAL;
    const size_t w = s->mm <= 8 ? 1 : 2;
    if (new_pitch < s->most) {
        g_last_error = "update_ptrs_mixed: new_pitch below the largest nchanged of the set";
        return -EINVAL;
    }
    if (int r = batch_check("update_ptrs_mixed", table_pitch, (size_t)s->len + s->nroots, shard_len,
                            nstripes, align, w))
        return r < 0 ? r : 0;
    // nchg: per stripe, from the directory; here the set's largest
    UpdateMixedArgs a{{{{nullptr, 0, 0, shard_len, 0, 0, 0, 0}, nullptr, 0, 0, s->most, s->len, s->nroots, s->mm,
                        recon_row_pad(s->nroots)}, table, new_table, table_pitch, new_pitch, 0},
                      plan_of, s->d_set, s->nplans};
    DeviceGuard g(s->device);
    hipError_t e = launch_update(a, nstripes, align, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "update launch");
    return 0;
}

// ---- pointer forms of the staged decode: errors and erasures in stripes of separate buffers --------
namespace {

// ezrs_decode_ptrs(_ws): one stripe, the pointers by value; cw == null uses the stream's workspace.
int decode_ptrs(const ezrs_codec *c, void *const *shards, unsigned len, size_t shard_len, const DecodeOut &o,
                const CallerWs *cw, void *stream) {
    if (!c || !shards || !o.result) return -EINVAL;
    if (len < 1 || len > c->dev.load) return -EINVAL;
    const size_t w = sym_bytes(c->dev), P = (size_t)len + c->dev.nroots;
    if (P > kPtrsMax) {
        g_last_error = "decode_ptrs: len + NROOTS above EZRS_PTRS_MAX pointers";
        return -ENOTSUP;
    }
    if (shard_len == 0) return 0;
    if (shard_len > SIZE_MAX / w) return -EINVAL;
    PtrTable tab{};
    PtrRanges rg;
    for (size_t p = 0; p < P; ++p) {                // every buffer is read and may be written
        if (!(tab.p[p] = shards[p])) return ptrs_fail("decode_ptrs: a shard is NULL");
        rg.add(shards[p], shard_len * w);
    }
    rg.nwritten = rg.n;
    if (rg.clash()) return ptrs_fail("decode_ptrs: two shards' buffers overlap");
    if (int r = check_decode_out(c, shard_len, o)) return r;
    const IlPtrs pt{nullptr, P, rg.al, &tab};
    return il_run(c, nullptr, 0, 0, shard_len, len, shard_len, &o, cw, stream, &pt);
}

// ezrs_decode_ptrs_batch(_ws): the table on the device.
int decode_ptrs_batch(const ezrs_codec *c, void *const *table, size_t table_pitch, unsigned len,
                      size_t shard_len, size_t nstripes, unsigned align, const DecodeOut &o,
                      const CallerWs *cw, void *stream) {
    if (!c || !table || !o.result) return -EINVAL;
    if (len < 1 || len > c->dev.load) return -EINVAL;
    if (int r = batch_check("decode_ptrs_batch", table_pitch, (size_t)len + c->dev.nroots, shard_len, nstripes,
                            align, sym_bytes(c->dev)))
        return r < 0 ? r : 0;
    const size_t ncw = nstripes * shard_len;
    if (int r = check_decode_out(c, ncw, o)) return r;
    const IlPtrs pt{table, table_pitch, align, nullptr};
    return il_run(c, nullptr, 0, 0, shard_len, len, ncw, &o, cw, stream, &pt);
}

} // namespace

size_t ezrs_decode_ptrs_workspace_bytes(const ezrs_codec *c, unsigned len, size_t shard_len, size_t nstripes) {
    if (!c || len < 1 || len > c->dev.load || shard_len == 0 || nstripes == 0 || shard_len > SIZE_MAX / nstripes)
        return 0;
    return il_ptrs_head((size_t)len + c->dev.nroots) + il_ws_bytes(c, len, shard_len * nstripes);
}

int ezrs_decode_ptrs(const ezrs_codec *c, void *const *shards, unsigned len, size_t shard_len,
                     const uint32_t *eras, size_t eras_stride, const uint32_t *neras, int32_t *result,
                     uint32_t *positions, size_t pos_stride, void *corr, size_t corr_stride, void *stream) {
    return decode_ptrs(c, shards, len, shard_len,
                       {eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride}, nullptr, stream);
}

int ezrs_decode_ptrs_ws(const ezrs_codec *c, void *const *shards, unsigned len, size_t shard_len,
                        const uint32_t *eras, size_t eras_stride, const uint32_t *neras, int32_t *result,
                        uint32_t *positions, size_t pos_stride, void *corr, size_t corr_stride, void *ws,
                        size_t ws_bytes, void *stream) {
    const CallerWs cw{ws, ws_bytes};
    return decode_ptrs(c, shards, len, shard_len,
                       {eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride}, &cw, stream);
}

int ezrs_decode_ptrs_batch(const ezrs_codec *c, void *const *table, size_t table_pitch, unsigned len,
                           size_t shard_len, size_t nstripes, unsigned align, const uint32_t *eras,
                           size_t eras_stride, const uint32_t *neras, int32_t *result, uint32_t *positions,
                           size_t pos_stride, void *corr, size_t corr_stride, void *stream) {
    return decode_ptrs_batch(c, table, table_pitch, len, shard_len, nstripes, align,
                             {eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride}, nullptr,
                             stream);
}

int ezrs_decode_ptrs_batch_ws(const ezrs_codec *c, void *const *table, size_t table_pitch, unsigned len,
                              size_t shard_len, size_t nstripes, unsigned align, const uint32_t *eras,
                              size_t eras_stride, const uint32_t *neras, int32_t *result, uint32_t *positions,
                              size_t pos_stride, void *corr, size_t corr_stride, void *ws, size_t ws_bytes,
                              void *stream) {
    const CallerWs cw{ws, ws_bytes};
    return decode_ptrs_batch(c, table, table_pitch, len, shard_len, nstripes, align,
                             {eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride}, &cw,
                             stream);
}

// ---- selection: the failed codewords of a verify, and a decode of only those -----------------------
namespace {

// ezrs_select_failed(_ws): cw == null uses the stream's workspace.
int select_failed(const ezrs_codec *c, const int32_t *result, size_t n, uint64_t base, uint64_t *sel, size_t cap,
                  uint64_t *count, const CallerWs *cw, void *stream) {
    if (!c || !sel || !count || (n && !result)) return -EINVAL;
    if (n && base > UINT64_MAX - n) return -EINVAL;
    DeviceGuard g(c->device);
    void *ws = nullptr;
    if (int r = take_ws(c, cw, select_ws_bytes(n), stream, &ws)) return r;
    hipError_t e = launch_select_failed(result, n, base, sel, cap, count, ws, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(e, "selection launch");
}

// ezrs_decode_ptrs_select(_ws): rows of `sel` over the table of ezrs_decode_ptrs_batch.
int decode_ptrs_select(const ezrs_codec *c, void *const *table, size_t table_pitch, unsigned len,
                       size_t shard_len, size_t nstripes, const uint64_t *sel, size_t nsel, const uint64_t *count,
                       const DecodeOut &o, const CallerWs *cw, void *stream) {
    if (!c) return -EINVAL;
    if (nsel == 0) return 0;
    if (!table || !sel || !o.result) return -EINVAL;
    if (len < 1 || len > c->dev.load) return -EINVAL;
    const unsigned w = sym_bytes(c->dev);
    if (int r = batch_check("decode_ptrs_select", table_pitch, (size_t)len + c->dev.nroots, shard_len, nstripes, w, w))
        return r < 0 ? r : 0;
    if (int r = check_decode_out(c, nsel, o)) return r;
    const IlPtrs pt{table, table_pitch, w, nullptr};
    const IlSelect sl{sel, count, nstripes * shard_len};
    return il_run(c, nullptr, 0, 0, shard_len, len, nsel, &o, cw, stream, &pt, &sl);
}

// ezrs_decode_interleaved_select(_ws): rows of `sel` over the frames of ezrs_decode_interleaved.
int decode_il_select(const ezrs_codec *c, void *frames, size_t frame_pitch, size_t sym_stride, size_t depth,
                     unsigned len, size_t nframes, const uint64_t *sel, size_t nsel, const uint64_t *count,
                     const DecodeOut &o, const CallerWs *cw, void *stream) {
    if (!c) return -EINVAL;
    if (nsel == 0 || nframes == 0) return 0;
    size_t ncw;
    if (int r = il_check(c, frames, frame_pitch, sym_stride, depth, len, nframes, ncw)) return r;
    if (!sel) return -EINVAL;
    if (int r = check_decode_out(c, nsel, o)) return r;
    const IlSelect sl{sel, count, ncw};
    return il_run(c, frames, frame_pitch, sym_stride, depth, len, nsel, &o, cw, stream, nullptr, &sl);
}

} // namespace

size_t ezrs_select_workspace_bytes(size_t n) { return select_ws_bytes(n); }

int ezrs_select_failed(const ezrs_codec *c, const int32_t *result, size_t n, uint64_t base, uint64_t *sel,
                       size_t cap, uint64_t *count, void *stream) {
    return select_failed(c, result, n, base, sel, cap, count, nullptr, stream);
}

int ezrs_select_failed_ws(const ezrs_codec *c, const int32_t *result, size_t n, uint64_t base, uint64_t *sel,
                          size_t cap, uint64_t *count, void *ws, size_t ws_bytes, void *stream) {
    const CallerWs cw{ws, ws_bytes};
    return select_failed(c, result, n, base, sel, cap, count, &cw, stream);
}

size_t ezrs_decode_select_workspace_bytes(const ezrs_codec *c, unsigned len, size_t nsel) {
    if (!c || len < 1 || len > c->dev.load || nsel == 0) return 0;
    return il_ws_bytes(c, len, nsel);
}

int ezrs_decode_ptrs_select(const ezrs_codec *c, void *const *table, size_t table_pitch, unsigned len,
                            size_t shard_len, size_t nstripes, const uint64_t *sel, size_t nsel,
                            const uint64_t *count, const uint32_t *eras, size_t eras_stride, const uint32_t *neras,
                            int32_t *result, uint32_t *positions, size_t pos_stride, void *corr,
                            size_t corr_stride, void *stream) {
    return decode_ptrs_select(c, table, table_pitch, len, shard_len, nstripes, sel, nsel, count,
                              {eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride}, nullptr,
                              stream);
}

int ezrs_decode_ptrs_select_ws(const ezrs_codec *c, void *const *table, size_t table_pitch, unsigned len,
                               size_t shard_len, size_t nstripes, const uint64_t *sel, size_t nsel,
                               const uint64_t *count, const uint32_t *eras, size_t eras_stride,
                               const uint32_t *neras, int32_t *result, uint32_t *positions, size_t pos_stride,
                               void *corr, size_t corr_stride, void *ws, size_t ws_bytes, void *stream) {
    const CallerWs cw{ws, ws_bytes};
    return decode_ptrs_select(c, table, table_pitch, len, shard_len, nstripes, sel, nsel, count,
                              {eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride}, &cw,
                              stream);
}

int ezrs_decode_interleaved_select(const ezrs_codec *c, void *frames, size_t frame_pitch, size_t sym_stride,
                                   size_t depth, unsigned len, size_t nframes, const uint64_t *sel, size_t nsel,
                                   const uint64_t *count, const uint32_t *eras, size_t eras_stride,
                                   const uint32_t *neras, int32_t *result, uint32_t *positions, size_t pos_stride,
                                   void *corr, size_t corr_stride, void *stream) {
    return decode_il_select(c, frames, frame_pitch, sym_stride, depth, len, nframes, sel, nsel, count,
                            {eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride}, nullptr,
                            stream);
}

int ezrs_decode_interleaved_select_ws(const ezrs_codec *c, void *frames, size_t frame_pitch, size_t sym_stride,
                                      size_t depth, unsigned len, size_t nframes, const uint64_t *sel,
                                      size_t nsel, const uint64_t *count, const uint32_t *eras,
                                      size_t eras_stride, const uint32_t *neras, int32_t *result,
                                      uint32_t *positions, size_t pos_stride, void *corr, size_t corr_stride,
                                      void *ws, size_t ws_bytes, void *stream) {
    const CallerWs cw{ws, ws_bytes};
    return decode_il_select(c, frames, frame_pitch, sym_stride, depth, len, nframes, sel, nsel, count,
                            {eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride}, &cw,
                            stream);
}

int ezrs_update_bitmatrix(unsigned symbol_bits, unsigned poly, unsigned fcr, unsigned prim, unsigned nroots,
                          int dual, unsigned len, const uint32_t *changed, unsigned nchanged, uint16_t *cols,
                          size_t cols_cap) {
    if (!cols || !changed) return -EINVAL;
    CodecMath m;
    if (!m.build(CodecSpec{symbol_bits, poly, fcr, prim, nroots, dual ? 1 : 0})) return -EINVAL;
    if (!update_check(m, len, changed, nchanged)) return -EINVAL;
    if (cols_cap < (size_t)nroots * nchanged * symbol_bits) return -EINVAL;
    try {
        std::vector<uint16_t> c;
        if (!update_build(m, len, changed, nchanged, c)) return -EINVAL;
        std::copy(c.begin(), c.end(), cols);
    } catch (const std::bad_alloc &) {
        return -ENOMEM;
    }
    return 0;
}

// ---- host-memory pipeline ---------------------------------------------------------------------
namespace {

// Rows whose decode result is nonzero, compacted straight into pinned host memory (the kernel's
// stores cross PCIe; nothing to copy back afterwards): *cnt (device) counts them, hix[j] = chunk-
// relative row index of compacted row j (in no particular order), hout + j * pitch = its bytes,
// pitch = row_bytes rounded up to 16.  *cnt must be zero on entry.
__global__ void __launch_bounds__(256) k_compact_rows(const int32_t *result, size_t n, const char *rows,
                                                      size_t row_bytes, uint32_t *cnt, uint32_t *hix,
                                                      char *hout, size_t pitch) {
    __shared__ uint32_t slot[256];
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool mine = k < n && result[k] != 0;
    slot[threadIdx.x] = mine ? atomicAdd(cnt, 1u) : 0xFFFFFFFFu;
    if (mine) hix[slot[threadIdx.x]] = (uint32_t)k;
    __syncthreads();
    // the block copies its flagged rows, one row per wavefront at a time, 16 bytes per lane (byte
    // loads: rows of any length and alignment; one 16-byte store into the padded host row)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < 256; t += 4) {
        const uint32_t sl = slot[t];
        if (sl == 0xFFFFFFFFu) continue;
        const unsigned char *src = reinterpret_cast<const unsigned char *>(rows) + ((size_t)blockIdx.x * 256 + t) * row_bytes;
        char *dst = hout + (size_t)sl * pitch;
        for (size_t b = 16 * (size_t)lane; b < row_bytes; b += 16 * 64) {
            uint32_t v[4] = {0, 0, 0, 0};
            if (b + 16 <= row_bytes) {
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q >> 2] |= (uint32_t)src[b + q] << (8 * (q & 3));
            } else {
                for (size_t q = 0; b + q < row_bytes; ++q) v[q >> 2] |= (uint32_t)src[b + q] << (8 * (q & 3));
            }
            *reinterpret_cast<uint4 *>(dst + b) = make_uint4(v[0], v[1], v[2], v[3]);
        }
    }
}

hipError_t launch_compact_rows(const int32_t *result, size_t n, const char *rows, size_t row_bytes,
                               uint32_t *cnt, uint32_t *hix, char *hout, size_t pitch, hipStream_t st) {
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_compact_rows, dim3(grid), dim3(256), 0, st, result, n, rows, row_bytes, cnt, hix,
                       hout, pitch);
    return hipGetLastError();
}

// Device and pinned-host staging of the host-memory forms: two sets (one per pipeline stream).
int ensure_stage(ezrs_codec *c, size_t dbytes, size_t hbytes) {
    if (!c->streams[0])
        for (int i = 0; i < 2; ++i)
            HIP_TRY(hipStreamCreateWithFlags(&c->streams[i], hipStreamNonBlocking));
    HIP_TRY(c->d_stage.ensure(dbytes));
    HIP_TRY(c->h_stage.ensure(hbytes));
    return 0;
}

// Host threads for the CPU-side scatters of the host-memory forms (EZRS_HOST_THREADS, default 8).
size_t host_threads() {
    static const size_t n = [] {
        const char *e = getenv("EZRS_HOST_THREADS");
        const long v = e ? atol(e) : 8;
        return (size_t)(v < 1 ? 1 : v > 64 ? 64 : v);
    }();
    return n;
}

// Pinned (page-locked) host memory?  Pageable copies go through the runtime's own staging, which
// pipelines badly on single large copies: they get smaller chunks.
bool host_pinned(const void *p) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

size_t default_chunk(size_t row_bytes, bool pinned = true) {
    // staged rows per chunk: 64 MiB from pinned memory, 32 MiB from pageable (measured, 1 M
    // RS(255,223) rows: pageable decode 17.5 ms at 64 MiB, 6.6 ms at 32 MiB; pinned 5.4 / 6.9)
    const size_t target = (size_t)(pinned ? 64 : 32) << 20;
    size_t n = target / (row_bytes ? row_bytes : 1);
    return n ? n : 1;
}

// Encode of host rows.  PCIe traffic: the rows' data symbols go to the device (one linear copy
// of the rows' span when the row pitch is at most twice what a row needs, otherwise a CPU gather
// into pinned staging first), the kernel writes the parity as one compact [n][NR] block, and only
// that block comes back (a linear copy; a CPU scatter puts each row's NR symbols in place unless
// the caller's parity array is itself compact).  The caller's data symbols are never written.
//   rows != NULL: the rs_base:778-790 row form, parity at rows + len (data is rows)
int encode_host_core(ezrs_codec *c, const char *data, size_t data_stride, unsigned len,
                     char *parity, size_t parity_stride, size_t ncw, size_t chunk) {
    const size_t w = sym_bytes(c->dev), NR = c->dev.nroots;
    const size_t need = (size_t)len;                              // symbols a row must carry over
    const bool span = ncw == 1 || data_stride <= 2 * need + NR;    // linear copy of the rows' span
    // device row pitch (symbols); a single row is staged at pitch len whatever its stride (a stride
    // below len, 0 included, is legal for one codeword and must not size the staging)
    const size_t drow = ncw == 1 ? need : span ? data_stride : need;
    const bool par_direct = parity_stride == NR || ncw == 1;       // caller's parity is compact
    if (!chunk) chunk = default_chunk(drow * w, host_pinned(data));
    if (chunk > ncw) chunk = ncw;
    const size_t b_in = align_up(chunk * drow * w), b_par = align_up(chunk * NR * w),
                 b_ws = align_up(ws_bytes_for(c, chunk));
    const size_t h_in = span ? 0 : align_up(chunk * need * w), h_par = par_direct ? 0 : b_par;
    if (int r = ensure_stage(c, b_in + b_par + b_ws, h_in + h_par + 256)) return r;
    struct Pending { size_t k0 = 0, n = 0; bool live = false; } pend[2];
    // scatter of a chunk's compact parity into the caller's rows: split over host threads (a
    // single thread writing 32-byte pieces into 1 M rows takes ~5 ms, 2x the copy itself)
    auto scatter = [&](int s) {
        if (!pend[s].live || par_direct) return;
        const char *src = static_cast<const char *>(c->h_stage.p[s]) + h_in;
        const size_t n = pend[s].n, k0 = pend[s].k0;
        auto part = [&](size_t r0, size_t r1) {
            for (size_t r = r0; r < r1; ++r)
                std::memcpy(parity + (k0 + r) * parity_stride * w, src + r * NR * w, NR * w);
        };
        const size_t nt = n >= 65536 ? host_threads() : 1;
        if (nt <= 1) {
            part(0, n);
            return;
        }
        std::vector<std::thread> th;
        for (size_t t = 1; t < nt; ++t) th.emplace_back(part, n * t / nt, n * (t + 1) / nt);
        part(0, n / nt);
        for (auto &x : th) x.join();
    };
    for (size_t i = 0, k0 = 0; k0 < ncw; ++i, k0 += chunk) {
        const int s = (int)(i & 1);
        hipStream_t st = c->streams[s];
        const size_t n = ncw - k0 < chunk ? ncw - k0 : chunk;
        if (pend[s].live) {
            HIP_TRY(hipStreamSynchronize(st));
            scatter(s);
            pend[s].live = false;
        }
        char *d_in = static_cast<char *>(c->d_stage.p[s]), *d_par = d_in + b_in, *d_ws = d_par + b_par;
        char *hs = static_cast<char *>(c->h_stage.p[s]);
        const char *hd = data + k0 * data_stride * w;
        if (span) {
            HIP_TRY(hipMemcpyAsync(d_in, hd, ((n - 1) * data_stride + need) * w,
                                   hipMemcpyHostToDevice, st));
        } else {
            for (size_t r = 0; r < n; ++r) std::memcpy(hs + r * need * w, hd + r * data_stride * w, need * w);
            HIP_TRY(hipMemcpyAsync(d_in, hs, n * need * w, hipMemcpyHostToDevice, st));
        }
        EncodeArgs a{d_in, drow, len, d_par, NR, n};
        HIP_TRY(dispatch_encode(c, a, d_ws, st));
        if (par_direct)
            HIP_TRY(hipMemcpyAsync(parity + k0 * NR * w, d_par, n * NR * w, hipMemcpyDeviceToHost, st));
        else
            HIP_TRY(hipMemcpyAsync(hs + h_in, d_par, n * NR * w, hipMemcpyDeviceToHost, st));
        pend[s] = {k0, n, true};
    }
    for (int s = 0; s < 2; ++s) {
        HIP_TRY(hipStreamSynchronize(c->streams[s]));
        scatter(s);
    }
    return 0;
}

} // namespace

int ezrs_encode_host(ezrs_codec *c, const void *data, size_t data_stride, unsigned len,
                     void *parity, size_t parity_stride, size_t ncw, size_t chunk) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (int r = check_rows(c, data, data_stride, len, parity, parity_stride, ncw, false)) {
        if (!parity)
            g_last_error = "ezrs_encode_host: parity is required (rows that carry their own parity: "
                           "ezrs_encode_rows_host)";
        return r;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    return encode_host_core(c, static_cast<const char *>(data), data_stride, len,
                            static_cast<char *>(parity), parity_stride, ncw, chunk);
}

int ezrs_encode_rows_host(ezrs_codec *c, void *rows, size_t stride, unsigned len, size_t ncw,
                          size_t chunk) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    void *parity = nullptr;
    size_t parity_stride = 0;
    if (int r = check_rows(c, rows, stride, len, parity, parity_stride, ncw, true)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    return encode_host_core(c, static_cast<const char *>(rows), stride, len, static_cast<char *>(parity),
                            parity_stride, ncw, chunk);
}

int ezrs_decode_host(ezrs_codec *c, void *data, size_t data_stride, unsigned len, void *parity,
                     size_t parity_stride, const uint32_t *eras, size_t eras_stride,
                     const uint32_t *neras, int32_t *result, uint32_t *positions,
                     size_t pos_stride, void *corr, size_t corr_stride, size_t ncw, size_t chunk) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (int r = check_rows(c, data, data_stride, len, parity, parity_stride, ncw, true)) return r;
    if (int r = check_decode_out(c, ncw, {eras, eras_stride, neras, result, positions, pos_stride, corr,
                                          corr_stride}))
        return r;
    const unsigned w = sym_bytes(c->dev), NR = c->dev.nroots;
    // erasure columns to stage: the row stride (capped at NR); a single codeword may pass
    // eras_stride 0, and then carries neras[0] entries
    size_t ecols = eras ? (eras_stride < NR ? eras_stride : NR) : 0;
    if (eras && ncw == 1 && eras_stride == 0) ecols = neras ? (neras[0] < NR ? neras[0] : NR) : 0;
    if (eras && ecols == 0) eras = nullptr, neras = nullptr;
    const DecodeOut out{eras, eras_stride, neras, result, positions, pos_stride, corr, corr_stride};
    const bool inline_par = parity_stride == data_stride && data_stride >= (size_t)len + NR &&
                            static_cast<const char *>(parity) ==
                                static_cast<const char *>(data) + (size_t)len * w;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    // device row: the caller's whole row when parity is inline (one linear copy in)
    const size_t row = inline_par ? data_stride * w : (size_t)(len + NR) * w;
    if (!chunk) chunk = default_chunk(row, host_pinned(data));
    if (chunk > ncw) chunk = ncw;
    const size_t b_cw = align_up(chunk * row), b_er = align_up(chunk * ecols * 4),
                 b_ne = align_up(neras ? chunk * 4 : 0), b_rs = align_up(chunk * 4),
                 b_ps = align_up(positions ? chunk * NR * 4 : 0),
                 b_co = align_up(corr ? chunk * NR * w : 0),
                 b_sy = align_up(ws_bytes_for(c, chunk)), b_ct = 256;
    // pinned host staging: the compacted rows (16-byte pitch), their indices, the count
    const size_t pitch = (row + 15) & ~(size_t)15;
    const size_t h_cp = align_up(chunk * pitch), h_ix = align_up(chunk * 4), h_ct = 256;
    if (int r = ensure_stage(c, b_cw + b_er + b_ne + b_rs + b_ps + b_co + b_sy + b_ct, h_cp + h_ix + h_ct)) return r;
    // Only the codewords whose result is nonzero can differ from what was sent (a clean codeword is
    // never written; -1 may leave partial corrections, rs_base:1238-1241): the device compacts those
    // rows straight into pinned host memory, and only the results and the count are copied back, so
    // a chunk needs one synchronisation before its rows are scattered.
    struct Pending { size_t k0 = 0; bool live = false; } pend[2];
    auto finish = [&](int s) -> int {
        if (!pend[s].live) return 0;
        pend[s].live = false;
        HIP_TRY(hipStreamSynchronize(c->streams[s]));           // rows, indices, results, count
        const char *hb = static_cast<const char *>(c->h_stage.p[s]);
        const uint32_t *hix = reinterpret_cast<const uint32_t *>(hb + h_cp);
        const uint32_t cnt = *reinterpret_cast<const uint32_t *>(hb + h_cp + h_ix);
        const size_t k0 = pend[s].k0;
        for (uint32_t j = 0; j < cnt; ++j) {
            const size_t k = k0 + hix[j];
            const char *src = hb + (size_t)j * pitch;
            if (inline_par) {
                std::memcpy(static_cast<char *>(data) + k * data_stride * w, src, (size_t)(len + NR) * w);
            } else {
                std::memcpy(static_cast<char *>(data) + k * data_stride * w, src, (size_t)len * w);
                std::memcpy(static_cast<char *>(parity) + k * parity_stride * w, src + (size_t)len * w,
                            (size_t)NR * w);
            }
        }
        return 0;
    };
    for (size_t i = 0, k0 = 0; k0 < ncw; ++i, k0 += chunk) {
        const int s = (int)(i & 1);
        hipStream_t st = c->streams[s];
        const size_t n = ncw - k0 < chunk ? ncw - k0 : chunk;
        if (int r = finish(s)) return r;                        // chunk i-2 (this stream's buffers)
        char *base = static_cast<char *>(c->d_stage.p[s]);
        char *dcw = base, *der = dcw + b_cw, *dne = der + b_er, *drs = dne + b_ne, *dps = drs + b_rs,
             *dco = dps + b_ps, *dsy = dco + b_co, *dct = dsy + b_sy;
        char *hb = static_cast<char *>(c->h_stage.p[s]), *dhb = nullptr;
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&dhb), hb, 0));
        // the chunk as the caller holds it (h) and as it is staged on the device (d)
        const size_t ds = row / w;
        const DecodeArgs h = out.args(c, static_cast<char *>(data) + k0 * data_stride * w, data_stride, len,
                                      static_cast<char *>(parity) + k0 * parity_stride * w, parity_stride,
                                      k0, n);
        const DecodeOut staged{eras ? reinterpret_cast<uint32_t *>(der) : nullptr, ecols,
                               neras ? reinterpret_cast<uint32_t *>(dne) : nullptr,
                               reinterpret_cast<int32_t *>(drs),
                               positions ? reinterpret_cast<uint32_t *>(dps) : nullptr, NR,
                               corr ? dco : nullptr, NR};
        const DecodeArgs d = staged.args(c, dcw, ds, len, dcw + (size_t)len * w, ds, 0, n);
        const size_t span = ((n - 1) * data_stride + len + NR) * w;
        if (inline_par) {
            HIP_TRY(hipMemcpyAsync(dcw, h.data, span, hipMemcpyHostToDevice, st));
        } else {
            HIP_TRY(ezrs::copy2d(dcw, row, h.data, data_stride * w, (size_t)len * w, n,
                                 hipMemcpyHostToDevice, st));
            HIP_TRY(ezrs::copy2d(d.parity, row, h.parity, parity_stride * w, (size_t)NR * w, n,
                                 hipMemcpyHostToDevice, st));
        }
        if (eras)
            HIP_TRY(ezrs::copy2d(der, ecols * 4, h.eras, eras_stride * 4, ecols * 4, n,
                                 hipMemcpyHostToDevice, st));
        if (neras) HIP_TRY(hipMemcpyAsync(dne, h.neras, n * 4, hipMemcpyHostToDevice, st));
        if (positions)
            HIP_TRY(ezrs::copy2d(dps, (size_t)NR * 4, h.positions, pos_stride * 4, (size_t)NR * 4, n,
                                 hipMemcpyHostToDevice, st));
        if (corr)   // corr is copy-in/copy-out: entries the decode does not write keep their value
            HIP_TRY(ezrs::copy2d(dco, (size_t)NR * w, h.corr, corr_stride * w, (size_t)NR * w, n,
                                 hipMemcpyHostToDevice, st));
        HIP_TRY(dispatch_decode(c, d, reinterpret_cast<uint8_t *>(dsy), st));
        HIP_TRY(hipMemsetAsync(dct, 0, 4, st));
        HIP_TRY(launch_compact_rows(d.result, n, dcw, row, reinterpret_cast<uint32_t *>(dct),
                                    reinterpret_cast<uint32_t *>(dhb + h_cp), dhb, pitch, st));
        HIP_TRY(hipMemcpyAsync(h.result, drs, n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(hb + h_cp + h_ix, dct, 4, hipMemcpyDeviceToHost, st));
        if (positions)
            HIP_TRY(ezrs::copy2d(h.positions, pos_stride * 4, dps, (size_t)NR * 4, (size_t)NR * 4, n,
                                 hipMemcpyDeviceToHost, st));
        if (corr)
            HIP_TRY(ezrs::copy2d(h.corr, corr_stride * w, dco, (size_t)NR * w, (size_t)NR * w, n,
                                 hipMemcpyDeviceToHost, st));
        pend[s] = {k0, true};
    }
    for (int s = 0; s < 2; ++s)
        if (int r = finish(s)) return r;
    return 0;
}

int ezrs_host_alloc(void **ptr, size_t bytes) {
    if (!ptr) return -EINVAL;
    HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return 0;
}

int ezrs_host_free(void *ptr) {
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return 0;
}

} // extern "C"
