// ezbch.hip -- the C ABI of batched binary BCH on MI355X (gfx950), include/ezbch.h: codec tables,
// argument checks and the host-memory pipelines.  Host code only; there is no CPU path.
//
// Semantics: the Djelic / Linux lib/bch.c codec that the reference wraps as ezpwd::bch_base,
// ezpwd::bch<N,T> and ezpwd::BCH<N,K,T> (c++/ezpwd/bch:48-463) together with ezpwd::correct_bch
// (c++/ezpwd/bch_base:168-199), applied independently to every codeword of a batch:
//   encode : ECC = d(x) x^ecc_bits mod g(x), data bits MSB first, ECC left-justified big-endian in
//            ecc_bytes bytes, zero-initialised (bch:196-205)
//   decode : decode_bch's result (count / -EBADMSG / -EINVAL) and, as correct_bch, the reported
//            bits flipped in data and ECC; locations e address data[e/8] bit e%8 (ECC beyond
//            8*len), reported in ascending order (the reference's order is unpinned).
//
// Kernels: ezbch_lane.hip (one lane per codeword, and the fused decode of the plane-sliced codecs
// of ezbch_ps.hip) and ezbch_wave.hip (one wavefront per codeword), behind ezbch_internal.hpp.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/ezbch.h"
#include "ezbch_internal.hpp"
#include "ezbch_ps.hpp"
#include "ezrs_internal.hpp"
#include "ezrs_host.hpp"

using namespace ezbch;
using ezrs::bps_codec_id;

namespace {

using ezrs::align_up;
using ezrs::DeviceGuard;

thread_local std::string g_err;

int hip_fail(hipError_t e, const char *what) { return ezrs::hip_fail(g_err, e, what); }

// init_bch's default primitive polynomials, m = 5..15
const unsigned kDefaultPoly[11] = {0x25, 0x43, 0x83, 0x11d, 0x211, 0x409,
                                   0x805, 0x1053, 0x201b, 0x402b, 0x8003};

// Field tables and generator of init_bch(m, t, poly) (bch_base:49-69); false where init_bch fails.
struct HostBch {
    unsigned m = 0, n = 0, t = 0, poly = 0, ecc_bits = 0, ecc_bytes = 0;
    std::vector<uint16_t> ex, lg;
    std::vector<uint8_t> g;   // generator coefficients, x^0 first

    bool build(unsigned m_, unsigned t_, unsigned poly_) {
        if (m_ < 5 || m_ > 15) return false;
        m = m_;
        n = (1u << m) - 1;
        t = t_;
        if (t < 1 || m * t >= n) return false;
        poly = poly_ ? poly_ : kDefaultPoly[m - 5];
        if ((poly >> m) != 1) return false;
        ex.assign(2 * n, 0);
        lg.assign(n + 1, 0);
        std::vector<char> seen(n + 1, 0);
        for (unsigned i = 0, x = 1; i < n; ++i) {
            if (seen[x]) return false;                  // not primitive
            seen[x] = 1;
            ex[i] = ex[i + n] = (uint16_t)x;
            lg[x] = (uint16_t)i;
            x <<= 1;
            if (x >> m) x ^= poly;
        }
        std::vector<char> root(n, 0);                   // cyclotomic cosets of 1, 3, .., 2t-1
        for (unsigned i = 0; i < t; ++i)
            for (unsigned k = 0, j = 2 * i + 1; k < m; ++k, j = (2 * j) % n) root[j] = 1;
        std::vector<unsigned> gc(1, 1);
        auto mul = [&](unsigned a, unsigned b) -> unsigned { return (a && b) ? ex[lg[a] + lg[b]] : 0u; };
        for (unsigned j = 0; j < n; ++j) {
            if (!root[j]) continue;
            const unsigned r = ex[j];
            gc.push_back(0);
            for (size_t k = gc.size() - 1; k > 0; --k) gc[k] = gc[k - 1] ^ mul(gc[k], r);
            gc[0] = mul(gc[0], r);
        }
        g.resize(gc.size());
        for (size_t k = 0; k < gc.size(); ++k) {
            if (gc[k] > 1) return false;
            g[k] = (uint8_t)gc[k];
        }
        ecc_bits = (unsigned)g.size() - 1;
        ecc_bytes = (m * t + 7) / 8;
        return true;
    }

    // the lane path: t <= 64 and ecc_bits <= 1024; the wave path above
    bool wave() const { return t > (unsigned)kBigT || ecc_bits > 64u * kMaxNW; }
    unsigned nwl() const {
        const unsigned w = (ecc_bits + 63) / 64;             // 64-bit words
        return !wave() ? 0 : w <= 64 ? 1 : w <= 128 ? 2 : w <= 256 ? 4 : 8;
    }
    unsigned words() const {
        if (wave()) return 64 * nwl();
        return ecc_bits <= 64 ? 1 : ecc_bits <= 128 ? 2 : ecc_bits <= 256 ? 4 : ecc_bits <= 512 ? 8 : 16;
    }
    // step[v] = (v x^(E+8 nw 64-8) mod g) left-justified over nw words (w[0] most significant):
    // the remainder update for one data byte; laid out [v][word]
    std::vector<uint64_t> step_table() const {
        const unsigned E = ecc_bits, nw = words(), W = 64 * nw;
        std::vector<uint64_t> gl(nw, 0), tab(256 * nw);
        for (unsigned i = 0; i < E; ++i)
            if (g[i]) {
                const unsigned bit = W - E + i;                  // from the LSB of the whole
                gl[nw - 1 - bit / 64] |= 1ull << (bit % 64);
            }
        for (unsigned v = 0; v < 256; ++v) {
            std::vector<uint64_t> c(nw, 0);
            c[0] = (uint64_t)v << 56;
            for (int k = 0; k < 8; ++k) {
                const bool top = c[0] >> 63;
                for (unsigned i = 0; i < nw; ++i)
                    c[i] = (c[i] << 1) | (i + 1 < nw ? c[i + 1] >> 63 : 0);
                if (top)
                    for (unsigned i = 0; i < nw; ++i) c[i] ^= gl[i];
            }
            for (unsigned i = 0; i < nw; ++i) tab[v * nw + i] = c[i];
        }
        return tab;
    }
};

} // namespace

struct ezbch_codec {
    int device = 0;
    HostBch h;
    DevBch dev{};
    uint64_t *d_step = nullptr;
    uint16_t *d_tabs = nullptr;
    uint64_t *d_syn = nullptr;    // DevBch::syn_tab
    std::mutex mu;                // guards the host-pipeline buffers
    ezrs::StageBufs<1> d_stage;
    ezrs::StageBufs<1, hipHostMallocDefault> h_stage;   // pinned host staging (gathers, compact ECC)
    hipStream_t stream = nullptr;
};

namespace {

int create_impl(ezbch_codec **out, unsigned m, unsigned t, unsigned poly, int device, long want_k) {
    if (!out) return -EINVAL;
    *out = nullptr;
    HostBch h;
    if (!h.build(m, t, poly)) {
        g_err = "init_bch: invalid parameters (need 5 <= m <= 15, t >= 1, m*t < 2^m-1, a primitive "
                "polynomial of degree m)";
        return -EINVAL;
    }
    if (want_k >= 0 && (long)(h.n - h.ecc_bits) != want_k) {
        g_err = "BCH<N,K,T>: K does not match the codec init_bch builds (N - ecc_bits)";
        return -EINVAL;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0 || device < 0 || device >= ndev) {
        g_err = "no usable HIP device";
        return -ENODEV;
    }
    ezbch_codec *c = new (std::nothrow) ezbch_codec;
    if (!c) return -ENOMEM;
    c->device = device;
    c->h = std::move(h);
    DeviceGuard dg(device);
    const std::vector<uint64_t> tab = c->h.step_table();
    const size_t nt = c->h.ex.size() + c->h.lg.size();
    if ((e = hipMalloc(&c->d_step, tab.size() * 8)) != hipSuccess ||
        (e = hipMalloc(&c->d_tabs, nt * sizeof(uint16_t))) != hipSuccess ||
        (e = hipMemcpy(c->d_step, tab.data(), tab.size() * 8, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(c->d_tabs, c->h.ex.data(), c->h.ex.size() * 2, hipMemcpyHostToDevice)) !=
            hipSuccess ||
        (e = hipMemcpy(c->d_tabs + c->h.ex.size(), c->h.lg.data(), c->h.lg.size() * 2,
                       hipMemcpyHostToDevice)) != hipSuccess) {
        ezbch_destroy(c);
        return hip_fail(e, "BCH tables");
    }
    DevBch &d = c->dev;
    d.m = (int)m;
    d.n = (int)c->h.n;
    d.t = (int)t;
    d.ecc_bits = (int)c->h.ecc_bits;
    d.ecc_bytes = (int)c->h.ecc_bytes;
    d.lds_tabs = m <= 12;
    d.nw = (int)c->h.words();
    d.nwl = (int)c->h.nwl();
    for (int i = 0; i < kMaxNW && !d.nwl; ++i) {
        const int hi = (int)c->h.ecc_bits - 64 * i;             // significant bits in word i
        d.emask[i] = hi >= 64 ? ~0ull : hi <= 0 ? 0ull : ~0ull << (64 - hi);
    }
    d.step = c->d_step;
    d.ex = c->d_tabs;
    d.lg = c->d_tabs + c->h.ex.size();
    if (!d.nwl && d.nw == 1 && t <= 4) {    // syndrome byte tables (locate<T, 1>)
        std::vector<uint64_t> st(8 * 256, 0);
        const unsigned n = c->h.n, eb = c->h.ecc_bits;
        for (unsigned bb = 0; bb < 8; ++bb)
            for (unsigned v = 0; v < 256; ++v)
                for (unsigned i = 0; i < 8; ++i) {
                    if (!(v >> i & 1)) continue;
                    const unsigned lz = 63 - (56 - 8 * bb + i);      // the bit's leading-zero index
                    if (lz >= eb) continue;                           // masked (unused ECC bits)
                    const unsigned p = eb - 1 - lz;                   // S_j += alpha^(j p)
                    for (unsigned j = 1; j < 2 * t; j += 2)
                        st[bb * 256 + v] ^= (uint64_t)c->h.ex[(uint64_t)j * p % n] << (8 * (j - 1));
                }
        if ((e = hipMalloc(&c->d_syn, st.size() * 8)) != hipSuccess ||
            (e = hipMemcpy(c->d_syn, st.data(), st.size() * 8, hipMemcpyHostToDevice)) != hipSuccess) {
            ezbch_destroy(c);
            return hip_fail(e, "BCH syndrome tables");
        }
        d.syn_tab = c->d_syn;
    }
    d.bps = !d.nwl && c->h.ecc_bits % 8 == 0 && c->h.poly == kDefaultPoly[m - 5]
                ? bps_codec_id((int)m, (int)t, (int)c->h.ecc_bits) : -1;
    if (hipDeviceGetAttribute(&d.ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) d.ncu = 256;
    *out = c;
    return 0;
}

// Row geometry of a batch.  ecc == NULL is the row form, legal where row_form is set: the ECC
// follows the data in each row, and ecc / estride are resolved to it.  The stride rules hold for
// ncw > 1 only.
int check_rows(const ezbch_codec *c, const uint8_t *data, size_t dstride, unsigned len, uint8_t *&ecc,
               size_t &estride, size_t ncw, bool row_form) {
    if (!data || (!ecc && !row_form)) return -EINVAL;
    if (!ecc) {
        if (ncw > 1 && dstride < (size_t)len + c->h.ecc_bytes) return -EINVAL;
        ecc = const_cast<uint8_t *>(data) + len;
        estride = dstride;
    }
    if (ncw > 1 && (estride < c->h.ecc_bytes || dstride < len)) return -EINVAL;
    return 0;
}

// errloc rows hold up to t positions each.
bool bad_errloc(const ezbch_codec *c, const uint32_t *errloc, size_t errloc_stride, size_t ncw) {
    return errloc && ncw > 1 && errloc_stride < c->h.t;
}

// The kernels of one checked batch on the codec's device.
int run(const ezbch_codec *c, const BchArgs &a, bool decode, void *stream) {
    DeviceGuard g(c->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = decode ? launch_decode(c->dev, a, st) : launch_encode(c->dev, a, st);
    return e == hipSuccess ? 0 : hip_fail(e, decode ? "BCH decode launch" : "BCH encode launch");
}

int ensure_hstage(ezbch_codec *c, size_t bytes) {
    HIP_TRY(c->h_stage.ensure(bytes));
    return 0;
}

int ensure_stage(ezbch_codec *c, size_t bytes) {
    if (!c->stream) HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(c->d_stage.ensure(bytes));
    return 0;
}

} // namespace

extern "C" {

const char *ezbch_last_error(void) { return g_err.c_str(); }

int ezbch_create(ezbch_codec **out, unsigned m, unsigned t, unsigned prim_poly, int device) {
    return create_impl(out, m, t, prim_poly, device, -1);
}

int ezbch_create_nkt(ezbch_codec **out, unsigned n, unsigned k, unsigned t, int device) {
    unsigned m = 0;
    while (m < 16 && ((1u << m) - 1) < n) ++m;
    if (((1u << m) - 1) != n) {
        if (out) *out = nullptr;
        g_err = "BCH<N,K,T>: N must be 2^m - 1";
        return -EINVAL;
    }
    return create_impl(out, m, t, 0, device, (long)k);
}

int ezbch_destroy(ezbch_codec *c) {
    if (!c) return 0;
    DeviceGuard g(c->device);
    if (c->d_step) (void)hipFree(c->d_step);
    if (c->d_tabs) (void)hipFree(c->d_tabs);
    if (c->d_syn) (void)hipFree(c->d_syn);
    c->d_stage.release();
    c->h_stage.release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

int ezbch_get_info(const ezbch_codec *c, ezbch_info *info) {
    if (!c || !info) return -EINVAL;
    info->m = c->h.m;
    info->n = c->h.n;
    info->t = c->h.t;
    info->ecc_bits = c->h.ecc_bits;
    info->ecc_bytes = c->h.ecc_bytes;
    info->prim_poly = c->h.poly;
    info->device = c->device;
    return 0;
}

int ezbch_encode(const ezbch_codec *c, const uint8_t *data, size_t data_stride, unsigned len,
                 uint8_t *ecc, size_t ecc_stride, size_t ncw, void *stream) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (int r = check_rows(c, data, data_stride, len, ecc, ecc_stride, ncw, false)) return r;
    return run(c, BchArgs{data, nullptr, data_stride, len, ecc, ecc_stride, nullptr, nullptr, 0, ncw, 0},
               false, stream);
}

int ezbch_encode_rows(const ezbch_codec *c, uint8_t *rows, size_t stride, unsigned len,
                      size_t ncw, void *stream) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    uint8_t *ecc = nullptr;
    size_t ecc_stride = 0;
    if (int r = check_rows(c, rows, stride, len, ecc, ecc_stride, ncw, true)) return r;
    return ezbch_encode(c, rows, stride, len, ecc, ecc_stride, ncw, stream);
}

int ezbch_decode(const ezbch_codec *c, uint8_t *data, size_t data_stride, unsigned len,
                 uint8_t *ecc, size_t ecc_stride, int32_t *result, uint32_t *errloc,
                 size_t errloc_stride, size_t ncw, void *stream) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (!result) return -EINVAL;
    if (int r = check_rows(c, data, data_stride, len, ecc, ecc_stride, ncw, true)) return r;
    if (bad_errloc(c, errloc, errloc_stride, ncw)) return -EINVAL;
    return run(c, BchArgs{data, data, data_stride, len, ecc, ecc_stride, result, errloc, errloc_stride,
                          ncw, 0, 0}, true, stream);
}

int ezbch_decode_ecc(const ezbch_codec *c, const uint8_t *ecc, size_t ecc_stride, unsigned len,
                     int32_t *result, uint32_t *errloc, size_t errloc_stride, size_t ncw,
                     void *stream) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (!result || !ecc) return -EINVAL;
    if (ncw > 1 && ecc_stride < c->h.ecc_bytes) return -EINVAL;
    if (bad_errloc(c, errloc, errloc_stride, ncw)) return -EINVAL;
    return run(c, BchArgs{nullptr, nullptr, 0, len, const_cast<uint8_t *>(ecc), ecc_stride, result, errloc,
                          errloc_stride, ncw, 0, 0, 1}, true, stream);
}

int ezbch_decode_syn(const ezbch_codec *c, const uint32_t *syn, size_t syn_stride, unsigned len,
                     int32_t *result, uint32_t *errloc, size_t errloc_stride, size_t ncw,
                     void *stream) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (!result || !syn) return -EINVAL;
    if (ncw > 1 && syn_stride < 2 * (size_t)c->h.t) return -EINVAL;
    if (bad_errloc(c, errloc, errloc_stride, ncw)) return -EINVAL;
    return run(c, BchArgs{nullptr, nullptr, 0, len, nullptr, 0, result, errloc, errloc_stride, ncw, 0, 0, 1,
                          syn, syn_stride}, true, stream);
}

namespace {

// Host encode: rows' data bytes go to the device (one linear copy of the span when the pitch is at
// most twice the row, else a CPU gather into pinned staging), the kernel writes a compact
// [n][ecc_bytes] block, only that block comes back and a CPU scatter places each row's ECC.  The
// caller's data bytes are never written.
int bch_encode_host_core(ezbch_codec *c, const uint8_t *data, size_t data_stride, unsigned len,
                         uint8_t *ecc, size_t ecc_stride, size_t ncw, size_t chunk) {
    const size_t eb = c->h.ecc_bytes;
    // a single row is staged at pitch len whatever its stride (a stride below len, 0 included, is
    // legal for one codeword and must not size the staging)
    const bool span = ncw == 1 || data_stride <= 2 * (size_t)len + eb;
    const size_t drow = ncw == 1 ? len : span ? data_stride : len;
    const bool ecc_direct = ecc_stride == eb || ncw == 1;
    if (!chunk) chunk = ((size_t)64 << 20) / (drow ? drow : 1) + 1;
    if (chunk > ncw) chunk = ncw;
    const size_t b_in = align_up(chunk * drow + 16), b_ecc = align_up(chunk * eb);
    if (int r = ensure_stage(c, b_in + b_ecc)) return r;
    if (int r = ensure_hstage(c, (span ? 0 : align_up(chunk * len)) + (ecc_direct ? 0 : b_ecc) + 256))
        return r;
    uint8_t *st = static_cast<uint8_t *>(c->d_stage.p[0]), *dec = st + b_in;
    uint8_t *hs = static_cast<uint8_t *>(c->h_stage.p[0]);
    uint8_t *hin = hs, *hecc = hs + (span ? 0 : align_up(chunk * len));
    for (size_t k0 = 0; k0 < ncw; k0 += chunk) {
        const size_t n = ncw - k0 < chunk ? ncw - k0 : chunk;
        const uint8_t *hd = data + k0 * data_stride;
        if (span) {
            HIP_TRY(hipMemcpyAsync(st, hd, (n - 1) * data_stride + len, hipMemcpyHostToDevice, c->stream));
        } else {
            for (size_t r = 0; r < n; ++r) std::memcpy(hin + r * len, hd + r * data_stride, len);
            HIP_TRY(hipMemcpyAsync(st, hin, n * len, hipMemcpyHostToDevice, c->stream));
        }
        BchArgs a{st, nullptr, drow, len, dec, eb, nullptr, nullptr, 0, n, 0};
        HIP_TRY(launch_encode(c->dev, a, c->stream));
        HIP_TRY(hipMemcpyAsync(ecc_direct ? ecc + k0 * eb : hecc, dec, n * eb, hipMemcpyDeviceToHost,
                               c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!ecc_direct)
            for (size_t r = 0; r < n; ++r) std::memcpy(ecc + (k0 + r) * ecc_stride, hecc + r * eb, eb);
    }
    return 0;
}

} // namespace

int ezbch_encode_host(ezbch_codec *c, const uint8_t *data, size_t data_stride, unsigned len,
                      uint8_t *ecc, size_t ecc_stride, size_t ncw, size_t chunk) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (int r = check_rows(c, data, data_stride, len, ecc, ecc_stride, ncw, false)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    return bch_encode_host_core(c, data, data_stride, len, ecc, ecc_stride, ncw, chunk);
}

int ezbch_encode_rows_host(ezbch_codec *c, uint8_t *rows, size_t stride, unsigned len, size_t ncw,
                           size_t chunk) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    uint8_t *ecc = nullptr;
    size_t ecc_stride = 0;
    if (int r = check_rows(c, rows, stride, len, ecc, ecc_stride, ncw, true)) return r;
    return ezbch_encode_host(c, rows, stride, len, ecc, ecc_stride, ncw, chunk);
}

int ezbch_decode_syn_host(ezbch_codec *c, const uint32_t *syn, size_t syn_stride, unsigned len,
                          int32_t *result, uint32_t *errloc, size_t errloc_stride, size_t ncw) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (!result || !syn) return -EINVAL;
    const size_t S = 2 * (size_t)c->h.t, T = c->h.t;
    if (ncw > 1 && syn_stride < S) return -EINVAL;
    if (bad_errloc(c, errloc, errloc_stride, ncw)) return -EINVAL;
    if (ncw == 1) syn_stride = S, errloc_stride = T;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    const size_t b_syn = align_up(ncw * S * 4), b_res = align_up(ncw * 4);
    if (int r = ensure_stage(c, b_syn + b_res + ncw * T * 4)) return r;
    uint8_t *st = static_cast<uint8_t *>(c->d_stage.p[0]);
    uint32_t *dsyn = reinterpret_cast<uint32_t *>(st);
    int32_t *dres = reinterpret_cast<int32_t *>(st + b_syn);
    uint32_t *dloc = reinterpret_cast<uint32_t *>(st + b_syn + b_res);
    HIP_TRY(hipMemcpy2DAsync(dsyn, S * 4, syn, syn_stride * 4, S * 4, ncw, hipMemcpyHostToDevice, c->stream));
    if (int r = ezbch_decode_syn(c, dsyn, S, len, dres, errloc ? dloc : nullptr, T, ncw, c->stream)) return r;
    HIP_TRY(hipMemcpyAsync(result, dres, ncw * 4, hipMemcpyDeviceToHost, c->stream));
    if (errloc)
        HIP_TRY(hipMemcpy2DAsync(errloc, errloc_stride * 4, dloc, T * 4, T * 4, ncw, hipMemcpyDeviceToHost,
                                 c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ezbch_decode_host(ezbch_codec *c, uint8_t *data, size_t data_stride, unsigned len,
                      uint8_t *ecc, size_t ecc_stride, int32_t *result, uint32_t *errloc,
                      size_t errloc_stride, size_t ncw, size_t chunk) {
    if (!c) return -EINVAL;
    if (ncw == 0) return 0;
    if (!result) return -EINVAL;
    if (int r = check_rows(c, data, data_stride, len, ecc, ecc_stride, ncw, true)) return r;
    if (bad_errloc(c, errloc, errloc_stride, ncw)) return -EINVAL;
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard g(c->device);
    const size_t eb = c->h.ecc_bytes, row = (size_t)len + eb, T = c->h.t;
    if (!chunk) chunk = ((size_t)64 << 20) / row + 1;
    if (chunk > ncw) chunk = ncw;
    const size_t b_rows = align_up(chunk * row), b_res = align_up(chunk * 4);
    if (int r = ensure_stage(c, b_rows + b_res + align_up(errloc ? chunk * T * 4 : 0))) return r;
    uint8_t *st = static_cast<uint8_t *>(c->d_stage.p[0]);
    int32_t *dres = reinterpret_cast<int32_t *>(st + b_rows);
    uint32_t *dloc = reinterpret_cast<uint32_t *>(st + b_rows + b_res);
    for (size_t k0 = 0; k0 < ncw; k0 += chunk) {
        const size_t n = ncw - k0 < chunk ? ncw - k0 : chunk;
        if (len)
            HIP_TRY(ezrs::copy2d(st, row, data + k0 * data_stride, data_stride, len, n,
                                     hipMemcpyHostToDevice, c->stream));
        HIP_TRY(ezrs::copy2d(st + len, row, ecc + k0 * ecc_stride, ecc_stride, eb, n,
                                 hipMemcpyHostToDevice, c->stream));
        if (errloc)   // copy-in/copy-out: entries the decode does not write keep their value
            HIP_TRY(ezrs::copy2d(dloc, T * 4, errloc + k0 * errloc_stride, errloc_stride * 4,
                                     T * 4, n, hipMemcpyHostToDevice, c->stream));
        BchArgs a{st, st, row, len, st + len, row, dres, errloc ? dloc : nullptr, T, n, 0};
        HIP_TRY(launch_decode(c->dev, a, c->stream));
        if (len)
            HIP_TRY(ezrs::copy2d(data + k0 * data_stride, data_stride, st, row, len, n,
                                     hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(ezrs::copy2d(ecc + k0 * ecc_stride, ecc_stride, st + len, row, eb, n,
                                 hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(result + k0, dres, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (errloc)
            HIP_TRY(ezrs::copy2d(errloc + k0 * errloc_stride, errloc_stride * 4, dloc, T * 4,
                                     T * 4, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

} // extern "C"
