// txgen.cpp -- the synthetic sources and the TX generator of libgsdr.so (include/gsdr.h): gsdr_source_*,
// gsdr_txgen_* and gsdr_narrow_sc16_device.
//
// Host-side counterpart of TX_buffer_generator (ref: cpp/USRP_buffer_generator.cpp).  Every entry that writes samples
// exists for two wire formats, complex64 and sc16 (interleaved int16 I/Q): one body each, written for a format
// (Complex64 / Sc16 below), behind two extern "C" names.
//
// "ref:" citations are relative to /root/reference.
#include <cstdlib>
#include <string>
#include <vector>

#include "host_util.h"

using gsdr::ChirpShape;
using gsdr::chirp_shape;
using gsdr::create_error;
using gsdr::device_cus;
using gsdr::mod_rate;
using gsdr::phasor;

namespace gsdr {

// What a generator keeps per wire format.
template <typename T>
struct TxBuffers {
    DevBuf<T> d_stage;         // get() to host memory goes through here
    size_t stage_n = 0;        // samples d_stage holds
    // TONES through get_ptr: one period + one buffer of the comb in host memory, made once
    // (the reference's base_buffer, cpp/USRP_buffer_generator.cpp:77-95)
    T *h_period = nullptr;
    bool h_period_pinned = false;
};

}  // namespace gsdr

// ---- TX tone comb at scale (row f3) ------------------------------------------
struct gsdr_txgen {
    int device = -1;
    unsigned rate = 1;
    int n_tones = 0;
    gsdr::DevBuf<unsigned> d_fmod;
    gsdr::DevBuf<float2> d_q0, d_btab, d_ctab;
    // the TX_buffer_generator state (gsdr_txgen_create)
    int mode = -1;                     // GSDR_TONES / GSDR_CHIRP, -1: a bare tone comb (gsdr_txgen_tones_create)
    long long buffer_len = 0;
    unsigned long long period = 1, last = 0;
    gsdr_chirp_param cp{};
    float scale = 1.f;
    // several chirps added into one buffer (gsdr_txgen_create_ex, GSDR_CREATE_MULTI_CHIRP): n_chirps > 1, cp is chirp 0
    int n_chirps = 1;
    gsdr::MultiChirp mc{};
    gsdr::MultiScale msc{};
    gsdr::TxBuffers<gsdr_c64> c64;
    // sc16 output (gsdr_txgen_*_sc16): the gain of the narrowing, the counter of clipped components (device memory,
    // zeroed at creation), and a staging buffer (4 bytes per sample) and a period buffer of its own
    float sc16_gain = 32767.0f;
    gsdr::DevBuf<unsigned long long> d_clipped;
    gsdr::TxBuffers<gsdr_sc16> sc16;
};

namespace {

bool sc16_gain_ok(float gain) { return std::isfinite(gain) && gain > 0.f; }

// The two wire formats of the TX entries.  A format names its element type, the buffers of the generator it owns and
// the launchers that write it; where the entries of the two formats answer a caller differently (include/gsdr.h), the
// difference is a named property here and the one body asks for it.
struct Complex64 {
    using elem = gsdr_c64;
    static constexpr const char *suffix = "";   // entry names: gsdr_txgen_get, gsdr_source_chirp, ...
    // n == 0 is no special case: gsdr_txgen_tones_fill refuses a NULL out_dev as for any n, otherwise goes on to
    // hipSetDevice and a launcher that does nothing; gsdr_source_chirp checks its arguments and hands 0 to the launcher
    static constexpr bool empty_returns_first = false;
    // gsdr_source_chirp refuses bad arguments with -1 alone: what gsdr_last_error(NULL) said before, it still says
    static constexpr bool chirp_refusal_has_message = false;
    static gsdr::TxBuffers<elem> &buffers(gsdr_txgen *g) { return g->c64; }
    static const char *narrowing_fault(const elem *, float, const unsigned long long *) { return nullptr; }   // none to check
    static hipError_t tones(const gsdr_txgen *g, elem *out, long long n, unsigned long long start, hipStream_t st) {
        return gsdr::launch_tones_synth(reinterpret_cast<float2 *>(out), n, start, g->rate, g->d_fmod, g->d_q0, g->d_btab,
                                        g->d_ctab, g->n_tones, st);
    }
    static hipError_t chirp(elem *out, long long n, unsigned long long index0, const ChirpShape &cs, float scale, float,
                            unsigned long long *, hipStream_t st) {
        return gsdr::launch_source_chirp(reinterpret_cast<float2 *>(out), n, index0, cs, scale, st);
    }
    static hipError_t multichirp(elem *out, long long n, unsigned long long index0, const gsdr::MultiChirp &mc,
                                 const gsdr::MultiScale &sc, float, unsigned long long *, hipStream_t st) {
        return gsdr::launch_source_multichirp(reinterpret_cast<float2 *>(out), n, index0, mc, sc, st);
    }
};

struct Sc16 {
    using elem = gsdr_sc16;
    static constexpr const char *suffix = "_sc16";
    // n == 0 returns 0 before anything else is looked at (gsdr_txgen_tones_fill_sc16: behind the handle and n < 0);
    // a NULL out_dev is refused for n > 0 only
    static constexpr bool empty_returns_first = true;
    static constexpr bool chirp_refusal_has_message = true;
    static gsdr::TxBuffers<elem> &buffers(gsdr_txgen *g) { return g->sc16; }
    // gsdr_source_chirp_sc16 takes the gain and the counter from its caller: checked behind the other arguments
    static const char *narrowing_fault(const elem *out, float gain, const unsigned long long *clipped) {
        if (!sc16_gain_ok(gain)) return "the gain must be finite and > 0";
        if (((uintptr_t)out & 3) || ((uintptr_t)clipped & 7)) return "out_dev must be 4-byte, clipped_dev 8-byte aligned";
        return nullptr;
    }
    static hipError_t tones(const gsdr_txgen *g, elem *out, long long n, unsigned long long start, hipStream_t st) {
        return gsdr::launch_tones_synth_sc16(out, n, start, g->rate, g->d_fmod, g->d_q0, g->d_btab, g->d_ctab, g->n_tones,
                                             g->sc16_gain, g->d_clipped, st);
    }
    static hipError_t chirp(elem *out, long long n, unsigned long long index0, const ChirpShape &cs, float scale, float gain,
                            unsigned long long *clipped, hipStream_t st) {
        return gsdr::launch_source_chirp_sc16(out, n, index0, cs, scale, gain, clipped, st);
    }
    static hipError_t multichirp(elem *out, long long n, unsigned long long index0, const gsdr::MultiChirp &mc,
                                 const gsdr::MultiScale &sc, float gain, unsigned long long *clipped, hipStream_t st) {
        return gsdr::launch_source_multichirp_sc16(out, n, index0, mc, sc, gain, clipped, st);
    }
};

// "<entry><_sc16>: <what>" into gsdr_last_error(NULL); returns -1
template <typename Fmt>
int refuse(const char *entry, const char *what) {
    create_error() = std::string(entry) + Fmt::suffix + ": " + what;
    return -1;
}

bool set_device(const gsdr_txgen *g) { return g->device < 0 || hipSetDevice(g->device) == hipSuccess; }

// the generator's counter of clipped components: 8 bytes of device memory, zero (the creating call has set the device)
bool txgen_make_counter(gsdr_txgen *g) { return g->d_clipped.alloc_zeroed(1) == hipSuccess; }

// the staging buffer of the host entries: at least `samples` elements in device memory, grown on demand
template <typename T>
bool stage_reserve(gsdr::TxBuffers<T> &b, size_t samples) {
    if (b.d_stage && b.stage_n >= samples) return true;
    b.stage_n = 0;
    if (b.d_stage.alloc(samples) != hipSuccess) {   // (frees the shorter one first)
        (void)hipGetLastError();
        return false;
    }
    b.stage_n = samples;
    return true;
}

// the period buffer: pinned host memory, else malloc
template <typename T>
T *period_alloc(size_t count, bool &pinned) {
    T *p = nullptr;
    pinned = hipHostMalloc((void **)&p, count * sizeof(T)) == hipSuccess;
    if (!pinned) {
        (void)hipGetLastError();
        p = (T *)std::malloc(count * sizeof(T));
    }
    return p;
}

template <typename T>
void period_free(T *p, bool pinned) {
    if (!p) return;
    if (pinned) (void)hipHostFree(p);
    else std::free(p);
}

template <typename Fmt>
int tones_fill(gsdr_txgen *g, typename Fmt::elem *out_dev, long long n, long long start, void *hip_stream) {
    const bool need_out = !Fmt::empty_returns_first || n > 0;
    if (!g || n < 0 || (need_out && !out_dev)) return refuse<Fmt>("gsdr_txgen_tones_fill", "bad arguments");
    if (Fmt::empty_returns_first && n == 0) return 0;
    if (!set_device(g)) return refuse<Fmt>("gsdr_txgen_tones_fill", "hipSetDevice failed");
    const hipError_t e = Fmt::tones(g, out_dev, n, mod_rate(start, g->rate), (hipStream_t)hip_stream);
    if (e != hipSuccess) return refuse<Fmt>("gsdr_txgen_tones_fill", hipGetErrorString(e));
    return 0;
}

template <typename Fmt>
int source_chirp(typename Fmt::elem *out_dev, long long n, unsigned long long last_index, const gsdr_chirp_param *cp,
                 float scale, float gain, unsigned long long *clipped_dev, void *hip_stream) {
    if (Fmt::empty_returns_first && n == 0) return 0;
    const char *bad = nullptr;
    if (!out_dev || !cp || n < 0 || cp->num_steps < 1 || cp->length < 1) bad = "bad arguments";
    else bad = Fmt::narrowing_fault(out_dev, gain, clipped_dev);
    if (bad) return Fmt::chirp_refusal_has_message ? refuse<Fmt>("gsdr_source_chirp", bad) : -1;
    const ChirpShape cs = chirp_shape(*cp);
    const hipError_t e = Fmt::chirp(out_dev, n, last_index % cs.period, cs, scale, gain, clipped_dev, (hipStream_t)hip_stream);
    if (e != hipSuccess) return refuse<Fmt>("gsdr_source_chirp", hipGetErrorString(e));
    return 0;
}

// the sum of several chirps from the tables the kernel takes (mc, sc: checked by the caller)
template <typename Fmt>
int multichirp_launch(typename Fmt::elem *out_dev, long long n, unsigned long long last_index, const gsdr::MultiChirp &mc,
                      const gsdr::MultiScale &sc, float gain, unsigned long long *clipped_dev, void *hip_stream) {
    const hipError_t e = Fmt::multichirp(out_dev, n, last_index % mc.period, mc, sc, gain, clipped_dev, (hipStream_t)hip_stream);
    if (e != hipSuccess) return refuse<Fmt>("gsdr_source_multichirp", hipGetErrorString(e));
    return 0;
}

// gsdr_source_multichirp and gsdr_source_multichirp_sc16: every refusal has a message; n == 0 touches nothing
template <typename Fmt>
int source_multichirp(typename Fmt::elem *out_dev, long long n, unsigned long long last_index, const gsdr_chirp_param *cp,
                      const float *scale, int n_chirps, float gain, unsigned long long *clipped_dev, void *hip_stream) {
    if (n == 0) return 0;
    const char *bad = nullptr;
    gsdr::MultiChirp mc;
    gsdr::MultiScale sc{};
    if (!out_dev || !cp || !scale || n < 0) bad = "bad arguments";
    else if (n_chirps < 1 || n_chirps > GSDR_MULTI_CHIRP_MAX) bad = "n_chirps must be in [1, GSDR_MULTI_CHIRP_MAX]";
    else bad = gsdr::multi_chirp_shape(cp, n_chirps, mc);
    if (!bad) bad = Fmt::narrowing_fault(out_dev, gain, clipped_dev);
    if (bad) return refuse<Fmt>("gsdr_source_multichirp", bad);
    for (int c = 0; c < n_chirps; ++c) sc.s[c] = scale[c];
    return multichirp_launch<Fmt>(out_dev, n, last_index, mc, sc, gain, clipped_dev, hip_stream);
}

// ref: get_from_tones :226-229, get_from_chirp :208-221.  get_device and get report under one name: gsdr_txgen_get
template <typename Fmt>
int get_device(gsdr_txgen *g, typename Fmt::elem *out_dev, void *hip_stream) {
    if (!g || !out_dev || g->mode < 0) return refuse<Fmt>("gsdr_txgen_get", "bad arguments");
    int rc;
    if (g->mode == GSDR_TONES) {
        rc = tones_fill<Fmt>(g, out_dev, g->buffer_len, (long long)(g->last % g->rate), hip_stream);
    } else {
        if (!set_device(g)) return refuse<Fmt>("gsdr_txgen_get", "hipSetDevice failed");
        if (g->n_chirps > 1)
            rc = multichirp_launch<Fmt>(out_dev, g->buffer_len, g->last, g->mc, g->msc, g->sc16_gain, g->d_clipped, hip_stream);
        else
            rc = source_chirp<Fmt>(out_dev, g->buffer_len, g->last, &g->cp, g->scale, g->sc16_gain, g->d_clipped, hip_stream);
    }
    if (rc == 0) g->last = (g->last + (unsigned long long)g->buffer_len) % g->period;
    return rc;
}

template <typename Fmt>
int get_host(gsdr_txgen *g, typename Fmt::elem *out_host) {
    if (!g || !out_host || g->mode < 0) return refuse<Fmt>("gsdr_txgen_get", "bad arguments");
    if (!set_device(g)) return refuse<Fmt>("gsdr_txgen_get", "hipSetDevice failed");
    auto &b = Fmt::buffers(g);
    if (!stage_reserve(b, (size_t)g->buffer_len)) return refuse<Fmt>("gsdr_txgen_get", "device allocation failed");
    if (get_device<Fmt>(g, b.d_stage, nullptr) != 0) return -1;
    const hipError_t e = hipMemcpy(out_host, b.d_stage, (size_t)g->buffer_len * sizeof(typename Fmt::elem), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return refuse<Fmt>("gsdr_txgen_get", hipGetErrorString(e));
    return 0;
}

// ref: the TONES branch of the constructor (:77-95): base_buffer = one period (TONES_buffer_len samples) plus
// buffer_len more (a copy of its beginning), in host memory.  Made once, in pieces through the staging buffer of the
// format; the period buffer of the other format is neither needed nor made.
template <typename Fmt>
int prepare_host(gsdr_txgen *g) {
    using T = typename Fmt::elem;
    if (!g || g->mode != GSDR_TONES) return refuse<Fmt>("gsdr_txgen_prepare_host", "a TONES generator is needed");
    auto &b = Fmt::buffers(g);
    if (b.h_period) return 0;
    if (!set_device(g)) return refuse<Fmt>("gsdr_txgen_prepare_host", "hipSetDevice failed");
    const unsigned long long total = g->period + (unsigned long long)g->buffer_len;
    bool pinned = false;
    T *hp = period_alloc<T>((size_t)total, pinned);
    if (!hp) return refuse<Fmt>("gsdr_txgen_prepare_host", "cannot allocate the period buffer in host memory");
    const size_t piece = (size_t)(total < (8u << 20) ? total : (8u << 20));
    bool ok = stage_reserve(b, piece);
    for (unsigned long long off = 0; ok && off < total; off += piece) {
        const long long n = (long long)(total - off < piece ? total - off : piece);
        ok = tones_fill<Fmt>(g, b.d_stage, n, (long long)(off % g->rate), nullptr) == 0 &&
             hipMemcpy(hp + off, b.d_stage, (size_t)n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) {
        period_free(hp, pinned);
        if (create_error().empty()) refuse<Fmt>("gsdr_txgen_prepare_host", "generating the period failed");
        return -1;
    }
    b.h_period = hp;
    b.h_period_pinned = pinned;
    return 0;
}

// ref: get_from_tones (:226-229): *target = base_buffer + TONES_last_sample -- the caller's pointer is REPLACED by one
// into the generator's own period buffer (tx_single_link hands in an unallocated pointer for TONES,
// cpp/USRP_server_link_threads.cpp:568-584, and never frees what it gets back).
template <typename Fmt>
const typename Fmt::elem *get_ptr(gsdr_txgen *g) {
    if (!g || g->mode != GSDR_TONES) {
        refuse<Fmt>("gsdr_txgen_get_ptr", "a TONES generator is needed");
        return nullptr;
    }
    auto &b = Fmt::buffers(g);
    if (!b.h_period && prepare_host<Fmt>(g) != 0) return nullptr;
    const typename Fmt::elem *p = b.h_period + g->last;
    g->last = (g->last + (unsigned long long)g->buffer_len) % g->period;
    return p;
}

}  // namespace

extern "C" {

// ---- synthetic sources -----------------------------------------------------
int gsdr_source_tones(gsdr_c64 *out_dev, long long n, long long start, int rate, const int *freq,
                      const float *ampl, const float *phase, int n_tones, float sigma,
                      unsigned long long seed, void *hip_stream) {
    if (!out_dev || n < 0 || rate <= 0 || n_tones < 0) return -1;
    std::vector<unsigned> fm(n_tones > 0 ? n_tones : 1, 0u);
    for (int k = 0; k < n_tones; ++k) fm[k] = mod_rate(freq[k], rate);
    gsdr::DevBuf<unsigned> d_f;
    gsdr::DevBuf<float> d_a, d_p;
    const size_t cnt = fm.size();
    hipError_t e = d_f.alloc(cnt);
    if (e == hipSuccess) e = d_a.alloc(cnt);
    if (e == hipSuccess) e = d_p.alloc(cnt);
    if (e == hipSuccess) e = hipMemcpy(d_f, fm.data(), cnt * sizeof(unsigned), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_tones > 0) e = hipMemcpy(d_a, ampl, n_tones * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_tones > 0) e = hipMemcpy(d_p, phase, n_tones * sizeof(float), hipMemcpyHostToDevice);
    hipStream_t st = (hipStream_t)hip_stream;
    if (e == hipSuccess)
        e = gsdr::launch_source_tones(reinterpret_cast<float2 *>(out_dev), n, mod_rate(start, rate), (unsigned)rate,
                                      d_f, d_a, d_p, n_tones, sigma, seed, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        create_error() = std::string("gsdr_source_tones: ") + hipGetErrorString(e);
        return -1;
    }
    return 0;
}

int gsdr_source_chirp(gsdr_c64 *out_dev, long long n, unsigned long long last_index,
                      const gsdr_chirp_param *cp, float scale, void *hip_stream) {
    return source_chirp<Complex64>(out_dev, n, last_index, cp, scale, 0.f, nullptr, hip_stream);
}

int gsdr_source_chirp_sc16(gsdr_sc16 *out_dev, long long n, unsigned long long last_index, const gsdr_chirp_param *cp,
                           float scale, float gain, unsigned long long *clipped_dev, void *hip_stream) {
    return source_chirp<Sc16>(out_dev, n, last_index, cp, scale, gain, clipped_dev, hip_stream);
}

int gsdr_narrow_sc16_device(const gsdr_c64 *in_dev, gsdr_sc16 *out_dev, long long n, float gain,
                            unsigned long long *clipped_dev, void *hip_stream) {
    if (n == 0) return 0;
    const char *bad = nullptr;
    if (n < 0 || !in_dev || !out_dev) bad = "null buffer";
    else if (!sc16_gain_ok(gain)) bad = "the gain must be finite and > 0";
    else if (((uintptr_t)in_dev & 7) || ((uintptr_t)out_dev & 3) || ((uintptr_t)clipped_dev & 7))
        bad = "in_dev and clipped_dev must be 8-byte, out_dev 4-byte aligned";
    if (bad) {
        create_error() = std::string("gsdr_narrow_sc16_device: ") + bad;
        return -1;
    }
    const hipError_t e = gsdr::launch_narrow_sc16(reinterpret_cast<const float2 *>(in_dev), out_dev, n, gain, clipped_dev,
                                                  device_cus(), (hipStream_t)hip_stream);
    if (e != hipSuccess) {
        create_error() = std::string("gsdr_narrow_sc16_device: ") + hipGetErrorString(e);
        return -1;
    }
    return 0;
}

// ---- the TX generator --------------------------------------------------------
gsdr_txgen *gsdr_txgen_tones_create(int rate, const int *freq, const float *ampl, const float *phase, int n_tones,
                                    int device_index) {
    create_error().clear();
    if (rate <= 0 || n_tones < 0 || (n_tones > 0 && (!freq || !ampl))) {
        create_error() = "gsdr_txgen_tones_create: bad arguments";
        return nullptr;
    }
    if (device_index >= 0 && hipSetDevice(device_index) != hipSuccess) {
        create_error() = "gsdr_txgen_tones_create: hipSetDevice failed (no such GPU?)";
        return nullptr;
    }
    gsdr_txgen *g = new gsdr_txgen();
    g->device = device_index;
    g->rate = (unsigned)rate;
    g->n_tones = n_tones;
    const size_t N = (size_t)(n_tones > 0 ? n_tones : 1);
    std::vector<unsigned> fm(N, 0u);
    std::vector<float2> q0(N, make_float2(0.f, 0.f)), bt(N * 64), ct(N * 16);
    for (int k = 0; k < n_tones; ++k) {
        const unsigned r = mod_rate(freq[k], rate);
        fm[(size_t)k] = r;
        const double ph0 = phase ? (double)phase[k] : 0.0;
        q0[(size_t)k] = make_float2((float)((double)ampl[k] * std::cos(ph0)), (float)((double)ampl[k] * std::sin(ph0)));
        // w^m for the exact integer phase (f m) mod rate, TX sign: e^(+2 pi i ...)
        auto w = [&](unsigned long long m) {
            double re, im;
            phasor(((unsigned long long)r * m) % (unsigned long long)rate, (unsigned)rate, re, im);   // e^(-...)
            return make_float2((float)re, (float)-im);
        };
        for (int lo = 0; lo < 64; ++lo) bt[(size_t)k * 64 + lo] = w((unsigned long long)lo);
        for (int j = 0; j < 16; ++j) ct[(size_t)k * 16 + j] = w(64ULL * (unsigned long long)j);
    }
    const bool ok = g->d_fmod.upload(fm) == hipSuccess && g->d_q0.upload(q0) == hipSuccess &&
                    g->d_btab.upload(bt) == hipSuccess && g->d_ctab.upload(ct) == hipSuccess &&
                    txgen_make_counter(g) && hipStreamSynchronize(nullptr) == hipSuccess;
    if (!ok) {
        create_error() = "gsdr_txgen_tones_create: device allocation failed";
        gsdr_txgen_close(g);
        return nullptr;
    }
    return g;
}

void gsdr_txgen_close(gsdr_txgen *g) {
    if (!g) return;
    if (g->device >= 0) (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();
    period_free(g->c64.h_period, g->c64.h_period_pinned);
    period_free(g->sc16.h_period, g->sc16.h_period_pinned);
    delete g;
}

// ref: TX_buffer_generator::TX_buffer_generator, cpp/USRP_buffer_generator.cpp:10-160
gsdr_txgen *gsdr_txgen_create(const gsdr_param_c *p, const float *ampl, int n_ampl) {
    return gsdr_txgen_create_ex(p, ampl, n_ampl, 0u);
}

int gsdr_source_multichirp(gsdr_c64 *out_dev, long long n, unsigned long long last_index, const gsdr_chirp_param *cp,
                           const float *scale, int n_chirps, void *hip_stream) {
    return source_multichirp<Complex64>(out_dev, n, last_index, cp, scale, n_chirps, 0.f, nullptr, hip_stream);
}

int gsdr_source_multichirp_sc16(gsdr_sc16 *out_dev, long long n, unsigned long long last_index, const gsdr_chirp_param *cp,
                                const float *scale, int n_chirps, float gain, unsigned long long *clipped_dev,
                                void *hip_stream) {
    return source_multichirp<Sc16>(out_dev, n, last_index, cp, scale, n_chirps, gain, clipped_dev, hip_stream);
}

// flags: GSDR_CREATE_* (include/gsdr.h, "several chirps in one handle"); 0 is gsdr_txgen_create
gsdr_txgen *gsdr_txgen_create_ex(const gsdr_param_c *p, const float *ampl, int n_ampl, unsigned flags) {
    create_error().clear();
    auto fail = [](const char *msg) {
        create_error() = msg;
        return (gsdr_txgen *)nullptr;
    };
    if (flags & ~GSDR_CREATE_MULTI_CHIRP) return fail("unknown creation flag");
    if (!p) return fail("null parameters");
    if (p->buffer_len < 1) return fail("buffer_len must be positive");
    if (p->rate < 1) return fail("rate must be positive");
    if (p->n_wave_type < 1 || !p->wave_type) return fail("TX buffer generation needs at least one wave_type");
    const int last = p->wave_type[0];
    int chirps = 0;
    bool mixed = false;
    for (int i = 0; i < p->n_wave_type; ++i) {
        chirps += p->wave_type[i] == GSDR_CHIRP;
        mixed |= p->wave_type[i] != last;
    }
    if (chirps > 1 && !(flags & GSDR_CREATE_MULTI_CHIRP))      // :26-29
        return fail("Multiple chirp TX buffer generation has been requested. This feature is not implemented yet.");
    if (mixed)           // :31-34
        return fail("Mixed TX buffer generation has been requested. This feature is not implemented yet.");
    if (last == GSDR_NODSP || last == GSDR_SWONLY) return fail("NODSP CASE NOT IMPLEMENTED.");   // :41-44
    if (last == GSDR_RAMP || last == GSDR_DIRECT) return fail("RAMP CASE NOT IMPLEMENTED.");      // :46-49
    gsdr_txgen *g = nullptr;
    // NOISE: the reference's `case NOISE:` (:52-58) has no break and falls through into TONES, which overwrites its
    // get/close pointers: a TX NOISE request generates the tone comb of freq[] / ampl[] there, and so it does here
    if (last == GSDR_TONES || last == GSDR_NOISE) {
        const int n = p->n_wave_type;
        if (p->n_freq < n || !p->freq || n_ampl < n || !ampl) return fail("TONES needs freq[] and ampl[] for every wave_type entry");
        std::vector<int> tf((size_t)n);
        std::vector<float> ta((size_t)n);
        const int nt = gsdr_tx_tone_bins(p->rate, p->freq, ampl, n, tf.data(), ta.data());
        g = gsdr_txgen_tones_create(p->rate, tf.data(), ta.data(), nullptr, nt > 0 ? nt : 0, p->device_index);
        if (!g) return nullptr;
        // TONES_buffer_len: rate, or the multiple of it that holds one buffer (:60-75)
        g->period = (unsigned long long)p->rate * (unsigned long long)((p->buffer_len + p->rate - 1) / p->rate);
    } else if (last == GSDR_CHIRP) {
        if (p->n_freq < 1 || p->n_chirp_f < 1 || p->n_swipe_s < 1 || p->n_chirp_t < 1 || !p->freq || !p->chirp_f ||
            !p->swipe_s || !p->chirp_t)
            return fail("CHIRP needs freq[0], chirp_f[0], swipe_s[0] and chirp_t[0]");
        // several chirps: everything that can be refused is, before the device is touched
        gsdr::MultiChirp mc{};
        gsdr::MultiScale msc{};
        if (chirps > 1) {
            if (const char *bad = gsdr::multi_chirp_fault(p, chirps)) return fail(bad);
            gsdr_chirp_param all[GSDR_MULTI_CHIRP_MAX];
            for (int c = 0; c < chirps; ++c) {
                gsdr_chirp_derive_tx(p->rate, p->freq[c], p->chirp_f[c], p->swipe_s[0], p->chirp_t[0], &all[c]);
                msc.s[c] = c < n_ampl && ampl ? ampl[c] : 1.f;
            }
            if (const char *bad = gsdr::multi_chirp_shape(all, chirps, mc)) return fail(bad);
        }
        if (p->device_index >= 0 && hipSetDevice(p->device_index) != hipSuccess)
            return fail("hipSetDevice failed (no such GPU?)");
        g = new gsdr_txgen();
        g->n_chirps = chirps;
        g->mc = mc;
        g->msc = msc;
        g->device = p->device_index;
        g->rate = (unsigned)p->rate;
        // the TX side's own derivation: a step shorter than one sample also resets num_steps, and the slope
        // follows the reset value (:107-129)
        gsdr_chirp_derive_tx(p->rate, p->freq[0], p->chirp_f[0], p->swipe_s[0], p->chirp_t[0], &g->cp);
        if (g->cp.num_steps < 1 || g->cp.length < 1 || g->cp.num_steps > 0x7fffffffffffffffULL / g->cp.length) {
            delete g;
            return fail("chirp period overflows");
        }
        g->period = g->cp.num_steps * g->cp.length;
        g->scale = n_ampl > 0 && ampl ? ampl[0] : 1.f;
        if (!txgen_make_counter(g) || hipStreamSynchronize(nullptr) != hipSuccess) {
            gsdr_txgen_close(g);
            return fail("device allocation failed");
        }
    } else {
        return fail("Void TX generation operation has not been implemented yet!");
    }
    g->mode = last == GSDR_NOISE ? GSDR_TONES : last;
    g->buffer_len = p->buffer_len;
    g->last = 0;
    return g;
}

long long gsdr_txgen_buffer_len(const gsdr_txgen *g) { return g ? g->buffer_len : 0; }
int gsdr_txgen_mode(const gsdr_txgen *g) { return g ? g->mode : -1; }

// ---- the entries that write samples: complex64, and sc16 (include/gsdr.h, "sc16 output") -----------------------------
int gsdr_txgen_tones_fill(gsdr_txgen *g, gsdr_c64 *out_dev, long long n, long long start, void *hip_stream) {
    return tones_fill<Complex64>(g, out_dev, n, start, hip_stream);
}
int gsdr_txgen_tones_fill_sc16(gsdr_txgen *g, gsdr_sc16 *out_dev, long long n, long long start, void *hip_stream) {
    return tones_fill<Sc16>(g, out_dev, n, start, hip_stream);
}

int gsdr_txgen_get_device(gsdr_txgen *g, gsdr_c64 *out_dev, void *hip_stream) { return get_device<Complex64>(g, out_dev, hip_stream); }
int gsdr_txgen_get_device_sc16(gsdr_txgen *g, gsdr_sc16 *out_dev, void *hip_stream) { return get_device<Sc16>(g, out_dev, hip_stream); }

int gsdr_txgen_get(gsdr_txgen *g, gsdr_c64 *out_host) { return get_host<Complex64>(g, out_host); }
int gsdr_txgen_get_sc16(gsdr_txgen *g, gsdr_sc16 *out_host) { return get_host<Sc16>(g, out_host); }

int gsdr_txgen_prepare_host(gsdr_txgen *g) { return prepare_host<Complex64>(g); }
int gsdr_txgen_prepare_host_sc16(gsdr_txgen *g) { return prepare_host<Sc16>(g); }

const gsdr_c64 *gsdr_txgen_get_ptr(gsdr_txgen *g) { return get_ptr<Complex64>(g); }
const gsdr_sc16 *gsdr_txgen_get_ptr_sc16(gsdr_txgen *g) { return get_ptr<Sc16>(g); }

int gsdr_txgen_set_sc16_gain(gsdr_txgen *g, float gain) {
    const char *bad = nullptr;
    if (!g) bad = "gsdr_txgen_set_sc16_gain: null handle";
    else if (!sc16_gain_ok(gain)) bad = "gsdr_txgen_set_sc16_gain: the gain must be finite and > 0";
    else if (g->sc16.h_period) bad = "gsdr_txgen_set_sc16_gain: the sc16 period buffer exists already (it was made with the gain of that time)";
    if (bad) {
        create_error() = bad;
        return -1;
    }
    g->sc16_gain = gain;
    return 0;
}

float gsdr_txgen_sc16_gain(const gsdr_txgen *g) { return g ? g->sc16_gain : 0.f; }

// a diagnostic: waits for everything the device has been given
long long gsdr_txgen_sc16_clipped(gsdr_txgen *g) {
    if (!g || !g->d_clipped) {
        create_error() = "gsdr_txgen_sc16_clipped: null handle";
        return -1;
    }
    unsigned long long c = 0;
    hipError_t e = g->device >= 0 ? hipSetDevice(g->device) : hipSuccess;
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&c, g->d_clipped, sizeof(c), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        create_error() = std::string("gsdr_txgen_sc16_clipped: ") + hipGetErrorString(e);
        return -1;
    }
    return (long long)c;
}

}  // extern "C"
