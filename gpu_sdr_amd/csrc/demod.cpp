// demod.cpp -- C ABI of libgsdr.so (include/gsdr.h): handle lifecycle, mode
// dispatch and per-buffer sequencing of the RX demodulator.  The handle's state is laid out in demod_state.h; each
// mode's setup, enqueue and carry state is in its own file (demod_ddc.cpp, demod_pfb.cpp, demod_chirp.cpp), the
// pipelined entries in demod_pipeline.cpp.
//
// Host-side counterpart of RX_buffer_demodulator
// (ref: cpp/USRP_demodulator.cpp, headers/USRP_demodulator.hpp).  All device
// work is enqueued on one stream per demodulator, like the reference's
// internal_stream (ref: USRP_demodulator.cpp:44), but nothing here blocks
// except the host-pointer entry gsdr_demod_process().
//
// "ref:" citations are relative to /root/reference.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include <unistd.h>

#include "demod_state.h"

extern char **environ;

using gsdr::create_error;
using gsdr::device_cus;

std::string &gsdr::create_error() {
    thread_local std::string msg;
    return msg;
}

// The one reader of the environment ("Run-time knobs"): a variable that is unset or empty keeps the
// default; values out of range are mapped as noted in gsdr::Switches.
gsdr::Switches gsdr::read_switches() {
    auto is_set = [](const char *name) {
        const char *v = std::getenv(name);
        return v && *v ? v : nullptr;
    };
    auto env = [&](const char *name, int unset) {
        const char *v = is_set(name);
        return v ? std::atoi(v) : unset;
    };
    Switches s;
    s.ddc_mfma = env("GSDR_DDC_MFMA", 1) != 0;
    s.ddc_few = env("GSDR_DDC_FEW", 1) != 0;
    s.ddc_pipe = env("GSDR_DDC_PIPE", 1) != 0;
    s.ddc_k = env("GSDR_DDC_K", -1);
    s.ddc_waves = env("GSDR_DDC_WAVES_PER_SIMD", 0);
    if (s.ddc_waves <= 0 && is_set("GSDR_DDC_WAVES_PER_SIMD")) s.ddc_waves = 4;
    s.ddc_nch = env("GSDR_DDC_NCH", 0);
    s.ddc_lds = (unsigned)env("GSDR_DDC_LDS", 0);
    s.ddc_prefetch = env("GSDR_DDC_PREFETCH", 1);
    s.ddc_autotune = env("GSDR_DDC_AUTOTUNE", 1) != 0;
    s.mfma_asm = env("GSDR_MFMA_ASM", 4);
    s.mfma_tt = env("GSDR_MFMA_TT", 1) == 2 ? 2 : 1;
    s.mfma_pk = env("GSDR_MFMA_PK", 32) == 16 ? 16 : 32;
    s.mfma_w = env("GSDR_MFMA_W", 4) == 2 ? 2 : 4;
    s.mfma_rt = env("GSDR_MFMA_RT", 0);
    if (s.mfma_rt < 0 || s.mfma_rt > 2) s.mfma_rt = 0;
    s.mfma_w8 = env("GSDR_MFMA_W8", 1) != 0;
    s.mfma_prec = env("GSDR_MFMA_PREC", -1);
    s.mfma_3m = env("GSDR_MFMA_3M", -1);
    s.mfma_3m_rot = env("GSDR_MFMA_3M_ROT", -1);
    s.mfma_fold = env("GSDR_MFMA_FOLD", -1);
    s.mfma_fold_products = env("GSDR_MFMA_FOLD_PRODUCTS", -1);
    s.mfma_wave_tones = env("GSDR_MFMA_WAVE_TONES", -1);
    s.mfma_span = env("GSDR_MFMA_SPAN", -1);
    s.mfma_timing = env("GSDR_MFMA_TIMING", 0);
    s.noise_fft = env("GSDR_NOISE_FFT", 1) != 0;
    s.tones_fft = env("GSDR_TONES_FFT", 1) != 0;
    s.pfb_lds = env("GSDR_PFB_LDS", 1) != 0;
    s.pfb_bluestein = is_set("GSDR_PFB_BLUESTEIN") ? env("GSDR_PFB_BLUESTEIN", 0) != 0 : -1;
    s.pfb_cu = env("GSDR_PFB_CU", -1);
    s.pfb_direct = env("GSDR_PFB_DIRECT", 1) != 0;
    s.pfb_col = env("GSDR_PFB_COL", -1);
    if (s.pfb_col > 0) s.pfb_col = 1;
    s.pfb_cu_nt = env("GSDR_PFB_CU_NT", 0);
    s.pfb_teams = env("GSDR_PFB_TEAMS", 1) != 0;
    s.pfb_radix8 = env("GSDR_PFB_RADIX8", 1) != 0;
    s.pfb_fr = env("GSDR_PFB_FR", 0);
    s.pfb_wide = env("GSDR_PFB_WIDE", -1);
    s.mix_few = env("GSDR_MIX_FEW", 32);
    s.chirp_split = env("GSDR_CHIRP_SPLIT", 1) != 0;
    s.pipe_queues = env("GSDR_PIPE_QUEUES", 1) != 0;
    s.pipe_overlap = env("GSDR_PIPE_OVERLAP", 1) != 0;
    s.pipe_streams = env("GSDR_PIPE_STREAMS", gsdr::rx::kPipeStreams);
    if (s.pipe_streams < 1 || s.pipe_streams > gsdr::rx::kPipeStreams) s.pipe_streams = gsdr::rx::kPipeStreams;
    return s;
}

namespace gsdr {
namespace rx {

namespace {

constexpr int kMaxEvents = 8192;   // profiling ring

int fail_create(gsdr_demod *h, const std::string &msg) {
    create_error() = msg;
    if (h) gsdr_demod_close(h);
    return -1;
}

}  // namespace

int refuse(gsdr_demod *h, const char *msg) {
    h->err = msg;
    return -1;
}

int refuse_null(gsdr_demod *h, const void *in, const void *out) {
    if (!h) return -1;
    if (!in || !out) {
        h->err = "null buffer";
        return -1;
    }
    return 0;
}

// Orders `st` behind every stream in h->dirty and forgets those; keep_pipeline: the compute streams of the pipeline
// stay (its protocol orders them, pipeline_compute).
int join_streams(gsdr_demod *h, hipStream_t st, bool keep_pipeline) {
    auto keep = [&](hipStream_t s) {
        for (int i = 0; keep_pipeline && i < kPipeStreams; ++i)
            if (s == h->pl.s_main[i]) return true;
        return false;
    };
    size_t w = 0;
    for (size_t i = 0; i < h->dirty.size(); ++i) {
        hipStream_t s = h->dirty[i];
        if (s == st || keep(s)) {
            h->dirty[w++] = s;
            continue;
        }
        if (!h->ev_join) HIPCHK(h, hipEventCreateWithFlags(h->ev_join.out(), hipEventDisableTiming));
        if (hipEventRecord(h->ev_join, s) != hipSuccess) {
            // nothing that could still be waited for: forget the stream rather than fail every later call
            (void)hipGetLastError();
            continue;
        }
        HIPCHK(h, hipStreamWaitEvent(st, h->ev_join, 0));
    }
    h->dirty.resize(w);
    bool have = false;
    for (hipStream_t s : h->dirty) have |= (s == st);
    if (!have) h->dirty.push_back(st);
    return 0;
}

int record_begin(gsdr_demod *h, hipStream_t st, hipEvent_t *stop) {
    *stop = nullptr;
    if (!h->prof.on || h->prof.ev_used >= (size_t)kMaxEvents) return 0;
    if (h->prof.seen++ % (unsigned long long)h->prof.every != 0) return 0;
    if (h->prof.ev_used == h->prof.ev_pool.size()) {
        gsdr::Event a, b;
        HIPCHK(h, hipEventCreate(a.out()));
        HIPCHK(h, hipEventCreate(b.out()));
        h->prof.ev_pool.emplace_back(std::move(a), std::move(b));
    }
    HIPCHK(h, hipEventRecord(h->prof.ev_pool[h->prof.ev_used].first, st));
    *stop = h->prof.ev_pool[h->prof.ev_used].second;
    h->prof.ev_used++;
    return 0;
}

// gsdr_demod_create with the switches given (gsdr_demod_prepare's rehearsal twin takes its parent's) and the
// GSDR_CREATE_* flags of gsdr_demod_create_ex
gsdr_demod *demod_create(const gsdr_param_c *p, const gsdr::Switches &sw, unsigned flags) {
    create_error().clear();
    if (flags & ~GSDR_CREATE_MULTI_CHIRP) {
        create_error() = "unknown creation flag";
        return nullptr;
    }
    if (!p) {
        create_error() = "null parameters";
        return nullptr;
    }
    gsdr_demod *h = new gsdr_demod();
    h->sw = sw;
    h->flags = flags;
    {
        h->pc = *p;
        auto keep = [](auto &dst, const auto *src, int n) {
            dst.assign(src && n > 0 ? src : nullptr, src && n > 0 ? src + n : nullptr);
            return dst.empty() ? nullptr : dst.data();
        };
        h->pc.wave_type = keep(h->pc_wave_type, p->wave_type, p->n_wave_type);
        h->pc.freq = keep(h->pc_freq, p->freq, p->n_freq);
        h->pc.chirp_f = keep(h->pc_chirp_f, p->chirp_f, p->n_chirp_f);
        h->pc.swipe_s = keep(h->pc_swipe_s, p->swipe_s, p->n_swipe_s);
        h->pc.chirp_t = keep(h->pc_chirp_t, p->chirp_t, p->n_chirp_t);
    }

    // ---- mode selection, ref: USRP_demodulator.cpp:15-39 ----
    int last = GSDR_NODSP;
    if (p->n_wave_type > 0 && p->wave_type) last = p->wave_type[0];
    bool mixed = false;
    int chirps = 0;
    for (int i = 0; i < p->n_wave_type; ++i) {
        if (p->wave_type[i] != last) mixed = true;
        if (p->wave_type[i] == GSDR_CHIRP) chirps++;
    }
    const bool multi = (flags & GSDR_CREATE_MULTI_CHIRP) != 0;
    if (chirps > 1 && !multi) {
        fail_create(h, "Multiple chirp RX buffer demodulation has been requested. This feature is not implemented yet.");
        return nullptr;
    }
    if (mixed) {
        fail_create(h, "Mixed RX buffer demodulation has been requested. This feature is not implemented yet.");
        return nullptr;
    }
    h->mode = last;
    h->N = p->n_wave_type;
    h->L = p->buffer_len;
    h->decim = p->decim;
    if (h->L <= 0) {
        fail_create(h, "buffer_len must be positive");
        return nullptr;
    }
    if (last == GSDR_CHIRP && chirps > 1) {      // (one chirp with the flag is the plain single-chirp handle)
        if (const char *bad = gsdr::multi_chirp_fault(p, chirps)) {
            fail_create(h, bad);
            return nullptr;
        }
        h->ch.chirps = chirps;
    }

    {
        h->device = p->device_index;
        if (h->device >= 0 && hipSetDevice(h->device) != hipSuccess) {
            fail_create(h, "hipSetDevice failed (no such GPU?)");
            return nullptr;
        }
        h->cus = device_cus();
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        // ref: :41-44 low priority stream for tone modes, :186-189 high for chirp
        // (into a local first: the owner takes the stream only when the call has succeeded, whatever a failed one wrote)
        hipStream_t s = nullptr;
        hipError_t e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, last == GSDR_CHIRP ? hi : lo);
        if (e != hipSuccess) {
            fail_create(h, std::string("cannot create a HIP stream: ") + hipGetErrorString(e));
            return nullptr;
        }
        *h->stream.out() = s;
    }

    int rc = 0;
    switch (last) {
        case GSDR_DIRECT: rc = setup_direct(h, p); break;
        case GSDR_TONES:
        case GSDR_NOISE: rc = setup_pfb(h, p); break;
        case GSDR_CHIRP: rc = setup_chirp(h, p); break;
        case GSDR_NODSP:  // ref: :315-321
            h->capacity = h->L;
            h->kernel_name = "memcpy";
            break;
        default:  // ref: :322-325
            fail_create(h, "Void demodulation operation has not been implemented yet!");
            return nullptr;
    }
    if (rc) {
        fail_create(h, h->err.empty() ? "device setup failed" : h->err);
        return nullptr;
    }
    // hipMemset returns before the fill has run (it is asynchronous on the null stream), and the streams
    // of this library do not wait for the null stream: without this the zeroing of a carry buffer could
    // land after the first call had written the carry (seen with several handles created and used from
    // several threads, scratch/concurrent_handles.py: the second buffer of a TONES handle came out wrong)
    if (hipStreamSynchronize(nullptr) != hipSuccess) {
        fail_create(h, "device setup did not complete");
        return nullptr;
    }
    return h;
}

// The body of gsdr_demod_process_device and of its sc16 twin.  in16 != nullptr: the samples arrive as sc16 and are
// widened into `wide` first (NODSP: straight into out) -- BEHIND the join below, because `wide` belongs to the handle:
// enqueued in front of it, the widening of this call could overwrite the buffer while the predecessor call, on another
// stream, still reads it.
int process_device_body(gsdr_demod *h, const float2 *in, const gsdr_sc16 *in16, float2 *wide, float2 *out, hipStream_t st) {
    // An in-order call is a join point: it runs behind everything this handle has in flight on
    // other streams (an earlier call on another stream, overlapped calls still running).  Free on
    // the usual path (same stream as the call before).  Overlapped calls order themselves among
    // their compute streams (pipeline_compute) and only join the in-order streams.
    if (!h->pl.overlap) {
        if (join_streams(h, st, /*keep_pipeline=*/false)) return -1;
    }
    if (in16) {
        if (h->mode == GSDR_NODSP) wide = out;
        HIPCHK(h, gsdr::launch_widen_sc16(in16, wide, h->L, h->sc16_scale, h->cus, st));
        if (h->mode == GSDR_NODSP) return (int)h->L;
        in = wide;
    }
    int n;
    switch (h->mode) {
        case GSDR_DIRECT: n = enqueue_direct(h, in, out, st); break;
        case GSDR_TONES:
        case GSDR_NOISE: n = h->pfb.avg_k > 1 ? enqueue_pfb_average(h, in, out, st) : enqueue_pfb(h, in, out, st); break;
        case GSDR_CHIRP: n = enqueue_chirp(h, in, out, st); break;
        case GSDR_NODSP:  // ref: process_nodsp :335-339
            HIPCHK(h, hipMemcpyAsync(out, in, (size_t)h->L * sizeof(float2),
                                     hipMemcpyDeviceToDevice, st));
            return (int)h->L;     // no state passes from call to call
        default: h->err = "unsupported mode"; return -1;
    }
    return n;
}

// The staging buffers of the host-pointer entry are made as a pair: both set or both empty.  (Were d_in kept when d_out
// cannot be had, the next call would skip the allocation and hand a null d_out to the kernels.)
int staging_pair(gsdr_demod *h) {
    if (h->host.d_in) return 0;
    hipError_t e = h->host.d_in.alloc((size_t)h->L);
    if (e == hipSuccess) e = h->host.d_out.alloc((size_t)h->capacity);
    if (e == hipSuccess) return 0;
    h->host.d_in.reset(), h->host.d_out.reset();
    h->err = std::string("staging allocation of the host entry: ") + hipGetErrorString(e);
    return -1;
}

}  // namespace rx
}  // namespace gsdr

using namespace gsdr::rx;

extern "C" {

const char *gsdr_last_error(const gsdr_demod *h) {
    return h ? h->err.c_str() : create_error().c_str();
}

gsdr_demod *gsdr_demod_create(const gsdr_param_c *p) { return demod_create(p, gsdr::read_switches(), 0u); }

gsdr_demod *gsdr_demod_create_ex(const gsdr_param_c *p, unsigned flags) { return demod_create(p, gsdr::read_switches(), flags); }

// gsdr_demod_process_device and gsdr_demod_process_device_sc16 (in16_dev != nullptr)
static int process_device(gsdr_demod *h, const gsdr_c64 *in_dev, const gsdr_sc16 *in16_dev, gsdr_c64 *out_dev,
                          void *hip_stream) {
    if (refuse_null(h, in16_dev ? (const void *)in16_dev : in_dev, out_dev)) return -1;
    if (h->device >= 0) HIPCHK(h, hipSetDevice(h->device));
    if (in16_dev && h->mode != GSDR_NODSP && !h->d_wide) HIPCHK(h, h->d_wide.alloc((size_t)h->L));
    // NULL is HIP's null stream, as everywhere in HIP
    return process_device_body(h, reinterpret_cast<const float2 *>(in_dev), in16_dev, in16_dev ? h->d_wide : nullptr,
                               reinterpret_cast<float2 *>(out_dev), (hipStream_t)hip_stream);
}

int gsdr_demod_process_device(gsdr_demod *h, const gsdr_c64 *in_dev, gsdr_c64 *out_dev, void *hip_stream) {
    return process_device(h, in_dev, nullptr, out_dev, hip_stream);
}

int gsdr_demod_process_device_sc16(gsdr_demod *h, const gsdr_sc16 *in_dev, gsdr_c64 *out_dev, void *hip_stream) {
    return process_device(h, nullptr, in_dev, out_dev, hip_stream);
}

// gsdr_demod_process and gsdr_demod_process_sc16 (in16_host != nullptr)
static int process_host(gsdr_demod *h, const gsdr_c64 *in_host, const gsdr_sc16 *in16_host, gsdr_c64 *out_host) {
    if (refuse_null(h, in16_host ? (const void *)in16_host : in_host, out_host)) return -1;
    if (h->mode == GSDR_NODSP) {  // ref: :335-339, a host memcpy; sc16 samples are widened on the host instead
        if (in16_host) gsdr_widen_sc16_host(in16_host, out_host, h->L, h->sc16_scale);
        else std::memcpy(out_host, in_host, (size_t)h->L * sizeof(gsdr_c64));
        return (int)h->L;
    }
    if (h->device >= 0) HIPCHK(h, hipSetDevice(h->device));
    if (staging_pair(h)) return -1;
    if (in16_host) {
        // half the bytes over the host link; widened into the staging buffer of the complex64 entry
        if (!h->host.d_in16) HIPCHK(h, h->host.d_in16.alloc((size_t)h->L));
        HIPCHK(h, hipMemcpyAsync(h->host.d_in16, in16_host, (size_t)h->L * sizeof(gsdr_sc16), hipMemcpyHostToDevice, h->stream));
    } else {
        HIPCHK(h, hipMemcpyAsync(h->host.d_in, in_host, (size_t)h->L * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    }
    // complex64: the samples are in d_in; sc16: they are in d_in16 and the body widens them into d_in
    const int ret = in16_host ? process_device_body(h, nullptr, h->host.d_in16, h->host.d_in, h->host.d_out, h->stream)
                              : process_device_body(h, h->host.d_in, nullptr, nullptr, h->host.d_out, h->stream);
    if (ret < 0) return ret;
    if (ret > 0)
        HIPCHK(h, hipMemcpyAsync(out_host, h->host.d_out, (size_t)ret * sizeof(float2),
                                 hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // ref: :393,:462,:555
    return ret;
}

int gsdr_demod_process(gsdr_demod *h, const gsdr_c64 *in_host, gsdr_c64 *out_host) {
    return process_host(h, in_host, nullptr, out_host);
}

int gsdr_demod_process_sc16(gsdr_demod *h, const gsdr_sc16 *in_host, gsdr_c64 *out_host) {
    return process_host(h, nullptr, in_host, out_host);
}

// Nothing may be released while a stream of the handle can still run a kernel that reads it: wait for them, then delete
void gsdr_demod_close(gsdr_demod *h) {
    if (!h) return;
    if (h->device >= 0) (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (int i = 0; i < kPipeStreams; ++i)
        if (h->pl.s_main[i]) (void)hipStreamSynchronize(h->pl.s_main[i]);
    if (h->pl.s_up) (void)hipStreamSynchronize(h->pl.s_up);
    if (h->pl.s_down) (void)hipStreamSynchronize(h->pl.s_down);
    delete h;
}

int gsdr_demod_set_sc16_scale(gsdr_demod *h, float scale) {
    if (!h) return -1;
    if (!std::isfinite(scale) || !(scale > 0.f)) {
        h->err = "sc16 scale must be finite and > 0";
        return -1;
    }
    h->sc16_scale = scale;
    return 0;
}

float gsdr_demod_sc16_scale(const gsdr_demod *h) { return h ? h->sc16_scale : 0.f; }

// gsdr_frame_average_host (host_logic.cpp) leaves its message here
void gsdr_note_error_(const char *msg) { create_error() = msg ? msg : ""; }

int gsdr_widen_sc16_device(const gsdr_sc16 *in_dev, gsdr_c64 *out_dev, long long n, float scale, void *hip_stream) {
    if (n < 0 || (n > 0 && (!in_dev || !out_dev))) {
        create_error() = "gsdr_widen_sc16_device: null buffer";
        return -1;
    }
    const hipError_t e = gsdr::launch_widen_sc16(in_dev, reinterpret_cast<float2 *>(out_dev), n, scale, device_cus(),
                                                 (hipStream_t)hip_stream);
    if (e != hipSuccess) {
        create_error() = std::string("gsdr_widen_sc16_device: ") + hipGetErrorString(e);
        return -1;
    }
    return 0;
}

int gsdr_pfb_lds_stages(int fft_tones, int *radices) {
    int tmp[16];
    const int n = gsdr::pfb_lds_plan(fft_tones, tmp, gsdr::read_switches().pfb_radix8);
    if (radices)
        for (int i = 0; i < n && i < 16; ++i) radices[i] = tmp[i];
    return n;
}

int gsdr_demod_mode(const gsdr_demod *h) { return h ? h->mode : -1; }

int gsdr_demod_channels(const gsdr_demod *h) { return h ? h->N : 0; }

long long gsdr_demod_out_capacity(const gsdr_demod *h) { return h ? h->capacity : 0; }

float gsdr_demod_fcut(const gsdr_demod *h) { return h ? h->fcut : 0.f; }

void gsdr_demod_profile_enable(gsdr_demod *h, int enable) {
    if (!h) return;
    h->prof.on = enable != 0;
    h->prof.every = enable > 1 ? enable : 1;
    h->prof.seen = 0;
    h->prof.ev_used = 0;
}

int gsdr_demod_profile_read(gsdr_demod *h, double *total_ms) {
    if (total_ms) *total_ms = 0.0;
    if (!h || h->prof.ev_used == 0) return 0;
    if (h->device >= 0) (void)hipSetDevice(h->device);
    double sum = 0.0;
    int n = 0;
    for (size_t i = 0; i < h->prof.ev_used; ++i) {
        if (hipEventSynchronize(h->prof.ev_pool[i].second) != hipSuccess) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->prof.ev_pool[i].first, h->prof.ev_pool[i].second) == hipSuccess) {
            sum += ms;
            n++;
        }
    }
    if (total_ms) *total_ms = sum;
    return n;
}

const char *gsdr_demod_kernel_name(const gsdr_demod *h) { return h ? h->kernel_name : "none"; }

void gsdr_reload_env(void) {}   // kept for callers built against older headers: a handle reads the switches once

const char *gsdr_build_info(void) {
#ifdef GSDR_TIMING_BUILD
    return "abi 1; arch gfx950; timing_build 1";
#else
    return "abi 1; arch gfx950; timing_build 0";
#endif
}

int gsdr_demod_describe(const gsdr_demod *h, char *buf, int cap) {
    if (!h || !buf || cap < 1) return 0;
    static const char *modes[] = {"TONES", "CHIRP", "NOISE", "RAMP", "NODSP", "SWONLY", "DIRECT"};
    std::string s = "{\"mode\": \"";
    s += (h->mode >= 0 && h->mode <= 6) ? modes[h->mode] : "?";
    s += "\", \"kernel\": \"";
    s += h->kernel_name;
    s += "\", \"family\": \"";
    s += h->pfb.lds ? (h->pfb.blue ? "polyphase filter + Bluestein (two fp32 Stockham FFTs) inside the LDS + bin selection, one launch"
                                   : "polyphase filter + fp32 Stockham FFT inside the LDS + bin selection, one launch") :
         h->pfb.noise_fft ? "fp32 Stockham FFT behind the polyphase filter" : h->mx.on ? "f16 MFMA, hi/lo split" : (h->mode == GSDR_CHIRP ? "fp32 VALU, integer phase" : (h->ddc.flat ? "packed fp32 VALU" : "fp32 VALU"));
    s += "\", \"channels\": " + std::to_string(h->ddc.channels > 0 ? h->ddc.channels : h->N);
    // each mode's part (appended only by a handle of that mode), then what every handle reports
    if (h->mode == GSDR_CHIRP) describe_chirp(h, s);
    if (h->pfb.lds) describe_pfb_lds(h, s);
    describe_mfma(h, s);
    s += ", \"pipeline_streams\": " + std::to_string(h->sw.pipe_streams);
    describe_frame_average(h, s);
    s += ", \"timing_build\": ";
#ifdef GSDR_TIMING_BUILD
    s += "1";
#else
    s += "0";
#endif
    s += ", \"env\": {";
    bool first = true;
    for (char **e = environ; e && *e; ++e) {
        if (std::strncmp(*e, "GSDR_", 5) != 0) continue;
        const char *eq = std::strchr(*e, '=');
        if (!eq) continue;
        std::string k(*e, eq - *e), v(eq + 1);
        for (auto &c : v)
            if (c == '"' || c == '\\' || (unsigned char)c < 0x20) c = '?';
        s += (first ? "\"" : ", \"") + k + "\": \"" + v + "\"";
        first = false;
    }
    s += "}}";
    const int n = (int)s.size() < cap - 1 ? (int)s.size() : cap - 1;
    std::memcpy(buf, s.data(), (size_t)n);
    buf[n] = 0;
    return n;
}

}  // extern "C"
