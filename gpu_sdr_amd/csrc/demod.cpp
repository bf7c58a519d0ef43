// demod.cpp -- C ABI of libgsdr.so (include/gsdr.h): handle lifecycle, mode
// dispatch, per-buffer sequencing and carry state of the RX demodulator.
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

#include "host_util.h"

extern char **environ;

using gsdr::ChirpShape;
using gsdr::chirp_shape;
using gsdr::create_error;
using gsdr::DdcLaunch;
using gsdr::DdcShape;
using gsdr::device_cus;
using gsdr::mod_rate;
using gsdr::phasor;

std::string &gsdr::create_error() {
    thread_local std::string msg;
    return msg;
}

namespace {

constexpr int kMaxF = 8;           // tap phases the DDC kernel is instantiated for
constexpr int kMaxEvents = 8192;   // profiling ring
// Pipelined entries: compute streams that consecutive DIRECT calls go to in turn, and the
// sets of staging buffers / scale slots that keeps the calls in flight apart (pipeline_compute)
constexpr int kPipeStreams = 3;
constexpr int kChirpPartials = 16384;    // float2 slots for the partial sums of split chirp points (chirp_lockin_split_kernel)
constexpr int kStageSets = kPipeStreams + 1;
constexpr int kScaleSlots = kPipeStreams + 2;

}  // namespace

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
    s.pipe_streams = env("GSDR_PIPE_STREAMS", kPipeStreams);
    if (s.pipe_streams < 1 || s.pipe_streams > kPipeStreams) s.pipe_streams = kPipeStreams;
    return s;
}

struct gsdr_demod {
    gsdr::Switches sw;      // the GSDR_* switches, read when the handle was created
    int mode = GSDR_NODSP;
    int device = -1;
    std::string err;
    // Every d_* buffer, stream and event below is an owner (dev_owner.h) and is released by `delete`.  gsdr_demod_close
    // synchronises the streams first -- the one ordering that matters -- so the order among the releases is not
    // observable; the streams are declared in front of everything else all the same, so that the buffers and events go
    // before them and `stream` goes last.  (The caller's streams in `dirty` are not the handle's and stay raw.)
    gsdr::Stream stream;
    gsdr::Stream s_up, s_down;                  // pipelined host-pointer entry: upload and download
    // pipelined entries (gsdr_demod_submit*): consecutive DIRECT calls go to these compute streams in turn, so that
    // their kernels overlap (see pipeline_compute)
    gsdr::Stream s_main[kPipeStreams];

    int N = 0;              // channels = wave_type.size()
    int ddc_channels = 0;   // tones the DDC kernels run (== N except NOISE: fft_tones)
    long long L = 0;        // buffer_len
    long long decim = 0;
    long long capacity = 0; // max samples process() can return
    float fcut = 0.f;

    // host-pointer entry staging
    gsdr::DevBuf<float2> d_in, d_out;           // allocated together: both set or both empty (staging_pair)
    // sc16 input (gsdr_demod_*_sc16): the scale of the widening; the half-size upload buffer of the host-pointer
    // entry (widened into d_in); the buffer gsdr_demod_process_device_sc16 widens the caller's samples into
    float sc16_scale = 1.0f / 32768.0f;
    gsdr::DevBuf<gsdr_sc16> d_in16;
    gsdr::DevBuf<float2> d_wide;
    int cus = 256;                     // compute units of the device (grid of the widening kernel)
    // pipelined host-pointer entry (gsdr_demod_submit / _wait)
    struct Slot {
        gsdr::DevBuf<float2> d_in, d_out;
        gsdr::DevBuf<gsdr_sc16> d_in16;    // gsdr_demod_submit_sc16: upload target, widened into d_in
        gsdr::Event up, done, down;
        hipEvent_t wait_ev = nullptr;      // what gsdr_demod_wait() waits for: down (host) / done (device); not owned
        int n = 0;
    } slot[GSDR_PIPELINE_DEPTH];
    bool pipe_ready = false;             // pipeline_init() succeeded
    int pipe_head = 0, pipe_count = 0;   // oldest outstanding slot, number outstanding

    // ---- DDC (DIRECT / TONES) ----
    int F = 0, K = 16, M = 0, Npad = 0, TW = 0, R = 0;
    unsigned nco_rate = 1;
    unsigned long long idx = 0;        // DIRECT_current_index (ref :88, :437-440)
    int target_waves = 4096;           // resident waves the DDC grid is sized for
    int simds = 1024;                  // SIMDs of the device (4 per CU)
    int nch_max = 1;                   // chunks of the DIRECT launch (fixed nblk)
    int tails_nch = 0;                 // chunk count the tails buffer was sized for (0: not yet)
    double waves_ratio = 1.3;          // grid waves / resident waves (autotuned in create)
    std::vector<float> window;         // taps (DIRECT) / PFB window / VNA profile, real part
    gsdr::DevBuf<float> d_taps_t;
    gsdr::DevBuf<float> d_taps_p;      // zero-padded [nsub*K+2][FP] copy for ddc_flat_kernel
    bool pipe = false;                 // ddc_flat_kernel (F <= 4) instead of ddc_kernel
    int pad = 0;                       // samples the flat kernel reads past a block (nsub*K - M)
    gsdr::DevBuf<float2> d_stage;      // padded copy of the input when pad > 0 (DIRECT only)
    gsdr::DevBuf<float2> d_btab;
    gsdr::DevBuf<double2> d_wk, d_wrem;
    gsdr::DevBuf<unsigned> d_fmod;
    gsdr::DevBuf<float2> d_tails;
    gsdr::DevBuf<float2> d_carry[2];
    int parity = 0;
    // ---- DDC on the matrix cores (ddc_mfma.hip) ----
    bool mfma = false;
    bool few = false;                  // DIRECT: a handful of tones at a long decimation run ddc_few_kernel (a wave per chunk and tone)
    int mf_TT = 1, mf_PK = 32, mf_W = 4;   // tone tiles per wave, phasor block, waves per workgroup
    gsdr::MfmaKernel mf_kind = gsdr::MfmaKernel::AsmRing;
    gsdr::MfmaShape mf{};              // fields that do not change between calls
    int last_rt = 0;                   // row tiles per workgroup of the last launch (describe())
    // pre-converted operands (ddc_convert_kernel + ddc_mfma_ring16p_kernel) for launches of many
    // rounds: one image set per staging set (the main kernels of the calls in flight read theirs)
    bool prec = false;                 // image sets allocated: the path may be chosen
    gsdr::DevBuf<uint4> d_img[kStageSets];
    // the product loop of a handle with three real products per complex multiply (DESIGN.md sections 4.1d - 4.1h; a row
    // of gsdr::product_loop): decided once, in setup_mfma (product_loop_chosen); such a handle sends EVERY matrix-core
    // launch through that row's kernel pair.  Null: four products per block, the loop chosen per launch (enqueue_mfma)
    const gsdr::ProductLoop *loop = nullptr;
    gsdr::DevBuf<uint4> d_bfrag3;
    gsdr::DevBuf<float4> d_ptab3;
    gsdr::DevBuf<uint4> d_bfrag;
    gsdr::DevBuf<float2> d_ptab, d_dtab;
    gsdr::DevBuf<float> d_mtaps;
    gsdr::DevBuf<unsigned> d_mfmod;
    // kScaleSlots tables of segment maxima (absmax_kernel), one per call in turn; seg_k blocks of M samples per segment
    gsdr::DevBuf<unsigned> d_segmax;
    int seg_k = 1, nseg_alloc = 0;
    // [carry | first rows' samples | zeros] and [last rows' samples | zeros], see absmax_kernel.
    // kStageSets of each, used in turn: the staging pass of call j writes set j (and the carry
    // part of head j+1) while the main kernels of calls j-1 .. j-kPipeStreams+1 may still read theirs.
    gsdr::DevBuf<float2> d_head[kStageSets];
    gsdr::DevBuf<float2> d_tail[kStageSets];
    gsdr::Event ev_abs[4];             // pipelined entries: staging pass of call j done
    // Streams that carry work of this handle nobody has been ordered behind yet.  The carry, the
    // scale slots, the raw windows and the head/tail copies pass from one call to the next ON THE
    // DEVICE: a call that runs on another stream than its predecessors first joins them (an event
    // recorded on the old stream at that moment covers everything enqueued there before).
    // A stream of the CALLER's stays in this list only until the next call on the handle (which joins it and
    // forgets it): include/gsdr.h asks the caller to keep a stream alive that long.  (An event of the handle's own
    // recorded behind every call would lift that condition, and was tried: an event record costs 3 - 4 us of stream
    // time, which doubled the step period of the chirp path -- 5.1 -> 9.2 us -- and showed in every in-order figure.)
    // If recording on a remembered stream returns an error, the entry is dropped and the call goes on.  (A stream
    // destroyed before that is beyond help: HIP faults inside hipEventRecord, tests/test_gpu_parity.py.)
    std::vector<hipStream_t> dirty;
    gsdr::Event ev_join;
    bool pipe_overlap = false;         // set around the compute of an overlapped call
    unsigned long long pipe_seq = 0;   // overlapped calls so far
    unsigned long long call_no = 0;    // absmax slot rotation
    // ---- TONES ----
    std::vector<int> bins;
    int nfft = 0, batching = 0;
    gsdr_buffer_helper bh{};
    // raw_input (ref :143): kStageSets windows used in turn.  The staging of call j copies the
    // unconsumed end of window j-1 to the front of window j and appends the new buffer, so the
    // kernels of call j-1 may still read their window (the reference moves it in place, :504-509).
    gsdr::DevBuf<float2> d_win[kStageSets];
    unsigned long long win_seq = 0;    // TONES/NOISE calls so far
    long long prev_spare_begin = 0, prev_spare_samples = 0;
    // ---- NOISE through the FFT stage (fft_kernels.hip) ----
    bool noise_fft = false;
    gsdr::FftPlan fft{};
    gsdr::DevBuf<float2> d_fft_a, d_fft_b;           // frames / scratch, batching * max(nfft, m) each
    gsdr::DevBuf<float2> d_fft_c;                    // TONES through these stages: the spectra the bins are picked from
    gsdr::DevBuf<float> d_fft_win;                   // the PFB window on the device
    // ---- the parameters this handle was created with (gsdr_demod_prepare's rehearsal builds a twin) ----
    gsdr_param_c pc{};
    unsigned flags = 0;                              // GSDR_CREATE_* of gsdr_demod_create_ex (the twin takes the same)
    std::vector<int> pc_wave_type, pc_freq, pc_chirp_f, pc_swipe_s;
    std::vector<float> pc_chirp_t;
    // ---- TONES / NOISE, a frame per workgroup: filter + in-LDS transform + bin selection (fft_kernels.hip) ----
    bool pfb_lds = false;
    bool pfb_blue = false;                           // ... through Bluestein's identity (h->fft holds chirp, transform, twiddles)
    gsdr::DevBuf<float2> d_pfb_tw;                   // w_nfft^k
    gsdr::DevBuf<int> d_pfb_sel;                     // TONES: bin of every output column
    gsdr::DevBuf<float2> d_pfb_carry[kStageSets];    // the samples a call leaves over (at most F*nfft)
    // what launch_pfb_lds chose call by call (gsdr_demod_describe: pfb_last, pfb_calls)
    gsdr::PfbChoice pfb_last{};
    int pfb_last_frames = -1;                        // frames of the last call; -1: no call yet
    unsigned long long pfb_calls_cu = 0, pfb_calls_lds = 0, pfb_calls_direct[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long pfb_calls_teams = 0, pfb_calls_runs = 0, pfb_calls_short = 0;   // with teams, G >= 2, a short last run
    // ---- TONES / NOISE, mean of avg_k consecutive frames (gsdr_demod_set_frame_average; 1: off, nothing below is used) ----
    int avg_k = 1, avg_kind = GSDR_AVERAGE_COMPLEX;
    int avg_count = 0;                               // frames of the open group, summed in d_avg_acc[avg_seq % 2]
    unsigned long long avg_seq = 0;                  // launches of pfb_average_kernel so far: they read one accumulator, write the other
    gsdr::DevBuf<float2> d_avg_frames;               // [batching][ddc_channels]: where the PFB writes its frames instead of `out`
    gsdr::DevBuf<float2> d_avg_acc[2];               // [ddc_channels] each
    // ---- CHIRP ----
    ChirpShape cs{};                   // (several chirps: chirp 0; num_steps, length and the period are common to all)
    int chirps = 1;                    // > 1: a GSDR_CREATE_MULTI_CHIRP handle; mc holds f0 and chirpness of every chirp
    gsdr::MultiChirp mc{};
    int ppt = 0;
    gsdr_vna_helper vh{};
    gsdr::DevBuf<float> d_profile;
    gsdr::DevBuf<float2> d_chirp_part; // partial sums of chirp_lockin_split_kernel (kChirpPartials float2)
    gsdr::DevBuf<float2> d_ccarry[2];
    int cparity = 0;
    int carry_len = 0;                 // spare_size (ref :54,:369)
    unsigned long long last_index = 0; // ref :217,:355
    unsigned long long chirp_calls[3] = {0, 0, 0};   // calls of this handle by the form that ran (gsdr::ChirpForm)
    long long chirp_parts = 1;         // waves per point of the last call (> 1: it was split)

    // ---- profiling ----
    bool prof = false;
    int prof_every = 1;                // time every n-th launch (an event pair costs ~3 us of stream time)
    unsigned long long prof_seen = 0;
    std::vector<std::pair<gsdr::Event, gsdr::Event>> ev_pool;
    size_t ev_used = 0;
    const char *kernel_name = "none";
};

namespace {

#define HIPCHK(h, expr)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                 \
            return -1;                                                                    \
        }                                                                                 \
    } while (0)

int fail_create(gsdr_demod *h, const std::string &msg) {
    create_error() = msg;
    if (h) gsdr_demod_close(h);
    return -1;
}

// Builds the per-tone NCO tables of the DDC kernel (see ddc_kernels.hip):
//   fmod[n] = f_n mod rate, btab[lo][n] = w_n^lo, wk[n] = w_n^K, wrem[n] = w_n^R.
int build_nco_tables(gsdr_demod *h, const std::vector<long long> &tone, unsigned rate) {
    const int Npad = h->Npad, K = h->K;
    std::vector<unsigned> fmod(Npad, 0u);
    std::vector<float2> btab((size_t)K * Npad);
    std::vector<double2> wk(Npad), wrem(Npad);
    for (int n = 0; n < Npad; ++n) {
        const unsigned long long fm = n < h->ddc_channels ? mod_rate(tone[n], rate) : 0u;
        fmod[n] = (unsigned)fm;
        for (int lo = 0; lo < K; ++lo) {
            double re, im;
            phasor((fm * (unsigned long long)lo) % rate, rate, re, im);
            btab[(size_t)lo * Npad + n] = make_float2((float)re, (float)im);
        }
        double re, im;
        phasor((fm * (unsigned long long)K) % rate, rate, re, im);
        wk[n] = make_double2(re, im);
        phasor((fm * (unsigned long long)h->R) % rate, rate, re, im);
        wrem[n] = make_double2(re, im);
    }
    HIPCHK(h, h->d_fmod.upload(fmod));
    HIPCHK(h, h->d_btab.upload(btab));
    HIPCHK(h, h->d_wk.upload(wk));
    HIPCHK(h, h->d_wrem.upload(wrem));
    return 0;
}

// taps_t[m*F + j] = h[j*M + m]: the F tap phases of input sample m, contiguous.
int upload_taps_transposed(gsdr_demod *h) {
    std::vector<float> t((size_t)h->M * h->F);
    for (int j = 0; j < h->F; ++j)
        for (int m = 0; m < h->M; ++m) t[(size_t)m * h->F + j] = h->window[(size_t)j * h->M + m];
    HIPCHK(h, h->d_taps_t.upload(t));
    if (h->pipe) {
        const int FP = h->F == 3 ? 4 : h->F;
        std::vector<float> p((size_t)(h->M + h->pad + 2) * FP, 0.f);
        for (int j = 0; j < h->F; ++j)
            for (int m = 0; m < h->M; ++m) p[(size_t)m * FP + j] = h->window[(size_t)j * h->M + m];
        HIPCHK(h, h->d_taps_p.upload(p));
    }
    return 0;
}

// Chunk count closest to `want` (within +-20 %) that splits nblk blocks most
// evenly: the launch ends with its longest chunk.
long long balanced_near(long long want, int nblk, long long cap) {
    if (want < 1) want = 1;
    if (want > cap) want = cap;
    long long lo = want - want / 5, hi = want + want / 5;
    if (lo < 1) lo = 1;
    if (hi > cap) hi = cap;
    long long best_nch = want;
    double best = -1.0;
    for (long long nch = lo; nch <= hi; ++nch) {
        const long long longest = (nblk + nch - 1) / nch;
        const double balance = ((double)nblk / (double)nch) / (double)longest;
        const double score = balance - 0.05 * std::fabs((double)(nch - want)) / (double)want;
        if (score > best) {
            best = score;
            best_nch = nch;
        }
    }
    return best_nch;
}

// Number of chunks the blocks of one launch are cut into (one wave per chunk x
// 64 tones).  `h->waves_ratio` = grid waves / resident waves; 1.3 by default
// (measured on C3: a grid 1.3x what is resident -- the dispatcher hands the
// surplus workgroups to whichever CU frees up first -- beats an exactly
// resident one by 9 %), replaced by the autotuned value when create() could
// time the candidates (profiles/r01_chunk_sweeps.log shows why a fixed rule is
// not enough: C2 is best at 0.8, C3 at 1.3-1.7).
int pick_chunks(const gsdr_demod *h, int nblk) {
    if (nblk <= 0) return 1;
    const int TW = h->TW > 0 ? h->TW : 1;
    const long long cap = (h->F > 1) ? nblk / (h->F - 1) : nblk;  // every chunk >= F-1 blocks
    if (cap < 1) return 1;
    long long nch = h->sw.ddc_nch > 0
                        ? (h->sw.ddc_nch < cap ? h->sw.ddc_nch : cap)
                        : balanced_near((long long)(h->waves_ratio * h->target_waves) / TW, nblk, cap);
    // never more chunks than the tails buffer has slots for (0 = not allocated yet)
    if (h->tails_nch > 0 && nch > h->tails_nch) nch = h->tails_nch;
    return (int)(nch < 1 ? 1 : nch);
}

int setup_ddc_common(gsdr_demod *h, int F, int M, unsigned rate,
                     const std::vector<long long> &tone, int max_nblk, bool allow_flat = true) {
    h->F = F;
    h->M = M;
    h->nco_rate = rate;
    if (h->ddc_channels <= 0) h->ddc_channels = h->N;
    h->Npad = ((h->ddc_channels + 63) / 64) * 64;
    h->TW = h->Npad / 64;
    // ddc_flat_kernel (packed math, pipelined scalar loads) covers F <= 4 and is the engine of
    // GSDR_DDC_MFMA=0, where no matrix-core loop runs on the GPU at all.  With the matrix cores enabled,
    // a shape they do not take (windows shorter than a buffer row, ...) goes to the generic ddc_kernel:
    // it is compiled without packed FP32, which is not safe beside the matrix-core loop of another
    // handle on the same GPU (rule 3).  GSDR_DDC_PIPE=0 forces the generic kernel.
    h->pipe = allow_flat && h->sw.ddc_pipe && F <= 4 && !h->sw.ddc_mfma;
    if (h->pipe) {
        // sub-block length: whole sub-blocks per block, cheapest total
        // (padded samples + ~3.3 sample-equivalents of fold work per sub-block).  40 since round 3: half the
        // folds and phasor steps of 20 at 124 instead of 82 registers (4 waves per SIMD instead of 5):
        // C3 460 -> 440 us in order (profiles/r03_flat_k.log)
        int forced = h->sw.ddc_k;
        if (forced != 12 && forced != 16 && forced != 20 && forced != 40) forced = 0;
        double best = 1e300;
        for (int k : {40, 20, 16, 12}) {
            if (forced && forced != k) continue;
            const long long nsub = (M + k - 1) / k;
            const double cost = (double)nsub * (k + 3.3);
            if (cost < best) {
                best = cost;
                h->K = k;
            }
        }
        const int nsub = (M + h->K - 1) / h->K;
        h->pad = nsub * h->K - M;
        h->R = M - (nsub - 1) * h->K;   // length of the last sub-block in real samples
    } else {
        h->K = h->sw.ddc_k == 32 ? 32 : 16;
        h->R = M % h->K;
    }
    // resident waves per SIMD of the kernel actually used (VGPR-limited)
    h->simds = device_cus() * 4;
    h->target_waves = h->simds * (h->sw.ddc_waves > 0 ? h->sw.ddc_waves : h->pipe ? 6 : 4);
    // the tails buffer must hold the largest chunk count any launch may pick:
    // largest autotune ratio (1.7) x the +20 % window of balanced_near(), or the
    // forced count, but never more than one chunk per F-1 blocks
    {
        const long long cap = (F > 1) ? max_nblk / (F - 1) : max_nblk;
        long long worst = (long long)(1.7 * 1.2 * h->target_waves) / h->TW + 2;
        if (h->sw.ddc_nch > worst) worst = h->sw.ddc_nch;
        if (worst > cap) worst = cap;
        h->tails_nch = (int)(worst < 1 ? 1 : worst);
    }
    h->waves_ratio = 1.3;
    h->nch_max = pick_chunks(h, max_nblk);
    if (build_nco_tables(h, tone, rate)) return -1;
    if (upload_taps_transposed(h)) return -1;
    const size_t tail_elems = (size_t)(h->tails_nch + 1) * (size_t)(F > 1 ? F - 1 : 1) * h->Npad;
    HIPCHK(h, h->d_tails.alloc_zeroed(tail_elems));
    return 0;
}

// the tables and launch switches of the handle that every DdcLaunch carries
void set_tables(const gsdr_demod *h, DdcLaunch &a) {
    a.taps_t = h->d_taps_t;
    a.taps_p = h->d_taps_p;
    a.btab = h->d_btab;
    a.wk = h->d_wk;
    a.wrem = h->d_wrem;
    a.fmod = h->d_fmod;
    a.lds_bytes = h->sw.ddc_lds;
    a.sh.prefetch = h->sw.ddc_prefetch;
}

// fields of DdcShape the kernels derive nothing from on the device
void finish_shape(DdcShape &sh) {
    sh.cbase = sh.nblk / (sh.nch > 0 ? sh.nch : 1);
    sh.crem = sh.nblk % (sh.nch > 0 ? sh.nch : 1);
    sh.rate_magic = 0xffffffffffffffffULL / sh.rate;
    sh.inv_rate = 1.0 / (double)sh.rate;
    sh.m_mod_rate = (unsigned)sh.M % sh.rate;
}

// Pre-converted operands (ddc_convert_kernel + ddc_mfma_ring16p_kernel) for a launch of
// ngt row tiles of the AsmRing16 kernel.  GSDR_MFMA_PREC: 1 = always (tests), 0 = never, default:
//   in-order entries      launches of four rounds of workgroups or more (-9 % at 16 k ... 64 k tones;
//                         below that the pass, which runs in front of the loop there, costs more);
//   overlapped entries    launches of half a round or more with windows of 32 blocks or more: the
//                         pass of buffer j+1 runs beside the loop of buffer j (C3 139 -> 130.5 us per
//                         buffer, TONES 1024/1230 76.8 -> 74.0; C2, 13 blocks: neutral, not used).
bool prec_pays(const gsdr_demod *h, long long ngt, bool overlap) {
    const long long wgs4 = ((ngt + 7) / 8) * 8 * h->mf.ntq;
    const long long nhi = (h->mf.nk8 + 3) / 4;
    return h->sw.mfma_prec == 1 ||
           (h->sw.mfma_prec < 0 && (wgs4 >= 4LL * (h->simds / 2) || (overlap && wgs4 >= h->simds / 4 && nhi >= 32)));
}

// Three real products per complex multiply for a handle that has pre-converted images.
// The three operands a+b, d-c, c+d carry sqrt(2) more quantisation noise than a, b, c, d; on the weakest tones of a
// 60 dB comb that stays inside the project's rule (error <= max(1e-5, 3 x the reference's own fp32 error)) only
// where the window is long enough to average it: kMac3MinBlocks is the shortest window, in 32-sample blocks, from
// which test_gpu_mfma3.py::test_hdr_comb_sets_threshold measured the rule kept at every tested length.
// GSDR_MFMA_3M: 1 = wherever there are images, 0 = never.
constexpr long long kMac3MinBlocks = 94;

// A three-product handle rotates its partial sums into the accumulators once per pair of blocks
// (ddc_mfma_ring16p3r2_kernel) instead of once per block: half the rotation FMAs, phasor images
// of 64 samples instead of 32, and fewer fp32 roundings at the size of the partial sums (one rotation stage per pair,
// the small cross terms of the hi/lo split summed first).  kRot2MinBlocks is the shortest window from which
// test_gpu_mfma3r2.py::test_hdr_comb_default_keeps_the_rule measured the rule of kMac3MinBlocks kept at every tested
// length (err / bound 0.84, 0.78, 0.56 at 94, 125, 250 blocks; shorter windows were not measured and keep the
// 32-sample loop).  GSDR_MFMA_3M_ROT: 2 = every three-product handle, 1 (or anything else) = never.
constexpr long long kRot2MinBlocks = 94;

// A handle that rotates once per pair folds each 64-sample span about its centre (ddc_convert3f_kernel +
// ddc_mfma_ring16p3f_kernel): the phasor of sample j and of its partner 63 - j are conjugates, so
// two of the three sums run over 32 sums / differences of partners: 48 MFMAs per span instead of 72, still three real
// products per complex multiply and one rotation per two blocks.  The folded operands are sums of two products, which
// costs precision on the weakest tones of a 60 dB comb; kFoldMinBlocks is the shortest of the tested windows (94, 125,
// 250 blocks) from which test_gpu_fold.py::test_hdr_comb_fold_keeps_the_rule measured the rule of kMac3MinBlocks kept at
// it and every longer tested one (err / bound 0.84, 0.70, 0.51 at 94, 125, 250 blocks, against 0.84, 0.78, 0.56 not
// folded; DESIGN.md section 4.1f, profiles/fold_parity_margins.json).  GSDR_MFMA_FOLD: 1 = every handle that rotates per pair, 0 (or anything else) = never.
constexpr long long kFoldMinBlocks = 94;

// The arithmetic of a folded handle.  The plain four products fold completely -- the same
// four units of K = 32 and 48 MFMAs per span as the Gauss fold, whose third sum has no symmetry -- and need two
// product tile sets, the images of c and d only and 64 rotation FMAs per span instead of 96.  complex_mac,
// rotation_blocks and fold in describe() name the rule that selected the handle (the three above: unchanged);
// fold_products names what it computes.  GSDR_MFMA_FOLD_PRODUCTS: 3 = the Gauss fold, 4 = the
// direct fold, unset = kFoldProductsDefault.
constexpr int kFoldProductsDefault = 4;

// The wave tile of a handle that sums the plain four products: 16 rows x 64 tones
// (ddc_mfma_ring16p4fw_kernel) copies and reads half the operand bytes of 32 x 32 (ddc_mfma_ring16p4f_kernel) for the
// same MFMAs per wave and the same bits, but splits the rows over twice the workgroups and the tones over half of them.
// It is taken where it launches no more waves for the handle's largest row count -- many tones; with 128 tones or
// fewer it would run twice the workgroups, half of their waves idle.  GSDR_MFMA_WAVE_TONES: 64 = every such handle,
// 32 = never, unset = by that rule.
//
// The span of a handle on the wide tile: 128 samples folded about their centre
// (ddc_convert4f2_kernel + ddc_mfma_ring16p4fw2_kernel) take the MFMAs of two 64-sample spans and one rotation, one P
// load, one barrier and one ring rotation instead of two.  GSDR_MFMA_SPAN: 128 = every handle on the wide tile, 64 = never,
// unset = a handle that took the wide tile by its own rule (GSDR_MFMA_WAVE_TONES unset: a forced wave tile keeps the
// 64-sample spans and their bits) with a window of kSpan128MinBlocks blocks or more; 0: the unset rule never takes it.
constexpr long long kSpan128MinBlocks = 125;

// The row of gsdr::product_loop for a handle by the six rules above, each asked only of a handle the one before it
// took; null without images.  nhi: the window in 32-sample blocks; max_rows, ntg: the handle's largest row count and
// its tone groups.
const gsdr::ProductLoop *product_loop_chosen(const gsdr_demod *h, bool images, long long nhi, long long max_rows, long long ntg) {
    using K = gsdr::MfmaKernel;
    const gsdr::Switches &sw = h->sw;
    const bool mac3 = images && (sw.mfma_3m == 1 || (sw.mfma_3m < 0 && nhi >= kMac3MinBlocks));
    const bool rot2 = mac3 && nhi >= 1 && (sw.mfma_3m_rot == 2 || (sw.mfma_3m_rot < 0 && nhi >= kRot2MinBlocks));
    const bool fold = rot2 && (sw.mfma_fold == 1 || (sw.mfma_fold < 0 && nhi >= kFoldMinBlocks));
    const int p = sw.mfma_fold_products, w = sw.mfma_wave_tones;
    const int products = p == 3 || p == 4 ? p : kFoldProductsDefault;
    const bool wide = w == 32 || w == 64 ? w == 64 : ((max_rows + 15) / 16) * ((ntg + 7) / 8) <= ((max_rows + 31) / 32) * ((ntg + 3) / 4);
    const bool span128 = sw.mfma_span == 128 || (sw.mfma_span < 0 && w < 0 && kSpan128MinBlocks > 0 && nhi >= kSpan128MinBlocks);
    const K kind = !mac3 ? K::AsmRing16P : !rot2 ? K::AsmRing16P3 : !fold ? K::AsmRing16P3R2 : products != 4 ? K::AsmRing16P3F
                   : !wide ? K::AsmRing16P4F : span128 ? K::AsmRing16P4FW2 : K::AsmRing16P4FW;
    return images ? gsdr::product_loop(kind) : nullptr;
}

// Tables and fixed shape of ddc_mfma_kernel.  `direct`: rows reach F-1 blocks
// back into the previous buffer (raw-sample carry); otherwise (TONES/NOISE) row o
// starts at block o of the raw window.
int setup_mfma(gsdr_demod *h, bool direct, const std::vector<long long> &tone) {
    const int F = h->F, M = h->M;
    const unsigned rate = h->nco_rate;
    h->mf_TT = h->sw.mfma_tt;
    h->mf_PK = h->sw.mfma_pk;
    h->mf_W = h->sw.mfma_w;
    if (h->mf_W > h->mf_PK / 8) h->mf_W = h->mf_PK / 8;   // every wave converts whole k-steps
    // the assembly main loops exist for the default shape only; GSDR_MFMA_ASM: 4 = LDS operand ring
    // on v_mfma_f32_16x16x32_f16 (default since round 2: the same cycles per FLOP for less energy,
    // +7 % on C3 under the power cap), 5 = that loop for workgroups of eight waves, 2 = the ring on
    // v_mfma_f32_32x32x16_f16 (round 1's production kernel), 0 = the compiler-scheduled kernel (A/B runs, tests)
    const int asm_kind = h->sw.mfma_asm;
    const bool asm_shape = h->mf_TT == 1 && h->mf_PK == 32 && h->mf_W == 4;
    h->mf_kind = gsdr::MfmaKernel::Cxx;
    if (asm_kind == 2 && asm_shape) h->mf_kind = gsdr::MfmaKernel::AsmRing;
    if (asm_kind == 4 && asm_shape) h->mf_kind = gsdr::MfmaKernel::AsmRing16;      // tools/gen_ddc_mfma_ring16.py
    if (asm_kind == 5 && asm_shape) h->mf_kind = gsdr::MfmaKernel::AsmRing16W8;    // tools/gen_ddc_mfma_ring16w8.py
    gsdr::MfmaPlan pl{};
    pl.TT = h->mf_TT;
    pl.PK = h->mf_PK;
    pl.M = M;
    pl.MF = M * F;
    pl.nk8 = (pl.MF + 7) / 8;
    pl.rate = rate;
    pl.x16 = h->mf_kind == gsdr::MfmaKernel::AsmRing16 || h->mf_kind == gsdr::MfmaKernel::AsmRing16W8;
    const int nt32 = (h->ddc_channels + 31) / 32;
    pl.ntg = (nt32 + pl.TT - 1) / pl.TT;
    std::vector<unsigned> fmod_in(h->ddc_channels);
    for (int n = 0; n < h->ddc_channels; ++n) fmod_in[n] = mod_rate(tone[n], rate);
    std::vector<uint4> bfrag;
    std::vector<float2> ptab, dtab;
    std::vector<float> taps;
    std::vector<unsigned> fmod;
    float unscale = 1.f;
    gsdr::mfma_build_tables(pl, fmod_in, h->window.data(), bfrag, ptab, dtab, taps, fmod, unscale);
    HIPCHK(h, h->d_bfrag.upload(bfrag));
    HIPCHK(h, h->d_ptab.upload(ptab));
    HIPCHK(h, h->d_dtab.upload(dtab));
    HIPCHK(h, h->d_mtaps.upload(taps));
    HIPCHK(h, h->d_mfmod.upload(fmod));
    {
        // maxima per segment of the call's logical stream [carry | buffer] (TONES: the raw window, allocated
        // 2 * nfft * batching long): a segment is one block of M samples, several when blocks are short
        h->seg_k = M >= 64 ? 1 : (64 + M - 1) / M;
        const long long t_max = direct ? (long long)(F - 1) * M + h->L : 2LL * h->nfft * h->batching;
        const long long seg_len = (long long)h->seg_k * M;
        h->nseg_alloc = (int)((t_max + seg_len - 1) / seg_len) + 2;
        HIPCHK(h, h->d_segmax.alloc_zeroed((size_t)kScaleSlots * h->nseg_alloc));
    }
    gsdr::MfmaShape &sh = h->mf;
    sh.N = h->ddc_channels;
    sh.NT32 = pl.ntg * pl.TT;
    sh.ntg = pl.ntg;
    sh.ntq = (pl.ntg + h->mf_W - 1) / h->mf_W;
    sh.M = M;
    sh.MF = pl.MF;
    sh.F = F;
    sh.nk8 = pl.nk8;
    sh.woff = direct ? -(F - 1) : 0;
    sh.carry_len = direct ? (F - 1) * M : 0;
    sh.rate = rate;
    sh.rate_magic = 0xffffffffffffffffULL / rate;
    sh.inv_rate = 1.0 / (double)rate;
    sh.m_mod_rate = (unsigned)M % rate;
    sh.unscale = unscale;
#ifdef GSDR_TIMING_BUILD
    sh.timing_mode = h->sw.mfma_timing;   // ablation builds only (scratch/), never shipped
#else
    sh.timing_mode = 0;
#endif
    sh.rt = h->sw.mfma_rt;   // 0: chosen per launch in enqueue_mfma
    if (direct) {
        // row tile 0 and the last row tile read from copies with the carry in front
        // and zeros behind (sizes: ddc_mfma_kernel's reach, 8*nk8 samples per row)
        const size_t reach = (size_t)((pl.nk8 + pl.PK / 8 - 1) / (pl.PK / 8)) * pl.PK;   // whole phasor blocks
        const size_t head_n = (size_t)sh.carry_len + 32u * (size_t)M + reach + 8;
        const size_t tail_n = (size_t)(32 + F) * (size_t)M + reach + 8;
        for (int i = 0; i < kStageSets; ++i) {
            HIPCHK(h, h->d_head[i].alloc_zeroed(head_n));
            HIPCHK(h, h->d_tail[i].alloc_zeroed(tail_n));
        }
    }
    // pre-converted operands: allocated when a launch of this handle may use them (the largest row count, in an
    // overlapped entry), up to 8 GiB of images
    if (h->mf_kind == gsdr::MfmaKernel::AsmRing16) {
        const long long max_rows = direct ? h->L / M : (long long)h->batching;
        const long long ngt_max = (max_rows + 31) / 32;
        const long long nhi = (pl.nk8 + 3) / 4;
        const gsdr::ProductLoop *row = product_loop_chosen(h, prec_pays(h, ngt_max, /*overlap=*/true), nhi, max_rows, pl.ntg);
        // uint4 per image set: 12 / 8 KiB per block, folded 16 KiB per pair of blocks
        const size_t img_n = row ? (size_t)ngt_max * (size_t)((nhi + row->image_blocks - 1) / row->image_blocks) * row->image_uint4 : 0;
        if (img_n * sizeof(uint4) > (size_t)8 << 30) row = nullptr;
        for (int i = 0; i < kStageSets && row; ++i) HIPCHK(h, h->d_img[i].alloc(img_n));
        h->prec = row != nullptr;
        h->loop = row && row->build_tables ? row : nullptr;      // AsmRing16P's row: chosen per launch
        if (h->loop) {
            std::vector<uint4> bfrag3;
            std::vector<float4> ptab3;
            row->build_tables(pl, fmod, bfrag3, ptab3);
            HIPCHK(h, h->d_bfrag3.upload(bfrag3));
            HIPCHK(h, h->d_ptab3.upload(ptab3));
        }
    }
    h->mfma = true;
    h->kernel_name = gsdr::ddc_mfma_kernel_name(h->loop ? h->loop->kind : h->mf_kind);
    return 0;
}

// absmax pass over `in` + ddc_mfma_kernel over `nout` rows.  DIRECT: raw == nullptr,
// the rows read `in` (and its head/tail copies).  TONES: the pass also appends
// `in` to the raw window at raw_new0 and the rows read raw[0 .. nx).
int enqueue_mfma(gsdr_demod *h, const float2 *in, float2 *raw, long long raw_new0, long long nx,
                 int nout, unsigned idx_base, float2 *out, hipStream_t st, const float2 *spare_src = nullptr,
                 long long spare_n = 0);

// Orders `st` behind every stream in h->dirty for which keep(s) is false, and forgets those.
template <typename Keep>
int join_streams(gsdr_demod *h, hipStream_t st, Keep keep) {
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
    if (!h->prof || h->ev_used >= (size_t)kMaxEvents) return 0;
    if (h->prof_seen++ % (unsigned long long)h->prof_every != 0) return 0;
    if (h->ev_used == h->ev_pool.size()) {
        gsdr::Event a, b;
        HIPCHK(h, hipEventCreate(a.out()));
        HIPCHK(h, hipEventCreate(b.out()));
        h->ev_pool.emplace_back(std::move(a), std::move(b));
    }
    HIPCHK(h, hipEventRecord(h->ev_pool[h->ev_used].first, st));
    *stop = h->ev_pool[h->ev_used].second;
    h->ev_used++;
    return 0;
}

// ---------------------------------------------------------------------------
// per-mode enqueue
// ---------------------------------------------------------------------------

// Grid size of the DDC launch, measured instead of guessed: times the real
// launch (ddc kernel + fixup) on scratch buffers for a few grid/resident ratios
// and keeps the fastest.  Runs once in create(); GSDR_DDC_AUTOTUNE=0 keeps 1.3.
int autotune_chunks(gsdr_demod *h, int nblk) {
    h->waves_ratio = 1.3;
    if (!h->pipe || h->sw.ddc_nch > 0 || !h->sw.ddc_autotune || nblk < 1) {
        h->nch_max = pick_chunks(h, nblk);
        return 0;
    }
    const size_t n_in = (size_t)nblk * h->M + h->pad + 8;
    const size_t n_out = (size_t)nblk * h->ddc_channels;
    gsdr::DevBuf<float2> x, y;
    HIPCHK(h, x.alloc(n_in));
    if (y.alloc(n_out) != hipSuccess) {
        h->err = "autotune scratch allocation failed";
        return -1;
    }
    (void)hipMemset(x, 0x3c, n_in * sizeof(float2));  // 0.0115f everywhere: finite, non-zero
    gsdr::Event e0, e1;
    (void)hipEventCreate(e0.out());
    (void)hipEventCreate(e1.out());
    const double cand[] = {0.8, 1.0, 1.3, 1.7};
    double best_ms = 1e30, best_ratio = 1.3;
    int rc = 0;
    for (double r : cand) {
        h->waves_ratio = r;
        DdcLaunch a{};
        a.x = x;
        set_tables(h, a);
        a.out = y;
        a.tails = h->d_tails;
        a.tails_nch = h->tails_nch;
        a.pipe = true;
        a.sh.N = h->ddc_channels;
        a.sh.Npad = h->Npad;
        a.sh.TW = h->TW;
        a.sh.rate = h->nco_rate;
        a.sh.M = h->M;
        a.sh.nblk = nblk;
        a.sh.nch = pick_chunks(h, nblk);
        a.sh.xlast = (long long)nblk * h->M + h->pad - 4;
        finish_shape(a.sh);
        float ms = 0.f;
        for (int it = 0; it < 4 && !rc; ++it) {  // first iteration warms up
            if (it == 1) rc |= hipEventRecord(e0, h->stream) != hipSuccess;
            rc |= gsdr::launch_ddc(h->F, h->K, a, h->stream, nullptr) != hipSuccess;
        }
        rc |= hipEventRecord(e1, h->stream) != hipSuccess;
        rc |= hipEventSynchronize(e1) != hipSuccess;
        if (rc || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
            rc = 1;
            break;
        }
        if (ms < best_ms) {
            best_ms = ms;
            best_ratio = r;
        }
    }
    if (rc) {
        h->err = "autotune launch failed";
        return -1;
    }
    h->waves_ratio = best_ratio;
    h->nch_max = pick_chunks(h, nblk);
    return 0;
}

int enqueue_mfma(gsdr_demod *h, const float2 *in, float2 *raw, long long raw_new0, long long nx,
                 int nout, unsigned idx_base, float2 *out, hipStream_t st, const float2 *spare_src,
                 long long spare_n) {
    // tables of segment maxima: this call's, and the one the staging pass clears for the next call.
    // kScaleSlots of them, so that the pass of call j (filling table j, clearing table j+1) leaves
    // alone what the main kernels of the calls still in flight read (tables j-1 .. j-kPipeStreams+1).
    const int cur = (int)(h->call_no % kScaleSlots), next = (int)((h->call_no + 1) % kScaleSlots);
    const int hs = (int)(h->call_no % kStageSets), hs_next = (int)((h->call_no + 1) % kStageSets);
    gsdr::MfmaLaunch a{};
    a.sh = h->mf;
    a.sh.nout = nout;
    a.sh.ngt = (nout + 31) / 32;
    a.sh.nx = nx;
    a.sh.idx_base = idx_base;
    a.sh.seg_k = h->seg_k;
    gsdr::StageLaunch sg{};
    sg.x = in;
    sg.n = h->L;
    sg.seg = h->d_segmax + (size_t)cur * h->nseg_alloc;
    sg.seg_clear = h->d_segmax + (size_t)next * h->nseg_alloc;
    sg.nseg_alloc = h->nseg_alloc;
    sg.seg_len = (long long)h->seg_k * a.sh.M;
    if (h->loop) a.sh.rt = 1;       // one kernel pair for every launch of the handle
    if (a.sh.rt == 0) {
        // Two row tiles per workgroup (the second keeps the phasor images: 64 KiB less to load, one
        // preamble less, half as many workgroups).  Measured at decim 100 (13-block windows) for
        // 128 .. 2048 tones, in order and overlapped (scratch/rt_probe.py): it pays in exactly one
        // place, a launch of between one and two rounds of workgroups in the overlapped entries
        // (256 tones, 626 workgroups: 31.3 -> 29.4 us per buffer), where the neighbouring launches
        // fill the compute units that 313 longer workgroups leave free; everywhere else it is
        // neutral or costs up to 15 % (in order, few workgroups).
        const int nblk = (a.sh.nk8 + 3) / 4;
        const long long wgs = (long long)a.sh.ngt * a.sh.ntq;
        a.sh.rt = h->pipe_overlap && nblk <= 32 && wgs >= 512 && wgs < 1024 ? 2 : 1;
    }
    h->last_rt = a.sh.rt;
    if (raw) {
        // TONES: one pass brings the carried samples to the front of this call's raw window,
        // appends the buffer and takes its maximum; every row reads the window itself
        // (allocated twice as long as it gets)
        if (spare_n != raw_new0) {
            h->err = "raw window bookkeeping out of step";
            return -1;
        }
        sg.b = spare_src;
        sg.nb = spare_n;
        sg.b_dst = raw;
        sg.head_cur = raw + raw_new0;
        sg.head_n = h->L;
        sg.tail0 = h->L;
        HIPCHK(h, gsdr::launch_absmax(sg, st));
        if (h->pipe_overlap) HIPCHK(h, hipEventRecord(h->ev_abs[h->pipe_seq % 4], st));
        a.x = a.head = a.tail = raw;
        a.sh.tail0 = 0;
    } else {
        const int cl = a.sh.carry_len;
        const long long t0 = a.sh.ngt > 1 ? (long long)(32 * (a.sh.ngt - 1) + a.sh.woff) * a.sh.M : h->L;
        const int ks = h->mf_PK / 8;
        long long head_n = 32LL * a.sh.M + (long long)((a.sh.nk8 + ks - 1) / ks) * h->mf_PK + 8;
        if (head_n > h->L) head_n = h->L;
        sg.b = h->d_head[hs];       // the carry: the last cl samples of the previous buffer, left there by its pass
        sg.nb = cl;
        sg.head_cur = h->d_head[hs];
        sg.head_n = head_n;
        sg.head_next = h->d_head[hs_next];
        sg.carry_len = cl;
        sg.tail = h->d_tail[hs];
        sg.tail0 = t0;
        HIPCHK(h, gsdr::launch_absmax(sg, st));
        if (h->pipe_overlap) HIPCHK(h, hipEventRecord(h->ev_abs[h->pipe_seq % 4], st));
        a.x = in;
        a.head = h->d_head[hs];
        a.tail = h->d_tail[hs];
        a.sh.tail0 = t0;
    }
    a.taps = h->d_mtaps;
    a.bfrag = h->d_bfrag;
    a.ptab = h->d_ptab;
    a.dtab = h->d_dtab;
    a.fmod = h->d_mfmod;
    a.segmax = sg.seg;
    a.out = out;
    hipEvent_t stop = nullptr;
    if (record_begin(h, st, &stop)) return -1;
    // One launch at a time (in-order entries) that needs the two workgroups per compute unit the
    // 4-wave kernel is resident with: the hardware serves the older of the two first, the younger ends
    // 40 % later and runs the tail alone.  If the launch fits the compute
    // units as 8-wave workgroups (same tables, same loop, the two waves of a SIMD barrier-coupled
    // partners), that kernel ends 4-7 % earlier (C3: 145 against 152-158 us).  The overlapped entries
    // keep the 4-wave kernel: there the next buffer's workgroups fill the slots the older ones free.
    gsdr::MfmaKernel kind = h->mf_kind;
    if (h->loop) {
        // whatever the entry, the stream pattern or the row count: one arithmetic per handle
        kind = h->loop->kind;
        a.img = h->d_img[hs];
        a.bfrag3 = h->d_bfrag3;
        a.ptab3 = h->d_ptab3;
    } else if (kind == gsdr::MfmaKernel::AsmRing16 && h->prec && a.sh.rt <= 1 && prec_pays(h, a.sh.ngt, h->pipe_overlap)) {
        kind = gsdr::MfmaKernel::AsmRing16P;
        a.img = h->d_img[hs];
    } else if (kind == gsdr::MfmaKernel::AsmRing16 && !h->pipe_overlap && h->sw.mfma_w8) {
        const long long wgs4 = (long long)((a.sh.ngt + 7) / 8) * 8 * a.sh.ntq;
        const long long wgs8 = (long long)((a.sh.ngt + 7) / 8) * 8 * ((a.sh.ntg + 7) / 8);
        if (a.sh.rt <= 1 && wgs4 > h->simds / 4 && wgs4 <= h->simds / 2 && wgs8 <= h->simds / 4)
            kind = gsdr::MfmaKernel::AsmRing16W8;
    }
    h->kernel_name = gsdr::ddc_mfma_kernel_name(kind);
    HIPCHK(h, gsdr::launch_ddc_mfma(kind, h->mf_TT, h->mf_PK, h->mf_W, a, st));
    if (stop) HIPCHK(h, hipEventRecord(stop, st));
    h->call_no++;
    return 0;
}

// ref: process_direct, cpp/USRP_demodulator.cpp:400-464
int enqueue_direct(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    DdcLaunch a{};
    a.x = in;
    set_tables(h, a);
    a.pipe = h->pipe && h->decim > 0 && h->L >= 4;
    a.few = h->few;
    a.out = out;
    a.sh.N = h->N;
    a.sh.Npad = h->Npad;
    a.sh.TW = h->TW;
    a.sh.rate = h->nco_rate;
    a.sh.idx0 = h->idx;
    a.sh.g_off = 0;
    long long ret;
    hipEvent_t stop = nullptr;
    if (h->decim > 0 && h->mfma) {
        const unsigned rate = h->nco_rate;
        const unsigned back = (unsigned)(((unsigned long long)(h->F - 1) * h->M) % rate);
        const unsigned idx_base = (unsigned)((h->idx + rate - back) % rate);
        if (enqueue_mfma(h, in, nullptr, 0, h->L, (int)(h->L / h->M), idx_base, out, st)) return -1;
        ret = (long long)h->N * (h->L / h->M);               // :459
    } else if (h->decim > 0) {
        a.tails = h->d_tails;
        a.tails_nch = h->tails_nch;
        a.carry_in = h->d_carry[h->parity];
        a.carry_out = h->d_carry[h->parity ^ 1];
        a.sh.M = h->M;
        a.sh.nblk = (int)(h->L / h->M);
        a.sh.nch = h->nch_max;
        a.sh.xlast = h->L - 4;
        if (a.pipe && h->pad > 0) {
            // the last sub-block of a block reads `pad` samples past it (zero taps);
            // behind the last block that would leave the caller's buffer
            HIPCHK(h, hipMemcpyAsync(h->d_stage, in, (size_t)h->L * sizeof(float2),
                                     hipMemcpyDeviceToDevice, st));
            a.x = h->d_stage;
            a.sh.xlast = h->L + h->pad - 4;
        }
        finish_shape(a.sh);
        if (record_begin(h, st, &stop)) return -1;
        HIPCHK(h, gsdr::launch_ddc(h->F, h->K, a, st, stop));
        h->parity ^= 1;
        ret = (long long)h->N * (h->L / h->M);               // :459
    } else {
        a.sh.M = h->K;
        a.sh.total = h->L;
        a.sh.nblk = (int)((h->L + h->K - 1) / h->K);
        long long nch = h->target_waves / h->TW;
        if (nch < 1) nch = 1;
        if (nch > a.sh.nblk) nch = a.sh.nblk;
        a.sh.nch = (int)nch;
        finish_shape(a.sh);
        if (record_begin(h, st, &stop)) return -1;
        HIPCHK(h, gsdr::launch_mix(h->K, a, h->sw.mix_few, st));
        if (stop) HIPCHK(h, hipEventRecord(stop, st));
        ret = (long long)h->N * h->L;                        // :457
    }
    h->idx = (h->idx + (unsigned long long)h->L) % h->nco_rate;  // :437-440
    return (int)ret;
}

// ref: process_pfb_spec (decim == 0), cpp/USRP_demodulator.cpp:568-649: polyphase filter, forward FFT of
// every complete frame, all bins kept.  Frame bookkeeping and the carry of the unconsumed samples
// are those of enqueue_pfb (the raw windows rotate, see there).
int enqueue_noise_fft(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    const int cb = h->bh.current_batch;
    float2 *win = h->d_win[h->win_seq % kStageSets];
    if (h->prev_spare_samples > 0)   // :590-596 of the previous call
        HIPCHK(h, hipMemcpyAsync(win, h->d_win[(h->win_seq + kStageSets - 1) % kStageSets] + h->prev_spare_begin,
                                 (size_t)h->prev_spare_samples * sizeof(float2), hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemcpyAsync(win + h->bh.new_0, in, (size_t)h->L * sizeof(float2), hipMemcpyDeviceToDevice, st));  // :573-577
    if (cb > 0) {
        hipEvent_t stop = nullptr;
        if (record_begin(h, st, &stop)) return -1;
        HIPCHK(h, gsdr::launch_pfb_filter(win, h->d_fft_win, h->nfft, h->F, cb, h->d_fft_a, st));   // :580
        if (h->d_fft_c) {                                                                            // TONES: :531-540
            HIPCHK(h, gsdr::fft_forward(h->fft, h->d_fft_a, h->d_fft_c, h->d_fft_b, cb, st));
            HIPCHK(h, gsdr::launch_pfb_select(h->d_fft_c, h->nfft, cb, h->d_pfb_sel, h->ddc_channels, out, st));
        } else {
            HIPCHK(h, gsdr::fft_forward(h->fft, h->d_fft_a, out, h->d_fft_b, cb, st));               // :583
        }
        if (stop) HIPCHK(h, hipEventRecord(stop, st));
    }
    h->prev_spare_begin = h->bh.spare_begin;
    h->prev_spare_samples = h->bh.spare_samples > 0 ? h->bh.spare_samples : 0;
    h->win_seq++;
    const int ret = h->ddc_channels * cb;   // :546 (TONES), copy_size :638 (NOISE: every bin)
    gsdr_buffer_helper_update(&h->bh);      // :552 / :644
    return ret;
}

// ref: process_pfb (:486-565) and process_pfb_spec (:568-649), decim == 0: one launch, a frame per
// workgroup.  The logical raw_input is [what the previous call left over | the new buffer]; nothing is
// staged: the kernel reads both parts in place and writes this call's leftovers (:504-509, :590-596)
// into the other carry buffer.  h->kernel_name becomes the kernel launched.
int enqueue_pfb_lds(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    const int cb = h->bh.current_batch;
    const float2 *carry = h->d_pfb_carry[h->win_seq % kStageSets];
    float2 *carry_out = h->d_pfb_carry[(h->win_seq + 1) % kStageSets];
    const int spare_n = h->bh.spare_samples > 0 ? h->bh.spare_samples : 0;
    if (spare_n > h->nfft * h->F) {
        h->err = "PFB carry larger than a window";
        return -1;
    }
    const int *sel = h->mode == GSDR_NOISE ? nullptr : h->d_pfb_sel;
    const long long wlen = (long long)h->bh.new_0 + h->L;
    const gsdr::FftPlan *blue = h->pfb_blue ? &h->fft : nullptr;
    const float2 *tw = h->pfb_blue ? h->fft.d_tw : h->d_pfb_tw;
    hipEvent_t stop = nullptr;
    if (record_begin(h, st, &stop)) return -1;
    HIPCHK(h, gsdr::launch_pfb_lds(carry, h->bh.new_0, in, h->d_fft_win, tw, h->nfft, h->F, cb, sel, h->ddc_channels, out,
                                   carry_out, h->bh.spare_begin, spare_n, wlen, st, blue, h->sw, &h->kernel_name, &h->pfb_last));
    {
        const gsdr::PfbChoice &c = h->pfb_last;
        h->pfb_last_frames = cb;
        (c.cu ? h->pfb_calls_cu : h->pfb_calls_lds)++;
        if (c.cu && c.direct >= 0 && c.direct <= 5) h->pfb_calls_direct[c.direct]++;
        if (c.cu && c.teams) h->pfb_calls_teams++;
        if (c.G >= 2) h->pfb_calls_runs++;
        if (cb > 0 && c.G >= 1 && cb % c.G != 0) h->pfb_calls_short++;
    }
    if (stop) HIPCHK(h, hipEventRecord(stop, st));
    h->win_seq++;
    const int ret = h->ddc_channels * cb;  // :546 (TONES), copy_size :638 (NOISE)
    gsdr_buffer_helper_update(&h->bh);     // :552 / :644
    return ret;
}

// ref: process_pfb (decim == 0 branch), cpp/USRP_demodulator.cpp:486-565
int enqueue_pfb(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    if (h->pfb_lds) return enqueue_pfb_lds(h, in, out, st);
    if (h->noise_fft) return enqueue_noise_fft(h, in, out, st);
    // :491-495  new buffer goes after the carried samples
    const int cb = h->bh.current_batch;
    float2 *win = h->d_win[h->win_seq % kStageSets];
    const float2 *spare = h->prev_spare_samples > 0
                              ? h->d_win[(h->win_seq + kStageSets - 1) % kStageSets] + h->prev_spare_begin
                              : nullptr;
    if (!(cb > 0 && h->mfma)) {
        // :504-509 of the previous call (carry the unconsumed samples to the front), then :491-495
        if (spare)
            HIPCHK(h, hipMemcpyAsync(win, spare, (size_t)h->prev_spare_samples * sizeof(float2),
                                     hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(win + h->bh.new_0, in, (size_t)h->L * sizeof(float2),
                                 hipMemcpyDeviceToDevice, st));
        if (h->pipe_overlap) HIPCHK(h, hipEventRecord(h->ev_abs[h->pipe_seq % 4], st));
    }
    if (cb > 0 && h->mfma) {
        if (enqueue_mfma(h, in, win, h->bh.new_0, (long long)(cb + h->F - 1) * h->M, cb, 0u, out, st, spare,
                         h->prev_spare_samples))
            return -1;
    } else if (cb > 0) {
        DdcLaunch a{};
        a.x = win;
        set_tables(h, a);
        a.out = out;
        a.tails = h->d_tails;
        a.tails_nch = h->tails_nch;
        a.carry_in = nullptr;   // frames never reach back before raw_input[0]
        a.carry_out = nullptr;
        a.sh.N = h->ddc_channels;
        a.sh.Npad = h->Npad;
        a.sh.TW = h->TW;
        a.sh.rate = h->nco_rate;
        a.sh.idx0 = 0;          // raw_input[0] is always on the frame grid
        a.sh.M = h->M;
        a.sh.nblk = cb + h->F - 1;  // frame r spans blocks r .. r+F-1
        a.pipe = h->pipe;
        a.sh.xlast = (long long)a.sh.nblk * h->M + h->pad - 4;  // a window is allocated twice as long
        a.sh.g_off = h->F - 1;      // DDC output G <-> frame r = G-(F-1)
        const int nch = pick_chunks(h, a.sh.nblk);
        a.sh.nch = nch;
        finish_shape(a.sh);
        hipEvent_t stop = nullptr;
        if (record_begin(h, st, &stop)) return -1;
        HIPCHK(h, gsdr::launch_ddc(h->F, h->K, a, st, stop));
    }
    // :504-509 the unconsumed samples go to the front of the next call's window (see above)
    h->prev_spare_begin = h->bh.spare_begin;
    h->prev_spare_samples = h->bh.spare_samples > 0 ? h->bh.spare_samples : 0;
    h->win_seq++;
    const int ret = h->ddc_channels * cb;  // :546 (TONES), copy_size :638 (NOISE)
    gsdr_buffer_helper_update(&h->bh);   // :552
    return ret;
}

// TONES / NOISE with gsdr_demod_set_frame_average(k > 1): the PFB writes its frames to the handle's frame buffer, and
// pfb_average_kernel behind it on the same stream writes the groups that complete to `out` and the sums of the open
// group to the other accumulator.  The bookkeeping is host integers, so the returned length is known at once.  The
// chain of accumulators is ordered like the raw-window carry: by the stream, and by join_streams when it changes.
int enqueue_pfb_average(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    const int cb = h->bh.current_batch;
    const size_t ev0 = h->ev_used;
    if (enqueue_pfb(h, in, h->d_avg_frames, st) < 0) return -1;
    if (cb <= 0) return 0;
    const long long rows = ((long long)h->avg_count + cb) / h->avg_k;
    HIPCHK(h, gsdr::launch_pfb_average(h->d_avg_frames, cb, h->ddc_channels, h->avg_k, h->avg_kind, h->avg_count,
                                       h->d_avg_acc[h->avg_seq % 2], h->d_avg_acc[(h->avg_seq + 1) % 2], out, st));
    // the profile pair of this call (if it is a timed one) closes behind the averaging: recorded again, an event keeps the later point
    if (h->ev_used > ev0) HIPCHK(h, hipEventRecord(h->ev_pool[h->ev_used - 1].second, st));
    h->avg_seq++;
    h->avg_count = (int)(((long long)h->avg_count + cb) % h->avg_k);
    return (int)(rows * h->ddc_channels);
}

// ref: process_chirp, cpp/USRP_demodulator.cpp:342-397
int enqueue_chirp(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    hipEvent_t stop = nullptr;
    int ret;
    gsdr::ChirpPlan plan;                // the form the launcher took (gsdr_demod_describe: chirp_calls, chirp_parts)
    if (h->decim <= 0) {
        if (record_begin(h, st, &stop)) return -1;
        if (h->chirps > 1) HIPCHK(h, gsdr::launch_chirp_multi_demod(in, out, h->L, h->last_index, h->mc, st, &plan));
        else HIPCHK(h, gsdr::launch_chirp_demod(in, out, h->L, h->last_index, h->cs, st, &plan));
        if (stop) HIPCHK(h, hipEventRecord(stop, st));
        ret = (int)(h->L * h->chirps);   // :390
    } else {
        const int valid = h->vh.valid_size;      // :361
        // chirp index of the first carried sample
        const unsigned long long idx0 =
            (h->last_index + h->cs.period - (unsigned long long)h->carry_len % h->cs.period) %
            h->cs.period;
        if (record_begin(h, st, &stop)) return -1;
        if (h->chirps > 1)
            HIPCHK(h, gsdr::launch_chirp_multi_lockin(h->d_ccarry[h->cparity], h->carry_len, in, h->d_profile, h->ppt, valid,
                                                      out, idx0, h->mc, st, h->sw.chirp_split, h->d_chirp_part,
                                                      h->d_chirp_part ? kChirpPartials : 0, &plan));
        else
            HIPCHK(h, gsdr::launch_chirp_lockin(h->d_ccarry[h->cparity], h->carry_len, in,
                                                h->d_profile, h->ppt, valid, out, idx0, h->cs, st, h->sw.chirp_split,
                                                h->d_chirp_part, h->d_chirp_part ? kChirpPartials : 0, &plan));
        if (stop) HIPCHK(h, hipEventRecord(stop, st));
        // :369-380 the reference keeps the last new0 DEMODULATED samples; we
        // keep the same raw samples and re-demodulate them next call.
        const int new0 = h->vh.new0;
        if (new0 > 0) {
            // they are the tail of the logical stage [carry | in]
            const long long from_in = (long long)new0 <= h->L ? new0 : h->L;
            const long long from_carry = new0 - from_in;
            float2 *dst = h->d_ccarry[h->cparity ^ 1];
            if (from_carry > 0)
                HIPCHK(h, hipMemcpyAsync(dst, h->d_ccarry[h->cparity] + (h->carry_len - from_carry),
                                         (size_t)from_carry * sizeof(float2),
                                         hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(dst + from_carry, in + (h->L - from_in),
                                     (size_t)from_in * sizeof(float2), hipMemcpyDeviceToDevice,
                                     st));
            h->cparity ^= 1;
        }
        h->carry_len = new0;
        gsdr_vna_helper_update(&h->vh);  // :382
        ret = valid * h->chirps;         // rows [point][chirp]
    }
    h->last_index = (h->last_index + (unsigned long long)h->L) % h->cs.period;  // :355
    if (plan.form >= 0 && plan.form < 3) {
        h->chirp_calls[plan.form]++;
        h->chirp_parts = plan.parts;
    }
    return ret;
}

// ---------------------------------------------------------------------------
// creation: one setup function per mode and engine; each returns 0, or -1 with the message in h->err
// ---------------------------------------------------------------------------

int refuse(gsdr_demod *h, const char *msg) {
    h->err = msg;
    return -1;
}

// ref: :59-119
int setup_direct(gsdr_demod *h, const gsdr_param_c *p) {
    const gsdr::Switches &sw = h->sw;
    if (p->rate <= 0) return refuse(h, "rate must be positive");
    if (!(p->n_freq >= h->N && p->freq)) return refuse(h, "DIRECT needs one frequency per wave_type entry");
    const std::vector<long long> tone(p->freq, p->freq + h->N);
    if (h->decim <= 0) {
        // undecimated: only the NCO tables are needed
        h->F = 1;
        h->M = 1;
        h->window.assign(1, 1.f);
        if (setup_ddc_common(h, 1, 1, (unsigned)p->rate, tone, 1, /*allow_flat=*/false)) return -1;
        h->kernel_name = gsdr::mix_kernel_name(h->N, h->TW, h->L, h->K, sw.mix_few);
        h->capacity = (long long)h->N * h->L;
        return 0;
    }
    if (h->L % h->decim != 0) return refuse(h, "buffer_len must be a multiple of decim (ref: fir.cu:20)");
    if (p->pf_average < 1 || p->pf_average > kMaxF) return refuse(h, "pf_average must be in [1,8] for DIRECT with decimation");
    if (h->decim > 0x7fffffffLL / p->pf_average) return refuse(h, "decim*pf_average overflows");
    const int F = (int)p->pf_average, M = (int)h->decim;
    h->window.resize((size_t)M * F);
    // ref: :99 taps, cut-off 0.75/(2*decim) narrowed to float
    gsdr_make_sinc_window(M * F, (float)(0.75 / (M * 2)), h->window.data());
    if (setup_ddc_common(h, F, M, (unsigned)p->rate, tone, (int)(h->L / M))) return -1;
    if (h->pipe && h->pad > 0 && h->d_stage.alloc_zeroed((size_t)h->L + h->pad) != hipSuccess)
        return refuse(h, "staging allocation failed");
    h->kernel_name = h->pipe ? gsdr::ddc_flat_kernel_name() : gsdr::ddc_kernel_name();
    for (auto &c : h->d_carry)
        if (c.alloc_zeroed((size_t)(F > 1 ? F - 1 : 1) * h->Npad) != hipSuccess) return refuse(h, "carry allocation failed");
    // (rows read whole 32-sample phasor blocks: the padding behind a window must stay
    //  within the next block, or middle rows would read past the buffer)
    // A handful of tones at a long decimation: every engine below walks a block's samples in sequence per
    // tone lane / matrix column, and a launch is as long as one workgroup's walk (72 us per 1 M-sample
    // buffer for 1 ... 256 tones at decim 1000).  ddc_few_kernel splits the block over the lanes of a wave
    // per (chunk, tone): 16 tones at decim 1000 in 15 us (profiles/r03_shape_sweep.log).  GSDR_DDC_FEW=0: off.
    h->few = sw.ddc_mfma && sw.ddc_few && !h->pipe && M >= 512 && h->N <= 32 && h->TW == 1;
    if (h->few) h->kernel_name = gsdr::ddc_few_kernel_name();
    if (!h->few && sw.ddc_mfma && h->L / M >= F - 1 && h->L >= 4 && F <= 33 && (M * F + 31) / 32 * 32 - M * F <= M &&
        setup_mfma(h, /*direct=*/true, tone))
        return -1;
    if (!h->mfma && autotune_chunks(h, (int)(h->L / M))) return -1;
    h->capacity = (long long)h->N * (h->L / M);
    return 0;
}

// TONES / NOISE, a frame per workgroup -- polyphase filter, transform inside the LDS, bin selection: the
// reference's own algorithm (:486-565, :568-649) at one read of the window and one write of the selected bins per
// buffer.  blue_m > 0: through Bluestein's identity at that padded length.
int setup_pfb_lds(gsdr_demod *h, bool noise, int F, const std::vector<long long> &tone, long long blue_m) {
    h->pfb_lds = true;
    h->pfb_blue = blue_m > 0;
    h->F = F;
    h->M = h->nfft;
    std::vector<float2> tw((size_t)h->nfft);
    for (int k = 0; k < h->nfft; ++k) {
        const double a = -2.0 * M_PI * (double)k / (double)h->nfft;
        tw[(size_t)k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    const std::vector<int> sel(tone.begin(), tone.end());
    bool ok = h->d_pfb_tw.upload(tw) == hipSuccess && h->d_fft_win.upload(h->window) == hipSuccess &&
              (noise || h->d_pfb_sel.upload(sel) == hipSuccess);
    // Bluestein: the chirp, its transform and the twiddles of length m (fft_plan_build makes exactly these)
    if (ok && h->pfb_blue) ok = gsdr::fft_plan_build(h->fft, h->nfft) == 0 && h->fft.m == (int)blue_m;
    for (int i = 0; i < kStageSets && ok; ++i) ok = h->d_pfb_carry[i].alloc_zeroed((size_t)h->nfft * F + 8) == hipSuccess;
    if (!ok) return refuse(h, "PFB allocation failed");
    // the kernel of a call of L / nfft frames (each launch reports its own, enqueue_pfb_lds)
    h->kernel_name = gsdr::pfb_kernel_name(gsdr::pfb_choose(h->nfft, F, h->pfb_blue ? &h->fft : nullptr,
                                                            (int)(h->L / h->nfft), h->ddc_channels, device_cus(), h->sw));
    return 0;
}

// Frames the LDS kernel does not take: the polyphase filter and one launch per radix stage through memory (§4.5) --
// NOISE keeps every bin, TONES (tones_global) picks its bins out of a scratch spectrum.  For TONES this replaces one
// DDC per bin when the frame is long (above 8192 points a frame is a window of 32 768+ samples: the DDC rows become
// thousand-block loops on a handful of workgroups)
int setup_pfb_global(gsdr_demod *h, bool tones_global, int F, const std::vector<long long> &tone) {
    h->noise_fft = true;
    h->F = F;
    h->M = h->nfft;
    h->kernel_name = gsdr::fft_kernel_name();
    if (tones_global) {
        const std::vector<int> sel(tone.begin(), tone.end());
        if (h->d_pfb_sel.upload(sel) != hipSuccess || h->d_fft_c.alloc((size_t)h->nfft * (size_t)h->batching) != hipSuccess)
            return refuse(h, "TONES allocation failed");
    }
    if (gsdr::fft_plan_build(h->fft, h->nfft) != 0) return refuse(h, "cannot plan an FFT of fft_tones points");
    const size_t len = (size_t)(h->fft.m > h->nfft ? h->fft.m : h->nfft) * (size_t)h->batching;
    bool ok = h->d_fft_a.alloc(len) == hipSuccess && h->d_fft_b.alloc(len) == hipSuccess &&
              h->d_fft_win.upload(h->window) == hipSuccess;
    for (int i = 0; i < kStageSets && ok; ++i) ok = h->d_win[i].alloc_zeroed((size_t)h->nfft * h->batching * 2) == hipSuccess;
    return ok ? 0 : refuse(h, "NOISE allocation failed");
}

// Every selected bin as a tone of the DDC kernels (GSDR_PFB_LDS=0 with GSDR_TONES_FFT=0 / GSDR_NOISE_FFT=0)
int setup_pfb_ddc(gsdr_demod *h, int F, const std::vector<long long> &tone) {
    const int rc = setup_ddc_common(h, F, h->nfft, (unsigned)h->nfft, tone, (int)(h->L / h->nfft) + F + 6);
    h->kernel_name = h->pipe ? gsdr::ddc_flat_kernel_name() : gsdr::ddc_kernel_name();
    if (rc) return -1;
    // raw_input (:143) plus an equally long half of padding behind it, kStageSets times
    for (auto &w : h->d_win)
        if (w.alloc_zeroed((size_t)h->nfft * h->batching * 2) != hipSuccess) return refuse(h, "raw_input allocation failed");
    // every carried sample of the raw window must come from the previous buffer
    // (absmax covers this buffer and the one before)
    // and the padding behind the last window must stay inside the raw buffer's spare half
    if (h->sw.ddc_mfma && (long long)h->nfft * (F + 1) <= h->L && (long long)h->nfft * h->batching >= 40 &&
        setup_mfma(h, /*direct=*/false, tone))
        return -1;
    if (!h->mfma && autotune_chunks(h, (int)(h->L / h->nfft) + F - 1)) return -1;
    return 0;
}

// TONES, ref: :121-175, :702-768; NOISE, ref: :264-313 (full spectrum: every FFT bin is a channel)
int setup_pfb(gsdr_demod *h, const gsdr_param_c *p) {
    const gsdr::Switches &sw = h->sw;
    const bool noise = (h->mode == GSDR_NOISE);
    if (p->rate <= 0) return refuse(h, "rate must be positive");
    if (p->fft_tones < 1) return refuse(h, "fft_tones must be >= 1");
    if (p->pf_average < 1 || p->pf_average > kMaxF) return refuse(h, "pf_average must be in [1,8] for TONES/NOISE");
    if (!(noise || (p->n_freq >= h->N && p->freq))) return refuse(h, "TONES needs one frequency per wave_type entry");
    if (h->decim > 0)
        return refuse(h, "TONES/NOISE with decim > 0 is not supported: the reference path is broken "
                         "(ref: kernels.cu:718-719,747,779, USRP_demodulator.cpp:172,516)");
    if ((long long)p->fft_tones * p->pf_average > 0x7fffffffLL) return refuse(h, "fft_tones*pf_average overflows");
    // NOISE: polyphase filter + batched FFT of every frame (fft_kernels.hip), any fft_tones.
    // GSDR_NOISE_FFT=0 evaluates every bin as a DDC tone instead (round 1's path: O(fft_tones)
    // per sample, kept for A/B runs and refused above 16384 bins)
    const bool noise_fft = noise && sw.noise_fft;
    if (noise && !noise_fft && p->fft_tones > 16384)
        return refuse(h, "NOISE without the FFT stage (GSDR_NOISE_FFT=0) supports fft_tones <= 16384");
    h->nfft = p->fft_tones;
    const int F = (int)p->pf_average;
    h->fcut = (float)(1. / (2 * h->nfft));                     // :131, :274
    h->window.resize((size_t)h->nfft * F);
    gsdr_make_sinc_window(h->nfft * F, h->fcut, h->window.data());  // :134, :277
    h->batching = gsdr_pfb_batching(h->L, h->nfft, F);         // :706
    const int n_ch = noise ? h->nfft : h->N;                   // channels of the DDC launch
    h->bins.resize(n_ch);
    if (noise) {
        for (int u = 0; u < n_ch; ++u) h->bins[u] = u;         // process_pfb_spec keeps every bin
    } else {
        gsdr_pfb_tone_bins(p->rate, h->nfft, p->freq, h->N, h->bins.data());  // :722-733
    }
    std::vector<long long> tone(n_ch);
    for (int u = 0; u < n_ch; ++u) tone[u] = h->bins[u] < 0 ? 0 : h->bins[u];
    // buffer_helper(n_tones, buffer_len, average, n_eff_tones): :159 / :301
    gsdr_buffer_helper_init(&h->bh, h->nfft, (int)h->L, F, n_ch);
    h->ddc_channels = n_ch;
    h->capacity = (long long)n_ch * h->batching;               // :147 / :288
    // The engine.  In the LDS: frames of up to 8192 points without a prime factor above 127;
    // GSDR_PFB_LDS=0, GSDR_TONES_FFT=0 (TONES only) or such a length leave TONES to the DDC
    // kernels (every selected bin as a tone) and NOISE to the global-memory FFT stages.
    int radices16[16];
    const bool direct_ok = gsdr::pfb_lds_plan(h->nfft, radices16, sw.pfb_radix8) >= 0;
    // a prime factor above 127 (or GSDR_PFB_BLUESTEIN=1: any length, for tests): Bluestein's identity inside
    // the workgroup, when a frame at the padded length m = 2^ceil(log2(2 nfft - 1)) fits the LDS
    const long long blue_m = gsdr::pfb_blue_length(h->nfft, F, sw.pfb_bluestein, gsdr::pfb_switches(sw));
    const bool blue_ok = blue_m > 0;
    if (sw.pfb_lds && (direct_ok || blue_ok) && (noise ? noise_fft : sw.tones_fft))
        return setup_pfb_lds(h, noise, F, tone, blue_ok ? blue_m : 0);
    const bool tones_global = !noise && sw.tones_fft;
    if (noise_fft || tones_global) return setup_pfb_global(h, tones_global, F, tone);
    return setup_pfb_ddc(h, F, tone);
}

// ref: :177-262
int setup_chirp(gsdr_demod *h, const gsdr_param_c *p) {
    if (p->rate <= 0) return refuse(h, "rate must be positive");
    if (!(p->n_freq >= 1 && p->n_chirp_f >= 1 && p->n_swipe_s >= 1 && p->n_chirp_t >= 1 && p->freq && p->chirp_f &&
          p->swipe_s && p->chirp_t))
        return refuse(h, "CHIRP needs freq[0], chirp_f[0], swipe_s[0] and chirp_t[0]");
    gsdr_chirp_param cp;
    gsdr_chirp_derive(p->rate, p->freq[0], p->chirp_f[0], p->swipe_s[0], p->chirp_t[0], &cp);
    if (!(cp.num_steps >= 1 && cp.length >= 1 && cp.num_steps <= 0x7fffffffffffffffULL / cp.length))
        return refuse(h, "chirp period overflows");
    h->cs = chirp_shape(cp);
    // several chirps (demod_create has checked what they must share): chirp c differs in f0 and chirpness alone
    const bool multi = h->chirps > 1;
    if (multi) {
        gsdr_chirp_param all[GSDR_MULTI_CHIRP_MAX];
        for (int c = 0; c < h->chirps; ++c)
            gsdr_chirp_derive(p->rate, p->freq[c], p->chirp_f[c], p->swipe_s[0], p->chirp_t[0], &all[c]);
        if (const char *bad = gsdr::multi_chirp_shape(all, h->chirps, h->mc)) return refuse(h, bad);
    }
    if (h->decim <= 0) {
        h->kernel_name = multi ? gsdr::chirp_multi_demod_kernel_name() : gsdr::chirp_demod_kernel_name();
        h->capacity = h->L * h->chirps;
        return 0;
    }
    const unsigned long long ppt = cp.length * (unsigned long long)h->decim;  // :231
    if (!(ppt >= 1 && ppt <= (unsigned long long)h->L)) return refuse(h, "chirp lock-in needs length*decim <= buffer_len");
    h->ppt = (int)ppt;
    gsdr_vna_helper_init(&h->vh, h->ppt, (int)h->L);       // :235
    h->window.resize(h->ppt);
    gsdr_make_flat_window(h->ppt, h->ppt / 10, h->window.data());  // :246
    h->kernel_name = multi ? gsdr::chirp_multi_lockin_kernel_name() : gsdr::chirp_lockin_kernel_name();
    h->capacity = (h->L / h->ppt + 1) * h->chirps;
    if (h->d_profile.upload(h->window) != hipSuccess || h->d_ccarry[0].alloc((size_t)h->ppt) != hipSuccess ||
        h->d_ccarry[1].alloc((size_t)h->ppt) != hipSuccess || h->d_chirp_part.alloc((size_t)kChirpPartials) != hipSuccess)
        return refuse(h, "chirp allocation failed");
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
        h->chirps = chirps;
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

}  // namespace

extern "C" {

const char *gsdr_last_error(const gsdr_demod *h) {
    return h ? h->err.c_str() : create_error().c_str();
}

gsdr_demod *gsdr_demod_create(const gsdr_param_c *p) { return demod_create(p, gsdr::read_switches(), 0u); }
gsdr_demod *gsdr_demod_create_ex(const gsdr_param_c *p, unsigned flags) { return demod_create(p, gsdr::read_switches(), flags); }

// The body of gsdr_demod_process_device and of its sc16 twin.  in16 != nullptr: the samples arrive as sc16 and are
// widened into `wide` first (NODSP: straight into out) -- BEHIND the join below, because `wide` belongs to the handle:
// enqueued in front of it, the widening of this call could overwrite the buffer while the predecessor call, on another
// stream, still reads it.
static int process_device_body(gsdr_demod *h, const float2 *in, const gsdr_sc16 *in16, float2 *wide, float2 *out,
                               hipStream_t st);

// What every entry that takes a buffer starts with: -1 without a handle, "null buffer" into the handle without a buffer
static int refuse_null(gsdr_demod *h, const void *in, const void *out) {
    if (!h) return -1;
    if (!in || !out) {
        h->err = "null buffer";
        return -1;
    }
    return 0;
}

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

static int process_device_body(gsdr_demod *h, const float2 *in, const gsdr_sc16 *in16, float2 *wide, float2 *out,
                               hipStream_t st) {
    // An in-order call is a join point: it runs behind everything this handle has in flight on
    // other streams (an earlier call on another stream, overlapped calls still running).  Free on
    // the usual path (same stream as the call before).  Overlapped calls order themselves among
    // their compute streams (pipeline_compute) and only join the in-order streams.
    if (!h->pipe_overlap) {
        if (join_streams(h, st, [](hipStream_t) { return false; })) return -1;
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
        case GSDR_NOISE: n = h->avg_k > 1 ? enqueue_pfb_average(h, in, out, st) : enqueue_pfb(h, in, out, st); break;
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
static int staging_pair(gsdr_demod *h) {
    if (h->d_in) return 0;
    hipError_t e = h->d_in.alloc((size_t)h->L);
    if (e == hipSuccess) e = h->d_out.alloc((size_t)h->capacity);
    if (e == hipSuccess) return 0;
    h->d_in.reset(), h->d_out.reset();
    h->err = std::string("staging allocation of the host entry: ") + hipGetErrorString(e);
    return -1;
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
        if (!h->d_in16) HIPCHK(h, h->d_in16.alloc((size_t)h->L));
        HIPCHK(h, hipMemcpyAsync(h->d_in16, in16_host, (size_t)h->L * sizeof(gsdr_sc16), hipMemcpyHostToDevice, h->stream));
    } else {
        HIPCHK(h, hipMemcpyAsync(h->d_in, in_host, (size_t)h->L * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    }
    // complex64: the samples are in d_in; sc16: they are in d_in16 and the body widens them into d_in
    const int ret = in16_host ? process_device_body(h, nullptr, h->d_in16, h->d_in, h->d_out, h->stream)
                              : process_device_body(h, h->d_in, nullptr, nullptr, h->d_out, h->stream);
    if (ret < 0) return ret;
    if (ret > 0)
        HIPCHK(h, hipMemcpyAsync(out_host, h->d_out, (size_t)ret * sizeof(float2),
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

// what pipeline_init's all-or-nothing rule needs: nothing of the pipeline is left
static void pipeline_teardown(gsdr_demod *h) {
    for (auto &sl : h->slot) {
        sl.up.reset(), sl.done.reset(), sl.down.reset();
        sl.wait_ev = nullptr;
    }
    for (auto &st : h->s_main) st.reset();
    for (auto &e : h->ev_abs) e.reset();
    h->s_up.reset(), h->s_down.reset();
    h->pipe_ready = false;
}

static int pipeline_init_parts(gsdr_demod *h);

// streams and events of the pipelined entries, created on first use; all or nothing: a partial
// failure leaves no half-built pipeline behind for the next call to trip over
static int pipeline_init(gsdr_demod *h) {
    if (h->pipe_ready) return 0;
    if (pipeline_init_parts(h)) {
        const std::string keep = h->err;
        pipeline_teardown(h);
        h->err = keep;
        return -1;
    }
    h->pipe_ready = true;
    return 0;
}

static int pipeline_init_parts(gsdr_demod *h) {
    HIPCHK(h, hipStreamCreateWithFlags(h->s_up.out(), hipStreamNonBlocking));
    HIPCHK(h, hipStreamCreateWithFlags(h->s_down.out(), hipStreamNonBlocking));
    for (auto &sl : h->slot) {
        HIPCHK(h, hipEventCreateWithFlags(sl.up.out(), hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(sl.done.out(), hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(sl.down.out(), hipEventDisableTiming));
    }
    // The compute streams must sit on different hardware queues to overlap.  HIP deals the
    // streams of one priority class out to few queues (4 by default) that every other stream
    // of that class in the process shares too (torch alone creates dozens), and which streams
    // end up together is luck (measured: 53 vs 33 us per C2 buffer from run to run, and again
    // with the second handle of a process).  A stream created with a compute-unit mask gets a
    // queue of its own: ask for one with every unit enabled.  GSDR_PIPE_QUEUES=0 (or a runtime
    // that refuses) falls back to streams of the low-priority class, which is what the
    // reference gives its demodulator stream (cpp/USRP_demodulator.cpp:43-44).
    int prio_least = 0, prio_greatest = 0;
    HIPCHK(h, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    hipDeviceProp_t prop;
    int dev = 0;
    HIPCHK(h, hipGetDevice(&dev));
    HIPCHK(h, hipGetDeviceProperties(&prop, dev));
    std::vector<uint32_t> all_units((size_t)(prop.multiProcessorCount + 31) / 32, 0xffffffffu);
    if (prop.multiProcessorCount % 32) all_units.back() = (1u << (prop.multiProcessorCount % 32)) - 1u;
    for (int i = 0; i < kPipeStreams; ++i) {
        hipStream_t s = nullptr;      // (the owner takes it only when the call has succeeded)
        if (h->sw.pipe_queues && hipExtStreamCreateWithCUMask(&s, (uint32_t)all_units.size(), all_units.data()) == hipSuccess) {
            *h->s_main[i].out() = s;
            continue;
        }
        (void)hipGetLastError();
        HIPCHK(h, hipStreamCreateWithPriority(h->s_main[i].out(), hipStreamNonBlocking, prio_least));
    }
    for (int i = 0; i < 4; ++i) HIPCHK(h, hipEventCreateWithFlags(h->ev_abs[i].out(), hipEventDisableTiming));
    return 0;
}

// The kernels of one pipelined buffer; records sl.done behind them.  `up`: event the input
// becomes ready with (nullptr: it is ready).
//
// DIRECT on the staged matrix-core kernel: call j runs on compute stream j % S (S =
// GSDR_PIPE_STREAMS, kPipeStreams = 3 by default), so the kernels of consecutive buffers
// overlap and the next buffer fills the compute units that the last workgroups of this one
// leave idle.  What call j needs from its neighbours:
//   - its staging pass follows the pass of call j-1 (which wrote the carry in front of this
//     call's head copy and cleared this call's scale slot): one event, long complete when
//     it is waited for;
//   - everything it overwrites was last read by main kernels that are finished: call j-S ran
//     on the same stream, calls j-S-1 .. sit in front of pass j-1 on their streams.  The main
//     kernels of calls j-1 .. j-S+1 may still run: they read head/tail sets j-1 .. j-S+1 and
//     slots j-1 .. j-S, the pass of call j writes head/tail set j, the carry part of head j+1,
//     slot j and clears slot j+1 -- disjoint modulo kStageSets = S+1 and kScaleSlots = S+2.
// Every other mode keeps the one compute stream.  GSDR_PIPE_OVERLAP=0 does so for DIRECT too.
// in16 != nullptr (NODSP through gsdr_demod_submit_device_sc16 only): sc16 samples, widened straight into out.
static int pipeline_compute(gsdr_demod *h, gsdr_demod::Slot &sl, hipEvent_t up, const float2 *in, float2 *out,
                            const gsdr_sc16 *in16 = nullptr) {
    const bool ddc = (h->mode == GSDR_DIRECT && h->decim > 0) ||
                     h->mode == GSDR_TONES || h->mode == GSDR_NOISE;
    // TONES / NOISE inside the LDS keep the one compute stream: a launch is 10 - 15 us, the events that tie the calls
    // of rotating streams together (carry, completion) cost more than their overlap gives -- per 1 M-sample buffer
    // 16.3 against 12.0 us in order at 1024 points, 17.0 against 10.2 at 256, 25.7 against 15.4 at 1230
    // (profiles/r03_pfb_api_ab.log)
    // ... and so does a handle that averages frames (gsdr_demod_set_frame_average): its accumulators pass from call to
    // call in stream order
    const bool overlap = h->sw.pipe_overlap && h->mfma && !h->pfb_lds && ddc && h->avg_k <= 1;
    hipStream_t cs = overlap ? h->s_main[h->pipe_seq % (unsigned)h->sw.pipe_streams] : h->stream;
    if (up) HIPCHK(h, hipStreamWaitEvent(cs, up, 0));
    if (overlap) {
        // behind in-order calls made on other streams since (their carry, slot and window writes);
        // the compute streams of the pipeline are ordered by the protocol above
        if (join_streams(h, cs, [h](hipStream_t s) {
                for (int i = 0; i < kPipeStreams; ++i)
                    if (s == h->s_main[i]) return true;
                return false;
            }))
            return -1;
    }
    if (overlap && h->pipe_seq > 0) HIPCHK(h, hipStreamWaitEvent(cs, h->ev_abs[(h->pipe_seq - 1) % 4], 0));
    h->pipe_overlap = overlap;
    const int n = process_device_body(h, in, in16, nullptr, out, cs);
    h->pipe_overlap = false;
    if (overlap) h->pipe_seq++;
    if (n < 0) return -1;
    HIPCHK(h, hipEventRecord(sl.done, cs));
    return n;
}

// the device buffers of a pipeline slot, each created when the first entry that needs it asks for it
static int slot_buffers(gsdr_demod *h, gsdr_demod::Slot &sl, bool in, bool out, bool in16) {
    if (in && !sl.d_in) HIPCHK(h, sl.d_in.alloc((size_t)h->L));
    if (out && !sl.d_out) HIPCHK(h, sl.d_out.alloc((size_t)h->capacity));
    if (in16 && !sl.d_in16) HIPCHK(h, sl.d_in16.alloc((size_t)h->L));
    return 0;
}

int gsdr_demod_prepare(gsdr_demod *h, int what) {
    if (!h) return -1;
    if (h->device >= 0) HIPCHK(h, hipSetDevice(h->device));
    if (h->mode == GSDR_NODSP) return 0;
    if ((what & GSDR_PREPARE_HOST) && staging_pair(h)) return -1;
    if (what & (GSDR_PREPARE_PIPELINE | GSDR_PREPARE_PIPELINE_HOST)) {
        if (pipeline_init(h)) return -1;
    }
    const bool sc16 = (what & GSDR_PREPARE_SC16) != 0;
    if (sc16 && (what & GSDR_PREPARE_HOST) && !h->d_in16) HIPCHK(h, h->d_in16.alloc((size_t)h->L));
    if (sc16 && !h->d_wide) HIPCHK(h, h->d_wide.alloc((size_t)h->L));
    for (auto &sl : h->slot) {
        const bool host = (what & GSDR_PREPARE_PIPELINE_HOST) != 0;
        if (slot_buffers(h, sl, host || (sc16 && (what & GSDR_PREPARE_PIPELINE)), host, host && sc16)) return -1;
    }
    // first use of a stream (its hardware queue), of the copy engines in both directions and of
    // the code object costs milliseconds: pay them here, not on the first packets
    HIPCHK(h, gsdr::launch_warm(h->stream));
    // the averaging kernel's first launch, on a frame of zeros; nothing has gone through the handle yet (otherwise the
    // kernel has run already), so no group is open and the sums it leaves in the other accumulator are never read
    if (h->avg_k > 1 && h->win_seq == 0) {
        HIPCHK(h, hipMemsetAsync(h->d_avg_frames, 0, (size_t)h->ddc_channels * sizeof(float2), h->stream));
        HIPCHK(h, gsdr::launch_pfb_average(h->d_avg_frames, 1, h->ddc_channels, h->avg_k, h->avg_kind, 0, h->d_avg_acc[0],
                                           h->d_avg_acc[1], h->d_avg_frames, h->stream));
    }
    if (h->pipe_ready) {
        for (int i = 0; i < kPipeStreams; ++i) HIPCHK(h, gsdr::launch_warm(h->s_main[i]));
        float2 *pin = nullptr;
        // (no more than the slot holds: a copy past a buffer of fewer than 512 samples is refused, and the error it
        // leaves behind was reported by the next launch that asked for one -- the rehearsal's)
        const size_t warm = (size_t)h->L * sizeof(float2) < 4096 ? (size_t)h->L * sizeof(float2) : 4096;
        if (h->slot[0].d_in && hipHostMalloc((void **)&pin, 4096) == hipSuccess) {
            std::memset(pin, 0, 4096);
            (void)hipMemcpyAsync(h->slot[0].d_in, pin, warm, hipMemcpyHostToDevice, h->s_up);
            (void)hipStreamSynchronize(h->s_up);
            (void)hipMemcpyAsync(pin, h->slot[0].d_in, warm, hipMemcpyDeviceToHost, h->s_down);
            (void)hipStreamSynchronize(h->s_down);
            (void)hipHostFree(pin);
        }
    }
    HIPCHK(h, hipDeviceSynchronize());
    if (what & GSDR_PREPARE_REHEARSE) {
        // a twin with the same parameters takes the process-wide first-use costs (see include/gsdr.h)
        gsdr_demod *twin = demod_create(&h->pc, h->sw, h->flags);
        gsdr_c64 *pin_in = nullptr, *pin_out = nullptr;
        bool ok = twin != nullptr;
        ok = ok && (h->avg_k <= 1 || gsdr_demod_set_frame_average(twin, h->avg_k, h->avg_kind) == 0);
        ok = ok && hipHostMalloc((void **)&pin_in, (size_t)h->L * sizeof(gsdr_c64)) == hipSuccess;
        ok = ok && hipHostMalloc((void **)&pin_out, (size_t)(h->capacity > 0 ? h->capacity : 1) * sizeof(gsdr_c64)) == hipSuccess;
        if (ok) {
            std::memset(pin_in, 0, (size_t)h->L * sizeof(gsdr_c64));
            ok = gsdr_demod_prepare(twin, what & ~GSDR_PREPARE_REHEARSE) == 0;
            if (ok && (what & GSDR_PREPARE_HOST))
                for (int k = 0; k < 2 && ok; ++k) ok = gsdr_demod_process(twin, pin_in, pin_out) >= 0;
            // `count` buffers through a submit entry of the twin, waiting whenever the pipeline is full
            auto rehearse_submit = [&](auto submit, int count) {
                int pending = 0;
                for (int k = 0; k < count && ok; ++k) {
                    if (pending == GSDR_PIPELINE_DEPTH) {
                        ok = gsdr_demod_wait(twin) >= 0;
                        --pending;
                    }
                    ok = ok && submit() == 0;
                    ++pending;
                }
                while (ok && pending-- > 0) ok = gsdr_demod_wait(twin) >= 0;
            };
            if (ok && (what & GSDR_PREPARE_PIPELINE_HOST))
                rehearse_submit([&] { return gsdr_demod_submit(twin, pin_in, pin_out); }, 2 * GSDR_PIPELINE_DEPTH + 2);
            // the sc16 forms of the same entries (first launch of the widening kernel, on both streams it runs on);
            // the zeros of pin_in serve as L sc16 samples too
            const gsdr_sc16 *pin_in16 = reinterpret_cast<const gsdr_sc16 *>(pin_in);
            if (ok && sc16 && (what & GSDR_PREPARE_HOST))
                for (int k = 0; k < 2 && ok; ++k) ok = gsdr_demod_process_sc16(twin, pin_in16, pin_out) >= 0;
            if (ok && sc16 && (what & GSDR_PREPARE_PIPELINE_HOST))
                rehearse_submit([&] { return gsdr_demod_submit_sc16(twin, pin_in16, pin_out); }, GSDR_PIPELINE_DEPTH + 2);
        }
        if (!ok) h->err = std::string("rehearsal failed: ") + (twin ? twin->err : create_error());
        if (pin_in) (void)hipHostFree(pin_in);
        if (pin_out) (void)hipHostFree(pin_out);
        if (twin) gsdr_demod_close(twin);
        if (!ok) return -1;
    }
    return 0;
}

// What every submit entry starts with: the refusals, the device, the pipeline, and the slot the buffer goes to.  The slot
// is free: its previous download (or kernels) were waited for in gsdr_demod_wait().
static int submit_begin(gsdr_demod *h, const void *in, const void *out, gsdr_demod::Slot **slot) {
    if (refuse_null(h, in, out)) return -1;
    if (h->pipe_count >= GSDR_PIPELINE_DEPTH) {
        h->err = "pipeline full: call gsdr_demod_wait() first";
        return -1;
    }
    if (h->device >= 0) HIPCHK(h, hipSetDevice(h->device));
    if (pipeline_init(h)) return -1;
    *slot = &h->slot[(h->pipe_head + h->pipe_count) % GSDR_PIPELINE_DEPTH];
    return 0;
}

// ... and ends with: the n samples of the slot are there when wait_ev has happened
static int submit_end(gsdr_demod *h, gsdr_demod::Slot &sl, hipEvent_t wait_ev, int n) {
    sl.wait_ev = wait_ev;
    sl.n = n;
    h->pipe_count++;
    return 0;
}

// gsdr_demod_submit and gsdr_demod_submit_sc16 (in16_host != nullptr)
static int submit_host(gsdr_demod *h, const gsdr_c64 *in_host, const gsdr_sc16 *in16_host, gsdr_c64 *out_host) {
    gsdr_demod::Slot *slot = nullptr;
    if (submit_begin(h, in16_host ? (const void *)in16_host : in_host, out_host, &slot)) return -1;
    auto &sl = *slot;
    if (slot_buffers(h, sl, true, true, in16_host != nullptr)) return -1;
    if (in16_host) {
        // half the bytes, then the widening, both on the upload stream in front of sl.up: it overlaps the kernels of
        // the buffer before and does not lengthen the compute stream
        HIPCHK(h, hipMemcpyAsync(sl.d_in16, in16_host, (size_t)h->L * sizeof(gsdr_sc16), hipMemcpyHostToDevice, h->s_up));
        HIPCHK(h, gsdr::launch_widen_sc16(sl.d_in16, sl.d_in, h->L, h->sc16_scale, h->cus, h->s_up));
    } else {
        HIPCHK(h, hipMemcpyAsync(sl.d_in, in_host, (size_t)h->L * sizeof(float2), hipMemcpyHostToDevice, h->s_up));
    }
    HIPCHK(h, hipEventRecord(sl.up, h->s_up));
    const int n = pipeline_compute(h, sl, sl.up, sl.d_in, sl.d_out);
    if (n < 0) return -1;
    HIPCHK(h, hipStreamWaitEvent(h->s_down, sl.done, 0));
    if (n > 0)
        HIPCHK(h, hipMemcpyAsync(out_host, sl.d_out, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, h->s_down));
    HIPCHK(h, hipEventRecord(sl.down, h->s_down));
    return submit_end(h, sl, sl.down, n);
}

int gsdr_demod_submit(gsdr_demod *h, const gsdr_c64 *in_host, gsdr_c64 *out_host) {
    return submit_host(h, in_host, nullptr, out_host);
}

int gsdr_demod_submit_sc16(gsdr_demod *h, const gsdr_sc16 *in_host, gsdr_c64 *out_host) {
    return submit_host(h, nullptr, in_host, out_host);
}

// gsdr_demod_submit_device and gsdr_demod_submit_device_sc16 (in16_dev != nullptr)
static int submit_device(gsdr_demod *h, const gsdr_c64 *in_dev, const gsdr_sc16 *in16_dev, gsdr_c64 *out_dev) {
    gsdr_demod::Slot *slot = nullptr;
    if (submit_begin(h, in16_dev ? (const void *)in16_dev : in_dev, out_dev, &slot)) return -1;
    auto &sl = *slot;
    float2 *out = reinterpret_cast<float2 *>(out_dev);
    int n;
    if (!in16_dev) {
        n = pipeline_compute(h, sl, nullptr, reinterpret_cast<const float2 *>(in_dev), out);
    } else if (h->mode == GSDR_NODSP) {
        n = pipeline_compute(h, sl, nullptr, nullptr, out, in16_dev);
    } else {
        // in16_dev is complete (the contract of the complex64 entry): widened into the slot's input buffer -- free, its last
        // reader was waited for in gsdr_demod_wait() -- on the upload stream, beside the kernels of the buffer before
        if (slot_buffers(h, sl, true, false, false)) return -1;
        HIPCHK(h, gsdr::launch_widen_sc16(in16_dev, sl.d_in, h->L, h->sc16_scale, h->cus, h->s_up));
        HIPCHK(h, hipEventRecord(sl.up, h->s_up));
        n = pipeline_compute(h, sl, sl.up, sl.d_in, out);
    }
    if (n < 0) return -1;
    return submit_end(h, sl, sl.done, n);
}

int gsdr_demod_submit_device(gsdr_demod *h, const gsdr_c64 *in_dev, gsdr_c64 *out_dev) {
    return submit_device(h, in_dev, nullptr, out_dev);
}

int gsdr_demod_submit_device_sc16(gsdr_demod *h, const gsdr_sc16 *in_dev, gsdr_c64 *out_dev) {
    return submit_device(h, nullptr, in_dev, out_dev);
}

int gsdr_demod_wait(gsdr_demod *h) {
    if (!h) return -1;
    if (h->pipe_count == 0) return -2;
    if (h->device >= 0) HIPCHK(h, hipSetDevice(h->device));
    auto &sl = h->slot[h->pipe_head];
    const hipError_t e = hipEventSynchronize(sl.wait_ev);
    // the slot leaves the queue whatever happened: a failed wait must not leave the pipeline "full"
    h->pipe_head = (h->pipe_head + 1) % GSDR_PIPELINE_DEPTH;
    h->pipe_count--;
    if (e != hipSuccess) {
        h->err = std::string("hipEventSynchronize: ") + hipGetErrorString(e);
        return -1;
    }
    return sl.n;
}

// Nothing may be released while a stream of the handle can still run a kernel that reads it: wait for them, then delete
void gsdr_demod_close(gsdr_demod *h) {
    if (!h) return;
    if (h->device >= 0) (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (int i = 0; i < kPipeStreams; ++i)
        if (h->s_main[i]) (void)hipStreamSynchronize(h->s_main[i]);
    if (h->s_up) (void)hipStreamSynchronize(h->s_up);
    if (h->s_down) (void)hipStreamSynchronize(h->s_down);
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

int gsdr_demod_set_frame_average(gsdr_demod *h, int k, int kind) {
    if (!h) return -1;
    if (h->mode != GSDR_TONES && h->mode != GSDR_NOISE) {
        h->err = "frame average: only TONES and NOISE handles have frames to average";
        return -1;
    }
    if (k < 1 || k > GSDR_FRAME_AVERAGE_MAX) {
        h->err = "frame average: k must be in [1, " + std::to_string(GSDR_FRAME_AVERAGE_MAX) + "]";
        return -1;
    }
    if (kind != GSDR_AVERAGE_COMPLEX && kind != GSDR_AVERAGE_POWER) {
        h->err = "frame average: kind must be GSDR_AVERAGE_COMPLEX (0) or GSDR_AVERAGE_POWER (1)";
        return -1;
    }
    if (h->win_seq > 0 || h->pipe_count > 0) {
        h->err = "frame average: must be set before the first buffer goes through the handle";
        return -1;
    }
    if (h->device >= 0) HIPCHK(h, hipSetDevice(h->device));
    if (k > 1) {
        // everything the averaging needs, now (nothing is allocated by the first packets); kept when k changes again
        if (!h->d_avg_frames) HIPCHK(h, h->d_avg_frames.alloc((size_t)h->ddc_channels * (size_t)h->batching));
        for (auto &p : h->d_avg_acc) {
            if (!p) HIPCHK(h, p.alloc((size_t)h->ddc_channels));
            HIPCHK(h, hipMemset(p, 0, (size_t)h->ddc_channels * sizeof(float2)));
        }
    }
    const long long capacity = (long long)h->ddc_channels * ((h->batching + k - 1) / k);
    if (capacity > h->capacity) {
        // output staging that gsdr_demod_prepare sized for a larger k: nothing has used it yet, the entries make it anew
        h->d_out.reset();
        h->d_in.reset();                  // (the host entry allocates the two together)
        for (auto &sl : h->slot) sl.d_out.reset();
    }
    h->avg_k = k;
    h->avg_kind = kind;
    h->avg_count = 0;
    h->capacity = capacity;
    return 0;
}

int gsdr_demod_frame_average(const gsdr_demod *h, int *kind) {
    if (kind) *kind = h ? h->avg_kind : GSDR_AVERAGE_COMPLEX;
    return h ? h->avg_k : 0;
}

int gsdr_frame_average_device(const gsdr_c64 *frames_dev, int n_frames, int n_ch, int k, int kind, int count,
                              const gsdr_c64 *acc_in_dev, gsdr_c64 *acc_out_dev, gsdr_c64 *out_dev, void *hip_stream) {
    const char *bad = nullptr;
    if (n_frames < 0 || n_ch < 1) bad = "n_frames must be >= 0 and n_ch >= 1";
    else if (k < 1 || k > GSDR_FRAME_AVERAGE_MAX) bad = "k must be in [1, 1048576]";
    else if (kind != GSDR_AVERAGE_COMPLEX && kind != GSDR_AVERAGE_POWER) bad = "kind must be GSDR_AVERAGE_COMPLEX or GSDR_AVERAGE_POWER";
    else if (count < 0 || count >= k) bad = "count must be in [0, k)";
    else if (!acc_out_dev || (n_frames > 0 && !frames_dev) || (count > 0 && !acc_in_dev) ||
             (((long long)count + n_frames) / k > 0 && !out_dev)) bad = "null buffer";
    else if (((uintptr_t)frames_dev | (uintptr_t)acc_in_dev | (uintptr_t)acc_out_dev | (uintptr_t)out_dev) & 7) bad = "pointers must be 8-byte aligned";
    if (bad) {
        create_error() = std::string("gsdr_frame_average_device: ") + bad;
        return -1;
    }
    const hipError_t e = gsdr::launch_pfb_average(reinterpret_cast<const float2 *>(frames_dev), n_frames, n_ch, k, kind, count,
                                                  reinterpret_cast<const float2 *>(acc_in_dev), reinterpret_cast<float2 *>(acc_out_dev),
                                                  reinterpret_cast<float2 *>(out_dev), (hipStream_t)hip_stream);
    if (e != hipSuccess) {
        create_error() = std::string("gsdr_frame_average_device: ") + hipGetErrorString(e);
        return -1;
    }
    return (int)(((long long)count + n_frames) / k);
}

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

int gsdr_demod_get_window(const gsdr_demod *h, float *w, int cap) {
    if (!h) return 0;
    const int n = (int)h->window.size();
    if (w)
        for (int i = 0; i < n && i < cap; ++i) w[i] = h->window[i];
    return n;
}

int gsdr_demod_get_bins(const gsdr_demod *h, int *bins, int cap) {
    if (!h) return 0;
    const int n = (int)h->bins.size();
    if (bins)
        for (int i = 0; i < n && i < cap; ++i) bins[i] = h->bins[i];
    return n;
}

void gsdr_demod_profile_enable(gsdr_demod *h, int enable) {
    if (!h) return;
    h->prof = enable != 0;
    h->prof_every = enable > 1 ? enable : 1;
    h->prof_seen = 0;
    h->ev_used = 0;
}

int gsdr_demod_profile_read(gsdr_demod *h, double *total_ms) {
    if (total_ms) *total_ms = 0.0;
    if (!h || h->ev_used == 0) return 0;
    if (h->device >= 0) (void)hipSetDevice(h->device);
    double sum = 0.0;
    int n = 0;
    for (size_t i = 0; i < h->ev_used; ++i) {
        if (hipEventSynchronize(h->ev_pool[i].second) != hipSuccess) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ev_pool[i].first, h->ev_pool[i].second) == hipSuccess) {
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
    s += h->pfb_lds ? (h->pfb_blue ? "polyphase filter + Bluestein (two fp32 Stockham FFTs) inside the LDS + bin selection, one launch"
                                   : "polyphase filter + fp32 Stockham FFT inside the LDS + bin selection, one launch") :
         h->noise_fft ? "fp32 Stockham FFT behind the polyphase filter" : h->mfma ? "f16 MFMA, hi/lo split" : (h->mode == GSDR_CHIRP ? "fp32 VALU, integer phase" : (h->pipe ? "packed fp32 VALU" : "fp32 VALU"));
    s += "\", \"channels\": " + std::to_string(h->ddc_channels > 0 ? h->ddc_channels : h->N);
    if (h->mode == GSDR_CHIRP) {
        s += ", \"chirps\": " + std::to_string(h->chirps);
        // calls so far by the lock-in (or undecimated) form that ran, and the waves per point of the last one
        s += ", \"chirp_calls\": {\"plain\": " + std::to_string(h->chirp_calls[gsdr::kChirpPlain]) + ", \"split\": " +
             std::to_string(h->chirp_calls[gsdr::kChirpSplit]) + ", \"generic\": " +
             std::to_string(h->chirp_calls[gsdr::kChirpGeneric]) + "}";
        s += ", \"chirp_parts\": " + std::to_string(h->chirp_parts);
    }
    if (h->pfb_lds) {
        // the shape launch_pfb_lds chose for the last call (pfb_plan.h; frames -1: no call yet), and this handle's calls
        // so far by kernel, by the run kernel's filter (direct variant 0 - 5, 0: staged), with teams, with runs of
        // G >= 2 frames and with a last run short of G frames
        const gsdr::PfbChoice &c = h->pfb_last;
        auto n = [](unsigned long long v) { return std::to_string(v); };
        s += std::string(", \"pfb_last\": {\"kernel\": \"") + (h->pfb_last_frames < 0 ? "none" : gsdr::pfb_kernel_name(c)) + "\"";
        s += ", \"threads\": " + std::to_string(c.threads) + ", \"G\": " + std::to_string(c.G);
        s += ", \"direct\": " + std::to_string(c.direct) + ", \"dir_s\": " + std::to_string(c.dir_s);
        s += ", \"dir_gs\": " + std::to_string(c.dir_gs) + ", \"col\": " + std::to_string(c.col);
        s += ", \"teams\": " + std::to_string(c.teams) + ", \"twl\": " + std::to_string(c.twl);
        s += ", \"lds\": " + n(c.lds) + ", \"frames\": " + std::to_string(h->pfb_last_frames) + "}";
        s += ", \"pfb_calls\": {\"pfb_cu_kernel\": " + n(h->pfb_calls_cu) + ", \"pfb_lds_kernel\": " + n(h->pfb_calls_lds) + ", \"direct\": [";
        for (int v = 0; v < 6; ++v) s += (v ? ", " : "") + n(h->pfb_calls_direct[v]);
        s += "], \"teams\": " + n(h->pfb_calls_teams) + ", \"runs\": " + n(h->pfb_calls_runs) + ", \"short_last_run\": " + n(h->pfb_calls_short) + "}";
    }
    s += ", \"row_tiles_per_workgroup\": " + std::to_string(h->mfma ? h->last_rt : 0);
    // every other handle reports what the four-product loop's row says
    const gsdr::ProductLoop &pr = h->mfma && h->loop ? *h->loop : *gsdr::product_loop(gsdr::MfmaKernel::AsmRing16P);
    s += ", \"complex_mac\": " + std::to_string(pr.complex_mac);
    s += ", \"complex_mac_min_blocks\": " + std::to_string(kMac3MinBlocks);
    s += ", \"rotation_blocks\": " + std::to_string(pr.rotation_blocks);
    s += ", \"rotation_min_blocks\": " + std::to_string(kRot2MinBlocks);
    s += ", \"fold\": " + std::to_string(pr.fold);
    s += ", \"fold_min_blocks\": " + std::to_string(kFoldMinBlocks);
    s += ", \"fold_products\": " + std::to_string(pr.fold_products);
    s += ", \"wave_tones\": " + std::to_string(pr.wave_tones);
    s += ", \"span_samples\": " + std::to_string(pr.image_blocks == 4 ? 128 : 64);
    s += ", \"span128_min_blocks\": " + std::to_string(kSpan128MinBlocks);
    s += ", \"pipeline_streams\": " + std::to_string(h->sw.pipe_streams);
    s += ", \"frame_average\": " + std::to_string(h->avg_k);
    s += std::string(", \"frame_average_kind\": \"") + (h->avg_kind == GSDR_AVERAGE_POWER ? "power" : "complex") + "\"";
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
