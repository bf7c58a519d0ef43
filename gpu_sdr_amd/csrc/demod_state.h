// demod_state.h -- the RX handle (struct gsdr_demod of include/gsdr.h): what every mode uses, and the state of each
// mode and of each entry family as a member by value.  The functions of the handle are in one file per mode --
// demod_ddc.cpp (DIRECT and the DDC engines), demod_pfb.cpp (TONES / NOISE), demod_chirp.cpp (CHIRP),
// demod_pipeline.cpp (the submit entries) -- and demod.cpp (creation, the process entries, describe); those that
// cross a file are declared at the end.  Internal to csrc/.
#ifndef GSDR_DEMOD_STATE_H
#define GSDR_DEMOD_STATE_H

#include <string>
#include <utility>
#include <vector>

#include "host_util.h"

#define HIPCHK(h, expr)                                                                   \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                 \
            return -1;                                                                    \
        }                                                                                 \
    } while (0)

namespace gsdr {
namespace rx {

// Pipelined entries: compute streams that consecutive DIRECT calls go to in turn, and the
// sets of staging buffers / scale slots that keeps the calls in flight apart (pipeline_compute)
constexpr int kPipeStreams = 3;
constexpr int kChirpPartials = 16384;    // float2 slots for the partial sums of split chirp points (chirp_lockin_split_kernel)
constexpr int kStageSets = kPipeStreams + 1;
constexpr int kScaleSlots = kPipeStreams + 2;

// host-pointer entry staging (gsdr_demod_process, gsdr_demod_process_sc16)
struct HostEntry {
    DevBuf<float2> d_in, d_out;           // allocated together: both set or both empty (staging_pair)
    DevBuf<gsdr_sc16> d_in16;             // the half-size upload buffer of the sc16 host-pointer entry (widened into d_in)
};

// The pipelined entries (gsdr_demod_submit* / _wait).  The streams stand in front of the slots and events, so that
// those go before them (gsdr_demod, below).
struct Pipeline {
    Stream s_up, s_down;                  // pipelined host-pointer entry: upload and download
    // pipelined entries (gsdr_demod_submit*): consecutive DIRECT calls go to these compute streams in turn, so that
    // their kernels overlap (see pipeline_compute)
    Stream s_main[kPipeStreams];
    // pipelined host-pointer entry (gsdr_demod_submit / _wait)
    struct Slot {
        DevBuf<float2> d_in, d_out;
        DevBuf<gsdr_sc16> d_in16;         // gsdr_demod_submit_sc16: upload target, widened into d_in
        Event up, done, down;
        hipEvent_t wait_ev = nullptr;     // what gsdr_demod_wait() waits for: down (host) / done (device); not owned
        int n = 0;
    } slot[GSDR_PIPELINE_DEPTH];
    bool ready = false;                   // pipeline_init() succeeded
    int head = 0, count = 0;              // oldest outstanding slot, number outstanding
    bool overlap = false;                 // set around the compute of an overlapped call
    unsigned long long seq = 0;           // overlapped calls so far
    Event ev_abs[4];                      // pipelined entries: staging pass of call j done
};

// ---- DDC on the VALU kernels (DIRECT; TONES / NOISE with every bin a tone) ----
struct DdcState {
    int channels = 0;                  // tones the DDC kernels run (== N except NOISE: fft_tones)
    int F = 0, K = 16, M = 0, Npad = 0, TW = 0, R = 0;
    unsigned nco_rate = 1;
    unsigned long long idx = 0;        // DIRECT_current_index (ref :88, :437-440)
    int target_waves = 4096;           // resident waves the DDC grid is sized for
    int simds = 1024;                  // SIMDs of the device (4 per CU)
    int nch_max = 1;                   // chunks of the DIRECT launch (fixed nblk)
    int tails_nch = 0;                 // chunk count the tails buffer was sized for (0: not yet)
    double waves_ratio = 1.3;          // grid waves / resident waves (autotuned in create)
    DevBuf<float> d_taps_t;
    DevBuf<float> d_taps_p;            // zero-padded [nsub*K+2][FP] copy for ddc_flat_kernel
    bool flat = false;                 // ddc_flat_kernel (F <= 4) instead of ddc_kernel
    int pad = 0;                       // samples the flat kernel reads past a block (nsub*K - M)
    DevBuf<float2> d_stage;            // padded copy of the input when pad > 0 (DIRECT only)
    DevBuf<float2> d_btab;
    DevBuf<double2> d_wk, d_wrem;
    DevBuf<unsigned> d_fmod;
    DevBuf<float2> d_tails;
    DevBuf<float2> d_carry[2];
    int parity = 0;
    bool few = false;                  // DIRECT: a handful of tones at a long decimation run ddc_few_kernel (a wave per chunk and tone)
};

// ---- DDC on the matrix cores (ddc_mfma.hip) ----
struct MfmaState {
    bool on = false;
    int mf_TT = 1, mf_PK = 32, mf_W = 4;   // tone tiles per wave, phasor block, waves per workgroup
    MfmaKernel mf_kind = MfmaKernel::AsmRing;
    MfmaShape mf{};                    // fields that do not change between calls
    int last_rt = 0;                   // row tiles per workgroup of the last launch (describe())
    // pre-converted operands (ddc_convert_kernel + ddc_mfma_ring16p_kernel) for launches of many
    // rounds: one image set per staging set (the main kernels of the calls in flight read theirs)
    bool prec = false;                 // image sets allocated: the path may be chosen
    DevBuf<uint4> d_img[kStageSets];
    // the product loop of a handle with three real products per complex multiply (DESIGN.md sections 4.1d - 4.1h; a row
    // of gsdr::product_loop): decided once, in setup_mfma (product_loop_chosen); such a handle sends EVERY matrix-core
    // launch through that row's kernel pair.  Null: four products per block, the loop chosen per launch (enqueue_mfma)
    const ProductLoop *loop = nullptr;
    DevBuf<uint4> d_bfrag3;
    DevBuf<float4> d_ptab3;
    DevBuf<uint4> d_bfrag;
    DevBuf<float2> d_ptab, d_dtab;
    DevBuf<float> d_mtaps;
    DevBuf<unsigned> d_mfmod;
    // kScaleSlots tables of segment maxima (absmax_kernel), one per call in turn; seg_k blocks of M samples per segment
    DevBuf<unsigned> d_segmax;
    int seg_k = 1, nseg_alloc = 0;
    // [carry | first rows' samples | zeros] and [last rows' samples | zeros], see absmax_kernel.
    // kStageSets of each, used in turn: the staging pass of call j writes set j (and the carry
    // part of head j+1) while the main kernels of calls j-1 .. j-kPipeStreams+1 may still read theirs.
    DevBuf<float2> d_head[kStageSets];
    DevBuf<float2> d_tail[kStageSets];
    unsigned long long call_no = 0;    // absmax slot rotation
};

// ---- TONES / NOISE ----
struct PfbState {
    std::vector<int> bins;
    int nfft = 0, batching = 0;
    int taps = 0;                      // pf_average: windows of `taps` frames of nfft samples (the FFT engines; the DDC engine keeps its own F, M)
    gsdr_buffer_helper bh{};
    // raw_input (ref :143): kStageSets windows used in turn.  The staging of call j copies the
    // unconsumed end of window j-1 to the front of window j and appends the new buffer, so the
    // kernels of call j-1 may still read their window (the reference moves it in place, :504-509).
    DevBuf<float2> d_win[kStageSets];
    unsigned long long win_seq = 0;    // TONES/NOISE calls so far
    long long prev_spare_begin = 0, prev_spare_samples = 0;
    // ---- NOISE through the FFT stage (fft_kernels.hip) ----
    bool noise_fft = false;
    FftPlan fft{};
    DevBuf<float2> d_fft_a, d_fft_b;           // frames / scratch, batching * max(nfft, m) each
    DevBuf<float2> d_fft_c;                    // TONES through these stages: the spectra the bins are picked from
    DevBuf<float> d_fft_win;                   // the PFB window on the device
    // ---- TONES / NOISE, a frame per workgroup: filter + in-LDS transform + bin selection (fft_kernels.hip) ----
    bool lds = false;
    bool blue = false;                         // ... through Bluestein's identity (fft holds chirp, transform, twiddles)
    DevBuf<float2> d_tw;                       // w_nfft^k
    DevBuf<int> d_sel;                         // TONES: bin of every output column
    DevBuf<float2> d_carry[kStageSets];        // the samples a call leaves over (at most taps*nfft)
    // what launch_pfb_lds chose call by call (gsdr_demod_describe: pfb_last, pfb_calls)
    PfbChoice last{};
    int last_frames = -1;                      // frames of the last call; -1: no call yet
    unsigned long long calls_cu = 0, calls_lds = 0, calls_direct[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long calls_teams = 0, calls_runs = 0, calls_short = 0;   // with teams, G >= 2, a short last run
    // ---- TONES / NOISE, mean of avg_k consecutive frames (gsdr_demod_set_frame_average; 1: off, nothing below is used) ----
    int avg_k = 1, avg_kind = GSDR_AVERAGE_COMPLEX;
    int avg_count = 0;                         // frames of the open group, summed in d_avg_acc[avg_seq % 2]
    unsigned long long avg_seq = 0;            // launches of pfb_average_kernel so far: they read one accumulator, write the other
    DevBuf<float2> d_avg_frames;               // [batching][channels]: where the PFB writes its frames instead of `out`
    DevBuf<float2> d_avg_acc[2];               // [channels] each
};

// ---- CHIRP ----
struct ChirpState {
    ChirpShape cs{};                   // (several chirps: chirp 0; num_steps, length and the period are common to all)
    int chirps = 1;                    // > 1: a GSDR_CREATE_MULTI_CHIRP handle; mc holds f0 and chirpness of every chirp
    MultiChirp mc{};
    int ppt = 0;
    gsdr_vna_helper vh{};
    DevBuf<float> d_profile;
    DevBuf<float2> d_part;             // partial sums of chirp_lockin_split_kernel (kChirpPartials float2)
    DevBuf<float2> d_carry[2];
    int parity = 0;
    int carry_len = 0;                 // spare_size (ref :54,:369)
    unsigned long long last_index = 0; // ref :217,:355
    unsigned long long calls[3] = {0, 0, 0};   // calls of this handle by the form that ran (gsdr::ChirpForm)
    long long parts = 1;               // waves per point of the last call (> 1: it was split)
};

// ---- profiling ----
struct Profile {
    bool on = false;
    int every = 1;                     // time every n-th launch (an event pair costs ~3 us of stream time)
    unsigned long long seen = 0;
    std::vector<std::pair<Event, Event>> ev_pool;
    size_t ev_used = 0;
};

}  // namespace rx
}  // namespace gsdr

struct gsdr_demod {
    gsdr::Switches sw;      // the GSDR_* switches, read when the handle was created
    int mode = GSDR_NODSP;
    int device = -1;
    std::string err;
    // Every d_* buffer, stream and event below is an owner (dev_owner.h) and is released by `delete`.  gsdr_demod_close
    // synchronises the streams first -- the one ordering that matters -- so the order among the releases is not
    // observable; the streams are declared in front of everything else all the same (`pl` holds its own in front of its
    // slots and events), so that the buffers and events go before them and `stream` goes last.  (The caller's streams
    // in `dirty` are not the handle's and stay raw.)
    gsdr::Stream stream;
    gsdr::rx::Pipeline pl;

    int N = 0;              // channels = wave_type.size()
    long long L = 0;        // buffer_len
    long long decim = 0;
    long long capacity = 0; // max samples process() can return
    float fcut = 0.f;
    int cus = 256;                     // compute units of the device (grid of the widening kernel)
    std::vector<float> window;         // taps (DIRECT) / PFB window / VNA profile, real part
    // sc16 input (gsdr_demod_*_sc16): the scale of the widening; the buffer gsdr_demod_process_device_sc16 widens the
    // caller's samples into (the host-pointer entries have upload buffers of their own: host.d_in16, Slot::d_in16)
    float sc16_scale = 1.0f / 32768.0f;
    gsdr::DevBuf<float2> d_wide;
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
    // ---- the parameters this handle was created with (gsdr_demod_prepare's rehearsal builds a twin) ----
    gsdr_param_c pc{};
    unsigned flags = 0;                              // GSDR_CREATE_* of gsdr_demod_create_ex (the twin takes the same)
    std::vector<int> pc_wave_type, pc_freq, pc_chirp_f, pc_swipe_s;
    std::vector<float> pc_chirp_t;
    const char *kernel_name = "none";

    gsdr::rx::HostEntry host;
    gsdr::rx::DdcState ddc;
    gsdr::rx::MfmaState mx;
    gsdr::rx::PfbState pfb;
    gsdr::rx::ChirpState ch;
    gsdr::rx::Profile prof;
};

namespace gsdr {
namespace rx {

// ---- demod.cpp ----
gsdr_demod *demod_create(const gsdr_param_c *p, const Switches &sw, unsigned flags);
int refuse(gsdr_demod *h, const char *msg);                   // the message into h->err; -1
// What every entry that takes a buffer starts with: -1 without a handle, "null buffer" into the handle without a buffer
int refuse_null(gsdr_demod *h, const void *in, const void *out);
// Orders `st` behind every stream in h->dirty (keep_pipeline: but for the compute streams of the pipeline, which its
// protocol orders), and forgets those.
int join_streams(gsdr_demod *h, hipStream_t st, bool keep_pipeline);
int record_begin(gsdr_demod *h, hipStream_t st, hipEvent_t *stop);
int staging_pair(gsdr_demod *h);
int process_device_body(gsdr_demod *h, const float2 *in, const gsdr_sc16 *in16, float2 *wide, float2 *out, hipStream_t st);

// ---- demod_pipeline.cpp ----
// the staging pass of an overlapped call is done: the next call's pass waits for this
int record_staged(gsdr_demod *h, hipStream_t st);

// ---- demod_ddc.cpp ----
int setup_direct(gsdr_demod *h, const gsdr_param_c *p);
int setup_ddc_common(gsdr_demod *h, int F, int M, unsigned rate, const std::vector<long long> &tone, int max_nblk,
                     bool allow_flat = true);
int setup_mfma(gsdr_demod *h, bool direct, const std::vector<long long> &tone, long long max_rows, long long t_max);
int autotune_chunks(gsdr_demod *h, int nblk);
int pick_chunks(const gsdr_demod *h, int nblk);
DdcLaunch ddc_launch_of(const gsdr_demod *h);
void finish_shape(DdcShape &sh);
// absmax pass over `in` + ddc_mfma_kernel over `nout` rows.  DIRECT: raw == nullptr,
// the rows read `in` (and its head/tail copies).  TONES: the pass also appends
// `in` to the raw window at raw_new0 and the rows read raw[0 .. nx).
int enqueue_mfma(gsdr_demod *h, const float2 *in, float2 *raw, long long raw_new0, long long nx, int nout, unsigned idx_base,
                 float2 *out, hipStream_t st, const float2 *spare_src = nullptr, long long spare_n = 0);
int enqueue_direct(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st);
void describe_mfma(const gsdr_demod *h, std::string &s);     // (the describe_* append their part of gsdr_demod_describe's text)

// ---- demod_pfb.cpp ----
int setup_pfb(gsdr_demod *h, const gsdr_param_c *p);
int enqueue_pfb(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st);
int enqueue_pfb_average(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st);
void describe_pfb_lds(const gsdr_demod *h, std::string &s);
void describe_frame_average(const gsdr_demod *h, std::string &s);

// ---- demod_chirp.cpp ----
int setup_chirp(gsdr_demod *h, const gsdr_param_c *p);
int enqueue_chirp(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st);
void describe_chirp(const gsdr_demod *h, std::string &s);

}  // namespace rx
}  // namespace gsdr

#endif
