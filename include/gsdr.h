/*
 * gsdr.h -- C ABI of libgsdr.so, the MI355X-native RX demodulation engine.
 *
 * Drop-in boundary for the demodulation path of zjc263/GPU_SDR
 * (RX_buffer_demodulator, /root/reference/headers/USRP_demodulator.hpp:13-33).
 * Plain pointers and sizes only; no HIP, torch or C++ types cross this header.
 * The C++ class of the same name that the reference's server code compiles
 * against is provided header-only on top of this ABI in
 * include/USRP_demodulator.hpp; INTEGRATION.md shows the binding.
 *
 * Citations "ref:" are relative to /root/reference.
 */
#ifndef GSDR_H
#define GSDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSDR_ABI_VERSION 1

/* complex64, layout-identical to CUDA/HIP float2 (x = re, y = im).
 * ref: every buffer in headers/USRP_demodulator.hpp is float2*. */
typedef struct gsdr_c64 { float x, y; } gsdr_c64;
/* interleaved 16-bit I/Q as a radio delivers it (UHD "sc16": I first), 4 bytes per sample */
typedef struct gsdr_sc16 { int16_t i, q; } gsdr_sc16;

/* ref: headers/USRP_server_settings.hpp:114  enum w_type */
enum gsdr_w_type {
    GSDR_TONES = 0, GSDR_CHIRP = 1, GSDR_NOISE = 2, GSDR_RAMP = 3,
    GSDR_NODSP = 4, GSDR_SWONLY = 5, GSDR_DIRECT = 6
};

/* Flattened view of the fields of `struct param` that the demodulator reads.
 * ref: headers/USRP_server_settings.hpp:130-167 (same names, same meaning).
 * Vectors become (pointer, count) pairs; the pointers are only read during
 * gsdr_demod_create(). */
typedef struct gsdr_param_c {
    int rate;                 /* param::rate  [samples/s]                     */
    long long decim;          /* param::decim (size_t)                        */
    int fft_tones;            /* param::fft_tones                             */
    long long pf_average;     /* param::pf_average (size_t)                   */
    long long buffer_len;     /* param::buffer_len (size_t)                   */
    const int *wave_type;     /* param::wave_type, values of gsdr_w_type      */
    int n_wave_type;
    const int *freq;          /* param::freq [Hz]                             */
    int n_freq;
    const float *chirp_t;     /* param::chirp_t [s]                           */
    int n_chirp_t;
    const int *chirp_f;       /* param::chirp_f [Hz]                          */
    int n_chirp_f;
    const int *swipe_s;       /* param::swipe_s                               */
    int n_swipe_s;
    int device_index;         /* server_settings::GPU_device_index
                                 (ref: USRP_server_settings.hpp:197); -1 =
                                 keep the calling thread's current device     */
} gsdr_param_c;

typedef struct gsdr_demod gsdr_demod;

/* ---- demodulator lifecycle (replaces RX_buffer_demodulator) ------------- */

/* ref: RX_buffer_demodulator::RX_buffer_demodulator, cpp/USRP_demodulator.cpp:7-327.
 * Returns NULL on failure; gsdr_last_error(NULL) then holds the reason.  Where
 * the reference calls exit(-1) (mixed wave types :36-39, more than one CHIRP
 * :31-34, unsupported type :322-325) this returns NULL with the same message. */
gsdr_demod *gsdr_demod_create(const gsdr_param_c *p);

/* ---- several chirps in one handle (an extension: the reference announces it and exits, ref:
 * cpp/USRP_demodulator.cpp:31-34, cpp/USRP_buffer_generator.cpp:26-29) -------------------------------------------
 * gsdr_demod_create_ex / gsdr_txgen_create_ex take creation flags.  flags == 0 is exactly gsdr_demod_create /
 * gsdr_txgen_create, refusals included; a bit this header does not define is refused before anything else ("unknown
 * creation flag").  GSDR_CREATE_MULTI_CHIRP lifts the "Multiple chirp ..." refusal: wave_type = CHIRP x C, 1 <= C <=
 * GSDR_MULTI_CHIRP_MAX, demodulates (RX) or adds up (TX) C chirps in one pass over the buffer.  C == 1 is the
 * single-chirp handle, launch for launch; mixed wave types stay refused as before.
 *   - freq[c], chirp_f[c]: the span of chirp c; n_freq >= C and n_chirp_f >= C ("CHIRP needs freq[] and chirp_f[] for
 *     every wave_type entry");
 *   - swipe_s, chirp_t: shared, one entry each or C equal ones ("multi-chirp needs one swipe_s and one chirp_t for all
 *     chirps"): num_steps, length, the samples per point, the period and the running index are common, f0 and the
 *     chirpness per chirp (gsdr_chirp_derive for RX, gsdr_chirp_derive_tx for TX).
 * All of this is refused before the device is touched.
 * RX: gsdr_demod_channels() is C, rows are [point][chirp] ([sample][chirp] with decim == 0), a call returns valid * C
 * (buffer_len * C), gsdr_demod_out_capacity() is (buffer_len / ppt + 1) * C (buffer_len * C).  Column c is what a
 * single-CHIRP handle made from (rate, freq[c], chirp_f[c], swipe_s, chirp_t, decim, buffer_len) returns for the same
 * stream of buffers -- same lengths, same carry, same index, call by call; the carry of raw samples and the window
 * bookkeeping exist once per handle.  Every RX entry serves such a handle (process, process_device, submit,
 * submit_device, wait, their sc16 forms, prepare -- the rehearsal twin is made with the same flags --, profile_*), under
 * the extents contract below; gsdr_demod_set_frame_average stays TONES / NOISE only.  gsdr_demod_kernel_name reports
 * chirp_multi_lockin_kernel / chirp_multi_demod_kernel when C > 1, gsdr_demod_describe adds "chirps": C.
 * TX: x[s] = term_0[s] + term_1[s] + ... + term_(C-1)[s], term_c the sample gsdr_source_chirp writes for chirp c with
 * scale ampl[c] (1 without ampl): (fl32(sin_c * scale_c), fl32(-cos_c * scale_c)).  The terms are added in chirp order
 * starting FROM term_0, real and imaginary part apart, every addition one IEEE single-precision operation, nothing fused.
 * The sc16 entries are that sum narrowed, bit for bit, clipped components counted on the sum.  get, get_device and their
 * sc16 forms serve such a generator (the running index wraps at num_steps * length); gsdr_txgen_get_ptr* stays TONES only.
 * gsdr_source_multichirp[_sc16] is the kernel on its own: n_chirps in [1, GSDR_MULTI_CHIRP_MAX], every cp[c] with the
 * same num_steps and length (both >= 1), scale[c] per chirp (host arrays, read during the call), device out_dev as for
 * gsdr_source_chirp[_sc16]; asynchronous on hip_stream; -1 with the reason in gsdr_last_error(NULL).  n == 0 touches
 * nothing, not even the pointers. */
#define GSDR_CREATE_MULTI_CHIRP 1u
#define GSDR_MULTI_CHIRP_MAX 16
gsdr_demod *gsdr_demod_create_ex(const gsdr_param_c *p, unsigned flags);

/* ref: RX_buffer_demodulator::process, cpp/USRP_demodulator.cpp:330.
 * in_host : buffer_len complex64 (host, pinned or pageable), not modified.
 * out_host: room for gsdr_demod_out_capacity() complex64.
 * Synchronous like the reference (returns after the stream has drained).
 * Returns the number of valid complex samples written to out_host
 * ([sample][channel] interleaved), or -1 on a device error. */
int gsdr_demod_process(gsdr_demod *h, const gsdr_c64 *in_host, gsdr_c64 *out_host);

/* Same contract with DEVICE pointers, enqueued on `hip_stream` (a hipStream_t
 * passed as void*; NULL = HIP's null stream, as in every HIP call) and NOT
 * synchronised: the caller orders it against the producer of in_dev and the
 * consumer of out_dev through that stream.
 * The returned length is known on the host before the kernels finish.  This
 * is the entry the synthetic in-HBM source and bench.py use.
 * Consecutive calls may use different streams, and may be mixed with the
 * submit entries below: the state a call inherits (FIR carry, NCO index, raw
 * windows) is ordered on the device -- a call on another stream than its
 * predecessor first waits for it (one event; nothing on the usual path).
 * For that the handle remembers the stream of a call until the NEXT call on
 * the handle has been made: a stream passed here must stay alive that long
 * (or until gsdr_demod_close()); HIP itself faults on a destroyed stream. */
int gsdr_demod_process_device(gsdr_demod *h, const gsdr_c64 *in_dev,
                              gsdr_c64 *out_dev, void *hip_stream);

/* Pipelined host-pointer entry (an extension: the reference's process() is
 * synchronous and serialises H2D, compute and D2H of successive buffers, ref:
 * cpp/USRP_demodulator.cpp:393,462,555).  gsdr_demod_submit() enqueues the
 * upload on a copy stream, the kernels on the compute stream and the download
 * on a third stream, linked by events, and returns at once; up to
 * GSDR_PIPELINE_DEPTH buffers may be outstanding.  gsdr_demod_wait() blocks
 * until the OLDEST outstanding buffer is complete in its out_host and returns
 * its valid length (-1: device error, -2: nothing outstanding).  in_host and
 * out_host must stay valid until that wait returns and should be pinned
 * (hipHostMalloc), otherwise the copies degrade to synchronous ones.
 * Do not mix with gsdr_demod_process() while buffers are outstanding. */
#define GSDR_PIPELINE_DEPTH 4
int gsdr_demod_submit(gsdr_demod *h, const gsdr_c64 *in_host, gsdr_c64 *out_host);
int gsdr_demod_wait(gsdr_demod *h);
/* The same pipeline for a device-resident source (a synthetic generator, a GPU-direct
 * receiver): in_dev must be complete when the call is made, out_dev must be a different
 * buffer for every outstanding call; gsdr_demod_wait() returns when out_dev is complete.
 * Both submit entries run the DIRECT and TONES/NOISE kernels of consecutive buffers on
 * three streams in turn: the next buffer starts on the compute units the last workgroups of this one
 * leave idle (GSDR_PIPE_OVERLAP=0: strictly one after the other). */
int gsdr_demod_submit_device(gsdr_demod *h, const gsdr_c64 *in_dev, gsdr_c64 *out_dev);

/* Extents and alignment of device pointers -- gsdr_demod_process_device, gsdr_demod_submit_device and their sc16
 * forms below:
 *  - exactly buffer_len samples are read from in_dev: in_dev[0, buffer_len).  Nothing in front of it or behind it is
 *    read, whatever the decimation, the tile sizes of the kernel or the padding of its windows (where a kernel
 *    reads in whole blocks, the rows that would leave the buffer are served from copies the handle owns), and
 *    in_dev is never written;
 *  - only out_dev[0, gsdr_demod_out_capacity()) is written, and the returned length n is <= that capacity;
 *    out_dev[0, n) is valid, what a call leaves in out_dev[n, capacity) is unspecified;
 *  - the pointers need their natural alignment only: 8 bytes for gsdr_c64, 4 bytes for gsdr_sc16 input.  They may
 *    point anywhere into a larger allocation, and the output does not depend, bit for bit, on where they point or on
 *    what lies around the buffers.
 * (What tests/test_gpu_extents.py can and cannot see of this: DESIGN.md section 3.)
 * The writers further down (gsdr_txgen_get_device, gsdr_txgen_tones_fill, gsdr_source_tones, gsdr_source_chirp,
 * gsdr_source_multichirp)
 * write exactly the n (gsdr_txgen_get_device: buffer_len) samples they are asked for, to an 8-byte aligned out_dev.
 * Their sc16 forms (gsdr_txgen_get_device_sc16, gsdr_txgen_tones_fill_sc16, gsdr_source_chirp_sc16,
 * gsdr_source_multichirp_sc16) and
 * gsdr_narrow_sc16_device write exactly n (buffer_len) samples of gsdr_sc16 to an out_dev that needs 4-byte alignment
 * only and may point anywhere into a larger allocation: nothing in front of it or behind it is written, and the output
 * does not depend on where it points. */

/* Creates now what the entries above would otherwise create on first use (device
 * staging buffers of the host-pointer entries, the streams, events and per-slot
 * buffers of the pipelined ones), so that the first buffers of a measurement are not
 * late: the reference's constructor allocates everything up front as well (ref:
 * cpp/USRP_demodulator.cpp:59-119), and include/USRP_demodulator.hpp calls this from
 * its constructor.  `what` is a bit set; returns 0 or -1. */
#define GSDR_PREPARE_HOST 1           /* gsdr_demod_process                  */
#define GSDR_PREPARE_PIPELINE 2       /* gsdr_demod_submit_device / _wait    */
#define GSDR_PREPARE_PIPELINE_HOST 4  /* gsdr_demod_submit / _wait           */
/* GSDR_PREPARE_REHEARSE: also runs a throw-away twin of this demodulator (same parameters) through a
 * few buffers of zeros on every entry, then closes it.  The first launches of a kernel, the first
 * asynchronous copies from a pinned buffer and the first uses of a stream cost the process 5 - 7 ms
 * each, once (measured: calls 0, 1 and 6 of the first handle's submit() loop; later handles of the
 * process show none): the rehearsal pays them at set-up time, so that the first packets are not late.
 * The state of `h` itself (carry, NCO phase, call count) is untouched. */
#define GSDR_PREPARE_REHEARSE 8
/* GSDR_PREPARE_SC16: also what the sc16 entries below create on first use -- the half-size upload buffers of the
 * host-pointer entries the other bits name, the input buffers of the pipeline slots (gsdr_demod_submit_device_sc16)
 * and the buffer gsdr_demod_process_device_sc16 widens into; with GSDR_PREPARE_REHEARSE the twin also goes through the
 * sc16 host-pointer entries named, so that the first launch of the widening kernel is not paid by the first packet.
 * Without this bit nothing of that is allocated. */
#define GSDR_PREPARE_SC16 16
int gsdr_demod_prepare(gsdr_demod *h, int what);

/* ---- sc16 input (an extension: the reference has UHD convert to fc32 on the host, ref:
 * cpp/USRP_hardware_manager.cpp:764-816) -------------------------------------------------
 * Every RX entry above in a form that takes interleaved int16 I/Q.  Each is exactly "widen, then the complex64
 * entry": sample k becomes (float(i) * scale, float(q) * scale) -- an exact conversion and one IEEE single-precision
 * multiply, nothing fused into it -- and the demodulation that follows is the one of the complex64 entry, kernel
 * for kernel.  Contracts, return values and ordering rules are those of the complex64 entries; both kinds of call
 * may be mixed freely on one handle (the stream state does not know the difference).  The host-pointer entries
 * upload 4 bytes per sample instead of 8 and widen on the device (NODSP: gsdr_demod_process_sc16 widens on the
 * host, the device entries widen straight into out_dev).
 * The scale is a property of the handle: 2^-15 by default (exact: full scale maps to [-1, 1)); it must be finite
 * and > 0, otherwise gsdr_demod_set_sc16_scale returns -1, leaves a message in gsdr_last_error(h) and keeps the
 * old value.  A caller who wants the values their UHD would have delivered as fc32 sets the factor that UHD applies. */
int gsdr_demod_set_sc16_scale(gsdr_demod *h, float scale);
float gsdr_demod_sc16_scale(const gsdr_demod *h);
int gsdr_demod_process_sc16(gsdr_demod *h, const gsdr_sc16 *in_host, gsdr_c64 *out_host);
int gsdr_demod_process_device_sc16(gsdr_demod *h, const gsdr_sc16 *in_dev, gsdr_c64 *out_dev, void *hip_stream);
int gsdr_demod_submit_sc16(gsdr_demod *h, const gsdr_sc16 *in_host, gsdr_c64 *out_host);
int gsdr_demod_submit_device_sc16(gsdr_demod *h, const gsdr_sc16 *in_dev, gsdr_c64 *out_dev);
/* The widening on its own.  _device: in_dev (4-byte aligned) and out_dev (8-byte aligned) are device pointers to n
 * samples, the kernel is enqueued on hip_stream and not synchronised; returns 0, or -1 with the reason in
 * gsdr_last_error(NULL).  _host: the same arithmetic on the CPU, bit for bit (needs no GPU). */
int gsdr_widen_sc16_device(const gsdr_sc16 *in_dev, gsdr_c64 *out_dev, long long n, float scale, void *hip_stream);
void gsdr_widen_sc16_host(const gsdr_sc16 *in, gsdr_c64 *out, long long n, float scale);

/* ---- sc16 output (an extension: the reference hands fc32 to UHD, which converts on the host) -----------------
 * A radio takes sc16 on the wire.  Every TX generator entry further down has a form that writes gsdr_sc16 (I first,
 * 4 bytes per sample) straight from the kernel that made the sample: half the bytes to store and to copy, and no
 * conversion pass on the host.  Each is exactly "the complex64 entry, then narrow", bit for bit, for any start and n.
 * Narrowing a float32 component c with a float32 gain is three steps, every one a single IEEE single-precision
 * operation, nothing fused:
 *   1. v = fl32(c * gain);
 *   2. r = v rounded to the nearest integer, ties to even;
 *   3. q = 0 if v is NaN;  32767 if r > 32767 (+Inf included);  -32768 if r < -32768 (-Inf included);  else (int16) r.
 * (Round to nearest even plus saturation is what UHD's SIMD fc32 -> sc16 converters do.)  A component is CLIPPED when
 * v is NaN, r > 32767 or r < -32768; r == -32768 is representable and no clip.  In numpy terms:
 * np.rint(x.view(float32) * float32(gain)), clipped to [-32768, 32767], NaN -> 0, .astype(int16).
 * The narrowing on its own.  _device: in_dev (8-byte aligned) and out_dev (4-byte aligned, anywhere in a larger
 * allocation) are device pointers to n samples; exactly n samples are written; gain must be finite and > 0; when
 * clipped_dev is given (8-byte aligned device memory) the kernel ADDS the number of clipped components of the call to
 * it -- at most one atomic per wave, none for a wave that clipped nothing.  Enqueued on hip_stream, not synchronised;
 * returns 0, or -1 with the reason in gsdr_last_error(NULL).  _host: the same arithmetic on the CPU, bit for bit (needs
 * no GPU; any gain is taken as it is); returns the number of clipped components.  n == 0 touches nothing, not even
 * the pointers. */
int gsdr_narrow_sc16_device(const gsdr_c64 *in_dev, gsdr_sc16 *out_dev, long long n, float gain,
                            unsigned long long *clipped_dev, void *hip_stream);
long long gsdr_narrow_sc16_host(const gsdr_c64 *in, gsdr_sc16 *out, long long n, float gain);

/* ---- mean of k consecutive frames, TONES and NOISE (an extension: what the reference's decimate_spectra /
 * decimate_pfb intend and do not deliver, ref: cpp/kernels.cu:704-790, cpp/USRP_demodulator.cpp:511-534,593-624;
 * gsdr_demod_create() keeps refusing param::decim > 0 for these modes) ------------------------------------------
 * A property of the handle like the sc16 scale: with k > 1 every RX entry returns, instead of one row per frame, one
 * row per GROUP of k consecutive frames -- group g is frames [g*k, (g+1)*k) counted from the creation of the handle --
 * and a call returns channels x the number of groups that complete in it (possibly 0), rows [group][channel].  The
 * open group is carried to the next call, on whatever entry or stream that call is made.
 * Arithmetic, per channel, real and imaginary part separately, every operation one IEEE single-precision operation
 * rounded to nearest and nothing fused:  acc = t_0 (not 0 + t_0);  acc = acc + t_j in frame order;  when the k-th
 * frame is in, the row is acc * (1.0f / k).  GSDR_AVERAGE_COMPLEX: t_j is the frame value.  GSDR_AVERAGE_POWER:
 * t_j.x = re*re + im*im (two products, one sum), t_j.y = 0.  The result does not depend on where the stream is cut
 * into buffers, and an Inf or NaN reaches exactly the groups that hold it.
 * gsdr_demod_set_frame_average: TONES and NOISE handles, 1 <= k <= GSDR_FRAME_AVERAGE_MAX, before the first buffer
 * has gone through the handle and with nothing outstanding; otherwise -1, a message in gsdr_last_error(h), and the
 * old setting stays.  It allocates what it needs at once, and gsdr_demod_out_capacity() becomes
 * channels * ceil(batching / k).  k == 1 is "off": the handle runs launch for launch as if the setter had never been
 * called.  gsdr_demod_frame_average returns k (1 = off; 0 for a NULL handle) and the kind through *kind. */
#define GSDR_AVERAGE_COMPLEX 0   /* mean of the complex frames */
#define GSDR_AVERAGE_POWER   1   /* mean of |X|^2 in .x, 0 in .y: what a noise spectrum needs (a complex mean of noise tends to 0) */
#define GSDR_FRAME_AVERAGE_MAX 1048576
int gsdr_demod_set_frame_average(gsdr_demod *h, int k, int kind);
int gsdr_demod_frame_average(const gsdr_demod *h, int *kind /* may be NULL */);
/* The averaging on its own.  frames: [n_frames][n_ch]; count (0 <= count < k) frames of the open group are already
 * summed in acc_in[n_ch] (not read when count == 0); writes the completed groups to out ([rows][n_ch]) and the new open
 * group's partial sums to acc_out[n_ch] (zeros when none is open); acc_in and acc_out must not overlap.  Returns
 * rows = (count + n_frames) / k, or -1 (gsdr_last_error(NULL)).  _device: device pointers, 8-byte aligned, one kernel
 * enqueued on hip_stream and not synchronised; _host: the same bits on the CPU (needs no GPU). */
int gsdr_frame_average_device(const gsdr_c64 *frames_dev, int n_frames, int n_ch, int k, int kind, int count,
                              const gsdr_c64 *acc_in_dev, gsdr_c64 *acc_out_dev, gsdr_c64 *out_dev, void *hip_stream);
int gsdr_frame_average_host(const gsdr_c64 *frames, int n_frames, int n_ch, int k, int kind, int count,
                            const gsdr_c64 *acc_in, gsdr_c64 *acc_out, gsdr_c64 *out);

/* ref: RX_buffer_demodulator::close, cpp/USRP_demodulator.cpp:333 (+ :466-698).
 * Frees every device allocation and the stream, then the handle itself. */
void gsdr_demod_close(gsdr_demod *h);

/* Last error text of a handle, or of the calling thread's last failed
 * gsdr_demod_create() when h == NULL.  Never NULL. */
const char *gsdr_last_error(const gsdr_demod *h);

/* ---- introspection ------------------------------------------------------ */
int gsdr_abi_version(void);
/* "abi 1; arch gfx950; timing_build 0".  timing_build 1 marks an ablation build
 * (-DGSDR_TIMING_BUILD, scratch/ only) whose kernels can be told to skip work;
 * the shipped library is always 0 and bench.py refuses anything else. */
const char *gsdr_build_info(void);
/* Does nothing.  The GSDR_* environment switches (A/B runs, kernel variants in the tests) are read
 * when a handle is created, and the handle keeps them; set them before gsdr_demod_create().  Kept for callers
 * built against older headers, where it made later launches read some of the switches again. */
void gsdr_reload_env(void);
/* One-line JSON object describing the engine this handle resolved to: mode,
 * kernel (that of the last launch, see gsdr_demod_kernel_name), kernel family,
 * row tiles per workgroup, pipeline streams, and every GSDR_* environment
 * variable that is set in the process (the handle itself read the switches
 * when it was created).  CHIRP handles add "chirp_calls": {"plain": a, "split": b, "generic": c}, this handle's calls
 * so far by the form that ran (gsdr_chirp_lockin_plan; undecimated calls are plain or generic), and "chirp_parts",
 * the waves per point of the last call.  TONES / NOISE handles that run inside the LDS add "pfb_last", the shape of the last
 * call as gsdr_pfb_plan gives it -- {"kernel", "threads", "G", "direct", "dir_s", "dir_gs", "col", "teams", "twl", "lds",
 * "frames"}, kernel "none" and frames -1 before the first call -- and "pfb_calls", the calls so far: {"pfb_cu_kernel": a,
 * "pfb_lds_kernel": b, "direct": [six counts, the run kernel's calls by filter variant 0 - 5], "teams": with teams,
 * "runs": with G >= 2, "short_last_run": with a frame count that is no multiple of G}.  Returns the text length (truncated to cap-1
 * characters + NUL). */
int gsdr_demod_describe(const gsdr_demod *h, char *buf, int cap);
/* gsdr_w_type actually dispatched (ref: USRP_demodulator.cpp:19-25,56). */
int gsdr_demod_mode(const gsdr_demod *h);
/* parameters->wave_type.size(), what rx_single_link stores in
 * RX_wrapper.channels (ref: cpp/USRP_server_link_threads.cpp:657). */
int gsdr_demod_channels(const gsdr_demod *h);
/* Upper bound of the value process() can return for this configuration. */
long long gsdr_demod_out_capacity(const gsdr_demod *h);
/* RX_buffer_demodulator::fcut (ref: USRP_demodulator.cpp:131). */
float gsdr_demod_fcut(const gsdr_demod *h);
/* Copies the FIR taps / PFB window / VNA profile in use (real part) into w
 * (up to cap floats); returns its length. */
int gsdr_demod_get_window(const gsdr_demod *h, float *w, int cap);
/* TONES: copies the tone->FFT-bin table (ref: USRP_demodulator.cpp:726-733). */
int gsdr_demod_get_bins(const gsdr_demod *h, int *bins, int cap);

/* Per-kernel device timing of the dominant kernel with hipEvents recorded on
 * the launch stream.  enable != 0 starts a fresh accumulation; enable = n > 1
 * times every n-th launch only (a pair of events costs a few microseconds of
 * stream time, which a throughput measurement should not carry on every step). */
void gsdr_demod_profile_enable(gsdr_demod *h, int enable);
/* Synchronises the recorded events; returns the number of timed launches and
 * their summed duration in milliseconds. */
int gsdr_demod_profile_read(gsdr_demod *h, double *total_ms);
/* Name of the kernel that carried the last call (as rocprofv3 reports it; the
 * CHIRP lock-in reports chirp_lockin_kernel for all its variants, a handle of
 * several chirps chirp_multi_lockin_kernel or chirp_multi_demod_kernel); before
 * the first call, the one a call of buffer_len samples runs. */
const char *gsdr_demod_kernel_name(const gsdr_demod *h);

/* ---- host-side pieces of the path (usable without a GPU) ---------------- */
/* ref: make_sinc_window, cpp/kernels.cu:258-310 (real part; imag is 0). */
void gsdr_make_sinc_window(int length, float fc, float *w);
/* ref: make_flat_window, cpp/kernels.cu:208-253. */
void gsdr_make_flat_window(int length, int side, float *w);

/* ref: class buffer_helper, cpp/USRP_server_memory_management.cpp:104-156,
 * headers/USRP_server_memory_management.hpp:77-101 (same field names). */
typedef struct gsdr_buffer_helper {
    int n_tones, eff_length, buffer_len, average, n_eff_tones;
    int new_0, copy_size, current_batch, spare_samples, spare_begin;
} gsdr_buffer_helper;
void gsdr_buffer_helper_init(gsdr_buffer_helper *b, int n_tones, int buffer_len,
                             int average, int n_eff_tones);
void gsdr_buffer_helper_update(gsdr_buffer_helper *b);

/* ref: class VNA_decimator_helper, cpp/USRP_server_memory_management.cpp:30-56. */
typedef struct gsdr_vna_helper {
    int valid_size, new0, total_len, spare_begin, ppt, buffer_len;
} gsdr_vna_helper;
void gsdr_vna_helper_init(gsdr_vna_helper *v, int ppt, int buffer_len);
void gsdr_vna_helper_update(gsdr_vna_helper *v);

/* ref: upload_multitone_parameters, cpp/USRP_demodulator.cpp:722-733.
 * bins[u] = -1 when no bin matches (the reference leaves it uninitialised). */
void gsdr_pfb_tone_bins(int rate, int fft_tones, const int *freq, int n, int *bins);
/* ref: cpp/USRP_demodulator.cpp:706 */
int gsdr_pfb_batching(long long buffer_len, int fft_tones, long long pf_average);
/* The radix stages of the in-LDS transform of an fft_tones-point frame (TONES / NOISE as one launch per buffer:
 * polyphase filter + FFT inside the LDS + bin selection): writes the radices into radices[0..15] in stage order and
 * returns their number, or -1 when the length has no such plan (more than 8192 points, a prime factor above 127).
 * Such lengths up to 4096 points still run inside the LDS, through Bluestein's identity at the padded length
 * 2^ceil(log2(2 fft_tones - 1)); longer ones through the global-memory FFT stages -- for TONES and NOISE alike
 * (round 3: every TONES frame length takes filter + FFT + selection, as the reference's cufftPlanMany takes any
 * fft_tones).  Host only.  Replaces the reference's cufftPlanMany for the PFB
 * (ref: cpp/USRP_demodulator.cpp:149-152, :292-295). */
int gsdr_pfb_lds_stages(int fft_tones, int *radices);

/* ref: struct chirp_parameter, headers/kernels.cuh:58-64 and its derivation
 * in cpp/USRP_demodulator.cpp:192-214. */
typedef struct gsdr_chirp_param {
    unsigned long long num_steps, length;
    unsigned int chirpness;
    int f0;
} gsdr_chirp_param;
void gsdr_chirp_derive(int rate, int freq0, int chirp_f, int swipe_s,
                       float chirp_t, gsdr_chirp_param *cp);
/* The TX side's own derivation (ref: cpp/USRP_buffer_generator.cpp:107-129): as above, but a step shorter than
 * one sample also resets num_steps to chirp_t * rate before the slope is taken from it (:118-125). */
void gsdr_chirp_derive_tx(int rate, int freq0, int chirp_f, int swipe_s,
                          float chirp_t, gsdr_chirp_param *cp);

/* Which form of the lock-in a CHIRP call takes -- the rule the library's own launchers ask, host only.  The call
 * integrates `valid` points of ppt samples each, the first at chirp index index0, for `chirps` chirps at once:
 *   PLAIN    a wave per point (the 32-bit fast kernel);
 *   SPLIT    the 256-sample stretches of a point dealt to *parts waves of *per_part stretches (the last may hold
 *            fewer), their partial sums -- valid * parts * chirps of partial_cap slots -- added in fixed order:
 *            few points (valid <= 512) of at least 16 stretches, at least four stretches per wave; split == 0
 *            (GSDR_CHIRP_SPLIT=0) never;
 *   GENERIC  the 64-bit kernel: length >= 2^23, num_steps >= 2^31 - 1, a period of num_steps * length >= 2^32 - 1,
 *            or points that are not whole steps starting on a step boundary (ppt % length, index0 % length).
 * PLAIN: *parts = 1, *per_part = every stretch of a point; GENERIC: 1 and 0.  parts and per_part may be NULL.
 * Returns the form, or -1 for arguments no handle has (a zero or overflowing sweep, ppt, valid or chirps < 1,
 * chirps > GSDR_MULTI_CHIRP_MAX, partial_cap < 0).  A handle uses partial_cap 16384 and reports the forms its
 * calls took in gsdr_demod_describe: "chirp_calls" and "chirp_parts". */
#define GSDR_CHIRP_FORM_PLAIN 0
#define GSDR_CHIRP_FORM_SPLIT 1
#define GSDR_CHIRP_FORM_GENERIC 2
int gsdr_chirp_lockin_plan(unsigned long long num_steps, unsigned long long length, long long ppt,
                           unsigned long long index0, int valid, int chirps, int split, int partial_cap, int *parts,
                           int *per_part);

/* The kernel and shape a TONES / NOISE call inside the LDS takes (csrc/pfb_plan.h: the function launch_pfb_lds itself
 * asks, call by call; host only, no GPU needed).  in: frames of nfft points, avg taps, blue_m the padded Bluestein length
 * of the handle or 0 (gsdr_pfb_blue_length), the complete frames of the call, its output columns per frame (NOISE: nfft),
 * the device's compute units, and the GSDR_PFB_* switches by value (unset: pfb_cu -1, pfb_direct 1, pfb_col -1,
 * pfb_cu_nt 0, pfb_teams 1, pfb_radix8 1, pfb_fr 0, pfb_wide -1).  out: cu 1 pfb_cu_kernel (a run of G consecutive
 * frames per workgroup), 0 pfb_lds_kernel (a set of G frames per workgroup; the fields from b_off on are 0 then);
 * direct: the run kernel's filter, 0 staged through the LDS (col 1: column-wise, 0: point-wise), else straight out of
 * global memory with <columns per thread, blocks> registers: 1 <1, 11>, 2 <2, 7>, 5 <3, 5>, 3 <4, 4>, 4 <1, 11> in
 * dir_s groups of threads that own dir_gs consecutive frames each; teams: the frames of a run go through the stages
 * on teams of threads / G threads; len: the transform length (nfft or blue_m) and radices[n_radices] its stages.
 * Returns 0, or -1 for arguments no handle has (a length the LDS kernels do not take, blue_m that is not that length).
 * gsdr_pfb_plan_many: `count` plans in one call (the first refusal ends it with -1). */
typedef struct gsdr_pfb_plan_in {
    int nfft, avg, blue_m, frames, n_out, cus;
    int pfb_cu, pfb_direct, pfb_col, pfb_cu_nt, pfb_teams, pfb_radix8, pfb_fr, pfb_wide;
} gsdr_pfb_plan_in;
typedef struct gsdr_pfb_plan_out {
    int cu, threads, G, twl, lds, b_off, b_len, col, direct, dir_s, dir_gs, teams;
    int len, n_radices, radices[16];
} gsdr_pfb_plan_out;
int gsdr_pfb_plan(const gsdr_pfb_plan_in *in, gsdr_pfb_plan_out *out);
int gsdr_pfb_plan_many(const gsdr_pfb_plan_in *in, int count, gsdr_pfb_plan_out *out);
/* The padded length a handle of nfft points and avg taps runs Bluestein's identity at inside the LDS, 0 when it
 * transforms the frames directly or not in the LDS at all; pfb_bluestein: GSDR_PFB_BLUESTEIN (-1 unset), pfb_direct
 * and pfb_radix8 as above. */
int gsdr_pfb_blue_length(int nfft, int avg, int pfb_bluestein, int pfb_direct, int pfb_radix8);

/* The engine a DIRECT handle takes and the shape of one of its launches (csrc/ddc_plan.h: the functions the handle
 * itself asks when it is created and call by call; host only, no GPU needed).  in: the shape (tones, rate, decim,
 * pf_average, buffer_len) as gsdr_param_c holds it; rows, the output rows of the launch asked about (0: those of a
 * whole buffer, buffer_len / decim, which is what every DIRECT call launches); overlapped 0 an in-order entry
 * (gsdr_demod_process*), 1 a pipelined one (gsdr_demod_submit*); the device's compute units; and the switches by value
 * as read_switches leaves them (unset: ddc_mfma 1, ddc_few 1, ddc_pipe 1, ddc_k -1, ddc_waves 0, ddc_nch 0, mfma_asm 4,
 * mfma_tt 1, mfma_pk 32, mfma_w 4, mfma_rt 0, mfma_w8 1, and -1 for mfma_prec, mfma_3m, mfma_3m_rot, mfma_fold,
 * mfma_fold_products, mfma_wave_tones, mfma_span).
 * out: the engine; for the VALU engines (FLAT, GENERIC, and the table length K of MIX) the sub-block length K with pad
 * and R, the resident waves the grid is sized for, the chunk slots of the tails buffer, and the chunks of a launch of
 * `rows` blocks at the grid ratio 1.3 (a handle on the flat kernel times its own ratio at creation) with the count the
 * balancing started from; for the matrix cores the values gsdr_demod_describe reports -- complex_mac, rotation_blocks,
 * fold, fold_products, wave_tones, span_samples --, whether the handle holds pre-converted images (apart from the
 * 8 GiB cap of an image set, which only the handle applies), whether this launch is pre-converted,
 * row_tiles_per_workgroup and whether it runs the eight-wave kernel; fields of the other engines are 0.  The four
 * thresholds (windows in 32-sample blocks) are given whatever the engine.
 * Returns 0, or -1 for what gsdr_demod_create refuses of these fields (rate, tones, buffer_len < 1; with decim > 0:
 * buffer_len no multiple of decim, pf_average outside [1, 8], decim * pf_average above 2^31 - 1) and for rows outside
 * [0, buffer_len / decim] or cus < 1. */
#define GSDR_DDC_ENGINE_MIX 0        /* decim <= 0: mix_kernel / mix_few_kernel */
#define GSDR_DDC_ENGINE_FEW 1        /* ddc_few_kernel */
#define GSDR_DDC_ENGINE_FLAT 2       /* ddc_flat_kernel */
#define GSDR_DDC_ENGINE_GENERIC 3    /* ddc_kernel */
#define GSDR_DDC_ENGINE_MFMA 4       /* the matrix cores */
typedef struct gsdr_ddc_plan_in {
    long long decim, pf_average, buffer_len;
    int tones, rate, rows, overlapped, cus;
    int ddc_mfma, ddc_few, ddc_pipe, ddc_k, ddc_waves, ddc_nch;
    int mfma_asm, mfma_tt, mfma_pk, mfma_w, mfma_rt, mfma_w8, mfma_prec;
    int mfma_3m, mfma_3m_rot, mfma_fold, mfma_fold_products, mfma_wave_tones, mfma_span;
} gsdr_ddc_plan_in;
typedef struct gsdr_ddc_plan_out {
    int engine;
    int K, pad, R, target_waves, tails_nch, chunks, chunks_want;
    int complex_mac, rotation_blocks, fold, fold_products, wave_tones, span_samples;
    int images, preconverted, row_tiles_per_workgroup, eight_waves;
    int complex_mac_min_blocks, rotation_min_blocks, fold_min_blocks, span128_min_blocks;
} gsdr_ddc_plan_out;
int gsdr_ddc_plan(const gsdr_ddc_plan_in *in, gsdr_ddc_plan_out *out);

/* ---- the pyUSRP command surface (host only) ------------------------------
 * One JSON command per measurement arrives on the async socket, framed by an
 * 8-byte header; results leave on the data socket as 21-byte header + complex64
 * payload (wire formats: SURVEY.md section 9). */
typedef struct gsdr_command gsdr_command;   /* a parsed and checked usrp_param */

/* ref: string2param (cpp/USRP_JSON_interpreter.cpp:19-257) followed by chk_param
 * (:268-439): every key of A_TXRX, B_TXRX, A_RX2, B_RX2 is mandatory; buffer_len
 * 0 or outside [50000, 6000000] -> 1000000; PFB modes force pf_average >= 1 and
 * fft_tones >= 2; |freq|, |chirp_f| <= rate for TONES/CHIRP.  NULL = the command
 * must be nack'ed; gsdr_command_error() says why. */
gsdr_command *gsdr_command_parse(const char *json, int len);
void gsdr_command_free(gsdr_command *c);
const char *gsdr_command_error(void);
int gsdr_command_device(const gsdr_command *c);            /* usrp_param::usrp_number */

/* the fields of `struct param` that gsdr_param_c does not carry
 * (ref: headers/USRP_server_settings.hpp:130-167) */
typedef struct gsdr_antenna_info {
    int mode;                 /* ant_mode: 0 TX, 1 RX, 2 OFF */
    double rf;                /* param::tone                     */
    int gain, bw, tuning_mode;
    long long samples;
    double delay;
    float burst_on, burst_off;
    long long data_mem_mult;
    const float *ampl;
    int n_ampl;
} gsdr_antenna_info;
/* antenna: 0 A_TXRX, 1 B_TXRX, 2 A_RX2, 3 B_RX2 (usrp_param member order).  The
 * pointers inside *p and *info stay valid until gsdr_command_free(). */
int gsdr_command_antenna(const gsdr_command *c, int antenna, gsdr_param_c *p, gsdr_antenna_info *info);

/* ref: server_ack / server_nack (cpp/USRP_JSON_interpreter.cpp:441-457), in the
 * layout boost::property_tree::write_json produces.  Returns the text length. */
int gsdr_server_reply(int is_ack, const char *payload, char *buf, int cap);
/* ref: Async_server::format_header, cpp/USRP_server_network.cpp:497-501: {0, len} */
void gsdr_format_async_header(int message_len, unsigned char out[8]);
/* ref: RX_wrapper without its pointer (headers/USRP_server_settings.hpp:216-224)
 * and Sync_server::format_net_buffer (cpp/USRP_server_network.cpp:164-191) */
typedef struct gsdr_rx_header {
    int usrp_number;
    char front_end_code;
    int packet_number, length, errors, channels;
} gsdr_rx_header;
void gsdr_format_rx_header(const gsdr_rx_header *h, unsigned char out[21]);

/* ---- synthetic in-memory IQ source (replaces the UHD hardware manager for
 * benchmarking; shaped after software_rx_thread, ref:
 * cpp/USRP_hardware_manager.cpp:1331-1395) ------------------------------- */
/* Fills out_dev[0..n) on the device with
 *   sum_k ampl[k]*exp(i*(2*pi*freq[k]*((start+j) mod rate)/rate + phase[k]))
 *   + sigma*(g1 + i*g2)         (g: counter-based unit gaussians from `seed`)
 * freq/ampl/phase are HOST arrays of n_tones entries.  Returns after the
 * kernel has finished on `hip_stream` (setup helper, not part of the hot path). */
int gsdr_source_tones(gsdr_c64 *out_dev, long long n, long long start, int rate,
                      const int *freq, const float *ampl, const float *phase,
                      int n_tones, float sigma, unsigned long long seed,
                      void *hip_stream);
/* The tone set the reference's TX tone generator actually produces (host only; ref:
 * tone_gen, cpp/kernels.cu:617-635): tones are ASSIGNED to bins of a length-`rate`
 * spectrum (index f, or rate + f for f <= 0), so of tones on one bin the last wins, and
 * an index outside [0, rate) -- a 0 Hz tone lands on `rate` -- is dropped (the reference
 * writes it past its allocation; the inverse FFT never sees it).  Writes the surviving
 * tones (signed Hz, amplitude) to out_freq/out_ampl (room for n each), returns their
 * count.  Feed the result to gsdr_source_tones with phase 0 for the TX buffer
 * (ref: TX_buffer_generator TONES, cpp/USRP_buffer_generator.cpp:60-95,226-229). */
int gsdr_tx_tone_bins(int rate, const int *freq, const float *ampl, int n,
                      int *out_freq, float *out_ampl);

/* TX tone comb generator at scale (row f3).  ref: tone_gen (cpp/kernels.cu:589-684) builds one period of
 * `rate` samples by an inverse FFT when the generator is set up and TX_buffer_generator::get_from_tones
 * (cpp/USRP_buffer_generator.cpp:226-229) serves slices of it; this generator synthesises every buffer on
 * demand from exact integer phases (no 1.6 GB period at 200 Msps), faster than the stream needs it
 * (2048 tones: 17 x real time at 200 Msps).  freq/ampl are the tones gsdr_tx_tone_bins() returned (signed Hz,
 * one per bin), phase their initial phases in radians (NULL = 0).  x[s] = sum_k ampl_k e^(i phase_k)
 * e^(+2 pi i freq_k s / rate).  gsdr_txgen_tones_fill writes samples start .. start + n - 1 (start taken
 * mod rate) into device memory on hip_stream; asynchronous.  Returns 0 / -1 (gsdr_last_error(NULL)). */
typedef struct gsdr_txgen gsdr_txgen;
gsdr_txgen *gsdr_txgen_tones_create(int rate, const int *freq, const float *ampl, const float *phase, int n_tones,
                                    int device_index);
int gsdr_txgen_tones_fill(gsdr_txgen *g, gsdr_c64 *out_dev, long long n, long long start, void *hip_stream);
void gsdr_txgen_close(gsdr_txgen *g);

/* The reference's TX_buffer_generator as one object (ref: headers/USRP_buffer_generator.hpp:47-66,
 * cpp/USRP_buffer_generator.cpp:10-160): created from the TX parameters, every get() hands out the next
 * buffer_len samples.  TONES: the tone comb above (tone set as gsdr_tx_tone_bins(); the sample index wraps at
 * rate * ceil(buffer_len / rate), :60-75); CHIRP: the chirp_gen law (cpp/kernels.cu:335-372) scaled by ampl[0],
 * with the TX side's own num_steps reset (:111-115), the running index wrapping at num_steps * length.  Where
 * the reference exits (mixed or several CHIRP wave types, NODSP/SWONLY/RAMP/DIRECT)
 * create returns NULL with the same text in gsdr_last_error(NULL).  gsdr_txgen_get: to host memory
 * (synchronous, like the reference's get); gsdr_txgen_get_device: to device memory on hip_stream. */
gsdr_txgen *gsdr_txgen_create(const gsdr_param_c *p, const float *ampl, int n_ampl);
int gsdr_txgen_get(gsdr_txgen *g, gsdr_c64 *out_host);
/* TONES as the reference hands them out (ref: get_from_tones, cpp/USRP_buffer_generator.cpp:226-229): the next
 * buffer_len samples as a pointer INTO the generator's own host memory -- one period of the comb plus one buffer
 * (rate * ceil(buffer_len / rate) + buffer_len samples, :60-95), valid and unchanged until gsdr_txgen_close().  The
 * caller's buffer is not touched: tx_single_link passes an unallocated pointer for TONES and queues what it gets
 * back (ref: cpp/USRP_server_link_threads.cpp:568-584).  The period is generated on the GPU the first time it is
 * needed, or by gsdr_txgen_prepare_host() (what the reference's constructor does with its inverse FFT of length
 * `rate`: 1.6 GB of host memory at 200 Msps, there as here).  NULL on failure (gsdr_last_error(NULL)). */
const gsdr_c64 *gsdr_txgen_get_ptr(gsdr_txgen *g);
int gsdr_txgen_prepare_host(gsdr_txgen *g);
/* GSDR_TONES or GSDR_CHIRP (a NOISE request is TONES: the reference's `case NOISE` falls through, :52-58) */
int gsdr_txgen_mode(const gsdr_txgen *g);
int gsdr_txgen_get_device(gsdr_txgen *g, gsdr_c64 *out_dev, void *hip_stream);
long long gsdr_txgen_buffer_len(const gsdr_txgen *g);
/* TX chirp law (ref: chirp_gen, cpp/kernels.cu:335-372) written to device. */
int gsdr_source_chirp(gsdr_c64 *out_dev, long long n, unsigned long long last_index,
                      const gsdr_chirp_param *cp, float scale, void *hip_stream);

/* ---- sc16 output of the TX generators (the contract: "sc16 output" further up) ------------------------------
 * Every entry writes exactly the bits that narrowing the output of its complex64 entry gives.  The sc16 and the
 * complex64 entries of one handle advance the same running index and may be mixed freely.
 * The gain is a property of the handle: 32767 by default; it must be finite and > 0, otherwise
 * gsdr_txgen_set_sc16_gain returns -1, leaves a message in gsdr_last_error(NULL) and keeps the old value.  It is
 * refused in the same way once the handle's sc16 period buffer exists (the buffer was made with the old gain and
 * stays unchanged until close).
 * gsdr_txgen_get_sc16: through a device staging buffer of 4 bytes per sample, 4 bytes per sample copied to the host.
 * gsdr_txgen_get_ptr_sc16 / gsdr_txgen_prepare_host_sc16: TONES only, like the complex64 pair, on a host buffer of
 * their own -- period + buffer_len samples of gsdr_sc16, pinned when possible, made once in pieces through the device,
 * valid and unchanged until gsdr_txgen_close(); the complex64 period buffer is not allocated for it.
 * Clipped components: a generator owns one counter in device memory, zeroed at creation; all its sc16 entries add to
 * it (the period + buffer_len samples generated for the period buffer once).  gsdr_txgen_sc16_clipped synchronises the
 * generator's device and returns the total since creation (-1: device error).  It is a diagnostic -- look at it after
 * a run or while setting a level -- and not meant for the per-buffer loop: it stalls the device.
 * gsdr_source_chirp_sc16: the TX chirp law narrowed; s * scale is rounded to float32 before the gain multiplies it.
 * n == 0 touches nothing, not even the pointers. */
int gsdr_txgen_set_sc16_gain(gsdr_txgen *g, float gain);
float gsdr_txgen_sc16_gain(const gsdr_txgen *g);
int gsdr_txgen_tones_fill_sc16(gsdr_txgen *g, gsdr_sc16 *out_dev, long long n, long long start, void *hip_stream);
int gsdr_txgen_get_device_sc16(gsdr_txgen *g, gsdr_sc16 *out_dev, void *hip_stream);
int gsdr_txgen_get_sc16(gsdr_txgen *g, gsdr_sc16 *out_host);
int gsdr_txgen_prepare_host_sc16(gsdr_txgen *g);
const gsdr_sc16 *gsdr_txgen_get_ptr_sc16(gsdr_txgen *g);
long long gsdr_txgen_sc16_clipped(gsdr_txgen *g);
int gsdr_source_chirp_sc16(gsdr_sc16 *out_dev, long long n, unsigned long long last_index,
                           const gsdr_chirp_param *cp, float scale, float gain,
                           unsigned long long *clipped_dev, void *hip_stream);

/* ---- several chirps in one TX buffer ("several chirps in one handle" further up has the contract) ------------ */
gsdr_txgen *gsdr_txgen_create_ex(const gsdr_param_c *p, const float *ampl, int n_ampl, unsigned flags);
int gsdr_source_multichirp(gsdr_c64 *out_dev, long long n, unsigned long long last_index,
                           const gsdr_chirp_param *cp, const float *scale, int n_chirps, void *hip_stream);
int gsdr_source_multichirp_sc16(gsdr_sc16 *out_dev, long long n, unsigned long long last_index,
                                const gsdr_chirp_param *cp, const float *scale, int n_chirps, float gain,
                                unsigned long long *clipped_dev, void *hip_stream);

/* ---- trigger on the device: glitch events and snippets from demodulated rows (an extension: the reference's
 * triggers run in its Python client, ref: pyUSRP/USRP_triggers.py, amplitude_trigger) -------------------------------
 * A trigger object sees ONE stream of rows of n_ch complex64 each -- the [row][channel] layout every RX entry writes
 * for DIRECT, TONES, averaged frames and multi-chirp handles.  Rows are numbered 0, 1, 2, ... from creation (or from
 * gsdr_trigger_reset) and arrive in FEEDS of n_rows >= 0 rows.  Nothing below depends on where the stream is cut into
 * feeds, with the two exceptions stated under "Capacity" and "Levels".
 * Quantity.  Channel c has six floats {bx, by, dx, dy, lo, hi}.  For sample y of channel c:
 *     t0 = y.x - bx;  t1 = y.y - by;  p0 = t0 * dx;  p1 = t1 * dy;  q = p0 + p1
 *   every operation one IEEE single-precision operation rounded to nearest, nothing fused.  up = q > hi,
 *   dn = !up && q < lo; the channel HITS in that row iff up || dn.  A NaN q never hits; lo = -Inf, hi = +Inf switches
 *   a channel off.  No value of a level is refused.
 * Row record.  A row hits iff any channel hits.  Its record: channel = the lowest-numbered hitting channel, side = +1
 *   for up and -1 for dn, q = that channel's q, n_hit = the number of hitting channels.
 * Trigger.  Row r is a trigger iff it hits and no row in [max(0, r - holdoff), r - 1] hits (hits closer than that are
 *   the same glitch, chained hit to hit).  holdoff = 0 makes every hitting row a trigger.
 * Emission.  A trigger at r owns the snippet rows [r - pre, r + post).  It is emitted by the feed that delivers row
 *   r + post - 1: with that feed covering stream rows [R0, R1), iff R0 <= r + post - 1 < R1.  A trigger with r < pre is
 *   never emitted (its hit still holds off later rows); one whose last row never arrives is never emitted.  Snippets of
 *   different triggers may overlap; each is a full copy.
 * Output of a feed, in ascending trigger row: events[e]; snippets[e][pre + post][n_ch], the input rows bit for bit (NaN
 *   payloads and -0 included); the counts {n_events, n_dropped}.
 * Capacity.  Of the triggers a feed would emit, the first max_events in row order are written and the rest are only
 *   counted in n_dropped.  With n_dropped == 0 in every feed the concatenated output of a stream is the same for every
 *   cutting.
 * Levels.  gsdr_trigger_set_levels takes effect for the rows of later feeds.  A row's record is made with the levels in
 *   force in the feed that delivered it and is never re-evaluated.
 *
 * gsdr_trigger_create: 1 <= n_ch <= 2^20, 1 <= max_rows <= 2^20, pre >= 0, post >= 1, pre + post <= 65536,
 *   0 <= holdoff <= 2^30, 1 <= max_events <= 2^20, levels[n_ch] not NULL; anything else is refused before the device is
 *   touched: NULL, and gsdr_last_error(NULL) starts with "gsdr_trigger_create: " and names the argument.  device_index
 *   >= -1 as in gsdr_param_c; GSDR_TRIGGER_HOST makes a host-only object that touches no GPU: gsdr_trigger_feed_host,
 *   _set_levels (the stream is ignored), _reset, _rows and _close are valid on it.  gsdr_trigger_feed_host is refused on
 *   a device object and the device feeds on a host object (-1, gsdr_last_error(NULL)).  Everything the device feeds need
 *   is allocated here, every byte count in 64 bits; gsdr_trigger_feed alone allocates its staging (max_events events
 *   and snippets) the first time it is called.
 * gsdr_trigger_feed_device: asynchronous on hip_stream (hipStream_t as void*), no synchronisation, no host read-back.
 *   Reads exactly rows_dev[0, n_rows * n_ch); writes counts_dev[0..1] = {n_events, n_dropped} and at most max_events
 *   events and snippets: nothing outside events_dev[0, max_events), snippets_dev[0, max_events * (pre + post) * n_ch)
 *   and counts_dev[0, 2) is written, what lies behind n_events is unspecified.  The pointers need natural alignment
 *   only (8 bytes for rows, events, snippets; 4 for counts) and may point anywhere into larger allocations.  n_rows >
 *   max_rows or n_rows < 0: -1, state unchanged.  n_rows == 0 is a valid feed that emits nothing and touches no row
 *   pointer.  Returns 0.
 * gsdr_trigger_feed: the same launches, then waits for hip_stream and copies to the host only n_events events and
 *   n_events snippets (events_host / snippets_host behind them stay untouched); returns n_events, *n_dropped when given.
 * gsdr_trigger_feed_host: the same bits on the CPU.
 * Stream order.  Like the handle's device entries, the feeds are ordered by the caller through hip_stream -- but a
 *   trigger object does NOT remember streams or wait by itself: consecutive calls on one object (feeds, set_levels) must
 *   be ordered by the caller, on the same stream or through the caller's own events, and rows_dev must stay unchanged
 *   until the feed that reads it has finished.  gsdr_trigger_set_levels copies the levels before it returns.
 * gsdr_trigger_reset: row numbering restarts at 0, carried rows and hit records are dropped (the levels stay).  The
 *   caller must have ordered it behind the feeds in flight.  gsdr_trigger_rows: rows fed since creation / reset. */
#define GSDR_TRIGGER_HOST (-2)
typedef struct gsdr_trigger_level { float bx, by, dx, dy, lo, hi; } gsdr_trigger_level;
typedef struct gsdr_trigger_event { long long row; int channel; int side; float q; int n_hit; } gsdr_trigger_event;
typedef struct gsdr_trigger gsdr_trigger;
gsdr_trigger *gsdr_trigger_create(int n_ch, int max_rows, int pre, int post, int holdoff, int max_events,
                                  const gsdr_trigger_level *levels, int device_index);
int gsdr_trigger_set_levels(gsdr_trigger *t, const gsdr_trigger_level *levels, void *hip_stream);
int gsdr_trigger_feed_device(gsdr_trigger *t, const gsdr_c64 *rows_dev, int n_rows, gsdr_trigger_event *events_dev,
                             gsdr_c64 *snippets_dev, int *counts_dev /* [2] */, void *hip_stream);
int gsdr_trigger_feed(gsdr_trigger *t, const gsdr_c64 *rows_dev, int n_rows, gsdr_trigger_event *events_host,
                      gsdr_c64 *snippets_host, int *n_dropped, void *hip_stream);
int gsdr_trigger_feed_host(gsdr_trigger *t, const gsdr_c64 *rows, int n_rows, gsdr_trigger_event *events,
                           gsdr_c64 *snippets, int *n_dropped);
int gsdr_trigger_reset(gsdr_trigger *t);
long long gsdr_trigger_rows(const gsdr_trigger *t);
void gsdr_trigger_close(gsdr_trigger *t);

/* ---- Welch spectra on the device: running noise spectra from demodulated rows (an extension: the reference's client
 * does this on the host, ref: pyUSRP/USRP_noise.py:655-703, spec_from_samples, scipy.signal.welch per channel) ----------
 * A welch object sees ONE stream of rows of n_ch complex64 each -- the [row][channel] layout every RX entry writes --
 * numbered from 0 (since creation or gsdr_welch_reset), arriving in FEEDS of 0 <= n_rows <= max_rows rows.
 * Segments.  Segment s is rows [s*step, s*step + nperseg); the feed that delivers its last row completes it.  After
 *   `total` rows n_seg = total < nperseg ? 0 : (total - nperseg)/step + 1: the host knows it without a read-back.
 * Per segment and channel, the real and imaginary part treated as the complex number they form, N = nperseg,
 *   t_n = n - (N-1)/2:
 *   1. detrend, in double: m = (1/N) sum x_n, b = sum x_n t_n / sum t_n^2, d_n = fl32(x_n - (m + b t_n)) -- the
 *      subtraction in double, rounded once to float32.  GSDR_WELCH_DETREND_LINEAR as written, _CONSTANT: b = 0,
 *      _NONE: d_n = x_n.  (A float32 subtraction loses 1e-4 .. 1e-2 of the density when the noise is 1e-3 .. 1e-5 of the
 *      carrier: the double subtraction is part of the contract.)
 *   2. window, in float32: e_n = d_n w_n; w is the caller's nperseg floats, or with window == NULL the periodic Hann
 *      window 0.5 - 0.5 cos(2 pi n / N), evaluated in double and rounded to float (scipy's default).
 *   3. transform: Z = FFT_N(e), forward, unnormalised, complex float32.
 *   4. accumulate, for k = 0 .. N/2, Zm = conj Z[(N-k) mod N]: X = (Z[k] + Zm)/2 is the spectrum of the real part,
 *      Y = (Z[k] - Zm)/(2i) that of the imaginary part; three DOUBLE accumulators per bin take A0 += |X|^2,
 *      A1 += |Y|^2, A2 += Re(X conj Y), in segment order.
 *   5. mean: a double S += the sum of the segment's first `step` rows, in a fixed order inside the segment and in
 *      segment order across segments; S / (n_seg step) is the mean of rows [0, n_seg step).
 * Reading.  psd[n_ch][2][N/2+1] floats: [c][0] is the one-sided density of the real part of g_c z, [c][1] of its
 *   imaginary part.  With g = gr + i gi:  P_re = gr^2 A0 + gi^2 A1 - 2 gr gi A2,  P_im = gi^2 A0 + gr^2 A1 + 2 gr gi A2,
 *   each times f_k / (fs sum w_n^2 n_seg), f_k = 2 for 0 < k < N/2 and 1 otherwise, sum w^2 in double from the float
 *   values; all in double, rounded once to float.  mode chooses g: GSDR_WELCH_RAW g = 1; _ROTATE g = |m|/m with m the
 *   object's own mean (the reference's rotate=True); _DBC g = 1/m (the reference's dbc; its later mean subtraction is
 *   the detrend); _GAIN g = gain[c], n_ch complex64.  For ROTATE and DBC m == 0 or a non-finite m gives g = 1.  The
 *   detrend is linear, so it commutes with g: the rotation is chosen when reading, from the mean of the whole run.
 *   A read does not disturb the accumulation, returns n_seg (clamped to INT_MAX), and with n_seg == 0 writes nothing
 *   and returns 0.
 * Cutting.  The device output -- psd for every mode, and the mean -- does not depend, bit for bit, on where the stream
 *   is cut into feeds.
 * Poison.  An Inf or NaN reaches exactly the channel that holds it, from the segment that holds it onward; every other
 *   channel keeps its bits.
 * gsdr_welch_create: 1 <= n_ch <= 2^20, 1 <= max_rows <= 2^20, nperseg a power of two in [16, 8192] (the in-LDS plan
 *   range), nperseg/8 <= step <= nperseg, detrend one of the three values, device_index >= -1 as in gsdr_param_c or
 *   GSDR_WELCH_HOST for a host-only object that touches no GPU.  Anything else is refused before the device is
 *   touched: NULL, and gsdr_last_error(NULL) starts with "gsdr_welch_create: " and names the argument.  Everything a
 *   feed needs is allocated here, every byte count in 64 bits; a failed allocation is a refusal that states the MiB.
 * gsdr_welch_feed_device: asynchronous on hip_stream (hipStream_t as void*), no synchronisation, no read-back; reads
 *   exactly rows_dev[0, n_rows n_ch).  n_rows outside [0, max_rows]: -1, state unchanged.  n_rows == 0 is valid and
 *   touches no pointer.  0, or -1 with gsdr_last_error(NULL).
 * gsdr_welch_read_device: asynchronous; writes exactly psd_dev[0, n_ch 2 (N/2+1)); gain_dev is read for _GAIN only;
 *   fs must be finite and > 0.  gsdr_welch_mean_device: mean_dev[0, n_ch) = S / (n_seg step) as complex64, returns
 *   n_seg, nothing written with n_seg == 0.  gsdr_welch_read: read_device into the object's own buffer, waits for
 *   hip_stream and copies psd (and the mean, if mean_host is given) to the host; gain_host is host memory.
 *   Pointers need their natural alignment only (8 bytes complex, 4 float) and may point anywhere into larger allocations.
 * gsdr_welch_feed_host / gsdr_welch_read_host: GSDR_WELCH_HOST objects only (and the device entries are refused on
 *   them).  The host twin computes the same estimator in DOUBLE throughout (no rounding of d_n, a radix-2 double
 *   transform) and returns doubles: psd[n_ch][2][N/2+1] and, if given, mean[n_ch][2].  It is the estimator's statement
 *   in code, not a bit twin of the device.
 * Stream order is the caller's, as for the trigger: the object remembers no stream and waits for none; rows_dev must
 *   stay unchanged until the feed that reads it has finished.  gsdr_welch_reset: zeroes the accumulators and restarts
 *   the row numbering; the caller must have ordered it behind the feeds in flight (on a device object it waits for the
 *   device).  gsdr_welch_rows / _segments: rows fed and segments complete since creation / reset. */
#define GSDR_WELCH_HOST (-2)
#define GSDR_WELCH_DETREND_NONE 0
#define GSDR_WELCH_DETREND_CONSTANT 1
#define GSDR_WELCH_DETREND_LINEAR 2
#define GSDR_WELCH_RAW 0
#define GSDR_WELCH_ROTATE 1
#define GSDR_WELCH_DBC 2
#define GSDR_WELCH_GAIN 3
typedef struct gsdr_welch gsdr_welch;
gsdr_welch *gsdr_welch_create(int n_ch, int max_rows, int nperseg, int step, int detrend,
                              const float *window /* nperseg, or NULL */, int device_index);
int gsdr_welch_feed_device(gsdr_welch *w, const gsdr_c64 *rows_dev, int n_rows, void *hip_stream);
int gsdr_welch_read_device(gsdr_welch *w, int mode, const gsdr_c64 *gain_dev, double fs, float *psd_dev, void *hip_stream);
int gsdr_welch_read(gsdr_welch *w, int mode, const gsdr_c64 *gain_host, double fs, float *psd_host,
                    gsdr_c64 *mean_host /* n_ch, may be NULL */, void *hip_stream);
int gsdr_welch_mean_device(gsdr_welch *w, gsdr_c64 *mean_dev, void *hip_stream);
int gsdr_welch_feed_host(gsdr_welch *w, const gsdr_c64 *rows, int n_rows);
int gsdr_welch_read_host(gsdr_welch *w, int mode, const gsdr_c64 *gain, double fs, double *psd,
                         double *mean /* n_ch x 2, may be NULL */);
int gsdr_welch_reset(gsdr_welch *w);
long long gsdr_welch_rows(const gsdr_welch *w);
long long gsdr_welch_segments(const gsdr_welch *w);
void gsdr_welch_close(gsdr_welch *w);

/* ---- FIR decimation on the device: a second decimation stage behind demodulated rows (an extension: the reference's
 * client decimates on the host, ref: pyUSRP/USRP_noise.py:1401-1402, scipy.signal.decimate(ftype='fir') per channel) ---
 * A decim object sees ONE stream of rows of n_ch complex64 each -- the [row][channel] layout every RX entry writes --
 * numbered from 0 (since creation or gsdr_decim_reset), arriving in FEEDS of 0 <= n_rows <= max_rows rows.  Its
 * parameters: the factor q, T real float32 taps h[0..T), and an offset p >= 0, the stream row on which the window of
 * output 0 ends.
 * Output law.  y[o] = sum_{t<T} h[t] x[o q + p - (T-1) + t], per channel, real and imaginary part apart; rows before
 *   the stream (index < 0) are zero.  After `total` rows the object has emitted
 *   n_out(total) = total <= p ? 0 : (total - 1 - p)/q + 1 output rows: the host knows it without a read-back.  A feed
 *   emits n_out(total + n_rows) - n_out(total) rows [out_row][channel], possibly 0.  p = q - 1 is the DDC's own frame
 *   law; p = (T-1)/2 with odd symmetric taps is scipy.signal.decimate(zero_phase=True).
 * Arithmetic.  The order is fixed, so that device, host twin and any cutting give the same bits.  F = ceil(T/q).
 *   Chunk j (0 <= j < F) is the taps t with max(0, T - (j+1)q) <= t < T - jq: chunks are cut from the END of the taps,
 *   so chunk j of output o always covers the absolute row block [(o-j)q + p + 1 - q, (o-j)q + p + 1).  A chunk sum
 *   starts at +0 and takes its taps in ascending t, acc = fma(h[t], x, acc), each step one IEEE single-precision fused
 *   multiply-add; rows before the stream are skipped (a chunk whose whole block lies before the stream is +0).  The
 *   output is the chunk sums added oldest first, (((P_{F-1} + P_{F-2}) + ...) + P_0), each addition one float32
 *   addition, nothing else fused.  A block's contribution to its F outputs depends on that block alone.
 * Cutting.  The concatenated output does not depend, bit for bit, on where the stream is cut into feeds.
 * Poison.  An Inf or NaN reaches exactly the outputs whose T-row window holds it, zero taps included, in its own
 *   channel; everything else keeps its bits.
 * gsdr_decim_create: 1 <= n_ch <= 2^20, 1 <= max_rows <= 2^20, 1 <= q <= 4096, 1 <= n_taps <= 64 q, every tap finite,
 *   0 <= offset <= 2^30, device_index >= -1 as in gsdr_param_c or GSDR_DECIM_HOST for a host-only object that touches
 *   no GPU; taps == NULL requires n_taps == 0 and q >= 2 and selects the default taps.  Anything else is refused before
 *   the device is touched: NULL, and gsdr_last_error(NULL) starts with "gsdr_decim_create: " and names the argument.
 *   Everything a feed needs is allocated here, every byte count in 64 bits; a failed allocation is a refusal that
 *   states the MiB.
 * Default taps: scipy's FIR decimation design, T = 20 q + 1, firwin(T, 1/q, window='hamming') -- the ideal low-pass with
 *   cutoff 1/q of Nyquist times the symmetric Hamming window, scaled to sum 1 -- evaluated in double and rounded once
 *   to float32.  gsdr_decim_default_taps(q, w): host only; writes 20 q + 1 floats and returns that count, or -1
 *   (q outside [2, 4096], w NULL).
 * gsdr_decim_next_rows: the rows a feed of n_rows would emit now (-1: n_rows outside [0, max_rows]);
 *   gsdr_decim_out_capacity: the most rows one feed can emit, (max_rows - 1)/q + 1.
 * gsdr_decim_feed_device: asynchronous on hip_stream (hipStream_t as void*), no synchronisation, no read-back, at most
 *   three launches; reads exactly rows_dev[0, n_rows n_ch), writes exactly out_dev[0, emitted n_ch); returns the rows
 *   emitted, or -1 with gsdr_last_error(NULL).  Pointers need 8-byte alignment only and may point anywhere into larger
 *   allocations.  n_rows == 0 is valid and touches no pointer; n_rows outside [0, max_rows]: -1, state unchanged.
 * gsdr_decim_feed: the same launches, then waits for hip_stream and copies the emitted rows to out_host.
 * gsdr_decim_feed_host: GSDR_DECIM_HOST objects only (and the device feeds are refused on them): a BIT TWIN of the
 *   device (std::fmaf, plain float additions).
 * Stream order is the caller's, as for the trigger and Welch objects: the object remembers no stream and waits for
 *   none; rows_dev must stay unchanged until the feed that reads it has finished.  gsdr_decim_reset restarts the row
 *   numbering; the caller must have ordered it behind the feeds in flight.  gsdr_decim_get_taps: copies min(cap, T)
 *   taps and returns T.  gsdr_decim_rows / _rows_out: rows fed and rows emitted since creation / reset.  On a NULL
 *   object close is a no-op, the getters return 0, the feeds and reset return -1 with the reason. */
#define GSDR_DECIM_HOST (-2)
typedef struct gsdr_decim gsdr_decim;
gsdr_decim *gsdr_decim_create(int n_ch, int max_rows, int q, int n_taps, const float *taps /* n_taps, or NULL */,
                              long long offset, int device_index);
int gsdr_decim_next_rows(const gsdr_decim *d, int n_rows);
long long gsdr_decim_out_capacity(const gsdr_decim *d);
int gsdr_decim_feed_device(gsdr_decim *d, const gsdr_c64 *rows_dev, int n_rows, gsdr_c64 *out_dev, void *hip_stream);
int gsdr_decim_feed(gsdr_decim *d, const gsdr_c64 *rows_dev, int n_rows, gsdr_c64 *out_host, void *hip_stream);
int gsdr_decim_feed_host(gsdr_decim *d, const gsdr_c64 *rows, int n_rows, gsdr_c64 *out);
int gsdr_decim_get_taps(const gsdr_decim *d, float *w, int cap);
int gsdr_decim_reset(gsdr_decim *d);
long long gsdr_decim_rows(const gsdr_decim *d);
long long gsdr_decim_rows_out(const gsdr_decim *d);
void gsdr_decim_close(gsdr_decim *d);
int gsdr_decim_default_taps(int q, float *w);

/* ---- VNA sweep accumulator on the device: the mean of every frequency point over the sweeps, behind demodulated CHIRP
 * rows (an extension: the reference's client reads the whole stream back and averages it on the host, ref:
 * pyUSRP/USRP_VNA.py:683-804, VNA_analysis) ---------------------------------------------------------------------------
 * A sweep object sees ONE stream of rows of n_ch complex64 each -- the [row][channel] layout every RX entry writes, one
 * channel per chirp of a CHIRP handle -- numbered first_row, first_row + 1, ..., arriving in FEEDS of
 * 0 <= n_rows <= GSDR_SWEEP_MAX_FEED rows.  It folds them onto the n_points points of one sweep and keeps, per point and
 * channel, sums and sums of squares in double.  Only what a read asks for leaves the device: n_points x n_ch means,
 * optionally as many variances, and one complex number per channel for the line delay.
 * Fold.  Row r belongs to point p(r) = (r / group) mod n_points, in 64-bit integer arithmetic.  group = 1 for the
 *   lock-in's rows (decim >= 1: one row per point), group = length for an undecimated CHIRP handle (decim == 0: one row
 *   per sample); a larger group merges adjacent points.  first_row attaches an object to a handle that has already run:
 *   the number of rows the handle wrote before the first one fed.
 * Accumulate.  Each (p, c) has four doubles S.re, S.im, Q.re, Q.im, all +0 at creation / reset.  A row x adds
 *   S += (double)x and Q += (double)x (double)x per component (the square of a float32 is exact in double: fused or not,
 *   the update is the same).  Each accumulator takes its rows strictly in stream order, one IEEE double addition per
 *   row.  That is the whole order rule.
 * Cutting.  No result depends, bit for bit, on where the stream is cut into feeds.
 * Counts.  n[p] is the number of rows r in [first_row, first_row + total) with p(r) = p, a closed form of first_row,
 *   total, group and n_points: with W = n_points group and below(x) = (x / W) group + min(max(x mod W - p group, 0),
 *   group), n[p] = below(first_row + total) - below(first_row).  The host knows it without a read-back:
 *   gsdr_sweep_point_rows(s, p) (0 for p outside [0, n_points)); gsdr_sweep_sweeps(s) = (min over p of n[p]) / group, the
 *   complete passes over every point; gsdr_sweep_rows(s) = total.
 * Read (does not disturb the accumulation; any number of reads).  mean[p][c] = fl32(S / n[p]) per component: one double
 *   division, one rounding to float.  var[p][c], a complex64 that holds the variance of the real and of the imaginary
 *   part, = fl32(max(fma(-S, S / n, Q) / (n - 1), 0)): the fma is part of the contract (std::fma on the host, __fma_rn
 *   on the device), and a NaN stays a NaN.  n[p] == 0 writes (+0, +0) to both; n[p] == 1 gives the variance (+0, +0).
 *   What this variance resolves: the sums hold |mean|^2 n to 2^-53 relative, so its relative error is about
 *   n 2^-53 |mean|^2 / var at the worst -- measured on x86-64 against numpy.var in float64 for noise at 1e-5 of the
 *   carrier, the worst of 1 600 variances: 1.3e-5 at n = 64, 1.6e-4 at n = 4096 (medians 3e-8 and 2e-5).
 *   Noise further below the carrier than that needs a shifted or Welford form, which is not built.
 * Phase slope.  D[c] = sum_{p=0}^{n_points-2} m[p+1][c] conj(m[p][c]) in double, m the float32 means a read returns
 *   (every product of two of their components is exact in double).  Term p is (a c + b d) + i (b c - a d) for
 *   m[p+1] = a + i b, m[p] = c + i d: each component two exact products and one rounding.  The terms are added from +0
 *   in ascending p inside blocks of 256 consecutive p; the block sums are added in ascending block order, starting from
 *   block 0's sum.  n_points == 1 gives +0.  tau[c] = -arg D[c] / (2 pi f_step) is the line delay of channel c for
 *   points f_step apart, the `D` of the reference's resonator fit, unambiguous for |tau| < 1 / (2 f_step).  A non-finite
 *   mean in channel c makes D[c] non-finite; every other channel keeps its bits.
 * Poison.  An Inf or NaN reaches exactly the (point, channel) accumulators whose rows hold it; every other mean and
 *   variance keeps its bits.
 * gsdr_sweep_create: 1 <= n_ch <= 2^20, 1 <= n_points <= 2^24 with n_points n_ch <= 2^25 (32 bytes each: 1 GiB at
 *   most), 1 <= group <= 2^30, 0 <= first_row <= 2^62, device_index >= -1 as in gsdr_param_c or GSDR_SWEEP_HOST for a
 *   host-only object that touches no GPU.  Anything else is refused before the device is touched: NULL, and
 *   gsdr_last_error(NULL) starts with "gsdr_sweep_create: " and names the argument.  Everything a feed, a
 *   gsdr_sweep_read_device and a slope need is allocated here, every byte count in 64 bits; a failed allocation is a
 *   refusal that states the MiB.
 * gsdr_sweep_feed_device: ONE launch on hip_stream (hipStream_t as void*): no allocation, no synchronisation, no
 *   read-back; reads exactly rows_dev[0, n_rows n_ch) and writes nothing the caller can see; 0, or -1 with
 *   gsdr_last_error(NULL).  Pointers need 8-byte alignment only and may point anywhere into larger allocations.
 *   n_rows == 0 is valid and touches no pointer; n_rows outside [0, GSDR_SWEEP_MAX_FEED], or a stream of more than
 *   GSDR_SWEEP_MAX_ROWS rows: -1, state unchanged.
 * gsdr_sweep_read_device: one launch on hip_stream; writes exactly mean_dev[0, n_points n_ch) and, where var_dev is not
 *   NULL, var_dev[0, n_points n_ch).  gsdr_sweep_read: the same launch into a staging buffer of the object (allocated
 *   by the first such call), then waits for hip_stream and copies to mean_host and (may be NULL) var_host.
 * gsdr_sweep_slope: d_host takes n_ch x (re, im) doubles.  On a device object two launches on hip_stream, then it waits
 *   and copies; on a host object the twin (hip_stream is ignored).
 * gsdr_sweep_feed_host / _read_host: GSDR_SWEEP_HOST objects only (and the device feed and reads are refused on them):
 *   a BIT TWIN of the device for the means, the variances and D.
 * Stream order is the caller's, as for the trigger, Welch and decim objects: the object remembers no stream and waits
 *   for none; rows_dev must stay unchanged until the feed that reads it has finished.  gsdr_sweep_reset(s, first_row):
 *   zeroes the accumulators and restarts the row numbering at first_row (in [0, 2^62]); the caller must have ordered it
 *   behind the feeds and reads in flight (on a device object it waits for the device).  On a NULL object close is a
 *   no-op, the getters return 0, the rest return -1 with the reason.
 * Host-only helpers.  gsdr_sweep_shape_for_chirp: the fold of a CHIRP handle's rows.  decim >= 1: ppt = length decim
 *   samples per row, n_points = num_steps length / ppt, group = 1 -- refused (-1) when ppt does not divide the period
 *   num_steps length: the points then do not repeat from sweep to sweep (and the client's swipe_s / decim is wrong too).
 *   decim == 0: n_points = num_steps, group = length.  Also -1: a NULL pointer, decim < 0, num_steps or length 0, a
 *   result outside the limits of gsdr_sweep_create.
 *   gsdr_vna_axis: the frequency axis of VNA_analysis (ref: pyUSRP/USRP_VNA.py:738-742), all in double:
 *   df = trunc((2^32 - 1)(chirp_f - freq0) / (swipe_s - 1) / rate), the kernel's integer slope (negative for a downward
 *   sweep); stop = freq0 + df (swipe_s - 1) rate / (2^32 - 1); f[i] = rf + numpy.linspace(freq0, stop, n_points)[i]:
 *   freq0 + i step with step = (stop - freq0) / (n_points - 1), the last point exactly stop (n_points == 1: freq0).
 *   -1: f NULL, swipe_s < 2, n_points < 1, rate <= 0. */
#define GSDR_SWEEP_HOST (-2)
#define GSDR_SWEEP_MAX_FEED (1 << 24)
#define GSDR_SWEEP_MAX_ROWS (1LL << 61)
typedef struct gsdr_sweep gsdr_sweep;
gsdr_sweep *gsdr_sweep_create(int n_ch, long long n_points, long long group, long long first_row, int device_index);
int gsdr_sweep_feed_device(gsdr_sweep *s, const gsdr_c64 *rows_dev, int n_rows, void *hip_stream);
int gsdr_sweep_feed_host(gsdr_sweep *s, const gsdr_c64 *rows, int n_rows);
int gsdr_sweep_read_device(gsdr_sweep *s, gsdr_c64 *mean_dev, gsdr_c64 *var_dev /* may be NULL */, void *hip_stream);
int gsdr_sweep_read(gsdr_sweep *s, gsdr_c64 *mean_host, gsdr_c64 *var_host /* may be NULL */, void *hip_stream);
int gsdr_sweep_read_host(gsdr_sweep *s, gsdr_c64 *mean, gsdr_c64 *var /* may be NULL */);
int gsdr_sweep_slope(gsdr_sweep *s, double *d_host /* n_ch x 2 */, void *hip_stream);
int gsdr_sweep_reset(gsdr_sweep *s, long long first_row);
long long gsdr_sweep_rows(const gsdr_sweep *s);
long long gsdr_sweep_sweeps(const gsdr_sweep *s);
long long gsdr_sweep_point_rows(const gsdr_sweep *s, long long p);
void gsdr_sweep_close(gsdr_sweep *s);
int gsdr_sweep_shape_for_chirp(const gsdr_chirp_param *cp, long long decim, long long *n_points, long long *group);
int gsdr_vna_axis(double rate, double freq0, double chirp_f, double swipe_s, long long n_points, double rf, double *f);

/* ---- resonator map on the device: demodulated I/Q to resonance-frequency shift and quality factor, behind demodulated
 * rows (an extension: the reference's client does it on the host, per channel, after every timestream has crossed PCIe
 * and TCP, ref: pyUSRP/USRP_noise.py:1070-1108, calculate_frequency_timestream; its frequency-noise entries,
 * :1660-1667, are empty stubs) -----------------------------------------------------------------------------------------
 * A resmap object sees FEEDS of 0 <= n_rows <= max_rows rows of n_ch complex64 each -- the [row][channel] layout every RX
 * entry writes -- and emits the same number of rows of n_out complex64.  Output column k is computed from input column
 * channels[k]: the list may select a subset, reorder and repeat; channels == NULL is the identity and requires
 * n_out == n_ch.  Each sample is mapped on its own: the object carries no stream state except its offsets.
 * Constants.  Each output column has, in double, n = (nr, ni) the cable term, g = (gr, gi) = 1/n, K = (kr, ki) = n/Qe,
 *   hf0 = f0/2 in Hz and two offsets x0, y0 (0 until gsdr_resmap_set_offsets).  gsdr_resmap_constants derives
 *   GSDR_RESMAP_NCONST = 7 doubles {nr, ni, gr, gi, kr, ki, hf0} on the host from the reference's fit tuple and the tone:
 *   f_tone in Hz, f0 in MHz, A, phi, D, Qe = Qe_re + i Qe_im.  theta = 1e-6 D (f_tone - f0 1e6) + phi,
 *   n = A (cos 2 pi theta, sin 2 pi theta), g = (nr, -ni) / (nr nr + ni ni),
 *   K = (nr Qe_re + ni Qe_im, ni Qe_re - nr Qe_im) / (Qe_re Qe_re + Qe_im Qe_im), hf0 = f0 1e6 / 2, all in double as
 *   written.  It is the only place they are computed: the device and the twin receive the same numbers.  -1, with
 *   gsdr_last_error(NULL) = "gsdr_resmap_constants: " and the argument's name: a non-finite input, A <= 0, f0 <= 0,
 *   Qe == 0 (named as Qe_re and Qe_im), constants NULL.
 * Arithmetic.  One law, in double; sx, sy are the input sample promoted to double.  Every multiply that feeds an add is
 *   an explicit fused multiply-add (so that no compiler's contraction can change the law); +, - and / are IEEE double
 *   operations; every output is rounded once to float32.
 *   GSDR_RESMAP_CAL, the calibrated S21 s/n (what diagnostic_VNA_noise plots):
 *     zr = fma(sx, gr, -(sy gi)), zi = fma(sx, gi, sy gr); out = (fl32(zr - x0), fl32(zi - y0)).
 *   GSDR_RESMAP_X_DQR and GSDR_RESMAP_X_QR, q = (1/Qe) / (1 - s/n) = K / (n - s):
 *     wr = nr - sx, wi = ni - sy, m = fma(wr, wr, wi wi), a = fma(kr, wr, ki wi), b = fma(ki, wr, -(kr wi)),
 *     qr = a / m, qi = b / m.  out.x = fl32(fma(hf0, qi, -x0)), the shift of the resonance frequency in Hz, in both;
 *     out.y = fl32(qr - y0) in X_DQR, the inverse Qr (linear in dissipation: what a spectrum wants), and
 *     out.y = fl32(m / a - y0) in X_QR, the reference's 1 / Re(q).
 *   A sample equal to n gives what IEEE gives (0/0, m/0) and traps nothing.  An Inf or NaN in a sample reaches that
 *   sample's output and no other.  The offsets stand in for the reference's "- np.mean(...)": a caller reads a mean
 *   from the first feed or from the Welch object behind the map and sets it once; the subtraction then happens in
 *   double, before the only rounding.
 * gsdr_resmap_create: 1 <= n_ch <= 2^20, 1 <= max_rows <= 2^20, 1 <= n_out <= 2^20, channels NULL (n_out == n_ch) or
 *   n_out entries in [0, n_ch), constants n_out x GSDR_RESMAP_NCONST finite doubles, kind one of the three,
 *   device_index >= -1 as in gsdr_param_c or GSDR_RESMAP_HOST for a host-only object that touches no GPU.  Anything else
 *   is refused before the device is touched: NULL, and gsdr_last_error(NULL) starts with "gsdr_resmap_create: " and
 *   names the argument.  Everything gsdr_resmap_feed_device and gsdr_resmap_set_offsets need is allocated here; a failed
 *   allocation is a refusal that states the MiB.
 * gsdr_resmap_set_offsets: xy holds n_out x (x0, y0) doubles, all finite, and is copied before the call returns; NULL
 *   sets zeros.  On a device object the new offsets are ordered on hip_stream: feeds enqueued on it before the call see
 *   the old ones, feeds enqueued after it the new ones.  On a host object it is immediate.
 * gsdr_resmap_feed_device: ONE launch on hip_stream (hipStream_t as void*): no allocation, no synchronisation, no
 *   read-back; reads exactly rows_dev[0, n_rows n_ch), writes exactly out_dev[0, n_rows n_out); returns n_rows, or -1
 *   with gsdr_last_error(NULL).  Pointers need 8-byte alignment only and may point anywhere into larger allocations.
 *   n_rows == 0 is valid and touches no pointer; n_rows outside [0, max_rows]: -1.  out_dev == rows_dev is allowed
 *   exactly when the channel list is the identity (NULL, or n_out == n_ch and channels[k] == k); any other overlap of
 *   the two extents is refused.
 * gsdr_resmap_feed: the same launch into a staging buffer of the object (max_rows n_out samples, allocated by the first
 *   such call), then waits for hip_stream and copies to out_host.
 * gsdr_resmap_feed_host: GSDR_RESMAP_HOST objects only (and the device feeds are refused on them): a BIT TWIN of the
 *   device; rows and out may be the same buffer under the rule above.
 * Getters: gsdr_resmap_n_out, gsdr_resmap_kind; gsdr_resmap_get_constants / _get_offsets / _get_channels copy
 *   min(cap, n_out) columns (7 doubles, 2 doubles, 1 int each; the identity is written out) and return n_out.
 * Stream order is the caller's, as for the trigger, Welch, decim and sweep objects: the object remembers no stream and
 *   waits for none; rows_dev must stay unchanged until the feed that reads it has finished.  On a NULL object close is
 *   a no-op, the getters return 0, the feeds and set_offsets return -1 with the reason. */
#define GSDR_RESMAP_HOST (-2)
#define GSDR_RESMAP_CAL 0
#define GSDR_RESMAP_X_DQR 1
#define GSDR_RESMAP_X_QR 2
#define GSDR_RESMAP_NCONST 7
typedef struct gsdr_resmap gsdr_resmap;
int gsdr_resmap_constants(double f_tone, double f0, double A, double phi, double D, double Qe_re, double Qe_im,
                          double *constants /* GSDR_RESMAP_NCONST */);
gsdr_resmap *gsdr_resmap_create(int n_ch, int max_rows, int n_out, const int *channels /* n_out, or NULL */,
                                const double *constants /* n_out x GSDR_RESMAP_NCONST */, int kind, int device_index);
int gsdr_resmap_set_offsets(gsdr_resmap *r, const double *xy /* n_out x 2, or NULL */, void *hip_stream);
int gsdr_resmap_feed_device(gsdr_resmap *r, const gsdr_c64 *rows_dev, int n_rows, gsdr_c64 *out_dev, void *hip_stream);
int gsdr_resmap_feed(gsdr_resmap *r, const gsdr_c64 *rows_dev, int n_rows, gsdr_c64 *out_host, void *hip_stream);
int gsdr_resmap_feed_host(gsdr_resmap *r, const gsdr_c64 *rows, int n_rows, gsdr_c64 *out);
int gsdr_resmap_n_out(const gsdr_resmap *r);
int gsdr_resmap_kind(const gsdr_resmap *r);
int gsdr_resmap_get_constants(const gsdr_resmap *r, double *constants, int cap);
int gsdr_resmap_get_offsets(const gsdr_resmap *r, double *xy, int cap);
int gsdr_resmap_get_channels(const gsdr_resmap *r, int *channels, int cap);
void gsdr_resmap_close(gsdr_resmap *r);

/* ---- row statistics on the device: per-channel moments, histograms and trigger levels, behind demodulated rows (an
 * extension: the reference's only trigger in use takes the median and the standard deviation of each packet on the host,
 * ref: pyUSRP/USRP_triggers.py:165-248, amplitude_trigger) ---------------------------------------------------------------
 * A stats object sees ONE stream of rows of n_ch complex64 each -- the [row][channel] layout every RX entry and the
 * resmap object write -- numbered 0, 1, 2, ... from creation (or from gsdr_stats_reset), arriving in FEEDS of
 * 0 <= n_rows <= max_rows rows.  Per channel it keeps sums in double, the extremes and a histogram of one real quantity
 * q; a read gives the mean, the variance and the extremes, gsdr_stats_quantiles order statistics to within one bin, and
 * gsdr_stats_levels a table gsdr_trigger_set_levels takes: rows -> (resmap ->) stats -> levels -> trigger stays on the
 * card, 24 bytes per channel cross to the host and back.
 * Axes.  axes[c] is the trigger's own struct.  {bx, by, dx, dy} are the projection; lo < hi, both finite, is the
 *   HISTOGRAM RANGE of channel c (not a trigger level).  From them the host derives once, in double:
 *   p = 0.5 ((double)lo + (double)hi), the pivot; inv_w = n_bins / ((double)hi - (double)lo);
 *   w = ((double)hi - (double)lo) / n_bins, the width of a bin.
 * Per sample y of channel c, every operation one IEEE operation rounded to nearest, nothing fused:
 *     t0 = y.x - bx;  t1 = y.y - by;  p0 = t0 * dx;  p1 = t1 * dy;  q = p0 + p1        (float32: exactly the trigger's q)
 *   A non-finite q (NaN, +-Inf) counts in `bad` and enters nothing else.  Otherwise:
 *   Chains.  Row r of channel c belongs to chain j = r mod lanes.  With d = (double)q - p the chain does S_j = S_j + d
 *     and Q_j = Q_j + fl64(d d), and keeps min_j = (q < min_j ? q : min_j) and max_j = (q > max_j ? q : max_j) in
 *     float32 (an equal value, -0 against +0 included, leaves the earlier one).  A chain starts at S = Q = +0,
 *     min = +Inf, max = -Inf and takes its rows in stream order.
 *   Bins.  q < lo: `under`.  Otherwise k = floor(((double)q - (double)lo) inv_w) in double; k >= n_bins: `over` (so
 *     q == hi is over); else bins[k].  Counters are unsigned 64-bit; counts[c] has n_bins + 3 of them:
 *     [0] = under, [1 .. n_bins] = the bins, [n_bins + 1] = over, [n_bins + 2] = bad.
 * Read (does not disturb the accumulation; any number of reads).  n = under + sum of bins + over.  The chains are combined
 *   by the fixed halving tree: for h = lanes/2, lanes/4, ..., 1: s[j] = s[j] (+) s[j + h] for j < h, where (+) adds S and
 *   Q in double and takes min and max by the rule above with s[j] the earlier.  mean = p + S / n;
 *   var = (Q - S (S / n)) / (n - 1), a negative result replaced by +0, a NaN kept: every operation rounded, no fma.
 *   n == 0: mean and var are NaN, min = +Inf, max = -Inf.  n == 1: var is NaN.  One gsdr_stats_summary of 64 bytes per
 *   channel.  The variance divides by n - 1.
 *   What the pivot buys: the sums hold d = q - p, not q, so the variance loses n 2^-52 (1 + ((mean - p) / sigma)^2) at
 *   the worst -- below 1e-9 relative up to n = 2^17 with the pivot within 10 sigma of the mean.  A range that wide of
 *   the data is what the two-pass use is for: a coarse range first, gsdr_stats_levels, then gsdr_stats_reset with
 *   mean -/+ 8 sigma.
 * Quantile pr in (0, 1].  t = max(1, ceil(pr (double)n)), one double multiply.  n == 0: NaN.  under >= t: -Inf.
 *   Otherwise the first bin k whose cumulative count under + bins[0] + ... + bins[k] reaches t; with C the count below
 *   it and h its own: (double)lo + ((double)k + (((double)(t - C) - 0.5) / (double)h)) w, in that order of operations.  A
 *   rank in `over`: +Inf.  The estimate and the order statistic x_(t) lie in the same bin: the error is below w by
 *   construction.
 * Levels.  gsdr_stats_levels writes out_host[n_ch]: bx .. dy copied from the axes, lo = fl32(c - nsigma sigma),
 *   hi = fl32(c + nsigma sigma) with c the mean (GSDR_STATS_CENTRE_MEAN) or the quantile 0.5
 *   (GSDR_STATS_CENTRE_MEDIAN), sigma = sqrt(var) and nsigma sigma one double product.  A channel is switched off
 *   (lo = -Inf, hi = +Inf) when on is not NULL and on[c] == 0, when n < 2, or when c or sigma is not finite.  sigma
 *   divides by n - 1 where the reference's np.std divides by n: the ratio is sqrt(1 - 1/n).  nsigma must be finite
 *   and >= 0.
 * Consequences.  No result depends, bit for bit, on where the stream is cut into feeds.  The host twin returns the
 *   device's bits.  A non-finite sample changes only its own channel's `bad`.  The sums (not the counts, the extremes
 *   or the quantiles) depend on `lanes`, reproducibly, and on nothing else about the launch.
 * gsdr_stats_create: 1 <= n_ch <= 2^20, 1 <= max_rows <= 2^20, 1 <= n_bins <= 4096; lanes 0 (a host rule picks it, a
 *   pure function of n_ch and max_rows: the smallest power of two with n_ch lanes >= 65536, at most the largest power
 *   of two <= max_rows and at most 32768) or a power of two in [1, 32768]; axes[n_ch] not NULL with lo < hi finite in
 *   every entry; device_index >= -1 as in gsdr_param_c or GSDR_STATS_HOST for a host-only object that touches no GPU.
 *   Anything else is refused before the device is touched: NULL, and gsdr_last_error(NULL) starts with
 *   "gsdr_stats_create: " and names the argument.  Everything every entry needs is allocated here (24 bytes per chain
 *   and channel, 8 (n_bins + 3) per channel, the staging of the reads), every byte count in 64 bits; a failed
 *   allocation is a refusal that states the MiB.
 * gsdr_stats_feed_device: ONE launch on hip_stream (hipStream_t as void*): no allocation, no synchronisation, no
 *   read-back; reads exactly rows_dev[0, n_rows n_ch) and writes nothing the caller can see; 0, or -1 with
 *   gsdr_last_error(NULL).  rows_dev needs 8-byte alignment only and may point anywhere into a larger allocation.
 *   n_rows == 0 is valid and touches no pointer; n_rows outside [0, max_rows]: -1, state unchanged.
 * gsdr_stats_read_device: one launch on hip_stream; writes exactly summary_dev[0, n_ch) (8-byte aligned).
 *   gsdr_stats_read: the same launch into the object's staging, then waits for hip_stream and copies to summary_host.
 * gsdr_stats_counts (counts_host[n_ch][n_bins + 3]), gsdr_stats_quantiles (1 <= n_p <= GSDR_STATS_MAX_QUANTILES,
 *   every pr in (0, 1], out_host[n_ch][n_p] doubles) and gsdr_stats_levels take either kind of object: on a device
 *   object they enqueue on hip_stream, wait for it and copy; on a host object the stream is ignored.
 * gsdr_stats_feed_host / _read_host: GSDR_STATS_HOST objects only (and the device feed and reads are refused on them): a
 *   BIT TWIN of the device.
 * gsdr_stats_reset(s, axes): restarts the row numbering at 0 and empties the chains and the counters; with axes not NULL
 *   the object takes the new ranges and projections (checked as at creation; a refusal leaves everything as it was).
 *   On a device object it waits for the device, zeroes, and waits again.
 * Stream order is the caller's, as for the trigger: the object remembers no stream and waits for none.  Consecutive calls
 *   on one object must be ordered by the caller (one stream, or events between streams); rows_dev must stay unchanged
 *   until the feed that reads it has finished.  On a NULL object close is a no-op, the getters return 0, the rest
 *   return -1 with the reason.
 * gsdr_stats_plan: the launch of one feed of an object with n_ch channels, n_bins bins and `lanes` chains per channel
 *   (what gsdr_stats_lanes reports; csrc/stats_state.h: the function the feed itself asks; host only, no GPU needed,
 *   like gsdr_pfb_plan and gsdr_ddc_plan).  out[0] tile: the channels of a workgroup, the largest power of two that is
 *   at most n_ch, at most 32, and whose table tile (n_bins + 3) 4 bytes fits into 65536 bytes of LDS; out[1] tiles:
 *   ceil(n_ch / tile), the grid's x; out[2] splits: ceil(lanes / (256 / tile)), the grid's y; out[3] lds_bytes: the
 *   table's bytes.  No result of the object depends on any of them.  Returns 0, or -1 for a NULL out and for what
 *   gsdr_stats_create refuses of n_ch and n_bins; lanes must be a power of two in [1, 32768] (0, the rule, needs
 *   max_rows: ask the object). */
#define GSDR_STATS_HOST (-2)
#define GSDR_STATS_MAX_BINS 4096
#define GSDR_STATS_MAX_LANES 32768
#define GSDR_STATS_MAX_QUANTILES 16
#define GSDR_STATS_CENTRE_MEAN 0
#define GSDR_STATS_CENTRE_MEDIAN 1
typedef struct gsdr_stats_summary {
    unsigned long long n, bad, under, over;
    double mean, var;
    float min, max;
    unsigned char reserved[8]; /* zero */
} gsdr_stats_summary;
typedef struct gsdr_stats gsdr_stats;
gsdr_stats *gsdr_stats_create(int n_ch, int max_rows, int n_bins, int lanes, const gsdr_trigger_level *axes, int device_index);
int gsdr_stats_feed_device(gsdr_stats *s, const gsdr_c64 *rows_dev, int n_rows, void *hip_stream);
int gsdr_stats_feed_host(gsdr_stats *s, const gsdr_c64 *rows, int n_rows);
int gsdr_stats_read_device(gsdr_stats *s, gsdr_stats_summary *summary_dev, void *hip_stream);
int gsdr_stats_read(gsdr_stats *s, gsdr_stats_summary *summary_host, void *hip_stream);
int gsdr_stats_read_host(gsdr_stats *s, gsdr_stats_summary *summary);
int gsdr_stats_counts(gsdr_stats *s, unsigned long long *counts_host /* n_ch x (n_bins + 3) */, void *hip_stream);
int gsdr_stats_quantiles(gsdr_stats *s, const double *pr, int n_p, double *out_host /* n_ch x n_p */, void *hip_stream);
int gsdr_stats_levels(gsdr_stats *s, int centre, double nsigma, const unsigned char *on /* n_ch bytes, or NULL */,
                      gsdr_trigger_level *out_host, void *hip_stream);
int gsdr_stats_reset(gsdr_stats *s, const gsdr_trigger_level *axes /* n_ch, or NULL */);
long long gsdr_stats_rows(const gsdr_stats *s);
int gsdr_stats_lanes(const gsdr_stats *s);
int gsdr_stats_n_bins(const gsdr_stats *s);
int gsdr_stats_plan(int n_ch, int n_bins, int lanes, int out[4] /* tile, tiles, splits, lds_bytes */);
void gsdr_stats_close(gsdr_stats *s);

/* ---- channel covariance on the device: sums of products across channels, covariance and correlation matrices, behind
 * demodulated rows (an extension: the reference's users take numpy.cov of timestreams that have crossed PCIe and TCP) -----
 * A cov object sees ONE stream of rows of n_ch complex64 each -- the [row][channel] layout every RX entry and the resmap
 * object write -- numbered 0, 1, 2, ... from creation (or from gsdr_cov_reset), arriving in FEEDS of 0 <= n_rows <=
 * max_rows rows.  It keeps, in double, the sums and the sums of products of n_var real VARIABLES; only n_var^2 doubles
 * leave the card, and only when read.
 * Variables.  Variable i is a real projection of ONE channel: axes[i] = {channel, bx, by, dx, dy, reserved = 0, pivot},
 *   32 bytes, 0 <= channel < n_ch.  A channel may appear in any order, more than once, or not at all: two axes on one
 *   channel ({dx, dy} = {1, 0} and {0, 1}) give both quadratures, so the full real covariance of complex data is
 *   expressible.
 * Per sample y of the channel of variable i, every operation one IEEE operation rounded to nearest, nothing fused:
 *     t0 = y.x - bx;  t1 = y.y - by;  p0 = t0 * dx;  p1 = t1 * dy;  v = p0 + p1      (float32: exactly the trigger's and the
 *   stats object's q);  d_i = (double)v - pivot, one double subtraction.
 * Accumulation.  Row r belongs to chain r mod lanes.  Per chain, in stream order, a row does S[i] = S[i] + d_i for every
 *   i and G[i][j] = fma(d_i, d_j, G[i][j]) for every j <= i: ONE fused multiply-add per row and cell (the cell (i, j) with
 *   j > i IS the cell (j, i)).  A chain starts at +0 everywhere.
 * Read (does not disturb the accumulation; any number of reads).  The chains are joined by the fixed halving tree of the
 *   stats object, per cell of S and G: for h = lanes/2, lanes/4, ..., 1: X[k] = X[k] + X[k + h] for k < h.  With n the
 *   rows fed (the host knows it: nothing is read back) a read writes out[n_var][n_var] doubles, the cell j <= i mirrored
 *   into (j, i), and, where asked for, mean[n_var]:
 *   GSDR_COV_SUMS  out = the joined G, mean = the joined S.
 *   GSDR_COV_COV   m_j = S_j / n;  C_ij = fma(-S_i, m_j, G_ij) / (n - 1) for j <= i; a diagonal cell below 0 becomes +0, a
 *                  NaN stays;  mean_i = pivot_i + S_i / n.  n < 2: every cell is NaN; n == 0: the mean is NaN too.
 *   GSDR_COV_CORR  s_i = sqrt(C_ii) (of the diagonal as GSDR_COV_COV gives it); rho_ij = C_ij / p with p = s_i s_j one
 *                  double product stored first; the diagonal is exactly 1.0 where C_ii is finite and > 0 and NaN otherwise;
 *                  mean as for GSDR_COV_COV.
 *   What the pivot buys: the sums hold d = v - pivot, so C loses about n 2^-53 |mean - pivot|^2 / sigma^2 relative: with
 *   the pivots at the carriers 1e-12 sqrt(C_ii C_jj) holds with three decades to spare; with pivots of 0 on carriers
 *   1 000 sigma away the distance to numpy.cov is 2e-10 - 3e-9 (profiles/cov_margins.json): 9 digits, and the bar is missed.
 * Consequences.  No result depends, bit for bit, on where the stream is cut into feeds, or on anything about the launch
 *   except `lanes`.  The host twin returns the device's bits.  A non-finite sample of variable i takes what IEEE gives:
 *   it reaches S[i] and row and column i of G, and every other cell is bitwise that of the clean stream.  There is NO
 *   per-pair exclusion of non-finite samples (and no count of them: the stats object has one).
 *   The arithmetic is plain double FMAs in a fixed order per cell; the matrix-core FP64 instructions are not used,
 *   because the order in which they add their k terms is not documented.
 * gsdr_cov_create: 1 <= n_ch <= 2^20, 1 <= n_var <= GSDR_COV_MAX_VARS, 1 <= max_rows <= 2^20; lanes 0 (a host rule picks
 *   it, a pure function of n_var and max_rows: the smallest power of two with pairs x lanes >= 512 x 128 / tile workgroups
 *   -- pairs and tile as gsdr_cov_plan reports them -- at most the largest power of two <= max_rows, at most
 *   GSDR_COV_MAX_LANES, and within the bound on the cells) or a power of two in [1, GSDR_COV_MAX_LANES]; lanes x n_var (n_var + 1) / 2 <= 2^28
 *   cells (2 GiB of doubles); axes[n_var] not NULL, every field finite, reserved 0, channel in [0, n_ch);
 *   device_index >= -1 as in gsdr_param_c, or GSDR_COV_HOST for a host-only object that touches no GPU.  Anything else
 *   is refused before the device is touched: NULL, and gsdr_last_error(NULL) starts with "gsdr_cov_create: " and names
 *   the argument.  Everything every entry needs is allocated here (the chains, max_rows x n_var doubles of projected
 *   rows, the staging of gsdr_cov_read), every byte count in 64 bits; a failed allocation is a refusal that states the MiB.
 * gsdr_cov_feed_device: at most TWO launches on hip_stream (hipStream_t as void*): no allocation, no synchronisation, no
 *   read-back; reads exactly rows_dev[0, n_rows n_ch) (8-byte aligned, anywhere in a larger allocation) and writes
 *   nothing the caller can see; 0, or -1 with gsdr_last_error(NULL).  n_rows == 0 is valid and touches no pointer;
 *   n_rows outside [0, max_rows]: -1, state unchanged.
 * gsdr_cov_read_device: one launch on hip_stream; writes exactly out_dev[0, n_var^2) and, where mean_dev is not NULL,
 *   mean_dev[0, n_var) (both 8-byte aligned).  gsdr_cov_read: the same launch into the object's staging, then waits for
 *   hip_stream and copies to out_host and, where not NULL, mean_host.  kind is one of the three GSDR_COV_* kinds.
 * gsdr_cov_feed_host / _read_host: GSDR_COV_HOST objects only (and the device entries are refused on them): a BIT TWIN
 *   of the device.
 * gsdr_cov_reset(c, axes): restarts the row numbering at 0 and zeroes the chains; with axes not NULL the object takes new
 *   variables (n_var of them, checked as at creation; a refusal leaves everything as it was).  On a device object it
 *   waits for the device, zeroes, and waits again.
 * Stream order is the caller's, as for the stats object: the object remembers no stream and waits for none; rows_dev must
 *   stay unchanged until the feed that reads it has finished.  On a NULL object close is a no-op, the getters return 0,
 *   the rest return -1 with the reason.
 * gsdr_cov_plan: the launches of one feed (csrc/cov_state.h: the function the feed itself asks; host only).  out[0]
 *   tile T: 16, 32 or 64 -- the smallest that holds n_var -- or 128 beyond; out[1] tiles = ceil(n_var / T); out[2] pairs
 *   = tiles (tiles + 1) / 2, the accumulate grid's x; out[3] the accumulate grid's y = lanes; out[4] the bytes of LDS of
 *   an accumulate workgroup, 256 T; out[5] the variables a workgroup of the project pass spans (by 256 / out[5] rows): the
 *   smallest power of two that holds n_var, at most 256.  No result depends on any of them.  Returns 0, or -1 for a NULL out and for what gsdr_cov_create
 *   refuses of n_ch, n_var and lanes (lanes must be a power of two here: 0, the rule, needs max_rows: ask the object). */
#define GSDR_COV_HOST (-2)
#define GSDR_COV_MAX_VARS 4096
#define GSDR_COV_MAX_LANES 4096
#define GSDR_COV_SUMS 0
#define GSDR_COV_COV 1
#define GSDR_COV_CORR 2
typedef struct gsdr_cov_axis {
    int channel;
    float bx, by, dx, dy;
    int reserved; /* zero */
    double pivot;
} gsdr_cov_axis;
typedef struct gsdr_cov gsdr_cov;
gsdr_cov *gsdr_cov_create(int n_ch, int n_var, int max_rows, int lanes, const gsdr_cov_axis *axes, int device_index);
int gsdr_cov_feed_device(gsdr_cov *c, const gsdr_c64 *rows_dev, int n_rows, void *hip_stream);
int gsdr_cov_feed_host(gsdr_cov *c, const gsdr_c64 *rows, int n_rows);
int gsdr_cov_read_device(gsdr_cov *c, int kind, double *out_dev /* n_var x n_var */, double *mean_dev /* n_var, or NULL */,
                         void *hip_stream);
int gsdr_cov_read(gsdr_cov *c, int kind, double *out_host, double *mean_host /* or NULL */, void *hip_stream);
int gsdr_cov_read_host(gsdr_cov *c, int kind, double *out, double *mean /* or NULL */);
int gsdr_cov_reset(gsdr_cov *c, const gsdr_cov_axis *axes /* n_var, or NULL */);
long long gsdr_cov_rows(const gsdr_cov *c);
int gsdr_cov_lanes(const gsdr_cov *c);
int gsdr_cov_n_var(const gsdr_cov *c);
int gsdr_cov_plan(int n_ch, int n_var, int lanes, int out[6] /* tile, tiles, pairs, lanes, lds_bytes, project_x */);
void gsdr_cov_close(gsdr_cov *c);

#ifdef __cplusplus
}
#endif
#endif /* GSDR_H */
