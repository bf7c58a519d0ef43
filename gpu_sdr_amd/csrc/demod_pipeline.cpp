// demod_pipeline.cpp -- the pipelined entries of the RX handle (gsdr_demod_submit* / gsdr_demod_wait) and
// gsdr_demod_prepare: the streams and slots of the pipeline, the compute streams that consecutive DIRECT calls rotate
// over, and what orders the calls in flight.
#include <cstring>

#include "demod_state.h"

namespace gsdr {
namespace rx {

int record_staged(gsdr_demod *h, hipStream_t st) {
    if (h->pl.overlap) HIPCHK(h, hipEventRecord(h->pl.ev_abs[h->pl.seq % 4], st));
    return 0;
}

namespace {

// what pipeline_init's all-or-nothing rule needs: nothing of the pipeline is left
void pipeline_teardown(gsdr_demod *h) {
    for (auto &sl : h->pl.slot) {
        sl.up.reset(), sl.done.reset(), sl.down.reset();
        sl.wait_ev = nullptr;
    }
    for (auto &st : h->pl.s_main) st.reset();
    for (auto &e : h->pl.ev_abs) e.reset();
    h->pl.s_up.reset(), h->pl.s_down.reset();
    h->pl.ready = false;
}

int pipeline_init_parts(gsdr_demod *h);

// streams and events of the pipelined entries, created on first use; all or nothing: a partial
// failure leaves no half-built pipeline behind for the next call to trip over
int pipeline_init(gsdr_demod *h) {
    if (h->pl.ready) return 0;
    if (pipeline_init_parts(h)) {
        const std::string keep = h->err;
        pipeline_teardown(h);
        h->err = keep;
        return -1;
    }
    h->pl.ready = true;
    return 0;
}

int pipeline_init_parts(gsdr_demod *h) {
    HIPCHK(h, hipStreamCreateWithFlags(h->pl.s_up.out(), hipStreamNonBlocking));
    HIPCHK(h, hipStreamCreateWithFlags(h->pl.s_down.out(), hipStreamNonBlocking));
    for (auto &sl : h->pl.slot) {
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
            *h->pl.s_main[i].out() = s;
            continue;
        }
        (void)hipGetLastError();
        HIPCHK(h, hipStreamCreateWithPriority(h->pl.s_main[i].out(), hipStreamNonBlocking, prio_least));
    }
    for (int i = 0; i < 4; ++i) HIPCHK(h, hipEventCreateWithFlags(h->pl.ev_abs[i].out(), hipEventDisableTiming));
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
int pipeline_compute(gsdr_demod *h, gsdr::rx::Pipeline::Slot &sl, hipEvent_t up, const float2 *in, float2 *out,
                            const gsdr_sc16 *in16 = nullptr) {
    const bool ddc = (h->mode == GSDR_DIRECT && h->decim > 0) ||
                     h->mode == GSDR_TONES || h->mode == GSDR_NOISE;
    // TONES / NOISE inside the LDS keep the one compute stream: a launch is 10 - 15 us, the events that tie the calls
    // of rotating streams together (carry, completion) cost more than their overlap gives -- per 1 M-sample buffer
    // 16.3 against 12.0 us in order at 1024 points, 17.0 against 10.2 at 256, 25.7 against 15.4 at 1230
    // (profiles/r03_pfb_api_ab.log)
    // ... and so does a handle that averages frames (gsdr_demod_set_frame_average): its accumulators pass from call to
    // call in stream order
    const bool overlap = h->sw.pipe_overlap && h->mx.on && !h->pfb.lds && ddc && h->pfb.avg_k <= 1;
    hipStream_t cs = overlap ? h->pl.s_main[h->pl.seq % (unsigned)h->sw.pipe_streams] : h->stream;
    if (up) HIPCHK(h, hipStreamWaitEvent(cs, up, 0));
    if (overlap) {
        // behind in-order calls made on other streams since (their carry, slot and window writes);
        // the compute streams of the pipeline are ordered by the protocol above
        if (join_streams(h, cs, /*keep_pipeline=*/true)) return -1;
    }
    if (overlap && h->pl.seq > 0) HIPCHK(h, hipStreamWaitEvent(cs, h->pl.ev_abs[(h->pl.seq - 1) % 4], 0));
    h->pl.overlap = overlap;
    const int n = process_device_body(h, in, in16, nullptr, out, cs);
    h->pl.overlap = false;
    if (overlap) h->pl.seq++;
    if (n < 0) return -1;
    HIPCHK(h, hipEventRecord(sl.done, cs));
    return n;
}

// the device buffers of a pipeline slot, each created when the first entry that needs it asks for it
int slot_buffers(gsdr_demod *h, gsdr::rx::Pipeline::Slot &sl, bool in, bool out, bool in16) {
    if (in && !sl.d_in) HIPCHK(h, sl.d_in.alloc((size_t)h->L));
    if (out && !sl.d_out) HIPCHK(h, sl.d_out.alloc((size_t)h->capacity));
    if (in16 && !sl.d_in16) HIPCHK(h, sl.d_in16.alloc((size_t)h->L));
    return 0;
}

}  // namespace

}  // namespace rx
}  // namespace gsdr

using namespace gsdr::rx;

extern "C" {

int gsdr_demod_prepare(gsdr_demod *h, int what) {
    if (!h) return -1;
    if (h->device >= 0) HIPCHK(h, hipSetDevice(h->device));
    if (h->mode == GSDR_NODSP) return 0;
    if ((what & GSDR_PREPARE_HOST) && staging_pair(h)) return -1;
    if (what & (GSDR_PREPARE_PIPELINE | GSDR_PREPARE_PIPELINE_HOST)) {
        if (pipeline_init(h)) return -1;
    }
    const bool sc16 = (what & GSDR_PREPARE_SC16) != 0;
    if (sc16 && (what & GSDR_PREPARE_HOST) && !h->host.d_in16) HIPCHK(h, h->host.d_in16.alloc((size_t)h->L));
    if (sc16 && !h->d_wide) HIPCHK(h, h->d_wide.alloc((size_t)h->L));
    for (auto &sl : h->pl.slot) {
        const bool host = (what & GSDR_PREPARE_PIPELINE_HOST) != 0;
        if (slot_buffers(h, sl, host || (sc16 && (what & GSDR_PREPARE_PIPELINE)), host, host && sc16)) return -1;
    }
    // first use of a stream (its hardware queue), of the copy engines in both directions and of
    // the code object costs milliseconds: pay them here, not on the first packets
    HIPCHK(h, gsdr::launch_warm(h->stream));
    // the averaging kernel's first launch, on a frame of zeros; nothing has gone through the handle yet (otherwise the
    // kernel has run already), so no group is open and the sums it leaves in the other accumulator are never read
    if (h->pfb.avg_k > 1 && h->pfb.win_seq == 0) {
        HIPCHK(h, hipMemsetAsync(h->pfb.d_avg_frames, 0, (size_t)h->ddc.channels * sizeof(float2), h->stream));
        HIPCHK(h, gsdr::launch_pfb_average(h->pfb.d_avg_frames, 1, h->ddc.channels, h->pfb.avg_k, h->pfb.avg_kind, 0, h->pfb.d_avg_acc[0],
                                           h->pfb.d_avg_acc[1], h->pfb.d_avg_frames, h->stream));
    }
    if (h->pl.ready) {
        for (int i = 0; i < kPipeStreams; ++i) HIPCHK(h, gsdr::launch_warm(h->pl.s_main[i]));
        float2 *pin = nullptr;
        // (no more than the slot holds: a copy past a buffer of fewer than 512 samples is refused, and the error it
        // leaves behind was reported by the next launch that asked for one -- the rehearsal's)
        const size_t warm = (size_t)h->L * sizeof(float2) < 4096 ? (size_t)h->L * sizeof(float2) : 4096;
        if (h->pl.slot[0].d_in && hipHostMalloc((void **)&pin, 4096) == hipSuccess) {
            std::memset(pin, 0, 4096);
            (void)hipMemcpyAsync(h->pl.slot[0].d_in, pin, warm, hipMemcpyHostToDevice, h->pl.s_up);
            (void)hipStreamSynchronize(h->pl.s_up);
            (void)hipMemcpyAsync(pin, h->pl.slot[0].d_in, warm, hipMemcpyDeviceToHost, h->pl.s_down);
            (void)hipStreamSynchronize(h->pl.s_down);
            (void)hipHostFree(pin);
        }
    }
    HIPCHK(h, hipDeviceSynchronize());
    if (what & GSDR_PREPARE_REHEARSE) {
        // a twin with the same parameters takes the process-wide first-use costs (see include/gsdr.h)
        gsdr_demod *twin = demod_create(&h->pc, h->sw, h->flags);
        gsdr_c64 *pin_in = nullptr, *pin_out = nullptr;
        bool ok = twin != nullptr;
        ok = ok && (h->pfb.avg_k <= 1 || gsdr_demod_set_frame_average(twin, h->pfb.avg_k, h->pfb.avg_kind) == 0);
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
        if (!ok) h->err = std::string("rehearsal failed: ") + (twin ? twin->err : gsdr::create_error());
        if (pin_in) (void)hipHostFree(pin_in);
        if (pin_out) (void)hipHostFree(pin_out);
        if (twin) gsdr_demod_close(twin);
        if (!ok) return -1;
    }
    return 0;
}

// What every submit entry starts with: the refusals, the device, the pipeline, and the slot the buffer goes to.  The slot
// is free: its previous download (or kernels) were waited for in gsdr_demod_wait().
static int submit_begin(gsdr_demod *h, const void *in, const void *out, gsdr::rx::Pipeline::Slot **slot) {
    if (refuse_null(h, in, out)) return -1;
    if (h->pl.count >= GSDR_PIPELINE_DEPTH) {
        h->err = "pipeline full: call gsdr_demod_wait() first";
        return -1;
    }
    if (h->device >= 0) HIPCHK(h, hipSetDevice(h->device));
    if (pipeline_init(h)) return -1;
    *slot = &h->pl.slot[(h->pl.head + h->pl.count) % GSDR_PIPELINE_DEPTH];
    return 0;
}

// ... and ends with: the n samples of the slot are there when wait_ev has happened
static int submit_end(gsdr_demod *h, gsdr::rx::Pipeline::Slot &sl, hipEvent_t wait_ev, int n) {
    sl.wait_ev = wait_ev;
    sl.n = n;
    h->pl.count++;
    return 0;
}

// gsdr_demod_submit and gsdr_demod_submit_sc16 (in16_host != nullptr)
static int submit_host(gsdr_demod *h, const gsdr_c64 *in_host, const gsdr_sc16 *in16_host, gsdr_c64 *out_host) {
    gsdr::rx::Pipeline::Slot *slot = nullptr;
    if (submit_begin(h, in16_host ? (const void *)in16_host : in_host, out_host, &slot)) return -1;
    auto &sl = *slot;
    if (slot_buffers(h, sl, true, true, in16_host != nullptr)) return -1;
    if (in16_host) {
        // half the bytes, then the widening, both on the upload stream in front of sl.up: it overlaps the kernels of
        // the buffer before and does not lengthen the compute stream
        HIPCHK(h, hipMemcpyAsync(sl.d_in16, in16_host, (size_t)h->L * sizeof(gsdr_sc16), hipMemcpyHostToDevice, h->pl.s_up));
        HIPCHK(h, gsdr::launch_widen_sc16(sl.d_in16, sl.d_in, h->L, h->sc16_scale, h->cus, h->pl.s_up));
    } else {
        HIPCHK(h, hipMemcpyAsync(sl.d_in, in_host, (size_t)h->L * sizeof(float2), hipMemcpyHostToDevice, h->pl.s_up));
    }
    HIPCHK(h, hipEventRecord(sl.up, h->pl.s_up));
    const int n = pipeline_compute(h, sl, sl.up, sl.d_in, sl.d_out);
    if (n < 0) return -1;
    HIPCHK(h, hipStreamWaitEvent(h->pl.s_down, sl.done, 0));
    if (n > 0)
        HIPCHK(h, hipMemcpyAsync(out_host, sl.d_out, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, h->pl.s_down));
    HIPCHK(h, hipEventRecord(sl.down, h->pl.s_down));
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
    gsdr::rx::Pipeline::Slot *slot = nullptr;
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
        HIPCHK(h, gsdr::launch_widen_sc16(in16_dev, sl.d_in, h->L, h->sc16_scale, h->cus, h->pl.s_up));
        HIPCHK(h, hipEventRecord(sl.up, h->pl.s_up));
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
    if (h->pl.count == 0) return -2;
    if (h->device >= 0) HIPCHK(h, hipSetDevice(h->device));
    auto &sl = h->pl.slot[h->pl.head];
    const hipError_t e = hipEventSynchronize(sl.wait_ev);
    // the slot leaves the queue whatever happened: a failed wait must not leave the pipeline "full"
    h->pl.head = (h->pl.head + 1) % GSDR_PIPELINE_DEPTH;
    h->pl.count--;
    if (e != hipSuccess) {
        h->err = std::string("hipEventSynchronize: ") + hipGetErrorString(e);
        return -1;
    }
    return sl.n;
}

}  // extern "C"
