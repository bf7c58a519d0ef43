// demod_chirp.cpp -- CHIRP: the undecimated demodulation and the lock-in of one chirp or of several at once.
//
// "ref:" citations name the reference's files, as in demod.cpp.
#include "demod_state.h"

namespace gsdr {
namespace rx {

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
    h->ch.cs = chirp_shape(cp);
    // several chirps (demod_create has checked what they must share): chirp c differs in f0 and chirpness alone
    const bool multi = h->ch.chirps > 1;
    if (multi) {
        gsdr_chirp_param all[GSDR_MULTI_CHIRP_MAX];
        for (int c = 0; c < h->ch.chirps; ++c)
            gsdr_chirp_derive(p->rate, p->freq[c], p->chirp_f[c], p->swipe_s[0], p->chirp_t[0], &all[c]);
        if (const char *bad = gsdr::multi_chirp_shape(all, h->ch.chirps, h->ch.mc)) return refuse(h, bad);
    }
    if (h->decim <= 0) {
        h->kernel_name = multi ? gsdr::chirp_multi_demod_kernel_name() : gsdr::chirp_demod_kernel_name();
        h->capacity = h->L * h->ch.chirps;
        return 0;
    }
    const unsigned long long ppt = cp.length * (unsigned long long)h->decim;  // :231
    if (!(ppt >= 1 && ppt <= (unsigned long long)h->L)) return refuse(h, "chirp lock-in needs length*decim <= buffer_len");
    h->ch.ppt = (int)ppt;
    gsdr_vna_helper_init(&h->ch.vh, h->ch.ppt, (int)h->L);       // :235
    h->window.resize(h->ch.ppt);
    gsdr_make_flat_window(h->ch.ppt, h->ch.ppt / 10, h->window.data());  // :246
    h->kernel_name = multi ? gsdr::chirp_multi_lockin_kernel_name() : gsdr::chirp_lockin_kernel_name();
    h->capacity = (h->L / h->ch.ppt + 1) * h->ch.chirps;
    if (h->ch.d_profile.upload(h->window) != hipSuccess || h->ch.d_carry[0].alloc((size_t)h->ch.ppt) != hipSuccess ||
        h->ch.d_carry[1].alloc((size_t)h->ch.ppt) != hipSuccess || h->ch.d_part.alloc((size_t)kChirpPartials) != hipSuccess)
        return refuse(h, "chirp allocation failed");
    return 0;
}

// ref: process_chirp, cpp/USRP_demodulator.cpp:342-397
int enqueue_chirp(gsdr_demod *h, const float2 *in, float2 *out, hipStream_t st) {
    hipEvent_t stop = nullptr;
    int ret;
    gsdr::ChirpPlan plan;                // the form the launcher took (gsdr_demod_describe: chirp_calls, chirp_parts)
    if (h->decim <= 0) {
        if (record_begin(h, st, &stop)) return -1;
        if (h->ch.chirps > 1) HIPCHK(h, gsdr::launch_chirp_multi_demod(in, out, h->L, h->ch.last_index, h->ch.mc, st, &plan));
        else HIPCHK(h, gsdr::launch_chirp_demod(in, out, h->L, h->ch.last_index, h->ch.cs, st, &plan));
        if (stop) HIPCHK(h, hipEventRecord(stop, st));
        ret = (int)(h->L * h->ch.chirps);   // :390
    } else {
        const int valid = h->ch.vh.valid_size;      // :361
        // chirp index of the first carried sample
        const unsigned long long idx0 =
            (h->ch.last_index + h->ch.cs.period - (unsigned long long)h->ch.carry_len % h->ch.cs.period) %
            h->ch.cs.period;
        if (record_begin(h, st, &stop)) return -1;
        if (h->ch.chirps > 1)
            HIPCHK(h, gsdr::launch_chirp_multi_lockin(h->ch.d_carry[h->ch.parity], h->ch.carry_len, in, h->ch.d_profile, h->ch.ppt, valid,
                                                      out, idx0, h->ch.mc, st, h->sw.chirp_split, h->ch.d_part,
                                                      h->ch.d_part ? kChirpPartials : 0, &plan));
        else
            HIPCHK(h, gsdr::launch_chirp_lockin(h->ch.d_carry[h->ch.parity], h->ch.carry_len, in,
                                                h->ch.d_profile, h->ch.ppt, valid, out, idx0, h->ch.cs, st, h->sw.chirp_split,
                                                h->ch.d_part, h->ch.d_part ? kChirpPartials : 0, &plan));
        if (stop) HIPCHK(h, hipEventRecord(stop, st));
        // :369-380 the reference keeps the last new0 DEMODULATED samples; we
        // keep the same raw samples and re-demodulate them next call.
        const int new0 = h->ch.vh.new0;
        if (new0 > 0) {
            // they are the tail of the logical stage [carry | in]
            const long long from_in = (long long)new0 <= h->L ? new0 : h->L;
            const long long from_carry = new0 - from_in;
            float2 *dst = h->ch.d_carry[h->ch.parity ^ 1];
            if (from_carry > 0)
                HIPCHK(h, hipMemcpyAsync(dst, h->ch.d_carry[h->ch.parity] + (h->ch.carry_len - from_carry),
                                         (size_t)from_carry * sizeof(float2),
                                         hipMemcpyDeviceToDevice, st));
            HIPCHK(h, hipMemcpyAsync(dst + from_carry, in + (h->L - from_in),
                                     (size_t)from_in * sizeof(float2), hipMemcpyDeviceToDevice,
                                     st));
            h->ch.parity ^= 1;
        }
        h->ch.carry_len = new0;
        gsdr_vna_helper_update(&h->ch.vh);  // :382
        ret = valid * h->ch.chirps;         // rows [point][chirp]
    }
    h->ch.last_index = (h->ch.last_index + (unsigned long long)h->L) % h->ch.cs.period;  // :355
    if (plan.form >= 0 && plan.form < 3) {
        h->ch.calls[plan.form]++;
        h->ch.parts = plan.parts;
    }
    return ret;
}

void describe_chirp(const gsdr_demod *h, std::string &s) {
    s += ", \"chirps\": " + std::to_string(h->ch.chirps);
    // calls so far by the lock-in (or undecimated) form that ran, and the waves per point of the last one
    s += ", \"chirp_calls\": {\"plain\": " + std::to_string(h->ch.calls[gsdr::kChirpPlain]) + ", \"split\": " +
         std::to_string(h->ch.calls[gsdr::kChirpSplit]) + ", \"generic\": " +
         std::to_string(h->ch.calls[gsdr::kChirpGeneric]) + "}";
    s += ", \"chirp_parts\": " + std::to_string(h->ch.parts);
}

}  // namespace rx
}  // namespace gsdr
