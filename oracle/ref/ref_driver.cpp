/*
 * ref_driver.cpp -- plain C entry points over the reference's RX path, compiled
 * for the host by oracle/build_ref.py together with the reference's own
 * sources (the rewritten copies in oracle/_ref/src).  TEST INFRASTRUCTURE ONLY.
 *
 * Every entry calls reference code; nothing here restates it.  The one liberty
 * is reading RX_buffer_demodulator's private chirp parameters, for which the
 * class's access specifiers are opened in this translation unit only.
 */
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include <cublas_v2.h>
#include <cuda_runtime.h>
#include <cufft.h>
#include <curand_kernel.h>

/* standard and stand-in headers are complete above, so the switch reaches only the reference's classes */
#define private public
#include <USRP_demodulator.hpp>
#undef private

thread_local uint3 threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

namespace {
struct RefDemod {
    param p;
    RX_buffer_demodulator *d;
    std::vector<float2> in;
};
}  // namespace

extern "C" {

/* wave_type as the reference's enum: TONES 0, CHIRP 1, NOISE 2, NODSP 4, DIRECT 6.
 * TONES / DIRECT: one channel per entry of freq.  CHIRP: freq[0] is the start
 * frequency.  NOISE / NODSP: freq is ignored.  Returns NULL for what the
 * reference would not run (it exits or asserts there). */
void *ref_demod_create(int wave_type, int rate, long buffer_len, long decim, int fft_tones, long pf_average,
                       const int *freq, int n_freq, float chirp_t, int chirp_f, int swipe_s)
{
    if (buffer_len <= 0 || rate <= 0 || decim < 0 || pf_average < 0) return nullptr;
    const w_type wt = static_cast<w_type>(wave_type);
    RefDemod *h = new RefDemod();
    param &p = h->p;
    p.mode = RX;
    p.rate = rate;
    p.buffer_len = (size_t)buffer_len;
    p.decim = (size_t)decim;
    p.fft_tones = fft_tones;
    p.pf_average = (size_t)pf_average;
    int channels = 1;
    if (wt == DIRECT || wt == TONES) {
        if (n_freq < 1) { delete h; return nullptr; }
        channels = n_freq;
        if (wt == DIRECT && decim > 0 && buffer_len % decim) { delete h; return nullptr; }
    }
    for (int k = 0; k < channels; ++k) {
        p.freq.push_back((wt == NOISE || wt == NODSP) ? 0 : freq[k]);
        p.wave_type.push_back(wt);
    }
    if (wt == CHIRP) {
        p.chirp_t.push_back(chirp_t);
        p.chirp_f.push_back(chirp_f);
        p.swipe_s.push_back(swipe_s);
    }
    h->in.resize((size_t)buffer_len);
    h->d = new RX_buffer_demodulator(&p, false);
    return h;
}

/* one buffer of buffer_len samples; out must hold ref_demod_out_capacity()
 * samples (the reference copies more than it returns in TONES mode). */
int ref_demod_process(void *hv, const float2 *in, float2 *out)
{
    RefDemod *h = static_cast<RefDemod *>(hv);
    std::memcpy(h->in.data(), in, h->in.size() * sizeof(float2));
    float2 *ip = h->in.data(), *op = out;
    return h->d->process(&ip, &op);
}

long ref_demod_out_capacity(void *hv)
{
    RefDemod *h = static_cast<RefDemod *>(hv);
    const long L = (long)h->p.buffer_len, n = (long)h->p.wave_type.size();
    long cap = L * n;
    const w_type wt = h->p.wave_type[0];
    if (wt == TONES || wt == NOISE) {   /* batching is set in these modes only */
        const long frames = (long)h->d->batching * (n > h->p.fft_tones ? n : h->p.fft_tones);
        if (frames > cap) cap = frames;
    }
    return cap + L;
}

void ref_demod_close(void *hv)
{
    RefDemod *h = static_cast<RefDemod *>(hv);
    h->d->close();
    delete h->d;
    delete h;
}

/* the chirp parameters RX_buffer_demodulator derived (CHIRP mode only) */
void ref_demod_chirp_params(void *hv, unsigned long *num_steps, unsigned long *length, unsigned *chirpness, int *f0)
{
    const chirp_parameter &c = static_cast<RefDemod *>(hv)->d->h_parameter;
    *num_steps = c.num_steps;
    *length = c.length;
    *chirpness = c.chirpness;
    *f0 = c.f0;
}

/* real parts of the reference's windows */
void ref_make_sinc_window(int length, float fc, float *w)
{
    float2 *h = make_sinc_window(length, fc, false, true);
    for (int i = 0; i < length; ++i) w[i] = h[i].x;
    std::free(h);
}

void ref_make_flat_window(int length, int side, float *w)
{
    float2 *d = make_flat_window(length, side, false);
    for (int i = 0; i < length; ++i) w[i] = d[i].x;
    cudaFree(d);
}

/* buffer_helper after construction and after each of steps - 1 updates: ten
 * ints per step, in the order n_tones, eff_length, buffer_len, average,
 * n_eff_tones, new_0, copy_size, current_batch, spare_samples, spare_begin */
void ref_buffer_helper_seq(int n_tones, int buffer_len, int average, int n_eff_tones, int steps, int *out)
{
    buffer_helper b(n_tones, buffer_len, average, n_eff_tones);
    for (int s = 0; s < steps; ++s) {
        if (s) b.update();
        int *o = out + 10 * s;
        o[0] = b.n_tones; o[1] = b.eff_length; o[2] = b.buffer_len; o[3] = b.average; o[4] = b.n_eff_tones;
        o[5] = b.new_0; o[6] = b.copy_size; o[7] = b.current_batch; o[8] = b.spare_samples; o[9] = b.spare_begin;
    }
}

/* VNA_decimator_helper likewise: valid_size, new0, total_len, spare_begin per step */
void ref_vna_helper_seq(int ppt, int buffer_len, int steps, int *out)
{
    VNA_decimator_helper v(ppt, buffer_len);
    for (int s = 0; s < steps; ++s) {
        if (s) v.update();
        int *o = out + 4 * s;
        o[0] = v.valid_size; o[1] = v.new0; o[2] = v.total_len; o[3] = v.spare_begin;
    }
}

/* TX: the reference's chirp_gen kernel through its wrapper */
void ref_chirp_gen(unsigned long num_steps, unsigned long length, unsigned chirpness, int f0,
                   unsigned long last_index, unsigned n, float scale, float2 *out)
{
    chirp_parameter c;
    std::memset(&c, 0, sizeof(c));
    c.num_steps = num_steps;
    c.length = length;
    c.chirpness = chirpness;
    c.f0 = f0;
    chirp_gen_wrapper(out, n, &c, last_index, nullptr, scale);
}

/* TX: the reference's tone comb, one period of `rate` samples.  Returns -1,
 * writing nothing, for a tone whose bin falls outside the vector (0 Hz,
 * |f| >= rate): the reference writes out of bounds there. */
int ref_tone_gen(const int *freq, const float *ampl, int n_tones, int rate, float scale, float2 *out)
{
    for (int i = 0; i < n_tones; ++i) {
        const long b = freq[i] > 0 ? freq[i] : (long)rate + freq[i];
        if (b < 0 || b >= rate) return -1;
    }
    std::vector<int> f(freq, freq + n_tones);
    std::vector<float> a(ampl, ampl + n_tones);
    tone_parameters t;
    t.tones_number = n_tones;
    t.tone_frquencies = f.data();
    t.tones_amplitudes = a.data();
    float2 *h = tone_gen(&t, rate, scale, false);
    if (!h) return -1;
    std::memcpy(out, h, (size_t)rate * sizeof(float2));
    std::free(h);
    return 0;
}

}  // extern "C"
