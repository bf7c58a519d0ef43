// decim_host.cpp -- the FIR decimator's creation, default taps, count law and host twin (the contract: include/gsdr.h,
// "FIR decimation on the device"; the blocks and the ring: decim_state.h).  The host twin keeps the same ring of chunk
// sums as the device and walks the rows in stream order; every chain of fused multiply-adds and every addition is the
// one decim_partial_kernel / decim_combine_kernel (decim_kernels.hip) make, so the bits are the same.  No HIP here.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "decim_state.h"
#include "stage_host.h"

extern "C" {

int gsdr_decim_dev_create_(gsdr_decim *d) __attribute__((weak));

namespace {
// output row of block k (complete) out of the ring: the chunk sums oldest first
GSDR_NO_CONTRACT
void decim_emit_host(const gsdr_decim *d, long long k, gsdr_c64 *out) {
    GSDR_NO_CONTRACT_BODY
    const size_t n_ch = (size_t)d->n_ch, F = (size_t)d->F;
    for (size_t c = 0; c < n_ch; ++c) {
        float sx = 0.f, sy = 0.f;
        for (int j = d->F - 1; j >= 0; --j) {
            const long long kb = k - j;
            gsdr_c64 p{0.f, 0.f};
            if (kb >= 0) p = d->ring[((size_t)(kb % d->ring_blocks) * F + (size_t)j) * n_ch + c];
            if (j == d->F - 1) {
                sx = p.x, sy = p.y;
            } else {
                const float tx = sx + p.x, ty = sy + p.y;
                sx = tx, sy = ty;
            }
        }
        out[c].x = sx, out[c].y = sy;
    }
}
}  // namespace

int gsdr_decim_default_taps(int q, float *w) {
    if (q < 2 || q > 4096 || !w) return -1;
    const int T = 20 * q + 1, mid = 10 * q;
    std::vector<double> h((size_t)T);
    for (int n = 0; n <= mid; ++n) {
        const int m = n - mid;
        const double x = M_PI * (double)m / (double)q;
        const double s = m == 0 ? 1.0 : std::sin(x) / x;
        const double win = 0.54 - 0.46 * std::cos(2.0 * M_PI * (double)n / (double)(T - 1));
        h[(size_t)n] = h[(size_t)(T - 1 - n)] = s / (double)q * win;
    }
    double sum = 0.0;
    for (double v : h) sum += v;
    for (int n = 0; n < T; ++n) w[n] = (float)(h[(size_t)n] / sum);
    return T;
}

gsdr_decim *gsdr_decim_create(int n_ch, int max_rows, int q, int n_taps, const float *taps, long long offset, int device_index) {
    const char *const me = "gsdr_decim_create";
    std::string bad;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (q < 1 || q > 4096) bad = "q must be in [1, 4096]";
    else if (!taps && n_taps != 0) bad = "taps must not be NULL with n_taps != 0 (NULL and 0 select the default taps)";
    else if (!taps && q < 2) bad = "q must be >= 2 for the default taps (taps == NULL)";
    else if (taps && (n_taps < 1 || n_taps > 64 * q)) bad = "n_taps must be in [1, 64 q]";
    else if (offset < 0 || offset > (1LL << 30)) bad = "offset must be in [0, 1073741824]";
    else bad = stage_device_fault(device_index, "GSDR_DECIM_HOST", gsdr_decim_dev_create_ != nullptr);
    if (bad.empty() && taps)
        for (int t = 0; t < n_taps; ++t)
            if (!std::isfinite(taps[t])) {
                bad = "taps must all be finite";
                break;
            }
    if (!bad.empty()) {                                    // here, not in the frame: the sizes below divide by q
        stage_refuse(me, bad);
        return nullptr;
    }
    const int T = taps ? n_taps : 20 * q + 1, F = (T + q - 1) / q;
    const long long ring_blocks = (long long)(max_rows - 1) / q + 2 + F;
    const unsigned long long ring_bytes = (unsigned long long)ring_blocks * (unsigned long long)F * (unsigned long long)n_ch * sizeof(gsdr_c64);
    return stage_create<gsdr_decim>(
        me, bad, device_index, "n_ch, max_rows, q and n_taps: no host memory for the carried chunk sums (" + std::to_string(ring_bytes >> 20) + " MiB)",
        [&](gsdr_decim &d) {
            d.n_ch = n_ch, d.max_rows = max_rows, d.q = q, d.n_taps = T, d.offset = offset, d.F = F, d.ring_blocks = ring_blocks;
            d.taps.resize((size_t)T);
            if (taps) std::copy(taps, taps + T, d.taps.begin());
            else gsdr_decim_default_taps(q, d.taps.data());
            if (device_index != GSDR_DECIM_HOST) return;
            if (ring_bytes > (unsigned long long)PTRDIFF_MAX) throw std::bad_alloc();
            d.ring.assign((size_t)(ring_bytes / sizeof(gsdr_c64)), gsdr_c64{0.f, 0.f});
        },
        gsdr_decim_dev_create_);
}

int gsdr_decim_next_rows(const gsdr_decim *d, int n_rows) {
    if (!d) return 0;
    if (n_rows < 0 || n_rows > d->max_rows) return stage_refuse("gsdr_decim_next_rows", "n_rows must be in [0, max_rows]");
    return (int)(gsdr_decim_out_of(d->total + n_rows, d->offset, d->q) - gsdr_decim_out_of(d->total, d->offset, d->q));
}

long long gsdr_decim_out_capacity(const gsdr_decim *d) { return d ? (long long)(d->max_rows - 1) / d->q + 1 : 0; }

int gsdr_decim_get_taps(const gsdr_decim *d, float *w, int cap) {
    if (!d) return 0;
    if (w && cap > 0) std::copy(d->taps.begin(), d->taps.begin() + std::min(cap, d->n_taps), w);
    return d->n_taps;
}

int gsdr_decim_reset(gsdr_decim *d) {
    if (!d) return stage_refuse("gsdr_decim_reset", "null object");
    // the ring needs no clearing: a block's sums start at +0 with its first row, and no output reads a block before row 0
    d->total = 0;
    return 0;
}

long long gsdr_decim_rows(const gsdr_decim *d) { return d ? d->total : 0; }

long long gsdr_decim_rows_out(const gsdr_decim *d) { return d ? gsdr_decim_out_of(d->total, d->offset, d->q) : 0; }

void gsdr_decim_close(gsdr_decim *d) { stage_close(d); }

int gsdr_decim_feed_host(gsdr_decim *d, const gsdr_c64 *rows, int n_rows, gsdr_c64 *out) {
    const char *const me = "gsdr_decim_feed_host";
    if (const char *why = stage_host_fault(d, "a device object takes gsdr_decim_feed or gsdr_decim_feed_device")) return stage_refuse(me, why);
    if (n_rows < 0 || n_rows > d->max_rows) return stage_refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows) return stage_refuse(me, "null buffer: rows");
    const int emitted = (int)(gsdr_decim_out_of(d->total + n_rows, d->offset, d->q) - gsdr_decim_out_of(d->total, d->offset, d->q));
    if (emitted > 0 && !out) return stage_refuse(me, "null buffer: out");
    const size_t n_ch = (size_t)d->n_ch, F = (size_t)d->F;
    const long long q = d->q, r0 = gsdr_decim_r0(d->offset, d->q), shift = d->offset / q;
    const int T = d->n_taps;
    const float *h = d->taps.data();
    int at = 0;
    for (int i = 0; i < n_rows; ++i) {
        const long long R = d->total + i, k = (R - r0) / q;
        const int pos = (int)(R - r0 - k * q);                                 // the row's place in its block
        gsdr_c64 *blk = d->ring.data() + (size_t)(k % d->ring_blocks) * F * n_ch;
        if (pos == 0 || R == 0) std::fill(blk, blk + F * n_ch, gsdr_c64{0.f, 0.f});
        const gsdr_c64 *x = rows + (size_t)i * n_ch;
        for (int j = 0; j < d->F; ++j) {
            const long long t = (long long)T - (long long)(j + 1) * q + pos;
            if (t < 0) continue;
            const float w = h[t];
            gsdr_c64 *a = blk + (size_t)j * n_ch;
            for (size_t c = 0; c < n_ch; ++c) {
                a[c].x = std::fmaf(w, x[c].x, a[c].x);
                a[c].y = std::fmaf(w, x[c].y, a[c].y);
            }
        }
        if (pos == q - 1 && k - shift >= 0) decim_emit_host(d, k, out + (size_t)at++ * n_ch);
    }
    d->total += n_rows;
    return emitted;
}

}  // extern "C"
