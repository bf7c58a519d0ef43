// resmap_host.cpp -- the resonator map's constants, creation, offsets and host twin (the contract: include/gsdr.h,
// "resonator map on the device"; the per-sample law: gsdr_resmap_sample, resmap_state.h).  The twin calls the function
// resmap_kernel (resmap_kernels.hip) calls, on the same tables: the bits are the same.  No HIP here.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "resmap_state.h"
#include "stage_host.h"

extern "C" {

int gsdr_resmap_dev_create_(gsdr_resmap *r) __attribute__((weak));
int gsdr_resmap_dev_set_offsets_(gsdr_resmap *r, void *hip_stream) __attribute__((weak));

GSDR_NO_CONTRACT
int gsdr_resmap_constants(double f_tone, double f0, double A, double phi, double D, double Qe_re, double Qe_im, double *constants) {
    GSDR_NO_CONTRACT_BODY
    const char *const me = "gsdr_resmap_constants";
    const char *bad = nullptr;
    if (!std::isfinite(f_tone)) bad = "f_tone must be finite";
    else if (!std::isfinite(f0) || !(f0 > 0.0)) bad = "f0 must be finite and > 0 (MHz)";
    else if (!std::isfinite(A) || !(A > 0.0)) bad = "A must be finite and > 0";
    else if (!std::isfinite(phi)) bad = "phi must be finite";
    else if (!std::isfinite(D)) bad = "D must be finite";
    else if (!std::isfinite(Qe_re)) bad = "Qe_re must be finite";
    else if (!std::isfinite(Qe_im)) bad = "Qe_im must be finite";
    else if (Qe_re == 0.0 && Qe_im == 0.0) bad = "Qe_re and Qe_im: Qe must not be 0";
    else if (!constants) bad = "constants must not be NULL";
    if (bad) return stage_refuse(me, bad);
    const double f0_hz = f0 * 1e6;
    const double df = f_tone - f0_hz;
    const double slope = 1e-6 * D;
    const double cable = slope * df;
    const double theta = cable + phi;
    const double arg = 2.0 * M_PI * theta;
    const double nr = A * std::cos(arg), ni = A * std::sin(arg);
    const double nr2 = nr * nr, ni2 = ni * ni;
    const double nn = nr2 + ni2;
    const double qr2 = Qe_re * Qe_re, qi2 = Qe_im * Qe_im;
    const double qq = qr2 + qi2;
    const double rr = nr * Qe_re, ii = ni * Qe_im, ir = ni * Qe_re, ri = nr * Qe_im;
    const double kr_num = rr + ii, ki_num = ir - ri;
    constants[0] = nr;
    constants[1] = ni;
    constants[2] = nr / nn;
    constants[3] = -ni / nn;
    constants[4] = kr_num / qq;
    constants[5] = ki_num / qq;
    constants[6] = f0_hz / 2.0;
    return 0;
}

gsdr_resmap *gsdr_resmap_create(int n_ch, int max_rows, int n_out, const int *channels, const double *constants, int kind, int device_index) {
    std::string bad;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (n_out < 1 || n_out > (1 << 20)) bad = "n_out must be in [1, 1048576]";
    else if (!channels && n_out != n_ch) bad = "channels must not be NULL with n_out != n_ch (NULL is the identity)";
    else if (!constants) bad = "constants must not be NULL";
    else if (kind != GSDR_RESMAP_CAL && kind != GSDR_RESMAP_X_DQR && kind != GSDR_RESMAP_X_QR) bad = "kind must be GSDR_RESMAP_CAL, GSDR_RESMAP_X_DQR or GSDR_RESMAP_X_QR";
    else bad = stage_device_fault(device_index, "GSDR_RESMAP_HOST", gsdr_resmap_dev_create_ != nullptr);
    if (bad.empty() && channels)
        for (int k = 0; k < n_out; ++k)
            if (channels[k] < 0 || channels[k] >= n_ch) {
                bad = "channels must all be in [0, n_ch)";
                break;
            }
    if (bad.empty())
        for (size_t i = 0; i < (size_t)n_out * GSDR_RESMAP_NCONST; ++i)
            if (!std::isfinite(constants[i])) {
                bad = "constants must all be finite";
                break;
            }
    return stage_create<gsdr_resmap>(
        "gsdr_resmap_create", bad, device_index, "n_out: no host memory for the tables (" + std::to_string(((size_t)n_out * 84) >> 20) + " MiB)",
        [&](gsdr_resmap &r) {
            r.n_ch = n_ch, r.max_rows = max_rows, r.n_out = n_out, r.kind = kind;
            r.channels.resize((size_t)n_out);
            r.cols.resize((size_t)n_out);
            r.offsets.assign(2 * (size_t)n_out, 0.0);
            r.identity = n_out == n_ch;
            for (int k = 0; k < n_out; ++k) {
                r.channels[(size_t)k] = channels ? channels[k] : k;
                r.identity = r.identity && r.channels[(size_t)k] == k;
                const double *c = constants + (size_t)k * GSDR_RESMAP_NCONST;
                r.cols[(size_t)k] = gsdr_resmap_col{c[0], c[1], c[2], c[3], c[4], c[5], c[6], 0.0};
            }
        },
        gsdr_resmap_dev_create_);
}

void gsdr_resmap_close(gsdr_resmap *r) { stage_close(r); }

int gsdr_resmap_set_offsets(gsdr_resmap *r, const double *xy, void *hip_stream) {
    const char *const me = "gsdr_resmap_set_offsets";
    if (!r) return stage_refuse(me, "null object");
    if (xy)
        for (size_t i = 0; i < 2 * (size_t)r->n_out; ++i)
            if (!std::isfinite(xy[i])) return stage_refuse(me, "xy must all be finite");
    if (xy) std::copy(xy, xy + 2 * (size_t)r->n_out, r->offsets.begin());
    else std::fill(r->offsets.begin(), r->offsets.end(), 0.0);
    if (!r->dev) return 0;
    return gsdr_resmap_dev_set_offsets_ ? gsdr_resmap_dev_set_offsets_(r, hip_stream) : stage_refuse(me, "no device part in this build");
}

int gsdr_resmap_n_out(const gsdr_resmap *r) { return r ? r->n_out : 0; }

int gsdr_resmap_kind(const gsdr_resmap *r) { return r ? r->kind : 0; }

int gsdr_resmap_get_constants(const gsdr_resmap *r, double *constants, int cap) {
    if (!r) return 0;
    for (int k = 0; constants && k < std::min(cap, r->n_out); ++k) {
        const gsdr_resmap_col &c = r->cols[(size_t)k];
        const double v[GSDR_RESMAP_NCONST] = {c.nr, c.ni, c.gr, c.gi, c.kr, c.ki, c.hf0};
        std::copy(v, v + GSDR_RESMAP_NCONST, constants + (size_t)k * GSDR_RESMAP_NCONST);
    }
    return r->n_out;
}

int gsdr_resmap_get_offsets(const gsdr_resmap *r, double *xy, int cap) {
    if (!r) return 0;
    if (xy && cap > 0) std::copy(r->offsets.begin(), r->offsets.begin() + 2 * (std::ptrdiff_t)std::min(cap, r->n_out), xy);
    return r->n_out;
}

int gsdr_resmap_get_channels(const gsdr_resmap *r, int *channels, int cap) {
    if (!r) return 0;
    if (channels && cap > 0) std::copy(r->channels.begin(), r->channels.begin() + std::min(cap, r->n_out), channels);
    return r->n_out;
}

int gsdr_resmap_feed_host(gsdr_resmap *r, const gsdr_c64 *rows, int n_rows, gsdr_c64 *out) {
    const char *const me = "gsdr_resmap_feed_host";
    if (const char *why = stage_host_fault(r, "a device object takes gsdr_resmap_feed or gsdr_resmap_feed_device")) return stage_refuse(me, why);
    if (n_rows < 0 || n_rows > r->max_rows) return stage_refuse(me, "n_rows must be in [0, max_rows]");
    if (n_rows == 0) return 0;
    if (!rows) return stage_refuse(me, "null buffer: rows");
    if (!out) return stage_refuse(me, "null buffer: out");
    const size_t n_ch = (size_t)r->n_ch, n_out = (size_t)r->n_out;
    if (!(rows == out && r->identity)) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(rows), b = reinterpret_cast<uintptr_t>(out);
        const uintptr_t na = (uintptr_t)n_rows * n_ch * sizeof(gsdr_c64), nb = (uintptr_t)n_rows * n_out * sizeof(gsdr_c64);
        if (a < b + nb && b < a + na) return stage_refuse(me, "out overlaps rows (out == rows is allowed with the identity channel list only)");
    }
    for (size_t i = 0; i < (size_t)n_rows; ++i) {
        const gsdr_c64 *x = rows + i * n_ch;
        gsdr_c64 *y = out + i * n_out;
        for (size_t k = 0; k < n_out; ++k) {
            const gsdr_c64 s = x[(size_t)r->channels[k]];
            gsdr_resmap_sample(r->kind, r->cols[k], r->offsets[2 * k], r->offsets[2 * k + 1], s.x, s.y, y[k].x, y[k].y);
        }
    }
    return n_rows;
}

}  // extern "C"
