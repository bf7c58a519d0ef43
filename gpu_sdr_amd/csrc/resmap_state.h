// resmap_state.h -- the resonator map (include/gsdr.h, "resonator map on the device") as resmap_host.cpp, resmap.cpp and
// resmap_kernels.hip share it: the object, a column's constants as the tables hold them, and THE PER-SAMPLE LAW, one
// inline host-and-device function that the kernel and the host twin both include -- there is one text of the
// arithmetic.  resmap_host.cpp owns creation, the refusals, gsdr_resmap_constants and the host twin; resmap.cpp hangs the
// device part on `dev` through the hooks below (its release: stage_state.h).  No HIP here: resmap_host.cpp is built without resmap.cpp by a host compiler
// (tests/test_resmap_sanitizers.py), where the hooks are absent and only host objects exist.
#ifndef GSDR_RESMAP_STATE_H
#define GSDR_RESMAP_STATE_H

#include <vector>

#include "../../include/gsdr.h"
#include "stage_state.h"

#if defined(__HIPCC__)
#define GSDR_RESMAP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GSDR_RESMAP_HD inline
#endif

// one output column's constants, 64 bytes: what the device table and the twin hold
struct gsdr_resmap_col {
    double nr, ni, gr, gi, kr, ki, hf0, unused;
};
static_assert(sizeof(gsdr_resmap_col) == 64, "a column of the table is 8 doubles");

struct gsdr_resmap {
    int n_ch = 0, max_rows = 0, n_out = 0, kind = 0;
    int device = GSDR_RESMAP_HOST;
    bool identity = false;                    // channels[k] == k for all k and n_out == n_ch
    std::vector<int> channels;                // [n_out], the identity written out
    std::vector<gsdr_resmap_col> cols;        // [n_out]
    std::vector<double> offsets;              // [n_out][x0, y0]: what set_offsets was given last
    gsdr::StageDev *dev = nullptr;            // gsdr::ResmapDev (resmap.cpp)
};

// The law of include/gsdr.h, operation for operation.  No product here feeds a plain addition or subtraction: each is
// an operand of an explicit fused multiply-add (its addend, or one that is negated first) -- so a compiler that
// contracts has nothing to contract, and __builtin_fma is one IEEE operation on either side (v_fma_f64 on the device,
// fma() or the FMA instruction on the host).  The divisions are IEEE double divisions on both (hipcc expands them to
// the correctly rounded sequence unless fast math is asked for, and it is not).  KIND is a constant where the kernel
// calls this.
GSDR_RESMAP_HD void gsdr_resmap_sample(int kind, const gsdr_resmap_col &c, double x0, double y0, float sxf, float syf, float &ox, float &oy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double sx = (double)sxf, sy = (double)syf;
    if (kind == GSDR_RESMAP_CAL) {
        const double pr = sy * c.gi, pi = sy * c.gr;
        const double zr = __builtin_fma(sx, c.gr, -pr);
        const double zi = __builtin_fma(sx, c.gi, pi);
        const double rx = zr - x0, ry = zi - y0;
        ox = (float)rx, oy = (float)ry;
        return;
    }
    const double wr = c.nr - sx, wi = c.ni - sy;
    const double ww = wi * wi, kw = c.ki * wi, lw = c.kr * wi;
    const double m = __builtin_fma(wr, wr, ww);
    const double a = __builtin_fma(c.kr, wr, kw);
    const double b = __builtin_fma(c.ki, wr, -lw);
    const double qi = b / m;
    const double fx = __builtin_fma(c.hf0, qi, -x0);
    double y;
    if (kind == GSDR_RESMAP_X_DQR) {
        const double qr = a / m;
        y = qr - y0;
    } else {
        const double Q = m / a;
        y = Q - y0;
    }
    ox = (float)fx, oy = (float)y;
}

extern "C" {
// resmap.cpp; weak in resmap_host.cpp.  _create_: allocates and uploads the tables (offsets zero), 0 or -1 with the
// message noted; it is called after every bound has been checked.  _set_offsets_: r->offsets to the device, ordered on
// the stream.
int gsdr_resmap_dev_create_(gsdr_resmap *r);
int gsdr_resmap_dev_set_offsets_(gsdr_resmap *r, void *hip_stream);
}

#endif
