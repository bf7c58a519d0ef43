// fft_lds.h -- the pieces of the in-LDS transform that more than one kernel file uses: the complex helpers, the radix
// butterflies and one Stockham stage between two LDS buffers.  fft_kernels.hip (the PFB of TONES / NOISE) and
// welch_kernels.hip (the Welch segments) include it; the text is the one fft_kernels.hip held, so both get the same
// instructions.  Device code only, internal to csrc/.
#pragma once
#include <hip/hip_runtime.h>

namespace gsdr {
namespace {

// (make_float2 of the HIP headers is not always_inline: inside a kernel with other target features it
//  would stay a real call, s_swappc_b64 -- `make asm` + grep is the check)
__device__ __forceinline__ float2 mk2(float x, float y) {
    float2 v;
    v.x = x;
    v.y = y;
    return v;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return mk2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

template <int R>
__device__ __forceinline__ void butterfly(float2 (&u)[R], const float2 *__restrict__ tw, int n) {
    if constexpr (R == 2) {
        const float2 a = u[0], b = u[1];
        u[0] = mk2(a.x + b.x, a.y + b.y);
        u[1] = mk2(a.x - b.x, a.y - b.y);
    } else if constexpr (R == 4) {
        // forward DFT-4: w = -i
        const float2 a0 = mk2(u[0].x + u[2].x, u[0].y + u[2].y), a1 = mk2(u[0].x - u[2].x, u[0].y - u[2].y);
        const float2 b0 = mk2(u[1].x + u[3].x, u[1].y + u[3].y), b1 = mk2(u[1].x - u[3].x, u[1].y - u[3].y);
        u[0] = mk2(a0.x + b0.x, a0.y + b0.y);
        u[2] = mk2(a0.x - b0.x, a0.y - b0.y);
        u[1] = mk2(a1.x + b1.y, a1.y - b1.x);   // a1 - i*b1
        u[3] = mk2(a1.x - b1.y, a1.y + b1.x);   // a1 + i*b1
    } else if constexpr (R == 8) {
        // DFT-8 = two DFT-4 (even / odd inputs) + four constant twiddles: X[k] = E[k] + w8^k O[k], X[k+4] = E[k] - w8^k O[k]
        float2 e[4] = {u[0], u[2], u[4], u[6]}, o[4] = {u[1], u[3], u[5], u[7]};
        butterfly<4>(e, tw, n);
        butterfly<4>(o, tw, n);
        constexpr float h = 0.70710678118654752440f;
        const float2 t0 = o[0];
        const float2 t1 = mk2((o[1].x + o[1].y) * h, (o[1].y - o[1].x) * h);      // * (1 - i) / sqrt 2
        const float2 t2 = mk2(o[2].y, -o[2].x);                                   // * -i
        const float2 t3 = mk2((o[3].y - o[3].x) * h, -(o[3].x + o[3].y) * h);     // * (-1 - i) / sqrt 2
        const float2 t[4] = {t0, t1, t2, t3};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            u[k] = mk2(e[k].x + t[k].x, e[k].y + t[k].y);
            u[k + 4] = mk2(e[k].x - t[k].x, e[k].y - t[k].y);
        }
    } else if constexpr (R == 6 || R == 10) {
        // DFT-2P (P = 3, 5) = two DFT-P (even / odd inputs) + constant twiddles: X[k] = E[k mod P] + w_2P^k O[k mod P]
        constexpr int P = R / 2;
        float2 e[P], o[P];
#pragma unroll
        for (int i = 0; i < P; ++i) {
            e[i] = u[2 * i];
            o[i] = u[2 * i + 1];
        }
        butterfly<P>(e, tw, n);
        butterfly<P>(o, tw, n);
        // w_2P^k = (cos, -sin)(2 pi k / 2P), k < P (the other half is its negative)
        constexpr float c6[3] = {1.f, 0.5f, -0.5f}, s6[3] = {0.f, 0.86602540378443864676f, 0.86602540378443864676f};
        constexpr float c10[5] = {1.f, 0.80901699437494742410f, 0.30901699437494742410f, -0.30901699437494742410f, -0.80901699437494742410f};
        constexpr float s10[5] = {0.f, 0.58778525229247312917f, 0.95105651629515357212f, 0.95105651629515357212f, 0.58778525229247312917f};
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const float wr = P == 3 ? c6[k] : c10[k], wi = -(P == 3 ? s6[k] : s10[k]);
            const float2 t = mk2(o[k].x * wr - o[k].y * wi, o[k].x * wi + o[k].y * wr);
            // X[k] = E[k] + t, X[k + P] = E[k] - t   (w_2P^(k+P) = -w_2P^k; (k + P) mod P = k)
            u[k] = mk2(e[k].x + t.x, e[k].y + t.y);
            u[k + P] = mk2(e[k].x - t.x, e[k].y - t.y);
        }
    } else if constexpr (R == 16) {
        // DFT-16 as 4 x 4 (round 3): r = r0 + 4 r1, q = q1 + 4 q0,
        //     X[q1 + 4 q0] = sum_r0 w4^(q0 r0) [ w16^(q1 r0) sum_r1 w4^(q1 r1) x[r0 + 4 r1] ]
        // -- two levels of radix-4 butterflies in registers with nine constant twiddles between them: one LDS (or
        // memory) round trip, one barrier and one set of index arithmetic where two radix-4 stages have two
        float2 y[4][4];
#pragma unroll
        for (int r0 = 0; r0 < 4; ++r0) {
            float2 v[4] = {u[r0], u[r0 + 4], u[r0 + 8], u[r0 + 12]};
            butterfly<4>(v, tw, n);
#pragma unroll
            for (int q1 = 0; q1 < 4; ++q1) y[r0][q1] = v[q1];
        }
        // w16^m = (cos, -sin)(2 pi m / 16), m = q1 r0
        constexpr float c1 = 0.92387953251128673848f, s1 = 0.38268343236508978178f, h = 0.70710678118654752440f;
        auto mulc = [](float2 a, float wr, float wi) { return mk2(a.x * wr - a.y * wi, a.x * wi + a.y * wr); };
        y[1][1] = mulc(y[1][1], c1, -s1);      // m = 1
        y[1][2] = mulc(y[1][2], h, -h);        // m = 2
        y[1][3] = mulc(y[1][3], s1, -c1);      // m = 3
        y[2][1] = mulc(y[2][1], h, -h);        // m = 2
        y[2][2] = mk2(y[2][2].y, -y[2][2].x);  // m = 4: -i
        y[2][3] = mulc(y[2][3], -h, -h);       // m = 6
        y[3][1] = mulc(y[3][1], s1, -c1);      // m = 3
        y[3][2] = mulc(y[3][2], -h, -h);       // m = 6
        y[3][3] = mulc(y[3][3], -c1, s1);      // m = 9
#pragma unroll
        for (int q1 = 0; q1 < 4; ++q1) {
            float2 v[4] = {y[0][q1], y[1][q1], y[2][q1], y[3][q1]};
            butterfly<4>(v, tw, n);
#pragma unroll
            for (int q0 = 0; q0 < 4; ++q0) u[q1 + 4 * q0] = v[q0];
        }
    } else {
        // odd prime: out[q] = sum_r u[r] * w_R^(q r), roots from the table (n is a multiple of R)
        float2 root[R];
        const int step = n / R;
#pragma unroll
        for (int m = 0; m < R; ++m) root[m] = tw[(size_t)m * step];
        float2 v[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            float2 acc = u[0];
#pragma unroll
            for (int r = 1; r < R; ++r) {
                const float2 t = cmul(u[r], root[(q * r) % R]);
                acc.x += t.x;
                acc.y += t.y;
            }
            v[q] = acc;
        }
#pragma unroll
        for (int q = 0; q < R; ++q) u[q] = v[q];
    }
}

// x / d as umulhi(x, magic(d)) (0: d == 1), exact while x * d < 2^32; magic(d) = floor(2^32 / d) + 1
__device__ __forceinline__ int fdiv(int x, unsigned magic) {
    return magic ? (int)__umulhi((unsigned)x, magic) : x;
}

// one Stockham stage of radix R over FR transforms of length n that lie one behind the other in the LDS: p = product of
// the earlier radices, t = n / R, tws = n / (p R); tw: w_n^k, k < n
template <int R>
__device__ __forceinline__ void lds_stage(const float2 *src, float2 *dst, int n, int p, int t, int tws, unsigned mag_t,
                                          unsigned mag_p, const float2 *__restrict__ tw, int FR, int tid, int NT) {
    for (int g = tid; g < FR * t; g += NT) {
        const int fr = FR == 1 ? 0 : fdiv(g, mag_t), i = g - fr * t;
        const int k = i - fdiv(i, mag_p) * p;
        const int j = (i - k) * R + k;
        const float2 *xb = src + fr * n;
        float2 *yb = dst + fr * n;
        float2 u[R];
#pragma unroll
        for (int r = 0; r < R; ++r) u[r] = xb[i + r * t];
        if (p != 1) {                             // the first stage has no twiddles in front (k == 0)
            const int kt = k * tws;
#pragma unroll
            for (int r = 1; r < R; ++r) u[r] = cmul(u[r], tw[r * kt]);
        }
        butterfly<R>(u, tw, n);
#pragma unroll
        for (int r = 0; r < R; ++r) yb[j + r * p] = u[r];
    }
}

}  // namespace
}  // namespace gsdr
