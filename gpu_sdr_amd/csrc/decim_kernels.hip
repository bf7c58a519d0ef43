// decim_kernels.hip -- FIR decimation of demodulated rows (the contract: include/gsdr.h, "FIR decimation on the
// device"; the blocks and the ring: decim_state.h; the design: DESIGN.md section 4.11).  Two launches per feed:
//   decim_partial_kernel  one thread per (block, channel) and group of JT chunks, the channel running fastest across
//                         the lanes: it walks the block's rows once, in stream order, and keeps the JT chunk sums in
//                         registers -- JT independent chains of fused multiply-adds.  A row is one float2 per lane
//                         (a coalesced line where n_ch >= 64; with few channels the lanes of a wave hold different
//                         blocks and a line serves the next rows of the walk out of the cache).  The tap of (chunk, row
//                         in block) is the same for every lane, whatever its block: wave-uniform loads.  The sums of a
//                         block the feed leaves open go to the ring as they are and the next feed goes on from them, in
//                         the same thread order -- a chain does not see the cut.
//   decim_combine_kernel  one thread per (output row, channel): the F chunk sums of the output out of the ring, added
//                         oldest first.
// Every (block, chunk, channel) of the ring is read and written by one thread of the first launch, and the second only
// reads the ring: no workgroup reads what another of the same launch writes.  Compiler-scheduled and GSDR_NO_PK: they
// run beside another handle's matrix-core loop.
#include "decim_kernels.h"

#include "ddc_kernels.h"

namespace gsdr {
namespace {

// (make_float2 of the HIP headers is not always_inline: inside a GSDR_NO_PK kernel it would stay a real call)
__device__ __forceinline__ float2 f2(float x, float y) {
    float2 v;
    v.x = x, v.y = y;
    return v;
}

constexpr int kDecimDepth = 8;           // rows a thread of decim_partial_kernel has in flight
static_assert(kDecimDepth <= kDecimTapsPad, "a turn's taps may reach kDecimDepth - 1 floats past the last block row");

struct DecimPart {
    const float2 *rows;
    float2 *ring;
    const float *taps;                   // [F q + kDecimDepth], see DecimFeed
    unsigned long long items;            // blocks touched x n_ch
    int n, n_ch, q, F, pad;              // pad = F q - T: chunk F - 1 starts at row `pad` of its block
    unsigned ring_blocks, slot_f;        // ring slot of the first block touched
    int rel0;                            // feed row of the first row of the first block touched, in (-q, 0]
    int first_feed;                      // the stream starts with this feed: every block is new
    int i_begin, i_end;                  // rows of a block any thread takes: [0, q), or the one block's own range
};

template <int JT>
__global__ __launch_bounds__(256) GSDR_NO_PK void decim_partial_kernel(const DecimPart a) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256ULL + (unsigned long long)threadIdx.x;
    const bool live = g < a.items;
    const unsigned kb = live ? (unsigned)(g / (unsigned)a.n_ch) : 0u;
    const unsigned c = live ? (unsigned)(g - (unsigned long long)kb * (unsigned)a.n_ch) : 0u;
    const int j0 = (int)blockIdx.y * JT;
    const int rel = a.rel0 + (int)kb * a.q;                       // feed row of the block's first row
    const int lo = rel < 0 ? -rel : 0, hi = a.n - rel < a.q ? a.n - rel : a.q;
    const bool carried = live && rel < 0 && !a.first_feed;        // the block began in an earlier feed
    unsigned slot = a.slot_f + kb;                                // kb < ring_blocks
    slot = slot >= a.ring_blocks ? slot - a.ring_blocks : slot;
    float2 *part = a.ring + ((size_t)slot * (size_t)a.F + (size_t)j0) * (size_t)a.n_ch + c;
    // chunk j0 + u of this thread, or the last chunk where the group reaches past F (loaded, never used)
    const int last = a.F - 1 - j0 < JT - 1 ? a.F - 1 - j0 : JT - 1;
    float ax[JT], ay[JT];
    {
        float2 v[JT];
        if (carried) {                                             // one test for the JT loads: they go out together
#pragma unroll
            for (int u = 0; u < JT; ++u) v[u] = part[(size_t)(u < last ? u : last) * (size_t)a.n_ch];
        }
#pragma unroll
        for (int u = 0; u < JT; ++u) ax[u] = carried ? v[u].x : 0.f, ay[u] = carried ? v[u].y : 0.f;
    }
    const float2 *x = a.rows + c;
    // The chains wait for nothing but the rows: kDecimDepth rows are loaded before the first is used.  Nothing is loaded
    // behind a test of its own -- a row outside the thread's [lo, hi) comes from the nearest row of the feed, a tap past
    // the block from the padding behind the taps, and a select drops the product -- so the row loads of a turn go out
    // together and the taps of a chunk come as one wave-uniform run.  (With every load behind its own branch the kernel
    // waited a round trip per row and one per tap.)
    for (int ib = a.i_begin; ib < a.i_end; ib += kDecimDepth) {
        float2 v[kDecimDepth];
#pragma unroll
        for (int s = 0; s < kDecimDepth; ++s) {
            int r = rel + ib + s;
            r = r < 0 ? 0 : (r > a.n - 1 ? a.n - 1 : r);
            v[s] = x[(size_t)r * (size_t)a.n_ch];
        }
        float w[JT][kDecimDepth];
#pragma unroll
        for (int u = 0; u < JT; ++u) {
            const float *t = a.taps + (a.F - 1 - j0 - (u < last ? u : last)) * a.q + ib;      // uniform
#pragma unroll
            for (int s = 0; s < kDecimDepth; ++s) w[u][s] = t[s];
        }
#pragma unroll
        for (int s = 0; s < kDecimDepth; ++s) {
            const int i = ib + s;
            const bool mine = live && i >= lo && i < hi;           // i < hi <= i_end
#pragma unroll
            for (int u = 0; u < JT; ++u) {
                const int j = j0 + u;
                const bool use = mine && j < a.F && (j < a.F - 1 || i >= a.pad);
                const float fx = __builtin_fmaf(w[u][s], v[s].x, ax[u]), fy = __builtin_fmaf(w[u][s], v[s].y, ay[u]);
                ax[u] = use ? fx : ax[u];
                ay[u] = use ? fy : ay[u];
            }
        }
    }
    if (live) {
#pragma unroll
        for (int u = 0; u < JT; ++u)
            if (j0 + u < a.F) part[(size_t)u * (size_t)a.n_ch] = f2(ax[u], ay[u]);
    }
}

struct DecimComb {
    const float2 *ring;
    float2 *out;
    unsigned long long items;            // n_emit x n_ch
    int n_ch, F;
    unsigned ring_blocks, slot_s;        // ring slot of block ks (as if the ring went on before the stream)
    long long ks;                        // block of chunk F - 1 of the first output: may be < 0
};

__global__ __launch_bounds__(256) GSDR_NO_PK void decim_combine_kernel(const DecimComb a) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256ULL + (unsigned long long)threadIdx.x;
    if (g >= a.items) return;
    const unsigned oo = (unsigned)(g / (unsigned)a.n_ch);
    const unsigned c = (unsigned)(g - (unsigned long long)oo * (unsigned)a.n_ch);
    const long long kb = a.ks + (long long)oo;                    // block of chunk F - 1
    const int before = kb >= 0 ? 0 : (-kb >= (long long)a.F ? a.F : (int)-kb);      // chunks before the stream: +0
    unsigned slot = a.slot_s + oo;                                // oo < ring_blocks
    slot = slot >= a.ring_blocks ? slot - a.ring_blocks : slot;
    const float2 *r = a.ring + c;
    // step m takes chunk F - 1 - m of block kb + m (ring slot `slot`, then the next); the additions are a chain, the
    // loads are not: 8 in flight
    const size_t step = (size_t)a.n_ch, per = (size_t)a.F * step;
    const int F1 = a.F - 1;
    float2 s = before > 0 ? f2(0.f, 0.f) : r[(size_t)slot * per + (size_t)F1 * step];
    slot = slot + 1 == a.ring_blocks ? 0 : slot + 1;
    int m = 1;
    for (; m + 8 <= a.F; m += 8) {
        float2 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            t[u] = m + u >= before ? r[(size_t)slot * per + (size_t)(F1 - m - u) * step] : f2(0.f, 0.f);
            slot = slot + 1 == a.ring_blocks ? 0 : slot + 1;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s.x = s.x + t[u].x, s.y = s.y + t[u].y;
    }
    for (; m < a.F; ++m) {
        const float2 t = m >= before ? r[(size_t)slot * per + (size_t)(F1 - m) * step] : f2(0.f, 0.f);
        slot = slot + 1 == a.ring_blocks ? 0 : slot + 1;
        s.x = s.x + t.x, s.y = s.y + t.y;
    }
    a.out[g] = s;
}

template <int JT>
hipError_t launch_partial(const DecimPart &a, unsigned blocks, hipStream_t st) {
    hipLaunchKernelGGL(decim_partial_kernel<JT>, dim3(blocks, (unsigned)((a.F + JT - 1) / JT)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace

// A thread keeps JT chunk sums: the feed's rows are read ceil(F / JT) times (once from memory, the rest out of the
// caches), by that many times the threads.  7 divides the default taps' F = 21: three threads per (block, channel),
// which the feeds of the README's table need to fill the device (C3: 11 blocks x 2048 channels).
int decim_chunks_per_thread(int F) { return F <= 1 ? 1 : F <= 3 ? 3 : 7; }

hipError_t launch_decim_feed(const DecimFeed &f, hipStream_t st) {
    if (f.n < 1 || f.n_ch < 1 || f.q < 1 || f.T < 1 || f.F != (f.T + f.q - 1) / f.q || !f.rows || !f.ring || !f.taps || f.first_row < 0 ||
        f.r0 > 0 || f.r0 <= -(long long)f.q || f.n_emit < 0 || (f.n_emit > 0 && !f.out))
        return hipErrorInvalidValue;
    const long long q = f.q;
    const long long kf = (f.first_row - f.r0) / q, kl = (f.first_row + f.n - 1 - f.r0) / q, nb = kl - kf + 1;
    // the ring holds the blocks this feed touches and the F - 1 before them that its outputs take
    if (nb + f.F - 1 > (long long)f.ring_blocks) return hipErrorInvalidValue;
    DecimPart p{};
    p.rows = f.rows, p.ring = f.ring, p.taps = f.taps;
    p.items = (unsigned long long)nb * (unsigned long long)f.n_ch;
    p.n = f.n, p.n_ch = f.n_ch, p.q = f.q, p.F = f.F, p.pad = f.F * f.q - f.T;
    p.ring_blocks = f.ring_blocks, p.slot_f = (unsigned)(kf % (long long)f.ring_blocks);
    p.rel0 = (int)(kf * q + f.r0 - f.first_row);
    p.first_feed = f.first_row == 0;
    p.i_begin = 0, p.i_end = f.q;
    if (nb == 1) {
        p.i_begin = p.rel0 < 0 ? -p.rel0 : 0;
        p.i_end = f.n - p.rel0 < f.q ? f.n - p.rel0 : f.q;
    }
    const unsigned long long blocks = (p.items + 255ULL) / 256ULL;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    switch (decim_chunks_per_thread(f.F)) {
        case 1: e = launch_partial<1>(p, (unsigned)blocks, st); break;
        case 3: e = launch_partial<3>(p, (unsigned)blocks, st); break;
        default: e = launch_partial<7>(p, (unsigned)blocks, st); break;
    }
    if (e != hipSuccess || f.n_emit == 0) return e;
    // the outputs of this feed are complete with blocks of this feed
    if (f.k_out < kf || f.k_out + f.n_emit - 1 > kl) return hipErrorInvalidValue;
    DecimComb c{};
    c.ring = f.ring, c.out = f.out;
    c.items = (unsigned long long)f.n_emit * (unsigned long long)f.n_ch;
    c.n_ch = f.n_ch, c.F = f.F, c.ring_blocks = f.ring_blocks;
    c.ks = f.k_out - (f.F - 1);
    const long long rb = (long long)f.ring_blocks;
    c.slot_s = (unsigned)(((c.ks % rb) + rb) % rb);
    const unsigned long long cblocks = (c.items + 255ULL) / 256ULL;
    if (cblocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decim_combine_kernel, dim3((unsigned)cblocks), dim3(256), 0, st, c);
    return hipGetLastError();
}

}  // namespace gsdr
