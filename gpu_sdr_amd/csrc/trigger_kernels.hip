// trigger_kernels.hip -- the trigger on demodulated rows (the contract: include/gsdr.h, "trigger on the device"; the
// design: DESIGN.md section 4.9).  Three launches per feed:
//   trigger_hits_kernel     the row pass: one record per row (lowest hitting channel, side, q, number of hits), and the
//                           records of the last post - 1 rows moved to the head of this feed's window;
//   trigger_select_kernel   which hitting rows are triggers, which of them this feed emits, in row order, cut at
//                           max_events; writes the events and the counts;
//   trigger_capture_kernel  copies the snippets of the emitted events, and the last pre + post - 1 rows for the next feed.
// All compiler-scheduled and GSDR_NO_PK: they run beside another handle's matrix-core loop.
#include "trigger_kernels.h"

#include "ddc_kernels.h"

namespace gsdr {
namespace {

constexpr long long kNoHit = -(1LL << 40);       // "no hitting row yet": further than any holdoff from every row
constexpr int kSelectThreads = 1024;

// (the HIP headers' __ballot, __shfl, __syncthreads, make_int4, ... are not always_inline: inside a kernel with other
//  target features -- GSDR_NO_PK -- they would stay real calls; the builtins they wrap are used directly)
__device__ __forceinline__ int4 mk4(int x, int y, int z, int w) {
    int4 v;
    v.x = x, v.y = y, v.z = z, v.w = w;
    return v;
}
__device__ __forceinline__ void wg_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ int f2i(float f) { return __builtin_bit_cast(int, f); }
__device__ __forceinline__ float i2f(int i) { return __builtin_bit_cast(float, i); }

// the quantity of include/gsdr.h: five single-precision operations, nothing fused (plain operators under the pragma,
// as in average_term of fft_kernels.hip); returns +1 (up), -1 (dn) or 0
__device__ __forceinline__ int trigger_side(float2 y, const float2 *__restrict__ lv, float &q) {
#pragma clang fp contract(off)
    const float2 b = lv[0], d = lv[1], th = lv[2];
    const float t0 = y.x - b.x;
    const float t1 = y.y - b.y;
    const float p0 = t0 * d.x;
    const float p1 = t1 * d.y;
    q = p0 + p1;
    const bool up = q > th.y;
    const bool dn = !up && q < th.x;
    return up ? 1 : (dn ? -1 : 0);
}

// the records a feed inherits: window entries [0, P) are entries [n_prev, n_prev + P) of the window before; of a young
// stream only the last rec_valid exist
__device__ __forceinline__ void trigger_move_carry(int P, int n_prev, int rec_valid, const int4 *__restrict__ rec_in,
                                                   const unsigned char *__restrict__ flag_in, int4 *__restrict__ rec_out,
                                                   unsigned char *__restrict__ flag_out) {
    const int stride = (int)gridDim.x * (int)blockDim.x;
    for (int j = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x; j < P; j += stride) {
        const bool have = j >= P - rec_valid;
        rec_out[j] = have ? rec_in[n_prev + j] : mk4(0, 0, 0, 0);
        flag_out[j] = have ? flag_in[n_prev + j] : (unsigned char)0;
    }
}

// n_ch <= 64: a wave holds 64 >> lw rows of W = 1 << lw >= n_ch lanes each; a lane keeps its channel, and so its
// levels, over all the rows its wave takes.  The record of a row comes from two ballots.
__global__ __launch_bounds__(256) GSDR_NO_PK void trigger_hits_kernel(const float2 *__restrict__ rows, int n, int n_ch, int lw,
                                                                      const float2 *__restrict__ levels, int P, int n_prev,
                                                                      int rec_valid, const int4 *__restrict__ rec_in,
                                                                      const unsigned char *__restrict__ flag_in,
                                                                      int4 *__restrict__ rec_out,
                                                                      unsigned char *__restrict__ flag_out) {
    trigger_move_carry(P, n_prev, rec_valid, rec_in, flag_in, rec_out, flag_out);
    const int lane = (int)threadIdx.x & 63;
    const int wave = ((int)blockIdx.x * 256 + (int)threadIdx.x) >> 6, waves = (int)gridDim.x * 4;
    const int W = 1 << lw, rpw = 64 >> lw;
    const int sub = lane >> lw, c = lane & (W - 1);
    const bool has_c = c < n_ch;
    const float2 *lv = levels + (size_t)(has_c ? c : 0) * 3;
    const unsigned long long seg_mask = lw == 6 ? ~0ULL : ((1ULL << W) - 1ULL);
    const int groups = (n + rpw - 1) / rpw;
    for (int g = wave; g < groups; g += waves) {              // wave-uniform trip count
        const int row = g * rpw + sub;
        const bool valid = has_c && row < n;
        float q = 0.f;
        int side = 0;
        if (valid) side = trigger_side(rows[(size_t)row * (size_t)n_ch + c], lv, q);
        const unsigned long long hit_all = __builtin_amdgcn_ballot_w64(side != 0), up_all = __builtin_amdgcn_ballot_w64(side > 0);
        const unsigned long long seg = (hit_all >> (sub << lw)) & seg_mask;
        const int low = seg ? __builtin_ctzll(seg) : 0;
        const int src = (sub << lw) + low;
        const float q_low = i2f(__builtin_amdgcn_ds_bpermute(src << 2, f2i(q)));      // every lane of the wave is here
        if (c == 0 && row < n) {
            rec_out[P + row] = seg ? mk4(low, ((up_all >> src) & 1ULL) ? 1 : -1, f2i(q_low), __builtin_popcountll(seg))
                                   : mk4(0, 0, 0, 0);
            flag_out[P + row] = seg ? (unsigned char)1 : (unsigned char)0;
        }
    }
}

// n_ch > 64: a workgroup takes a row at a time, 256 channels per step; each wave keeps its lowest hit and its count, the
// four meet in the LDS (no atomics)
__global__ __launch_bounds__(256) GSDR_NO_PK void trigger_hits_wide_kernel(const float2 *__restrict__ rows, int n, int n_ch,
                                                                           const float2 *__restrict__ levels, int P, int n_prev,
                                                                           int rec_valid, const int4 *__restrict__ rec_in,
                                                                           const unsigned char *__restrict__ flag_in,
                                                                           int4 *__restrict__ rec_out,
                                                                           unsigned char *__restrict__ flag_out) {
    __shared__ int4 s_rec[4];
    trigger_move_carry(P, n_prev, rec_valid, rec_in, flag_in, rec_out, flag_out);
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int row = (int)blockIdx.x; row < n; row += (int)gridDim.x) {     // workgroup-uniform
        const float2 *x = rows + (size_t)row * (size_t)n_ch;
        int low = 0x7fffffff, side_low = 0, cnt = 0;
        float q_low = 0.f;
        for (int base = 0; base < n_ch; base += 256) {
            const int c = base + tid;
            float q = 0.f;
            int side = 0;
            if (c < n_ch) side = trigger_side(x[c], levels + (size_t)c * 3, q);
            const unsigned long long hit = __builtin_amdgcn_ballot_w64(side != 0), up = __builtin_amdgcn_ballot_w64(side > 0);
            const int l = hit ? __builtin_ctzll(hit) : 0;
            const float ql = i2f(__builtin_amdgcn_readlane(f2i(q), __builtin_amdgcn_readfirstlane(l)));
            if (hit && cnt == 0) {
                low = base + w * 64 + l;
                side_low = ((up >> l) & 1ULL) ? 1 : -1;
                q_low = ql;
            }
            cnt += __builtin_popcountll(hit);
        }
        if (lane == 0) s_rec[w] = mk4(low, side_low, f2i(q_low), cnt);
        wg_sync();
        if (tid == 0) {
            int4 best = s_rec[0];
            for (int k = 1; k < 4; ++k) {
                const int4 o = s_rec[k];
                const int total = best.w + o.w;
                if (o.w > 0 && (best.w == 0 || o.x < best.x)) best = o;
                best.w = total;
            }
            rec_out[P + row] = best.w ? best : mk4(0, 0, 0, 0);
            flag_out[P + row] = best.w ? (unsigned char)1 : (unsigned char)0;
        }
        wg_sync();
    }
}

// Selection, one workgroup.  Thread t owns the window entries [t * L, (t + 1) * L): inside such a chunk only the FIRST
// hit depends on rows outside it, through the last hitting row before the chunk.  Pass 1 walks the chunk and reports
// {first hit, last hit, emitted triggers not counting the first hit}; a prefix maximum over the chunks' last hits
// resolves every first hit, a prefix sum over the counts gives each chunk its place in the output; pass 2 walks again,
// writes the trigger bits (the next feeds inherit them) and the events in row order, the first max_events of them.
template <typename T, typename Op>
__device__ __forceinline__ T block_scan_inclusive(T v, T *s, Op op) {
    const int t = (int)threadIdx.x;
    s[t] = v;
    wg_sync();
    for (int off = 1; off < kSelectThreads; off <<= 1) {
        const T o = t >= off ? s[t - off] : v;
        wg_sync();
        if (t >= off) v = op(v, o);
        s[t] = v;
        wg_sync();
    }
    return v;
}

// Walks the flags of the window entries [j0, j1) in order, j0 a multiple of 64: 64 bytes per step, four 16-byte loads in
// flight, and a word of four quiet rows -- nearly every word -- costs one comparison.  (The buffer is padded by 64
// bytes; what lies behind j1 is not looked at.)
template <typename F>
__device__ __forceinline__ void walk_flags(const unsigned char *__restrict__ flags, int j0, int j1, F &&on_flag) {
    for (int jg = j0; jg < j1; jg += 64) {
        const uint4 *p = reinterpret_cast<const uint4 *>(flags + jg);
        const uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
        const unsigned w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            unsigned rest = w[k];
            while (rest) {                                        // the non-zero bytes of the word, lowest first
                const int b = __builtin_ctz(rest) >> 3;
                const int j = jg + 4 * k + b;
                if (j < j1) on_flag((rest >> (8 * b)) & 0xffu, j);
                rest &= ~(0xffu << (8 * b));
            }
        }
    }
}

__global__ __launch_bounds__(kSelectThreads) GSDR_NO_PK void trigger_select_kernel(
    int n, int P, int pre, int holdoff, int max_events, long long R0, unsigned char *__restrict__ flags,
    const int4 *__restrict__ recs, long long *__restrict__ last_hit, gsdr_trigger_event *__restrict__ events,
    int *__restrict__ counts) {
    __shared__ long long s_max[kSelectThreads];
    __shared__ int s_sum[kSelectThreads];
    const int t = (int)threadIdx.x;
    const int E = P + n;
    const int L = ((E + kSelectThreads - 1) / kSelectThreads + 63) & ~63;      // a chunk is whole 64-byte steps
    const int j0 = t * L < E ? t * L : E, j1 = j0 + L < E ? j0 + L : E;
    const long long base = R0 - P;                              // stream row of window entry 0
    const long long before = R0 > 0 ? *last_hit : kNoHit;       // read by every thread before thread 0 rewrites it below
    // an emitted entry: a trigger whose last snippet row this feed delivers (j < n) and whose first one exists
    const int j_emit0 = base >= pre ? 0 : (int)(pre - base < E ? pre - base : E);

    int first = -1, last = -1, cnt = 0;
    walk_flags(flags, j0, j1, [&](unsigned f, int j) {
        bool trig = false;
        if (j < P) {
            trig = (f & 2u) != 0;
        } else if (f & 1u) {
            if (first < 0) first = j;
            else trig = j - last > holdoff;
            last = j;
        }
        if (trig && j < n && j >= j_emit0) ++cnt;
    });
    block_scan_inclusive(last >= 0 ? base + last : kNoHit, s_max, [](long long a, long long b) { return a > b ? a : b; });
    long long prev = t > 0 ? s_max[t - 1] : kNoHit;
    if (before > prev) prev = before;
    const long long newest = s_max[kSelectThreads - 1] > before ? s_max[kSelectThreads - 1] : before;
    bool first_trig = false;
    if (first >= 0) {
        first_trig = base + first - prev > holdoff;
        if (first_trig && first < n && first >= j_emit0) ++cnt;
    }
    const int upto = block_scan_inclusive(cnt, s_sum, [](int a, int b) { return a + b; });
    const int total = s_sum[kSelectThreads - 1];
    int e = upto - cnt;

    last = -1;
    walk_flags(flags, j0, j1, [&](unsigned f, int j) {
        bool trig = false;
        if (j < P) {
            trig = (f & 2u) != 0;
        } else if (f & 1u) {
            trig = j == first ? first_trig : j - last > holdoff;
            last = j;
            if (trig) flags[j] = (unsigned char)3;
        }
        if (trig && j < n && j >= j_emit0) {
            if (e < max_events) {
                const int4 r = recs[j];
                gsdr_trigger_event ev;
                ev.row = base + j;
                ev.channel = r.x;
                ev.side = r.y;
                ev.q = i2f(r.z);
                ev.n_hit = r.w;
                events[e] = ev;
            }
            ++e;
        }
    });
    if (t == 0) {
        counts[0] = total < max_events ? total : max_events;
        counts[1] = total < max_events ? 0 : total - max_events;
        *last_hit = newest;
    }
}

// Snippets and carry, element by element.  Workgroups [0, cap_blocks) copy the snippets of the counts[0] events the
// selection wrote and leave when they are beyond them; workgroups behind those build the next feed's carried rows from
// [carried rows | this feed's rows].
__global__ __launch_bounds__(256) GSDR_NO_PK void trigger_capture_kernel(const gsdr_trigger_event *__restrict__ events,
                                                                         const int *__restrict__ counts,
                                                                         const float2 *__restrict__ rows, int n, int n_ch, int pre,
                                                                         int S, long long R0, const float2 *__restrict__ carry_in,
                                                                         float2 *__restrict__ carry_out,
                                                                         float2 *__restrict__ snippets, int cap_blocks) {
    const long long K = S - 1;
    if ((int)blockIdx.x < cap_blocks) {
        const long long total = (long long)counts[0] * S * n_ch;
        const long long stride = (long long)cap_blocks * 256;
        for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
            const long long sr = idx / n_ch;
            const int c = (int)(idx - sr * n_ch);
            const long long e = sr / S;
            const int k = (int)(sr - e * S);
            const long long rel = events[e].row - pre + k - R0;              // in [-K, n)
            snippets[idx] = rel >= 0 ? rows[(size_t)rel * (size_t)n_ch + c] : carry_in[(size_t)(K + rel) * (size_t)n_ch + c];
        }
    } else {
        const long long total = K * n_ch;
        const long long stride = (long long)((int)gridDim.x - cap_blocks) * 256;
        for (long long idx = (long long)((int)blockIdx.x - cap_blocks) * 256 + threadIdx.x; idx < total; idx += stride) {
            const long long kr = idx / n_ch;
            const int c = (int)(idx - kr * n_ch);
            const long long p = kr + n;                                      // row of [carried | fed] that becomes carried row kr
            carry_out[idx] = p < K ? carry_in[(size_t)p * (size_t)n_ch + c] : rows[(size_t)(p - K) * (size_t)n_ch + c];
        }
    }
}

}  // namespace

hipError_t launch_trigger_feed(const TriggerFeed &f, hipStream_t st) {
    if (f.n < 1 || f.n_ch < 1 || !f.rows || !f.events || !f.snippets || !f.counts) return hipErrorInvalidValue;
    const int P = f.post - 1, S = f.pre + f.post;
    const float2 *lv = reinterpret_cast<const float2 *>(f.levels);
    const int4 *rec_in = reinterpret_cast<const int4 *>(f.rec_in);
    int4 *rec_out = reinterpret_cast<int4 *>(f.rec_out);
    if (f.n_ch <= 64) {
        int lw = 0;
        while ((1 << lw) < f.n_ch) ++lw;
        const int groups = (f.n + (64 >> lw) - 1) / (64 >> lw);
        // up to eight row groups per wave, so that a lane's levels serve several rows; never more than 2048 workgroups
        int blocks = (groups + 31) / 32;
        if (blocks > 2048) blocks = 2048;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(trigger_hits_kernel, dim3((unsigned)blocks), dim3(256), 0, st, f.rows, f.n, f.n_ch, lw, lv, P, f.n_prev,
                           f.rec_valid, rec_in, f.flag_in, rec_out, f.flag_out);
    } else {
        const int blocks = f.n < 65536 ? f.n : 65536;
        hipLaunchKernelGGL(trigger_hits_wide_kernel, dim3((unsigned)blocks), dim3(256), 0, st, f.rows, f.n, f.n_ch, lv, P, f.n_prev,
                           f.rec_valid, rec_in, f.flag_in, rec_out, f.flag_out);
    }
    hipLaunchKernelGGL(trigger_select_kernel, dim3(1), dim3(kSelectThreads), 0, st, f.n, P, f.pre, f.holdoff, f.max_events, f.R0,
                       f.flag_out, rec_out, f.last_hit, f.events, f.counts);
    const long long cap_elems = (long long)f.max_events * S * f.n_ch, carry_elems = (long long)(S - 1) * f.n_ch;
    long long cap_blocks = (cap_elems + 255) / 256, carry_blocks = (carry_elems + 255) / 256;
    if (cap_blocks > 8192) cap_blocks = 8192;
    if (carry_blocks > 2048) carry_blocks = 2048;
    hipLaunchKernelGGL(trigger_capture_kernel, dim3((unsigned)(cap_blocks + carry_blocks)), dim3(256), 0, st, f.events, f.counts,
                       f.rows, f.n, f.n_ch, f.pre, S, f.R0, f.carry_in, f.carry_out, f.snippets, (int)cap_blocks);
    return hipGetLastError();
}

}  // namespace gsdr
