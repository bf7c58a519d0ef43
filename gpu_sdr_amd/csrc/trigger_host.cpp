// trigger_host.cpp -- the trigger's creation, bookkeeping and host twin (the contract: include/gsdr.h, "trigger on the
// device").  The host twin streams like the device path does -- it carries the last pre + post - 1 rows, the records of
// the last post - 1 rows and the last hitting row, and never recomputes a record -- so that set_levels between feeds
// means the same on both.  trigger_hits_kernel / trigger_select_kernel / trigger_capture_kernel (trigger_kernels.hip)
// give the same bits.  No HIP here.
#include <cstring>
#include <vector>

#include "stage_host.h"
#include "trigger_state.h"

extern "C" {

int gsdr_trigger_dev_create_(gsdr_trigger *t, const gsdr_trigger_level *levels) __attribute__((weak));
int gsdr_trigger_dev_set_levels_(gsdr_trigger *t, const gsdr_trigger_level *levels, void *hip_stream) __attribute__((weak));

namespace {
GSDR_NO_CONTRACT
inline gsdr_trigger_rec trigger_row_host(const gsdr_c64 *row, const gsdr_trigger_level *lv, int n_ch) {
    GSDR_NO_CONTRACT_BODY
    gsdr_trigger_rec rec{0, 0, 0.f, 0};
    for (int c = 0; c < n_ch; ++c) {
        const float t0 = row[c].x - lv[c].bx;
        const float t1 = row[c].y - lv[c].by;
        const float p0 = t0 * lv[c].dx;
        const float p1 = t1 * lv[c].dy;
        const float q = p0 + p1;
        const bool up = q > lv[c].hi;
        const bool dn = !up && q < lv[c].lo;
        if (!(up || dn)) continue;
        if (rec.n_hit == 0) {
            rec.channel = c;
            rec.side = up ? 1 : -1;
            rec.q = q;
        }
        ++rec.n_hit;
    }
    return rec;
}
}  // namespace

gsdr_trigger *gsdr_trigger_create(int n_ch, int max_rows, int pre, int post, int holdoff, int max_events,
                                  const gsdr_trigger_level *levels, int device_index) {
    std::string bad;
    if (n_ch < 1 || n_ch > (1 << 20)) bad = "n_ch must be in [1, 1048576]";
    else if (max_rows < 1 || max_rows > (1 << 20)) bad = "max_rows must be in [1, 1048576]";
    else if (pre < 0) bad = "pre must be >= 0";
    else if (post < 1) bad = "post must be >= 1";
    else if ((long long)pre + post > 65536) bad = "pre + post must be <= 65536";
    else if (holdoff < 0 || holdoff > (1 << 30)) bad = "holdoff must be in [0, 1073741824]";
    else if (max_events < 1 || max_events > (1 << 20)) bad = "max_events must be in [1, 1048576]";
    else if (!levels) bad = "levels must not be NULL";
    else bad = stage_device_fault(device_index, "GSDR_TRIGGER_HOST", gsdr_trigger_dev_create_ != nullptr);
    return stage_create<gsdr_trigger>(
        "gsdr_trigger_create", bad, device_index, "pre + post and n_ch: no host memory for the carried rows",
        [&](gsdr_trigger &t) {
            t.n_ch = n_ch, t.max_rows = max_rows, t.pre = pre, t.post = post, t.holdoff = holdoff, t.max_events = max_events;
            if (device_index != GSDR_TRIGGER_HOST) return;        // the levels of a device object live on the device
            t.levels.assign(levels, levels + n_ch);
            t.carry.assign((size_t)(pre + post - 1) * (size_t)n_ch, gsdr_c64{0.f, 0.f});
            t.recs.assign((size_t)(post - 1), gsdr_trigger_rec{0, 0, 0.f, 0});
            t.trig.assign((size_t)(post - 1), 0);
        },
        [&](gsdr_trigger *t) { return gsdr_trigger_dev_create_(t, levels); });
}

int gsdr_trigger_set_levels(gsdr_trigger *t, const gsdr_trigger_level *levels, void *hip_stream) {
    if (!t || !levels) return stage_refuse("gsdr_trigger_set_levels", "null argument");
    if (t->device != GSDR_TRIGGER_HOST) return gsdr_trigger_dev_set_levels_(t, levels, hip_stream);
    t->levels.assign(levels, levels + t->n_ch);
    return 0;
}

int gsdr_trigger_reset(gsdr_trigger *t) {
    if (!t) return stage_refuse("gsdr_trigger_reset", "null object");
    // the device path reads `total` on the host and takes nothing from the carry of a stream that has just begun
    t->total = 0;
    t->last_hit = -1;
    for (auto &r : t->recs) r = gsdr_trigger_rec{0, 0, 0.f, 0};
    for (auto &f : t->trig) f = 0;
    return 0;
}

long long gsdr_trigger_rows(const gsdr_trigger *t) { return t ? t->total : 0; }

void gsdr_trigger_close(gsdr_trigger *t) { stage_close(t); }

int gsdr_trigger_feed_host(gsdr_trigger *t, const gsdr_c64 *rows, int n_rows, gsdr_trigger_event *events,
                           gsdr_c64 *snippets, int *n_dropped) {
    const char *const me = "gsdr_trigger_feed_host";
    if (const char *why = stage_host_fault(t, "a device object takes gsdr_trigger_feed or gsdr_trigger_feed_device")) return stage_refuse(me, why);
    if (n_rows < 0 || n_rows > t->max_rows) return stage_refuse(me, "n_rows must be in [0, max_rows]");
    if (n_dropped) *n_dropped = 0;
    if (n_rows == 0) return 0;
    if (!rows || !events || !snippets) return stage_refuse(me, "null buffer");
    const size_t n_ch = (size_t)t->n_ch, n = (size_t)n_rows;
    const size_t P = (size_t)(t->post - 1), K = (size_t)(t->pre + t->post - 1), S = (size_t)(t->pre + t->post);
    const long long R0 = t->total, base = R0 - (long long)P;     // window entry j is stream row base + j
    std::vector<gsdr_trigger_rec> wrec;
    std::vector<unsigned char> wtrig;
    try {
        wrec.resize(P + n);
        wtrig.assign(P + n, 0);
    } catch (const std::bad_alloc &) {
        return stage_refuse(me, "out of memory");
    }
    for (size_t j = 0; j < P; ++j) wrec[j] = t->recs[j], wtrig[j] = t->trig[j];
    for (size_t i = 0; i < n; ++i) {
        const gsdr_trigger_rec rec = trigger_row_host(rows + i * n_ch, t->levels.data(), t->n_ch);
        wrec[P + i] = rec;
        if (rec.n_hit > 0) {
            const long long r = R0 + (long long)i;
            wtrig[P + i] = (t->last_hit < 0 || r - t->last_hit > t->holdoff) ? 1 : 0;
            t->last_hit = r;
        }
    }
    int n_events = 0, dropped = 0;
    for (size_t j = 0; j < n; ++j) {
        const long long r = base + (long long)j;
        if (!wtrig[j] || r < t->pre) continue;
        if (n_events >= t->max_events) {
            ++dropped;
            continue;
        }
        events[n_events] = gsdr_trigger_event{r, wrec[j].channel, wrec[j].side, wrec[j].q, wrec[j].n_hit};
        gsdr_c64 *dst = snippets + (size_t)n_events * S * n_ch;
        for (size_t k = 0; k < S; ++k) {
            const long long rel = r - t->pre + (long long)k - R0;     // in [-K, n)
            const gsdr_c64 *src = rel >= 0 ? rows + (size_t)rel * n_ch : t->carry.data() + (size_t)((long long)K + rel) * n_ch;
            std::memcpy(dst + k * n_ch, src, n_ch * sizeof(gsdr_c64));
        }
        ++n_events;
    }
    if (K > 0) {
        if (n >= K) {
            std::memcpy(t->carry.data(), rows + (n - K) * n_ch, K * n_ch * sizeof(gsdr_c64));
        } else {
            std::memmove(t->carry.data(), t->carry.data() + n * n_ch, (K - n) * n_ch * sizeof(gsdr_c64));
            std::memcpy(t->carry.data() + (K - n) * n_ch, rows, n * n_ch * sizeof(gsdr_c64));
        }
    }
    for (size_t j = 0; j < P; ++j) t->recs[j] = wrec[n + j], t->trig[j] = wtrig[n + j];
    t->total += n_rows;
    if (n_dropped) *n_dropped = dropped;
    return n_events;
}

}  // extern "C"
