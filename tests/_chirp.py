"""Helpers of tests/test_gpu_chirp_positions.py: CHIRP handles walked through a long stream, compared with a
reference that knows nothing of the streaming state.

The stream is ONE buffer x of L samples fed on every call: the sample at stream position s is x[s % L], call k holds
[k L, (k + 1) L).  The reference demodulates any stretch of the stream from its position alone --
oracle.chirp_demod(cp, s % period, samples) -- and integrates a lock-in point as the float64 sum
sum_p w[p] d[p] over dem.window(); which positions a call's points start at comes from the oracle's VnaHelper (the
points it completes and the samples it carries over), not from the handle under test.
"""
import json
import os
import time

import numpy as np

from test_gpu_parity import TOL, crandn, rel_err_per_tone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("plain", "split", "generic")


class Law:
    """A sweep law shared by the chirps `spans` ((freq, chirp_f) each): the parameters g.chirp_derive gives, with the
    length and period the test relies on asserted -- the derivation is in float32 and must not be assumed."""

    def __init__(self, oracle, rate, steps, chirp_t, spans, length, period=None):
        import gpu_sdr_amd as g
        self.rate, self.steps, self.chirp_t, self.spans = rate, steps, chirp_t, list(spans)
        self.cps = []
        for f0, f1 in self.spans:
            cp = g.chirp_derive(rate, f0, f1, steps, chirp_t)
            assert (cp.num_steps, cp.length) == (steps, length), (rate, steps, chirp_t, cp.num_steps, cp.length)
            self.cps.append(oracle.ChirpParam(cp.num_steps, cp.length, cp.chirpness, cp.f0))
        self.length, self.period = length, steps * length
        assert period is None or self.period == period, (self.period, period)

    def handle(self, decim, L, cols=None, multi=None):
        """A handle for the chirps `cols` of the law (all by default); several chirps, or multi=True, through
        GSDR_CREATE_MULTI_CHIRP"""
        import gpu_sdr_amd as g
        sp = [self.spans[c] for c in (range(len(self.spans)) if cols is None else cols)]
        p = g.param(mode="RX", rate=self.rate, buffer_len=L, decim=decim, freq=[s[0] for s in sp], chirp_f=[s[1] for s in sp],
                    swipe_s=[self.steps], chirp_t=[self.chirp_t], wave_type=[g.w_type.CHIRP] * len(sp))
        dem = g.RX_buffer_demodulator(p, device_index=0, multi_chirp=len(sp) > 1 if multi is None else multi)
        assert dem.channels == len(sp)
        return dem


class Reference:
    """Demodulated stretches of the stream x[s % L] by the chirps of a law, computed once per (chirp, stretch) and
    shared by the handles of a walk (a single-chirp handle is chirp 0 of the multi-chirp one)."""

    def __init__(self, oracle, law, x):
        self.oracle, self.law, self.x = oracle, law, x
        self._memo = {}

    def demod(self, c, s0, n):
        """complex64[n]: stream positions [s0, s0 + n) demodulated by chirp c"""
        key = (self.law.spans[c], s0, n)
        if key not in self._memo:
            L = self.x.size
            reps = (s0 % L + n + L - 1) // L
            smp = np.tile(self.x, reps)[s0 % L:s0 % L + n]
            self._memo[key] = self.oracle.chirp_demod(self.law.cps[c], s0 % self.law.period, smp)
        return self._memo[key]

    def points(self, c, s0, valid, w):
        """complex128[valid]: the points of w.size samples each that start at stream position s0, by chirp c"""
        d = self.demod(c, s0, valid * w.size).reshape(valid, w.size)
        return d.astype(np.complex128) @ w.astype(np.float64)


def clean_env(monkeypatch, env):
    """Only `env` of the engine switches is set (GSDR_LIB*, which pick the library itself, stay as they are); a handle
    reads them when it is created."""
    for k in [k for k in os.environ if k.startswith("GSDR_") and not k.startswith("GSDR_LIB")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def expect_calls(dem, parts=None, **calls):
    """describe()["chirp_calls"] is exactly `calls` (forms not named: 0), "chirp_parts" is `parts` when given"""
    d = dem.describe()
    want = dict({f: 0 for f in FORMS}, **calls)
    assert d["chirp_calls"] == want, (d["chirp_calls"], want)
    if parts is not None:
        assert d["chirp_parts"] == parts, (d["chirp_parts"], parts)


class Feed:
    """One handle of a walk.  decim > 0: lock-in, every point of a compared call is compared; decim == 0: undecimated,
    `windows(k)` -> [(first, count)] are the samples of call k that are compared (None: all of them)."""

    def __init__(self, name, dem, law, decim, L, cols=None, windows=None):
        self.name, self.dem, self.law, self.decim, self.L, self.windows = name, dem, law, decim, L, windows
        self.cols = list(range(len(law.spans)) if cols is None else cols)      # the chirps of the law the handle was made for
        self.C = dem.channels
        assert self.C == len(self.cols)
        self.w = dem.window() if decim else None
        if decim:
            assert self.w.size == law.length * decim
        self.got, self.where, self.valids = [], [], []

    def chunks(self, k, carry, valid):
        """[(first row, rows, stream position)] of the compared rows of call k"""
        if self.decim:
            return [(0, valid, k * self.L - carry)]
        return [(a, n, k * self.L + a) for a, n in (self.windows(k) if self.windows else [(0, self.L)])]


def walk(dev, oracle, ref, feeds, x, calls, compare):
    """Feeds the device buffer x to every handle `calls` times in one loop; the calls in `compare` are kept.  Every
    returned length is checked against the oracle's VnaHelper; returns ({name: worst relative error per chirp over all
    compared rows of the handle together}, seconds of the loop)."""
    import torch
    L = x.size
    xd = torch.from_numpy(x).to(dev)
    outs = [torch.empty(f.dem.out_capacity, dtype=torch.complex64, device=dev) for f in feeds]
    helpers = [oracle.VnaHelper(f.w.size, L) if f.decim else None for f in feeds]
    carries = [0] * len(feeds)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(calls):
        for i, f in enumerate(feeds):
            n = f.dem.process_device(xd, outs[i])
            h = helpers[i]
            valid = h.valid_size if h else L
            assert n == valid * f.C and n <= f.dem.out_capacity, (f.name, k, n, valid, f.C)
            f.valids.append(valid)
            if k in compare:
                rows = outs[i][:n].view(valid, f.C)
                for a, cnt, s0 in f.chunks(k, carries[i], valid):
                    assert s0 >= 0 and (not f.decim or s0 % f.w.size == 0), (f.name, k, s0)
                    f.got.append(rows[a:a + cnt].clone())
                    f.where.append((s0, cnt))
            if h:
                carries[i] = h.new0
                h.update()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    errs = {}
    for f in feeds:
        y = np.concatenate([g.cpu().numpy() for g in f.got])
        yr = np.empty(y.shape, dtype=np.complex128)
        at = 0
        for s0, cnt in f.where:
            for j, c in enumerate(f.cols):
                yr[at:at + cnt, j] = ref.points(c, s0, cnt, f.w) if f.decim else ref.demod(c, s0, cnt)
            at += cnt
        assert at == y.shape[0] >= 8, (f.name, at)          # the norm is over all compared rows, never over a few
        assert np.isfinite(y.view(np.float32)).all(), f.name
        errs[f.name] = rel_err_per_tone(y, yr, f.name)
    return errs, seconds


def margin_file(update):
    """Keeps profiles/chirp_positions_margins.json at what this run measured (worst error and loop time per test)."""
    path = os.path.join(ROOT, "profiles", "chirp_positions_margins.json")
    try:
        old = json.load(open(path)) if os.path.exists(path) else {}
        doc = dict(old)
        doc.update(update)
        if doc != old:
            with open(path, "w") as fh:
                json.dump(doc, fh, indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass


def check(test, errs, seconds, calls):
    """Prints and records every figure, then asserts the bar"""
    worst = max(float(e.max()) for e in errs.values())
    print(f"{test}: {calls} calls in {seconds:.3f} s, worst relative error {worst:.3e} "
          + ", ".join(f"{k} {float(e.max()):.2e}" for k, e in errs.items()))
    margin_file({test: {"calls": calls, "walk_seconds": round(seconds, 3), "worst_relative_error": worst,
                        "per_handle": {k: float(e.max()) for k, e in errs.items()}}})
    for name, e in errs.items():
        assert e.max() <= TOL, (test, name, e.tolist())


