"""A float64 model of TONES and NOISE at decim 0, and the plan of a call (gsdr_pfb_plan) for the tests to assert.

The model states the operation and nothing of how a kernel computes it: the stream is carried across calls as
buffer_helper counts frames (frame r of a call exists while (r + avg) * nfft < carried + new samples, strictly), a
frame is sum_i x[(r + i) * nfft + k] * w[i * nfft + k] in complex128 with w = oracle.make_sinc_window(avg * nfft,
float(1 / (2 nfft))) -- never the window a handle reports --, and numpy.fft.fft transforms it; TONES keeps the
oracle's bins.  tests/test_pfb_model_host.py holds the model to oracle.Pfb / oracle.Noise (whose O(nfft^2) DFT is
too slow for hundreds of long frames); tests/test_gpu_pfb_runs.py holds the device to the model.

Plain module: numpy only at import, the oracle and the library are handed in.
"""
import ctypes as C

import numpy as np

# the GSDR_PFB_* switches gsdr_pfb_plan takes by value, with the values of an unset environment
SWITCH_DEFAULTS = {"pfb_cu": -1, "pfb_direct": 1, "pfb_col": -1, "pfb_cu_nt": 0, "pfb_teams": 1, "pfb_radix8": 1,
                   "pfb_fr": 0, "pfb_wide": -1}
ENV_OF_SWITCH = {k: "GSDR_" + k.upper() for k in SWITCH_DEFAULTS}
PLAN_IN_FIELDS = ("nfft", "avg", "blue_m", "frames", "n_out", "cus") + tuple(SWITCH_DEFAULTS)
PLAN_OUT_FIELDS = ("cu", "threads", "G", "twl", "lds", "b_off", "b_len", "col", "direct", "dir_s", "dir_gs", "teams",
                   "len", "n_radices")
PLAN_IN_DTYPE = np.dtype([(n, np.int32) for n in PLAN_IN_FIELDS])
PLAN_OUT_DTYPE = np.dtype([(n, np.int32) for n in PLAN_OUT_FIELDS] + [("radices", np.int32, (16,))])


def switches_of_env(env):
    """{"GSDR_PFB_CU": "1", ...} -> the switch values gsdr_pfb_plan takes (what read_switches makes of them)"""
    sw = dict(SWITCH_DEFAULTS)
    for k, name in ENV_OF_SWITCH.items():
        if name in env:
            sw[k] = int(env[name])
    for k in ("pfb_direct", "pfb_teams", "pfb_radix8"):
        sw[k] = int(sw[k] != 0)
    return sw


def blue_length(lib, nfft, avg, sw=None, pfb_bluestein=-1):
    sw = sw or SWITCH_DEFAULTS
    return lib.gsdr_pfb_blue_length(nfft, avg, pfb_bluestein, sw["pfb_direct"], sw["pfb_radix8"])


def plan(lib, nfft, avg, frames, cus, n_out=None, sw=None, blue_m=None):
    """The plan of one call as a dict (None: gsdr_pfb_plan refuses the arguments); blue_m None: what a handle takes."""
    sw = {**SWITCH_DEFAULTS, **(sw or {})}
    if blue_m is None:
        blue_m = blue_length(lib, nfft, avg, sw)
    rows = np.zeros(1, dtype=PLAN_IN_DTYPE)
    rows[0] = (nfft, avg, blue_m, frames, nfft if n_out is None else n_out, cus) + tuple(sw[k] for k in SWITCH_DEFAULTS)
    out = np.zeros(1, dtype=PLAN_OUT_DTYPE)
    if lib.gsdr_pfb_plan_many(rows.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p)) != 0:
        return None
    d = {k: int(out[0][k]) for k in PLAN_OUT_FIELDS}
    d["radices"] = [int(v) for v in out[0]["radices"][:d["n_radices"]]]
    d["blue_m"] = blue_m
    return d


def plan_many(lib, rows):
    """rows: a PLAN_IN_DTYPE array every row of which the rule takes -> a PLAN_OUT_DTYPE array"""
    rows = np.ascontiguousarray(rows)
    out = np.zeros(rows.size, dtype=PLAN_OUT_DTYPE)
    rc = lib.gsdr_pfb_plan_many(rows.ctypes.data_as(C.c_void_p), rows.size, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, "gsdr_pfb_plan refused a row"
    return out


def plan_class(p):
    """The class of a plan the host table has one row per: (kernel, threads, direct, col, teams, G >= 2, dir_gs >= 2,
    dir_s >= 2, Bluestein, first stage a prime above 13).  (The rule itself asks radices[0] > 13, which a first stage
    of radix 16 answers too: frames from 4096 points on and Bluestein lengths.  tests/test_pfb_plan_host.py pins that.)"""
    return ("cu" if p["cu"] else "lds", p["threads"], p["direct"], p["col"], p["teams"], int(p["G"] >= 2),
            int(p["dir_gs"] >= 2), int(p["dir_s"] >= 2), int(p["blue_m"] > 0),
            int(bool(p["radices"]) and p["radices"][0] > 16))


def describe_matches_plan(last, p, frames):
    """describe()["pfb_last"] of a call of `frames` frames against the plan p of that call"""
    want = {"kernel": "pfb_cu_kernel" if p["cu"] else "pfb_lds_kernel", "frames": frames}
    want.update({k: p[k] for k in ("threads", "G", "direct", "dir_s", "dir_gs", "col", "teams", "twl", "lds")})
    assert last == want, (last, want)


class Model:
    """TONES (bins: the column -> bin table) or NOISE (bins None) in float64, fed buffers of any length."""

    def __init__(self, oracle, nfft, avg, bins=None):
        self.nfft, self.avg = int(nfft), int(avg)
        self.w = oracle.make_sinc_window(self.nfft * self.avg, np.float32(1.0 / (2 * self.nfft))).astype(np.float64)
        self.w = self.w.reshape(self.avg, self.nfft)
        self.bins = None if bins is None else np.where(np.asarray(bins) < 0, 0, np.asarray(bins)).astype(np.int64)
        self.carry = np.zeros(0, dtype=np.complex128)

    def frames_of(self, n_new):
        """complete frames of a call that brings n_new samples"""
        lim = self.carry.size + n_new - self.avg * self.nfft
        return 0 if lim <= 0 else (lim + self.nfft - 1) // self.nfft

    def process(self, x):
        nfr = self.frames_of(len(x))
        s = np.concatenate([self.carry, np.asarray(x).astype(np.complex128)])
        self.last_stream = s                   # what the call's frames were made of (the fp32 emulation takes the same)
        n = self.nfft
        fr = np.zeros((nfr, n), dtype=np.complex128)
        for i in range(self.avg):
            fr += s[i * n:(i + nfr) * n].reshape(nfr, n) * self.w[i]
        self.carry = s[nfr * n:]
        y = np.fft.fft(fr, axis=1)
        return y if self.bins is None else y[:, self.bins]


def fp32_emulation(x_stream, nfft, avg, w32, nfr):
    """What a correct float32 evaluation gives for the first nfr frames of a stream: complex64 accumulation in tap
    order, then a radix-2 / mixed transform in complex64 (numpy.fft computes in double: every stage of a
    decimation-in-time split is cast back to complex64, sub-transforms of odd length in one step)."""
    n = nfft
    s = np.asarray(x_stream, dtype=np.complex64)
    acc = np.zeros((nfr, n), dtype=np.complex64)
    w32 = np.asarray(w32, dtype=np.float32).reshape(avg, n)
    for i in range(avg):
        acc = (acc + s[i * n:(i + nfr) * n].reshape(nfr, n) * w32[i]).astype(np.complex64)

    def fft32(a):
        m = a.shape[-1]
        if m % 2 or m <= 2:
            return np.fft.fft(a.astype(np.complex128), axis=-1).astype(np.complex64)
        e, o = fft32(a[..., 0::2]), fft32(a[..., 1::2])
        tw = np.exp(-2j * np.pi * np.arange(m // 2) / m).astype(np.complex64)
        t = (o * tw).astype(np.complex64)
        return np.concatenate([(e + t).astype(np.complex64), (e - t).astype(np.complex64)], axis=-1)

    return fft32(acc)


def tones_on_bins(rng, n, nfft, bins, w, scale=10.0):
    """crandn plus len(bins) tones placed on the bins, each standing `scale` x rms above the noise IN ITS BIN: a frame
    or column that is swapped or stale then moves a large, known value.  w: the window (its taps sum to 1, so a tone
    of amplitude a on a bin arrives there as a; a noise bin has rms sqrt(2 sum w^2) for crandn's variance of 2).
    The tones are sized in the spectrum and not in the stream on purpose: a tone of 10 x the STREAM's rms stands 150
    (128 points) to 860 times (4096) above the noise bins, and a correct float32 evaluation of filter and transform
    (fp32_emulation) is then 6e-6 to 3e-5 from the model in the noise bins beside it -- rounding of the tone's partial
    sums, relative to a bin that holds almost nothing.  The per-bin bar of 1e-5 would measure the input."""
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    k = np.arange(n)
    a = scale * np.sqrt(2.0 * np.sum(np.asarray(w, dtype=np.float64) ** 2))
    for j, b in enumerate(bins):
        x += a * np.exp(2j * np.pi * ((b * k) % nfft) / nfft + 1j * (0.7 + j))
    return x.astype(np.complex64)
