"""Models of the resonator map (include/gsdr.h, "resonator map on the device") for the CPU and GPU tests.

reference_law   the reference's law restated in numpy complex128 from its formula: divide by the cable term
                A exp(2 pi i (1e-6 D (f_tone - f0) + phi)), q = (1/Qe) / (1 - z), f0 Im(q) / 2 and Re(q) or 1 / Re(q).
contract_bits   a bit model of the contract: every operation of its arithmetic on exact rationals
                (fractions.Fraction), rounded once to double, the outputs rounded once more to float32.  Inf, NaN and
                exact zeros follow IEEE 754 (numpy's float64), where a rational has nothing to say.
synthesise      a resonator's samples for known x(t) and 1/Qr(t): s = n (1 - dQe / (dQr + 2 i x)), as complex64.

Plain module, no GPU work and no library call at import time.
"""
from fractions import Fraction

import numpy as np

KINDS = ("cal", "x_dqr", "x_qr")
VALUE_KINDS = ("ordinary", "denormal", "1e38", "inf", "nan", "equal_n")
U32 = 2.0 ** -24                # unit roundoff of float32


def fit_of(rng, qr_lo=3e3, qr_hi=1e5):
    """One random fit tuple (f0 [MHz], A, phi, D, Qi, Qr, Qe_re, Qe_im, a) and a tone [Hz] inside the resonance."""
    qr = float(np.exp(rng.uniform(np.log(qr_lo), np.log(qr_hi))))
    ratio = rng.uniform(0.15, 0.45)                          # Qr / |Qe|: |1 - z| < 1/2 < |z| near the resonance
    qe = qr / ratio
    qe_im = qe * rng.uniform(-0.2, 0.2)
    qe_re = float(np.sqrt(qe * qe - qe_im * qe_im))
    qi = 1.0 / (1.0 / qr - (1.0 / complex(qe_re, qe_im)).real)
    f0 = rng.uniform(100.0, 900.0)
    tone = f0 * 1e6 * (1.0 + rng.uniform(-0.3, 0.3) / qr)
    fit = (f0, rng.uniform(0.01, 2.0), rng.uniform(-0.5, 0.5), rng.uniform(-200.0, 200.0), qi, qr, qe_re, qe_im, 0.0)
    return fit, float(tone)


def cable_term(fit, tone):
    f0, A, phi, D = fit[:4]
    return A * np.exp(2j * np.pi * (1e-6 * D * (tone - f0 * 1e6) + phi))


def reference_law(s, fit, tone, kind):
    """complex128 [n]: the calibrated S21 (cal), or x + i y with x the frequency shift in Hz and y = Re(q) or 1/Re(q)."""
    f0, qe = fit[0] * 1e6, complex(fit[6], fit[7])
    z = np.asarray(s).astype(np.complex128) / cable_term(fit, tone)
    if kind == "cal":
        return z
    with np.errstate(all="ignore"):
        q = (1.0 / qe) / (1.0 - z)
        return f0 * q.imag / 2.0 + 1j * (q.real if kind == "x_dqr" else 1.0 / q.real)


def synthesise(fit, tone, x, dqr):
    """complex64 [n]: the samples of a resonator at fractional frequency shift x(t) and inverse quality factor dqr(t)."""
    dqe = 1.0 / complex(fit[6], fit[7])
    q = np.asarray(dqr, dtype=np.float64) + 2j * np.asarray(x, dtype=np.float64)
    return (cable_term(fit, tone) * (1.0 - dqe / q)).astype(np.complex64)


# ---- the bit model -----------------------------------------------------------------------------------------------------
def _rnd(v):
    """an exact rational, not 0, to the nearest double (ties to even: int / int in Python is correctly rounded)"""
    try:
        return float(v)
    except OverflowError:
        return float("inf") if v > 0 else float("-inf")


def _ieee(op, a, b):
    with np.errstate(all="ignore"):
        a, b = np.float64(a), np.float64(b)
        return float({"+": a + b, "-": a - b, "*": a * b, "/": a / b}[op])


def _op(op, a, b):
    """one IEEE double operation: exact in rationals and rounded once; Inf, NaN and zeros by IEEE's rules"""
    if not (np.isfinite(a) and np.isfinite(b)) or (op == "/" and b == 0.0):
        return _ieee(op, a, b)
    fa, fb = Fraction(a), Fraction(b)
    v = {"+": fa + fb, "-": fa - fb, "*": fa * fb, "/": fa / fb if op == "/" else 0}[op]
    return _ieee(op, a, b) if v == 0 else _rnd(v)             # a zero takes its sign from IEEE (the result is exact)


def _fma(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    v = Fraction(a) * Fraction(b) + Fraction(c)
    if v != 0:
        return _rnd(v)
    if a == 0.0 or b == 0.0:                                  # an exact zero product plus a zero: the signs decide
        return _ieee("+", _ieee("*", a, b), c)
    return 0.0                                                # exact cancellation: +0 in round-to-nearest


def _f32(v):
    with np.errstate(all="ignore"):
        return np.float32(np.float64(v))


def contract_sample(kind, c, x0, y0, s):
    """One sample by the contract's arithmetic.  c: the 7 constants (nr, ni, gr, gi, kr, ki, hf0) as floats."""
    nr, ni, gr, gi, kr, ki, hf0 = (float(v) for v in c)
    sx, sy = float(np.float32(s.real)), float(np.float32(s.imag))
    if kind == "cal":
        zr = _fma(sx, gr, -_op("*", sy, gi))
        zi = _fma(sx, gi, _op("*", sy, gr))
        return _f32(_op("-", zr, x0)), _f32(_op("-", zi, y0))
    wr, wi = _op("-", nr, sx), _op("-", ni, sy)
    m = _fma(wr, wr, _op("*", wi, wi))
    a = _fma(kr, wr, _op("*", ki, wi))
    b = _fma(ki, wr, -_op("*", kr, wi))
    qi = _op("/", b, m)
    fx = _fma(hf0, qi, -float(x0))
    y = _op("-", _op("/", a, m), y0) if kind == "x_dqr" else _op("-", _op("/", m, a), y0)
    return _f32(fx), _f32(y)


def contract_bits(kind, constants, rows, channels=None, offsets=None):
    """complex64 [n][n_out] by the bit model.  constants: [n_out][7]; rows: complex64 [n][n_ch]."""
    constants = np.asarray(constants, dtype=np.float64)
    n_out = constants.shape[0]
    channels = list(range(n_out)) if channels is None else list(channels)
    offsets = np.zeros((n_out, 2)) if offsets is None else np.asarray(offsets, dtype=np.float64).reshape(n_out, 2)
    rows = np.asarray(rows, dtype=np.complex64)
    out = np.zeros((rows.shape[0], n_out), dtype=np.complex64)
    parts = out.view(np.float32)                              # [n][2 n_out]: the float32 results go in as they are
    for k in range(n_out):
        for i in range(rows.shape[0]):
            x, y = contract_sample(kind, constants[k], float(offsets[k, 0]), float(offsets[k, 1]), rows[i, channels[k]])
            parts[i, 2 * k], parts[i, 2 * k + 1] = x, y
    return out


def same_values(a, b):
    """Bit for bit, except that a NaN matches any NaN (the contract fixes neither sign nor payload of a NaN)."""
    a, b = np.ascontiguousarray(a, dtype=np.complex64), np.ascontiguousarray(b, dtype=np.complex64)
    if a.shape != b.shape:
        return False
    fa, fb = a.view(np.float32).reshape(-1), b.view(np.float32).reshape(-1)
    na, nb = np.isnan(fa), np.isnan(fb)
    return bool(np.array_equal(na, nb) and np.array_equal(fa.view(np.int32)[~na], fb.view(np.int32)[~nb]))


def first_difference(a, b):
    """for a failing same_values: where and what"""
    fa = np.ascontiguousarray(a, dtype=np.complex64).view(np.float32).reshape(-1)
    fb = np.ascontiguousarray(b, dtype=np.complex64).view(np.float32).reshape(-1)
    bad = np.flatnonzero(~((np.isnan(fa) & np.isnan(fb)) | (fa.view(np.int32) == fb.view(np.int32))))
    return None if bad.size == 0 else (int(bad.size), int(bad[0]), float(fa[bad[0]]), float(fb[bad[0]]))


# ---- inputs --------------------------------------------------------------------------------------------------------------
def noisy_stream(rng, fit, tone, rows):
    """A resonator's timestream: x within a fifth of a linewidth, 1/Qr within a few per cent, both moving."""
    qr = fit[5]
    t = np.arange(rows)
    x = (0.02 + 0.2 * np.sin(0.37 * t + rng.uniform(0, 6.0)) + 0.05 * rng.standard_normal(rows)) / qr
    dqr = (1.0 + 0.03 * np.cos(0.11 * t) + 0.01 * rng.standard_normal(rows)) / qr
    return synthesise(fit, tone, x, dqr), x, dqr


def value_samples(value_kind, fit, tone, count, seed):
    """complex64 [count] of one value kind (VALUE_KINDS) for a column with this fit"""
    rng = np.random.default_rng(seed)
    s = noisy_stream(rng, fit, tone, count)[0]
    if value_kind == "ordinary":
        return s
    if value_kind == "denormal":
        tiny = rng.integers(1, 1 << 22, size=(count, 2)).astype(np.uint32) | (rng.integers(0, 2, size=(count, 2)).astype(np.uint32) << 31)
        return tiny.view(np.float32).reshape(count, 2).copy().view(np.complex64).reshape(count)
    if value_kind == "1e38":
        return (rng.choice([-1.0, 1.0], size=count) * 1e38 * rng.uniform(0.5, 3.0, size=count)
                + 1j * rng.choice([-1.0, 1.0], size=count) * 1e38 * rng.uniform(0.5, 3.0, size=count)).astype(np.complex64)
    if value_kind in ("inf", "nan"):
        bad = np.float32(np.inf if value_kind == "inf" else np.nan)
        f = s.view(np.float32).reshape(count, 2).copy()
        where = rng.integers(0, 3, size=count)               # the real part, the imaginary part, both
        f[where != 1, 0] = bad * rng.choice([-1.0, 1.0]).astype(np.float32)
        f[where != 0, 1] = bad
        return f.view(np.complex64).reshape(count)
    if value_kind == "equal_n":
        # the sample IS the cable term only where that is a float32 pair: such columns are made by exact_n_constants
        raise ValueError("equal_n needs exact_n_constants")
    raise ValueError(value_kind)


def exact_n_constants(lib_constants, fit, tone):
    """(constants [7], n as complex64) of a column whose cable term is exactly a float32 pair: the library's constants of
    the fit with n rounded to float32 and g, K rederived in double -- what any caller may hand to gsdr_resmap_create."""
    c = np.array(lib_constants, dtype=np.float64)
    n32 = np.complex64(complex(c[0], c[1]))
    n = complex(n32)
    qe = complex(fit[6], fit[7])
    g, k = 1.0 / n, n / qe
    return np.array([n.real, n.imag, g.real, g.imag, k.real, k.imag, c[6]]), n32
