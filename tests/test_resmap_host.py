"""The resonator map's host twin and gsdr_resmap_constants (include/gsdr.h, "resonator map on the device") without a
GPU: the twin against the bit model of the contract (tests/_resmap.py, exact rationals rounded once per operation), against
the reference's law restated in complex128, and against the closed form of a synthesised resonator; the constants, the
refusals, channel lists, offsets, poison, NULL objects.

Bounds.  Twin against complex128: |err| <= 2^-24 |ref| (1 + 1e-6) + 1e-12 (|unshifted value| + |offset|) per output
component -- one float32 rounding on top of double arithmetic.  Closed form: the float32 rounding of the INPUT alone moves
q = dQe / (1 - z) by |dq| <= |q| |dz| / |1 - z| with |dz| <= 2^-24 |z|, so the frequency shift by f0/2 |dq|, 1/Qr by
|dq| and Qr by |dq| / Re(q)^2; the outputs must stay within twice that.  (The second half pays for the float32 rounding of
the output, which is at most the first half wherever |z| >= |1 - z| -- the synthesised resonators are chosen so, and the
test says so -- and for the double arithmetic, 1e-9 of it.)

The measured worst of the complex128 comparison is written to the file that GSDR_RESMAP_MARGINS names, when it is set;
profiles/resmap_margins.json is the committed copy."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from _resmap import (KINDS, U32, VALUE_KINDS, cable_term, contract_bits, exact_n_constants, first_difference, fit_of, noisy_stream,
                     reference_law, same_values, value_samples)


@pytest.fixture(scope="module")
def resmap(gsdr_lib):
    from gpu_sdr_amd import resmap
    return resmap


def columns(resmap, n, seed, **kw):
    rng = np.random.default_rng(seed)
    fits, tones = zip(*[fit_of(rng, **kw) for _ in range(n)])
    return list(fits), np.array(tones), resmap.resmap_constants(fits, tones)


def twin(resmap, kind, constants, rows, channels=None, offsets=None, max_rows=None):
    rows = np.ascontiguousarray(rows, dtype=np.complex64)
    h = resmap.host_resmap(rows.shape[1], max_rows or max(rows.shape[0], 1), constants, channels=channels, kind=kind)
    if offsets is not None:
        h.set_offsets(offsets)
    out = h.feed(rows)
    h.close()
    return out


@pytest.mark.parametrize("value_kind", VALUE_KINDS)
@pytest.mark.parametrize("kind", KINDS)
def test_twin_equals_the_bit_model(resmap, kind, value_kind):
    """4 columns x 60 samples of one value kind.  "equal_n": columns whose cable term is a float32 pair; every third
    sample is that pair, the others lie one or two float32 steps beside it."""
    n_col, n = 4, 60
    fits, tones, constants = columns(resmap, n_col, seed=11)
    rows = np.zeros((n, n_col), dtype=np.complex64)
    for k in range(n_col):
        if value_kind == "equal_n":
            constants[k], n32 = exact_n_constants(constants[k], fits[k], tones[k])
            re = np.full(n, n32.real, dtype=np.float32)
            im = np.full(n, n32.imag, dtype=np.float32)
            re[1::3] = np.nextafter(re[1::3], np.float32(np.inf))
            im[2::3] = np.nextafter(np.nextafter(im[2::3], np.float32(-np.inf)), np.float32(-np.inf))
            rows[:, k] = re + 1j * im
            assert rows[0, k] == n32 and rows[1, k] != n32
        else:
            rows[:, k] = value_samples(value_kind, fits[k], tones[k], n, seed=100 + k)
    got = twin(resmap, kind, constants, rows)
    want = contract_bits(kind, constants, rows)
    assert same_values(got, want), first_difference(got, want)
    f = got.view(np.float32)
    if value_kind in ("ordinary", "denormal"):                                   # (1e38: Qr = m / a passes float32's range)
        assert np.all(np.isfinite(f))
    if value_kind == "equal_n" and kind != "cal":
        assert np.all(np.isnan(f[0::3])) and np.all(np.isfinite(f[1::3]))        # 0/0; its neighbours are ordinary numbers
    if value_kind in ("inf", "nan"):
        assert np.all((~np.isfinite(f)).reshape(n, n_col, 2).all(axis=2))         # every sample's output shows it, in both parts


def complex128_bound(ref_component, unshifted_component, offset):
    return U32 * np.abs(ref_component) * (1 + 1e-6) + 1e-12 * (np.abs(unshifted_component) + np.abs(offset))


def test_twin_against_the_complex128_restatement(resmap):
    """200 random resonators, Qr from 3e3 to 1e5, 48 rows each, all three kinds, without offsets and with the mean of the
    stream as the offsets."""
    n_col, n = 200, 48
    fits, tones, constants = columns(resmap, n_col, seed=5)
    rng = np.random.default_rng(6)
    rows = np.stack([noisy_stream(rng, fits[k], tones[k], n)[0] for k in range(n_col)], axis=1)
    worst = {}
    for kind in KINDS:
        plain = np.stack([reference_law(rows[:, k], fits[k], tones[k], kind) for k in range(n_col)], axis=1)
        for label, offsets in (("plain", np.zeros((n_col, 2))), ("mean", np.stack([plain.real.mean(axis=0), plain.imag.mean(axis=0)], axis=1))):
            got = twin(resmap, kind, constants, rows, offsets=offsets).astype(np.complex128)
            ref = plain - (offsets[:, 0] + 1j * offsets[:, 1])
            for part in ("real", "imag"):
                err = np.abs(getattr(got, part) - getattr(ref, part))
                bound = complex128_bound(getattr(ref, part), getattr(plain, part), offsets[:, 0 if part == "real" else 1])
                rel = float((err / np.abs(getattr(ref, part))).max())
                worst[f"{kind} {label} {part}"] = rel
                print(f"resmap twin vs complex128, {kind} {label} {part}: worst relative {rel:.3e}, worst err / bound {float((err / bound).max()):.3f}")
                assert np.all(err <= bound), (kind, label, part, float((err / bound).max()))
    path = os.environ.get("GSDR_RESMAP_MARGINS")
    if path:
        doc = {"bound": "2^-24 |ref| (1 + 1e-6) + 1e-12 (|unshifted value| + |offset|) per output component",
               "metric": "max over 200 resonators x 48 rows of |twin - complex128| / |complex128| ('mean': with the stream's mean as the offsets, relative to the shifted value)",
               "worst_without_offsets": max(v for k, v in worst.items() if " plain " in k), "per_case": worst}
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(doc, fh, indent=1)


@pytest.mark.parametrize("kind", ["x_dqr", "x_qr"])
def test_closed_form_of_a_synthesised_resonator(resmap, kind):
    n_col, n = 24, 400
    fits, tones, constants = columns(resmap, n_col, seed=21)
    rng = np.random.default_rng(22)
    rows = np.zeros((n, n_col), dtype=np.complex64)
    xs, dqrs = np.zeros((n, n_col)), np.zeros((n, n_col))
    for k in range(n_col):
        rows[:, k], xs[:, k], dqrs[:, k] = noisy_stream(rng, fits[k], tones[k], n)
    got = twin(resmap, kind, constants, rows)
    worst = 0.0
    for k in range(n_col):
        f0, dqe = fits[k][0] * 1e6, 1.0 / complex(fits[k][6], fits[k][7])
        q = dqrs[:, k] + 2j * xs[:, k]
        z = 1.0 - dqe / q
        assert np.all(np.abs(z) >= np.abs(1.0 - z))              # where the output's rounding is no more than the input's
        dq = U32 * np.abs(q) * np.abs(z) / np.abs(1.0 - z)
        ex = np.abs(got[:, k].real.astype(np.float64) - f0 * xs[:, k])
        if kind == "x_dqr":
            ey, by = np.abs(got[:, k].imag.astype(np.float64) - dqrs[:, k]), dq
        else:
            ey, by = np.abs(got[:, k].imag.astype(np.float64) - 1.0 / dqrs[:, k]), dq / dqrs[:, k] ** 2
        worst = max(worst, float((ex / (f0 / 2 * dq)).max()), float((ey / by).max()))
        assert np.all(ex <= 2 * f0 / 2 * dq) and np.all(ey <= 2 * by), (k, float((ex / (f0 / 2 * dq)).max()), float((ey / by).max()))
    print(f"resmap closed form, {kind}: worst error {worst:.3f} of the input-rounding bound (bar 2)")


def test_constants_agree_with_complex128(resmap, gsdr_lib):
    fits, tones, constants = columns(resmap, 300, seed=31)
    for fit, tone, c in zip(fits, tones, constants):
        n = cable_term(fit, tone)
        qe = complex(fit[6], fit[7])
        for got, want in ((complex(c[0], c[1]), n), (complex(c[2], c[3]), 1.0 / n), (complex(c[4], c[5]), n / qe)):
            # the phase 2 pi theta is known to 2^-53 |2 pi theta|: |theta| < 1e3 here, 1e-12 holds with room
            assert abs(got - want) <= 1e-12 * abs(want), (fit, tone)
        assert c[6] == fit[0] * 1e6 / 2


def test_constants_refuse_by_name(resmap, gsdr_lib):
    from gpu_sdr_amd import GsdrError
    names = ["f_tone", "f0", "A", "phi", "D", "Qe_re", "Qe_im"]
    good = [4.0e8, 400.0, 0.5, 0.1, 30.0, 2e4, 1e3]
    out = (C.c_double * 7)()
    assert gsdr_lib.gsdr_resmap_constants(*good, out) == 0
    for i, name in enumerate(names):
        for bad in (float("nan"), float("inf"), -float("inf")):
            args = list(good)
            args[i] = bad
            assert gsdr_lib.gsdr_resmap_constants(*args, out) == -1
            msg = gsdr_lib.gsdr_last_error(None).decode()
            assert msg.startswith("gsdr_resmap_constants: ") and name in msg.split(": ", 1)[1].split(" ")[0], msg
    for i, bad in ((1, 0.0), (1, -400.0), (2, 0.0), (2, -0.5)):
        args = list(good)
        args[i] = bad
        assert gsdr_lib.gsdr_resmap_constants(*args, out) == -1
        assert gsdr_lib.gsdr_last_error(None).decode().startswith(f"gsdr_resmap_constants: {names[i]} ")
    args = list(good)
    args[5] = args[6] = 0.0
    assert gsdr_lib.gsdr_resmap_constants(*args, out) == -1 and "Qe" in gsdr_lib.gsdr_last_error(None).decode()
    args[6] = 1e3                                                    # purely imaginary Qe is a number like any other
    assert gsdr_lib.gsdr_resmap_constants(*args, out) == 0
    assert gsdr_lib.gsdr_resmap_constants(*good, None) == -1 and "constants" in gsdr_lib.gsdr_last_error(None).decode()
    with pytest.raises(GsdrError, match="gsdr_resmap_constants: A "):
        resmap.resmap_constants([(400.0, -1.0, 0, 0, 1e5, 1e4, 2e4, 0, 0)], [4e8])


def test_create_refuses_by_name(resmap, gsdr_lib):
    _, _, k = columns(resmap, 3, seed=41)
    kp = k.ctypes.data
    ch = np.array([0, 2, 1], dtype=np.int32)
    HOST = -2

    def refused(name, *args):
        assert not gsdr_lib.gsdr_resmap_create(*args)
        msg = gsdr_lib.gsdr_last_error(None).decode()
        assert msg.startswith("gsdr_resmap_create: " + name), (name, msg)

    refused("n_ch", 0, 8, 3, ch.ctypes.data, kp, 1, HOST)
    refused("n_ch", (1 << 20) + 1, 8, 3, ch.ctypes.data, kp, 1, HOST)
    refused("max_rows", 3, 0, 3, None, kp, 1, HOST)
    refused("max_rows", 3, (1 << 20) + 1, 3, None, kp, 1, HOST)
    refused("n_out", 3, 8, 0, ch.ctypes.data, kp, 1, HOST)
    refused("n_out", 3, 8, (1 << 20) + 1, ch.ctypes.data, kp, 1, HOST)
    refused("channels", 4, 8, 3, None, kp, 1, HOST)                  # NULL is the identity: n_out == n_ch
    refused("channels", 2, 8, 3, ch.ctypes.data, kp, 1, HOST)        # an entry >= n_ch
    refused("channels", 3, 8, 3, np.array([0, -1, 1], dtype=np.int32).ctypes.data, kp, 1, HOST)
    refused("constants", 3, 8, 3, None, None, 1, HOST)
    bad = k.copy()
    bad[2, 4] = np.nan
    refused("constants", 3, 8, 3, None, bad.ctypes.data, 1, HOST)
    refused("kind", 3, 8, 3, None, kp, 3, HOST)
    refused("kind", 3, 8, 3, None, kp, -1, HOST)
    refused("device_index", 3, 8, 3, None, kp, 1, -3)
    h = gsdr_lib.gsdr_resmap_create(3, 8, 3, None, kp, 2, HOST)
    assert h and gsdr_lib.gsdr_resmap_n_out(h) == 3 and gsdr_lib.gsdr_resmap_kind(h) == 2
    gsdr_lib.gsdr_resmap_close(h)


def test_feed_refusals_and_null_objects(resmap, gsdr_lib):
    from gpu_sdr_amd import GsdrError
    _, _, k = columns(resmap, 3, seed=42)
    x = np.ones((9, 3), dtype=np.complex64)
    y = np.zeros((9, 3), dtype=np.complex64)
    h = resmap.host_resmap(3, 8, k, kind="cal")
    with pytest.raises(GsdrError, match=r"gsdr_resmap_feed_host: .*n_rows"):
        h.feed(x)
    L = gsdr_lib
    assert L.gsdr_resmap_feed_host(h._h, x.ctypes.data, -1, y.ctypes.data) == -1
    assert L.gsdr_resmap_feed_host(h._h, None, 0, None) == 0                       # touches no pointer
    assert L.gsdr_resmap_feed_host(h._h, None, 1, y.ctypes.data) == -1 and "rows" in L.gsdr_last_error(None).decode()
    assert L.gsdr_resmap_feed_host(h._h, x.ctypes.data, 1, None) == -1 and "out" in L.gsdr_last_error(None).decode()
    assert L.gsdr_resmap_feed_device(h._h, x.ctypes.data, 1, y.ctypes.data, None) == -1      # a host object
    assert L.gsdr_resmap_feed(h._h, x.ctypes.data, 1, y.ctypes.data, None) == -1
    bad = np.zeros((3, 2))
    bad[1, 1] = np.inf
    assert L.gsdr_resmap_set_offsets(h._h, bad.ctypes.data, None) == -1 and "xy" in L.gsdr_last_error(None).decode()
    assert np.array_equal(h.offsets, np.zeros((3, 2)))
    # in place with the identity; any other overlap is refused
    want = h.feed(x[:8])
    z = x[:8].copy()
    assert L.gsdr_resmap_feed_host(h._h, z.ctypes.data, 8, z.ctypes.data) == 8 and same_values(z, want)
    z = x.copy()
    assert L.gsdr_resmap_feed_host(h._h, z.ctypes.data, 8, z.ctypes.data + 8) == -1 and "overlaps" in L.gsdr_last_error(None).decode()
    h.close()
    g = resmap.host_resmap(3, 8, k, channels=[2, 1, 0], kind="cal")
    z = x.copy()
    assert L.gsdr_resmap_feed_host(g._h, z.ctypes.data, 8, z.ctypes.data) == -1 and "overlaps" in L.gsdr_last_error(None).decode()
    g.close()
    # NULL objects
    L.gsdr_resmap_close(None)
    assert L.gsdr_resmap_n_out(None) == 0 and L.gsdr_resmap_kind(None) == 0 and L.gsdr_resmap_get_constants(None, None, 0) == 0
    assert L.gsdr_resmap_get_offsets(None, None, 0) == 0 and L.gsdr_resmap_get_channels(None, None, 0) == 0
    assert L.gsdr_resmap_feed_host(None, x.ctypes.data, 1, y.ctypes.data) == -1 and "null object" in L.gsdr_last_error(None).decode()
    assert L.gsdr_resmap_feed_device(None, None, 0, None, None) == -1 and L.gsdr_resmap_feed(None, None, 0, None, None) == -1
    assert L.gsdr_resmap_set_offsets(None, None, None) == -1


@pytest.mark.parametrize("kind", KINDS)
def test_channel_lists(resmap, kind):
    """Subsets, reversals and repeats: output column k is the map of input column channels[k] with the constants of k."""
    n_ch, n = 7, 33
    rng = np.random.default_rng(51)
    fits, tones, k_all = columns(resmap, n_ch, seed=52)
    rows = np.stack([noisy_stream(rng, fits[c], tones[c], n)[0] for c in range(n_ch)], axis=1)
    whole = twin(resmap, kind, k_all, rows)
    for channels in ([4], [6, 5, 4, 3, 2, 1, 0], [1, 3, 5], [2, 2, 2, 0, 6, 2], list(range(7))):
        h = resmap.host_resmap(n_ch, n, k_all[channels], channels=channels, kind=kind)
        got = h.feed(rows)
        assert np.array_equal(h.channels, channels) and np.array_equal(h.constants, k_all[channels]) and h.n_out == len(channels)
        h.close()
        assert got.shape == (n, len(channels)) and same_values(got, whole[:, channels]), channels
    # a column mapped with ANOTHER column's constants is the map of those constants, not of the input column's
    other = twin(resmap, kind, k_all[[0]], rows, channels=[3])
    assert same_values(other, contract_bits(kind, k_all[[0]], rows, channels=[3]))


@pytest.mark.parametrize("kind", KINDS)
def test_offsets_are_subtracted_in_double(resmap, kind):
    """Offsets equal to the first feed's means (as a caller sets them), and ones a float32 subtraction would lose: the bit
    model subtracts exact rationals."""
    n_ch, n = 3, 40
    rng = np.random.default_rng(61)
    fits, tones, k = columns(resmap, n_ch, seed=62)
    rows = np.stack([noisy_stream(rng, fits[c], tones[c], n)[0] for c in range(n_ch)], axis=1)
    h = resmap.host_resmap(n_ch, n, k, kind=kind)
    first = h.feed(rows).astype(np.complex128)
    for offsets in (np.stack([first.real.mean(axis=0), first.imag.mean(axis=0)], axis=1),
                    np.stack([first.real[0] * (1 + 2.0 ** -30), first.imag[0] * (1 - 2.0 ** -29)], axis=1)):
        h.set_offsets(offsets)
        assert np.array_equal(h.offsets, offsets)
        got = h.feed(rows)
        want = contract_bits(kind, k, rows, offsets=offsets)
        assert same_values(got, want), first_difference(got, want)
    # what is left of row 0 is the rounding error of its float32 and 2^-30 of the value: small, and not lost
    assert np.all(got[0].real != 0) and np.all(np.abs(got[0].real) < 2.0 ** -23 * np.abs(first[0].real))
    h.set_offsets(None)
    assert same_values(h.feed(rows), first.astype(np.complex64))
    h.close()


@pytest.mark.parametrize("kind", KINDS)
def test_poison_stays_in_its_sample(resmap, kind):
    n_ch, n = 5, 50
    rng = np.random.default_rng(71)
    fits, tones, k = columns(resmap, n_ch, seed=72)
    rows = np.stack([noisy_stream(rng, fits[c], tones[c], n)[0] for c in range(n_ch)], axis=1)
    channels = [0, 1, 1, 4, 3]
    clean = twin(resmap, kind, k, rows, channels=channels)
    bad = rows.copy()
    bad[7, 1] = np.complex64(complex(np.inf, 0.0))
    bad[20, 4] = np.complex64(complex(0.0, np.nan))
    bad[31, 2] = np.complex64(complex(np.nan, np.nan))            # a column nobody maps
    got = twin(resmap, kind, k, bad, channels=channels)
    hit = np.zeros((n, n_ch), dtype=bool)
    hit[7, 1] = hit[7, 2] = hit[20, 3] = True
    finite = np.isfinite(got.real) & np.isfinite(got.imag)
    assert np.array_equal(~finite, hit)
    assert same_values(got[~hit], clean[~hit])
