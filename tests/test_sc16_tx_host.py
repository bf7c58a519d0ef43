"""sc16 output, the part that needs no GPU: gsdr_narrow_sc16_host (and the Python wrapper over it) against the numpy
model of include/gsdr.h, bit for bit, with the clipped count.  Per component: v = float32(c * gain), r = rint(v) (ties
to even), saturated to [-32768, 32767], NaN -> 0; clipped when v is NaN or r leaves the range."""
import ctypes as C

import numpy as np
import pytest


def narrow_model(x, gain):
    """(int16 array of shape (n, 2), number of clipped components) of a complex64 array, by the contract."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.ascontiguousarray(x, dtype=np.complex64).view(np.float32) * np.float32(gain)
        assert v.dtype == np.float32
        r = np.rint(v)
        nan = np.isnan(v)
        clipped = int(np.count_nonzero(nan | (r > 32767) | (r < -32768)))
        q = np.where(nan, np.float32(0), np.clip(r, -32768, 32767)).astype(np.int16)
    return q.reshape(-1, 2), clipped


def all_values():
    """Every int16 value k and k +- 0.25, 0.5, 0.75 (all exact in float32: every tie and both saturation edges), plus
    +-0, denormals, +-1e10, +-Inf and NaN -- each once in the I and once, permuted, in the Q position."""
    k = np.arange(-32768, 32768, dtype=np.float32)
    parts = [k] + [k + np.float32(d) for d in (-0.75, -0.5, -0.25, 0.25, 0.5, 0.75)]
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1e10, -1e10, np.inf, -np.inf, np.nan,
                        32767.5, -32768.5, -32768.75, 32767.49, -32768.0, 32767.0], dtype=np.float32)
    v = np.concatenate(parts + [special])
    for d, part in zip((-0.75, -0.5, -0.25, 0.25, 0.5, 0.75), parts[1:]):
        assert np.array_equal(part.astype(np.float64), k.astype(np.float64) + d)          # exact in float32
    x = np.empty((v.size, 2), dtype=np.float32)
    x[:, 0] = v
    x[:, 1] = np.random.default_rng(16).permutation(v)
    return np.ascontiguousarray(x).view(np.complex64).reshape(-1)


def host_narrow(lib, x, gain):
    out = np.full((x.size, 2), 12345, dtype=np.int16)
    n = lib.gsdr_narrow_sc16_host(x.ctypes.data, out.ctypes.data, x.size, C.c_float(gain))
    return out, int(n)


def test_model_edges():
    """The model itself on the edges the contract names."""
    x = np.array([32767.5 + 0j, -32768.5 + 0j, -32768.75 + 0j, 0.5 + 1.5j, 2.5 - 0.5j, np.nan + 0j, complex(np.inf, -np.inf)],
                 dtype=np.complex64)
    q, c = narrow_model(x, 1.0)
    assert q.tolist() == [[32767, 0], [-32768, 0], [-32768, 0], [0, 2], [2, 0], [0, 0], [32767, -32768]]
    assert c == 1 + 0 + 1 + 0 + 0 + 1 + 2


def test_narrow_host_every_value_bit_exact(gsdr_lib):
    x = all_values()
    want, want_clipped = narrow_model(x, 1.0)
    got, clipped = host_narrow(gsdr_lib, x, 1.0)
    np.testing.assert_array_equal(got, want)
    assert clipped == want_clipped and clipped > 0
    # and through the package: a numpy array takes the host path
    import gpu_sdr_amd as g
    out, count = g.narrow_sc16(x, gain=1.0, return_clipped=True)
    assert out.dtype == np.int16 and out.shape == (x.size, 2)
    np.testing.assert_array_equal(out, want)
    assert count == want_clipped
    np.testing.assert_array_equal(g.narrow_sc16(x, gain=1.0), want)


@pytest.mark.parametrize("gain", [32767.0, 32768.0, 1.0 / 3.0], ids=["32767", "32768", "1/3"])
def test_narrow_host_gaussian_bit_exact(gsdr_lib, gain):
    rng = np.random.default_rng(5)
    # sigma 0.5 at full-scale gains clips a few per cent; at gain 1/3 the values are spread over the whole int16 range
    sigma = 0.5 if gain > 1 else 60000.0
    x = (rng.standard_normal(20000) * sigma + 1j * rng.standard_normal(20000) * sigma).astype(np.complex64)
    want, want_clipped = narrow_model(x, gain)
    got, clipped = host_narrow(gsdr_lib, x, gain)
    np.testing.assert_array_equal(got, want)
    assert clipped == want_clipped and clipped > 0
    assert np.unique(got).size > 1000


def test_narrow_host_n0_touches_nothing(gsdr_lib):
    x = all_values()[:8].copy()
    out = np.full((8, 2), 77, dtype=np.int16)
    assert gsdr_lib.gsdr_narrow_sc16_host(x.ctypes.data, out.ctypes.data, 0, C.c_float(1.0)) == 0
    assert (out == 77).all()
    assert gsdr_lib.gsdr_narrow_sc16_host(None, None, 0, C.c_float(1.0)) == 0      # not even the pointers


def test_narrow_host_writes_n_samples_only(gsdr_lib):
    x = all_values()[40000:40007].copy()
    out = np.full((9, 2), 77, dtype=np.int16)
    gsdr_lib.gsdr_narrow_sc16_host(x.ctypes.data, out[1:].ctypes.data, 7, C.c_float(1.0))      # offset by one sample
    assert (out[0] == 77).all() and (out[8] == 77).all()
    np.testing.assert_array_equal(out[1:8], narrow_model(x, 1.0)[0])


def test_narrow_wrapper_refuses_bad_gain_and_layouts(gsdr_lib):
    import gpu_sdr_amd as g
    x = np.zeros(4, dtype=np.complex64)
    for gain in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            g.narrow_sc16(x, gain=gain)
    with pytest.raises(TypeError):
        g.narrow_sc16(np.zeros(4, dtype=np.complex128))
    with pytest.raises(TypeError):
        g.narrow_sc16(np.zeros(8, dtype=np.complex64)[::2])                  # not contiguous
    with pytest.raises(TypeError):
        g.narrow_sc16(x, out=np.zeros(8, dtype=np.int16))                    # no (..., 2) shape
    with pytest.raises(ValueError):
        g.narrow_sc16(x, out=np.zeros((3, 2), dtype=np.int16))


def test_round_trip_is_the_identity(gsdr_lib):
    """widen(narrow(x)) == x at gain 32768 / scale 2^-15 for every int16 pair, and narrow(widen(q)) == q."""
    import gpu_sdr_amd as g
    v = np.arange(-32768, 32768, dtype=np.int16)
    q = np.empty((v.size, 2), dtype=np.int16)
    q[:, 0] = v
    q[:, 1] = np.random.default_rng(16).permutation(v)
    x = g.widen_sc16(q, scale=2.0 ** -15)
    back, count = g.narrow_sc16(x, gain=32768.0, return_clipped=True)
    np.testing.assert_array_equal(back, q)
    assert count == 0
    again = g.widen_sc16(back, scale=2.0 ** -15)
    np.testing.assert_array_equal(again.view(np.uint32), x.view(np.uint32))
