"""sc16 input, the part that needs no GPU: gsdr_widen_sc16_host (and the Python wrapper over it) against numpy,
bit for bit.  The widening is an exact int16 -> float32 conversion followed by ONE IEEE float32 multiply, so
`np.float32(v) * np.float32(scale)` is the value, not an approximation of it."""
import ctypes as C

import numpy as np
import pytest

SCALES = [2.0 ** -15, 1.0 / 32767.0, 1.0]


def every_int16_pair():
    """65 536 samples: every int16 value once in the I position and once, permuted, in the Q position."""
    v = np.arange(-32768, 32768, dtype=np.int16)
    x = np.empty((v.size, 2), dtype=np.int16)
    x[:, 0] = v
    x[:, 1] = np.random.default_rng(16).permutation(v)
    return x


def widened(x16, scale):
    """The expected complex64: float32(v) * float32(scale), per component."""
    f = x16.astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(f).view(np.complex64).reshape(x16.shape[:-1])


def bits(z):
    return np.ascontiguousarray(z).view(np.uint32)


@pytest.mark.parametrize("scale", SCALES, ids=["2^-15", "1/32767", "1"])
def test_widen_host_every_value_bit_exact(gsdr_lib, scale):
    x = every_int16_pair()
    assert sorted(x[:, 1].tolist()) == list(range(-32768, 32768)) and not np.array_equal(x[:, 0], x[:, 1])
    out = np.full(x.shape[0], np.nan + 0j, dtype=np.complex64)
    gsdr_lib.gsdr_widen_sc16_host(x.ctypes.data, out.ctypes.data, x.shape[0], C.c_float(scale))
    np.testing.assert_array_equal(bits(out), bits(widened(x, scale)))
    # and through the package: a numpy array takes the host path
    import gpu_sdr_amd as g
    np.testing.assert_array_equal(bits(g.widen_sc16(x, scale=scale)), bits(widened(x, scale)))


def test_widen_host_default_scale_is_lossless(gsdr_lib):
    import gpu_sdr_amd as g
    x = every_int16_pair()
    y = g.widen_sc16(x)
    assert y.dtype == np.complex64 and y.shape == (65536,)
    back = np.ascontiguousarray(y).view(np.float32).reshape(-1, 2) * np.float32(32768.0)
    np.testing.assert_array_equal(back.astype(np.int16), x)


def test_widen_host_n0_writes_nothing(gsdr_lib):
    x = every_int16_pair()[:8].copy()
    out = np.full(8, 7 - 3j, dtype=np.complex64)
    gsdr_lib.gsdr_widen_sc16_host(x.ctypes.data, out.ctypes.data, 0, C.c_float(1.0))
    np.testing.assert_array_equal(out, np.full(8, 7 - 3j, dtype=np.complex64))
    gsdr_lib.gsdr_widen_sc16_host(None, None, 0, C.c_float(1.0))      # nothing is touched, not even the pointers


def test_widen_host_writes_n_samples_only(gsdr_lib):
    x = every_int16_pair()[1000:1007].copy()
    out = np.full(9, 7 - 3j, dtype=np.complex64)
    gsdr_lib.gsdr_widen_sc16_host(x.ctypes.data, out[1:].ctypes.data, 7, C.c_float(2.0 ** -15))
    assert out[0] == 7 - 3j and out[8] == 7 - 3j
    np.testing.assert_array_equal(bits(out[1:8]), bits(widened(x, 2.0 ** -15)))


def test_widen_wrapper_rejects_other_layouts(gsdr_lib):
    import gpu_sdr_amd as g
    with pytest.raises(TypeError):
        g.widen_sc16(np.zeros((4, 2), dtype=np.float32))
    with pytest.raises(TypeError):
        g.widen_sc16(np.zeros(8, dtype=np.int16))                    # no (..., 2) shape
    with pytest.raises(TypeError):
        g.widen_sc16(np.zeros((4, 4), dtype=np.int16)[:, :2])        # not contiguous
    with pytest.raises(ValueError):
        g.widen_sc16(np.zeros((4, 2), dtype=np.int16), out=np.zeros(3, dtype=np.complex64))
