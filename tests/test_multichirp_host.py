"""Several chirps in one handle (GSDR_CREATE_MULTI_CHIRP, include/gsdr.h): everything that is decided before the first
HIP call -- the refusals of gsdr_demod_create_ex, gsdr_txgen_create_ex and gsdr_source_multichirp[_sc16], byte for
byte, and the headers as plain C / plain C++.  No GPU: no request below passes every check of its entry, so no
launcher and no device call is reached (on a machine without a GPU such a call would leave its own message)."""
import ctypes as C
import os
import subprocess

import pytest

from gpu_sdr_amd import _lib
from gpu_sdr_amd._lib import ChirpParamC
from test_entry_refusals import ALIGNED, CHIRP, DIRECT, OFF2, OFF4, PLANTED, TONES, last_error, make_param, plant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI = _lib.CREATE_MULTI_CHIRP
RX_MULTI = b"Multiple chirp RX buffer demodulation has been requested. This feature is not implemented yet."
TX_MULTI = b"Multiple chirp TX buffer generation has been requested. This feature is not implemented yet."
RX_MIXED = b"Mixed RX buffer demodulation has been requested. This feature is not implemented yet."
TX_MIXED = b"Mixed TX buffer generation has been requested. This feature is not implemented yet."
PER_CHIRP = b"CHIRP needs freq[] and chirp_f[] for every wave_type entry"
SHARED = b"multi-chirp needs one swipe_s and one chirp_t for all chirps"
TOO_MANY = b"multi-chirp takes at most GSDR_MULTI_CHIRP_MAX (16) chirps"


def chirps(n, **over):
    """wave_type = CHIRP x n with arrays that pass every check, then `over`."""
    kw = dict(wave_type=[CHIRP] * n, freq=tuple(10 * c for c in range(n)), chirp_f=tuple(100 + c for c in range(n)),
              swipe_s=(10,), chirp_t=(0.01,))
    kw.update(over)
    return kw


def rx_create(lib, flags, **kw):
    p, keep = make_param(**kw)
    plant(lib)
    h = lib.gsdr_demod_create_ex(C.byref(p), flags)
    del keep
    return h, last_error(lib)


def tx_create(lib, flags, **kw):
    p, keep = make_param(**kw)
    plant(lib)
    h = lib.gsdr_txgen_create_ex(C.byref(p), None, 0, flags)
    del keep
    return h, last_error(lib)


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "gsdr.h")).read()
    assert "#define GSDR_CREATE_MULTI_CHIRP 1u" in text and "#define GSDR_MULTI_CHIRP_MAX 16" in text
    assert (_lib.CREATE_MULTI_CHIRP, _lib.MULTI_CHIRP_MAX) == (1, 16)


def test_flags_zero_is_the_plain_entry(gsdr_lib):
    """Two chirps without the flag: the reference's refusal, the bytes gsdr_demod_create / gsdr_txgen_create leave."""
    lib = gsdr_lib
    p, keep = make_param(**chirps(2))
    plant(lib)
    assert lib.gsdr_demod_create(C.byref(p)) is None
    plain_rx = last_error(lib)
    plant(lib)
    assert lib.gsdr_txgen_create(C.byref(p), None, 0) is None
    plain_tx = last_error(lib)
    del keep
    assert rx_create(lib, 0, **chirps(2)) == (None, plain_rx) and plain_rx == RX_MULTI
    assert tx_create(lib, 0, **chirps(2)) == (None, plain_tx) and plain_tx == TX_MULTI
    # and the other refusals of the plain entries, in their order
    assert rx_create(lib, 0, wave_type=[CHIRP, TONES, CHIRP], buffer_len=0, freq=(1, 2, 3)) == (None, RX_MULTI)
    assert rx_create(lib, 0, wave_type=[TONES, DIRECT], freq=(10, 20)) == (None, RX_MIXED)
    assert rx_create(lib, 0, wave_type=[DIRECT], freq=(10,), buffer_len=0) == (None, b"buffer_len must be positive")
    assert tx_create(lib, 0, wave_type=[TONES], buffer_len=0) == (None, b"buffer_len must be positive")
    assert lib.gsdr_demod_create_ex(None, 0) is None and last_error(lib) == b"null parameters"
    assert lib.gsdr_txgen_create_ex(None, None, 0, 0) is None and last_error(lib) == b"null parameters"


@pytest.mark.parametrize("flags", [2, 3, 0x80000000, 0xFFFFFFFE])
def test_unknown_flag_bit_is_refused_first(gsdr_lib, flags):
    lib = gsdr_lib
    for kw in (chirps(2), chirps(1), dict(wave_type=[DIRECT], freq=(10,), buffer_len=0)):
        assert rx_create(lib, flags, **kw) == (None, b"unknown creation flag")
        assert tx_create(lib, flags, **kw) == (None, b"unknown creation flag")
    plant(lib)
    assert lib.gsdr_demod_create_ex(None, flags) is None and last_error(lib) == b"unknown creation flag"
    plant(lib)
    assert lib.gsdr_txgen_create_ex(None, None, 0, flags) is None and last_error(lib) == b"unknown creation flag"


MULTI_REFUSALS = [
    ("seventeen_chirps", chirps(17), TOO_MANY),
    ("unequal_swipe_s", chirps(3, swipe_s=(10, 10, 11)), SHARED),
    ("unequal_chirp_t", chirps(3, chirp_t=(0.01, 0.02, 0.01)), SHARED),
    ("two_swipe_s_for_three_chirps", chirps(3, swipe_s=(10, 10)), SHARED),
    ("two_chirp_t_for_three_chirps", chirps(3, chirp_t=(0.01, 0.01)), SHARED),
    ("freq_short", chirps(3, freq=(10, 20)), PER_CHIRP),
    ("chirp_f_short", chirps(3, chirp_f=(100, 200)), PER_CHIRP),
    ("one_freq_for_sixteen", chirps(16, freq=(10,)), PER_CHIRP),
]


@pytest.mark.parametrize("kwargs,msg", [c[1:] for c in MULTI_REFUSALS], ids=[c[0] for c in MULTI_REFUSALS])
def test_multi_chirp_create_refusals(gsdr_lib, kwargs, msg):
    """With the flag set: each comes back before the device is chosen (device_index 0 would otherwise be asked for)."""
    assert rx_create(gsdr_lib, MULTI, **kwargs) == (None, msg)
    assert tx_create(gsdr_lib, MULTI, **kwargs) == (None, msg)


def test_mixed_types_stay_refused_with_the_flag(gsdr_lib):
    lib = gsdr_lib
    for wt in ([CHIRP, TONES, CHIRP], [CHIRP, CHIRP, DIRECT], [TONES, CHIRP]):
        kw = chirps(len(wt), wave_type=wt)
        assert rx_create(lib, MULTI, **kw) == (None, RX_MIXED)
        assert tx_create(lib, MULTI, **kw) == (None, TX_MIXED)
    # the order of the older checks stands: mixed before the length, the length before the multi-chirp checks
    assert rx_create(lib, MULTI, **chirps(3, wave_type=[CHIRP, TONES, CHIRP], buffer_len=0)) == (None, RX_MIXED)
    assert rx_create(lib, MULTI, **chirps(17, buffer_len=0)) == (None, b"buffer_len must be positive")
    assert tx_create(lib, MULTI, **chirps(17, buffer_len=0)) == (None, b"buffer_len must be positive")


def cps(n, num_steps=10, length=35):
    arr = (ChirpParamC * n)()
    for c in range(n):
        arr[c].num_steps, arr[c].length, arr[c].chirpness, arr[c].f0 = num_steps, length, 1000 + c, c
    return arr


def test_source_multichirp_refusals(gsdr_lib):
    lib = gsdr_lib
    one = (C.c_float * 17)(*([1.0] * 17))

    def c64(out, n, cp, scale, k):
        plant(lib)
        return lib.gsdr_source_multichirp(out, n, 0, cp, scale, k, None), last_error(lib)

    def sc16(out, n, cp, scale, k, gain=32767.0, clipped=None):
        plant(lib)
        return lib.gsdr_source_multichirp_sc16(out, n, 0, cp, scale, k, gain, clipped, None), last_error(lib)

    # n == 0 touches nothing, not even the pointers
    assert c64(None, 0, None, None, 0) == (0, PLANTED)
    assert sc16(None, 0, None, None, 99, gain=0.0, clipped=OFF4) == (0, PLANTED)
    for call, sfx, out in ((c64, b"", ALIGNED), (sc16, b"_sc16", ALIGNED)):
        pre = b"gsdr_source_multichirp" + sfx + b": "
        assert call(None, 4, cps(2), one, 2) == (-1, pre + b"bad arguments")
        assert call(out, 4, None, one, 2) == (-1, pre + b"bad arguments")
        assert call(out, 4, cps(2), None, 2) == (-1, pre + b"bad arguments")
        assert call(out, -1, cps(2), one, 2) == (-1, pre + b"bad arguments")
        for k in (0, -1, 17):
            assert call(out, 4, cps(17), one, k) == (-1, pre + b"n_chirps must be in [1, GSDR_MULTI_CHIRP_MAX]")
        bad = cps(3)
        bad[2].length = 36
        assert call(out, 4, bad, one, 3) == (-1, pre + b"the chirps must share num_steps and length")
        bad = cps(3)
        bad[1].num_steps = 11
        assert call(out, 4, bad, one, 3) == (-1, pre + b"the chirps must share num_steps and length")
        assert call(out, 4, cps(2, num_steps=0), one, 2) == (-1, pre + b"chirp period overflows")
        assert call(out, 4, cps(2, num_steps=1 << 62, length=4), one, 2) == (-1, pre + b"chirp period overflows")
    # the sc16 form then checks the gain and the alignment, like gsdr_source_chirp_sc16
    pre = b"gsdr_source_multichirp_sc16: "
    for gain in (0.0, -1.0, float("nan"), float("inf")):
        assert sc16(OFF2, 4, cps(2), one, 2, gain=gain) == (-1, pre + b"the gain must be finite and > 0")
    assert sc16(OFF2, 4, cps(2), one, 2) == (-1, pre + b"out_dev must be 4-byte, clipped_dev 8-byte aligned")
    assert sc16(ALIGNED, 4, cps(2), one, 2, clipped=OFF4) == (-1, pre + b"out_dev must be 4-byte, clipped_dev 8-byte aligned")


def test_headers_compile_as_plain_c_and_cxx(tmp_path):
    """gsdr.h with the new entries is still C99; the C++ drop-in classes take the flags as a trailing argument."""
    inc = os.path.join(ROOT, "include")
    c_src = tmp_path / "multi.c"
    c_src.write_text('#include "gsdr.h"\n'
                     "gsdr_demod *rx(const gsdr_param_c *p) { return gsdr_demod_create_ex(p, GSDR_CREATE_MULTI_CHIRP); }\n"
                     "gsdr_txgen *tx(const gsdr_param_c *p, const float *a) { return gsdr_txgen_create_ex(p, a, GSDR_MULTI_CHIRP_MAX, 0u); }\n"
                     "int src(gsdr_c64 *o, const gsdr_chirp_param *cp, const float *s) { return gsdr_source_multichirp(o, 4, 0, cp, s, 2, 0); }\n"
                     "int src16(gsdr_sc16 *o, const gsdr_chirp_param *cp, const float *s) {\n"
                     "    return gsdr_source_multichirp_sc16(o, 4, 0, cp, s, 2, 32767.0f, 0, 0); }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(c_src)])
    cxx = tmp_path / "multi.cpp"
    cxx.write_text('#include "USRP_demodulator.hpp"\n#include "USRP_buffer_generator.hpp"\n'
                   "RX_buffer_demodulator *rx(param *p) { return new RX_buffer_demodulator(p, false, GSDR_CREATE_MULTI_CHIRP); }\n"
                   "RX_buffer_demodulator *rx_plain(param *p) { return new RX_buffer_demodulator(p); }\n"
                   "TX_buffer_generator *tx(param *p) { return new TX_buffer_generator(p, GSDR_CREATE_MULTI_CHIRP); }\n"
                   "TX_buffer_generator *tx_plain(param *p) { return new TX_buffer_generator(p); }\n")
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", inc, str(cxx)])


def test_python_interfaces_take_multi_chirp():
    import inspect
    import gpu_sdr_amd as g
    from gpu_sdr_amd import generator, source
    assert inspect.signature(g.RX_buffer_demodulator.__init__).parameters["multi_chirp"].default is False
    assert inspect.signature(generator.TX_buffer_generator.__init__).parameters["multi_chirp"].default is False
    assert list(inspect.signature(source.device_chirps).parameters) == ["out", "last_index", "cps", "scales", "stream"]
