"""The guard-zone helper of tests/_extents.py, checked on the CPU with numpy standing in for the device: a checker
that cannot fail would make every test of tests/test_gpu_extents.py vacuous."""
import numpy as np
import pytest

import _extents as E


def _x(n=37):
    rng = np.random.default_rng(n)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _floats(a):
    return a.view(np.float32)


@pytest.mark.parametrize("pattern", E.PATTERNS)
@pytest.mark.parametrize("off", [0, 1])
def test_layout(off, pattern):
    x = _x()
    whole, view = E.guarded_input(x, off, pattern, None)
    assert whole.dtype == np.complex64 and view.base is not None and np.shares_memory(whole, view)
    assert view.ctypes.data % 16 == 8 * off and view.ctypes.data - whole.ctypes.data == 8 * (E.G + off)
    np.testing.assert_array_equal(view.view(np.int32), x.view(np.int32))
    front, back = _floats(whole[:E.G + off]), _floats(whole[E.G + off + x.size:])
    assert back.size >= 2 * E.G
    for g in (front, back):
        if pattern == "nan":
            assert (g.view(np.uint32) == E.IN_NAN_BITS).all() and np.isnan(g).all()
        else:
            assert np.isfinite(g).all() and (np.abs(g) == np.float32(E.HUGE)).all()
            assert (np.sign(g[:-1]) == -np.sign(g[1:])).all()          # alternating signs
    out, oview = E.guarded_output(101, off, None)
    assert oview.shape == (101,) and oview.ctypes.data % 16 == 8 * off
    assert (out.view(np.uint32) == E.OUT_SENTINEL_BITS).all() and np.isnan(_floats(out)).all()
    assert E.OUT_SENTINEL_BITS != E.IN_NAN_BITS
    # quiet NaNs: the hardware leaves their payload alone when it copies them
    assert E.OUT_SENTINEL_BITS & 0x7FC00000 == 0x7FC00000 and E.IN_NAN_BITS & 0x7FC00000 == 0x7FC00000


@pytest.mark.parametrize("pattern", E.PATTERNS)
@pytest.mark.parametrize("off", [0, 1])
def test_clean_run_passes(off, pattern):
    x = _x()
    whole, view = E.guarded_input(x, off, pattern, None)
    out, oview = E.guarded_output(50, off, None)
    oview[:31] = 1.5 - 2j                       # the callee wrote 31 samples ...
    oview[40:44] = 7.0                          # ... and scribbled inside its capacity, which the ABI allows
    E.check_output(out, oview, 31)
    E.check_output(out, oview, 0)
    E.check_input_untouched(whole, x, off, pattern)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("where", ["just in front", "far in front", "just behind", "far behind"])
def test_one_float_in_an_output_guard_is_seen(off, where):
    cap = 50
    out, oview = E.guarded_output(cap, off, None)
    oview[:] = 1.0
    first = E.G + off
    k = {"just in front": 2 * first - 1, "far in front": 0, "just behind": 2 * (first + cap),
         "far behind": _floats(out).size - 1}[where]
    _floats(out)[k] = 0.0
    with pytest.raises(AssertionError, match="in front of" if "front" in where else "behind"):
        E.check_output(out, oview, cap)
    # a write of the sentinel's own NaN with another payload is a write too (compared as integers)
    out, oview = E.guarded_output(cap, off, None)
    oview[:] = 1.0
    out.view(np.uint32)[k] = E.OUT_SENTINEL_BITS ^ 1
    with pytest.raises(AssertionError):
        E.check_output(out, oview, cap)


@pytest.mark.parametrize("pattern", E.PATTERNS)
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("where", ["just in front", "far in front", "just behind", "far behind", "a sample"])
def test_one_float_of_the_input_allocation_is_seen(off, pattern, where):
    x = _x()
    whole, view = E.guarded_input(x, off, pattern, None)
    first = E.G + off
    k = {"just in front": 2 * first - 1, "far in front": 0, "just behind": 2 * (first + x.size),
         "far behind": _floats(whole).size - 1, "a sample": 2 * first + 5}[where]
    whole.view(np.uint32)[k] ^= 1               # one bit: a NaN stays a NaN, 1e30 stays about 1e30
    with pytest.raises(AssertionError, match="modified"):
        E.check_input_untouched(whole, x, off, pattern)


def test_unwritten_output_and_bad_lengths_are_seen():
    out, oview = E.guarded_output(50, 1, None)
    oview[:30] = 2.0
    _floats(oview)[2 * 17 + 1] = _floats(out)[0]        # one float of sample 17 still holds the sentinel
    with pytest.raises(AssertionError, match="not finite"):
        E.check_output(out, oview, 30)
    E.check_output(out, oview, 17)
    for n in (-1, 51):
        with pytest.raises(AssertionError, match="outside"):
            E.check_output(out, oview, n)
    # an input guard that was copied into the output is not "written" either
    oview[:30] = 2.0
    _floats(oview)[3] = np.array(E.IN_NAN_BITS, dtype=np.uint32).view(np.float32)
    with pytest.raises(AssertionError, match="not finite"):
        E.check_output(out, oview, 30)


def test_wrong_arguments():
    with pytest.raises(ValueError):
        E.guarded_input(_x(), 2, "nan", None)
    with pytest.raises(ValueError):
        E.guarded_input(_x(), 0, "zeros", None)
