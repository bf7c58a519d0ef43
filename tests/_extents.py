"""Guard zones around the buffers a test hands to a device entry of include/gsdr.h.

The entries take plain device pointers: `in_dev` holds buffer_len samples, `out_dev` has room for
gsdr_demod_out_capacity() samples, both need their natural alignment only.  A tensor of its own is aligned to
512 bytes and rounded up in size, so a kernel that strays a few samples past an end, or that needs 16-byte
alignment, passes every test that allocates its buffers one by one.  Here a buffer sits in the MIDDLE of one
larger allocation, G samples of guard on each side, 0 or 1 sample past a 16-byte boundary.  All guard memory is
the test's own: a stray access lands in it and is seen, nothing is placed beside unmapped memory.

Plain module, no GPU work at import time; every function takes numpy arrays (dev=None, the CPU test of this
helper) or torch tensors on `dev`.
"""
import numpy as np

G = 65_536                      # guard samples on each side of a buffer

# Bit patterns, one per float.  Both NaNs are quiet (bit 22 set) and differ in their payload, so a guard of the
# input that turned up in the output would be told from an output that was never written.
IN_NAN_BITS = 0x7FC1A5A5        # input guards, pattern "nan": shows 0 x guard (a zero-padded tap times an over-read)
OUT_SENTINEL_BITS = 0x7FD5C3C3  # outputs, guards and region alike, before the call
HUGE = 1e30                     # input guards, pattern "huge": +1e30, -1e30, ... finite, shows a max / scale
                                # reduction that reached into the guard (hardware max drops NaNs; 0 x huge hides itself)
PATTERNS = ("nan", "huge")


def _guard_floats(pattern, nfloat):
    if pattern == "nan":
        return np.full(nfloat, IN_NAN_BITS, dtype=np.uint32).view(np.float32)
    if pattern == "huge":
        g = np.full(nfloat, HUGE, dtype=np.float32)
        g[1::2] = -HUGE
        return g
    raise ValueError(f"pattern must be one of {PATTERNS}")


def _layout(x, off, pattern):
    """The host image of guarded_input(x, off, pattern): [G guard | off guard | x | 1 - off guard | G guard]."""
    if off not in (0, 1):
        raise ValueError("off must be 0 or 1")
    x = np.ascontiguousarray(x, dtype=np.complex64)
    n = x.size
    whole = _guard_floats(pattern, 2 * (2 * G + n + 1)).view(np.complex64).copy()
    whole[G + off:G + off + n] = x
    return whole


def _host(a):
    """numpy array of the same bits (a torch tensor is copied to the host)."""
    return a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()


def _addr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def _place(whole_host, off, n, dev):
    if dev is None:
        whole = whole_host
    else:
        import torch
        whole = torch.from_numpy(whole_host).to(dev)       # a plain copy: every bit, NaN payloads included
    view = whole[G + off:G + off + n]
    # (numpy aligns to 16 bytes or more, the device allocator to 512)
    assert _addr(whole) % 16 == 0 and _addr(view) % 16 == 8 * off, "the view must start `off` samples past 16 bytes"
    return whole, view


def guarded_input(x, off, pattern, dev):
    """(whole, view): `x` inside one complex64 allocation with G samples of `pattern` on each side; `view` holds
    x and starts `off` (0 or 1) samples past a 16-byte-aligned address."""
    return _place(_layout(x, off, pattern), off, np.asarray(x).size, dev)


def guarded_output(cap, off, dev):
    """(whole, view): a view of `cap` samples inside one complex64 allocation; every float of the allocation, the
    view included, is the sentinel NaN."""
    whole = np.full(2 * (2 * G + cap + 1), OUT_SENTINEL_BITS, dtype=np.uint32).view(np.complex64)
    return _place(whole, off, cap, dev)


def check_output(whole, view, n):
    """Both guard zones are still the sentinel, bit for bit; 0 <= n <= cap; every float of view[:n] was written
    (is finite).  view[n:cap] belongs to the callee (the ABI allows writes there) and is not looked at."""
    cap = int(view.shape[0])
    first = (_addr(view) - _addr(whole)) // 8
    assert 0 <= n <= cap, f"returned length {n} outside [0, {cap}]"
    bits = _host(whole).view(np.int32)
    sentinel = np.array(OUT_SENTINEL_BITS, dtype=np.uint32).view(np.int32)
    for name, zone, base in (("in front of", bits[:2 * first], 0), ("behind", bits[2 * (first + cap):], 2 * (first + cap))):
        bad = np.flatnonzero(zone != sentinel)
        assert bad.size == 0, (f"{bad.size} floats written {name} the output, the first {(base + bad[0] - 2 * first) / 2:g} "
                               f"samples from its start (capacity {cap})")
    got = bits[2 * first:2 * (first + n)].view(np.float32)
    bad = np.flatnonzero(~np.isfinite(got))
    assert bad.size == 0, f"{bad.size} floats of out[0, {n}) are not finite (not written?), the first at sample {bad[0] // 2}"


def check_input_untouched(whole, x, off, pattern):
    """The guards and the samples are bit for bit what guarded_input(x, off, pattern, .) put there."""
    bits = _host(whole).view(np.int32)
    want = _layout(x, off, pattern).view(np.int32)
    assert want.shape == bits.shape, "not a tensor of guarded_input for this x"
    bad = np.flatnonzero(bits != want)
    assert bad.size == 0, (f"the input allocation was modified: {bad.size} floats differ, the first "
                           f"{(bad[0] - 2 * (G + off)) / 2:g} samples from the start of the buffer")
