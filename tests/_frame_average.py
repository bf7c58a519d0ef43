"""Shared by tests/test_frame_average_host.py and tests/test_gpu_frame_average.py: the numpy float32 model of the
frame averaging (the arithmetic of include/gsdr.h, operation for operation) and the inputs of the kernel cases."""
import numpy as np

# (n_frames, n_ch, k, count)
CASES = [(1, 1, 1, 0), (7, 3, 2, 1), (40, 64, 5, 3), (3, 1000, 8, 6), (2, 130, 16, 0), (257, 1230, 16, 15)]
KINDS = ("complex", "power")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.complex64).view(np.uint32)


def term(frames, kind):
    """t_j of the contract: the frame (complex) or (fl32(fl32(re*re) + fl32(im*im)), 0) (power)."""
    frames = np.asarray(frames, dtype=np.complex64)
    if kind == "complex":
        return frames
    re, im = frames.real.astype(np.float32), frames.imag.astype(np.float32)
    t = np.zeros(frames.shape, dtype=np.complex64)
    with np.errstate(all="ignore"):
        t.real = (re * re).astype(np.float32) + (im * im).astype(np.float32)
    return t


def model(frames, k, kind, count=0, acc=None):
    """-> (out [rows][n_ch], acc_out [n_ch], count_out); float32 operations only, one rounding each."""
    frames = np.asarray(frames, dtype=np.complex64)
    n_ch = frames.shape[1]
    t = term(frames, kind)
    inv = np.float32(1.0) / np.float32(k)
    re = acc.real.astype(np.float32).copy() if count else None
    im = acc.imag.astype(np.float32).copy() if count else None
    rows = []
    with np.errstate(all="ignore"):
        for f in range(frames.shape[0]):
            if count == 0:
                re, im = t[f].real.astype(np.float32).copy(), t[f].imag.astype(np.float32).copy()   # acc = t_0: keeps -0
            else:
                re, im = (re + t[f].real).astype(np.float32), (im + t[f].imag).astype(np.float32)
            count += 1
            if count == k:
                row = np.empty(n_ch, dtype=np.complex64)
                row.real, row.imag = re * inv, im * inv
                rows.append(row)
                count = 0
    acc_out = np.zeros(n_ch, dtype=np.complex64)
    if count:
        acc_out.real, acc_out.imag = re, im
    out = np.stack(rows) if rows else np.empty((0, n_ch), dtype=np.complex64)
    return out, acc_out, count


def case_input(n_frames, n_ch, k, count, seed=0):
    """Unit noise with -0, denormals and values whose squares round; frame `nan_f` is NaN, frame `inf_f` is +Inf
    (when the case has that many frames); the accumulator of the open group is the model's own sum of `count` frames.
    -> frames, acc (None when count == 0), nan_f, inf_f"""
    rng = np.random.default_rng(1000 * n_frames + 10 * k + count + seed)
    def noise(n):
        x = (rng.standard_normal((n, n_ch)) + 1j * rng.standard_normal((n, n_ch))).astype(np.complex64)
        x.real[rng.random((n, n_ch)) < 0.05] = -0.0
        x.imag[rng.random((n, n_ch)) < 0.05] = -0.0
        tiny = rng.random((n, n_ch)) < 0.03
        x[tiny] *= np.float32(1e-22)                 # squares are denormal
        x[rng.random((n, n_ch)) < 0.03] *= np.float32(1e15)
        return x
    frames = noise(n_frames)
    nan_f = 2 if n_frames > 4 else None
    inf_f = n_frames - 2 if n_frames > 30 else None
    if nan_f is not None:
        frames[nan_f] = np.complex64(complex(np.nan, np.nan))
    if inf_f is not None:
        frames[inf_f] = np.complex64(complex(np.inf, np.inf))
    acc = None
    if count:
        _, acc, c = model(noise(count), k, "complex", 0, None)
        assert c == count
    return frames, acc, nan_f, inf_f


def nonfinite_groups(n_frames, k, count, marked):
    """group slots (0 = the one open on entry) that hold one of the frames in `marked`"""
    return sorted({(count + f) // k for f in marked if f is not None})
