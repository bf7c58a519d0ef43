"""What the FIR decimator's tests share (include/gsdr.h, "FIR decimation on the device"): a float64 oracle of the output
law, inputs with fixed seeds, caller taps, the cuttings of a stream into feeds and the runners of the two objects.
Plain module, no GPU work at import time."""
import numpy as np

PARITY_BAR = 1e-5          # per channel, ||y - y_oracle||_2 / ||y_oracle||_2: the project's parity bar


def n_out(total, offset, q):
    """Output rows complete after `total` rows."""
    return 0 if total <= offset else (total - 1 - offset) // q + 1


def oracle(x, q, taps, offset):
    """y[o] = sum_t h[t] x[o q + p - (T-1) + t] in float64, on the float32 rows and the float32 taps; rows before the
    stream are zero.  [n_out][n_ch] complex128."""
    x = np.asarray(x)
    rows, n_ch = x.shape
    h = np.asarray(taps, dtype=np.float32).astype(np.float64)
    T = h.shape[0]
    xp = np.zeros((rows + T - 1, n_ch), dtype=np.complex128)
    xp[T - 1:] = x
    m = n_out(rows, offset, q)
    y = np.zeros((m, n_ch), dtype=np.complex128)
    for o in range(m):
        s = o * q + offset                       # x row o q + p - (T-1) sits at xp[o q + p]
        y[o] = h @ xp[s:s + T]
    return y


def rel_err(y, y_ref):
    """Per channel ||y - y_ref|| / ||y_ref||, the largest."""
    y, y_ref = np.asarray(y, dtype=np.complex128), np.asarray(y_ref, dtype=np.complex128)
    assert y.shape == y_ref.shape, (y.shape, y_ref.shape)
    num, den = np.linalg.norm(y - y_ref, axis=0), np.linalg.norm(y_ref, axis=0)
    assert np.all(den > 0)
    return float((num / den).max())


def carrier(rows, n_ch, seed=1):
    """0.3+0.4j per channel, scaled by channel, plus 1e-3 complex Gaussian noise."""
    rng = np.random.default_rng(seed)
    scale = 1.0 + np.arange(n_ch) / max(n_ch, 1)
    z = (0.3 + 0.4j) * scale[None, :] + 1e-3 * (rng.standard_normal((rows, n_ch)) + 1j * rng.standard_normal((rows, n_ch)))
    return z.astype(np.complex64)


def noise(rows, n_ch, seed=2):
    """Unit complex Gaussian."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, n_ch)) + 1j * rng.standard_normal((rows, n_ch))).astype(np.complex64)


INPUTS = {"carrier": carrier, "noise": noise}


def caller_taps(T, seed=3):
    """Asymmetric signed taps with one zero among them (none where T == 1)."""
    rng = np.random.default_rng(seed + T)
    h = (rng.standard_normal(T) / np.sqrt(T) + 0.5 / T).astype(np.float32)
    if T > 1:
        h[T // 3] = 0.0
    return h


def cuttings(total, q, max_rows=None):
    """name -> feed sizes that add up to `total`: one feed, feeds of 1, of 7 and of q - 1 rows, uneven feeds with empty
    ones among them, and feeds of max_rows (a third of the stream unless given)."""
    def chop(n):
        n = max(int(n), 1)
        return [min(n, total - at) for at in range(0, total, n)]
    uneven, at, k = [0], 0, 0
    steps = [3, 0, q + 1, 0, 0, 2 * q - 1, 1, 5 * q + 2, 0, q]
    while at < total:
        n = min(steps[k % len(steps)], total - at)
        uneven.append(n)
        at += n
        k += 1
    uneven.append(0)
    cuts = {"one": [total], "ones": chop(1), "sevens": chop(7), "q-1": chop(q - 1), "uneven": uneven,
            "max_rows": chop(max_rows if max_rows else total // 3 + 1)}
    assert all(sum(c) == total for c in cuts.values())
    return cuts


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.complex64), np.ascontiguousarray(b, dtype=np.complex64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_host(decimate, x, q, taps, offset, cut=None, max_rows=None):
    """The host twin over x cut as `cut` (one feed by default): the emitted rows concatenated, [n_out][n_ch] complex64."""
    rows, n_ch = x.shape
    cut = [rows] if cut is None else cut
    d = decimate.host_decimator(n_ch, max_rows or max(max(cut), 1), q, taps=taps, offset=offset)
    out, at, seen = [], 0, 0
    for n in cut:
        want = d.next_rows(n)
        y = d.feed(x[at:at + n])
        assert y.shape == (want, n_ch)
        out.append(y.copy())
        at += n
        seen += want
        assert d.rows_seen == at and d.rows_out == seen == n_out(at, d.offset, q)
    d.close()
    assert at == rows
    return np.concatenate(out) if out else np.zeros((0, n_ch), dtype=np.complex64)


def run_device(decimate, x, q, taps, offset, dev, cut=None, max_rows=None, stream=None):
    """The device object over x cut as `cut`, each feed's rows uploaded as a tensor of their own, the outputs written
    back to back into one tensor and downloaded at the end."""
    import torch
    rows, n_ch = x.shape
    cut = [rows] if cut is None else cut
    d = decimate.device_decimator(n_ch, max_rows or max(max(cut), 1), q, taps=taps, offset=offset, device_index=0)
    total_out = n_out(rows, d.offset, q)
    out = torch.zeros((max(total_out, 1), n_ch), dtype=torch.complex64, device=dev)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    torch.cuda.synchronize()                              # the upload is done before another stream reads it
    at, seen = 0, 0
    for n in cut:
        want = d.next_rows(n)
        m = d.feed_device(xd[at:at + n], out[seen:seen + want], stream=stream)
        assert m == want
        at += n
        seen += m
    assert at == rows and seen == total_out == d.rows_out
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    y = out[:total_out].cpu().numpy()
    d.close()
    return y
