"""What the FIR decimator's tests share (include/gsdr.h, "FIR decimation on the device"): a float64 oracle of the output
law, a bit model of its arithmetic (fma32, contract_bits), the run shapes of the kernels, inputs with fixed seeds,
caller taps, value cases, the cuttings of a stream into feeds and the runners of the two objects.
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


def fma32(a, b, c):
    """float32(a * b + c), rounded once: the IEEE single-precision fused multiply-add, element by element.
    The product of two float32 is exact in float64 (48 bits).  Its sum with c is not: TwoSum gives the exact error of
    the float64 addition, and where that is not zero the sum is moved to the neighbour with an odd last bit (rounding
    to odd), which the one rounding to float32 that follows cannot tell from the exact sum (53 >= 2 * 24 + 2 bits, the
    subnormal float32 included: they keep fewer bits).  float32(float64(a) * b + c) rounds twice and is wrong on ties."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) != 0
        nudge = np.isfinite(s) & (e != 0) & ~odd
        s = np.where(nudge, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def contract_bits(x, q, taps, offset):
    """The paragraph "Arithmetic" of include/gsdr.h, literally: a loop over outputs, chunks and taps, no ring and no
    state, vectorised over the channels only (real and imaginary parts are 2 n_ch float32 lanes).  F = ceil(T / q);
    chunk j is the taps max(0, T - (j+1) q) <= t < T - j q; a chunk sum starts at +0 and takes its taps in ascending t,
    acc = fma(h[t], x, acc), rows before the stream skipped; the output is (((P_{F-1} + P_{F-2}) + ...) + P_0) in
    float32 additions.  [n_out][n_ch] complex64."""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    rows, n_ch = x.shape
    xf = x.view(np.float32)                                  # [rows][2 n_ch]
    h = np.asarray(taps, dtype=np.float32)
    T = h.shape[0]
    F = (T + q - 1) // q
    m = n_out(rows, offset, q)
    y = np.zeros((m, 2 * n_ch), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for o in range(m):
            first = o * q + offset - (T - 1)                 # the stream row under tap 0
            s = None
            for j in range(F - 1, -1, -1):                   # oldest chunk first
                acc = np.zeros(2 * n_ch, dtype=np.float32)
                for t in range(max(0, T - (j + 1) * q), T - j * q):
                    if first + t >= 0:
                        acc = fma32(h[t], xf[first + t], acc)
                s = acc if s is None else (s + acc).astype(np.float32)
            y[o] = s
    return y.view(np.complex64)


# ---- the run shapes of decim_kernels.hip: every F = ceil(T / q) at which decim_partial_kernel changes its chunks per
# thread or clamps its last group (1 | 2, 3 | 4, 7, 8, 14, 15, 21, 22, 63, 64), every F at which decim_combine_kernel's
# turns of eight and its tail change (8 | 9, 10 | 16, 17), and the factors around the 8 rows a thread has in flight
RUN_F = (1, 2, 3, 4, 7, 8, 9, 10, 14, 15, 16, 17, 21, 22, 63, 64)
RUN_Q = (1, 3, 8, 9, 17)
RUN_N_CH = (1, 3, 64, 65, 255, 257)


def run_tap_counts(F, q):
    """T with ceil(T / q) == F: pad = F q - T of 0, of q - 1 and in between; for F == 1 also one T < q."""
    Ts = [F * q, (F - 1) * q + 1, (F - 1) * q + 1 + q // 2]
    if F == 1 and q > 2:
        Ts.append(q - 2)
    Ts = sorted({T for T in Ts if T >= 1})
    assert all((T + q - 1) // q == F for T in Ts)
    return Ts


def run_modelled(F, q):
    """Where contract_bits is affordable (one fma32 call per output and tap): every F for q in {1, 3}, F <= 22 else."""
    return q in (1, 3) or F <= 22


def run_shapes(q):
    """The device cases of one q: (name, n_ch, q, T, offset, rows).  n_ch and the offset cycle over the whole grid
    (all q), so every F meets few and many channels."""
    shapes, i = [], 0
    for qq in RUN_Q:
        for F in RUN_F:
            for T in run_tap_counts(F, qq):
                n_ch = RUN_N_CH[i % 6]
                offset = (0, qq - 1, (T - 1) // 2, T + 5)[(i // 6 + i) % 4]
                if qq == q:
                    shapes.append((f"F{F}_q{qq}_T{T}_p{offset}_c{n_ch}", n_ch, qq, T, offset, offset + (F + 12) * qq + 3))
                i += 1
    return shapes


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


def same_values(a, b):
    """same_bits, but a NaN matches any NaN: componentwise the class (finite, +Inf, -Inf, NaN) is the same and
    everything that is not a NaN has the same bits.  The bits of a NaN that an Inf - Inf generates are not compared: x86
    and the GPU give their default NaN different signs, and the contract fixes neither."""
    a = np.ascontiguousarray(a, dtype=np.complex64).view(np.float32)
    b = np.ascontiguousarray(b, dtype=np.complex64).view(np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return np.array_equal(a.view(np.uint32)[keep], b.view(np.uint32)[keep])


VALUE_KINDS = ("subnormal", "minus_zero", "overflow")


def values_case(kind):
    """(x, taps, q, offset) of a value case: n_ch = 3, q = 5, T = 33 (F = 7, pad 2), 120 rows, offset 16.
    subnormal: rows of about 1e-30 and taps of about 1e-9: every product and sum is subnormal or zero.
    minus_zero: every row -0 - 0j.
    overflow: rows 40 .. 79 of channel 1 are +-3e38 in both parts and the taps are four times the usual: chunk sums
    reach +Inf and -Inf and the combine adds them to NaN; the rest is noise."""
    q, T, offset, rows = 5, 33, 16, 120
    h = caller_taps(T)
    if kind == "subnormal":
        return (noise(rows, 3, seed=81) * np.float32(1e-30)).astype(np.complex64), (h * np.float32(1e-9)).astype(np.float32), q, offset
    if kind == "minus_zero":
        x = np.zeros((rows, 3), dtype=np.complex64)
        x.view(np.float32)[:] = np.float32(-0.0)
        return x, h, q, offset
    assert kind == "overflow"
    rng = np.random.default_rng(82)
    x = noise(rows, 3, seed=83)
    x.view(np.float32)[40:80, 2:4] = (np.float32(3e38) * rng.choice([-1.0, 1.0], size=(40, 2))).astype(np.float32)
    return x, (h * np.float32(4)).astype(np.float32), q, offset


def check_values_model(kind, y):
    """That the model's output of a value case holds what the case is there for."""
    f = np.ascontiguousarray(y, dtype=np.complex64).view(np.float32)
    if kind == "subnormal":
        small = (f != 0) & (np.abs(f) < np.finfo(np.float32).tiny)
        assert small.mean() >= 0.5 and np.all(np.abs(f) < np.finfo(np.float32).tiny), small.mean()
    elif kind == "minus_zero":
        assert f.size > 0 and not f.view(np.uint32).any()                # +0, every bit
    else:
        hot, rest = f[:, 2:4], np.delete(f, [2, 3], axis=1)
        assert np.all(np.isfinite(rest))
        counts = [np.isfinite(hot).sum(), (hot == np.inf).sum(), (hot == -np.inf).sum(), np.isnan(hot).sum()]
        assert min(counts) >= 3, counts


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
