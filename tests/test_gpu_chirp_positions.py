"""The RX chirp kernels away from the start of a sweep, at period wraps, and in every lock-in form (plain, split + sum,
generic; single- and multi-chirp), on the GPU against the CPU oracle.

Every other CHIRP test starts a handle at stream index 0 and feeds it a handful of buffers.  Here a handle walks through
a stream (tests/_chirp.py: one device buffer fed on every call) to where the kernels' 32-bit arithmetic wraps
(q(fi) = fi (fi + 1) / 2 passes 2^32 at step 92 682), to the end of the sweep and over its wrap, past chirp index 2^32 on
the 64-bit kernels; and tiny shapes sit on every edge of the rule that picks the lock-in form (csrc/chirp_plan.h).
Which form ran is asserted from describe()["chirp_calls"] in every test.

Bar: per chirp ||y - y_ref||_2 / ||y_ref||_2 <= TOL of tests/test_gpu_parity.py, the norm over all compared rows of a
handle together (at least 8); every returned length exactly.  Worst errors and loop times of a run go to
profiles/chirp_positions_margins.json.
"""
import ctypes as C

import numpy as np
import pytest

import _chirp as ch
import _extents as ex
from test_gpu_multichirp import spans
from test_gpu_parity import TOL, crandn, rel_err_per_tone

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------
# a. late positions at the smallest size: 100 000 steps of 3 samples
# ---------------------------------------------------------------------------
RATE_A = 1_000_000


def law_a(oracle_mod):
    # q(fi) passes 2^32 at fi = 92 682: sample 278 046 of the 300 000 of a sweep
    return ch.Law(oracle_mod, RATE_A, 100_000, 0.35, spans(RATE_A, 5), length=3, period=300_000)


def test_late_positions_undecimated(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """Five buffers of 77 777 samples: the sweep's end and its wrap fall inside the fourth.  Every sample."""
    ch.clean_env(monkeypatch, {})
    law, L, calls = law_a(oracle_mod), 77_777, 5
    assert 3 * L < 278_046 < law.period < 4 * L
    x = crandn(np.random.default_rng(101), L)
    feeds = [ch.Feed("single", law.handle(0, L, cols=[0]), law, 0, L, cols=[0]), ch.Feed("five", law.handle(0, L), law, 0, L)]
    assert [f.dem.kernel_name for f in feeds] == ["chirp_demod_kernel", "chirp_multi_demod_kernel"]
    errs, sec = ch.walk(cuda_device, oracle_mod, ch.Reference(oracle_mod, law, x), feeds, x, calls, set(range(calls)))
    for f in feeds:
        ch.expect_calls(f.dem, parts=1, plain=calls)
        f.dem.close()
    ch.check("late_positions_undecimated", errs, sec, calls)


@pytest.mark.parametrize("decim,L,calls,form,parts", [(2, 77_777, 5, "plain", 1), (7, 77_777, 5, "plain", 1),
                                                      (17, 25_000, 14, "split", 4)],
                         ids=["decim2", "decim7_point_over_the_wrap", "decim17_split"])
def test_late_positions_lockin(cuda_device, gsdr_lib, oracle_mod, monkeypatch, decim, L, calls, form, parts):
    """Lock-in through the end of the sweep on a single-chirp and a five-chirp handle.  100 000 steps are no multiple of
    7 or 17, so a point lies over the wrap: fi goes from the last step to step 0 inside it.  decim 17 at L = 25 000:
    490 or 491 points of 17 stretches per call, dealt to four waves in parts of 5, 5, 5, 2."""
    ch.clean_env(monkeypatch, {})
    law = law_a(oracle_mod)
    assert calls * L > law.period + L and (law.steps % decim != 0 or decim == 2)
    x = crandn(np.random.default_rng(102 + decim), L)
    feeds = [ch.Feed("single", law.handle(decim, L, cols=[0]), law, decim, L, cols=[0]),
             ch.Feed("five", law.handle(decim, L), law, decim, L)]
    assert [f.dem.kernel_name for f in feeds] == ["chirp_lockin_kernel", "chirp_multi_lockin_kernel"]
    errs, sec = ch.walk(cuda_device, oracle_mod, ch.Reference(oracle_mod, law, x), feeds, x, calls, set(range(calls)))
    for f in feeds:
        if decim == 17:
            assert 490 in f.valids and set(f.valids) <= {490, 491}, f.valids
        ch.expect_calls(f.dem, parts=parts, **{form: calls})
        f.dem.close()
    ch.check(f"late_positions_lockin_decim{decim}", errs, sec, calls)


# ---------------------------------------------------------------------------
# b. the benchmark's own sweep (C4) from its first buffer to its wrap
# ---------------------------------------------------------------------------
def test_c4_sweep_to_its_end_and_over_the_wrap(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """1e6 steps of 200 samples at 200 Msps, 1 M-sample buffers: 200 calls are one sweep.  Compared in full: call 0;
    18 and 19 (q passes 2^32 at step 92 682, sample 18.5 M); 100 (A = f0 + fi c crosses zero); 199, the last buffer
    of the sweep; 200 and 201, the first two of the next."""
    ch.clean_env(monkeypatch, {})
    rate, L, calls = 200_000_000, 1_000_000, 202
    law = ch.Law(oracle_mod, rate, 1_000_000, 1.0, [(-100_000_000, 100_000_000)] + spans(rate, 5), length=200, period=200_000_000)
    compare = {0, 18, 19, 100, 199, 200, 201}
    assert 18 * L < 92_682 * 200 < 19 * L and 200 * L == law.period
    x = crandn(np.random.default_rng(103), L)
    five = [1, 2, 3, 4, 5]
    feeds = [ch.Feed("lockin", law.handle(1, L, cols=[0]), law, 1, L, cols=[0]),
             ch.Feed("undecimated", law.handle(0, L, cols=[0]), law, 0, L, cols=[0]),
             ch.Feed("lockin_five", law.handle(1, L, cols=five), law, 1, L, cols=five)]
    assert [f.dem.kernel_name for f in feeds] == ["chirp_lockin_kernel", "chirp_demod_kernel", "chirp_multi_lockin_kernel"]
    errs, sec = ch.walk(cuda_device, oracle_mod, ch.Reference(oracle_mod, law, x), feeds, x, calls, compare)
    for f in feeds:
        assert f.valids == [5000 if f.decim else L] * calls
        ch.expect_calls(f.dem, parts=1, plain=calls)
        f.dem.close()
    ch.check("c4_sweep_to_its_end_and_over_the_wrap", errs, sec, calls)


# ---------------------------------------------------------------------------
# c. beyond 2^32: the 64-bit kernels with e >= 2^32 and at the wrap of a period above 2^32
# ---------------------------------------------------------------------------
def test_generic_kernels_beyond_2_to_32(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """A sweep of 4.3e9 samples in buffers of 2^22: chirp index 2^32 is where call 1024 starts, the period wraps in call
    1025.  Compared: calls 1023 ... 1026 -- every lock-in point; undecimated the first and last 20 000 samples of each
    and 20 000 around the wrap."""
    ch.clean_env(monkeypatch, {})
    rate, L, W = 200_000_000, 1 << 22, 20_000
    law = ch.Law(oracle_mod, rate, 1_000_000, 21.5, spans(rate, 2), length=4300)
    assert (1 << 32) < law.period < (1 << 32) + 2 * L and (1 << 32) % L == 0
    k32, kwrap = (1 << 32) // L, law.period // L
    compare, calls = {k32 - 1, k32, kwrap, kwrap + 1}, kwrap + 2
    at_wrap = law.period - kwrap * L
    assert len(compare) == 4 and W < at_wrap < L - 2 * W

    def windows(k):
        return [(0, W), (L - W, W)] + ([(at_wrap - W // 2, W)] if k == kwrap else [])
    x = crandn(np.random.default_rng(104), L)
    feeds = [ch.Feed("undecimated", law.handle(0, L, cols=[0]), law, 0, L, cols=[0], windows=windows),
             ch.Feed("lockin", law.handle(1, L, cols=[0]), law, 1, L, cols=[0]),
             ch.Feed("lockin_two", law.handle(1, L), law, 1, L)]
    assert [f.dem.kernel_name for f in feeds] == ["chirp_demod_kernel", "chirp_lockin_kernel", "chirp_multi_lockin_kernel"]
    errs, sec = ch.walk(cuda_device, oracle_mod, ch.Reference(oracle_mod, law, x), feeds, x, calls, compare)
    for f in feeds:
        ch.expect_calls(f.dem, parts=1, generic=calls)
        f.dem.close()
    ch.check("generic_kernels_beyond_2_to_32", errs, sec, calls)


# ---------------------------------------------------------------------------
# d. every form and every edge of the rule, tiny shapes
# ---------------------------------------------------------------------------
RATE_D = 1_000_000
EDGES = {
    # name: (steps, chirp_t, length, decim, L, calls, calls that split, waves per point then: one chirp, five chirps)
    "len1_decim15_not_split": (10, 1e-5, 1, 15, 1000, 5, 0, 1, 1),          # 15 stretches: one short of a split
    "len1_decim16_split_4x4": (10, 1e-5, 1, 16, 1000, 5, 5, 4, 4),          # the smallest split; a point is 1.6 sweeps
    "valid_512_and_513": (10, 1e-5, 1, 16, 8200, 6, 3, 4, 4),               # 512 points split, 513 do not: in turn
    "len200_decim16_steps7": (7, 1.403e-3, 200, 16, 10_000, 5, 5, 4, 4),    # every stretch a new step; a point 2.3 sweeps
    "len257_decim8_steps5": (5, 1.2875e-3, 257, 8, 10_000, 5, 5, 4, 4),     # a step's second stretch: one live sample
    "len600_decim6_steps5": (5, 3.0025e-3, 600, 6, 10_000, 5, 5, 4, 4),     # 18 stretches in parts of 5, 5, 5, 3: parts
    #                                                                         start mid-step, a wrap inside every point
    "len16_decim260_one_point": (37, 6.105e-4, 16, 260, 4200, 9, 9, 65, 65),    # 65 parts: the sum kernel's second round
    "two_steps": (2, 6.01e-4, 300, 8, 10_000, 5, 5, 4, 4),                  # the smallest sweep
}


@pytest.mark.parametrize("shape", list(EDGES))
def test_rule_edges(cuda_device, gsdr_lib, oracle_mod, monkeypatch, shape):
    """Each shape three ways: as the library chooses, with GSDR_CHIRP_SPLIT=0 (plain, whatever the shape) and as a
    five-chirp handle.  A call splits when it completes at most 512 points and a point has at least 16 stretches; the
    counters must say so call by call."""
    steps, t, length, decim, L, calls, split_calls, parts1, parts5 = EDGES[shape]
    law = ch.Law(oracle_mod, RATE_D, steps, t, spans(RATE_D, 5), length=length)
    ch.clean_env(monkeypatch, {"GSDR_CHIRP_SPLIT": "0"})
    off = law.handle(decim, L, cols=[0])
    ch.clean_env(monkeypatch, {})
    feeds = [ch.Feed("chosen", law.handle(decim, L, cols=[0]), law, decim, L, cols=[0]),
             ch.Feed("split_off", off, law, decim, L, cols=[0]), ch.Feed("five", law.handle(decim, L), law, decim, L)]
    x = crandn(np.random.default_rng(105 + decim + length), L)
    errs, sec = ch.walk(cuda_device, oracle_mod, ch.Reference(oracle_mod, law, x), feeds, x, calls, set(range(calls)))
    for f, parts in zip(feeds, (parts1, 1, parts5)):
        if shape == "valid_512_and_513":
            assert f.valids == [512, 513] * 3
        else:
            assert max(f.valids) <= 512
        last_split = parts > 1 and f.valids[-1] <= 512
        split = 0 if f.name == "split_off" else split_calls
        ch.expect_calls(f.dem, parts=parts if last_split else 1, split=split, plain=calls - split)
        # ... and it is what the host-side plan says for the last call
        p = C.c_int()
        form = gsdr_lib.gsdr_chirp_lockin_plan(steps, length, length * decim, 0, f.valids[-1], f.C, int(f.name != "split_off"),
                                               16384, C.byref(p), None)
        assert (form, p.value) == ((1, parts) if last_split else (0, 1)), (f.name, form, p.value)
        f.dem.close()
    ch.check(f"rule_edges_{shape}", errs, sec, calls)


def test_sixteen_chirps_fill_the_partial_sums(cuda_device, gsdr_lib, oracle_mod, monkeypatch):
    """16 chirps, 512 points of 64 stretches per call: two waves per point, 512 * 2 * 16 partial sums -- the 16 384
    slots of the buffer to the last one.  Beside it the same shape with the split off, as one chirp (eight waves per
    point) and as five (six).  Then two calls of the 16-chirp handle into a guarded output."""
    import torch
    steps, t, decim, L, calls = 10, 1e-5, 64, 32_768, 4
    law = ch.Law(oracle_mod, RATE_D, steps, t, spans(RATE_D, 16), length=1)
    ch.clean_env(monkeypatch, {"GSDR_CHIRP_SPLIT": "0"})
    off = law.handle(decim, L)
    ch.clean_env(monkeypatch, {})
    five = list(range(5))
    feeds = [ch.Feed("sixteen", law.handle(decim, L), law, decim, L), ch.Feed("sixteen_split_off", off, law, decim, L),
             ch.Feed("one", law.handle(decim, L, cols=[0]), law, decim, L, cols=[0]),
             ch.Feed("five", law.handle(decim, L, cols=five), law, decim, L, cols=five)]
    x = crandn(np.random.default_rng(106), L)
    ref = ch.Reference(oracle_mod, law, x)
    errs, sec = ch.walk(cuda_device, oracle_mod, ref, feeds, x, calls, set(range(calls)))
    for f, parts in zip(feeds, (2, 1, 8, 6)):
        assert f.valids == [512] * calls
        ch.expect_calls(f.dem, parts=parts, **({"split": calls} if parts > 1 else {"plain": calls}))
    assert 512 * 2 * 16 == 16384
    ch.check("sixteen_chirps_fill_the_partial_sums", errs, sec, calls)
    # the output of the full partial-sum buffer lands in out[0, 512 * 16) and nowhere else
    dem, w = feeds[0].dem, feeds[0].w
    xd = torch.from_numpy(x).to(cuda_device)
    for k, o in ((calls, 0), (calls + 1, 1)):
        wout, vout = ex.guarded_output(dem.out_capacity, o, cuda_device)
        n = dem.process_device(xd, vout)
        torch.cuda.synchronize()
        ex.check_output(wout, vout, n)
        assert n == 512 * 16
        y = vout[:n].cpu().numpy().reshape(512, 16)
        yr = np.stack([ref.points(c, k * L, 512, w) for c in range(16)], axis=1)
        assert rel_err_per_tone(y, yr, "guarded").max() <= TOL
    ch.expect_calls(dem, parts=2, split=calls + 2)
    for f in feeds:
        f.dem.close()
