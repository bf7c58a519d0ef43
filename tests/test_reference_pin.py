"""The oracle and recipe B against the reference's OWN code (CPU only).

oracle/_ref/libgsdr_ref.so is the reference's RX path -- its kernels (run serially), its FIR
class, RX_buffer_demodulator and the buffer helpers -- compiled for the host by
oracle/build_ref.py; only cuBLAS and cuFFT are stand-ins (fp64 accumulate, oracle/ref/include/).
tests/golden/ref_*.npz were recorded from it (tests/golden/make_ref_golden.py).

Checks: every fixture case against oracle.* and recipe_b (per tone <= 1e-6 relative, every
length exact; these need no library), the fixtures re-recorded bit for bit, 40 seeded random
shapes side by side, and exact equality of the windows, the buffer_helper / VNA helper
sequences, the chirp parameters and the TX chirp.  Tests that need the library skip only with
the reason "oracle/_ref not built".
"""
import json
import os

import numpy as np
import pytest

from golden import make_ref_golden as G
from oracle import recipe_b, refpin

HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 1e-6
needs_ref = pytest.mark.skipif(not refpin.available(), reason=refpin.SKIP_REASON)
MODES = ["direct", "tones", "noise", "chirp", "nodsp"]


def load(mode):
    return np.load(os.path.join(HERE, "golden", f"ref_{mode}.npz"), allow_pickle=False)


def case_ids():
    return [(m, c) for m in MODES for c in range(len(G.CASES[m]))]


def rel_err(y, yr):
    y, yr = np.asarray(y, np.complex128), np.asarray(yr, np.complex128)
    den = np.linalg.norm(yr, axis=0)
    return float(np.max(np.linalg.norm(y - yr, axis=0) / np.where(den == 0, 1.0, den))) if yr.size else 0.0


class _RecipeB:
    """recipe_b behind the oracle's constructor signatures, fp64 accumulate."""

    @staticmethod
    def Direct(freq, rate, decim, f, L):
        return recipe_b.Direct(freq, rate, decim, f, L, acc=np.complex128)

    @staticmethod
    def Pfb(freq, rate, nfft, avg, L):
        return recipe_b.Pfb(freq, rate, nfft, avg, L)

    @staticmethod
    def Noise(nfft, avg, L):
        return recipe_b.Pfb([0] * nfft, 1, nfft, avg, L, bins=list(range(nfft)))

    @staticmethod
    def Chirp(*a):
        return recipe_b.Chirp(*a, acc=np.complex128)


def run(dem, x, L, nch):
    outs = [np.asarray(dem.process(x[b * L:(b + 1) * L])).reshape(-1, nch) for b in range(len(x) // L)]
    return np.concatenate(outs), [o.size for o in outs]


@pytest.mark.parametrize("mode,c", case_ids(), ids=lambda v: str(v))
@pytest.mark.parametrize("impl", ["oracle", "recipe_b"])
def test_fixture_against_restatements(oracle_mod, mode, c, impl):
    """The two restatements reproduce what the compiled reference returned."""
    if mode == "nodsp":
        g = load(mode)
        assert np.array_equal(g[f"c{c}_y"], g[f"c{c}_x"]) and list(g[f"c{c}_lengths"]) == [256, 256]
        return
    g = load(mode)
    cfg = json.loads(str(g[f"c{c}_config"]))
    dem, nch = G.make_ref(mode, cfg, oracle_mod if impl == "oracle" else _RecipeB)
    y, lengths = run(dem, g[f"c{c}_x"], cfg["buffer_len"], nch)
    assert lengths == list(g[f"c{c}_lengths"])
    e = rel_err(y, g[f"c{c}_y"].reshape(-1, nch))
    assert e <= BAR, (mode, c, impl, e)


@needs_ref
@pytest.mark.parametrize("mode", MODES)
def test_fixtures_regenerate_bit_for_bit(mode):
    g = load(mode)
    assert json.loads(str(g["sources"])) == G.source_digests(), "fixture recorded from other reference sources"
    for c, cfg in enumerate(G.CASES[mode]):
        assert json.loads(str(g[f"c{c}_config"])) == cfg
        x, y, n = G.record(mode, c, cfg)
        assert np.array_equal(x, g[f"c{c}_x"]), (mode, c, "input")
        assert np.array_equal(n, g[f"c{c}_lengths"]), (mode, c, "lengths")
        assert np.array_equal(y, g[f"c{c}_y"]), (mode, c, "outputs")


@needs_ref
def test_tx_fixture_regenerates_and_matches_oracle(oracle_mod):
    g = np.load(os.path.join(HERE, "golden", "ref_tx.npz"), allow_pickle=False)
    new = G.record_tx()
    for k, v in new.items():
        assert np.array_equal(g[k], v), k
    for i, t in enumerate(G.TX_CHIRP):
        cp = oracle_mod.ChirpParam(t["num_steps"], t["length"], t["chirpness"], t["f0"])
        y = oracle_mod.chirp_gen(cp, t["last_index"], t["n"], t["scale"])
        assert np.array_equal(y, g[f"chirp{i}_y"]), i
    for i, t in enumerate(G.TX_TONES):
        yo = oracle_mod.tone_gen(t["freq"], t["ampl"], t["rate"], 0, t["rate"], t["scale"])
        yb = recipe_b.tone_gen(t["freq"], t["ampl"], t["rate"], t["scale"])
        ref = g[f"tones{i}_y"]
        scale = np.abs(ref).max()
        assert np.abs(yo - ref).max() <= BAR * scale, i
        assert np.abs(yb - ref).max() <= BAR * scale, i


@needs_ref
@pytest.mark.parametrize("length,fc", [(40, 0.0375), (41, 0.0375), (4, 0.125), (1000, 1 / 2000), (4096, 1 / 2048),
                                      (700, 0.75 / 200), (7, 0.75 / 2), (1, 0.375)])
def test_sinc_window_exact(oracle_mod, length, fc):
    w = refpin.make_sinc_window(length, fc)
    assert np.array_equal(w, oracle_mod.make_sinc_window(length, fc), equal_nan=True)   # length 1: 0 / 0, NaN
    # numpy's float32 sin / cos are not the C library's: a few ulp
    assert np.allclose(recipe_b.make_sinc_window(length, np.float32(fc)), w, rtol=0,
                       atol=4e-7 * np.nanmax(np.abs(w), initial=0.0), equal_nan=True)


@needs_ref
@pytest.mark.parametrize("length,side", [(20, 2), (7, 0), (70, 7), (810, 81), (1, 0), (33, 16)])
def test_flat_window_exact(oracle_mod, length, side):
    w = refpin.make_flat_window(length, side)
    assert np.array_equal(w, oracle_mod.make_flat_window(length, side))
    assert np.array_equal(w, recipe_b.make_flat_window(length, side))


@needs_ref
@pytest.mark.parametrize("n_tones,L,avg,n_eff", [(10, 103, 4, 3), (64, 1024, 1, 4), (100, 1234, 3, 100),
                                                (194, 1500, 3, 5), (1024, 700, 4, 1), (7, 7, 1, 7), (1000, 60_000, 6, 2)])
def test_buffer_helper_sequence_exact(oracle_mod, n_tones, L, avg, n_eff):
    seq = refpin.buffer_helper_seq(n_tones, L, avg, n_eff, 12)
    o = oracle_mod.BufferHelper(n_tones, L, avg, n_eff)
    b = recipe_b.BufferHelper(n_tones, L, avg, n_eff)
    for step, s in enumerate(seq):
        assert s == o.state(), (step, s, o.state())
        assert s == {k: getattr(b, k) for k in refpin.BUFFER_HELPER_FIELDS}, step
        o.update()
        b.update()


@needs_ref
@pytest.mark.parametrize("ppt,L", [(7, 2000), (40, 400), (810, 500), (1, 10), (3, 1)])
def test_vna_helper_sequence_exact(oracle_mod, ppt, L):
    o, b = oracle_mod.VnaHelper(ppt, L), recipe_b.VnaHelper(ppt, L)
    for step, s in enumerate(refpin.vna_helper_seq(ppt, L, 12)):
        assert s == o.state(), (step, s)
        assert s == {k: getattr(b, k) for k in refpin.VNA_HELPER_FIELDS}, step
        o.update()
        b.update()


CHIRP_PARAMS = [(200_000_000, -90_000_000, 90_000_000, 1000, 3.5e-5), (1_000_000, 1000, 200_000, 37, 0.01),
                (1_000_000, -200_000, 300_000, 100, 8e-4), (100_000_000, 0, 1_000_000, 0, 1e-4),
                (1_000_000, 5000, 7000, 2, 0.5), (200_000_000, 99_000_000, -99_000_000, 7, 1e-6)]


@needs_ref
@pytest.mark.parametrize("args", CHIRP_PARAMS, ids=lambda a: str(a))
def test_chirp_parameters_exact(oracle_mod, args):
    dem = refpin.Chirp(*args, 0, 1000)
    want = dem.chirp_params()
    dem.close()
    cp = oracle_mod.chirp_params(*args)
    assert want == {k: getattr(cp, k) for k in ("num_steps", "length", "chirpness", "f0")}
    assert tuple(want.values()) == tuple(recipe_b.chirp_params(*args))


def random_case(seed):
    """A seeded shape of one mode, within what the reference runs."""
    rng = np.random.default_rng(9000 + seed)
    mode = ["direct", "direct", "tones", "noise", "chirp"][seed % 5]
    nbuf = int(rng.integers(2, 5))
    if mode == "direct":
        rate = int(rng.choice([1000, 48_000, 1_000_000, 200_000_000, 2_147_483_000]))
        decim = int(rng.choice([0, 1, 3, 20, 100]))
        L = max(decim, 1) * int(rng.integers(2, 40))
        N = int(rng.choice([1, 3, 32, 33]))
        freq = [int(f) for f in rng.integers(-rate // 2, rate // 2 + 1, size=N)]
        pf = int(rng.integers(1 + (decim == 1), 8))      # one tap in all: the reference's window is NaN
        cfg = dict(rate=rate, decim=decim, pf_average=pf, buffer_len=L, nbuf=nbuf, freq=freq)
    elif mode in ("tones", "noise"):
        nfft = int(rng.choice([8, 10, 32, 37, 64, 100, 128]))
        rate = int(rng.choice([1000, 1_000_000, 200_000_000]))
        L = int(rng.integers(nfft // 2 + 1, 12 * nfft))
        cfg = dict(fft_tones=nfft, pf_average=int(rng.integers(1, 5)), buffer_len=L, nbuf=nbuf + 1)
        if mode == "tones":
            cfg.update(rate=rate, freq=[int(f) for f in rng.integers(-rate // 2, rate // 2, size=int(rng.integers(1, 6)))])
    else:
        rate = int(rng.choice([1_000_000, 200_000_000]))
        steps = int(rng.integers(2, 300))
        length = int(rng.integers(1, 30))
        f0, f1 = (int(v) for v in rng.integers(-rate // 2, rate // 2, size=2))
        decim = int(rng.choice([0, 1, 2, 5]))
        cfg = dict(rate=rate, freq=f0, chirp_f=f1, swipe_s=steps, chirp_t=steps * length / rate, decim=decim,
                   buffer_len=max(length * decim, int(rng.integers(50, 700))), nbuf=nbuf)   # ppt <= buffer_len
    return mode, cfg


@needs_ref
@pytest.mark.parametrize("seed", range(40))
def test_random_shape_against_restatements(oracle_mod, seed):
    mode, cfg = random_case(seed)
    x, y, n = G.record(mode, 1000 + seed, cfg)
    nch = len(G.case_freq(cfg)) if mode in ("direct", "tones") else cfg["fft_tones"] if mode == "noise" else 1
    yr = y.reshape(-1, nch)
    for impl in (oracle_mod, _RecipeB):
        dem, _ = G.make_ref(mode, cfg, impl)
        yo, lengths = run(dem, x, cfg["buffer_len"], nch)
        assert lengths == list(n), (mode, cfg, impl)
        e = rel_err(yo, yr)
        assert e <= BAR, (mode, cfg, impl, e)
