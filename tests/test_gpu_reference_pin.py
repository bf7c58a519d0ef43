"""libgsdr against the reference's OWN code: tests/golden/ref_*.npz (recorded from the reference
compiled for the host, tests/golden/make_ref_golden.py) and, where oracle/_ref/libgsdr_ref.so
travelled with the tree, a seeded fuzz through both side by side.

Bar: the suite's own, per tone ||y - y_ref|| / ||y_ref|| <= 1e-5 and every length exact; each
worst error goes to the margin record.
"""
import json
import os

import numpy as np
import pytest

from golden import make_ref_golden as G
from oracle import refpin
from test_gpu_parity import PFB_VARIANTS, TOL, crandn, engine, rel_err_per_tone, run_device, run_host  # noqa: F401
from test_reference_pin import random_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RX_MODES = ["direct", "tones", "noise", "chirp", "nodsp"]


def load(mode):
    return np.load(os.path.join(HERE, "golden", f"ref_{mode}.npz"), allow_pickle=False)


def make_gsdr(mode, cfg):
    import gpu_sdr_amd as g
    L = cfg["buffer_len"]
    if mode == "direct":
        freq = G.case_freq(cfg)
        p = g.param(mode="RX", rate=cfg["rate"], buffer_len=L, decim=cfg["decim"], pf_average=cfg["pf_average"],
                    freq=freq, wave_type=[g.w_type.DIRECT] * len(freq))
        nch = len(freq)
    elif mode == "tones":
        p = g.param(mode="RX", rate=cfg["rate"], buffer_len=L, decim=0, pf_average=cfg["pf_average"],
                    fft_tones=cfg["fft_tones"], freq=list(cfg["freq"]), wave_type=[g.w_type.TONES] * len(cfg["freq"]))
        nch = len(cfg["freq"])
    elif mode == "noise":
        p = g.param(mode="RX", rate=1_000_000, buffer_len=L, decim=0, pf_average=cfg["pf_average"],
                    fft_tones=cfg["fft_tones"], freq=[0], wave_type=[g.w_type.NOISE])
        nch = cfg["fft_tones"]
    elif mode == "chirp":
        p = g.param(mode="RX", rate=cfg["rate"], buffer_len=L, decim=cfg["decim"], freq=[cfg["freq"]],
                    chirp_f=[cfg["chirp_f"]], swipe_s=[cfg["swipe_s"]], chirp_t=[cfg["chirp_t"]],
                    wave_type=[g.w_type.CHIRP])
        nch = 1
    else:
        p = g.param(mode="RX", rate=1_000_000, buffer_len=L, wave_type=[g.w_type.NODSP])
        nch = 1
    return g.RX_buffer_demodulator(p, device_index=0), nch


def run_case(mode, cfg, x, yr, lengths, entry, dev, label=None):
    dem, nch = make_gsdr(mode, cfg)
    L = cfg["buffer_len"]
    outs = []
    for b in range(len(x) // L):
        xb = x[b * L:(b + 1) * L]
        use_host = entry == "host" or (entry == "mixed" and b % 2)
        outs.append(run_host(dem, xb) if use_host else run_device(dem, xb, dev))
    kernel = dem.kernel_name if mode != "nodsp" else ""
    dem.close()
    assert [len(o) for o in outs] == list(lengths), (mode, cfg)
    y = np.concatenate(outs).reshape(-1, nch)
    e = float(rel_err_per_tone(y, np.asarray(yr).reshape(-1, nch), label).max()) if y.size else 0.0
    assert e <= TOL, (mode, cfg, kernel, e)
    return kernel


def fixture_ids(modes):
    return [(m, c) for m in modes for c in range(len(G.CASES[m]))]


@pytest.mark.parametrize("mode,c", fixture_ids(RX_MODES), ids=lambda v: str(v))
@pytest.mark.parametrize("entry", ["host", "device"])
def test_reference_fixture(cuda_device, gsdr_lib, mode, c, entry, engine):
    g = load(mode)
    cfg = json.loads(str(g[f"c{c}_config"]))
    run_case(mode, cfg, g[f"c{c}_x"], g[f"c{c}_y"], g[f"c{c}_lengths"], entry, cuda_device)


@pytest.mark.parametrize("env,kernel,what", PFB_VARIANTS,
                         ids=["+".join(f"{k[9:]}={x}" for k, x in v[0].items()) or "default" for v in PFB_VARIANTS])
@pytest.mark.parametrize("mode,c", fixture_ids(["tones", "noise"]), ids=lambda v: str(v))
def test_reference_fixture_pfb_variants(cuda_device, gsdr_lib, monkeypatch, mode, c, env, kernel, what):
    """The TONES / NOISE fixtures under every switch of test_noise_every_kernel_variant."""
    for k in [k for k in os.environ if k.startswith("GSDR_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        g = load(mode)
        cfg = json.loads(str(g[f"c{c}_config"]))
        run_case(mode, cfg, g[f"c{c}_x"], g[f"c{c}_y"], g[f"c{c}_lengths"], "mixed", cuda_device, what)
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("c", range(len(G.CASES["direct"])))
@pytest.mark.parametrize("switch", ["default", "GSDR_DDC_FEW=0", "GSDR_MIX_FEW=0"])
def test_reference_fixture_few_tone_kernels(cuda_device, gsdr_lib, monkeypatch, c, switch):
    """The DIRECT fixtures with the library's own kernel choice (mix_few_kernel / ddc_few_kernel where
    they take the shape) and with each few-tone kernel switched off."""
    for k in [k for k in os.environ if k.startswith("GSDR_")]:
        monkeypatch.delenv(k)
    if switch != "default":
        k, v = switch.split("=")
        monkeypatch.setenv(k, v)
    g = load("direct")
    cfg = json.loads(str(g[f"c{c}_config"]))
    kernel = run_case("direct", cfg, g[f"c{c}_x"], g[f"c{c}_y"], g[f"c{c}_lengths"], "mixed", cuda_device)
    n = len(G.case_freq(cfg))
    if cfg["decim"] == 0 and n <= 32:
        assert (kernel == "mix_few_kernel") == (switch != "GSDR_MIX_FEW=0"), kernel


@pytest.mark.skipif(not refpin.available(), reason=refpin.SKIP_REASON)
@pytest.mark.parametrize("seed", range(120))
def test_reference_fuzz(cuda_device, gsdr_lib, seed):
    """Seeded shapes (48 DIRECT, 24 each of TONES, NOISE and CHIRP) through libgsdr and the compiled
    reference side by side."""
    mode, cfg = random_case(seed)
    x, y, n = G.record(mode, 2000 + seed, cfg)
    run_case(mode, cfg, x, y, n, "mixed", cuda_device, mode)
