"""Records tests/golden/ref_*.npz FROM THE REFERENCE'S OWN CODE: oracle/_ref/libgsdr_ref.so,
which oracle/build_ref.py compiles for the host from the reference's sources (kernels, FIR
class, RX_buffer_demodulator, buffer helpers) with double-accumulating stand-ins for cuBLAS and
cuFFT.  Run `python tests/golden/make_ref_golden.py` after `__graft_entry__.build()`.

Each file holds, per case c: `c{c}_config` (JSON), `c{c}_x` (the seeded input, all buffers
back to back), `c{c}_y` (the outputs back to back, [rows, channels] flattened) and
`c{c}_lengths` (complex samples returned per call); `sources` holds the sha256 of every
reference file the library was built from.  tests/test_reference_pin.py re-records every case
and requires the same bits; tests/test_gpu_reference_pin.py runs libgsdr on the same inputs.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import refpin  # noqa: E402

# mode -> cases.  DIRECT: decim 0 is the NCO mix alone; <= 32 tones take mix_few_kernel / ddc_few
# shapes in libgsdr, 33 the wider kernels.
CASES = {
    "direct": [
        # tones at 0 and +-rate/2; rate 500 < 4 buffers of 150: the NCO index wraps inside the fourth
        dict(rate=500, decim=0, pf_average=1, buffer_len=150, nbuf=4, freq=[0, 250, -250, -61]),
        # 33 tones undecimated
        dict(rate=1_000_000, decim=0, pf_average=4, buffer_len=32, nbuf=3, seed_freq=33),
        # tf * ((j + idx) % rate) > 2^31: the 64-bit phase product at 200 Msps
        dict(rate=200_000_000, decim=0, pf_average=1, buffer_len=200, nbuf=3,
             freq=[99_999_999, -99_999_999, 12_345_679, -100_000_000]),
        # (decim 1 with pf_average 1 is one tap, and the reference's window of length 1 is NaN: 0 / 0 in its
        #  Hamming term; the oracle agrees, the shape is left out)
        dict(rate=10_000, decim=1, pf_average=2, buffer_len=100, nbuf=4, freq=[1, -2500, 4999, -5000]),
        dict(rate=10_000, decim=1, pf_average=4, buffer_len=100, nbuf=4, freq=[0, 3333, -3333]),
        dict(rate=1_000_000, decim=20, pf_average=7, buffer_len=400, nbuf=4, freq=[-1, 0, 250_000, -499_999, 500_000]),
        dict(rate=1000, decim=20, pf_average=4, buffer_len=400, nbuf=5, freq=[0, 37, -211, 499, -500]),
        dict(rate=1_000_000, decim=100, pf_average=4, buffer_len=500, nbuf=4, seed_freq=33),
        dict(rate=1_000_000, decim=100, pf_average=1, buffer_len=1000, nbuf=3, freq=[-300_000, 7, 123_457]),
        # decimation 20 with a 7-tap-phase FIR at 200 Msps: large phase products through the filter
        dict(rate=200_000_000, decim=20, pf_average=7, buffer_len=200, nbuf=4, freq=[99_999_999, -77_777_777, 3]),
    ],
    "tones": [
        # nfft does not divide L: buffer_helper carries; negative and edge bins
        dict(rate=1000, fft_tones=10, pf_average=4, buffer_len=103, nbuf=6, freq=[-500, -451, 0, 120, 499]),
        dict(rate=1_000_000, fft_tones=64, pf_average=1, buffer_len=1024, nbuf=3, freq=[-500_000, -15_625, 0, 484_375]),
        dict(rate=1_000_000, fft_tones=100, pf_average=3, buffer_len=1234, nbuf=4, freq=[-499_999, -10_000, 1, 490_000]),
        # 194 = 2 * 97: a large prime factor
        dict(rate=200_000_000, fft_tones=194, pf_average=3, buffer_len=1500, nbuf=3,
             freq=[-100_000_000, -3_000_000, 0, 5_154_639, 98_969_071]),
        dict(rate=1_000_000, fft_tones=40, pf_average=4, buffer_len=1000, nbuf=3, freq=[-475_000, 25_000]),
    ],
    "noise": [
        dict(fft_tones=64, pf_average=4, buffer_len=1000, nbuf=3),
        dict(fft_tones=100, pf_average=2, buffer_len=1234, nbuf=3),
    ],
    "chirp": [
        # without lock-in; f0 < 0: the frequency word wraps the 64-bit index
        dict(rate=200_000_000, freq=-90_000_000, chirp_f=90_000_000, swipe_s=1000, chirp_t=3.5e-5, decim=0,
             buffer_len=500, nbuf=3),
        # long steps: the 64-bit index truncated to int32 far from 0
        dict(rate=1_000_000, freq=1000, chirp_f=200_000, swipe_s=37, chirp_t=0.01, decim=0, buffer_len=500, nbuf=3),
        # lock-in, ppt = 7 does not divide L: the spare_size carry runs
        dict(rate=200_000_000, freq=-90_000_000, chirp_f=90_000_000, swipe_s=1000, chirp_t=3.5e-5, decim=1,
             buffer_len=500, nbuf=3),
        # lock-in, ppt = 8 * 5 = 40 divides L
        dict(rate=1_000_000, freq=-200_000, chirp_f=300_000, swipe_s=100, chirp_t=8e-4, decim=5, buffer_len=400,
             nbuf=3),
        # lock-in, ppt = 270 * 3 (libgsdr and the oracle refuse ppt > buffer_len)
        dict(rate=1_000_000, freq=1000, chirp_f=200_000, swipe_s=37, chirp_t=0.01, decim=3, buffer_len=1000, nbuf=4),
    ],
    "nodsp": [
        dict(buffer_len=256, nbuf=2),
    ],
}

TX_CHIRP = [
    dict(num_steps=1000, length=7, chirpness=3869339, f0=-1932735282, last_index=6500, n=5000, scale=1.0),
    dict(num_steps=37, length=270, chirpness=23741624, f0=4294967, last_index=9980, n=3000, scale=0.5),
]
TX_TONES = [
    dict(rate=1000, freq=[100, -250, 499, -499, 1, -1], ampl=[0.1, 0.2, 0.05, 0.3, 0.01, 0.02], scale=1.0),
    dict(rate=4096, freq=[2047, -2048, 17, 17, -3], ampl=[0.25, 0.125, 0.5, 0.1, 0.01], scale=0.5),
]

REF_SOURCE_NAMES = ["cpp/kernels.cu", "cpp/fir.cu", "cpp/USRP_demodulator.cpp",
                    "cpp/USRP_server_memory_management.cpp", "cpp/USRP_server_console_print.cpp"]


def crandn(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def case_freq(cfg):
    if "freq" in cfg:
        return [int(f) for f in cfg["freq"]]
    rng = np.random.default_rng(cfg["seed_freq"])
    r = cfg["rate"]
    return [int(f) for f in rng.integers(-r // 2 + 1, r // 2, size=cfg["seed_freq"])]


def make_ref(mode, cfg, impl=None):
    """A demodulator for a case; impl is refpin (default) or a module with the oracle's API."""
    m = impl or refpin
    L = cfg["buffer_len"]
    if mode == "direct":
        return m.Direct(case_freq(cfg), cfg["rate"], cfg["decim"], cfg["pf_average"], L), len(case_freq(cfg))
    if mode == "tones":
        return m.Pfb(cfg["freq"], cfg["rate"], cfg["fft_tones"], cfg["pf_average"], L), len(cfg["freq"])
    if mode == "noise":
        return m.Noise(cfg["fft_tones"], cfg["pf_average"], L), cfg["fft_tones"]
    if mode == "chirp":
        return m.Chirp(cfg["rate"], cfg["freq"], cfg["chirp_f"], cfg["swipe_s"], cfg["chirp_t"], cfg["decim"], L), 1
    return refpin.Nodsp(L), 1


def case_input(mode, c, cfg):
    rng = np.random.default_rng([sorted(CASES).index(mode), c, 20261016])
    return crandn(rng, cfg["buffer_len"] * cfg["nbuf"])


def record(mode, c, cfg, x=None):
    """(x, y, lengths) of one case, from the compiled reference."""
    x = case_input(mode, c, cfg) if x is None else x
    dem, nch = make_ref(mode, cfg)
    L = cfg["buffer_len"]
    outs = [dem.process(x[b * L:(b + 1) * L]).ravel() for b in range(len(x) // L)]
    dem.close()
    return x, np.concatenate(outs), np.array([len(o) for o in outs], dtype=np.int64)


def record_tx():
    out = {}
    for i, t in enumerate(TX_CHIRP):
        out[f"chirp{i}_config"] = np.array(json.dumps(t))
        out[f"chirp{i}_y"] = refpin.chirp_gen(t["num_steps"], t["length"], t["chirpness"], t["f0"], t["last_index"],
                                             t["n"], t["scale"])
    for i, t in enumerate(TX_TONES):
        out[f"tones{i}_config"] = np.array(json.dumps(t))
        out[f"tones{i}_y"] = refpin.tone_gen(t["freq"], t["ampl"], t["rate"], t["scale"])
    return out


def source_digests():
    with open(os.path.join(os.path.dirname(refpin.LIB_PATH), "SOURCES.json")) as fh:
        sha = json.load(fh)["sha256"]
    return {k: sha[k] for k in REF_SOURCE_NAMES}


def main():
    if not refpin.available():
        sys.exit("oracle/_ref/libgsdr_ref.so is missing: run __graft_entry__.build() where the reference is")
    sources = np.array(json.dumps(source_digests(), sort_keys=True))
    total = 0
    for mode, cases in CASES.items():
        doc = {"sources": sources}
        for c, cfg in enumerate(cases):
            x, y, n = record(mode, c, cfg)
            doc.update({f"c{c}_config": np.array(json.dumps(cfg)), f"c{c}_x": x, f"c{c}_y": y, f"c{c}_lengths": n})
        path = os.path.join(HERE, f"ref_{mode}.npz")
        np.savez_compressed(path, **doc)
        total += os.path.getsize(path)
        print(f"{path}: {len(cases)} cases, {os.path.getsize(path)} bytes")
    path = os.path.join(HERE, "ref_tx.npz")
    np.savez_compressed(path, sources=sources, **record_tx())
    total += os.path.getsize(path)
    print(f"{path}: {os.path.getsize(path)} bytes; all ref_*.npz {total} bytes")


if __name__ == "__main__":
    main()
