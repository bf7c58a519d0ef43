"""TONES / NOISE inside the LDS (csrc/fft_kernels.hip: pfb_cu_kernel, pfb_lds_kernel), every shape a call can run in.

launch_pfb_lds decides each call anew from its frame count and the device's compute units (csrc/pfb_plan.h): kernel,
512 or 1024 threads, G frames per workgroup, one of five register shapes of the direct filter or the staged filter,
thread groups, teams, Bluestein, a prime first stage.  Here

  * every call's describe()["pfb_last"] equals gsdr_pfb_plan for that call's frame count on this device, the handle's
    "pfb_calls" equal the sums over its calls, and the class a case was written for is asserted, so that a case which
    slides into another branch fails instead of passing quietly;
  * the reference is the float64 model of tests/_pfb.py (held to the oracle in tests/test_pfb_model_host.py): the
    length of every call exact, and for every call of 8 frames and more the project's parity bar TOL = 1e-5 per bin
    (column) over the call's frames and per frame over its bins (frames of 8 columns and more); shorter calls are
    held to the bar as a whole;
  * the input is noise plus three tones on bins, ten times the rms of their bin (tests/_pfb.py: tones_on_bins says
    why in the spectrum), so a frame or column that is swapped or stale moves a large, known value;
  * a handle is fed four to six buffers, the device and the host entry in turn, the first against the zero carry; a
    handle's buffer length is fixed, so where frames must not depend on G a second handle is fed the same stream cut
    differently and held to the same model;
  * every device-entry call writes into an output with NaN guard zones (tests/_extents.py) that must stay untouched:
    a thread group that writes a frame which does not exist lands there.

Frame counts derive from the compute units torch reports: frames = a10 * cus // 10 + b.  The figures of every case --
worst per-bin and per-frame error, the same for a float32 emulation of filter and transform on the same input, the
classes that ran -- go to pfb_run_margins.json beside the parity margins (tests/_margins.py: write_record; committed
copy: profiles/pfb_run_margins.json).

Not covered here: timing, the global-memory FFT path (tests/test_gpu_parity.py), pfb_average_kernel
(tests/test_gpu_frame_average.py).
"""
import os

import numpy as np
import pytest

import _extents
import _margins
import _pfb
from test_pfb_plan_host import TABLE

pytestmark = pytest.mark.gpu

TOL = 1e-5
PFB_LDS_KERNELS = ("pfb_cu_kernel", "pfb_lds_kernel")
SWITCH_ENV = ("GSDR_PFB_CU", "GSDR_PFB_DIRECT", "GSDR_PFB_COL", "GSDR_PFB_CU_NT", "GSDR_PFB_RADIX8", "GSDR_PFB_TEAMS",
              "GSDR_PFB_FR", "GSDR_PFB_WIDE", "GSDR_PFB_BLUESTEIN", "GSDR_PFB_LDS", "GSDR_NOISE_FFT", "GSDR_TONES_FFT")
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    if not RECORD:
        return
    doc = {"bar": TOL,
           "metric": "worst over the calls of a case of ||y - model|| / ||model||, per bin over the call's frames and per "
                     "frame over its bins; fp32_*: the same for a numpy float32 emulation of filter and transform on the "
                     "case's last call of 8 frames or more",
           "classes": "(kernel, threads, direct, col, teams, G >= 2, dir_gs >= 2, dir_s >= 2, Bluestein, prime first stage)",
           "cases": RECORD}
    _margins.write_record("pfb_run_margins.json", doc, sort_keys=True)


@pytest.fixture(scope="module")
def cus(cuda_device):
    import torch
    return int(torch.cuda.get_device_properties(cuda_device).multi_processor_count)


def frames_of(spec, cus):
    a10, b = spec
    return a10 * cus // 10 + b


def tone_freqs(nfft, bins):
    """(rate, freq): TONES frequencies that the reference's tone -> bin rule maps to exactly `bins`"""
    half = nfft // 2
    return 1000 * nfft, [(((b - half) % nfft) - half) * 1000 for b in bins]


def run_stream(dev, lib, oracle, monkeypatch, cus, nfft, avg, L, calls, env=None, bins=None, seed=0, keep=False):
    """One handle through `calls` buffers of L samples of one seeded stream.  Asserts lengths, plan, counters, guard
    zones and the bar; returns what ran: {"plans", "frames", "per_bin", "per_frame", "fp32_per_bin", "fp32_per_frame",
    "out" (keep: every call's output)}."""
    import torch
    import gpu_sdr_amd as g
    env = env or {}
    for k in SWITCH_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        if bins is None:
            n_out = nfft
            p = g.param(mode="RX", rate=1_000_000, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft, freq=[0],
                        wave_type=[g.w_type.NOISE])
            model_bins = None
        else:
            n_out = len(bins)
            rate, freq = tone_freqs(nfft, bins)
            p = g.param(mode="RX", rate=rate, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft, freq=freq,
                        wave_type=[g.w_type.TONES] * n_out)
            model_bins = oracle.pfb_tone_bins(rate, nfft, freq)
            assert list(model_bins) == list(bins)
        dem = g.RX_buffer_demodulator(p, device_index=0)
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
    try:
        assert dem.kernel_name in PFB_LDS_KERNELS, dem.kernel_name
        d = dem.describe()
        assert d["pfb_last"]["kernel"] == "none" and d["pfb_last"]["frames"] == -1
        assert d["pfb_calls"] == {"pfb_cu_kernel": 0, "pfb_lds_kernel": 0, "direct": [0] * 6, "teams": 0, "runs": 0, "short_last_run": 0}
        sw = _pfb.switches_of_env(env)
        blue_m = _pfb.blue_length(lib, nfft, avg, sw, int(env.get("GSDR_PFB_BLUESTEIN", -1)))
        model = _pfb.Model(oracle, nfft, avg, model_bins)
        w32 = oracle.make_sinc_window(nfft * avg, np.float32(1.0 / (2 * nfft)))
        rng = np.random.default_rng(9000 + 7 * nfft + avg + seed)
        on = sorted({1 % nfft, (nfft // 3) % nfft, (nfft - 2) % nfft})
        res = {"plans": [], "frames": [], "per_bin": 0.0, "per_frame": 0.0, "fp32_per_bin": None, "fp32_per_frame": None, "out": []}
        want_calls = {"pfb_cu_kernel": 0, "pfb_lds_kernel": 0, "direct": [0] * 6, "teams": 0, "runs": 0, "short_last_run": 0}
        cap = dem.out_capacity
        for c in range(calls):
            x = _pfb.tones_on_bins(rng, L, nfft, on, model.w)
            frames = model.frames_of(L)
            yr = model.process(x)
            if c % 2 == 0:                                  # device entry, guarded output
                xin = torch.from_numpy(x).to(dev)
                whole, view = _extents.guarded_output(cap, c // 2 % 2, dev)
                n = dem.process(xin, view)
                torch.cuda.synchronize()
                _extents.check_output(whole, view, n)
                y = view[:n].cpu().numpy()
            else:                                           # host entry
                out = np.empty(cap, dtype=np.complex64)
                n = dem.process(np.ascontiguousarray(x), out)
                y = out[:n].copy()
            assert n == frames * n_out, (c, n, frames, n_out)
            y = y.reshape(frames, n_out)
            d = dem.describe()
            plan = _pfb.plan(lib, nfft, avg, frames, cus, n_out, sw, blue_m)
            assert plan is not None
            _pfb.describe_matches_plan(d["pfb_last"], plan, frames)
            assert dem.kernel_name == d["pfb_last"]["kernel"]
            want_calls["pfb_cu_kernel" if plan["cu"] else "pfb_lds_kernel"] += 1
            if plan["cu"]:
                want_calls["direct"][plan["direct"]] += 1
                want_calls["teams"] += plan["teams"]
            want_calls["runs"] += int(plan["G"] >= 2)
            want_calls["short_last_run"] += int(frames > 0 and frames % plan["G"] != 0)
            assert d["pfb_calls"] == want_calls, (c, d["pfb_calls"], want_calls)
            res["plans"].append(plan)
            res["frames"].append(frames)
            if keep:
                res["out"].append(y)
            if frames == 0:
                continue
            diff = y.astype(np.complex128) - yr
            e_all = float(np.linalg.norm(diff) / np.linalg.norm(yr))
            print(f"call {c}: {frames} frames, G {plan['G']}, all together {e_all:.3e}")
            assert e_all <= TOL, (c, e_all)
            if frames >= 8:
                eb = np.linalg.norm(diff, axis=0) / np.linalg.norm(yr, axis=0)
                print(f"call {c}: per bin {eb.max():.3e} (bin {int(eb.argmax())})")
                res["per_bin"] = max(res["per_bin"], float(eb.max()))
                emu = _pfb.fp32_emulation(model.last_stream, nfft, avg, w32, frames)
                emu = emu if model_bins is None else emu[:, model_bins]
                res["fp32_per_bin"] = float((np.linalg.norm(emu - yr, axis=0) / np.linalg.norm(yr, axis=0)).max())
                if n_out >= 8:
                    ef = np.linalg.norm(diff, axis=1) / np.linalg.norm(yr, axis=1)
                    print(f"call {c}: per frame {ef.max():.3e} (frame {int(ef.argmax())})")
                    res["per_frame"] = max(res["per_frame"], float(ef.max()))
                    res["fp32_per_frame"] = float((np.linalg.norm(emu - yr, axis=1) / np.linalg.norm(yr, axis=1)).max())
                    assert ef.max() <= TOL, (c, int(ef.argmax()), float(ef.max()))
                assert eb.max() <= TOL, (c, int(eb.argmax()), float(eb.max()))
        return res
    finally:
        dem.close()


def note(res, **more):
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    rec = RECORD.setdefault(test, {"per_bin": 0.0, "per_frame": 0.0, "fp32_per_bin": 0.0, "fp32_per_frame": 0.0, "classes": []})
    for k in ("per_bin", "per_frame", "fp32_per_bin", "fp32_per_frame"):
        rec[k] = max(rec[k], res[k] or 0.0)
    rec["classes"] = sorted(set(rec["classes"]) | {str(_pfb.plan_class(p)) + f" G={p['G']} dir_s={p['dir_s']} dir_gs={p['dir_gs']}"
                                                   for p, f in zip(res["plans"], res["frames"]) if f > 0})
    rec.update(more)


def buffer_len(nfft, frames):
    """a buffer that gives `frames` frames per call from the second call on (frames - avg in the first), one sample
    short of whole frames where the frame is long enough for that to hold for six calls"""
    return frames * nfft - (1 if nfft >= 16 else 0)


# ---------------------------------------------------------------------------------------------------------------------
# every row of the host table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", TABLE, ids=lambda r: "nfft%d_avg%d_%dx+%d" % r[:4])
def test_every_class_of_the_host_table_runs(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, row):
    """The row's shape on the device: the calls from the second on have the row's frame count and must be of its class."""
    nfft, avg, a10, b, cls = row[:5]
    frames = frames_of((a10, b), cus)
    res = run_stream(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, avg, buffer_len(nfft, frames), 4)
    assert res["frames"][1:] == [frames] * 3, res["frames"]
    for p in res["plans"][1:]:
        assert _pfb.plan_class(p) == cls, (_pfb.plan_class(p), cls)
    note(res)


# ---------------------------------------------------------------------------------------------------------------------
# the cases the run kernel's branches were never seen in
# ---------------------------------------------------------------------------------------------------------------------
def last_run(lib, nfft, avg, frames, cus, sw, k):
    """the frame count nearest to `frames` that runs the same kernel with the same G and whose last run holds k frames"""
    base = _pfb.plan(lib, nfft, avg, frames, cus, sw=sw)
    for d in range(0, 4 * base["G"] + 2):
        for f in (frames + d, frames - d):
            p = _pfb.plan(lib, nfft, avg, f, cus, sw=sw) if f > 0 else None
            if p and f % base["G"] == k and (p["cu"], p["G"], p["threads"]) == (base["cu"], base["G"], base["threads"]):
                return f
    raise AssertionError("no such frame count near %d" % frames)


# name, nfft, avg, (a10, b), environment, what the steady calls must be (field: value, or field: (">=", value))
CASES = [
    # thread groups (variant 4)
    ("groups_teams_G2", 128, 4, (23, 0), {}, {"direct": 4, "teams": 1, "G": 2, "dir_s": 4, "dir_gs": 1, "threads": 512}),
    ("groups_G5_gs2", 128, 4, (80, 1), {}, {"direct": 4, "G": 5, "dir_s": 4, "dir_gs": 2}),
    ("groups_G17_gs5", 128, 4, (320, 1), {}, {"direct": 4, "G": 17, "dir_s": 4, "dir_gs": 5}),
    ("groups_200", 200, 4, (80, 1), {}, {"direct": 4, "dir_s": 2, "dir_gs": (">=", 2), "threads": 512}),
    ("groups_101_prime_first", 101, 4, (80, 1), {}, {"direct": 4, "threads": 1024, "dir_s": 10, "G": (">=", 2), "prime": 1}),
    ("groups_10_51", 10, 4, (320, 1), {}, {"direct": 4, "dir_s": 51, "G": (">=", 2), "threads": 512}),
    # variant 1
    ("v1_512_G2_teams", 512, 4, (20, 1), {}, {"direct": 1, "G": 2, "teams": 1, "threads": 512}),
    ("v1_512_G3", 512, 4, (40, 1), {}, {"direct": 1, "G": 3, "teams": 0}),
    ("v1_512_G5", 512, 4, (80, 1), {}, {"direct": 1, "G": 5, "dir_gs": 5}),
    ("v1_1024_G3", 1024, 4, (23, 0), {}, {"direct": 1, "G": 3, "threads": 1024}),
    ("v1_1024_G5", 1024, 4, (40, 1), {}, {"direct": 1, "G": 5}),
    ("v1_1024_G4_teams", 1024, 4, (40, 0), {}, {"direct": 1, "G": 4, "teams": 1}),
    ("v1_1024_G2_teams", 1024, 4, (20, 0), {}, {"direct": 1, "G": 2, "teams": 1}),
    # variant 2
    ("v2_600_G2_teams", 600, 4, (20, 1), {}, {"direct": 2, "G": 2, "teams": 1, "threads": 512}),
    ("v2_600_G3", 600, 4, (40, 1), {}, {"direct": 2, "G": 3, "threads": 512}),
    ("v2_1230_G3_mfma", 1230, 4, (20, 1), {}, {"direct": 2, "G": 3, "prime": 1, "threads": 1024}),
    ("v2_1230_G4_mfma", 1230, 4, (30, 1), {}, {"direct": 2, "G": 4, "prime": 1}),
    ("v2_1536_fill_above", 1536, 4, (20, 0), {}, {"direct": 2, "G": 2, "cu": 1}),
    ("v2_1536_fill_below", 1536, 4, (20, 1), {}, {"cu": 0, "G": 1}),
    # variants 5 and 3: a frame per workgroup by construction
    ("v5_2600", 2600, 4, (10, -1), {}, {"direct": 5, "G": 1}),
    ("v5_3001_bluestein", 3001, 4, (10, -1), {}, None),
    ("v3_4096", 4096, 4, (10, -1), {}, {"direct": 3, "G": 1}),
    # Bluestein with runs
    ("bluestein_1018_G3", 1018, 4, (23, 0), {}, {"blue": 1, "G": 3}),
    ("bluestein_1004_G4", 1004, 4, (43, 0), {}, {"blue": 1, "G": 4}),          # (two buffers of 2048 points a frame: four fit)
    # the staged filter with runs
    ("staged_1000_5taps", 1000, 5, (23, 0), {}, {"direct": 0, "col": 0, "G": 3}),
    ("staged_1000_6taps", 1000, 6, (40, 1), {}, {"direct": 0, "col": 0, "G": 5}),
    ("staged_1016_5taps_prime", 1016, 5, (23, 0), {}, {"direct": 0, "col": 0, "G": 3, "prime": 1}),
    ("staged_1000_col_rotation", 1000, 4, (40, 1), {"GSDR_PFB_DIRECT": "0"}, {"direct": 0, "col": 1, "G": 5}),
    ("staged_1000_pointwise_4taps", 1000, 4, (40, 1), {"GSDR_PFB_DIRECT": "0", "GSDR_PFB_COL": "0"}, {"direct": 0, "col": 0, "G": 5}),
    # one, two and three taps through the direct filter: blocks beyond gw + F - 1 stay unloaded
    ("direct_1tap", 1024, 1, (23, 0), {}, {"direct": 1, "G": 3}),
    ("direct_2taps", 1024, 2, (40, 1), {}, {"direct": 1, "G": 5}),
    ("direct_3taps", 600, 3, (40, 1), {}, {"direct": 2, "G": 3}),
    ("direct_2taps_groups", 128, 2, (80, 1), {}, {"direct": 4, "G": 5, "dir_gs": 2}),
    # forced shapes: teams of one wave take the fence, not the counter barrier
    ("forced_1024_teams_of_64", 256, 4, (160, 0), {"GSDR_PFB_CU": "1", "GSDR_PFB_CU_NT": "1024"},
     {"threads": 1024, "G": 16, "teams": 1, "direct": 4, "dir_s": 4, "dir_gs": 4}),
    ("forced_512_teams_of_64", 256, 4, (160, 0), {"GSDR_PFB_CU": "1", "GSDR_PFB_CU_NT": "512"},
     {"threads": 512, "G": 8, "teams": 1, "direct": 4, "dir_s": 2, "dir_gs": 4}),
    ("forced_1024_teams_of_8_waves", 256, 4, (20, 0), {"GSDR_PFB_CU": "1", "GSDR_PFB_CU_NT": "1024"},
     {"threads": 1024, "G": 2, "teams": 1}),
]


def check_steady(plan, want):
    for k, v in (want or {}).items():
        got = {"blue": int(plan["blue_m"] > 0), "prime": int(bool(plan["radices"]) and plan["radices"][0] > 16)}.get(k, plan.get(k))
        if isinstance(v, tuple):
            assert got >= v[1], (k, got, v, plan)
        else:
            assert got == v, (k, got, v, plan)


# (cases with a frame per workgroup have no short run)
RUN_SHAPES = [(c, last) for c in CASES
              for last in (("whole",) if c[0] in ("v2_1536_fill_below", "v5_2600", "v5_3001_bluestein", "v3_4096") else ("whole", "short_by_1", "one_frame"))]


@pytest.mark.parametrize("case,last", RUN_SHAPES, ids=lambda v: v[0] if isinstance(v, tuple) else v)
def test_run_shapes(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, case, last):
    """Every branch of the run kernel at a frame count that makes the last run whole, one frame short (G - 1 frames:
    the last thread group has fewer frames than the others, or none) and one frame long (every group but the first
    has gw <= 0)."""
    name, nfft, avg, spec, env, want = case
    frames = frames_of(spec, cus)
    sw = _pfb.switches_of_env(env)
    G = _pfb.plan(gsdr_lib, nfft, avg, frames, cus, sw=sw)["G"]
    if last != "whole":
        assert G >= 2, "a case listed with short runs must have runs"
        frames = last_run(gsdr_lib, nfft, avg, frames, cus, sw, G - 1 if last == "short_by_1" else 1)
    res = run_stream(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, avg, buffer_len(nfft, frames), 4, env)
    assert res["frames"][1:] == [frames] * 3
    for p in res["plans"][1:]:
        check_steady(p, want)
        if last != "whole" and p["cu"]:
            assert frames % p["G"] == (p["G"] - 1 if last == "short_by_1" else 1)
    note(res)


@pytest.mark.parametrize("nfft,env", [(2600, {"GSDR_PFB_CU": "1"}), (3001, {}), (4096, {})], ids=["2600_forced", "3001", "4096"])
def test_single_frames_and_calls_without_a_frame(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, env):
    """buffers of one frame: four calls that only move the carry, then a frame per call, through variants 5 and 3
    (one frame of 2600 points fills too few units: the run kernel is forced there)"""
    res = run_stream(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, 4, nfft, 6, env)
    assert res["frames"] == [0, 0, 0, 0, 1, 1]
    assert all(p["cu"] == 1 and p["direct"] == (3 if nfft == 4096 else 5) for p in res["plans"])
    note(res)


@pytest.mark.parametrize("nfft,avg,spec,cut", [(128, 4, (80, 1), (23, 0)), (1024, 4, (40, 1), (20, 0)), (1000, 5, (40, 1), (23, 0)),
                                               (1018, 4, (43, 0), (10, 1))], ids=lambda v: str(v))
def test_frames_do_not_depend_on_the_run_they_were_computed_in(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, avg, spec, cut):
    """one stream, two handles that cut it into buffers of different lengths (other G, other position in the run):
    the frames both return are the model's, and each other's to twice the bar"""
    fa, fb = frames_of(spec, cus), frames_of(cut, cus)
    total = 4 * fa * nfft
    rng = np.random.default_rng(31 + nfft)
    model = _pfb.Model(oracle_mod, nfft, avg)
    stream = _pfb.tones_on_bins(rng, total, nfft, [1, nfft // 3, nfft - 2], model.w)
    got = []
    for frames in (fa, fb):
        L = frames * nfft
        # run_stream draws its own stream: feed this one through a handle by hand
        import gpu_sdr_amd as g
        for k in SWITCH_ENV:
            monkeypatch.delenv(k, raising=False)
        p = g.param(mode="RX", rate=1_000_000, buffer_len=L, decim=0, pf_average=avg, fft_tones=nfft, freq=[0], wave_type=[g.w_type.NOISE])
        dem = g.RX_buffer_demodulator(p, device_index=0)
        ys, Gs = [], set()
        for c in range(total // L):
            out = np.empty(dem.out_capacity, dtype=np.complex64)
            n = dem.process(np.ascontiguousarray(stream[c * L:(c + 1) * L]), out)
            ys.append(out[:n].reshape(-1, nfft).copy())
            Gs.add(dem.describe()["pfb_last"]["G"])
        dem.close()
        got.append((np.concatenate(ys), Gs))
    ref = _pfb.Model(oracle_mod, nfft, avg).process(stream)
    assert got[0][1] != got[1][1], "the two cuts must run other G"
    nmin = min(got[0][0].shape[0], got[1][0].shape[0])
    assert nmin >= 8
    for y, _ in got:
        e = np.linalg.norm(y - ref[:y.shape[0]], axis=0) / np.linalg.norm(ref[:y.shape[0]], axis=0)
        assert e.max() <= TOL
    e = np.linalg.norm(got[0][0][:nmin] - got[1][0][:nmin], axis=0) / np.linalg.norm(ref[:nmin], axis=0)
    assert e.max() <= 2 * TOL


TEAM_SHAPES = [(128, 4, (23, 0)), (1024, 4, (20, 0)), (600, 4, (20, 1))]


@pytest.mark.parametrize("nfft,avg,spec", TEAM_SHAPES, ids=lambda v: str(v))
def test_teams_off_against_the_default(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, avg, spec):
    """GSDR_PFB_TEAMS=0 where the default has teams on: both are the model's; whether they agree bit for bit is
    recorded, not asserted"""
    frames = frames_of(spec, cus)
    L = buffer_len(nfft, frames)
    a = run_stream(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, avg, L, 4, {}, keep=True)
    b = run_stream(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, avg, L, 4, {"GSDR_PFB_TEAMS": "0"}, keep=True)
    assert all(p["teams"] == 1 for p in a["plans"][1:]) and all(p["teams"] == 0 for p in b["plans"])
    same = all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a["out"], b["out"]))
    note(a, teams_off_bit_identical=bool(same))
    note(b)


TONES_SHAPES = [(128, 4, (80, 1)), (512, 4, (40, 1)), (1024, 4, (20, 0)), (1230, 4, (20, 1)), (1018, 4, (23, 0)), (1000, 5, (23, 0))]


@pytest.mark.parametrize("select", ["one", "all_permuted", "duplicates"])
@pytest.mark.parametrize("nfft,avg,spec", TONES_SHAPES, ids=lambda v: str(v))
def test_tones_bin_selection_in_every_run_shape(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, avg, spec, select):
    """TONES through the shapes above: one column, every bin in a permuted order, repeated bins"""
    rng = np.random.default_rng(nfft)
    bins = {"one": [nfft // 3], "all_permuted": [int(v) for v in rng.permutation(nfft)],
            "duplicates": [1, 1, nfft - 2, nfft // 3, 1, nfft - 2, 0, nfft // 2, nfft // 3]}[select]
    frames = frames_of(spec, cus)
    res = run_stream(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, avg, buffer_len(nfft, frames), 4, bins=bins)
    assert all(p["cu"] == 1 and p["G"] >= 2 for p in res["plans"][1:])
    note(res)


def test_tones_with_more_columns_than_bins_fall_to_the_frame_set_kernel(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus):
    """n_out > nfft: the run kernel's bin table holds nfft entries, pfb_lds_kernel takes the call and still matches"""
    nfft, avg = 128, 4
    bins = [int(v) for v in np.random.default_rng(3).integers(0, nfft, nfft + 5)]
    frames = frames_of((80, 1), cus)
    res = run_stream(cuda_device, gsdr_lib, oracle_mod, monkeypatch, cus, nfft, avg, buffer_len(nfft, frames), 4, bins=bins)
    assert all(p["cu"] == 0 for p in res["plans"])
    assert _pfb.plan(gsdr_lib, nfft, avg, frames, cus)["cu"] == 1           # (with nfft columns the run kernel has it)
    note(res)
