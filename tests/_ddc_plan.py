"""gsdr_ddc_plan for the tests: the engine of a DIRECT handle and the shape of one of its launches, asked of the library
(csrc/ddc_plan.h through host_logic.cpp: the functions the handle itself asks).  No GPU needed.  Plain module, not
collected; the library is handed in."""
import ctypes as C

from gpu_sdr_amd._lib import DdcPlanInC, DdcPlanOutC

ENGINES = ("mix", "few", "flat", "generic", "mfma")        # GSDR_DDC_ENGINE_*

# the switches gsdr_ddc_plan takes by value, with the values of an unset environment
SWITCH_DEFAULTS = {"ddc_mfma": 1, "ddc_few": 1, "ddc_pipe": 1, "ddc_k": -1, "ddc_waves": 0, "ddc_nch": 0,
                   "mfma_asm": 4, "mfma_tt": 1, "mfma_pk": 32, "mfma_w": 4, "mfma_rt": 0, "mfma_w8": 1, "mfma_prec": -1,
                   "mfma_3m": -1, "mfma_3m_rot": -1, "mfma_fold": -1, "mfma_fold_products": -1, "mfma_wave_tones": -1,
                   "mfma_span": -1}
ENV_OF_SWITCH = {k: "GSDR_" + k.upper() for k in SWITCH_DEFAULTS}
ENV_OF_SWITCH["ddc_waves"] = "GSDR_DDC_WAVES_PER_SIMD"
DESCRIBE = ("complex_mac", "rotation_blocks", "fold", "fold_products", "wave_tones", "span_samples")
OUT_FIELDS = tuple(n for n, _ in DdcPlanOutC._fields_)


def switches_of_env(env):
    """{"GSDR_MFMA_3M": "1", ...} -> the switch values gsdr_ddc_plan takes (what read_switches makes of them)"""
    sw = dict(SWITCH_DEFAULTS)
    for k, name in ENV_OF_SWITCH.items():
        if env.get(name):
            sw[k] = int(env[name])
    for k in ("ddc_mfma", "ddc_few", "ddc_pipe", "mfma_w8"):
        sw[k] = int(sw[k] != 0)
    if sw["ddc_waves"] <= 0 and env.get("GSDR_DDC_WAVES_PER_SIMD"):
        sw["ddc_waves"] = 4
    sw["mfma_tt"] = 2 if sw["mfma_tt"] == 2 else 1
    sw["mfma_pk"] = 16 if sw["mfma_pk"] == 16 else 32
    sw["mfma_w"] = 2 if sw["mfma_w"] == 2 else 4
    if not 0 <= sw["mfma_rt"] <= 2:
        sw["mfma_rt"] = 0
    return sw


def plan(lib, N, M, F, L, rows=0, overlapped=False, cus=256, env=None, rate=1_000_000):
    """The plan as a dict (None: gsdr_ddc_plan refuses the arguments); "engine" by name, "describe" the six values in
    the order of DESCRIBE."""
    sw = switches_of_env(env or {})
    a = DdcPlanInC(decim=M, pf_average=F, buffer_len=L, tones=N, rate=rate, rows=rows, overlapped=int(overlapped), cus=cus, **sw)
    out = DdcPlanOutC()
    if lib.gsdr_ddc_plan(C.byref(a), C.byref(out)) != 0:
        return None
    d = {k: int(getattr(out, k)) for k in OUT_FIELDS}
    d["engine"] = ENGINES[d["engine"]]
    d["describe"] = tuple(d[k] for k in DESCRIBE)
    return d


def describe_matches_plan(d, p):
    """describe() of a DIRECT handle after a call against the plan of that call: the kernel family, the six values
    and the row tiles per workgroup."""
    if p["engine"] != "mfma":
        want = {"few": "ddc_few_kernel", "flat": "ddc_flat_kernel", "generic": "ddc_kernel"}.get(p["engine"])
        assert want is None or d["kernel"] == want, (d, p)
        assert not d["kernel"].startswith("ddc_mfma"), (d, p)
        assert d["row_tiles_per_workgroup"] == 0, (d, p)
        assert tuple(d[k] for k in DESCRIBE) == (4, 1, 0, 0, 32, 64), (d, p)
        return
    assert d["family"] == "f16 MFMA, hi/lo split", (d, p)
    assert tuple(d[k] for k in DESCRIBE) == p["describe"], (d, p)
    assert d["row_tiles_per_workgroup"] == p["row_tiles_per_workgroup"], (d, p)
    assert (d["kernel"] == "ddc_mfma_ring16p_kernel") == bool(p["preconverted"]), (d, p)
    assert (d["kernel"] == "ddc_mfma_ring16w8_kernel") == bool(p["eight_waves"]), (d, p)
    for k in ("complex_mac_min_blocks", "rotation_min_blocks", "fold_min_blocks", "span128_min_blocks"):
        assert d[k] == p[k], (k, d, p)
