"""Every refusal of five of the six row-stage objects (gsdr_trigger_*, gsdr_welch_*, gsdr_decim_*, gsdr_sweep_*,
gsdr_resmap_*; those of gsdr_stats_*: tests/test_stats_host.py) that returns before the first HIP call: the return value and the exact bytes gsdr_last_error(NULL) gives afterwards, in
the manner of tests/test_entry_refusals.py.  No GPU call is made: every object below is a host twin, and no call passes
every check of a device entry.  The one text libgsdr.so cannot give -- "this build has host objects only", the answer
of a build without a device part -- is pinned for all six by a stand-alone program built from the host sources alone
(host_logic.cpp and the X_host.cpp: tests/_sanitized.py)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from _sanitized import HOST_SOURCES
from gpu_sdr_amd._lib import ChirpParamC, TriggerLevelC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = -2                      # GSDR_TRIGGER_HOST, _WELCH_, _DECIM_, _SWEEP_, _RESMAP_
PLANTED = b"null parameters"
# never dereferenced: each is used only where an earlier check refuses the call
PTR = 0x1000
M = 1 << 20
NAN, INF = float("nan"), float("inf")


def last_error(lib):
    return lib.gsdr_last_error(None)


def plant(lib):
    """Leaves a known message behind: the next refusal must replace it (or, where it is silent, keep it)."""
    assert lib.gsdr_txgen_create(None, None, 0) is None
    assert last_error(lib) == PLANTED


def refused(lib, call, rc, msg):
    plant(lib)
    assert call() == rc
    assert last_error(lib) == msg


def silent(lib, call, rc):
    plant(lib)
    assert call() == rc
    assert last_error(lib) == PLANTED


def floats(*v):
    return (C.c_float * len(v))(*v)


def doubles(*v):
    return (C.c_double * len(v))(*v)


def ints(*v):
    return (C.c_int * len(v))(*v)


KEPT = []


def addr(a):
    """The address of a ctypes array that stays alive as long as this module does."""
    KEPT.append(a)
    return C.addressof(a)


# ---- trigger -------------------------------------------------------------------------------------------------------

LEVELS = (TriggerLevelC * 2)()
TRIGGER_OK = dict(n_ch=2, max_rows=8, pre=1, post=2, holdoff=0, max_events=4, levels=addr(LEVELS), device_index=HOST)
TRIGGER_CREATE = [
    (dict(n_ch=0), b"n_ch must be in [1, 1048576]"),
    (dict(n_ch=M + 1), b"n_ch must be in [1, 1048576]"),
    (dict(max_rows=0), b"max_rows must be in [1, 1048576]"),
    (dict(max_rows=M + 1), b"max_rows must be in [1, 1048576]"),
    (dict(pre=-1), b"pre must be >= 0"),
    (dict(post=0), b"post must be >= 1"),
    (dict(pre=65536, post=1), b"pre + post must be <= 65536"),
    (dict(holdoff=-1), b"holdoff must be in [0, 1073741824]"),
    (dict(holdoff=(1 << 30) + 1), b"holdoff must be in [0, 1073741824]"),
    (dict(max_events=0), b"max_events must be in [1, 1048576]"),
    (dict(max_events=M + 1), b"max_events must be in [1, 1048576]"),
    (dict(levels=None), b"levels must not be NULL"),
    (dict(device_index=-3), b"device_index must be >= -1 or GSDR_TRIGGER_HOST"),
    # the order of the checks decides the message of a doubly wrong request
    (dict(levels=None, device_index=-3), b"levels must not be NULL"),
]


def trigger_create(lib, **over):
    a = dict(TRIGGER_OK, **over)
    return lib.gsdr_trigger_create(a["n_ch"], a["max_rows"], a["pre"], a["post"], a["holdoff"], a["max_events"], a["levels"],
                                   a["device_index"])


@pytest.mark.parametrize("over,msg", TRIGGER_CREATE, ids=[",".join(c[0]) + "=" + str(list(c[0].values())[0]) for c in TRIGGER_CREATE])
def test_trigger_create_refusals(gsdr_lib, over, msg):
    refused(gsdr_lib, lambda: trigger_create(gsdr_lib, **over), None, b"gsdr_trigger_create: " + msg)


def test_trigger_null_object(gsdr_lib):
    L = gsdr_lib
    refused(L, lambda: L.gsdr_trigger_set_levels(None, addr(LEVELS), None), -1, b"gsdr_trigger_set_levels: null argument")
    refused(L, lambda: L.gsdr_trigger_reset(None), -1, b"gsdr_trigger_reset: null object")
    refused(L, lambda: L.gsdr_trigger_feed_host(None, PTR, 1, PTR, PTR, None), -1, b"gsdr_trigger_feed_host: null object")
    refused(L, lambda: L.gsdr_trigger_feed_device(None, PTR, 1, PTR, PTR, PTR, None), -1, b"gsdr_trigger_feed_device: null object")
    refused(L, lambda: L.gsdr_trigger_feed(None, PTR, 1, PTR, PTR, None, None), -1, b"gsdr_trigger_feed: null object")
    silent(L, lambda: L.gsdr_trigger_rows(None), 0)
    silent(L, lambda: L.gsdr_trigger_close(None), None)


def test_trigger_host_object(gsdr_lib):
    L = gsdr_lib
    t = trigger_create(L)
    assert t
    try:
        refused(L, lambda: L.gsdr_trigger_set_levels(t, None, None), -1, b"gsdr_trigger_set_levels: null argument")
        hint = b": a host object (GSDR_TRIGGER_HOST) takes gsdr_trigger_feed_host"
        refused(L, lambda: L.gsdr_trigger_feed_device(t, PTR, 1, PTR, PTR, PTR, None), -1, b"gsdr_trigger_feed_device" + hint)
        refused(L, lambda: L.gsdr_trigger_feed(t, PTR, 1, PTR, PTR, None, None), -1, b"gsdr_trigger_feed" + hint)
        for n in (-1, 9):
            refused(L, lambda: L.gsdr_trigger_feed_host(t, PTR, n, PTR, PTR, None), -1, b"gsdr_trigger_feed_host: n_rows must be in [0, max_rows]")
        for rows, ev, sn in ((None, PTR, PTR), (PTR, None, PTR), (PTR, PTR, None)):
            refused(L, lambda: L.gsdr_trigger_feed_host(t, rows, 1, ev, sn, None), -1, b"gsdr_trigger_feed_host: null buffer")
        silent(L, lambda: L.gsdr_trigger_feed_host(t, None, 0, None, None, None), 0)      # an empty feed touches nothing
    finally:
        L.gsdr_trigger_close(t)


# ---- welch ---------------------------------------------------------------------------------------------------------

WELCH_OK = dict(n_ch=2, max_rows=64, nperseg=16, step=8, detrend=2, window=None, device_index=HOST)
WELCH_CREATE = [
    (dict(n_ch=0), b"n_ch must be in [1, 1048576]"),
    (dict(n_ch=M + 1), b"n_ch must be in [1, 1048576]"),
    (dict(max_rows=0), b"max_rows must be in [1, 1048576]"),
    (dict(max_rows=M + 1), b"max_rows must be in [1, 1048576]"),
    (dict(nperseg=8, step=8), b"nperseg must be a power of two in [16, 8192]"),
    (dict(nperseg=16384, step=8192), b"nperseg must be a power of two in [16, 8192]"),
    (dict(nperseg=48, step=24), b"nperseg must be a power of two in [16, 8192]"),
    (dict(step=1), b"step must be in [nperseg / 8, nperseg]"),
    (dict(step=17), b"step must be in [nperseg / 8, nperseg]"),
    (dict(detrend=3), b"detrend must be GSDR_WELCH_DETREND_NONE, _CONSTANT or _LINEAR"),
    (dict(detrend=-1), b"detrend must be GSDR_WELCH_DETREND_NONE, _CONSTANT or _LINEAR"),
    (dict(device_index=-3), b"device_index must be >= -1 or GSDR_WELCH_HOST"),
    (dict(detrend=3, device_index=-3), b"detrend must be GSDR_WELCH_DETREND_NONE, _CONSTANT or _LINEAR"),
]


def welch_create(lib, **over):
    a = dict(WELCH_OK, **over)
    return lib.gsdr_welch_create(a["n_ch"], a["max_rows"], a["nperseg"], a["step"], a["detrend"], a["window"], a["device_index"])


@pytest.mark.parametrize("over,msg", WELCH_CREATE, ids=[",".join(c[0]) + "=" + str(list(c[0].values())[0]) for c in WELCH_CREATE])
def test_welch_create_refusals(gsdr_lib, over, msg):
    refused(gsdr_lib, lambda: welch_create(gsdr_lib, **over), None, b"gsdr_welch_create: " + msg)


def test_welch_null_object(gsdr_lib):
    L = gsdr_lib
    refused(L, lambda: L.gsdr_welch_reset(None), -1, b"gsdr_welch_reset: null object")
    refused(L, lambda: L.gsdr_welch_feed_host(None, PTR, 1), -1, b"gsdr_welch_feed_host: null object")
    refused(L, lambda: L.gsdr_welch_read_host(None, 0, None, 1.0, PTR, None), -1, b"gsdr_welch_read_host: null object")
    refused(L, lambda: L.gsdr_welch_feed_device(None, PTR, 1, None), -1, b"gsdr_welch_feed_device: null object")
    refused(L, lambda: L.gsdr_welch_read_device(None, 0, None, 1.0, PTR, None), -1, b"gsdr_welch_read_device: null object")
    refused(L, lambda: L.gsdr_welch_mean_device(None, PTR, None), -1, b"gsdr_welch_mean_device: null object")
    refused(L, lambda: L.gsdr_welch_read(None, 0, None, 1.0, PTR, None, None), -1, b"gsdr_welch_read: null object")
    silent(L, lambda: L.gsdr_welch_rows(None), 0)
    silent(L, lambda: L.gsdr_welch_segments(None), 0)
    silent(L, lambda: L.gsdr_welch_close(None), None)


def test_welch_host_object(gsdr_lib):
    L = gsdr_lib
    w = welch_create(L)
    assert w
    try:
        hint = b": a host object (GSDR_WELCH_HOST) takes gsdr_welch_feed_host / gsdr_welch_read_host"
        refused(L, lambda: L.gsdr_welch_feed_device(w, PTR, 1, None), -1, b"gsdr_welch_feed_device" + hint)
        refused(L, lambda: L.gsdr_welch_read_device(w, 0, None, 1.0, PTR, None), -1, b"gsdr_welch_read_device" + hint)
        refused(L, lambda: L.gsdr_welch_mean_device(w, PTR, None), -1, b"gsdr_welch_mean_device" + hint)
        refused(L, lambda: L.gsdr_welch_read(w, 0, None, 1.0, PTR, None, None), -1, b"gsdr_welch_read" + hint)
        for n in (-1, 65):
            refused(L, lambda: L.gsdr_welch_feed_host(w, PTR, n), -1, b"gsdr_welch_feed_host: n_rows must be in [0, max_rows]")
        refused(L, lambda: L.gsdr_welch_feed_host(w, None, 1), -1, b"gsdr_welch_feed_host: null buffer: rows")
        silent(L, lambda: L.gsdr_welch_feed_host(w, None, 0), 0)
        for mode in (-1, 4):
            refused(L, lambda: L.gsdr_welch_read_host(w, mode, None, 1.0, PTR, None), -1,
                    b"gsdr_welch_read_host: mode must be GSDR_WELCH_RAW, _ROTATE, _DBC or _GAIN")
        for fs in (0.0, -1.0, NAN, INF):
            refused(L, lambda: L.gsdr_welch_read_host(w, 0, None, fs, PTR, None), -1, b"gsdr_welch_read_host: fs must be finite and > 0")
        refused(L, lambda: L.gsdr_welch_read_host(w, 3, None, 1.0, PTR, None), -1,
                b"gsdr_welch_read_host: gain must not be NULL with GSDR_WELCH_GAIN")
        refused(L, lambda: L.gsdr_welch_read_host(w, 0, None, 1.0, None, None), -1, b"gsdr_welch_read_host: null buffer: psd")
        silent(L, lambda: L.gsdr_welch_read_host(w, 0, None, 1.0, PTR, None), 0)          # no segment yet: nothing is written
    finally:
        L.gsdr_welch_close(w)


# ---- decim ---------------------------------------------------------------------------------------------------------

TAPS3 = floats(0.25, 0.5, 0.25)
DECIM_OK = dict(n_ch=2, max_rows=8, q=2, n_taps=3, taps=addr(TAPS3), offset=0, device_index=HOST)
DECIM_CREATE = [
    (dict(n_ch=0), b"n_ch must be in [1, 1048576]"),
    (dict(n_ch=M + 1), b"n_ch must be in [1, 1048576]"),
    (dict(max_rows=0), b"max_rows must be in [1, 1048576]"),
    (dict(max_rows=M + 1), b"max_rows must be in [1, 1048576]"),
    (dict(q=0), b"q must be in [1, 4096]"),
    (dict(q=4097), b"q must be in [1, 4096]"),
    (dict(taps=None), b"taps must not be NULL with n_taps != 0 (NULL and 0 select the default taps)"),
    (dict(taps=None, n_taps=0, q=1), b"q must be >= 2 for the default taps (taps == NULL)"),
    (dict(n_taps=0), b"n_taps must be in [1, 64 q]"),
    (dict(n_taps=129), b"n_taps must be in [1, 64 q]"),
    (dict(offset=-1), b"offset must be in [0, 1073741824]"),
    (dict(offset=(1 << 30) + 1), b"offset must be in [0, 1073741824]"),
    (dict(device_index=-3), b"device_index must be >= -1 or GSDR_DECIM_HOST"),
    (dict(taps=addr(floats(0.5, NAN, 0.5))), b"taps must all be finite"),
    (dict(taps=addr(floats(0.5, 0.5, INF))), b"taps must all be finite"),
    # the taps are looked at last
    (dict(taps=addr(floats(NAN, 0.5, 0.5)), device_index=-3), b"device_index must be >= -1 or GSDR_DECIM_HOST"),
]


def decim_create(lib, **over):
    a = dict(DECIM_OK, **over)
    return lib.gsdr_decim_create(a["n_ch"], a["max_rows"], a["q"], a["n_taps"], a["taps"], a["offset"], a["device_index"])


@pytest.mark.parametrize("over,msg", DECIM_CREATE, ids=[f"{i}:" + ",".join(c[0]) for i, c in enumerate(DECIM_CREATE)])
def test_decim_create_refusals(gsdr_lib, over, msg):
    refused(gsdr_lib, lambda: decim_create(gsdr_lib, **over), None, b"gsdr_decim_create: " + msg)


def test_decim_null_object(gsdr_lib):
    L = gsdr_lib
    refused(L, lambda: L.gsdr_decim_reset(None), -1, b"gsdr_decim_reset: null object")
    refused(L, lambda: L.gsdr_decim_feed_host(None, PTR, 1, PTR), -1, b"gsdr_decim_feed_host: null object")
    refused(L, lambda: L.gsdr_decim_feed_device(None, PTR, 1, PTR, None), -1, b"gsdr_decim_feed_device: null object")
    refused(L, lambda: L.gsdr_decim_feed(None, PTR, 1, PTR, None), -1, b"gsdr_decim_feed: null object")
    silent(L, lambda: L.gsdr_decim_next_rows(None, 1), 0)
    silent(L, lambda: L.gsdr_decim_out_capacity(None), 0)
    silent(L, lambda: L.gsdr_decim_get_taps(None, None, 0), 0)
    silent(L, lambda: L.gsdr_decim_rows(None), 0)
    silent(L, lambda: L.gsdr_decim_rows_out(None), 0)
    silent(L, lambda: L.gsdr_decim_close(None), None)
    for q in (1, 4097):
        silent(L, lambda: L.gsdr_decim_default_taps(q, floats(0.0)), -1)
    silent(L, lambda: L.gsdr_decim_default_taps(2, None), -1)


def test_decim_host_object(gsdr_lib):
    L = gsdr_lib
    d = decim_create(L)
    assert d
    try:
        hint = b": a host object (GSDR_DECIM_HOST) takes gsdr_decim_feed_host"
        refused(L, lambda: L.gsdr_decim_feed_device(d, PTR, 1, PTR, None), -1, b"gsdr_decim_feed_device" + hint)
        refused(L, lambda: L.gsdr_decim_feed(d, PTR, 1, PTR, None), -1, b"gsdr_decim_feed" + hint)
        for n in (-1, 9):
            refused(L, lambda: L.gsdr_decim_next_rows(d, n), -1, b"gsdr_decim_next_rows: n_rows must be in [0, max_rows]")
            refused(L, lambda: L.gsdr_decim_feed_host(d, PTR, n, PTR), -1, b"gsdr_decim_feed_host: n_rows must be in [0, max_rows]")
        refused(L, lambda: L.gsdr_decim_feed_host(d, None, 1, PTR), -1, b"gsdr_decim_feed_host: null buffer: rows")
        assert L.gsdr_decim_next_rows(d, 1) == 1                  # offset 0: the first row completes an output row
        rows = floats(*([0.0] * 4))
        refused(L, lambda: L.gsdr_decim_feed_host(d, addr(rows), 1, None), -1, b"gsdr_decim_feed_host: null buffer: out")
        silent(L, lambda: L.gsdr_decim_feed_host(d, None, 0, None), 0)
    finally:
        L.gsdr_decim_close(d)


# ---- sweep ---------------------------------------------------------------------------------------------------------

SWEEP_OK = dict(n_ch=2, n_points=4, group=1, first_row=0, device_index=HOST)
SWEEP_CREATE = [
    (dict(n_ch=0), b"n_ch must be in [1, 1048576]"),
    (dict(n_ch=M + 1), b"n_ch must be in [1, 1048576]"),
    (dict(n_points=0), b"n_points must be in [1, 16777216]"),
    (dict(n_points=(1 << 24) + 1), b"n_points must be in [1, 16777216]"),
    (dict(n_points=1 << 24, n_ch=3), b"n_points * n_ch must be <= 33554432 (32 bytes each)"),
    (dict(group=0), b"group must be in [1, 1073741824]"),
    (dict(group=(1 << 30) + 1), b"group must be in [1, 1073741824]"),
    (dict(first_row=-1), b"first_row must be in [0, 2^62]"),
    (dict(first_row=(1 << 62) + 1), b"first_row must be in [0, 2^62]"),
    (dict(device_index=-3), b"device_index must be >= -1 or GSDR_SWEEP_HOST"),
    (dict(first_row=-1, device_index=-3), b"first_row must be in [0, 2^62]"),
]


def sweep_create(lib, **over):
    a = dict(SWEEP_OK, **over)
    return lib.gsdr_sweep_create(a["n_ch"], a["n_points"], a["group"], a["first_row"], a["device_index"])


@pytest.mark.parametrize("over,msg", SWEEP_CREATE, ids=[",".join(c[0]) + "=" + str(list(c[0].values())[0]) for c in SWEEP_CREATE])
def test_sweep_create_refusals(gsdr_lib, over, msg):
    refused(gsdr_lib, lambda: sweep_create(gsdr_lib, **over), None, b"gsdr_sweep_create: " + msg)


def test_sweep_null_object(gsdr_lib):
    L = gsdr_lib
    refused(L, lambda: L.gsdr_sweep_reset(None, 0), -1, b"gsdr_sweep_reset: null object")
    refused(L, lambda: L.gsdr_sweep_feed_host(None, PTR, 1), -1, b"gsdr_sweep_feed_host: null object")
    refused(L, lambda: L.gsdr_sweep_read_host(None, PTR, None), -1, b"gsdr_sweep_read_host: null object")
    refused(L, lambda: L.gsdr_sweep_slope(None, PTR, None), -1, b"gsdr_sweep_slope: null object")
    refused(L, lambda: L.gsdr_sweep_feed_device(None, PTR, 1, None), -1, b"gsdr_sweep_feed_device: null object")
    refused(L, lambda: L.gsdr_sweep_read_device(None, PTR, None, None), -1, b"gsdr_sweep_read_device: null object")
    refused(L, lambda: L.gsdr_sweep_read(None, PTR, None, None), -1, b"gsdr_sweep_read: null object")
    silent(L, lambda: L.gsdr_sweep_rows(None), 0)
    silent(L, lambda: L.gsdr_sweep_sweeps(None), 0)
    silent(L, lambda: L.gsdr_sweep_point_rows(None, 0), 0)
    silent(L, lambda: L.gsdr_sweep_close(None), None)


def test_sweep_host_object(gsdr_lib):
    L = gsdr_lib
    s = sweep_create(L)
    assert s
    try:
        hint = b": a host object (GSDR_SWEEP_HOST) takes gsdr_sweep_feed_host and gsdr_sweep_read_host"
        refused(L, lambda: L.gsdr_sweep_feed_device(s, PTR, 1, None), -1, b"gsdr_sweep_feed_device" + hint)
        refused(L, lambda: L.gsdr_sweep_read_device(s, PTR, None, None), -1, b"gsdr_sweep_read_device" + hint)
        refused(L, lambda: L.gsdr_sweep_read(s, PTR, None, None), -1, b"gsdr_sweep_read" + hint)
        for first_row in (-1, (1 << 62) + 1):
            refused(L, lambda: L.gsdr_sweep_reset(s, first_row), -1, b"gsdr_sweep_reset: first_row must be in [0, 2^62]")
        for n in (-1, (1 << 24) + 1):
            refused(L, lambda: L.gsdr_sweep_feed_host(s, PTR, n), -1, b"gsdr_sweep_feed_host: n_rows must be in [0, 16777216]")
        refused(L, lambda: L.gsdr_sweep_feed_host(s, None, 1), -1, b"gsdr_sweep_feed_host: null buffer: rows")
        silent(L, lambda: L.gsdr_sweep_feed_host(s, None, 0), 0)
        refused(L, lambda: L.gsdr_sweep_read_host(s, None, None), -1, b"gsdr_sweep_read_host: null buffer: mean")
        refused(L, lambda: L.gsdr_sweep_slope(s, None, None), -1, b"gsdr_sweep_slope: null buffer: d_host")
        silent(L, lambda: L.gsdr_sweep_point_rows(s, -1), 0)
        silent(L, lambda: L.gsdr_sweep_point_rows(s, 4), 0)
    finally:
        L.gsdr_sweep_close(s)


def test_sweep_shape_for_chirp_refusals(gsdr_lib):
    L = gsdr_lib
    me = b"gsdr_sweep_shape_for_chirp: "
    np_, g = C.c_longlong(0), C.c_longlong(0)

    def call(cp, decim, n_points=np_, group=g):
        return lambda: L.gsdr_sweep_shape_for_chirp(None if cp is None else C.byref(cp), decim, None if n_points is None else C.byref(n_points),
                                                    None if group is None else C.byref(group))

    cp = ChirpParamC(10, 35, 1000, 0)
    refused(L, call(None, 0), -1, me + b"null pointer")
    refused(L, call(cp, 0, n_points=None), -1, me + b"null pointer")
    refused(L, call(cp, 0, group=None), -1, me + b"null pointer")
    refused(L, call(cp, -1), -1, me + b"decim must be >= 0")
    for bad in (ChirpParamC(0, 35, 0, 0), ChirpParamC(10, 0, 0, 0), ChirpParamC(1 << 40, 1 << 40, 0, 0)):
        refused(L, call(bad, 0), -1, me + b"cp: num_steps and length must be >= 1, their product <= 2^62")
    for bad in (ChirpParamC((1 << 24) + 1, 1, 0, 0), ChirpParamC(1, (1 << 30) + 1, 0, 0)):
        refused(L, call(bad, 0), -1, me + b"cp: num_steps > 2^24 or length > 2^30 (the limits of gsdr_sweep_create)")
    refused(L, call(cp, 11), -1, me + b"decim: a row of length * decim samples is longer than the period")
    refused(L, call(cp, 3), -1,
            me + b"decim: length * decim does not divide the period num_steps * length, the points do not repeat from sweep to sweep")
    refused(L, call(ChirpParamC(1 << 25, 1, 0, 0), 1), -1, me + b"cp, decim: more than 2^24 points")


def test_vna_axis_refusals(gsdr_lib):
    L = gsdr_lib
    f = doubles(0.0, 0.0)
    refused(L, lambda: L.gsdr_vna_axis(1e6, 0.0, 1e5, 10.0, 2, 0.0, None), -1, b"gsdr_vna_axis: null buffer: f")
    for swipe_s in (1.0, NAN):
        refused(L, lambda: L.gsdr_vna_axis(1e6, 0.0, 1e5, swipe_s, 2, 0.0, f), -1, b"gsdr_vna_axis: swipe_s must be >= 2")
    refused(L, lambda: L.gsdr_vna_axis(1e6, 0.0, 1e5, 10.0, 0, 0.0, f), -1, b"gsdr_vna_axis: n_points must be >= 1")
    for rate in (0.0, -1.0, NAN):
        refused(L, lambda: L.gsdr_vna_axis(rate, 0.0, 1e5, 10.0, 2, 0.0, f), -1, b"gsdr_vna_axis: rate must be > 0")


# ---- resmap --------------------------------------------------------------------------------------------------------

CONSTANTS2 = doubles(*([1.0] * 14))
CHANNELS2 = ints(0, 1)
RESMAP_OK = dict(n_ch=2, max_rows=8, n_out=2, channels=None, constants=addr(CONSTANTS2), kind=1, device_index=HOST)
RESMAP_CREATE = [
    (dict(n_ch=0), b"n_ch must be in [1, 1048576]"),
    (dict(n_ch=M + 1), b"n_ch must be in [1, 1048576]"),
    (dict(max_rows=0), b"max_rows must be in [1, 1048576]"),
    (dict(max_rows=M + 1), b"max_rows must be in [1, 1048576]"),
    (dict(n_out=0), b"n_out must be in [1, 1048576]"),
    (dict(n_out=M + 1), b"n_out must be in [1, 1048576]"),
    (dict(n_out=1), b"channels must not be NULL with n_out != n_ch (NULL is the identity)"),
    (dict(constants=None), b"constants must not be NULL"),
    (dict(kind=-1), b"kind must be GSDR_RESMAP_CAL, GSDR_RESMAP_X_DQR or GSDR_RESMAP_X_QR"),
    (dict(kind=3), b"kind must be GSDR_RESMAP_CAL, GSDR_RESMAP_X_DQR or GSDR_RESMAP_X_QR"),
    (dict(device_index=-3), b"device_index must be >= -1 or GSDR_RESMAP_HOST"),
    (dict(channels=addr(ints(0, 2))), b"channels must all be in [0, n_ch)"),
    (dict(channels=addr(ints(-1, 0))), b"channels must all be in [0, n_ch)"),
    (dict(constants=addr(doubles(*([1.0] * 13 + [NAN])))), b"constants must all be finite"),
    (dict(constants=addr(doubles(*([INF] + [1.0] * 13)))), b"constants must all be finite"),
    # the tables are looked at last, the channels before the constants
    (dict(channels=addr(ints(0, 2)), device_index=-3), b"device_index must be >= -1 or GSDR_RESMAP_HOST"),
    (dict(channels=addr(ints(0, 2)), constants=addr(doubles(*([NAN] * 14)))), b"channels must all be in [0, n_ch)"),
]


def resmap_create(lib, **over):
    a = dict(RESMAP_OK, **over)
    return lib.gsdr_resmap_create(a["n_ch"], a["max_rows"], a["n_out"], a["channels"], a["constants"], a["kind"], a["device_index"])


@pytest.mark.parametrize("over,msg", RESMAP_CREATE, ids=[f"{i}:" + ",".join(c[0]) for i, c in enumerate(RESMAP_CREATE)])
def test_resmap_create_refusals(gsdr_lib, over, msg):
    refused(gsdr_lib, lambda: resmap_create(gsdr_lib, **over), None, b"gsdr_resmap_create: " + msg)


def test_resmap_constants_refusals(gsdr_lib):
    L = gsdr_lib
    out = doubles(*([0.0] * 7))
    ok = dict(f_tone=1e8, f0=100.0, A=1.0, phi=0.0, D=0.0, Qe_re=1e4, Qe_im=0.0)
    cases = [(dict(f_tone=NAN), b"f_tone must be finite"), (dict(f0=INF), b"f0 must be finite and > 0 (MHz)"),
             (dict(f0=0.0), b"f0 must be finite and > 0 (MHz)"), (dict(A=NAN), b"A must be finite and > 0"),
             (dict(A=-1.0), b"A must be finite and > 0"), (dict(phi=INF), b"phi must be finite"), (dict(D=NAN), b"D must be finite"),
             (dict(Qe_re=INF), b"Qe_re must be finite"), (dict(Qe_im=NAN), b"Qe_im must be finite"),
             (dict(Qe_re=0.0, Qe_im=0.0), b"Qe_re and Qe_im: Qe must not be 0")]
    for over, msg in cases:
        a = dict(ok, **over)
        refused(L, lambda: L.gsdr_resmap_constants(*a.values(), out), -1, b"gsdr_resmap_constants: " + msg)
    refused(L, lambda: L.gsdr_resmap_constants(*ok.values(), None), -1, b"gsdr_resmap_constants: constants must not be NULL")


def test_resmap_null_object(gsdr_lib):
    L = gsdr_lib
    refused(L, lambda: L.gsdr_resmap_set_offsets(None, None, None), -1, b"gsdr_resmap_set_offsets: null object")
    refused(L, lambda: L.gsdr_resmap_feed_host(None, PTR, 1, PTR), -1, b"gsdr_resmap_feed_host: null object")
    refused(L, lambda: L.gsdr_resmap_feed_device(None, PTR, 1, PTR, None), -1, b"gsdr_resmap_feed_device: null object")
    refused(L, lambda: L.gsdr_resmap_feed(None, PTR, 1, PTR, None), -1, b"gsdr_resmap_feed: null object")
    silent(L, lambda: L.gsdr_resmap_n_out(None), 0)
    silent(L, lambda: L.gsdr_resmap_kind(None), 0)
    silent(L, lambda: L.gsdr_resmap_get_constants(None, None, 0), 0)
    silent(L, lambda: L.gsdr_resmap_get_offsets(None, None, 0), 0)
    silent(L, lambda: L.gsdr_resmap_get_channels(None, None, 0), 0)
    silent(L, lambda: L.gsdr_resmap_close(None), None)


def test_resmap_host_object(gsdr_lib):
    L = gsdr_lib
    r = resmap_create(L)
    swapped = resmap_create(L, channels=addr(ints(1, 0)))
    assert r and swapped
    try:
        hint = b": a host object (GSDR_RESMAP_HOST) takes gsdr_resmap_feed_host"
        refused(L, lambda: L.gsdr_resmap_feed_device(r, PTR, 1, PTR, None), -1, b"gsdr_resmap_feed_device" + hint)
        refused(L, lambda: L.gsdr_resmap_feed(r, PTR, 1, PTR, None), -1, b"gsdr_resmap_feed" + hint)
        for xy in (doubles(0.0, NAN, 0.0, 0.0), doubles(0.0, 0.0, 0.0, INF)):
            refused(L, lambda: L.gsdr_resmap_set_offsets(r, addr(xy), None), -1, b"gsdr_resmap_set_offsets: xy must all be finite")
        silent(L, lambda: L.gsdr_resmap_set_offsets(r, None, None), 0)                   # NULL: zeros
        for n in (-1, 9):
            refused(L, lambda: L.gsdr_resmap_feed_host(r, PTR, n, PTR), -1, b"gsdr_resmap_feed_host: n_rows must be in [0, max_rows]")
        refused(L, lambda: L.gsdr_resmap_feed_host(r, None, 1, PTR), -1, b"gsdr_resmap_feed_host: null buffer: rows")
        refused(L, lambda: L.gsdr_resmap_feed_host(r, PTR, 1, None), -1, b"gsdr_resmap_feed_host: null buffer: out")
        silent(L, lambda: L.gsdr_resmap_feed_host(r, None, 0, None), 0)
        overlap = b"gsdr_resmap_feed_host: out overlaps rows (out == rows is allowed with the identity channel list only)"
        refused(L, lambda: L.gsdr_resmap_feed_host(r, PTR, 1, PTR + 8), -1, overlap)
        refused(L, lambda: L.gsdr_resmap_feed_host(swapped, PTR, 1, PTR), -1, overlap)
    finally:
        L.gsdr_resmap_close(r)
        L.gsdr_resmap_close(swapped)


# ---- a build without a device part ---------------------------------------------------------------------------------

HOST_ONLY_DRIVER = r'''
#include <cstdio>
#include <string>
#include "gsdr.h"

static std::string noted;
extern "C" void gsdr_note_error_(const char *msg) { noted = msg ? msg : ""; }

int main() {
    const gsdr_trigger_level levels[2] = {};
    const gsdr_trigger_level axes[2] = {{0.f, 0.f, 1.f, 0.f, -1.f, 1.f}, {0.f, 0.f, 1.f, 0.f, -1.f, 1.f}};
    const float taps[3] = {0.25f, 0.5f, 0.25f};
    double constants[2 * GSDR_RESMAP_NCONST];
    for (double &c : constants) c = 1.0;
    for (int device_index = -1; device_index <= 0; ++device_index) {
        void *made[6] = {gsdr_trigger_create(2, 8, 1, 2, 0, 4, levels, device_index), nullptr, nullptr, nullptr, nullptr, nullptr};
        std::printf("%s\n", noted.c_str());
        made[1] = gsdr_welch_create(2, 64, 16, 8, 2, nullptr, device_index);
        std::printf("%s\n", noted.c_str());
        made[2] = gsdr_decim_create(2, 8, 2, 3, taps, 0, device_index);
        std::printf("%s\n", noted.c_str());
        made[3] = gsdr_sweep_create(2, 4, 1, 0, device_index);
        std::printf("%s\n", noted.c_str());
        made[4] = gsdr_resmap_create(2, 8, 2, nullptr, constants, GSDR_RESMAP_X_DQR, device_index);
        std::printf("%s\n", noted.c_str());
        made[5] = gsdr_stats_create(2, 8, 4, 0, axes, device_index);
        std::printf("%s\n", noted.c_str());
        for (void *m : made)
            if (m) return 1;
    }
    return 0;
}
'''
HOST_ONLY_LINES = ["gsdr_%s_create: device_index: this build has host objects only (GSDR_%s_HOST)" % (s, s.upper())
                   for s in ("trigger", "welch", "decim", "sweep", "resmap", "stats")] * 2


def test_create_refusal_of_a_build_without_a_device_part(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    (tmp_path / "driver.cpp").write_text(HOST_ONLY_DRIVER)
    exe = tmp_path / "driver"
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(tmp_path / "driver.cpp"), *HOST_SOURCES, "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.splitlines() == HOST_ONLY_LINES
