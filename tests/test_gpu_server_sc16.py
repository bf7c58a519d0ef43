"""gsdr_server --wire sc16: the software loop-back in the format a real link carries.  The TX generator hands the RX
thread sc16 buffers (gsdr_txgen_get_sc16), the demodulator takes them through gsdr_demod_submit_sc16 with its scale set
to 1 / the generator's gain; the packets on the data socket are complex64 as ever."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_parity import TOL, rel_err_per_tone
from test_gpu_server import HEADER, ROOT, connect, free_port, recv_all, recv_async, send_command
from test_sc16_tx_host import narrow_model

pytestmark = pytest.mark.gpu


@pytest.fixture()
def sc16_server(cuda_device, gsdr_lib):
    exe = os.path.join(ROOT, "gpu_sdr_amd", "gsdr_server")
    assert os.path.exists(exe), "gpu_sdr_amd/gsdr_server is built by __graft_entry__.build()"
    pa, pd = free_port(), free_port()
    proc = subprocess.Popen([exe, "--async", str(pa), "--data", str(pd), "--device", "0", "--sw_loop", "--wire", "sc16", "--once"])
    data = connect(pd)
    asyn = connect(pa)
    yield asyn, data
    asyn.close()
    data.close()
    try:
        proc.wait(timeout=20)
    except subprocess.TimeoutExpired:
        proc.kill()


def test_tones_into_direct_over_an_sc16_wire(sc16_server, oracle_mod):
    from make_commands import get_noise_direct
    import gpu_sdr_amd as g
    asyn, data = sc16_server
    rate, L, M, N, nbuf = 10_000_000, 100_000, 100, 8, 3
    tones = [-4_000_000 + 1_000_000 * k + 1234 for k in range(N)]
    cmd = get_noise_direct(tones, rate, nbuf * L / rate, M, 300e6)
    for key in ("A_TXRX", "A_RX2"):
        cmd[key]["buffer_len"] = L
    send_command(asyn, cmd)
    assert recv_async(asyn) == {"type": "ack", "payload": "Message received"}
    rows = []
    for k in range(nbuf):
        h = np.frombuffer(recv_all(data, 21), dtype=HEADER)[0]
        assert (h["usrp_number"], h["front_end_code"], h["packet_number"], h["errors"], h["channels"]) == (0, b"B", k, 0, N)
        assert h["length"] == N * (L // M)
        rows.append(np.frombuffer(recv_all(data, int(h["length"]) * 8), dtype=np.complex64).reshape(-1, N))
    reply = recv_async(asyn)
    assert reply["type"] == "ack" and "EOM" in reply["payload"]
    y = np.concatenate(rows)
    # the oracle chain with the wire in it: tone_gen -> narrow at the generator's default gain -> widen by 1 / gain -> DIRECT
    ref = oracle_mod.Direct(tones, rate, M, cmd["A_RX2"]["pf_average"], L)
    want = []
    for k in range(nbuf):
        tx = oracle_mod.tone_gen(tones, [1.0 / N] * N, rate, k * L, L)
        wire, clipped = narrow_model(tx, 32767.0)
        assert clipped == 0 and np.abs(wire).max() > 10000
        want.append(ref.process(g.widen_sc16(wire, scale=float(np.float32(1.0) / np.float32(32767.0)))))
    want = np.concatenate(want)
    assert y.shape == want.shape
    assert rel_err_per_tone(y, want).max() <= TOL
    assert np.abs(np.abs(y[8:]).mean(axis=0) - 1.0 / N).max() < 0.01 / N           # the tones arrive at their amplitude
