"""describe() of a DIRECT handle after a call is what gsdr_ddc_plan says of that call on this device: the kernel
family, the six values of the product loop and the row tiles per workgroup -- the handle and the exported function ask
the same rules (csrc/ddc_plan.h), and tests/test_ddc_plan_host.py pins those.  Modelled on pfb_last_is_the_plan of
tests/test_gpu_parity.py.

Windows of 93 / 94 / 124 / 125 blocks of 32 samples (F = 4, M = 8 T: the thresholds of the product loops lie between)
in buffers of 34 rows (two row tiles, the second of two rows), 64 / 65 / 288 tones (one and two tone waves; nine tone
groups, the wide tile's shape), with no switch set and under every row of tests/_product_loops.py::LOOPS; one in-order
call, then one through submit_device.  What the calls compute is the other tests' business.
"""
import numpy as np
import pytest

import _ddc_plan
from _product_loops import LOOPS
from test_gpu_extents import clean_env
from test_gpu_parity import crandn, cuda_device_cus, make_direct

pytestmark = pytest.mark.gpu

RATE, F, ROWS = 200_000_000, 4, 34
ENVS = dict({"unforced": {}}, **{name: env for name, (env, _) in LOOPS.items()})


@pytest.mark.parametrize("N", [64, 65, 288])
@pytest.mark.parametrize("forced", list(ENVS))
def test_describe_is_the_plan(cuda_device, gsdr_lib, monkeypatch, forced, N):
    import torch
    env = ENVS[forced]
    clean_env(monkeypatch, env)
    cus = cuda_device_cus()
    for M in (744, 752, 992, 1000):
        L = ROWS * M
        rng = np.random.default_rng(N + M)
        freq = rng.choice(np.arange(-RATE // 2 + 1, RATE // 2), size=N, replace=False)
        x = torch.from_numpy(crandn(rng, L)).to(cuda_device)
        dem = make_direct(freq, RATE, M, F, L)
        out = torch.empty(dem.out_capacity, dtype=torch.complex64, device=cuda_device)
        torch.cuda.synchronize()
        for overlapped in (False, True):
            if overlapped:
                dem.submit_device(x, out)
                n = dem.wait()
            else:
                n = dem.process(x, out)
            torch.cuda.synchronize()
            assert n == N * ROWS, (forced, N, M, overlapped, n)
            plan = _ddc_plan.plan(gsdr_lib, N, M, F, L, rows=ROWS, overlapped=overlapped, cus=cus, env=env, rate=RATE)
            assert plan is not None and plan["engine"] == "mfma", (forced, N, M, plan)
            if forced != "unforced":
                assert plan["describe"][:5] == LOOPS[forced][1], (forced, N, M, plan)
            _ddc_plan.describe_matches_plan(dem.describe(), plan)
        dem.close()
