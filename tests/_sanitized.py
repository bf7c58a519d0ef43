"""What the host-twin sanitizer tests share (test_{trigger,welch,decim,sweep,resmap,stats,sc16_tx}_sanitizers.py): a
driver program with its own main is built together with the host sources alone (HOST_SOURCES: host_logic.cpp and the
stages' X_host.cpp) by plain g++ under AddressSanitizer + UndefinedBehaviorSanitizer and run as a stand-alone program.
Nothing is loaded into Python, nothing is preloaded.  What the program must print and what its stderr must not hold
stays with each test."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu_sdr_amd", "csrc")
# every source of the library that needs no HIP: what a build without a device part is made of
HOST_SOURCES = sorted([os.path.join(CSRC, "host_logic.cpp")] + glob.glob(os.path.join(CSRC, "*_host.cpp")))


def build_and_run(driver: str, tmp_path) -> subprocess.CompletedProcess:
    """The finished run of `driver` (C++ source) linked with HOST_SOURCES; skips where g++ or its sanitizer runtime
    is missing, fails where the build does."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    (tmp_path / "driver.cpp").write_text(driver)
    exe = tmp_path / "driver"
    build = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow",
                            "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                            str(tmp_path / "driver.cpp"), *HOST_SOURCES, "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
