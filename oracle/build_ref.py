"""Recipe: compile the reference's own RX path for the host into oracle/_ref/libgsdr_ref.so.

TEST INFRASTRUCTURE ONLY.  Nothing from the reference is committed: this recipe reads its
sources at build time (from $GSDR_REF_SRC, default /root/reference) and every copy or
rewrite of them goes to oracle/_ref/, which git ignores.  The committed pieces are ours:
the stand-in headers for the closed libraries under oracle/ref/include/ (CUDA runtime,
cuBLAS, cuFFT, cuRAND, thrust) and the C driver oracle/ref/ref_driver.cpp.

What is compiled from the reference, unchanged apart from the launch syntax:
  cpp/kernels.cu           every kernel and wrapper (launches run serially, see cuda_runtime.h)
  cpp/fir.cu               the FIR class of the decimating DDC
  cpp/USRP_demodulator.cpp RX_buffer_demodulator: create / process / close, all modes
  cpp/USRP_server_memory_management.cpp   from the VNA helper on (buffer_helper,
                           pfb_decimator_helper, VNA_decimator_helper, gp_decimator_helper)
  cpp/USRP_server_console_print.cpp       (the demodulator prints warnings)
Reference headers are copied as they are, except three that pull in boost / UHD for
declarations the RX path does not use; of those, filtered copies keep only named blocks
(see _FILTERED).

Rewrites: `k<<<g, b[, smem[, stream]]>>>(` -> `ref_launch(k, g, b, ` and the one
`extern __shared__` array -> a static array of the largest block.  The build fails if a
rewritten source holds a barrier, a warp shuffle or a ballot: the serial launch would be
wrong for it.

When the reference is absent (as on the GPU machines) an existing oracle/_ref/ is left as
it is and nothing fails.
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
LIB = os.path.join(OUT, "libgsdr_ref.so")
STANDIN = os.path.join(HERE, "ref", "include")
DRIVER = os.path.join(HERE, "ref", "ref_driver.cpp")

SOURCES = ["cpp/kernels.cu", "cpp/fir.cu", "cpp/USRP_demodulator.cpp",
           "cpp/USRP_server_memory_management.cpp", "cpp/USRP_server_console_print.cpp"]
HEADERS = ["headers/kernels.cuh", "headers/fir.hpp", "headers/USRP_demodulator.hpp",
           "headers/USRP_server_console_print.hpp"]
# header -> (includes the filtered copy needs, blocks kept: (keyword, name))
_FILTERED = {
    "headers/USRP_server_settings.hpp": (
        ["<string>", "<vector>", "<stdexcept>", "<algorithm>", "<sstream>", "<cmath>", "<cassert>",
         "<cuda_runtime.h>", '"USRP_server_console_print.hpp"'],
        [("enum", "w_type"), ("enum", "ant_mode"), ("struct", "param")]),
    "headers/USRP_server_diagnostic.hpp": (['"USRP_server_settings.hpp"'], []),
    "headers/USRP_server_memory_management.hpp": (
        ['"USRP_server_settings.hpp"', "<cmath>"],
        [("class", "VNA_decimator_helper"), ("class", "gp_decimator_helper"),
         ("class", "pfb_decimator_helper"), ("class", "buffer_helper")]),
}
# the part of the memory-management source that holds the helpers (the rest is boost threading)
_MEMORY_FROM = "VNA_decimator_helper::VNA_decimator_helper"

CXXFLAGS = ["-O2", "-std=c++14", "-fpermissive", "-fwrapv", "-ffp-contract=off", "-fPIC", "-shared", "-w"]
FORBIDDEN = ("__syncthreads", "__shfl", "__ballot")


def ref_src() -> str:
    return os.environ.get("GSDR_REF_SRC", "/root/reference")


def _block(text: str, keyword: str, name: str) -> str:
    """`keyword name ... { ... };` with balanced braces."""
    m = re.search(r"^\s*%s\s+%s\b[^{;]*\{" % (keyword, re.escape(name)), text, re.M)
    if not m:
        raise RuntimeError(f"build_ref: no `{keyword} {name}` block in the reference header")
    depth, i = 0, m.end() - 1
    while True:
        c = text[i]
        depth += c == "{"
        depth -= c == "}"
        i += 1
        if depth == 0:
            break
    end = text.index(";", i) + 1
    return text[m.start():end].strip("\n")


def _launches(text: str) -> str:
    """k<<<cfg>>>( -> ref_launch(k, g, b, ; shared memory size and stream are dropped."""
    out, pos = [], 0
    for m in re.finditer(r"(\w+)\s*<<<", text):
        if m.start() < pos:
            continue
        close = text.index(">>>", m.end())
        cfg, depth, parts, cur = text[m.end():close], 0, [], ""
        for c in cfg:
            if c == "," and depth == 0:
                parts.append(cur)
                cur = ""
                continue
            depth += c in "([{"
            depth -= c in ")]}"
            cur += c
        parts.append(cur)
        after = re.match(r"\s*\(", text[close + 3:])
        if not after or len(parts) < 2:
            raise RuntimeError(f"build_ref: cannot rewrite the launch of {m.group(1)}")
        out.append(text[pos:m.start()])
        out.append(f"ref_launch({m.group(1)}, {parts[0].strip()}, {parts[1].strip()}, ")
        pos = close + 3 + after.end()
    out.append(text[pos:])
    return "".join(out)


def _shared(text: str) -> str:
    return re.sub(r"extern\s+__shared__\s+(\w+)\s+(\w+)\s*\[\s*\]\s*;",
                  r"static \1 \2[1024]; /* build_ref: one block at a time, at most 1024 threads */", text)


def _inputs(src: str):
    return ([os.path.join(src, f) for f in SOURCES + HEADERS + list(_FILTERED)]
            + [os.path.join(STANDIN, r, f) for r, _, fs in os.walk(STANDIN) for f in fs]
            + [DRIVER, os.path.abspath(__file__)])


def _up_to_date(inputs) -> bool:
    if not os.path.exists(LIB):
        return False
    t = os.path.getmtime(LIB)
    return all(os.path.getmtime(p) <= t for p in inputs)


def build(force: bool = False, verbose: bool = False) -> str | None:
    """Build oracle/_ref/libgsdr_ref.so; returns its path, or None when neither the reference
    nor an earlier build is there."""
    src = ref_src()
    if not os.path.isdir(os.path.join(src, "cpp")):
        return LIB if os.path.exists(LIB) else None
    inputs = _inputs(src)
    missing = [p for p in inputs if not os.path.exists(p)]
    if missing:
        raise RuntimeError(f"build_ref: missing inputs {missing}")
    if not force and _up_to_date(inputs):
        return LIB

    inc, srcdir = os.path.join(OUT, "include"), os.path.join(OUT, "src")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(inc)
    os.makedirs(srcdir)
    digests = {}

    def read(rel):
        with open(os.path.join(src, rel), "rb") as fh:
            data = fh.read()
        digests[rel] = hashlib.sha256(data).hexdigest()
        return data.decode("utf-8", errors="replace")

    for rel in HEADERS:
        with open(os.path.join(inc, os.path.basename(rel)), "w") as fh:
            fh.write(read(rel))
    for rel, (includes, blocks) in _FILTERED.items():
        text = read(rel)
        guard = "GSDR_REF_FILTERED_" + re.sub(r"\W", "_", os.path.basename(rel)).upper()
        body = [f"/* build_ref: blocks of {rel} the RX path needs; boost / UHD parts left out */",
                f"#ifndef {guard}", f"#define {guard}"]
        body += [f"#include {i}" for i in includes]
        body += [_block(text, k, n) for k, n in blocks]
        body.append("#endif")
        with open(os.path.join(inc, os.path.basename(rel)), "w") as fh:
            fh.write("\n".join(body) + "\n")

    units = []
    for rel in SOURCES:
        text = read(rel)
        if rel.endswith("memory_management.cpp"):
            start = text.index(_MEMORY_FROM)
            start = text.rfind("\n", 0, start) + 1
            text = '#include "USRP_server_memory_management.hpp"\n' + text[start:]
        text = _shared(_launches(text))
        bad = [w for w in FORBIDDEN if w in text]
        if bad:
            raise RuntimeError(f"build_ref: {rel} uses {bad}; a serial launch would not run it as written")
        if "<<<" in text:
            raise RuntimeError(f"build_ref: a launch in {rel} was not rewritten")
        dst = os.path.join(srcdir, os.path.basename(rel) + (".cpp" if rel.endswith(".cu") else ""))
        with open(dst, "w") as fh:
            fh.write(text)
        units.append(dst)

    cxx = os.environ.get("CXX", "g++")
    cmd = ([cxx] + CXXFLAGS + ["-I", STANDIN, "-I", inc, "-o", LIB] + units + [DRIVER]
           + ["-lm", "-Wl,--no-undefined"])
    subprocess.run(cmd, check=True, stdout=None if verbose else subprocess.DEVNULL)
    with open(os.path.join(OUT, "SOURCES.json"), "w") as fh:
        json.dump({"sha256": digests, "cxx": cmd[0], "flags": CXXFLAGS}, fh, indent=1, sort_keys=True)
    return LIB


if __name__ == "__main__":
    path = build(force="-f" in sys.argv, verbose=True)
    print(path or "reference not found: nothing built")
