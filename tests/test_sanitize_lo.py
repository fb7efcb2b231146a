"""CPU: the loopback gather's host side (halo_amd/csrc/lo_gather_host.cc) built alone with g++
-fsanitize=address,undefined and driven by tools/fuzz_lo.cc, a stand-alone program: random
halo_lo_gather_host calls in both modes over exactly-sized heap buffers (the batch ends with its last
frame's last byte; regions, summaries and per-packet arrays hold what the call may write and no
more), each checked against an in-program restatement, with leak detection on. Nothing is loaded
into Python. The same source file is compiled into the library (halo_amd/build.py), so what is
fuzzed here is what ships."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_lo_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_lo"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", *inc,
                    os.path.join(ROOT, "halo_amd", "csrc", "lo_gather_host.cc"),
                    os.path.join(ROOT, "tools", "fuzz_lo.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "3000", "0x10C4A"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"lo fuzz: (\d+) calls, modes (\d+) (\d+), cuts (\d+), skips (\d+), packets (\d+), beyond (\d+)", r.stdout)
    assert m, r.stdout
    calls, fwd, tx, cuts, skips, packets, beyond = map(int, m.groups())
    assert calls == 3000 and min(fwd, tx) > 1200  # both modes
    assert cuts > 500 and skips > 500            # a region cut and a skip occurred, many times
    assert packets > 5000 and beyond > 200       # ... and listed packets beyond the written prefix


def test_library_links_the_fuzzed_sources():
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert {"lo_gather_host.cc", "lo_gather.hip"} <= set(mod.SOURCES) and "lo_gather.h" in mod.HEADERS


def test_lo_host_source_has_no_hip_dependency():
    for name in ("lo_gather_host.cc", "lo_gather.h"):
        src = open(os.path.join(ROOT, "halo_amd", "csrc", name)).read()
        assert "hip_runtime" not in src.replace("#if defined(__HIPCC__)\n#include <hip/hip_runtime.h>", "")
