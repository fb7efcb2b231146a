"""CPU: the local responders' host side (halo_amd/csrc/tx_respond_host.cc over tx_respond.h and
rx_dispatch.h, and halo_rx_dispatch in halo_amd/csrc/host_logic.cc) built alone with
g++ -fsanitize=address,undefined and driven by tools/fuzz_respond.cc, a stand-alone program: random
halo_tx_respond_host calls over exactly-sized heap buffers (records, offsets, lengths, verdict / op
/ result arrays, the port map, descriptors, sources, addresses, actions), each optional input
present or absent and `cap` below, at and above the count, each checked against an in-program
restatement, with leak detection on. Nothing is loaded into Python. The same source files are
compiled into the library (halo_amd/build.py), so what is fuzzed here is what ships."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_respond_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_respond"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", *inc,
                    os.path.join(ROOT, "halo_amd", "csrc", "tx_respond_host.cc"),
                    os.path.join(ROOT, "halo_amd", "csrc", "host_logic.cc"),
                    os.path.join(ROOT, "tools", "fuzz_respond.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "3000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"respond fuzz: (\d+) calls, kinds (\d+) (\d+) (\d+) (\d+), replies (\d+), cut (\d+), l3 (\d+), "
                  r"absent (\d+) (\d+) (\d+) (\d+)", r.stdout)
    assert m, r.stdout
    calls, echo, ttl, syn, synack, replies, cut, l3, *absent = map(int, m.groups())
    assert calls == 3000 and min(echo, ttl, syn, synack) > 300  # every kind, many times
    assert replies > 5000 and cut > 300 and l3 > 300            # a cap below the count, LoChan batches
    assert min(absent) > 300                                     # every optional input left out


def test_library_links_the_fuzzed_sources():
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert {"tx_respond_host.cc", "tx_respond.hip", "host_logic.cc"} <= set(mod.SOURCES)
    assert {"tx_respond.h", "rx_dispatch.h"} <= set(mod.HEADERS)


def test_respond_host_sources_have_no_hip_dependency():
    for name in ("tx_respond_host.cc", "tx_respond.h", "rx_dispatch.h"):
        src = open(os.path.join(ROOT, "halo_amd", "csrc", name)).read()
        assert "hip_runtime" not in src.replace("#if defined(__HIPCC__)\n#include <hip/hip_runtime.h>", "")
