"""CPU: local delivery's host side (halo_amd/csrc/rx_deliver_host.cc over rx_deliver.h and
rx_dispatch.h, and halo_rx_dispatch in halo_amd/csrc/host_logic.cc) built alone with
g++ -fsanitize=address,undefined and driven by tools/fuzz_deliver.cc, a stand-alone program: random
halo_rx_deliver_host calls over exactly-sized heap buffers (the batch ends with its last frame's
last byte), each port map and the index present or absent, the region below, at and above the
total, records whose payload overruns their frame, LoChan batches, payloads at every byte
alignment, each checked against an in-program restatement — as is the dword arithmetic the kernels
share with the host side — with leak detection on. Nothing is loaded into Python. The same source
files are compiled into the library (halo_amd/build.py), so what is fuzzed here is what ships."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_deliver_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_deliver"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", *inc,
                    os.path.join(ROOT, "halo_amd", "csrc", "rx_deliver_host.cc"),
                    os.path.join(ROOT, "halo_amd", "csrc", "host_logic.cc"),
                    os.path.join(ROOT, "tools", "fuzz_deliver.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "3000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"deliver fuzz: (\d+) calls, kinds (\d+) (\d+) (\d+), records (\d+), skipped (\d+), cut (\d+), l3 (\d+), "
                  r"absent (\d+) (\d+) (\d+), align (\d+) (\d+) (\d+) (\d+)", r.stdout)
    assert m, r.stdout
    calls, udp, tcp, dhcp, records, skipped, cut, l3, no_udp, no_tcp, no_index, *align = map(int, m.groups())
    assert calls == 3000 and min(udp, tcp, dhcp) > 300           # every kind, many times
    assert records > 5000 and skipped > 300                      # and records that overrun their frame
    assert cut > 300 and l3 > 300                                # a region below the total, LoChan batches
    assert min(no_udp, no_tcp, no_index) > 300                   # every optional input left out
    assert min(align) > 1000                                     # payloads at each of the four source alignments


def test_library_links_the_fuzzed_sources():
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert {"rx_deliver_host.cc", "rx_deliver.hip", "host_logic.cc"} <= set(mod.SOURCES)
    assert {"rx_deliver.h", "rx_dispatch.h"} <= set(mod.HEADERS)


def test_deliver_host_sources_have_no_hip_dependency():
    for name in ("rx_deliver_host.cc", "rx_deliver.h", "rx_dispatch.h"):
        src = open(os.path.join(ROOT, "halo_amd", "csrc", name)).read()
        assert "hip_runtime" not in src.replace("#if defined(__HIPCC__)\n#include <hip/hip_runtime.h>", "")
