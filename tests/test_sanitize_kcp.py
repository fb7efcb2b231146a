"""CPU: KCP ingest's host side (halo_amd/csrc/rx_kcp_host.cc over rx_kcp.h) built alone with
g++ -fsanitize=address,undefined and driven by tools/fuzz_kcp.cc, a stand-alone program: random
halo_kcp_ingest_host calls over exactly-sized heap buffers (the stream ends with its last payload
byte), every byte-check mode, every structural failure and wrong hash fields, ENet packets and
near misses, other kinds and ports, unwritten records, capacities and index_cap below, at and
above what the delivery needs, each checked against an in-program restatement — as is the CRC
arithmetic the kernels share with the host side, run as a lane group runs it over funnelled
dwords — with leak detection on. Nothing is loaded into Python. The same source files are compiled
into the library (halo_amd/build.py), so what is fuzzed here is what ships."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_kcp_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_kcp"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", *inc, os.path.join(ROOT, "halo_amd", "csrc", "rx_kcp_host.cc"),
                    os.path.join(ROOT, "tools", "fuzz_kcp.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "3000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"kcp fuzz: (\d+) calls, modes (\d+) (\d+) (\d+) (\d+), kcp (\d+), rets (\d+) (\d+) (\d+) (\d+) (\d+), "
                  r"enet (\d+) (\d+) (\d+) (\d+), ignored (\d+), segs (\d+), passed (\d+), failed (\d+), cut (\d+), unwritten (\d+), "
                  r"others (\d+), capped (\d+), lanes (\d+), align (\d+) (\d+) (\d+) (\d+)", r.stdout)
    assert m, r.stdout
    v = list(map(int, m.groups()))
    calls, modes, kcp, rets, enet = v[0], v[1:5], v[5], v[6:11], v[11:15]
    ignored, segs, passed, failed, cut, unwritten, others, capped, lanes = v[15:24]
    align = v[24:]
    assert calls == 3000 and lanes == 3000 and min(modes) > 500            # every mode, many times
    assert kcp > 10000 and min(rets) > 500 and min(enet) > 200              # every return value and ENet type
    assert ignored > 1000 and segs > 20000 and min(passed, failed) > 2000   # byte checks that pass and that fail
    assert min(cut, unwritten, others, capped) > 300                        # capacity cuts and everything not selected
    assert min(align) > 3000                                                # segment data at each of the four alignments


def test_library_links_the_fuzzed_sources():
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert {"rx_kcp_host.cc", "rx_kcp.hip"} <= set(mod.SOURCES) and "rx_kcp.h" in mod.HEADERS


def test_kcp_host_sources_have_no_hip_dependency():
    for name in ("rx_kcp_host.cc", "rx_kcp.h"):
        src = open(os.path.join(ROOT, "halo_amd", "csrc", name)).read()
        assert "hip_runtime" not in src and "__global__" not in src
