"""CPU: KCP emit's host side (halo_amd/csrc/tx_kcp_host.cc over tx_kcp.h) built alone with
g++ -fsanitize=address,undefined and driven by tools/fuzz_kcp_emit.cc, a stand-alone program: random
halo_kcp_emit_host calls over exactly-sized heap buffers (the payload ends with its last data byte,
the stream and the record arrays hold exactly their capacities), every byte-check mode, every
non-OK status, ENet entries, gaps, and capacities below, at and above what the batch needs, each
checked against an in-program restatement, with leak detection on. Nothing is loaded into Python.
The same source files are compiled into the library (halo_amd/build.py), so what is fuzzed here is
what ships."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_kcp_emit_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_kcp_emit"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", *inc, os.path.join(ROOT, "halo_amd", "csrc", "tx_kcp_host.cc"),
                    os.path.join(ROOT, "tools", "fuzz_kcp_emit.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "3000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"kcp emit fuzz: (\d+) calls, modes (\d+) (\d+) (\d+) (\d+), status (\d+) (\d+) (\d+) (\d+), cut_dgram (\d+), "
                  r"cut_stream (\d+), enet (\d+), dgrams (\d+), segs (\d+), empty (\d+), gaps (\d+), align (\d+) (\d+) (\d+) (\d+)", r.stdout)
    assert m, r.stdout
    v = list(map(int, m.groups()))
    calls, modes, status, cut_dgram, cut_stream, enet, dgrams, segs, empty, gaps = v[0], v[1:5], v[5:9], *v[9:16]
    assert calls == 3000 and min(modes) > 500       # every mode, many times
    assert min(status) > 300                        # every status was reached
    assert cut_dgram > 300 and cut_stream > 300     # and both capacity cuts
    assert enet > 1000 and dgrams > 10000 and segs > 20000 and empty > 500 and gaps > 1000
    assert min(v[16:]) > 3000                       # segments at each of the four destination alignments


def test_library_links_the_fuzzed_sources():
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert {"tx_kcp_host.cc", "tx_kcp.hip"} <= set(mod.SOURCES) and {"tx_kcp.h", "kcp_check_host.h", "kcp_crc_device.h"} <= set(mod.HEADERS)


def test_kcp_emit_host_sources_have_no_hip_dependency():
    for name in ("tx_kcp_host.cc", "tx_kcp.h", "kcp_check_host.h"):
        src = open(os.path.join(ROOT, "halo_amd", "csrc", name)).read()
        assert "hip_runtime" not in src and "__global__" not in src
