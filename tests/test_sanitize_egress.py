"""CPU: the egress step's host side (halo_amd/csrc/tx_egress_host.cc, and halo_ring_write_span in
halo_amd/csrc/host_logic.cc) built alone with g++ -fsanitize=address,undefined and driven by
tools/fuzz_egress.cc, a stand-alone program: random halo_tx_egress_host calls of all three kinds
over exactly-sized heap buffers (frames, selectors, outputs, summaries, index lists), each checked
against an in-program restatement, and every port's stream published into a small ring and read
back, with leak detection on. Nothing is loaded into Python. The same source files are compiled into
the library (halo_amd/build.py), so what is fuzzed here is what ships."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_egress_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_egress"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", *inc,
                    os.path.join(ROOT, "halo_amd", "csrc", "tx_egress_host.cc"),
                    os.path.join(ROOT, "halo_amd", "csrc", "host_logic.cc"),
                    os.path.join(ROOT, "tools", "fuzz_egress.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "3000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"egress fuzz: (\d+) calls, kinds (\d+) (\d+) (\d+), cuts (\d+), skips (\d+), records (\d+), "
                  r"ring records (\d+), ring short (\d+), ring refused (\d+)", r.stdout)
    assert m, r.stdout
    calls, k0, k1, k2, cuts, skips, records, ring_records, ring_short, ring_refused = map(int, m.groups())
    assert calls == 3000 and min(k0, k1, k2) > 800  # every kind
    assert cuts > 500 and skips > 500               # a region cut and a skip occurred, many times
    assert records > 10000 and ring_records > 1000 and ring_short > 20 and ring_refused > 20


def test_library_links_the_fuzzed_sources():
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert {"tx_egress_host.cc", "tx_egress.hip", "host_logic.cc"} <= set(mod.SOURCES) and "tx_egress.h" in mod.HEADERS


def test_egress_host_source_has_no_hip_dependency():
    for name in ("tx_egress_host.cc", "tx_egress.h"):
        src = open(os.path.join(ROOT, "halo_amd", "csrc", name)).read()
        assert "hip_runtime" not in src.replace("#if defined(__HIPCC__)\n#include <hip/hip_runtime.h>", "")
