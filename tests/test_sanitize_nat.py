"""CPU: the NAT flow table's host control plane (halo_amd/csrc/nat_table.cc) built alone with
g++ -fsanitize=address,undefined and driven by tools/fuzz_nat.cc, a stand-alone program: a few
hundred thousand random control-plane calls (add, both gets, port mappings, the miss slow path,
expire across the uint32 wrap of TimeNow, list into exactly-sized short buffers, layout statistics
at automatic and forced capacity) with leak detection on. Nothing is loaded into Python. The same
source file is compiled into the library (halo_amd/build.py), so what is fuzzed here is what ships."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_nat_table_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_nat"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror", *inc,
                    os.path.join(ROOT, "halo_amd", "csrc", "nat_table.cc"), os.path.join(ROOT, "tools", "fuzz_nat.cc"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "300000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"nat fuzz: (\d+) calls, (\d+) flows added, (\d+) nil, (\d+) get hits, (\d+) removed, "
                  r"(\d+) resolves, (\d+) lists, (\d+) range", r.stdout)
    assert m, r.stdout
    calls, added, nil, hits, removed, resolves, lists, rng = map(int, m.groups())
    assert calls == 300000 and added > 10000 and nil > 100 and hits > 100 and removed > 10000
    assert resolves > 1000 and lists > 1000 and rng > 0


def test_library_links_the_fuzzed_source():
    """libhalo_rx.so is built from the same nat_table.cc (halo_amd/build.py SOURCES), next to the
    kernels that read the image it compiles."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "nat_table.cc" in mod.SOURCES and "nat_lookup.hip" in mod.SOURCES


def test_nat_table_source_has_no_hip_dependency():
    """nat_table.cc and the headers it includes compile with plain g++: no HIP include on the path."""
    src = open(os.path.join(ROOT, "halo_amd", "csrc", "nat_table.cc")).read()
    hdr = open(os.path.join(ROOT, "halo_amd", "csrc", "nat_table.h")).read()
    assert "hip_runtime" not in src and "hip_runtime" not in hdr
