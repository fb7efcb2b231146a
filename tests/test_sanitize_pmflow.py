"""CPU: the port-mapping return-flow table's host control plane (halo_amd/csrc/pmflow_table.cc) built
alone with g++ -fsanitize=address,undefined and driven by tools/fuzz_pmflow.cc, a stand-alone
program: a few hundred thousand random control-plane calls (record into full and roomy tables, get
with and without a stamp, expire across the uint32 wrap of TimeNow, list into exactly-sized short
buffers, layout statistics at automatic and forced capacity, refused items) with leak detection on.
Nothing is loaded into Python. The same source file is compiled into the library
(halo_amd/build.py), so what is fuzzed here is what ships."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_pmflow_table_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_pmflow"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror", *inc,
                    os.path.join(ROOT, "halo_amd", "csrc", "pmflow_table.cc"), os.path.join(ROOT, "tools", "fuzz_pmflow.cc"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "200000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"pmflow fuzz: (\d+) calls, (\d+) tables, (\d+) items, (\d+) added, (\d+) dropped, (\d+) overwritten, "
                  r"(\d+) removed, (\d+) lists, (\d+) get hits, (\d+) get misses, (\d+) range, (\d+) refused", r.stdout)
    assert m, r.stdout
    calls, tables, items, added, dropped, over, removed, lists, hits, misses, rng, refused = map(int, m.groups())
    assert calls == 200000 and tables > 100 and items > 100000 and added > 5000 and dropped > 1000 and over > 1000
    assert removed > 5000 and lists > 1000 and hits > 1000 and misses > 1000 and rng > 0 and refused > 100


def test_library_links_the_fuzzed_source():
    """libhalo_rx.so is built from the same pmflow_table.cc (halo_amd/build.py SOURCES), next to the
    kernels that read the image it compiles."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "pmflow_table.cc" in mod.SOURCES and "pmflow_fwd.hip" in mod.SOURCES


def test_pmflow_table_source_has_no_hip_dependency():
    """pmflow_table.cc and the headers it includes compile with plain g++: no HIP include on the path."""
    src = open(os.path.join(ROOT, "halo_amd", "csrc", "pmflow_table.cc")).read()
    hdr = open(os.path.join(ROOT, "halo_amd", "csrc", "pmflow_table.h")).read()
    assert "hip_runtime" not in src and "hip_runtime" not in hdr
