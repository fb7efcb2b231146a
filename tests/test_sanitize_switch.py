"""CPU: the L2 switch's host side (halo_amd/csrc/switch_table.cc) built alone with
g++ -fsanitize=address,undefined and driven by tools/fuzz_switch.cc, a stand-alone program: random
create / forward / expire / list calls in host mode (exactly-sized frame and list buffers, `now`
across the uint32 wrap, tables that fill up), each result checked against a restatement of the
sequential loop, with leak detection on. Nothing is loaded into Python. The same source file is
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
def test_switch_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_switch"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror", *inc,
                    os.path.join(ROOT, "halo_amd", "csrc", "switch_table.cc"),
                    os.path.join(ROOT, "tools", "fuzz_switch.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "60000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"switch fuzz: (\d+) calls, (\d+) switches, (\d+) frames, (\d+) removed, (\d+) lists, (\d+) range, "
                  r"verdicts (\d+) (\d+) (\d+) (\d+) (\d+) (\d+)", r.stdout)
    assert m, r.stdout
    calls, switches, frames, removed, lists, rng, *verdicts = map(int, m.groups())
    assert calls == 60000 and switches > 100 and frames > 100000 and removed > 1000 and lists > 1000 and rng > 100
    assert all(v > 1000 for v in verdicts), verdicts


def test_library_links_the_fuzzed_source():
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "switch_table.cc" in mod.SOURCES and "switch_fwd.hip" in mod.SOURCES and "switch_table.h" in mod.HEADERS


def test_switch_table_source_has_no_hip_dependency():
    for name in ("switch_table.cc", "switch_table.h"):
        src = open(os.path.join(ROOT, "halo_amd", "csrc", name)).read()
        assert "hip_runtime" not in src.replace("#if defined(__HIPCC__)\n#include <hip/hip_runtime.h>", "")
