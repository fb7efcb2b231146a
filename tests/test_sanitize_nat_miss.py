"""CPU: the host parts of the NAT miss path (halo_amd/csrc/nat_table.cc: halo_nat_collect_misses_host,
halo_nat_resolve_items and the body they share with halo_nat_resolve_misses) built alone with
g++ -fsanitize=address,undefined and driven by tools/fuzz_nat_miss.cc, a stand-alone program: random
batches with heavy key reuse, zero ports, select masks and short caps in both directions and NAT
types, the twin-table property checked in C, every output array exactly sized, leak detection on.
Nothing is loaded into Python. The same source file is compiled into the library."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]
FIELDS = ("batches", "items", "duplicates", "alone", "sport0 duplicates", "short caps", "drops", "added", "wan batches",
          "wan flow hits", "deselected", "mapping hits", "removed")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_nat_miss_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_nat_miss"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror", *inc,
                    os.path.join(ROOT, "halo_amd", "csrc", "nat_table.cc"), os.path.join(ROOT, "tools", "fuzz_nat_miss.cc"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "4000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"nat miss fuzz: " + ", ".join(rf"(\d+) {f}" for f in FIELDS), r.stdout)
    assert m, r.stdout
    c = dict(zip(FIELDS, map(int, m.groups())))
    assert c["batches"] == 4000 and c["items"] > 50000 and c["duplicates"] > 50000
    for f in FIELDS[3:]:  # every class was reached
        assert c[f] > 100, (f, c)


def test_library_links_the_fuzzed_source_and_the_kernels():
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "nat_table.cc" in mod.SOURCES and "nat_miss.hip" in mod.SOURCES
