"""CPU: the ARP neighbour cache's host control plane (halo_amd/csrc/arp_table.cc) built alone with
g++ -fsanitize=address,undefined and driven by tools/fuzz_arp.cc, a stand-alone program: random
create / set / get / handle_msgs / build_request / expire / refresh_list / list calls (exactly-sized
message, verdict, reply and list buffers, `now` across the uint32 wrap, tables that fill up), each
result checked against an in-program restatement, with leak detection on. Nothing is loaded into
Python. The same source file is compiled into the library (halo_amd/build.py), so what is fuzzed
here is what ships."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_arp_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_arp"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror", *inc,
                    os.path.join(ROOT, "halo_amd", "csrc", "arp_table.cc"),
                    os.path.join(ROOT, "tools", "fuzz_arp.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "60000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"arp fuzz: (\d+) calls, (\d+) tables, (\d+) msgs, (\d+) replies, (\d+) removed, (\d+) refresh, "
                  r"(\d+) lists, (\d+) dirty, gets (\d+) (\d+) (\d+), not_learned (\d+), full_replies (\d+), "
                  r"verdicts (\d+) (\d+) (\d+) (\d+)", r.stdout)
    assert m, r.stdout
    calls, tables, msgs, replies, removed, refresh, lists, dirty, g0, g1, g2, not_learned, full_replies, *verdicts = map(
        int, m.groups())
    assert calls == 60000 and tables > 100 and msgs > 50000 and replies > 1000 and removed > 1000 and refresh > 1000
    assert lists > 1000 and dirty > 1000 and min(g0, g1, g2) > 100
    assert not_learned > 100 and full_replies > 10  # a full table still answers
    assert all(v > 1000 for v in verdicts), verdicts  # BAD_OP, SRC_MISMATCH, CONFLICT, ACCEPTED all occurred


def test_library_links_the_fuzzed_source():
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "arp_table.cc" in mod.SOURCES and "arp_fwd.hip" in mod.SOURCES and "arp_table.h" in mod.HEADERS


def test_arp_table_source_has_no_hip_dependency():
    for name in ("arp_table.cc", "arp_table.h"):
        src = open(os.path.join(ROOT, "halo_amd", "csrc", name)).read()
        assert "hip_runtime" not in src.replace("#if defined(__HIPCC__)\n#include <hip/hip_runtime.h>", "")
