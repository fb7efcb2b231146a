"""CPU: the DHCP service's host side (halo_amd/csrc/rx_dhcp_host.cc, tx_dhcp_host.cc and
dhcp_table.cc over rx_dhcp.h and dhcp_table.h) built alone with g++ -fsanitize=address,undefined
and driven by tools/fuzz_dhcp.cc, a stand-alone program: random deliveries in heap buffers sized
exactly to the stream (a read past a payload's last byte is an error), decoded, handled by a server
that lives across calls, the replies built and decoded again, each step checked against an
in-program restatement, with leak detection on. Nothing is loaded into Python. The same source
files are compiled into the library (halo_amd/build.py), so what is fuzzed here is what ships."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"]
HOST_FILES = ("rx_dhcp_host.cc", "tx_dhcp_host.cc", "dhcp_table.cc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_dhcp_fuzz_asan_ubsan(tmp_path):
    inc = [f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'halo_amd', 'csrc')}"]
    exe = tmp_path / "fuzz_dhcp"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror", *inc,
                    *[os.path.join(ROOT, "halo_amd", "csrc", f) for f in HOST_FILES],
                    os.path.join(ROOT, "tools", "fuzz_dhcp.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:" + env.get("ASAN_OPTIONS", "")
    r = subprocess.run([str(exe), "4000", "0x5EED"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"dhcp fuzz: (\d+) calls, msgs (\d+), status((?: \d+){5}), verdicts((?: \d+){14}), reused (\d+), events (\d+), "
                  r"built (\d+), kinds((?: \d+){5}), cut (\d+), unwritten (\d+), others (\d+), capped (\d+), align((?: \d+){4})", r.stdout)
    assert m, r.stdout
    g = m.groups()
    ints = lambda s: list(map(int, s.split()))  # noqa: E731
    assert int(g[0]) == 4000 and int(g[1]) > 30000
    assert min(ints(g[2])) > 1000                               # every status, many times
    assert min(ints(g[3])) > 40                                 # every verdict of the state machine
    assert int(g[4]) > 5 and int(g[5]) > 50 and int(g[6]) > 2000  # renewals / reuse, client events, built replies
    assert min(ints(g[7])) > 10                                 # every reply kind built and decoded again
    assert min(int(g[8]), int(g[9]), int(g[10]), int(g[11])) > 300  # capacity cuts and everything not selected
    assert min(ints(g[12])) > 3000                              # hostnames at each of the four alignments


def test_library_links_the_fuzzed_sources():
    import importlib.util

    spec = importlib.util.spec_from_file_location("halo_build", os.path.join(ROOT, "halo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert {*HOST_FILES, "rx_dhcp.hip", "tx_dhcp.hip"} <= set(mod.SOURCES) and {"rx_dhcp.h", "dhcp_table.h"} <= set(mod.HEADERS)


def test_dhcp_host_sources_have_no_hip_dependency():
    for name in (*HOST_FILES, "rx_dhcp.h", "dhcp_table.h"):
        src = open(os.path.join(ROOT, "halo_amd", "csrc", name)).read()
        assert "hip_runtime" not in src and "__global__" not in src
