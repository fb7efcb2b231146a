#!/usr/bin/env python3
"""Hash the gfx950 device assembly and the host assembly of every library source, per checkout.

    python tools/device_asm.py [CHECKOUT ...] > profiles/knobs/NAME.sha256

A refactor that claims "no kernel changed" proves it by running this on the parent and on the tree and
comparing the two outputs line by line. SOURCES and the compile flags are read from the checkout's own
halo_amd/build.py; the bench library's flow_hash.hip (-O2, probe on) and tools/bench_loop.hip are hashed too.
Clang derives __hip_cuid_<16 hex> / __hip_gpubin_handle_<16 hex> from the file's text: they are masked.
"""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

MASK = re.compile(rb"__hip_(cuid|gpubin_handle)_[0-9a-f]{16}")


def plan(root):
    text = open(os.path.join(root, "halo_amd", "build.py")).read()
    sources = eval(re.search(r"^SOURCES = (\[.*?\])", text, re.S | re.M).group(1))
    lists = re.findall(r"(?:flags|cmd) = \[(.*?)\]\n", text, re.S)
    lib = [f for f in re.findall(r'"(-[^"]+)"', lists[0]) if f not in ("-I", "-Wall")]
    bench = [f for f in re.findall(r'"(-[^"]+)"', [l for l in lists if "BENCH_SRC" in l][0])
             if f[:2] in ("--", "-O", "-s", "-f", "-D") and f != "-shared"]
    inc = ["-I", "include", "-I", "halo_amd/csrc"]
    jobs = [("lib", "halo_amd/csrc/" + s, lib + inc) for s in sources]
    jobs += [("bench", "halo_amd/csrc/flow_hash.hip", bench + inc), ("bench", "tools/bench_loop.hip", bench + inc)]
    return jobs


def asm(root, src, flags, side):
    out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "--cuda-%s-only" % side, "-S", src, "-o", "-"],
                         cwd=root, check=True, capture_output=True).stdout
    return hashlib.sha256(MASK.sub(b"__hip_\\1_X", out)).hexdigest()


def main():
    for root in sys.argv[1:] or ["."]:
        jobs = [(k, s, f, side) for k, s, f in plan(root) for side in ("device", "host") if side == "host" or s.endswith(".hip")]
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
            sums = list(ex.map(lambda j: asm(root, j[1], j[2], j[3]), jobs))
        for (kind, src, flags, side), h in zip(jobs, sums):
            print("%s  %-5s %-6s %s" % (h, kind, side, src))


if __name__ == "__main__":
    main()
