#!/usr/bin/env python3
"""Hash the gfx950 device assembly and the host assembly of every library source, per checkout.

    python tools/device_asm.py [CHECKOUT ...] > profiles/knobs/NAME.sha256
    python tools/device_asm.py --kernels [CHECKOUT ...] > profiles/rx_split/NAME.sha256

A refactor that claims "no kernel changed" proves it by running this on the parent and on the tree and
comparing the two outputs line by line. SOURCES and the compile flags are read from the checkout's own
halo_amd/build.py; the bench library's flow_hash.hip (-O2, probe on) and tools/bench_loop.hip are hashed too.
Clang derives __hip_cuid_<16 hex> / __hip_gpubin_handle_<16 hex> from the file's text: they are masked.

--kernels: one line per device function of every .hip source, sorted by symbol and without the source's
name, so that a kernel that moved to another file keeps its line: the hash of its body, the hash of its
kernel descriptor (.amdhsa_*: registers, LDS, scratch; "-" for a function that is no kernel), the build
(lib / bench) and the symbol. ';' comments are dropped, and the function's ordinal in its module is masked
where labels carry it (.LBB<n>_<k>, .LJTI<n>_<k>): it changes with the kernels around it. The function's own
symbol is masked in its body and in its descriptor, so that a renamed kernel keeps its hashes.
"""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

MASK = re.compile(rb"__hip_(cuid|gpubin_handle)_[0-9a-f]{16}")
ORDINAL = re.compile(rb"\.(LBB|LJTI)\d+_")


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


def compile_asm(root, src, flags, side):
    out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, "--cuda-%s-only" % side, "-S", src, "-o", "-"],
                         cwd=root, check=True, capture_output=True).stdout
    return MASK.sub(b"__hip_\\1_X", out)


def asm(root, src, flags, side):
    return hashlib.sha256(compile_asm(root, src, flags, side)).hexdigest()


def kernels(root, src, flags):
    """{symbol: (body hash, descriptor hash or "-")} of one source's device assembly."""
    lines = [ORDINAL.sub(rb".\1_", l.split(b";")[0].rstrip()) for l in compile_asm(root, src, flags, "device").split(b"\n")]
    lines = [l for l in lines if l]
    funcs = [m.group(1) for l in lines for m in [re.match(rb"\s*\.type\s+(\S+),@function$", l)] if m]
    found = {}
    for sym in funcs:
        body = lines[lines.index(sym + b":"):]
        body = body[:next(i for i, l in enumerate(body) if l.startswith(b".Lfunc_end"))]
        desc = b"-"
        if b"\t.amdhsa_kernel " + sym in lines:
            d = lines[lines.index(b"\t.amdhsa_kernel " + sym):]
            desc = hashlib.sha256(b"\n".join(d[:d.index(b"\t.end_amdhsa_kernel") + 1]).replace(sym, b"SELF")).hexdigest().encode()
        found[sym.decode()] = (hashlib.sha256(b"\n".join(body).replace(sym, b"SELF")).hexdigest(), desc.decode())
    return found


def main():
    args = sys.argv[1:]
    per_kernel = "--kernels" in args
    for root in [a for a in args if a != "--kernels"] or ["."]:
        jobs = [(k, s, f, side) for k, s, f in plan(root) for side in ("device", "host") if side == "host" or s.endswith(".hip")]
        if per_kernel:
            jobs = [j for j in jobs if j[3] == "device"]
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
            if per_kernel:
                found = list(ex.map(lambda j: kernels(root, j[1], j[2]), jobs))
                rows = sorted((sym, kind, body, desc) for (kind, _, _, _), ks in zip(jobs, found) for sym, (body, desc) in ks.items())
                for sym, kind, body, desc in rows:
                    print("%s  %s  %-5s %s" % (body, desc, kind, sym))
                continue
            sums = list(ex.map(lambda j: asm(root, j[1], j[2], j[3]), jobs))
        for (kind, src, flags, side), h in zip(jobs, sums):
            print("%s  %-5s %-6s %s" % (h, kind, side, src))


if __name__ == "__main__":
    main()
