"""CPU: the list of compile-time tuning knobs the sources still carry.

A knob is a macro the build may override with -D: a `#define HALO_X` inside an `#ifndef HALO_Y ...
#endif` block, or a HALO_X that an `#if` tests and no file defines (set on the command line alone).
Every settled one was retired into a constant or a single code path; a new one has to be added to
KNOBS on purpose, with its measurement, or retired before merge."""
from __future__ import annotations

import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOBS = {
    # the bench library's build of flow_hash.hip (halo_amd/build.py: build_bench; bench.py)
    "HALO_XXH3_PROBE", "HALO_XXH3_PROBE_ENTRY",
    # found or rewritten by their #define text in tests/tx_cases.py, build_cases.py, scale_cases.py
    "HALO_TX_G1_MAX", "HALO_TXB_PAIR", "HALO_TXB_BIG_G", "HALO_TXB_BIG_U", "HALO_TXB_G1_WAVES",
    "HALO_TXB_MAX_BLOCKS", "HALO_TXB_SPLIT",
    # deleting its unreachable branch changed the compiled LoChan lane kernels: put back as it was
    "HALO_RX_LANE_DOT2",
}


def _sources():
    csrc = os.path.join(ROOT, "halo_amd", "csrc")
    files = [f for ext in ("hip", "h", "cc") for f in glob.glob(os.path.join(csrc, "*." + ext))]
    return sorted(files) + [os.path.join(ROOT, "tools", "bench_loop.hip")]


def knobs_of(text: str) -> tuple[set, set, set]:
    """(defined under an #ifndef guard, defined anywhere, tested by #if / #elif) HALO_* names."""
    guarded = set()
    for block in re.findall(r"^[ \t]*#[ \t]*ifndef[ \t]+HALO_\w+.*?^[ \t]*#[ \t]*endif", text, re.S | re.M):
        guarded |= set(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(HALO_\w+)", block, re.M))
    defined = set(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(HALO_\w+)", text, re.M))
    tested = set()
    for line in re.findall(r"^[ \t]*#[ \t]*(?:el)?if[ \t]+(.*)$", text, re.M):
        tested |= set(re.findall(r"\bHALO_\w+", line))
    return guarded, defined, tested


def test_the_knob_list_is_exact():
    files = _sources()
    assert len(files) > 20
    guarded, defined, tested = set(), set(), set()
    for path in files + glob.glob(os.path.join(ROOT, "include", "*.h")):
        with open(path) as fh:
            g, d, t = knobs_of(fh.read())
        if os.sep + "include" + os.sep not in path:  # the public headers define the ABI's names, no knobs
            guarded |= g
            tested |= t
        defined |= d
    assert guarded | (tested - defined) == KNOBS, sorted((guarded | (tested - defined)) ^ KNOBS)


def test_the_reader_sees_every_form():
    text = ("#ifndef HALO_A\n#define HALO_A 1\n#define HALO_B 2\n#endif\n  #ifndef HALO_C  // note\n  #define HALO_C (HALO_A * 2u)\n"
            "  #endif\n#define HALO_D 4\n#if HALO_E && !HALO_A\n#elif HALO_F\n#endif\nint x = HALO_G;\n")
    guarded, defined, tested = knobs_of(text)
    assert guarded == {"HALO_A", "HALO_B", "HALO_C"}
    assert defined == guarded | {"HALO_D"}
    assert tested - defined == {"HALO_E", "HALO_F"}
