"""CPU: what the transmit-rewrite sweep on the device rests on (tests/tx_cases.py). The hint ladder
of halo_tx_fixup_batch_device as tx_fixup.hip has it still gives the widths the GPU tests' hints
were chosen for; the case table reaches every path of the kernel's two summing passes at every
width, which the committed fixtures do not; the C oracle, which is the expectation of every GPU
comparison, equals the Python restatement (oracle/ref_tx_py.py) on the table; and the buffer
comparison names the case a difference lies in."""
from __future__ import annotations

import collections
import os

import numpy as np
import pytest

from tests import tx_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = {"default": 65535, "rungs": ((128, 1), (1024, 4), (4096, 8)), "rest": 16, "kHdrDw": 13, "U0": 4, "U": 4}
# lanes per frame -> the hints that select it (0 stands for 65535)
RANGES = {1: (1, 128), 4: (129, 1024), 8: (1025, 4096), 16: (4097, 65535)}
FLOOR = 256   # cases per reach cell: four full waves of the lane-per-frame kernel
RUN = 128     # consecutive cases of one class: a whole 64-frame wave wherever the run starts


def test_ladder_follows_the_source():
    """The ladder found in tx_fixup.hip is the one the hints were chosen for, with the ranges
    1..128, 129..1024, 1025..4096, 4097.. and 0 equal to 65535; the header copy and the loops'
    strides are the ones the table's lengths are built around."""
    lad = T.read_ladder()
    assert lad == LADDER
    assert T.HDR == 4 * lad["kHdrDw"] and T.ITER_BYTES == 16 * lad["U"] == 16 * lad["U0"]
    assert tuple(T.HINTS) == T.WIDTHS == tuple(RANGES)
    for g, (lo, hi) in RANGES.items():
        assert T.width_of(lo) == T.width_of(hi) == g, (g, lo, hi)
        assert {T.width_of(h) for h in range(lo, min(hi, 5000) + 1)} == {g}
        assert T.width_of(T.HINTS[g]) == g and (T.HINTS[g] == 0 or lo <= T.HINTS[g] <= hi)
    assert T.width_of(0) == T.width_of(65535) == T.width_of((1 << 32) - 1) == 16


@pytest.mark.parametrize("old,new,moved", [
    ("#define HALO_TX_G1_MAX 128", "#define HALO_TX_G1_MAX 60", 64), ("else if (h <= 1024)", "else if (h <= 999)", 1000),
    ("else if (h <= 4096)", "else if (h <= 3999)", 4000), ("max_len_hint : 65535u", "max_len_hint : 4096u", 0),
    ("else if (h <= 1024) hipLaunchKernelGGL(halo::tx_fixup_kernel<4>", "else if (h <= 1024) hipLaunchKernelGGL(halo::tx_fixup_kernel<8>", 1000),
    ("\n    else hipLaunchKernelGGL(halo::tx_fixup_kernel<16>", "\n    else hipLaunchKernelGGL(halo::tx_fixup_kernel<8>", 0),
    ("if (h <= HALO_TX_G1_MAX) hipLaunchKernelGGL(halo::tx_fixup_kernel<1>", "if (h <= HALO_TX_G1_MAX) hipLaunchKernelGGL(halo::tx_fixup_kernel<4>", 64)])
def test_an_edited_rung_is_noticed(tmp_path, old, new, moved):
    """An edit of any rung of a copy of the source changes the ladder read from it and the width of
    a hint the GPU tests use: test_ladder_follows_the_source would fail on such a tree."""
    with open(T.TX_FIXUP_HIP) as fh:
        src = fh.read()
    assert src.count(old) == 1, old
    path = tmp_path / "tx_fixup.hip"
    path.write_text(src.replace(old, new))
    lad = T.read_ladder(str(path))
    assert lad != LADDER and T.width_of(moved, lad) != T.width_of(moved)


@pytest.mark.parametrize("old,new", [("kHdrDw = 13;", "kHdrDw = 14;"), ("constexpr int U = 4;", "constexpr int U = 2;"),
                                     ("constexpr int U0 = 4;", "constexpr int U0 = 8;")])
def test_an_edited_stride_is_noticed(tmp_path, old, new):
    with open(T.TX_FIXUP_HIP) as fh:
        src = fh.read()
    assert src.count(old) == 1, old
    path = tmp_path / "tx_fixup.hip"
    path.write_text(src.replace(old, new))
    assert T.read_ladder(str(path)) != LADDER


def _plan_arrays(plans):
    return {k: np.array([p[k] for p in plans], np.int64) for k in ("L", "ip_hi", "go_hi", "dp_hi", "l4a", "l4b")}


def test_table_holds_what_it_claims():
    c = T.sweep()
    assert len(c.lens) == 80_424 and c.blob.nbytes < 32 << 20
    assert int(c.lens.max()) == T.MAX_FRAME and int(c.lens.min()) == 34
    assert set(c.ihl.tolist()) == set(T.IHLS) and set(c.proto.tolist()) == set(T.PROTOS)
    assert set(c.rel.tolist()) == set(range(len(T.RELATIONS)))
    want_l4 = set(T.l4_lengths())
    assert {0, 1, 4, 8, 9, 17, 18, 19, 20, 29, 30, 31, 32, 33, 34, 50, 51, 52, 53, 1440, 1441} <= want_l4
    for g in T.WIDTHS:
        assert {64 * g + d for d in (-35, -34, -33, -2, -1, 0, 1, 2, 3, 5)} <= want_l4
    for ihl in T.IHLS:  # no length and no IHL thinned: every length under every IHL, but past 1514 bytes
        got = set(c.l4len[c.ihl == ihl].tolist())
        assert got == {n for n in want_l4 if 14 + 4 * ihl + n <= T.MAX_FRAME}, ihl
    assert set(T.STEP_SETS) <= set(c.steps.tolist()) and len(set(c.steps.tolist())) > 24
    # the frames are what the parameters say: real IHL, a total length that includes the options
    s = c.start
    assert np.array_equal(c.blob[s + 14], 0x40 | c.ihl) and np.array_equal(c.blob[s + 23], c.proto)
    assert np.array_equal(c.blob[s + 16].astype(np.int64) << 8 | c.blob[s + 17], c.total_len)
    assert np.all(c.blob[s + 12] == 8) and np.all(c.blob[s + 13] == 0)
    assert set(c.blob[s + 22].tolist()) == set(T.TTLS)
    L = c.lens.astype(np.int64)
    body = 14 + 4 * c.ihl.astype(np.int64) + c.l4len
    rel = {name: c.rel == k for k, name in enumerate(T.RELATIONS)}
    tl = c.total_len.astype(np.int64)
    assert np.array_equal(L, body + 3 * rel["padded"])
    assert np.all(tl[rel["exact"] | rel["padded"]] == (body - 14)[rel["exact"] | rel["padded"]])
    assert np.all(tl[rel["short5"]] == (body - 19)[rel["short5"]]) and np.all(tl[rel["long4"]] == (body - 10)[rel["long4"]])
    assert np.all((34 + tl - 4 * c.ihl)[rel["long_options"]] == L[rel["long_options"]])  # dp_hi == L
    pad = np.flatnonzero(rel["padded"])
    assert all(np.all(c.blob[s[pad] + L[pad] - k] != 0) for k in (1, 2, 3))
    # the orders: one multiset; mixed neighbours differ in step set
    u = T.ordered("uniform")
    assert T.ordered("mixed") is c and np.array_equal(np.sort(u.ident), c.ident) and not np.array_equal(u.ident, c.ident)
    assert np.mean(c.steps[1:] != c.steps[:-1]) > 0.95


def test_table_reaches_every_pass_two_cell():
    """Under CheckSumEnable, plan_of finds at least FLOOR cases of the table in every cell: the
    IPv4 sum past the header copy, the IPv4 sum ending at the frame's end, pass 2 entered, pass 2
    with a second iteration at every width, the same with the range ending inside the frame and at
    an odd byte, and pass 2 with dp_hi == L."""
    c = T.sweep()
    a = _plan_arrays(T.plans(1))
    L, ip_hi, l4b, dp_hi = a["L"], a["ip_hi"], a["l4b"], a["dp_hi"]
    fill = (c.steps & T.DPDK_FILL) != 0
    assert np.all(l4b[l4b > 0] == dp_hi[l4b > 0]) and np.all(a["go_hi"][l4b > 0] == L[l4b > 0])
    cells = {"ip_hi > 52": ip_hi > T.HDR, "ip_hi == L with the fill": (ip_hi == L) & fill,
             "pass 2 entered": l4b > T.HDR, "pass 2 with dp_hi == L": (l4b > T.HDR) & (dp_hi == L)}
    for g in T.WIDTHS:
        second = l4b > T.ITER_BYTES * g
        cells[f"G{g}: pass 2, second iteration"] = second
        cells[f"G{g}: the same, ending inside the frame"] = second & (l4b < L)
        cells[f"G{g}: the same, ending at an odd byte"] = second & (l4b % 2 == 1)
    counts = {name: int(m.sum()) for name, m in cells.items()}
    print(counts)
    short = {name: k for name, k in counts.items() if k < FLOOR}
    assert not short, short
    # pass 1's later iterations see an IPv4 tail and an L4 range that ends inside the frame as well
    for g in T.WIDTHS:
        assert int(((ip_hi > T.HDR) & (a["l4a"] > T.ITER_BYTES * g)).sum()) >= FLOOR
        assert int(((a["l4a"] > T.ITER_BYTES * g) & (a["l4a"] < L)).sum()) >= FLOOR
    # with CheckSumEnable off no UDP / TCP recalculation is summed, so pass 2 never runs
    assert not _plan_arrays(T.plans(0))["l4b"].any()


def test_uniform_order_has_whole_waves_of_every_class():
    u = T.ordered("uniform")
    cls = [T.plans(1)[i]["cls"] for i in u.ident.tolist()]
    runs = collections.defaultdict(int)
    k = 0
    while k < len(cls):
        j = k
        while j < len(cls) and cls[j] == cls[k]:
            j += 1
        runs[cls[k]] = max(runs[cls[k]], j - k)
        k = j
    assert set(runs) == {p["cls"] for p in T.plans(1)} and len(runs) >= 20
    assert {"iptail/go+dp>52", "ipgen/go+dp>52", "iptail/go+dp<=52", "ip34/go", "ip34/dp", "ip0/-"} <= set(runs)
    short = {name: n for name, n in runs.items() if n < RUN}
    assert not short, short
    # and in the mixed order no wave of 64 neighbours that holds a pass-2 case is of one class
    m = [p["cls"] for p in T.plans(1)]
    waves = [set(m[k:k + 64]) for k in range(0, len(m), 64)]
    loop = [w for w in waves if any(name.endswith("+dp>52") for name in w)]
    assert len(loop) > 200 and all(len(w) >= 3 for w in loop)


def test_fixtures_do_not_reach_pass_two():
    """What the committed fixtures (tests/golden/tx.json) reach, by the same plan_of: no entry
    enters the pass-2 loop under either flag value, and the IPv4 tail and a fill range that ends
    inside the frame past byte 64 are reached by three entries each under each flag value, all
    82-byte frames. (An extended fixture set changes these figures with it.)"""
    from tests.helpers import tx_golden

    meta, blob, _ = tx_golden(ROOT)
    assert len(meta["entries"]) == 3025
    for flag in (0, 1):
        plans = []
        for e in meta["entries"]:
            f = meta["frames"][e["frame"]]
            plans.append(T.plan_of(blob[f["offset"]:f["offset"] + f["len"]], e["op"][0], flag))
        a = _plan_arrays(plans)
        assert int((a["l4b"] > T.HDR).sum()) == 0
        tail = a["ip_hi"] > T.HDR
        inside = (a["dp_hi"] > 64) & (a["dp_hi"] < a["L"])
        assert int(tail.sum()) == 3 and set(a["L"][tail].tolist()) == {82}
        assert int(inside.sum()) == 3 and set(a["L"][inside].tolist()) == {82}


@pytest.fixture(scope="module")
def mixed_oracle(oracle_lib):
    """flag -> (layout, the C oracle's buffer and result bytes) of the mixed order (shared, read-only)."""
    c = T.ordered("mixed")
    lay = T.layout(c, np.random.default_rng(0x1A70))
    return lay, {flag: oracle_lib.tx_batch(*lay, c.ops, flags=flag, threads=4) for flag in (0, 1)}


def test_every_result_byte_occurs(mixed_oracle):
    _lay, want = mixed_oracle
    for flag in (0, 1):
        assert set(want[flag][1].tolist()) == set(range(8)), flag


def test_oracle_equals_python_reference(mixed_oracle):
    """The C oracle's frames and result bytes == the Python restatement's (oracle/ref_tx_py.tx_frame)
    on every 5th case of the table, both flag values: every (protocol, IHL, total-length relation)
    cell and every step set is in the sample. A few seconds of per-byte Python checksums."""
    from oracle import ref_tx_py as R

    c = T.ordered("mixed")
    (data, offs, lens), want = mixed_oracle
    pick = np.arange(0, len(lens), 5)
    cells = set(zip(c.proto[pick].tolist(), c.ihl[pick].tolist(), c.rel[pick].tolist()))
    assert cells == {(p, i, r) for p in T.PROTOS for i in T.IHLS for r in range(len(T.RELATIONS))}
    assert set(T.STEP_SETS) <= set(c.steps[pick].tolist())
    for i in pick.tolist():
        o, n = int(offs[i]) * 4, int(lens[i])
        op = c.ops[i]
        for flag in (0, 1):
            b = bytearray(data[o:o + n].tobytes())
            r = R.tx_frame(b, int(op["steps"]), int(op["dst_ip"]), int(op["dst_port"]), int(op["src_ip"]),
                           int(op["src_port"]), check_sum_enable=bool(flag))
            out, res = want[flag]
            assert r == int(res[i]) and bytes(b) == out[o:o + n].tobytes(), T.describe(c, i, flag)


def test_oracle_touches_nothing_but_headers(mixed_oracle):
    """The oracle leaves gaps, padding dwords and every byte past the header copy as they were."""
    c = T.ordered("mixed")
    (data, offs, lens), want = mixed_oracle
    keep = np.ones(len(data), bool)
    for o, n in zip((offs.astype(np.int64) * 4).tolist(), lens.tolist()):
        keep[o + 14:o + min(n, T.HDR)] = False
    for flag in (0, 1):
        assert np.array_equal(want[flag][0][keep], data[keep]) and not np.array_equal(want[flag][0], data)


def test_buffer_comparison_names_the_case(mixed_oracle):
    c = T.ordered("mixed")
    (data, offs, lens), want = mixed_oracle
    out, res = want[1]
    T.first_difference(c, 1, out.copy(), out, offs, res.copy(), res, "same")
    i = 4321 + int(np.flatnonzero(lens[4321:] % 4 == 1)[0])  # its last dword has padding bytes of its own
    o, n = int(offs[i]) * 4, int(lens[i])
    for at, where in ((o + 40, "frame offset 40"), (o + n, "0 bytes behind the frame")):
        got = out.copy()
        got[at] ^= 0x5A
        with pytest.raises(AssertionError, match=f"{where}.*case {i} .*IHL {int(c.ihl[i])} L {n} .*plan"):
            T.first_difference(c, 1, got, out, offs, res, res, "stray")
    bad = res.copy()
    bad[i] ^= 4
    with pytest.raises(AssertionError, match=f"result bytes differ.*case {i} "):
        T.first_difference(c, 1, out, out, offs, bad, res, "res")
