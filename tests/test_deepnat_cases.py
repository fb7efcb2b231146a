"""CPU: what the hostile-quote corpus of tests/deepnat_cases.py reaches, from the references alone.
The C restatement (ora_icmp_quote / ora_icmp_deep_nat) and the Python one (ref_tx_py.icmp_quote /
icmp_ttl_deep_nat) agree on every row under both CheckSumEnable values, and the coverage the GPU
tests of tests/test_gpu_deep_nat.py rely on is asserted from the C oracle's output: a condition
the corpus misses is a reason to change the generator, not the condition."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import ref_py as R
from oracle import ref_tx_py as T
from tests import deepnat_cases as D


@pytest.fixture(scope="module")
def ran(oracle_lib):
    """en -> (quote records, rewritten frames, applied flags) of the C oracle over the corpus."""
    c = D.corpus()
    out = {}
    for en in (0, 1):
        q = np.zeros(len(c.frames), oracle_lib.RESULT_DTYPE)
        frames, applied = [], np.zeros(len(c.frames), bool)
        for k, f in enumerate(c.frames):
            q[k] = oracle_lib.icmp_quote(f, en)
            w, ok = oracle_lib.icmp_deep_nat(f, int(c.nat["lan_ip"][k]), int(c.nat["lan_port"][k]),
                                             bool(c.nat["found"][k]), en)
            frames.append(w)
            applied[k] = ok
        out[en] = (q, frames, applied)
    return out


def test_corpus_shape():
    c = D.corpus()
    n, total = len(c.frames), int(c.lens.sum())
    assert 3500 <= n <= 4500 and 2_000_000 <= total <= 4_000_000, (n, total)
    assert int(c.lens.max()) == 65535 and int((c.lens == 65535).sum()) == 1
    assert D.corpus() is c and not c.nat.flags.writeable
    hostile = c.kind == "hostile"
    for proto in D.PROTOS:
        rows = hostile & (c.proto == proto)
        assert set(range(28, 42)) <= set(c.qlen[rows].tolist()), proto
        assert {0, 1} == set((c.qlen[rows] & 1).tolist()), proto
        assert set(range(0, 10)) == set(c.pad[rows].tolist()), proto
        for lo, hi in [(e - 4, e + 4) for e in D.EDGES] + [(D.MAX_FRAME - 4, D.MAX_FRAME)]:
            assert set(range(lo, hi + 1)) <= set(c.lens[rows].tolist()), (proto, lo)
    assert set(c.nat["found"].tolist()) == {0, 1, 255}


def test_pack_layout():
    c = D.corpus()
    data, offs, lens = D.pack(c.frames, np.random.default_rng(3))
    start = offs.astype(np.int64) * 4
    end = start + ((lens.astype(np.int64) + 3) & ~3)
    gaps = start[1:] - end[:-1]
    assert set(gaps.tolist()) == {0, 4, 8, 12} and data.size - int(end[-1]) in (64, 68, 72, 76)
    outside = np.ones(data.size, bool)
    for o, f in zip(start.tolist(), c.frames):
        assert data[o:o + len(f)].tobytes() == f
        outside[o:o + len(f)] = False
    assert outside.sum() > 64 and np.all(data[outside] != 0)


def _py_record(oracle_lib, frame: bytes, en: int):
    rec = np.zeros(1, oracle_lib.RESULT_DTYPE)[0]
    rec["ethertype"], rec["ip_proto"] = 0x0800, 0xFF
    st, args = ("ETH_LEN", None) if len(frame) < 14 else T.icmp_quote(frame[14:], bool(en))
    rec["status"] = R.STATUS.index(st)
    if args:
        rec["ip_proto"], rec["src_ip"], rec["sport"], rec["dst_ip"], rec["dport"] = args
    return rec


def test_c_and_python_references_agree(oracle_lib, ran):
    c = D.corpus()
    for en in (0, 1):
        q, frames, applied = ran[en]
        for k, f in enumerate(c.frames):
            assert q[k].tobytes() == _py_record(oracle_lib, f, en).tobytes(), D.describe(c, k, en)
            ok, out = False, f
            if len(f) >= 14:
                eth = bytearray(f[14:])
                ok = T.icmp_ttl_deep_nat(eth, int(c.nat["lan_ip"][k]), int(c.nat["lan_port"][k]),
                                         bool(c.nat["found"][k]), bool(en))
                out = f[:14] + bytes(eth)
            assert bool(applied[k]) == ok and frames[k] == out, D.describe(c, k, en)


def test_every_row_has_the_status_it_names(ran):
    c = D.corpus()
    for en in (0, 1):
        q, _, applied = ran[en]
        bad = np.flatnonzero(q["status"] != c.status[:, en])
        assert bad.size == 0, D.describe(c, int(bad[0]), en)
        # every checksum-valid row with `found` set is applied, and nothing else
        assert np.array_equal(applied, (c.status[:, en] == 0) & (c.nat["found"] != 0))
    control = np.char.startswith(c.kind.astype(str), "control:")
    names = {k.split(":")[1] for k in c.kind[control]}
    assert names >= {f"L{L}" for L in (0, 13, 14, 33, 34, 41, 61, 1515, 1522, 9014, 65535)}
    assert names >= {"bad_icmp_cksum", "bad_ip_cksum", "type3", "type8", "quote27", "found0", "found1", "found255"}
    assert np.all(c.status[~control] == 0)


@pytest.mark.parametrize("en", [0, 1])
def test_coverage_of_the_rewrite(ran, en):
    c = D.corpus()
    _, frames, applied = ran[en]
    other = ~np.isin(c.proto, (1, 6, 17))
    for name, rows in (("icmp", c.proto == 1), ("tcp", c.proto == 6), ("udp", c.proto == 17), ("other", other)):
        assert (applied & rows).sum() >= 50, name
    tcp = applied & (c.proto == 6)
    assert (tcp & (c.qlen >= 28) & (c.qlen <= 37)).sum() >= 20 and (tcp & (c.qlen >= 38)).sum() >= 20
    assert (applied & (c.proto == 17) & (c.qlen >= 28)).sum() >= 20
    assert (applied & (c.inner_tl < 20)).sum() >= 10
    small = applied & (c.lens <= D.MAX_FRAME)
    step = (((c.lens + 3) >> 2) - 1) // 64  # the last 64-dword staging step the frame's dwords need
    for s in range(6):
        for r in range(4):
            assert (small & (step == s) & (c.lens % 4 == r)).any(), (s, r)
    assert (applied & (c.lens == D.MAX_FRAME)).any()
    assert not applied[c.lens > D.MAX_FRAME].any()
    # an applied frame differs from its input; a padded one leaves with an ICMP sum that does not
    # verify over its total length (NatChangeDst sums the untrimmed payload)
    k = int(np.flatnonzero(applied & (c.pad > 0) & (c.pad % 2 == 0))[0])
    tl = int.from_bytes(frames[k][16:18], "big")
    assert frames[k] != c.frames[k] and R.get_checksum(frames[k][34:14 + tl]) != 0
    assert R.get_checksum(frames[k][34:]) == 0


def test_zero_sum_rows_store_zero(ran):
    c = D.corpus()
    _, frames, applied = ran[1]
    zero = np.flatnonzero(c.zero_at >= 0)
    per = {}
    for k in zero:
        at = int(c.zero_at[k])
        assert applied[k] and frames[k][at:at + 2] == b"\0\0", D.describe(c, int(k), 1)
        assert c.frames[k][at:at + 2] != b"\0\0", D.describe(c, int(k), 1)  # the zero is the kernel's, not the input's
        per.setdefault(c.kind[k], set()).add(int(c.proto[k]))
    assert set(per) == {"zero:" + name for name in D.ZERO_AT}
    for name in ("inner_ip", "outer_ip", "outer_icmp"):
        assert per["zero:" + name] == {1, 6, 17} and (c.kind == "zero:" + name).sum() >= 4, name
    for name, proto in (("inner_icmp", 1), ("inner_tcp", 6), ("inner_udp", 17)):
        assert per["zero:" + name] == {proto} and (c.kind == "zero:" + name).sum() >= 4, name
    # the UDP rows: Go stores the zero as it is, where DPDK's fill would send 0xFFFF
    assert all(frames[k][D.ZERO_AT["inner_udp"]:][:2] == b"\0\0" for k in np.flatnonzero(c.kind == "zero:inner_udp"))
