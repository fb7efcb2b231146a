"""GPU: IcmpTtlDeepNat (engine/icmp_engine.go:55-86) — halo_tx_icmp_deep_nat_batch_device through
the C ABI against the committed fixtures (tests/gen_golden_deepnat.py, the Python restatement)
and the C oracle (ora_icmp_quote / ora_icmp_deep_nat), bit-exact: quote records, rewritten frames
and the applied flags; the quote records' NAT_WAN flow keys are NatGetFlowByWan's. The second half
runs the hostile-quote corpus of tests/deepnat_cases.py: whole buffers with random gaps, guard
elements behind the outputs, batch sizes around a block, absent outputs, and the forward path's
order (this kernel, then tx_fixup, on one stream over one buffer)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from tests import deepnat_cases as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dn():
    g = os.path.join(ROOT, "tests", "golden")
    meta = json.load(open(os.path.join(g, "deep_nat.json")))
    blob = np.fromfile(os.path.join(g, "deep_nat.bin"), dtype=np.uint8)
    expect = np.fromfile(os.path.join(g, "deep_nat_expect.bin"), dtype=np.uint8)
    return meta, blob, expect


def _run(dev, data, offs, lens, en, nat=None):
    import torch

    from halo_amd import protocol

    n = len(lens)
    d = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    o = torch.from_numpy(np.ascontiguousarray(offs.astype(np.uint32)).view(np.int32)).to(dev)
    ln = torch.from_numpy(np.ascontiguousarray(lens.astype(np.uint16)).view(np.int16)).to(dev)
    q = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=dev)
    a = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    nd = None if nat is None else torch.from_numpy(nat.view(np.uint8)).to(dev)
    protocol.icmp_ttl_deep_nat_batch(d, o, ln, nat=nd, check_sum_enable=bool(en), quote=q, applied=a)
    torch.cuda.synchronize()
    return d.cpu().numpy(), protocol.records(q), a.cpu().numpy()


def _arrays(meta, blob):
    fr = meta["frames"]
    offs = np.array([e["offset"] // 4 for e in fr], np.uint32)
    lens = np.array([e["len"] for e in fr], np.uint16)
    return blob.copy(), offs, lens


@pytest.mark.parametrize("en", [0, 1])
def test_quote_records_vs_oracle_and_fixtures(dev, dn, oracle_lib, en):
    meta, blob, _ = dn
    data, offs, lens = _arrays(meta, blob)
    out, q, a = _run(dev, data, offs, lens, en)
    assert np.array_equal(out, data), "frames must be untouched without NAT results"
    assert np.all(a == 0)
    for k, e in enumerate(meta["frames"]):
        f = blob[e["offset"]:e["offset"] + e["len"]].tobytes()
        want = oracle_lib.icmp_quote(f, en)
        assert q[k].tobytes() == want.tobytes(), e["name"]
        assert int(q[k]["status"]) == e["quote"][str(en)]["status"], e["name"]


@pytest.mark.parametrize("en", [0, 1])
@pytest.mark.parametrize("found", [0, 1])
def test_rewrite_vs_fixtures(dev, dn, en, found):
    from halo_amd._lib import DEEP_NAT_DTYPE

    meta, blob, expect = dn
    data, offs, lens = _arrays(meta, blob)
    nat = np.zeros(len(lens), DEEP_NAT_DTYPE)
    nat["lan_ip"], nat["lan_port"], nat["found"] = meta["lan_ip"], meta["lan_port"], found
    out, _, a = _run(dev, data, offs, lens, en, nat)
    k_ = f"{en}{found}"
    for k, e in enumerate(meta["frames"]):
        o, eo, L = e["offset"], e["expect_offset"][k_], e["len"]
        assert int(a[k]) == e["applied"][k_], e["name"]
        assert out[o:o + L].tobytes() == expect[eo:eo + L].tobytes(), e["name"]


def test_random_ttl_messages_vs_oracle(dev, oracle_lib):
    """20k time-exceeded frames quoting random UDP/TCP/ICMP packets at random quote lengths, a
    quarter corrupted by one bit, random NAT results: every frame and flag vs the oracle."""
    from halo_amd._lib import DEEP_NAT_DTYPE
    from oracle import ref_py as R

    rng = np.random.default_rng(0xD33F)
    frames = []
    for k in range(20_000):
        proto = int(rng.choice([1, 6, 17]))
        pl = bytes(rng.integers(0, 256, int(rng.integers(0, 600)), dtype=np.uint8))
        src, dst = bytes(rng.integers(0, 256, 4, dtype=np.uint8)), bytes(rng.integers(0, 256, 4, dtype=np.uint8))
        if proto == 17:
            seg = R.build_udp(pl, int(rng.integers(1, 65536)), int(rng.integers(1, 65536)), src, dst)
        elif proto == 6:
            seg = R.build_tcp(pl, int(rng.integers(1, 65536)), int(rng.integers(1, 65536)), src, dst, 1, 2, 0x10)
        else:
            seg = R.build_icmp(pl, 8, bytes(rng.integers(0, 256, 2, dtype=np.uint8)), 5)
        inner = R.build_ipv4(seg, proto, src, dst)
        q = inner[:int(rng.integers(20, len(inner) + 1))]
        msg = R.build_icmp(q, 11, b"\0\0", 0)
        f = bytearray(R.build_eth(R.build_ipv4(msg, 1, bytes([192, 0, 2, 1]), src), bytes(6), bytes(6), 0x0800))
        if rng.integers(0, 8) == 0:
            f += bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8))  # padding
        if rng.integers(0, 4) == 0:
            bit = int(rng.integers(14 * 8, len(f) * 8))
            f[bit >> 3] ^= 1 << (bit & 7)
        frames.append(bytes(f))
    lens = np.array([len(f) for f in frames], np.uint16)
    sizes = (lens.astype(np.int64) + 3) & ~3
    offs = np.zeros(len(frames), np.int64)
    offs[1:] = np.cumsum(sizes)[:-1]
    data = np.zeros(int(sizes.sum()) + 16, np.uint8)
    for o, f in zip(offs, frames):
        data[o:o + len(f)] = np.frombuffer(f, np.uint8)
    nat = np.zeros(len(frames), DEEP_NAT_DTYPE)
    nat["lan_ip"] = rng.integers(0, 1 << 32, len(frames), dtype=np.uint64).astype(np.uint32)
    nat["lan_port"] = rng.integers(0, 1 << 16, len(frames))
    nat["found"] = rng.integers(0, 8, len(frames)) != 0
    for en in (0, 1):
        out, q, a = _run(dev, data, offs // 4, lens, en, nat)
        n_applied = 0
        for k, f in enumerate(frames):
            want_q = oracle_lib.icmp_quote(f, en)
            assert q[k].tobytes() == want_q.tobytes(), k
            wf, ok = oracle_lib.icmp_deep_nat(f, int(nat["lan_ip"][k]), int(nat["lan_port"][k]), bool(nat["found"][k]), en)
            assert int(a[k]) == int(ok), k
            assert out[offs[k]:offs[k] + len(f)].tobytes() == wf, k
            n_applied += ok
        assert n_applied > 10_000


def test_quote_flow_key_is_nat_get_flow_by_wan(dev, dn, oracle_lib):
    """hashcode(NAT_WAN) of the GPU quote records == the oracle's hash of a record built from the
    Python restatement's NatGetFlowByWan arguments (remote ip/port, wan ip/port, proto)."""
    import torch

    from halo_amd import hashcode
    from halo_amd._lib import FLOW_NAT_WAN, NAT_SYMMETRIC

    meta, blob, _ = dn
    data, offs, lens = _arrays(meta, blob)
    _, q, _ = _run(dev, data, offs, lens, 1)
    ok = [k for k, e in enumerate(meta["frames"]) if e["quote"]["1"]["args"]]
    recs = torch.from_numpy(q[ok].view(np.uint8).reshape(-1, 32).copy()).to(dev)
    h, _ = hashcode.flow_hash(recs, FLOW_NAT_WAN, NAT_SYMMETRIC)
    want = np.zeros(len(ok), oracle_lib.RESULT_DTYPE)
    for j, k in enumerate(ok):
        proto, remote, rport, wan, wport = meta["frames"][k]["quote"]["1"]["args"]
        want[j]["ip_proto"], want[j]["src_ip"], want[j]["sport"] = proto, remote, rport
        want[j]["dst_ip"], want[j]["dport"] = wan, wport
    wh, _ = oracle_lib.flow_hash_batch(want, FLOW_NAT_WAN, NAT_SYMMETRIC)
    assert np.array_equal(h.cpu().numpy().view(np.uint64), wh)


# ---- the hostile-quote corpus (tests/deepnat_cases.py): whole buffers, guards, batch sizes --------
GUARD = 0xA5


def _launch(dev, data, offs, lens, en, nat, n=None, quote=True, applied=True, then=None):
    """One call over the first n frames (default: all) with `quote` / `applied` prefilled with GUARD
    and one guard element behind each; `then(d, o, ln)` queues more work on the same stream before
    the one synchronize. Returns (buffer, quote bytes [n + 1, 32] or None, applied [n + 1] or None)."""
    import torch

    from halo_amd import protocol

    n = len(lens) if n is None else n
    d = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    o = torch.from_numpy(np.ascontiguousarray(offs[:n].astype(np.uint32)).view(np.int32)).to(dev)
    ln = torch.from_numpy(np.ascontiguousarray(lens[:n].astype(np.uint16)).view(np.int16)).to(dev)
    q = torch.full((n + 1, 32), GUARD, dtype=torch.uint8, device=dev) if quote else None
    a = torch.full((n + 1,), GUARD, dtype=torch.uint8, device=dev) if applied else None
    nd = None if nat is None else torch.from_numpy(np.array(nat[:n]).view(np.uint8)).to(dev)  # (a writable copy)
    protocol.icmp_ttl_deep_nat_batch(d, o, ln, nat=nd, check_sum_enable=bool(en), quote=q, applied=a)
    extra = then(d, o, ln) if then else None
    torch.cuda.synchronize()
    out = (d.cpu().numpy(), None if q is None else q.cpu().numpy(), None if a is None else a.cpu().numpy())
    return out + (extra,) if then else out


def _check_outputs(c, idx, en, q, a, want_q, want_a, what):
    """Quote records byte for byte, applied flags, and the guard element behind each."""
    n = len(want_a)
    if q is not None:
        assert np.all(q[n] == GUARD), f"{what}: the quote record behind the last was written"
        bad = np.flatnonzero(np.any(q[:n] != want_q.view(np.uint8).reshape(n, 32), axis=1))
        assert bad.size == 0, (f"{what}: {bad.size} quote records differ; first got {q[bad[0]].tobytes().hex()} want "
                               f"{want_q[bad[0]].tobytes().hex()}; {D.describe(c, int(bad[0] if idx is None else idx[bad[0]]), en)}")
    if a is not None:
        assert a[n] == GUARD, f"{what}: the applied flag behind the last was written"
        bad = np.flatnonzero(a[:n] != want_a)
        assert bad.size == 0, (f"{what}: {bad.size} applied flags differ; first got {int(a[bad[0]])} want "
                               f"{int(want_a[bad[0]])}; {D.describe(c, int(bad[0] if idx is None else idx[bad[0]]), en)}")


@pytest.fixture(scope="module")
def hostile(oracle_lib):
    """en -> the corpus laid out once in a buffer of random bytes, and the C oracle's buffer, quote
    records and applied flags for it (computed once per en, shared, not modified)."""
    from halo_amd._lib import DEEP_NAT_DTYPE

    assert D.NAT_DTYPE == DEEP_NAT_DTYPE
    c = D.corpus()
    lay = D.pack(c.frames, np.random.default_rng(0xA11))
    wants = {}

    def get(en):
        if en not in wants:
            wants[en] = D.expected(oracle_lib, *lay, c.nat, en)
            for w in wants[en]:
                w.setflags(write=False)
        return c, lay, wants[en]

    return get


@pytest.mark.parametrize("en", [0, 1])
def test_hostile_quotes_whole_buffer(dev, hostile, en):
    """The corpus in one call: checksum-valid time-exceeded messages whose quote is hostile (any
    IHL, total length and protocol byte, TCP quotes below the guard of 38), frames in every staging
    step up to 1514 bytes, padding, rows whose recomputed checksum is 0x0000, and control rows from
    0 to 65,535 bytes. The whole buffer, gaps and tail of random bytes included, every quote record
    and every applied flag equal the C oracle's; the guard elements behind both outputs survive."""
    c, (data, offs, lens), (want, want_q, want_a) = hostile(en)
    got, q, a = _launch(dev, data, offs, lens, en, c.nat)
    what = f"GPU deep NAT corpus en={en}"
    _check_outputs(c, None, en, q, a, want_q, want_a, what)
    D.first_difference(c, None, en, got, want, offs, lens, what)
    assert int(want_a.sum()) > 3000


@pytest.fixture(scope="module")
def applied_rows(oracle_lib):
    """The corpus rows the rewrite applies to under either CheckSumEnable value."""
    c = D.corpus()
    return np.flatnonzero((c.status[:, 0] == 0) & (c.status[:, 1] == 0) & (c.nat["found"] != 0))


def test_batch_sizes_around_a_block(dev, oracle_lib, applied_rows):
    """Prefixes of 41 applied rows with n on both sides of one and two blocks of four waves: the
    `i >= n` exit and the last block's idle waves. The frames behind the prefix are in the buffer
    and belong to what must stay untouched."""
    c = D.corpus()
    idx = applied_rows[np.linspace(0, len(applied_rows) - 1, 41).astype(np.int64)]
    nat = c.nat[idx]
    data, offs, lens = D.pack([c.frames[k] for k in idx], np.random.default_rng(0xB10C))
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 41):
        want, want_q, want_a = D.expected(oracle_lib, data, offs, lens, nat, 1, n=n)
        behind = int(offs[n]) * 4 if n < len(idx) else data.size
        assert want_a.all() and np.array_equal(want[behind:], data[behind:])
        got, q, a = _launch(dev, data, offs, lens, 1, nat, n=n)
        what = f"GPU deep NAT, first {n} of 41 frames"
        _check_outputs(c, idx, 1, q, a, want_q, want_a, what)
        D.first_difference(c, idx, 1, got, want, offs, lens, what)


def test_absent_outputs(dev, hostile):
    """quote and / or applied absent with NAT answers given: the buffer equals the full run's (the
    oracle's). NAT answers absent: quote records as ever, applied all zero, the buffer untouched."""
    c, (data, offs, lens), (want, want_q, want_a) = hostile(1)
    for quote, applied in ((False, True), (True, False), (False, False)):
        got, q, a = _launch(dev, data, offs, lens, 1, c.nat, quote=quote, applied=applied)
        what = f"GPU deep NAT corpus, quote {'given' if quote else 'absent'}, applied {'given' if applied else 'absent'}"
        assert (q is None) == (not quote) and (a is None) == (not applied)
        _check_outputs(c, None, 1, q, a, want_q, want_a, what)
        D.first_difference(c, None, 1, got, want, offs, lens, what)
    got, q, a = _launch(dev, data, offs, lens, 1, None)
    _check_outputs(c, None, 1, q, a, want_q, np.zeros_like(want_a), "GPU deep NAT corpus, no NAT answers")
    D.first_difference(c, None, 1, got, data, offs, lens, "GPU deep NAT corpus, no NAT answers")


@pytest.fixture(scope="module")
def forward(oracle_lib, applied_rows):
    """The forward path's batch: the corpus' applied rows and 500 plain UDP / TCP frames in a seeded
    random order, NAT answers for all of them, DNAT | TTL | SNAT with random addresses; en -> the
    buffer after oracle.icmp_deep_nat and then oracle.tx_batch, and the result bytes."""
    from halo_amd import protocol
    from oracle import ref_py as R

    c = D.corpus()
    rng = np.random.default_rng(0xF0D)
    frames, nat_rows = [c.frames[k] for k in applied_rows], [c.nat[k] for k in applied_rows]
    for k in range(500):
        src, dst = bytes(rng.integers(0, 256, 4, dtype=np.uint8)), bytes(rng.integers(0, 256, 4, dtype=np.uint8))
        pl = bytes(rng.integers(0, 256, int(rng.integers(0, 1400)), dtype=np.uint8))
        sp, dp = int(rng.integers(1, 65536)), int(rng.integers(1, 65536))
        seg = R.build_udp(pl, sp, dp, src, dst) if k & 1 else R.build_tcp(pl, sp, dp, src, dst, 1, 2, 0x10)
        ip = R.build_ipv4(seg, 17 if k & 1 else 6, src, dst, ttl=int(rng.choice([1, 2, 64, 255])))
        frames.append(R.build_eth(ip, bytes(6), bytes(6), 0x0800))
        nat_rows.append(np.array((int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 16)), 1, 0), D.NAT_DTYPE))
    order = rng.permutation(len(frames))
    idx = np.concatenate([applied_rows, np.full(500, -1)])[order]
    nat = np.array(nat_rows, D.NAT_DTYPE)[order]
    lay = D.pack([frames[k] for k in order], rng)
    ops = protocol.tx_ops(len(frames), protocol.TX_NAT_DST | protocol.TX_TTL | protocol.TX_NAT_SRC)
    for f in ("dst_ip", "src_ip"):
        ops[f] = rng.integers(0, 1 << 32, len(frames), dtype=np.uint64).astype(np.uint32)
    for f in ("dst_port", "src_port"):
        ops[f] = rng.integers(0, 1 << 16, len(frames))
    wants = {}

    def get(en):
        if en not in wants:
            mid, _, applied = D.expected(oracle_lib, *lay, nat, en)
            assert np.array_equal(applied != 0, idx >= 0)
            wants[en] = oracle_lib.tx_batch(mid, lay[1], lay[2], ops, flags=en, threads=8)
        return idx, nat, lay, ops, wants[en]

    return get


@pytest.mark.parametrize("en", [0, 1])
@pytest.mark.parametrize("g", [4, 16])
def test_forward_order_deep_nat_then_fixup(dev, forward, g, en):
    """Ipv4RouteForward's order on one buffer: IcmpTtlDeepNat, then DNAT, TTL and SNAT of the same
    bytes, as two kernels back to back on one stream with no synchronize between them. The whole
    buffer equals oracle.icmp_deep_nat followed by oracle.tx_batch, at 4 and at 16 lanes per frame
    in the second kernel."""
    import torch

    from halo_amd import protocol
    from tests import tx_cases as T

    hint = T.HINTS[g]
    assert T.width_of(hint) == g
    idx, nat, (data, offs, lens), ops, (want, want_res) = forward(en)

    res = torch.full((len(lens),), GUARD, dtype=torch.uint8, device=dev)
    op = torch.from_numpy(np.ascontiguousarray(ops).view(np.uint8)).to(dev)  # before the first kernel: no copy between

    def fixup(d, o, ln):
        protocol.tx_fixup_batch(d, o, ln, op, check_sum_enable=bool(en), max_len_hint=hint, result=res)
        return res

    got, _, _, res = _launch(dev, data, offs, lens, en, nat, then=fixup)
    what = f"GPU deep NAT then tx_fixup G{g} en={en}"
    bad = np.flatnonzero(res.cpu().numpy() != want_res)
    assert bad.size == 0, f"{what}: {bad.size} result bytes differ, first at position {int(bad[0])}"
    c = D.corpus()
    if not np.array_equal(got, want):  # name the frame; a plain frame (row -1) is described by its position
        first = int(np.searchsorted(offs.astype(np.int64) * 4, int(np.flatnonzero(got != want)[0]), side="right")) - 1
        assert idx[first] >= 0, f"{what}: buffers differ first in plain frame at position {first}, L {int(lens[first])}"
        D.first_difference(c, idx, en, got, want, offs, lens, what)
