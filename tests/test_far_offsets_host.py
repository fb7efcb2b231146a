"""CPU: the far placements of tests/far_cases.py through the host twins over a sparse numpy buffer of
8 GiB + 64 MiB (only the pages of the four bands are ever committed): halo_switch_forward in host
mode, halo_tx_egress_host, halo_lo_gather_host, halo_rx_deliver_host, halo_tx_respond_host and the
CPU parse entry, against the same models and the same expectations tests/test_gpu_far_offsets.py
holds the device entries to. This is what shows, without a GPU, that the placement helper and the
expectations are right at byte offsets past 4 GiB and dword offsets past 2^31. Also: the placement's
own geometry, and the completeness check — every HALO_API entry of include/halo_rx.h that takes
`d_offsets_dw` has a row in the GPU file's table."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from tests import far_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
N = F.N_FRAMES


@pytest.fixture(scope="module")
def far():
    """One sparse buffer for the module; every test writes its own bands into it."""
    buf = F.new_host_buffer()
    yield buf
    del buf


# ---- the placement itself --------------------------------------------------------------------------
@pytest.mark.parametrize("order", F.ORDERS)
def test_placement_geometry(order):
    rng = np.random.default_rng(3)
    lens = rng.choice(np.array([0, 14, 42, 60, 61, 62, 63, 64, 100, 1514]), N)
    which = F.band_of(N, order)
    for b in (1, 2):  # the pivots are whole frames
        m = np.flatnonzero(which == b)
        if m.size:
            lens[m[m.size // 2]] = 64
    offs, ln, bands = F.place(lens, order)
    o = offs.astype(np.int64) * 4
    end = o + lens
    assert offs.dtype == np.uint32 and ln.dtype == np.uint16 and np.array_equal(ln, lens)
    # frames do not overlap, lie on dword boundaries, inside the buffer, inside their band
    by_addr = np.argsort(o, kind="stable")
    assert np.all(o[by_addr][1:] >= ((end + 3) & ~3)[by_addr][:-1]) and int(((end + 3) & ~3).max()) <= F.FAR_BYTES
    for b in bands:
        assert np.all(o[b.members] >= b.lo) and np.all(end[b.members] <= b.hi)
        assert b.span_lo == max(b.lo - 64, 0) and b.span_hi == min(b.hi + 64, F.FAR_BYTES)
        # dense: each member starts where the one before it ends (padded)
        assert np.array_equal(o[b.members][1:], ((end + 3) & ~3)[b.members][:-1])
    d = F.describe((offs, ln, bands))
    assert d["last_end"] == F.FAR_BYTES  # T ends at the buffer's last byte
    assert int(o.min()) == 0             # N starts at byte 0
    if order == "first_far":
        assert d["bands"] == ["N", "T"]
        assert np.all(o[::64] > F.MARK8) and np.all(np.delete(o, np.s_[::64]) < (1 << 22))
        return
    assert d["bands"] == ["N", "X4", "X8", "T"]
    x4, x8 = bands[1], bands[2]
    p4, p8 = x4.members[len(x4.members) // 2], x8.members[len(x8.members) // 2]
    assert int(o[p4]) == (1 << 32) - 20 and int(o[p8]) == 1 << 33
    assert len(x4.members) // 2 >= 64 and len(x4.members) - len(x4.members) // 2 - 1 >= 64
    # T and the upper half of X8 start at or past 8 GiB; the lower half of X8 and the frames after X4's pivot past 4 GiB
    assert d["beyond_8g"] == N // 4 + N // 8 and d["beyond_4g"] == d["beyond_8g"] + N // 8 + N // 8 - 1
    assert d["straddle_4g"] == 1 and d["at_8g"] >= 1
    assert int((offs >= 1 << 31).sum()) == d["beyond_8g"] and int((offs.view(np.int32) < 0).sum()) == d["beyond_8g"]
    if order == "banded":
        assert np.all(np.diff(o) >= 0)  # index order is memory order
    else:
        step = np.diff(o[:64])
        assert (step > (1 << 31)).any() and (step < -(1 << 32)).any()  # rising and falling steps inside one window
        assert all(len(set(F.band_of(N, order)[w:w + 64])) == 4 for w in range(0, N, 64))


def test_host_buffer_round_trip_and_truncated_offsets_disagree(far):
    """What to_host wrote is read back frame by frame through the u32 offsets; the same read with
    offsets cut to 30 bits (a 32-bit byte address) finds other bytes for every frame past 4 GiB."""
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes() for ln in rng.choice([42, 60, 64, 100, 1514], N)]
    for order in F.ORDERS:
        pl = F.place(frames, order)
        F.to_host(pl, frames, far)
        F.assert_bands(pl, far, frames, order)
        for i, at in enumerate(F.byte_offsets(pl[0])):
            assert far[at:at + len(frames[i])].tobytes() == frames[i]
        wrapped = [(at & 0xFFFFFFFF) for at in F.byte_offsets(pl[0])]
        wrong = sum(far[w:w + len(frames[i])].tobytes() != frames[i] for i, w in enumerate(wrapped))
        assert wrong == F.describe(pl)["beyond_4g"] > 0


# ---- the CPU parse entry ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", F.ORDERS)
def test_cpu_parse_entry(far, oracle_lib, order):
    from halo_amd import cpu, synth
    from halo_amd._lib import NetIf

    lay = synth.layout(N, size_mode=synth.SIZE_IMIX, proto_mode=synth.PROTO_MIX, mutate_shift=3, first_index=55)
    on = oracle_lib.NetIf.make()
    data = oracle_lib.synth_batch(synth.SEED, 55, lay["lens"], lay["kinds"], on, offsets_dw=lay["offsets_dw"])
    want, whist = oracle_lib.rx_batch(data, lay["lens"], on, 1, offsets_dw=lay["offsets_dw"])
    assert np.count_nonzero(want["status"]) > N // 40
    frames = F.frames_of(data, lay["offsets_dw"], lay["lens"])
    pl = F.place(frames, order)
    F.to_host(pl, frames, far)
    hist = np.zeros(14, np.uint32)
    got = cpu.parse_frames_cpu(far, pl[0].astype(np.uint64) * 4, pl[1], netif=NetIf.make(), hist=hist)
    assert got.tobytes() == want.tobytes() and np.array_equal(hist, whist)
    # the oracle itself at the far offsets: the expectation does not depend on the placement
    far_want, _ = oracle_lib.rx_batch(far, pl[1], on, 1, offsets_dw=pl[0])
    assert far_want.tobytes() == want.tobytes()


# ---- the switch -------------------------------------------------------------------------------------
def test_switch_host(far):
    from halo_amd.switch import Switch
    from tests import switch_cases as K
    from tests import switch_model as M

    vlans = [1, 1, 1, 2, 2, 2, 3, 3]
    sw, model = Switch(vlans, 128, max_batch=N), M.SwitchModel(vlans, 128)
    rng = np.random.default_rng(21)
    seen = np.zeros(6, np.uint64)
    for call, order in enumerate(F.ORDERS * 2):  # the second round finds the first one's MACs learned
        frames, _ = K.numpy_random_frames(rng, 300, N)
        pl = F.place(frames, order)
        F.to_host(pl, frames, far)
        res, cnt = sw.forward(call % len(vlans), far, pl[0], pl[1], 100 + call)
        v, p, t, c = model.forward(call % len(vlans), frames, 100 + call)
        assert np.array_equal(res["verdict"], v) and np.array_equal(res["out_port"], p) and np.array_equal(res["tx_len"], t)
        assert np.array_equal(cnt, c)
        seen += c
        F.assert_bands(pl, far, frames, order)
    assert M.listed(sw.ListSwitchMacAddr()) == model.entries()
    assert seen[M.UNICAST] > N and (seen > 0).all(), seen
    sw.close()


# ---- egress -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", F.ORDERS)
def test_egress_host(far, order):
    from halo_amd import egress as E
    from tests import egress_cases as C
    from tests import egress_model as EM

    frames, _, _, _, masks = C.mixed(31, N, 3)
    pl = F.place(frames, order)
    F.to_host(pl, frames, far)
    free = EM.egress(frames, masks, 3, 1 << 40)
    region = C.region_for(int(free.ports["bytes"].max()))
    cap = int(free.ports["frames"].max()) + 3
    want = EM.egress(frames, masks, 3, region, cap)
    assert want.skipped > 0 and int(want.ports["frames"].min()) > N // 8
    out = np.full(3 * region + 32, FILL, np.uint8)
    r = E.egress_host(E.EGRESS_KIND_MASKS, far, pl[0], pl[1], masks, 3, region, cap, out=out, skipped=np.array([7], np.uint32))
    assert np.array_equal(r.ports, want.ports) and r.n_skipped - 7 == want.skipped
    assert np.array_equal(r.out, want.out(FILL, size=len(out)))
    assert all(np.array_equal(r.index(p), want.index[p]) for p in range(3))
    F.assert_bands(pl, far, frames, order)


# ---- loopback gather --------------------------------------------------------------------------------
@pytest.mark.parametrize("tx", [False, True], ids=["forward", "tx"])
@pytest.mark.parametrize("order", F.ORDERS)
def test_lo_gather_host(far, order, tx):
    from halo_amd import loopback as L
    from tests import lo_cases as C
    from tests import lo_model as LM

    frames, _, _, _, results = C.mixed(77 + tx, N, 4, tx)
    pl = F.place(frames, order)
    F.to_host(pl, frames, far)
    nifs = LM.netifs_of_results(results, 4)
    free = LM.gather(frames, nifs, 4, 1 << 34, 0, tx)
    region = C.region_for(int(free.ports["bytes"].max()))
    cap = int(free.ports["frames"].max()) + 3
    want = LM.gather(frames, nifs, 4, region, cap, tx)
    assert int(want.ports["frames_written"].sum()) > N // 8 and want.skipped > 0
    out = np.full(4 * region + 64, FILL, np.uint8)
    r = L.gather_host(far, pl[0], pl[1], results, 4, region, cap, tx=tx, out=out, skipped=np.full(1, 7, np.uint32))
    assert np.array_equal(r.ports, want.ports) and r.n_skipped - 7 == want.skipped
    assert np.array_equal(r.out, want.out(FILL, size=len(out)))
    for p in range(4):
        assert np.array_equal(r.pkt_off_dw(p), np.asarray(want.pkt_off[p], np.uint32)), p
        assert np.array_equal(r.pkt_len(p), np.asarray(want.pkt_len[p], np.uint16)), p
        assert np.array_equal(r.index(p), np.asarray(want.index[p], np.uint32)), p
    F.assert_bands(pl, far, frames, order)


# ---- local delivery ---------------------------------------------------------------------------------
@pytest.mark.parametrize("order", F.ORDERS)
def test_deliver_host(far, order):
    from tests import deliver_cases as C
    from tests import deliver_model as DM
    from tests.test_deliver_host import _host

    frames = C.batch(61, N, "all")[:N // 2] + C.batch(62, N // 2, "edges")
    nif = C.model_netif()
    want = DM.want_of(frames, nif, udp_ports=C.UDP_SERVED, tcp_ports=C.TCP_SERVED, dhcp=True)
    assert len(want.recs) > N // 2
    pl = F.place(frames, order)
    F.to_host(pl, frames, far)
    recs = C.records(frames, nif)
    o = _host(far, pl[0], pl[1], recs, False, (want.total_bytes + 15) & ~15, len(want.recs) + 2)
    C.check_outputs(o, want, order)
    F.assert_bands(pl, far, frames, order)


# ---- the responders ---------------------------------------------------------------------------------
@pytest.mark.parametrize("order", F.ORDERS)
def test_respond_host(far, order):
    """halo_tx_respond_host reads no frame byte: its descriptors' payload_off must be 4 * offsets_dw[i]
    plus the payload's place in the frame, in Python integers — past 2^32 and 2^33 here — and
    tx_build's model over the far buffer at those offsets builds the reply frames."""
    from halo_amd import cpu
    from halo_amd._lib import BUILD_DESC_DTYPE, RESPOND_SRC_DTYPE
    from halo_amd.respond import respond_host, tcp_port_map
    from tests import respond_cases as C
    from tests import respond_model as RM

    frames, nat, steps, result = C.columns(C.batch(905, N, "mixed"))
    pl = F.place(frames, order)
    F.to_host(pl, frames, far)
    for nat_enable in (False, True):
        recs = cpu.parse_frames_cpu(far, pl[0].astype(np.uint64) * 4, pl[1], netif=C.lib_netif(nat_enable))
        want = RM.respond(frames, pl[0], C.model_netif(nat_enable), nat=nat, fix=(steps, result), tcp_ports=C.SERVED)
        r = respond_host(pl[0], pl[1], recs, netif=C.lib_netif(nat_enable), nat_verdict=nat, ops=C.ops_array(steps),
                         fixup_result=result, tcp_ports=tcp_port_map(C.SERVED))
        desc, src, dst_ip = want.arrays(BUILD_DESC_DTYPE, RESPOND_SRC_DTYPE)
        assert r.count == want.count > N // 8
        assert np.array_equal(r.desc, desc) and np.array_equal(r.src, src) and np.array_equal(r.dst_ip, dst_ip)
        assert np.array_equal(r.kind_counts, want.kind_counts) and np.array_equal(r.actions, want.actions)
        # payload_off in Python integers: inside the source frame, wherever that frame lies
        for k, (i, rep) in enumerate(want.replies):
            at = 4 * int(pl[0][i])
            assert at <= int(r.desc["payload_off"][k]) == rep["payload_off"] <= at + len(frames[i])
        if order != "first_far":
            assert int((r.desc["payload_off"] >= F.MARK8).sum()) > 16 and int((r.desc["payload_off"] >= F.MARK4).sum()) > 64
        # the replies built from the far buffer are those built from the frames themselves
        data, offs, _ = C.pack(3, frames)
        near = RM.respond(frames, offs, C.model_netif(nat_enable), nat=nat, fix=(steps, result), tcp_ports=C.SERVED)
        assert RM.build_frames(want.replies, far, C.MAC, 7) == RM.build_frames(near.replies, data, C.MAC, 7)


# ---- every entry that takes dword offsets has a far row ---------------------------------------------
def offsets_entries() -> list:
    """The HALO_API functions of include/halo_rx.h with a `d_offsets_dw` parameter."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "halo_rx.h")).read(), flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"HALO_API\s+[\w\s\*]+?\b(halo_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
                  if re.search(r"\bd_offsets_dw\b", m.group(2)))


def test_every_offsets_entry_has_a_far_row():
    from tests import test_gpu_far_offsets as G

    names = offsets_entries()
    assert len(names) >= 17 and "halo_rx_parse_batch_device" in names and "halo_lo_gather_device" in names
    rows = {e for entries in G.ROWS.values() for e in entries}
    missing = [n for n in names if n not in rows]
    assert not missing, f"no far-offset row in tests/test_gpu_far_offsets.py for {missing}"
    # and every row names a test of that file
    for test in G.ROWS:
        assert callable(getattr(G, test, None)), test
