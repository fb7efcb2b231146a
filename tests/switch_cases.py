"""Shared by tests/test_switch_host.py and tests/test_gpu_switch.py: a halo_amd.switch.Switch run
next to tests/switch_model.SwitchModel, compared after every call, and the edge cases of the
switch's semantics as functions of a `make(**config) -> Pair` factory (host or device)."""
from __future__ import annotations

import numpy as np

from tests import switch_model as M

BCAST = b"\xff" * 6
MCAST_SRC = bytes([0x01, 0x00, 0x5E, 0x00, 0x00, 0x01])


class Pair:
    """A Switch and its model. Every call runs on both and everything observable must be equal:
    verdicts, out_port, tx_len, the cumulative counters and the listed table."""

    total = np.zeros(6, np.uint64)  # counters over every Pair of the process (every verdict must occur)

    def __init__(self, vlans, capacity, max_batch=4096, slots_log2=0, device=None, epoch=None):
        from halo_amd.switch import Switch

        self.sw = Switch(vlans, capacity, max_batch=max_batch, slots_log2=slots_log2,
                         device=None if device is None else device.index)
        self.model = M.SwitchModel(vlans, capacity)
        self.device = device
        self.counts = None
        self.want_counts = np.zeros(6, np.uint32)
        if device is not None:
            import torch

            self.counts = torch.zeros(6, dtype=torch.int32, device=device)
            if epoch is not None:  # the scratch set's call number: start next to its wrap
                self.sw.debug_set_epoch(epoch)

    def _arrays(self, packed):
        data, offs, lens = packed
        if self.device is None:
            return data, offs, lens
        import torch

        return (torch.from_numpy(data).to(self.device), torch.from_numpy(offs.view(np.int32)).to(self.device),
                torch.from_numpy(lens.view(np.int16)).to(self.device))

    def forward_many(self, calls):
        """calls: [(port, frames, now)] or [(port, frames, now, packed)]. Every call's arrays are
        uploaded and its result buffer made first (an upload from pageable memory synchronises the
        stream); then the calls are issued in a loop that makes no transfer, allocation or other
        synchronising call, so on a device switch they queue up on the one stream behind each other;
        only then is any result read."""
        staged = []
        for c in calls:
            arrays = self._arrays(c[3] if len(c) > 3 else M.pack(c[1]))
            res = None
            if self.device is not None:
                import torch

                res = torch.empty((len(c[1]), 4), dtype=torch.uint8, device=self.device)
            staged.append((arrays, res))
        outs = []
        for c, (arrays, res) in zip(calls, staged):
            res, self.counts = self.sw.forward(c[0], *arrays, c[2], results=res, counts=self.counts)
            outs.append((arrays, res))
        got_all = []
        for (port, frames, now, *_), (_, res) in zip(calls, outs):
            v, p, t, c = self.model.forward(port, frames, now)
            self.want_counts += c
            Pair.total += c
            if self.device is not None:
                from halo_amd._lib import SW_RESULT_DTYPE

                res = res.cpu().numpy().view(SW_RESULT_DTYPE)[:, 0]
            assert np.array_equal(res["verdict"], v), ("verdict", np.flatnonzero(res["verdict"] != v)[:8])
            assert np.array_equal(res["out_port"], p), ("out_port", np.flatnonzero(res["out_port"] != p)[:8])
            assert np.array_equal(res["tx_len"], t), ("tx_len", np.flatnonzero(res["tx_len"] != t)[:8])
            got_all.append((v, p, t))
        counts = self.counts if self.device is None else self.counts.cpu().numpy().view(np.uint32)
        assert np.array_equal(counts, self.want_counts), (counts, self.want_counts)
        self.check_table()
        return got_all

    def forward(self, port, frames, now, lead_dw=None):
        packed = M.pack(frames, lead_dw)
        return self.forward_many([(port, frames, now, packed)])[0]

    def expire(self, now):
        got, want = self.sw.expire(now), self.model.expire(now)
        assert got == want, (got, want)
        self.check_table()
        return got

    def check_table(self):
        got = self.sw.ListSwitchMacAddr()
        assert len(got) == len(self.model.table)
        assert M.listed(got) == self.model.entries()
        assert int(self.sw.layout_stats()["entries"]) == len(self.model.table)

    def close(self):
        self.sw.close()


A, B, C, D = M.mac(1), M.mac(2), M.mac(3), M.mac(4)
V4 = [10, 10, 10, 20]  # ports 0-2 in VLAN 10, port 3 in VLAN 20


def case_in_batch_order(make):
    s = make(vlans=V4, capacity=16)
    s.forward(1, [M.frame(BCAST, D)], 5)  # D is in T0 on port 1
    frames = [M.frame(A, A),       # src == dst: UNICAST to the ingress port
              M.frame(B, A),       # B not yet seen: FLOOD
              M.frame(A, B),       # teaches B
              M.frame(B, A),       # now UNICAST
              M.frame(D, A),       # D held on port 1 ...
              M.frame(BCAST, D),   # ... moves to port 0 here
              M.frame(D, A)]       # ... and is port 0 from now on
    v, p, _ = s.forward(0, frames, 7)
    assert list(v) == [M.UNICAST, M.FLOOD, M.UNICAST, M.UNICAST, M.UNICAST, M.FLOOD, M.UNICAST]
    assert list(p) == [0, 0xFF, 0, 0, 1, 0xFF, 0]
    s.close()


def case_no_learning_on_drops(make):
    s = make(vlans=V4, capacity=16)
    s.forward(2, [M.frame(BCAST, B)], 1)
    frames = [M.frame(B, A, 41),               # ETH_LEN: A not learned
              M.frame(B, A, 1515),
              M.frame(B, A, 64, 0x8100),       # ETH_TYPE (a VLAN tag is not parsed): A not learned
              M.frame(B, MCAST_SRC),           # multicast source with a known destination: dropped
              M.frame(A, C),                   # A still unknown: FLOOD
              M.frame(BCAST, C),               # broadcast always floods
              M.frame(B, C, 64, 0x05DC), M.frame(B, C, 64, 0x0806), M.frame(B, C, 64, 0x86DD)]
    v, p, t = s.forward(0, frames, 2)
    assert list(v) == [M.ETH_LEN, M.ETH_LEN, M.ETH_TYPE, M.SRC_MCAST, M.FLOOD, M.FLOOD] + [M.UNICAST] * 3
    assert list(t[:4]) == [0, 0, 0, 0] and list(p[6:]) == [2, 2, 2]
    assert A not in s.model.table and MCAST_SRC not in s.model.table
    s.close()


def case_capacity(make):
    s = make(vlans=V4, capacity=5)
    k1, k2 = M.mac(100), M.mac(101)
    s.forward(1, [M.frame(BCAST, k1), M.frame(BCAST, k2)], 10)  # 3 free entries
    n = [M.mac(200 + k) for k in range(6)]
    frames = [M.frame(k1, n[0]), M.frame(BCAST, k1), M.frame(n[0], n[1]), M.frame(n[3], n[0]), M.frame(k2, n[2]),
              M.frame(n[0], n[3]),   # the table is full from here: n3, n4, n5 are never admitted
              M.frame(n[1], n[4]), M.frame(BCAST, k2), M.frame(n[3], n[1]), M.frame(n[0], n[3]), M.frame(n[5], n[2]),
              M.frame(n[2], n[5]), M.frame(n[4], n[0]), M.frame(k1, n[4])]
    v, p, t = s.forward(0, frames, 20)
    assert list(v) == [M.UNICAST, M.FLOOD, M.UNICAST, M.FLOOD, M.UNICAST, M.TABLE_FULL, M.TABLE_FULL, M.FLOOD,
                       M.FLOOD, M.TABLE_FULL, M.FLOOD, M.TABLE_FULL, M.FLOOD, M.TABLE_FULL]
    assert s.model.table[k1] == [0, 20] and s.model.table[k2] == [0, 20]  # known MACs still refresh
    assert p[0] == 1 and p[4] == 1  # k1 / k2 were on port 1 until their own frames moved them
    # exactly full at entry: nothing new gets in, held MACs refresh and unicast
    v, _, _ = s.forward(2, [M.frame(k1, n[5]), M.frame(n[5], k1), M.frame(k1, k1)], 30)
    assert list(v) == [M.TABLE_FULL, M.FLOOD, M.UNICAST]
    s.close()
    one = make(vlans=[1, 1], capacity=1)
    v, _, _ = one.forward(0, [M.frame(B, A), M.frame(A, B), M.frame(A, A), M.frame(B, A)], 1)
    assert list(v) == [M.FLOOD, M.TABLE_FULL, M.UNICAST, M.FLOOD]
    one.close()


def case_expiry(make):
    s = make(vlans=V4, capacity=4)
    s.forward(0, [M.frame(BCAST, A)], 1000)
    s.forward(1, [M.frame(BCAST, B)], 1001)
    assert s.expire(1300) == 0 and s.expire(1301) == 1 and s.expire(1302) == 1  # 300 stays, 301 leaves
    s.forward(2, [M.frame(BCAST, C)], 0xFFFFFF00)
    assert s.expire(40) == 0      # (u32)(0xFFFFFF00 + 300) = 44: 40 > 44 is false
    assert s.expire(0xFFFFFF80) == 1  # 0xFFFFFF80 > 44: gone, although only 128 s old (the reference's wrap)
    # 1000 s old: still unicasts before the tick, floods after it
    s.forward(3, [M.frame(BCAST, D)], 5000)
    v, p, _ = s.forward(0, [M.frame(D, A)], 6000)
    assert (v[0], p[0]) == (M.UNICAST, 3)
    assert s.expire(6000) == 1
    v, _, _ = s.forward(0, [M.frame(D, A)], 6000)
    assert v[0] == M.FLOOD
    # freed capacity is reused: fill to 4, expire all but one, fill again
    s.forward(1, [M.frame(BCAST, M.mac(50 + k)) for k in range(4)], 7000)
    assert len(s.model.table) == 4
    s.forward(0, [M.frame(BCAST, A)], 7200)
    assert s.expire(7400) == 3
    v, _, _ = s.forward(1, [M.frame(BCAST, M.mac(60 + k)) for k in range(4)], 7401)
    assert list(v) == [M.FLOOD] * 3 + [M.TABLE_FULL]
    s.close()


def case_length_edges(make):
    s = make(vlans=V4, capacity=16)
    lens = [41, 42, 59, 60, 61, 1514, 1515]
    v, _, t = s.forward(0, [M.frame(BCAST, A, n) for n in lens], 1)
    assert list(v) == [M.ETH_LEN] + [M.FLOOD] * 5 + [M.ETH_LEN]
    assert list(t) == [0, 60, 60, 60, 61, 1514, 0]
    # headers (bytes 0..13) straddling a 64-byte line: frames starting 12, 8 and 4 bytes before one
    frames = [M.frame(A, M.mac(10 + k), 64) for k in range(8)]
    lead = [13, 1, 1, 0, 0, 3, 0, 0]
    starts = set((M.pack(frames, lead)[1] * 4 % 64).tolist())
    assert {52, 56, 60} <= starts
    v, p, _ = s.forward(1, frames, 2, lead_dw=lead)
    assert list(v) == [M.UNICAST] * 8 and list(p) == [0] * 8
    s.close()


def case_long_lengths(make):
    """Lengths past 1514 up to the u16's end are ETH_LEN like 1515: no bit of the length may reach
    another field of a record or of the kernels' per-frame state. Learning frames sit between them."""
    s = make(vlans=V4, capacity=16)
    s.forward(1, [M.frame(BCAST, B)], 1)
    lens = [2047, 2048, 4095, 4096, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x7FFF, 0x8000, 0xF000, 65535]
    frames = []
    for n in lens:
        frames += [M.frame(B, A, n), M.frame(B, C, 64), M.frame(B, MCAST_SRC, n), M.frame(B, A, n, 0x1234)]
    v, p, t = s.forward(0, frames, 2)
    assert list(v) == [M.ETH_LEN, M.UNICAST, M.ETH_LEN, M.ETH_LEN] * len(lens)
    assert list(p) == [0xFF, 1, 0xFF, 0xFF] * len(lens) and list(t) == [0, 64, 0, 0] * len(lens)
    assert A not in s.model.table
    s.close()


def every_verdict(make):
    s = make(vlans=[1, 1], capacity=1)
    v, _, _ = s.forward(0, [M.frame(B, A, 20), M.frame(B, A, 64, 0x1234), M.frame(B, MCAST_SRC), M.frame(B, A),
                            M.frame(A, B), M.frame(A, A)], 1)
    assert sorted(v) == list(range(6))
    s.close()


def random_frames(rng, pool, n, p_bad=0.08):
    """n frames between MACs of `pool` with a share of broadcasts and of each drop class."""
    src, dst = rng.integers(0, len(pool), n), rng.integers(0, len(pool), n)
    kind = rng.random(n)
    out = []
    for i in range(n):
        d, s_, ln, et = pool[dst[i]], pool[src[i]], int(rng.choice([42, 60, 64, 128, 1514])), 0x0800
        k = kind[i]
        if k < p_bad / 4:
            ln = int(rng.choice([0, 13, 41, 1515, 2000]))
        elif k < p_bad / 2:
            et = int(rng.choice([0x8100, 0x0000, 0x0801]))
        elif k < 3 * p_bad / 4:
            s_ = MCAST_SRC
        elif k < p_bad:
            d = BCAST
        out.append(M.frame(d, s_, ln, et))
    return out


def differential(make, calls, max_n, seed, pool_size=300, capacity=128, slots_log2=0, epoch=None):
    rng = np.random.default_rng(seed)
    vlans = [1, 1, 1, 2, 2, 2, 3, 3]
    s = make(vlans=vlans, capacity=capacity, max_batch=max_n, slots_log2=slots_log2, epoch=epoch)
    pool = [M.mac(1000 + k) for k in range(pool_size)]
    now = 0xFFFFFE00  # crosses the u32 wrap during the run
    for _ in range(calls):
        now = (now + int(rng.integers(0, 90))) & 0xFFFFFFFF
        n = int(rng.integers(0, max_n + 1)) if rng.random() < 0.7 else int(rng.integers(0, 40))
        # a window of the pool, so MACs fall idle, age out and come back
        lo = int(rng.integers(0, pool_size - 40))
        s.forward(int(rng.integers(0, len(vlans))), random_frames(rng, pool[lo:lo + int(rng.integers(20, 200))], n), now)
        if rng.random() < 0.3:
            s.expire(now)
    s.close()


# ---- past one grid and one scan pass (tests/scale_cases.py has the boundaries) --------------------
def numpy_frames(dst_ids, src_ids, lens=None, ethertypes=None, src_mcast=None, dst_bcast=None):
    """Frames between the MACs M.mac(id), built without a Python loop per byte: (frames as a list
    of bytes for the model, packed = (bytes, offsets_dw, lens) for the switch). Frames lie back to
    back at dword boundaries; a frame shorter than its header is cut like M.frame's."""
    n = len(dst_ids)
    lens = np.full(n, 64, np.uint16) if lens is None else np.asarray(lens, np.uint16)
    hdr = np.zeros((n, 14), np.uint8)
    for ids, base in ((np.asarray(dst_ids, np.uint32), 0), (np.asarray(src_ids, np.uint32), 6)):
        hdr[:, base], hdr[:, base + 1] = 0x02, 0x10
        for b in range(4):
            hdr[:, base + 2 + b] = (ids >> (8 * (3 - b))) & 0xFF
    if dst_bcast is not None:
        hdr[dst_bcast, 0:6] = 0xFF
    if src_mcast is not None:
        hdr[src_mcast, 6:12] = np.frombuffer(MCAST_SRC, np.uint8)
    et = np.full(n, 0x0800, np.uint16) if ethertypes is None else np.asarray(ethertypes, np.uint16)
    hdr[:, 12], hdr[:, 13] = et >> 8, et & 0xFF
    size = (lens.astype(np.int64) + 3) & ~3
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum(size)[:-1]
    data = np.zeros(int(size.sum()) + 16, np.uint8)
    col = np.arange(14)
    keep = col[None, :] < lens[:, None]
    data[(offs[:, None] + col[None, :])[keep]] = hdr[keep]
    frames = [data[o:o + ln].tobytes() for o, ln in zip(offs.tolist(), lens.tolist())]
    return frames, (data, (offs // 4).astype(np.uint32), lens)


def numpy_random_frames(rng, pool_size, n, p_bad=0.08):
    """random_frames, vectorised: the same drop classes in the same shares between MACs
    M.mac(0 .. pool_size - 1); lengths 42 / 60 / 64 / 128 and, one frame in 512, 1514."""
    src, dst = rng.integers(0, pool_size, n), rng.integers(0, pool_size, n)
    kind = rng.random(n)
    lens = rng.choice(np.array([42, 60, 64, 128], np.uint16), n)
    lens[rng.integers(0, 512, n) == 0] = 1514
    bad_len = kind < p_bad / 4
    lens[bad_len] = rng.choice(np.array([0, 13, 41, 1515, 2000], np.uint16), int(bad_len.sum()))
    et = np.full(n, 0x0800, np.uint16)
    bad_et = (kind >= p_bad / 4) & (kind < p_bad / 2)
    et[bad_et] = rng.choice(np.array([0x8100, 0x0000, 0x0801], np.uint16), int(bad_et.sum()))
    return numpy_frames(dst, src, lens, et, src_mcast=(kind >= p_bad / 2) & (kind < 3 * p_bad / 4),
                        dst_bcast=(kind >= 3 * p_bad / 4) & (kind < p_bad))


def scale_new_macs(make):
    """Every frame a broadcast from a new source, one scan pass plus 300 frames; the capacity ends
    admission inside tile 1,025, the first tile of the scan's second pass: its rank is the carry."""
    from tests import scale_cases as S

    n = S.past("sw_scan_pass", 300)
    tile, width = S.BOUNDARIES["sw_scan_pass"]["first_past"] - 1, 256
    cap = tile + 100
    assert tile % width == 0 and tile // width == 1024 and cap < n
    s = make(vlans=[1, 1], capacity=cap, max_batch=n)
    ids = np.arange(n, dtype=np.uint32)
    frames, packed = numpy_frames(ids, ids, dst_bcast=np.ones(n, bool))
    (v, _, _), = s.forward_many([(0, frames, 1, packed)])
    assert np.array_equal(v, np.r_[np.full(cap, M.FLOOD, np.uint8), np.full(n - cap, M.TABLE_FULL, np.uint8)])
    s.close()


def scale_differential(make):
    """Random sources and destinations over a pool larger than the capacity, past the resolve
    kernel's grid: irregular per-tile counts of new MACs through the scan's carry, room running out
    beyond tile 1,024, held MACs another port taught, and every counter over two trips."""
    from tests import scale_cases as S

    n, pool, cap = S.past("sw_resolve_trip", 257), 400_000, 250_000
    rng = np.random.default_rng(17)
    s = make(vlans=[1, 1, 2], capacity=cap, max_batch=n)
    f0, p0 = numpy_random_frames(rng, 3_000, 2_000)
    frames, packed = numpy_random_frames(rng, pool, n)
    s.forward_many([(1, f0, 40, p0)])
    held = len(s.model.table)
    (v, p, _), = s.forward_many([(0, frames, 77, packed)])
    full = np.flatnonzero(v == M.TABLE_FULL)
    pass_frames = S.BOUNDARIES["sw_scan_pass"]["first_past"] - 1
    assert held > 500 and len(s.model.table) == cap and full.size and full[0] > pass_frames
    assert (p[v == M.UNICAST] == 1).any() and (p[v == M.UNICAST] == 0).any()
    assert (np.bincount(v, minlength=6) > 0).all()  # every verdict, so every counter, occurred
    s.close()


def scale_rebuild(make):
    """A table of 2^20 slots: two calls at different times fill it, an expiry tick removes the first
    call's half through the rebuild kernel's second trip, and one call addressed to every MAC
    unicasts to the survivors and floods the rest."""
    from tests import scale_cases as S

    cap, half = 300_000, 150_000
    s = make(vlans=[1, 1, 1], capacity=cap, max_batch=cap)
    slots = int(s.sw.layout_stats()["slots"])
    assert slots == 1 << 20 and slots >= S.BOUNDARIES["sw_rebuild_trip"]["first_past"]
    # an odd multiplier mod 2^32: distinct ids spread over the hash's input
    ids = (np.arange(cap, dtype=np.uint64) * 2654435761 & 0xFFFFFFFF).astype(np.uint32)
    for k, now in ((0, 1000), (1, 1200)):
        part = ids[k * half:(k + 1) * half]
        frames, packed = numpy_frames(part, part, dst_bcast=np.ones(half, bool))
        s.forward_many([(k, frames, now, packed)])
    assert len(s.model.table) == cap
    assert s.expire(1400) == half
    frames, packed = numpy_frames(ids, np.full(cap, ids[-1], np.uint32))
    (v, p, _), = s.forward_many([(2, frames, 1401, packed)])
    assert np.all(v[:half] == M.FLOOD) and np.all(v[half:] == M.UNICAST)
    assert np.all(p[half:-1] == 1) and p[-1] == 2  # the last MAC is the sender: it moved to port 2
    s.close()


SCALE_CASES = {"new_macs": scale_new_macs, "differential": scale_differential, "rebuild": scale_rebuild}

CASES = {"in_batch_order": case_in_batch_order, "no_learning_on_drops": case_no_learning_on_drops,
         "capacity": case_capacity, "expiry": case_expiry, "length_edges": case_length_edges, "long_lengths": case_long_lengths,
         "every_verdict": every_verdict}
