"""GPU: the device mode of the L2 switch (halo_amd/csrc/switch_fwd.hip through
halo_amd.switch.Switch) against the sequential dict model (tests/switch_model.py). After every call
the verdicts, out_port, tx_len, the counters and the listed table must equal the model's
(tests/switch_cases.Pair). The shapes are the smallest at which each path can go wrong: the batch
sizes around a wavefront and a 256-frame tile of the admission scan, a batch of several tiles that
is no multiple of one, forced probe collisions, and one large call."""
from __future__ import annotations

import numpy as np
import pytest

from tests import switch_cases as K
from tests import switch_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    dev = torch.device("cuda:0")
    return lambda **kw: K.Pair(device=dev, **kw)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_edge_case(make, name):
    K.CASES[name](make)


# 1000 = three full 256-frame tiles of the admission scan and a fourth of 232
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_sizes(make, n):
    rng = np.random.default_rng(100 + n)
    s = make(vlans=[1, 1, 2, 2], capacity=n // 3 + 2, max_batch=max(n, 1))
    pool = [M.mac(k) for k in range(n // 2 + 3)]
    s.forward(1, K.random_frames(rng, pool[:len(pool) // 3 + 1], n // 4), 10)  # a T0 to meet
    s.forward(0, K.random_frames(rng, pool, n), 20)
    s.forward(2, K.random_frames(rng, pool, n), 30)
    s.close()


def test_new_macs_in_every_tile(make):
    """Every frame brings a new MAC and room ends inside the third tile: the admission rank of a
    frame is its tile's prefix plus its rank inside the tile."""
    n, cap = 1000, 700
    s = make(vlans=[1, 1], capacity=cap, max_batch=n)
    v, _, _ = s.forward(0, [M.frame(K.BCAST, M.mac(k)) for k in range(n)], 1)
    assert list(v) == [M.FLOOD] * cap + [M.TABLE_FULL] * (n - cap)
    s.close()


def test_collisions(make):
    """16 slots, 15 entries: chains collide and wrap, and every lookup and insert still lands."""
    s = make(vlans=[1, 1, 1], capacity=15, slots_log2=4, max_batch=64)
    macs = [M.mac(7000 + k) for k in range(20)]
    s.forward(1, [M.frame(K.BCAST, m) for m in macs], 50)
    st = s.sw.layout_stats()
    assert int(st["slots"]) == 16 and int(st["entries"]) == 15
    assert int(st["longest_chain"]) > 1 and int(st["wrapped"]) >= 1, st
    v, p, _ = s.forward(0, [M.frame(m, macs[0]) for m in macs], 60)
    assert list(v) == [M.UNICAST] * 15 + [M.FLOOD] * 5 and list(p[1:15]) == [1] * 14
    # survivors behind removed entries of their probe chains are still found after the tick
    s.forward(2, [M.frame(K.BCAST, m) for m in macs[1:15:2]], 300)
    assert s.expire(360) == 7
    v, p, _ = s.forward(0, [M.frame(m, macs[0]) for m in macs[:15]], 361)
    assert list(v) == [M.UNICAST] + [M.UNICAST if k % 2 else M.FLOOD for k in range(1, 15)]
    assert int(s.sw.layout_stats()["entries"]) == 8
    s.forward(1, [M.frame(K.BCAST, m) for m in macs[10:]], 362)  # freed slots are reused
    s.close()


def test_long_differential(make):
    # the scratch set's call number starts six calls before its 16-bit wrap
    K.differential(make, calls=50, max_n=2048, seed=5, epoch=65530)


def test_differential_forced_collisions(make):
    K.differential(make, calls=12, max_n=300, seed=6, pool_size=120, capacity=100, slots_log2=7)


def test_back_to_back_calls_on_one_stream(make):
    """Eight calls queued on one stream with nothing between them (Pair.forward_many uploads first
    and reads last), across the scratch set's epoch wrap: each call starts from the entry count,
    the table and the scratch set the one before it left, and room runs out on the way."""
    rng = np.random.default_rng(9)
    s = make(vlans=[1, 1, 1], capacity=120, max_batch=4096, epoch=65531)
    pool = [M.mac(k) for k in range(260)]
    sizes = [4000, 300, 4096, 1, 2500, 0, 4096, 700]
    s.forward_many([(k % 3, K.random_frames(rng, pool[20 * k:20 * k + 100], n), 10 + k) for k, n in enumerate(sizes)])
    assert len(s.model.table) == 120
    s.close()


def test_large_scale(make):
    """One call of 2^18 frames over 100,000 MACs with capacity 65,536."""
    n, n_macs, cap = 1 << 18, 100_000, 65_536
    rng = np.random.default_rng(3)
    s = make(vlans=[1, 1, 2], capacity=cap, max_batch=n)
    ids = rng.integers(0, n_macs, (n, 2)).astype(np.uint32)
    arr = np.zeros((n, 64), np.uint8)
    for col, base in ((1, 0), (0, 6)):  # dst from ids[:, 1], src from ids[:, 0]
        arr[:, base] = 0x02
        for b in range(4):
            arr[:, base + 2 + b] = (ids[:, col] >> (8 * (3 - b))) & 0xFF
    arr[:, 12] = 0x08
    frames = [r.tobytes() for r in arr]
    packed = (np.concatenate([arr.ravel(), np.zeros(16, np.uint8)]), np.arange(n, dtype=np.uint32) * 16,
              np.full(n, 64, np.uint16))
    (v, _, _), = s.forward_many([(0, frames, 77, packed)])
    assert len(s.model.table) == cap and (v == M.TABLE_FULL).any() and (v == M.UNICAST).any()
    s.close()


def test_device_arguments(make):
    from halo_amd._lib import HALO_E_RANGE, HaloError

    s = make(vlans=[1, 1], capacity=4, max_batch=8)
    with pytest.raises(HaloError) as e:
        s.sw.forward(0, *s._arrays(M.pack([M.frame(K.BCAST, K.A)] * 9)), 1)
    assert e.value.code == HALO_E_RANGE
    s.forward(0, [], 1)
    s.close()


def test_every_verdict_occurred(make):
    K.every_verdict(make)
    assert (K.Pair.total > 0).all(), K.Pair.total
