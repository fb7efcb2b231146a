"""CPU: the host mode of the L2 switch (halo_amd/csrc/switch_table.cc through halo_amd.switch.Switch,
device=None) against the sequential dict model (tests/switch_model.py): the edge cases of
tests/switch_cases.py, a random differential run, argument validation and flood masks."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import switch_cases as K
from tests import switch_model as M


def make(**kw):
    return K.Pair(device=None, **kw)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_edge_case(name):
    K.CASES[name](make)


@pytest.mark.parametrize("name", sorted(K.SCALE_CASES))
def test_scale_case(name):
    """The expectations of tests/test_gpu_scale.py's switch cases, proven in host mode first."""
    K.SCALE_CASES[name](make)


def test_random_differential():
    K.differential(make, calls=60, max_n=300, seed=11)
    K.differential(make, calls=30, max_n=200, seed=12, pool_size=60, capacity=7)


def test_flood_masks_across_vlans():
    from halo_amd.switch import Switch

    vlans = [10, 20, 10, 30, 20, 10]
    s, m = Switch(vlans, 8), M.SwitchModel(vlans, 8)
    for p in range(len(vlans)):
        assert s.flood_mask(p) == m.flood_mask(p)
    assert s.flood_mask(0) == 0b100100 and s.flood_mask(1) == 0b010000
    assert s.flood_mask(3) == 0  # alone in its VLAN
    s64 = Switch([7] * 64, 8)
    assert s64.flood_mask(63) == (1 << 63) - 1 and s64.flood_mask(0) == (1 << 64) - 2


def test_argument_validation():
    from halo_amd import _lib
    from halo_amd._lib import HALO_E_INVAL, HALO_E_RANGE, HALO_OK, SwitchConfig, lib

    def create(n_ports=2, capacity=4, slots_log2=0, max_batch=8, device=-1):
        cfg, h = SwitchConfig(), ctypes.c_void_p()
        cfg.n_ports, cfg.capacity, cfg.slots_log2, cfg.max_batch, cfg.device = n_ports, capacity, slots_log2, max_batch, device
        return lib.halo_switch_create(ctypes.byref(cfg), ctypes.byref(h)), h

    assert lib.halo_switch_create(None, None) == HALO_E_INVAL
    for bad in (dict(n_ports=0), dict(n_ports=65), dict(capacity=0), dict(capacity=4, slots_log2=2),
                dict(capacity=5, slots_log2=2), dict(slots_log2=29), dict(max_batch=0), dict(max_batch=(1 << 24) + 1),
                dict(device=-2)):
        assert create(**bad)[0] == HALO_E_INVAL, bad
    rc, h = create(capacity=3, slots_log2=2)  # 4 slots > 3 entries
    assert rc == HALO_OK
    st = np.zeros(1, _lib.SW_LAYOUT_DTYPE)
    assert lib.halo_switch_layout_stats(h, _lib.ptr(st)) == HALO_OK and int(st["slots"][0]) == 4
    assert lib.halo_switch_destroy(h) == HALO_OK
    rc, h = create(capacity=5)
    assert rc == HALO_OK
    assert lib.halo_switch_layout_stats(h, _lib.ptr(st)) == HALO_OK and int(st["slots"][0]) == 16  # >= 2 * capacity
    data, offs, lens = M.pack([M.frame(K.BCAST, K.A)] * 9)
    res, cnt = np.zeros(9, _lib.SW_RESULT_DTYPE), np.zeros(6, np.uint32)
    args = (_lib.ptr(data), _lib.ptr(offs), _lib.ptr(lens))
    assert lib.halo_switch_forward(h, 2, *args, 1, 0, _lib.ptr(res), None, None) == HALO_E_INVAL  # port >= n_ports
    assert lib.halo_switch_forward(h, 0, *args, 9, 0, _lib.ptr(res), None, None) == HALO_E_RANGE  # n > max_batch
    assert lib.halo_switch_forward(h, 0, None, None, None, 0, 0, None, None, None) == HALO_OK      # n == 0
    for k in range(4):
        a = [*args, 1, 0, _lib.ptr(res)]
        a[k if k < 3 else 5] = None
        assert lib.halo_switch_forward(h, 0, *a, None, None) == HALO_E_INVAL
    assert lib.halo_switch_forward(None, 0, *args, 1, 0, _lib.ptr(res), None, None) == HALO_E_INVAL
    assert lib.halo_switch_forward(h, 0, *args, 8, 0, _lib.ptr(res), _lib.ptr(cnt), None) == HALO_OK
    assert cnt[M.FLOOD] == 8 and cnt.sum() == 8
    assert lib.halo_switch_forward(h, 0, *args, 8, 0, _lib.ptr(res), None, None) == HALO_OK  # counts are optional
    m = ctypes.c_uint64()
    assert lib.halo_switch_flood_mask(h, 2, ctypes.byref(m)) == HALO_E_INVAL
    assert lib.halo_switch_flood_mask(h, 0, None) == HALO_E_INVAL
    n = ctypes.c_uint32()
    assert lib.halo_switch_list(h, None, 1, ctypes.byref(n)) == HALO_E_INVAL
    assert lib.halo_switch_list(h, None, 0, None) == HALO_E_INVAL
    assert lib.halo_switch_list(h, None, 0, ctypes.byref(n)) == HALO_OK and n.value == 1
    assert lib.halo_switch_expire(None, 0, None) == HALO_E_INVAL
    assert lib.halo_switch_expire(h, 0, None) == HALO_OK
    assert lib.halo_switch_layout_stats(h, None) == HALO_E_INVAL
    assert lib.halo_switch_destroy(h) == HALO_OK
    assert lib.halo_switch_destroy(None) == HALO_E_INVAL


def test_short_list_buffer():
    s = make(vlans=[1, 1], capacity=8)
    s.forward(0, [M.frame(K.BCAST, M.mac(k)) for k in range(5)], 3)
    assert len(s.sw.ListSwitchMacAddr(cap=2)) == 2 and len(s.sw.ListSwitchMacAddr(cap=0)) == 0
    assert M.listed(s.sw.ListSwitchMacAddr(cap=2)) <= s.model.entries()
    s.close()


def test_every_verdict_occurred():
    K.every_verdict(make)
    assert (K.Pair.total > 0).all(), K.Pair.total
