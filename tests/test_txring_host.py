"""CPU: the tx ring producer's entry points (halo_amd/csrc/tx_ring_host.cc) answer every argument
error before a device is looked for — so the answers are the same with and without a GPU — the
workspace size behaves, attach refuses every malformed ring header and flag, halo_tx_ring_result_t
has the layout of TXRING_RESULT_DTYPE, and the copy grid's edge in tests/txring_cases.py follows the
source."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import txring_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL = -1


@pytest.fixture(scope="module")
def L():
    from halo_amd import _lib

    return _lib.lib


def _ring(data_size=4096, at=0):
    """A created ring at byte `at` of a page-aligned host array."""
    from halo_amd import _lib

    mem = _lib.host_array(at + _lib.RING_HEADER + data_size)
    assert _lib.lib.halo_ring_create(mem.ctypes.data + at, _lib.RING_HEADER + data_size) == 0
    return mem


def _attach(L, mem, at=0, offset=0, flags=0, device=0):
    h = ctypes.c_void_p()
    rc = L.halo_tx_ring_attach(device, mem.ctypes.data + at, offset, flags, ctypes.byref(h))
    if rc == 0:  # only reachable with a device: the refusals below never get here
        assert L.halo_tx_ring_detach(h) == 0
    else:
        assert not h.value
    return rc


def test_write_refuses_bad_arguments_before_any_device(L):
    """A handle that is never dereferenced on an error path: 64 zero bytes."""
    fake = np.zeros(64, np.uint8)
    h = fake.ctypes.data
    span = np.zeros(256 + 16, np.uint8)
    sp = span.ctypes.data + (-span.ctypes.data) % 16
    need = int(L.halo_tx_ring_workspace(128))
    assert need > 0
    ws = np.zeros(need + 32, np.uint8)
    wp = ws.ctypes.data + (-ws.ctypes.data) % 16
    res = np.zeros(24 + 16, np.uint8)
    rp = res.ctypes.data + (-res.ctypes.data) % 8
    W = L.halo_tx_ring_write_span_device
    assert W(None, sp, 128, rp, wp, need, None) == INVAL              # null handle
    assert W(h, None, 128, rp, wp, need, None) == INVAL               # null span with bytes
    for k in (1, 2, 3):
        assert W(h, sp + k, 128, rp, wp, need, None) == INVAL         # misaligned span
        assert W(h, sp, 128 + k, rp, wp, need + 64, None) == INVAL    # span_bytes & 3
    assert W(h, sp, 128, rp, None, need, None) == INVAL               # null workspace
    for k in (4, 8, 12):
        assert W(h, sp, 128, rp, wp + k, need, None) == INVAL         # misaligned workspace
    assert W(h, sp, 128, rp, wp, need - 1, None) == INVAL             # workspace too small
    assert W(h, sp, 128, rp, wp, 0, None) == INVAL
    assert W(h, sp, 128, rp + 4, wp, need, None) == INVAL             # misaligned result
    assert W(h, sp, 1 << 34, rp, wp, 1 << 40, None) == INVAL          # beyond the record walk's span
    assert L.halo_tx_ring_detach(None) == INVAL
    assert L.halo_tx_ring_debug_copy_mode(None, 0) == INVAL
    assert L.halo_tx_ring_debug_copy_mode(h, 2) == INVAL
    assert not fake.any() and not ws.any() and not res.any()


def test_workspace_is_zero_when_too_large_and_never_decreases(L):
    assert L.halo_tx_ring_workspace(1 << 34) == 0
    assert L.halo_tx_ring_workspace((16 << 30) - (64 << 10) + 4) == 0
    assert L.halo_tx_ring_workspace((16 << 30) - (64 << 10)) > 0
    sizes = [0, 4, 8, 64, 16380, 16384, 16388, 65536, 1 << 20, (1 << 20) + 4, 71 << 20, 1 << 30]
    got = [int(L.halo_tx_ring_workspace(s)) for s in sizes]
    assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])), got
    # it holds the record walk's workspace and the walk's outputs for a record every 8 bytes
    for s, g in zip(sizes, got):
        assert g >= int(L.halo_rx_ring_scan_workspace(s, C.MAX_RECORD)) + 6 * (s // 8)


def test_attach_refuses_malformed_rings_and_flags(L):
    from halo_amd._lib import RING_PERSISTENT, RING_REGISTER

    assert L.halo_tx_ring_attach(0, None, 0, 0, ctypes.byref(ctypes.c_void_p())) == INVAL
    good = _ring()
    assert L.halo_tx_ring_attach(0, good.ctypes.data, 0, 0, None) == INVAL
    m = _ring()
    m[8] = 2                                                    # layout version
    assert _attach(L, m) == INVAL
    m = _ring()
    m[72:80].view(np.uint64)[0] = 4096 - 8                      # not a power of two
    m[80:88].view(np.uint64)[0] = 4096 - 9
    assert _attach(L, m) == INVAL
    m = _ring()
    m[80:88].view(np.uint64)[0] = 4094                          # mask != size - 1
    assert _attach(L, m) == INVAL
    m = _ring()
    m[0:8].view(np.uint64)[0] = 4096 + 4                        # head - tail > size
    assert _attach(L, m) == INVAL
    m = _ring()
    m[64:72].view(np.uint64)[0] = 4                             # tail ahead of head
    assert _attach(L, m) == INVAL
    m = _ring()
    m[0:8].view(np.uint64)[0] = 6                               # a cursor off the 4-byte grid
    assert _attach(L, m) == INVAL
    assert _attach(L, good, offset=8) == INVAL                  # a wrong offset
    assert _attach(L, good, flags=RING_PERSISTENT) == INVAL
    assert _attach(L, good, flags=RING_REGISTER | RING_PERSISTENT) == INVAL
    assert _attach(L, good, flags=0x4) == INVAL
    assert _attach(L, good, flags=0x80000000 | RING_REGISTER) == INVAL
    # a registered ring starts on a page of its own, as for halo_rx_ring_attach
    off_page = _ring(at=64)
    assert _attach(L, off_page, at=64, flags=RING_REGISTER) == INVAL
    # a well-formed ring gets past the checks: a device is then looked for
    assert _attach(L, good, flags=RING_REGISTER) in (0, -2, -3)


def test_result_struct_layout_matches_dtype(tmp_path):
    from halo_amd._lib import TXRING_RESULT_DTYPE

    fields = list(TXRING_RESULT_DTYPE.names)
    src = tmp_path / "txr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "halo_rx.h"\nint main(void){\n'
                   + "".join(f'printf("%zu\\n", offsetof(halo_tx_ring_result_t, {f}));\n' for f in fields)
                   + 'printf("%zu\\n%u\\n%u\\n%u\\n%u\\n", sizeof(halo_tx_ring_result_t), HALO_TXRING_OK, '
                     'HALO_TXRING_SHORT, HALO_TXRING_BAD_SPAN, HALO_TXRING_MAX_RECORD);\nreturn 0;}\n')
    exe = tmp_path / "txr"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    from halo_amd import _lib

    assert vals == [TXRING_RESULT_DTYPE.fields[f][1] for f in fields] + [
        24, _lib.TXRING_OK, _lib.TXRING_SHORT, _lib.TXRING_BAD_SPAN, _lib.TXRING_MAX_RECORD]
    assert C.MAX_RECORD == _lib.TXRING_MAX_RECORD


def test_copy_grid_edge_follows_the_source():
    c = C.read_constants()
    assert C.derived(c) == {k: v["first_past"] for k, v in C.BOUNDARIES.items()}, (c, C.derived(c))
    for v in C.BOUNDARIES.values():
        assert set(v["constants"]) <= set(c)
    assert C.past("txring_copy_grid", 100) == C.block_bytes(c) * c["copy_blocks"] + 100


def test_span_builders_agree_with_the_host_producer(L):
    """span_of is what halo_ring_write_batch leaves in an empty ring (plus zero alignment bytes),
    and every malformed span is refused by the host call in a ring where only it is at fault."""
    from halo_amd import ring as R

    frames, span = C.mixed_span(3, 65)
    ring = R.RingBuffer(1 << 17)
    assert ring.write(frames) == len(frames) and ring.head == span.nbytes
    assert np.array_equal(ring.data[:span.nbytes], span)
    assert list(C.ends_of(frames))[-1] == span.nbytes
    twin = R.RingBuffer(1 << 17)
    assert twin.write_span(span) == (len(frames), span.nbytes)
    for kind in ("zero", "half_plus_4", "past_end"):
        rc = L.halo_ring_write_span(twin.mem.ctypes.data, C.bad_span(kind, twin.size).ctypes.data,
                                    C.bad_span(kind, twin.size).nbytes, None, None)
        assert rc == INVAL, kind
    big = C.bad_span("walk_capacity", twin.size)
    assert R.RingBuffer(1 << 17).write_span(big) == (5, big.nbytes)  # the host accepts it
