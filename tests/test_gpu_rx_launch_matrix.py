"""GPU: every rx kernel instance through its entry point — the six (layout, fuse) pairs the library
instantiates times every kernel variant, with and without a status histogram — on a batch one frame
past a window of every kernel: records, histogram, flow hashes and route ids against the C oracle.
What the kernels compute is pinned elsewhere, at size; this pins that each call reaches the right
instance with the right grid and LDS bytes, so a batch of a few hundred frames is enough.

The batch: the golden frames followed by plain 64-byte UDP frames up to one frame past a multiple of
the mix kernel's 256-frame window (the 309 golden frames make that 513: two mix windows, eight
64-frame wave windows, and one frame). The strided uniform layout has its own batch: 257 golden
frames padded to one length."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests.helpers import assert_records_equal, golden_arrays, strip_ethernet

pytestmark = pytest.mark.gpu
L3 = 0x10
N_UNIFORM, UNIFORM_LEN = 257, 1514
ROUTES = [[0, 0, 1, 0], [0xC0A86400, 0xFFFFFF00, 0, 1], [0xC0A86464, 0xFFFFFFFF, 0, 2], [0x0A000000, 0xFF000000, 5, 3],
          [0x0A000000, 0xFF000000, 6, 3]]
FLOW = (1, 0, 1000003)  # flow kind, NAT type, buckets
# lanes per frame as _lib.variant_flags takes them: lane, 4, 8, 16, mix, stream, automatic (with
# hint 0: the mixed-block stream instance on the dense layouts)
VARIANTS = [1, 4, 8, 16, -1, -2, 0]
PAIRS = ["ragged", "ragged_l3", "strided_lens", "strided_uniform", "flow", "route"]


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a device"
    from halo_amd import _lib

    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    return torch.device("cuda:0")


def _want(oracle_lib, **kw):
    """{csum flag: (records, histogram)} from the C oracle."""
    extra = kw.pop("extra", 0)
    return {f: oracle_lib.rx_batch(netif=oracle_lib.NetIf.make(), flags=f | extra, **kw) for f in (0, 1)}


@pytest.fixture(scope="module")
def batches(dev, golden, oracle_lib):
    """Per (layout, fuse) pair: the device arrays of its batch and the oracle's answers."""
    import torch

    from halo_amd.route import RouteTable

    meta, blob = golden
    data, offs, lens, _ = golden_arrays(meta, blob)
    n = (len(lens) + 255) // 256 * 256 + 1
    ni = oracle_lib.NetIf.make()
    plain = []
    for i in range(n - len(lens)):
        length, kind = oracle_lib.synth_kind(0x4C4D, i, 0, 64, 0, 0)
        assert length == 64
        plain.append(np.frombuffer(oracle_lib.synth_frame(0x4C4D, i, 64, kind, ni), np.uint8))
    start = (len(data) + 3) & ~3
    data = np.concatenate([data, np.zeros(start - len(data), np.uint8), *plain, np.zeros(16, np.uint8)])
    offs = np.concatenate([offs, (start // 4 + 16 * np.arange(len(plain))).astype(np.uint32)])
    lens = np.concatenate([lens, np.full(len(plain), 64, np.uint16)])

    def to_dev(a, view=None):
        return torch.from_numpy(np.ascontiguousarray(a if view is None else a.view(view))).to(dev)

    b = {}
    ragged = dict(d=to_dev(data), o=to_dev(offs, np.int32), ln=to_dev(lens, np.int16), n=n,
                  want=_want(oracle_lib, data=data, lens=lens, offsets_dw=offs))
    b["ragged"] = b["flow"] = b["route"] = ragged
    assert (ragged["want"][1][0]["status"][-len(plain):] == 0).all() and len(plain) >= 64  # a whole plain window

    pk, poffs, plens = strip_ethernet(data, offs, lens)  # the L3 slices, as test_gpu_loopback.py makes them
    b["ragged_l3"] = dict(d=to_dev(pk), o=to_dev(poffs, np.int32), ln=to_dev(plens, np.int16), n=n,
                          want=_want(oracle_lib, data=pk, lens=plens, offsets_dw=poffs, extra=L3))

    stride = (int(lens.max()) + 3) & ~3
    sl = np.zeros((n, stride), np.uint8)
    for i in range(n):
        sl[i, :lens[i]] = data[4 * int(offs[i]):4 * int(offs[i]) + int(lens[i])]
    b["strided_lens"] = dict(d=to_dev(sl.reshape(-1)), ln=to_dev(lens, np.int16), n=n, stride=stride,
                             want=_want(oracle_lib, data=sl.reshape(-1), lens=lens, stride=stride))

    ustride = (UNIFORM_LEN + 3) & ~3
    fit = np.nonzero(lens <= UNIFORM_LEN)[0][:N_UNIFORM]
    assert len(fit) == N_UNIFORM
    su = sl[fit, :ustride].reshape(-1).copy()
    b["strided_uniform"] = dict(d=to_dev(su), n=N_UNIFORM, stride=ustride, length=UNIFORM_LEN,
                                want=_want(oracle_lib, data=su, lens=None, stride=ustride, length=UNIFORM_LEN))

    g, o = RouteTable(0), oracle_lib.RouteTable()
    for r in ROUTES:
        assert g.AddRoute(RouteTable.entry(*r)) == o.add(r)
    g.sync()
    b["route_table"] = g
    b["want_route"] = {f: o.find_batch(ragged["want"][f][0]["dst_ip"]) for f in (0, 1)}
    b["want_flow"] = {f: oracle_lib.flow_hash_batch(ragged["want"][f][0], *FLOW) for f in (0, 1)}
    return b


def _launch(pair, b, flags, out, hist, hashes, aux):
    """One call of the pair's entry point on the current stream (aux: the flow buckets or the route ids)."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf

    L, ni, s = _lib.lib, NetIf.make(), torch.cuda.current_stream().cuda_stream
    x, h = b[pair], _lib.ptr(hist)
    if pair == "ragged" or pair == "ragged_l3":
        fl = flags | (L3 if pair == "ragged_l3" else 0)
        return L.halo_rx_parse_batch_device(x["d"].data_ptr(), x["o"].data_ptr(), x["ln"].data_ptr(), x["n"], fl, ni, 0,
                                            out.data_ptr(), h, s)
    if pair == "strided_lens":
        return L.halo_rx_parse_strided_device(x["d"].data_ptr(), x["stride"], x["ln"].data_ptr(), 0, x["n"], flags, ni,
                                              out.data_ptr(), h, s)
    if pair == "strided_uniform":
        return L.halo_rx_parse_strided_device(x["d"].data_ptr(), x["stride"], None, x["length"], x["n"], flags, ni,
                                              out.data_ptr(), h, s)
    if pair == "flow":
        return L.halo_rx_parse_flow_batch_device(x["d"].data_ptr(), x["o"].data_ptr(), x["ln"].data_ptr(), x["n"], flags,
                                                 ni, 0, out.data_ptr(), h, FLOW[0], FLOW[1], hashes.data_ptr(), FLOW[2],
                                                 aux.data_ptr(), s)
    return L.halo_rx_parse_route_batch_device(x["d"].data_ptr(), x["o"].data_ptr(), x["ln"].data_ptr(), x["n"], flags, ni,
                                              0, out.data_ptr(), h, b["route_table"]._t, aux.data_ptr(), s)


@pytest.mark.parametrize("with_hist", [False, True], ids=["nohist", "hist"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("pair", PAIRS)
def test_every_instance_reached(dev, batches, pair, variant, with_hist):
    import torch

    from halo_amd import _lib, protocol

    n = batches[pair]["n"]
    for csum in (1, 0):  # the stream kernel has an instance for each
        want, want_hist = batches[pair]["want"][csum]
        out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device=dev)
        hist = torch.zeros(14, dtype=torch.int32, device=dev) if with_hist else None
        hashes = torch.zeros(n, dtype=torch.int64, device=dev)
        aux = torch.full((n,), -2, dtype=torch.int32, device=dev)
        assert _launch(pair, batches, csum | _lib.variant_flags(variant), out, hist, hashes, aux) == 0
        torch.cuda.synchronize()
        assert_records_equal(protocol.records(out), want[:n], None, f"{pair} variant {variant} csum {csum}")
        if with_hist:
            assert np.array_equal(hist.cpu().numpy().view(np.uint32), want_hist)
        if pair == "flow":
            wh, wb = batches["want_flow"][csum]
            assert np.array_equal(hashes.cpu().numpy().view(np.uint64), wh)
            assert np.array_equal(aux.cpu().numpy().view(np.uint32), wb)
        if pair == "route":
            assert np.array_equal(aux.cpu().numpy().view(np.uint32), batches["want_route"][csum])


@pytest.mark.parametrize("with_hist", [False, True], ids=["nohist", "hist"])
@pytest.mark.parametrize("variant", [1, 4], ids=["lane_one_launch", "g4_per_batch"])
def test_multi_batch_matches_separate_launches(dev, batches, variant, with_hist):
    """halo_rx_parse_batches_device on batches of 65, 0 and 129 frames: the lane kernel takes them as
    one grid, 4 lanes per frame is the per-batch fallback; both as three separate launches."""
    import torch

    from halo_amd import _lib
    from halo_amd._lib import NetIf

    x = batches["ragged"]
    cuts = [(0, 65), (65, 65), (65, 194)]
    flags = 1 | _lib.variant_flags(variant)
    s = torch.cuda.current_stream().cuda_stream

    def run(multi):
        outs = [torch.full((max(hi - lo, 1), 32), 0xEE, dtype=torch.uint8, device=dev) for lo, hi in cuts]
        hist = torch.zeros(14, dtype=torch.int32, device=dev) if with_hist else None
        if multi:
            descs = (_lib.BatchDesc * 3)()
            for j, (lo, hi) in enumerate(cuts):
                descs[j] = _lib.BatchDesc(x["d"].data_ptr(), _lib.ptr(x["o"][lo:]), _lib.ptr(x["ln"][lo:]),
                                          outs[j].data_ptr(), hi - lo, 0)
            assert _lib.lib.halo_rx_parse_batches_device(ctypes.cast(descs, ctypes.c_void_p), 3, flags, NetIf.make(), 0,
                                                         _lib.ptr(hist), s) == 0
        else:
            for (lo, hi), o in zip(cuts, outs):
                assert _lib.lib.halo_rx_parse_batch_device(x["d"].data_ptr(), _lib.ptr(x["o"][lo:]), _lib.ptr(x["ln"][lo:]),
                                                           hi - lo, flags, NetIf.make(), 0, o.data_ptr(), _lib.ptr(hist),
                                                           s) == 0
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs], None if hist is None else hist.cpu().numpy()

    got, got_hist = run(True)
    ref, ref_hist = run(False)
    want = x["want"][1][0]
    for (lo, hi), g, r in zip(cuts, got, ref):
        assert np.array_equal(g, r)
        if hi > lo:
            assert_records_equal(g.reshape(-1).view(want.dtype), want[lo:hi], None, f"batch [{lo}, {hi})")
    if with_hist:
        assert np.array_equal(got_hist, ref_hist) and got_hist.sum() == 194
