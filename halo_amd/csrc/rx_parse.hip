// rx_parse.hip — the hot path: batched Ethernet -> IPv4 -> UDP/TCP/ICMP parse and
// 16-bit one's-complement Internet checksum verification on gfx950 (MI355X).
//
// Restates, per frame and bit-exactly:
//   protocol.GetCheckSum        protocol/utils.go:11-31
//   protocol.ParseEthFrm        protocol/ethernet.go:29-55
//   protocol.ParseIpv4Pkt       protocol/ipv4.go:48-86
//   protocol.ParseUdpPkt        protocol/udp.go:21-49
//   protocol.ParseTcpPkt        protocol/tcp.go:36-70
//   protocol.ParseIcmpPkt       protocol/icmp.go:33-63
//   protocol.NatGetSrcDstPort   protocol/ipv4.go:229-246
//   NetIf.RxEthernet / RxIpv4 branch inputs  engine/ethernet_engine.go:22, ipv4_engine.go:24,31
//
// Execution shape (DESIGN.md "Kernels"): a group of G lanes of one 64-wide wavefront owns a
// frame; 64/G frames per wave. Lane j of the group loads dwords [4j, 4j+4) + k*4G of the frame
// with one 16-byte load per step, so a wave-instruction covers 64/G frames' consecutive bytes
// (coalesced). The 48-byte header (dwords 0..11) sits in group lanes 0..2 after the first load
// and is broadcast to the group (DPP quad_perm / row_newbcast for G = 4 / 16, v_readlane for
// G = 64, ds_bpermute otherwise); every lane then runs the header checks redundantly (no
// divergence, no second broadcast). Only the L4 segment sum needs a cross-lane reduction
// (DPP butterflies). G = 1 (small frames): each lane owns a whole frame, reads its header with
// its own three 16-byte loads and needs no cross-lane traffic at all. Mixed sizes packed in
// memory (IMIX) take the byte-stream kernel (rx_stream_kernel, rx_stream.hip): a lane per frame for the
// header, the whole wave for one coalesced pass over the window's bytes, and every L4 sum as a
// difference of a running prefix.
//
// The files:
//   rx_frame.h     the per-frame device code every kernel is built from, and the checksum arithmetic
//   rx_hist.h      the status histogram, device half: a block's counts into its queue's tree
//   rx_hist.hip    ... host half: the devices' tree sets (hist_trees), stream_device
//   rx_lane.hip    lane per frame: rx_lane_kernel, rx_lane_lean_kernel, rx_lane_multi_kernel,
//                  ring_service_kernel (launch_ring_service)
//   rx_group.hip   G lanes per frame, uniform batches: rx_group_kernel
//   rx_stream.hip  mixed sizes: rx_stream_kernel (dense bytes), rx_mix_kernel (size classes)
//   rx_launch.h    one launcher per family, taking (layout, fuse) at run time
//   rx_parse.hip   this file: the C entry points, their checks, and the choice of kernel
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "route_view.h"
#include "rx_launch.h"

namespace halo {
namespace {

constexpr int kVariantMix = -1, kVariantStream = 2, kVariantStreamMixed = 3;

// Kernel variant (from the sweeps in profiles/r01/tune_*.log and
// profiles/r02/stream/): a variant named in the call's flags wins; frames all <= 64 B go lane
// per frame; frames packed densely in memory (ragged layouts, or strided with little slack)
// up to 1 KB, or of mixed sizes, take the byte-stream kernel; longer uniform frames take 8 or 16
// lanes per frame; mixed sizes that are not dense take the size-class mix kernel.
int pick_variant(uint32_t max_len, bool uniform, bool dense, uint32_t flags) {
    switch ((flags & HALO_RX_VARIANT_MASK) >> HALO_RX_VARIANT_SHIFT) {
        case HALO_RX_VARIANT_LANE: return 1;
        case HALO_RX_VARIANT_G4: return 4;
        case HALO_RX_VARIANT_G8: return 8;
        case HALO_RX_VARIANT_G16: return 16;
        case HALO_RX_VARIANT_MIX: return kVariantMix;
        case HALO_RX_VARIANT_STREAM: return kVariantStream;
        default: break;
    }
    if (flags & HALO_RX_UNIFORM_LEN) uniform = max_len != 0;
    if (max_len != 0 && max_len <= 64) return 1;
    if (!uniform) return dense ? kVariantStreamMixed : kVariantMix;
    if (max_len <= 1024) return dense ? kVariantStream : max_len <= 128 ? 1 : 4;
    if (max_len <= 4096) return 8;
    return 16;
}

int launch_parse(const RxParams& p_in, int layout, uint32_t max_len, bool uniform, hipStream_t s) {
    // ragged batches are taken as packed back to back (the stream kernel checks each window and
    // sums a sparse one frame by frame); strided frames of one length are dense when the stride
    // wastes < 1/4; strided frames with their own lengths may be anything below the stride
    RxParams p = p_in;
    p.hist_out = p.hist;
    if (p.hist && !(p.hist = hist_trees(stream_device(s), s))) return HALO_E_NOMEM;  // counts go through a tree
    const bool dense = layout == 0 || layout == 3 || (layout == 2 && p.stride <= max_len + max_len / 4 + 64);
    const int v = pick_variant(max_len, uniform, dense, p.flags);
    const int fuse = layout != 0 ? 0 : p.flow_hash ? 1 : p.route_out ? 2 : 0;  // ragged: the only layout with the fused passes
    switch (v) {
        case 1: return launch_lane(p, layout, fuse, s);
        case kVariantStream: return launch_stream(p, layout, fuse, false, s);
        case kVariantStreamMixed: return launch_stream(p, layout, fuse, true, s);
        case 4: case 8: case 16: return launch_group(p, layout, fuse, v, s);
        default: return launch_mix(p, layout, fuse, s);
    }
}

int fill_common(RxParams& p, uint32_t n, uint32_t flags, const halo_rx_netif_t* netif,
                halo_rx_result_t* d_out, uint32_t* d_hist) {
    if (!netif || !d_out) return HALO_E_INVAL;
    if (flags & ~(HALO_RX_CSUM_ENABLE | HALO_RX_JUMBO_EXT | HALO_RX_RECORD_COMPACT | HALO_RX_UNIFORM_LEN |
                  HALO_RX_L3_START | HALO_RX_VARIANT_MASK))
        return HALO_E_INVAL;
    if (((flags & HALO_RX_VARIANT_MASK) >> HALO_RX_VARIANT_SHIFT) > HALO_RX_VARIANT_STREAM) return HALO_E_INVAL;
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return HALO_E_INVAL;
    p.n = n;
    p.flags = flags;
    p.mac_lo = (uint32_t)netif->mac[0] | ((uint32_t)netif->mac[1] << 8) | ((uint32_t)netif->mac[2] << 16) |
               ((uint32_t)netif->mac[3] << 24);
    p.mac_hi = (uint32_t)netif->mac[4] | ((uint32_t)netif->mac[5] << 8);
    p.own_ip = netif->ip;
    p.out = d_out;
    p.hist = d_hist;
    return HALO_OK;
}

}  // namespace
}  // namespace halo

extern "C" HALO_API int halo_rx_parse_batch_device(const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                                   const uint16_t* d_lens, uint32_t n, uint32_t flags,
                                                   const halo_rx_netif_t* netif, uint32_t max_len_hint,
                                                   halo_rx_result_t* d_out, uint32_t* d_status_hist,
                                                   halo_stream_t stream) {
    halo::RxParams p{};
    int rc = halo::fill_common(p, n, flags, netif, d_out, d_status_hist);
    if (rc) return rc;
    if (n == 0) return HALO_OK;
    if (!d_bytes || !d_offsets_dw || !d_lens) return HALO_E_INVAL;
    if ((rc = halo::check_device())) return rc;
    p.bytes = d_bytes;
    p.offsets_dw = d_offsets_dw;
    p.lens = d_lens;
    return halo::launch_parse(p, (flags & HALO_RX_L3_START) ? 3 : 0, max_len_hint, false,
                              static_cast<hipStream_t>(stream));
}

extern "C" HALO_API int halo_rx_parse_flow_batch_device(const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                                        const uint16_t* d_lens, uint32_t n, uint32_t flags,
                                                        const halo_rx_netif_t* netif, uint32_t max_len_hint,
                                                        halo_rx_result_t* d_out, uint32_t* d_status_hist,
                                                        uint32_t flow_kind, uint32_t nat_type, uint64_t* d_hash,
                                                        uint32_t bucket_count, uint32_t* d_bucket,
                                                        halo_stream_t stream) {
    if (flow_kind > HALO_FLOW_NAT_WAN || !d_hash || (reinterpret_cast<uintptr_t>(d_hash) & 7u)) return HALO_E_INVAL;
    if (d_bucket && bucket_count == 0) return HALO_E_INVAL;
    halo::RxParams p{};
    int rc = halo::fill_common(p, n, flags, netif, d_out, d_status_hist);
    if (rc) return rc;
    if (flags & HALO_RX_L3_START) return HALO_E_INVAL;  // LoChan packets: plain ragged parse only
    if (n == 0) return HALO_OK;
    if (!d_bytes || !d_offsets_dw || !d_lens) return HALO_E_INVAL;
    if ((rc = halo::check_device())) return rc;
    p.bytes = d_bytes;
    p.offsets_dw = d_offsets_dw;
    p.lens = d_lens;
    p.flow_hash = d_hash;
    p.flow_bucket = d_bucket;
    p.flow_buckets = bucket_count;
    p.flow_kind = flow_kind;
    p.flow_nat = nat_type;
    return halo::launch_parse(p, 0, max_len_hint, false, static_cast<hipStream_t>(stream));
}

extern "C" HALO_API int halo_rx_parse_route_batch_device(const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                                         const uint16_t* d_lens, uint32_t n, uint32_t flags,
                                                         const halo_rx_netif_t* netif, uint32_t max_len_hint,
                                                         halo_rx_result_t* d_out, uint32_t* d_status_hist,
                                                         const halo_route_table_t* table, uint32_t* d_route_ids,
                                                         halo_stream_t stream) {
    halo::RouteViewLock lk(table);  // until the fused kernel is enqueued
    halo::LpmView v{};
    if (halo::route_view(table, &v) || !d_route_ids) return HALO_E_INVAL;
    halo::RxParams p{};
    int rc = halo::fill_common(p, n, flags, netif, d_out, d_status_hist);
    if (rc) return rc;
    if (flags & HALO_RX_L3_START) return HALO_E_INVAL;  // LoChan packets: plain ragged parse only
    if (n == 0) return HALO_OK;
    if (!d_bytes || !d_offsets_dw || !d_lens) return HALO_E_INVAL;
    if ((rc = halo::check_device())) return rc;
    p.bytes = d_bytes;
    p.offsets_dw = d_offsets_dw;
    p.lens = d_lens;
    p.rt_tbl24 = v.tbl24;
    p.rt_tbl8 = v.tbl8;
    p.rt_lists = v.lists;
    p.rt_ids = v.ids;
    p.route_out = d_route_ids;
    return halo::launch_parse(p, 0, max_len_hint, false, static_cast<hipStream_t>(stream));
}

extern "C" HALO_API int halo_rx_parse_strided_device(const uint8_t* d_bytes, uint64_t stride,
                                                     const uint16_t* d_lens, uint32_t len, uint32_t n,
                                                     uint32_t flags, const halo_rx_netif_t* netif,
                                                     halo_rx_result_t* d_out, uint32_t* d_status_hist,
                                                     halo_stream_t stream) {
    halo::RxParams p{};
    int rc = halo::fill_common(p, n, flags, netif, d_out, d_status_hist);
    if (rc) return rc;
    if (flags & HALO_RX_L3_START) return HALO_E_INVAL;  // LoChan packets: plain ragged parse only
    if (n == 0) return HALO_OK;
    if (!d_bytes || (stride & 3u) || (n > 1 && stride == 0)) return HALO_E_INVAL;
    if (!d_lens && n > 1 && len > stride) return HALO_E_INVAL;
    if ((rc = halo::check_device())) return rc;
    p.bytes = d_bytes;
    p.lens = d_lens;
    p.stride = stride;
    p.len = len;
    // with per-frame lengths only the stride bounds them (mixed sizes possible)
    const uint32_t max_len = d_lens ? (uint32_t)(stride < 65535 ? stride : 65535) : len;
    return halo::launch_parse(p, d_lens ? 1 : 2, max_len, d_lens == nullptr, static_cast<hipStream_t>(stream));
}

extern "C" HALO_API int halo_rx_parse_batches_device(const halo_rx_batch_desc_t* batches, uint32_t k, uint32_t flags,
                                                     const halo_rx_netif_t* netif, uint32_t max_len_hint,
                                                     uint32_t* d_status_hist, halo_stream_t stream) {
    if (!batches || k == 0 || k > halo::kMultiMax) return HALO_E_INVAL;
    halo::MultiBatches mp{};
    uint64_t windows = 0;
    uint32_t live = 0;
    for (uint32_t j = 0; j < k; ++j) {
        const halo_rx_batch_desc_t& d = batches[j];
        if (d.n == 0) {
            mp.win_end[j] = (uint32_t)windows;
            continue;
        }
        int rc = halo::fill_common(mp.p, d.n, flags, netif, d.d_out, d_status_hist);
        if (rc) return rc;
        if (!d.d_bytes || !d.d_offsets_dw || !d.d_lens) return HALO_E_INVAL;
        windows += (d.n + 63u) / 64u;
        mp.win_end[j] = (uint32_t)windows;
        mp.n[j] = d.n;
        mp.bytes[j] = d.d_bytes;
        mp.offsets_dw[j] = d.d_offsets_dw;
        mp.lens[j] = d.d_lens;
        mp.out[j] = d.d_out;
        ++live;
    }
    if (!live) return netif ? HALO_OK : HALO_E_INVAL;
    int rc = halo::check_device();
    if (rc) return rc;
    const uint32_t v = (flags & HALO_RX_VARIANT_MASK) >> HALO_RX_VARIANT_SHIFT;
    const bool lane = v == HALO_RX_VARIANT_LANE || (v == HALO_RX_VARIANT_AUTO && max_len_hint && max_len_hint <= 64);
    if (!lane) {  // the larger-frame kernels are per batch: one launch each, in order, on `stream`
        for (uint32_t j = 0; j < k && rc == HALO_OK; ++j)
            if (batches[j].n)
                rc = halo_rx_parse_batch_device(batches[j].d_bytes, batches[j].d_offsets_dw, batches[j].d_lens,
                                                batches[j].n, flags, netif, max_len_hint, batches[j].d_out,
                                                d_status_hist, stream);
        return rc;
    }
    mp.k = k;
    mp.p.n = 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    mp.p.hist_out = d_status_hist;
    if (d_status_hist && !(mp.p.hist = halo::hist_trees(halo::stream_device(s), s))) return HALO_E_NOMEM;
    return halo::launch_lane_multi(mp, (flags & HALO_RX_L3_START) ? 3 : 0, windows, s);
}
