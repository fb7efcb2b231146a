// tx_respond.hip — the device side of the local responders (include/halo_rx.h, "local
// responders") on gfx950: from a parsed, device-resident batch to the dense list of reply
// descriptors in frame order, which halo_tx_build_batch_device consumes with the batch's own bytes
// as payload. A device-side halo_rx_dispatch comes with it (d_actions).
//
// Three launches, the shape of the ARP gather (arp_fwd.hip):
//   count    one lane per frame, one tile of kTile frames per workgroup: the decision of
//            tx_respond.h from the record (two 16-byte loads) and the verdict / op / result bytes,
//            the frame's action byte, per-tile reply count, per-kind totals (LDS, then one atomic
//            per kind and workgroup)
//   scan     one workgroup: exclusive scan over the tiles, kScanPass tiles per pass, four
//            consecutive tiles per lane; *d_count = the total
//   scatter  the decision again (plus lens and offsets_dw), rank = tile base + waves before (LDS)
//            + lanes below (ballot + mbcnt), and for rank < cap the 40-byte descriptor as five
//            8-byte stores, the 8-byte source word and the destination address
// No frame byte is read. Every load of a frame's inputs depends on its index alone, except the
// served-port word, which a LOCAL_TCP frame with SYN set reads after its record.
#include <hip/hip_runtime.h>

#include "arp_table.h"
#include "halo_common.h"
#include "tile_scan.h"
#include "tx_respond.h"

namespace halo {
namespace {

using respond::kNone;
using respond::kTile;
using respond::Rec;
using respond::Reply;

static_assert(kTile == arp::kGatherTile, "the responders' tile is the gather's");
static_assert(sizeof(halo_tx_build_desc_t) == 40 && sizeof(halo_respond_src_t) == 8 && sizeof(halo_tx_op_t) == 16 &&
                  sizeof(halo_rx_result_t) == 32,
              "layouts the kernels index by hand");

struct Args {
    const halo_rx_result_t* recs;
    const uint8_t* nat_verdict;   // optional
    const uint8_t* ops;           // optional, 16-byte halo_tx_op_t: byte 0 = steps
    const uint8_t* fixup_result;  // with ops
    const uint32_t* tcp_ports;    // optional
    uint32_t n, flags, own_ip, nat_enable;
};

// Frame i's reply: every load here depends on i alone and they are issued together.
__device__ __forceinline__ Reply reply_of(const Args& a, uint32_t i, uint32_t len, uint32_t off_dw) {
    const uint4* p = reinterpret_cast<const uint4*>(a.recs) + 2ull * i;
    const uint4 lo = p[0], hi = p[1];
    const uint32_t nat = a.nat_verdict ? a.nat_verdict[i] : kNone;
    const uint32_t fix = a.ops ? (uint32_t)a.ops[16ull * i] | (uint32_t)a.fixup_result[i] << 8 : 0u;
    return respond::decide(Rec{lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}, len, off_dw, nat, fix, a.tcp_ports, a.own_ip,
                           a.nat_enable != 0, a.flags);
}

__global__ void __launch_bounds__(kTile) respond_count_kernel(const Args a, uint32_t* __restrict__ tiles,
                                                              uint8_t* __restrict__ actions, uint32_t* kind_counts) {
    __shared__ uint32_t s_kind[HALO_RESPOND_KIND_COUNT];
    if (threadIdx.x < HALO_RESPOND_KIND_COUNT) s_kind[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t kind = kNone;
    if (i < a.n) {
        const Reply o = reply_of(a, i, 0u, 0u);  // length and offset shape the descriptor, not the decision
        kind = o.kind;
        if (actions) actions[i] = (uint8_t)o.action;
    }
    for (uint32_t k = 0; k < HALO_RESPOND_KIND_COUNT; ++k) {
        const uint32_t c = (uint32_t)__popcll(__ballot(kind == k));
        if (lane == k && c) atomicAdd(&s_kind[k], c);
    }
    __syncthreads();
    if (threadIdx.x == 0) tiles[blockIdx.x] = s_kind[0] + s_kind[1] + s_kind[2] + s_kind[3];
    if (kind_counts && threadIdx.x < HALO_RESPOND_KIND_COUNT && s_kind[threadIdx.x])
        atomicAdd(kind_counts + threadIdx.x, s_kind[threadIdx.x]);
}
static_assert(HALO_RESPOND_KIND_COUNT == 4, "the tile total above names each kind");

// One workgroup: tiles[t] becomes the number of replies in the tiles before t; *count = all.
__global__ void __launch_bounds__(256) respond_scan_kernel(uint32_t* tiles, uint32_t n_tiles, uint32_t* count) {
    const uint32_t total = scan_tiles(tiles, n_tiles);
    if (threadIdx.x == 0) *count = total;
}

__global__ void __launch_bounds__(kTile) respond_scatter_kernel(const Args a, const uint32_t* __restrict__ offsets_dw,
                                                                const uint16_t* __restrict__ lens,
                                                                const uint32_t* __restrict__ tiles,
                                                                halo_tx_build_desc_t* __restrict__ desc,
                                                                halo_respond_src_t* __restrict__ src,
                                                                uint32_t* __restrict__ dst_ip, uint32_t cap) {
    const uint32_t i = blockIdx.x * kTile + threadIdx.x;
    Reply o;
    o.kind = kNone;
    if (i < a.n) o = reply_of(a, i, lens[i], offsets_dw[i]);
    const bool sel = o.kind != kNone;
    const uint64_t votes = tile_votes<kTile>(sel);
    if (!sel) return;
    const uint32_t rank = tile_rank<kTile>(votes, tiles[blockIdx.x]);
    if (rank >= cap) return;
    uint2* d = reinterpret_cast<uint2*>(desc + rank);
    d[0] = make_uint2((uint32_t)o.payload_off, (uint32_t)(o.payload_off >> 32));
    d[1] = make_uint2(o.w2, o.w3);
    d[2] = make_uint2(o.src_ip, o.dst_ip);
    d[3] = make_uint2(o.seq, o.ack);
    d[4] = make_uint2(0u, 0u);  // dst_mac (TxIpv4's, filled by the encap), mode ETH, pad
    *reinterpret_cast<uint2*>(src + rank) = make_uint2(i, o.kind);
    if (dst_ip) dst_ip[rank] = o.dst_ip;
}

int ops_run(const uint32_t* d_offsets_dw, const uint16_t* d_lens, const halo_rx_result_t* d_records, uint32_t n,
            uint32_t flags, const halo_rx_netif_t* netif, const uint8_t* d_nat_verdict, const halo_tx_op_t* d_ops,
            const uint8_t* d_fixup_result, const uint32_t* d_tcp_ports, halo_tx_build_desc_t* d_desc,
            halo_respond_src_t* d_src, uint32_t* d_dst_ip, uint32_t cap, uint32_t* d_count, uint32_t* d_kind_counts,
            uint8_t* d_actions, void* d_workspace, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return hipMemsetAsync(d_count, 0, sizeof(uint32_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    const Args a{d_records, d_nat_verdict, reinterpret_cast<const uint8_t*>(d_ops), d_fixup_result, d_tcp_ports,
                 n,         flags,         netif->ip,                               netif->nat_enable ? 1u : 0u};
    uint32_t* tiles = static_cast<uint32_t*>(d_workspace);
    const uint32_t n_tiles = (uint32_t)tiles_of(n, kTile);
    hipLaunchKernelGGL(respond_count_kernel, dim3(n_tiles), dim3(kTile), 0, st, a, tiles, d_actions, d_kind_counts);
    hipLaunchKernelGGL(respond_scan_kernel, dim3(1), dim3(256), 0, st, tiles, n_tiles, d_count);
    hipLaunchKernelGGL(respond_scatter_kernel, dim3(n_tiles), dim3(kTile), 0, st, a, d_offsets_dw, d_lens, tiles, d_desc,
                       d_src, d_dst_ip, cap);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const respond::DeviceOps kDeviceOps = {ops_run};

}  // namespace

namespace respond {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace respond
}  // namespace halo
