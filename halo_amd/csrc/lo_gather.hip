// lo_gather.hip — the device side of the loopback gather (include/halo_rx.h, "loopback") on gfx950: a
// stable multi-way partition of a decided, device-resident ragged batch into one L3 batch per out
// NetIf, the packets a NetIf's LoChan receives in the order its sender sends them.
// lo_gather_host.cc checks the arguments and holds the host loop; lo_gather.h holds the selection
// and layout arithmetic both share.
//
// The kernels are port_streams.h's count / scan / scatter, a NetIf for a port. This file holds what
// is the gather's own: the stage of either mode (the first word of the ARP result and the length,
// in tx mode the frame dword with bytes 16-19; a packet's size; its dwords; the three per-packet
// entries) and the entry behind lo::device_ops().
// The copy: a frame starts on a dword and the packet 14 bytes in, so destination dword j is
// funnelled out of source dwords 3 + j and 4 + j at a fixed shift of 2 bytes (v_alignbyte_b32).
// The upper one is loaded only when a packet byte lies in it; the last destination dword is masked
// to pkt_len, so the zeros up to the 4-byte boundary come with it.
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "lo_gather.h"
#include "port_streams.h"

namespace halo {
namespace {

static_assert(lo::kTile == kPortTile && HALO_ARP_MAX_NETIFS == kMaxStreamPorts, "port_streams.h's tile and port limit");

struct LoParams : PortStreamParams {  // sel: halo_arp_result_t, two u32 per frame; n_ports: the NetIfs
    uint32_t* pkt_off_dw;
    uint16_t* pkt_len;
};

template <bool kTx>
struct LoStage {
    using Params = LoParams;

    // Frame i's NetIf as a one-bit mask (0: not selected, or not sendable) and its packet length;
    // *skip: selected but not sendable. Nothing of an unselected frame is loaded but its result word.
    static __device__ __forceinline__ uint64_t frame_ports(const Params& q, uint32_t i, uint32_t* plen, bool* skip) {
        *plen = 0;
        *skip = false;
        if (i >= q.n) return 0;
        const uint32_t p = lo::netif_of(static_cast<const uint32_t*>(q.sel)[2ull * i], q.n_ports);
        if (p >= q.n_ports) return 0;
        const uint32_t len = q.lens[i];
        bool ok;
        if (kTx) {
            ok = lo::tx_has_total_len(len);
            if (ok) {
                *plen = lo::tx_total_len(reinterpret_cast<const uint32_t*>(q.bytes)[(uint64_t)q.offsets_dw[i] + 4]);
                ok = lo::tx_sendable(*plen, len);
            }
        } else {
            ok = lo::fwd_sendable(len, q.flags);
            if (ok) *plen = len - lo::kEthHeader;
        }
        if (ok) return 1ull << p;
        *plen = 0;
        *skip = true;
        return 0;
    }

    static __device__ __forceinline__ uint32_t size(uint32_t plen) { return lo::packet_size(plen); }

    // Dword j of the packet of plen bytes in the frame at src (j < packet_size(plen) / 4): frame bytes
    // 14 + 4j .. 17 + 4j, the last dword masked to plen. The upper source dword holds frame bytes
    // 16 + 4j and up: it is loaded only when the packet reaches it, so no load goes past the word that
    // holds the packet's last byte.
    static __device__ __forceinline__ uint32_t word(const uint32_t* __restrict__ src, uint32_t plen, uint32_t j) {
        const uint32_t lo_w = src[3 + j];
        const uint32_t hi_w = plen > 4 * j + 2 ? src[4 + j] : 0u;
        uint32_t w = __builtin_amdgcn_alignbyte(hi_w, lo_w, 2);
        const uint32_t rest = plen - 4 * j;  // >= 1
        if (rest < 4) w &= (1u << 8 * rest) - 1u;
        return w;
    }

    static __device__ __forceinline__ void list(const Params& q, uint64_t slot, uint32_t i, uint32_t plen, bool fits,
                                                uint64_t byte_off) {
        q.pkt_off_dw[slot] = fits ? (uint32_t)(byte_off / 4) : lo::kNotWritten;
        q.pkt_len[slot] = (uint16_t)plen;
        q.index[slot] = i;
    }
};

int ops_run(const halo_lo_config_t* cfg, const uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* d_lens,
            uint32_t n, const halo_arp_result_t* d_results, uint8_t* d_out, halo_egress_port_t* d_ports,
            uint32_t* d_pkt_off_dw, uint16_t* d_pkt_len, uint32_t* d_index, uint32_t* d_skipped, void* d_workspace,
            halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0)
        return hipMemsetAsync(d_ports, 0, cfg->n_netifs * sizeof(halo_egress_port_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    LoParams q{};
    q.bytes = d_bytes, q.offsets_dw = d_offsets_dw, q.lens = d_lens, q.sel = d_results;
    fill_port_streams(q, n, cfg->n_netifs, cfg->flags, cfg->region_bytes, d_workspace);
    q.index_cap = cfg->index_cap;
    q.out = d_out, q.ports = d_ports, q.pkt_off_dw = d_pkt_off_dw, q.pkt_len = d_pkt_len, q.index = d_index;
    q.skipped = d_skipped;
    if (cfg->flags & HALO_LO_TX) launch_port_streams<LoStage<true>>(q, st);
    else launch_port_streams<LoStage<false>>(q, st);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const lo::DeviceOps kDeviceOps = {ops_run};

}  // namespace

namespace lo {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace lo
}  // namespace halo
