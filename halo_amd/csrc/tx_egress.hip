// tx_egress.hip — the device side of the egress step (include/halo_rx.h, "egress") on gfx950: a
// stable multi-way partition of a device-resident ragged batch into one stream of ring records per
// egress port. tx_egress_host.cc checks the arguments and holds the host loop; tx_egress.h holds the
// layout arithmetic both share.
//
// The kernels are port_streams.h's count / scan / scatter. This file holds what is the egress
// step's own: the stage (how each kind's selector becomes a port mask, a ring record's size, its
// dwords, the index entry), one front end per selector kind, and the entry behind
// egress::device_ops(). A record's source and destination are 4-byte aligned by construction.
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "port_streams.h"
#include "tx_egress.h"

namespace halo {
namespace {

static_assert(egress::kTile == kPortTile && HALO_EGRESS_MAX_PORTS == kMaxStreamPorts, "port_streams.h's tile and port limit");

template <uint32_t KIND>
struct EgressStage {
    using Params = PortStreamParams;

    static __device__ __forceinline__ uint64_t frame_mask(const Params& q, uint32_t i) {
        if (KIND == HALO_EGRESS_KIND_MASKS) return egress::mask_of_masks(static_cast<const uint64_t*>(q.sel)[i]);
        if (KIND == HALO_EGRESS_KIND_ARP) return egress::mask_of_arp(static_cast<const uint32_t*>(q.sel)[2ull * i]);
        return egress::mask_of_switch(static_cast<const uint32_t*>(q.sel)[i], q.flood);
    }

    // Frame i's ports (0: none, or not sendable) and length; *skip: selected but not sendable.
    static __device__ __forceinline__ uint64_t frame_ports(const Params& q, uint32_t i, uint32_t* len, bool* skip) {
        *len = 0;
        *skip = false;
        if (i >= q.n) return 0;
        const uint64_t m = frame_mask(q, i) & q.valid;
        if (!m) return 0;
        *len = q.lens[i];
        if (egress::sendable(*len, q.flags)) return m;
        *skip = true;
        return 0;
    }

    static __device__ __forceinline__ uint32_t size(uint32_t len) { return egress::record_size(len); }

    // Dword j of the record of a frame of len bytes at src: the length word, the frame's dwords with
    // the last one masked to len, zeros to the record's end. The load stays inside the frame's words.
    static __device__ __forceinline__ uint32_t word(const uint32_t* __restrict__ src, uint32_t len, uint32_t j) {
        const uint32_t data_dw = (len + 3) / 4;
        const uint32_t at = j == 0 ? 0u : (j > data_dw ? data_dw - 1 : j - 1);
        uint32_t w = src[at];
        if (j == data_dw && (len & 3u)) w &= (1u << 8 * (len & 3u)) - 1u;
        return j == 0 ? egress::tx_len(len) : (j > data_dw ? 0u : w);
    }

    static __device__ __forceinline__ void list(const Params& q, uint64_t slot, uint32_t i, uint32_t, bool, uint64_t) {
        q.index[slot] = i;
    }
};

int ops_run(const halo_egress_config_t* cfg, uint32_t kind, const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
            const uint16_t* d_lens, uint32_t n, const void* d_selectors, uint64_t flood_mask, uint8_t* d_out,
            halo_egress_port_t* d_ports, uint32_t* d_index, uint32_t* d_skipped, void* d_workspace, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0)
        return hipMemsetAsync(d_ports, 0, cfg->n_ports * sizeof(halo_egress_port_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    PortStreamParams q{};
    q.bytes = d_bytes, q.offsets_dw = d_offsets_dw, q.lens = d_lens, q.sel = d_selectors;
    q.flood = flood_mask, q.valid = egress::port_bits(cfg->n_ports);
    fill_port_streams(q, n, cfg->n_ports, cfg->flags, cfg->region_bytes, d_workspace);
    q.index_cap = d_index ? cfg->index_cap : 0u;
    q.out = d_out, q.ports = d_ports, q.index = d_index, q.skipped = d_skipped;
    if (kind == HALO_EGRESS_KIND_MASKS) launch_port_streams<EgressStage<HALO_EGRESS_KIND_MASKS>>(q, st);
    else if (kind == HALO_EGRESS_KIND_ARP) launch_port_streams<EgressStage<HALO_EGRESS_KIND_ARP>>(q, st);
    else launch_port_streams<EgressStage<HALO_EGRESS_KIND_SWITCH>>(q, st);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const egress::DeviceOps kDeviceOps = {ops_run};

}  // namespace

namespace egress {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace egress
}  // namespace halo
