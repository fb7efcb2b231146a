// rx_dhcp_host.cc — the DHCP decode's C entry points (include/halo_rx.h, "DHCP"): the argument
// checks of halo_dhcp_decode_device, answered before any device is looked for, and
// halo_dhcp_decode_host, the sequential loop with the same outputs. No HIP: the kernels live in
// rx_dhcp.hip behind dhcp::device_ops(), and this file compiles alone with g++ (tools/fuzz_dhcp.cc
// drives it under ASan/UBSan).
#include <string.h>

#include "rx_dhcp.h"

namespace halo {
namespace dhcp {
namespace {

// What both entry points ask
int check(const uint8_t* stream, const halo_deliver_summary_t* dsum, const halo_deliver_index_t* index, uint32_t index_cap,
          const halo_dhcp_msg_t* msgs, uint32_t msg_cap, const halo_dhcp_summary_t* summary) {
    if (!summary || !dsum) return HALO_E_INVAL;
    if (index_cap && (!stream || !index)) return HALO_E_INVAL;
    if (msg_cap && !msgs) return HALO_E_INVAL;
    return HALO_OK;
}

struct HostBytes {  // a payload in host memory, any alignment: byte loads, nothing past the span
    const uint8_t* p;
    uint32_t span(uint32_t pos, uint32_t cnt) const {
        uint32_t v = 0;
        for (uint32_t i = 0; i < cnt; ++i) v |= (uint32_t)p[pos + i] << 8u * i;
        return v;
    }
};

}  // namespace
}  // namespace dhcp
}  // namespace halo

using namespace halo;  // host_layout.h
using namespace halo::dhcp;

extern "C" HALO_API uint64_t halo_dhcp_decode_workspace(uint32_t index_cap) { return dhcp::workspace_bytes(index_cap); }

extern "C" HALO_API int halo_dhcp_decode_device(const uint8_t* d_stream, const halo_deliver_summary_t* d_deliver_summary,
                                                const halo_deliver_index_t* d_index, uint32_t index_cap,
                                                halo_dhcp_msg_t* d_msgs, uint32_t msg_cap, halo_dhcp_summary_t* d_summary,
                                                void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream) {
    int rc;
    if ((rc = check(d_stream, d_deliver_summary, d_index, index_cap, d_msgs, msg_cap, d_summary))) return rc;
    if (misaligned(d_msgs, 16) || misaligned(d_index, 8) || misaligned(d_summary, 8) || misaligned(d_deliver_summary, 8) ||
        misaligned(d_workspace, 8) || misaligned(d_stream, 4))
        return HALO_E_INVAL;
    if (index_cap && (!d_workspace || workspace_bytes < halo_dhcp_decode_workspace(index_cap))) return HALO_E_INVAL;
    const dhcp::DeviceOps* ops = dhcp::device_ops ? dhcp::device_ops() : nullptr;
    return ops ? ops->decode(d_stream, d_deliver_summary, d_index, index_cap, d_msgs, msg_cap, d_summary, d_workspace, stream)
               : HALO_E_NODEV;
}

extern "C" HALO_API int halo_dhcp_decode_host(const uint8_t* stream, const halo_deliver_summary_t* deliver_summary,
                                              const halo_deliver_index_t* index, uint32_t index_cap, halo_dhcp_msg_t* msgs,
                                              uint32_t msg_cap, halo_dhcp_summary_t* summary) {
    int rc;
    if ((rc = check(stream, deliver_summary, index, index_cap, msgs, msg_cap, summary))) return rc;
    uint32_t s[kSummaryWords];  // no alignment asked of host memory: built here, copied out
    memset(s, 0, sizeof s);
    const uint32_t records = load_u32(deliver_summary);  // halo_deliver_summary_t.records
    const uint32_t nrec = records < index_cap ? records : index_cap;
    for (uint32_t k = 0; k < nrec; ++k) {
        const uint32_t off = load_u32(reinterpret_cast<const uint8_t*>(index) + 8ull * k + 4);
        if (off == kNotWritten) continue;
        const uint8_t* rec = stream + off;
        const uint32_t hw1 = load_u32(rec + 4);
        if (!selected(hw1)) continue;
        const uint32_t j = s[0]++;
        if (j >= msg_cap) continue;
        uint32_t w[kMsgWords];
        const uint32_t status = msg_words(HostBytes{rec + deliver::kHdrBytes}, k, hw1, load_u32(rec + 8), load_u32(rec + 12), w);
        memcpy(reinterpret_cast<uint8_t*>(msgs) + 4ull * kMsgWords * j, w, sizeof w);
        ++s[1];
        ++s[2 + status];
        if (status == HALO_DHCP_OK) ++s[2 + HALO_DHCP_STATUS_COUNT + type_slot(w[2], (w[1] >> 16) & 0xFFu)];
    }
    memcpy(summary, s, sizeof s);
    return HALO_OK;
}
