// tx_dhcp.hip — the device side of the DHCP reply build (include/halo_rx.h, "DHCP") on gfx950:
// from 32-byte reply descriptors to the UDP payloads BuildDhcpPkt makes, in fixed 288-byte slots,
// and one transmit-build descriptor per reply. tx_dhcp_host.cc checks the arguments and holds the
// host loop; rx_dhcp.h holds the byte function of a slot and the descriptor's words both share.
//
// One launch: one lane per output dword. Slot i is dwords [72 i, 72 i + 72) of the payload buffer,
// so the lanes of a wave store consecutive dwords whatever the replies' kinds are, every dword has
// one writer and nothing is scanned. A lane loads its reply's 32 bytes (the 72 lanes of a slot load
// the same two 16-byte words: one request per wave and slot), makes its dword of four values of
// the byte function of (kind, position) — 59 of the 72 are constants or a header field, the option
// dwords a few selects — and stores it; the slot's lane 0 also stores the 40-byte descriptor.
// No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "rx_dhcp.h"

namespace halo {
namespace {

static_assert(sizeof(halo_dhcp_reply_t) == 32 && sizeof(halo_tx_build_desc_t) == 4 * dhcp::kDescWords &&
                  sizeof(halo_dhcp_config_t) == 24 && dhcp::kSlotWords == 72,
              "layouts the kernel indexes by hand");
static_assert(offsetof(halo_dhcp_reply_t, chaddr) == 12 && offsetof(halo_dhcp_reply_t, req_ip) == 20 &&
                  offsetof(halo_tx_build_desc_t, dst_mac) == 32 && offsetof(halo_tx_build_desc_t, src_ip) == 16,
              "layouts the kernel indexes by hand");

constexpr uint32_t kBlock = 256;

struct BuildParams {
    const uint4* replies;  // 32-byte records as two 16-byte words
    uint32_t n;
    dhcp::Addrs addrs;
    uint32_t* payload;
    uint2* descs;  // 40-byte records as five 8-byte words
};

__global__ void __launch_bounds__(kBlock) dhcp_build_kernel(const BuildParams q) {
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (uint64_t)q.n * dhcp::kSlotWords) return;
    const uint32_t i = (uint32_t)(t / dhcp::kSlotWords), d = (uint32_t)(t % dhcp::kSlotWords);
    const uint4 lo = q.replies[2ull * i], hi = q.replies[2ull * i + 1];
    const dhcp::Reply r{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
    q.payload[t] = dhcp::reply_word(r, q.addrs, d);
    if (d == 0) {
        uint32_t w[dhcp::kDescWords];
        dhcp::desc_words(r, q.addrs, i, w);
        uint2* o = q.descs + 5ull * i;
#pragma unroll
        for (uint32_t x = 0; x < 5; ++x) o[x] = make_uint2(w[2 * x], w[2 * x + 1]);
    }
}

int ops_build(const halo_dhcp_config_t* cfg, const halo_dhcp_reply_t* d_replies, uint32_t n, uint8_t* d_payload,
              halo_tx_build_desc_t* d_descs, halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    if (n == 0) return HALO_OK;
    BuildParams q{};
    q.replies = reinterpret_cast<const uint4*>(d_replies), q.n = n;
    q.addrs = dhcp::Addrs{cfg->ip, cfg->network_mask, cfg->dns};
    q.payload = reinterpret_cast<uint32_t*>(d_payload), q.descs = reinterpret_cast<uint2*>(d_descs);
    const uint64_t blocks = ((uint64_t)n * dhcp::kSlotWords + kBlock - 1) / kBlock;  // n <= 2^23: below 2^31
    hipLaunchKernelGGL(dhcp_build_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), q);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const dhcp::BuildOps kBuildOps = {ops_build};

}  // namespace

namespace dhcp {
const BuildOps* build_ops() { return &kBuildOps; }
}  // namespace dhcp
}  // namespace halo
