// rx_dhcp.hip — the device side of the DHCP decode (include/halo_rx.h, "DHCP") on gfx950: from a
// delivery stream in HBM to one 128-byte message record per DHCP delivery record. rx_dhcp_host.cc
// checks the arguments and holds the host loop; rx_dhcp.h holds the walk and the record's words
// both share.
//
// Launches, all on the caller's stream, the record count read on the device:
//   count   one lane per delivery index entry, a tile of kTile entries per workgroup: the record
//           header's kind alone; the tile's count of DHCP records goes to the workspace.
//   scan    one workgroup: tile_scan.h's scan over the tile counts; writes the whole summary (the
//           total, zeros elsewhere), so nothing has to be cleared first.
//   write   one lane per entry again, now with the message's rank: RxDhcp's port test,
//           ParseDhcpPkt's checks and ParseDhcpOption's walk over the aligned dwords that hold the
//           payload (the fixed header lies 4-byte aligned, so its fields are plain dword loads; the
//           option bytes and the hostname start anywhere and are funnelled with v_alignbyte_b32);
//           the record as eight 16-byte stores; the counters through LDS, then one global atomic
//           per workgroup and non-zero counter.
// The walk's state is registers (rx_dhcp.h, Options): no scratch. A wave's lanes walk option lists
// of different lengths and wait for the longest; DESIGN.md §28 has what that costs.
#include <hip/hip_runtime.h>

#include "halo_common.h"
#include "rx_dhcp.h"
#include "tile_scan.h"

namespace halo {
namespace {

using dhcp::kTile;

static_assert(sizeof(halo_dhcp_msg_t) == 4 * dhcp::kMsgWords && sizeof(halo_dhcp_summary_t) == 4 * dhcp::kSummaryWords &&
                  sizeof(halo_deliver_index_t) == 8 && sizeof(halo_deliver_hdr_t) == 24,
              "layouts the kernels index by hand");
static_assert(offsetof(halo_dhcp_summary_t, status_counts) == 8 && offsetof(halo_dhcp_summary_t, type_counts) == 28 &&
                  offsetof(halo_dhcp_msg_t, hostname) == 64 && offsetof(halo_dhcp_msg_t, req_ip) == 32 &&
                  offsetof(halo_dhcp_msg_t, mask_n) == 48,
              "layouts the kernels index by hand");

struct DhcpParams {
    const uint32_t* stream;  // the delivery stream as dwords
    const halo_deliver_summary_t* dsum;
    const uint2* index;
    uint32_t index_cap, n_tiles, msg_cap;
    uint4* msgs;  // 128-byte records as eight 16-byte words
    uint32_t* summary;
    uint32_t* tile_n;  // workspace: [tile] count: the tile's DHCP records; scan: those before the tile
};

// A payload in the stream: bytes pos .. pos + cnt - 1 from the aligned dwords that hold them (the
// upper one is loaded only when one of the bytes lies in it).
struct DevBytes {
    const uint32_t* dw;
    uint32_t base;  // the payload's byte offset in the stream
    __device__ __forceinline__ uint32_t span(uint32_t pos, uint32_t cnt) const {
        const uint32_t a = base + pos, s = a & 3u;
        const uint32_t lo = dw[a >> 2], hi = s + cnt > 4u ? dw[(a >> 2) + 1] : 0u;
        const uint32_t v = deliver::funnel(lo, hi, s);
        return cnt < 4u ? v & ((1u << 8u * cnt) - 1u) : v;
    }
};

// the stream byte offset of index entry k's record when it is a DHCP record, else kNotWritten
__device__ __forceinline__ uint32_t dhcp_record(const DhcpParams& q, uint32_t k) {
    if (k >= q.index_cap || k >= q.dsum->records) return dhcp::kNotWritten;
    const uint32_t off = q.index[k].y;
    if (off == dhcp::kNotWritten) return off;
    return dhcp::selected(q.stream[(off >> 2) + 1]) ? off : dhcp::kNotWritten;  // a record starts 4-byte aligned
}

__global__ void __launch_bounds__(kTile) dhcp_count_kernel(const DhcpParams q) {
    tile_count(q.tile_n, [&] { return dhcp_record(q, blockIdx.x * kTile + threadIdx.x) != dhcp::kNotWritten; });
}

__global__ void __launch_bounds__(256) dhcp_scan_kernel(const DhcpParams q) {
    const uint32_t msgs = scan_tiles(q.tile_n, q.n_tiles);
    if (threadIdx.x < dhcp::kSummaryWords) q.summary[threadIdx.x] = threadIdx.x == 0 ? msgs : 0u;
}

// the workgroup's counters: the summary's words 1 .. 15 (msgs_written, status_counts, type_counts)
constexpr uint32_t kCounters = dhcp::kSummaryWords;

__global__ void __launch_bounds__(kTile) dhcp_write_kernel(const DhcpParams q) {
    __shared__ uint32_t s_cnt[kCounters];
    if (threadIdx.x < kCounters) s_cnt[threadIdx.x] = 0;
    const uint32_t k = blockIdx.x * kTile + threadIdx.x;
    const uint32_t off = dhcp_record(q, k);
    const bool sel = off != dhcp::kNotWritten;
    const uint64_t votes = tile_votes<kTile>(sel);  // the barrier: s_cnt is cleared
    const uint32_t j = tile_rank<kTile>(votes, q.tile_n[blockIdx.x]);
    if (sel && j < q.msg_cap) {  // monotone in k: the messages that fit are a prefix
        const uint32_t* rec = q.stream + (off >> 2);
        uint32_t w[dhcp::kMsgWords];
        const uint32_t status = dhcp::msg_words(DevBytes{q.stream, off + deliver::kHdrBytes}, k, rec[1], rec[2], rec[3], w);
        uint4* o = q.msgs + 8ull * j;
#pragma unroll
        for (uint32_t x = 0; x < 8; ++x) o[x] = make_uint4(w[4 * x], w[4 * x + 1], w[4 * x + 2], w[4 * x + 3]);
        atomicAdd(&s_cnt[1], 1u);
        atomicAdd(&s_cnt[2 + status], 1u);
        if (status == HALO_DHCP_OK) atomicAdd(&s_cnt[2 + HALO_DHCP_STATUS_COUNT + dhcp::type_slot(w[2], (w[1] >> 16) & 0xFFu)], 1u);
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < kCounters && s_cnt[threadIdx.x]) atomicAdd(&q.summary[threadIdx.x], s_cnt[threadIdx.x]);
}

int ops_decode(const uint8_t* d_stream, const halo_deliver_summary_t* d_deliver_summary, const halo_deliver_index_t* d_index,
               uint32_t index_cap, halo_dhcp_msg_t* d_msgs, uint32_t msg_cap, halo_dhcp_summary_t* d_summary, void* d_workspace,
               halo_stream_t stream) {
    const int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (index_cap == 0)
        return hipMemsetAsync(d_summary, 0, sizeof(halo_dhcp_summary_t), st) == hipSuccess ? HALO_OK : HALO_E_HIP;
    DhcpParams q{};
    q.stream = reinterpret_cast<const uint32_t*>(d_stream), q.dsum = d_deliver_summary;
    q.index = reinterpret_cast<const uint2*>(d_index);
    q.index_cap = index_cap, q.n_tiles = (uint32_t)tiles_of(index_cap, kTile), q.msg_cap = msg_cap;
    q.msgs = reinterpret_cast<uint4*>(d_msgs), q.summary = reinterpret_cast<uint32_t*>(d_summary);
    q.tile_n = static_cast<uint32_t*>(d_workspace);
    hipLaunchKernelGGL(dhcp_count_kernel, dim3(q.n_tiles), dim3(kTile), 0, st, q);
    hipLaunchKernelGGL(dhcp_scan_kernel, dim3(1), dim3(256), 0, st, q);
    hipLaunchKernelGGL(dhcp_write_kernel, dim3(q.n_tiles), dim3(kTile), 0, st, q);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const dhcp::DeviceOps kDeviceOps = {ops_decode};

}  // namespace

namespace dhcp {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace dhcp
}  // namespace halo
