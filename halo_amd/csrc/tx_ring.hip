// tx_ring.hip — the tx ring producer's device side (include/halo_rx.h, "the tx ring producer";
// DESIGN.md §23): halo_ring_write_span with the span in HBM and the ring mapped for the device.
//
// A write is the record walk of ring_rx.hip over the examined window (guess, link, copy: it
// validates every header and yields every record's offset), then three small launches:
//   plan    — one wave reads the walk's info, head and tail (tail: system-scope acquire), decides
//             BAD_SPAN / OK / SHORT and, for SHORT, finds the cut by a 64-ary search over the walk's
//             ascending record offsets (four rounds for 2^20 records, not twenty dependent loads);
//   copy    — a grid of at most 256 workgroups (copy_blocks) strides over the taken bytes, split at the
//             data area's end; 16-byte stores aligned on the DESTINATION (the ring is host memory
//             behind PCIe, where whole aligned lines matter), 4-byte aligned 16-byte loads from HBM;
//   publish — one lane, behind the kernel boundary: system-scope release store of head + bytes
//             (only when bytes > 0), and the result.
// No workgroup waits on another and nothing waits for the consumer: a full ring is SHORT.
#include <hip/hip_runtime.h>

#include <new>

#include "halo_common.h"
#include "tx_ring.h"

namespace halo {
namespace {

using txring::Plan;

constexpr uint32_t kCopyThreads = 256;
constexpr uint32_t kCopyUnroll = 4;  // 16-byte units a lane has in flight per pass
constexpr uint32_t kCopyBlockBytes = kCopyThreads * kCopyUnroll * 16;  // a workgroup's bytes per pass

struct Params {
    const uint32_t* span;
    uint64_t span_bytes, window;
    uint8_t* d_mem;  // the ring header as the device sees it; the data area follows
    uint64_t size;
    const halo_rx_ring_scan_t* info;  // the walk's, over the window (not read when window == 0)
    const uint32_t* off_dw;           // record k's data starts at span dword off_dw[k]
    Plan* plan;
    halo_tx_ring_result_t* result;    // optional
};

// Span byte offset of record k's header; k == n: the end of the last record.
__device__ __forceinline__ uint64_t record_start(const Params& p, uint32_t k, uint32_t n, uint64_t end) {
    return k < n ? 4ull * (p.off_dw[k] - 1u) : end;
}

__global__ void __launch_bounds__(64) txring_plan_kernel(const Params p) {
    const uint32_t lane = threadIdx.x;
    // head is the producer's own word (the previous call's publish precedes this kernel in stream
    // order); tail is the consumer's: the counterpart of the host's __ATOMIC_ACQUIRE load
    const uint64_t head = __hip_atomic_load(reinterpret_cast<const uint64_t*>(p.d_mem), __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_SYSTEM);
    const uint64_t tail = __hip_atomic_load(reinterpret_cast<const uint64_t*>(p.d_mem + 64), __ATOMIC_ACQUIRE,
                                            __HIP_MEMORY_SCOPE_SYSTEM);
    const uint64_t room = txring::room(p.size, head, tail);
    uint32_t n = 0, stop = HALO_RING_STOP_EMPTY;
    uint64_t end = 0;
    if (p.window) {
        n = p.info->n_frames;
        stop = p.info->stop;
        end = p.info->end_bytes;
    }
    // a record cut by the window (not by the span's end) is not an error: it is simply not taken
    const bool bad = stop == HALO_RING_STOP_BAD_LEN || stop == HALO_RING_STOP_CAPACITY ||
                     (stop == HALO_RING_STOP_PARTIAL && p.window == p.span_bytes);
    uint32_t records = 0;
    uint64_t take = 0;
    if (!bad) {
        if (end <= room) {
            records = n;
            take = end;
        } else {
            // the last k with record_start(k) <= room, in [lo, hi]: record_start(0) = 0 <= room and
            // record_start(n) = end > room. 64 probes a round.
            uint32_t lo = 0, hi = n - 1;
            while (lo < hi) {  // uniform
                const uint64_t width = hi - lo, step = (width + 63) / 64;
                const uint32_t k = lo + (uint32_t)min(width, (uint64_t)(lane + 1) * step);
                const uint32_t c = (uint32_t)__popcll(__ballot(record_start(p, k, n, end) <= room));
                const uint32_t below = lo + (uint32_t)min(width, (uint64_t)c * step);
                hi = c == 64 ? below : lo + (uint32_t)min(width, (uint64_t)(c + 1) * step) - 1u;
                lo = below;
            }
            records = lo;
            take = record_start(p, lo, n, end);
        }
    }
    if (lane == 0) {
        Plan pl;
        pl.head = head;
        pl.take = take;
        pl.records = records;
        pl.status = bad ? HALO_TXRING_BAD_SPAN : take == p.span_bytes ? HALO_TXRING_OK : HALO_TXRING_SHORT;
        *p.plan = pl;
    }
}

typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));

// n_dw dwords from src (HBM) to dst (the mapped ring), both 4-byte aligned, by the whole grid.
// QUAD: dst's first up to three dwords and last up to three go singly, everything between as
// 16-byte stores on 16-byte boundaries of dst (a wave stores 1 KiB of whole lines) from 16-byte
// loads at src's alignment. Otherwise plain dwords (a wave: 256 contiguous bytes an instruction).
template <bool QUAD>
__device__ __forceinline__ void copy_segment(uint32_t* dst, const uint32_t* src, uint64_t n_dw) {
    const uint32_t tid = threadIdx.x;
    if constexpr (QUAD) {
        const uint64_t lead = min(n_dw, (uint64_t)(((16u - ((uint32_t)reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2));
        const uint64_t nq = (n_dw - lead) >> 2, rest = lead + 4 * nq;
        if (blockIdx.x == 0) {
            if (tid < lead) dst[tid] = src[tid];
            if (tid >= 64 && rest + (tid - 64) < n_dw) dst[rest + (tid - 64)] = src[rest + (tid - 64)];
        }
        uint4* dq = reinterpret_cast<uint4*>(dst + lead);
        const u32x4a4* sq = reinterpret_cast<const u32x4a4*>(src + lead);
        constexpr uint64_t kPer = (uint64_t)kCopyThreads * kCopyUnroll;
        for (uint64_t q0 = blockIdx.x * kPer + tid; q0 < nq; q0 += gridDim.x * kPer) {
            u32x4a4 v[kCopyUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kCopyUnroll; ++u)
                if (q0 + u * kCopyThreads < nq) v[u] = sq[q0 + u * kCopyThreads];
#pragma unroll
            for (uint32_t u = 0; u < kCopyUnroll; ++u)
                if (q0 + u * kCopyThreads < nq) dq[q0 + u * kCopyThreads] = make_uint4(v[u].x, v[u].y, v[u].z, v[u].w);
        }
    } else {
        constexpr uint32_t kDw = 4 * kCopyUnroll;  // the same bytes per workgroup and pass
        constexpr uint64_t kPer = (uint64_t)kCopyThreads * kDw;
        for (uint64_t i0 = blockIdx.x * kPer + tid; i0 < n_dw; i0 += gridDim.x * kPer) {
            uint32_t v[kDw];
#pragma unroll
            for (uint32_t u = 0; u < kDw; ++u)
                if (i0 + u * kCopyThreads < n_dw) v[u] = src[i0 + u * kCopyThreads];
#pragma unroll
            for (uint32_t u = 0; u < kDw; ++u)
                if (i0 + u * kCopyThreads < n_dw) dst[i0 + u * kCopyThreads] = v[u];
        }
    }
}

template <bool QUAD>
__global__ void __launch_bounds__(kCopyThreads) txring_copy_kernel(const Params p) {
    const uint64_t head = p.plan->head, take = p.plan->take;
    if (take == 0) return;  // uniform: BAD_SPAN, or no room for the first record
    // take <= room <= size (plan), so the two segments never overlap and stay inside the data area
    const uint64_t pos = head & (p.size - 1), first = min(take, p.size - pos);
    uint32_t* data = reinterpret_cast<uint32_t*>(p.d_mem + kRbHeader);
    copy_segment<QUAD>(data + (pos >> 2), p.span, first >> 2);
    if (first < take) copy_segment<QUAD>(data, p.span + (first >> 2), (take - first) >> 2);  // around the end
}

__global__ void __launch_bounds__(64) txring_publish_kernel(const Params p) {
    if (threadIdx.x != 0) return;
    const Plan pl = *p.plan;
    if (pl.take) {
        // every copied byte left the copy kernel before this one started; the release orders this
        // lane's view of them before the store the consumer acquires
        __threadfence_system();
        __hip_atomic_store(reinterpret_cast<uint64_t*>(p.d_mem), pl.head + pl.take, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (p.result) {
        halo_tx_ring_result_t r;
        r.status = pl.status;
        r.records = pl.records;
        r.bytes = pl.take;
        r.head = pl.head + pl.take;
        *p.result = r;
    }
}

uint32_t copy_blocks(uint64_t bytes) {
    const uint64_t kMax = 256;  // one workgroup per CU
    const uint64_t b = (bytes + kCopyBlockBytes - 1) / kCopyBlockBytes;
    return (uint32_t)(b > kMax ? kMax : (b ? b : 1));
}

// Device address of host memory [p, p + bytes) when the runtime maps it in one piece, else nullptr.
void* runtime_view(const void* p, uint64_t bytes) {
    void *d0 = nullptr, *d1 = nullptr;
    if (hipHostGetDevicePointer(&d0, const_cast<void*>(p), 0) != hipSuccess ||
        hipHostGetDevicePointer(&d1, const_cast<uint8_t*>(static_cast<const uint8_t*>(p)) + bytes - 1, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return static_cast<uint8_t*>(d1) - static_cast<uint8_t*>(d0) == (ptrdiff_t)(bytes - 1) ? d0 : nullptr;
}

int ops_attach(int device, uint8_t* mem, uint64_t size, uint32_t attach_flags, halo_tx_ring** out) {
    // a registered ring pins the whole pages it spans: it must start on a page of its own
    const uint64_t page = host_page_size(), bytes = kRbHeader + size;
    const bool reg = attach_flags & HALO_RING_REGISTER;
    if (reg && (reinterpret_cast<uintptr_t>(mem) % page)) return HALO_E_INVAL;
    int rc = halo_rx_init(device);
    if (rc) return rc;
    auto* r = new (std::nothrow) halo_tx_ring;
    if (!r) return HALO_E_NOMEM;
    r->device = device;
    r->mem = mem;
    r->size = size;
    if (reg) {
        if ((rc = host_reg_add(mem, (bytes + page - 1) / page * page, kRegRing))) {  // INVAL: shares a page with a live one
            delete r;
            return rc;
        }
        r->registered = true;
    }
    r->d_mem = static_cast<uint8_t*>(host_reg_device_view(mem, bytes));
    if (!r->d_mem) r->d_mem = static_cast<uint8_t*>(runtime_view(mem, bytes));
    if (!r->d_mem) {  // not mapped for the device (or, after a registration, no device view of it)
        // after a registration: HALO_E_HIP, and the pages may still be pinned if the removal fails too
        // (the caller keeps the ring memory allocated on HALO_E_HIP from a registering attach)
        if (reg) (void)host_reg_remove(mem, kRegRing);
        delete r;
        return reg ? HALO_E_HIP : HALO_E_INVAL;
    }
    *out = r;
    return HALO_OK;
}

int ops_detach(halo_tx_ring* r) {
    (void)hipSetDevice(r->device);
    // the caller's streams are not known here: wait for the device, so that no kernel of a write
    // still stores into the ring when its memory is unmapped or freed
    int rc = drain_device(r->device);
    if (r->registered && host_reg_remove(r->mem, kRegRing) != HALO_OK) rc = HALO_E_HIP;
    delete r;
    return rc == HALO_OK ? HALO_OK : HALO_E_HIP;
}

int ops_write(halo_tx_ring* r, const uint8_t* d_span, uint64_t span_bytes, halo_tx_ring_result_t* d_result,
              uint8_t* ws, uint64_t ws_bytes, halo_stream_t stream) {
    if (hipSetDevice(r->device) != hipSuccess) return HALO_E_NODEV;
    int rc = check_device();
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const txring::Layout l = txring::layout(span_bytes, 0);
    Params p{};
    p.span = reinterpret_cast<const uint32_t*>(d_span);
    p.span_bytes = span_bytes;
    p.window = txring::window(span_bytes, r->size);
    p.d_mem = r->d_mem;
    p.size = r->size;
    p.info = reinterpret_cast<const halo_rx_ring_scan_t*>(ws + txring::kInfoOff);
    p.off_dw = reinterpret_cast<const uint32_t*>(ws + l.off_dw);
    p.plan = reinterpret_cast<Plan*>(ws + txring::kPlanOff);
    p.result = d_result;
    if (p.window) {
        rc = halo_rx_ring_scan_device(d_span, p.window, r->size, HALO_TXRING_MAX_RECORD, 0,
                                      reinterpret_cast<uint32_t*>(ws + l.off_dw), reinterpret_cast<uint16_t*>(ws + l.lens),
                                      reinterpret_cast<halo_rx_ring_scan_t*>(ws + txring::kInfoOff), ws + l.scan,
                                      ws_bytes - l.scan, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(txring_plan_kernel, dim3(1), dim3(64), 0, st, p);
    if (p.window) {
        if (r->copy_dwords)
            hipLaunchKernelGGL(txring_copy_kernel<false>, dim3(copy_blocks(p.window)), dim3(kCopyThreads), 0, st, p);
        else
            hipLaunchKernelGGL(txring_copy_kernel<true>, dim3(copy_blocks(p.window)), dim3(kCopyThreads), 0, st, p);
    }
    hipLaunchKernelGGL(txring_publish_kernel, dim3(1), dim3(64), 0, st, p);
    return hipGetLastError() == hipSuccess ? HALO_OK : HALO_E_HIP;
}

const txring::DeviceOps kDeviceOps = {ops_attach, ops_detach, ops_write};

}  // namespace

namespace txring {
const DeviceOps* device_ops() { return &kDeviceOps; }
}  // namespace txring
}  // namespace halo
