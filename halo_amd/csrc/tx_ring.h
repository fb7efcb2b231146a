// tx_ring.h — the tx ring producer (include/halo_rx.h, "the tx ring producer"): what the entry
// points (tx_ring_host.cc) and the kernels (tx_ring.hip) must agree on — a record's size, the room
// rule, the examined window, the workspace layout — and the handle. Plain C++17, no HIP:
// tx_ring_host.cc holds only argument checks and reaches the device side through device_ops().
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HALO_TXRING_FN __host__ __device__ __forceinline__
#else
#define HALO_TXRING_FN inline
#endif
#include <stdint.h>

#include "../../include/halo_rx.h"

// The producer's handle: the ring as the host and as the device see it.
struct halo_tx_ring {
    int device = 0;
    uint8_t* mem = nullptr;    // the RingBuffer header; the data area follows
    uint8_t* d_mem = nullptr;  // the same bytes, the device's address
    uint64_t size = 0;
    bool registered = false;   // this attach registered the ring (detach unregisters)
    bool copy_dwords = false;  // halo_tx_ring_debug_copy_mode: the plain-dword copy kernel
};

// Measurement hook, exported but not part of the public header (tools/bench_txring.py and one test
// reach it by name): mode 0 = the copy kernel's 16-byte stores aligned on the ring (the default),
// 1 = plain 4-byte accesses. The ring bytes are the same. Not while a write is being enqueued.
extern "C" HALO_API int halo_tx_ring_debug_copy_mode(halo_tx_ring_t* ring, uint32_t mode);

namespace halo {
namespace txring {

// ringBufferRecordSize (mem/ring_buffer.go:47-50): u32 length + bytes, 4-byte aligned
HALO_TXRING_FN uint64_t record_size(uint32_t len) { return (4ull + len + 3ull) & ~3ull; }

// Free bytes of a ring of `size` with the cursors `head` and `tail`, as halo_ring_write_span has it:
// nothing when the cursors are out of order or tail is not on a record boundary.
HALO_TXRING_FN uint64_t room(uint64_t size, uint64_t head, uint64_t tail) {
    const uint64_t used = head - tail;
    return used <= size && !(tail & 3u) ? size - used : 0;
}

// The bytes of a span the device examines: no prefix longer than the ring can be taken.
HALO_TXRING_FN uint64_t window(uint64_t span_bytes, uint64_t size) { return span_bytes < size ? span_bytes : size; }

// Workspace of a write: the walk's info and the plan (one 256-byte block), the walk's record
// offsets (u32 per record; a record is >= 8 bytes) and lengths (u16), then the walk's own workspace
// (halo_rx_ring_scan_workspace). Every part starts 16-byte aligned.
constexpr uint64_t kCtlBytes = 256, kInfoOff = 0, kPlanOff = 64;
struct Layout {
    uint64_t off_dw, lens, scan, bytes;
};
HALO_TXRING_FN uint64_t up16(uint64_t x) { return (x + 15ull) & ~15ull; }
HALO_TXRING_FN Layout layout(uint64_t span_bytes, uint64_t scan_bytes) {
    const uint64_t max_records = span_bytes / 8;
    Layout l{};
    l.off_dw = kCtlBytes;
    l.lens = l.off_dw + up16(4 * max_records);
    l.scan = l.lens + up16(2 * max_records);
    l.bytes = l.scan + up16(scan_bytes);
    return l;
}

// What the plan kernel leaves for the copy and publish kernels.
struct Plan {
    uint64_t head;     // the producer's cursor before the call
    uint64_t take;     // bytes to copy: a whole number of records
    uint32_t records;
    uint32_t status;   // HALO_TXRING_*
};

// The device side (tx_ring.hip); tx_ring_host.cc reaches it only through this, after it has checked
// every argument and the ring's header.
struct DeviceOps {
    int (*attach)(int device, uint8_t* mem, uint64_t size, uint32_t attach_flags, halo_tx_ring** out);
    int (*detach)(halo_tx_ring* r);
    int (*write)(halo_tx_ring* r, const uint8_t* d_span, uint64_t span_bytes, halo_tx_ring_result_t* d_result,
                 uint8_t* d_workspace, uint64_t workspace_bytes, halo_stream_t stream);
};
// Defined by tx_ring.hip; absent (null) in a host-only build, where the calls are HALO_E_NODEV.
const DeviceOps* device_ops() __attribute__((weak));

}  // namespace txring
}  // namespace halo
