// tx_ring_host.cc — the tx ring producer's C entry points (include/halo_rx.h, "the tx ring
// producer"): every argument check and the validation of the ring's header, answered before any
// device is looked for. Checks only; no HIP: attach's registration and the kernels live in
// tx_ring.hip behind txring::device_ops().
#include "host_layout.h"
#include "host_logic.h"
#include "tx_ring.h"

using namespace halo;  // host_layout.h
using namespace halo::txring;

extern "C" HALO_API int halo_tx_ring_attach(int device, void* ring_mem, int64_t offset, uint32_t attach_flags,
                                            halo_tx_ring_t** out) {
    if (!out) return HALO_E_INVAL;
    *out = nullptr;
    uint64_t size = 0, tail = 0;
    uint8_t* mem = static_cast<uint8_t*>(ring_mem);
    const int rc = halo::validate_ring(mem, offset, &size, &tail);
    if (rc) return rc;
    if (attach_flags & ~HALO_RING_REGISTER) return HALO_E_INVAL;  // PERSISTENT is a consumer's flag
    if (device < 0) return HALO_E_NODEV;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->attach(device, mem, size, attach_flags, out) : HALO_E_NODEV;
}

extern "C" HALO_API int halo_tx_ring_detach(halo_tx_ring_t* r) {
    if (!r) return HALO_E_INVAL;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->detach(r) : HALO_E_NODEV;
}

extern "C" HALO_API int halo_tx_ring_debug_copy_mode(halo_tx_ring_t* r, uint32_t mode) {
    if (!r || mode > 1) return HALO_E_INVAL;
    r->copy_dwords = mode == 1;
    return HALO_OK;
}

extern "C" HALO_API uint64_t halo_tx_ring_workspace(uint64_t span_bytes) {
    // the walk's workspace for the whole span serves every window of it (it grows with the span)
    const uint64_t scan = halo_rx_ring_scan_workspace(span_bytes, HALO_TXRING_MAX_RECORD);
    return scan ? layout(span_bytes, scan).bytes : 0;
}

extern "C" HALO_API int halo_tx_ring_write_span_device(halo_tx_ring_t* r, const uint8_t* d_span, uint64_t span_bytes,
                                                       halo_tx_ring_result_t* d_result, void* d_workspace,
                                                       uint64_t workspace_bytes, halo_stream_t stream) {
    if (!r) return HALO_E_INVAL;
    if ((span_bytes & 3u) || (span_bytes && (!d_span || misaligned(d_span, 4)))) return HALO_E_INVAL;
    if (misaligned(d_result, 8)) return HALO_E_INVAL;
    if (!d_workspace || misaligned(d_workspace, 16)) return HALO_E_INVAL;
    const uint64_t need = halo_tx_ring_workspace(span_bytes);
    if (!need || workspace_bytes < need) return HALO_E_INVAL;
    const DeviceOps* ops = device_ops ? device_ops() : nullptr;
    return ops ? ops->write(r, d_span, span_bytes, d_result, static_cast<uint8_t*>(d_workspace), workspace_bytes, stream)
               : HALO_E_NODEV;
}
