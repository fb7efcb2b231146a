// rx_hist.hip — the host half of the rx kernels' status histogram, process-wide: a device's set of
// trees (made once, at first use, and never freed), the probe that checks every dispatch carries
// the AQL barrier bit the trees rely on, and the key words' reset and test hook. The device half is
// rx_hist.h; the layout and the protocol are described in halo_common.h.
#include <hip/hip_runtime.h>

#include <mutex>

#include "halo_common.h"

namespace halo {

int stream_device(hipStream_t s) {
    int dev = -1;
    if (s != nullptr && s != hipStreamPerThread) {
        if (hipStreamGetDevice(s, &dev) == hipSuccess) return dev;
        (void)hipGetLastError();
        return -1;
    }
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return dev;
}

namespace {
std::mutex g_trees_mu;
uint32_t* g_trees[64];      // a device's set: made once, never freed (graphs hold its address)
bool g_no_barriers[64];     // the probe found a dispatch without the barrier bit: keys stay poisoned

// Writes its own AQL packet header (the barrier bit is bit 8) to *out.
__global__ void dispatch_header_probe(unsigned long long* out) {
    if (threadIdx.x == 0) *out = *static_cast<const volatile uint16_t*>((const void*)__builtin_amdgcn_dispatch_ptr());
}

// flush_hist relies on every dispatch carrying the barrier bit (the runtime's in-order streams do:
// profiles/r05/queue_probe.log) instead of re-reading the packet in every block, which costs 4x the
// launch. Checked once per device on the null stream and a fresh stream; without the bit the keys
// are poisoned, and every launch adds straight into the caller's counters (slow, exact).
bool barrier_bits_set(unsigned long long* scratch) {
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return false;
    hipLaunchKernelGGL(dispatch_header_probe, dim3(1), dim3(64), 0, nullptr, scratch);
    hipLaunchKernelGGL(dispatch_header_probe, dim3(1), dim3(64), 0, st, scratch + 1);
    unsigned long long h[2] = {0, 0};
    const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess &&
                    hipStreamSynchronize(nullptr) == hipSuccess &&
                    hipMemcpy(h, scratch, sizeof h, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipStreamDestroy(st);
    return ok && ((h[0] >> 8) & 1u) && ((h[1] >> 8) & 1u);
}
}  // namespace

uint32_t* hist_trees(int device, hipStream_t capture_probe) {
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> g(g_trees_mu);
    uint32_t*& p = g_trees[device];
    if (p) return p;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(capture_probe, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return nullptr;  // no allocation inside a capture: halo_rx_init(device) makes the set beforehand
    }
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    if (cur != device && hipSetDevice(device) != hipSuccess) return nullptr;
    void* m = nullptr;
    bool ok = hipMalloc(&m, kHistSetBytes) == hipSuccess;
    const bool barriers = ok && barrier_bits_set(static_cast<unsigned long long*>(m) + kHistKeyWords);
    ok = ok && hipMemsetAsync(m, 0, kHistSetBytes, nullptr) == hipSuccess &&
         (barriers || hipMemsetAsync(m, 0xFF, 8ull * kHistTrees, nullptr) == hipSuccess) &&
         hipStreamSynchronize(nullptr) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (m) (void)hipFree(m);
        m = nullptr;
    }
    if (cur != device) (void)hipSetDevice(cur);
    g_no_barriers[device] = ok && !barriers;
    p = static_cast<uint32_t*>(m);
    return p;
}

namespace {
// Writes the key words of `device`'s set (g_trees_mu held): all 0 (free), all ~0 (poisoned), or
// ids no queue has for all but the first `free_keys` slots.
int write_keys(int device, int fill, uint32_t free_keys) {
    uint32_t* set = g_trees[device];
    if (!set) return HALO_E_NOMEM;
    unsigned long long k[kHistKeyWords];
    for (uint32_t j = 0; j < kHistKeyWords; ++j)
        k[j] = fill == 0 ? 0ull : fill == 1 ? ~0ull : (j < free_keys ? 0ull : 0x40ull * (j + 1));  // not a queue address
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return HALO_E_NODEV;
    if (cur != device && hipSetDevice(device) != hipSuccess) return HALO_E_NODEV;
    const bool ok = hipMemcpy(set, k, sizeof k, hipMemcpyHostToDevice) == hipSuccess;
    if (cur != device) (void)hipSetDevice(cur);
    return ok ? HALO_OK : HALO_E_HIP;
}
}  // namespace

int hist_trees_reset_keys(int device) {
    if (device < 0 || device >= 64) return HALO_E_NODEV;
    std::lock_guard<std::mutex> g(g_trees_mu);
    if (!g_trees[device]) return HALO_OK;
    return write_keys(device, g_no_barriers[device] ? 1 : 0, 0);
}

int hist_keys_debug(int device, int op, uint32_t arg) {
    if (device < 0 || device >= 64) return HALO_E_NODEV;
    if (op == 3) return hist_trees_reset_keys(device);
    if (!hist_trees(device, nullptr)) return HALO_E_NOMEM;
    std::lock_guard<std::mutex> g(g_trees_mu);
    if (op == 1) return write_keys(device, 1, 0);
    if (op == 2) return arg > kHistTrees ? HALO_E_INVAL : write_keys(device, 2, arg);
    if (op != 0) return HALO_E_INVAL;
    unsigned long long k[kHistKeyWords];
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) return HALO_E_NODEV;
    if (cur != device && hipSetDevice(device) != hipSuccess) return HALO_E_NODEV;
    const bool ok = hipMemcpy(k, g_trees[device], sizeof k, hipMemcpyDeviceToHost) == hipSuccess;
    if (cur != device) (void)hipSetDevice(cur);
    if (!ok) return HALO_E_HIP;
    int claimed = 0;
    for (uint32_t j = 0; j < kHistTrees; ++j) claimed += k[j] != 0 && k[j] != ~0ull;
    return claimed;
}
}  // namespace halo
