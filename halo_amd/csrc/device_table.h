// device_table.h — the host side of a device-resident table, shared by the .hip files that keep one
// (nat_lookup.hip, arp_fwd.hip, pmflow_fwd.hip, route_lpm.hip; switch_fwd.hip takes the device
// helpers): switching to the table's device, growing a device array, the two generations a sync
// writes and publishes under lookups in flight, the stamp array two generations share, the walk
// over a route table's ids, and the lifecycle of the NAT, ARP and return-flow tables' device copy:
// Exclusive, fold, sync_begin and the fold / publish / destroy entries. HIP code only: a *_table.h
// never includes it, they stay plain C++.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <vector>

#include "halo_common.h"

namespace halo {

struct DeviceScope {  // run on `dev`, restore the caller's current device
    int prev = -1;
    explicit DeviceScope(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceScope() {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
    }
};

// HALO_OK when this process has a HIP device `device`; else HALO_E_NODEV, HIP's error cleared.
inline int device_present(int device) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || device >= cnt) {
        (void)hipGetLastError();
        return HALO_E_NODEV;
    }
    return HALO_OK;
}

// Room for `need` elements: a new array of twice the size (256 at first) replaces the old one,
// whose contents are not kept.
template <typename T>
int grow(T*& p, size_t& cap, size_t need) {
    if (need <= cap) return HALO_OK;
    size_t c = cap ? cap : 256;
    while (c < need) c *= 2;
    T* q = nullptr;
    if (hipMalloc(&q, c * sizeof(T)) != hipSuccess) return HALO_E_NOMEM;
    if (p) (void)hipFree(p);
    p = q;
    cap = c;
    return HALO_OK;
}

// The device copies of a table, double-buffered: lookups read the published generation; a sync
// compiles into the other one and then publishes it, so a lookup in flight never sees a table
// being rewritten or freed. Nothing here takes a lock: the entry points do, visibly.
template <typename Gen>
struct Generations {
    Gen gen[2];
    int device = -1;
    std::atomic<int> active{-1};  // published generation, -1 before the first sync
    // Lookups hold it shared from taking their view until their kernel is enqueued; a sync, a fold
    // or an expiry holds it exclusively while it drains the device and rewrites the unpublished
    // generation, so no lookup can be enqueued against a generation between its view and the drain.
    mutable std::shared_mutex view_mu;

    // The published generation, null before the first sync; view_mu held, shared or exclusively.
    const Gen* published() const {
        const int a = active.load(std::memory_order_acquire);
        return a < 0 ? nullptr : &gen[a];
    }
    // The generation to write, null when the device could not be drained. The caller holds view_mu
    // exclusively and runs on `device` under a ParkResidents (the drains, hipFree and the copies).
    Gen* begin_write() {
        const int cur = active.load(std::memory_order_acquire);
        // the generation written now was last published before `cur`: lookups launched while it was
        // active may still be running on any stream of the device, so drain the device first
        // (resident consumers are stopped for it, so a persistent ring's kernel cannot hold the write
        // lock, and the lookups behind it, for its 20 ms idle window)
        if (cur >= 0 && drain_device(device) != HALO_OK) return nullptr;
        return &gen[cur < 0 ? 0 : 1 - cur];
    }
    // Publishes the generation begin_write handed out, now written.
    int publish() {
        // hipMemcpy from pageable memory returns once the host buffer is consumed, not when the copy
        // has landed: wait for it before publishing
        if (drain_device(device) != HALO_OK) return HALO_E_HIP;
        const int cur = active.load(std::memory_order_acquire);
        active.store(cur < 0 ? 0 : 1 - cur, std::memory_order_release);
        return HALO_OK;
    }
};

// LastAliveTime of the NAT and return-flow tables: one u32 per flow id, written by the lookups, in
// an array both generations share.
struct Stamps {
    uint32_t* d_stamps = nullptr;
    size_t cap = 0;
    uint32_t n = 0;  // ids the device copy knows (next_id at the last publish)

    // Drain `device` and read the stamps it wrote, for the table's merge_stamps. The caller holds
    // view_mu exclusively and has seen a published generation.
    int read_back(int device, std::vector<uint32_t>* back) const {
        if (drain_device(device) != HALO_OK) return HALO_E_HIP;
        back->resize(n);
        if (n && hipMemcpy(back->data(), d_stamps, n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
            return HALO_E_HIP;
        return HALO_OK;
    }
    // Every live flow's merged stamp (the fold ran under the same lock, so nothing newer exists on
    // the device); a new flow's slot thereby starts from its host stamp. Between begin_write and
    // publish: the array is shared, so growing it replaces it for both generations, which is safe
    // only because the device is drained and no lookup can take a view (view_mu) until the sync returns.
    int upload(const std::vector<uint32_t>& stamps) {
        const int rc = grow(d_stamps, cap, stamps.size() ? stamps.size() : 1);
        if (rc) return rc;
        if (!stamps.empty() &&
            hipMemcpy(d_stamps, stamps.data(), stamps.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
            return HALO_E_HIP;
        n = (uint32_t)stamps.size();
        return HALO_OK;
    }
};

// word(entry) of every route into `out`, by route id: ids are dense and never reused, so 0, 1, ...
// until HALO_E_RANGE.
template <typename T, typename F>
int route_words(const halo_route_table_t* routes, std::vector<T>* out, F word) {
    for (uint32_t id = 0;; ++id) {
        halo_route_entry_t e;
        const int rc = halo_route_get(routes, id, &e);
        if (rc == HALO_E_RANGE) return HALO_OK;
        if (rc) return rc;
        out->push_back(word(e));
    }
}

// The exclusive section of an entry point that writes a table's device copy (a sync, a fold, a
// publish after an expiry), t->sync_mu held, in the one safe order: run on the table's device; park
// the resident consumers, so that no ring kernel holds the write lock for its idle window and the
// drains and hipFree end; then view_mu exclusively: no lookup between its view and its launch.
struct Exclusive {
    DeviceScope scope;
    ParkResidents park;
    std::unique_lock<std::shared_mutex> lock;
    template <typename Gen>
    explicit Exclusive(Generations<Gen>& d) : scope(d.device), park(d.device), lock(d.view_mu) {}
};

// The lifecycle of a `Table` {sync_mu, std::atomic<void*> dev} whose device copy is a `Dev :
// Generations<Gen>`. A Dev supplies what differs between the tables: `int write(Table*)`, a
// generation from a compiled image and its publish(), Exclusive held; `void free_arrays()`, the
// hipFree of all it allocated, the device drained; and beside a `Stamps stamps` member (ARP has
// none and is never folded) `merge_stamps(Table&, const uint32_t*, uint32_t)`, the table's own.
template <typename Dev, typename Table>
Dev* dev_of(const Table* t) {
    return static_cast<Dev*>(t->dev.load(std::memory_order_acquire));
}

// Drain the device and merge the stamps it wrote into the host table. Exclusive held.
template <typename Dev, typename Table>
auto fold(Table* t, Dev* d) -> decltype(d->stamps, int()) {
    if (!d->published()) return HALO_OK;
    std::vector<uint32_t> back;
    const int rc = d->stamps.read_back(d->device, &back);
    if (!rc && !back.empty()) Dev::merge_stamps(*t, back.data(), (uint32_t)back.size());
    return rc;
}
inline int fold(...) { return HALO_OK; }  // a device copy without stamps

// DeviceOps::fold, ahead of an expiry; t->sync_mu held.
template <typename Dev, typename Table>
int fold_entry(Table* t) {
    Dev* d = dev_of<Dev>(t);
    if (!d) return HALO_OK;
    Exclusive x(*d);
    return fold(t, d);
}

// DeviceOps::publish, after an expiry removed entries; t->sync_mu held.
template <typename Dev, typename Table>
int publish_entry(Table* t) {
    Dev* d = dev_of<Dev>(t);
    if (!d || !d->published()) return HALO_OK;  // never synced: nothing to rebuild
    Exclusive x(*d);
    const int rc = fold(t, d);  // again: a lookup enqueued since the fold may have stamped a flow that stays
    return rc ? rc : d->write(t);
}

// The head of a sync, t->sync_mu held: one device per table, the device is there and usable, and
// the table's device object, which the first sync creates. The caller goes on with `Exclusive x(**out);`.
template <typename Dev, typename Table>
int sync_begin(Table* t, int device, Dev** out) {
    Dev* d = dev_of<Dev>(t);
    if (d && d->device >= 0 && d->device != device) return HALO_E_INVAL;  // one device per table
    int rc;
    if ((rc = device_present(device))) return rc;
    DeviceScope ds(device);
    if ((rc = check_device())) return rc;
    if (!d) {
        d = new (std::nothrow) Dev;
        if (!d) return HALO_E_NOMEM;
        d->device = device;
        t->dev.store(d, std::memory_order_release);
    }
    *out = d;
    return HALO_OK;
}

// DeviceOps::destroy: no call on the table is running or will start.
template <typename Dev, typename Table>
void destroy(Table* t) {
    Dev* d = dev_of<Dev>(t);
    if (!d) return;
    if (d->device >= 0) {
        DeviceScope ds(d->device);
        ParkResidents park(d->device);  // through the frees: hipFree waits for every kernel
        (void)drain_device(d->device);  // no lookup may still read the tables
        d->free_arrays();
    }
    delete d;
    t->dev.store(nullptr, std::memory_order_release);
}

}  // namespace halo
