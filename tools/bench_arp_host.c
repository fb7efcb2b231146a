/* bench_arp_host.c — the host side of tools/bench_arp.py: filling a table with many neighbours,
 * and the per-record host loop the device L2 step replaces (halo_route_get + halo_arp_get for
 * every forwarded record, on one core). Built by bench_arp.py with gcc against libhalo_rx.so. */
#include <stdint.h>

#include "halo_rx.h"

/* neighbours base_ip .. base_ip + count - 1 on `netif`, MAC 02:4e:<ip> */
int bench_arp_fill(halo_arp_table_t* t, uint32_t netif, uint32_t base_ip, uint32_t count, uint32_t now) {
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t ip = base_ip + k;
        const uint8_t mac[6] = {0x02, 0x4E, (uint8_t)(ip >> 24), (uint8_t)(ip >> 16), (uint8_t)(ip >> 8), (uint8_t)ip};
        const int rc = halo_arp_set(t, netif, ip, mac, now);
        if (rc) return rc;
    }
    return HALO_OK;
}

/* For each record: route id -> (next hop, out NetIf) -> MAC. Returns the number found; the MACs'
 * bytes are folded into *sink so that the loads are not dead. */
uint32_t bench_arp_host_loop(const halo_arp_table_t* t, const halo_route_table_t* routes, const uint32_t* route_ids,
                             const uint32_t* dst_ips, uint32_t n, uint32_t* sink) {
    uint32_t hits = 0, acc = 0;
    for (uint32_t i = 0; i < n; ++i) {
        halo_route_entry_t r;
        if (halo_route_get(routes, route_ids[i], &r) != HALO_OK) continue;
        halo_arp_entry_t e;
        uint32_t found = 0;
        if (halo_arp_get(t, r.netif, r.next_hop ? r.next_hop : dst_ips[i], &e, &found) != HALO_OK) continue;
        if (found == HALO_ARP_GET_FOUND) {
            ++hits;
            acc += e.mac[5];
        }
    }
    *sink = acc;
    return hits;
}
