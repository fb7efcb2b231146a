// dhcp_table.h — the DHCP server object (include/halo_rx.h, "DHCP", THE SERVER OBJECT): the lease
// table and RxDhcp's state machine (engine/dhcp_engine.go:216-434) over decoded message records.
// Host C++17, no HIP: dhcp_table.cc compiles alone with g++ (tools/fuzz_dhcp.cc drives it under
// ASan/UBSan) and into libhalo_rx.so.
//
// Reference state: per NetIf a DhcpLeaseTable, IpAddrHash -> DhcpLease {IpAddr, MacAddr, ExpTime,
// HostName}, every lease allocated from the Router's StaticAllocator (`capacity` stands in for its
// running out), and the client's DhcpClientTransactionId. The table here is an ordered map keyed by
// the address: DISCOVER's scan asks only "is networkU + ii leased", which any map answers, and
// ListDhcp comes out in ascending address order.
#pragma once
#include <stdint.h>

#include <map>

#include "../../include/halo_rx.h"

struct halo_dhcp_server {
    halo_dhcp_config_t cfg;
    std::map<uint32_t, halo_dhcp_lease_t> leases;
    uint8_t client_xid[4];
    bool client_xid_set;  // DhcpClientTransactionId is nil until DhcpDiscover: no xid equals it
};
