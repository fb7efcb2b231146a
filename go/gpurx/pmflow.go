package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"errors"
	"unsafe"
)

// Port-mapping return flows (halo_rx.h "port-mapping return flows"): the Router's
// NatPortMappingFlowTable, which sends the replies of a port-forwarded connection back out of the
// WAN NetIf it came in on. The host table is the control plane (Record is the Get / MallocType / Set
// of engine/ipv4_engine.go:238-266 over a batch, Get the lookup of :164-179, TableClear one
// NatPortMappingFlowClear tick); SyncDevice compiles it into HBM. LookupDevice is the LAN-side half
// over a device-resident batch, RecordDevice lists the frames of a WAN-side batch that record a
// flow, EncapViaDevice is EncapDevice with the out-interface override and ArpDropDevice takes the
// frames Record dropped out of the egress. NetIfs are indices, as in the ARP table. Device calls are
// asynchronous on the null stream.

// Verdicts of LookupDevice (HALO_PMFLOW_V_*).
const (
	PmflowNone     = 0
	PmflowMiss     = 1
	PmflowHit      = 2
	PmflowOverride = 3
	PmflowVerdicts = 4
)

// PmflowItem mirrors halo_pmflow_item_t: one frame to record, as RecordDevice writes it.
type PmflowItem struct {
	Index      uint32
	RemoteIp   uint32
	LanIp      uint32
	RemotePort uint16
	LanPort    uint16
	WanPort    uint16
	Proto      uint8
	Pad        uint8
}

// PmflowEntry mirrors halo_pmflow_entry_t: a NatPortMappingFlow with its key.
type PmflowEntry struct {
	RemoteIp   uint32
	LanIp      uint32
	LastAlive  uint32
	Id         uint32
	RemotePort uint16
	LanPort    uint16
	WanPort    uint16
	Proto      uint8
	WanNetIf   uint8
}

// PmflowVia mirrors halo_pmflow_via_t: what LookupDevice hands to EncapViaDevice.
type PmflowVia struct {
	Verdict  uint8
	WanNetIf uint8 // 0xFF when there is none
	WanPort  uint16
	NextHop  uint32
}

// PmflowTable owns a halo_pmflow_table_t.
type PmflowTable struct {
	h      *C.halo_pmflow_table_t
	NetIfs int
}

// NewPmflowTable makes the table of a Router's NetIfs (NetIf 0 first); gateways[q] is
// IpAddrToU(NetIf.Gateway) of NetIf q, 0 for nil; capacity is the StaticAllocator's room.
func NewPmflowTable(netifs []*NetIfCfg, gateways []uint32, capacity int) (*PmflowTable, error) {
	if len(netifs) < 1 || len(netifs) > int(C.HALO_ARP_MAX_NETIFS) || len(gateways) != len(netifs) {
		return nil, errors.New("gpurx: a return-flow table has 1..64 NetIfs and a gateway for each")
	}
	var cfg C.halo_pmflow_config_t
	cfg.n_netifs = C.uint32_t(len(netifs))
	for q, n := range netifs {
		c, err := n.c()
		if err != nil {
			return nil, err
		}
		cfg.netif[q] = c
		cfg.gateway[q] = C.uint32_t(gateways[q])
	}
	cfg.capacity = C.uint32_t(capacity)
	t := &PmflowTable{NetIfs: len(netifs)}
	if err := halo(C.halo_pmflow_table_create(&cfg, &t.h)); err != nil {
		return nil, err
	}
	return t, nil
}

// Close destroys the table and its device copy.
func (t *PmflowTable) Close() error {
	if t.h == nil {
		return nil
	}
	err := halo(C.halo_pmflow_table_destroy(t.h))
	t.h = nil
	return err
}

// Record applies items in order for frames NetIf inNetif received, at Router.TimeNow = now.
// dropped[k] = 1 where the table was full: that frame must not be sent. It returns the inserts.
func (t *PmflowTable) Record(inNetif int, items []PmflowItem, now uint32, dropped []uint8) (int, error) {
	k := len(items)
	if k == 0 {
		return 0, nil
	}
	if len(dropped) < k {
		return 0, errors.New("gpurx: dropped shorter than items")
	}
	var added C.uint32_t
	err := halo(C.halo_pmflow_record(t.h, C.uint32_t(inNetif), (*C.halo_pmflow_item_t)(unsafe.Pointer(&items[0])), C.uint32_t(k),
		C.uint32_t(now), (*C.uint8_t)(unsafe.Pointer(&dropped[0])), &added))
	return int(added), err
}

// Get is the host lookup; with stamp the flow's LastAliveTime becomes now, as the forward path does.
func (t *PmflowTable) Get(remoteIp uint32, remotePort uint16, lanIp uint32, lanPort uint16, proto uint8, now uint32,
	stamp bool) (PmflowEntry, bool, error) {
	var e PmflowEntry
	var found C.uint32_t
	var at *C.uint32_t
	cnow := C.uint32_t(now)
	if stamp {
		at = &cnow
	}
	err := halo(C.halo_pmflow_get(t.h, C.uint32_t(remoteIp), C.uint16_t(remotePort), C.uint32_t(lanIp), C.uint16_t(lanPort),
		C.uint8_t(proto), at, (*C.halo_pmflow_entry_t)(unsafe.Pointer(&e)), &found))
	return e, found == 1, err
}

// TableClear is one NatPortMappingFlowClear tick; it returns the number of flows removed.
// Synchronise the streams of earlier lookups first.
func (t *PmflowTable) TableClear(now uint32) (int, error) {
	var n C.uint32_t
	err := halo(C.halo_pmflow_expire(t.h, C.uint32_t(now), &n))
	return int(n), err
}

// List copies the flows out in ascending id.
func (t *PmflowTable) List() ([]PmflowEntry, error) {
	var n C.uint32_t
	if err := halo(C.halo_pmflow_list(t.h, nil, 0, &n)); err != nil {
		return nil, err
	}
	out := make([]PmflowEntry, int(n)+1)
	if err := halo(C.halo_pmflow_list(t.h, (*C.halo_pmflow_entry_t)(unsafe.Pointer(&out[0])), C.uint32_t(len(out)-1), &n)); err != nil {
		return nil, err
	}
	if int(n) < len(out)-1 {
		return out[:n], nil
	}
	return out[:len(out)-1], nil
}

// Dirty reports whether the host table differs from the published device copy.
func (t *PmflowTable) Dirty() bool { return C.halo_pmflow_dirty(t.h) == 1 }

// SyncDevice compiles and publishes the device copy; routes adds the NetIf of every route id,
// which LookupDevice needs.
func (t *PmflowTable) SyncDevice(routes *C.halo_route_table_t, device int) error {
	return halo(C.halo_pmflow_sync_device(t.h, routes, C.int(device)))
}

// LookupDevice is the LAN-side half for n device-resident records with their route ids: dOps is
// updated, dVia (8 bytes per record) and dHit (1 byte) are written; dSelect and dCounts are optional.
func (t *PmflowTable) LookupDevice(dRecords unsafe.Pointer, n int, now uint32, dRouteIds, dSelect, dOps, dVia, dHit,
	dCounts unsafe.Pointer) error {
	return halo(C.halo_pmflow_lookup_device(t.h, (*C.halo_rx_result_t)(dRecords), C.uint32_t(n), C.uint32_t(now),
		(*C.uint32_t)(dRouteIds), (*C.uint8_t)(dSelect), (*C.halo_tx_op_t)(dOps), (*C.halo_pmflow_via_t)(dVia), (*C.uint8_t)(dHit),
		(*C.uint32_t)(dCounts), nil))
}

// PmflowRecordWorkspace is the scratch RecordDevice needs for n frames, in bytes.
func PmflowRecordWorkspace(n int) uint64 { return uint64(C.halo_pmflow_record_workspace(C.uint32_t(n))) }

// RecordDevice lists the frames NetIf inNetif received that record a flow, after EncapDevice in
// stream order: at most cap items to dItems in frame order, their number to *dCount.
func (t *PmflowTable) RecordDevice(inNetif int, dRecords, dWanVerdict, dOps, dArpResults unsafe.Pointer, n int, now uint32,
	dItems unsafe.Pointer, cap int, dCount, dWorkspace unsafe.Pointer, workspaceBytes uint64) error {
	return halo(C.halo_pmflow_record_device(t.h, C.uint32_t(inNetif), (*C.halo_rx_result_t)(dRecords), (*C.uint8_t)(dWanVerdict),
		(*C.halo_tx_op_t)(dOps), (*C.halo_arp_result_t)(dArpResults), C.uint32_t(n), C.uint32_t(now), (*C.halo_pmflow_item_t)(dItems),
		C.uint32_t(cap), (*C.uint32_t)(dCount), dWorkspace, C.uint64_t(workspaceBytes), nil))
}

// ArpDropDevice turns the results of the k frames listed in dIndex into ArpNone, so that the egress
// leaves them out.
func ArpDropDevice(dResults, dIndex unsafe.Pointer, k int) error {
	return halo(C.halo_arp_drop_device((*C.halo_arp_result_t)(dResults), (*C.uint32_t)(dIndex), C.uint32_t(k), nil))
}

// EncapViaDevice is EncapDevice with the return-flow override: where dVia says PmflowOverride the
// out NetIf and next hop come from it. A nil dVia gives EncapDevice's results.
func (t *ArpTable) EncapViaDevice(dFrames, dOffsets, dLens unsafe.Pointer, n int, dRouteIds unsafe.Pointer, inNetif int, dSelect,
	dVia, dResults, dCounts, dMissCount unsafe.Pointer) error {
	return halo(C.halo_arp_encap_via_device(t.h, (*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens), C.uint32_t(n),
		(*C.uint32_t)(dRouteIds), C.uint32_t(inNetif), (*C.uint8_t)(dSelect), (*C.halo_pmflow_via_t)(dVia),
		(*C.halo_arp_result_t)(dResults), (*C.uint32_t)(dCounts), (*C.uint32_t)(dMissCount), nil))
}
