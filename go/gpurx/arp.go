package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"errors"
	"unsafe"
)

// The ARP neighbour cache (halo_rx.h "ARP neighbour cache"): a Router's ArpCacheTables as one table
// keyed by (netif, ip). The host table is the control plane (SetArpCache, GetArpCache, HandleArp,
// the clear and refresh ticks of engine/arp_engine.go); SyncDevice compiles it into HBM, and
// EncapDevice is the last step of Ipv4RouteForward over a device-resident batch: route id -> next
// hop -> MAC -> the Ethernet header, in place. Device lookups see the table as of the last
// SyncDevice; the engine loop re-syncs when Dirty. Device calls are asynchronous on the null stream.

// Verdicts of LookupDevice / EncapDevice (HALO_ARP_V_*).
const (
	ArpNone       = 0
	ArpNoRoute    = 1
	ArpRoutePanic = 2
	ArpLoopback   = 3
	ArpOwnIp      = 4
	ArpMiss       = 5
	ArpHit        = 6
	ArpVerdicts   = 7
)

// Verdict byte of HandleArp (HALO_ARP_H_*): a code in the low four bits and two flag bits.
const (
	ArpBadOp       = 0
	ArpSrcMismatch = 1
	ArpConflict    = 2
	ArpAccepted    = 3
	ArpCodeMask    = 0x0F
	ArpNotLearned  = 0x40
	ArpReplyBuilt  = 0x80
)

// GetArpCache's outcome (HALO_ARP_GET_*).
const (
	ArpGetAbsent = 0
	ArpGetFound  = 1
	ArpGetOwnIp  = 2
)

// ArpEntry mirrors halo_arp_entry_t (engine.ArpCache with the NetIf as an index).
type ArpEntry struct {
	Ip      uint32
	Mac     [6]byte
	NetIf   uint8
	Pad     uint8
	ExpTime uint32
}

// ArpMsg mirrors halo_arp_msg_t: one received ARP message as GatherDevice writes it.
type ArpMsg struct {
	Index  uint32
	NetIf  uint8
	Pad    uint8
	EthSrc [6]byte
	Arp    [28]byte
}

// ArpResult mirrors halo_arp_result_t.
type ArpResult struct {
	Verdict  uint8
	OutNetIf uint8 // 0xFF when there is none
	TxLen    uint16
	TargetIp uint32 // the address looked up: what an ArpMiss owes a SendArpReq for
}

// ArpTable owns a halo_arp_table_t.
type ArpTable struct {
	h      *C.halo_arp_table_t
	NetIfs int
}

// NewArpTable makes the table of a Router's NetIfs (NetIf 0 first); capacity is the most entries
// all NetIfs hold together.
func NewArpTable(netifs []*NetIfCfg, capacity int) (*ArpTable, error) {
	if len(netifs) < 1 || len(netifs) > int(C.HALO_ARP_MAX_NETIFS) {
		return nil, errors.New("gpurx: an ARP table has 1..64 NetIfs")
	}
	var cfg C.halo_arp_config_t
	cfg.n_netifs = C.uint32_t(len(netifs))
	for q, n := range netifs {
		c, err := n.c()
		if err != nil {
			return nil, err
		}
		cfg.netif[q] = c
	}
	cfg.capacity = C.uint32_t(capacity)
	t := &ArpTable{NetIfs: len(netifs)}
	if err := halo(C.halo_arp_table_create(&cfg, &t.h)); err != nil {
		return nil, err
	}
	return t, nil
}

// Close destroys the table and its device copy.
func (t *ArpTable) Close() error {
	if t.h == nil {
		return nil
	}
	err := halo(C.halo_arp_table_destroy(t.h))
	t.h = nil
	return err
}

// SetArpCache is NetIf.SetArpCache at Router.TimeNow = now.
func (t *ArpTable) SetArpCache(netif int, ip uint32, mac []byte, now uint32) error {
	if len(mac) != 6 {
		return errors.New("gpurx: a MAC has 6 bytes")
	}
	return halo(C.halo_arp_set(t.h, C.uint32_t(netif), C.uint32_t(ip), (*C.uint8_t)(unsafe.Pointer(&mac[0])), C.uint32_t(now)))
}

// GetArpCache is NetIf.GetArpCache on the host table: the outcome (ArpGet*) and, when found, the entry.
func (t *ArpTable) GetArpCache(netif int, ip uint32) (int, ArpEntry, error) {
	var e ArpEntry
	var found C.uint32_t
	err := halo(C.halo_arp_get(t.h, C.uint32_t(netif), C.uint32_t(ip), (*C.halo_arp_entry_t)(unsafe.Pointer(&e)), &found))
	return int(found), e, err
}

// HandleArp runs NetIf.HandleArp over msgs in order. verdicts[k] is message k's verdict byte; the
// reply frames (60 bytes each) are appended to replies, which is returned with the number of
// inserts and MAC changes.
func (t *ArpTable) HandleArp(msgs []ArpMsg, now uint32, verdicts []uint8, replies []byte) ([]byte, int, error) {
	n := len(msgs)
	if n == 0 {
		return replies, 0, nil
	}
	if len(verdicts) < n {
		return replies, 0, errors.New("gpurx: verdicts shorter than msgs")
	}
	buf := make([]byte, 60*n)
	var nr, nc C.uint32_t
	err := halo(C.halo_arp_handle_msgs(t.h, (*C.halo_arp_msg_t)(unsafe.Pointer(&msgs[0])), C.uint32_t(n), C.uint32_t(now),
		(*C.uint8_t)(unsafe.Pointer(&verdicts[0])), (*C.uint8_t)(unsafe.Pointer(&buf[0])), &nr, &nc))
	if err != nil {
		return replies, 0, err
	}
	return append(replies, buf[:60*int(nr)]...), int(nc), nil
}

// SendArpReq builds the frame NetIf.SendArpReq(target) transmits; with the NetIf's own address it
// is SendFreeArp's.
func (t *ArpTable) SendArpReq(netif int, target uint32) ([]byte, error) {
	out := make([]byte, 60)
	err := halo(C.halo_arp_build_request(t.h, C.uint32_t(netif), C.uint32_t(target), (*C.uint8_t)(unsafe.Pointer(&out[0]))))
	return out, err
}

// ArpTableClear is one clear tick; it returns the number of entries removed. A device copy that
// lost entries is republished before it returns.
func (t *ArpTable) ArpTableClear(now uint32) (int, error) {
	var n C.uint32_t
	err := halo(C.halo_arp_expire(t.h, C.uint32_t(now), &n))
	return int(n), err
}

// ArpTableRefresh is one refresh tick: the (netif, ip) pairs to SendArpReq for.
func (t *ArpTable) ArpTableRefresh(now uint32) ([]uint8, []uint32, error) {
	var n C.uint32_t
	if err := halo(C.halo_arp_refresh_list(t.h, C.uint32_t(now), nil, nil, 0, &n)); err != nil {
		return nil, nil, err
	}
	nifs, ips := make([]uint8, int(n)+1), make([]uint32, int(n)+1)
	if err := halo(C.halo_arp_refresh_list(t.h, C.uint32_t(now), (*C.uint8_t)(unsafe.Pointer(&nifs[0])),
		(*C.uint32_t)(unsafe.Pointer(&ips[0])), C.uint32_t(len(ips)-1), &n)); err != nil {
		return nil, nil, err
	}
	k := len(ips) - 1
	if int(n) < k {
		k = int(n)
	}
	return nifs[:k], ips[:k], nil
}

// ListArp copies the cache out (order unspecified).
func (t *ArpTable) ListArp() ([]ArpEntry, error) {
	var n C.uint32_t
	if err := halo(C.halo_arp_list(t.h, nil, 0, &n)); err != nil {
		return nil, err
	}
	out := make([]ArpEntry, int(n)+1)
	if err := halo(C.halo_arp_list(t.h, (*C.halo_arp_entry_t)(unsafe.Pointer(&out[0])), C.uint32_t(len(out)-1), &n)); err != nil {
		return nil, err
	}
	if int(n) < len(out)-1 {
		return out[:n], nil
	}
	return out[:len(out)-1], nil
}

// Dirty reports whether the host table differs from the published device copy.
func (t *ArpTable) Dirty() bool { return C.halo_arp_dirty(t.h) == 1 }

// SyncDevice compiles and publishes the device copy; routes (optional) adds the route-entry array
// EncapDevice needs.
func (t *ArpTable) SyncDevice(routes *C.halo_route_table_t, device int) error {
	return halo(C.halo_arp_sync_device(t.h, routes, C.int(device)))
}

// LookupDevice is GetArpCache for n device-resident addresses on one NetIf: dMac8 gets 8 bytes per
// entry, dVerdict one; *dMissCount is incremented.
func (t *ArpTable) LookupDevice(netif int, dIps unsafe.Pointer, n int, dMac8, dVerdict, dMissCount unsafe.Pointer) error {
	return halo(C.halo_arp_lookup_device(t.h, (*C.uint32_t)(dIps), nil, C.uint32_t(netif), C.uint32_t(n), (*C.uint8_t)(dMac8),
		(*C.uint8_t)(dVerdict), (*C.uint32_t)(dMissCount), nil))
}

// EncapDevice is the forward path's L2 step for the frames NetIf inNetif received, after Rewrite
// in stream order: every pointer is a device pointer; dSelect and dCounts are optional.
func (t *ArpTable) EncapDevice(dFrames, dOffsets, dLens unsafe.Pointer, n int, dRouteIds unsafe.Pointer, inNetif int, dSelect,
	dResults, dCounts, dMissCount unsafe.Pointer) error {
	return halo(C.halo_arp_encap_device(t.h, (*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens), C.uint32_t(n),
		(*C.uint32_t)(dRouteIds), C.uint32_t(inNetif), (*C.uint8_t)(dSelect), (*C.halo_arp_result_t)(dResults),
		(*C.uint32_t)(dCounts), (*C.uint32_t)(dMissCount), nil))
}

// ArpGatherWorkspace is the scratch GatherDevice needs for n frames, in bytes.
func ArpGatherWorkspace(n int) uint64 { return uint64(C.halo_arp_gather_workspace(C.uint32_t(n))) }

// ArpGatherDevice writes the ARP messages of a parsed device-resident batch to dMsgs in frame
// order (at most cap of them) and their number to *dCount.
func ArpGatherDevice(dFrames, dOffsets, dLens, dRecords unsafe.Pointer, n, netif int, dMsgs unsafe.Pointer, cap int, dCount,
	dWorkspace unsafe.Pointer, workspaceBytes uint64) error {
	return halo(C.halo_arp_gather_device((*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens),
		(*C.halo_rx_result_t)(dRecords), C.uint32_t(n), C.uint32_t(netif), (*C.halo_arp_msg_t)(dMsgs), C.uint32_t(cap),
		(*C.uint32_t)(dCount), dWorkspace, C.uint64_t(workspaceBytes), nil))
}
