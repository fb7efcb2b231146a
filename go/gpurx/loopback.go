package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"errors"
	"unsafe"
)

// The loopback step (halo_rx.h "loopback"): the producer side of a NetIf's LoChan. Ipv4RouteForward
// copies a packet addressed to the out NetIf's own address into that NetIf's LoChan and returns
// before the SNAT step (engine/ipv4_engine.go:193-201); TxIpv4 does the same for a locally built
// packet (:71-80). LoopbackMark is that test ahead of the NAT lookup, from records; LoopbackGather
// partitions the batch the encap has decided on into one L3 batch per out NetIf, in frame order,
// as a HALO_RX_L3_START parse takes it; LoopbackGatherHost is the same loop over host memory.

// LoNotWritten is the PktOff of a listed packet beyond its NetIf's written prefix.
const LoNotWritten = 0xFFFFFFFF

// LoopbackMark sets dMark[i] (one byte per record) to 1 where the encap of a batch NetIf inNetif
// received will say LOOPBACK, else 0: the skip array of the out NetIf's NAT lookup. Every pointer is
// a device pointer; dVia (optional) is PmflowLookupDevice's. The null stream.
func (t *ArpTable) LoopbackMark(dRecords unsafe.Pointer, n int, dRouteIds unsafe.Pointer, inNetif int, dVia,
	dMark unsafe.Pointer) error {
	return halo(C.halo_arp_loopback_mark_device(t.h, (*C.halo_rx_result_t)(dRecords), C.uint32_t(n), (*C.uint32_t)(dRouteIds),
		C.uint32_t(inNetif), (*C.halo_pmflow_via_t)(dVia), (*C.uint8_t)(dMark), nil))
}

// LoopbackWorkspace is the device workspace a gather over n frames and `netifs` NetIfs needs.
func LoopbackWorkspace(n, netifs int) uint64 {
	return uint64(C.halo_lo_gather_workspace(C.uint32_t(n), C.uint32_t(netifs)))
}

// LoopbackDevice describes the device buffers of a LoopbackGather: every pointer is a device
// pointer. Out is NetIfs * Region bytes, 16-byte aligned; Summary is NetIfs halo_egress_port_t;
// PktOff, PktLen (u16) and Index are NetIfs * IndexCap entries each; Skipped (optional) one u32,
// incremented. Tx: after the tx encap, packets are totalLen bytes.
type LoopbackDevice struct {
	NetIfs         int
	IndexCap       int
	Region         uint64
	Tx             bool
	Jumbo          bool
	Out            unsafe.Pointer
	Summary        unsafe.Pointer
	PktOff         unsafe.Pointer
	PktLen         unsafe.Pointer
	Index          unsafe.Pointer
	Skipped        unsafe.Pointer
	Workspace      unsafe.Pointer
	WorkspaceBytes uint64
}

func loConfig(netifs, indexCap int, region uint64, tx, jumbo bool) C.halo_lo_config_t {
	t, j := 0, 0
	if tx {
		t = 1
	}
	if jumbo {
		j = 1
	}
	return C.gpurx_lo_config(C.uint32_t(netifs), C.int(t), C.int(j), C.uint64_t(region), C.uint32_t(indexCap))
}

// LoopbackGather follows EncapDevice (or the tx encap, with Tx) on the null stream: dResults are
// its halo_arp_result_t.
func (d *LoopbackDevice) LoopbackGather(dFrames, dOffsets, dLens unsafe.Pointer, n int, dResults unsafe.Pointer) error {
	cfg := loConfig(d.NetIfs, d.IndexCap, d.Region, d.Tx, d.Jumbo)
	return halo(C.halo_lo_gather_device(&cfg, (*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens),
		C.uint32_t(n), (*C.halo_arp_result_t)(dResults), (*C.uint8_t)(d.Out), (*C.halo_egress_port_t)(d.Summary),
		(*C.uint32_t)(d.PktOff), (*C.uint16_t)(d.PktLen), (*C.uint32_t)(d.Index), (*C.uint32_t)(d.Skipped), d.Workspace,
		C.uint64_t(d.WorkspaceBytes), nil))
}

// Loopback owns the outputs of LoopbackGatherHost calls: NetIfs regions of Region bytes, the
// summaries and the per-packet arrays. One Loopback serves one caller at a time.
type Loopback struct {
	NetIfs   int
	Region   uint64
	IndexCap int
	Tx       bool
	Jumbo    bool
	Out      []byte
	Summary  []EgressPort
	PktOff   []uint32 // [netif * IndexCap + k]: the dword offset of the NetIf's k-th packet in its region
	PktLen   []uint16
	Index    []uint32 // the batch index of the NetIf's k-th packet
	Skipped  uint32   // selected frames that were not sendable, summed over the calls
}

// NewLoopback makes the buffers for `netifs` NetIfs with `region` bytes of packets each.
func NewLoopback(netifs int, region uint64, indexCap int) (*Loopback, error) {
	if netifs < 1 || netifs > int(C.HALO_ARP_MAX_NETIFS) {
		return nil, errors.New("gpurx: a loopback gather has 1..64 NetIfs")
	}
	cells := netifs*indexCap + 1
	return &Loopback{NetIfs: netifs, Region: region, IndexCap: indexCap, Out: make([]byte, uint64(netifs)*region+1),
		Summary: make([]EgressPort, netifs), PktOff: make([]uint32, cells), PktLen: make([]uint16, cells),
		Index: make([]uint32, cells)}, nil
}

// LoopbackGatherHost partitions a batch in host memory (frames at 4 * off[k], lens[k] bytes each)
// whose L2 step has been decided: res holds one ArpResult per frame.
func (l *Loopback) LoopbackGatherHost(buf []byte, off []uint32, lens []uint16, res []ArpResult) error {
	n := len(lens)
	if n == 0 {
		for p := range l.Summary {
			l.Summary[p] = EgressPort{}
		}
		return nil
	}
	if len(off) < n || len(res) < n || len(buf) == 0 {
		return errors.New("gpurx: fewer offsets or results than frames")
	}
	cfg := loConfig(l.NetIfs, l.IndexCap, l.Region, l.Tx, l.Jumbo)
	return halo(C.halo_lo_gather_host(&cfg, (*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint32_t)(unsafe.Pointer(&off[0])),
		(*C.uint16_t)(unsafe.Pointer(&lens[0])), C.uint32_t(n), (*C.halo_arp_result_t)(unsafe.Pointer(&res[0])),
		(*C.uint8_t)(unsafe.Pointer(&l.Out[0])), (*C.halo_egress_port_t)(unsafe.Pointer(&l.Summary[0])),
		(*C.uint32_t)(unsafe.Pointer(&l.PktOff[0])), (*C.uint16_t)(unsafe.Pointer(&l.PktLen[0])),
		(*C.uint32_t)(unsafe.Pointer(&l.Index[0])), (*C.uint32_t)(unsafe.Pointer(&l.Skipped))))
}

// Packets is NetIf p's written packets as (region, dword offsets, lengths): what a L3-start parse takes.
func (l *Loopback) Packets(p int) ([]byte, []uint32, []uint16) {
	k := int(l.Summary[p].FramesWritten)
	if k > l.IndexCap {
		k = l.IndexCap
	}
	lo := uint64(p) * l.Region
	return l.Out[lo : lo+l.Summary[p].BytesWritten], l.PktOff[p*l.IndexCap : p*l.IndexCap+k], l.PktLen[p*l.IndexCap : p*l.IndexCap+k]
}
