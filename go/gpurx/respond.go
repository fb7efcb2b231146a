package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"errors"
	"unsafe"
)

// The local responders (halo_rx.h "local responders"): the answers the reference gives from inside
// its receive loop — RxIcmp's echo reply (engine/icmp_engine.go:12-23), Ipv4RouteForward's
// time-exceeded message (engine/ipv4_engine.go:133-142) and RxTcp's handshake replies
// (engine/tcp_engine.go:20-24) — for a parsed batch at once: one dense list of build descriptors
// in frame order, which the batched Build* call consumes with the rx batch itself as payload.
// ArpEncapTxDevice is TxIpv4's route / ARP step (engine/ipv4_engine.go:50-99) on the built frames.

// Kinds of reply (HALO_RESPOND_*).
const (
	RespondEcho      = 0
	RespondTtl       = 1
	RespondTcpSyn    = 2
	RespondTcpSynAck = 3
	RespondKinds     = 4
)

// BuildDesc mirrors halo_tx_build_desc_t (40 bytes).
type BuildDesc struct {
	PayloadOff uint64
	PayloadLen uint16
	Proto      uint8
	Aux        uint8
	SrcPort    uint16
	DstPort    uint16
	SrcIp      uint32
	DstIp      uint32
	Seq        uint32
	Ack        uint32
	DstMac     [6]byte
	Mode       uint8
	Pad        uint8
}

// RespondSrc mirrors halo_respond_src_t: which frame a reply answers, and its kind.
type RespondSrc struct {
	Index uint32
	Kind  uint8
	Pad   [3]uint8
}

// TcpPortMap is the served-port bitmap (TcpServiceMap's keys): 65,536 bits as 2,048 words.
type TcpPortMap [2048]uint32

// Serve marks a port as served.
func (m *TcpPortMap) Serve(port uint16) { m[port>>5] |= 1 << (port & 31) }

// RespondInputs are the optional per-frame inputs; an absent one means its rows never fire.
// Ops and FixupResult come together (the fixup call's operands and result bytes).
type RespondInputs struct {
	NatVerdict  []uint8 // halo_nat_lookup_wan's verdict bytes
	Ops         unsafe.Pointer
	FixupResult []uint8
	TcpPorts    *TcpPortMap
	L3Start     bool // the records are LoChan packets (HALO_RX_L3_START)
}

// Replies owns the outputs of host calls: at most Cap replies are written, Count is the total.
type Replies struct {
	Cap        int
	Desc       []BuildDesc
	Src        []RespondSrc
	DstIp      []uint32
	Count      uint32
	KindCounts [RespondKinds]uint32 // summed over the calls
	Actions    []uint8              // halo_rx_dispatch's action of every frame of the last call
}

// NewReplies makes the buffers for up to cap replies per call.
func NewReplies(cap int) *Replies {
	return &Replies{Cap: cap, Desc: make([]BuildDesc, cap+1), Src: make([]RespondSrc, cap+1), DstIp: make([]uint32, cap+1)}
}

func bytesPtr(b []uint8) *C.uint8_t {
	if len(b) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&b[0]))
}

// Respond runs the sequential loop over a parsed host batch: offsets (dwords), lengths and the
// 32-byte records of n frames that NetIf nif received.
func (r *Replies) Respond(offsets []uint32, lens []uint16, records []Result, nif *NetIfCfg, in *RespondInputs) error {
	n := len(records)
	if len(offsets) < n || len(lens) < n {
		return errors.New("gpurx: fewer offsets or lengths than records")
	}
	cn, err := nif.c()
	if err != nil {
		return err
	}
	if cap(r.Actions) < n+1 {
		r.Actions = make([]uint8, n+1)
	}
	r.Actions = r.Actions[:n+1]
	if n == 0 {
		r.Count = 0
		return nil
	}
	var flags C.uint32_t
	var ports *C.uint32_t
	if in.L3Start {
		flags = C.HALO_RX_L3_START
	}
	if in.TcpPorts != nil {
		ports = (*C.uint32_t)(unsafe.Pointer(&in.TcpPorts[0]))
	}
	return halo(C.halo_tx_respond_host((*C.uint32_t)(unsafe.Pointer(&offsets[0])), (*C.uint16_t)(unsafe.Pointer(&lens[0])),
		(*C.halo_rx_result_t)(unsafe.Pointer(&records[0])), C.uint32_t(n), flags, &cn, bytesPtr(in.NatVerdict),
		(*C.halo_tx_op_t)(in.Ops), bytesPtr(in.FixupResult), ports, (*C.halo_tx_build_desc_t)(unsafe.Pointer(&r.Desc[0])),
		(*C.halo_respond_src_t)(unsafe.Pointer(&r.Src[0])), (*C.uint32_t)(unsafe.Pointer(&r.DstIp[0])), C.uint32_t(r.Cap),
		(*C.uint32_t)(unsafe.Pointer(&r.Count)), (*C.uint32_t)(unsafe.Pointer(&r.KindCounts[0])),
		(*C.uint8_t)(unsafe.Pointer(&r.Actions[0]))))
}

// Written is the number of replies the last call wrote: min(Count, Cap).
func (r *Replies) Written() int {
	if int(r.Count) < r.Cap {
		return int(r.Count)
	}
	return r.Cap
}

// RespondWorkspace is the device workspace a device call over n frames needs, in bytes.
func RespondWorkspace(n int) uint64 { return uint64(C.halo_tx_respond_workspace(C.uint32_t(n))) }

// RespondDevice describes the device buffers of a device call: every pointer is a device pointer.
// NatVerdict, Ops with FixupResult, TcpPorts, DstIp, KindCounts and Actions are optional.
type RespondDevice struct {
	NatVerdict, Ops, FixupResult, TcpPorts unsafe.Pointer
	Desc, Src, DstIp                       unsafe.Pointer
	Cap                                    int
	Count, KindCounts, Actions             unsafe.Pointer
	Workspace                              unsafe.Pointer
	WorkspaceBytes                         uint64
	L3Start                                bool
}

// Run issues the three launches on the null stream for a parsed device-resident batch.
func (d *RespondDevice) Run(dOffsets, dLens, dRecords unsafe.Pointer, n int, nif *NetIfCfg) error {
	cn, err := nif.c()
	if err != nil {
		return err
	}
	var flags C.uint32_t
	if d.L3Start {
		flags = C.HALO_RX_L3_START
	}
	return halo(C.halo_tx_respond_device((*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens), (*C.halo_rx_result_t)(dRecords),
		C.uint32_t(n), flags, &cn, (*C.uint8_t)(d.NatVerdict), (*C.halo_tx_op_t)(d.Ops), (*C.uint8_t)(d.FixupResult),
		(*C.uint32_t)(d.TcpPorts), (*C.halo_tx_build_desc_t)(d.Desc), (*C.halo_respond_src_t)(d.Src), (*C.uint32_t)(d.DstIp),
		C.uint32_t(d.Cap), (*C.uint32_t)(d.Count), (*C.uint32_t)(d.KindCounts), (*C.uint8_t)(d.Actions), d.Workspace,
		C.uint64_t(d.WorkspaceBytes), nil))
}

// EncapTxDevice is TxIpv4's step for frames NetIf selfNetif originated (the built replies): a
// x.x.x.255 destination leaves selfNetif to the broadcast MAC without a route, a destination that
// is the out NetIf's own address is ArpLoopback whatever NatEnable says; the rest is EncapDevice's.
func (t *ArpTable) EncapTxDevice(dFrames, dOffsets, dLens unsafe.Pointer, n int, dRouteIds unsafe.Pointer, selfNetif int,
	dSelect, dResults, dCounts, dMissCount unsafe.Pointer) error {
	return halo(C.halo_arp_encap_tx_device(t.h, (*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens),
		C.uint32_t(n), (*C.uint32_t)(dRouteIds), C.uint32_t(selfNetif), (*C.uint8_t)(dSelect),
		(*C.halo_arp_result_t)(dResults), (*C.uint32_t)(dCounts), (*C.uint32_t)(dMissCount), nil))
}
