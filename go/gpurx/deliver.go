package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"encoding/binary"
	"errors"
	"unsafe"
)

// Local delivery (halo_rx.h "local delivery"): what RxUdp / RxTcp hand to the registered service
// handlers (engine/udp_engine.go:10-21, engine/tcp_engine.go:10-26) and RxUdpBroadcast to RxDhcp
// (engine/udp_engine.go:35-44), for a parsed batch at once: one stream of records — a 24-byte
// header, the payload, zeros to the next 4-byte boundary — in frame order, the order in which the
// reference calls the handlers.

// Kinds of delivery record (HALO_DELIVER_*).
const (
	DeliverUdp   = 0
	DeliverTcp   = 1
	DeliverDhcp  = 2
	DeliverKinds = 3
)

// DeliverNotWritten is the offset of an index entry beyond the written prefix.
const DeliverNotWritten = 0xFFFFFFFF

// DeliverHdr mirrors halo_deliver_hdr_t.
type DeliverHdr struct {
	Frame      uint32
	Kind       uint8
	TcpFlags   uint8
	PayloadLen uint16
	RemoteIp   uint32
	RemotePort uint16
	LocalPort  uint16
	Seq        uint32
	Ack        uint32
}

// DeliverSummary mirrors halo_deliver_summary_t.
type DeliverSummary struct {
	Records        uint32 // frames delivered, also beyond the region
	RecordsWritten uint32 // the prefix of them that fits the region wholly
	Bytes          uint64
	BytesWritten   uint64
	KindCounts     [DeliverKinds]uint32
	Skipped        uint32 // selected, but the record's payload overruns the frame
}

// DeliverIndex mirrors halo_deliver_index_t.
type DeliverIndex struct {
	Frame  uint32
	Offset uint32
}

// PortMap is a served-port bitmap (UdpServiceMap's or TcpServiceMap's keys).
type PortMap = TcpPortMap

// Delivery owns the outputs of host calls: Region bytes of stream, the summary and the index.
type Delivery struct {
	Region   uint64
	IndexCap int
	L3Start  bool // the records are LoChan packets (HALO_RX_L3_START)
	Dhcp     bool // deliver broadcast UDP to ports 67 / 68 (HALO_DELIVER_DHCP)
	Out      []byte
	Summary  DeliverSummary
	Index    []DeliverIndex
}

// NewDelivery makes the buffers for `region` bytes of stream and indexCap index entries.
func NewDelivery(region uint64, indexCap int) *Delivery {
	return &Delivery{Region: region, IndexCap: indexCap, Out: make([]byte, region+1), Index: make([]DeliverIndex, indexCap+1)}
}

func deliverCfg(region uint64, indexCap int, l3, dhcp bool) C.halo_deliver_config_t {
	var cfg C.halo_deliver_config_t
	if l3 {
		cfg.flags |= C.HALO_RX_L3_START
	}
	if dhcp {
		cfg.flags |= C.HALO_DELIVER_DHCP
	}
	cfg.index_cap = C.uint32_t(indexCap)
	cfg.region_bytes = C.uint64_t(region)
	return cfg
}

func portsPtr(m *PortMap) *C.uint32_t {
	if m == nil {
		return nil
	}
	return (*C.uint32_t)(unsafe.Pointer(&m[0]))
}

// Deliver runs the sequential loop over a parsed host batch: the bytes, offsets (dwords), lengths
// and 32-byte records of n frames that NetIf nif received. A nil map means no service of that
// protocol.
func (d *Delivery) Deliver(buf []byte, offsets []uint32, lens []uint16, records []Result, nif *NetIfCfg, udp, tcp *PortMap) error {
	n := len(records)
	if len(offsets) < n || len(lens) < n {
		return errors.New("gpurx: fewer offsets or lengths than records")
	}
	cn, err := nif.c()
	if err != nil {
		return err
	}
	if n == 0 || len(buf) == 0 {
		d.Summary = DeliverSummary{}
		return nil
	}
	cfg := deliverCfg(d.Region, d.IndexCap, d.L3Start, d.Dhcp)
	return halo(C.halo_rx_deliver_host(&cfg, (*C.uint8_t)(unsafe.Pointer(&buf[0])), (*C.uint32_t)(unsafe.Pointer(&offsets[0])),
		(*C.uint16_t)(unsafe.Pointer(&lens[0])), (*C.halo_rx_result_t)(unsafe.Pointer(&records[0])), C.uint32_t(n), &cn,
		portsPtr(udp), portsPtr(tcp), (*C.uint8_t)(unsafe.Pointer(&d.Out[0])),
		(*C.halo_deliver_summary_t)(unsafe.Pointer(&d.Summary)), (*C.halo_deliver_index_t)(unsafe.Pointer(&d.Index[0]))))
}

// Stream is the written records.
func (d *Delivery) Stream() []byte { return d.Out[:d.Summary.BytesWritten] }

// Entries is the first min(Records, IndexCap) index entries.
func (d *Delivery) Entries() []DeliverIndex {
	k := int(d.Summary.Records)
	if k > d.IndexCap {
		k = d.IndexCap
	}
	return d.Index[:k]
}

// Each calls fn with the header and payload of every written record, in stream order; the payload
// aliases Out.
func (d *Delivery) Each(fn func(h DeliverHdr, payload []byte)) {
	s := d.Stream()
	for at := 0; at+24 <= len(s); {
		h := DeliverHdr{Frame: binary.LittleEndian.Uint32(s[at:]), Kind: s[at+4], TcpFlags: s[at+5],
			PayloadLen: binary.LittleEndian.Uint16(s[at+6:]), RemoteIp: binary.LittleEndian.Uint32(s[at+8:]),
			RemotePort: binary.LittleEndian.Uint16(s[at+12:]), LocalPort: binary.LittleEndian.Uint16(s[at+14:]),
			Seq: binary.LittleEndian.Uint32(s[at+16:]), Ack: binary.LittleEndian.Uint32(s[at+20:])}
		fn(h, s[at+24:at+24+int(h.PayloadLen)])
		at += 24 + (int(h.PayloadLen)+3)&^3
	}
}

// DeliverWorkspace is the device workspace a device call over n frames needs, in bytes.
func DeliverWorkspace(n int) uint64 { return uint64(C.halo_rx_deliver_workspace(C.uint32_t(n))) }

// DeliverDevice describes the device buffers of a device call: every pointer is a device pointer.
// Out is Region bytes (a multiple of 16, at most 2^32 - 16), 16-byte aligned; Summary one
// halo_deliver_summary_t; Index (optional) IndexCap halo_deliver_index_t; UdpPorts and TcpPorts
// (optional) 2,048 u32 each.
type DeliverDevice struct {
	Region             uint64
	IndexCap           int
	L3Start, Dhcp      bool
	UdpPorts, TcpPorts unsafe.Pointer
	Out, Summary       unsafe.Pointer
	Index              unsafe.Pointer
	Workspace          unsafe.Pointer
	WorkspaceBytes     uint64
}

// Run issues the launches on the null stream for a parsed device-resident batch.
func (d *DeliverDevice) Run(dFrames, dOffsets, dLens, dRecords unsafe.Pointer, n int, nif *NetIfCfg) error {
	cn, err := nif.c()
	if err != nil {
		return err
	}
	cfg := deliverCfg(d.Region, d.IndexCap, d.L3Start, d.Dhcp)
	return halo(C.halo_rx_deliver_device(&cfg, (*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens),
		(*C.halo_rx_result_t)(dRecords), C.uint32_t(n), &cn, (*C.uint32_t)(d.UdpPorts), (*C.uint32_t)(d.TcpPorts),
		(*C.uint8_t)(d.Out), (*C.halo_deliver_summary_t)(d.Summary), (*C.halo_deliver_index_t)(d.Index), d.Workspace,
		C.uint64_t(d.WorkspaceBytes), nil))
}
