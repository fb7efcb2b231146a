package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"errors"
	"unsafe"
)

// KCP ingest (halo_rx.h "KCP ingest"): the stateless part of the KCP receive path — what
// Listener.packetInput (protocol/kcp/session.go:866-921) and KCP.Input's loop (kcp.go:613-709) do
// to a datagram's bytes before any session state is touched — over the UDP payloads of one served
// port in a delivery stream: ENet control packets told from KCP datagrams, the segment walk with
// its conv, length and cmd checks, and the byte check of every PUSH segment. A session then runs
// Input's state machine from the descriptors; one difference: a client-side session that knows its
// own conv compares it with the record's Conv0 itself.

// Byte-check modes (kcp.go:34-41).
const (
	KcpCheckDisabled = -1
	KcpCheckZero     = 0
	KcpCheckCRC32    = 1
	KcpCheckXXH3     = 2
)

// Datagram kinds, ENet conn types (in ParseEnet's order) and segment check bytes.
const (
	KcpDgramKcp  = 0
	KcpDgramEnet = 1

	KcpEnetSyn  = 0
	KcpEnetEst  = 1
	KcpEnetFin  = 2
	KcpEnetPing = 3

	KcpSegCheckNA     = 0
	KcpSegCheckPassed = 1
	KcpSegCheckFailed = 2
)

// KcpDgram mirrors halo_kcp_dgram_t (40 bytes).
type KcpDgram struct {
	Index      uint32 // the datagram's entry in the delivery index
	Kind       uint8
	ConnType   uint8
	Ret        int8 // Input's return value: 0 or -1..-4
	Reserved   uint8
	Conv0      uint64 // KCP: LE u64 at byte 0; ENet: rawConv
	NSegs      uint16 // processed segments
	NWalked    uint16 // segments with a descriptor, >= NSegs
	FirstSeg   uint32
	PayloadLen uint32
	SessionId  uint32 // ENet fields
	Conv       uint32
	EnetType   uint32
}

// KcpSeg mirrors halo_kcp_seg_t (32 bytes).
type KcpSeg struct {
	Dgram    uint32
	Cmd      uint8
	Frg      uint8
	Wnd      uint16
	Ts       uint32
	Sn       uint32
	Una      uint32
	Len      uint32
	DataOff  uint32 // byte offset of the data in the delivery stream
	Check    uint8
	Reserved [3]uint8
}

// KcpSummary mirrors halo_kcp_summary_t (96 bytes). Dgrams, Segs and Ignored are totals over the
// delivery; the other counters describe the written datagrams.
type KcpSummary struct {
	Dgrams        uint32
	DgramsWritten uint32
	Segs          uint32
	SegsWritten   uint32
	RetCounts     [5]uint32 // written KCP datagrams with Ret == -i
	EnetCounts    [4]uint32
	Ignored       uint32
	BytesHashed   uint64
	InPkts        uint64 // DefaultSnmp.InPkts / InBytes / KCPInErrors / InSegs
	InBytes       uint64
	InErrs        uint64
	InSegs        uint64
}

// KcpIngest owns the outputs of host calls.
type KcpIngest struct {
	Port          uint16
	ByteCheckMode int
	Dgrams        []KcpDgram
	Segs          []KcpSeg
	Summary       KcpSummary
}

// NewKcpIngest makes the buffers for dgramCap datagram records and segCap segment descriptors.
func NewKcpIngest(port uint16, byteCheckMode, dgramCap, segCap int) *KcpIngest {
	return &KcpIngest{Port: port, ByteCheckMode: byteCheckMode, Dgrams: make([]KcpDgram, dgramCap+1), Segs: make([]KcpSeg, segCap+1)}
}

func kcpCfg(port uint16, mode, dgramCap, segCap int) C.halo_kcp_config_t {
	return C.gpurx_kcp_config(C.int(mode), C.uint32_t(port), C.uint32_t(dgramCap), C.uint32_t(segCap))
}

// Ingest runs the sequential loop over the written records of a host Delivery. A Delivery made
// without an index (IndexCap 0) is an error; an empty delivery zeroes the summary, as the C call does.
func (k *KcpIngest) Ingest(d *Delivery) error {
	if d == nil || d.IndexCap == 0 || len(d.Index) == 0 || len(d.Out) == 0 {
		return errors.New("gpurx: KcpIngest needs a Delivery with an index")
	}
	cfg := kcpCfg(k.Port, k.ByteCheckMode, len(k.Dgrams)-1, len(k.Segs)-1)
	return halo(C.halo_kcp_ingest_host(&cfg, (*C.uint8_t)(unsafe.Pointer(&d.Out[0])),
		(*C.halo_deliver_summary_t)(unsafe.Pointer(&d.Summary)), (*C.halo_deliver_index_t)(unsafe.Pointer(&d.Index[0])),
		C.uint32_t(d.IndexCap), (*C.halo_kcp_dgram_t)(unsafe.Pointer(&k.Dgrams[0])), (*C.halo_kcp_seg_t)(unsafe.Pointer(&k.Segs[0])),
		(*C.halo_kcp_summary_t)(unsafe.Pointer(&k.Summary))))
}

// Written is the written datagram records.
func (k *KcpIngest) Written() []KcpDgram { return k.Dgrams[:k.Summary.DgramsWritten] }

// SegmentsOf is the processed segments' descriptors of written datagram j.
func (k *KcpIngest) SegmentsOf(j int) []KcpSeg {
	g := k.Dgrams[j]
	return k.Segs[g.FirstSeg : g.FirstSeg+uint32(g.NSegs)]
}

// Feed calls back per written datagram, in stream order: onKcp with the record, its processed
// segments' descriptors and their data (aliasing the delivery's stream), onEnet for an ENet
// control packet. Either may be nil.
func (k *KcpIngest) Feed(d *Delivery, onKcp func(g KcpDgram, segs []KcpSeg, data [][]byte), onEnet func(g KcpDgram)) {
	s := d.Stream()
	for j, g := range k.Written() {
		if g.Kind == KcpDgramEnet {
			if onEnet != nil {
				onEnet(g)
			}
			continue
		}
		if onKcp == nil {
			continue
		}
		segs := k.SegmentsOf(j)
		data := make([][]byte, len(segs))
		for i, x := range segs {
			data[i] = s[x.DataOff : x.DataOff+x.Len]
		}
		onKcp(g, segs, data)
	}
}

// KcpIngestWorkspace is the device workspace a device call needs, in bytes.
func KcpIngestWorkspace(indexCap, segCap int) uint64 {
	return uint64(C.halo_kcp_ingest_workspace(C.uint32_t(indexCap), C.uint32_t(segCap)))
}

// KcpIngestDevice describes the device buffers of a device call: every pointer is a device
// pointer. Dgrams is DgramCap halo_kcp_dgram_t (8-byte aligned), Segs SegCap halo_kcp_seg_t
// (16-byte aligned), Summary one halo_kcp_summary_t.
type KcpIngestDevice struct {
	Port             uint16
	ByteCheckMode    int
	DgramCap, SegCap int
	Dgrams, Segs     unsafe.Pointer
	Summary          unsafe.Pointer
	Workspace        unsafe.Pointer
	WorkspaceBytes   uint64
}

// Run issues the launches on the null stream over the outputs of a DeliverDevice call: its
// stream, its device-resident summary and its index of indexCap entries.
func (k *KcpIngestDevice) Run(dStream, dDeliverSummary, dIndex unsafe.Pointer, indexCap int) error {
	cfg := kcpCfg(k.Port, k.ByteCheckMode, k.DgramCap, k.SegCap)
	return halo(C.halo_kcp_ingest_device(&cfg, (*C.uint8_t)(dStream), (*C.halo_deliver_summary_t)(dDeliverSummary),
		(*C.halo_deliver_index_t)(dIndex), C.uint32_t(indexCap), (*C.halo_kcp_dgram_t)(k.Dgrams), (*C.halo_kcp_seg_t)(k.Segs),
		(*C.halo_kcp_summary_t)(k.Summary), k.Workspace, C.uint64_t(k.WorkspaceBytes), nil))
}
