package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"errors"
	"unsafe"
)

// KCP emit (halo_rx.h "KCP emit"): the stateless tail of the KCP transmit path — KCP.flush's
// packing of a session's send list into datagrams of at most mtu bytes (protocol/kcp/kcp.go:770-950,
// makeSpace / flushBuffer), segment.encode (kcp.go:134-155) with the byte check of every PUSH, the
// copy of the data, and BuildEnet's control packets (enet.go:75-97) — from entries and segment
// descriptors to the stream of UDP payloads and one BuildDesc per datagram, ready for BuildBatch
// with the stream as its payload. A session decides what to send (which segments, ts, wnd, una, sn)
// and calls this from update() / uncork() instead of encoding and copying itself.

// Per-entry status.
const (
	KcpEmitOK         = 0
	KcpEmitSegTooLong = 1 // some H + len > mtu
	KcpEmitBadMtu     = 2 // mtu <= H or mtu > 1472
	KcpEmitBadRange   = 3 // a range outside the list or into the previous entry, data outside the payload, a bad ENet entry
	KcpEmitMax        = 1 << 23
)

// KcpOutSession mirrors halo_kcp_out_session_t (40 bytes): one flush (Kind KcpDgramKcp) or one
// control packet (KcpDgramEnet).
type KcpOutSession struct {
	Conv      uint64 // kcp.conv
	FirstSeg  uint32 // its range in the segment list
	NSegs     uint32
	DstIp     uint32 // s.remote
	DstPort   uint16
	Mtu       uint16 // kcp.mtu
	Kind      uint8
	ConnType  uint8 // ENet: KcpEnet*
	Reserved  uint16
	SessionId uint32 // ENet: BuildEnet's arguments
	EnetConv  uint32
	EnetType  uint32
}

// KcpOutDgram mirrors halo_kcp_out_dgram_t (16 bytes).
type KcpOutDgram struct {
	Offset   uint32 // of the datagram in the stream, a multiple of 4
	Len      uint16
	NSegs    uint16
	Session  uint32
	FirstSeg uint32
}

// KcpEmitSummary mirrors halo_kcp_emit_summary_t (88 bytes). Sessions, Dgrams, Segs, Bytes and
// StatusCounts are totals over the call; the other counters describe the written prefix.
type KcpEmitSummary struct {
	Sessions        uint32
	SessionsWritten uint32
	Dgrams          uint32
	DgramsWritten   uint32
	Segs            uint32
	SegsWritten     uint32
	StatusCounts    [4]uint32
	Bytes           uint64
	BytesWritten    uint64
	BytesHashed     uint64
	OutSegs         uint64 // DefaultSnmp.OutSegs / OutPkts / OutBytes
	OutPkts         uint64
	OutBytes        uint64
}

// KcpEmit owns the outputs of host calls.
type KcpEmit struct {
	ByteCheckMode int
	SrcIp         uint32
	SrcPort       uint16
	Stream        []byte
	Dgrams        []KcpOutDgram
	Descs         []BuildDesc
	Status        []uint8
	Summary       KcpEmitSummary
}

// NewKcpEmit makes the buffers for dgramCap datagrams in streamCap stream bytes.
func NewKcpEmit(byteCheckMode int, srcIp uint32, srcPort uint16, dgramCap, streamCap int) *KcpEmit {
	return &KcpEmit{ByteCheckMode: byteCheckMode, SrcIp: srcIp, SrcPort: srcPort, Stream: make([]byte, streamCap+4),
		Dgrams: make([]KcpOutDgram, dgramCap+1), Descs: make([]BuildDesc, dgramCap+1)}
}

func kcpEmitCfg(mode int, srcIp uint32, srcPort uint16, dgramCap, streamCap int) C.halo_kcp_emit_config_t {
	return C.gpurx_kcp_emit_config(C.int(mode), C.uint32_t(srcIp), C.uint32_t(srcPort), C.uint32_t(dgramCap), C.uint32_t(streamCap))
}

// Emit runs the sequential loop: sessions over segs, whose DataOff point into payload.
func (k *KcpEmit) Emit(sessions []KcpOutSession, segs []KcpSeg, payload []byte) error {
	if len(sessions) == 0 {
		k.Summary = KcpEmitSummary{}
		return nil
	}
	if len(segs) == 0 || len(payload) == 0 {
		return errors.New("gpurx: KcpEmit needs a segment list and a payload")
	}
	if len(k.Status) < len(sessions) {
		k.Status = make([]uint8, len(sessions))
	}
	cfg := kcpEmitCfg(k.ByteCheckMode, k.SrcIp, k.SrcPort, len(k.Dgrams)-1, len(k.Stream)-4)
	return halo(C.halo_kcp_emit_host(&cfg, (*C.halo_kcp_out_session_t)(unsafe.Pointer(&sessions[0])), C.uint32_t(len(sessions)),
		(*C.halo_kcp_seg_t)(unsafe.Pointer(&segs[0])), C.uint32_t(len(segs)), (*C.uint8_t)(unsafe.Pointer(&payload[0])),
		C.uint64_t(len(payload)), (*C.uint8_t)(unsafe.Pointer(&k.Stream[0])), (*C.halo_kcp_out_dgram_t)(unsafe.Pointer(&k.Dgrams[0])),
		(*C.halo_tx_build_desc_t)(unsafe.Pointer(&k.Descs[0])), (*C.uint8_t)(unsafe.Pointer(&k.Status[0])),
		(*C.halo_kcp_emit_summary_t)(unsafe.Pointer(&k.Summary))))
}

// Written is the written datagram records.
func (k *KcpEmit) Written() []KcpOutDgram { return k.Dgrams[:k.Summary.DgramsWritten] }

// Datagram is the UDP payload of written datagram j (aliasing the stream).
func (k *KcpEmit) Datagram(j int) []byte {
	g := k.Dgrams[j]
	return k.Stream[g.Offset : g.Offset+uint32(g.Len)]
}

// KcpEmitWorkspace is the device workspace a device call needs, in bytes.
func KcpEmitWorkspace(nSessions, nSegs int) uint64 {
	return uint64(C.halo_kcp_emit_workspace(C.uint32_t(nSessions), C.uint32_t(nSegs)))
}

// KcpEmitDevice describes the device buffers of a device call: every pointer is a device pointer.
// Stream is StreamCap bytes (4-byte aligned), Dgrams DgramCap halo_kcp_out_dgram_t (16-byte
// aligned), Descs DgramCap halo_tx_build_desc_t (8-byte aligned), Status one byte per entry,
// Summary one halo_kcp_emit_summary_t.
type KcpEmitDevice struct {
	ByteCheckMode       int
	SrcIp               uint32
	SrcPort             uint16
	DgramCap, StreamCap int
	Stream              unsafe.Pointer
	Dgrams, Descs       unsafe.Pointer
	Status, Summary     unsafe.Pointer
	Workspace           unsafe.Pointer
	WorkspaceBytes      uint64
}

// Run issues the launches on the null stream: nSessions entries (8-byte aligned) over nSegs
// descriptors (16-byte aligned; a KcpIngestDevice's Segs serves) whose data lie in dPayload.
func (k *KcpEmitDevice) Run(dSessions unsafe.Pointer, nSessions int, dSegs unsafe.Pointer, nSegs int, dPayload unsafe.Pointer,
	payloadBytes uint64) error {
	cfg := kcpEmitCfg(k.ByteCheckMode, k.SrcIp, k.SrcPort, k.DgramCap, k.StreamCap)
	return halo(C.halo_kcp_emit_device(&cfg, (*C.halo_kcp_out_session_t)(dSessions), C.uint32_t(nSessions), (*C.halo_kcp_seg_t)(dSegs),
		C.uint32_t(nSegs), (*C.uint8_t)(dPayload), C.uint64_t(payloadBytes), (*C.uint8_t)(k.Stream), (*C.halo_kcp_out_dgram_t)(k.Dgrams),
		(*C.halo_tx_build_desc_t)(k.Descs), (*C.uint8_t)(k.Status), (*C.halo_kcp_emit_summary_t)(k.Summary), k.Workspace,
		C.uint64_t(k.WorkspaceBytes), nil))
}
