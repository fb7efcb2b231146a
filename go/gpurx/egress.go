package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"errors"
	"unsafe"
)

// The egress step (halo_rx.h "egress"): the forward path's last stage, TxEthernet -> BuildEthFrm ->
// EthTxFunc -> RingBufferProducer.WritePacket (engine/ethernet_engine.go:34-49, :117-129,
// mem/ring_buffer.go:249-295), for a whole batch at once. A batch that Switch.Forward or the ARP
// encap has decided on is partitioned into one byte stream per egress port, each frame laid out as
// the ring record WritePacket would write (u32 length max(len, 60), the bytes, zero padding), and
// WriteSpan publishes a port's stream into its tx ring with one release store of head.

// Kinds of selector (HALO_EGRESS_KIND_*).
const (
	EgressKindMasks  = 0
	EgressKindArp    = 1
	EgressKindSwitch = 2
)

// EgressPort mirrors halo_egress_port_t.
type EgressPort struct {
	Frames        uint32 // records selected for the port, also beyond the region
	FramesWritten uint32 // the prefix of them that fits the region wholly
	Bytes         uint64
	BytesWritten  uint64
}

// Egress owns the outputs of egress calls over host memory: Ports regions of Region bytes, the
// per-port summaries and index lists. One Egress serves one caller at a time.
type Egress struct {
	Ports    int
	Region   uint64
	IndexCap int
	Jumbo    bool
	Out      []byte
	Summary  []EgressPort
	Index    []uint32 // [port * IndexCap + k]: the batch index of the port's k-th record
	Skipped  uint32   // selected frames that were not sendable, summed over the calls
}

// NewEgress makes the buffers for `ports` egress ports with `region` bytes of stream each.
func NewEgress(ports int, region uint64, indexCap int) (*Egress, error) {
	if ports < 1 || ports > int(C.HALO_EGRESS_MAX_PORTS) {
		return nil, errors.New("gpurx: an egress has 1..64 ports")
	}
	return &Egress{Ports: ports, Region: region, IndexCap: indexCap, Out: make([]byte, uint64(ports)*region+1),
		Summary: make([]EgressPort, ports), Index: make([]uint32, ports*indexCap+1)}, nil
}

func (e *Egress) cfg() C.halo_egress_config_t {
	var cfg C.halo_egress_config_t
	cfg.n_ports = C.uint32_t(e.Ports)
	if e.Jumbo {
		cfg.flags = C.HALO_RX_JUMBO_EXT
	}
	cfg.region_bytes = C.uint64_t(e.Region)
	cfg.index_cap = C.uint32_t(e.IndexCap)
	return cfg
}

// Switch partitions a batch a host switch has forwarded (b.Res holds its verdicts): SwUnicast goes
// to OutPort, SwFlood to every port of flood (Switch.FloodMask of the ingress port), everything
// else nowhere.
func (e *Egress) Switch(b *SwBatch, flood uint64) error {
	n := b.Len()
	if n == 0 {
		for p := range e.Summary {
			e.Summary[p] = EgressPort{}
		}
		return nil
	}
	cfg := e.cfg()
	return halo(C.halo_tx_egress_host(&cfg, C.HALO_EGRESS_KIND_SWITCH, (*C.uint8_t)(unsafe.Pointer(&b.Buf[:1][0])),
		(*C.uint32_t)(unsafe.Pointer(&b.Off[0])), (*C.uint16_t)(unsafe.Pointer(&b.Lens[0])), C.uint32_t(n),
		unsafe.Pointer(&b.Res[0]), C.uint64_t(flood), (*C.uint8_t)(unsafe.Pointer(&e.Out[0])),
		(*C.halo_egress_port_t)(unsafe.Pointer(&e.Summary[0])), (*C.uint32_t)(unsafe.Pointer(&e.Index[0])),
		(*C.uint32_t)(unsafe.Pointer(&e.Skipped))))
}

// Masks is the same for explicit port masks: bit p of masks[k] sends frame k to port p.
func (e *Egress) Masks(b *SwBatch, masks []uint64) error {
	n := b.Len()
	if n == 0 || len(masks) < n {
		return errors.New("gpurx: an empty batch, or fewer masks than frames")
	}
	cfg := e.cfg()
	return halo(C.halo_tx_egress_host(&cfg, C.HALO_EGRESS_KIND_MASKS, (*C.uint8_t)(unsafe.Pointer(&b.Buf[:1][0])),
		(*C.uint32_t)(unsafe.Pointer(&b.Off[0])), (*C.uint16_t)(unsafe.Pointer(&b.Lens[0])), C.uint32_t(n),
		unsafe.Pointer(&masks[0]), 0, (*C.uint8_t)(unsafe.Pointer(&e.Out[0])),
		(*C.halo_egress_port_t)(unsafe.Pointer(&e.Summary[0])), (*C.uint32_t)(unsafe.Pointer(&e.Index[0])),
		(*C.uint32_t)(unsafe.Pointer(&e.Skipped))))
}

// Stream is port p's written records.
func (e *Egress) Stream(p int) []byte {
	lo := uint64(p) * e.Region
	return e.Out[lo : lo+e.Summary[p].BytesWritten]
}

// PortIndex is the batch indices of port p's first min(Frames, IndexCap) records.
func (e *Egress) PortIndex(p int) []uint32 {
	k := int(e.Summary[p].Frames)
	if k > e.IndexCap {
		k = e.IndexCap
	}
	return e.Index[p*e.IndexCap : p*e.IndexCap+k]
}

// EgressWorkspace is the device workspace a device call over n frames and `ports` ports needs.
func EgressWorkspace(n, ports int) uint64 {
	return uint64(C.halo_tx_egress_workspace(C.uint32_t(n), C.uint32_t(ports)))
}

// EgressDevice describes the device buffers of a device call: every pointer is a device pointer.
// Out is Ports * Region bytes, 16-byte aligned; Summary is Ports halo_egress_port_t; Index
// (optional) Ports * IndexCap u32; Skipped (optional) one u32, incremented.
type EgressDevice struct {
	Ports          int
	IndexCap       int
	Region         uint64
	Jumbo          bool
	Out            unsafe.Pointer
	Summary        unsafe.Pointer
	Index          unsafe.Pointer
	Skipped        unsafe.Pointer
	Workspace      unsafe.Pointer
	WorkspaceBytes uint64
}

func (d *EgressDevice) cfg() C.halo_egress_config_t {
	e := Egress{Ports: d.Ports, Region: d.Region, IndexCap: d.IndexCap, Jumbo: d.Jumbo}
	return e.cfg()
}

// ArpDevice follows ArpEncapDevice on the null stream: dResults are its halo_arp_result_t.
func (d *EgressDevice) ArpDevice(dFrames, dOffsets, dLens unsafe.Pointer, n int, dResults unsafe.Pointer) error {
	cfg := d.cfg()
	return halo(C.halo_tx_egress_arp_device(&cfg, (*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens),
		C.uint32_t(n), (*C.halo_arp_result_t)(dResults), (*C.uint8_t)(d.Out), (*C.halo_egress_port_t)(d.Summary),
		(*C.uint32_t)(d.Index), (*C.uint32_t)(d.Skipped), d.Workspace, C.uint64_t(d.WorkspaceBytes), nil))
}

// SwitchDevice follows Switch.ForwardDevice on the null stream.
func (d *EgressDevice) SwitchDevice(dFrames, dOffsets, dLens unsafe.Pointer, n int, dResults unsafe.Pointer,
	flood uint64) error {
	cfg := d.cfg()
	return halo(C.halo_tx_egress_switch_device(&cfg, (*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens),
		C.uint32_t(n), (*C.halo_sw_result_t)(dResults), C.uint64_t(flood), (*C.uint8_t)(d.Out),
		(*C.halo_egress_port_t)(d.Summary), (*C.uint32_t)(d.Index), (*C.uint32_t)(d.Skipped), d.Workspace,
		C.uint64_t(d.WorkspaceBytes), nil))
}

// MasksDevice takes one u64 port mask per frame.
func (d *EgressDevice) MasksDevice(dFrames, dOffsets, dLens unsafe.Pointer, n int, dMasks unsafe.Pointer) error {
	cfg := d.cfg()
	return halo(C.halo_tx_egress_masks_device(&cfg, (*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens),
		C.uint32_t(n), (*C.uint64_t)(dMasks), (*C.uint8_t)(d.Out), (*C.halo_egress_port_t)(d.Summary),
		(*C.uint32_t)(d.Index), (*C.uint32_t)(d.Skipped), d.Workspace, C.uint64_t(d.WorkspaceBytes), nil))
}

// WriteSpan publishes a run of whole records (Egress.Stream(p)) into the ring at `ring` (the
// memory of a mem.RingBuffer this process produces into): the longest prefix of records that fits
// the free space, one release store of head. It returns the records and bytes taken.
func WriteSpan(ring unsafe.Pointer, span []byte) (int, uint64, error) {
	if len(span) == 0 {
		return 0, 0, nil
	}
	var recs C.uint32_t
	var taken C.uint64_t
	err := halo(C.halo_ring_write_span(ring, (*C.uint8_t)(unsafe.Pointer(&span[0])), C.uint64_t(len(span)), &recs, &taken))
	return int(recs), uint64(taken), err
}
