package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"errors"
	"unsafe"
)

// The L2 switch (halo_rx.h "L2 switch"): engine.Switch's MAC table and SwitchPort.RxEthernet /
// HandleEthernet (engine/ethernet_engine.go:58-114) over one batch of frames from one port.
// A Switch made with device < 0 is a host switch: frames, offsets and lengths are Go memory and
// Forward runs the reference's loop in C. With device >= 0 the table lives in HBM, the arrays are
// device pointers and Forward is asynchronous on the null stream; calls on one Switch are issued
// by one goroutine at a time, in the order they are to be applied.

// Verdicts of Forward (HALO_SW_V_*).
const (
	SwEthLen    = 0
	SwEthType   = 1
	SwSrcMcast  = 2
	SwTableFull = 3
	SwUnicast   = 4
	SwFlood     = 5
	SwVerdicts  = 6
)

// SwResult mirrors halo_sw_result_t.
type SwResult struct {
	Verdict uint8
	OutPort uint8 // the egress port of SwUnicast, else 0xFF
	TxLen   uint16
}

// SwEntry mirrors halo_switch_entry_t (engine.SwitchMacAddr with the port as an index).
type SwEntry struct {
	Mac        [6]byte
	Port       uint8
	Pad        uint8
	CreateTime uint32
}

// Switch owns a halo_switch_t.
type Switch struct {
	h      *C.halo_switch_t
	Ports  int
	Device int
}

// NewSwitch makes a switch with one VLAN id per port (SwitchPortConfig.VlanId, in port order).
// capacity is the most MAC entries the table takes; maxBatch the most frames per Forward.
func NewSwitch(vlanIds []uint16, capacity, maxBatch, device int) (*Switch, error) {
	if len(vlanIds) < 1 || len(vlanIds) > int(C.HALO_SW_MAX_PORTS) {
		return nil, errors.New("gpurx: a switch has 1..64 ports")
	}
	var cfg C.halo_switch_config_t
	cfg.n_ports = C.uint32_t(len(vlanIds))
	for q, v := range vlanIds {
		cfg.vlan_id[q] = C.uint16_t(v)
	}
	cfg.capacity = C.uint32_t(capacity)
	cfg.max_batch = C.uint32_t(maxBatch)
	cfg.device = C.int(device)
	s := &Switch{Ports: len(vlanIds), Device: device}
	if err := halo(C.halo_switch_create(&cfg, &s.h)); err != nil {
		return nil, err
	}
	return s, nil
}

// Close destroys the switch.
func (s *Switch) Close() error {
	if s.h == nil {
		return nil
	}
	err := halo(C.halo_switch_destroy(s.h))
	s.h = nil
	return err
}

// FloodMask is the set of ports a flood from `port` goes out of: bit q = port q.
func (s *Switch) FloodMask(port int) (uint64, error) {
	var m C.uint64_t
	err := halo(C.halo_switch_flood_mask(s.h, C.uint32_t(port), &m))
	return uint64(m), err
}

// ForwardDevice is one batch of a device switch: every pointer is a device pointer. dCounts
// (optional, SwVerdicts u32 counters) is incremented.
func (s *Switch) ForwardDevice(port int, dFrames, dOffsets, dLens unsafe.Pointer, n int, now uint32, dResults,
	dCounts unsafe.Pointer) error {
	return halo(C.halo_switch_forward(s.h, C.uint32_t(port), (*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets),
		(*C.uint16_t)(dLens), C.uint32_t(n), C.uint32_t(now), (*C.halo_sw_result_t)(dResults), (*C.uint32_t)(dCounts), nil))
}

// SwBatch collects the frames one port received, at 4-byte aligned offsets, for a host switch.
type SwBatch struct {
	Buf  []byte
	Off  []uint32 // in dwords
	Lens []uint16
	Res  []SwResult
}

// NewSwBatch makes a batch of up to max frames.
func NewSwBatch(max int) *SwBatch {
	return &SwBatch{Buf: make([]byte, 0, max*1516), Off: make([]uint32, 0, max), Lens: make([]uint16, 0, max),
		Res: make([]SwResult, max)}
}

// Reset empties the batch, keeping its memory.
func (b *SwBatch) Reset() { b.Buf, b.Off, b.Lens = b.Buf[:0], b.Off[:0], b.Lens[:0] }

// Len is the number of frames in the batch.
func (b *SwBatch) Len() int { return len(b.Lens) }

// Add copies one frame in (EthRxFunc's slice aliases a reused buffer). A frame longer than 65535
// bytes is cut: every length past 1514 gets the same SwEthLen verdict.
func (b *SwBatch) Add(frame []byte) {
	if len(frame) > 0xFFFF {
		frame = frame[:0xFFFF]
	}
	b.Off = append(b.Off, uint32(len(b.Buf)/4))
	b.Lens = append(b.Lens, uint16(len(frame)))
	b.Buf = append(b.Buf, frame...)
	for len(b.Buf)%4 != 0 {
		b.Buf = append(b.Buf, 0)
	}
}

// Frame is frame k of the batch.
func (b *SwBatch) Frame(k int) []byte {
	return b.Buf[4*uint64(b.Off[k]) : 4*uint64(b.Off[k])+uint64(b.Lens[k])]
}

// Forward runs a host switch over the batch: b.Res[k] is frame k's verdict.
func (s *Switch) Forward(port int, b *SwBatch, now uint32) error {
	n := b.Len()
	if n == 0 {
		return nil
	}
	if s.Device >= 0 {
		return errors.New("gpurx: Forward takes host memory; a device switch uses ForwardDevice")
	}
	return halo(C.halo_switch_forward(s.h, C.uint32_t(port), (*C.uint8_t)(unsafe.Pointer(&b.Buf[:1][0])),
		(*C.uint32_t)(unsafe.Pointer(&b.Off[0])), (*C.uint16_t)(unsafe.Pointer(&b.Lens[0])), C.uint32_t(n),
		C.uint32_t(now), (*C.halo_sw_result_t)(unsafe.Pointer(&b.Res[0])), nil, nil))
}

// Expire is one SwitchMacAddrClear tick; it returns the number of entries removed.
func (s *Switch) Expire(now uint32) (int, error) {
	var n C.uint32_t
	err := halo(C.halo_switch_expire(s.h, C.uint32_t(now), &n))
	return int(n), err
}

// ListSwitchMacAddr copies the table out (order unspecified).
func (s *Switch) ListSwitchMacAddr() ([]SwEntry, error) {
	var n C.uint32_t
	if err := halo(C.halo_switch_list(s.h, nil, 0, &n)); err != nil {
		return nil, err
	}
	out := make([]SwEntry, int(n)+1)
	if err := halo(C.halo_switch_list(s.h, (*C.halo_switch_entry_t)(unsafe.Pointer(&out[0])), C.uint32_t(len(out)-1),
		&n)); err != nil {
		return nil, err
	}
	if int(n) < len(out)-1 {
		return out[:n], nil
	}
	return out[:len(out)-1], nil
}
