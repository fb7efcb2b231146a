package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"errors"
	"unsafe"
)

// The tx ring producer (halo_rx.h "the tx ring producer"): WriteSpan with the span in device memory.
// An egress stream (EgressDevice) is published into its tx ring where it lies in HBM: the device
// finds the records, reads head and tail, copies what fits into the mapped ring and publishes head
// with one release store. The host reads a 24-byte result and touches no frame byte. WriteSpan
// remains the call for polls at the reference's cadence.

// Status of a device write (HALO_TXRING_*).
const (
	TxRingOK      = 0 // the whole span was taken
	TxRingShort   = 1 // a proper prefix (possibly nothing): resubmit span + Bytes once the consumer has read
	TxRingBadSpan = 2 // a malformed record in the examined window: nothing written
)

// TxRingResult mirrors halo_tx_ring_result_t.
type TxRingResult struct {
	Status  uint32
	Records uint32
	Bytes   uint64
	Head    uint64 // the ring's head after the call
}

// TxRing is the device producer of one ring. One producer per ring; its writes go to one stream.
type TxRing struct {
	h *C.halo_tx_ring_t
}

// AttachTxRing attaches to the ring at `ring` (the memory of a mem.RingBuffer this process produces
// into; offset as for NewRingBufferProducer). With register the ring is registered for the device,
// as AttachRing does; without it the memory must already be mapped for the device, e.g. by a
// consumer attached to the same ring.
func AttachTxRing(device int, ring unsafe.Pointer, offset int64, register bool) (*TxRing, error) {
	var flags C.uint32_t
	if register {
		flags = C.HALO_RING_REGISTER
	}
	t := &TxRing{}
	if err := halo(C.halo_tx_ring_attach(C.int(device), ring, C.int64_t(offset), flags, &t.h)); err != nil {
		return nil, err
	}
	return t, nil
}

// Close waits for the device's work on the ring and detaches. On error the ring memory may still
// be mapped for the device: keep it allocated.
func (t *TxRing) Close() error {
	if t.h == nil {
		return nil
	}
	h := t.h
	t.h = nil
	return halo(C.halo_tx_ring_detach(h))
}

// TxRingWorkspace is the device workspace a write of spanBytes needs (0: the span is too large).
func TxRingWorkspace(spanBytes uint64) uint64 {
	return uint64(C.halo_tx_ring_workspace(C.uint64_t(spanBytes)))
}

// WriteSpanDevice enqueues the write of spanBytes bytes of whole records at dSpan (device memory,
// 4-byte aligned) on the null stream. dResult (optional) is device or mapped host memory holding a
// TxRingResult once the stream has reached it; dWorkspace is TxRingWorkspace(spanBytes) bytes of
// device memory, 16-byte aligned. Writes on one stream chain: each starts at the head the one
// before it published.
func (t *TxRing) WriteSpanDevice(dSpan unsafe.Pointer, spanBytes uint64, dResult, dWorkspace unsafe.Pointer,
	workspaceBytes uint64) error {
	if t.h == nil {
		return errors.New("gpurx: the tx ring is closed")
	}
	return halo(C.halo_tx_ring_write_span_device(t.h, (*C.uint8_t)(dSpan), C.uint64_t(spanBytes),
		(*C.halo_tx_ring_result_t)(dResult), dWorkspace, C.uint64_t(workspaceBytes), nil))
}
