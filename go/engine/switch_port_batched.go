package engine

// The batched SwitchPort.PacketHandle: a sketch of the file a halo maintainer adds to package
// engine to run a switch's MAC learning and forwarding decision through package gpurx. It keeps
// PacketHandle's loop — each frame goes out of the ports the reference would have sent it to, in
// frame order — but learns and decides a whole batch in one call, lays the batch out as one stream
// of ring records per egress port in a second (what TxEthernet -> BuildEthFrm -> WritePacket
// would write frame by frame) and publishes each port's stream into its tx ring with one call.
//
// Reference: engine/engine.go:491-505 (SwitchPort.PacketHandle), engine/ethernet_engine.go:58-129
// (RxEthernet, HandleEthernet, TxEthernet), mem/ring_buffer.go:249-295 (WritePacket).
//
// Differences in timing, not in one port's results: the reference interleaves the ports' frames
// under SwitchMacAddrLock one frame at a time, while here a port's batch is applied as a whole, so
// two ports that learn the same MAC in overlapping polls may order differently below batch
// granularity. sw serialises the batches (one Forward at a time); port indexes are positions in
// SwitchConfig.SwitchPortList. SwitchMacAddrClear becomes one sw.Expire(TimeNow) per tick.

import (
	"fmt"
	"unsafe"

	"github.com/flswld/halo/cpu"
	"github.com/flswld/halo/gpurx"
)

// PacketHandleBatched replaces `go switchPort.PacketHandle()` for port number `port` of a switch
// whose table lives behind sw (a host switch: gpurx.NewSwitch(vlans, capacity, batch, -1)).
// txRings[q] is the memory of the tx ring port q's EthTxFunc writes into (dpdk.go:202-213: the
// RingBufferProducer's RingBuffer), and txLocks[q] the lock under which port q's ring is produced
// into: several ingress ports may egress to one port. lock serialises the switch's batches.
func (s *SwitchPort) PacketHandleBatched(sw *gpurx.Switch, port int, txRings []unsafe.Pointer, txLocks []*cpu.SpinLock,
	lock *cpu.SpinLock, batch int) {
	if s.Config.BindCpuCore >= 0 {
		cpu.BindCpuCore(s.Config.BindCpuCore)
	}
	if batch <= 0 {
		batch = 256
	}
	flood, err := sw.FloodMask(port)
	if err != nil {
		Log(fmt.Sprintf("switch flood mask error: %v\n", err))
		s.Switch.StopWaitGroup.Done()
		return
	}
	b := gpurx.NewSwBatch(batch)
	// a flood sends every frame of the batch to every port: a region holds a whole batch of
	// full-size records (4 + 1514, rounded up to 4) and the next multiple of 16
	eg, err := gpurx.NewEgress(len(txRings), (uint64(batch)*1520+15)&^15, 0)
	if err != nil {
		Log(fmt.Sprintf("switch egress error: %v\n", err))
		s.Switch.StopWaitGroup.Done()
		return
	}
	for !s.Switch.Stop.Load() {
		b.Reset()
		for b.Len() < batch {
			f := s.Config.EthRxFunc()
			if f == nil {
				break // the batch ends at the first empty poll
			}
			b.Add(f)
		}
		if b.Len() == 0 {
			continue
		}
		lock.Lock()
		err := sw.Forward(port, b, s.Switch.TimeNow)
		lock.Unlock()
		if err != nil {
			Log(fmt.Sprintf("switch forward error, %d frames dropped: %v\n", b.Len(), err))
			continue
		}
		for k := 0; k < b.Len(); k++ {
			if v := b.Res[k].Verdict; v == gpurx.SwEthLen || v == gpurx.SwEthType {
				Log(fmt.Sprintf("parse ethernet frame error: verdict %d\n", v))
			}
		}
		// one egress call for the batch, then one ring write per port that got something
		if err := eg.Switch(b, flood); err != nil {
			Log(fmt.Sprintf("switch egress error, %d frames dropped: %v\n", b.Len(), err))
			continue
		}
		for q := range txRings {
			span := eg.Stream(q)
			if len(span) == 0 {
				continue
			}
			txLocks[q].Lock()
			taken, _, err := gpurx.WriteSpan(txRings[q], span)
			txLocks[q].Unlock()
			if err != nil {
				Log(fmt.Sprintf("tx ring write error on port %d: %v\n", q, err))
			} else if taken < int(eg.Summary[q].FramesWritten) {
				// a full ring: WritePacket drops the frame too (dpdk.go:202-213 ignores its result)
				Log(fmt.Sprintf("tx ring of port %d full, %d frames dropped\n", q, int(eg.Summary[q].FramesWritten)-taken))
			}
		}
	}
	s.Switch.StopWaitGroup.Done()
}
