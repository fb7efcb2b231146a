package engine

// The batched SwitchPort.PacketHandle: a sketch of the file a halo maintainer adds to package
// engine to run a switch's MAC learning and forwarding decision through package gpurx. It keeps
// PacketHandle's loop and TxEthernet's surface — each frame goes out of the ports the reference
// would have sent it to, in frame order — but learns and decides a whole batch in one call and
// then transmits per verdict.
//
// Reference: engine/engine.go:491-505 (SwitchPort.PacketHandle), engine/ethernet_engine.go:58-129
// (RxEthernet, HandleEthernet, TxEthernet).
//
// Differences in timing, not in one port's results: the reference interleaves the ports' frames
// under SwitchMacAddrLock one frame at a time, while here a port's batch is applied as a whole, so
// two ports that learn the same MAC in overlapping polls may order differently below batch
// granularity. sw serialises the batches (one Forward at a time); port indexes are positions in
// SwitchConfig.SwitchPortList. SwitchMacAddrClear becomes one sw.Expire(TimeNow) per tick.

import (
	"fmt"

	"github.com/flswld/halo/cpu"
	"github.com/flswld/halo/gpurx"
)

// PacketHandleBatched replaces `go switchPort.PacketHandle()` for port number `port` of a switch
// whose table lives behind sw (a host switch: gpurx.NewSwitch(vlans, capacity, batch, -1)).
// ports[q] is the SwitchPort with index q; lock serialises the switch's batches across its ports.
func (s *SwitchPort) PacketHandleBatched(sw *gpurx.Switch, port int, ports []*SwitchPort, lock *cpu.SpinLock, batch int) {
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
			r := b.Res[k]
			switch r.Verdict {
			case gpurx.SwUnicast:
				ports[r.OutPort].txFrame(b.Frame(k))
			case gpurx.SwFlood:
				for q := 0; q < len(ports); q++ {
					if flood&(1<<uint(q)) != 0 {
						ports[q].txFrame(b.Frame(k))
					}
				}
			case gpurx.SwEthLen, gpurx.SwEthType:
				Log(fmt.Sprintf("parse ethernet frame error: verdict %d\n", r.Verdict))
			}
		}
	}
	s.Switch.StopWaitGroup.Done()
}

// txFrame is TxEthernet for a frame whose header is already in place: BuildEthFrm copies the
// payload behind the same addresses and EtherType and pads to 60 bytes (the record's TxLen).
func (s *SwitchPort) txFrame(frm []byte) bool {
	ethProto := uint16(frm[12])<<8 | uint16(frm[13])
	return s.TxEthernet(frm[14:], frm[0:6], frm[6:12], ethProto)
}
