package gpurx

// #include "gpurx_shim.h"
import "C"

import (
	"errors"
	"unsafe"
)

// The DHCP service (halo_rx.h "DHCP"): engine/dhcp_engine.go for a batch at once. The decode
// restates RxDhcp's port test, ParseDhcpPkt and ParseDhcpOption over the DHCP records of a delivery
// stream; DhcpServer is the lease table and RxDhcp's state machine, one per NetIf; the reply build
// makes BuildDhcpPkt's payloads in 288-byte slots and the descriptors the transmit build takes.
// Where the Go code would panic the record says DhcpRefPanic. The option order of a built message
// is the order of the map literals in dhcp_engine.go: one the reference can produce, not the only one.

// Message statuses, directions, option bits and message types.
const (
	DhcpOK       = 0
	DhcpPorts    = 1
	DhcpShort    = 2
	DhcpCookie   = 3
	DhcpRefPanic = 4

	DhcpToServer = 0
	DhcpToClient = 1
	DhcpDirNone  = 2

	DhcpOptMask     = 0x01
	DhcpOptRouter   = 0x02
	DhcpOptDns      = 0x04
	DhcpOptHostname = 0x08
	DhcpOptReqIp    = 0x10
	DhcpOptMsgType  = 0x20
	DhcpOptDnsShort = 0x40

	DhcpDiscover = 1
	DhcpOffer    = 2
	DhcpRequest  = 3
	DhcpAck      = 5
	DhcpNak      = 6
	DhcpRelease  = 7
)

// Verdict codes of DhcpServer.Handle (the low nibble) and their flag bits.
const (
	DhcpHNone          = 0
	DhcpHOffer         = 1
	DhcpHNoAddr        = 2
	DhcpHNoReqIp       = 3
	DhcpHNakZero       = 4
	DhcpHNakSubnet     = 5
	DhcpHNakOtherMac   = 6
	DhcpHNakFull       = 7
	DhcpHAckNak        = 8
	DhcpHRefPanic      = 9
	DhcpHReleased      = 10
	DhcpHReleaseAbsent = 11
	DhcpHClientRequest = 12
	DhcpHClientAck     = 13
	DhcpHMask          = 0x0F
	DhcpHFReused       = 0x40
	DhcpHFReply        = 0x80
)

// DhcpSlotBytes is the payload buffer's stride of the reply build.
const DhcpSlotBytes = 288

// DhcpMsg mirrors halo_dhcp_msg_t (128 bytes).
type DhcpMsg struct {
	Index      uint32 // the message's entry in the delivery index
	Status     uint8
	Dir        uint8
	MsgType    uint8
	Reserved0  uint8
	Options    uint32   // DhcpOpt*
	Xid        [4]uint8 // pkt[4:8]
	Yiaddr     uint32   // IpAddrToU(pkt[16:20])
	Chaddr     [6]uint8
	PayloadLen uint16
	RemoteIp   uint32 // RxDhcp's ipv4SrcAddr
	ReqIp      uint32 // IpAddrToU(option 50's data)
	Mask       [4]uint8
	Gateway    [4]uint8
	Dns        [4]uint8
	MaskN      uint8
	GatewayN   uint8
	Reserved1  [2]uint8
	Reserved2  [3]uint32
	Hostname   [64]uint8 // mem.StaticString64
}

// DhcpSummary mirrors halo_dhcp_summary_t (64 bytes). Msgs is the total; the counts describe the
// written messages.
type DhcpSummary struct {
	Msgs         uint32
	MsgsWritten  uint32
	StatusCounts [5]uint32
	TypeCounts   [9]uint32
}

// DhcpLease mirrors halo_dhcp_lease_t (80 bytes).
type DhcpLease struct {
	Ip       uint32
	Mac      [6]uint8
	Reserved uint16
	ExpTime  uint32
	Hostname [64]uint8
}

// DhcpReply mirrors halo_dhcp_reply_t (32 bytes). Kind is a message type.
type DhcpReply struct {
	Kind      uint8
	Reserved0 [3]uint8
	Xid       [4]uint8
	Yiaddr    uint32
	Chaddr    [6]uint8
	Reserved1 uint16
	ReqIp     uint32
	ServerId  uint32
	Reserved2 uint32
}

// DhcpClientEvent mirrors halo_dhcp_client_event_t (24 bytes): a client ACK for the caller to apply
// (the NetIf's address, the two AddRoute calls, the DNS copy, SendFreeArp).
type DhcpClientEvent struct {
	Msg      uint32
	Ip       uint32
	Mask     [4]uint8
	Gateway  [4]uint8
	Dns      [4]uint8
	MaskN    uint8
	GatewayN uint8
	Options  uint8
	Reserved uint8
}

// DhcpDecode owns the outputs of host decode calls.
type DhcpDecode struct {
	Msgs    []DhcpMsg
	Summary DhcpSummary
}

// NewDhcpDecode makes the buffer for msgCap message records.
func NewDhcpDecode(msgCap int) *DhcpDecode {
	return &DhcpDecode{Msgs: make([]DhcpMsg, msgCap+1)}
}

// Decode runs the sequential loop over the written records of a host Delivery made with Dhcp set
// and an index.
func (k *DhcpDecode) Decode(d *Delivery) error {
	if d == nil || d.IndexCap == 0 || len(d.Index) == 0 || len(d.Out) == 0 {
		return errors.New("gpurx: DhcpDecode needs a Delivery with an index")
	}
	return halo(C.halo_dhcp_decode_host((*C.uint8_t)(unsafe.Pointer(&d.Out[0])), (*C.halo_deliver_summary_t)(unsafe.Pointer(&d.Summary)),
		(*C.halo_deliver_index_t)(unsafe.Pointer(&d.Index[0])), C.uint32_t(d.IndexCap), (*C.halo_dhcp_msg_t)(unsafe.Pointer(&k.Msgs[0])),
		C.uint32_t(len(k.Msgs)-1), (*C.halo_dhcp_summary_t)(unsafe.Pointer(&k.Summary))))
}

// Written is the written message records.
func (k *DhcpDecode) Written() []DhcpMsg { return k.Msgs[:k.Summary.MsgsWritten] }

// DhcpDecodeWorkspace is the device workspace a device call needs, in bytes.
func DhcpDecodeWorkspace(indexCap int) uint64 {
	return uint64(C.halo_dhcp_decode_workspace(C.uint32_t(indexCap)))
}

// DhcpDecodeDevice describes the device buffers of a device call: every pointer is a device
// pointer. Msgs is MsgCap halo_dhcp_msg_t (16-byte aligned), Summary one halo_dhcp_summary_t.
type DhcpDecodeDevice struct {
	MsgCap         int
	Msgs, Summary  unsafe.Pointer
	Workspace      unsafe.Pointer
	WorkspaceBytes uint64
}

// Run issues the launches on the null stream over the outputs of a DeliverDevice call.
func (k *DhcpDecodeDevice) Run(dStream, dDeliverSummary, dIndex unsafe.Pointer, indexCap int) error {
	return halo(C.halo_dhcp_decode_device((*C.uint8_t)(dStream), (*C.halo_deliver_summary_t)(dDeliverSummary),
		(*C.halo_deliver_index_t)(dIndex), C.uint32_t(indexCap), (*C.halo_dhcp_msg_t)(k.Msgs), C.uint32_t(k.MsgCap),
		(*C.halo_dhcp_summary_t)(k.Summary), k.Workspace, C.uint64_t(k.WorkspaceBytes), nil))
}

// DhcpServer is one NetIf's lease table and state machine. Not safe for concurrent use: the
// reference's DhcpLock is the caller's.
type DhcpServer struct {
	h   *C.halo_dhcp_server_t
	cfg C.halo_dhcp_config_t
}

// NewDhcpServer makes the server object; ip, mask and dns are in IpAddrToU form, capacity is the
// most leases.
func NewDhcpServer(ip, mask, dns uint32, mac [6]byte, serverEnable, clientEnable bool, capacity int) (*DhcpServer, error) {
	b := func(v bool) C.int {
		if v {
			return 1
		}
		return 0
	}
	s := &DhcpServer{cfg: C.gpurx_dhcp_config(C.uint32_t(ip), C.uint32_t(mask), C.uint32_t(dns), (*C.uint8_t)(unsafe.Pointer(&mac[0])),
		b(serverEnable), b(clientEnable), C.uint32_t(capacity))}
	if err := halo(C.halo_dhcp_server_create(&s.cfg, &s.h)); err != nil {
		return nil, err
	}
	return s, nil
}

// Close frees the server object.
func (s *DhcpServer) Close() {
	C.halo_dhcp_server_destroy(s.h)
	s.h = nil
}

// Handle is RxDhcp for every message record, in order: the replies in the order the reference
// would send them, one verdict per message and one event per client ACK.
func (s *DhcpServer) Handle(msgs []DhcpMsg, now uint64) (replies []DhcpReply, verdicts []uint8, events []DhcpClientEvent, err error) {
	n := len(msgs)
	if n == 0 {
		return nil, nil, nil, nil
	}
	replies, verdicts, events = make([]DhcpReply, 2*n), make([]uint8, n), make([]DhcpClientEvent, n)
	var nr, ne C.uint32_t
	err = halo(C.halo_dhcp_handle_msgs(s.h, (*C.halo_dhcp_msg_t)(unsafe.Pointer(&msgs[0])), C.uint32_t(n), C.uint64_t(now),
		(*C.halo_dhcp_reply_t)(unsafe.Pointer(&replies[0])), C.uint32_t(2*n), (*C.uint8_t)(unsafe.Pointer(&verdicts[0])), &nr,
		(*C.halo_dhcp_client_event_t)(unsafe.Pointer(&events[0])), C.uint32_t(n), &ne))
	return replies[:nr], verdicts, events[:ne], err
}

// Leases is ListDhcp, in ascending address order.
func (s *DhcpServer) Leases() []DhcpLease {
	n := int(C.halo_dhcp_list(s.h, nil, 0))
	if n == 0 {
		return nil
	}
	out := make([]DhcpLease, n)
	n = int(C.halo_dhcp_list(s.h, (*C.halo_dhcp_lease_t)(unsafe.Pointer(&out[0])), C.uint32_t(n)))
	return out[:n]
}

// Clear is one DhcpLeaseClear tick: it deletes the leases with now > ExpTime and returns how many.
func (s *DhcpServer) Clear(now uint64) int { return int(C.halo_dhcp_clear(s.h, C.uint64_t(now))) }

// SetDns sets the DNS address the server hands out (a WAN client's ACK copies it there).
func (s *DhcpServer) SetDns(dns uint32) error {
	s.cfg.dns = C.uint32_t(dns)
	return halo(C.halo_dhcp_set_dns(s.h, C.uint32_t(dns)))
}

// Discover is DhcpDiscover with the caller's random xid: it sets the client's transaction id and
// returns the DISCOVER message.
func (s *DhcpServer) Discover(xid [4]byte) (DhcpReply, error) {
	var r DhcpReply
	err := halo(C.halo_dhcp_discover(s.h, (*C.uint8_t)(unsafe.Pointer(&xid[0])), (*C.halo_dhcp_reply_t)(unsafe.Pointer(&r))))
	return r, err
}

// BuildReplies is the host reply build: the payload buffer (len(replies) slots of DhcpSlotBytes)
// and one BuildDesc per reply.
func (s *DhcpServer) BuildReplies(replies []DhcpReply) (payload []byte, descs []BuildDesc, err error) {
	n := len(replies)
	if n == 0 {
		return nil, nil, nil
	}
	payload, descs = make([]byte, n*DhcpSlotBytes), make([]BuildDesc, n)
	err = halo(C.halo_dhcp_reply_build_host(&s.cfg, (*C.halo_dhcp_reply_t)(unsafe.Pointer(&replies[0])), C.uint32_t(n),
		(*C.uint8_t)(unsafe.Pointer(&payload[0])), (*C.halo_tx_build_desc_t)(unsafe.Pointer(&descs[0]))))
	return payload, descs, err
}

// BuildRepliesDevice issues the reply build on the null stream: dReplies is n halo_dhcp_reply_t
// (16-byte aligned), dPayload n * DhcpSlotBytes bytes, dDescs n halo_tx_build_desc_t.
func (s *DhcpServer) BuildRepliesDevice(dReplies unsafe.Pointer, n int, dPayload, dDescs unsafe.Pointer) error {
	return halo(C.halo_dhcp_reply_build_device(&s.cfg, (*C.halo_dhcp_reply_t)(dReplies), C.uint32_t(n), (*C.uint8_t)(dPayload),
		(*C.halo_tx_build_desc_t)(dDescs), nil))
}
