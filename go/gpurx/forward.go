package gpurx

// #include "gpurx_shim.h"
import "C"

import "unsafe"

// The forward and transmit calls (SURVEY.md §8f rows f2-f4) a batched Ipv4RouteForward /
// Tx* would make, on device-resident batches: frames, offsets (u32 dwords), lengths and records in
// HBM, addressed by device pointers. All are asynchronous on the null stream.

// RouteBatch is NetIf.FindRoute -> RouteTable.FindRoute (engine/ipv4_engine.go:351-390) for every
// record's destination: ids index the RouteEntry objects registered with halo_route_update in
// RouteTable.AddRoute order (HALO_ROUTE_NONE / HALO_ROUTE_PANIC as FindRoute's nil / div-by-zero).
func RouteBatch(t *C.halo_route_table_t, dRecords unsafe.Pointer, n int, dIds unsafe.Pointer) error {
	return halo(C.halo_route_lookup_records_device(t, (*C.halo_rx_result_t)(dRecords), C.uint32_t(n),
		(*C.uint32_t)(dIds), nil))
}

// NatKeys is NatWanFlowHash.GetHashCode with NatGetFlowByWan's key normalisation
// (engine/ipv4_engine.go:471-479, :554-581) for every record, and its bucket in a table of nb
// buckets (hashmap/hashmap.go:64), for a caller that keeps NatWanFlowTable in Go and probes its
// buckets without hashing. A NATing interface whose table lives behind halo_nat_table_t does not
// need it: NatLookupWan / NatLookupLan / NatLookupQuote below hash, probe and fill the ops on the
// device, and only new flows come back to the host (halo_nat_resolve_misses, or one item per new
// key through NatCollectMisses / NatResolveItems / NatApplyAnswers).
func NatKeys(dRecords unsafe.Pointer, n int, natType int, dHash, dBucket unsafe.Pointer, nb uint32) error {
	return halo(C.halo_flow_hash_device((*C.halo_rx_result_t)(dRecords), C.uint32_t(n), C.HALO_FLOW_NAT_WAN,
		C.uint32_t(natType), (*C.uint64_t)(dHash), C.uint32_t(nb), (*C.uint32_t)(dBucket), nil))
}

// NatLookupWan is the inbound half of Ipv4RouteForward (engine/ipv4_engine.go:111-130) for every
// record: CheckNatPortMapping(WanToLan) else NatGetFlowByWan on the device copy of t (synced with
// halo_nat_sync_device). A hit ORs HALO_TX_NAT_DST into dOps[i].steps, writes dst_ip / dst_port and
// stamps the flow with now; dVerdict[i] is HALO_NAT_V_*, dRef[i] the flow id or mapping index, and
// *dMissCount (zeroed by the caller) counts the HALO_NAT_V_MISS records. dSkip (optional) is
// DeepNat's dApplied.
func NatLookupWan(t *C.halo_nat_table_t, dRecords unsafe.Pointer, n int, now uint32, dSkip, dOps, dVerdict, dRef,
	dMissCount unsafe.Pointer) error {
	return halo(C.halo_nat_lookup_wan_device(t, (*C.halo_rx_result_t)(dRecords), C.uint32_t(n), C.uint32_t(now),
		(*C.uint8_t)(dSkip), (*C.halo_tx_op_t)(dOps), (*C.uint8_t)(dVerdict), (*C.uint32_t)(dRef),
		(*C.uint32_t)(dMissCount), nil))
}

// NatLookupLan is the outbound half (engine/ipv4_engine.go:203-225) on the out-interface's table:
// CheckNatPortMapping(LanToWan) else NatGetFlowByHash; a hit ORs HALO_TX_NAT_SRC and writes src_ip /
// src_port. A miss is a new flow: copy the MISS records back and run halo_nat_resolve_misses, which
// calls NatAddFlow in packet order, or take the miss path below, which leaves the batch in HBM.
func NatLookupLan(t *C.halo_nat_table_t, dRecords unsafe.Pointer, n int, now uint32, dSkip, dOps, dVerdict, dRef,
	dMissCount unsafe.Pointer) error {
	return halo(C.halo_nat_lookup_lan_device(t, (*C.halo_rx_result_t)(dRecords), C.uint32_t(n), C.uint32_t(now),
		(*C.uint8_t)(dSkip), (*C.halo_tx_op_t)(dOps), (*C.uint8_t)(dVerdict), (*C.uint32_t)(dRef),
		(*C.uint32_t)(dMissCount), nil))
}

// The miss path: what halo_nat_resolve_misses does for a batch, with records, verdicts and ops left
// in HBM. NatCollectMisses lists the records NatLookupLan / NatLookupWan left as HALO_NAT_V_MISS,
// once per key and in packet order; the caller copies *dCount and that many items to the host,
// NatResolveItems runs CheckNatPortMapping / the flow lookup / NatAddFlow on each, the caller copies
// the answers back, and NatApplyAnswers writes them into dOps / dVerdict / dRef of every record of a
// listed key. A new flow's first packets then leave with their SNAT in the batch that created it.

// NatMissWorkspace is the device scratch NatCollectMisses needs for n records (scratchLog2 0:
// automatic).
func NatMissWorkspace(n int, scratchLog2 uint32) uint64 {
	return uint64(C.halo_nat_miss_workspace(C.uint32_t(n), C.uint32_t(scratchLog2)))
}

// NatCollectMisses: dir is HALO_FLOW_NAT_LAN or HALO_FLOW_NAT_WAN; dSelect (optional, one byte per
// record) narrows the MISS records, e.g. to the packets whose TTL survives; dItems receives up to
// itemCap halo_nat_miss_item_t, *dCount the number listed, dPos[i] the list position of record i's
// key (HALO_NAT_NO_FLOW where not selected).
func NatCollectMisses(t *C.halo_nat_table_t, dir uint32, dRecords, dVerdict, dSelect unsafe.Pointer, n int,
	scratchLog2 uint32, dItems unsafe.Pointer, itemCap int, dCount, dPos, dWs unsafe.Pointer, wsBytes uint64) error {
	return halo(C.halo_nat_collect_misses_device(t, C.uint32_t(dir), (*C.halo_rx_result_t)(dRecords),
		(*C.uint8_t)(dVerdict), (*C.uint8_t)(dSelect), C.uint32_t(n), C.uint32_t(scratchLog2),
		(*C.halo_nat_miss_item_t)(dItems), C.uint32_t(itemCap), (*C.uint32_t)(dCount), (*C.uint32_t)(dPos), dWs,
		C.uint64_t(wsBytes), nil))
}

// NatCollectMissesCompact is NatCollectMisses over halo_rx_record16_t records.
func NatCollectMissesCompact(t *C.halo_nat_table_t, dir uint32, dRecords, dVerdict, dSelect unsafe.Pointer, n int,
	scratchLog2 uint32, dItems unsafe.Pointer, itemCap int, dCount, dPos, dWs unsafe.Pointer, wsBytes uint64) error {
	return halo(C.halo_nat_collect_misses_compact_device(t, C.uint32_t(dir), (*C.halo_rx_record16_t)(dRecords),
		(*C.uint8_t)(dVerdict), (*C.uint8_t)(dSelect), C.uint32_t(n), C.uint32_t(scratchLog2),
		(*C.halo_nat_miss_item_t)(dItems), C.uint32_t(itemCap), (*C.uint32_t)(dCount), (*C.uint32_t)(dPos), dWs,
		C.uint64_t(wsBytes), nil))
}

// NatResolveItems answers k listed items (host memory) in order on the authoritative table and
// returns the number of flows NatAddFlow created.
func NatResolveItems(t *C.halo_nat_table_t, dir uint32, items unsafe.Pointer, k int, now uint32,
	answers unsafe.Pointer) (int, error) {
	var added C.uint32_t
	err := halo(C.halo_nat_resolve_items(t, C.uint32_t(dir), (*C.halo_nat_miss_item_t)(items), C.uint32_t(k),
		C.uint32_t(now), (*C.halo_nat_answer_t)(answers), &added))
	return int(added), err
}

// NatApplyAnswers writes the k answers (device memory, 16-byte aligned) into the ops, verdicts and
// refs of the records whose dPos is below k; dCounts (optional, HALO_NAT_V_DROP+1 u32) is incremented
// per verdict. A record the host answered HALO_NAT_V_DROP must not be transmitted.
func NatApplyAnswers(dir uint32, dPos unsafe.Pointer, n int, dAnswers unsafe.Pointer, k int, dOps, dVerdict, dRef,
	dCounts unsafe.Pointer) error {
	return halo(C.halo_nat_apply_answers_device(C.uint32_t(dir), (*C.uint32_t)(dPos), C.uint32_t(n),
		(*C.halo_nat_answer_t)(dAnswers), C.uint32_t(k), (*C.halo_tx_op_t)(dOps), (*C.uint8_t)(dVerdict),
		(*C.uint32_t)(dRef), (*C.uint32_t)(dCounts), nil))
}

// NatLookupQuote is IcmpTtlDeepNat's NatGetFlowByWan (engine/icmp_engine.go:75-82) between DeepNat's
// two calls: dQuote is what the first call wrote, dNat what the second call reads.
func NatLookupQuote(t *C.halo_nat_table_t, dQuote unsafe.Pointer, n int, dNat unsafe.Pointer) error {
	return halo(C.halo_nat_lookup_quote_device(t, (*C.halo_rx_result_t)(dQuote), C.uint32_t(n),
		(*C.halo_tx_deep_nat_t)(dNat), nil))
}

// ParseWithNatKeys is the receive parse and NatKeys in one pass over the frames (records equal to
// the plain parse's; the keys are hashed before the records leave registers).
func ParseWithNatKeys(dFrames, dOffsets, dLens unsafe.Pointer, n int, netif *NetIfCfg, dOut, dHash, dBucket unsafe.Pointer,
	natType int, nb uint32) error {
	nif, err := netif.c()
	if err != nil {
		return err
	}
	return halo(C.halo_rx_parse_flow_batch_device((*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets),
		(*C.uint16_t)(dLens), C.uint32_t(n), csumFlag(), &nif, 0, (*C.halo_rx_result_t)(dOut), nil,
		C.HALO_FLOW_NAT_WAN, C.uint32_t(natType), (*C.uint64_t)(dHash), C.uint32_t(nb), (*C.uint32_t)(dBucket), nil))
}

// Rewrite is NatChangeDst / HandleIpv4PktTtl / NatChangeSrc / ReCalc* and eth_tx's checksum fill
// (protocol/ipv4.go:134-302, cgo/dpdk.c:333-365) for every frame, in place, in Ipv4RouteForward's
// order; dOps holds one halo_tx_op_t per frame (the addresses and ports the NAT tables resolved).
func Rewrite(dFrames, dOffsets, dLens, dOps, dResult unsafe.Pointer, n int, maxLen uint32) error {
	return halo(C.halo_tx_fixup_batch_device((*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets), (*C.uint16_t)(dLens),
		C.uint32_t(n), (*C.halo_tx_op_t)(dOps), csumFlag(), C.uint32_t(maxLen), (*C.uint8_t)(dResult), nil))
}

// BuildBatch is TxUdp / TxTcp / TxIcmp -> TxIpv4 -> TxEthernet for n descriptors
// (halo_tx_build_desc_t); iphId lives in device memory (dIphId, u16) and advances by the number
// of packets built, in descriptor order (protocol/ipv4.go:33,89-131).
func BuildBatch(dDesc unsafe.Pointer, n int, dPayload unsafe.Pointer, srcMac []byte, dFrames unsafe.Pointer,
	stride int, dLens, dResult, dIphId, dWs unsafe.Pointer, wsBytes uint64, maxPayload uint32) error {
	netif := NetIfCfg{MacAddr: srcMac, IpAddr: []byte{0, 0, 0, 0}}
	nif, err := netif.c()
	if err != nil {
		return err
	}
	return halo(C.halo_tx_build_batch_device((*C.halo_tx_build_desc_t)(dDesc), C.uint32_t(n), (*C.uint8_t)(dPayload),
		csumFlag(), &nif, C.uint32_t(maxPayload), (*C.uint8_t)(dFrames), C.uint32_t(stride), (*C.uint16_t)(dLens),
		(*C.uint8_t)(dResult), (*C.uint16_t)(dIphId), dWs, C.uint64_t(wsBytes), nil))
}

// BuildWorkspace is the device scratch BuildBatch needs for n descriptors.
func BuildWorkspace(n int) uint64 { return uint64(C.halo_tx_build_workspace(C.uint32_t(n))) }

// DeepNat is IcmpTtlDeepNat (engine/icmp_engine.go:55-86) for a batch: with dNat == nil it writes
// the quote records (NatGetFlowByWan's arguments; look them up with NatLookupQuote), then, called
// again with the lookups' results, rewrites the frames in place.
func DeepNat(dFrames, dOffsets, dLens, dNat, dQuote, dApplied unsafe.Pointer, n int) error {
	return halo(C.halo_tx_icmp_deep_nat_batch_device((*C.uint8_t)(dFrames), (*C.uint32_t)(dOffsets),
		(*C.uint16_t)(dLens), C.uint32_t(n), (*C.halo_tx_deep_nat_t)(dNat), csumFlag(),
		(*C.halo_rx_result_t)(dQuote), (*C.uint8_t)(dApplied), nil))
}
