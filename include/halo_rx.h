/*
 * halo_rx.h — C ABI of the MI355X-native receive parse-and-checksum engine.
 *
 * This is the drop-in boundary for halo's software receive path.
 * The reference has no FFI on this path: the parsers are plain Go functions that
 * engine.(*NetIf).PacketHandle calls once per frame. This ABI replaces that per-frame
 * chain with one call per BATCH of frames:
 *
 *   reference (one frame at a time)                       replaced by
 *   -----------------------------------------------------  -------------------------------
 *   protocol.ParseEthFrm        protocol/ethernet.go:29-55 \
 *   protocol.ParseIpv4Pkt       protocol/ipv4.go:48-86      |
 *   protocol.ParseUdpPkt        protocol/udp.go:21-49       |  halo_rx_parse_batch_device()
 *   protocol.ParseTcpPkt        protocol/tcp.go:36-70       |  halo_rx_parse_strided_device()
 *   protocol.ParseIcmpPkt       protocol/icmp.go:33-63      |  (one halo_rx_result_t per frame)
 *   protocol.GetCheckSum        protocol/utils.go:11-31     |
 *   protocol.NatGetSrcDstPort   protocol/ipv4.go:229-246    |
 *   protocol.IpAddrToU          protocol/utils.go:34-44    /
 *   protocol.CheckSumEnable     protocol/utils.go:8         -> HALO_RX_CSUM_ENABLE bit of `flags`
 *   NetIf.RxEthernet filter     engine/ethernet_engine.go:22 -> HALO_RX_F_MAC_MATCH
 *   NetIf.RxIpv4 branch inputs  engine/ipv4_engine.go:24,31  -> HALO_RX_F_IP_BCAST / _DST_IS_OWN
 *   NetIf.PacketHandle loop     engine/engine.go:339-385    -> halo_rx_parse_batch_host() (pinned H2D,
 *                                                              kernel, D2H) + halo_rx_dispatch()
 *
 * Conventions (SURVEY.md §8b "Error convention"):
 *   - Every entry point returns int: 0 (HALO_OK) or a negative HALO_E_* code. A malformed
 *     frame is DATA (its status code in halo_rx_result_t), never a call failure.
 *   - The caller owns every buffer. No globals: `flags` replaces protocol.CheckSumEnable.
 *   - Calls are thread-safe per (device, stream).
 *   - There is no CPU fallback: without a gfx950 device every compute entry point
 *     returns HALO_E_NODEV / HALO_E_ARCH. The CPU entry point SURVEY.md §8b also lists,
 *     halo_rx_parse_batch_cpu, is a separate library a caller picks by name
 *     (include/halo_rx_cpu.h, libhalo_rx_cpu.so); nothing here calls it.
 *
 * Frame layout in device memory (DESIGN.md "Data layout in HBM"):
 *   - ragged:  frame i starts at bytes + 4*offsets_dw[i] (4-byte aligned starts, as the
 *              reference's ring records are: mem/ring_buffer.go:47-50) and is lens[i] bytes
 *              long. u32 dword offsets address 16 GiB per call.
 *   - strided: frame i starts at bytes + i*stride (stride a multiple of 4), length
 *              lens[i] or, when lens == NULL, the uniform length `len`.
 *   Read contract: no kernel reads a 4 KB page that holds no byte of a frame of the call, so the
 *   frames may sit in several allocations (or around unmapped holes) addressed from one base.
 *   The per-frame kernels never read past the 4-byte word holding a frame's last byte; the
 *   byte-stream kernel (HALO_RX_VARIANT_STREAM) reads whole 16-byte-aligned blocks between a
 *   window's (64 consecutive frames') lowest and highest frame bytes only when every page of
 *   that range holds a frame byte, and otherwise sums that window frame by frame. Bytes between
 *   frames that it does read never enter a record.
 */
#ifndef HALO_RX_H
#define HALO_RX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define HALO_API __attribute__((visibility("default")))
#else
#define HALO_API
#endif

/* ---- return codes ------------------------------------------------------------------ */
#define HALO_OK 0
#define HALO_E_INVAL (-1)   /* bad argument (null pointer, bad stride/flags)              */
#define HALO_E_NODEV (-2)   /* no HIP device / device index out of range                  */
#define HALO_E_ARCH (-3)    /* device is not gfx950 (MI355X)                              */
#define HALO_E_HIP (-4)     /* a HIP runtime call or kernel launch failed                 */
#define HALO_E_NOMEM (-5)   /* device or pinned host allocation failed                    */
#define HALO_E_RANGE (-6)   /* batch too large for the addressing mode                    */

/* ---- flags (replaces the protocol.CheckSumEnable package global, protocol/utils.go:8) - */
#define HALO_RX_CSUM_ENABLE 0x1u /* verify IPv4 header + UDP/TCP checksums (ICMP: always)  */
#define HALO_RX_JUMBO_EXT 0x2u   /* build-defined extension: lift the 1514/1500/1480 caps   */
                                 /* to 9014/9000/8980 (MTU 9000); arithmetic unchanged      */
#define HALO_RX_RECORD_COMPACT 0x4u /* write halo_rx_record16_t (16 B) instead of            */
                                    /* halo_rx_result_t (32 B); device entry points and      */
                                    /* halo_rx_parse_batch_cpu (include/halo_rx_cpu.h) only  */
#define HALO_RX_UNIFORM_LEN 0x8u    /* ragged batch whose frames all have length max_len_hint */
                                    /* (a speed hint: picks the uniform-length kernel table)  */
/* Every buffer starts at its IPv4 header: the packets of a NetIf's LoChan, which
 * PacketHandle drains every 99 polls through ParseIpv4Pkt -> own-address filter -> local
 * Rx{Icmp,Udp,Tcp} (engine/engine.go:353-381; fed by TxIpv4's loopback copy,
 * engine/ipv4_engine.go:72-79). The record is the one of the Ethernet chain minus its
 * Ethernet layer: ParseIpv4Pkt's own length check (len<20 || len>1500, ipv4.go:49) is the
 * first check and can fail (HALO_RX_IP_LEN); ethertype is 0x0800 (the channel carries IPv4
 * only); MAC_MATCH is never set; payload_off is in packet coordinates (IPv4 payload at 20,
 * UDP/ICMP payload at 28, TCP at 20 + headerLen) and 0/0 when ParseIpv4Pkt fails;
 * NatGetSrcDstPort's ports are 0 for packets shorter than 26 B (ipv4.go:230). Map the records
 * to the drain's decisions with halo_rx_dispatch_loopback. Ragged device and host entry
 * points only (halo_rx_parse_batch_device / _host); not with the fused passes or strided
 * layouts (HALO_E_INVAL).                                                                   */
#define HALO_RX_L3_START 0x10u
/* Per-call kernel variant (tuning and tests; results are identical for every value, only speed
 * changes): flags |= HALO_RX_VARIANT_x << HALO_RX_VARIANT_SHIFT. AUTO picks from max_len_hint /
 * the uniform length; LANE = one lane per frame; G4/G8/G16 = that many lanes per frame; MIX =
 * the size-class kernel (each wave sorts 256 frames by size and runs lane-per-frame, 4-, 8- and
 * 16-lane passes); STREAM = the byte-stream kernel (one frame header per lane, every L4
 * segment summed from one coalesced pass over the window's bytes). Device parse entry points
 * only.                                                                                     */
#define HALO_RX_VARIANT_SHIFT 8
#define HALO_RX_VARIANT_MASK 0x700u
#define HALO_RX_VARIANT_AUTO 0u
#define HALO_RX_VARIANT_LANE 1u
#define HALO_RX_VARIANT_G4 2u
#define HALO_RX_VARIANT_G8 3u
#define HALO_RX_VARIANT_G16 4u
#define HALO_RX_VARIANT_MIX 5u
#define HALO_RX_VARIANT_STREAM 6u

/* ---- per-frame status: the FIRST failing check in reference order, 0 = OK ---------- */
typedef enum halo_rx_status {
    HALO_RX_OK = 0,
    HALO_RX_ETH_LEN = 1,              /* len<42 || len>1514        protocol/ethernet.go:31    */
    HALO_RX_ETH_TYPE = 2,             /* EtherType not whitelisted protocol/ethernet.go:39-50 */
    HALO_RX_IP_LEN = 3,               /* len<20 || len>1500        protocol/ipv4.go:49        */
    HALO_RX_IP_VER = 4,               /* pkt[0] != 0x45            protocol/ipv4.go:52        */
    HALO_RX_IP_FRAG = 5,              /* flags/offset not DF|0     protocol/ipv4.go:59        */
    HALO_RX_IP_PROTO = 6,             /* proto not ICMP/TCP/UDP    protocol/ipv4.go:63-72     */
    HALO_RX_IP_HDR_CKSUM = 7,         /* GetCheckSum(hdr) != 0     protocol/ipv4.go:74-78     */
    HALO_RX_IP_TOTLEN_UNDERFLOW = 8,  /* totalLen < 20: Go panics  protocol/ipv4.go:84 (build-defined) */
    HALO_RX_IP_TOTLEN_OVERRUN = 9,    /* totalLen > len(pkt): Go reads stale bytes or panics (build-defined) */
    HALO_RX_L4_LEN = 10,              /* udp.go:22 / tcp.go:37 / icmp.go:34                   */
    HALO_RX_ICMP_TYPE = 11,           /* type not 8/0/11           protocol/icmp.go:38-47     */
    HALO_RX_ICMP_CODE = 12,           /* code != 0                 protocol/icmp.go:49        */
    HALO_RX_L4_CKSUM = 13,            /* udp.go:42 / tcp.go:54 / icmp.go:53                   */
    HALO_RX_STATUS_COUNT = 14
} halo_rx_status_t;

/* ---- per-frame flags: what engine/{ethernet,ipv4}_engine.go branch on ---------------- */
#define HALO_RX_F_MAC_MATCH 0x01u  /* dst MAC == own || broadcast   engine/ethernet_engine.go:22 */
#define HALO_RX_F_IP_BCAST 0x02u   /* dst IP byte 3 == 255           engine/ipv4_engine.go:24     */
#define HALO_RX_F_DST_IS_OWN 0x04u /* dst IP == own IP               engine/ipv4_engine.go:31     */

/* ---- per-frame result record (32 B, written once per frame) ---------------------------
 * Each field is the output of the reference layer that produced it, filled only when that
 * layer returned without error (Go returns zero values / nil slices on error):
 *   ethertype     ParseEthFrm ethProto (0xFFFF on error: ETH_PROTO_UNKNOWN)
 *   ip_proto      ParseIpv4Pkt ipHeadProto (0xFF when not IPv4 or on error: IPH_PROTO_UNKNOWN)
 *   src_ip/dst_ip IpAddrToU(srcAddr/dstAddr)   (0 when ParseIpv4Pkt did not succeed)
 *   ip_total_len  IPv4 totalLen field           (0 when ParseIpv4Pkt did not succeed)
 *   sport/dport   NatGetSrcDstPort(ethPayload)  (ICMP: echo id twice; 0 when IP failed)
 *   l4_aux        TCP flags (tcp.go:50) or ICMP type (icmp.go:38)   (0 unless L4 succeeded)
 *   l4_seq        TCP seqNum, or ICMP id<<16 | seq                   (0 unless L4 succeeded)
 *   l4_ack        TCP ackNum                                         (0 unless L4 succeeded)
 *   payload_off/payload_len  the innermost successfully returned payload slice, in frame
 *                 coordinates: Ethernet frm[14:], IPv4 pkt[20:totalLen], UDP pkt[8:],
 *                 TCP pkt[headerLen:] (headerLen = data-offset nibble used as BYTES,
 *                 protocol/tcp.go:49,68), ICMP pkt[8:]. 0/0 on an Ethernet error.
 * The kernel evaluates the L4 parser selected by ip_proto for EVERY IPv4 frame; which of
 * those verdicts the reference engine would actually have evaluated follows from `flags`
 * (see halo_rx_dispatch).                                                               */
typedef struct halo_rx_result {
    uint8_t status;        /* halo_rx_status_t */
    uint8_t flags;         /* HALO_RX_F_*      */
    uint16_t ethertype;
    uint8_t ip_proto;
    uint8_t l4_aux;
    uint16_t ip_total_len;
    uint32_t src_ip;
    uint32_t dst_ip;
    uint16_t sport;
    uint16_t dport;
    uint16_t payload_off;
    uint16_t payload_len;
    uint32_t l4_seq;
    uint32_t l4_ack;
} halo_rx_result_t;

/* ---- compact per-frame record (16 B; flags |= HALO_RX_RECORD_COMPACT) ------------------
 * The verdict and the extracted 5-tuple only: the fields of halo_rx_result_t named the same,
 * with the EtherType folded into flags bits 4-5 (HALO_RX_F_ET_*; the EtherType is 0xFFFF when
 * status is HALO_RX_ETH_LEN or HALO_RX_ETH_TYPE, whatever those bits hold).                */
#define HALO_RX_F_ET_SHIFT 4
#define HALO_RX_F_ET_IPV4 0x00u    /* 0x0800 */
#define HALO_RX_F_ET_ARP 0x10u     /* 0x0806 */
#define HALO_RX_F_ET_IPV6 0x20u    /* 0x86DD */
#define HALO_RX_F_ET_8023 0x30u    /* 0x05DC */
typedef struct halo_rx_record16 {
    uint8_t status;
    uint8_t flags;     /* HALO_RX_F_* | HALO_RX_F_ET_* */
    uint8_t ip_proto;
    uint8_t l4_aux;
    uint32_t src_ip;
    uint32_t dst_ip;
    uint16_t sport;
    uint16_t dport;
} halo_rx_record16_t;

/* ---- the interface a frame is received on (engine.NetIfConfig, engine/engine.go:65-81) - */
typedef struct halo_rx_netif {
    uint8_t mac[6];  /* NetIf.MacAddr                              */
    uint8_t pad[2];
    uint32_t ip;     /* IpAddrToU(NetIf.IpAddr), host integer      */
    uint32_t nat_enable; /* NetIfConfig.NatEnable (only halo_rx_dispatch reads it) */
} halo_rx_netif_t;

typedef void* halo_stream_t; /* a hipStream_t (NULL = the device's null stream) */

/* ---- device / library -------------------------------------------------------------- */
HALO_API const char* halo_rx_version(void);
/* Selects `device` for the calling thread, checks that it is a gfx950 part and makes the device's
 * status-histogram trees (8.7 MB, zeroed, kept for the life of the process): call it before
 * capturing histogram-on parses in a hipGraph, since a capture cannot allocate (such a call
 * returns HALO_E_NOMEM when the trees were never made). A failure to make the trees does not fail
 * this call: the next histogram-on call outside a capture tries again. Idempotent. */
HALO_API int halo_rx_init(int device);
/* Waits for all work on `device` the way hipDeviceSynchronize does, after stopping this library's
 * resident consumers on it (rings attached with HALO_RING_PERSISTENT, host contexts with
 * halo_rx_host_ctx_set_resident). A caller's own hipDeviceSynchronize / torch.cuda.synchronize()
 * waits for those kernels too, and they end only 20 ms after their last request (never, while
 * another thread keeps them busy); this call does not. The consumers restart on their next request.
 * Like hipDeviceSynchronize on ROCm 7, it does NOT wait for the per-thread stream
 * (hipStreamPerThread) of a host thread that has already exited: synchronise that stream on its
 * own thread before the thread ends. */
HALO_API int halo_rx_device_synchronize(int device);
/* Drains `device` (as halo_rx_device_synchronize) and hands back every status-histogram tree key,
 * so that the HSA queues of streams destroyed since no longer hold trees (64 keys per device; a
 * queue that finds none left counts straight into the caller's counters, exact but ~9x slower at
 * 1M frames). The trees themselves stay: graphs captured with histogram-on parses remain valid and
 * count exactly when replayed after this call. Rings, contexts and route tables stay valid. Must
 * not run while another thread launches parses on `device`. */
HALO_API int halo_rx_release(int device);
/* TESTING ONLY — the histogram tree keys of `device`. op 0: returns how many keys HSA queues have
 * claimed (>= 0); op 1: poisons every key (every histogram-on launch takes the fallback); op 2:
 * occupies all keys but `arg` (<= 64) with ids no queue has; op 3: frees every key as
 * halo_rx_release does. Ops 1-3 drain the device first and must not run alongside parses. */
HALO_API int halo_rx_debug_hist_keys(int device, int op, uint32_t arg);
HALO_API const char* halo_rx_strerror(int code);
HALO_API const char* halo_rx_status_name(int status);

/* ---- device-resident batch parse (the hot path) --------------------------------------
 * All pointers are device pointers. `d_out` receives n records (halo_rx_result_t, or
 * halo_rx_record16_t with HALO_RX_RECORD_COMPACT; 16-byte aligned). `d_status_hist`, if not
 * NULL, receives HALO_RX_STATUS_COUNT u32 counters that are INCREMENTED (the caller
 * zeroes them). `max_len_hint` (a bound on every frame's length; 0 = unknown) selects the
 * lanes-per-frame variant; with HALO_RX_UNIFORM_LEN every frame has exactly that length.
 * Asynchronous on `stream`.                                                              */
HALO_API int halo_rx_parse_batch_device(const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                        const uint16_t* d_lens, uint32_t n, uint32_t flags,
                                        const halo_rx_netif_t* netif, uint32_t max_len_hint,
                                        halo_rx_result_t* d_out, uint32_t* d_status_hist,
                                        halo_stream_t stream);

HALO_API int halo_rx_parse_strided_device(const uint8_t* d_bytes, uint64_t stride,
                                          const uint16_t* d_lens, uint32_t len, uint32_t n,
                                          uint32_t flags, const halo_rx_netif_t* netif,
                                          halo_rx_result_t* d_out, uint32_t* d_status_hist,
                                          halo_stream_t stream);

/* ---- several device-resident batches in one launch ------------------------------------
 * The reference's receive loop is an unbounded stream of polls (engine/engine.go:344-351); a
 * caller holding K ragged batches at once (consecutive batches of one queue, or the batches of
 * several NetIf queues) hands them over together. Each batch keeps its own arrays and records,
 * exactly as K halo_rx_parse_batch_device calls on `stream` would produce them; the status
 * histogram (optional) counts all of them. With frames of at most 64 B (max_len_hint 1..64, or
 * HALO_RX_VARIANT_LANE) the K batches run as ONE grid of lane-per-frame waves, so the launch ramp
 * and tail are paid once per K batches instead of once per batch; larger frames take one launch
 * per batch. k <= 32; `batches` is a host array read during the call; batches with n = 0 are
 * skipped. Flags as halo_rx_parse_batch_device (HALO_RX_L3_START included). Asynchronous.   */
typedef struct halo_rx_batch_desc {
    const uint8_t* d_bytes;
    const uint32_t* d_offsets_dw;
    const uint16_t* d_lens;
    halo_rx_result_t* d_out; /* n records (or halo_rx_record16_t), 16-byte aligned */
    uint32_t n;
    uint32_t pad;
} halo_rx_batch_desc_t;    /* 40 B */
HALO_API int halo_rx_parse_batches_device(const halo_rx_batch_desc_t* batches, uint32_t k, uint32_t flags,
                                          const halo_rx_netif_t* netif, uint32_t max_len_hint,
                                          uint32_t* d_status_hist, halo_stream_t stream);

/* ---- host-memory batch parse -----------------------------------
 * Frames in HOST memory (any alignment, ragged byte offsets). Stages them into pinned
 * buffers, copies H2D, runs the kernel and copies results D2H, double-buffered in chunks
 * of `chunk_frames` (0 = default). Synchronous: returns when `out` is filled.           */
typedef struct halo_rx_host_ctx halo_rx_host_ctx_t;
HALO_API int halo_rx_host_ctx_create(int device, uint32_t chunk_frames, uint64_t chunk_bytes,
                                     halo_rx_host_ctx_t** ctx);
HALO_API int halo_rx_host_ctx_destroy(halo_rx_host_ctx_t* ctx);
HALO_API int halo_rx_parse_batch_host(halo_rx_host_ctx_t* ctx, const uint8_t* bytes,
                                      const uint64_t* offsets, const uint16_t* lens, uint32_t n,
                                      uint32_t flags, const halo_rx_netif_t* netif,
                                      halo_rx_result_t* out, uint32_t* status_hist);
/* Frames whose offsets are 4-byte aligned relative to each other and that lie inside one live
 * registration (halo_rx_host_register, or a ring attached with HALO_RING_REGISTER) are parsed
 * in place: the kernel reads them over PCIe, no staging copy (zero-copy mode, the default), and
 * writes the records straight into `out` when `out` is registered as well. Otherwise frames
 * whose offsets are ascending and relatively aligned (a drained ring segment, a packed batch)
 * are sent with one DMA per chunk straight from `bytes`, and other batches are repacked into
 * pinned staging by the CPU. halo_rx_host_ctx_set_zero_copy(ctx, 0) keeps registered batches
 * on the DMA path. Registered memory must stay registered until the call returns.         */
HALO_API int halo_rx_host_ctx_set_zero_copy(halo_rx_host_ctx_t* ctx, int enable);
/* Resident consumer for small batches (the latency path of a batched PacketHandle: EthRxFunc polls
 * gathered into batches of a few frames to a few thousand, engine/engine.go:339-385, and of the
 * single-frame Parse* wrappers an Ipv4PktFwdHook calls, engine/engine.go:132). Batches of at most
 * `max_frames` frames (<= 16384; 0 turns the path off) whose frames fit `max_bytes` of staging
 * (0: min(1516 * max_frames, 64 MiB); at most 64 MiB) are copied into pinned staging this context
 * owns, and a kernel resident on 8 CUs — waiting on a control block in pinned memory — parses them
 * there and writes the records into `out` (directly when `out` lies in a live registration): no
 * launch and no stream synchronisation per call. The kernel leaves 20 ms after its last request and
 * the next call relaunches it; a device drain (halo_rx_host_unregister, a ring detach, a route sync)
 * stops it first and serves calls by launches until the drain is over. Same records as the chunked
 * path. Larger batches take the chunked path. */
HALO_API int halo_rx_host_ctx_set_resident(halo_rx_host_ctx_t* ctx, uint32_t max_frames, uint64_t max_bytes);
/* Bounds the wait for one resident request (default 2 s; 0 restores it). A request that times out
 * is retired before the call returns HALO_E_HIP: the consumer is stopped and its kernel has ended,
 * so nothing is written into the caller's arrays afterwards. (Diagnostics and fault injection.) */
HALO_API int halo_rx_host_ctx_set_service_timeout(halo_rx_host_ctx_t* ctx, uint64_t us);
typedef struct halo_rx_host_stats {
    uint64_t calls;            /* halo_rx_parse_batch_host calls with frames                     */
    uint64_t frames;           /* frames parsed                                                   */
    uint64_t resident_calls;   /* calls served on the resident path                              */
    uint64_t resident_parked;  /* resident calls served by a launch while a device drain ran     */
    uint64_t service_launches; /* resident consumer launches (first use, after idle exits)       */
    uint64_t pack_ns;          /* resident path: host time packing frames into pinned staging    */
    uint64_t wait_ns;          /* resident path: request to completion                            */
    uint64_t service_gpu_ns;   /* resident consumer: GPU time per request (first group in to last
                                  group out), summed                                              */
} halo_rx_host_stats_t;
HALO_API int halo_rx_host_ctx_get_stats(const halo_rx_host_ctx_t* ctx, halo_rx_host_stats_t* out);
/*
 * Registration pins whole pages, so the library enforces: `ptr` page-aligned and `bytes` a
 * multiple of the page size (hugepages, mmap regions; halo_amd._lib.host_array in Python), and
 * no page shared with a live registration (this call's or a ring's) — otherwise HALO_E_INVAL,
 * before any HIP call. Unregister before the memory is freed: `ptr` must be the base of a live
 * registration made here (else HALO_E_INVAL); the call first waits for all work this library
 * queued on every device it used, then unregisters and checks that the runtime no longer maps
 * the range (HALO_E_HIP if it still does: keep the memory allocated then).                 */
HALO_API int halo_rx_host_register(const void* ptr, uint64_t bytes);
HALO_API int halo_rx_host_unregister(const void* ptr);
/* Live registrations (halo_rx_host_register + rings attached with HALO_RING_REGISTER). The
 * second form also copies up to `cap` (base, bytes) pairs, in address order; either array may
 * be NULL. Both return the total count. */
HALO_API uint32_t halo_rx_host_registered_count(void);
HALO_API uint32_t halo_rx_host_registrations(void** bases, uint64_t* bytes, uint32_t cap);

/* Multi-GPU host batch: frames [0, n) are split into n_ctx contiguous index
 * ranges balanced by bytes; ctxs[k] (one host context per device, or several on one device)
 * parses range k on its own host thread with halo_rx_parse_batch_host. Records land in out[i]
 * in frame order; `status_hist` gets the sum. No data crosses devices, no collective.
 * `shard_first` (optional, n_ctx + 1 entries) receives the range boundaries.              */
HALO_API int halo_rx_shard_multi(halo_rx_host_ctx_t* const* ctxs, uint32_t n_ctx, const uint8_t* bytes,
                                 const uint64_t* offsets, const uint16_t* lens, uint32_t n, uint32_t flags,
                                 const halo_rx_netif_t* netif, halo_rx_result_t* out, uint32_t* status_hist,
                                 uint32_t* shard_first);

/* ---- halo's SPSC packet ring as the batch source --------------------
 * The ring is the reference's own shared-memory layout (mem/ring_buffer.go:18-26 =
 * cgo/ring_buffer.h:20-55): a 128-byte header (head @0, layout version 1 @8, tail @64,
 * size @72, mask @80, buffer @88) followed by a power-of-two data area of records
 * `u32 len` + bytes, each padded to 4 bytes (mem/ring_buffer.go:47-50). The DPDK lcore
 * (cgo/dpdk.c:280-307) or engine.Wire.Tx (engine/engine.go:548-553) is the producer.
 *
 * A consumer replaces the per-record ReadPacket (mem/ring_buffer.go:298-352) + EthRxFunc +
 * RxEthernet loop: each poll takes every record between its cursor and the producer's head
 * (at most max_bytes / max_frames) and returns one record per frame, exactly the frames and
 * the order repeated ReadPacket(buf[capacity]) calls would return. The span goes to HBM raw,
 * record boundaries are found on the GPU, the frames are parsed where they lie; the host only
 * reads `head` and, on commit, writes `tail` (release), as ReadPacket does.              */
#define HALO_RING_STOP_EMPTY 0u      /* every record in the span was taken (usedSpace < 4)        */
#define HALO_RING_STOP_BAD_LEN 1u    /* record length 0 or > size/2: ReadPacket returns false     */
#define HALO_RING_STOP_PARTIAL 2u    /* next record not wholly in the span (usedSpace < totalSize;
                                        also when max_bytes cut it)                              */
#define HALO_RING_STOP_CAPACITY 3u   /* record longer than the receive buffer (len(data)):
                                        ReadPacket leaves it, and the tail, in place              */
#define HALO_RING_STOP_MAX 4u        /* max_frames taken, more records available                  */
#define HALO_RING_STOP_BAD_CURSOR 5u /* head - tail > size: ReadPacket returns false              */
#define HALO_RING_REGISTER 0x1u      /* attach: hipHostRegister the ring for full-rate DMA. The ring
                                        must start on a page boundary; the whole pages through the end
                                        of its data area are registered and must not be shared with
                                        another live registration (HALO_E_INVAL; see
                                        halo_rx_host_register)                                      */
#define HALO_RING_PERSISTENT 0x2u    /* attach (with HALO_RING_REGISTER): small polls of up to 16384
                                        frames are served by a resident consumer kernel (8
                                        workgroups, one per CU) that waits on a control block in
                                        pinned memory: a poll writes a request and spins on its
                                        completion, with no kernel launch and no stream
                                        synchronisation. The kernel exits after 20 ms without a
                                        request (the next poll relaunches it) and at detach. Same
                                        records, stops and cursor as the other paths.                */

typedef struct halo_rx_ring_scan {
    uint32_t n_frames;  /* frames taken                                                      */
    uint32_t stop;      /* HALO_RING_STOP_*: why the walk ended                              */
    uint64_t end_bytes; /* ring bytes the frames occupy: the tail advance                    */
    uint32_t max_len;   /* longest frame taken                                               */
    uint32_t pad;
} halo_rx_ring_scan_t;

typedef struct halo_rx_ring halo_rx_ring_t;

/* Attach as the ring's consumer: ring_buffer_mapping + ring_buffer_consumer_init
 * (cgo/ring_buffer.h:158-204, :228-246; mem/ring_buffer.go:150-200, :226-246): layout version,
 * fill bytes, size/mask, head - tail <= size, and `offset` == this mapping's data address minus
 * the stored buffer pointer (0 in the creating process). capacity = the receive buffer's
 * len(data) (0: 1514, dpdk/dpdk.go:139; at most 16376); max_bytes (0: min(size, 256 MiB)) and
 * max_frames (0: max_bytes / 8) bound one poll. The header is validated before any device call. */
HALO_API int halo_rx_ring_attach(int device, void* ring_mem, int64_t offset, uint32_t capacity,
                                 uint64_t max_bytes, uint32_t max_frames, uint32_t attach_flags,
                                 halo_rx_ring_t** out);
/* Synchronises the ring's streams and frees its resources. HALO_E_HIP: the ring memory could not be
 * unregistered (the caller must then keep it allocated). */
HALO_API int halo_rx_ring_detach(halo_rx_ring_t* ring);
/* Parse the next frames (flags: HALO_RX_CSUM_ENABLE | HALO_RX_JUMBO_EXT; full records). They
 * stay in the ring until commit: positions[i] (optional) is frame i's record position in the
 * stream (the tail value before its ReadPacket; the frame's bytes start 4 bytes later, modulo
 * the size). Polls without a commit continue after the previous poll's frames. Synchronous. */
HALO_API int halo_rx_ring_poll(halo_rx_ring_t* ring, uint32_t flags, const halo_rx_netif_t* netif,
                               halo_rx_result_t* out, uint32_t* status_hist, uint64_t* positions,
                               halo_rx_ring_scan_t* info);
/* Small polls (rings attached with HALO_RING_REGISTER; default: spans up to 4 MiB): the host
 * reads the records' length fields as ReadPacket does and ONE rx launch parses the frames in
 * place in the registered ring, writing the records straight into `out` when it is pinned or
 * registered. Same results, stop and cursor as the pipelined path (a poll whose span has a frame
 * wrapping around the data area's end takes the pipelined path). `bytes` = 0 turns the small
 * path off; at most 16 MiB; HALO_E_INVAL for an unregistered ring.                         */
HALO_API int halo_rx_ring_set_small_poll(halo_rx_ring_t* ring, uint64_t bytes);
/* Release everything polled so far to the producer: tail = cursor (store-release). */
HALO_API int halo_rx_ring_commit(halo_rx_ring_t* ring);
/* Counters of a consumer since attach (observability; cheap enough to keep on): where a poll's
 * time goes. Times are host steady-clock ns, except service_gpu_ns (the resident consumer's own
 * real-time counter, from seeing a request to publishing its records). */
typedef struct halo_rx_ring_stats {
    uint64_t polls;            /* halo_rx_ring_poll calls that found records                      */
    uint64_t frames;           /* frames returned                                                  */
    uint64_t small_polls;      /* polls on the small path (one launch, or a service request)      */
    uint64_t service_requests; /* small polls served by the resident consumer (HALO_RING_PERSISTENT) */
    uint64_t service_launches; /* resident consumer launches (first use, after idle exits)       */
    uint64_t walk_ns;          /* small polls: the host's ReadPacket walk of the length fields    */
    uint64_t wait_ns;          /* small polls: launch + synchronisation, or request to completion */
    uint64_t service_gpu_ns;   /* resident consumer: GPU time per request, summed                 */
} halo_rx_ring_stats_t;
HALO_API int halo_rx_ring_get_stats(const halo_rx_ring_t* ring, halo_rx_ring_stats_t* out);
/* HALO_RING_PERSISTENT rings: bounds the wait for one resident request (default 2 s; 0 restores
 * it). A poll whose request times out retires it before returning HALO_E_HIP (the consumer is
 * stopped and its kernel has ended: nothing is written into `out` afterwards) and leaves the cursor
 * where it was, so the next poll parses the same frames. (Diagnostics and fault injection.)    */
HALO_API int halo_rx_ring_set_service_timeout(halo_rx_ring_t* ring, uint64_t us);

/* The record walk alone, device-resident: `used` bytes of ring data in stream order at d_span
 * (4-byte aligned; used a multiple of 4, <= ring_size), ring_size = RingBuffer.size. Writes
 * n = info.n_frames (offset in dwords, length) pairs and *d_info. Workspace: at least
 * halo_rx_ring_scan_workspace(used, capacity) bytes of device memory. Asynchronous.       */
HALO_API uint64_t halo_rx_ring_scan_workspace(uint64_t used, uint32_t capacity);
HALO_API int halo_rx_ring_scan_device(const uint8_t* d_span, uint64_t used, uint64_t ring_size,
                                      uint32_t capacity, uint32_t max_frames, uint32_t* d_offsets_dw,
                                      uint16_t* d_lens, halo_rx_ring_scan_t* d_info, void* d_workspace,
                                      uint64_t workspace_bytes, halo_stream_t stream);

/* The producer side, for rings this process creates (engine.NewWire / Wire.Tx,
 * engine/engine.go:520-553): RingBufferCreate (mem/ring_buffer.go:93-126) over `bytes` of
 * 64-byte-aligned memory (128-byte header + a power-of-two data area), and WritePacket
 * (mem/ring_buffer.go:249-295) for every frame in order — a frame the ring refuses (full,
 * empty, longer than size/2) is dropped, as the DPDK rx lcore drops it (cgo/dpdk.c:288-305).
 * accepted[i] (optional) = 1 if frame i was written; *written = the count. Host only.      */
HALO_API int halo_ring_create(void* memory, uint64_t bytes);
HALO_API int halo_ring_write_batch(void* memory, const uint8_t* bytes, const uint64_t* offsets,
                                   const uint16_t* lens, uint32_t n, uint8_t* accepted, uint32_t* written);

/* ---- forward / transmit direction: in-place header rewrite + checksum fill --------------
 * (SURVEY.md §8f row f2). Frame i's IPv4 packet is pkt = frame[14 : len] — exactly the slice
 * engine.RxIpv4 hands to Ipv4RouteForward (engine/ipv4_engine.go:31-37) — and each frame gets
 * the steps set in ops[i].steps, applied in this order (the order Ipv4RouteForward applies
 * them, engine/ipv4_engine.go:108-269):
 *   HALO_TX_NAT_DST   NatChangeDst(pkt, dst_ip, dst_port)      protocol/ipv4.go:277-302
 *   HALO_TX_TTL       HandleIpv4PktTtl(pkt)                    protocol/ipv4.go:134-145
 *   HALO_TX_NAT_SRC   NatChangeSrc(pkt, src_ip, src_port)      protocol/ipv4.go:249-275
 *   HALO_TX_RECALC    ReCalcIpv4CheckSum + the L4 ReCalc* picked by pkt[9]
 *                                                               protocol/ipv4.go:148-226
 *   HALO_TX_DPDK_FILL eth_tx's software checksum fill (cgo/dpdk.c:333-365: rte_ipv4_cksum and
 *                     rte_ipv4_udptcp_cksum of DPDK 20.11, the reference's pinned DPDK)
 * `flags & HALO_RX_CSUM_ENABLE` is protocol.CheckSumEnable for the Go steps (ReCalcIcmp and
 * DPDK_FILL ignore it, as the reference does). Every length guard of the Go functions is kept:
 * a step whose guard fails leaves the packet as Go would. Result byte per frame: HALO_TX_R_*. */
#define HALO_TX_NAT_DST 0x01u
#define HALO_TX_TTL 0x02u
#define HALO_TX_NAT_SRC 0x04u
#define HALO_TX_RECALC 0x08u
#define HALO_TX_DPDK_FILL 0x10u
#define HALO_TX_R_TTL_ALIVE 0x01u /* HandleIpv4PktTtl returned true                        */
#define HALO_TX_R_SKIPPED 0x02u   /* a step's length guard left the packet (partly) as is   */
#define HALO_TX_R_OVERRUN 0x04u   /* DPDK_FILL: IPv4 totalLen runs past the frame (DPDK would
                                     read stale mbuf bytes); L4 checksum left zero          */
typedef struct halo_tx_op {
    uint8_t steps;     /* HALO_TX_* */
    uint8_t pad;
    uint16_t dst_port; /* NatChangeDst port */
    uint32_t dst_ip;   /* NatChangeDst address, IpAddrToU form */
    uint16_t src_port; /* NatChangeSrc port */
    uint16_t pad2;
    uint32_t src_ip;   /* NatChangeSrc address, IpAddrToU form */
} halo_tx_op_t;       /* 16 B */

/* Device pointers; frames rewritten in place; `d_result` (optional) gets one byte per frame.
 * Ragged layout as halo_rx_parse_batch_device. Asynchronous on `stream`.                */
HALO_API int halo_tx_fixup_batch_device(uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                        const uint16_t* d_lens, uint32_t n,
                                        const halo_tx_op_t* d_ops, uint32_t flags,
                                        uint32_t max_len_hint, uint8_t* d_result,
                                        halo_stream_t stream);

/* ---- IcmpTtlDeepNat (engine/icmp_engine.go:55-86) -------------------------------------------
 * The forward path calls it on every received Ethernet payload of a NATing interface before its
 * own DNAT (engine/ipv4_engine.go:111-130): when the packet is an ICMP time-exceeded message
 * (ParseIpv4Pkt and ParseIcmpPkt pass, type ICMP_TTL) quoting at least 28 bytes of the original
 * packet, it looks the quoted flow up with NatGetFlowByWan(quoted dst, its dst port, quoted src,
 * its src port, quoted proto) and, when a flow exists, rewrites the quote's source to the flow's
 * LAN host (NatChangeSrc on the quote, with its ReCalc* — TCP's needs 38 quoted bytes) and the
 * message's destination to the LAN host with "port" 0 (NatChangeDst on the untrimmed Ethernet
 * payload: its ICMP checksum covers Ethernet padding). The lookup is not part of this call
 * (halo_nat_lookup_quote_device does it on the device, or the caller on its own table): call
 * once with d_nat = NULL to get per frame a quote record — status HALO_RX_OK when the message
 * qualifies, else the failing rx status, HALO_RX_IP_PROTO (not ICMP), HALO_RX_ICMP_TYPE (not
 * ICMP_TTL) or HALO_RX_L4_LEN (quote < 28 B); ip_proto = the quoted protocol; src_ip / sport =
 * the quoted destination and its port, dst_ip / dport = the quoted source and its port, so that
 * halo_flow_hash_device(HALO_FLOW_NAT_WAN) of the records is NatGetFlowByWan's key — then again
 * with the lookups' results in d_nat to rewrite the frames in place. d_applied[i] = 1 when frame
 * i was rewritten (IcmpTtlDeepNat returned true). Frames are the ragged layout of the rx parse;
 * `flags & HALO_RX_CSUM_ENABLE` is protocol.CheckSumEnable. A slow path: one wavefront per frame. */
typedef struct halo_tx_deep_nat {
    uint32_t lan_ip;   /* NatFlow.LanHostIpAddr (IpAddrToU form)       */
    uint16_t lan_port; /* NatFlow.LanHostPort                          */
    uint8_t found;     /* NatGetFlowByWan returned a flow               */
    uint8_t pad;
} halo_tx_deep_nat_t;  /* 8 B */
HALO_API int halo_tx_icmp_deep_nat_batch_device(uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                                const uint16_t* d_lens, uint32_t n,
                                                const halo_tx_deep_nat_t* d_nat, uint32_t flags,
                                                halo_rx_result_t* d_quote, uint8_t* d_applied,
                                                halo_stream_t stream);

/* ---- transmit direction: batch packet construction (the Build* half) --
 * The locally originated send chain, one frame per descriptor:
 *   NetIf.TxUdp / TxTcp / TxIcmp   engine/{udp,tcp,icmp}_engine.go:24-32 / :29-37 / :26-34
 *    -> protocol.BuildUdpPkt        protocol/udp.go:52-91   (payload <= 1472)
 *       protocol.BuildTcpPkt        protocol/tcp.go:73-123  (payload <= 1460; 20 B header, window 256)
 *       protocol.BuildIcmpPkt       protocol/icmp.go:66-89  (payload <= 1472; code 0)
 *    -> NetIf.TxIpv4                engine/ipv4_engine.go:50-99
 *       protocol.BuildIpv4Pkt       protocol/ipv4.go:89-131 (iphId++ per packet, TTL 0x80, no frag)
 *    -> NetIf.TxEthernet            engine/ethernet_engine.go:34-50
 *       protocol.BuildEthFrm        protocol/ethernet.go:58-82 (src MAC = the NetIf's, pad to 60 B)
 * `flags & HALO_RX_CSUM_ENABLE` is protocol.CheckSumEnable: it gates the IPv4 header, UDP and
 * TCP checksums (0 when off); the ICMP checksum is always filled (icmp.go:84-87). TxIpv4's
 * control-plane decisions (FindRoute, the ARP cache, broadcast) are the caller's — or, on the
 * device, halo_arp_encap_tx_device's over the built frames ("local responders" below): each
 * descriptor carries the destination MAC they produced (zeros when that call fills it) and its mode:
 *   HALO_TX_BUILD_ETH       the Ethernet frame TxEthernet hands to EthTxFunc
 *   HALO_TX_BUILD_LOOPBACK  the IPv4 packet alone: the copy TxIpv4 puts into the NetIf's LoChan
 *                           when the destination is its own address (engine/ipv4_engine.go:72-79),
 *                           which the L3 loopback parse (HALO_RX_L3_START) consumes.
 * iphId (protocol/ipv4.go:33, process-global in Go) is the device u16 *d_ip_id: BuildIpv4Pkt's
 * `iphId++` runs once per packet that reaches it, in descriptor order, so the k-th successfully
 * built packet of the batch (k = 1, 2, ...) carries id *d_ip_id + k, and *d_ip_id is advanced by
 * the number built. A descriptor whose Build* call returns an error is not built (no iphId step,
 * length 0, result code below). */
#define HALO_TX_BUILD_ETH 0u
#define HALO_TX_BUILD_LOOPBACK 1u
#define HALO_TX_B_OK 0u
#define HALO_TX_B_PAYLOAD_LEN 1u /* "payload len must <= 1472" (udp.go:55, icmp.go:71) / "<= 1460" (tcp.go:78) */
#define HALO_TX_B_PROTO 2u       /* build-defined: proto is not UDP (17), TCP (6) or ICMP (1)          */
#define HALO_TX_B_SLOT 3u        /* build-defined: the frame is longer than out_stride                  */
typedef struct halo_tx_build_desc {
    uint64_t payload_off;  /* byte offset of the L4 payload in d_payload (any alignment)         */
    uint16_t payload_len;
    uint8_t proto;         /* IPH_PROTO_UDP / _TCP / _ICMP (protocol/ipv4.go:27-32)               */
    uint8_t aux;           /* TCP flags; ICMP type                                                */
    uint16_t src_port;     /* UDP/TCP source port; ICMP: the 2 icmpId bytes as a big-endian u16  */
    uint16_t dst_port;     /* UDP/TCP destination port; ICMP: icmpSeq                            */
    uint32_t src_ip;       /* IpAddrToU(srcAddr): the NetIf's address for Tx*                    */
    uint32_t dst_ip;       /* IpAddrToU(dstAddr)                                                 */
    uint32_t seq;          /* TCP seqNum                                                         */
    uint32_t ack;          /* TCP ackNum                                                         */
    uint8_t dst_mac[6];    /* ETH mode: TxIpv4's broadcast / ARP-cache result                    */
    uint8_t mode;          /* HALO_TX_BUILD_*                                                    */
    uint8_t pad;
} halo_tx_build_desc_t;    /* 40 B */

/* Device scratch for n descriptors (bytes, 4-byte aligned; no initialisation needed). One
 * launch at a time per workspace. */
HALO_API uint64_t halo_tx_build_workspace(uint32_t n);
/* Build n frames into fixed output slots: frame i at d_frames + i * out_stride (a multiple of
 * 4, at least 60), d_out_lens[i] = its length (0 when not built), d_result[i] (optional) =
 * HALO_TX_B_*. The bytes of a slot past the frame's last 4-byte word are left untouched.
 * `max_payload_hint` (0 = unknown) picks the lanes per frame. Asynchronous on `stream`.     */
HALO_API int halo_tx_build_batch_device(const halo_tx_build_desc_t* d_desc, uint32_t n, const uint8_t* d_payload,
                                        uint32_t flags, const halo_rx_netif_t* netif, uint32_t max_payload_hint,
                                        uint8_t* d_frames, uint32_t out_stride, uint16_t* d_out_lens,
                                        uint8_t* d_result, uint16_t* d_ip_id, void* d_workspace,
                                        uint64_t workspace_bytes, halo_stream_t stream);

/* ---- flow-key hashing --------------------------------------------
 * hashcode.GetHashCodeXXH3 (hashcode/hashcode.go:15-17 -> hashcode/xxh3.go:43-287, XXH3-64 with
 * the default secret and seed 0, ported from github.com/zeebo/xxh3 v1.1.0) over a batch of byte
 * strings, and the NAT flow-table keys the forward path hashes for every NATed packet. */
#define HALO_FLOW_NAT_LAN 0u  /* NatFlowHash{remote=dst, dport, lan host=src, sport, proto} as
                                 NatGetFlowByHash builds it (engine/ipv4_engine.go:524-551)   */
#define HALO_FLOW_NAT_WAN 1u  /* NatWanFlowHash{remote=src, sport, wan=dst, dport, proto} as
                                 NatGetFlowByWan builds it (engine/ipv4_engine.go:554-581)    */
#define HALO_NAT_SYMMETRIC 0u /* NetIfConfig.NatType (engine/ipv4_engine.go:423-426): remote  */
#define HALO_NAT_FULL_CONE 1u /* address/port kept (symmetric) or zeroed (any other value)   */

/* d_hash[i] = XXH3-64(d_bytes[d_offsets[i] : d_offsets[i] + d_lens[i]]). Byte offsets, any
 * alignment. Asynchronous on `stream`. */
HALO_API int halo_xxh3_64_batch_device(const uint8_t* d_bytes, const uint64_t* d_offsets, const uint32_t* d_lens,
                                       uint32_t n, uint64_t* d_hash, halo_stream_t stream);

/* For each parsed record: build the 13-byte little-endian flow key of `kind` (the ICMP remote
 * port is 0, the remote address and port are 0 unless nat_type is HALO_NAT_SYMMETRIC), hash it
 * with XXH3-64 (NatFlowHash.GetHashCode, engine/ipv4_engine.go:451-459; NatWanFlowHash
 * :471-479) into d_hash[i], and, when d_bucket is non-null, write the hashmap bucket
 * hash % bucket_count (hashmap/hashmap.go:64) into d_bucket[i]. Records are used as they are;
 * callers hash the records whose engine action is FORWARD. */
HALO_API int halo_flow_hash_device(const halo_rx_result_t* d_records, uint32_t n, uint32_t kind, uint32_t nat_type,
                                   uint64_t* d_hash, uint32_t bucket_count, uint32_t* d_bucket,
                                   halo_stream_t stream);

/* The same over compact records (HALO_RX_RECORD_COMPACT parse output): the five key fields are the
 * whole 16-byte record, so nothing is fetched that the key does not use (a full record's key fields
 * are 20 of its 32 bytes). Identical hashes and buckets for the same frames.                      */
HALO_API int halo_flow_hash_compact_device(const halo_rx_record16_t* d_records, uint32_t n, uint32_t kind,
                                           uint32_t nat_type, uint64_t* d_hash, uint32_t bucket_count,
                                           uint32_t* d_bucket, halo_stream_t stream);

/* The rx parse (halo_rx_parse_batch_device, same arguments and records) with the NAT flow key
 * of every record hashed in the same pass, exactly as halo_flow_hash_device would hash the
 * records it writes: the engine's receive -> forward -> NAT lookup chain without re-reading the
 * records. Full or compact records (flags); d_hash (8-byte aligned) and d_bucket as above.     */
HALO_API int halo_rx_parse_flow_batch_device(const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                             const uint16_t* d_lens, uint32_t n, uint32_t flags,
                                             const halo_rx_netif_t* netif, uint32_t max_len_hint,
                                             halo_rx_result_t* d_out, uint32_t* d_status_hist,
                                             uint32_t flow_kind, uint32_t nat_type, uint64_t* d_hash,
                                             uint32_t bucket_count, uint32_t* d_bucket, halo_stream_t stream);

/* ---- route lookup ---------------------------------------------------
 * RouteTable (engine/ipv4_engine.go:270-390): a binary trie of route lists, longest-prefix
 * FindRoute with an ECMP pick lastMatch[fnv32a(ip) % len] (engine/engine.go:159). The trie is
 * the control plane and is kept on the host exactly as UpdateRoute builds it (including lists
 * emptied by DeleteRoute, which still end a lookup); halo_route_sync_device compiles it into a
 * DIR-24-8 table in HBM (a 2^24-entry first level, 256-entry second-level blocks for prefixes
 * longer than /24) and lookups run on the GPU only. Route ids identify the RouteEntry objects:
 * each insertion gets a fresh id. */
typedef struct halo_route_table halo_route_table_t;
typedef struct halo_route_entry {
    uint32_t dst_ip;       /* IpAddrToU(DstIpAddr)   */
    uint32_t network_mask; /* IpAddrToU(NetworkMask) */
    uint32_t next_hop;     /* IpAddrToU(NextHop); 0 for nil (direct routes) */
    uint32_t netif;        /* the caller's id for the NetIf name */
} halo_route_entry_t;
#define HALO_ROUTE_NONE 0xFFFFFFFFu  /* FindRoute returns nil (no route)                        */
#define HALO_ROUTE_PANIC 0xFFFFFFFEu /* the longest match is a list DeleteRoute emptied: Go's
                                        `% uint32(len(lastMatch))` divides by zero (:382)       */

HALO_API int halo_route_table_create(halo_route_table_t** out);
HALO_API int halo_route_table_destroy(halo_route_table_t* t);
/* UpdateRoute(old, new) (:304-348): walks old's prefix, drops entries equal to old (dst, mask,
 * next hop, netif), appends new (if non-null, with a fresh id written to *new_id). AddRoute is
 * update(r, r), DeleteRoute is update(r, NULL) (:293-301). */
HALO_API int halo_route_update(halo_route_table_t* t, const halo_route_entry_t* old_route,
                               const halo_route_entry_t* new_route, uint32_t* new_id);
HALO_API int halo_route_get(const halo_route_table_t* t, uint32_t id, halo_route_entry_t* out);
/* Compile the trie into the device table on `device` (allocates / grows HBM; synchronous).
 * Double-buffered: the new table is written into the generation not in use, after the device
 * has drained every lookup that could still read that one (a device synchronisation), and is
 * then published. A lookup sees the table last published when it was launched — never one
 * being rewritten, as FindRoute under RouteTable.RLock never does (engine/ipv4_engine.go:351).
 * Lookups and syncs may run on different threads: a lookup holds the table's read lock from
 * taking its view until its kernel is enqueued, and a sync takes the write lock before it
 * drains the device, so no launch can slip in between (RWMutex semantics, :270-275). */
HALO_API int halo_route_sync_device(halo_route_table_t* t, int device);
/* FindRoute for each address (IpAddrToU form) / each record's dst_ip: route id, HALO_ROUTE_NONE
 * or HALO_ROUTE_PANIC. Asynchronous on `stream`; uses the last synced table. */
HALO_API int halo_route_lookup_device(const halo_route_table_t* t, const uint32_t* d_ips, uint32_t n,
                                      uint32_t* d_route_ids, halo_stream_t stream);
HALO_API int halo_route_lookup_records_device(const halo_route_table_t* t, const halo_rx_result_t* d_records,
                                              uint32_t n, uint32_t* d_route_ids, halo_stream_t stream);
/* The rx parse (halo_rx_parse_batch_device, same arguments and records) with FindRoute of every
 * record's dst_ip in the same pass — the RxIpv4 -> Ipv4RouteForward -> FindRoute chain
 * (engine/ipv4_engine.go:18-47, :108-269, :351-390) without re-reading the records: d_route_ids
 * equals halo_route_lookup_records_device over the records written.                         */
HALO_API int halo_rx_parse_route_batch_device(const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                              const uint16_t* d_lens, uint32_t n, uint32_t flags,
                                              const halo_rx_netif_t* netif, uint32_t max_len_hint,
                                              halo_rx_result_t* d_out, uint32_t* d_status_hist,
                                              const halo_route_table_t* table, uint32_t* d_route_ids,
                                              halo_stream_t stream);

/* ---- NAT flow table (the table between the hash, the route and the rewrite) ------------------
 * A NATing NetIf's NatFlowTable / NatWanFlowTable / NatPortAlloc / NatPortMappingTable
 * (engine/ipv4_engine.go:423-759). The control plane stays on the host exactly as the reference
 * builds it (NatAddFlow's port allocation included) and is the authority; halo_nat_sync_device
 * compiles both indexes and the port-mapping list into open-addressing tables in HBM, and the
 * lookups of Ipv4RouteForward's inbound (:111-130) and outbound (:203-225) halves and of
 * IcmpTtlDeepNat (engine/icmp_engine.go:55-86) run on the GPU over the parsed records, writing the
 * halo_tx_op_t array halo_tx_fixup_batch_device consumes. Only new flows (device MISS) take a
 * host slow path: halo_nat_resolve_misses over host copies of the whole batch, or the miss path
 * below (halo_nat_collect_misses_device -> halo_nat_resolve_items -> halo_nat_apply_answers_device),
 * which brings only one item per new key to the host. One table per NATing NetIf. All addresses are in
 * IpAddrToU form. The router-global NatPortMappingFlowTable (:160-186, :238-266) is its own
 * table ("port-mapping return flows" below). The ARP step that follows the rewrite is
 * halo_arp_encap_device ("ARP neighbour cache" below).
 *
 * Flow ids identify NatFlow objects: each NatAddFlow gets a fresh id, never reused, so that an id
 * read from a device table that is one generation old still names the same flow. LastAliveTime
 * lives in a u32 stamp array in HBM indexed by flow id, shared by both device generations: a
 * device hit stores `now` there (plain store; concurrent streams with different `now` are last
 * writer wins, as the unlocked Go field is), halo_nat_expire and halo_nat_sync_device copy the
 * array back, and the merged stamp is the later of the host's and the device's in serial-number
 * order ((int32_t)(a - b) > 0): the true last touch whenever TimeNow does not go backwards.     */
typedef struct halo_nat_table halo_nat_table_t;
typedef struct halo_nat_config {
    uint32_t wan_ip;        /* IpAddrToU(NetIf.IpAddr): NatFlow.WanIpAddr and the mapping SNAT address */
    uint32_t nat_type;      /* HALO_NAT_SYMMETRIC / HALO_NAT_FULL_CONE (NetIfConfig.NatType)          */
    uint32_t capacity_log2; /* 0: automatic (load <= 0.5); else the device tables have exactly
                               2^capacity_log2 slots (<= 28; tests). An index that does not fit
                               (entries >= slots) makes sync / layout_stats return HALO_E_RANGE   */
    uint32_t pad;
} halo_nat_config_t;
typedef struct halo_nat_flow { /* engine.NatFlow (:429-439) */
    uint32_t remote_ip;   /* RemoteIpAddr (normalised: 0 unless symmetric)   */
    uint32_t wan_ip;      /* WanIpAddr                                        */
    uint32_t lan_ip;      /* LanHostIpAddr                                    */
    uint32_t last_alive;  /* LastAliveTime (host copy; device stamps are folded in by expire / sync) */
    uint16_t remote_port; /* RemotePort (normalised: 0 unless symmetric; 0 for ICMP)                  */
    uint16_t wan_port;    /* WanPort                                          */
    uint16_t lan_port;    /* LanHostPort                                      */
    uint8_t proto;        /* Ipv4HeadProto                                    */
    uint8_t pad;
    uint32_t id;          /* the flow id (HALO_NAT_NO_FLOW: nil)              */
} halo_nat_flow_t;        /* 28 B */
#define HALO_NAT_NO_FLOW 0xFFFFFFFFu
#define HALO_NAT_MAX_PORT_MAPPINGS 256u
/* per-record verdict of a lookup */
#define HALO_NAT_V_NONE 0u    /* ip_proto == 0xFF: ParseIpv4Pkt failed, Ipv4RouteForward never runs  */
#define HALO_NAT_V_SKIP 1u    /* d_skip[i] != 0: IcmpTtlDeepNat applied, the DNAT is skipped (:116)  */
#define HALO_NAT_V_MISS 2u    /* no mapping, no flow in the device table                              */
#define HALO_NAT_V_FLOW 3u    /* a NatFlow; ref = flow id                                             */
#define HALO_NAT_V_MAPPING 4u /* a NatPortMappingEntry; ref = its index in call order                 */
#define HALO_NAT_V_DROP 5u    /* halo_nat_resolve_misses only: NatAddFlow returned nil (:214-217)     */
typedef struct halo_nat_layout_stats { /* index 0 = LAN (NatFlowTable), 1 = WAN (NatWanFlowTable) */
    uint32_t slots;            /* slots per index (a power of two)                               */
    uint32_t port_mappings;
    uint32_t entries[2];
    uint32_t longest_chain[2]; /* most slots any entry's lookup reads (1 = at its home slot)     */
    uint32_t wrapped[2];       /* entries whose probe chain runs past the last slot to slot 0    */
} halo_nat_layout_stats_t;

HALO_API int halo_nat_table_create(const halo_nat_config_t* cfg, halo_nat_table_t** out);
HALO_API int halo_nat_table_destroy(halo_nat_table_t* t);
/* NatPortMappingTable, appended in call order as InitRouter appends (engine/engine.go:228);
 * CheckNatPortMapping (:683-707) takes the first match in that order. At most
 * HALO_NAT_MAX_PORT_MAPPINGS entries (HALO_E_RANGE beyond). */
HALO_API int halo_nat_port_mapping_add(halo_nat_table_t* t, uint16_t wan_port, uint32_t lan_ip, uint16_t lan_port,
                                       uint8_t proto);
/* NatAddFlow (:584-680): nil when lan_port or remote_port is 0; one port allocator per normalised
 * remote address, ports taken sequentially from 32768, wrapping to 0 = exhausted (nil); both
 * indexes point at the one flow (an existing LAN key is replaced, as HashMap.Set does);
 * LastAliveTime = now. nil is out->id = *flow_id = HALO_NAT_NO_FLOW, not a call failure. `out` and
 * `flow_id` are optional. */
HALO_API int halo_nat_add_flow(halo_nat_table_t* t, uint32_t lan_ip, uint32_t remote_ip, uint16_t lan_port,
                               uint16_t remote_port, uint8_t proto, uint32_t now, halo_nat_flow_t* out,
                               uint32_t* flow_id);
/* NatGetFlowByHash (:524-551) / NatGetFlowByWan (:554-581) on the authoritative host table: the
 * key is normalised by the table's nat_type and compared whole (hashmap/hashmap.go:63-80). */
HALO_API int halo_nat_get_flow_lan(const halo_nat_table_t* t, uint32_t remote_ip, uint16_t remote_port,
                                   uint32_t lan_ip, uint16_t lan_port, uint8_t proto, halo_nat_flow_t* out,
                                   uint32_t* flow_id);
HALO_API int halo_nat_get_flow_wan(const halo_nat_table_t* t, uint32_t remote_ip, uint16_t remote_port,
                                   uint32_t wan_ip, uint16_t wan_port, uint8_t proto, halo_nat_flow_t* out,
                                   uint32_t* flow_id);
/* The slow path for the records a device lookup left as HALO_NAT_V_MISS; host memory only.
 * dir = HALO_FLOW_NAT_WAN (inbound half) or HALO_FLOW_NAT_LAN (outbound half). Walks the MISS
 * records in ascending index order (port allocation depends on packet order), repeats the lookup
 * on the host table (port mapping, then flow) and, for LAN, runs NatAddFlow on a miss; nil becomes
 * HALO_NAT_V_DROP (:214-217). A WAN miss stays MISS (:120-124). A hit writes the op fields and
 * verdict the device would have written and stamps the flow with `now`, so results do not depend
 * on when the device copy was last synced. verdicts_out (may alias verdicts) gets every verdict;
 * *n_added (optional) the flows added. */
HALO_API int halo_nat_resolve_misses(halo_nat_table_t* t, uint32_t dir, const halo_rx_result_t* records,
                                     const uint8_t* verdicts, uint32_t n, uint32_t now, halo_tx_op_t* ops,
                                     uint8_t* verdicts_out, uint32_t* n_added);
/* One NatTableClear tick (:723-759): every flow with (uint32_t)(now - LastAliveTime) > 60 leaves
 * both indexes and frees its port; an allocator left without ports is dropped. The stamps the
 * device wrote are folded in first (a device drain), so THE CALLER MUST HAVE SYNCHRONISED THE
 * STREAMS ITS LOOKUPS RAN ON before this call: a lookup still running may stamp a flow after the
 * fold. When flows were removed and the table has a device copy, the copy is rebuilt and
 * published before the call returns: no later lookup hits a removed flow. */
HALO_API int halo_nat_expire(halo_nat_table_t* t, uint32_t now, uint32_t* n_removed);
/* ListNat (:710-720): up to `cap` flows into `out` (NULL with cap 0 to count), *n = the total.
 * Order unspecified. */
HALO_API int halo_nat_list(const halo_nat_table_t* t, halo_nat_flow_t* out, uint32_t cap, uint32_t* n);
/* The device layout a sync would produce now (host only, no device needed). */
HALO_API int halo_nat_layout_stats(const halo_nat_table_t* t, halo_nat_layout_stats_t* out);
/* Compile both indexes and the port mappings into HBM on `device` (one device per table;
 * synchronous; the caller's current device is restored). Entries are 32-byte slots (the whole
 * 13-byte key, the translation, the flow id) placed by linear probing from
 * XXH3-64(key) & (slots - 1) — the hash of halo_flow_hash_device. Double-buffered as
 * halo_route_sync_device: the device is drained, the stamps are folded into the host table, the
 * generation not in use is rewritten and then published; a lookup holds the table's read lock
 * from taking its view until its kernel is enqueued. */
HALO_API int halo_nat_sync_device(halo_nat_table_t* t, int device);
/* The inbound half of Ipv4RouteForward (:111-130) for each record: CheckNatPortMapping(WanToLan,
 * dport, proto) else NatGetFlowByWan(src, sport, dst, dport, proto). Per record:
 *   ip_proto == 0xFF              -> HALO_NAT_V_NONE, op untouched
 *   d_skip && d_skip[i] != 0      -> HALO_NAT_V_SKIP, op untouched (d_skip = deep NAT's d_applied)
 *   hit   -> ops[i].steps |= HALO_TX_NAT_DST; dst_ip / dst_port = the LAN host; no other op field
 *            is written; d_verdict[i] = HALO_NAT_V_FLOW / _MAPPING; d_ref[i] = flow id / mapping
 *            index; a flow's stamp = now
 *   miss  -> HALO_NAT_V_MISS, d_ref[i] = HALO_NAT_NO_FLOW, *d_miss_count += 1 (the caller zeroes it)
 * Records are used as they are: the caller selects the FORWARD records, as with
 * halo_flow_hash_device. Records and ops 16-byte aligned. Uses the table last published
 * (HALO_E_INVAL before the first sync); n == 0 is OK. Asynchronous on `stream`. */
HALO_API int halo_nat_lookup_wan_device(const halo_nat_table_t* t, const halo_rx_result_t* d_records, uint32_t n,
                                        uint32_t now, const uint8_t* d_skip, halo_tx_op_t* d_ops,
                                        uint8_t* d_verdict, uint32_t* d_ref, uint32_t* d_miss_count,
                                        halo_stream_t stream);
/* The outbound half (:203-225) on this (the out-interface's) table: CheckNatPortMapping(LanToWan,
 * src, sport, proto) -> NatChangeSrc(wan_ip, entry.WanPort), else NatGetFlowByHash(dst, dport, src,
 * sport, proto) -> NatChangeSrc(WanIpAddr, WanPort). A hit ORs HALO_TX_NAT_SRC and writes src_ip /
 * src_port only. A MISS is a new flow: halo_nat_resolve_misses runs NatAddFlow. */
HALO_API int halo_nat_lookup_lan_device(const halo_nat_table_t* t, const halo_rx_result_t* d_records, uint32_t n,
                                        uint32_t now, const uint8_t* d_skip, halo_tx_op_t* d_ops,
                                        uint8_t* d_verdict, uint32_t* d_ref, uint32_t* d_miss_count,
                                        halo_stream_t stream);
/* The same over compact records. */
HALO_API int halo_nat_lookup_wan_compact_device(const halo_nat_table_t* t, const halo_rx_record16_t* d_records,
                                                uint32_t n, uint32_t now, const uint8_t* d_skip,
                                                halo_tx_op_t* d_ops, uint8_t* d_verdict, uint32_t* d_ref,
                                                uint32_t* d_miss_count, halo_stream_t stream);
HALO_API int halo_nat_lookup_lan_compact_device(const halo_nat_table_t* t, const halo_rx_record16_t* d_records,
                                                uint32_t n, uint32_t now, const uint8_t* d_skip,
                                                halo_tx_op_t* d_ops, uint8_t* d_verdict, uint32_t* d_ref,
                                                uint32_t* d_miss_count, halo_stream_t stream);
/* IcmpTtlDeepNat's NatGetFlowByWan (engine/icmp_engine.go:75-82), between the two passes of
 * halo_tx_icmp_deep_nat_batch_device and straight from the quote records the first pass writes:
 * d_nat[i] = {LanHostIpAddr, LanHostPort, found}; found = 0 (and zero fields) where the quote
 * status is not HALO_RX_OK or no flow exists. No port mapping, no stamp (the reference sets
 * neither). */
HALO_API int halo_nat_lookup_quote_device(const halo_nat_table_t* t, const halo_rx_result_t* d_quote_records,
                                          uint32_t n, halo_tx_deep_nat_t* d_nat, halo_stream_t stream);

/* The miss path: what halo_nat_resolve_misses does for a batch, with the records, verdicts and
 * ops left in HBM. The host table stays the authority (ports are allocated there, in packet
 * order); the device lists, once per key and in ascending record index, what the host must see
 * (collect), the host answers each item (halo_nat_resolve_items), and the device writes the
 * answers into the ops, verdicts and refs of every record of the key (apply). Over the same
 * arrays the three calls leave the ops, the verdicts and the host table exactly as
 * halo_nat_resolve_misses does.
 *
 * A record is SELECTED when d_verdict[i] == HALO_NAT_V_MISS and (d_select == NULL or
 * d_select[i] != 0). Its key is the normalised key the lookup of `dir` uses (port 0 for ICMP's
 * remote port, no remote half unless the table is symmetric). The REPRESENTATIVE of a selected
 * record is the lowest-indexed selected record with the same key. Answering a key once is exact
 * because a later record of the key meets what the first one left: a flow the first one added is
 * a hit from then on; a port mapping or a WAN answer depends on nothing a record changes; and a
 * DROP by port exhaustion repeats, since nothing frees a port inside a batch. ONE CLASS IS ORDER
 * SENSITIVE and is never deduplicated: a LAN record with dport == 0 and sport != 0. NatAddFlow
 * refuses a raw remotePort of 0 (engine/ipv4_engine.go:584-587), but the key is normalised first,
 * so under full-cone NAT A(dport 0), B(dport 5), C(dport 0) of one LAN host and port share a key
 * and give DROP, FLOW (added), FLOW (hit): copying A's DROP to B and C would be wrong. Each such
 * record is listed on its own, is its own representative and nobody else's. A record with
 * sport == 0 needs no such care: no flow with LAN port 0 can exist, so its answer (MAPPING or
 * DROP) is a function of its key alone; a GRE or ESP flood lists one item. WAN has no adds: every
 * WAN key is deduplicated. */
typedef struct halo_nat_miss_item { /* 20 B, 4-byte aligned; the raw record fields, not normalised */
    uint32_t index;                 /* the record's index in its batch (the first of its key) */
    uint32_t src_ip, dst_ip;
    uint16_t sport, dport;
    uint8_t proto, pad[3];
} halo_nat_miss_item_t;
typedef struct halo_nat_answer { /* 16 B, 16-byte aligned on the device */
    uint32_t ip;                 /* the translation a hit writes (dst_* for WAN, src_* for LAN) */
    uint32_t ref;                /* flow id / mapping index / HALO_NAT_NO_FLOW */
    uint16_t port;
    uint8_t verdict;             /* HALO_NAT_V_FLOW / _MAPPING / _DROP / _MISS (WAN: stays MISS) */
    uint8_t pad[5];
} halo_nat_answer_t;
/* Bytes of device scratch halo_nat_collect_misses_*device needs for n records (4-byte aligned): the
 * in-batch table (u32 per slot), one u32 per 256-record tile and one u32 per record.
 * scratch_log2 == 0: automatic, the power of two >= 2n (at least 16 slots); otherwise exactly
 * 2^scratch_log2 slots (tests). 0 when the combination is out of range (scratch_log2 > 31, or
 * n > 2^30 with automatic sizing). */
HALO_API uint64_t halo_nat_miss_workspace(uint32_t n, uint32_t scratch_log2);
/* Collect: d_items receives the representatives, densely, in ascending index; *d_count is SET to
 * their number, also when it exceeds `cap` (only the first `cap` items are written); d_pos[i] =
 * the list position of record i's representative, for every i < n (also a position >= cap), and
 * HALO_NAT_NO_FLOW for a record that is not selected. Records and verdicts are read only; records
 * 16-byte aligned, d_items / d_count / d_pos / d_workspace 4-byte aligned. One workspace serves
 * any number of calls on one stream: the call re-initialises what it needs. HALO_E_RANGE, before
 * any launch, when the slot count is not greater than n (or out of range as above); HALO_E_INVAL
 * for a bad argument, a short workspace, or before the table's first sync; n == 0 is OK (*d_count
 * = 0). Asynchronous on `stream`: one memset and five kernels. */
HALO_API int halo_nat_collect_misses_device(const halo_nat_table_t* t, uint32_t dir,
                                            const halo_rx_result_t* d_records, const uint8_t* d_verdict,
                                            const uint8_t* d_select, uint32_t n, uint32_t scratch_log2,
                                            halo_nat_miss_item_t* d_items, uint32_t cap, uint32_t* d_count,
                                            uint32_t* d_pos, void* d_workspace, uint64_t workspace_bytes,
                                            halo_stream_t stream);
/* The same over compact records. */
HALO_API int halo_nat_collect_misses_compact_device(const halo_nat_table_t* t, uint32_t dir,
                                                    const halo_rx_record16_t* d_records, const uint8_t* d_verdict,
                                                    const uint8_t* d_select, uint32_t n, uint32_t scratch_log2,
                                                    halo_nat_miss_item_t* d_items, uint32_t cap, uint32_t* d_count,
                                                    uint32_t* d_pos, void* d_workspace, uint64_t workspace_bytes,
                                                    halo_stream_t stream);
/* The same outputs from a sequential loop over host arrays: no device, no scratch. */
HALO_API int halo_nat_collect_misses_host(const halo_nat_table_t* t, uint32_t dir, const halo_rx_result_t* records,
                                          const uint8_t* verdict, const uint8_t* select, uint32_t n,
                                          halo_nat_miss_item_t* items, uint32_t cap, uint32_t* count, uint32_t* pos);
/* Resolve (host memory only): the loop body of halo_nat_resolve_misses over items[0..k) in order —
 * the port mapping, then the host flow lookup, then NatAddFlow for LAN; nil becomes DROP, a WAN
 * miss stays MISS (ip, port 0; ref HALO_NAT_NO_FLOW), a hit stamps the flow with `now`. answers[j]
 * = {the translation, ref, verdict}; *n_added (optional) the flows added. */
HALO_API int halo_nat_resolve_items(halo_nat_table_t* t, uint32_t dir, const halo_nat_miss_item_t* items, uint32_t k,
                                    uint32_t now, halo_nat_answer_t* answers, uint32_t* n_added);
/* Apply: for a record with d_pos[i] < k, by d_answers[d_pos[i]].verdict —
 *   FLOW / MAPPING  what the device lookup would have written: ops[i].steps |= HALO_TX_NAT_DST (WAN)
 *                   or _SRC (LAN) and this direction's ip and port, nothing else; d_verdict[i] and
 *                   d_ref[i] are updated
 *   DROP            d_verdict[i] = DROP, d_ref[i] = HALO_NAT_NO_FLOW; the op is left alone
 *   MISS            nothing is written
 * A record with d_pos[i] == HALO_NAT_NO_FLOW or d_pos[i] >= k (its representative was beyond the
 * collect's cap) is left untouched: a later halo_nat_resolve_misses over what is still MISS
 * finishes the batch in the right order. d_counts (optional; HALO_NAT_V_DROP + 1 u32) is
 * INCREMENTED, per verdict, by the number of records with d_pos[i] < k. Ops and answers 16-byte
 * aligned. Needs no table. Asynchronous on `stream`. */
HALO_API int halo_nat_apply_answers_device(uint32_t dir, const uint32_t* d_pos, uint32_t n,
                                           const halo_nat_answer_t* d_answers, uint32_t k, halo_tx_op_t* d_ops,
                                           uint8_t* d_verdict, uint32_t* d_ref, uint32_t* d_counts,
                                           halo_stream_t stream);

/* ---- L2 switch: batched MAC learning and forwarding -----------------------------------------
 * engine.Switch / SwitchPort (engine/ethernet_engine.go:51-163, engine/engine.go:388-505): one MAC
 * table per switch, n_ports ports with a VlanId each. A batch is the frames ONE port received, in
 * receive order; frame i is handled exactly as SwitchPort.RxEthernet handles it after frames
 * 0..i-1 of the batch:
 *   1. ParseEthFrm: len < 42 || len > 1514 -> ETH_LEN; EtherType not in {0x05DC, 0x0800, 0x0806,
 *      0x86DD} -> ETH_TYPE. Nothing learned, nothing forwarded.
 *   2. src[0] & 1 -> SRC_MCAST. Nothing learned, nothing forwarded.
 *   3. learn: a source not in the table is inserted unless the table holds `capacity` entries
 *      (the failed MallocType, :79-83: TABLE_FULL, nothing forwarded); the entry's port = the
 *      ingress port and CreateTime = now, whether it is new or not.
 *   4. forward: dst in the table -> UNICAST to the entry's port (which may be the ingress port),
 *      else FLOOD to every other port of the ingress port's VLAN (halo_switch_flood_mask). The
 *      lookup sees what frames 0..i learned. Age is not checked: only halo_switch_expire removes.
 *   5. tx_len = BuildEthFrm's length, max(len, 60), for a forwarded frame; 0 for a dropped one.
 * Only bytes 0-13 of a frame and its length are read. The frame bytes reach per-port transmit
 * streams, padded, through halo_tx_egress_switch_device ("egress" below). Not covered: batches that
 * mix ingress ports, VLAN tags.
 *
 * A switch is either a host switch (cfg.device = -1: host pointers, the sequential loop, `stream`
 * ignored) or a device switch (cfg.device >= 0: device pointers; table, entry count and scratch
 * live in HBM and halo_switch_forward is asynchronous on `stream` with no host round trip).
 * ORDERING: calls on one switch are applied in call order. A device switch has ONE scratch set, so
 * every halo_switch_forward on it must be issued on one stream, or be ordered by the caller;
 * halo_switch_expire / _list / _layout_stats drain the device first and are synchronous. Calls on
 * one switch must not run concurrently from several host threads.
 * FAILURE: argument errors (HALO_E_INVAL / _RANGE) leave the switch as it was. HALO_E_HIP from a
 * device switch means a runtime call failed after the call had begun to change device state; the
 * table is then undefined, every later call on the switch returns HALO_E_HIP, and the only valid
 * call is halo_switch_destroy. */
typedef struct halo_switch halo_switch_t;
#define HALO_SW_MAX_PORTS 64u
typedef struct halo_switch_config {
    uint32_t n_ports;                    /* 1..64                                                   */
    uint16_t vlan_id[HALO_SW_MAX_PORTS]; /* SwitchPortConfig.VlanId of ports 0..n_ports-1           */
    uint32_t capacity;                   /* most MAC entries (the StaticAllocator's room); > 0      */
    uint32_t slots_log2;                 /* 0: automatic, the next power of two >= 2 * capacity;
                                            else exactly 2^slots_log2 slots (<= 28; tests force
                                            collisions with it). slots must exceed capacity         */
    uint32_t max_batch;                  /* most frames per halo_switch_forward (1..2^24)           */
    int device;                          /* -1: host mode; else the HIP device of the table         */
} halo_switch_config_t;
typedef struct halo_sw_result {
    uint8_t verdict;   /* HALO_SW_V_*                                  */
    uint8_t out_port;  /* the egress port of a UNICAST, else 0xFF      */
    uint16_t tx_len;   /* max(len, 60) when forwarded, else 0          */
} halo_sw_result_t;    /* 4 B */
#define HALO_SW_V_ETH_LEN 0u
#define HALO_SW_V_ETH_TYPE 1u
#define HALO_SW_V_SRC_MCAST 2u
#define HALO_SW_V_TABLE_FULL 3u
#define HALO_SW_V_UNICAST 4u
#define HALO_SW_V_FLOOD 5u
#define HALO_SW_V_COUNT 6u
#define HALO_SW_MAC_AGE 300u /* SwitchMacAddrClear: seconds */
typedef struct halo_switch_entry { /* engine.SwitchMacAddr */
    uint8_t mac[6];
    uint8_t port;          /* NetIf, as the port's index */
    uint8_t pad;
    uint32_t create_time;  /* CreateTime                 */
} halo_switch_entry_t;     /* 12 B */
typedef struct halo_switch_layout_stats {
    uint32_t slots;         /* slots of the device table (a power of two)                        */
    uint32_t entries;
    uint32_t longest_chain; /* most slots any entry's lookup reads (1 = at its home slot); 0 in host mode */
    uint32_t wrapped;       /* entries whose probe chain runs past the last slot to slot 0; 0 in host mode */
} halo_switch_layout_stats_t;

/* HALO_E_INVAL: null pointer, n_ports outside 1..64, capacity 0, slots <= capacity, slots_log2 >
 * 28, max_batch outside 1..2^24, device < -1. HALO_E_NODEV / _ARCH / _NOMEM as elsewhere. */
HALO_API int halo_switch_create(const halo_switch_config_t* cfg, halo_switch_t** out);
HALO_API int halo_switch_destroy(halo_switch_t* sw);
/* Bit q of *mask: a FLOOD from `port` goes out of port q (q != port, same VlanId). */
HALO_API int halo_switch_flood_mask(const halo_switch_t* sw, uint32_t port, uint64_t* mask);
/* One batch from ingress `port` at time `now` (Switch.TimeNow). Frame i is the lens[i] bytes at
 * bytes + 4 * offsets_dw[i], as halo_rx_parse_batch_device takes them. results[i] gets its verdict
 * (4-byte aligned); `counts`, if not NULL, is HALO_SW_V_COUNT u32 counters that are INCREMENTED.
 * HALO_E_INVAL: port >= n_ports, a null array with n > 0. HALO_E_RANGE: n > max_batch. n == 0 is OK. */
HALO_API int halo_switch_forward(halo_switch_t* sw, uint32_t port, const uint8_t* bytes, const uint32_t* offsets_dw,
                                 const uint16_t* lens, uint32_t n, uint32_t now, halo_sw_result_t* results,
                                 uint32_t* counts, halo_stream_t stream);
/* One SwitchMacAddrClear tick: every entry with now > (uint32_t)(CreateTime + 300) is removed
 * (the u32 add wraps, as Go's does). Synchronous; the room freed is usable by the next batch.
 * n_removed is optional. */
HALO_API int halo_switch_expire(halo_switch_t* sw, uint32_t now, uint32_t* n_removed);
/* ListSwitchMacAddr: up to `cap` entries into `out` (host memory; NULL with cap 0 to count),
 * *n = the total. Synchronises. Order unspecified. */
HALO_API int halo_switch_list(halo_switch_t* sw, halo_switch_entry_t* out, uint32_t cap, uint32_t* n);
HALO_API int halo_switch_layout_stats(halo_switch_t* sw, halo_switch_layout_stats_t* out);
/* TESTING ONLY — a device switch tags the entries of its per-call scratch set with a 16-bit call
 * number and clears the set when that number wraps, once in 65535 calls. This sets the number the
 * last call is taken to have had (0..65535; synchronous, clears the set), so that a test reaches
 * the wrap in a few calls. HALO_E_INVAL for a host switch. */
HALO_API int halo_switch_debug_set_epoch(halo_switch_t* sw, uint32_t epoch);

/* ---- ARP neighbour cache: batched next-hop resolve and L2 rewrite ----------------------------
 * A Router's ARP state (engine/arp_engine.go, protocol/arp.go): up to 64 NetIfs, each with its own
 * IpAddr and MacAddr, one cache keyed by (netif, ip) and one `capacity` shared by all NetIfs (the
 * room of the shared StaticAllocator). The host table is the control plane and the authority;
 * halo_arp_sync_device compiles it into an open-addressing table in HBM, and the last step of
 * Ipv4RouteForward (engine/ipv4_engine.go:180-201, :226-236, :267) — route id -> (next hop, out
 * NetIf) -> GetArpCache -> the Ethernet header TxEthernet / BuildEthFrm writes — runs on the GPU
 * over a device-resident batch, after halo_tx_fixup_batch_device in stream order. A gather kernel
 * brings a batch's ARP messages to the host in frame order for halo_arp_handle_msgs.
 *
 * Reference semantics kept, quirks included. All addresses are in IpAddrToU form.
 *   SetArpCache (:60-76): an absent key is inserted unless the table holds `capacity` entries (then
 *     nothing happens, silently); an existing key is always refreshed, also when the table is full;
 *     ExpTime = (uint32_t)(now + 300); the MAC is not checked (a group MAC is stored).
 *   GetArpCache (:31-46): ip == the NetIf's own IpAddr -> nil and no request; a present key -> the
 *     entry whatever its ExpTime (only a clear tick removes); an absent key -> nil, and the caller
 *     owes one SendArpReq per call (the reference does not deduplicate).
 *   HandleArp (:79-105), in this order: op (payload bytes 6-7) not 1 or 2 -> BAD_OP (bytes 0-5 are
 *     never checked); sha != the frame's Ethernet source -> SRC_MISMATCH; spa == own IpAddr ->
 *     CONFLICT; SetArpCache(spa, sha); a REQUEST whose tpa is the own IpAddr is answered even when
 *     the table was full; a reply that is not for us still learns.
 *   ArpTableClear (:129-147): every entry with now > ExpTime goes (plain u32 compare of a value that
 *     wrapped when stored). ArpTableRefresh (:108-126): one request per entry with
 *     now > (uint32_t)(ExpTime - 10); the subtraction wraps, so ExpTime < 10 is never refreshed.
 *
 * ORDERING: device lookups see the table as of the last halo_arp_sync_device (or the last
 * halo_arp_expire that removed an entry). An entry learned since is a device MISS — a dropped
 * packet and a redundant request, what the reference gives a packet that arrives just before the
 * ARP reply. The engine loop re-syncs when halo_arp_dirty.
 * FAILURE: argument errors (HALO_E_INVAL / _RANGE) leave the table as it was; a malformed ARP
 * message is data (its verdict). A library built without the device side answers HALO_E_NODEV to
 * the *_device calls.
 * A forwarded frame is not padded in place (frames are packed at 4-byte boundaries and the padding
 * would overwrite a neighbour): tx_len tells the caller, and halo_tx_egress_arp_device ("egress"
 * below) writes the padded copy and the per-port index lists.
 * Locally originated packets take TxIpv4's variant of the step, halo_arp_encap_tx_device, on the
 * frames halo_tx_build_batch_device built ("local responders" below).
 * Not covered: Router.Ipv4PktFwdHook; compact records in the gather (DHCP: its own section below);
 * UDP service replies (the handlers' job). The LoChan copy of a LOOPBACK: halo_lo_gather_device
 * ("loopback" below). */
typedef struct halo_arp_table halo_arp_table_t;
#define HALO_ARP_MAX_NETIFS 64u
#define HALO_ARP_AGE 300u          /* SetArpCache: ExpTime = now + 300             */
#define HALO_ARP_REFRESH_AHEAD 10u /* ArpTableRefresh: now > ExpTime - 10          */
typedef struct halo_arp_config {
    uint32_t n_netifs;                          /* 1..64                                                */
    halo_rx_netif_t netif[HALO_ARP_MAX_NETIFS]; /* NetIfs 0..n_netifs-1: mac, ip and nat_enable are read */
    uint32_t capacity;                          /* most entries, all NetIfs together; > 0               */
    uint32_t slots_log2;                        /* 0: automatic, the next power of two >= 2 * capacity;
                                                   else exactly 2^slots_log2 slots (<= 28; tests force
                                                   collisions with it). slots must exceed capacity       */
} halo_arp_config_t;
typedef struct halo_arp_entry { /* engine.ArpCache, with the NetIf whose table holds it */
    uint32_t ip;       /* IpAddr  */
    uint8_t mac[6];    /* MacAddr */
    uint8_t netif;
    uint8_t pad;
    uint32_t exp_time; /* ExpTime */
} halo_arp_entry_t;    /* 16 B */
typedef struct halo_arp_msg { /* one received ARP message, as halo_arp_gather_device writes it */
    uint32_t index;     /* the frame's index in its batch          */
    uint8_t netif;      /* the NetIf that received it              */
    uint8_t pad;
    uint8_t eth_src[6]; /* frame bytes 6-11                         */
    uint8_t arp[28];    /* frame bytes 14-41, verbatim              */
} halo_arp_msg_t;       /* 40 B */
/* halo_arp_handle_msgs verdict byte: one HALO_ARP_H_* code | flag bits */
#define HALO_ARP_H_BAD_OP 0u
#define HALO_ARP_H_SRC_MISMATCH 1u
#define HALO_ARP_H_CONFLICT 2u
#define HALO_ARP_H_ACCEPTED 3u
#define HALO_ARP_H_COUNT 4u
#define HALO_ARP_H_MASK 0x0Fu
#define HALO_ARP_H_F_NOT_LEARNED 0x40u /* ACCEPTED, but SetArpCache found the table full */
#define HALO_ARP_H_F_REPLY 0x80u       /* a reply frame was built                         */
/* halo_arp_get's *found */
#define HALO_ARP_GET_ABSENT 0u /* nil; the caller owes a SendArpReq          */
#define HALO_ARP_GET_FOUND 1u
#define HALO_ARP_GET_OWN_IP 2u /* nil; ip is the NetIf's own, no request     */
/* verdicts of halo_arp_lookup_device (NONE, OWN_IP, MISS, HIT) and halo_arp_encap_device (all) */
#define HALO_ARP_V_NONE 0u        /* not selected, not an IPv4 frame of >= 34 bytes, a route id or
                                     NetIf the device copy does not know: nothing read or written  */
#define HALO_ARP_V_NO_ROUTE 1u    /* HALO_ROUTE_NONE                                               */
#define HALO_ARP_V_ROUTE_PANIC 2u /* HALO_ROUTE_PANIC                                              */
#define HALO_ARP_V_LOOPBACK 3u    /* dst == the out NetIf's IpAddr, in NetIf not NATing (:180-201);
                                     the LoChan copy: halo_lo_gather_device ("loopback")          */
#define HALO_ARP_V_OWN_IP 4u      /* GetArpCache(own IpAddr): nil, no request                      */
#define HALO_ARP_V_MISS 5u        /* nil: the packet is dropped, one SendArpReq(target_ip) is owed */
#define HALO_ARP_V_HIT 6u         /* the frame's bytes 0-11 were rewritten                         */
#define HALO_ARP_V_COUNT 7u
typedef struct halo_arp_result {
    uint8_t verdict;    /* HALO_ARP_V_*                                                          */
    uint8_t out_netif;  /* the route's NetIf (LOOPBACK, OWN_IP, MISS, HIT), else 0xFF            */
    uint16_t tx_len;    /* BuildEthFrm's length, max(len, 60), on HIT; else 0                    */
    uint32_t target_ip; /* the address looked up (OWN_IP, MISS, HIT): next hop or dst; else 0    */
} halo_arp_result_t;    /* 8 B */
typedef struct halo_arp_layout_stats {
    uint32_t slots;         /* slots of the device table (a power of two)                          */
    uint32_t entries;
    uint32_t longest_chain; /* most slots any entry's lookup reads (1 = at its home slot)          */
    uint32_t wrapped;       /* entries whose probe chain runs past the last slot to slot 0         */
} halo_arp_layout_stats_t;

/* HALO_E_INVAL: null pointer, n_netifs outside 1..64, capacity 0, slots <= capacity, slots_log2 > 28. */
HALO_API int halo_arp_table_create(const halo_arp_config_t* cfg, halo_arp_table_t** out);
HALO_API int halo_arp_table_destroy(halo_arp_table_t* t);
/* SetArpCache on NetIf `netif` at time `now` (Router.TimeNow). HALO_E_RANGE: netif >= n_netifs. */
HALO_API int halo_arp_set(halo_arp_table_t* t, uint32_t netif, uint32_t ip, const uint8_t mac[6], uint32_t now);
/* GetArpCache on the host table: *found = HALO_ARP_GET_*; *entry (optional) is filled when FOUND. */
HALO_API int halo_arp_get(const halo_arp_table_t* t, uint32_t netif, uint32_t ip, halo_arp_entry_t* entry,
                          uint32_t* found);
/* HandleArp over msgs[0..n) in ascending order at time `now`. verdicts[i] = HALO_ARP_H_* | flags.
 * The k-th reply built (60 bytes: BuildArpPkt(REPLY, own mac, own ip, sha, spa) inside
 * BuildEthFrm(dst = sha, src = own mac, 0x0806), zero-padded) goes to reply_frames + 60 * k when
 * reply_frames is not NULL — only 60 bytes per reply are written, so 60 * n always suffices;
 * *n_replies counts them either way. *n_changed = inserts + entries whose MAC changed: what makes a re-sync worthwhile.
 * n_replies / n_changed are optional. HALO_E_RANGE, nothing applied: a msgs[i].netif >= n_netifs. */
HALO_API int halo_arp_handle_msgs(halo_arp_table_t* t, const halo_arp_msg_t* msgs, uint32_t n, uint32_t now,
                                  uint8_t* verdicts, uint8_t* reply_frames, uint32_t* n_replies,
                                  uint32_t* n_changed);
/* SendArpReq(target_ip) of NetIf `netif`: BuildArpPkt(REQUEST, mac, ip, ff:ff:ff:ff:ff:ff, target)
 * — the body's target MAC is the broadcast MAC, not zeros — to the Ethernet broadcast, padded to
 * 60 bytes. target_ip == the NetIf's own ip is SendFreeArp. */
HALO_API int halo_arp_build_request(const halo_arp_table_t* t, uint32_t netif, uint32_t target_ip, uint8_t out[60]);
/* One ArpTableClear tick. Synchronous; when it removed an entry and a device copy exists, the copy
 * is rebuilt and published before the call returns. n_removed is optional. */
HALO_API int halo_arp_expire(halo_arp_table_t* t, uint32_t now, uint32_t* n_removed);
/* One ArpTableRefresh tick: the (netif, ip) of up to `cap` entries to SendArpReq for; *n = the total. */
HALO_API int halo_arp_refresh_list(const halo_arp_table_t* t, uint32_t now, uint8_t* netif_out, uint32_t* ip_out,
                                   uint32_t cap, uint32_t* n);
/* ListArp of every NetIf: up to `cap` entries (NULL with cap 0 to count), *n = the total. */
HALO_API int halo_arp_list(const halo_arp_table_t* t, halo_arp_entry_t* out, uint32_t cap, uint32_t* n);
/* The layout halo_arp_sync_device would upload now. Host only. */
HALO_API int halo_arp_layout_stats(const halo_arp_table_t* t, halo_arp_layout_stats_t* out);
/* 1 when the host table differs from the last published device copy (or none exists): an insert or
 * a changed MAC since. A refresh of ExpTime alone does not count — the device holds no ExpTime. */
HALO_API int halo_arp_dirty(const halo_arp_table_t* t);

/* Compile the cache into HBM on `device` and publish it (synchronous): 16-byte slots {ip, used |
 * netif, mac[0..3], mac[4..5]}, linear probing from a splitmix64 finaliser of (netif << 32 | ip),
 * more slots than `capacity` so every chain ends at an empty slot, rebuilt by every sync (no
 * tombstones); the NetIf array; and, when `routes` is not NULL, a {next_hop, netif} array indexed by
 * route id, read through halo_route_get for ids 0, 1, ... until HALO_E_RANGE (ids are never
 * reused). Two generations under halo_nat_sync_device's discipline: the unused one is rewritten
 * after a device drain and published with a release store; a lookup holds the table's read lock
 * from taking its view until its kernel is enqueued. One device per table; the caller's current
 * device is restored. */
HALO_API int halo_arp_sync_device(halo_arp_table_t* t, const halo_route_table_t* routes, int device);
/* GetArpCache for n (netif, ip) pairs: d_netifs[i], or `netif` for all when d_netifs is NULL.
 * d_verdict[i] = NONE (netif >= n_netifs), OWN_IP, MISS or HIT; d_mac8[8 * i .. + 6) = the MAC on HIT
 * (8 bytes per entry, 8-byte aligned, zero otherwise). *d_miss_count is INCREMENTED by the MISSes.
 * Read-only on the table (the reference does not touch ExpTime on use). Asynchronous on `stream`.
 * HALO_E_INVAL before the first sync. n == 0 is OK. */
HALO_API int halo_arp_lookup_device(const halo_arp_table_t* t, const uint32_t* d_ips, const uint8_t* d_netifs,
                                    uint32_t netif, uint32_t n, uint8_t* d_mac8, uint8_t* d_verdict,
                                    uint32_t* d_miss_count, halo_stream_t stream);
/* The forward path's L2 step for frames (ragged layout) that NetIf `in_netif` received, given the
 * route id FindRoute returned for each. d_select (optional): d_select[i] == 0 -> NONE (pass, for
 * instance, the fixup result's HALO_TX_R_TTL_ALIVE bit). A selected frame shorter than 34 bytes, or
 * whose bytes 12-13 are not 08 00, or whose route id is beyond the uploaded array (or names a NetIf
 * >= n_netifs) -> NONE, and no byte of it is read past its length or written. Otherwise:
 *   HALO_ROUTE_NONE -> NO_ROUTE; HALO_ROUTE_PANIC -> ROUTE_PANIC;
 *   dst (the frame's CURRENT bytes 30-33, so the post-DNAT address) == netif[out].ip and
 *     netif[in_netif].nat_enable == 0 -> LOOPBACK;
 *   target = the route's next_hop when nonzero, else dst; target == netif[out].ip -> OWN_IP;
 *   target absent -> MISS; present -> HIT: bytes 0-5 = the entry's MAC, bytes 6-11 = netif[out].mac
 *   (exactly bytes 0-11 are written), tx_len = max(len, 60).
 * d_results: 8-byte aligned. d_counts (optional): HALO_ARP_V_COUNT u32 counters, INCREMENTED;
 * *d_miss_count is INCREMENTED by the MISSes. Asynchronous on `stream`. HALO_E_INVAL before the
 * first sync and when the last sync had routes == NULL; HALO_E_RANGE: in_netif >= n_netifs. */
HALO_API int halo_arp_encap_device(const halo_arp_table_t* t, uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                   const uint16_t* d_lens, uint32_t n, const uint32_t* d_route_ids,
                                   uint32_t in_netif, const uint8_t* d_select, halo_arp_result_t* d_results,
                                   uint32_t* d_counts, uint32_t* d_miss_count, halo_stream_t stream);
/* TxIpv4's L3 / L2 step (engine/ipv4_engine.go:50-99) for frames NetIf `self_netif` originated —
 * the slots halo_tx_build_batch_device filled, with the route id FindRoute(dst) returned for each.
 * Arguments, outputs, counters and errors are halo_arp_encap_device's, with two differences:
 *   a destination whose last byte (frame byte 33) is 255: the route id is not consulted; HIT,
 *     out_netif = self_netif, bytes 0-5 = ff x 6, bytes 6-11 = netif[self_netif].mac, tx_len =
 *     max(len, 60), target_ip = 0 (:60-61, :85-86, :92-93);
 *   otherwise dst == netif[out].ip -> LOOPBACK whatever nat_enable says (:71-80). The LoChan copy,
 *     exactly totalLen bytes from byte 14, is halo_lo_gather_device's with HALO_LO_TX ("loopback").
 * Everything else is unchanged: NONE (also a slot that was not built: length 0), NO_ROUTE,
 * ROUTE_PANIC, OWN_IP, MISS, HIT and the exact bytes written. HALO_E_RANGE: self_netif >= n_netifs. */
HALO_API int halo_arp_encap_tx_device(const halo_arp_table_t* t, uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                      const uint16_t* d_lens, uint32_t n, const uint32_t* d_route_ids,
                                      uint32_t self_netif, const uint8_t* d_select, halo_arp_result_t* d_results,
                                      uint32_t* d_counts, uint32_t* d_miss_count, halo_stream_t stream);
/* The ARP messages of a parsed batch: the records halo_rx_dispatch maps to HALO_RX_ACT_ARP (status
 * OK, EtherType 0x0806, MAC_MATCH) written densely to d_msgs (8-byte aligned) in ascending frame
 * index, with `netif` in every message. *d_count is SET to the number selected, also beyond `cap`;
 * only the first `cap` are written. Reads bytes 6-11 and 14-41 of a selected frame and nothing of
 * any other. d_workspace: halo_arp_gather_workspace(n) bytes, 4-byte aligned. Three launches on
 * `stream` (tile counts, scan, scatter). */
HALO_API uint64_t halo_arp_gather_workspace(uint32_t n);
HALO_API int halo_arp_gather_device(const uint8_t* d_bytes, const uint32_t* d_offsets_dw, const uint16_t* d_lens,
                                    const halo_rx_result_t* d_records, uint32_t n, uint32_t netif,
                                    halo_arp_msg_t* d_msgs, uint32_t cap, uint32_t* d_count, void* d_workspace,
                                    uint64_t workspace_bytes, halo_stream_t stream);

/* ---- port-mapping return flows: source-in, source-out -----------------------------------------
 * The Router's NatPortMappingFlowTable (engine/ipv4_engine.go:160-186, :203-207, :238-266,
 * :489-516): what sends the replies of a statically port-forwarded connection back out of the WAN
 * NetIf the connection came in on, with that NetIf's address and the mapping's WAN port as source.
 * One table per Router. The host table is the control plane and the authority; halo_pmflow_sync_device
 * compiles it into an open-addressing table in HBM and the two per-packet halves run on the GPU:
 *
 *   reference                                      here
 *   :160-179  Get(reversed 5-tuple) on a non-NAT   halo_pmflow_lookup_device over the records the
 *             in-NetIf, LastAliveTime = TimeNow    LAN-side NetIf received (host: halo_pmflow_get)
 *   :180-186  out NetIf / next hop forced to the   d_via[i] = OVERRIDE, consumed by
 *             flow's WanNetIf and its Gateway      halo_arp_encap_via_device
 *   :203-207  NatChangeSrc(outNetIf.IpAddr,        ops[i]: HALO_TX_NAT_SRC, src_ip, src_port; d_hit[i]
 *             flow.WanPort) ahead of the           = 1 is the d_skip of the out NetIf's
 *             out-NetIf's own mapping / flow       halo_nat_lookup_lan_device
 *   :238-266  Get / MallocType / Set after route   halo_pmflow_record_device lists the frames after
 *             and ARP succeeded; full -> return    halo_arp_encap_device; halo_pmflow_record applies
 *             before TxEthernet                    them in frame order; dropped_out ->
 *                                                  halo_arp_drop_device
 *   :497-516  NatPortMappingFlowClear              halo_pmflow_expire
 *
 * KEY: the whole 13-byte NatFlowHash {remote_ip, remote_port, lan_ip, lan_port, proto}, compared
 * whole, normalised by no NAT type. VALUE: {wan_netif (an index, as everywhere here), wan_port,
 * last_alive, id}; ids are fresh per insert and never reused, and LastAliveTime lives on the device
 * as one u32 per id shared by both generations, exactly as the NAT flow table's does (above).
 * Only TCP and UDP flows can exist: the record is made for a NatPortMappingEntry, and
 * CheckNatPortMapping (:683-707) matches no other protocol. halo_pmflow_record therefore refuses an
 * item of another protocol (HALO_E_INVAL), and the device lookup answers such a record (ICMP, ...)
 * MISS without a probe.
 * STAMPING: the reference stamps only packets that passed the TTL step (:133-142). Records carry
 * no TTL, so a caller that does not deselect dead packets (d_select) stamps for them too — the
 * convention the NAT lookups already have.
 * ORDERING: device lookups see the table as of the last halo_pmflow_sync_device (or the last
 * halo_pmflow_expire that removed a flow). A flow recorded since is a device MISS for the lookup
 * (halo_pmflow_get on the host answers for it) and is listed again by halo_pmflow_record_device,
 * where halo_pmflow_record overwrites it identically: results do not depend on the sync cadence.
 * FAILURE: argument errors (HALO_E_INVAL / _RANGE) leave the table as it was and are checked before
 * a device is looked for. A library built without the device side answers HALO_E_NODEV to the
 * *_device calls. Not covered: Router.Ipv4PktFwdHook; device-side inserts (order and the
 * capacity check depend on frame order, as NatAddFlow's do); interface names. */
typedef struct halo_pmflow_table halo_pmflow_table_t;
typedef struct halo_pmflow_config {
    uint32_t n_netifs;                          /* 1..64                                               */
    halo_rx_netif_t netif[HALO_ARP_MAX_NETIFS]; /* NetIfs 0..n_netifs-1: ip and nat_enable are read    */
    uint32_t gateway[HALO_ARP_MAX_NETIFS];      /* IpAddrToU(NetIf.Gateway); 0 for nil                 */
    uint32_t capacity;                          /* most flows (the StaticAllocator's room); > 0        */
    uint32_t capacity_log2;                     /* 0: automatic (load <= 0.5); else the device table has
                                                   exactly 2^capacity_log2 slots (<= 28; tests). A table
                                                   that does not fit (entries >= slots) makes sync /
                                                   layout_stats return HALO_E_RANGE                     */
} halo_pmflow_config_t;
typedef struct halo_pmflow_item { /* one frame to record, as halo_pmflow_record_device writes it */
    uint32_t index;       /* the frame's index in its batch                  */
    uint32_t remote_ip;   /* the frame's source address                      */
    uint32_t lan_ip;      /* NatPortMappingEntry.LanHostIpAddr               */
    uint16_t remote_port; /* the frame's source port                         */
    uint16_t lan_port;    /* NatPortMappingEntry.LanHostPort                 */
    uint16_t wan_port;    /* NatPortMappingEntry.WanPort                     */
    uint8_t proto;        /* 6 or 17                                         */
    uint8_t pad;
} halo_pmflow_item_t;     /* 20 B */
typedef struct halo_pmflow_entry { /* a NatPortMappingFlow with its key */
    uint32_t remote_ip;
    uint32_t lan_ip;
    uint32_t last_alive; /* LastAliveTime (host copy; device stamps are folded in by expire / sync) */
    uint32_t id;
    uint16_t remote_port;
    uint16_t lan_port;
    uint16_t wan_port;   /* WanPort  */
    uint8_t proto;
    uint8_t wan_netif;   /* WanNetIf */
} halo_pmflow_entry_t;   /* 24 B */
#define HALO_PMFLOW_V_NONE 0u     /* ip_proto == 0xFF or not selected: nothing looked up                */
#define HALO_PMFLOW_V_MISS 1u     /* no flow: the route and the out NetIf's own NAT lookup decide        */
#define HALO_PMFLOW_V_HIT 2u      /* a flow, and the route already points at its WAN NetIf (or the route
                                     id is HALO_ROUTE_PANIC, which the encap reports)                    */
#define HALO_PMFLOW_V_OVERRIDE 3u /* a flow, and the route names another NetIf, none (HALO_ROUTE_NONE:
                                     an empty outNetIfName differs from any WanNetIf, :182) or an id the
                                     device copy does not know: (out NetIf, next hop) are forced          */
#define HALO_PMFLOW_V_COUNT 4u
typedef struct halo_pmflow_via {
    uint8_t verdict;    /* HALO_PMFLOW_V_*                                   */
    uint8_t wan_netif;  /* HIT, OVERRIDE: the flow's WanNetIf; else 0xFF     */
    uint16_t wan_port;  /* HIT, OVERRIDE: the flow's WanPort; else 0         */
    uint32_t next_hop;  /* HIT, OVERRIDE: gateway[wan_netif]; else 0         */
} halo_pmflow_via_t;    /* 8 B */
typedef struct halo_pmflow_layout_stats {
    uint32_t slots;
    uint32_t entries;
    uint32_t longest_chain; /* most slots any entry's lookup reads (1 = at its home slot) */
    uint32_t wrapped;       /* entries whose probe chain runs past the last slot to slot 0 */
} halo_pmflow_layout_stats_t;

/* HALO_E_INVAL: null pointer, n_netifs outside 1..64, capacity 0; HALO_E_RANGE: capacity_log2 > 28. */
HALO_API int halo_pmflow_table_create(const halo_pmflow_config_t* cfg, halo_pmflow_table_t** out);
HALO_API int halo_pmflow_table_destroy(halo_pmflow_table_t* t);
/* :238-266 for items[0..k) in ascending order, frames NetIf `in_netif` received, at time `now`.
 * An absent key is inserted unless the table holds `capacity` flows: then dropped_out[j] = 1 (the
 * reference returns before TxEthernet: the frame is not sent) and nothing is stored. A present key
 * always has wan_netif = in_netif, wan_port and last_alive overwritten, also when the table is full.
 * dropped_out[j] = 0 otherwise. *n_added (optional) = the inserts. HALO_E_RANGE: in_netif >=
 * n_netifs. HALO_E_INVAL, nothing applied: a null array with k > 0, an item whose proto is not 6 or 17. */
HALO_API int halo_pmflow_record(halo_pmflow_table_t* t, uint32_t in_netif, const halo_pmflow_item_t* items,
                                uint32_t k, uint32_t now, uint8_t* dropped_out, uint32_t* n_added);
/* The host lookup of :164-179: *found = 1 and *out (optional) = the flow, or *found = 0. When
 * now_or_no_stamp is not NULL a found flow's LastAliveTime = *now_or_no_stamp (:176), and *out
 * shows it. */
HALO_API int halo_pmflow_get(halo_pmflow_table_t* t, uint32_t remote_ip, uint16_t remote_port, uint32_t lan_ip,
                             uint16_t lan_port, uint8_t proto, const uint32_t* now_or_no_stamp,
                             halo_pmflow_entry_t* out, uint32_t* found);
/* One NatPortMappingFlowClear tick (:497-516): every flow with (uint32_t)(now - LastAliveTime) > 60
 * leaves. The stamps the device wrote are folded in first, the later in serial-number order as
 * halo_nat_expire does, so THE CALLER MUST HAVE SYNCHRONISED THE STREAMS ITS LOOKUPS RAN ON. When
 * flows were removed and a device copy exists, it is rebuilt and published before the call returns. */
HALO_API int halo_pmflow_expire(halo_pmflow_table_t* t, uint32_t now, uint32_t* n_removed);
/* Up to `cap` flows in ascending id (NULL with cap 0 to count), *n = the total. */
HALO_API int halo_pmflow_list(const halo_pmflow_table_t* t, halo_pmflow_entry_t* out, uint32_t cap, uint32_t* n);
/* The layout halo_pmflow_sync_device would upload now. Host only. */
HALO_API int halo_pmflow_layout_stats(const halo_pmflow_table_t* t, halo_pmflow_layout_stats_t* out);
/* 1 when the host table differs from the published device copy (or none exists): an insert, a
 * changed wan_netif / wan_port or a removal since. A refreshed LastAliveTime alone does not count. */
HALO_API int halo_pmflow_dirty(const halo_pmflow_table_t* t);
/* Compile the table into HBM on `device` and publish it (synchronous): 32-byte slots {remote ip,
 * lan ip, remote port | lan port << 16, used | proto; wan_netif, wan_port, id, pad} placed by linear
 * probing from XXH3-64(key) & (slots - 1), the hash of halo_flow_hash_device; the NetIf {ip,
 * nat_enable, gateway} array; and, when `routes` is not NULL, the NetIf of every route id, read
 * through halo_route_get as halo_arp_sync_device reads it. Two generations under
 * halo_nat_sync_device's discipline (drain, fold the stamps, rewrite the unused generation,
 * release-publish; a lookup holds the read lock until its kernel is enqueued). One device per table. */
HALO_API int halo_pmflow_sync_device(halo_pmflow_table_t* t, const halo_route_table_t* routes, int device);
/* The LAN-side half (:160-186, :203-207) for the records a non-NAT NetIf received, given the route
 * id FindRoute returned for each. Key: remote = dst_ip : dport, LAN host = src_ip : sport, ip_proto.
 *   ip_proto == 0xFF, or d_select && d_select[i] == 0 -> NONE
 *   ip_proto not 6 / 17, or no such flow              -> MISS
 *   a flow -> its stamp = now (plain store), then HIT / OVERRIDE as defined above; if
 *     netif[wan_netif].nat_enable: ops[i].steps |= HALO_TX_NAT_SRC, src_ip = netif[wan_netif].ip,
 *     src_port = wan_port. No other op field is written, and no op of a NONE or MISS record.
 * d_via[i] (8-byte aligned) and d_hit[i] (1 on HIT / OVERRIDE, else 0: the d_skip of the out NetIf's
 * halo_nat_lookup_lan_device) are written for every record. d_counts (optional):
 * HALO_PMFLOW_V_COUNT u32 counters, INCREMENTED. Records and ops 16-byte aligned; route ids and
 * counts 4. HALO_E_INVAL before the first sync and when the last sync had routes == NULL. n == 0
 * is OK. Asynchronous on `stream`. */
HALO_API int halo_pmflow_lookup_device(const halo_pmflow_table_t* t, const halo_rx_result_t* d_records, uint32_t n,
                                       uint32_t now, const uint32_t* d_route_ids, const uint8_t* d_select,
                                       halo_tx_op_t* d_ops, halo_pmflow_via_t* d_via, uint8_t* d_hit,
                                       uint32_t* d_counts, halo_stream_t stream);
/* The WAN-side half (:238-266) for the frames NATing NetIf `in_netif` received, after
 * halo_arp_encap_device in stream order. Frame i is a candidate when d_wan_verdict[i] ==
 * HALO_NAT_V_MAPPING and d_arp_results[i].verdict == HALO_ARP_V_HIT; its key is remote = the record's
 * src_ip : sport, LAN host = ops[i].dst_ip : dst_port, the record's ip_proto; wan_port = the record's
 * dport. A candidate the device copy holds with the same (wan_netif = in_netif, wan_port) is only
 * stamped with `now`; every other candidate is written densely to d_items (4-byte aligned) in
 * ascending frame index, for halo_pmflow_record. *d_count is SET to the number listed, also beyond
 * `cap`; only the first `cap` are written. d_workspace: halo_pmflow_record_workspace(n) bytes, 4-byte
 * aligned; one workspace serves any number of calls on one stream. Three launches (count, scan,
 * scatter). HALO_E_INVAL before the first sync; HALO_E_RANGE: in_netif >= n_netifs. */
HALO_API uint64_t halo_pmflow_record_workspace(uint32_t n);
HALO_API int halo_pmflow_record_device(const halo_pmflow_table_t* t, uint32_t in_netif,
                                       const halo_rx_result_t* d_records, const uint8_t* d_wan_verdict,
                                       const halo_tx_op_t* d_ops, const halo_arp_result_t* d_arp_results, uint32_t n,
                                       uint32_t now, halo_pmflow_item_t* d_items, uint32_t cap, uint32_t* d_count,
                                       void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream);
/* For the frames halo_pmflow_record dropped: d_results[d_index[j]] = {HALO_ARP_V_NONE, 0xFF, 0, 0}
 * for j < k, so that halo_tx_egress_arp_device leaves them out. Bytes 0-11 of such a frame were
 * already rewritten by the encap and stay so. Every d_index[j] must be below the batch size. */
HALO_API int halo_arp_drop_device(halo_arp_result_t* d_results, const uint32_t* d_index, uint32_t k,
                                  halo_stream_t stream);
/* halo_arp_encap_device with the return-flow override (:180-186). Where d_via[i].verdict ==
 * HALO_PMFLOW_V_OVERRIDE, (next hop, out NetIf) = (d_via[i].next_hop, d_via[i].wan_netif) and the
 * route id is not consulted; a wan_netif >= n_netifs gives NONE. Everything after that point is
 * halo_arp_encap_device's: LOOPBACK against netif[out].ip with the in NetIf's nat_enable, target =
 * next hop when nonzero else dst, OWN_IP / MISS / HIT. d_via: 8-byte aligned; NULL: the results
 * equal halo_arp_encap_device's. */
HALO_API int halo_arp_encap_via_device(const halo_arp_table_t* t, uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                       const uint16_t* d_lens, uint32_t n, const uint32_t* d_route_ids,
                                       uint32_t in_netif, const uint8_t* d_select, const halo_pmflow_via_t* d_via,
                                       halo_arp_result_t* d_results, uint32_t* d_counts, uint32_t* d_miss_count,
                                       halo_stream_t stream);

/* ---- egress: per-port transmit streams in ring-record form -----------------------------------
 * The forward path's last step: TxEthernet -> BuildEthFrm (zero-pad to 60 bytes) -> EthTxFunc ->
 * RingBufferProducer.WritePacket into the egress port's tx ring (engine/ethernet_engine.go:34-49,
 * :117-129, protocol/ethernet.go:58-82, dpdk/dpdk.go:202-213, mem/ring_buffer.go:249-295). A stable
 * multi-way partition of a device-resident ragged batch into one contiguous byte stream per egress
 * port: port p's stream starts at d_out + p * region_bytes and holds the port's frames in ascending
 * frame index, each laid out exactly as one ring record:
 *   u32 little-endian tx_len = max(len, 60); the frame's len bytes; zeros up to tx_len (BuildEthFrm's
 *   padding); zeros up to the next 4-byte boundary. Record size = (4 + tx_len + 3) & ~3.
 * WritePacket leaves the alignment bytes unwritten; zero is this build's definition, so that outputs
 * compare whole. halo_ring_write_span then publishes a stream into a tx ring with one or two copies
 * and one release store of head.
 *
 * WHICH PORTS a frame goes to (bits at or above n_ports are ignored everywhere):
 *   masks:  bit p of d_masks[i].
 *   arp:    verdict == HALO_ARP_V_HIT -> port out_netif; every other verdict -> nowhere.
 *   switch: UNICAST -> out_port (which may be the ingress port, as in the reference); FLOOD -> every
 *           bit of flood_mask, the value halo_switch_flood_mask gives for the batch's ingress port;
 *           every other verdict -> nowhere. The order among the ports of a flood is not observable
 *           (the streams are separate; the reference iterates a Go map there).
 * SENDABLE: 14 <= len <= 1514 (9014 with HALO_RX_JUMBO_EXT): BuildEthFrm refuses a payload over 1500
 *   bytes and TxEthernet then sends nothing. A frame selected for at least one port below n_ports
 *   but not sendable is emitted nowhere and counted once in *d_skipped (optional, INCREMENTED).
 * REGION OVERFLOW (build-defined): port p's records are written while they fit wholly in
 *   region_bytes; the first record that does not fit ends the port's written prefix. `frames` and
 *   `bytes` are still the totals, as halo_arp_gather_device's *d_count is beyond `cap`, so the caller
 *   can resubmit the tail. (WritePacket on a full ring drops one frame and may take a later, shorter
 *   one.)
 * INDEX LISTS: d_index[p * index_cap + k] = the batch index of port p's k-th record; the first
 *   min(frames, index_cap) entries per port are written, also for records beyond the region.
 * READS: nothing of a frame that is not selected and sendable; nothing past the 4-byte word that
 *   holds a selected frame's last byte, and the bytes of that word beyond len (a neighbour's, or a
 *   gap's) do not reach the output. The input batch is never written.
 * WRITES: exactly [p * region_bytes, p * region_bytes + bytes_written) of each port, the n_ports
 *   summaries, the index entries above, *d_skipped; nothing else.
 * The device calls are asynchronous on `stream` with no host round trip: three launches (per-tile
 * counts, a scan over tiles, the scatter). n == 0 is OK and zeroes the summaries. Every argument is
 * checked before any device call. HALO_E_INVAL: a null cfg / d_ports, a null array with n > 0,
 * n_ports outside 1..64, flags other than HALO_RX_JUMBO_EXT, region_bytes not a multiple of 16,
 * d_out null with region_bytes > 0 or not 16-byte aligned, d_index null with index_cap > 0, a
 * misaligned array (offsets, index, skipped: 4; lens: 2; masks, arp results, summaries, workspace: 8;
 * switch results: 4), workspace_bytes < halo_tx_egress_workspace(n, n_ports). HALO_E_NODEV / _ARCH
 * as elsewhere. */
#define HALO_EGRESS_MAX_PORTS 64u
#define HALO_EGRESS_KIND_MASKS 0u  /* halo_tx_egress_host's `kind`: selectors are uint64_t masks  */
#define HALO_EGRESS_KIND_ARP 1u    /* ... halo_arp_result_t                                        */
#define HALO_EGRESS_KIND_SWITCH 2u /* ... halo_sw_result_t, with flood_mask                        */
typedef struct halo_egress_port { /* SET by the call, one per port */
    uint32_t frames;         /* records selected for the port, also beyond the region */
    uint32_t frames_written; /* the prefix of them that fits the region wholly        */
    uint64_t bytes;          /* sum of their record sizes                             */
    uint64_t bytes_written;  /* <= region_bytes; a whole number of records            */
} halo_egress_port_t;        /* 24 B */
typedef struct halo_egress_config {
    uint32_t n_ports;      /* 1..64                                                                  */
    uint32_t flags;        /* HALO_RX_JUMBO_EXT lifts the 1514-byte cap to 9014, as elsewhere        */
    uint64_t region_bytes; /* port p's stream starts at d_out + p * region_bytes; a multiple of 16
                              for the device calls                                                   */
    uint32_t index_cap;    /* entries per port in d_index (0 with d_index NULL)                      */
    uint32_t reserved;     /* 0                                                                      */
} halo_egress_config_t;    /* 24 B */
/* Bytes of device workspace (8-byte aligned) a call over n frames and n_ports ports needs; 0 for
 * n_ports outside 1..64. One workspace serves any number of calls issued on one stream. */
HALO_API uint64_t halo_tx_egress_workspace(uint32_t n, uint32_t n_ports);
HALO_API int halo_tx_egress_masks_device(const halo_egress_config_t* cfg, const uint8_t* d_bytes,
                                         const uint32_t* d_offsets_dw, const uint16_t* d_lens, uint32_t n,
                                         const uint64_t* d_masks, uint8_t* d_out, halo_egress_port_t* d_ports,
                                         uint32_t* d_index, uint32_t* d_skipped, void* d_workspace,
                                         uint64_t workspace_bytes, halo_stream_t stream);
/* After halo_arp_encap_device in stream order: HIT frames carry the rewritten MACs. */
HALO_API int halo_tx_egress_arp_device(const halo_egress_config_t* cfg, const uint8_t* d_bytes,
                                       const uint32_t* d_offsets_dw, const uint16_t* d_lens, uint32_t n,
                                       const halo_arp_result_t* d_results, uint8_t* d_out,
                                       halo_egress_port_t* d_ports, uint32_t* d_index, uint32_t* d_skipped,
                                       void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream);
/* After halo_switch_forward (a device switch) in stream order. */
HALO_API int halo_tx_egress_switch_device(const halo_egress_config_t* cfg, const uint8_t* d_bytes,
                                          const uint32_t* d_offsets_dw, const uint16_t* d_lens, uint32_t n,
                                          const halo_sw_result_t* d_results, uint64_t flood_mask, uint8_t* d_out,
                                          halo_egress_port_t* d_ports, uint32_t* d_index, uint32_t* d_skipped,
                                          void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream);
/* The same outputs from the sequential loop over host memory; no HIP. `kind` = HALO_EGRESS_KIND_*
 * says what `selectors` points to; flood_mask is read for the switch kind only. The caller picks
 * it by name for polls at the reference's cadence, as the switch's host mode is picked. `out`
 * needs no alignment and region_bytes may be any value here. */
HALO_API int halo_tx_egress_host(const halo_egress_config_t* cfg, uint32_t kind, const uint8_t* bytes,
                                 const uint32_t* offsets_dw, const uint16_t* lens, uint32_t n, const void* selectors,
                                 uint64_t flood_mask, uint8_t* out, halo_egress_port_t* ports, uint32_t* index,
                                 uint32_t* skipped);
/* Publish a span of whole records (host memory, as one port's stream) into a ring made by
 * halo_ring_create. Every header is validated first: a length of 0, a length above size / 2 or a
 * record running past span_bytes returns HALO_E_INVAL with nothing written. The longest prefix of
 * records that fits the ring's free space is taken (tail is re-read once when short, as WritePacket
 * does), copied in stream order — positions are taken modulo the size, so the ring bytes are those
 * WritePacket would leave, plus the zero alignment bytes — and head is published once with a release
 * store. *records_written / *bytes_written (optional) say what was taken. Host only. */
HALO_API int halo_ring_write_span(void* ring_memory, const uint8_t* span, uint64_t span_bytes,
                                  uint32_t* records_written, uint64_t* bytes_written);

/* ---- loopback: LoChan packet streams from a decided batch ------------------------------------
 * The producer side of a NetIf's LoChan. Ipv4RouteForward copies a packet whose destination is the
 * out NetIf's own address (in NetIf not NATing) into that NetIf's LoChan and returns before the
 * SNAT step (engine/ipv4_engine.go:193-201, ahead of :203-225); TxIpv4 does the same for a locally
 * built packet (:71-80). PacketHandle drains the channel through ParseIpv4Pkt, the own-address
 * filter and the local Rx{Icmp,Udp,Tcp} (engine/engine.go:353-381): HALO_RX_L3_START parsing,
 * halo_rx_dispatch_loopback, the responders and local delivery under HALO_RX_L3_START.
 *
 * Two calls:
 *   halo_arp_loopback_mark_device  the encap's LOOPBACK test alone, from records, ahead of the NAT
 *       lookup: its mark is the d_skip of halo_nat_lookup_lan_device (OR'd with the return-flow
 *       hits), so a LoChan packet keeps its source and no NatAddFlow runs for it.
 *   halo_lo_gather_device / _host  after the encap in stream order: a stable multi-way partition of
 *       the batch's LOOPBACK frames into one L3 batch per out NetIf, in ascending frame index — the
 *       order in which the in NetIf's goroutine sends to each channel.
 *
 * MARK: d_mark[i] is SET to 1 iff ip_proto != 0xFF, and the route id is inside the uploaded array
 *   or d_via[i] (optional) says HALO_PMFLOW_V_OVERRIDE, and the out NetIf (the route's, or the
 *   via's) is below n_netifs, and record.dst_ip == netif[out].ip, and netif[in_netif].nat_enable
 *   == 0; else to 0, for every i < n. No frame byte is touched. For a non-NAT in NetIf nothing
 *   rewrites bytes 30-33 before the encap, so the mark equals (verdict == LOOPBACK) for every frame
 *   the encap selects. Records 16-byte aligned, route ids 4, via 8. HALO_E_INVAL before the first
 *   sync and when the last sync had routes == NULL; HALO_E_RANGE: in_netif >= n_netifs. n == 0 is OK.
 *
 * GATHER, which frames: verdict == HALO_ARP_V_LOOPBACK and out_netif < n_netifs.
 *   forward mode (flags without HALO_LO_TX, after halo_arp_encap_device / _via_device): the packet
 *     is bytes [14, len) of the frame as they are now — the whole ethPayload, Ethernet padding
 *     included, TTL already decremented (:134 runs before :195). pkt_len = len - 14. SENDABLE:
 *     34 <= len <= 1514 (9014 with HALO_RX_JUMBO_EXT).
 *   tx mode (HALO_LO_TX, after halo_arp_encap_tx_device): the packet is exactly totalLen bytes from
 *     byte 14, totalLen = big-endian frame bytes 16-17 (:76-78). SENDABLE: 20 <= totalLen <= len - 14.
 *   A selected frame that is not sendable goes nowhere and is counted once in *d_skipped (optional,
 *   INCREMENTED).
 * LAYOUT: NetIf p's packets start at d_out + p * region_bytes; each packet starts on a 4-byte
 *   boundary and is followed by zeros up to the next one: size = (pkt_len + 3) & ~3.
 * PER-PACKET ARRAYS, index_cap entries per NetIf, for k < min(frames, index_cap):
 *   d_pkt_off_dw[p * index_cap + k]  the packet's dword offset from its NetIf's region start, or
 *                                    0xFFFFFFFF beyond the written prefix
 *   d_pkt_len[p * index_cap + k]     pkt_len
 *   d_index[p * index_cap + k]       the source frame index
 *   so that (d_out + p * region_bytes, d_pkt_off_dw + p * index_cap, d_pkt_len + p * index_cap) with
 *   n = min(frames_written, index_cap) is what a HALO_RX_L3_START parse takes, as it lies.
 * SUMMARIES: one halo_egress_port_t per NetIf, SET, with egress's meaning: frames / bytes are the
 *   totals, frames_written / bytes_written the prefix that fits.
 * REGION OVERFLOW (build-defined): the egress rule. NetIf p's packets are written while they fit
 *   wholly in region_bytes; the first that does not fit ends the NetIf's written prefix, and the
 *   totals are still reported so that the caller can resubmit the tail. (The reference's channel
 *   holds 1,024 packets and blocks the sender when full, engine/engine.go:209; blocking has no
 *   batch meaning.)
 * READS: nothing of a frame that is not selected and — forward mode — sendable (tx mode reads the
 *   dword with bytes 16-19 of a selected frame of at least 34 bytes to learn totalLen); nothing past
 *   the 4-byte word that holds the packet's last byte, and the bytes of that word beyond the packet
 *   do not reach the output. The batch is never written.
 * WRITES: exactly [p * region_bytes, p * region_bytes + bytes_written) of each NetIf, the n_netifs
 *   summaries, the array entries above, *d_skipped; nothing else.
 * The device call is asynchronous on `stream` with no host round trip: three launches (per-tile
 * counts, a scan over tiles, the scatter). n == 0 is OK and zeroes the summaries. Every argument is
 * checked before any device call. HALO_E_INVAL: a null cfg / d_ports, a null array with n > 0,
 * n_netifs outside 1..64, flags other than HALO_RX_JUMBO_EXT | HALO_LO_TX, region_bytes not a
 * multiple of 16 or above 2^34, d_out null with region_bytes > 0 or not 16-byte aligned, any of the
 * three per-packet arrays null with index_cap > 0, a misaligned array (offsets, pkt_off, index,
 * skipped: 4; lens, pkt_len: 2; results, summaries, workspace: 8), workspace_bytes <
 * halo_lo_gather_workspace(n, n_netifs). HALO_E_NODEV / _ARCH as elsewhere.
 * Not covered: Router.Ipv4PktFwdHook; a blocking channel; compact records in the mark; a loopback
 * step in the engine loop's NetIf. */
#define HALO_LO_TX 0x100u /* halo_lo_config_t.flags: tx mode, packets are totalLen bytes */
typedef struct halo_lo_config {
    uint32_t n_netifs;     /* 1..64                                                                  */
    uint32_t flags;        /* HALO_RX_JUMBO_EXT (forward mode's cap), HALO_LO_TX                     */
    uint64_t region_bytes; /* NetIf p's packets start at d_out + p * region_bytes; a multiple of 16
                              for the device call; at most 2^34                                      */
    uint32_t index_cap;    /* entries per NetIf in each of the three per-packet arrays               */
    uint32_t reserved;     /* 0                                                                      */
} halo_lo_config_t;        /* 24 B */
HALO_API int halo_arp_loopback_mark_device(const halo_arp_table_t* t, const halo_rx_result_t* d_records, uint32_t n,
                                           const uint32_t* d_route_ids, uint32_t in_netif,
                                           const halo_pmflow_via_t* d_via, uint8_t* d_mark, halo_stream_t stream);
/* Bytes of device workspace (8-byte aligned) a call over n frames and n_netifs NetIfs needs; 0 for
 * n_netifs outside 1..64. One workspace serves any number of calls issued on one stream. */
HALO_API uint64_t halo_lo_gather_workspace(uint32_t n, uint32_t n_netifs);
HALO_API int halo_lo_gather_device(const halo_lo_config_t* cfg, const uint8_t* d_bytes, const uint32_t* d_offsets_dw,
                                   const uint16_t* d_lens, uint32_t n, const halo_arp_result_t* d_results,
                                   uint8_t* d_out, halo_egress_port_t* d_ports, uint32_t* d_pkt_off_dw,
                                   uint16_t* d_pkt_len, uint32_t* d_index, uint32_t* d_skipped, void* d_workspace,
                                   uint64_t workspace_bytes, halo_stream_t stream);
/* The same outputs from the sequential loop over host memory; no HIP. The caller picks it by name
 * for polls at the reference's cadence. `out` needs no alignment and region_bytes may be any value
 * up to 2^34 here. */
HALO_API int halo_lo_gather_host(const halo_lo_config_t* cfg, const uint8_t* bytes, const uint32_t* offsets_dw,
                                 const uint16_t* lens, uint32_t n, const halo_arp_result_t* results, uint8_t* out,
                                 halo_egress_port_t* ports, uint32_t* pkt_off_dw, uint16_t* pkt_len, uint32_t* index,
                                 uint32_t* skipped);

/* ---- the tx ring producer: halo_ring_write_span from device memory ---------------------------
 * An egress stream (halo_tx_egress_*_device) is published into its tx ring where it lies in HBM:
 * the device finds the record boundaries, reads head and tail, copies the records that fit into the
 * mapped ring and publishes head. The host touches no frame byte and learns the outcome from a
 * 24-byte result. halo_ring_write_span stays the call for polls at the reference's cadence.
 *
 * ATTACH as the ring's producer. The header is validated as halo_rx_ring_attach and
 * halo_ring_write_span validate it (layout version, size and mask, head - tail <= size, 4-byte
 * cursors, `offset`), before any device call. With HALO_RING_REGISTER the ring is registered as an
 * rx ring is (page rules and HALO_E_INVAL answers of halo_rx_ring_attach; detach unregisters).
 * Without it the ring memory must already be mapped for the device in one piece (a live
 * registration of this library, e.g. the same ring attached by halo_rx_ring_attach with
 * HALO_RING_REGISTER, or pinned memory), else HALO_E_INVAL: one registration then carries a device
 * producer and a device consumer. HALO_RING_PERSISTENT and unknown flags: HALO_E_INVAL. HALO_E_HIP
 * from an attach with HALO_RING_REGISTER: the ring's pages may still be pinned, keep it allocated.
 *
 * WRITE a span: asynchronous on `stream`, no host round trip. d_span is device memory, 4-byte
 * aligned; span_bytes is a host value, a multiple of 4 (halo_egress_port_t.bytes_written). What
 * happens is what halo_ring_write_span does for the same ring state and span:
 *   1. every record header of the examined window is checked before a ring byte is written: a
 *      length of 0, a length above size / 2, or a record running past the span's end gives
 *      status = HALO_TXRING_BAD_SPAN (the host call's HALO_E_INVAL), nothing written, head unchanged;
 *   2. room = size - (head - tail), read on the device (tail: a system-scope acquire load); 0 when
 *      head - tail > size or tail & 3;
 *   3. the longest prefix of whole records with total size <= room is taken: status =
 *      HALO_TXRING_OK when that is the whole span, else HALO_TXRING_SHORT (possibly 0 records);
 *      `records` and `bytes` say what was taken, so the caller resubmits d_span + bytes;
 *   4. the prefix is copied to data[(head + k) & mask] — the ring bytes halo_ring_write_span leaves;
 *   5. head + bytes is published once, after every copied byte, by a system-scope release store,
 *      only when bytes > 0. tail and the rest of the header are never written;
 *   6. *d_result (optional; device or mapped host memory, 8-byte aligned) is written in stream order.
 * Nothing on the device waits: a full ring is answered with SHORT.
 *
 * BUILD-DEFINED DIFFERENCES from the host call:
 *   - only the first min(span_bytes, size) bytes are examined: no record beyond them is taken, a
 *     malformed record beyond them is not seen, and a record cut by that window is not an error;
 *   - a record longer than HALO_TXRING_MAX_RECORD (16,376) bytes is BAD_SPAN (the device record
 *     walk's capacity); the host accepts records up to size / 2;
 *   - span_bytes above what halo_rx_ring_scan_workspace accepts is HALO_E_INVAL
 *     (halo_tx_ring_workspace returns 0 for it);
 *   - span_bytes == 0 is OK and still writes the result: OK, 0, 0, head.
 *
 * ORDERING: one producer per ring. Calls on one stream chain without the host knowing head: each
 * reads it from the ring after the previous call's publish. Calls on two streams for one ring are
 * the caller's error. A host halo_ring_write_* on the same ring is legal once the stream is
 * synchronised. d_workspace (halo_tx_ring_workspace(span_bytes) bytes, 16-byte aligned) serves any
 * number of calls issued on one stream. The ring memory must stay mapped until detach returns.
 *
 * Argument checks come before a device is looked for. HALO_E_INVAL: a null handle; d_span null or
 * not 4-byte aligned with span_bytes > 0; span_bytes & 3; d_result not 8-byte aligned; d_workspace
 * null or not 16-byte aligned; workspace_bytes < halo_tx_ring_workspace(span_bytes) (which is never
 * 0 for a span it accepts). Then HALO_E_NODEV / _ARCH as elsewhere. */
#define HALO_TXRING_OK 0u       /* the whole span was taken                                     */
#define HALO_TXRING_SHORT 1u    /* a proper prefix (possibly nothing) was taken: the ring is full */
#define HALO_TXRING_BAD_SPAN 2u /* a malformed record in the examined window: nothing written   */
#define HALO_TXRING_MAX_RECORD 16376u
typedef struct halo_tx_ring_result {
    uint32_t status;  /* HALO_TXRING_*                       */
    uint32_t records; /* records taken                        */
    uint64_t bytes;   /* their bytes: a whole number of records */
    uint64_t head;    /* the ring's head after the call       */
} halo_tx_ring_result_t; /* 24 B */
typedef struct halo_tx_ring halo_tx_ring_t;
HALO_API int halo_tx_ring_attach(int device, void* ring_mem, int64_t offset, uint32_t attach_flags,
                                 halo_tx_ring_t** out);
/* Waits for the device's work on the ring and frees the handle. HALO_E_HIP: the ring memory could
 * not be unregistered (keep it allocated: its pages stay mapped for the device). */
HALO_API int halo_tx_ring_detach(halo_tx_ring_t* ring);
/* Bytes of device workspace a write of span_bytes needs; 0 for a span that is too large. Never
 * decreases with span_bytes. */
HALO_API uint64_t halo_tx_ring_workspace(uint64_t span_bytes);
HALO_API int halo_tx_ring_write_span_device(halo_tx_ring_t* ring, const uint8_t* d_span, uint64_t span_bytes,
                                            halo_tx_ring_result_t* d_result, void* d_workspace,
                                            uint64_t workspace_bytes, halo_stream_t stream);

/* ---- the reference engine's per-frame decision (engine/ethernet_engine.go:13-31,
 *      engine/ipv4_engine.go:18-47, engine/{udp,tcp,icmp}_engine.go) ------------------ */
typedef enum halo_rx_action {
    HALO_RX_ACT_DROP_ETH = 0,      /* ParseEthFrm error: logged and dropped              */
    HALO_RX_ACT_IGNORE_MAC = 1,    /* not for this NetIf (dst MAC filter)                */
    HALO_RX_ACT_ARP = 2,           /* -> HandleArp                                       */
    HALO_RX_ACT_IGNORE_TYPE = 3,   /* 802.3 / IPv6: silently ignored                     */
    HALO_RX_ACT_DROP_IP = 4,       /* ParseIpv4Pkt error (incl. build-defined totalLen)   */
    HALO_RX_ACT_BCAST_UDP = 5,     /* RxUdpBroadcast, UDP parse+verify OK (-> DHCP)      */
    HALO_RX_ACT_DROP_BCAST_UDP = 6,/* RxUdpBroadcast, UDP parse error                    */
    HALO_RX_ACT_IGNORE_BCAST = 7,  /* x.x.x.255 and not UDP                              */
    HALO_RX_ACT_FORWARD = 8,       /* Ipv4RouteForward (no L4 verification)              */
    HALO_RX_ACT_LOCAL_ICMP = 9,    /* RxIcmp OK                                          */
    HALO_RX_ACT_LOCAL_UDP = 10,    /* RxUdp OK -> UdpServiceMap                          */
    HALO_RX_ACT_LOCAL_TCP = 11,    /* RxTcp OK -> TcpServiceMap                          */
    HALO_RX_ACT_DROP_L4 = 12,      /* local L4 parse error: logged and dropped           */
    HALO_RX_ACT_LO_NOT_OWN = 13,   /* loopback drain: dst != NetIf.IpAddr, skipped       */
                                   /* (engine/engine.go:367-369)                         */
    HALO_RX_ACT_COUNT = 14
} halo_rx_action_t;

/* Host-side: maps n results to the action the reference engine takes (u8 per frame).
 * Pure host code over the kernel's records; no GPU needed. `action_hist` (optional)
 * receives HALO_RX_ACT_COUNT counters (incremented).                                    */
HALO_API int halo_rx_dispatch(const halo_rx_result_t* results, uint32_t n,
                              const halo_rx_netif_t* netif, uint8_t* actions,
                              uint32_t* action_hist);
/* The same over compact records. */
HALO_API int halo_rx_dispatch_compact(const halo_rx_record16_t* records, uint32_t n,
                                      const halo_rx_netif_t* netif, uint8_t* actions,
                                      uint32_t* action_hist);
/* PacketHandle's LoChan drain (engine/engine.go:353-381) over records parsed with
 * HALO_RX_L3_START: ParseIpv4Pkt error -> DROP_IP (:362-365); dst != NetIf.IpAddr ->
 * LO_NOT_OWN (:366-368); otherwise the local parse of ip_proto -> LOCAL_ICMP / LOCAL_UDP /
 * LOCAL_TCP, or DROP_L4 when it failed (:369-376). No broadcast or NAT branch: the drain
 * has none. */
HALO_API int halo_rx_dispatch_loopback(const halo_rx_result_t* results, uint32_t n,
                                       const halo_rx_netif_t* netif, uint8_t* actions,
                                       uint32_t* action_hist);

/* ---- local responders: echo, time-exceeded and TCP handshake replies -------------------------
 * The three answers the reference gives from inside its receive loop, for a parsed batch at once:
 * from the records (and offsets_dw / lens) to one dense list of halo_tx_build_desc_t in ascending
 * frame index — at most one reply per frame, and BuildIpv4Pkt's iphId++ runs in frame order — for
 * halo_tx_build_batch_device to consume with d_payload = the batch's own d_bytes. No payload is
 * copied and no frame byte is read. Per frame i, with a = halo_rx_dispatch's action of record i,
 * the first row that holds, in the reference's order:
 *   ECHO        a == LOCAL_ICMP and l4_aux == 8 (ICMP_REQUEST): RxIcmp answers TxIcmp(icmpPayload,
 *               ICMP_REPLY, icmpId, icmpSeq, src) (engine/icmp_engine.go:12-23). proto 1, aux 0,
 *               src_port = l4_seq >> 16 (the id), dst_port = l4_seq & 0xFFFF, payload = the
 *               record's payload_off / payload_len.
 *   ECHO        a == FORWARD, d_nat_verdict[i] == HALO_NAT_V_MISS, ip_proto == 1, status == OK,
 *               l4_aux == 8: Ipv4RouteForward returned false on a NATing NetIf and RxIpv4 hands an
 *               ICMP packet to RxIcmp (engine/ipv4_engine.go:31-36, :120-124). As above. Any other
 *               frame with verdict MISS gets nothing: the forward ended before its TTL step.
 *   TTL         a == FORWARD, ops[i].steps & HALO_TX_TTL and !(result[i] & HALO_TX_R_TTL_ALIVE):
 *               TxIcmp(ethPayload[:28], ICMP_TTL, {0,0}, 0, src) (engine/ipv4_engine.go:133-142).
 *               proto 1, aux 11, ports 0, payload = frame bytes [14, 14 + min(28, len - 14)) AS THE
 *               FIXUP LEFT THEM (post-DNAT, TTL as HandleIpv4PktTtl left it): build after the fixup
 *               in stream order.
 *   TCP_SYN     a == LOCAL_TCP, bit dport of d_tcp_ports set (TcpServiceMap), SYN && !ACK: TxTcp(nil,
 *               dport, sport, src, 1234567890, seq + 1, SYN|ACK) (engine/tcp_engine.go:16-21).
 *               proto 6, aux 0x12, src_port = dport, dst_port = sport, seq = 1234567890, ack =
 *               l4_seq + 1 (u32 wrap), payload length 0.
 *   TCP_SYNACK  the same with SYN && ACK: aux 0x10, seq = 1234567891, ack = l4_seq + 1 (:22-23).
 * Every kind: src_ip = netif->ip, dst_ip = the record's src_ip, payload_off = 4 * offsets_dw[i] +
 * the offset above, dst_mac zeros, mode HALO_TX_BUILD_ETH, pads zero. ip_id, the checksums and the
 * payload-length rejections stay halo_tx_build_batch_device's: an echo request above 1472 payload
 * bytes (HALO_RX_JUMBO_EXT) is emitted here and rejected there, as BuildIcmpPkt would.
 * d_nat_verdict (halo_nat_lookup_wan_device's), the pair d_ops / d_fixup_result
 * (halo_tx_fixup_batch_device's) and d_tcp_ports (65,536 bits as 2,048 u32, bit p & 31 of word
 * p >> 5) are each optional: an absent input means its rows never fire. Only one of d_ops and
 * d_fixup_result is HALO_E_INVAL. `flags`: HALO_RX_L3_START or 0. With HALO_RX_L3_START the
 * records are LoChan packets (engine/engine.go:353-381): the action is halo_rx_dispatch_loopback's,
 * only the LOCAL_* rows apply, and payload_off is in packet coordinates.
 * OUTPUTS: d_desc[k], d_src[k] = {frame index, kind} and d_dst_ip[k] (optional; what
 * halo_route_lookup_device takes) for the first min(count, cap) replies; *d_count is SET to the
 * total, also beyond `cap` (halo_arp_gather_device's convention); d_kind_counts (optional,
 * HALO_RESPOND_KIND_COUNT u32) is INCREMENTED by the totals per kind; d_actions (optional, n bytes)
 * = halo_rx_dispatch's (or _loopback's) action of every frame, a device-side dispatch. Nothing else
 * is written: entries at and beyond min(count, cap) stay as they were.
 * TxIpv4's L3 / L2 step for the built frames is halo_arp_encap_tx_device; the chain is respond ->
 * halo_tx_build_batch_device (payload = the rx batch) -> halo_route_lookup_device(d_dst_ip) ->
 * halo_arp_encap_tx_device -> halo_tx_egress_arp_device. A reply that then gets NO_ROUTE, MISS or
 * OWN_IP has still consumed its iphId (BuildIpv4Pkt runs before FindRoute): build every descriptor,
 * drop afterwards.
 * Not covered: Router.Ipv4PktFwdHook; UDP service replies (the
 * handlers' job). The LoChan copy of a LOOPBACK reply: halo_lo_gather_device with HALO_LO_TX.
 * The device call: three launches on `stream` (tile counts, scan, scatter), every argument checked
 * before a device is looked for. Alignment: d_records 16; d_desc, d_src 8; offsets, ops, ports map,
 * dst_ip, count, kind counts, workspace 4; lens 2. HALO_E_INVAL: null netif / d_count, a null
 * array with n > 0, d_desc or d_src null with cap > 0, other flags, a short workspace. n == 0 is OK
 * and sets *d_count = 0. */
#define HALO_RESPOND_ECHO 0u
#define HALO_RESPOND_TTL 1u
#define HALO_RESPOND_TCP_SYN 2u
#define HALO_RESPOND_TCP_SYNACK 3u
#define HALO_RESPOND_KIND_COUNT 4u
typedef struct halo_respond_src {
    uint32_t index; /* the answered frame's index in its batch */
    uint8_t kind;   /* HALO_RESPOND_*                          */
    uint8_t pad[3];
} halo_respond_src_t; /* 8 B */
/* Bytes of device workspace (4-byte aligned, no initialisation) for n frames. One workspace serves
 * any number of calls issued on one stream. */
HALO_API uint64_t halo_tx_respond_workspace(uint32_t n);
HALO_API int halo_tx_respond_device(const uint32_t* d_offsets_dw, const uint16_t* d_lens,
                                    const halo_rx_result_t* d_records, uint32_t n, uint32_t flags,
                                    const halo_rx_netif_t* netif, const uint8_t* d_nat_verdict,
                                    const halo_tx_op_t* d_ops, const uint8_t* d_fixup_result,
                                    const uint32_t* d_tcp_ports, halo_tx_build_desc_t* d_desc,
                                    halo_respond_src_t* d_src, uint32_t* d_dst_ip, uint32_t cap, uint32_t* d_count,
                                    uint32_t* d_kind_counts, uint8_t* d_actions, void* d_workspace,
                                    uint64_t workspace_bytes, halo_stream_t stream);
/* The same outputs from the sequential loop over host memory; no HIP. The caller picks it by name
 * for polls at the reference's cadence. Arrays need only their natural alignment. */
HALO_API int halo_tx_respond_host(const uint32_t* offsets_dw, const uint16_t* lens, const halo_rx_result_t* records,
                                  uint32_t n, uint32_t flags, const halo_rx_netif_t* netif, const uint8_t* nat_verdict,
                                  const halo_tx_op_t* ops, const uint8_t* fixup_result, const uint32_t* tcp_ports,
                                  halo_tx_build_desc_t* desc, halo_respond_src_t* src, uint32_t* dst_ip, uint32_t cap,
                                  uint32_t* count, uint32_t* kind_counts, uint8_t* actions);

/* ---- local delivery: service payload streams from a device-resident batch --------------------
 * RxIpv4's fourth outcome (engine/ipv4_engine.go:18-47): RxUdp / RxTcp hand a payload to the
 * handler registered for its destination port, and a broadcast UDP datagram to a DHCP port goes to
 * RxDhcp. For a parsed batch that lies in HBM: from the frames, their offsets_dw / lens and their
 * full records to ONE stream of delivery records in ascending frame index — the order in which the
 * reference calls the handlers, across all services — so that a host downloads the served payloads
 * and 24 bytes of header each, not the batch and its records. Per frame i, with a =
 * halo_rx_dispatch's action of record i:
 *   UDP   a == LOCAL_UDP and bit dport of d_udp_ports set (UdpServiceMap): handleFunc(UdpSession{
 *         src, sport}, udpPayload)                                  engine/udp_engine.go:10-21
 *   TCP   a == LOCAL_TCP and bit dport of d_tcp_ports set (TcpServiceMap): handleFunc(TcpSession{src,
 *         sport}, tcpPayload, seqNum, ackNum, flags) for EVERY such segment, handshake segments and
 *         empty payloads included (the handshake answers themselves are the responders')
 *                                                                   engine/tcp_engine.go:10-26
 *   DHCP  a == BCAST_UDP, dport == 67 or 68 (DhcpServerPort / DhcpClientPort) and HALO_DELIVER_DHCP
 *         in cfg->flags: RxDhcp(udpPayload, udpSrcPort, udpDstPort, ipv4SrcAddr). "DHCP" below
 *         decodes these records where they lie.                     engine/udp_engine.go:35-44
 * d_udp_ports / d_tcp_ports are 65,536 bits as 2,048 u32, bit p & 31 of word p >> 5, as
 * halo_tx_respond_device takes them; NULL = no service of that protocol. With HALO_RX_L3_START in
 * cfg->flags the records are LoChan packets (engine/engine.go:353-381): the action is
 * halo_rx_dispatch_loopback's, payload_off is in packet coordinates and the DHCP row cannot occur.
 * A selected frame whose record says payload_off + payload_len > lens[i] (a record that is not the
 * frame's) is delivered nowhere and counted in `skipped`: no record makes the call read outside
 * the frame it names.
 * A RECORD is halo_deliver_hdr_t (24 B, little-endian), the payload_len payload bytes (the record's
 * payload_off / payload_len slice of the frame: UDP pkt[8:], TCP pkt[headerLen:] with the
 * data-offset nibble taken as bytes, protocol/tcp.go:49,68, so a payload starts at any of the four
 * byte alignments), then zeros up to the next 4-byte boundary. Record size = 24 + ((payload_len +
 * 3) & ~3); every record starts 4-byte aligned.
 * REGION OVERFLOW (the egress rule): records are written while they fit wholly in region_bytes;
 *   the first that does not fit ends the written prefix. `records` and `bytes` remain the totals.
 * INDEX (optional): d_index[k] = {frame, offset} for k < min(records, index_cap); offset = the
 *   record's byte offset in d_out, or 0xFFFFFFFF beyond the written prefix (and, for the host call
 *   with a region above 4 GiB, for an offset that does not fit).
 * READS: no byte of a frame that is not delivered; nothing outside the 4-byte words that hold a
 *   delivered frame's bytes — only those that hold payload bytes are loaded, and the bytes of
 *   those words outside the payload (headers, a neighbour's, a gap's) never reach the output. A
 *   service-map word is read only for a LOCAL_UDP / LOCAL_TCP frame. The batch is never written.
 * WRITES: exactly [0, bytes_written) of d_out, the summary (SET) and the index entries above;
 *   nothing else.
 * The device call is asynchronous on `stream` with no host round trip: three launches (per-tile
 * counts, a scan over tiles that writes the summary, the scatter). n == 0 is OK and zeroes the
 * summary. Every argument is checked before any device call. HALO_E_INVAL: a null cfg /
 * netif / d_summary, a null array with n > 0, flags other than HALO_RX_L3_START |
 * HALO_DELIVER_DHCP, region_bytes not a multiple of 16 or above 2^32 - 16, d_out null with
 * region_bytes > 0, d_index null with index_cap > 0, a misaligned array (d_out, records: 16;
 * summary, index, workspace: 8; bytes, maps, offsets: 4; lens: 2), workspace_bytes <
 * halo_rx_deliver_workspace(n). HALO_E_NODEV / _ARCH as elsewhere.
 * Not covered: a stream per service (the order the reference shows is the batch's; local_port and
 * kind let a host split it). The DHCP engine: "DHCP" below. */
#define HALO_DELIVER_UDP 0u
#define HALO_DELIVER_TCP 1u
#define HALO_DELIVER_DHCP 2u /* the kind, and the bit of halo_deliver_config_t.flags that enables it */
#define HALO_DELIVER_KIND_COUNT 3u
typedef struct halo_deliver_hdr {
    uint32_t frame;       /* the frame's index in its batch         */
    uint8_t kind;         /* HALO_DELIVER_*                         */
    uint8_t tcp_flags;    /* l4_aux                                 */
    uint16_t payload_len; /* bytes that follow, before the padding  */
    uint32_t remote_ip;   /* src_ip                                 */
    uint16_t remote_port; /* sport                                  */
    uint16_t local_port;  /* dport                                  */
    uint32_t seq;         /* l4_seq                                 */
    uint32_t ack;         /* l4_ack                                 */
} halo_deliver_hdr_t;     /* 24 B */
typedef struct halo_deliver_config {
    uint32_t flags;        /* HALO_RX_L3_START | HALO_DELIVER_DHCP                                   */
    uint32_t index_cap;    /* entries in d_index (0 with d_index NULL)                               */
    uint64_t region_bytes; /* bytes of d_out; a multiple of 16 and at most 2^32 - 16 for the device call */
} halo_deliver_config_t;   /* 16 B */
typedef struct halo_deliver_summary { /* SET by the call */
    uint32_t records;         /* frames delivered, also beyond the region              */
    uint32_t records_written; /* the prefix of them that fits the region wholly        */
    uint64_t bytes;           /* sum of their record sizes                             */
    uint64_t bytes_written;   /* <= region_bytes; a whole number of records            */
    uint32_t kind_counts[HALO_DELIVER_KIND_COUNT]; /* of `records`, per kind            */
    uint32_t skipped;         /* selected, but the record's payload overruns the frame */
} halo_deliver_summary_t;     /* 40 B */
typedef struct halo_deliver_index {
    uint32_t frame;
    uint32_t offset; /* of the record in d_out; 0xFFFFFFFF: not written */
} halo_deliver_index_t; /* 8 B */
/* Bytes of device workspace (8-byte aligned, no initialisation) for n frames. One workspace serves
 * any number of calls issued on one stream. */
HALO_API uint64_t halo_rx_deliver_workspace(uint32_t n);
HALO_API int halo_rx_deliver_device(const halo_deliver_config_t* cfg, const uint8_t* d_bytes,
                                    const uint32_t* d_offsets_dw, const uint16_t* d_lens,
                                    const halo_rx_result_t* d_records, uint32_t n, const halo_rx_netif_t* netif,
                                    const uint32_t* d_udp_ports, const uint32_t* d_tcp_ports, uint8_t* d_out,
                                    halo_deliver_summary_t* d_summary, halo_deliver_index_t* d_index,
                                    void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream);
/* The same outputs from the sequential loop over host memory; no HIP. The caller picks it by name
 * for polls at the reference's cadence; it is never a fallback. Arrays need no alignment and
 * region_bytes may be any value here. */
HALO_API int halo_rx_deliver_host(const halo_deliver_config_t* cfg, const uint8_t* bytes, const uint32_t* offsets_dw,
                                  const uint16_t* lens, const halo_rx_result_t* records, uint32_t n,
                                  const halo_rx_netif_t* netif, const uint32_t* udp_ports, const uint32_t* tcp_ports,
                                  uint8_t* out, halo_deliver_summary_t* summary, halo_deliver_index_t* index);

/* ---- KCP ingest: segment walk and byte check over a delivery stream ---------------------------
 * The stateless part of the reference's KCP receive path, for the UDP payloads of one served port
 * in a delivery stream that lies in HBM: what Listener.packetInput (protocol/kcp/session.go:866-921)
 * and KCP.Input (kcp.go:613-709) do to a datagram's bytes before any session state is touched. A
 * host then runs Input's state machine from 32-byte segment descriptors whose checks are done, and
 * touches payload bytes only to hand them on.
 * INPUT: halo_rx_deliver_*'s stream, summary and index (index_cap entries). Considered: index
 *   entries k < min(summary.records, index_cap) with offset != 0xFFFFFFFF. SELECTED: those whose
 *   header says kind == HALO_DELIVER_UDP and local_port == cfg->port. The record count is read
 *   where the stream lies; the device call sizes its grids from index_cap.
 * cfg->byte_check_mode (kcp.go:34-41): -1 disabled, 0 zero, 1 CRC32 (IEEE, crc32.ChecksumIEEE), 2
 *   XXH3 (the low 32 bits of hashcode.GetHashCodeXXH3). The header size H is 28 when disabled,
 *   else 32 (a u32 hash field follows `length`).
 * A selected payload of L bytes (packetInput):
 *   L == 20   ParseEnet (enet.go:100-145): head (bytes 0..3) and tail (16..19) must both be those of
 *             SYN / EST / FIN / PING -> an ENET datagram record: conn_type, session_id, conv,
 *             enet_type (big-endian u32 at 4, 8, 12) and conv0 = rawConv, the little-endian u64 of
 *             bytes 4..11. No match: ignored.
 *   L >= H    a KCP datagram: conv0 = the little-endian u64 at byte 0 (the listener finds the
 *             session by it, so the session's kcp.conv == conv0), then Input's walk: while at least
 *             H bytes remain (a shorter tail is ignored, ret 0) read conv u64, cmd u8, frg u8, wnd
 *             u16, ts, sn, una, length u32 (and hash u32), advance H, and check in this order
 *               conv != conv0 -> ret -1;  length > bytes remaining -> -2;  cmd not in 81..84 -> -3;
 *               mode != -1 and cmd == 81 (PUSH) and hash != byte_check_hash(data[:length]) -> -4
 *             (zero mode: the field must be 0; a non-PUSH segment is never hashed). A failing check
 *             ends the datagram; else the segment is PROCESSED (inSegs++) and the walk advances
 *             `length` bytes. n_segs = processed segments, ret = what Input returns.
 *   else      ignored. Ignored payloads give no record and are counted.
 *   The one difference from Input: a client-side session that knows its own conv compares it with
 *   the record's conv0 itself (Input would return -1 at once; here the walk is relative to conv0).
 * OUTPUT, all little-endian, all SET (nothing is cleared beforehand):
 *   halo_kcp_dgram_t [dgram_cap]: one per selected, non-ignored datagram, in stream order.
 *   halo_kcp_seg_t [seg_cap]: one per WALKED segment — one that passed the conv, length and cmd
 *     checks, up to the first that fails one — datagrams contiguous and in order: datagram j owns
 *     [first_seg, first_seg + n_walked) and a consumer uses [first_seg, first_seg + n_segs). The
 *     entries from n_segs to n_walked (behind a failed byte check) exist so that the hash step runs
 *     over the plain segment list and needs no second compaction; their `check` is what their own
 *     hash comparison gave.
 *   halo_kcp_summary_t: dgrams / segs / ignored are totals over the whole delivery; every other
 *     counter describes the WRITTEN datagrams (their checks are the ones that ran).
 * CAPACITY (the egress rule): a datagram record and its segments are written while the datagram
 *   fits dgram_cap and all its walked segments fit seg_cap; the first datagram that does not fit
 *   ends the written prefix. Totals stay totals.
 * READS: nothing outside [0, bytes_written) of the stream rounded up to a 4-byte word, the delivery
 *   summary and the considered index entries; segment data only as aligned words that hold data
 *   bytes. The stream is never written. WRITES: exactly the written prefixes and the summary.
 * The device call is asynchronous on `stream` with no host round trip. Arguments are checked
 * before any device call. HALO_E_INVAL: a null cfg / summary / deliver_summary; byte_check_mode
 * outside -1..2; port above 65535; with index_cap > 0 a null stream or index; a null dgrams with
 * dgram_cap > 0 or segs with seg_cap > 0; for the device call a misaligned array (segs: 16;
 * dgrams, index, both summaries, workspace: 8; stream: 4) or workspace_bytes <
 * halo_kcp_ingest_workspace(index_cap, seg_cap). index_cap == 0, or an empty delivery, zeroes the
 * summary. A build without HIP answers HALO_E_NODEV.
 * Not covered: sessions, ARQ (parse_ack / parse_data / flush's decisions), the ENet handshake, FEC.
 * Transmit: "KCP emit" below. */
#define HALO_KCP_CHECK_DISABLED (-1)
#define HALO_KCP_CHECK_ZERO 0
#define HALO_KCP_CHECK_CRC32 1
#define HALO_KCP_CHECK_XXH3 2
#define HALO_KCP_DGRAM_KCP 0u
#define HALO_KCP_DGRAM_ENET 1u
#define HALO_KCP_ENET_SYN 0u /* conn_type, in ParseEnet's order */
#define HALO_KCP_ENET_EST 1u
#define HALO_KCP_ENET_FIN 2u
#define HALO_KCP_ENET_PING 3u
#define HALO_KCP_SEG_CHECK_NA 0u     /* not a PUSH segment, or byte check disabled */
#define HALO_KCP_SEG_CHECK_PASSED 1u
#define HALO_KCP_SEG_CHECK_FAILED 2u
typedef struct halo_kcp_config {
    int32_t byte_check_mode; /* HALO_KCP_CHECK_*                         */
    uint32_t port;           /* the served UDP port (local_port)         */
    uint32_t dgram_cap;      /* entries in dgrams                        */
    uint32_t seg_cap;        /* entries in segs                          */
} halo_kcp_config_t;         /* 16 B */
typedef struct halo_kcp_dgram {
    uint32_t index;       /* k: the datagram's entry in the delivery index                 */
    uint8_t kind;         /* HALO_KCP_DGRAM_*                                              */
    uint8_t conn_type;    /* ENET: HALO_KCP_ENET_*; KCP: 0                                 */
    int8_t ret;           /* KCP: Input's return value, 0 or -1..-4; ENET: 0               */
    uint8_t reserved;     /* 0                                                             */
    uint64_t conv0;       /* KCP: LE u64 at byte 0; ENET: rawConv                          */
    uint16_t n_segs;      /* processed segments (65,507 / 28 < 65,536)                     */
    uint16_t n_walked;    /* segments with a descriptor, >= n_segs                         */
    uint32_t first_seg;   /* of its descriptors in segs                                    */
    uint32_t payload_len; /* L                                                             */
    uint32_t session_id;  /* ENET fields (0 for KCP)                                       */
    uint32_t conv;
    uint32_t enet_type;
} halo_kcp_dgram_t;       /* 40 B */
typedef struct halo_kcp_seg {
    uint32_t dgram;    /* its datagram's position in dgrams                                */
    uint8_t cmd;       /* 81 PUSH, 82 ACK, 83 WASK, 84 WINS                                */
    uint8_t frg;
    uint16_t wnd;
    uint32_t ts, sn, una;
    uint32_t len;      /* data bytes                                                       */
    uint32_t data_off; /* byte offset of the data in the delivery stream                   */
    uint8_t check;     /* HALO_KCP_SEG_CHECK_*                                             */
    uint8_t reserved[3]; /* 0 */
} halo_kcp_seg_t;      /* 32 B */
typedef struct halo_kcp_summary { /* SET by the call */
    uint32_t dgrams;         /* selected, non-ignored datagrams, also beyond the capacities  */
    uint32_t dgrams_written;
    uint32_t segs;           /* their walked segments                                        */
    uint32_t segs_written;
    uint32_t ret_counts[5];  /* written KCP datagrams with ret == -i                         */
    uint32_t enet_counts[4]; /* written ENET datagrams per conn_type                         */
    uint32_t ignored;        /* selected payloads that are neither                           */
    uint64_t bytes_hashed;   /* CRC32 / XXH3: data bytes of the written PUSH descriptors     */
    uint64_t in_pkts;        /* DefaultSnmp.InPkts / InBytes / KCPInErrors / InSegs as       */
    uint64_t in_bytes;       /* kcpInput (session.go:722-726) and Input (kcp.go:710, only on */
    uint64_t in_errs;        /* ret == 0) add them for the written KCP datagrams             */
    uint64_t in_segs;
} halo_kcp_summary_t;        /* 96 B */
/* Bytes of device workspace (8-byte aligned, no initialisation). One workspace serves any number
 * of calls issued on one stream. */
HALO_API uint64_t halo_kcp_ingest_workspace(uint32_t index_cap, uint32_t seg_cap);
HALO_API int halo_kcp_ingest_device(const halo_kcp_config_t* cfg, const uint8_t* d_stream,
                                    const halo_deliver_summary_t* d_deliver_summary,
                                    const halo_deliver_index_t* d_index, uint32_t index_cap,
                                    halo_kcp_dgram_t* d_dgrams, halo_kcp_seg_t* d_segs, halo_kcp_summary_t* d_summary,
                                    void* d_workspace, uint64_t workspace_bytes, halo_stream_t stream);
/* The same outputs from the sequential loop over host memory; no HIP. Picked by name, never a
 * fallback. Arrays need no alignment. */
HALO_API int halo_kcp_ingest_host(const halo_kcp_config_t* cfg, const uint8_t* stream,
                                  const halo_deliver_summary_t* deliver_summary, const halo_deliver_index_t* index,
                                  uint32_t index_cap, halo_kcp_dgram_t* dgrams, halo_kcp_seg_t* segs,
                                  halo_kcp_summary_t* summary);

/* ---- KCP emit: pack, encode and byte-check a flush batch ---------------------------------------
 * The stateless tail of the reference's KCP transmit path, for payload that lies in HBM: what
 * KCP.flush (protocol/kcp/kcp.go:770-950) does to bytes once the session has decided what to send —
 * makeSpace / flushBuffer's greedy packing of segments into datagrams of at most mtu bytes,
 * segment.encode (kcp.go:134-155) with byte_check_hash(data) for every PUSH, the copy of the data —
 * and the listener's BuildEnet control packets (enet.go:75-97). The state machine (which segments,
 * ts / wnd / una / sn, RTO, cwnd, the ack list) stays with the host, which works from descriptors
 * only. The output is ready for halo_tx_build_batch_device with d_payload = d_stream.
 * INPUT
 *   halo_kcp_out_session_t [n_sessions], in the caller's order: one flush (KCP) or one control
 *     packet (ENET) each. Every entry's [first_seg, first_seg + n_segs) must lie in the segment list
 *     and start at or behind the previous ENTRY's end (entry s is held against entry s - 1 alone,
 *     whatever that one's status): ascending and disjoint, gaps allowed. An ENET entry has n_segs 0
 *     and any first_seg that keeps the order.
 *   halo_kcp_seg_t [n_segs]: the descriptor KCP ingest writes, so a relay hands ingest's output
 *     back. Used: cmd, frg, wnd, ts, sn, una, len, and data_off = the byte offset of the data in
 *     d_payload, at any alignment. dgram and check are ignored.
 *   d_payload [payload_bytes].
 *   cfg: byte_check_mode as in ingest (H = 28 when disabled, else 32), src_ip / src_port (the served
 *     port) for the descriptors, dgram_cap, stream_cap (bytes).
 * A KCP session (flush with reserved == 0: sess.headerSize is never set in the reference): size = 0;
 *   for each segment in order need = H + len; if size + need > mtu the datagram ends and size = 0;
 *   size += need; at the end a non-empty datagram is output. No segments, no datagram. The ack
 *   entries flush filters out are simply not in the list, and a makeSpace call that no encode
 *   follows changes nothing, so the packing is flush's. A segment (encode): conv u64, cmd, frg, wnd
 *   u16, ts, sn, una, len u32, and with H == 32 a u32 that is byte_check_hash(data) for cmd 81 in
 *   CRC32 / XXH3 mode and 0 otherwise; then len data bytes, for any cmd (cmd is not validated:
 *   encode does not).
 * An ENET entry: one 20-byte datagram, BuildEnet(conn_type, enet_type, session_id, enet_conv).
 * STATUS per entry, the first that applies:
 *   BAD_RANGE     first_seg + n_segs > n_segs; first_seg before the previous entry's end (so the
 *                 entry behind one whose range ends past the list is BAD_RANGE too); ENET with
 *                 conn_type > 3 or n_segs != 0; a kind that is neither
 *   BAD_MTU       KCP: mtu <= H or mtu > 1472 (BuildUdpPkt's limit)
 *   then per segment in order, the first that fails:
 *   BAD_RANGE     [data_off, data_off + len) not inside payload_bytes
 *   SEG_TOO_LONG  H + len > mtu (Go would index past kcp.buffer; Send never makes one)
 *   A non-OK entry emits nothing and does not end the written prefix.
 * OUTPUT, all little-endian, all SET (nothing is cleared beforehand)
 *   d_status [n_sessions], HALO_KCP_EMIT_*.
 *   d_stream [stream_cap]: the datagrams of the OK entries in order, each at a multiple of 4, pad
 *     bytes zero (also behind the last), so the stream is deterministic over [0, bytes_written).
 *   halo_kcp_out_dgram_t [dgram_cap] and halo_tx_build_desc_t [dgram_cap], one of each per
 *     datagram: payload_off / payload_len the datagram's, proto 17, src from cfg, dst from the
 *     entry, mode HALO_TX_BUILD_ETH, everything else zero (halo_arp_encap_tx_device fills the MAC).
 *   halo_kcp_emit_summary_t: sessions / dgrams / segs / bytes and status_counts are totals over the
 *     whole call (sessions counts the OK entries; bytes the stream bytes with padding); the other
 *     counters describe the written prefix.
 * CAPACITY (the egress rule): an OK entry's datagrams are written while all of them fit dgram_cap
 *   and stream_cap; the first OK entry that does not fit ends the written prefix. Totals stay
 *   totals. Ranges of OK entries can overlap only across a non-OK entry between them; they are then
 *   emitted as given, segs_written is held to n_segs as a third capacity, and the u32 totals are
 *   exact while they fit (disjoint ranges always do).
 * READS: the session and segment arrays; data only as aligned 4-byte words that hold data bytes of
 *   in-range segments. WRITES: exactly the written prefixes, all of d_status and the summary.
 * The device call is asynchronous on `stream` with no host round trip. Arguments are checked before
 * any device call. HALO_E_INVAL: a null cfg or summary; byte_check_mode outside -1..2; src_port
 * above 65535; n_sessions or n_segs above HALO_KCP_EMIT_MAX; a null sessions / status with
 * n_sessions > 0, segs with n_segs > 0, payload with payload_bytes > 0, dgrams / descs with
 * dgram_cap > 0, stream with stream_cap > 0; for the device call a misaligned array (segs, dgrams:
 * 16; sessions, descs, summary, workspace: 8; payload, stream: 4) or workspace_bytes <
 * halo_kcp_emit_workspace(n_sessions, n_segs). n_sessions == 0 zeroes the summary. A build without
 * HIP answers HALO_E_NODEV.
 * Not covered: SetDUP duplication, ReserveBytes, sessions, ARQ and the ENet state machine. */
#define HALO_KCP_EMIT_OK 0u
#define HALO_KCP_EMIT_SEG_TOO_LONG 1u
#define HALO_KCP_EMIT_BAD_MTU 2u
#define HALO_KCP_EMIT_BAD_RANGE 3u
#define HALO_KCP_EMIT_MAX (1u << 23) /* entries and segments per call: every total fits a u32 */
typedef struct halo_kcp_emit_config {
    int32_t byte_check_mode; /* HALO_KCP_CHECK_*                                       */
    uint32_t src_ip;         /* the descriptors' source                                */
    uint32_t src_port;       /* the served UDP port                                    */
    uint32_t dgram_cap;      /* entries in dgrams and descs                            */
    uint32_t stream_cap;     /* bytes in stream                                        */
    uint32_t reserved;       /* 0                                                      */
} halo_kcp_emit_config_t;    /* 24 B */
typedef struct halo_kcp_out_session {
    uint64_t conv;       /* KCP: kcp.conv                                              */
    uint32_t first_seg;  /* its range in the segment list                              */
    uint32_t n_segs;
    uint32_t dst_ip;     /* s.remote                                                   */
    uint16_t dst_port;
    uint16_t mtu;        /* KCP: kcp.mtu                                               */
    uint8_t kind;        /* HALO_KCP_DGRAM_KCP / _ENET                                 */
    uint8_t conn_type;   /* ENET: HALO_KCP_ENET_*                                      */
    uint16_t reserved;   /* 0                                                          */
    uint32_t session_id; /* ENET: BuildEnet's sessionId, conv and enetType             */
    uint32_t enet_conv;
    uint32_t enet_type;
} halo_kcp_out_session_t; /* 40 B */
typedef struct halo_kcp_out_dgram {
    uint32_t offset;    /* of the datagram in the stream, a multiple of 4              */
    uint16_t len;       /* its bytes                                                   */
    uint16_t n_segs;    /* segments in it (ENET: 0)                                    */
    uint32_t session;   /* the entry it belongs to                                     */
    uint32_t first_seg; /* its first segment's index in the segment list               */
} halo_kcp_out_dgram_t; /* 16 B */
typedef struct halo_kcp_emit_summary { /* SET by the call */
    uint32_t sessions;         /* OK entries, also beyond the capacities               */
    uint32_t sessions_written; /* those of the written prefix                          */
    uint32_t dgrams;
    uint32_t dgrams_written;
    uint32_t segs;             /* segments of the OK entries                           */
    uint32_t segs_written;
    uint32_t status_counts[4]; /* entries per HALO_KCP_EMIT_*                          */
    uint64_t bytes;            /* stream bytes, padding included                       */
    uint64_t bytes_written;
    uint64_t bytes_hashed;     /* CRC32 / XXH3: data bytes of the written PUSH segments */
    uint64_t out_segs;         /* DefaultSnmp.OutSegs (one per encode, kcp.go:153) and  */
    uint64_t out_pkts;         /* OutPkts / OutBytes as defaultTx adds them with dup == */
    uint64_t out_bytes;        /* 0 (udp_socket.go:60-82), for the written datagrams    */
} halo_kcp_emit_summary_t;     /* 88 B */
/* Bytes of device workspace (8-byte aligned, no initialisation). One workspace serves any number
 * of calls issued on one stream. */
HALO_API uint64_t halo_kcp_emit_workspace(uint32_t n_sessions, uint32_t n_segs);
HALO_API int halo_kcp_emit_device(const halo_kcp_emit_config_t* cfg, const halo_kcp_out_session_t* d_sessions,
                                  uint32_t n_sessions, const halo_kcp_seg_t* d_segs, uint32_t n_segs,
                                  const uint8_t* d_payload, uint64_t payload_bytes, uint8_t* d_stream,
                                  halo_kcp_out_dgram_t* d_dgrams, halo_tx_build_desc_t* d_descs, uint8_t* d_status,
                                  halo_kcp_emit_summary_t* d_summary, void* d_workspace, uint64_t workspace_bytes,
                                  halo_stream_t stream);
/* The same outputs from the sequential loop over host memory; no HIP. Picked by name, never a
 * fallback. Arrays need no alignment. */
HALO_API int halo_kcp_emit_host(const halo_kcp_emit_config_t* cfg, const halo_kcp_out_session_t* sessions,
                                uint32_t n_sessions, const halo_kcp_seg_t* segs, uint32_t n_segs, const uint8_t* payload,
                                uint64_t payload_bytes, uint8_t* stream, halo_kcp_out_dgram_t* dgrams,
                                halo_tx_build_desc_t* descs, uint8_t* status, halo_kcp_emit_summary_t* summary);

/* ---- DHCP: batched message decode, the lease table and the reply build -------------------------
 * engine/dhcp_engine.go, the reference's other in-tree service: RxDhcp (called from the receive
 * loop through RxUdpBroadcast), TxDhcp -> TxUdp -> TxIpv4's broadcast branch, ListDhcp and
 * DhcpLeaseClear. Three pieces: the stateless per-byte work runs where the bytes lie (DECODE over a
 * delivery stream, REPLY BUILD into the payloads and descriptors halo_tx_build_batch_device
 * takes), and a host control plane (the SERVER object: lease table and state machine) is the
 * authority; it works from 128-byte message descriptors and never touches a payload.
 *
 * DECODE. INPUT: halo_rx_deliver_*'s stream, summary and index, as "KCP ingest" takes them.
 *   Considered: index entries k < min(summary.records, index_cap) with offset != 0xFFFFFFFF (the
 *   record count is read where the stream lies). SELECTED: those whose header says kind ==
 *   HALO_DELIVER_DHCP. One halo_dhcp_msg_t per selected record, in stream order (RxDhcp's first
 *   lines, ParseDhcpPkt and ParseDhcpOption: dhcp_engine.go:216-230, :169-181, :70-122):
 *   direction  remote_port == 68 && local_port == 67: TO_SERVER; 67 -> 68: TO_CLIENT; any other
 *              pair: status PORTS (the reference does not parse it: only the header is read).
 *   payload_len < 240: SHORT. Bytes 236..239 not 63 82 53 63: COOKIE. Both leave every payload
 *              field of the record zero (ParseDhcpPkt returns nothing).
 *   xid = pkt[4:8] as raw bytes, yiaddr = IpAddrToU(pkt[16:20]), chaddr = pkt[28:34].
 *   options    ParseDhcpOption's loop over o = payload[240:], n = len(o), i = 0: stop when o[i] ==
 *              0xff; stop when i + 1 >= n (one byte remains); code = o[i], length = o[i + 1]; stop
 *              when i + 2 + length > n; keep codes 1, 3, 6, 12, 50, 53 (of a repeated code the last
 *              wins: the map entry is overwritten); i += 2 + length. Code 0 is an ordinary TLV.
 *   REF_PANIC  where the Go code would panic (HALO_ROUTE_PANIC is the precedent): the loop top
 *              reaches i == n (an empty option area, or an option that ends exactly at the end
 *              with no 0xff before it), or a code 53 has length 0 (data[0]), wherever it stands.
 *              Every option field of such a record is zero.
 *   fields     msg_type = option 53's data[0]; req_ip = IpAddrToU(option 50's data): 0 when its
 *              length is not 4; mask / gateway = the first min(length, 4) bytes of options 1 / 3
 *              and that count (what copy(i.NetworkMask, ..) / copy(i.Gateway, ..) take); dns =
 *              option 6's first four bytes; hostname = option 12 in mem.StaticString64 form:
 *              min(length, 63) bytes, zeros, the count in byte 63.
 *              BUILD-DEFINED: option 6 with length < 4 — `data[0:4]` reslices into the capacity
 *              of the caller's buffer, which this stage cannot know — counts as ABSENT, with
 *              HALO_DHCP_OPT_DNS_SHORT set; both bits describe the LAST option 6.
 *   A missing option 53 is no status: HALO_DHCP_OPT_MSG_TYPE is clear and the handler returns
 *   silently, as RxDhcp does.
 * CAPACITY (the egress rule): messages are written while they fit msg_cap; `msgs` stays the total.
 *   status_counts / type_counts describe the WRITTEN messages (type_counts[t]: OK messages with
 *   option 53 and msg_type t <= 8; type_counts[0] also counts every other OK message).
 * READS: nothing outside the 4-byte words that hold a selected record's header and payload bytes,
 *   the delivery summary and the considered index entries; of a PORTS record only the header. The
 *   stream is never written. WRITES: the written prefix and the summary (SET; nothing is cleared
 *   beforehand), nothing else.
 * The device call is asynchronous on `stream` with no host round trip: three launches (per-tile
 * counts from the headers' kind alone, the scan over tiles that writes the summary, the write with
 * the walk). Arguments are checked before any device call. HALO_E_INVAL: a null summary /
 * deliver_summary; with index_cap > 0 a null stream or index; a null msgs with msg_cap > 0; for
 * the device call a misaligned array (msgs: 16; index, both summaries, workspace: 8; stream: 4), a
 * null workspace with index_cap > 0 or workspace_bytes < halo_dhcp_decode_workspace(index_cap).
 * index_cap == 0, or an empty delivery, zeroes the summary. A build without HIP answers
 * HALO_E_NODEV. */
#define HALO_DHCP_OK 0u
#define HALO_DHCP_PORTS 1u     /* neither 68 -> 67 nor 67 -> 68                         */
#define HALO_DHCP_SHORT 2u     /* "dhcp packet len < 240 bytes"                         */
#define HALO_DHCP_COOKIE 3u    /* "dhcp magic cookie error"                             */
#define HALO_DHCP_REF_PANIC 4u /* the reference would panic in ParseDhcpOption          */
#define HALO_DHCP_STATUS_COUNT 5u
#define HALO_DHCP_TO_SERVER 0u
#define HALO_DHCP_TO_CLIENT 1u
#define HALO_DHCP_DIR_NONE 2u  /* with status PORTS */
#define HALO_DHCP_OPT_MASK 0x01u      /* option 1 present  */
#define HALO_DHCP_OPT_ROUTER 0x02u    /* option 3          */
#define HALO_DHCP_OPT_DNS 0x04u       /* option 6, length >= 4 */
#define HALO_DHCP_OPT_HOSTNAME 0x08u  /* option 12         */
#define HALO_DHCP_OPT_REQ_IP 0x10u    /* option 50         */
#define HALO_DHCP_OPT_MSG_TYPE 0x20u  /* option 53         */
#define HALO_DHCP_OPT_DNS_SHORT 0x40u /* the last option 6 had length < 4: build-defined absent */
#define HALO_DHCP_DISCOVER 1u /* DhcpOptionMsgType*: msg_type, and halo_dhcp_reply_t.kind */
#define HALO_DHCP_OFFER 2u
#define HALO_DHCP_REQUEST 3u
#define HALO_DHCP_ACK 5u
#define HALO_DHCP_NAK 6u
#define HALO_DHCP_RELEASE 7u
#define HALO_DHCP_TYPE_COUNT 9u
typedef struct halo_dhcp_msg {
    uint32_t index;       /* k: the message's entry in the delivery index                    */
    uint8_t status;       /* HALO_DHCP_OK .. _REF_PANIC                                      */
    uint8_t dir;          /* HALO_DHCP_TO_SERVER / _TO_CLIENT / _DIR_NONE                    */
    uint8_t msg_type;     /* option 53's data[0]                                             */
    uint8_t reserved0;    /* 0                                                               */
    uint32_t options;     /* HALO_DHCP_OPT_*                                                 */
    uint8_t xid[4];       /* pkt[4:8]                                                        */
    uint32_t yiaddr;      /* IpAddrToU(pkt[16:20])                                           */
    uint8_t chaddr[6];    /* pkt[28:34]                                                      */
    uint16_t payload_len; /* the delivery header's                                           */
    uint32_t remote_ip;   /* the delivery header's: RxDhcp's ipv4SrcAddr                     */
    uint32_t req_ip;      /* IpAddrToU(option 50's data)                                     */
    uint8_t mask[4];      /* option 1: the first mask_n bytes, zeros behind them             */
    uint8_t gateway[4];   /* option 3: the first gateway_n bytes                             */
    uint8_t dns[4];       /* option 6's data[0:4]                                            */
    uint8_t mask_n;       /* min(option 1's length, 4)                                       */
    uint8_t gateway_n;    /* min(option 3's length, 4)                                       */
    uint8_t reserved1[2]; /* 0 */
    uint32_t reserved2[3]; /* 0 */
    uint8_t hostname[64]; /* option 12 as mem.StaticString64                                 */
} halo_dhcp_msg_t;        /* 128 B */
typedef struct halo_dhcp_summary { /* SET by the call */
    uint32_t msgs;         /* selected records, also beyond msg_cap */
    uint32_t msgs_written;
    uint32_t status_counts[HALO_DHCP_STATUS_COUNT]; /* of the written messages */
    uint32_t type_counts[HALO_DHCP_TYPE_COUNT];
} halo_dhcp_summary_t;     /* 64 B */
/* Bytes of device workspace (8-byte aligned, no initialisation). One workspace serves any number
 * of calls issued on one stream. */
HALO_API uint64_t halo_dhcp_decode_workspace(uint32_t index_cap);
HALO_API int halo_dhcp_decode_device(const uint8_t* d_stream, const halo_deliver_summary_t* d_deliver_summary,
                                     const halo_deliver_index_t* d_index, uint32_t index_cap, halo_dhcp_msg_t* d_msgs,
                                     uint32_t msg_cap, halo_dhcp_summary_t* d_summary, void* d_workspace,
                                     uint64_t workspace_bytes, halo_stream_t stream);
/* The same outputs from the sequential loop over host memory; no HIP. Picked by name, never a
 * fallback. Arrays need no alignment. */
HALO_API int halo_dhcp_decode_host(const uint8_t* stream, const halo_deliver_summary_t* deliver_summary,
                                   const halo_deliver_index_t* index, uint32_t index_cap, halo_dhcp_msg_t* msgs,
                                   uint32_t msg_cap, halo_dhcp_summary_t* summary);

/* THE SERVER OBJECT: one per NetIf, as DhcpLeaseTable is; host memory, no HIP, not thread safe (the
 * reference's DhcpLock is the caller's). It restates dhcp_engine.go:216-434 call for call:
 *   a message whose status is not OK, whose direction's side is disabled or that has no option 53
 *   does nothing. TO_SERVER (server_enable):
 *   DISCOVER  reuses req_ip only when a lease for it exists with the same MAC; otherwise the first
 *             networkU + ii (u32 arithmetic), ii < 2^hostBits, hostBits = 32 - popcount(networkU) —
 *             the popcount of the network ADDRESS, as written; nothing is scanned when hostBits ==
 *             32 — whose last octet is neither 0 nor 255, that is not the own address and not
 *             leased. It records no lease. No address: no reply. Else one OFFER.
 *   REQUEST   no option 50: nothing. req_ip == 0, another subnet, leased to another MAC, or a new
 *             lease with the table at `capacity` (MallocType returning nil): NAK, in this order.
 *             Otherwise the lease is written (ExpTime = (uint32_t)(now + 3600), the hostname by
 *             StaticString64.Set: a renewed lease keeps the bytes behind a shorter name) and the
 *             replies are ACK FOLLOWED BY NAK: the dhcp_nak label sits directly behind the ACK's
 *             TxDhcp, so the reference falls through. A REQUEST that reaches HostName.Set with an
 *             empty hostname (option 12 absent or of length 0) is REF_PANIC: Set("") indexes
 *             element 0 of an empty slice (mem/static_allocator.go:219); no state change, no reply.
 *   RELEASE   deletes the lease keyed by remote_ip, whatever the MAC.
 *   TO_CLIENT (client_enable, own ip 0, xid equal to the client's transaction id):
 *   OFFER     one REQUEST reply (option 50 = yiaddr, option 54 = remote_ip).
 *   ACK       one halo_dhcp_client_event_t. The caller applies it (the NetIf's address, the two
 *             AddRoute calls, the DNS copy to the serving NetIfs, SendFreeArp) and, as the
 *             reference's own address is set from then on, ignores what follows it.
 * halo_dhcp_handle_msgs handles msgs[0..n) in order. verdicts[i] (optional) = a HALO_DHCP_H_*
 * code | flag bits. reply_cap must be at least 2 * n, and event_cap at least n unless events is
 * NULL with event_cap 0 (events are then counted, not stored): else HALO_E_INVAL, before any
 * state changes. halo_dhcp_list copies up to cap leases in ascending address order (ListDhcp; the
 * reference's order is its table's) and returns the count. halo_dhcp_clear is one DhcpLeaseClear tick:
 * leases with now > ExpTime, in plain u32, are deleted; returns how many. halo_dhcp_discover is
 * DhcpDiscover with the caller's random xid: it sets the client's transaction id and gives the
 * DISCOVER message. */
#define HALO_DHCP_H_NONE 0u          /* nothing to do (status, side disabled, no / other msg type, xid) */
#define HALO_DHCP_H_OFFER 1u
#define HALO_DHCP_H_NO_ADDR 2u       /* "dhcp server no ip found"                                     */
#define HALO_DHCP_H_NO_REQ_IP 3u     /* REQUEST without option 50                                     */
#define HALO_DHCP_H_NAK_ZERO 4u
#define HALO_DHCP_H_NAK_SUBNET 5u
#define HALO_DHCP_H_NAK_OTHER_MAC 6u
#define HALO_DHCP_H_NAK_FULL 7u
#define HALO_DHCP_H_ACK_NAK 8u       /* the lease is written; ACK, then NAK                           */
#define HALO_DHCP_H_REF_PANIC 9u     /* HostName.Set("")                                              */
#define HALO_DHCP_H_RELEASED 10u
#define HALO_DHCP_H_RELEASE_ABSENT 11u
#define HALO_DHCP_H_CLIENT_REQUEST 12u
#define HALO_DHCP_H_CLIENT_ACK 13u
#define HALO_DHCP_H_MASK 0x0Fu
#define HALO_DHCP_H_F_REUSED 0x40u   /* DISCOVER: the requested lease is offered again; REQUEST: a renewal */
#define HALO_DHCP_H_F_REPLY 0x80u    /* at least one reply was written                                */
typedef struct halo_dhcp_config {
    uint32_t ip;           /* IpAddrToU(NetIf.IpAddr); 0 for a client that has none yet   */
    uint32_t network_mask; /* IpAddrToU(NetIf.NetworkMask)                               */
    uint32_t dns;          /* IpAddrToU(NetIf.DnsServerAddr)                             */
    uint8_t mac[6];        /* NetIf.MacAddr                                              */
    uint8_t server_enable; /* Config.DhcpServerEnable                                    */
    uint8_t client_enable; /* Config.DhcpClientEnable                                    */
    uint32_t capacity;     /* the most leases: the stand-in for MallocType returning nil */
} halo_dhcp_config_t;      /* 24 B */
typedef struct halo_dhcp_lease {
    uint32_t ip;          /* IpAddrToU(DhcpLease.IpAddr) */
    uint8_t mac[6];
    uint16_t reserved;    /* 0 */
    uint32_t exp_time;
    uint8_t hostname[64]; /* mem.StaticString64 */
} halo_dhcp_lease_t;      /* 80 B */
typedef struct halo_dhcp_reply {
    uint8_t kind;        /* HALO_DHCP_OFFER / _ACK / _NAK / _REQUEST / _DISCOVER */
    uint8_t reserved0[3];
    uint8_t xid[4];
    uint32_t yiaddr;     /* IpAddrToU form; 0 for NAK / REQUEST / DISCOVER */
    uint8_t chaddr[6];
    uint16_t reserved1;
    uint32_t req_ip;     /* REQUEST: option 50 */
    uint32_t server_id;  /* REQUEST: option 54 */
    uint32_t reserved2;
} halo_dhcp_reply_t;     /* 32 B */
typedef struct halo_dhcp_client_event {
    uint32_t msg;       /* the ACK's position in msgs */
    uint32_t ip;        /* yiaddr */
    uint8_t mask[4], gateway[4], dns[4];
    uint8_t mask_n, gateway_n;
    uint8_t options;    /* HALO_DHCP_OPT_MASK | _ROUTER | _DNS: which were present */
    uint8_t reserved;
} halo_dhcp_client_event_t; /* 24 B */
typedef struct halo_dhcp_server halo_dhcp_server_t;
HALO_API int halo_dhcp_server_create(const halo_dhcp_config_t* cfg, halo_dhcp_server_t** out);
HALO_API void halo_dhcp_server_destroy(halo_dhcp_server_t* s);
HALO_API int halo_dhcp_handle_msgs(halo_dhcp_server_t* s, const halo_dhcp_msg_t* msgs, uint32_t n, uint64_t now,
                                   halo_dhcp_reply_t* replies, uint32_t reply_cap, uint8_t* verdicts, uint32_t* n_replies,
                                   halo_dhcp_client_event_t* events, uint32_t event_cap, uint32_t* n_events);
HALO_API uint32_t halo_dhcp_list(const halo_dhcp_server_t* s, halo_dhcp_lease_t* out, uint32_t cap);
HALO_API uint32_t halo_dhcp_clear(halo_dhcp_server_t* s, uint64_t now);
HALO_API int halo_dhcp_set_dns(halo_dhcp_server_t* s, uint32_t dns);
HALO_API int halo_dhcp_set_client_xid(halo_dhcp_server_t* s, const uint8_t xid[4]);
HALO_API int halo_dhcp_discover(halo_dhcp_server_t* s, const uint8_t xid[4], halo_dhcp_reply_t* reply);
HALO_API int halo_dhcp_server_config(const halo_dhcp_server_t* s, halo_dhcp_config_t* out);

/* REPLY BUILD: from n reply descriptors and the server's addresses (cfg: ip, network_mask, dns) to
 * the UDP payloads BuildDhcpPkt makes and one halo_tx_build_desc_t per reply, ready for
 * halo_tx_build_batch_device. Reply i lies at i * HALO_DHCP_SLOT_BYTES of the payload buffer, the
 * slot's tail zero. Lengths: 286 OFFER / ACK, 250 NAK, 270 REQUEST, 258 DISCOVER. The descriptor:
 * payload_off = i * 288, payload_len, proto 17, ports 67 -> 68 (OFFER / ACK / NAK) or 68 -> 67,
 * src_ip = cfg->ip, dst_ip 255.255.255.255, dst_mac ff:ff:ff:ff:ff:ff, HALO_TX_BUILD_ETH, the rest
 * zero: TxIpv4's dst[3] == 255 branch, so no ARP step follows. A reply of any other kind gives a
 * zero slot and an all-zero descriptor (proto 0: halo_tx_build answers HALO_TX_B_PROTO).
 * OPTION ORDER: BuildDhcpOption ranges over a Go map, so the reference's order is random per
 * packet. This build fixes it to the order of the map literals in the source — 53, 1, 3, 6, 51,
 * 59, 58, 54 for OFFER / ACK (lease 3600, rebinding 3150, renewal 1800); 53, 54 for NAK; 53, 61, 50,
 * 54, 55 for REQUEST; 53, 61, 55 for DISCOVER; then 0xff — an order the reference can produce, not
 * the only one.
 * One launch, asynchronous on `stream`; fixed slots, so no scan and one writer per dword. WRITES:
 * [0, n * 288) of d_payload and descs[0..n). HALO_E_INVAL: a null cfg; with n > 0 a null array; n
 * above 2^23; for the device call a misaligned array (d_replies: 16; d_descs: 8; d_payload: 4). */
#define HALO_DHCP_SLOT_BYTES 288u
#define HALO_DHCP_BUILD_MAX (1u << 23)
HALO_API int halo_dhcp_reply_build_device(const halo_dhcp_config_t* cfg, const halo_dhcp_reply_t* d_replies, uint32_t n,
                                          uint8_t* d_payload, halo_tx_build_desc_t* d_descs, halo_stream_t stream);
HALO_API int halo_dhcp_reply_build_host(const halo_dhcp_config_t* cfg, const halo_dhcp_reply_t* replies, uint32_t n,
                                        uint8_t* payload, halo_tx_build_desc_t* descs);

/* ---- synthetic traffic (bench + tests; SURVEY.md §8d generator) ----------------------
 * Every field of frame i is a pure function of (seed, i), so any shard of the global
 * stream [first_index, first_index + n) is generated independently.
 * halo_synth_layout (host): per-frame length, kind byte and ragged 4-byte-aligned dword
 * offsets (frames packed back to back, each rounded up to 4 bytes).
 *   size_mode : 0 = uniform `len`, 1 = IMIX 64/570/1500 at 7:4:1
 *   proto_mode: 0 = UDP, 1 = TCP, 2 = ICMP, 3 = mix UDP 50 / TCP 40 / ICMP 10
 *   mutate_shift: frame mutated with probability 2^-mutate_shift (0 = never)
 *   kinds[i]  : bits 0-1 protocol (0 UDP, 1 TCP, 2 ICMP), bit 7 = mutated
 *   *total_bytes = bytes the ragged layout spans.
 * halo_synth_frames_device: writes the frame bytes for a layout into d_bytes (ragged
 * dword offsets, or i*stride when d_offsets_dw == NULL). A mutated frame has one bit
 * flipped in [14, len) after its checksums were filled.                                 */
HALO_API int halo_synth_layout(uint64_t seed, uint64_t first_index, uint32_t n,
                               uint32_t size_mode, uint32_t len, uint32_t proto_mode,
                               uint32_t mutate_shift, uint16_t* lens, uint32_t* offsets_dw,
                               uint8_t* kinds, uint64_t* total_bytes);
HALO_API int halo_synth_frames_device(uint64_t seed, uint64_t first_index, uint32_t n,
                                      const uint16_t* d_lens, const uint32_t* d_offsets_dw,
                                      uint64_t stride, const uint8_t* d_kinds,
                                      const halo_rx_netif_t* netif, uint8_t* d_bytes,
                                      halo_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HALO_RX_H */
