"""Not a test: the corpus of hostile time-exceeded messages for IcmpTtlDeepNat (deep_nat.hip).

A quote inside a checksum-valid ICMP time-exceeded message is data a remote host chose. `corpus()`
builds about 4,000 such frames with oracle/ref_py.py's builders: every frame (bar the control rows)
has a valid outer IPv4 header checksum and a valid outer ICMP checksum, so it passes every check
of IcmpTtlDeepNat and reaches NatChangeSrc / NatChangeDst, and crosses

  the quote     random bytes; byte 9 from PROTOS, byte 0 from {0x45, 0x4F, 0x40, random}, the inner
                total length from {0, 19, 20, 21, qlen, qlen + 1, 0xFFFF, random}, fragment bits
                random; qlen every value 28..41 (both sides of the TCP guard 38), the values that
                put the frame length L within 4 of 256, 512, 768, 1024 and 1280 (the 64-dword
                staging steps of the wave) and at 1510..1514, random lengths in between
  padding       0..9 garbage bytes behind the outer total length: NatChangeDst sums the untrimmed
                payload, so such a frame leaves with an ICMP checksum that does not verify over
                its total length; that is the reference's behaviour
  zero sums     for each of the five recomputed checksums (inner IPv4, inner UDP / TCP / ICMP,
                outer IPv4, outer ICMP) rows whose recomputed value is 0x0000 under CheckSumEnable:
                one free 16-bit word (a header or payload half-word, or lan_port) is set to the
                value the C oracle stores with that word at zero, which is the complement of the
                rest of the sum. Go stores 0 there, also for UDP (no 0xFFFF substitution)
  control rows  frames that must stop at a named check: L in {0, 13, 14, 33, 34, 41, 61} and
                {1515, 1522, 9014, 65535}, a bad outer ICMP checksum, a bad outer IPv4 checksum,
                ICMP type 3 and 8, a quote of 27 bytes; and valid messages with `found` 0, 1, 255.

`pack()` lays frames out at 4-byte boundaries, 0..3 dwords apart, 64 bytes behind the last; every
gap and tail byte is random and non-zero, so a store that is too wide, or too early, shows in a
whole-buffer compare. `expected()` applies the C oracle frame by frame to a copy of such a buffer;
`first_difference()` names the first frame a GPU result differs in. tests/test_deepnat_cases.py
proves on the CPU what the corpus reaches."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle import ref_py as R

NAT_DTYPE = np.dtype([("lan_ip", "<u4"), ("lan_port", "<u2"), ("found", "u1"), ("pad", "u1")])  # halo_tx_deep_nat_t
PROTOS = (1, 6, 17, 47, 0, 255)  # byte 9 of the quote; the last three take the "addresses only" arm
EDGES = (256, 512, 768, 1024, 1280)  # frame lengths at which the wave's staging loop takes another step
MAX_FRAME = 1514
HEAD = 42  # Ethernet 14 + outer IPv4 20 + ICMP 8: the quote starts here
# frame offset of each recomputed checksum field (the inner L4 field depends on the quoted protocol)
ZERO_AT = {"inner_ip": HEAD + 10, "inner_udp": HEAD + 26, "inner_tcp": HEAD + 36, "inner_icmp": HEAD + 22,
           "outer_ip": 14 + 10, "outer_icmp": 14 + 22}
ST = {name: k for k, name in enumerate(R.STATUS)}
SEED = 0xD33B


def _bytes(rng, n: int) -> bytes:
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def ttl_frame(rng, quote: bytes, pad: bytes = b"", *, typ=11, ident=None, seq=None, icmp_bad=False, ip_bad=False) -> bytes:
    """Ethernet / IPv4 / ICMP `typ` around `quote`, checksums valid (unless broken on request), `pad`
    behind the IPv4 total length. The message's bytes 4..7 (unused in a time-exceeded message) and
    the addresses are random; `ident` (outer IPv4) and `seq` (message bytes 6..7) can be given."""
    seq = int(rng.integers(0, 1 << 16)) if seq is None else seq
    ident = int(rng.integers(0, 1 << 16)) if ident is None else ident
    msg = bytearray(R.build_icmp(quote, typ, _bytes(rng, 2), seq))
    if icmp_bad:
        msg[2] ^= 0x01
    ip = bytearray(R.build_ipv4(bytes(msg), 1, _bytes(rng, 4), _bytes(rng, 4), ident=ident,
                                ttl=int(rng.integers(1, 256)), frag=bytes([int(rng.choice([0, 0x40])), 0])))
    if ip_bad:
        ip[10] ^= 0x80
    return R.build_eth(bytes(ip) + pad, _bytes(rng, 6), _bytes(rng, 6), 0x0800, pad=False)


def hostile_quote(rng, qlen: int, proto: int) -> bytearray:
    """qlen random bytes with the fields IcmpTtlDeepNat and the ReCalc* functions look at drawn
    from their edge values."""
    q = bytearray(_bytes(rng, qlen))
    q[9] = proto
    q[0] = (0x45, 0x4F, 0x40, int(rng.integers(0, 256)))[int(rng.integers(0, 4))]
    tl = (0, 19, 20, 21, qlen, qlen + 1, 0xFFFF, int(rng.integers(0, 1 << 16)))[int(rng.integers(0, 8))]
    q[2:4] = tl.to_bytes(2, "big")
    return q


def _plan(rng):
    """(qlen, pad length, quote protocol) of the hostile rows."""
    rows = []
    for qlen in range(28, 42):
        for proto in PROTOS:
            for rep in range(6):
                rows.append((qlen, int(rng.integers(1, 10)) if rep & 1 else 0, proto))
    for edge in EDGES:
        for L in range(edge - 4, edge + 5):
            for k, proto in enumerate(PROTOS):
                pad = int(rng.integers(1, 10)) if (L + k) & 1 else 0
                rows.append((L - HEAD - pad, pad, proto))
    for L in range(MAX_FRAME - 4, MAX_FRAME + 1):
        for proto in PROTOS:
            for rep in range(3):
                pad = int(rng.integers(1, 10)) if rep else 0
                rows.append((L - HEAD - pad, pad, proto))
    for k in range(2600):
        pad = int(rng.integers(1, 10)) if rng.integers(0, 2) else 0
        L = int(rng.integers(HEAD + 28 + pad, MAX_FRAME + 1))
        rows.append((L - HEAD - pad, pad, PROTOS[k % len(PROTOS)]))
    return rows


def _zero_rows(rng, oracle):
    """(label, frame, lan_ip, lan_port) of the zero-sum rows. make(x) builds the row with its free
    word at x; the oracle's stored value with x = 0 is the complement of the rest of the sum, and
    with the free word at that value the sum is 0xFFFF and the stored value 0x0000."""
    out = []

    def solve(name, make):
        at = ZERO_AT[name]
        frame, ip, port = make(0)
        got, ok = oracle.icmp_deep_nat(frame, ip, port, True, 1)
        assert ok, name
        frame, ip, port = make(int.from_bytes(got[at:at + 2], "big"))
        got, ok = oracle.icmp_deep_nat(frame, ip, port, True, 1)
        assert ok and got[at:at + 2] == b"\0\0", (name, got[at:at + 2].hex())
        out.append((name, frame, ip, port))

    def fixed(qlen, proto, pad_len):
        """Everything of a row but its free word: quote, padding, NAT answer, and a generator whose
        state make() restarts from, so that both of its calls draw the same addresses."""
        return (hostile_quote(rng, qlen, proto), _bytes(rng, pad_len), int(rng.integers(0, 1 << 32)),
                int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 62)))

    for name_of, proto in (("inner_icmp", 1), ("inner_tcp", 6), ("inner_udp", 17)):
        for rep in range(4):
            qlen = int(rng.integers(44, 300)) | (rep & 1)  # odd and even quote lengths
            q, pad, ip, port, sub = fixed(qlen, proto, (0, 0, 3, 6)[rep])

            def make_port(x, q=q, pad=pad, ip=ip, sub=sub):  # free word: lan_port
                return ttl_frame(np.random.default_rng(sub), bytes(q), pad), ip, x

            def make_word(x, q=q, pad=pad, ip=ip, port=port, sub=sub):  # free word: quote bytes 40..41
                q2 = bytearray(q)
                q2[40:42] = x.to_bytes(2, "big")
                return ttl_frame(np.random.default_rng(sub), bytes(q2), pad), ip, port

            solve(name_of, make_port if rep < 2 else make_word)

            def make_ident(x, q=q, pad=pad, ip=ip, port=port, sub=sub):  # free word: the quoted identification
                q2 = bytearray(q)
                q2[4:6] = x.to_bytes(2, "big")
                return ttl_frame(np.random.default_rng(sub), bytes(q2), pad), ip, port

            def make_outer_ident(x, q=q, pad=pad, ip=ip, port=port, sub=sub):  # free word: outer identification
                return ttl_frame(np.random.default_rng(sub), bytes(q), pad, ident=x), ip, port

            def make_seq(x, q=q, pad=pad, ip=ip, port=port, sub=sub):  # free word: message bytes 6..7
                return ttl_frame(np.random.default_rng(sub), bytes(q), pad, seq=x), ip, port

            if rep >= 2:
                continue
            solve("inner_ip", make_ident)
            solve("outer_ip", make_outer_ident)
            solve("outer_icmp", make_seq)
    # the outer ICMP sum takes the padding in: two rows with odd and even padding per protocol
    for proto in (1, 6, 17):
        for pad_len in (5, 8):
            q, pad, ip, port, sub = fixed(int(rng.integers(44, 300)), proto, pad_len)
            solve("outer_icmp", lambda x, q=q, pad=pad, ip=ip, port=port, sub=sub:
                  (ttl_frame(np.random.default_rng(sub), bytes(q), pad, seq=x), ip, port))
    return out


def _control_rows(rng):
    """(label, frame, found, status without CheckSumEnable, status with it)."""
    rows = []
    whole = ttl_frame(rng, bytes(hostile_quote(rng, 64, 17)))
    for L, st in ((0, "ETH_LEN"), (13, "ETH_LEN"), (14, "IP_LEN"), (33, "IP_LEN")):
        rows.append((f"L{L}", whole[:L], 1, st, st))
    src, dst = _bytes(rng, 4), _bytes(rng, 4)
    for L in (34, 41):  # a valid IPv4 header in front of 0 and 7 ICMP bytes
        f = R.build_eth(R.build_ipv4(_bytes(rng, L - 34), 1, src, dst), _bytes(rng, 6), _bytes(rng, 6), 0x0800, pad=False)
        rows.append((f"L{L}", f, 1, "L4_LEN", "L4_LEN"))
    rows.append(("L61", ttl_frame(rng, _bytes(rng, 19)), 1, "L4_LEN", "L4_LEN"))
    rows.append(("quote27", ttl_frame(rng, bytes(hostile_quote(rng, 27, 17))), 1, "L4_LEN", "L4_LEN"))
    for L in (1515, 1522, 9014, 65535):
        rows.append((f"L{L}", ttl_frame(rng, bytes(hostile_quote(rng, L - HEAD, 6))), 1, "IP_LEN", "IP_LEN"))
    q = bytes(hostile_quote(rng, 120, 6))
    rows.append(("bad_icmp_cksum", ttl_frame(rng, q, icmp_bad=True), 1, "L4_CKSUM", "L4_CKSUM"))
    rows.append(("bad_ip_cksum", ttl_frame(rng, q, ip_bad=True), 1, "OK", "IP_HDR_CKSUM"))
    rows.append(("type3", ttl_frame(rng, q, typ=3), 1, "ICMP_TYPE", "ICMP_TYPE"))
    rows.append(("type8", ttl_frame(rng, q, typ=8), 1, "ICMP_TYPE", "ICMP_TYPE"))
    for found in (0, 1, 255):
        for proto in (17, 6):
            rows.append((f"found{found}", ttl_frame(rng, bytes(hostile_quote(rng, 90 + proto, proto)), _bytes(rng, 2)),
                         found, "OK", "OK"))
    return rows


@functools.lru_cache(maxsize=None)
def corpus(seed: int = SEED):
    """The corpus, read-only and shared: `frames` (a tuple of bytes), `nat` (one NAT_DTYPE row per
    frame) and per-frame labels: `kind` ("hostile", "zero:<checksum>", "control:<name>"), `proto`
    (byte 9 of the quote), `qlen`, `pad` (bytes behind the total length), `inner_tl` (the quoted
    total length), `zero_at` (frame offset of the field a zero-sum row aims at, else -1) and
    `status` ([n, 2]: the quote record's status without / with CheckSumEnable)."""
    from oracle import oracle

    rng = np.random.default_rng(seed)
    frames, kinds, found, ips, ports, status, zero_at = [], [], [], [], [], [], []

    def add(kind, frame, ip, port, fnd, st=("OK", "OK"), at=-1):
        frames.append(bytes(frame))
        kinds.append(kind)
        ips.append(ip)
        ports.append(port)
        found.append(fnd)
        status.append((ST[st[0]], ST[st[1]]))
        zero_at.append(at)

    for qlen, pad, proto in _plan(rng):
        f = ttl_frame(rng, bytes(hostile_quote(rng, qlen, proto)), _bytes(rng, pad))
        fnd = (0, 255)[int(rng.integers(0, 2))] if rng.integers(0, 12) == 0 else 1
        add("hostile", f, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 16)), fnd)
    for name, f, ip, port in _zero_rows(rng, oracle):
        add("zero:" + name, f, ip, port, 1, at=ZERO_AT[name])
    for name, f, fnd, st0, st1 in _control_rows(rng):
        add("control:" + name, f, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 16)), fnd, (st0, st1))
    # the rows in a seeded random order: every block of four waves mixes lengths and outcomes
    order = rng.permutation(len(frames))
    frames = tuple(frames[k] for k in order)
    n = len(frames)
    nat = np.zeros(n, NAT_DTYPE)
    nat["lan_ip"], nat["lan_port"], nat["found"] = np.array(ips, np.uint32)[order], np.array(ports)[order], np.array(found)[order]
    lens = np.array([len(f) for f in frames], np.int64)
    quoted = lens >= HEAD + 28
    tl = np.array([int.from_bytes(f[16:18], "big") if len(f) >= 18 else 0 for f in frames], np.int64)
    c = SimpleNamespace(
        frames=frames, nat=nat, lens=lens, kind=np.array(kinds, object)[order],
        proto=np.array([f[HEAD + 9] if ok else -1 for f, ok in zip(frames, quoted)], np.int64),
        qlen=np.where(quoted, tl - 28, -1), pad=np.where(quoted, lens - 14 - tl, 0),
        inner_tl=np.array([int.from_bytes(f[HEAD + 2:HEAD + 4], "big") if ok else -1 for f, ok in zip(frames, quoted)], np.int64),
        zero_at=np.array(zero_at, np.int64)[order], status=np.array(status, np.int64)[order])
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def pack(frames, rng):
    """(data, offsets_dw, lens): the frames in their order at 4-byte aligned starts, 0..3 dwords
    apart, 64 bytes behind the last; every byte outside a frame is random and non-zero."""
    L = np.array([len(f) for f in frames], np.int64)
    cell = ((L + 3) & ~3) + 4 * rng.integers(0, 4, len(L))
    offs = np.concatenate([[0], np.cumsum(cell)[:-1]])
    data = rng.integers(1, 256, int(offs[-1] + cell[-1]) + 64, dtype=np.uint8)
    for o, f in zip(offs.tolist(), frames):
        data[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return data, (offs // 4).astype(np.uint32), L.astype(np.uint16)


def expected(oracle, data, offsets_dw, lens, nat, en: int, n=None):
    """The C oracle on a copy of the buffer, for the first n frames (default: all): (buffer, quote
    records, applied flags). nat None: quote records only, the buffer unchanged."""
    n = len(lens) if n is None else n
    want = data.copy()
    quote = np.zeros(n, oracle.RESULT_DTYPE)
    applied = np.zeros(n, np.uint8)
    for k in range(n):
        o, L = int(offsets_dw[k]) * 4, int(lens[k])
        f = data[o:o + L].tobytes()
        quote[k] = oracle.icmp_quote(f, en)
        if nat is not None:
            out, ok = oracle.icmp_deep_nat(f, int(nat["lan_ip"][k]), int(nat["lan_port"][k]), bool(nat["found"][k]), en)
            want[o:o + L] = np.frombuffer(out, np.uint8)
            applied[k] = ok
    return want, quote, applied


def describe(c, i: int, en: int) -> str:
    return (f"frame {i}: {c.kind[i]}, L {int(c.lens[i])}, quote protocol {int(c.proto[i])}, qlen {int(c.qlen[i])}, "
            f"padding {int(c.pad[i])}, quoted total length {int(c.inner_tl[i])}, found {int(c.nat['found'][i])}, "
            f"lan_port {int(c.nat['lan_port'][i]):#06x}, status {R.STATUS[int(c.status[i, en])]}, CheckSumEnable {en}")


def first_difference(c, idx, en: int, got, want, offsets_dw, lens, what: str = "") -> None:
    """Bit-exact compare of a whole buffer; a difference names the first frame it shows in (`idx`
    maps a position in the buffer to its row of the corpus `c`; None: the same order) and whether
    it lies inside the frame or in the gap behind it."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    at = int(bad[0])
    byte_off = offsets_dw.astype(np.int64) * 4
    # (a zero-length frame shares its offset with its neighbour: take the last frame at or before)
    k = int(np.searchsorted(byte_off, at, side="right")) - 1
    rel = at - int(byte_off[k])
    where = f"frame offset {rel}" if rel < int(lens[k]) else f"{rel - int(lens[k])} bytes behind the frame (gap or tail)"
    hit = np.unique(np.searchsorted(byte_off, bad, side="right") - 1)
    row = k if idx is None else int(idx[k])
    raise AssertionError(f"{what}: {bad.size} buffer bytes differ in {hit.size} frames (first {hit[:8].tolist()}); first at "
                         f"buffer byte {at}, {where}: got {got[at:at + 8].tobytes().hex()} want "
                         f"{want[at:at + 8].tobytes().hex()}; position {k}, {describe(c, row, en)}")
