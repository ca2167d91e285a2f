"""TEST INFRASTRUCTURE: the IP layer restated at byte level, and its fixtures.

Handler is ip_dataHandler::add_mscDatagroup / process_ipVector / process_udpVector
(ip-datahandler.cpp:40-127, show_crcErrors on) over data groups laid out as dabgpu_pipe_packet
delivers them, with the layer's records: one result per group, the 100-datagram window, the
payloads in an output arena at multiples of 16.  It is pinned to the reference's own code by
tests/golden/ip_kat.npz (tests/golden/make_ip_golden.py).

Six rules where the reference is undefined or unbounded (include/dabgpu.h, dabgpu_ip_groups):
  1. bytes past a group's stored end read 0; a datagram over the CRC bytes of a group with the CRC
     flag reads them complemented (check_CRC_bits has inverted them in place);
  2. ipLength == 0 is NOT_V4;
  3. header bytes past ipLength read 0; a negative payload length is MALFORMED, after the window
     and checksum steps; length 0 is delivered;
  4. lengths are int32, quality is stored as int16;
  5. a record that points outside its arena is NOT_ACCEPTED;
  6. a payload that ends beyond the output arena is MALFORMED and still takes its place in the
     count of offsets.
"""
import numpy as np

import packet_py as pp
from mot_py import pack  # noqa: F401  (group byte strings -> records and arena, as dabgpu_pipe_packet lays them out)

STATE_DTYPE = np.dtype([("handled", "<i4"), ("crc_errors", "<i4")])
RESULT_DTYPE = np.dtype([("offset", "<i4"), ("nbytes", "<i4"), ("status", "<i2"), ("quality", "<i2"), ("ip_bytes", "<i4")])
RUN_DTYPE = np.dtype([("n_datagrams", "<i4"), ("n_bytes", "<i4"), ("counts", "<i4", (7,)), ("reserved", "<i4", (3,))])
DELIVERED, NOT_ACCEPTED, TOO_LONG, NOT_V4, CHECKSUM, NOT_UDP, MALFORMED = range(7)


def arena_bytes(group_slots: int, arena: int) -> int:
    """DABGPU_IP_ARENA_FOR"""
    return arena + 16 * group_slots


def _i16(v: int) -> int:
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


class Handler:
    """one ip_dataHandler (show_crcErrors on)"""

    def __init__(self, handled: int = 0, crc_errors: int = 0):
        self.handled, self.crc_errors = handled, crc_errors
        self.qualities = []                    # every show_ipErrors value
        self.datagrams = []                    # every writeDatagram payload

    def group(self, rec, arena) -> tuple:
        """one group -> (status, quality, ip_bytes, payload or None)"""
        off, nb, nxt, fl = int(rec["offset"]), int(rec["nbytes"]), int(rec["data_offset"]), int(rec["flags"])
        if not fl & pp.ACCEPTED or off < 0 or nb <= 0 or nxt < 0 or off + nb > len(arena):      # (:54), rule 5
            return NOT_ACCEPTED, -1, 0, None
        crc0 = nb - 2 if fl & pp.CRCF else nb

        def B(i):                              # rule 1
            return 0 if i < 0 or i >= nb else int(arena[off + i]) ^ (0xFF if i >= crc0 else 0)
        ip_len = B(nxt + 2) << 8 | B(nxt + 3)                                                  # (:79)
        if not ip_len < nb:                                                                    # (:80)
            return TOO_LONG, -1, ip_len, None
        D = lambda i: B(nxt + i) if i < ip_len else 0                                          # rule 3
        if ip_len == 0 or D(0) >> 4 != 4:      # rule 2; (:85) on a signed char only 0x40..0x4F give 4
            return NOT_V4, -1, ip_len, None
        hs = D(0) & 15
        quality = -1
        self.handled += 1                                                                      # (:100-104)
        if self.handled >= 100:
            quality = _i16(100 - self.crc_errors)
            self.qualities.append(quality)
            self.crc_errors = self.handled = 0
        s = sum(D(2 * i) << 8 | D(2 * i + 1) for i in range(2 * hs))
        s = (s >> 16) + (s & 0xFFFF)           # one fold (:107)
        if ~s & 0xFFFF:
            self.crc_errors += 1
            return CHECKSUM, quality, ip_len, None
        if D(9) != 17:
            return NOT_UDP, quality, ip_len, None
        n = ip_len - 4 * hs - 8
        if n < 0:
            return MALFORMED, quality, ip_len, None
        return DELIVERED, quality, ip_len, bytes(D(4 * hs + 8 + i) for i in range(n))

    def feed(self, records, arena, out_arena=None):
        """a run's groups -> (results RESULT_DTYPE, out bytes, run RUN_DTYPE record)"""
        out_arena = arena_bytes(len(records), len(arena)) if out_arena is None else out_arena
        res = np.zeros(len(records), RESULT_DTYPE)
        out = np.zeros(out_arena, np.uint8)
        run = np.zeros((), RUN_DTYPE)
        fill = 0
        for g, rec in enumerate(records):
            st, q, ipb, pay = self.group(rec, arena)
            off = n = 0
            if st == DELIVERED:
                off, n = fill, len(pay)
                fill += (n + 15) & ~15
                if off + n > out_arena:        # rule 6
                    st, off, n = MALFORMED, 0, 0
                else:
                    out[off:off + n] = np.frombuffer(pay, np.uint8)
                    self.datagrams.append(pay)
                    run["n_datagrams"] += 1
                    run["n_bytes"] += n
            res[g] = (off, n, st, q, ipb)
            run["counts"][st] += 1
        return res, out, run

    def state(self):
        return np.array((self.handled, self.crc_errors), STATE_DTYPE)


# ---- writers ------------------------------------------------------------------------------
def _csum_ok(h: bytes, hs: int) -> bool:
    """the reference's test (:105-108) on a header of 4 * hs bytes"""
    s = sum(h[2 * i] << 8 | h[2 * i + 1] for i in range(2 * hs))
    s = (s >> 16) + (s & 0xFFFF)
    return ~s & 0xFFFF == 0


def datagram(data=b"", hs=5, proto=17, version=4, bad=False, length=None, nibble=None, options=0xA5, ident=0x1234, cut=None):
    """an IPv4 datagram with a UDP header and data.  hs: the header's 32-bit words (its bytes past
    20 are options); nibble: the header-size nibble when it is not hs; length: the total-length field
    when it is not the true length; bad: a corrupted checksum; cut: keep only the first cut bytes (the
    checksum is made over what is left, the rest reading 0)"""
    n = max(hs, 5) * 4
    total = n + 8 + len(data)
    h = bytearray(n)
    h[0] = version << 4 | (hs if nibble is None else nibble)
    fld = total if length is None else length
    h[2:4] = bytes([fld >> 8, fld & 255])
    h[4:6] = bytes([ident >> 8, ident & 255])
    h[8], h[9] = 64, proto
    h[12:20] = bytes([10, 0, 0, 1, 239, 1, 2, 3])
    for i in range(20, n):
        h[i] = (options + 7 * i) & 255
    udp = bytes([0x22, 0xB8, 0x22, 0xB8, (8 + len(data)) >> 8, (8 + len(data)) & 255, 0, 0])
    whole = bytearray(bytes(h) + udp + bytes(data))
    if cut is not None:
        whole = whole[:cut]
    words = h[0] & 15
    view = bytes(whole[:4 * words]) + bytes(max(0, 4 * words - len(whole)))
    s = sum(view[2 * i] << 8 | view[2 * i + 1] for i in range(2 * words))
    while s >> 16:
        s = (s >> 16) + (s & 0xFFFF)
    c = ~s & 0xFFFF
    if len(whole) >= 12:
        whole[10:12] = bytes([c >> 8, c & 255])
        view = bytes(whole[:4 * words]) + bytes(max(0, 4 * words - len(whole)))
        assert words == 0 or _csum_ok(view, words), "a header the single fold refuses"
    if bad:
        whole[11] ^= 0x5A
    return bytes(whole)


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def second_fold_datagram(data=b"abcd"):
    """a 60-byte header whose words sum, after the one fold the reference does, to 0x10000 and more"""
    d = bytearray(datagram(data, hs=15))
    d[10:12] = b"\xFF\xFF"
    for i in range(20, 60):
        d[i] = 0xFF
    for ident in range(65536):
        d[4:6] = bytes([ident >> 8, ident & 255])
        s = sum(d[2 * i] << 8 | d[2 * i + 1] for i in range(30))
        if (s >> 16) + (s & 0xFFFF) >= 0x10000:
            return bytes(d)
    raise AssertionError("no such header")


def window_groups(rng):
    """230 datagrams that reach process_ipVector, 7 of them with a bad checksum at the 11th, 51st,
    99th, 100th, 101st, 151st and 202nd: the 100th's own error counts in the second window, so
    show_ipErrors gives 97 and 97 and the handler is left with 30 handled and 1 error.  Groups that
    do not get that far (a bad group CRC, version 6) lie in between."""
    bad = {10, 50, 98, 99, 100, 150, 201}
    groups = []
    for k in range(230):
        if k % 37 == 5:
            groups.append(pp.group(datagram(_bytes(rng, 6)), crcf=1, good=False))
        if k % 41 == 7:
            groups.append(pp.group(datagram(_bytes(rng, 6), version=6)))
        groups.append(pp.group(datagram(_bytes(rng, 4 + k % 9), bad=k in bad), crcf=k & 1))
    return groups


def fixtures():
    """the group sequences of tests/golden/ip_kat.npz: every read the reference makes on them is
    defined (next + ipLength <= the group's bytes, ipLength >= 10 and >= 4 * headerSize)"""
    rng = np.random.default_rng(59)
    fx = []

    def add(name, groups):
        fx.append(dict(name=name, groups=[bytes(g) for g in groups]))

    # good datagrams: with and without the group CRC, every optional header part
    add("plain", [pp.group(datagram(_bytes(rng, 40))), pp.group(datagram(_bytes(rng, 33)), crcf=1),
                  pp.group(datagram(_bytes(rng, 1)), ext=1), pp.group(datagram(_bytes(rng, 17)), seg=1, last=1, segno=3),
                  pp.group(datagram(_bytes(rng, 100)), ua=1, tidf=1, li=2), pp.group(datagram(_bytes(rng, 64)), ua=1, tidf=0, li=0),
                  pp.group(datagram(_bytes(rng, 31)), ua=1, tidf=0, li=5),
                  pp.group(datagram(_bytes(rng, 700)), ext=1, crcf=1, seg=1, ua=1, tidf=1, li=15, segno=9)])
    # a bad group CRC between two good groups
    add("group_crc", [pp.group(datagram(_bytes(rng, 20)), crcf=1), pp.group(datagram(_bytes(rng, 20)), crcf=1, good=False),
                      pp.group(datagram(_bytes(rng, 21)), crcf=1)])
    # ipLength against the group's bytes: nbytes - 2 is the longest the reference reads inside the group
    # (next >= 2, so ipLength == nbytes - 1 runs past it: rule_cases' "overhang"), nbytes is refused; trailing
    # bytes behind a shorter datagram are ignored
    d = datagram(_bytes(rng, 12))
    add("lengths", [pp.group(d), pp.group(datagram(_bytes(rng, 12), length=len(d) + 2)), pp.group(d + _bytes(rng, 9)),
                    pp.group(datagram(_bytes(rng, 12), length=len(d) + 1000))])
    # version 6, version nibble 0xC (a signed shift gives -4), version 0, version 5
    add("versions", [pp.group(datagram(_bytes(rng, 10), version=v)) for v in (6, 0xC, 4, 0, 5, 4)])
    # headerSize 0 (sums to 0: fails), 5, 6..8 and 15 (options)
    add("header_sizes", [pp.group(datagram(_bytes(rng, 30), nibble=0))] +
        [pp.group(datagram(_bytes(rng, 30), hs=h), crcf=h & 1) for h in (5, 6, 7, 8, 15)])
    # a sum the one fold leaves at 0x10000 and more, and corrupted checksums
    add("checksums", [pp.group(second_fold_datagram()), pp.group(datagram(_bytes(rng, 8), bad=True)),
                      pp.group(datagram(_bytes(rng, 8))), pp.group(datagram(_bytes(rng, 8), hs=7, bad=True), crcf=1)])
    # protocol 6 (and 1), payload length 0
    add("protocols", [pp.group(datagram(_bytes(rng, 24), proto=6)), pp.group(datagram(b"")), pp.group(datagram(_bytes(rng, 5), proto=1)),
                      pp.group(datagram(b"", hs=6), crcf=1)])
    # rule 1, the CRC overlap: the length field claims the group's two CRC bytes, which the reference
    # reads after check_CRC_bits has inverted them
    add("crc_overlap", [pp.group(datagram(_bytes(rng, 26), length=20 + 8 + 26 + 2), crcf=1),
                        pp.group(datagram(_bytes(rng, 3), length=20 + 8 + 3 + 1), crcf=1, ua=1, li=3)])
    add("window", window_groups(rng))
    return fx


def rule_cases():
    """cases that are not handed to the reference: its reads on them are undefined"""
    rng = np.random.default_rng(5900)
    out = []

    def add(name, groups):
        out.append(dict(name=name, groups=[bytes(g) for g in groups]))

    # header fields past the group's end: the group ends before, or inside, the length field
    add("short", [b"\x03\x00", b"\x03\x00\x45", b"\x03\x00\x45\x00\x01", pp.group(b"\x45\x00\x00\x03", crcf=1),
                  pp.group(b"", ext=1, seg=1, ua=1, li=15)])
    # next + ipLength > nbytes: ipLength == nbytes - 1 (next is at least 2), with and without the CRC flag
    d = datagram(_bytes(rng, 12))
    add("overhang", [pp.group(datagram(_bytes(rng, 12), length=len(d) + 1)),
                     pp.group(datagram(_bytes(rng, 12), length=len(d) + 3), crcf=1),
                     pp.group(datagram(_bytes(rng, 30), length=20 + 8 + 30 + 4), ext=1, seg=1, ua=1, li=4)])
    # ipLength == 0
    add("zero_length", [pp.group(datagram(_bytes(rng, 12), length=0)), pp.group(datagram(_bytes(rng, 12)))])
    # 4 * headerSize > ipLength: the sum runs past the vector; with the rest reading 0 it can still be good
    add("header_past_length", [pp.group(datagram(_bytes(rng, 4), hs=15, length=24, cut=24) + _bytes(rng, 3)),
                               pp.group(datagram(b"", hs=5, length=12, cut=12) + b"\x00\x00"),
                               pp.group(datagram(b"", hs=5, length=8, cut=8) + b"\x11\x11")])
    # a negative payload length: a good header, protocol 17, ipLength below 4 * headerSize + 8
    add("negative_payload", [pp.group(datagram(b"", hs=5, length=24, cut=24) + _bytes(rng, 4)),
                             pp.group(datagram(b"", hs=6, length=31, cut=31) + b"\x00"),
                             pp.group(datagram(_bytes(rng, 2)))])
    return out


KINDS = ("good", "good_crc", "good_opts", "group_crc", "too_long", "version", "checksum", "protocol", "negative", "overhang",
         "zero", "empty")
WEIGHTS = (0.30, 0.14, 0.10, 0.07, 0.06, 0.07, 0.09, 0.06, 0.04, 0.03, 0.02, 0.02)


def random_groups(seed: int, n: int = None):
    """a seeded slot: n groups (60..130 when not given) of every kind, the rule cases included.  The
    first len(KINDS) groups are one of each kind, so that every status occurs; more than half of what
    follows is deliverable."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(60, 131)) if n is None else n
    kinds = list(rng.permutation(len(KINDS))) + list(rng.choice(len(KINDS), max(0, n - len(KINDS)), p=WEIGHTS))
    groups = []
    for k in kinds[:n]:
        kind = KINDS[int(k)]
        data = _bytes(rng, int(rng.integers(0, 90)))
        hdr = dict(ext=int(rng.integers(0, 2)), seg=int(rng.integers(0, 2)), ua=int(rng.integers(0, 2)), li=int(rng.integers(0, 6)),
                   tidf=0, crcf=int(rng.integers(0, 2)))
        true = 28 + len(data)
        if kind == "good":
            g = pp.group(datagram(data), **hdr)
        elif kind == "good_crc":
            g = pp.group(datagram(data), **dict(hdr, crcf=1))
        elif kind == "good_opts":
            g = pp.group(datagram(data, hs=int(rng.integers(6, 16))), **hdr)
        elif kind == "group_crc":
            g = pp.group(datagram(data), **dict(hdr, crcf=1), good=False)
        elif kind == "too_long":
            g = pp.group(datagram(data, length=true + int(rng.integers(40, 4000))), **hdr)
        elif kind == "version":
            g = pp.group(datagram(data, version=int(rng.choice([0, 5, 6, 12, 15]))), **hdr)
        elif kind == "checksum":
            g = pp.group(datagram(data, bad=True, hs=int(rng.integers(5, 9))), **hdr)
        elif kind == "protocol":
            g = pp.group(datagram(data, proto=int(rng.choice([1, 6, 41]))), **hdr)
        elif kind == "negative":
            ln = int(rng.integers(12, 28))
            g = pp.group(datagram(b"", length=ln, cut=ln) + _bytes(rng, 3), **hdr)
        elif kind == "overhang":
            g = pp.group(datagram(data, length=true + int(rng.integers(1, 2 + (2 if hdr["crcf"] else 0)))), **hdr)
        elif kind == "zero":
            g = pp.group(datagram(data, length=0), **hdr)
        else:
            g = b""
        groups.append(bytes(g))
    return groups
