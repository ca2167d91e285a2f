"""TEST INFRASTRUCTURE: the packet-mode data layer restated at byte level, and its fixtures.

Assembler is mscDatagroup::handlePackets / handlePacket (msc-datagroup.cpp:221-319, with
show_crcErrors on) followed by the header parse and CRC of mot_databuilder::add_mscDatagroup
(mot-databuilder.cpp:37-95), with the layer's records: the per-CIF info, the 500-packet
window, the group records and the cap.  The assembling itself is oracle_py.Datagroups'
(imported unchanged; test_packet_cpu holds the two against each other bit for bit) and the
whole is pinned to the reference's own code by tests/golden/packet_kat.npz.

Three rules where the reference is undefined or unbounded (include/dabgpu.h):
  1. header fields past a group's end read 0 (a CRC-flagged group below 2 bytes: bad CRC);
  2. lengths are int32;
  3. a series above the cap keeps its first `cap` bytes, reports its full length, is flagged
     truncated and is not accepted.
"""
import binascii

import numpy as np

import oracle_py as orc  # noqa: F401  (Datagroups: the bit-level restatement this one is held against)

GROUP_BYTES = 8216
INFO_DTYPE = np.dtype([("status", "<i2"), ("packets", "<i2"), ("crc_errors", "<i2"), ("groups", "<i2"),
                       ("quality", "<i2"), ("address", "<i2")])
RUN_DTYPE = np.dtype([("n_groups", "<i4"), ("n_bytes", "<i4"), ("state", "<i4"), ("pending_bytes", "<i4")])
GROUP_DTYPE = np.dtype([("cif", "<i4"), ("offset", "<i4"), ("nbytes", "<i4"), ("data_offset", "<i4"),
                        ("data_nbytes", "<i4"), ("flags", "<u2"), ("segmentNumber", "<u2"), ("transportId", "<u2"),
                        ("groupType", "u1"), ("CI", "u1"), ("lengthInd", "u1"), ("reserved", "u1", (3,))])
EXT, CRCF, SEG, UA, LAST, TID, ACCEPTED, TRUNCATED = 1, 2, 4, 8, 16, 32, 64, 128


def crc16(data: bytes) -> int:
    """CRC-16-CCITT from all ones, inverted: what a packet or a data group ends with"""
    return binascii.crc_hqx(bytes(data), 0xFFFF) ^ 0xFFFF


def crc_good(data: bytes) -> bool:
    """check_CRC_bits on bytes; fewer than two: bad (rule 1)"""
    return len(data) >= 2 and crc16(data[:-2]) == (data[-2] << 8 | data[-1])


def parse_group(series: bytes, cap: int = GROUP_BYTES) -> dict:
    """the generic MSC data group header (mot-databuilder.cpp:37-95) of a completed series"""
    nb = len(series)
    st = bytes(series[:cap])
    B = lambda i: st[i] if i < len(st) else 0
    ext, crcf, seg, ua = B(0) >> 7, (B(0) >> 6) & 1, (B(0) >> 5) & 1, (B(0) >> 4) & 1
    trunc = nb > cap
    nxt = 2 + (2 if ext else 0)
    last = segno = tidf = tid = li = 0
    if seg:
        last, segno = B(nxt) >> 7, (B(nxt) & 0x7F) << 8 | B(nxt + 1)
        nxt += 2
    if ua:
        tidf, li = (B(nxt) >> 4) & 1, B(nxt) & 15
        nxt += 1
        if tidf:
            tid = B(nxt) << 8 | B(nxt + 1)
        nxt += li
    good = (not crcf) or (not trunc and crc_good(st))
    accepted = nb > 0 and not trunc and good
    flags = (EXT * ext | CRCF * crcf | SEG * seg | UA * ua | LAST * last | TID * tidf | ACCEPTED * accepted |
             TRUNCATED * trunc)
    return dict(nbytes=nb, stored=st, flags=flags, groupType=B(0) & 15, CI=B(1) >> 4, lengthInd=li, segmentNumber=segno,
                transportId=tid, data_offset=nxt, data_nbytes=max(0, nb - nxt - (2 if crcf else 0)))


class Assembler:
    """one mscDatagroup (DSCTy 60, show_crcErrors on) fed CIF rows of 3 * bitrate bytes"""

    def __init__(self, bitrate: int, cap: int = GROUP_BYTES):
        self.nbytes, self.cap = 3 * bitrate, cap
        self.state, self.addr, self.series = 0, -1, bytearray()
        self.handled = self.window_errors = 0
        self.qualities = []                    # every show_mscErrors value
        self.delivered = []                    # every completed series, whole
        self.begin_run()

    def begin_run(self):
        self.groups, self.arena = [], bytearray()

    def skip(self):
        """a CIF that is not fed"""
        return (-1, 0, 0, 0, -1, self.addr)

    def cif(self, q: int, row) -> tuple:
        """one fed CIF (slot q of the run) -> its dabgpu_packet_info"""
        data = bytearray(bytes(row[:self.nbytes]))
        assert len(data) == self.nbytes
        pos, left = 0, self.nbytes
        packets = errors = 0
        quality, n0 = -1, len(self.groups)
        while True:
            plen = ((data[pos] >> 6) + 1) * 24
            if left < plen:
                break
            self.handled += 1
            if self.handled >= 500:
                quality = 100 - self.window_errors // 5
                self.qualities.append(quality)
                self.window_errors = self.handled = 0
            packets += 1
            ok = crc_good(data[pos:pos + plen])
            data[pos + plen - 2] ^= 0xFF           # check_CRC_bits leaves the CRC field inverted
            data[pos + plen - 1] ^= 0xFF
            if ok:
                self._good(q, data, pos)
            else:
                errors += 1
                self.window_errors += 1
            left -= plen
            if left == 0:
                break
            pos += plen
        return (0, packets, errors, len(self.groups) - n0, quality, self.addr)

    def _good(self, q, data, pos):
        fl, addr, useful = (data[pos] >> 2) & 3, (data[pos] & 3) << 8 | data[pos + 1], data[pos + 2] & 0x7F
        if addr == 0:
            return
        if self.addr == -1:
            self.addr = addr
        if self.addr != addr:
            return
        take = data[pos + 3:pos + 3 + useful]      # whatever the packet's length; the slice stops at the CIF's end
        if self.state == 0:
            if fl == 2:
                self.state, self.series = 1, bytearray(take)
            elif fl == 3:
                self.series = bytearray(take)
                self._deliver(q)
            else:
                self.series = bytearray()
        elif fl == 0:
            self.series += take
        elif fl == 1:
            self.series += take
            self._deliver(q)
            self.state = 0
        elif fl == 2:
            self.series = bytearray(take)
        else:
            self.state, self.series = 0, bytearray()

    def _deliver(self, q):
        g = parse_group(bytes(self.series), self.cap)
        g["cif"], g["offset"] = q, len(self.arena)
        self.arena += g["stored"]
        self.groups.append(g)
        self.delivered.append(bytes(self.series))

    def run_record(self):
        return (len(self.groups), len(self.arena), self.state, len(self.series) if self.state else 0)

    def group_records(self):
        out = np.zeros(len(self.groups), GROUP_DTYPE)
        for r, g in zip(out, self.groups):
            for k in GROUP_DTYPE.names:
                if k != "reserved":
                    r[k] = g[k]
        return out


# ---- writers ------------------------------------------------------------------------------
def packet(lc, fl, addr, payload=b"", useful=None, bad=False, ci=0, fill=0):
    """a packet of (lc + 1) * 24 bytes; useful: the useful-length field when it is not len(payload)"""
    n = (lc + 1) * 24
    assert len(payload) <= n - 5
    u = len(payload) if useful is None else useful
    body = bytes([lc << 6 | ci << 4 | fl << 2 | addr >> 8, addr & 255, u & 0x7F]) + bytes(payload)
    body += bytes([fill]) * (n - 2 - len(body))
    c = crc16(body)
    out = bytearray(body + bytes([c >> 8, c & 255]))
    if bad:
        out[5] ^= 0x10
    return bytes(out)


def group(data=b"", ext=0, crcf=0, seg=0, ua=0, gtype=3, ci=0, last=0, segno=0, tidf=1, tid=0x1234, li=2, good=True):
    """an MSC data group: header as the flags say, data, CRC when flagged"""
    h = bytearray([ext << 7 | crcf << 6 | seg << 5 | ua << 4 | gtype, ci << 4])
    if ext:
        h += b"\xAB\xCD"
    if seg:
        h += bytes([last << 7 | segno >> 8, segno & 255])
    if ua:
        h += bytes([tidf << 4 | li])
        h += (bytes([tid >> 8, tid & 255]) + bytes(range(1, 14)))[:li]
    g = bytes(h) + bytes(data)
    if crcf:
        c = crc16(g) ^ (0 if good else 0x0400)
        g += bytes([c >> 8, c & 255])
    return g


def packetize(g: bytes, addr: int, lcs, ci0=0):
    """a group cut into packets whose length codes cycle through lcs"""
    out, pos, k = [], 0, 0
    while True:
        lc = lcs[k % len(lcs)]
        n = min((lc + 1) * 24 - 5, len(g) - pos)
        first, lastp = pos == 0, pos + n >= len(g)
        out.append(packet(lc, 3 if first and lastp else 2 if first else 1 if lastp else 0, addr, g[pos:pos + n], ci=(ci0 + k) & 3))
        pos += n
        k += 1
        if lastp:
            return out


def rows(packets, bitrate):
    """packets laid into CIFs of 3 * bitrate bytes in order; a CIF is closed with padding
    packets (address 0) when the next packet does not fit"""
    n, out, cur = 3 * bitrate, [], b""
    for p in packets:
        if len(cur) + len(p) > n:
            cur += packet(0, 0, 0) * ((n - len(cur)) // 24)
            out.append(cur)
            cur = b""
        cur += p
    cur += packet(0, 0, 0) * ((n - len(cur)) // 24)
    out.append(cur)
    return np.frombuffer(b"".join(out), np.uint8).reshape(len(out), n).copy()


def _bytes(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def fixtures():
    """the streams of tests/golden/packet_kat.npz: [{name, bitrate, rows [n_cif][3 * bitrate]}].
    Every read the reference makes on them is defined."""
    rng = np.random.default_rng(2026)
    fx = []
    # the sequence of test_consumers_cpu.test_packet_datagroups_match_reference
    seq = [(0, 3, 77, 10, False), (0, 0, 0, 0, False), (0, 2, 77, 19, False), (0, 0, 77, 19, False), (0, 1, 77, 5, False),
           (0, 2, 77, 19, False), (0, 0, 77, 17, True), (0, 1, 77, 5, False), (0, 2, 99, 18, False), (0, 3, 99, 8, False),
           (0, 2, 77, 12, False), (0, 2, 77, 12, False), (0, 1, 77, 3, False), (1, 3, 77, 40, False), (0, 3, 77, 1, False),
           (0, 0, 0, 0, False)]
    fx.append(dict(name="sequence", bitrate=32, rows=rows([packet(lc, fl, a, _bytes(rng, n), bad=bad)
                                                           for lc, fl, a, n, bad in seq], 32)))
    # all four lengths: at 8 kbit/s only the 24-byte packet fits its CIF, the others overrun it
    for br in (8, 32, 64):
        pk = []
        for k in range(12):
            lc = k & 3
            g = group(_bytes(rng, 4 + 7 * k), crcf=k & 1, seg=(k >> 1) & 1, segno=k)
            pk += packetize(g, 77, [lc]) if br > 8 else [packet(lc, 3, 77, g[:19])]
        fx.append(dict(name="lengths%d" % br, bitrate=br, rows=rows(pk, br) if br > 8 else
                       np.frombuffer(b"".join(p[:24] for p in pk), np.uint8).reshape(-1, 24).copy()))
    # a length code that overruns what is left of the CIF: the walk stops there
    r = rows(packetize(group(_bytes(rng, 60)), 77, [1]) + [packet(0, 3, 77, b"xyz")], 32)
    r[0, 48] |= 0x80                                   # the second packet of CIF 0 now claims 72 bytes of 48
    fx.append(dict(name="overrun", bitrate=32, rows=r))
    # useful lengths 92..127 in 24-byte packets at bytes 0 and 192 of 384: the copy runs over the
    # packet's own CRC field and the packets behind it, never past the CIF's end
    rr = []
    for u in range(92, 128, 2):
        cif = bytearray()
        for uu in (u, u + 1):
            cif += packet(0, 3, 77, _bytes(rng, 19), useful=uu)
            lcs = ([0] * 7, [1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0])[int(rng.integers(0, 3))]      # 168 bytes behind it
            cif += b"".join(packet(lc, (0, 1, 3)[int(rng.integers(0, 3))], 77 if rng.integers(0, 2) else 0, b"\x03" + _bytes(rng, 18),
                                   bad=bool(rng.integers(0, 3) == 0)) for lc in lcs)
        rr.append(bytes(cif))
    fx.append(dict(name="useful", bitrate=128, rows=np.frombuffer(b"".join(rr), np.uint8).reshape(len(rr), 384).copy()))
    # 1040 packets with scattered CRC errors: two 500-packet windows
    pk = []
    while len(pk) < 1040:
        pk += packetize(group(_bytes(rng, int(rng.integers(1, 120))), crcf=1), 77, [0])
    pk = [bytes(p[:7] + bytes([p[7] ^ 1]) + p[8:]) if rng.integers(0, 9) == 0 else p for p in pk[:1040]]
    fx.append(dict(name="window", bitrate=128, rows=rows(pk, 128)))
    # every combination of the four header flags, lengthInd 0, 3 and 15, good and bad group
    # CRCs, sizes from 1 byte to 4000 bytes
    pk = []
    for k in range(16):
        li = (0, 3, 15)[k % 3]
        g = group(_bytes(rng, 20 + 3 * k), ext=k & 1, crcf=(k >> 1) & 1, seg=(k >> 2) & 1, ua=(k >> 3) & 1, gtype=k & 15,
                  ci=(5 * k) & 15, last=k & 1, segno=1000 * k + 3, tidf=1 if li else 0, tid=0x8000 | k, li=li,
                  good=k not in (2, 11))
        pk += packetize(g, 77, [3, 1, 0], ci0=k)
    pk += packetize(b"\x03", 77, [0])                  # one byte
    for n, good in ((9, True), (30, True), (500, False), (1000, True), (4000, True)):     # 9: header and CRC alone
        pk += packetize(group(_bytes(rng, n - 9), crcf=1, seg=1, ua=1, segno=n, li=2, good=good), 77, [3])
    fx.append(dict(name="headers", bitrate=128, rows=rows(pk, 128)))
    return fx


def extra_fixtures():
    """cases the reference cannot run (its reads are undefined or its int16 wraps), for the
    three rules and the clip at the CIF's end: [{name, bitrate, cap, rows}]"""
    rng = np.random.default_rng(77)
    out = []
    # a useful length that reaches past the CIF's end: the last packet of the CIF claims 127
    pk = [packet(0, 2, 77, _bytes(rng, 19)), packet(0, 0, 77, _bytes(rng, 19)), packet(0, 0, 77, _bytes(rng, 19)),
          packet(0, 1, 77, _bytes(rng, 19), useful=127), packet(0, 3, 77, _bytes(rng, 19), useful=60)]
    out.append(dict(name="clip", bitrate=32, cap=GROUP_BYTES, rows=rows(pk, 32)))
    # groups shorter than their header (ext + seg + ua flags, then nothing), one with the CRC flag and 1 byte
    pk = []
    for g in (b"\xB3", b"\xB3\x50\x11", b"\xF3\x50\x11\x22\x93", b"\x43", b"\x33\x00\x80"):
        pk += packetize(g, 77, [0])
    out.append(dict(name="short", bitrate=32, cap=GROUP_BYTES, rows=rows(pk, 32)))
    # above 4095 bytes: int16 sizeinBits would wrap
    pk = packetize(group(_bytes(rng, 4500), crcf=1, seg=1, ua=1, li=2), 77, [3])
    out.append(dict(name="big", bitrate=128, cap=GROUP_BYTES, rows=rows(pk, 128)))
    # above a 256-byte cap: truncated, and the groups around it are whole
    pk = packetize(group(_bytes(rng, 100), crcf=1), 77, [1]) + packetize(group(_bytes(rng, 700), crcf=1), 77, [3, 0])
    pk += packetize(group(_bytes(rng, 250), crcf=1), 77, [2]) + packetize(group(_bytes(rng, 251), crcf=1), 77, [3])
    out.append(dict(name="cap", bitrate=128, cap=256, rows=rows(pk, 128)))
    return out
