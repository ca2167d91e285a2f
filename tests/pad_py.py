"""Byte-level restatement of the reference's padHandler (src/backend/data/pad-handler.cpp) as the
PAD layer defines it (include/dabgpu.h, dabgpu_pad_aus), and the fixtures of
tests/golden/pad_kat.npz.

Handler is one padHandler: processPAD on every good AU that opens with a data stream element.
The five function-local statics of dynamicLabel are members here (a process with one
padHandler cannot tell the difference).  Where the reference is undefined or unbounded the four
rules of the header apply, and every PAD that touches one is marked: Handler.touched holds, per
processPAD call, the set of rules (1..4) it met.  The fixtures are built so that none is marked;
rule_cases() are built so that each is."""
import os

import numpy as np

import mot_py
import packet_py as pp

LABEL_BYTES, LABEL_PIECES = 256, 64
LABEL_TRUNCATED = 1
LABEL_DTYPE = np.dtype([("cif", "<i4"), ("au", "<i4"), ("charset", "<i4"), ("nbytes", "<i4"), ("n_pieces", "<i4"),
                        ("flags", "<i4"), ("piece_len", "u1", (LABEL_PIECES,)), ("text", "u1", (LABEL_BYTES,))])
RUN_DTYPE = np.dtype([("n_labels", "<i4"), ("n_groups", "<i4"), ("n_bytes", "<i4"), ("aus", "<i4"), ("pads", "<i4"),
                      ("unhandled", "<i4"), ("undefined", "<i4", (4,)), ("crc_failed", "<i4"), ("guard_dropped", "<i4"),
                      ("rejected_sf", "<i4"), ("reserved", "<i4", (3,))])
GROUP_DTYPE = pp.GROUP_DTYPE
SUBFIELD = (4, 6, 8, 12, 16, 24, 32, 48)
BUF = 8192


def sf_slots(n_frames):
    return (4 * n_frames + 4) // 5 + 1


def au_slots(n_frames):
    return sf_slots(n_frames) * 6


def arena_bytes(n_frames):
    return (BUF + au_slots(n_frames) * 192 + 15) // 16 * 16


class Handler:
    def __init__(self):
        self.last, self.last_set = 0, False            # last_appType, and whether anything wrote it
        self.index, self.length = -1, 0                # msc_dataGroupIndex / msc_dataGroupLength
        self.buf, self.hiwater = bytearray(BUF), 0     # msc_dataGroupBuffer, bytes of it ever written
        self.charset, self.cs_set = 0, False
        self.remain, self.is_last, self.more = 0, False, False   # dynamicLabel's statics
        self.text, self.pieces = bytearray(), []       # dynamicLabelText as the bytes of its appends
        self.touched = []                              # per processPAD call: set of rules met
        self.labels, self.groups = [], []              # everything delivered so far
        self.begin_run()

    def begin_run(self, arena=None):
        self.run_labels, self.run_groups, self.arena, self.arena_cap = [], [], bytearray(), arena
        self.c = dict(aus=0, pads=0, unhandled=0, undefined=[0, 0, 0, 0], crc_failed=0, guard_dropped=0, rejected_sf=0)

    # ---- processPAD and below -------------------------------------------------------------
    def au(self, data: bytes, length: int, cif=0, au=0):
        """one AU: data readable bytes, length its aac_frame_length (negative: CRC failed)"""
        if length < 0:
            return
        self.c["aus"] += 1
        B = lambda i: data[i] if i < min(length, len(data)) else 0
        if (B(0) >> 5) & 7 != 4:
            return
        self.c["pads"] += 1
        count = B(1)
        self.pad(bytes(B(2 + i) for i in range(count)), cif, au)

    def pad(self, b: bytes, cif=0, au=0):
        self.cif, self.aui, self.t = cif, au, set()
        self._pad(b)
        for r in self.t:
            self.c["undefined"][r - 1] += 1
        self.touched.append(self.t)

    def _pad(self, b):
        count = len(b)
        if count < 2:                                  # rule 1
            self.t.add(1)
            return

        def rd(i):                                     # rule 2
            if i < 0:
                self.t.add(2)
                return 0
            return b[i]
        if (b[count - 2] >> 6) & 3 != 0:
            return
        x = (b[count - 2] >> 4) & 3
        if x == 1:                                     # handle_shortPAD
            ci = rd(count - 3)
            data = [rd(count - 4 - i) for i in range(3)]
            if ci & 31 in (2, 3):
                self.label(data, 3, ci)
            return
        if x != 2 or not (b[count - 1] >> 1) & 1:      # handle_variablePAD
            return
        base, table = count - 3, []
        while rd(base) & 31 != 0 and len(table) < 4:
            table.append(rd(base))
            base -= 1
        if len(table) < 4:
            base -= 1
        for i, ci in enumerate(table):
            app, n = ci & 31, SUBFIELD[ci >> 5]
            if app == 1:
                b0, b1 = rd(base), rd(base - 1)
                rd(base - 2), rd(base - 3)             # the reference reads its unused crc
                self.length, self.index = (b0 & 63) << 8 | b1, 0
                base -= 4
                self.last, self.last_set = 1, True
                continue
            if app not in (2, 3, 12, 13):
                self.last, self.last_set = app, True
                self.c["unhandled"] += 1
                return
            data = [rd(base - j) for j in range(n)]
            if app in (2, 3):
                self.label(data, n, ci)
            else:
                if not self.last_set:                  # rule 3: last_appType is read
                    self.t.add(3)
                if (app == 12 and self.last == 1) or (app == 13 and self.last in (12, 13)):
                    self.add_msc(data)
            self.last, self.last_set = app, True
            base -= n
            if base < 0 and i < len(table) - 1:
                return

    def append(self, piece):
        if not self.cs_set:                            # rule 3: charSet is read
            self.t.add(3)
        if len(self.text) + len(piece) > LABEL_BYTES or len(self.pieces) + 1 > LABEL_PIECES:
            self.t.add(4)
        self.text += bytes(piece)
        self.pieces.append(len(piece))

    def show(self):
        lab = dict(cif=self.cif, au=self.aui, charset=self.charset, text=bytes(self.text), pieces=list(self.pieces))
        self.labels.append(lab)
        self.run_labels.append(lab)

    def label(self, data, length, ci):                 # dynamicLabel
        if ci & 31 == 2:
            prefix = data[0] << 8 | data[1]
            field_1, cflag, first, last = (prefix >> 8) & 15, (prefix >> 12) & 1, (prefix >> 14) & 1, (prefix >> 13) & 1
            if first:
                self.charset, self.cs_set = (prefix >> 4) & 15, True
                self.text, self.pieces = bytearray(), []
            if cflag:
                self.text, self.pieces = bytearray(), []
                return
            total = field_1 + 1
            if length - 2 < total:
                dl, self.more = length - 2, True
            else:
                dl, self.more = total, False
            self.append(data[2:2 + dl])
            if last:
                if not self.more:
                    self.show()
                else:
                    self.is_last = True
            else:
                self.is_last = False
            self.remain = total - dl
        elif ci & 31 == 3 and self.more:
            if self.remain > length:
                dl = length
                self.remain -= length
            else:
                dl, self.more = self.remain, False
            self.append(data[:dl])
            if not self.more and self.is_last:
                self.show()

    def add_msc(self, data):                           # add_MSC_element
        if self.index < 0:                             # rule 3: no length indicator yet (the reference reads
            self.t.add(3)                              # an index nothing initialised)
            return
        if self.index + len(data) >= BUF:
            self.c["guard_dropped"] += 1
            return
        self.buf[self.index:self.index + len(data)] = bytes(data)
        self.index += len(data)
        self.hiwater = max(self.hiwater, self.index)
        if self.index < self.length:
            return
        self.build(self.length)
        self.index = 0

    def build(self, length):                           # build_MSC_segment
        def H(i):                                      # rule 3: a byte nothing ever wrote
            if i >= self.hiwater:
                self.t.add(3)
            return self.buf[i]
        b0 = H(0)
        H(1)
        gtype, ext, crcf, seg, ua = b0 & 15, b0 >> 7, (b0 >> 6) & 1, (b0 >> 5) & 1, (b0 >> 4) & 1
        good = True
        if crcf:
            if length < 2:
                self.t.add(3)
                good = False
            else:
                good = pp.crc16(self.buf[:length - 2]) == (self.buf[length - 2] << 8 | self.buf[length - 1])
            if not good:
                self.c["crc_failed"] += 1
        index, last, segno, tid, tidf, li = 4 if ext else 2, 0, 0xFFFF, 0xFFFF, 1, 0
        if seg:
            last, segno = H(index) >> 7, (H(index) & 0x7F) << 8 | H(index + 1)
            index += 2
        if ua:
            li = H(index) & 15
            if H(index) & 0x10:
                tid = H(index + 1) << 8 | H(index + 2)
                index += 3 + li - 2
            else:
                tidf = 0
        accepted = good and gtype in (3, 4) and tidf
        stored = bytes(self.buf[:length])
        trunc = self.arena_cap is not None and len(self.arena) + length > self.arena_cap
        if trunc:
            stored, accepted = b"", False
        flags = (pp.EXT * ext | pp.CRCF * crcf | pp.SEG * seg | pp.UA * ua | pp.LAST * last | pp.TID * tidf |
                 pp.ACCEPTED * bool(accepted) | pp.TRUNCATED * trunc)
        g = dict(cif=self.cif, offset=len(self.arena), nbytes=length, data_offset=index,
                 data_nbytes=max(0, length - index - 2 * crcf), flags=flags, segmentNumber=segno, transportId=tid,
                 groupType=gtype, CI=0, lengthInd=li, au=self.aui & 255, stored=stored,
                 data=bytes(self.buf[index:index + max(0, length - index - 2 * crcf)]))
        self.arena += stored
        self.groups.append(g)
        self.run_groups.append(g)

    # ---- the layer's records ----------------------------------------------------------------
    def feed(self, aus, arena=None):
        """a run: aus is a list of (bytes, length) or (bytes, length, cif, au)"""
        self.begin_run(arena)
        for k, a in enumerate(aus):
            self.au(a[0], a[1], a[2] if len(a) > 2 else k, a[3] if len(a) > 3 else k)
        return self

    def label_records(self):
        out = np.zeros(len(self.run_labels), LABEL_DTYPE)
        for r, l in zip(out, self.run_labels):
            r["cif"], r["au"], r["charset"], r["nbytes"], r["n_pieces"] = l["cif"], l["au"], l["charset"], len(l["text"]), len(l["pieces"])
            r["flags"] = LABEL_TRUNCATED * (len(l["text"]) > LABEL_BYTES or len(l["pieces"]) > LABEL_PIECES)
            t, p = l["text"][:LABEL_BYTES], l["pieces"][:LABEL_PIECES]
            r["text"][:len(t)] = np.frombuffer(t, np.uint8)
            r["piece_len"][:len(p)] = p
        return out

    def group_records(self):
        out = np.zeros(len(self.run_groups), GROUP_DTYPE)
        for r, g in zip(out, self.run_groups):
            for k in GROUP_DTYPE.names:
                if k != "reserved":
                    r[k] = g[k]
            r["reserved"][0] = g["au"]
        return out

    def run_record(self):
        r = np.zeros((), RUN_DTYPE)
        r["n_labels"], r["n_groups"], r["n_bytes"] = len(self.run_labels), len(self.run_groups), len(self.arena)
        for k in ("aus", "pads", "unhandled", "crc_failed", "guard_dropped", "rejected_sf"):
            r[k] = self.c[k]
        r["undefined"] = self.c["undefined"]
        return r


# ---- writers ------------------------------------------------------------------------------
def xpad(cis, fields, x_ind=2, ftype=0, ci_flag=1, marker=None, fill=b""):
    """a variable-size PAD.  cis: (application type, sub-field length) per content indicator;
    fields: the sub-fields' bytes in logical order (each padded with zeros to its length).  An
    end marker follows fewer than four CIs (marker=False leaves it out).  fill: bytes below the
    last sub-field (the PAD's first bytes)."""
    logical = bytearray([ci_flag << 1, ftype << 6 | x_ind << 4])
    for app, n in cis:
        logical.append(SUBFIELD.index(n) << 5 | app)
    if (len(cis) < 4) if marker is None else marker:
        logical.append(0)
    for (app, n), f in zip(cis, fields):
        assert len(f) <= n
        logical += bytes(f) + bytes(n - len(f))
    return bytes(fill) + bytes(reversed(logical))


def short_pad(app, data3, ftype=0, x_ind=1, fill=b"\0\0"):
    """a short PAD: one CI and three bytes (the reference reads them at fixed places)"""
    logical = bytearray([0, ftype << 6 | x_ind << 4, app]) + bytes(data3) + bytes(3 - len(data3))
    return bytes(fill) + bytes(reversed(logical))


def au_of(pad: bytes, tail=b"\x12\x34\x56", first=0x80):
    """an AU that opens with a data stream element holding the PAD; returns (bytes, length)"""
    a = bytes([first, len(pad)]) + bytes(pad) + bytes(tail)
    return a, len(a)


def seg_prefix(nbytes, first=0, last=0, cflag=0, charset=0, segno=0, toggle=0):
    f1 = (nbytes - 1) & 15
    return bytes([toggle << 7 | first << 6 | last << 5 | cflag << 4 | f1, ((charset if first else segno) & 15) << 4])


def label_pads(text: bytes, charset=0, sizes=(16,), seg_bytes=16, toggle=0):
    """a label as segments of at most seg_bytes, each opened by a type-2 sub-field and continued
    by type-3 sub-fields, one sub-field per PAD, their lengths cycling through sizes"""
    pads, k = [], 0
    segs = [text[i:i + seg_bytes] for i in range(0, len(text), seg_bytes)]
    for s, seg in enumerate(segs):
        stream = seg_prefix(len(seg), first=int(s == 0), last=int(s == len(segs) - 1), charset=charset, segno=s, toggle=toggle) + seg
        app = 2
        while stream:
            n = sizes[k % len(sizes)]
            k += 1
            pads.append(xpad([(app, n)], [stream[:n]]))
            stream, app = stream[n:], 3
    return pads


def group_pads(g: bytes, first=48, rest=48, per_pad=1):
    """an MSC data group as X-PAD: a length indicator (type 1) and a type-12 sub-field in the
    first PAD, type-13 sub-fields after it, per_pad of them in every later PAD"""
    pads = [xpad([(1, 4), (12, first)], [bytes([len(g) >> 8 & 63, len(g) & 255, 0, 0]), g[:first]])]
    g = g[first:]
    while g:
        cis, fields = [], []
        for _ in range(per_pad):
            if g:
                cis.append((13, rest))
                fields.append(g[:rest])
                g = g[rest:]
        pads.append(xpad(cis, fields))
    return pads


def slide(tid=0x4242, nbytes=100, seg=40, seed=5, name=b"pad.jpg"):
    rng = np.random.default_rng(seed)
    body = rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()
    groups = [mot_py.header_group(tid, nbytes, mot_py.name_param(name))] + mot_py.body_groups(tid, body, seg)
    return groups, body


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def fixtures():
    """the AU sequences of tests/golden/pad_kat.npz, each at most 64 AUs: dicts with name and
    aus, a list of (bytes, length).  No PAD of any touches rules 1-4 (the generator and
    test_pad_cpu assert it)."""
    rng = np.random.default_rng(20261)
    fx = []

    def add(name, pads_or_aus):
        aus = [p if isinstance(p, tuple) else au_of(p) for p in pads_or_aus]
        assert len(aus) <= 64, name
        fx.append(dict(name=name, aus=aus))

    G = lambda data, **kw: pp.group(data, **{**dict(crcf=1, seg=1, ua=1, gtype=4, tid=0x0BCD), **kw})
    # a one-byte label, its first segment also the last, in short PADs; a type 3 that nothing expects
    add("short", [short_pad(2, seg_prefix(1, 1, 1, charset=15) + b"A"), short_pad(3, b"xyz"),
                  short_pad(2, seg_prefix(1, 1, 1, charset=0) + b"B"), short_pad(7, b"abc"),
                  # a three-byte segment started in a short PAD and continued in the next
                  short_pad(2, seg_prefix(3, 1, 1, charset=0) + b"C"), short_pad(3, b"DE!"), short_pad(3, b"???")])
    add("one_subfield", [xpad([(2, 16)], [seg_prefix(11, 1, 1, charset=0) + b"hello world"])])
    add("segments", label_pads(b"first segment 16middle segment 2the last", charset=15, sizes=(24,)))
    add("continued", label_pads(b"sixteen bytes...and nine more", sizes=(6, 4, 8, 12)) +
        label_pads(b"again, other cut", sizes=(4,), toggle=1))
    add("clear", label_pads(b"to be cleared", sizes=(8,))[:1] +                  # a segment left waiting for its type 3
        [xpad([(2, 4)], [seg_prefix(1, 0, 0, cflag=1)]),                         # the clear command: moreXPad stays set
         xpad([(3, 8)], [b"STALE..."]), xpad([(3, 4)], [b"zzzz"]),               # ... so these are appended
         xpad([(2, 8)], [seg_prefix(3, 0, 1, segno=1) + b"end"])])
    add("four_cis", [xpad([(2, 6), (3, 4), (3, 4), (3, 4)], [seg_prefix(14, 1, 1) + b"abcd", b"efgh", b"ijkl", b"mn"]),
                     xpad([(2, 8), (3, 6)], [seg_prefix(10, 1, 1) + b"012345", b"6789"]),
                     xpad([(2, 6), (3, 4), (3, 4), (3, 4)], [seg_prefix(16, 1, 1) + b"ABCD", b"EFGH", b"IJKL", b"MNOP"], fill=b"\x55\xAA")])
    add("group_exact", group_pads(G(_bytes(rng, 96 - 9)), 48, 48))               # 2 + 2 + 3 header, 87 data, 2 CRC
    add("group_excess", group_pads(G(_bytes(rng, 61)), 24, 32))
    g = G(_bytes(rng, 23))                                                       # 32 bytes: every 13 after the first completes one
    add("group_repeat", group_pads(g, 16, 16) + [xpad([(13, 32)], [g]), xpad([(13, 16), (13, 16)], [g[:16], g[16:]]),
                                                 xpad([(13, 48)], [_bytes(rng, 48)])])
    add("group_crc", group_pads(G(_bytes(rng, 50)), 48, 48) + group_pads(G(_bytes(rng, 50), good=False), 48, 48) +
        group_pads(G(_bytes(rng, 30), crcf=0), 48, 48))
    hdr = []
    for ext in (0, 1):
        for seg in (0, 1):
            for ua in (0, 1):
                hdr += group_pads(G(_bytes(rng, 17 + 4 * ext + seg), ext=ext, seg=seg, ua=ua, gtype=3 + seg, last=ext, segno=5 + ua), 32, 32)
    hdr += group_pads(G(_bytes(rng, 20), li=6), 48, 48)
    add("group_header", hdr)
    add("group_no_tid", group_pads(G(_bytes(rng, 20), tidf=0), 48, 48) + group_pads(G(_bytes(rng, 20)), 48, 48))
    add("group_type6", group_pads(G(_bytes(rng, 40), gtype=6), 48, 48) + group_pads(G(_bytes(rng, 12), gtype=3), 48, 48))
    # a length the buffer cannot hold: the guard drops what would pass 8191, nothing completes
    big = [xpad([(1, 4), (12, 48), (13, 48), (13, 48)], [bytes([8200 >> 8, 8200 & 255, 0, 0])] + [_bytes(rng, 48)] * 3)]
    big += [xpad([(13, 48)] * 4, [_bytes(rng, 48)] * 4) for _ in range(44)]
    add("guard", big + group_pads(G(_bytes(rng, 9)), 48, 48))
    add("unhandled", [xpad([(2, 8), (5, 8), (2, 8)], [seg_prefix(4, 1, 1) + b"seen", b"whatever", seg_prefix(4, 1, 1) + b"lost"]),
                      xpad([(13, 8)], [b"13 after"]), xpad([(31, 4)], [b"...."]), short_pad(2, seg_prefix(1, 1, 1) + b"k")])
    # a 12 that no length indicator precedes is not taken; the 13 after it is (last_appType is 12) and
    # goes on filling a group of the old length; a 13 after a label is not
    add("orphan_12", group_pads(G(_bytes(rng, 9)), 48, 48) +
        [xpad([(2, 6)], [seg_prefix(2, 1, 1) + b"ok"]), xpad([(12, 8)], [b"no start"]), xpad([(13, 8)], [b"nor here"]),
         xpad([(2, 6), (13, 24)], [seg_prefix(2, 1, 1) + b"2!", G(_bytes(rng, 13))]), xpad([(13, 16)], [_bytes(rng, 16)])])
    add("fpad_type1", [xpad([(2, 6)], [seg_prefix(2, 1, 1) + b"no"], ftype=1), short_pad(2, seg_prefix(1, 1, 1) + b"n", ftype=2),
                       xpad([(2, 6)], [seg_prefix(2, 1, 1) + b"no"], ftype=3)])
    add("xpad_ind", [xpad([(2, 6)], [seg_prefix(2, 1, 1) + b"no"], x_ind=0), xpad([(2, 6)], [seg_prefix(2, 1, 1) + b"no"], x_ind=3),
                     xpad([(2, 6)], [seg_prefix(3, 1, 1) + b"yes"], x_ind=2)])
    add("ci_flag0", [xpad([(2, 6)], [seg_prefix(2, 1, 1) + b"no"], ci_flag=0), xpad([(2, 6)], [seg_prefix(3, 1, 1) + b"yes"])])
    # AUs the PAD layer never sees as PADs: another first element, a failed CRC; bytes past the length read 0
    other = au_of(xpad([(2, 6)], [seg_prefix(2, 1, 1) + b"no"]), first=0x20)
    bad = (au_of(xpad([(2, 6)], [seg_prefix(2, 1, 1) + b"no"]))[0], -1)
    cut = au_of(xpad([(2, 8)], [seg_prefix(6, 1, 1) + b"cutoff"]))
    add("au_kinds", [other, bad, (cut[0], 2 + 3 + 3), (bytes([0x80, 4]), 2), cut])
    sl, _ = slide()
    pads = []
    for rep in range(2):
        for g in sl:
            pads += group_pads(g, 48, 48, per_pad=1 + rep)
    add("slide", label_pads(b"Now: a slide", charset=15) + pads)
    # a seeded mix, built and not filtered: labels, groups and unhandled types interleaved
    mix = []
    for k in range(12):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            mix += label_pads(_bytes(rng, int(rng.integers(1, 40))), charset=int(rng.integers(0, 16)),
                              sizes=tuple(int(x) for x in rng.choice(SUBFIELD, 3)), seg_bytes=int(rng.integers(4, 17)))
        elif kind == 1:
            mix += group_pads(G(_bytes(rng, int(rng.integers(1, 120))), good=bool(rng.integers(0, 4)),
                                gtype=int(rng.choice([3, 4, 4, 6]))), int(rng.choice(SUBFIELD)), int(rng.choice(SUBFIELD[2:])),
                              per_pad=int(rng.integers(1, 4)))
        elif kind == 2:
            mix.append(short_pad(2, seg_prefix(int(rng.integers(1, 4)), 1, int(rng.integers(0, 2))) + _bytes(rng, 1)))
            mix.append(short_pad(3, _bytes(rng, 3)))
        else:
            mix.append(xpad([(int(rng.choice([4, 5, 14])), 8)], [_bytes(rng, 8)]))
    add("mix", mix[:64])
    return fx


def rule_cases():
    """PADs outside the golden file, each touching one of the rules 1-4 (name: rule<k>...)"""
    out = []
    lab = seg_prefix(2, 1, 1) + b"ok"
    out.append(dict(name="rule1", rule=1, aus=[(bytes([0x80, 0, 9, 9]), 4), (bytes([0x80, 1, 0x20]), 3), au_of(xpad([(2, 6)], [lab]))]))
    r2 = [short_pad(2, seg_prefix(1, 1, 1) + b"s", fill=b""),              # count 6 is the least a short PAD can have: 5 ...
          short_pad(2, seg_prefix(1, 1, 1) + b"s", fill=b"")[1:],          # ... reads its last data byte below the PAD
          bytes([0x10, 0]),                                                 # count 2: the CI itself lies below
          xpad([(2, 16)], [seg_prefix(14, 1, 1) + b"fourteen bytes"])[6:],  # a sub-field longer than what is left
          xpad([(1, 4)], [bytes([0, 40, 0, 0])])[3:],                       # a length indicator cut short
          xpad([(2, 8), (2, 8)], [seg_prefix(6, 1, 1) + b"sixsix", seg_prefix(6, 1, 1) + b"SIXSIX"])[12:],   # the :168 check
          bytes([0x43, 0x22, 0x20, 0x02])]                                  # CIs down to byte 0, the next read is below
    out.append(dict(name="rule2", rule=2, aus=[au_of(p) for p in r2]))
    G = lambda data, **kw: pp.group(data, **{**dict(crcf=1, seg=1, ua=1, gtype=4, tid=0x0BCD), **kw})
    r3 = [xpad([(13, 8)], [b"13 first"]),                                   # last_appType read before anything wrote it
          xpad([(2, 6)], [seg_prefix(2, 0, 1, segno=1) + b"cs"]),           # charSet read before a first segment
          xpad([(1, 4), (12, 4)], [bytes([0, 1, 0, 0]), bytes([0xF4, 0, 0, 0])]),   # one byte long: the header lies in bytes
          xpad([(1, 4), (12, 4)], [bytes([0, 1, 0, 0]), bytes([0x44, 0, 0, 0])])]   # ... nothing wrote; CRC flag and length 1
    out.append(dict(name="rule3", rule=3, aus=[au_of(p) for p in r3]))
    out.append(dict(name="rule4_bytes", rule=4, aus=[au_of(p) for p in label_pads(b"x" * 16, sizes=(24,)) +
                                                     [xpad([(2, 24)], [seg_prefix(16, 0, 0, segno=1) + b"y" * 16])] * 15 +
                                                     [xpad([(2, 6)], [seg_prefix(1, 0, 1, segno=2) + b"z"])]]))
    out.append(dict(name="rule4_pieces", rule=4, aus=[au_of(p) for p in [xpad([(2, 6)], [seg_prefix(1, 1, 0) + b"a"])] +
                                                      [xpad([(2, 6)], [seg_prefix(1, 0, 0, segno=1) + b"b"])] * 63 +
                                                      [xpad([(2, 6)], [seg_prefix(1, 0, 1, segno=1) + b"c"])]]))
    return out


def load_kat():
    """tests/golden/pad_kat.npz as a list of dicts: name, aus [(bytes, length)], the labels and the
    process_mscGroup calls the reference made"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pad_kat.npz"))
    out = []
    for i, name in enumerate(z["names"]):
        lens, nbs, raw = z["au_len_%d" % i].tolist(), z["au_nbytes_%d" % i].tolist(), z["au_bytes_%d" % i].tobytes()
        aus, pos = [], 0
        for ln, nb in zip(lens, nbs):
            aus.append((raw[pos:pos + nb], ln))
            pos += nb
        labels, pcs, text = [], z["label_pieces_%d" % i].tolist(), z["label_bytes_%d" % i].tobytes()
        ppos = tpos = 0
        for au, cs, npc, nb in z["labels_%d" % i].tolist():
            labels.append(dict(au=au, charset=cs, pieces=pcs[ppos:ppos + npc], text=text[tpos:tpos + nb]))
            ppos, tpos = ppos + npc, tpos + nb
        calls, cb, cpos = [], z["call_bytes_%d" % i].tobytes(), 0
        for au, gt, last, segno, tid, index, length in z["calls_%d" % i].tolist():
            calls.append(dict(au=au, groupType=gt, last=last, segmentNumber=segno & 0xFFFF, transportId=tid, index=index,
                              bytes=cb[cpos:cpos + length]))
            cpos += length
        out.append(dict(name=str(name), aus=aus, labels=labels, calls=calls))
    return out
