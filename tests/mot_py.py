"""Byte-level restatement of the MOT layer: motHandler::process_mscGroup in header mode
(mot-data.cpp:679-728: processHeader :56-133, processSegment :278-312, newEntry :612-656,
getHandle :590-609, isComplete :578-588, handleComplete :315-336, show_slide :337-346) over the
groups mot_databuilder::add_mscDatagroup passes on (accepted, with a transport id), with the
rules of include/dabgpu.h (dabgpu_mot_groups) where the reference is undefined or unbounded.

The kernel (csrc/k_mot.hip), the host motAssembler and this file are three statements of one
function; tests/golden/mot_kat.npz, written by the reference's own mot-data.cpp, pins them.
"""
import numpy as np

import packet_py as pp

BODY_BYTES = 65536          # DABGPU_MOT_BODY_BYTES
NAME_BYTES = 128            # DABGPU_MOT_NAME_BYTES
ENTRIES = 16
SLIDE, EPG, FILE = 1, 2, 3  # dabgpu_mot_object.kind
TOO_LARGE, OVERFLOW = 1, 2  # DABGPU_MOT_*

OBJECT_DTYPE = np.dtype([("group", "<i4"), ("cif", "<i4"), ("offset", "<i4"), ("nbytes", "<i4"),
                         ("transportId", "<u2"), ("contentType", "u1"), ("kind", "u1"), ("contentsubType", "<u2"),
                         ("flags", "<u2"), ("name_len", "<i4"), ("name", "u1", (NAME_BYTES,))])
RUN_DTYPE = np.dtype([("n_objects", "<i4"), ("n_bytes", "<i4"), ("malformed", "<i4"), ("bad_segment", "<i4"),
                      ("other_types", "<i4"), ("entries", "<i4"), ("reserved", "<i4", (2,))])
HEAD_DTYPE = np.dtype([("created", "<i4"), ("old_slide", "<i4"), ("reserved", "<i4", (2,))])
ENTRY_DTYPE = np.dtype([("order", "<i4"), ("transportId", "<i4"), ("bodySize", "<i4"), ("segmentSize", "<i4"),
                        ("numofSegments", "<i4"), ("contentType", "<i4"), ("contentsubType", "<i4"), ("flags", "<i4"),
                        ("marked", "<u4", (4,)), ("name_len", "<i4"), ("reserved", "<i4"), ("name", "u1", (NAME_BYTES,))])


def body_cap(max_body_bytes: int) -> int:
    return (max_body_bytes + 15) // 16 * 16


def state_bytes(max_body_bytes: int = BODY_BYTES) -> int:
    """dabgpu_mot_state_bytes"""
    return HEAD_DTYPE.itemsize + ENTRIES * ENTRY_DTYPE.itemsize + ENTRIES * body_cap(max_body_bytes)


def arena_bytes(group_slots: int, max_body_bytes: int = BODY_BYTES) -> int:
    """DABGPU_MOT_ARENA_BYTES for a run of group_slots groups"""
    return body_cap(max_body_bytes) + group_slots * 144


class Entry:
    def __init__(self):
        self.order = 0                   # 0: free (the reference's ordernumber -1)
        self.tid = self.bodySize = self.contentType = self.contentsubType = self.flags = 0
        self.segmentSize = self.numofSegments = 0
        self.marked = [False] * 128
        self.name = b""
        self.body = bytearray()


class Assembler:
    """one motHandler; feed(records, arena) takes the groups of one dabgpu_pipe_packet run"""

    def __init__(self, max_body_bytes: int = BODY_BYTES):
        self.cap = max_body_bytes
        self.table = [Entry() for _ in range(ENTRIES)]
        self.created = 0                 # ordernumber - 1
        self.old_slide = 0
        self.objects = []                # every object ever delivered, as dicts
        self.begin_run(1 << 30)

    def begin_run(self, out_arena: int):
        self.run_objects, self.nout, self.out_arena = [], 0, out_arena
        self.malformed = self.bad_segment = self.other_types = 0

    def handle(self, tid):
        for e in self.table:
            if e.order != 0 and e.tid == tid:
                return e
        return None

    def new_entry(self, tid, size, ct, cst, name):
        free = [e for e in self.table if e.order == 0]
        e = free[0] if free else min(self.table, key=lambda x: x.order)
        self.created += 1
        e.order, e.tid, e.bodySize, e.contentType, e.contentsubType = self.created, tid, size, ct, cst
        e.segmentSize = e.numofSegments = -1
        e.name = bytes(name)
        e.flags = TOO_LARGE if size > self.cap else 0
        e.body = bytearray(0 if e.flags else size)       # rule 4: bytes no segment wrote read 0
        # (the marks are those of the entry's previous tenant, as in the reference)
        return e

    def segment(self, e, data, n, size, last, g, cif):
        if e is None or e.flags & TOO_LARGE or size < 0:
            return
        if e.marked[n]:
            return
        if not last and e.segmentSize == -1:
            e.segmentSize = size
        if e.segmentSize == -1:
            return
        if n * e.segmentSize + size > e.bodySize:
            return
        e.body[n * e.segmentSize:n * e.segmentSize + size] = data[:size]
        e.marked[n] = True
        if last:
            e.numofSegments = n + 1
        if e.numofSegments != -1 and all(e.marked[:e.numofSegments]):
            self.complete(e, g, cif)

    def complete(self, e, g, cif):
        kind = SLIDE if e.contentType == 2 else EPG if e.contentType == 7 else FILE
        if kind == SLIDE:
            if self.old_slide:
                for i in range(e.numofSegments):
                    e.marked[i] = False
            self.old_slide = 1
        o = dict(group=g, cif=cif, offset=0, nbytes=0, transportId=e.tid, contentType=e.contentType, kind=kind,
                 contentsubType=e.contentsubType, flags=0, name_len=len(e.name), name=e.name[:NAME_BYTES], body=b"")
        if kind != EPG:
            off = (self.nout + 15) // 16 * 16
            if off + e.bodySize > self.out_arena:
                o["flags"] = OVERFLOW
            else:
                o.update(offset=off, nbytes=e.bodySize, body=bytes(e.body))
                self.nout = off + e.bodySize
        self.run_objects.append(o)
        self.objects.append(o)

    def group(self, g, rec, arena):
        """one dabgpu_datagroup record of a run and the run's stored bytes"""
        if rec["flags"] & (pp.ACCEPTED | pp.TID) != (pp.ACCEPTED | pp.TID):
            return
        gt, seg, last, tid = int(rec["groupType"]), int(rec["segmentNumber"]), bool(rec["flags"] & pp.LAST), int(rec["transportId"])
        hdr = gt == 3 and seg == 0
        if not hdr and gt != 4:
            self.other_types += 1                        # rule 6
            return
        dn, base = int(rec["data_nbytes"]), int(rec["offset"]) + int(rec["data_offset"])
        if (rec["offset"] < 0 or rec["data_offset"] < 0 or dn < 0 or rec["data_offset"] + dn > rec["nbytes"] or
                rec["offset"] + rec["nbytes"] > len(arena)):
            self.malformed += 1                          # a record that points outside its arena
            return
        d = bytes(arena[base:base + dn])
        B = lambda i: d[i] if 0 <= i < dn else 0         # rule 1
        size = (B(0) & 0x1F) << 8 | B(1)
        if dn < 2 or size + 2 > dn:
            self.malformed += 1
            return
        cif = int(rec["cif"])
        if not hdr:
            if seg >= 100:
                self.bad_segment += 1                    # rule 2
                return
            self.segment(self.handle(tid), d[2:], seg, size, last, g, cif)
            return
        hsize = (B(5) & 0x0F) << 9 | B(6) | B(7) >> 7    # the reference's formula: no shift of d[6]
        bsize = B(2) << 20 | B(3) << 12 | B(4) << 4 | B(5) >> 4
        if self.handle(tid) is not None:
            return
        S = lambda i: B(i + 2)
        ct, cst = (S(5) >> 1) & 0x3F, (S(5) & 1) << 8 | S(6)
        p, name = 7, bytearray()
        while p < hsize:
            pli, pid = S(p) >> 6, S(p) & 0x3F
            if pli == 0:
                p += 1
            elif pli == 1:
                p += 2
            elif pli == 2:
                p += 5
            else:
                if S(p + 1) & 0x80:
                    ln = (S(p + 1) & 0x7F) << 8 | S(p + 2)
                    p += 3
                else:
                    ln = S(p + 1) & 0x7F
                    p += 2
                if pid == 12:
                    name += bytes(S(p + i + 1) for i in range(ln - 1))
                p += ln
        e = self.new_entry(tid, bsize, ct, cst, name)
        if not last:
            self.segment(e, d[2 + hsize:], 0, size - hsize, False, g, cif)

    def feed(self, records, arena, out_arena=None):
        self.begin_run(arena_bytes(len(records), self.cap) if out_arena is None else out_arena)
        for g, rec in enumerate(records):
            self.group(g, rec, arena)
        return self.run_objects

    # ---- the records dabgpu_mot_groups writes ----------------------------------------------
    def object_records(self):
        out = np.zeros(len(self.run_objects), OBJECT_DTYPE)
        for r, o in zip(out, self.run_objects):
            for k in OBJECT_DTYPE.names:
                if k != "name":
                    r[k] = o[k]
            r["name"][:len(o["name"])] = np.frombuffer(o["name"], np.uint8)
        return out

    def run_record(self):
        r = np.zeros((), RUN_DTYPE)
        r["n_objects"], r["n_bytes"] = len(self.run_objects), self.nout
        r["malformed"], r["bad_segment"], r["other_types"] = self.malformed, self.bad_segment, self.other_types
        r["entries"] = sum(1 for e in self.table if e.order)
        return r

    def state(self):
        """(head record, entry records of the entries in use, their bodies): what the carried
        state holds that later groups can observe"""
        h = np.zeros((), HEAD_DTYPE)
        h["created"], h["old_slide"] = self.created, self.old_slide
        ent = np.zeros(ENTRIES, ENTRY_DTYPE)
        bodies = []
        for r, e in zip(ent, self.table):
            for i in range(128):                         # the marks outlive a tenant (newEntry leaves them)
                if e.marked[i]:
                    r["marked"][i >> 5] |= np.uint32(1 << (i & 31))
            if not e.order:
                bodies.append(b"")
                continue
            r["order"], r["transportId"], r["bodySize"] = e.order, e.tid, e.bodySize
            r["segmentSize"], r["numofSegments"] = e.segmentSize, e.numofSegments
            r["contentType"], r["contentsubType"], r["flags"], r["name_len"] = e.contentType, e.contentsubType, e.flags, len(e.name)
            nm = e.name[:NAME_BYTES]
            r["name"][:len(nm)] = np.frombuffer(nm, np.uint8)
            bodies.append(bytes(e.body))
        return h, ent, bodies


def parse_state(raw: np.ndarray, max_body_bytes: int = BODY_BYTES):
    """a slot's carried state as dabgpu_mot_groups leaves it -> (head, entries, bodies) as
    Assembler.state() gives them (fields of free entries other than the marks zeroed)"""
    raw = np.ascontiguousarray(raw, np.uint8)
    h = np.frombuffer(raw[:HEAD_DTYPE.itemsize].tobytes(), HEAD_DTYPE)[0]
    o = HEAD_DTYPE.itemsize
    ent = np.frombuffer(raw[o:o + ENTRIES * ENTRY_DTYPE.itemsize].tobytes(), ENTRY_DTYPE).copy()
    o += ENTRIES * ENTRY_DTYPE.itemsize
    cap, bodies = body_cap(max_body_bytes), []
    for i in range(ENTRIES):
        if ent[i]["order"] == 0:
            m = ent[i]["marked"].copy()
            ent[i] = np.zeros((), ENTRY_DTYPE)
            ent[i]["marked"] = m
            bodies.append(b"")
        elif ent[i]["flags"] & TOO_LARGE:
            bodies.append(b"")
        else:
            bodies.append(raw[o + i * cap:o + i * cap + int(ent[i]["bodySize"])].tobytes())
    return h, ent, bodies


# ---- writers ------------------------------------------------------------------------------
def header_core(body_size, params=b"", ct=2, cst=1, hsize=None):
    """the 7-byte MOT header core and its parameters; hsize: the header-size field.  Its
    default is twice the true size: process_mscGroup reads the field without the shift of its
    middle byte, so that value makes the reference walk exactly the parameters given here"""
    hs = 2 * (7 + len(params)) if hsize is None else hsize
    return bytes([(body_size >> 20) & 0xFF, (body_size >> 12) & 0xFF, (body_size >> 4) & 0xFF,
                  (body_size & 15) << 4 | (hs >> 9) & 15, (hs >> 1) & 0xFF, (hs & 1) << 7 | ct << 1 | cst >> 8,
                  cst & 0xFF]) + bytes(params)


def name_param(name: bytes, charset=0x40):
    """parameter 12 (ContentName): PLI 3, length, character-set byte, the name"""
    n = len(name) + 1
    ln = bytes([n]) if n < 128 else bytes([0x80 | n >> 8, n & 255])
    return bytes([0xC0 | 12]) + ln + bytes([charset]) + bytes(name)


def seg_data(payload: bytes, rep=0):
    """a segment: repetition count and size, then the bytes"""
    return bytes([rep << 5 | len(payload) >> 8, len(payload) & 255]) + bytes(payload)


def dg(gtype, tid, segno, last, data, crcf=1, tidf=1, good=True):
    return pp.group(data, crcf=crcf, seg=1, ua=1, gtype=gtype, last=last, segno=segno, tidf=tidf, tid=tid, good=good)


def header_group(tid, body_size, params=b"", ct=2, cst=1, last=1, extra=b"", hsize=None, **kw):
    """a group type 3, segment 0; extra: body bytes that follow the header in the same segment"""
    return dg(3, tid, 0, last, seg_data(header_core(body_size, params, ct, cst, hsize) + extra), **kw)


def body_groups(tid, body: bytes, seg_size, **kw):
    n = max(1, (len(body) + seg_size - 1) // seg_size)
    return [dg(4, tid, i, int(i == n - 1), seg_data(body[i * seg_size:(i + 1) * seg_size]), **kw) for i in range(n)]


def pack(groups, cifs=None):
    """group byte strings -> (dabgpu_datagroup records, arena) as dabgpu_pipe_packet lays them out"""
    rec = np.zeros(len(groups), pp.GROUP_DTYPE)
    arena = bytearray()
    for i, g in enumerate(groups):
        p = pp.parse_group(g)
        for k in pp.GROUP_DTYPE.names:
            if k in p:
                rec[i][k] = p[k]
        rec[i]["cif"] = i // 2 if cifs is None else cifs[i]
        rec[i]["offset"] = len(arena)
        arena += p["stored"]
    return rec, np.frombuffer(bytes(arena), np.uint8)


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def fixtures():
    """the group sequences of tests/golden/mot_kat.npz: every one keeps the reference inside
    its arrays (segment numbers < 100, bodies <= 32767 bytes, segmentSize + 2 <= data length,
    header size <= segment size, every completed body written in full)"""
    rng = np.random.default_rng(60)
    fx = []

    def add(name, groups):
        fx.append(dict(name=name, groups=[bytes(g) for g in groups]))

    b = _bytes(rng, 700)
    add("in_order", [header_group(0x0101, 700, name_param(b"slide1.jpg"))] + body_groups(0x0101, b, 256))
    # header and body in one segment; header size 0x109: bit 8 set, so the reference's formula
    # (d[6] unshifted) gives 0x84 | 1 = 133 where the field says 265
    b = _bytes(rng, 300)
    prm = name_param(b"combined.png") + b"\x00" * (0x109 - 7 - 15)
    core = header_core(300 + 132, prm, cst=3, hsize=0x109)
    hs_ref = (core[3] & 15) << 9 | core[4] | core[5] >> 7
    assert hs_ref == 133 and len(core) == 0x109
    add("combined", [dg(3, 0x0202, 0, 0, seg_data(core + b[:200])), dg(4, 0x0202, 1, 1, seg_data(b[200:]))] +
        [dg(4, 0x0202, 1, 1, seg_data(b[200:]))])
    b = _bytes(rng, 500)
    g = body_groups(0x0303, b, 200)
    add("last_first", [header_group(0x0303, 500), g[2], g[0], g[1], g[2]])
    b1, b2 = _bytes(rng, 450), _bytes(rng, 333)
    s1 = [header_group(0x0404, 450, name_param(b"first"))] + body_groups(0x0404, b1, 150)
    s2 = [header_group(0x0405, 333, name_param(b"second"), cst=1)] + body_groups(0x0405, b2, 111)
    add("repeats", s1 + s1 + s2 + s2 + s1)
    b1, b2 = _bytes(rng, 600), _bytes(rng, 610)
    g1, g2 = body_groups(0x0501, b1, 200), body_groups(0x0502, b2, 305)
    add("interleaved", [header_group(0x0501, 600), header_group(0x0502, 610), g1[0], g2[1], g1[2], g2[0], g1[1]])
    seq, bodies = [], [_bytes(rng, 40 + i) for i in range(17)]
    for i in range(17):
        seq.append(header_group(0x0600 + i, 40 + i, name_param(b"t%02d" % i), ct=2 if i % 3 else 5))
    # the first was evicted by the 17th: its segments are ignored.  The third completes first
    # (the first slide ever: its marks stay), so the second's marks are cleared when it completes
    for i in [2, 0, 1] + list(range(3, 17)):
        seq += body_groups(0x0600 + i, bodies[i], 32)
    seq.append(header_group(0x0600, 40, name_param(b"t00again")))     # evicts the second, whose entry is clean
    seq += body_groups(0x0600, bodies[0], 32) + body_groups(0x0601, bodies[1], 32)
    seq.append(header_group(0x0601, 41, name_param(b"t01again")))     # evicts the third: the new tenant inherits its marks
    seq += body_groups(0x0601, bodies[1], 32)
    add("evict", seq)
    b = _bytes(rng, 200)
    add("duplicate", [header_group(0x0707, 200, name_param(b"one")), header_group(0x0707, 100, name_param(b"two"), cst=2)] +
        body_groups(0x0707, b, 100))
    b = _bytes(rng, 300)
    g = body_groups(0x0808, b, 100)
    add("size_check", [header_group(0x0808, 300), g[0], dg(4, 0x0808, 2, 1, seg_data(b[200:] + b"\x55")), g[1], g[2]])
    b = _bytes(rng, 120)
    add("epg", [header_group(0x0909, 120, ct=7, cst=0)] + body_groups(0x0909, b, 60) + body_groups(0x0909, b, 60))
    b = _bytes(rng, 260)
    prm = b"\x05" + b"\x4a\x07" + name_param(b"dir_") + b"\x85\x01\x02\x03\x04" + name_param(b"file.html")
    add("file", [header_group(0x0A0A, 260, prm, ct=1, cst=2)] + body_groups(0x0A0A, b, 130))
    b = _bytes(rng, 90)
    add("other_types", [dg(6, 0x0B0B, 0, 0, seg_data(_bytes(rng, 30))), dg(5, 0x0B0B, 0, 1, seg_data(_bytes(rng, 20))),
                        header_group(0x0B0B, 90), dg(6, 0x0B0B, 1, 1, seg_data(_bytes(rng, 30))),
                        dg(3, 0x0B0B, 1, 1, seg_data(_bytes(rng, 12)))] + body_groups(0x0B0B, b, 45))
    b = _bytes(rng, 150)
    g = body_groups(0x0C0C, b, 50)
    add("filtered", [header_group(0x0C0C, 150, tidf=0), header_group(0x0C0C, 150, good=False), header_group(0x0C0C, 150),
                     dg(4, 0x0C0C, 0, 0, seg_data(b[:50]), good=False), dg(4, 0x0C0C, 0, 0, seg_data(b[:50]), tidf=0),
                     g[1], g[2], g[0]])
    return fx


def rule_cases():
    """cases outside the golden file: the rules of dabgpu_mot_groups where the reference is
    undefined or unbounded.  Each: name, groups, max_body_bytes"""
    rng = np.random.default_rng(61)
    out = []

    def add(name, groups, cap=BODY_BYTES):
        out.append(dict(name=name, groups=[bytes(g) for g in groups], cap=cap))

    b = _bytes(rng, 100)
    short = pp.group(b"\x00", crcf=1, seg=1, ua=1, gtype=4, last=1, segno=0, tid=0x1111)       # one data byte
    lying = dg(4, 0x1111, 0, 1, bytes([0, 101]) + b)                                          # claims 101, holds 100
    nohdr = dg(3, 0x1112, 0, 1, seg_data(b"\x00\x06\x40"))                                    # header fields past the end read 0
    add("rule1", [header_group(0x1111, 100), short, lying, nohdr] + body_groups(0x1111, b, 50))
    b = _bytes(rng, 101)
    add("rule2", [header_group(0x2222, 101), dg(4, 0x2222, 100, 1, seg_data(b[100:])), dg(4, 0x2222, 0x3FFF, 0, seg_data(b[:1])),
                  dg(4, 0x2222, 99, 1, seg_data(b[99:100]))] + [dg(4, 0x2222, i, 0, seg_data(b[i:i + 1])) for i in range(99)] +
        [dg(4, 0x2222, 99, 1, seg_data(b[99:100]))])
    b = _bytes(rng, 40000)
    add("rule3_big", [header_group(0x3333, 40000, name_param(b"big.jpg"))] + body_groups(0x3333, b, 4000))
    add("rule3_too_large", [header_group(0x3334, 5000), header_group(0x3335, 4096)] + body_groups(0x3334, b[:5000], 1000) +
        body_groups(0x3335, b[:4096], 1024) + [header_group(0x3334, 100)], cap=4096)
    b = _bytes(rng, 300)
    add("rule4", [header_group(0x4444, 300), dg(4, 0x4444, 0, 0, seg_data(b[:100])), dg(4, 0x4444, 2, 1, seg_data(b[200:])),
                  dg(4, 0x4444, 1, 0, seg_data(b[100:200])),
                  # a combined header whose header size exceeds its segment: the body part is dropped
                  dg(3, 0x4445, 0, 0, seg_data(header_core(50, b"", hsize=200))), dg(4, 0x4445, 0, 1, seg_data(b[:50])),
                  # unwritten bytes read 0: the only segment is the last and shorter than the body
                  header_group(0x4446, 80), dg(4, 0x4446, 0, 0, seg_data(b[:30])), dg(4, 0x4446, 1, 1, seg_data(b[:10]))])
    long_name = bytes(65 + i % 26 for i in range(300))
    add("rule5", [header_group(0x5555, 40, name_param(long_name) + name_param(b"tail"), ct=9)] + body_groups(0x5555, b[:40], 20))
    return out
