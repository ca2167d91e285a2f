"""TEST INFRASTRUCTURE for the FIC layer (dabgpu_fib_parse, csrc/k_fib.hip):
  - a FIB stream generator over the FIG builders of test_fib_cpu (fields drawn from small pools
    of SIds, SCIds and sub-channel ids so that entries collide), with FIBs that meet the overrun
    rule and FIBs of random bytes on request;
  - Processor: oracle_py.FibProcessor (fib-processor.cpp restated) fed zero-extended FIBs, which
    reports the FIBs that overran and packs database, events and table into the records of
    dabgpu.h (dabamd.FIC_*_DTYPE);
  - Host: the host class dabgpu::fib_processor behind tests/cpp/fic_wrap.cpp, with the same
    surface.
Both answer feed(fibs, ok, want, event_slots) with what one dabgpu_fib_parse call on one slot
returns: (db, events, table, run)."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_py as orc
from test_fib_cpu import _Bits, _fig, _random_fig, _random_fib   # noqa: F401  (the FIG builders, shared)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBCH_DABPLUS, SUBCH_MP2, SUBCH_PACKET, SUBCH_MOT, SUBCH_PAD = 1, 4, 8, 16, 32
ZEXT = 1280                                    # bits of a zero-extended FIB: past any read (a FIG 0/2 at byte 29)

LABELS = [l.ljust(16, b" ")[:16] for l in
          (b"Radio One", b"Radio One", b"Jazz & Blues", b"News 24", b"\x80\x8e\xa9 Caf\x82", b"Sport$ ^~`", b"Data Svc",
           b"Ensemble A", b"With\x00NUL")]


def dt():
    import dabamd
    return dabamd


def pools(rng, trial=0):
    sids = [int(x) for x in rng.integers(1, 0xFFFF, 6)] + [0xF0000000 + trial, 0x80001234]
    scids = [int(x) for x in rng.integers(0, 4096, 4)]
    subs = [int(x) for x in rng.integers(0, 64, 6)]
    return sids, scids, subs, LABELS


def fib_of(figs):
    """a FIB of the given FIGs (bytes), end marker and padding, CRC bytes zero"""
    body = b"".join(figs)
    assert len(body) <= 30
    return body + b"\xff" * (30 - len(body)) + b"\x00\x00"


# the two cases the overrun rule is stated on, with the FIBs they count (1 each): a FIG at byte 29
# with length 31 (FIG 0/1 through the CRC bytes), and a FIG 0/2 with 15 components at the end of the
# data field
STATED_OVERRUNS = [
    (bytes([0x00] * 29) + bytes([0x1F, 0x01, 0xA5]), 1),
    (bytes([0x00] * 23) + bytes([0x1F, 0x02, 0x12, 0x34, 0x0F, 0x3F, 0x14]) + bytes([0x2A, 0x80]), 1),
]


def overrunning_fib(rng, pl):
    """a FIB whose last FIG starts near the end of the data field and claims more than is left"""
    body = b""
    for _ in range(6):
        f = _random_fig(rng, pl)
        if len(body) + len(f) <= 26:
            body += f
    k = int(rng.integers(0, 5))
    sid = int(rng.choice(pl[0]))
    if k == 0:      # FIG 0/2 with a long component list
        tail = bytes([0x1F, 0x02]) + (sid & 0xFFFF).to_bytes(2, "big") + bytes([int(rng.integers(8, 16))])
    elif k == 1:    # FIG 1/1 whose label runs on
        tail = bytes([0x20 | 21, 0x01]) + (sid & 0xFFFF).to_bytes(2, "big")
    elif k == 2:    # FIG 0/17, 0/1 or 0/3 entries up to the claimed length
        tail = bytes([0x1F, int(rng.choice([17, 1, 3, 14, 16]))])
    elif k == 3:    # FIG 1/0
        tail = bytes([0x20 | 21, 0x00]) + (sid & 0xFFFF).to_bytes(2, "big")
    else:           # FIG 2/5
        tail = bytes([0x40 | 23, 0x05]) + (sid & 0xFFFFFFFF).to_bytes(4, "big")
    fill = bytes(rng.integers(0, 256, 30, dtype=np.uint8))
    pad = b"\x00" * int(rng.integers(0, max(1, 30 - len(body) - len(tail)) + 1))    # FIG 0/0 headers of length 0
    body = (body + pad + tail + fill)[:30] if len(body) + len(pad) + len(tail) <= 30 else (body + tail + fill)[:30]
    return body + bytes(rng.integers(0, 256, 2, dtype=np.uint8))


def random_fibs(rng, n, pl, overrun=0.0, noise=0.0):
    """[n, 32] uint8: well-formed FIBs, a share `overrun` of overrunning ones and a share `noise`
    of random bytes"""
    out = np.zeros((n, 32), np.uint8)
    for i in range(n):
        r = rng.random()
        if r < overrun:
            f = overrunning_fib(rng, pl)
        elif r < overrun + noise:
            f = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        else:
            f = _random_fib(rng, pl)
        out[i] = np.frombuffer(f, np.uint8)
    return out


def fig_counts(fib):
    """FIG headers process_FIB meets, by type (7: the end marker)"""
    c = np.zeros(8, np.int32)
    p = 0
    while p < 30:
        t = fib[p] >> 5
        c[t] += 1
        if t == 7:
            break
        p += (fib[p] & 31) + 1
    return c


class _Feed:
    """feed(): one dabgpu_fib_parse call on this database"""

    def feed(self, fibs, ok, want=0, event_slots=65):
        d = dt()
        run = np.zeros((), d.FIC_RUN_DTYPE)
        for i, (f, k) in enumerate(zip(fibs, ok)):
            if not k:
                run["skipped"] += 1
                continue
            f = bytes(bytearray(f))
            run["parsed"] += 1
            run["figs"] += fig_counts(f)
            run["overrun"] += int(self.fib(f, i))
        evs = self.take_events()
        run["n_events"] = len(evs)
        ev = np.zeros(event_slots, d.FIC_EVENT_DTYPE)
        m = min(len(evs), event_slots)
        if m:
            ev[:m] = evs[:m]
        t = self.table(want)
        run["table_changed"] = int(t.tobytes() != self.last_table.tobytes())
        self.last_table = t
        return self.db(), ev, t, run


class Processor(orc.FibProcessor, _Feed):
    """oracle_py.FibProcessor with the two rules of dabgpu_fib_parse (overrun: zero-extended
    FIBs; a bind with the component table full writes nothing) and the records of dabgpu.h"""

    def __init__(self):
        self.records = []
        self._L = ZEXT
        self.over = False
        self._fibno = 0
        self._svc = None
        self._raw = None
        super().__init__()
        self.last_table = np.zeros((), dt().FIC_TABLE_DTYPE)

    # ---- hooks into the restatement ----
    def _bits(self, d, off, n):
        if self._L - len(d) + off + n > 256:
            self.over = True
        return orc.FibProcessor._bits(d, off, n)

    def _find_service(self, sid):
        s = super()._find_service(sid)
        self._svc, self._svc_named = s, s["hasName"]
        return s

    def _label(self, d, off, charset):
        self._raw = (bytes(self._bits(d, off + 8 * i, 8) for i in range(16)), charset)
        return super()._label(d, off, charset)

    def _fig0_1(self, d, used):
        sid = self._bits(d, used * 8, 6)
        r = super()._fig0_1(d, used)
        self.ficList[sid]["inUse"] = True
        return r

    def _bind(self, tmid, sid, compnr, fields):
        if all(c["inUse"] for c in self.components):                  # rule 2 (the restatement would write slot -1)
            self._find_service(sid)                                    # (which may take a service entry first)
            return
        return super()._bind(tmid, sid, compnr, fields)

    def _named(self, suffix):
        s = self._svc
        if s is not None and not self._svc_named and s["hasName"]:
            s["raw"], s["charset"], s["suffix"] = self._raw[0], self._raw[1], suffix

    def _fig1(self, d):
        n0, self._svc = len(self.events), None
        ext = orc.FibProcessor._bits(d, 13, 3)
        if ext == 0:                                                   # (:877-881: the label is read whatever OE says)
            self._label(d, 32, orc.FibProcessor._bits(d, 8, 4))
        super()._fig1(d)
        self._named(ext == 5)
        for e in self.events[n0:]:
            if e[0] == "E":
                self.ens = (e[1], self._raw[0], self._raw[1])
                self.records.append((1, self._fibno, e[1], self._raw[1], self._raw[0]))
            else:
                self.records.append((2, self._fibno, self.services.index(self._svc), self._raw[1], self._raw[0]))

    def _fig2(self, d):
        self._svc = None
        super()._fig2(d)
        self._named(False)

    def clearEnsemble(self):
        super().clearEnsemble()
        for f in self.ficList:
            f["inUse"] = False
        for s in self.services:
            s.update(raw=bytes(16), charset=0, suffix=False)
        self.ens = None

    # ---- the operator's surface ----
    def fib(self, fib, index=0):
        """one FIB of 32 bytes; returns whether it overran"""
        bits = [(fib[i >> 3] >> (7 - (i & 7))) & 1 for i in range(256)] + [0] * (ZEXT - 256)
        self.over, self._fibno = False, index
        self.process_FIB(bits)
        return self.over

    def take_events(self):
        d = dt()
        ev = np.zeros(len(self.records), d.FIC_EVENT_DTYPE)
        for e, (kind, fib, ident, cs, raw) in zip(ev, self.records):
            e["kind"], e["fib"], e["id"], e["charset"] = kind, fib, ident, cs
            e["label"] = np.frombuffer(raw, np.uint8)
        self.records = []
        self.events.clear()
        return ev

    def table(self, want=0):
        """fib_processor::subchannels (host/fib_processor.cpp) as a dabgpu_fic_table"""
        t = np.zeros((), dt().FIC_TABLE_DTYPE)
        n = 0
        for sid, f in enumerate(self.ficList):
            if not f["inUse"]:
                continue
            fl = 0
            for c in self.components:
                if c["inUse"] and c["TMid"] == 0 and c["subchannelId"] == sid:
                    if c["ASCTy"] == 0o77:
                        fl |= SUBCH_DABPLUS
                    elif c["ASCTy"] == 0 and want & SUBCH_MP2:
                        fl |= SUBCH_MP2
            for c in self.components:
                if (c["inUse"] and c["TMid"] == 3 and c["DSCTy"] != 0 and c["subchannelId"] == sid
                        and not (c["DSCTy"] == 5 and c["DGflag"])):
                    if want & SUBCH_PACKET:
                        fl |= SUBCH_PACKET
                    if want & SUBCH_MOT and c["DSCTy"] == 60:
                        fl |= SUBCH_PACKET | SUBCH_MOT
            if fl & SUBCH_DABPLUS and want & SUBCH_PAD:
                fl |= SUBCH_PAD
            if fl & SUBCH_DABPLUS:
                fl &= ~SUBCH_MP2
            if fl & (SUBCH_DABPLUS | SUBCH_MP2):
                fl &= ~(SUBCH_PACKET | SUBCH_MOT)
            t["sub"][n] = (f["StartAddr"], f["Length"], f["BitRate"], f["protLevel"], f["uepFlag"], fl)
            t["ids"][n] = sid
            n += 1
        t["n"] = n
        return t

    def db(self):
        r = np.zeros((), dt().FIC_DB_DTYPE)
        for i, f in enumerate(self.ficList):
            x = r["sub"][i]
            for k in ("SubChId", "StartAddr", "Length", "uepFlag", "protLevel", "BitRate", "FEC_scheme"):
                x[k] = f[k]
            x["inUse"] = f["inUse"]
        for i, c in enumerate(self.components):
            x = r["components"][i]
            for k in ("inUse", "TMid", "componentNr", "ASCTy", "PS_flag", "subchannelId", "SCId", "CAflag", "DGflag", "DSCTy",
                      "packetAddress"):
                x[k] = c[k]
            x["service"] = max(c["service"], 0)
        for i, s in enumerate(self.services):
            x = r["services"][i]
            x["serviceId"] = s["serviceId"] if s["inUse"] else 0
            for k in ("inUse", "hasName", "hasLanguage", "charset", "language", "programType"):
                x[k] = s[k]
            x["data_suffix"] = s["suffix"]
            x["label"] = np.frombuffer(s["raw"], np.uint8)
        if self.ens:
            r["EId"], r["charset"], r["named"] = self.ens[0], self.ens[2], 1
            r["label"] = np.frombuffer(self.ens[1], np.uint8)
        else:
            r["named"] = 0 if self.firstTime else 1     # (an ensemble label with OE never arrives here: firstTime stays)
        r["table"] = self.last_table
        return r

    def lookup(self, label):
        """(kindofService, dataforAudioService or None, dataforDataService or None)"""
        return self.kindofService(label), self.dataforAudioService(label), self.dataforDataService(label)


_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        subprocess.run(["make", "-s", "-f", os.path.join(ROOT, "tests", "cpp", "Makefile.fic"),
                        os.path.join(ROOT, "tests", "cpp", "build", "libficwrap.so")], check=True, cwd=ROOT, timeout=300)
        L = C.CDLL(os.path.join(ROOT, "tests", "cpp", "build", "libficwrap.so"))
        vp, i32 = C.c_void_p, C.c_int
        for name, (args, res) in {"fw_new": ([], vp), "fw_free": ([vp], None), "fw_fib": ([vp, vp, i32], i32),
                                  "fw_clear": ([vp], None), "fw_export": ([vp, vp], None), "fw_import": ([vp, vp], None),
                                  "fw_events": ([vp, vp, i32], i32), "fw_table": ([vp, i32, vp], None),
                                  "fw_labels": ([vp, vp, i32], i32), "fw_ensemble": ([vp, vp, i32], i32),
                                  "fw_lookup": ([vp, C.c_char_p, vp], None)}.items():
            f = getattr(L, name)
            f.argtypes, f.restype = args, res
        _HOST = L
    return _HOST


class Host(_Feed):
    """dabgpu::fib_processor (host/fib_processor.cpp) behind tests/cpp/fic_wrap.cpp"""

    def __init__(self):
        self.L = host_lib()
        self.h = self.L.fw_new()
        self.last_table = np.zeros((), dt().FIC_TABLE_DTYPE)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.fw_free(self.h)
            self.h = None

    def fib(self, fib, index=0):
        b = np.frombuffer(bytes(fib), np.uint8).copy()
        return bool(self.L.fw_fib(self.h, b.ctypes.data, index))

    def clearEnsemble(self):
        self.L.fw_clear(self.h)

    def take_events(self):
        ev = np.zeros(4096, dt().FIC_EVENT_DTYPE)
        n = self.L.fw_events(self.h, ev.ctypes.data, len(ev))
        assert n <= len(ev)
        return ev[:n].copy()

    def table(self, want=0):
        t = np.zeros(1, dt().FIC_TABLE_DTYPE)
        self.L.fw_table(self.h, want, t.ctypes.data)
        return t[0].copy()

    def db(self):
        r = np.zeros(1, dt().FIC_DB_DTYPE)
        r[0]["table"] = self.last_table
        self.L.fw_export(self.h, r.ctypes.data)
        return r[0].copy()

    def load(self, db):
        r = np.zeros(1, dt().FIC_DB_DTYPE)
        r[0] = db
        self.L.fw_import(self.h, r.ctypes.data)
        self.last_table = r[0]["table"].copy()

    def labels(self):
        buf = C.create_string_buffer(8192)
        n = self.L.fw_labels(self.h, buf, len(buf))
        return [x.decode("utf-8", "replace") for x in buf.raw.split(b"\0")[:n]]

    def ensemble(self):
        buf = C.create_string_buffer(256)
        n = self.L.fw_ensemble(self.h, buf, len(buf))
        return buf.raw[:n].decode("utf-8", "replace")

    def lookup(self, label):
        out = np.zeros(22, np.int32)
        self.L.fw_lookup(self.h, label.encode("utf-8"), out.ctypes.data)
        return (int(out[0]), [int(x) for x in out[2:11]] if out[1] else None, [int(x) for x in out[12:22]] if out[11] else None)


# ---- the fixtures of tests/golden/fib_kat.npz (tests/golden/make_fib_golden.py) -------------
def fig0_1(entries):
    """entries: (subch, start, ("s", table index)) or (subch, start, ("l", option, level - 1, size))"""
    b = _Bits().put(0, 3).put(1, 5)
    for sub, start, form in entries:
        b.put(sub, 6).put(start, 10)
        if form[0] == "s":
            b.put(0, 2).put(form[1], 6)
        else:
            b.put(1, 1).put(form[1], 3).put(form[2], 2).put(form[3], 10)
    return _fig(0, b.bytes())


def fig0_2(sid, comps, pd=0):
    """comps: ("a", ASCTy, subch) or ("p", SCId)"""
    b = _Bits().put(0, 2).put(pd, 1).put(2, 5).put(sid, 32 if pd else 16).put(0, 4).put(len(comps), 4)
    for c in comps:
        if c[0] == "a":
            b.put(0, 2).put(c[1], 6).put(c[2], 6).put(1, 1).put(0, 1)
        else:
            b.put(3, 2).put(c[1], 12).put(1, 1).put(0, 1)
    return _fig(0, b.bytes())


def fig0_3(entries):
    """entries: (SCId, DG flag, DSCTy, subch, packet address)"""
    b = _Bits().put(0, 3).put(3, 5)
    for scid, dg, ty, sub, addr in entries:
        b.put(scid, 12).put(0, 4).put(dg, 1).put(0, 1).put(ty, 6).put(sub, 6).put(addr, 10).put(0, 16)
    return _fig(0, b.bytes())


def fig0_14(pairs):
    return _fig(0, bytes([14]) + bytes((i << 2) | f for i, f in pairs))


def fig0_17(entries):
    """entries: (SId, language or None, programme type, cc flag)"""
    b = _Bits().put(0, 3).put(17, 5)
    for sid, lang, pty, cc in entries:
        b.put(sid, 16).put(0, 2).put(0 if lang is None else 1, 1).put(cc, 1).put(0, 4)
        if lang is not None:
            b.put(lang, 8)
        b.put(0, 3).put(pty, 5)
        if cc:
            b.put(0, 8)
    return _fig(0, b.bytes())


def fig1(ext, sid, label, cs=0, oe=0):
    label = label.ljust(16, b" ")[:16]
    return _fig(1, bytes([(cs << 4) | (oe << 3) | ext]) + sid.to_bytes(4 if ext == 5 else 2, "big") + label + b"\xff\x00")


def fig2_5(sid, label, cs=0):
    return _fig(2, bytes([(cs << 4) | 5]) + sid.to_bytes(4, "big") + label.ljust(16, b" ")[:16] + b"\x00\x00")


def fixtures():
    """[(name, fibs [n, 32] uint8)]: what fib_kat.npz pins.  No FIB may meet the overrun rule
    (asserted by the generator, nothing is filtered)."""
    from dabamd.synth import Ensemble
    tx = [(0, 24, 32, 0o103, 0, 1, 0), (24, 84, 96, 2, 1, 0, 0), (120, 48, 64, 0o103, 0, 0, 5)]
    synth = np.packbits(Ensemble(2, subch=tx, figs=True).generate(5)["fic"].reshape(24, 256), axis=-1)
    f = lambda *figs: np.frombuffer(fib_of(list(figs)), np.uint8)
    D1, D2 = 0xE0002001, 0xE0002002
    fx = [("synth_figs", synth),
          ("fig0_1_forms", np.stack([
              f(fig0_1([(1, 0, ("s", 20)), (2, 100, ("l", 0, 2, 48)), (3, 200, ("l", 1, 0, 27)), (4, 300, ("l", 2, 1, 10))]),
                fig0_2(0x1001, [("a", 63, 1), ("a", 0, 2)])),
              f(fig0_2(0x1002, [("a", 63, 3)]), fig0_2(0x1003, [("a", 0, 4)]), fig0_17([(0x1001, 9, 5, 0), (0x1003, 3, 1, 1)])),
              f(fig1(1, 0x1001, b"First")), f(fig1(1, 0x1002, b"Second")), f(fig1(1, 0x1003, b"Third")),
              f(fig1(0, 0xE001, b"Ensemble one")), f(fig1(0, 0xE002, b"Ensemble two"))])),
          ("packet_fig0_3", np.stack([
              f(fig0_1([(5, 10, ("s", 3)), (6, 60, ("s", 30))]), fig0_2(D1, [("p", 100), ("p", 101)], pd=1), fig0_3([(100, 0, 60, 5, 17)])),
              f(fig0_3([(101, 1, 5, 6, 18), (999, 0, 1, 7, 3)]), fig0_2(D2, [("p", 102)], pd=1)),
              f(fig1(5, D1, b"Data one")), f(fig1(5, D2, b"Data two")), f(fig0_3([(102, 0, 59, 6, 5)]))])),
          ("fig0_14", np.stack([
              f(fig0_1([(0, 10, ("s", 3)), (6, 60, ("s", 30))]), fig0_2(D1, [("p", 100), ("p", 101)], pd=1), fig0_3([(100, 0, 60, 0, 17)])),
              f(fig0_3([(101, 0, 1, 6, 18)]), fig0_14([(6, 1), (0, 2), (9, 3)])), f(fig1(5, D1, b"FEC data"))])),
          ("fig0_17", np.stack([
              f(fig0_2(0x3001, [("a", 63, 1)]), fig0_2(0x3002, [("a", 63, 2)]), fig0_1([(1, 0, ("s", 0)), (2, 50, ("s", 5))])),
              f(fig0_17([(0x3001, 15, 10, 0), (0x3002, 8, 31, 1), (0x3003, None, 4, 0), (0x3001, None, 11, 1)])),
              f(fig1(1, 0x3001, b"Lang one")), f(fig1(1, 0x3002, b"Lang two")), f(fig0_17([(0x3002, 99, 2, 0)]))])),
          ("charsets_0_15", np.stack([
              f(fig0_2(0x4001, [("a", 63, 1)]), fig0_2(0x4002, [("a", 0, 2)]), fig0_17([(0x4001, 1, 1, 0), (0x4002, 2, 2, 0)])),
              f(fig1(0, 0xE00F, b"Ignored (OE)", cs=0, oe=1)), f(fig1(0, 0xE00F, "Ünïcode Ens".encode("utf-8"), cs=15)),
              f(fig1(1, 0x4001, b"\x80\x8e\xa9 Caf\x82 $^~`", cs=0)), f(fig1(1, 0x4002, "Zürich ☺".encode("utf-8"), cs=15)),
              f(fig1(1, 0x4001, b"Second name", cs=15)), f(fig1(1, 0x4003, b"With\x00NUL", cs=0))])),
          ("fig1_5_fig2_5", np.stack([
              f(fig0_1([(7, 0, ("s", 9))]), fig0_2(D1, [("p", 7)], pd=1), fig0_3([(7, 0, 60, 7, 1)])),
              f(fig0_2(D2, [("p", 8)], pd=1), fig0_3([(8, 0, 24, 7, 2)])),
              f(fig1(5, D1, b"One five")), f(fig2_5(D2, b"Two five")), f(fig2_5(D1, b"Too late")), f(fig1(5, D2, b"Too late"))]))]
    full = [f(fig0_17([(0x5000 + 7 * k + j, j, (k + j) % 32, 0) for j in range(5)])) for k in range(13)]
    full += [f(fig1(1, 0x5000, b"Entry zero")), f(fig1(1, 0x7777, b"Sixty-fifth")), f(fig0_17([(0x7778, 42, 17, 0)])),
             f(fig0_1([(9, 0, ("s", 1))]), fig0_2(0x5000, [("a", 63, 9)])), f(fig1(1, 0x5000 + 7 * 12 + 3, b"Last entry"))]
    fx.append(("full_service_table", np.stack(full)))
    return fx


def load_kat():
    """tests/golden/fib_kat.npz -> [dict(name, fibs, signals [(fib, kind, id, charset, bytes)],
    named [(slot, charset, first-piece bytes, n_pieces, kind, audio[9], data[10], defined[19])])]"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "fib_kat.npz"))
    out = []
    for i, name in enumerate(z["names"]):
        sb, nb = bytes(z["sig_bytes_%d" % i]), bytes(z["named_bytes_%d" % i])
        sigs, named, p = [], [], 0
        for fib, kind, ident, cs, n in z["sig_%d" % i].tolist():
            sigs.append((fib, kind, ident, cs, sb[p:p + n]))
            p += n
        p = 0
        for row, ok in zip(z["named_%d" % i].tolist(), z["defined_%d" % i].tolist()):
            named.append((row[0], row[1], nb[p:p + row[2]], row[3], row[4], row[5:14], row[14:24], ok))
            p += row[2]
        out.append(dict(name=str(name), fibs=z["fibs_%d" % i], signals=sigs, named=named))
    return out
