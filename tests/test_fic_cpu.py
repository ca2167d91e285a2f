"""The FIC layer's host end (host/fib_processor.cpp: the overrun rule, export_db / import_db) and
its records, without a GPU: the host class and tests/fib_py.Processor (oracle_py.FibProcessor with
the two rules of dabgpu_fib_parse) against the reference's own records (tests/golden/fib_kat.npz),
the host class against that restatement record for record on random FIBs, the round trip through
the public record, and the sizes and symbols the bindings rely on."""
import ctypes as C
import os
import re

import numpy as np

import fib_py as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, what):
    assert a.tobytes() == b.tobytes(), (what, [(n, a[n], b[n]) for n in a.dtype.names if a[n].tobytes() != b[n].tobytes()])


def test_host_class_equals_restatement_after_every_fib():
    """a few hundred random FIBs -- well-formed ones, FIBs whose last FIG runs past the data
    field and the CRC (the overrun rule) and FIBs of random bytes --, one FIB per call: the
    database, the events, the table and the run record (the overrun count with them) are equal
    after every FIB; clearEnsemble in between"""
    rng = np.random.default_rng(77)
    overran = 0
    for trial in range(3):
        pl = F.pools(rng, trial)
        fibs = F.random_fibs(rng, 160, pl, overrun=0.2, noise=0.1)
        h, p = F.Host(), F.Processor()
        for i, f in enumerate(fibs):
            if rng.integers(0, 60) == 0:
                h.clearEnsemble()
                p.clearEnsemble()
            want = int(rng.choice([0, 4, 8, 16, 32, 60]))
            a, b = h.feed([f], [1], want), p.feed([f], [1], want)
            for x, y, n in zip(a, b, ("db", "events", "table", "run")):
                _same(x, y, (trial, i, n, bytes(f).hex()))
            overran += int(a[3]["overrun"])
    assert overran > 20            # the rule was exercised


def test_overrun_rule_on_the_two_stated_cases():
    """a FIG at byte 29 with length 31, and a FIG 0/2 with 15 components at the end of the data
    field: both count as overrun, the reads past bit 255 are zeros (the CRC bytes before it are
    read as delivered)"""
    for fib, n_over in F.STATED_OVERRUNS:
        h, p = F.Host(), F.Processor()
        a, b = h.feed([np.frombuffer(fib, np.uint8)], [1]), p.feed([np.frombuffer(fib, np.uint8)], [1])
        for x, y in zip(a, b):
            _same(x, y, fib.hex())
        assert a[3]["overrun"] == n_over
    # 29 empty FIG 0 headers, then at byte 29 a FIG 0 of length 31 whose extension (1) is the first
    # CRC byte: ten FIG 0/1 entries, the first from the second CRC byte, the others zeros
    fib = F.STATED_OVERRUNS[0][0]
    db, ev, t, run = F.Host().feed([np.frombuffer(fib, np.uint8)], [1])
    assert run["figs"][0] == 30 and t["n"] == 2 and list(t["ids"][:2]) == [0, 41]
    # FIG 0/2 at byte 23: SId 0x1234, 15 components; the first lies in bytes 28..29, the second is the CRC
    fib = F.STATED_OVERRUNS[1][0]
    h, p = F.Host(), F.Processor()
    a, b = h.feed([np.frombuffer(fib, np.uint8)], [1]), p.feed([np.frombuffer(fib, np.uint8)], [1])
    for x, y in zip(a, b):
        _same(x, y, "fig 0/2")
    db, run = a[0], a[3]
    assert run["overrun"] == 1
    c = db["components"]
    assert c["inUse"].sum() == 15 and list(c["componentNr"][:15]) == list(range(15))
    assert (c["ASCTy"][0], c["subchannelId"][0]) == (0x3F, 5)                  # 0x3F14: TMid 0, ASCTy 63, SubChId 5
    assert (c["ASCTy"][1], c["subchannelId"][1]) == (42, 32)                   # bytes 30..31 = 0x2A80 as delivered
    assert c["TMid"][2:15].tolist() == [0] * 13 and not c["ASCTy"][2:15].any()  # past bit 255: zeros


def test_well_formed_fibs_never_overrun_and_lookups_match():
    """behaviour on well-formed FIBs is unchanged: none overruns, and labels, ensemble name and
    the three lookups equal the restatement's"""
    rng = np.random.default_rng(5)
    pl = F.pools(rng)
    fibs = F.random_fibs(rng, 300, pl)
    h, p = F.Host(), F.Processor()
    a, b = h.feed(fibs, np.ones(len(fibs), np.uint8), 60), p.feed(fibs, np.ones(len(fibs), np.uint8), 60)
    assert a[3]["overrun"] == 0 and a[3]["parsed"] == 300
    for x, y, n in zip(a, b, ("db", "events", "table", "run")):
        _same(x, y, n)
    assert h.labels() == p.labels() and len(h.labels()) > 3
    for q in sorted(set(h.labels())) + ["nothing"]:
        assert h.lookup(q) == p.lookup(q), q


def test_export_import_round_trip_reproduces_every_lookup():
    """export_db then import_db into a new fib_processor: the same record again, the same labels,
    ensemble name and lookup answers; and the imported one goes on parsing like the original"""
    rng = np.random.default_rng(6)
    pl = F.pools(rng)
    fibs = F.random_fibs(rng, 260, pl)
    ok = np.ones(len(fibs), np.uint8)
    h = F.Host()
    h.feed(fibs[:200], ok[:200], 60)
    db = h.db()
    g = F.Host()
    g.load(db)
    _same(g.db(), db, "round trip")
    assert g.labels() == h.labels() and g.ensemble() == h.ensemble() and len(g.labels()) > 3
    assert any(l.endswith(" (data)") for l in g.labels())
    for q in sorted(set(h.labels())) + ["nothing"]:
        assert g.lookup(q) == h.lookup(q), q
    a, b = h.feed(fibs[200:], ok[200:], 60), g.feed(fibs[200:], ok[200:], 60)
    for x, y, n in zip(a, b, ("db", "events", "table", "run")):
        _same(x, y, n)
    z = F.Host()                                                   # a zeroed record is a new fib_processor
    _same(z.db(), np.zeros((), F.dt().FIC_DB_DTYPE), "new")
    z.load(np.zeros((), F.dt().FIC_DB_DTYPE))
    a, b = z.feed(fibs, ok, 60), F.Host().feed(fibs, ok, 60)
    _same(a[0], b[0], "from zero")


def test_clear_keeps_language_and_programme_type():
    sid = 0x4321
    f17 = F._fig(0, F._Bits().put(0, 3).put(17, 5).put(sid, 16).put(0, 2).put(1, 1).put(0, 1).put(0, 4).put(9, 8).put(0, 3)
                 .put(21, 5).bytes())
    f11 = F._fig(1, bytes([0x01]) + sid.to_bytes(2, "big") + b"Radio One       " + b"\xff\x00")
    fib = np.frombuffer(F.fib_of([f17, f11]), np.uint8)
    for cls in (F.Host, F.Processor):
        h = cls()
        db = h.feed([fib], [1])[0]
        s = db["services"][0]
        assert (s["inUse"], s["hasName"], s["hasLanguage"], s["language"], s["programType"]) == (1, 1, 1, 9, 21)
        h.clearEnsemble()
        s = h.db()["services"][0]
        assert (s["inUse"], s["serviceId"], s["hasLanguage"], s["language"], s["programType"]) == (0, 0, 1, 9, 21)
        assert not s["label"].any()


def test_record_sizes_exports_and_header():
    import dabamd
    L = dabamd.lib()
    assert L.dabgpu_abi_version() == 7
    assert dabamd.fic_db_bytes() == dabamd.FIC_DB_DTYPE.itemsize == 5232
    assert (dabamd.FIC_TABLE_DTYPE.itemsize, dabamd.FIC_EVENT_DTYPE.itemsize, dabamd.FIC_RUN_DTYPE.itemsize) == (848, 32, 64)
    assert dabamd.FIC_DB_DTYPE.fields["table"][1] == 5232 - 848 and dabamd.FIC_TABLE_DTYPE.fields["sub"][1] == 16
    assert dabamd._SUBCH_DTYPE.itemsize == C.sizeof(dabamd.Subch)
    for name in ("dabgpu_fic_db_bytes", "dabgpu_fib_parse", "dabgpu_fic_clear", "dabgpu_pipe_fic_caps", "dabgpu_pipe_fic",
                 "dabgpu_pipe_fic_db", "dabgpu_pipe_fic_clear"):
        assert hasattr(L, name), name
    hdr = open(os.path.join(ROOT, "include", "dabgpu.h")).read()
    assert "#define DABGPU_ABI_VERSION 7" in hdr and "#define DABGPU_FIC_EVENT_SLOTS 65" in hdr
    for word in ("dabgpu_fic_db", "dabgpu_fic_event", "dabgpu_fic_table", "dabgpu_fic_run", "a read at or past bit 256",
                 "component table full writes nothing"):
        assert re.search(re.escape(word), hdr), word
    # the arguments the operator refuses before it touches the device
    assert L.dabgpu_fib_parse(None, None, 1, None, 0, None, 0, 0, None, 0, None, None) == -1


def test_host_class_and_restatement_equal_the_reference():
    """tests/golden/fib_kat.npz, written by the reference's own fib-processor.cpp compiled where it
    lies under the address and undefined-behaviour sanitizers (tests/golden/make_fib_golden.py):
    per fixture the signals in order (kind, EId, FIB, label bytes up to the first NUL, charset),
    the named services' slots and labels, and kindofService / dataforAudioService /
    dataforDataService for every label, on the fields the reference defines.  No fixture FIB
    meets the overrun rule."""
    kat = F.load_kat()
    assert [k["name"] for k in kat] == [n for n, _ in F.fixtures()]
    for k, (_, fibs) in zip(kat, F.fixtures()):
        assert np.array_equal(k["fibs"], fibs), k["name"]            # the file pins these fixtures
        for cls in (F.Host, F.Processor):
            what = (k["name"], cls.__name__)
            h = cls()
            db, ev, table, run = h.feed(k["fibs"], np.ones(len(k["fibs"]), np.uint8), 60)
            assert run["overrun"] == 0 and run["n_events"] == len(k["signals"]), what
            for e, (fib, kind, ident, cs, raw) in zip(ev, k["signals"]):
                assert (e["fib"], e["kind"], e["charset"]) == (fib, kind, cs), what
                assert bytes(e["label"]).split(b"\0")[0] == raw, what
                if kind == 1:
                    assert e["id"] == ident, what
                else:                                                  # addtoEnsemble carries the label alone
                    assert bytes(db["services"][e["id"]]["label"]).split(b"\0")[0] == raw, what
            sv = db["services"]
            assert [i for i in range(64) if sv[i]["inUse"] and sv[i]["hasName"]] == [n[0] for n in k["named"]], what
            labels = h.labels()
            assert len(labels) == len(k["named"]), what
            for text, (slot, cs, raw, npieces, kind, audio, data, ok) in zip(labels, k["named"]):
                s = sv[slot]
                assert bytes(s["label"]).split(b"\0")[0] == raw and s["charset"] == cs and s["data_suffix"] == npieces - 1, what
                got = h.lookup(text)
                assert got[0] == kind, (what, text)
                for ans, ref, mask in ((got[1], audio, ok[:9]), (got[2], data, ok[9:])):
                    if ans is None:                                    # the reference returned without filling anything in
                        assert all(v in (-7777, 0xEE) for v in ref), (what, text, ref)
                    else:
                        assert [a for a, m in zip(ans, mask) if m] == [r for r, m in zip(ref, mask) if m], (what, text, ans, ref)
                        assert sum(mask) >= 7, (what, text)
