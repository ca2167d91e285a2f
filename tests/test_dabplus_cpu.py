"""The crafted DAB+ superframes of tests/dabplus_py.py on the CPU: each case gives the record
it is named for, and the oracle's restatement (orc.MP4, orc.rs_dec, orc_firecode_check) is
pinned to the reference's own classes (oracle/_ref: reedSolomon, firecode_checker and
ref_mp4_add around them) on exactly the bytes that tests/test_gpu_dabplus_edges.py feeds the
GPU layer.

Two things the cases found out about the reference's rules, which the records here state:
- A table of 12-bit starts with AUs below 960 bytes ends by byte 4095 + 961, so above
  360 kbit/s (RSDims 46..48) no superframe can be accepted.  At RSDims 48 a `clean`
  superframe is therefore RS-clean with 5 good AUs and a last AU too long: status 2,
  au_crc mask 0x1F, the same corrections counted.  Every other width decodes with status 3.
- An AU that a crafted table puts past the superframe's 110 * RSDims bytes is read by the
  reference from uninitialised memory (its `outVector` is a stack buffer).  The GPU layer
  defines those bytes as zero and orc.MP4 does the same (a zeroed buffer); the cases that
  reach there (Case.past_end) are left out of the ref_mp4_add comparison, not of the oracle's."""
import ctypes as C

import numpy as np
import pytest

import dabplus_py as dp
import oracle_py as orc


def record(br, sf):
    """orc.MP4's record at the 5th CIF of a superframe fed to a new mp4Processor"""
    m = orc.MP4(br)
    o = None
    for i, row in enumerate(dp.rows_of(sf, br)):
        o = m.add(np.unpackbits(row))
        assert o["status"] == (0 if i < 4 else o["status"])
    return o


def every_case():
    """(width, case) of everything the GPU tests play, both streams"""
    seen = set()
    for plan in dp.every_plan():
        for w, cs in plan.items():
            for c in cs:
                if c.sf.tobytes() not in seen:
                    seen.add(c.sf.tobytes())
                    yield w, c


@pytest.fixture(scope="module")
def cases():
    return list(every_case())


def test_fire_code_encoder_passes_the_checker():
    rng = np.random.default_rng(7)
    for _ in range(200):
        b = rng.integers(0, 256, 11).astype(np.uint8)
        dp.fire_fix(b)
        assert orc.oracle().orc_firecode_check(orc.P(b)) == 1
        b[int(rng.integers(11))] ^= 1 << int(rng.integers(8))
        assert orc.oracle().orc_firecode_check(orc.P(b)) == 0


def test_au_crc_is_the_oracles():
    rng = np.random.default_rng(8)
    for ln in (0, 1, 63, 64, 65, 959):
        msg = np.zeros(ln + 2, np.uint8)
        msg[:ln] = rng.integers(0, 256, ln)
        c = dp.au_crc(msg[:ln])
        msg[ln], msg[ln + 1] = c >> 8, c & 0xFF
        assert orc.oracle().orc_dabplus_crc(orc.P(msg), C.c_int16(ln)) == 1
        msg[ln + 1] ^= 1
        assert orc.oracle().orc_dabplus_crc(orc.P(msg), C.c_int16(ln)) == 0


def test_clean_superframe_at_every_width():
    """status 3, nothing corrected, every CRC good -- at RSDims 48 status 2 with the 5 AUs that
    a table can place good (see the module's note)"""
    for w in dp.WIDTHS:
        for lay in dp.LAYOUTS:
            o = record(8 * w, dp.clean(8 * w, np.random.default_rng(w), layout=lay))
            assert o["n_corrected"] == 0
            if dp.fillable(8 * w):
                assert o["status"] == 3 and dp.mask_of(o) == (1 << o["num_aus"]) - 1, (w, lay)
                if dp.fit(8 * w, *lay) is not None:
                    assert o["num_aus"] == dp.LAYOUTS[lay][0]
            else:
                assert w == 48 and (o["status"], o["num_aus"], dp.mask_of(o)) == (2, 6, 0x1F)
    assert [w for w in range(1, 49) if not dp.fillable(8 * w)] == [46, 47, 48]


def test_every_case_is_what_its_name_says(cases):
    names = {}
    for w, c in cases:
        dp.check_expect(w, c, record(8 * w, c.sf))
        names.setdefault(c.name, set()).add(w)
    assert names["six_in_last_column"] == set(dp.FAIL_WIDTHS)
    for name in ("len_960_first", "start_4095"):
        assert names[name] == set(dp.AU_WIDTHS + dp.FORMAT_WIDTHS)
    # an AU that starts inside and ends past the end: every layout at widths 2 and 3, the 6-AU layout
    # at 33 (4 AUs below 960 bytes cannot span it); at 48 no 12-bit start lies past the end
    assert names["ends_past"] == {2, 3, 33} and 33 in names["len_960_later"] and names["last_too_long"] == {48}
    # the AU lengths of section 4 all occur: 0, 1, 63, 64, 65, and 959 at a width that holds it
    lens = {(w, ln) for w, c in cases if c.expect.get("lens") for ln in c.expect["lens"]}
    assert {(2, ln) for ln in dp.EDGE_LENS} <= lens and (33, 959) in lens and (33, 63) in lens


def test_miscorrecting_patterns_are_found():
    found = dp.miscorrecting()
    print("miscorrecting patterns of 6, 7, 8 errors:", [len(found[k]) for k in (6, 7, 8)])
    assert all(len(found[k]) >= 8 for k in (6, 7, 8))
    n3 = sum(record(8 * w, c.sf)["status"] == 3 for w in dp.WIDTHS for c in dp.cases_misc(w, 0))
    assert n3 > 0                                        # some miscorrected superframes pass the AU table


def test_rejected_superframes_are_followed_by_resynchronisation():
    """after a rejected superframe 4 blocks stay: the next 4 CIFs end misaligned windows (the fire
    code fails: 1), the 5th ends the next superframe"""
    for s in (0, 1):
        for w, cs in dp.plan_fail(s).items():
            m = orc.MP4(8 * w)
            got = [m.add(np.unpackbits(r))["status"] for r in dp.to_script(cs, 8 * w)]
            assert got == [0, 0, 0, 0, 2] + [1, 1, 1, 1, 2] * 2 + [1, 1, 1, 1, 3 if dp.fillable(8 * w) else 2], (w, got)
        for plan in dp.every_plan():
            assert all(len(cs) <= 8 for cs in plan.values())


def test_walk_scripts_are_what_they_say():
    for s in (0, 1):
        for w in dp.WIDTHS:
            br, rows = 8 * w, dp.script_walk(w, s)
            m = orc.MP4(br)
            got = [m.add(np.unpackbits(r))["status"] for r in rows]
            assert got == dp.walk_statuses(w, dp.walk_variant(w, s), len(rows)), (w, s, got)


# ---- the restatement against the reference's own classes --------------------------------
class _RefSt(C.Structure):
    _fields_ = [("bitRate", C.c_int), ("fill", C.c_int), ("blocks", C.c_int), ("ring", C.c_uint8 * (120 * 48))]


def ref_sequence(br, rows):
    """[(status, AUs with a good CRC)] of ref_mp4_add over the rows"""
    st = _RefSt()
    st.bitRate = br
    ok = C.c_int(0)
    out = []
    for r in rows:
        bits = np.unpackbits(r)
        out.append((orc.ref().ref_mp4_add(C.byref(st), orc.P(bits), C.byref(ok)), ok.value))
    return out


def orc_sequence(br, rows):
    m = orc.MP4(br)
    out = []
    for r in rows:
        o = m.add(np.unpackbits(r))
        out.append((o["status"], int(sum(o["au_crc"][:o["num_aus"]]))))
    return out


needs_ref = pytest.mark.skipif(orc.ref() is None, reason="oracle/_ref not built")


@needs_ref
def test_columns_and_headers_match_the_reference(cases):
    ref, n_cw, n_hdr, verdicts = orc.ref(), 0, 0, {}
    for w, c in cases:
        for j in range(w):
            cw = dp.column(c.sf, 8 * w, j)
            out = np.zeros(110, np.uint8)
            r = ref.ref_rs_dec(orc.P(cw), orc.P(out))
            o, ro = orc.rs_dec(cw)
            assert r == ro and np.array_equal(out, o), (w, c.name, j)
            verdicts[r] = verdicts.get(r, 0) + 1
            n_cw += 1
        hdr = np.ascontiguousarray(c.sf[:11])
        assert ref.ref_firecode_check(orc.P(hdr)) == orc.oracle().orc_firecode_check(orc.P(hdr)) == 1
        n_hdr += 1
    for k in (6, 7, 8):
        for pat in dp.miscorrecting()[k]:
            cw = dp.rs_encode(np.random.default_rng(k).integers(0, 256, 110).astype(np.uint8))
            for r, v in pat:
                cw[r] ^= v
            out = np.zeros(110, np.uint8)
            r = ref.ref_rs_dec(orc.P(cw), orc.P(out))
            o, ro = orc.rs_dec(cw)
            assert r == ro >= 0 and np.array_equal(out, o)
            n_cw += 1
    for s in (0, 1):
        for w in dp.WIDTHS:
            for row in dp.script_walk(w, s) + [dp.filler(8 * w, s)]:
                hdr = np.ascontiguousarray(row[:11])
                assert ref.ref_firecode_check(orc.P(hdr)) == orc.oracle().orc_firecode_check(orc.P(hdr))
                n_hdr += 1
    print("codeword columns compared with the reference's reedSolomon:", n_cw, "by verdict", dict(sorted(verdicts.items())))
    print("11-byte headers compared with the reference's firecode_checker:", n_hdr)
    assert n_cw > 4000 and verdicts[-1] > 20 and verdicts[5] > 500


@needs_ref
def test_cif_sequences_match_the_reference(cases):
    n_seq = n_cif = n_left_out = 0
    for w, c in cases:
        if c.past_end:
            n_left_out += 1
            continue
        rows = dp.rows_of(c.sf, 8 * w)
        assert ref_sequence(8 * w, rows) == orc_sequence(8 * w, rows), (w, c.name)
        n_seq += 1
        n_cif += 5
    # the scripts as the GPU tests string them: cases end to end, so that a rejected superframe
    # is followed by the re-synchronisation (blocks = 4); and the walk's scripts
    for plan in dp.every_plan():
        for w, cs in plan.items():
            rows = dp.to_script([c for c in cs if not c.past_end], 8 * w)
            assert ref_sequence(8 * w, rows) == orc_sequence(8 * w, rows), w
            n_seq += 1
            n_cif += len(rows)
    for s in (0, 1):
        for w in dp.WIDTHS:
            rows = dp.script_walk(w, s)
            assert ref_sequence(8 * w, rows) == orc_sequence(8 * w, rows), (w, s)
            n_seq += 1
            n_cif += len(rows)
    print("CIF sequences compared with ref_mp4_add:", n_seq, "of", n_cif, "CIFs;",
          n_left_out, "cases left out (an AU past the superframe)")
    assert n_seq > 300 and n_left_out >= 8
