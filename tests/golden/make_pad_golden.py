"""Generate tests/golden/pad_kat.npz from the REFERENCE's own PAD code.

The reference's src/backend/data/pad-handler.cpp is compiled where it lies (never copied), with
g++ -fsanitize=address,undefined -fno-sanitize-recover=all -DMOT_BASICS__ (as both of the
reference's build files define it) against the stand-in headers in
tests/cpp/pad_stubs -- first on the include path, so its QObject, QString, gui.h, charsets.h
(toQStringUsingCharset records bytes, charset and size in a byte-keeping QString) and mot-data.h
(motHandler hands process_mscGroup's arguments to the driver) win -- and that directory's
driver, into a temporary directory outside the repository.

The language level is C++20 on purpose: pad_crc (:367-373) shifts a negative int16_t left for
every byte above 0x7F, which is undefined before C++20 and defined since (the two's-complement
result every compiler gives); under an older standard the undefined-behaviour sanitizer stops
at the first such byte of any group with a CRC, so no realistic group could be pinned.

Two precautions.  dynamicLabel keeps state in function-local statics that outlive a handler:
the driver runs one fixture per process.  padHandler's constructor leaves last_appType,
msc_dataGroupIndex, msc_dataGroupLength and the group buffer uninitialised: every fixture runs
twice, the handler made by placement new in storage filled with 0x00 and with 0xA5, and the
file is written only if both runs give identical records -- no fixture reads such a member.
tests/pad_py.py marks every PAD that touches one of the layer's rules 1-4 (include/dabgpu.h,
dabgpu_pad_aus); no PAD of a fixture may be marked (asserted here: the fixtures are built that
way, none is filtered).  A run that trips a sanitizer fails: the fixture is then changed, not
excused.  Only the .npz is committed; a second run writes the same bytes (checked by its sha256:
the arrays are equal and numpy gives the zip members a fixed date).

Run from the repo root:  REF=/path/to/reference python tests/golden/make_pad_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import pad_py  # noqa: E402

REF = os.environ.get("REF") or sys.exit("set REF to the reference checkout")


def parse(raw):
    """the driver's output -> (labels, calls)"""
    pos = 0

    def ints(n):
        nonlocal pos
        v = np.frombuffer(raw, np.int32, n, pos).tolist()
        pos += 4 * n
        return v
    labels, calls = [], []
    for _ in range(ints(1)[0]):
        au, cs, npieces, nb = ints(4)
        pieces, charsets = ints(npieces), ints(npieces)
        labels.append(dict(au=au, charset=cs, pieces=pieces, charsets=charsets, text=raw[pos:pos + nb]))
        pos += nb
    for _ in range(ints(1)[0]):
        c = ints(7)
        calls.append((c, raw[pos:pos + c[6]]))
        pos += c[6]
    assert pos == len(raw)
    return labels, calls


def main():
    stubs = os.path.join(TESTS, "cpp", "pad_stubs")
    fx = pad_py.fixtures()
    out = {"names": np.array([f["name"] for f in fx])}
    for f in fx:
        h = pad_py.Handler().feed(f["aus"])
        assert len(f["aus"]) <= 64 and not any(h.touched), (f["name"], h.touched)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pad_golden")
        subprocess.run(["g++", "-O1", "-g", "-std=gnu++20", "-w", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-DMOT_BASICS__", "-I" + stubs, "-I" + REF + "/includes",
                        "-I" + REF + "/includes/backend/data", "-o", exe, os.path.join(stubs, "pad_golden_driver.cpp"),
                        REF + "/src/backend/data/pad-handler.cpp"], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        for i, f in enumerate(fx):
            fin = os.path.join(tmp, "in.bin")
            with open(fin, "wb") as w:
                w.write(np.int32(len(f["aus"])).tobytes())
                for a in f["aus"]:
                    w.write(np.array([a[1], len(a[0])], np.int32).tobytes() + bytes(a[0]))
            raws = []
            for fill in ("0x00", "0xA5"):                       # one process per fixture and fill
                fout = os.path.join(tmp, "out" + fill)
                subprocess.run([exe, fin, fout, fill], check=True, env=env,
                               stderr=subprocess.DEVNULL if os.environ.get("QUIET") else None)
                raws.append(open(fout, "rb").read())
            if raws[0] != raws[1]:
                sys.exit("fixture %s reads an uninitialised member: the two fills differ" % f["name"])
            labels, calls = parse(raws[0])
            for l in labels:                                    # charSet at the emission is what every piece was given
                assert l["charsets"] == [l["charset"]] * len(l["pieces"]), f["name"]
            out["au_len_%d" % i] = np.array([a[1] for a in f["aus"]], np.int32)
            out["au_nbytes_%d" % i] = np.array([len(a[0]) for a in f["aus"]], np.int32)
            out["au_bytes_%d" % i] = np.frombuffer(b"".join(bytes(a[0]) for a in f["aus"]), np.uint8)
            out["labels_%d" % i] = np.array([[l["au"], l["charset"], len(l["pieces"]), len(l["text"])] for l in labels],
                                            np.int32).reshape(-1, 4)      # au, charSet, pieces, bytes
            out["label_pieces_%d" % i] = np.array([p for l in labels for p in l["pieces"]], np.int32)
            out["label_piece_charsets_%d" % i] = np.array([p for l in labels for p in l["charsets"]], np.int32)
            out["label_bytes_%d" % i] = np.frombuffer(b"".join(l["text"] for l in labels), np.uint8)
            # au, groupType, last, segmentNumber, transportId, index, length
            out["calls_%d" % i] = np.array([c for c, _ in calls], np.int32).reshape(-1, 7)
            out["call_bytes_%d" % i] = np.frombuffer(b"".join(b for _, b in calls), np.uint8)
            print("%-14s %2d AUs  labels %s  calls %s" % (f["name"], len(f["aus"]), [bytes(l["text"][:12]) for l in labels][:4],
                                                         [(c[1], c[6]) for c, _ in calls][:8]))
    path = os.path.join(HERE, "pad_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
