"""Generate tests/golden/fib_kat.npz from the REFERENCE's own FIG parser.

The reference's src/backend/fib-processor.cpp is compiled where it lies (never copied), with
g++ -fsanitize=address,undefined -fno-sanitize-recover=all against the stand-in headers in
tests/cpp/fib_stubs -- first on the include path, so its QObject, QString (keeps bytes), gui.h,
charsets.h (toQStringUsingCharset records bytes and character set) win; fib-processor.h finds the
reference's msc-handler.h beside itself, so that header's include guard is defined on the command
line and the stand-in, which includes only the reference's dab-constants.h, is included first --
and that directory's stand-alone driver, into a temporary directory outside the repository.

Per fixture (tests/fib_py.fixtures) the file holds the FIBs, the signals nameofEnsemble /
addtoEnsemble in order with the FIB that raised them, and for every named service its slot, its
label as given to toQStringUsingCharset and what kindofService, dataforAudioService and
dataforDataService answer for that label.

Two precautions.  Every FIB stands alone in 256 bytes of heap, so a read past it stops the run:
no fixture FIB may meet the overrun rule of dabgpu_fib_parse (also asserted with
fib_py.Processor; nothing is filtered).  fib_processor's constructor leaves the service entries'
hasLanguage, language and programType to chance until a FIG 0/17 names the service: the driver
fills what `new` hands out, every fixture runs with the fills 0x00 and 0xA5, and `defined` marks
the lookup fields on which both runs agree (signals, slots, labels and kinds must agree, or the
fixture is refused).  A run that trips a sanitizer fails: the fixture is then changed, not
excused.  Only the .npz is committed.

Run from the repo root:  REF=/path/to/reference python tests/golden/make_fib_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(os.path.dirname(TESTS), "sdr-j-dab_amd"))
import fib_py  # noqa: E402

REF = os.environ.get("REF") or sys.exit("set REF to the reference checkout")


def parse(raw):
    pos = 0

    def ints(n):
        nonlocal pos
        v = np.frombuffer(raw, np.int32, n, pos).tolist()
        pos += 4 * n
        return v

    def qstring():
        nonlocal pos
        pieces = [tuple(ints(2)) for _ in range(ints(1)[0])]
        n = ints(1)[0]
        b = raw[pos:pos + n]
        pos += n
        return pieces, b
    sigs, named = [], []
    for _ in range(ints(1)[0]):
        fib, kind, ident = ints(3)
        pieces, b = qstring()
        assert len(pieces) == 1 and pieces[0][0] == len(b)
        sigs.append((fib, kind, ident, pieces[0][1], b))
    for _ in range(ints(1)[0]):
        slot = ints(1)[0]
        pieces, b = qstring()
        assert 1 <= len(pieces) <= 2 and len({c for _, c in pieces}) == 1
        if len(pieces) == 2:
            assert b[pieces[0][0]:] == b" (data)"
        named.append((slot, pieces[0][1], b[:pieces[0][0]], len(pieces), ints(1)[0], ints(9), ints(10)))
    assert pos == len(raw)
    return sigs, named


def main():
    stubs = os.path.join(TESTS, "cpp", "fib_stubs")
    fx = fib_py.fixtures()
    out = {"names": np.array([n for n, _ in fx])}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "fib_golden")
        subprocess.run(["g++", "-O1", "-g", "-std=gnu++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-DMSC_DECODER", "-include", os.path.join(stubs, "msc-handler.h"),
                        "-I" + stubs, "-I" + REF + "/includes", "-I" + REF + "/includes/backend", "-o", exe,
                        os.path.join(stubs, "fib_golden_driver.cpp"), REF + "/src/backend/fib-processor.cpp"], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        for i, (name, fibs) in enumerate(fx):
            p = fib_py.Processor()
            for k, fb in enumerate(fibs):
                assert not p.fib(bytes(fb), k), (name, k, "meets the overrun rule")
            fin = os.path.join(tmp, "in.bin")
            with open(fin, "wb") as w:
                w.write(np.int32(len(fibs)).tobytes() + np.ascontiguousarray(fibs, np.uint8).tobytes())
            runs = []
            for fill in ("0x00", "0xA5"):
                fout = os.path.join(tmp, "out" + fill)
                subprocess.run([exe, fin, fout, fill], check=True, env=env,
                               stderr=subprocess.DEVNULL if os.environ.get("QUIET") else None)
                runs.append(parse(open(fout, "rb").read()))
            (s0, n0), (s1, n1) = runs
            if s0 != s1 or [x[:5] for x in n0] != [x[:5] for x in n1]:
                sys.exit("fixture %s: signals, slots, labels or kinds depend on uninitialised members" % name)
            defined = [[int(a == b) for a, b in zip(x[5] + x[6], y[5] + y[6])] for x, y in zip(n0, n1)]
            out["fibs_%d" % i] = np.ascontiguousarray(fibs, np.uint8)
            out["sig_%d" % i] = np.array([[f, k, d, c, len(b)] for f, k, d, c, b in s0], np.int32).reshape(-1, 5)
            out["sig_bytes_%d" % i] = np.frombuffer(b"".join(b for *_, b in s0), np.uint8)
            out["named_%d" % i] = np.array([[sl, c, len(b), npc, kind] + a + d for sl, c, b, npc, kind, a, d in n0],
                                           np.int32).reshape(-1, 24)
            out["named_bytes_%d" % i] = np.frombuffer(b"".join(x[2] for x in n0), np.uint8)
            out["defined_%d" % i] = np.array(defined, np.uint8).reshape(-1, 19)
            print("%-20s %3d FIBs  %2d signals  %2d named  kinds %s" % (name, len(fibs), len(s0), len(n0), sorted({x[4] for x in n0})))
    path = os.path.join(HERE, "fib_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
