"""Generate tests/golden/ip_kat.npz from the REFERENCE's own IP handler.

The reference's src/backend/data/ip-datahandler.cpp (and virtual-datahandler.cpp, its base
class) is compiled where it lies (never copied), with g++ -fsanitize=address,undefined against
the stub headers in tests/cpp/ip_stubs (QObject, QByteArray, gui.h; the array checks every
index and holds exactly its size, so a read past a group through data() is seen) and that
directory's driver, into a temporary directory outside the repository.  The fixtures of
tests/ip_py.fixtures() are laid out as dabgpu_pipe_packet delivers them; every group with at
least four bytes goes through ip_dataHandler::add_mscDatagroup whole, its own CRC check included
(shorter ones the reference cannot take: it reads the header's first bits).  One process per
fixture.  The file keeps, per fixture, the group records, their bytes and every writeDatagram
and show_ipErrors call.  A run that trips a sanitizer or a bounds check fails: the fixture is
then changed, not excused.  Only the .npz is committed.

Run from the repo root:  REF=/path/to/reference python tests/golden/make_ip_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import ip_py  # noqa: E402

REF = os.environ.get("REF") or sys.exit("set REF to the reference checkout")


def main():
    stubs = os.path.join(TESTS, "cpp", "ip_stubs")
    fx = ip_py.fixtures()
    out = {"names": np.array([f["name"] for f in fx])}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "ip_golden")
        subprocess.run(["g++", "-O1", "-g", "-std=gnu++11", "-w", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I" + stubs, "-I" + REF + "/includes",
                        "-I" + REF + "/includes/backend/data", "-o", exe, os.path.join(stubs, "ip_golden_driver.cpp"),
                        REF + "/src/backend/data/ip-datahandler.cpp", REF + "/src/backend/data/virtual-datahandler.cpp"],
                       check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        for i, f in enumerate(fx):
            rec, arena = ip_py.pack(f["groups"])
            fed = [g for g, b in enumerate(f["groups"]) if len(b) >= 4]
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(fin, "wb") as w:
                w.write(np.int32(len(fed)).tobytes())
                for g in fed:
                    w.write(np.int32(len(f["groups"][g])).tobytes() + f["groups"][g])
            subprocess.run([exe, fin, fout], check=True, env=env,
                           stderr=subprocess.DEVNULL if os.environ.get("QUIET") else None)
            raw = open(fout, "rb").read()
            n, pos = int(np.frombuffer(raw, np.int32, 1, 0)[0]), 4
            ev, data = [], b""
            for _ in range(n):
                call, kind, value = np.frombuffer(raw, np.int32, 3, pos).tolist()
                pos += 12
                if kind == 0:
                    data += raw[pos:pos + value]
                    pos += value
                ev.append([fed[call], kind, value])
            assert pos == len(raw)
            out["groups_%d" % i] = np.frombuffer(rec.tobytes(), np.uint8)
            out["bytes_%d" % i] = arena
            out["events_%d" % i] = np.array(ev, np.int32).reshape(-1, 3)      # group, kind (0 datagram, 1 show_ipErrors), length or value
            out["event_bytes_%d" % i] = np.frombuffer(data, np.uint8)
            print("%-14s %3d groups  %3d calls  %3d datagrams  show_ipErrors %s" % (
                f["name"], len(rec), len(fed), sum(1 for e in ev if e[1] == 0), [e[2] for e in ev if e[1] == 1]))
    path = os.path.join(HERE, "ip_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
