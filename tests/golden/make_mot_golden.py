"""Generate tests/golden/mot_kat.npz from the REFERENCE's own MOT code.

The reference's src/backend/data/mot-data.cpp is compiled where it lies (never copied), with
g++ -fsanitize=address,undefined against the stub headers in tests/cpp/mot_stubs (QObject,
QByteArray, QString, QDir, QImage, QLabel, gui.h; the containers check every index) and that
directory's driver, into a temporary directory outside the repository.  The fixtures of
tests/mot_py.fixtures() are laid out as dabgpu_pipe_packet delivers them; the groups
mot_databuilder::add_mscDatagroup passes on (accepted, with a transport id) go through
motHandler::process_mscGroup.  The file keeps, per fixture, the group records, their bytes and
every slide and file the reference delivered.  Groups of type 6 are not handed to the
reference: the layer leaves directory mode out (include/dabgpu.h, dabgpu_mot_groups, rule 6)
because the reference analyses a directory before it is complete and then reads entries that
nothing initialised; with them kept away theDirectory stays NULL, as in the layer.  A run that trips a sanitizer or a bounds check
fails: the fixture is then changed, not excused.  Only the .npz is committed.

Run from the repo root:  REF=/path/to/reference python tests/golden/make_mot_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import mot_py  # noqa: E402
import packet_py as pp  # noqa: E402

REF = os.environ.get("REF") or sys.exit("set REF to the reference checkout")


def main():
    stubs = os.path.join(TESTS, "cpp", "mot_stubs")
    fx = mot_py.fixtures()
    out = {"names": np.array([f["name"] for f in fx])}
    packed = [mot_py.pack(f["groups"]) for f in fx]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mot_golden")
        subprocess.run(["g++", "-O1", "-g", "-std=gnu++11", "-w", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I" + stubs, "-I" + REF + "/includes",
                        "-I" + REF + "/includes/backend/data", "-o", exe, os.path.join(stubs, "mot_golden_driver.cpp"),
                        REF + "/src/backend/data/mot-data.cpp"], check=True)
        calls = []
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            for rec, arena in packed:
                fed = [g for g, r in enumerate(rec) if r["flags"] & (pp.ACCEPTED | pp.TID) == (pp.ACCEPTED | pp.TID) and
                       r["groupType"] != 6]
                calls.append(fed)
                f.write(np.int32(len(fed)).tobytes())
                for g in fed:
                    r = rec[g]
                    o = int(r["offset"]) + int(r["data_offset"])
                    f.write(np.array([r["groupType"], (r["flags"] >> 4) & 1, r["segmentNumber"], r["transportId"],
                                      r["data_nbytes"]], np.int32).tobytes())
                    f.write(arena[o:o + int(r["data_nbytes"])].tobytes())
        work = os.path.join(tmp, "files")
        os.mkdir(work)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), work], check=True, env=env,
                       stderr=subprocess.DEVNULL if os.environ.get("QUIET") else None)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    pos = 0
    for i, (f, (rec, arena)) in enumerate(zip(fx, packed)):
        n = int(np.frombuffer(raw, np.int32, 1, pos)[0])
        pos += 4
        ev, names, bodies = [], b"", b""
        for _ in range(n):
            call, kind, sub, nl, bl = np.frombuffer(raw, np.int32, 5, pos).tolist()
            pos += 20
            names += raw[pos:pos + nl]
            bodies += raw[pos + nl:pos + nl + bl]
            pos += nl + bl
            ev.append([calls[i][call], kind, sub, nl, bl])
        out["groups_%d" % i] = np.frombuffer(rec.tobytes(), np.uint8)
        out["bytes_%d" % i] = arena
        out["events_%d" % i] = np.array(ev, np.int32).reshape(-1, 5)      # group, kind, contentsubType, name and body length
        out["event_names_%d" % i] = np.frombuffer(names, np.uint8)
        out["event_bodies_%d" % i] = np.frombuffer(bodies, np.uint8)
        print("%-12s %3d groups  %3d calls  events %s" % (f["name"], len(rec), len(calls[i]), [e[:2] for e in ev]))
    assert pos == len(raw)
    path = os.path.join(HERE, "mot_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
