"""Generate tests/golden/packet_kat.npz from the REFERENCE's own packet-mode code.

The reference's src/backend/data/msc-datagroup.cpp and mot-databuilder.cpp are compiled where
they lie (never copied), with g++ -O2 against the stub headers in tests/cpp/packet_stubs
(QObject, QThread, QMutex, QWaitCondition, QByteArray, the handler, deconvolver and gui.h
headers) and that directory's driver, into a temporary directory outside the repository.
The fixtures of tests/packet_py.fixtures() go through mscDatagroup::handlePackets in
CIF-sized pieces with show_crcErrors on; the file keeps, per fixture, the rows, every group
handed to the data handler, every show_mscErrors value and what the MOT builder passes on
to motHandler::process_mscGroup.  Only the .npz is committed.

Run from the repo root:  REF=/path/to/reference python tests/golden/make_packet_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import packet_py  # noqa: E402

REF = os.environ.get("REF") or sys.exit("set REF to the reference checkout")


def main():
    stubs = os.path.join(TESTS, "cpp", "packet_stubs")
    fx = packet_py.fixtures()
    out = {"names": np.array([f["name"] for f in fx])}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "packet_golden")
        subprocess.run(["g++", "-O2", "-std=gnu++11", "-w", "-I" + stubs, "-I" + REF + "/includes",
                        "-I" + REF + "/includes/backend", "-I" + REF + "/includes/backend/data",
                        "-I" + REF + "/includes/various", "-o", exe, os.path.join(stubs, "packet_golden_driver.cpp"),
                        REF + "/src/backend/data/msc-datagroup.cpp", REF + "/src/backend/data/mot-databuilder.cpp",
                        "-lm", "-lpthread"], check=True)
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            for s in fx:
                f.write(np.array([s["bitrate"], len(s["rows"])], np.int32).tobytes())
                f.write(s["rows"].tobytes())
        subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    pos = 0

    def i32(n=1):
        nonlocal pos
        v = np.frombuffer(raw, np.int32, n, pos)
        pos += 4 * n
        return v
    for i, s in enumerate(fx):
        lens, data = [], b""
        for _ in range(int(i32()[0])):
            n = int(i32()[0])
            lens.append(n)
            data += raw[pos:pos + n]
            pos += n
        q = i32(int(i32()[0])).copy()
        mot = i32(4 * int(i32()[0])).reshape(-1, 4).copy()
        out["bitrate_%d" % i] = np.int32(s["bitrate"])
        out["rows_%d" % i] = s["rows"]
        out["group_len_%d" % i] = np.array(lens, np.int32)
        out["group_bytes_%d" % i] = np.frombuffer(data, np.uint8)
        out["quality_%d" % i] = q
        out["mot_%d" % i] = mot
        print("%-10s bitRate %3d  %3d CIFs  %3d groups  quality %s  %3d MOT calls" %
              (s["name"], s["bitrate"], len(s["rows"]), len(lens), q.tolist(), len(mot)))
    assert pos == len(raw)
    path = os.path.join(HERE, "packet_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
