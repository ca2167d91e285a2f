"""Generate tests/golden/mp2_kat.npz from the REFERENCE's own layer II decoder.

The reference's src/backend/audio/mp2processor.cpp is compiled where it lies (never
copied), with g++ -O2 against the three stub headers in tests/cpp/mp2_stubs (QObject,
gui.h, audiosink.h) and that directory's driver, into a temporary directory outside the
repository.  The streams of tests/mp2_py.fixtures() go through mp2Processor::addtoFrame
in CIF-sized pieces; the file keeps, per stream, the input bits (packed), the PCM of
every frame that reached the sink, and its rate.  Only the .npz is committed.

Run from the repo root:  python tests/golden/make_mp2_golden.py   (REF=/path/to/reference)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import mp2_py  # noqa: E402

REF = os.environ.get("REF", "/root/reference")


def main():
    stubs = os.path.join(TESTS, "cpp", "mp2_stubs")
    fx = mp2_py.fixtures()
    out = {"names": np.array([f["name"] for f in fx])}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mp2_golden")
        subprocess.run(["g++", "-O2", "-std=gnu++11", "-w", "-I" + stubs, "-I" + REF + "/includes/backend/audio",
                        "-I" + REF + "/includes/backend", "-o", exe, os.path.join(stubs, "mp2_golden_driver.cpp"),
                        REF + "/src/backend/audio/mp2processor.cpp", "-lm"], check=True)
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            for s in fx:
                f.write(np.array([s["bitrate"], len(s["bits"])], np.int32).tobytes())
                f.write(s["bits"].tobytes())
        subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    pos = 0
    for i, s in enumerate(fx):
        n = int(np.frombuffer(raw, np.int32, 1, pos)[0])
        pos += 4
        rec = np.frombuffer(raw, np.dtype([("rate", "<i4"), ("pcm", "<i2", (1152, 2))]), n, pos)
        pos += n * rec.dtype.itemsize
        out["bitrate_%d" % i] = np.int32(s["bitrate"])
        out["nbits_%d" % i] = np.int32(len(s["bits"]))
        out["bits_%d" % i] = np.packbits(s["bits"])
        out["pcm_%d" % i] = rec["pcm"].copy()
        out["rate_%d" % i] = rec["rate"].copy()
        print("%-10s bitRate %3d  %5d bits  %2d frames to the sink" % (s["name"], s["bitrate"], len(s["bits"]), n))
    assert pos == len(raw)
    path = os.path.join(HERE, "mp2_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
