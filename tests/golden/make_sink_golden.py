"""Generate tests/golden/sink_kat.npz from the REFERENCE's own audio sink.

The reference's src/output/audiosink.cpp and src/output/fir-filters.cpp are compiled where they
lie (never copied), with g++ -O2 -std=gnu++11 (no -ffast-math) against the stub headers in
tests/cpp/sink_stubs (QObject, QComboBox, QString, QDebug, portaudio.h, sndfile.h) and that
directory's driver, into a temporary directory outside the repository.  The driver subclasses
audioSink, selects the (stub) default device and, after every audioOut, drains exactly what
arrived in _O_Buffer through paCallback_o.  The file keeps the three filter kernels, a sweep of
all 65536 int16 values through one 48000 call, and the scripted sequences of
tests/sink_py.sequences(), one sink each: per call the rate, the PCM and the floats that
arrived.  Only the .npz is committed.

Run from the repo root:  python tests/golden/make_sink_golden.py   (REF=/path/to/reference)
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import sink_py  # noqa: E402

REF = os.environ.get("REF", "/root/reference")


def main():
    stubs = os.path.join(TESTS, "cpp", "sink_stubs")
    sweep = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16).reshape(32768, 2)
    seqs = [("sweep48", [(48000, sweep)])] + sink_py.sequences()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sink_golden")
        subprocess.run(["g++", "-O2", "-std=gnu++11", "-w", "-I" + stubs, "-I" + REF + "/includes", "-I" + REF + "/includes/output",
                        "-I" + REF + "/includes/various", "-o", exe, os.path.join(stubs, "sink_golden_driver.cpp"),
                        REF + "/src/output/audiosink.cpp", REF + "/src/output/fir-filters.cpp", "-lm"], check=True)
        with open(os.path.join(tmp, "in.bin"), "wb") as f:
            for _, calls in seqs:
                f.write(np.int32(len(calls)).tobytes())
                for rate, pcm in calls:
                    f.write(np.array([rate, len(pcm)], np.int32).tobytes())
                    f.write(np.ascontiguousarray(pcm, np.int16).tobytes())
        subprocess.run([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")], check=True)
        raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    out = {"coef": np.frombuffer(raw, np.float32, 15, 0).reshape(3, 5).copy(), "names": np.array([n for n, _ in seqs[1:]])}
    pos, total = 60, 0
    for name, calls in seqs:
        got = []
        for rate, pcm in calls:
            n = int(np.frombuffer(raw, np.int32, 1, pos)[0])
            pos += 4
            assert n == sink_py.n_out(len(pcm), rate), (name, rate, len(pcm), n)
            got.append(np.frombuffer(raw, np.float32, 2 * n, pos).reshape(n, 2).copy())
            pos += 8 * n
        if name == "sweep48":
            out["sweep48"] = got[0]              # the input is np.arange(-32768, 32768) as 32768 pairs
            continue
        out[name + "_rate"] = np.array([r for r, _ in calls], np.int32)
        out[name + "_amount"] = np.array([len(p) for _, p in calls], np.int32)
        out[name + "_pcm"] = np.concatenate([p for _, p in calls])
        out[name + "_out"] = np.concatenate(got)
        total += len(out[name + "_out"])
        print("%s: %d calls, %d pairs in, %d pairs out" % (name, len(calls), len(out[name + "_pcm"]), len(out[name + "_out"])))
    assert pos == len(raw)
    path = os.path.join(HERE, "sink_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", total, "scripted output pairs")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
