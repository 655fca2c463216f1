"""Generates tests/golden/read_model.npz from the REFERENCE's own repeat search compiled where it lies: for exactly the cases of
tests/read_model_cases.py the repeat length at every offset of every read, the PCR cache table and the modified qual / ins / del / gcp
bytes (oracle/_ref/ref_read_model reads), the counts of findNumberOfRepetitions on the 100 000 seeded triples through both overloads
(oracle/_ref/ref_read_model reps), and the digest of the cases.  Inputs are not stored: the cases module regenerates them from seeds.
The harness is oracle/ref_harness/ref_read_model_harness.cpp, built by `make -C oracle _ref/ref_read_model`; build products go to
oracle/_ref/ and are never committed.  The file is written with fixed zip timestamps: a second run reproduces it byte for byte.
Run in the build container (needs the reference tree; REF overrides its place)."""
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import read_model_cases as C  # noqa: E402

OUT = os.path.join(ROOT, "oracle", "_ref")
EXE = os.path.join(OUT, "ref_read_model")


def build():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "_ref/ref_read_model"] + (["REF=" + os.environ["REF"]] if "REF" in os.environ else []))
    return EXE


def ask(mode, text):
    """the harness's answer to ``text`` (it reads a file)"""
    path = os.path.join(OUT, "read_model_%s.txt" % mode)
    with open(path, "w") as f:
        f.write(text)
    return subprocess.run([EXE, mode, path], check=True, capture_output=True, text=True).stdout


def reps_counts(triples):
    """counts per triple; the two overloads must agree"""
    pairs = np.array([[int(x) for x in ln.split()] for ln in ask("reps", C.reps_text(triples)).splitlines()], dtype=np.int64).reshape(-1, 2)
    assert len(pairs) == len(triples) and np.array_equal(pairs[:, 0], pairs[:, 1]), "the two overloads of findNumberOfRepetitions disagree"
    return pairs[:, 0].astype(np.uint8)


def save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)


def main():
    build()
    cases = C.model_cases()
    got = C.parse_reads_answers(ask("reads", C.reads_text(cases)), cases)
    out = {"digest": np.array([C.digest()]), "reps": reps_counts(C.reps_triples()),
           "cache": np.array([cache or [0] * (C.MAX_REPEAT_LENGTH + 1) for cache, _ in got], dtype=np.uint8)}
    for k, key in enumerate(C.GOLDEN_KEYS):
        out[key] = np.frombuffer(b"".join(per_read[k] for _, reads in got for per_read in reads), dtype=np.uint8)
    dst = os.path.join(HERE, "read_model.npz")
    save(dst, out)
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(cases), "cases,", len(out["rl"]), "bases,", len(out["reps"]), "triples")


if __name__ == "__main__":
    main()
