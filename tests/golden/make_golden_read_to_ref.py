"""Generates tests/golden/read_to_ref.npz from the REFERENCE's own AlignmentUtils compiled where it lies: the answers (status, start,
elements) to the cases of tests/read_to_ref_cases.py on which the reference is defined, with those cases' checksum.  The harness is
tests/golden/ref_read_to_ref_harness.cpp; build products go to oracle/_ref/ and are never committed.
Run in the build container (needs the reference tree; REF overrides its place)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import read_to_ref_cases as C  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
M2 = os.path.join(REF, "deepmutect", "Mutect2Cpp-master", "src")
HTS = os.path.join(REF, "deepmutect", "htslib")
OUT = os.path.join(ROOT, "oracle", "_ref")
INC = [M2, M2 + "/intel/common", M2 + "/intel/pairhmm", M2 + "/haplotype", M2 + "/samtools", M2 + "/read", HTS, HTS + "/htslib",
       M2 + "/cigar", M2 + "/smithwaterman"]
SOURCES = [M2 + "/read/AlignmentUtils.cpp", M2 + "/cigar/Cigar.cpp", M2 + "/cigar/CigarElement.cpp", M2 + "/cigar/CigarOperator.cpp",
           M2 + "/smithwaterman/SWParameters.cpp"]


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "ref_read_to_ref")
    # -DNDEBUG: an offset beyond the padded list is left to the function's own "ran off the end" throw, not to its assert
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-DNDEBUG"] + ["-I" + i for i in INC] + [os.path.join(HERE, "ref_read_to_ref_harness.cpp")] + SOURCES
    subprocess.check_call(cmd + ["-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def line_of(c):
    sw, hap = C.encode(c["sw"]), C.encode(c["hap"])
    return " ".join([str(c["offset"]), str(c["hap_start"]), str(c["reference_start"]), str(len(sw))] + [str(int(e)) for e in sw]
                    + [str(len(hap))] + [str(int(e)) for e in hap] + [c["ref"].decode() or "-", c["read"].decode() or "-"])


def answers(exe, case_list):
    path = os.path.join(OUT, "read_to_ref_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(line_of(c) for c in case_list) + "\n")
    lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(case_list), (len(lines), len(case_list))
    return [[int(x) for x in ln.split()] for ln in lines]


def main():
    exe = build()
    out = {}
    for key, case_list in (("cpu", C.cases()), ("shape", C.shape_cases())):
        # only where the reference is defined: the restatement says where it is not
        defined = [i for i, c in enumerate(case_list) if C.to_ref(dict(c, stride=1 << 30, hard=(0, 0)))[0] != C.UNDEFINED]
        got = answers(exe, [case_list[i] for i in defined])
        off = np.zeros(len(got) + 1, np.uint32)
        off[1:] = np.cumsum([g[2] for g in got])
        out[key + "_digest"] = np.array([C.digest(case_list)], np.uint32)
        out[key + "_index"] = np.array(defined, np.uint32)
        out[key + "_status"] = np.array([g[0] for g in got], np.uint8)
        out[key + "_start"] = np.array([g[1] for g in got], np.int32)
        out[key + "_off"] = off
        out[key + "_elements"] = np.array([e for g in got for e in g[3:]], np.uint32)
    path = os.path.join(HERE, "read_to_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: len(out[k + "_index"]) for k in ("cpu", "shape")})


if __name__ == "__main__":
    main()
