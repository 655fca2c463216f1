"""Generates tests/golden/activity.npz from the REFERENCE's own code compiled where it lies: per case of tests/activity_cases.py the
element bytes (its PeUtils over its SAMRecord map) and the locus outputs (Mutect2Engine.cpp:58-150 restated in the harness against its
PeUtils and caches), its digamma(1..4096) and log10Factorial(0..4096), its per-quality error probabilities, and the cases' checksum.
The harness is tests/golden/ref_activity_harness.cpp; build products go to oracle/_ref/ and are never committed.
Run in the build container (needs the reference tree; REF overrides its place)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import activity_cases as A  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
M2 = os.path.join(REF, "deepmutect", "Mutect2Cpp-master", "src")
HTS = os.path.join(REF, "deepmutect", "htslib")
OUT = os.path.join(ROOT, "oracle", "_ref")
INC = [M2, M2 + "/intel/common", M2 + "/intel/pairhmm", M2 + "/haplotype", M2 + "/samtools", M2 + "/read", HTS, HTS + "/htslib",
       M2 + "/cigar", M2 + "/smithwaterman", M2 + "/utils", M2 + "/cache"]
SOURCES = [M2 + "/utils/PeUtils.cpp", M2 + "/samtools/SAMRecord.cpp", M2 + "/cache/DigammaCache.cpp", M2 + "/cache/Log10FactorialCache.cpp",
           M2 + "/cache/IntToDoubleFunctionCache.cpp", M2 + "/QualityUtils.cpp", M2 + "/cigar/Cigar.cpp", M2 + "/cigar/CigarElement.cpp",
           M2 + "/cigar/CigarOperator.cpp"]
N_TABLE = 4097


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "ref_activity")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-DNDEBUG"] + ["-I" + i for i in INC] + [os.path.join(HERE, "ref_activity_harness.cpp")] + SOURCES
    subprocess.check_call(cmd + ["-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def floats(words):
    return [float.fromhex(w) if w != "nan" else np.nan for w in words]


def main():
    exe = build()
    case_list = A.shape_cases() + [A.body_case()]
    path = os.path.join(OUT, "activity_cases.txt")
    with open(path, "w") as f:
        f.write(A.to_text(case_list))
    got = A.parse_answers(subprocess.run([exe, "cases", path], check=True, capture_output=True, text=True).stdout, case_list)
    rows = [floats(ln.split()) for ln in subprocess.run([exe, "tables", str(N_TABLE)], check=True, capture_output=True, text=True).stdout.splitlines()]
    out = {"digest": np.array([A.digest(case_list)], np.uint32)}
    out["elem_off"] = np.concatenate([[0], np.cumsum([len(w[0][0]) for w in got])]).astype(np.uint64)
    out["locus_off"] = np.concatenate([[0], np.cumsum([len(w[0][1]) for w in got])]).astype(np.uint64)
    out["elements"] = np.concatenate([w[0][0] for w in got]).astype(np.uint8)
    out["active"] = np.concatenate([w[0][1] for w in got]).astype(np.uint8)
    out["log_odds"] = np.concatenate([w[0][2] for w in got])
    out["depth"] = np.concatenate([w[0][3] for w in got]).astype(np.uint32)
    out["digamma"] = np.array([r[0] for r in rows[:N_TABLE]])
    out["log10_factorial"] = np.array([r[1] for r in rows[:N_TABLE]])
    per_q = np.array(rows[N_TABLE:])
    out["eps"], out["log_eps"], out["log_one_minus_eps"] = per_q[:, 0], per_q[:, 1], per_q[:, 2]
    dst = os.path.join(HERE, "activity.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(case_list), "cases,", len(out["elements"]), "elements,", len(out["active"]), "loci")


if __name__ == "__main__":
    main()
