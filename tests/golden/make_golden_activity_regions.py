"""Generates tests/golden/activity_regions.npz from the REFERENCE's own ActivityProfile.cpp and ActivityProfileState.cpp compiled where they
lie: per case of tests/activity_region_cases.py the regions, every state value (bit-exact) and the weights, and the cases' checksum.
The pop cadence, the cut and the accumulation into the state list are compiled reference code; the 20 lines of the band-pass subclass
are restated in the harness, tests/golden/ref_activity_regions_harness.cpp, which also says what else it defines itself.  Build
products go to oracle/_ref/ and are never committed.  Run in the build container (needs the reference tree; REF overrides its place)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import activity_region_cases as R  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
M2 = os.path.join(REF, "deepmutect", "Mutect2Cpp-master", "src")
HTS = os.path.join(REF, "deepmutect", "htslib")
OUT = os.path.join(ROOT, "oracle", "_ref")
INC = [M2, M2 + "/intel/common", M2 + "/intel/pairhmm", M2 + "/haplotype", M2 + "/samtools", M2 + "/read", HTS, HTS + "/htslib",
       M2 + "/cigar", M2 + "/smithwaterman", M2 + "/utils", M2 + "/cache"]
SOURCES = [M2 + "/ActivityProfile.cpp", M2 + "/ActivityProfileState.cpp"]


def build():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "ref_activity_regions")
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-ffp-contract=off"] + ["-I" + i for i in INC] + [os.path.join(HERE, "ref_activity_regions_harness.cpp")] + SOURCES
    subprocess.check_call(cmd + ["-Wl,--unresolved-symbols=ignore-all", "-o", exe])
    return exe


def main():
    exe = build()
    case_list = R.all_cases()
    path = os.path.join(OUT, "activity_region_cases.txt")
    with open(path, "w") as f:
        f.write(R.to_text(case_list))
    got = R.parse_answers(subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout, case_list)
    default = [w for c, (_, _, w) in zip(case_list, got) if c["weights"] is None]
    assert all(np.array_equal(w, default[0]) for w in default)
    out = {"digest": np.array([R.digest(case_list)], np.uint32), "weights": default[0],
           "region_off": np.concatenate([[0], np.cumsum([len(g[0]) for g in got])]).astype(np.uint64),
           "state_off": np.concatenate([[0], np.cumsum([len(g[1]) for g in got])]).astype(np.uint64),
           "regions": np.concatenate([g[0] for g in got]).astype(np.int32), "values": np.concatenate([g[1] for g in got])}
    dst = os.path.join(HERE, "activity_regions.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(case_list), "cases,", len(out["regions"]), "regions,", len(out["values"]), "states")


if __name__ == "__main__":
    main()
