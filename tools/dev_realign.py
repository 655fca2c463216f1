"""A/B of mgx_realign_regions against the composition of the calls that existed before it (mgx_pairhmm_regions, host searchBestAllele and
lastIndexOf, host assembly, mgx_sw_align_batch): builds tools/realign_ab.cpp against libmgx.so, runs the project's region leg (1 000
regions of 40 x 25) and a large-region leg (200 regions of 300 x 100, reads 100-151 against haplotypes 250-400), each with about 90 %
and about 0 % of the reads verbatim, and writes what the program printed.  Needs an MI355X.

    python tools/dev_realign.py [--out profiles/realign_ab.txt] [--rounds 6] [--build-only]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKGDIR = os.path.join(ROOT, "fast-genomic-data-processing_amd")
EXE = os.path.join(ROOT, "tools", "bin", "realign_ab")
# n_regions n_reads n_haps read_min read_max hap_min hap_max
LEGS = [("region leg", (1000, 40, 25, 20, 128, 64, 256)), ("large regions", (200, 300, 100, 100, 151, 250, 400))]
SHARES = (90, 0)


def build():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    src = os.path.join(ROOT, "tools", "realign_ab.cpp")
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= max(os.path.getmtime(src), os.path.getmtime(os.path.join(PKGDIR, "libmgx.so"))):
        return
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-L", PKGDIR, "-lmgx",
                           "-Wl,-rpath," + PKGDIR, "-o", EXE])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "realign_ab.txt"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    build()
    if a.build_only:
        return 0
    text = ["mgx_realign_regions (fused) against the composition of mgx_pairhmm_regions, host searchBestAllele + lastIndexOf, host assembly and",
            f"mgx_sw_align_batch (composed): one process per workload, the two take turns, one warm-up each, {a.rounds} rounds; wall time per call.", ""]
    for name, shape in LEGS:
        for share in SHARES:
            res = subprocess.run([EXE] + [str(x) for x in shape] + [str(share), str(a.rounds)], capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                sys.stderr.write(res.stdout + res.stderr)
                return res.returncode
            text += [f"== {name}, {share} % verbatim asked", res.stdout.rstrip(), ""]
            print(text[-3] + "\n" + text[-2], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
