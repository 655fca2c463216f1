"""A/B of the PairHMM queue's wire form (MGX_PAIRHMM_WIRE): the flag off and on taking turns in ONE process.

  independent   4 M independent 128 x 256 test cases, the generator and seed of bench.py's "queue" leg; 8 lanes, depth 2,
                65 536 test cases per batch: the PCIe-bound leg the wire form is for
  regions       1 000 regions of 40 reads x 25 haplotypes as one pair-list stream (reads and haplotypes shared inside a
                region): few bytes per test case, so this shows what the bit-packing costs where the link is not the bound

Per round: host -> host GCUPS, bytes_h2d per test case, pack_seconds and wait_seconds (summed over lanes).  The yardstick is
the flag-off run of the same process; a difference counts once it exceeds three times the off runs' spread.
Without --leg both legs run, each in a child process under its own time limit, and the run stops at the first that fails.

  python tools/dev_queue_wire.py [--rounds 6] [--pairs 4194304] [--lanes 8] [--leg independent|regions]
"""
import argparse
import importlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "fast-genomic-data-processing_amd"


def regions_stream(synth, n_regions=1000):
    distinct = [synth.gen_pairhmm_region(40, 25, 1000 + g, r_range=(20, 128), h_range=(64, 256)) for g in range(50)]
    keys = ("bases", "qual", "ins", "dele", "gcp", "hap_bases")
    parts = {k: [] for k in keys + ("read_off", "hap_off", "pair_read", "pair_hap")}
    rb = hb = nr = nh = cells = 0
    for g in range(n_regions):
        r = distinct[g % len(distinct)]
        for k in keys:
            parts[k].append(r[k])
        parts["read_off"].append(r["read_off"][:-1].astype(np.uint64) + np.uint64(rb)); parts["hap_off"].append(r["hap_off"][:-1].astype(np.uint64) + np.uint64(hb))
        parts["pair_read"].append(r["pair_read"].astype(np.uint32) + np.uint32(nr)); parts["pair_hap"].append(r["pair_hap"].astype(np.uint32) + np.uint32(nh))
        rb += int(r["read_off"][-1]); hb += int(r["hap_off"][-1]); nr += len(r["read_off"]) - 1; nh += len(r["hap_off"]) - 1
        cells += r["cells"]
    d = {k: np.concatenate(v) for k, v in parts.items()}
    d["read_off"] = np.concatenate([d["read_off"], np.array([rb], dtype=np.uint64)])
    d["hap_off"] = np.concatenate([d["hap_off"], np.array([hb], dtype=np.uint64)])
    d["cells"] = cells
    return d


def run_leg(leg, rounds, pairs, lanes):
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    if leg == "independent":
        d = synth.gen_pairhmm_pairs_fast(pairs, 0x5EED0003, threads=min(16, os.cpu_count() or 1))
        cells = pairs * 128 * 256
        what = f"{pairs} independent 128 x 256 test cases (seed 0x5EED0003)"
    else:
        d = regions_stream(synth)
        cells = d["cells"]
        what = f"1000 regions of 40 reads x 25 haplotypes as one pair-list stream of {len(d['pair_read'])} test cases"
    n = len(d["pair_read"])
    prepared = pkg.pairhmm.make_input(d)
    qs = {name: pkg.PairHMMQueue(devices=(0,), lanes_per_device=lanes, depth=2, batch_pairs=65536, flags=flags)
          for name, flags in (("off", 0), ("on", pkg.pairhmm.WIRE))}
    outs = {}
    for name, q in qs.items():                       # warm-up: pinned slabs are allocated on first use
        outs[name] = q.run(d, with_flags=True, prepared=prepared)
    same = bool(np.array_equal(outs["off"][0], outs["on"][0]) and np.array_equal(outs["off"][1], outs["on"][1]))
    del outs
    print(f"== {leg}: {what}; {lanes} lanes, depth 2, 65536 per batch; results and used_f64 flags identical off/on: {same}", flush=True)
    print(f"{'round':>5} {'wire':>4} {'GCUPS':>8} {'seconds':>8} {'B/test case':>11} {'H2D GB/s':>8} {'pack_s':>7} {'wait_s':>7}", flush=True)
    rate = {"off": [], "on": []}
    rows = {"off": [], "on": []}
    for r in range(rounds):
        for name in ("off", "on"):
            q = qs[name]
            t0 = time.perf_counter()
            q.run(d, prepared=prepared)
            dt = time.perf_counter() - t0
            st = q.stats()
            g = cells / dt / 1e9
            rate[name].append(g); rows[name].append((st["bytes_h2d"] / n, st["pack_seconds"], st["wait_seconds"]))
            print(f"{r:>5} {name:>4} {g:>8.0f} {dt:>8.4f} {st['bytes_h2d'] / n:>11.1f} {st['bytes_h2d'] / dt / 1e9:>8.1f} {st['pack_seconds']:>7.3f} {st['wait_seconds']:>7.3f}", flush=True)
    for q in qs.values():
        q.close()
    off, on = np.array(rate["off"]), np.array(rate["on"])
    spread = float(off.max() - off.min())
    diff = float(np.median(on) - np.median(off))
    for name, a in (("off", off), ("on", on)):
        b = np.array(rows[name])
        print(f"{name:>3}: median {np.median(a):.0f} GCUPS, spread (max - min) {a.max() - a.min():.0f}; bytes/test case {np.median(b[:, 0]):.1f}, "
              f"pack_s median {np.median(b[:, 1]):.3f}, wait_s median {np.median(b[:, 2]):.3f}", flush=True)
    verdict = "a difference" if abs(diff) > 3 * spread else "within three times the off runs' spread: no difference"
    print(f"on - off = {diff:+.0f} GCUPS ({100 * diff / np.median(off):+.1f} %), 3 x off spread = {3 * spread:.0f}: {verdict}", flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--pairs", type=int, default=4 << 20)
    ap.add_argument("--lanes", type=int, default=8)
    ap.add_argument("--leg", choices=("independent", "regions"))
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds a leg's child process may take")
    args = ap.parse_args()
    if args.leg:
        return run_leg(args.leg, args.rounds, args.pairs, args.lanes)
    for leg in ("independent", "regions"):
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--rounds", str(args.rounds),
               "--pairs", str(args.pairs), "--lanes", str(args.lanes)]
        rc = subprocess.call(cmd)
        if rc:
            print(f"leg {leg} ended with status {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
