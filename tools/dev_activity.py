"""mgx_activity_interval on one MI355X over a 1 Mbp interval at depths 30 and 300 (synth.gen_activity_interval; depth 300 is the depth-30
read set with every read ten times): one warm-up, then --rounds rounds; medians and max - min of the call's wall time and of the two
kernels' times (HIP events of a timing call), the kernels' algorithmic bytes (the reads' arrays once, one element byte written and read
twice) over those times, and next to them the serial single-thread host pass of csrc/activity_rule.h (tools/activity_host_pass.cpp),
whose outputs the device's are compared with.  The host pass is a yardstick for scale, not a criterion.  Needs an MI355X.

    python tools/dev_activity.py [--out profiles/activity_ab.txt] [--rounds 6] [--loci 1000000] [--build-only]
"""
import argparse
import ctypes as C
import importlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKGDIR = os.path.join(ROOT, "fast-genomic-data-processing_amd")
HOST = os.path.join(ROOT, "tools", "bin", "libactivity_host.so")
READ_LEN = (100, 151)


def build():
    os.makedirs(os.path.dirname(HOST), exist_ok=True)
    src = os.path.join(ROOT, "tools", "activity_host_pass.cpp")
    deps = [src, os.path.join(PKGDIR, "csrc", "activity_rule.h"), os.path.join(PKGDIR, "csrc", "activity_profile_rule.h"), os.path.join(PKGDIR, "csrc", "mgx_tables.cpp")]
    if os.path.exists(HOST) and os.path.getmtime(HOST) >= max(os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKGDIR, "csrc"), src,
                           os.path.join(PKGDIR, "csrc", "mgx_tables.cpp"), "-o", HOST])


def repeated(d, k):
    """every read k times in a row: the order of act_start is kept"""
    out = dict(d)
    n = len(d["read_start"])
    for key in ("read_start", "flags", "mate_start", "sample", "act_start", "act_stop"):
        out[key] = np.repeat(d[key], k)
    for off, flats in (("cigar_off", ("cigar",)), ("base_off", ("bases", "quals"))):
        lens = np.diff(d[off].astype(np.int64))
        idx = np.repeat(np.arange(n), k)
        starts = d[off][:-1].astype(np.int64)[idx]
        new_lens = lens[idx]
        out[off] = np.concatenate([[0], np.cumsum(new_lens)]).astype(np.uint64)
        gather = np.repeat(starts - out[off][:-1].astype(np.int64), new_lens) + np.arange(int(new_lens.sum()))
        for f in flats:
            out[f] = d[f][gather]
    return out


def stat(xs):
    return "%.3f ms (spread %.3f)" % (float(np.median(xs)), max(xs) - min(xs))


def measure(pkg, host, name, d, rounds):
    act = pkg.ActivityEngine(0)
    inp, hold = pkg.activity.make_input(d)
    n = int(inp.n_loci)
    plain, timed = act.params(has_normal=1), act.params(has_normal=1, flags=pkg.activity.TIMING)
    outs = {k: (np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.uint32)) for k in ("device", "host")}
    ptrs = {k: [a.ctypes.data_as(C.c_void_p) for a in v] for k, v in outs.items()}

    def device(p):
        t0 = time.perf_counter()
        pkg.native.check(act.lib.mgx_activity_interval(act.ctx, C.byref(inp), C.byref(p), *ptrs["device"]))
        return (time.perf_counter() - t0) * 1e3
    device(plain)                                                             # the warm-up
    wall = [device(plain) for _ in range(rounds)]
    ms_el, ms_lo = [], []
    for _ in range(rounds):
        device(timed)
        st = act.stats()
        ms_el.append(st["ms_elements"]); ms_lo.append(st["ms_locus"])
    st = act.stats()
    host.activity_host_pass(C.byref(inp), C.byref(plain), 65535, *ptrs["host"])          # the warm-up (builds its tables)
    t_host = []
    for _ in range(max(1, rounds // 3)):
        t0 = time.perf_counter(); host.activity_host_pass(C.byref(inp), C.byref(plain), 65535, *ptrs["host"]); t_host.append((time.perf_counter() - t0) * 1e3)
    same = (np.array_equal(outs["device"][0], outs["host"][0]), np.array_equal(outs["device"][2], outs["host"][2]),
            float(np.nanmax(np.abs(outs["device"][1] - outs["host"][1]), initial=0.0)), np.array_equal(np.isnan(outs["device"][1]), np.isnan(outs["host"][1])))
    n_reads, n_el = len(d["read_start"]), int(st["n_elements"])
    read_bytes = n_reads * (4 * 4 + 2 + 1) + len(d["cigar"]) * 4 + 2 * len(d["bases"]) + n
    b_el, b_lo = read_bytes + n_el, 2 * n_el + n_reads * 20 + n * 13          # elements: the reads' arrays once + one byte written; loci: the byte read twice, the windows, the outputs
    lines = [f"== {name}: {n} loci, {n_reads} reads, {n_el} pileup elements, mean depth {n_el / max(n, 1):.1f}, {int(st['n_active'])} active, {int(st['n_callable'])} callable",
             f"mgx_activity_interval, wall time of the call     {stat(wall)}",
             f"  k_pileup_elements (HIP events)                 {stat(ms_el)}; algorithmic bytes {b_el / 1e6:.1f} MB -> {b_el / 1e6 / float(np.median(ms_el)):.1f} GB/s",
             f"  k_locus_activity  (HIP events)                 {stat(ms_lo)}; algorithmic bytes {b_lo / 1e6:.1f} MB -> {b_lo / 1e6 / float(np.median(ms_lo)):.1f} GB/s",
             f"serial host pass of activity_rule.h, one thread  {stat(t_host)}",
             f"device against host pass: active identical {same[0]}, depth identical {same[1]}, NaN pattern identical {same[3]}, max |log-odds difference| {same[2]:.3g}", ""]
    act.close()
    del hold
    print("\n".join(lines), flush=True)
    return lines


def measure_regions(pkg, host, name, d, rounds):
    """interval_regions (reads to regions, one call) against interval + the header's serial profile pass on the host: wall times, the two
    new kernel groups' times (HIP events), the bytes each way downloads, the regions compared"""
    act = pkg.ActivityEngine(0)
    n = len(d["ref_bases"])
    contig = int(d["interval_start"]) + n + 1000

    def wall(f):
        t0 = time.perf_counter(); out = f(); return (time.perf_counter() - t0) * 1e3, out
    fused = lambda: act.interval_regions(d, contig, per_locus=False, profile=False, has_normal=1)
    wall(fused)                                                               # the warm-up
    t_fused = [wall(fused)[0] for _ in range(rounds)]
    ms_band, ms_cut = [], []
    for _ in range(rounds):
        act.interval_regions(d, contig, per_locus=False, profile=False, region_params=dict(flags=pkg.activity.TIMING), has_normal=1)
        st = act.region_stats()
        ms_band.append(st["ms_band"]); ms_cut.append(st["ms_cut"])
    regions = fused()[0]
    rp, _ = act.region_params()
    out = np.zeros((n + 1, 4), np.int32)

    def two_steps():
        active = act.interval(d, has_normal=1)[0]
        k = host.activity_profile_host_pass(int(d["interval_start"]), n, active.ctypes.data_as(C.c_void_p), contig, C.byref(rp), out.ctypes.data_as(C.c_void_p))
        return out[:k]
    wall(two_steps)
    t_two = [wall(two_steps)[0] for _ in range(rounds)]
    same = np.array_equal(two_steps(), regions)
    st = act.region_stats()
    lines = [f"== {name}: {n} loci, {len(d['read_start'])} reads; {int(st['n_states'])} states, {int(st['n_runs'])} runs, {len(regions)} regions",
             f"mgx_activity_interval_regions, wall time of the call              {stat(t_fused)}; downloads {16 * len(regions) + 512} bytes",
             f"  k_band_pass (HIP events)                                        {stat(ms_band)}",
             f"  runs, k_cut_runs, regions (HIP events, one small download in)   {stat(ms_cut)}",
             f"mgx_activity_interval + serial host pass of the profile rule      {stat(t_two)}; downloads {13 * n} bytes",
             f"regions identical {same}", ""]
    act.close()
    print("\n".join(lines), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "activity_ab.txt"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--loci", type=int, default=1_000_000)
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--regions-out", default=os.path.join(ROOT, "profiles", "activity_regions_ab.txt"))
    ap.add_argument("--regions-only", action="store_true")
    a = ap.parse_args()
    build()
    if a.build_only:
        return 0
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("fast-genomic-data-processing_amd")
    host = C.CDLL(HOST)
    host.activity_host_pass.restype = C.c_int
    host.activity_host_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    mean_len = (READ_LEN[0] + READ_LEN[1]) / 2
    base = pkg.synth.gen_activity_interval(int(a.loci * 30 / mean_len), a.loci, 0xAC7, len_range=READ_LEN)
    text = ["mgx_activity_interval on one MI355X: one interval per call, one warm-up, then %d rounds; median and max - min." % a.rounds,
            "HBM bytes by hardware counters: not measured; the bytes below are what the algorithm needs.", ""]
    host.activity_profile_host_pass.restype = C.c_int64
    host.activity_profile_host_pass.argtypes = [C.c_int32, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    rtext = ["Reads to regions on one MI355X: one interval per call, one warm-up, then %d rounds; median and max - min." % a.rounds, ""]
    for name, d in (("depth 30", base), ("depth 300", repeated(base, 10))):
        if not a.regions_only:
            text += measure(pkg, host, name, d, a.rounds)
        rtext += measure_regions(pkg, host, name, d, a.rounds)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if not a.regions_only:
        with open(a.out, "w") as f:
            f.write("\n".join(text))
    with open(a.regions_out, "w") as f:
        f.write("\n".join(rtext))
    return 0


if __name__ == "__main__":
    sys.exit(main())
