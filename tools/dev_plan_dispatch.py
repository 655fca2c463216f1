"""Development driver: the fixed dispatch script of profiles/pairhmm_plan_refactor_ab.txt section 3.  Run it under
`rocprofv3 --kernel-trace ... -- python3 tools/dev_plan_dispatch.py DIR`, DIR being the directory that holds the package to load (the
repository, or a copy of another revision's package with its built library), and compare the kernel traces of two libraries: kernel,
Grid_Size_X / Workgroup_Size_X and Workgroup_Size_X in start order per stream.  The sections -- the fixed ragged batch and the 6-region
call of tests/pairhmm_plan_cases.py, region() with a model, a pair batch on a WIRE context, a 3-lane queue over 20 batches -- are
separated by one pairhmm_best_allele_rows dispatch; the queue's section compares as a multiset.  Prints sha256 of every section's outputs."""
import ctypes as C
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("fast-genomic-data-processing_amd")
import pairhmm_plan_cases as cases  # noqa: E402

print("library:", pkg.native.lib_path(), flush=True)
synth = pkg.synth
eng = pkg.PairHMMEngine(0)
lib = eng.lib
digest = {}


def sha(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    digest[name] = h.hexdigest()


def separator():
    off = np.zeros(1, dtype=np.uint64); nh = np.ones(1, dtype=np.uint32); v = np.zeros(1); best = np.zeros(1, dtype=np.int32)
    rc = lib.mgx_pairhmm_best_alleles(eng.ctx, C.c_uint64(1), off.ctypes.data_as(C.c_void_p), nh.ctypes.data_as(C.c_void_p),
                                      v.ctypes.data_as(C.c_void_p), None, best.ctypes.data_as(C.c_void_p))
    assert rc == 0


lib.mgx_pairhmm_best_alleles.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 5
lib.mgx_pairhmm_best_alleles.restype = C.c_int

# 1. the fixed ragged batch
rl, hl = cases.fixed_pairs()
d = cases.make_batch(rl, hl, 11)
b = eng.batch(d); b.run(); out, used = b.results(with_flags=True); st = b.stats(); b.close()
sha("fixed_pairs", out, used)
print("fixed_pairs stats", {k: st[k] for k in ("n_pairs", "cells", "alg_bytes", "n_rerun_f64", "n_launches_f32", "n_launches_f64", "n_exact", "n_nhap_f32")}, flush=True)
separator()
# 2. the 6-region call
regs = [cases.make_batch(r, h, 20 + k, pairs=False) for k, (r, h) in enumerate(cases.fixed_regions())]
outs = eng.compute_regions(regs)
sha("fixed_regions", *outs)
separator()
# 3. region() with a model
d3 = synth.gen_pairhmm_region(40, 25, 31, r_range=(90, 151), h_range=(150, 400))
o3, k3 = eng.region(d3, np.full(40, 60, dtype=np.uint8))
sha("region_model", o3, k3)
separator()
# 4. a pair batch on a wire context
weng = pkg.PairHMMEngine(0, flags=pkg.pairhmm.WIRE)
d4 = synth.gen_pairhmm_pairs(6000, 41, r_range=(1, 128), h_range=(1, 256), hap_n_rate=0.01)
b = weng.batch(d4); b.run(); o4, u4 = b.results(with_flags=True); b.close()
sha("wire_pairs", o4, u4)
weng.close()
separator()
# 5. a 3-lane queue over 20 small batches
d5 = synth.gen_pairhmm_pairs(20 * 2000, 51, r_range=(1, 128), h_range=(1, 256))
q = pkg.pairhmm.PairHMMQueue(devices=(0,), lanes_per_device=3, depth=2, batch_pairs=2000)
o5, u5 = q.run(d5, with_flags=True)
sha("queue_pairs", o5, u5)
q.close()
separator()
eng.close()
for k, v in digest.items():
    print("sha256", k, v)
