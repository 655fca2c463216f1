"""The job layout of the Smith-Waterman library (csrc/sw_layout.h) on the CPU: tests/cpp/sw_layout_driver.cpp, built with -Werror under
AddressSanitizer + UBSan, prints the job table, the launches and the chunk cuts of a batch; this file checks them against what the
kernels index (restated here from the kernels' own address arithmetic), against the launch order the GPU tests go by
(sw_frontier.lane_groups) and against what the library reported for one fixed batch before the header existed
(sw_frontier.FIXED_STATS, measured through stats() on the device).  No GPU, nothing loaded into Python, all integer-exact."""
import os
import subprocess

import pytest

import sw_frontier as F

I16, HALF, STRIP = 0x200, 0x400, 0x800
JOB_KEYS = ("index", "out", "g", "rpl", "len1", "len2", "bt_off", "lr_off", "lc_off", "sc_off", "el_off")
CLASS_EDGE_REFS = sorted({32 * k + d for k in range(1, 65) for d in (-1, 0, 1)} | {2049, 4096, 4097})
ALTERNATES = (1, 2, 16, 17, 64, 65, 151, 4096, 4097, 32767)


class LayoutDriver:
    def __init__(self, workdir, sanitize=True):
        """sanitize=False: a plain build, for the GPU tests that only want the cuts (no sanitizer runs next to the device)"""
        self.exe = os.path.join(str(workdir), "sw_layout_san" if sanitize else "sw_layout_plain")
        how = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined"] if sanitize else ["-O2"]
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + how +
                              ["-I", F.CSRC, os.path.join(F.ROOT, "tests", "cpp", "sw_layout_driver.cpp"), "-o", self.exe])
        self.env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1") if sanitize else dict(os.environ)
        self.workdir, self.calls = str(workdir), 0

    def run(self, lens, strategies=None, params=F.STANDARD_NGS, paired=0, use16=1, limit=0, slices=0):
        """-> dict(layout, jobs, launches, cuts, slices); a cut or slice is (lo, hi, sum of the pairs' bounds, arena bytes, jobs)"""
        self.calls += 1
        path = os.path.join(self.workdir, f"batch_{self.calls}.txt")
        strategies = strategies or [F.STRATEGIES[q % 4] for q in range(len(lens))]
        with open(path, "w") as f:
            f.write("params %d %d %d %d\npaired %d\nuse16 %d\nlimit %d\nslices %d\n" % (*params, paired, use16, limit, slices))
            f.writelines("pair %d %d %d\n" % (l1, l2, st) for (l1, l2), st in zip(lens, strategies))
        res = subprocess.run([self.exe, path], capture_output=True, text=True, env=self.env, timeout=1800)
        os.unlink(path)
        assert res.returncode == 0 and not res.stderr, res.stdout[-1000:] + res.stderr[-4000:]
        out = dict(jobs=[], launches=[], cuts=[], slices=[])
        for line in res.stdout.splitlines():
            kind, *v = line.split()
            v = [int(x) for x in v]
            if kind == "layout":
                out["layout"] = dict(zip(("n_jobs", "bt_bytes", "n_pairs_i16", "n_pairs_strip", "n_strips"), v))
            elif kind == "job":
                out["jobs"].append(dict(zip(JOB_KEYS, v)))
            else:
                out[{"launch": "launches", "cut": "cuts", "slice": "slices"}[kind]].append(tuple(v))
        assert len(out["jobs"]) == out["layout"]["n_jobs"]
        return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return LayoutDriver(tmp_path_factory.mktemp("sw_layout"))


@pytest.fixture(scope="module")
def rule_driver(tmp_path_factory):
    return F.Driver(tmp_path_factory.mktemp("sw_i16_rule_for_layout"), sanitize=False)


def up16(x):
    return (x + 15) & ~15


def lanes(len1, rpl):
    return -(-len1 // rpl)


def regions_of(jobs):
    """what the kernels write of the back-trace arena, from their address arithmetic: {(kind, start): (bytes, [job indices])}.
    k_sw_fill / k_sw_fill_strip: slot (t * G + lane) of `slot` bytes, t = 1 .. steps, so (steps + 1) * G * slot bytes per strip, strip s
    at s * (len2 + 64) * 64 * 32; the strip kernel's boundary array has len2 + 1 entries of 8 bytes.  k_sw_fill16: the same with the
    lane group's longest sweep and most lanes and a slot of one word per four rows; lr[j * rpl + k] for j <= the longest sweep,
    lc[lane * rpl + k] for the group's lanes."""
    reg = {}

    def add(kind, start, size, x):
        old = reg.setdefault((kind, start), (size, []))
        assert old[0] == size, (kind, start, size, old)
        old[1].append(x)

    for x, J in enumerate(jobs):
        g, rpl = J["g"] & 0xFF, J["rpl"]
        if J["out"] < 0:
            continue
        if J["g"] & I16:
            A, B = (jobs[x - 1], J) if J["g"] & HALF else (J, jobs[x + 1])
            n_swp, n_lanes = max(A["len2"], B["len2"]), max(lanes(A["len1"], rpl), lanes(B["len1"], rpl))
            add("bt", J["bt_off"], (n_swp + n_lanes) * g * 4 * (-(-rpl // 4)), x)
            add("lr", J["lr_off"], (n_swp + 1) * rpl * 4, x)
            add("lc", J["lc_off"], n_lanes * rpl * 4, x)
        elif J["g"] & STRIP:
            full, slot = (J["len1"] - 1) // 2048, 32
            last = (J["len2"] + lanes(J["len1"] - 2048 * full, 32)) * 64 * slot
            add("bt", J["bt_off"], full * (J["len2"] + 64) * 64 * slot + last, x)
            add("bnd", J["lr_off"], (J["len2"] + 1) * 8, x)
        else:
            slot = rpl if rpl <= 2 else (rpl + 3) & ~3
            add("bt", J["bt_off"], (J["len2"] + lanes(J["len1"], rpl)) * g * slot, x)
    return reg


def check_layout(res, lens):
    jobs, arena = res["jobs"], res["layout"]["bt_bytes"]
    reg = regions_of(jobs)
    spans = sorted((start, start + size, kind, owners) for (kind, start), (size, owners) in reg.items())
    for (a0, a1, kind, owners), nxt in zip(spans, spans[1:] + [(arena,)]):
        assert a0 % 16 == 0 and a1 <= nxt[0], (kind, a0, a1, nxt[0], owners)          # aligned, inside the arena, disjoint from every other
    assert sum(up16(a1 - a0) for a0, a1, _, _ in spans) == arena                       # and the arena holds nothing else
    # sharing: exactly what the layout intends
    for (kind, start), (size, owners) in reg.items():
        assert len(owners) <= 2 and (len(owners) == 1 or (kind != "bnd" and owners[1] == owners[0] + 1 and owners[0] % 2 == 0)), (kind, owners)
    for x in range(0, len(jobs), 2):
        A, B = jobs[x], jobs[x + 1] if x + 1 < len(jobs) else None
        if not A["g"] & I16:
            continue
        assert not A["g"] & HALF and B["g"] & HALF and B["g"] & I16 and (A["g"] & 0xFF, A["rpl"]) == (B["g"] & 0xFF, B["rpl"])
        if A["out"] < 0:                 # a filler group owns nothing
            assert B["out"] < 0 and all(J[k] == 0 for J in (A, B) for k in ("len1", "len2", "bt_off", "lr_off", "lc_off"))
        elif B["out"] < 0:               # a filler partner: the pair's regions, nothing of its own
            assert B["len1"] == 0 and B["len2"] == 0 and all(A[k] == B[k] for k in ("bt_off", "lr_off", "lc_off"))
        else:
            assert A["bt_off"] == B["bt_off"] and A["len2"] >= B["len2"]
            assert (A["lr_off"] == B["lr_off"]) == ((A["len1"] - 1) // A["rpl"] == (B["len1"] - 1) // B["rpl"])      # both last rows in one lane
            assert (A["lc_off"] == B["lc_off"]) == (A["len2"] == B["len2"])
    # scores and elements: input order, len1 + len2 + 2 values and twice that
    real = sorted((J for J in jobs if J["out"] >= 0), key=lambda J: J["out"])
    assert [J["out"] for J in real] == list(range(len(lens))) and [(J["len1"], J["len2"]) for J in real] == [tuple(p) for p in lens]
    at = 0
    for J in real:
        assert J["sc_off"] == at and J["el_off"] == 2 * at
        at += J["len1"] + J["len2"] + 2
    return reg


def check_launches(res):
    jobs, launches = res["jobs"], res["launches"]
    assert [a for a, _, _ in launches] == [0] + [b for _, b, _ in launches[:-1]] and (launches[-1][1] if launches else 0) == len(jobs)
    kinds = []
    for a, b, m2 in launches:
        part, J0 = jobs[a:b], jobs[a]
        assert b > a and m2 == max(J["len2"] for J in part)
        if J0["g"] & I16:
            g = J0["g"] & 0xFF
            per_wave = 2 * (64 // g)
            assert all(J["g"] & I16 and J["g"] & 0xFF == g and (J["rpl"] > 16) == (J0["rpl"] > 16) for J in part)
            assert (b - a) % per_wave == 0
            for w in range(a, b, per_wave):          # a wavefront reads its class from its first job
                assert all(J["rpl"] == jobs[w]["rpl"] for J in jobs[w:w + per_wave])
            kinds.append(0)
        else:
            assert all((J["g"], J["rpl"]) == (J0["g"], J0["rpl"]) for J in part)
            kinds.append(2 if J0["g"] & STRIP else 1)
    assert kinds == sorted(kinds) and kinds.count(2) <= 1          # 16-bit launches, the 32-bit classes, the strip class last
    return len(launches)


def partners(res):
    return [(A["out"], B["out"] if B["out"] >= 0 else None) for A, B in zip(res["jobs"][::2], res["jobs"][1::2]) if A["g"] & I16 and A["out"] >= 0]


def spanning_batch(paired):
    """every 16-bit row class of the family at its shortest and its longest reference; alternates with ties and without"""
    lens = []
    for c, (r, lo, hi) in enumerate(F.class_lengths(paired)):
        lens += [(lo, 40 + c), (hi, 40), (hi, 40 + c), (lo, 40), (lo, 7)] + ([(hi, 40)] if c % 3 else [])
    return lens


@pytest.mark.parametrize("use16", [1, 0])
@pytest.mark.parametrize("paired", [0, 1])
def test_regions_and_launches(driver, paired, use16):
    lens = spanning_batch(paired) + [(2048, 700), (300, 4097), (2049, 1), (4097, 65), (9000, 300)] + list(F.FIXED_LENS)
    res = driver.run(lens, paired=paired, use16=use16)
    reg = check_layout(res, lens)
    check_launches(res)
    assert res["layout"]["n_pairs_strip"] == 3 + 2 and res["layout"]["n_strips"] == (2 + 3 + 5) + (2 + 3)       # FIXED_LENS holds two more
    assert (res["layout"]["n_pairs_i16"] > 0) == bool(use16)
    assert any(len(o) == 2 for (k, _), (_, o) in reg.items() if k == "lr") == bool(use16)          # every kind of share and of split occurs
    assert any(len(o) == 1 and res["jobs"][o[0]]["g"] & HALF for (k, _), (_, o) in reg.items() if k == "lc") == bool(use16)


@pytest.mark.parametrize("paired", [0, 1])
def test_an_odd_class_everywhere_stays_within_the_job_array(driver, paired):
    """one pair in every 16-bit class of the family (with MGX_SW_PAIRED the 64-lane classes hold the references over 1024 bases): every
    class is padded with the most fillers it can take.  The driver's job array holds n + 256 entries under ASan."""
    lens = [(hi, 30) for _, _, hi in F.class_lengths(bool(paired))] + ([(64 * r, 30) for r in (20, 24, 32)] if paired else [])
    res = driver.run(lens, paired=paired)
    check_layout(res, lens)
    check_launches(res)
    n_cls = len({(J["g"] & 0xFF, J["rpl"]) for J in res["jobs"]})
    assert res["layout"]["n_pairs_i16"] == len(lens) and n_cls == (18 + 3 if paired else 18)
    assert res["layout"]["n_jobs"] == sum(2 * (64 // (J["g"] & 0xFF)) for J in res["jobs"] if J["out"] >= 0) <= len(lens) + 256


@pytest.mark.parametrize("paired", [0, 1])
def test_launch_order_against_the_restatement(driver, rule_driver, paired):
    """sw_frontier.lane_groups is what the GPU frontier tests go by: the partners it predicts are the partners the header pairs"""
    for params in (F.STANDARD_NGS, F.FLAT):
        lens = spanning_batch(paired) + [(2048, 700), (64, 4097), (200, 4096)]
        res = driver.run(lens, params=params, paired=paired)
        adm = rule_driver.admitted(params, lens)
        assert partners(res) == F.lane_groups(lens, adm, bool(paired)) and 0 < sum(adm) < len(lens)
        assert res["layout"]["n_pairs_i16"] == sum(adm)
        assert {(J["g"] & 0xFF, J["rpl"]) for J in res["jobs"] if J["g"] & I16} == {F.shape16(l1, paired) for (l1, _), ok in zip(lens, adm) if ok}


@pytest.mark.parametrize("use16", [1, 0])
@pytest.mark.parametrize("paired", [0, 1])
def test_chunk_bound_covers_the_layout(driver, paired, use16):
    """The bound a chunk is cut by is at least what the chunk's layout takes: single pairs (a 16-bit one has a filler partner, and filler
    groups beside it), and lane groups of unequal partners (slices of two pairs, every reference under two alternates).  The bound only
    steers the cuts -- the arena is reserved at the layout's own size -- so this is about the formula not drifting from the layout,
    not about memory safety.  For a strip pair the bound is the pair's regions to the byte."""
    worst = 10.0
    for params in (F.STANDARD_NGS, F.ORIGINAL_DEFAULT):
        lens = [(n, m) for n in CLASS_EDGE_REFS for m in ALTERNATES]
        res = driver.run(lens, params=params, paired=paired, use16=use16, limit=1)
        assert [(lo, hi) for lo, hi, _, _, _ in res["cuts"]] == [(q, q + 1) for q in range(len(lens))]
        for (lo, hi, bound, arena, _), (n, m) in zip(res["cuts"], lens):
            assert bound >= arena and (n <= 2048 or bound == arena), (n, m, bound, arena)
            worst = min(worst, bound / arena if n <= 2048 else worst)
        lens = [(n, m) for n in CLASS_EDGE_REFS for k, m in enumerate(ALTERNATES) for n, m in ((n, m), (n - (n > 1), ALTERNATES[k - 1]))]
        res = driver.run(lens, params=params, paired=paired, use16=use16, slices=2)
        assert len(res["slices"]) == len(lens) // 2
        for lo, hi, bound, arena, n_jobs in res["slices"]:
            assert hi == lo + 2 and bound >= arena, (lens[lo:hi], bound, arena)
            worst = min(worst, bound / arena if lens[lo][0] <= 2048 else worst)
    print(f"paired {paired} use16 {use16}: smallest bound / layout of references up to 2048 bases = {worst:.3f}")


def test_chunk_cuts(driver):
    lens = [(1000, 500), (10, 10), (2048, 32767), (10, 10), (10, 10), (300, 150), (2049, 10), (64, 64)] * 3
    one = driver.run(lens[:1], limit=1 << 40)["cuts"]
    assert one == [(0, 1, one[0][2], one[0][3], one[0][4])]
    for limit in (1, 1 << 16, 1 << 20, 200 << 20, 1 << 40):
        res = driver.run(lens, limit=limit)
        cuts = res["cuts"]
        assert cuts[0][0] == 0 and cuts[-1][1] == len(lens) and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))       # [0, n) exactly
        assert all(hi > lo and bound >= arena for lo, hi, bound, arena, _ in cuts)
        assert all(bound <= limit or hi == lo + 1 for lo, hi, bound, _, _ in cuts)            # over the limit: a chunk of its own
        if limit == 1:
            assert len(cuts) == len(lens)
        if limit == 1 << 40:
            assert len(cuts) == 1 and cuts[0][3] == res["layout"]["bt_bytes"]
    # the pair after a cut would not have fitted
    res = driver.run(lens, limit=1 << 20)
    single = {q: b for q, _, b, _, _ in driver.run(lens, limit=1)["cuts"]}
    assert all(bound + single[hi] > 1 << 20 for _, hi, bound, _, _ in res["cuts"][:-1])


@pytest.mark.parametrize("knobs", sorted(F.FIXED_STATS), ids=str)
def test_the_fixed_batch_is_laid_out_as_the_library_reported(driver, knobs):
    """backtrace_bytes, n_launches, n_pairs_i16, n_pairs_strip, n_strips of sw_frontier.FIXED_LENS as stats() gave them on the device
    before the layout moved into the header; test_smithwaterman_gpu.py::test_stats_of_the_fixed_batch asserts the same of the library"""
    paired, use16 = knobs
    res = driver.run(list(F.FIXED_LENS), strategies=list(F.FIXED_STRATEGIES), paired=paired, use16=use16)
    check_layout(res, F.FIXED_LENS)
    L = res["layout"]
    assert (L["bt_bytes"], check_launches(res), L["n_pairs_i16"], L["n_pairs_strip"], L["n_strips"]) == F.FIXED_STATS[knobs]
