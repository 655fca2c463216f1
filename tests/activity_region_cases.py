"""Cases for the active regions on the device (mgx_activity_profile_regions / mgx_activity_interval_regions) and a Python restatement of
the reference's streaming code, statement by statement: BandPassActivityProfile::processState, ActivityProfile::add /
incorporateSingleState / popReadyAssemblyRegions / popReadyAssemblyRegion / findEndOfRegion / findFirstActivityBoundary / findBestCutSite /
isMinimum, driven as M2/main.cpp:267-328 drives them, with a pop attempt in front of every locus and the forced pops behind the last.
It is the witness the rule header and the device are held against.

A case: name, interval_start, prob (float64 per locus), contig_length, params (max_prob_propagation, active_prob_threshold, padding,
min_region_size, max_region_size) and weights: None = the reference's default band (F = 50; a test passes the same weight array to the
code under test and to the restatement, so that no machine's libm enters a comparison) or an explicit odd-length list.
"""
import hashlib
import math

import numpy as np

DEFAULTS = dict(max_prob_propagation=50, active_prob_threshold=0.002, padding=100, min_region_size=50, max_region_size=300)
SIZES = ((50, 300), (1, 20), (10, 60), (2, 2))
MAX_FILTER, SIGMA = 50, 17.0
BAND_TILE = 256          # MGX_ACTIVITY_BAND_TILE
CONTIG = 1 << 20
IDENTITY = (1.0,)        # F = 0: the smoothed value is the probability itself, so a cutter case writes its state values directly


# ---- the reference, restated ------------------------------------------------------------------------------------------------------------
def normal_distribution(mean, sd, x):
    return math.exp(-(x - mean) * (x - mean) / (2.0 * sd * sd)) / (sd * math.sqrt(2.0 * math.pi))


def make_kernel(filter_size, sigma):
    band = (filter_size << 1) + 1
    kernel = [normal_distribution(float(filter_size), sigma, float(i)) for i in range(band)]
    total = 0.0
    for e in kernel:
        total += e
    return [e / total for e in kernel]


def determine_filter_size(kernel, min_prob):
    middle = (len(kernel) - 1) >> 1
    end = middle
    while end > 0:
        if kernel[end - 1] < min_prob:
            break
        end -= 1
    return middle - end


def default_weights():
    """with this machine's libm"""
    f = determine_filter_size(make_kernel(MAX_FILTER, SIGMA), 1e-5)
    return make_kernel(f, SIGMA)


class Profile:
    """ActivityProfile with BandPassActivityProfile's processState; states are [position, value]"""

    def __init__(self, max_prob_propagation, threshold, weights, contig_length):
        self.state_list = []
        self.max_prob_propagation, self.threshold, self.contig_length = max_prob_propagation, threshold, contig_length
        self.kernel, self.filter_size = list(weights), (len(weights) - 1) // 2
        self.region_start = self.region_stop = None
        self.popped = {}          # position -> the value its state left the list with

    def is_empty(self):
        return not self.state_list

    def add(self, pos, prob):
        if self.region_start is None:
            self.region_start = self.region_stop = pos
        else:
            assert self.region_stop == pos - 1
            self.region_stop = pos
        for loc, value in self.process_state(pos, prob):
            self.incorporate_single_state(loc, value)

    def process_state(self, pos, prob):
        if prob > 0.0:
            out = []
            for i in range(-self.filter_size, self.filter_size + 1):
                loc = pos + i
                if not (loc < 0 or loc >= self.contig_length):
                    out.append((loc, prob * self.kernel[i + self.filter_size]))
            return out
        return [(pos, prob)]

    def incorporate_single_state(self, loc, value):
        size = len(self.state_list)
        position = loc - self.region_start
        if position >= 0:
            if position < size:
                self.state_list[position][1] = self.state_list[position][1] + value
            else:
                self.state_list.append([loc, value])

    def pop_ready_regions(self, extension, min_size, max_size, force):
        regions = []
        while True:
            got = self.pop_ready_region(extension, min_size, max_size, force)
            if got is None:
                return regions
            if got[4]:
                regions.append(got[:4])

    def pop_ready_regions_through_inactive(self, extension, min_size, max_size, force):
        """NOT the reference: goes on behind a dropped inactive piece, as a rule that takes a piece's pop time from its start alone does"""
        regions = []
        while True:
            before = len(self.state_list)
            got = self.pop_ready_region(extension, min_size, max_size, force)
            if got is None:
                if len(self.state_list) == before:
                    return regions
            elif got[4]:
                regions.append(got[:4])

    def pop_ready_region(self, extension, min_size, max_size, force):
        """None: nothing ready, or an inactive region was dropped (the reference returns nullptr for both, which ends the caller's loop)"""
        if not self.state_list:
            return None
        first = self.state_list[0]
        is_active = first[1] > self.threshold
        end_offset = self.find_end_of_region(is_active, min_size, max_size, force)
        if end_offset == -1:
            return None
        for loc, value in self.state_list[:end_offset + 1]:
            self.popped[loc] = value
        del self.state_list[:end_offset + 1]
        if not self.state_list:
            self.region_start = self.region_stop = None
        else:
            self.region_start = self.state_list[0][0]
        if not is_active:
            return None
        start, end = first[0], first[0] + end_offset
        return (start, end, max(0, start - extension), min(self.contig_length - 1, end + extension), True)

    def find_end_of_region(self, is_active, min_size, max_size, force):
        if not force and len(self.state_list) < max_size + self.max_prob_propagation + self.filter_size:
            return -1
        end = self.find_first_activity_boundary(is_active, max_size)
        if is_active and end == max_size:
            end = self.find_best_cut_site(end, min_size)
        return end - 1

    def find_first_activity_boundary(self, is_active, max_size):
        n, end = len(self.state_list), 0
        while end < n and end < max_size:
            if (self.state_list[end][1] > self.threshold) != is_active:
                break
            end += 1
        return end

    def find_best_cut_site(self, end, min_size):
        min_i, min_p = end - 1, 1.7976931348623157e308
        i = min_i
        while i >= min_size - 1:
            cur = self.state_list[i][1]
            if cur < min_p and self.is_minimum(i):
                min_p, min_i = cur, i
            i -= 1
        return min_i + 1

    def is_minimum(self, index):
        if index == len(self.state_list) - 1:
            return False
        if index < 1:
            return False
        p = self.state_list[index][1]
        return p <= self.state_list[index + 1][1] and p < self.state_list[index - 1][1]


def restate(case, weights, clock=True, early_return=True):
    """(regions int32 [n, 4], state values float64) as main.cpp's loop over one contiguous stretch gives them.  clock=False is the wrong
    rule "smooth everything, then cut": no pop before the last locus is in.  early_return=False is the wrong rule that ignores the return
    of popReadyAssemblyRegions behind a dropped inactive piece."""
    p = case["params"]
    prof = Profile(p["max_prob_propagation"], p["active_prob_threshold"], weights, case["contig_length"])
    regions = []
    args = (p["padding"], p["min_region_size"], p["max_region_size"])
    for k, prob in enumerate(case["prob"].tolist()):
        pos = case["interval_start"] + k
        if clock and not prof.is_empty():
            regions += (prof.pop_ready_regions if early_return else prof.pop_ready_regions_through_inactive)(*args, False)          # pileup.getPosition() == getEnd() + 1: never forced
        prof.add(pos, prob)
    # the reference's `while (!isEmpty())` relies on a pop of an inactive region ending one round of popReadyAssemblyRegions
    while not prof.is_empty():
        regions += prof.pop_ready_regions(*args, True)
    n = len(prof.popped)
    values = np.array([prof.popped[case["interval_start"] + k] for k in range(n)], np.float64)
    return np.array(regions, np.int32).reshape(-1, 4), values


_RESTATED = {}


def restated(case, weights):
    """restate(), once per (case, weights) and shared; the results are not to be changed"""
    key = (case["name"], tuple(weights))
    if key not in _RESTATED:
        _RESTATED[key] = restate(case, weights)
    return _RESTATED[key]


def weights_of(case, default):
    return list(default) if case["weights"] is None else list(case["weights"])


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def case(name, prob, interval_start=1000, contig_length=CONTIG, weights=None, **params):
    return dict(name=name, interval_start=interval_start, prob=np.ascontiguousarray(prob, dtype=np.float64), contig_length=contig_length,
                weights=weights, params=dict(DEFAULTS, **params))


def spikes(n, at):
    p = np.zeros(n)
    p[list(at)] = 1.0
    return p


def band_cases():
    F, mx = 50, DEFAULTS["max_region_size"]
    out = [case("one locus, active", [1.0]), case("one locus, inactive", [0.0])]
    out += [case("active at the first locus, interval at %d" % a, spikes(120, [0]), interval_start=a) for a in (0, 700)]
    out += [case("active at the last locus, contig ends %d beyond" % d, spikes(80, [10, 79]), contig_length=1000 + 80 + d) for d in (0, 1, F - 1, F, F + 1, 500)]
    out += [case("two actives %d apart" % d, spikes(250, [60, 60 + d])) for d in (F, F + 1, 2 * F, 2 * F + 1)]
    out += [case("actives at the tile size %+d" % d, spikes(3 * BAND_TILE, [BAND_TILE + d, 2 * BAND_TILE + d])) for d in (-1, 0, 1)]
    out.append(case("all inactive", np.zeros(400)))
    out.append(case("all active over 3 max + 7 loci", np.ones(3 * mx + 7)))
    rng = np.random.default_rng(0xF4AC)
    out.append(case("fractional probabilities and 0.0", rng.choice([0.0, 0.0, 0.0, 1e-3, 0.0625, 0.3, 0.7, 1.0], size=500)))
    for w in ((0.25, 0.5, 0.25), (0.05, 0.1, 0.2, 0.3, 0.2, 0.1, 0.05)):
        out.append(case("caller's weights, F = %d" % (len(w) // 2), (rng.random(400) < 0.08).astype(np.float64), weights=w))
    return out


def run_values(rng, n):
    """n state values well above the threshold with many local minima"""
    return 0.125 + rng.integers(1, 7000, size=n) / 8192.0


def framed(run, lead=7, tail=60):
    return np.concatenate([np.zeros(lead), run, np.zeros(tail)])


def cutter_cases(mn, mx):
    tag = " (min %d, max %d)" % (mn, mx)
    rng = np.random.default_rng(0xC077 + 1000 * mn + mx)
    sizes = dict(min_region_size=mn, max_region_size=mx)

    def direct(name, prob, **kw):
        return case(name + tag, prob, weights=IDENTITY, **sizes, **kw)
    out = [direct("run of %d" % n, framed(run_values(rng, n))) for n in (mx - 1, mx, mx + 1, 2 * mx, 2 * mx + 1)]
    at_end = run_values(rng, mx)
    out.append(direct("run of max at the end of the profile", framed(at_end, tail=0)))
    out.append(direct("run of max, then inactive states", framed(at_end)))
    # one deep dip at index min - 1 (scanned) or min - 2 (not scanned), a shallower one further on
    for d, what in ((mn - 1, "min - 1"), (mn - 2, "min - 2")):
        v = np.full(mx + 10, 0.5)
        if mx > 3:
            v[min(mx - 2, mn + 3)] = 0.375
        if d >= 0:
            v[d] = 0.125
        out.append(direct("lowest minimum at index " + what, framed(v)))
    v = np.full(mx + 10, 0.5)
    v[[max(mn - 1, 1), mx - 1]] = 0.25
    out.append(direct("two equal minima", framed(v)))
    out.append(direct("flat plateau", framed(np.full(mx + 10, 0.5))))
    out.append(direct("no local minimum", framed(0.25 + np.arange(mx + 10) / 4096.0)))
    out.append(case("one run of 20 000 states" + tag, np.concatenate([np.zeros(3), 0.25 + rng.integers(0, 3 << 10, size=20000 - 100) / 4096.0, np.zeros(3)]), **sizes))
    gaps = []
    for _ in range(1500):
        gaps += [1.0] * int(rng.integers(1, 4)) + [0.0] * int(rng.integers(1, 3))
    out.append(direct("1 500 runs of 1 to 3 states", np.array([0.0] + gaps)))
    return out


HEAD = 46          # with the default band and threshold a run starts this many states before its first locus of probability 1


def clock_case(seed):
    """A long active stretch whose first piece would end at index max - 1 if the state at index max were final: a gap of inactive loci
    centred behind state s + max - 1 makes that state a local minimum by a margin below one weight K[0]."""
    rng = np.random.default_rng(seed)
    mx, F = DEFAULTS["max_region_size"], 50
    lead = int(rng.integers(F, F + 40))                  # the run starts at state lead - HEAD
    n = lead - HEAD + mx + 4 * F + int(rng.integers(0, 200))
    p = np.ones(n)
    p[:lead] = 0.0
    centre, half = lead - HEAD + mx, int(rng.integers(5, 35))
    p[centre - half:centre + half] = 0.0
    for k in rng.integers(centre - 2 * F, centre + 2 * F, size=int(rng.integers(0, 6))):
        p[k] = 0.0
    return case("pop clock, seed %d" % seed, p)


CLOCK_SEEDS = (3, 16, 20)          # found by tests/activity_region_cases.py::search_clock_seeds: the clocked and the unclocked rule differ


def search_clock_seeds(weights, want=3, start=0):
    found, seed = [], start
    while len(found) < want:
        c = clock_case(seed)
        if not np.array_equal(restate(c, weights)[0], restate(c, weights, clock=False)[0]):
            found.append(seed)
        seed += 1
    return tuple(found)


def delay_case(seed):
    """clock_case's shape with the run starting within F states of the profile's start and no positive locus among the s loci in front
    of locus s + max + F - 1: the inactive piece [0, s) and the run's first piece become ready at that same locus, the call drops the
    inactive piece and returns, and the first piece is cut one locus later, with the K[0] term of locus s + max + F in."""
    rng = np.random.default_rng(seed)
    mx, F = DEFAULTS["max_region_size"], 50
    s = int(rng.integers(1, 13))
    lead = s + HEAD
    n = s + mx + 4 * F + int(rng.integers(0, 200))
    p = np.ones(n)
    p[:lead] = 0.0
    centre, half = s + mx, int(rng.integers(5, 35))
    p[centre - half:centre + half] = 0.0
    for k in rng.integers(centre - 2 * F, centre + F - 2, size=int(rng.integers(0, 6))):
        p[k] = 0.0
    t1 = s + mx + F - 1
    p[t1 - s:t1] = 0.0
    p[t1] = p[t1 + 1] = 1.0
    return case("delayed pop, seed %d" % seed, p)


DELAY_SEEDS = (30, 49, 160)          # found by seeded search: restate(early_return=False) gives other regions


def delay_cases():
    return [delay_case(s) for s in DELAY_SEEDS]


def clock_cases():
    out = [clock_case(s) for s in CLOCK_SEEDS]
    # the same shape with the profile ending before the list ever holds max + propagation + F states: the forced pop sees final values
    mx, F = DEFAULTS["max_region_size"], 50
    p = np.ones(F + mx + 70)
    p[:F] = 0.0
    p[mx - 12:mx + 12] = 0.0
    out.append(case("forced pop at the end of a long run", p, contig_length=1000 + len(p)))
    return out


def body_case():
    """3 000 loci of 0 / 1: sparse singles and bursts"""
    rng = np.random.default_rng(0xB0D1)
    p = (rng.random(3000) < 0.004).astype(np.float64)
    for a in rng.integers(0, 2900, size=6):
        n = int(rng.integers(20, 700))
        p[a:a + n] = np.maximum(p[a:a + n], (rng.random(len(p[a:a + n])) < 0.35).astype(np.float64))
    return case("body of 3 000 loci", p)


_CASES = []


def all_cases():
    if not _CASES:
        out = band_cases()
        for mn, mx in SIZES:
            out += cutter_cases(mn, mx)
        _CASES.extend(out + clock_cases() + delay_cases() + [body_case()])
        names = [c["name"] for c in _CASES]
        assert len(set(names)) == len(names)
    return _CASES


def digest(case_list):
    h = hashlib.sha256()
    for c in case_list:
        h.update(c["name"].encode())
        h.update(repr((c["interval_start"], c["contig_length"], c["weights"], sorted(c["params"].items()))).encode())
        h.update(c["prob"].tobytes())
    return int.from_bytes(h.digest()[:4], "little")


def number(x):
    x = float(x)
    return "1" if x == 1.0 else "0" if (x == 0.0 and math.copysign(1.0, x) > 0) else x.hex()


def to_text(case_list, default_weights=None):
    """the form tests/cpp/activity_profile_rule_driver.cpp reads: per case
    'case interval_start n_loci contig_length max_prob_propagation threshold padding min max n_weights', 'W weights' (n_weights 0: the
    reader builds the default band), 'P probabilities'"""
    lines = []
    for c in case_list:
        p = c["params"]
        w = c["weights"] if c["weights"] is not None else (default_weights if default_weights is not None else ())
        lines.append("case %d %d %d %d %s %d %d %d %d" % (c["interval_start"], len(c["prob"]), c["contig_length"], p["max_prob_propagation"],
                                                          float(p["active_prob_threshold"]).hex(), p["padding"], p["min_region_size"], p["max_region_size"], len(w)))
        lines.append("W " + " ".join(float(x).hex() for x in w))
        lines.append("P " + " ".join(number(x) for x in c["prob"]))
    return "\n".join(lines) + "\n"


def parse_answers(text, case_list):
    """per case (regions int32 [n, 4], values float64, weights float64): 'R n', n lines of four numbers, 'V values', 'K weights', 'end'"""
    out, lines, at = [], text.splitlines(), 0
    for _ in case_list:
        n = int(lines[at].split()[1])
        assert lines[at].startswith("R ")
        regions = np.array([[int(x) for x in ln.split()] for ln in lines[at + 1:at + 1 + n]], np.int32).reshape(-1, 4)
        at += 1 + n
        assert lines[at].startswith("V") and lines[at + 1].startswith("K") and lines[at + 2] == "end", lines[at][:40]
        values = np.array([float.fromhex(x) for x in lines[at].split()[1:]], np.float64)
        weights = np.array([float.fromhex(x) for x in lines[at + 1].split()[1:]], np.float64)
        out.append((regions, values, weights))
        at += 3
    assert at == len(lines)
    return out
