"""Shared restatements and cases for the realignment tests (tests/test_best_allele_host.py, tests/test_realign_gpu.py); not a test.

* ``search_best_allele``: AlleleLikelihoods::searchBestAllele(sample, r, canBeReference = true, priorities) restated sequentially, line for
  line (utils/genotyper/AlleleLikelihoods.h:92-146), second-best bookkeeping included, on the values after switchToNaturalLog
  (:462-476, MathUtils.cpp:16-18: log10 * std::log(10)) with the threshold 0.2 * std::log(10) (PairHMMLikelihoodCalculationEngine.cpp:23).
* ``last_index_of``: Mutect2Utils::lastIndexOf (Mutect2Utils.cpp:69-82) is bytes.rfind.
* ``compose``: (best, keep, sequences) -> expected (cigar, offset, score) per read through a Smith-Waterman oracle, with
  SWNativeAlignerWrapper's shortcut (smithwaterman/SWNativeAlignerWrapper.cpp:10-31).
* ``rule_rows``: the rows both best-allele tests use.
"""
import math

import numpy as np

LN10 = math.log(10)
assert LN10.hex() == "0x1.26bb1bbb55516p+1"          # what csrc/best_allele_rule.h multiplies by
THRESHOLD = 0.2 * LN10
NEG_INF = float("-inf")
SOFTCLIP, INDEL, LEADING_INDEL, IGNORE = 9, 10, 11, 12
TO_BEST_HAPLOTYPE = (10, -15, -30, -5)
NOT_ALIGNED = -2 ** 31
WIDTHS = (1, 2, 63, 64, 65, 129)


def search_best_allele(log10_row, priorities):
    """-> bestAlleleIndex.  priorities None: the overload without tie-breaking (AlleleLikelihoods.h:148-150)."""
    values = [float(x) * LN10 for x in log10_row]                     # switchToNaturalLog
    allele_count = len(values)
    if allele_count == 0:                                             # :94
        return -1
    best_allele_index = 0                                             # :99, canBeReference
    second_best_index = 0
    best_likelihood = values[best_allele_index]
    second_best_likelihood = NEG_INF
    for a in range(best_allele_index + 1, allele_count):              # :105-119
        candidate_likelihood = values[a]
        if candidate_likelihood > best_likelihood:
            second_best_index = best_allele_index
            best_allele_index = a
            second_best_likelihood = best_likelihood
            best_likelihood = candidate_likelihood
        elif candidate_likelihood > second_best_likelihood:
            second_best_index = a
            second_best_likelihood = candidate_likelihood
    if priorities is not None and best_likelihood - second_best_likelihood < THRESHOLD:      # :121 (inf - inf is a NaN: false)
        best_priority = priorities[best_allele_index]
        second_best_priority = priorities[second_best_index]
        for a in range(allele_count):                                 # :124-140
            candidate_likelihood = values[a]
            if a == best_allele_index or best_likelihood - candidate_likelihood > THRESHOLD:
                continue
            candidate_priority = priorities[a]
            if candidate_priority > best_priority:
                second_best_index = best_allele_index
                best_allele_index = a
                second_best_priority = best_priority
                best_priority = candidate_priority
            elif candidate_priority > second_best_priority:
                second_best_index = a
                second_best_priority = candidate_priority
    return best_allele_index


def last_index_of(ref, alt):
    return bytes(ref).rfind(bytes(alt))


def compose(sw_oracle, haps, reads, best, keep, strategy=SOFTCLIP, params=TO_BEST_HAPLOTYPE):
    """haps, reads: lists of bytes; -> (cigars, offsets, scores, n_verbatim) as mgx_realign_regions defines them"""
    cig, off, sc, n_verbatim = [], [], [], 0
    for r, read in enumerate(reads):
        if not keep[r]:
            cig.append(b""); off.append(NOT_ALIGNED); sc.append(0)
            continue
        hap = haps[int(best[r])]
        at = last_index_of(hap, read) if strategy in (SOFTCLIP, IGNORE) else -1
        if at >= 0:
            n_verbatim += 1
            cig.append(b"%dM" % len(read)); off.append(at); sc.append(len(read) * params[0])
        else:
            c, o, s = sw_oracle.align(np.frombuffer(hap, dtype=np.uint8), np.frombuffer(read, dtype=np.uint8), params, strategy)
            cig.append(c); off.append(o); sc.append(s)
    return cig, np.array(off, dtype=np.int64), np.array(sc, dtype=np.int64), n_verbatim


def sequences(d):
    """(haplotypes, reads) of a region dict as lists of bytes"""
    ro, ho = d["read_off"].astype(np.int64), d["hap_off"].astype(np.int64)
    b, h = np.asarray(d["bases"], dtype=np.uint8).tobytes(), np.asarray(d["hap_bases"], dtype=np.uint8).tobytes()
    return [h[ho[k]:ho[k + 1]] for k in range(len(ho) - 1)], [b[ro[k]:ro[k + 1]] for k in range(len(ro) - 1)]


# ---- rows for the rule --------------------------------------------------------------------------------------------
def _value_rows(n, rng):
    """(name, log10 values) of width n"""
    top = -3.25
    rows = [("all -inf", np.full(n, NEG_INF)), ]
    one = np.full(n, NEG_INF); one[rng.randint(n)] = -7.5
    rows.append(("one finite", one))
    dup = -4.0 - rng.randint(0, 40, n) / 8.0
    dup[rng.choice(n, size=min(n, 3), replace=False)] = top
    rows.append(("duplicates of the maximum", dup))
    # gaps of exactly 0.2 in log10, and one ulp either side of it; the rest clearly beyond the threshold
    gap = np.full(n, top - 1.0 - rng.randint(0, 8, n) / 4.0)
    exact = top - 0.2
    marks = [top, exact, np.nextafter(exact, 0.0), np.nextafter(exact, -10.0)]
    for a, mark in zip(rng.permutation(n), marks):
        gap[a] = mark
    rows.append(("gaps of 0.2 and an ulp either side", gap))
    # a normalised row: many values sit exactly on the cap (best - 4.5), many within the threshold, several exact ties
    cap = np.array([top, top, top - 0.125, top - 0.2, top - 0.25, top - 4.5, top - 4.5, top - 4.5])[rng.randint(0, 8, n)]
    rows.append(("capped with exact ties", cap))
    return rows


def _priority_rows(values, rng):
    """(name, priorities or None) for one row of values"""
    n = len(values)
    finite = np.where(np.isfinite(values))[0]
    b0 = int(np.argmax(values)) if len(finite) else 0
    out = [("null", None), ("all equal", np.full(n, 2.0)), ("negative", -1.0 - rng.randint(0, 4, n).astype(np.float64))]
    on_best = rng.randint(0, 3, n).astype(np.float64); on_best[b0] = 7.0
    out.append(("maximum on the likelihood-best", on_best))
    # the maximum priority on two alleles inside the threshold where the row has them (candidates), else on any two others
    nat = [float(x) * LN10 for x in values]
    near = [a for a in range(n) if a != b0 and not (nat[b0] - nat[a] > THRESHOLD)]
    pool = near if len(near) >= 2 else [a for a in range(n) if a != b0]
    two = rng.randint(0, 3, n).astype(np.float64)
    for a in (rng.choice(pool, size=min(2, len(pool)), replace=False) if pool else []):
        two[a] = 9.0
    out.append(("maximum on two candidates", two))
    return out


def rule_rows(seed=20240607):
    """[(name, log10 values float64 [n], priorities float64 [n] or None)]: every width x every kind of row x every kind of priorities,
    then random rows with integer priorities, -inf entries and gaps around 0.2."""
    rng = np.random.RandomState(seed)
    rows = []
    for n in WIDTHS:
        for vname, v in _value_rows(n, rng):
            for pname, p in _priority_rows(v, rng):
                rows.append((f"{n}: {vname} / {pname}", np.asarray(v, dtype=np.float64), p))
    steps = np.array([0.0, 0.2, np.nextafter(0.2, 0.0), np.nextafter(0.2, 1.0), 0.1, 0.3, 4.5])
    for k in range(400):
        n = int(rng.randint(1, 10)) if k % 4 else int(rng.choice(WIDTHS))
        top = -float(rng.randint(1, 200)) / 8.0
        v = top - steps[rng.randint(0, len(steps), n)]
        v[rng.rand(n) < 0.1] = NEG_INF
        rows.append((f"random {k}", v.astype(np.float64), rng.randint(-2, 4, n).astype(np.float64)))
    return rows
