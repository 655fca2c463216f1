"""Row F2 at its seams: the cases of tests/test_read_model_host.py and tests/test_read_model_gpu.py, and a restatement of the two
steps in plain Python on bytes and ints.

The restatement follows the reference (haplotypecaller/PairHMMLikelihoodCalculationEngine.cpp:45-61, 149-272,
utils/variant/GATKVariantContextUtils.cpp:59-106, utils/genotyper/AlleleLikelihoods.h:153-166, 372-419), not
oracle/pairhmm_oracle.c: repeat units are ``bytes`` slices compared with ``==``.  The answers of the reference's own compiled
repeat search for exactly these cases are in tests/golden/read_model.npz (tests/golden/make_golden_read_model.py)."""
import functools
import hashlib
import math

import numpy as np

MAX_STR_UNIT_LENGTH = 8
MAX_REPEAT_LENGTH = 20
MIN_ADJUSTED_QSCORE = 10
INITIAL_QSCORE = 40.0
MIN_USABLE_Q_SCORE = 6

DEFAULT_MODEL = dict(pcr_rate_factor=3, base_quality_threshold=18, constant_gcp=10)


# ---- the restatement ------------------------------------------------------------------------------------------------------

def count_repetitions(unit, test, leading):
    """findNumberOfRepetitions(repeatUnit, testString, leadingRepeats): whole copies of ``unit`` at the front (leading) or at the
    back of ``test``"""
    if len(test) == 0:
        return 0
    n, step = 0, len(unit)
    diff = len(test) - step
    starts = range(0, diff + 1, step) if leading else range(diff, -1, -step)
    for start in starts:
        if test[start:start + step] != unit:
            break
        n += 1
    return n


def repeat_length(read, offset, trace=None):
    """findTandemRepeatUnits.  ``trace`` (a dict) receives which unit lengths ended a search (``decided``) and, where the two
    units differ, the backward count of the forward unit (``differ``)."""
    length = len(read)
    head = read[:offset + 1]
    max_bw, best_bw_unit = 0, read[offset:offset + 1]
    for k in range(1, MAX_STR_UNIT_LENGTH + 1):
        if offset + 1 - k < 0:
            break
        max_bw = count_repetitions(read[offset - k + 1:offset + 1], head, False)
        if max_bw > 1:
            best_bw_unit = read[offset - k + 1:offset + 1]
            if trace is not None:
                trace.setdefault("decided", set()).add(k)
            break
    max_rl = max_bw
    if offset < length - 1:
        tail = read[offset + 1:]
        max_fw, best_fw_unit = 0, read[offset + 1:offset + 2]
        for k in range(1, MAX_STR_UNIT_LENGTH + 1):
            if offset + k + 1 > length:
                break
            max_fw = count_repetitions(read[offset + 1:offset + k + 1], tail, True)
            if max_fw > 1:
                best_fw_unit = read[offset + 1:offset + k + 1]
                if trace is not None:
                    trace.setdefault("decided", set()).add(k)
                break
        if best_fw_unit == best_bw_unit:
            max_rl = max_fw + max_bw
        else:
            max_bw = count_repetitions(best_fw_unit, head, False)
            max_rl = max_fw + max_bw
            if trace is not None:
                trace["differ"] = max_bw
    return min(max_rl, MAX_REPEAT_LENGTH)


def fast_round(d):
    return int(d + 0.5) if d > 0.0 else int(d - 0.5)


def pcr_cache(rate):
    """pcrIndelErrorModelCache: the quality a repeat of 0..20 units caps ins / del at"""
    return [max(MIN_ADJUSTED_QSCORE, fast_round(INITIAL_QSCORE - math.exp(i / (rate * math.pi))) + 1) & 0xFF for i in range(MAX_REPEAT_LENGTH + 1)]


def restated_model(read, qual, ins, dele, gcp, mapq, rate, thr, gcp_const):
    """modifyReadQualities and the gap-continuation bytes of one read -> (qual, ins, dele, gcp) as bytes.  rate 0: no PCR model;
    gcp_const < 0: the caller's gcp."""
    qual, ins, dele = bytearray(qual), bytearray(ins), bytearray(dele)
    length = len(read)
    if rate:
        cache = pcr_cache(rate)
        for i in range(1, length):
            c = cache[repeat_length(read, i - 1)]
            ins[i - 1] = min(ins[i - 1], c)
            dele[i - 1] = min(dele[i - 1], c)
    for i in range(length):
        q = min(qual[i], mapq)
        qual[i] = MIN_USABLE_Q_SCORE if q < thr else q
        if ins[i] < MIN_USABLE_Q_SCORE:
            ins[i] = MIN_USABLE_Q_SCORE
        if dele[i] < MIN_USABLE_Q_SCORE:
            dele[i] = MIN_USABLE_Q_SCORE
    gcp = bytes(gcp) if gcp_const < 0 else bytes([gcp_const & 0xFF]) * length
    return bytes(qual), bytes(ins), bytes(dele), gcp


def restated_normalize_filter(rows, read_len, log10_rate, max_err):
    """normalizeLikelihoods and the filterPoorlyModeledEvidence decision.  ``rows``: one sequence of log10 values per read.
    -> (rows as a list of lists, capped as a list of lists of bool, keep as a list of 0 / 1)"""
    out, capped, keep = [], [], []
    for row, length in zip(rows, read_len):
        row = [float(x) for x in row]
        best = -math.inf
        for x in row:
            if x > best:
                best = x
        hit = [False] * len(row)
        if not math.isinf(log10_rate) and len(row) > 1:
            cap = best + log10_rate
            hit = [x < cap for x in row]
            row = [cap if h else x for x, h in zip(row, hit)]
        max_errors = min(2.0, float(math.ceil(int(length) * max_err)))
        keep.append(0 if best < max_errors * -4.0 else 1)
        out.append(row)
        capped.append(hit)
    return out, capped, keep


# ---- read-model cases -----------------------------------------------------------------------------------------------------

def _arr(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _letters(rng, n, alphabet=b"ACGT"):
    return bytes(_arr(alphabet)[rng.randint(0, len(alphabet), n)])


def _read(rng, bases, mapq=60, qual=None, ins=None, dele=None, gcp=None):
    n = len(bases)
    rnd = lambda lo, hi: bytes(rng.randint(lo, hi, n).astype(np.uint8))  # noqa: E731
    return dict(bases=bytes(bases), mapq=int(mapq), qual=rnd(2, 42) if qual is None else bytes(qual), ins=rnd(3, 60) if ins is None else bytes(ins),
                dele=rnd(3, 60) if dele is None else bytes(dele), gcp=rnd(0, 94) if gcp is None else bytes(gcp))


def _paste(bases, at, piece):
    assert 0 <= at and at + len(piece) <= len(bases)
    return bases[:at] + piece + bases[at + len(piece):]


# units of 1..9 bases without a period of their own
UNITS = [b"A", b"AC", b"ACG", b"ACGT", b"ACGTC", b"ACGTCT", b"ACGTCTG", b"ACGTCTGA", b"ACGTCTGAT"]
GAP_VALUES = [0, 5, 6, 7] + list(range(9, 42)) + [127, 128, 200, 255]


def _case(name, reads, **model):
    m = dict(DEFAULT_MODEL)
    m.update(model)
    return dict(name=name, reads=reads, model=m)


@functools.lru_cache(maxsize=None)
def model_cases():
    """Every case: a name, a list of reads (bases, qual, ins, dele, gcp as bytes, mapq) and the model they run under."""
    rng = np.random.RandomState(20240611)
    cases = []

    # lengths: the 128-thread stride and the 1024-base LDS staging limit
    reads = [_read(rng, _letters(rng, n, b"AC")) for n in (1, 2, 3, 127, 128, 129, 1100)]
    for n in (1023, 1024, 1025):
        b = _letters(rng, n)
        b = _paste(b, 3, b"G" + b"A" * 7 + b"C")
        b = _paste(b, 13, b"ACGT" * 4)
        b = _paste(b, n - 27, b"TGCA" * 4 + b"G")
        b = _paste(b, n - 8, b"C" + b"T" * 7)            # a homopolymer that ends with the read
        reads.append(_read(rng, b))
    cases.append(_case("lengths", reads))

    # unit lengths 1..8 as the deciding unit with 2 and 3 copies; 9 bases twice must not be found
    reads = []
    for unit in UNITS:
        for copies in (2, 3):
            if len(unit) == 9 and copies == 3:
                continue
            reads.append(_read(rng, b"TGCAG" + unit * copies + b"GTCAT", ins=[45] * (10 + len(unit) * copies), dele=[45] * (10 + len(unit) * copies)))
            reads.append(_read(rng, unit * copies, ins=[45] * (len(unit) * copies), dele=[45] * (len(unit) * copies)))
    cases.append(_case("unit_lengths", reads))

    # the cap of 20: totals of 19, 20, 21 and 40; the backward count has no inner cap
    reads = []
    for total in (19, 20, 21, 40):
        for unit in (b"A", b"AC", b"ACGTCTGA"):
            b = b"CG" + unit * total + b"GC"
            reads.append(_read(rng, b, ins=[45] * len(b), dele=[45] * len(b)))
    reads.append(_read(rng, b"T" * 1025))
    reads.append(_read(rng, b"T" * 1024))
    cases.append(_case("cap", reads))

    # read ends: offset 0, len - 2, len - 1 (the last base gets no PCR change)
    reads = []
    for b in (b"A", b"AA", b"AAA", b"AC", b"AAC", b"CAA", b"ACAC", b"AAAAACGT", b"TGCAAAAA", b"ACACACAC", b"ACGTACGT", b"ACGTACGTA", b"GACGTACGT"):
        reads.append(_read(rng, b, ins=[45] * len(b), dele=[45] * len(b)))
    cases.append(_case("read_ends", reads))

    # the forward unit differs from the backward unit
    reads = []
    for b in (b"TTCTTCCCC",              # the reference's own example: (TTC)2 behind, (C)3 ahead, one more C behind = 4
              b"ACACACCCC",              # the backward unit (AC)3 contains the forward unit C: one C behind
              b"AGAGAGCCC",              # it does not: no C behind, the backward count is 0
              b"ACGTTT",                 # the backward search stops where a unit would start before the read
              b"GTTTACGACG",             # ... with a repeat of its own ahead
              b"AAAACCCC", b"ACACGTGT", b"AACAACTTGTTG"):
        reads.append(_read(rng, b, ins=[45] * len(b), dele=[45] * len(b)))
        wide = b"GATC" + b + b"TCAG"
        reads.append(_read(rng, wide, ins=[45] * len(wide), dele=[45] * len(wide)))
    cases.append(_case("units_differ", reads))

    # bases are compared as bytes: lower case, N, bytes >= 128
    reads = []
    for b in (b"aaaaAAAA", b"acacACAC", b"AaAaAaAa", b"NNNNNNAN", b"ANANANNN", bytes([200] * 5 + [201, 200] * 3 + [72, 200]),
              bytes([65, 193] * 4 + [193] * 4), bytes([255] * 6 + [0] * 6), b"AC" * 3 + bytes([0xC1, 0x43]) * 3):
        reads.append(_read(rng, b, ins=[45] * len(b), dele=[45] * len(b)))
    cases.append(_case("bytes", reads))

    # base qualities against the threshold and MAPQ
    ramp = bytes([0, 5, 6, 7, 16, 17, 18, 19, 20, 29, 30, 31, 59, 60, 61, 93, 127, 128, 129, 200, 254, 255])
    flat30 = bytes([30] * len(ramp))
    reads = []
    for mapq, qual in ((60, ramp), (17, flat30), (18, flat30), (19, flat30), (0, ramp), (255, ramp), (254, ramp), (128, ramp), (127, ramp), (6, ramp), (5, ramp)):
        reads.append(_read(rng, _letters(rng, len(ramp), b"AC"), mapq=mapq, qual=qual))
    cases.append(_case("base_qualities", reads))
    cases.append(_case("base_qualities_thr6", reads, base_quality_threshold=6))

    # gap qualities: 0, 5, 6, 7, every value around the cache's, >= 128, at every repeat length the reads reach
    reads = []
    for k, n in enumerate((100, 141, 187)):
        b = _letters(rng, n, b"AC")
        b = _paste(b, 20, b"A" * (9 + 5 * k))
        ins = [GAP_VALUES[(i + k) % len(GAP_VALUES)] for i in range(n)]
        dele = [GAP_VALUES[(7 * i + 3 + k) % len(GAP_VALUES)] for i in range(n)]
        reads.append(_read(rng, b, ins=ins, dele=dele))
    for rate in (1, 2, 3):
        cases.append(_case("gap_qualities_rate%d" % rate, reads, pcr_rate_factor=rate))

    # the model's switches on one repeat-rich read set
    reads = [_read(rng, _paste(_letters(rng, n, b"AC"), 5, unit * copies))
             for n, unit, copies in ((40, b"A", 12), (60, b"AC", 9), (90, b"ACG", 5), (131, b"ACGTCTGA", 4), (257, b"T", 30), (33, b"GT", 3))]
    for rate, thr, gcp in ((0, 18, 10), (1, 18, 10), (2, 18, 10), (3, 18, -1), (3, 18, 0), (3, 6, 10), (1, 6, -1), (0, 6, -1)):
        cases.append(_case("model_rate%d_thr%d_gcp%d" % (rate, thr, gcp), reads, pcr_rate_factor=rate, base_quality_threshold=thr, constant_gcp=gcp))

    # body: 300 reads of 20..300 bases over two letters with pasted units
    reads = []
    for r in range(300):
        n = int(rng.randint(20, 301))
        b = _letters(rng, n, b"AC" if r % 3 else b"GT")
        for _ in range(int(rng.randint(0, 4))):
            unit = UNITS[int(rng.randint(len(UNITS)))]
            piece = (unit * int(rng.randint(2, 26)))[:n - 1]
            b = _paste(b, int(rng.randint(0, n - len(piece) + 1)), piece)
        reads.append(_read(rng, b, mapq=int(rng.randint(0, 61))))
    cases.append(_case("body", reads))
    return cases


def case_region(case, hap=b"ACGTTGCAAGCTTACGGATCCATGACGTTGCA"):
    """A case as a region for the engine and the oracle: its reads against one short haplotype (the recurrence is not what these
    cases are about).  -> (region dict with the explicit pair list, mapq)"""
    reads = case["reads"]
    ro = np.concatenate([[0], np.cumsum([len(r["bases"]) for r in reads])]).astype(np.uint64)
    d = {k: _arr(b"".join(r[k] for r in reads)).copy() for k in ("bases", "qual", "ins", "dele", "gcp")}
    d.update(read_off=ro, hap_off=np.array([0, len(hap)], dtype=np.uint64), hap_bases=_arr(hap).copy(),
             pair_read=np.arange(len(reads), dtype=np.uint32), pair_hap=np.zeros(len(reads), dtype=np.uint32))
    return d, np.array([r["mapq"] for r in reads], dtype=np.uint8)


def _hex(b):
    return bytes(b).hex() or "-"


def reads_text(cases):
    """the cases in the form oracle/_ref/ref_read_model reads them"""
    lines = []
    for c in cases:
        m = c["model"]
        lines.append("case %d %d %d %d" % (m["pcr_rate_factor"], m["base_quality_threshold"], m["constant_gcp"], len(c["reads"])))
        for r in c["reads"]:
            lines.append(" ".join([str(r["mapq"])] + [_hex(r[k]) for k in ("bases", "qual", "ins", "dele", "gcp")]))
    return "\n".join(lines) + "\n"


N_REPS = 100000


@functools.lru_cache(maxsize=None)
def reps_triples():
    """100 000 seeded (unit, test string, leading) triples over two letters: units of 1..9 bases, test strings of 0..64; half
    of the test strings hold whole copies of the unit at the end that is searched"""
    rng = np.random.RandomState(77)
    pool = _letters(rng, 1 << 16, b"AC")
    where = rng.randint(0, len(pool) - 128, (N_REPS, 2))
    unit_len = rng.randint(1, 10, N_REPS)
    test_len = rng.randint(0, 65, N_REPS)
    copies = rng.randint(0, 9, N_REPS)
    leading = rng.randint(0, 2, N_REPS)
    built = rng.randint(0, 2, N_REPS)
    out = []
    for i in range(N_REPS):
        unit = pool[where[i, 0]:where[i, 0] + unit_len[i]]
        test = pool[where[i, 1]:where[i, 1] + test_len[i]]
        if built[i]:
            rep = unit * int(copies[i])
            test = (rep + test if leading[i] else test + rep)
            test = test[:64] if leading[i] else test[-64:]
        out.append((unit, test, int(leading[i])))
    return out


def reps_text(triples):
    return "".join("%d %s %s\n" % (lead, _hex(unit), _hex(test)) for unit, test, lead in triples)


def digest():
    """of everything the golden file's answers were made for"""
    return hashlib.sha256((reads_text(model_cases()) + reps_text(reps_triples())).encode()).hexdigest()


def parse_reads_answers(text, cases):
    """the harness's output -> per case (cache or None, [(rl, qual, ins, dele, gcp) per read])"""
    lines = text.splitlines()
    at, out = 0, []
    unhex = lambda w: b"" if w == "-" else bytes.fromhex(w)  # noqa: E731
    for c in cases:
        head = lines[at].split(); at += 1
        assert head[0] == "cache"
        cache = None if head[1] == "-" else [int(x) for x in head[1:]]
        per_read = []
        for r in c["reads"]:
            w = lines[at].split(); at += 1
            got = tuple(unhex(x) for x in w)
            assert len(got) == 5 and all(len(g) == len(r["bases"]) for g in got)
            per_read.append(got)
        out.append((cache, per_read))
    assert at == len(lines)
    return out


GOLDEN_KEYS = ("rl", "qual", "ins", "dele", "gcp")


def golden_answers(z, cases):
    """tests/golden/read_model.npz (loaded) -> the shape parse_reads_answers gives"""
    flat = {k: bytes(z[k]) for k in GOLDEN_KEYS}
    at, out = 0, []
    for ci, c in enumerate(cases):
        cache = [int(x) for x in z["cache"][ci]] if c["model"]["pcr_rate_factor"] else None
        per_read = []
        for r in c["reads"]:
            n = len(r["bases"])
            per_read.append(tuple(flat[k][at:at + n] for k in GOLDEN_KEYS))
            at += n
        out.append((cache, per_read))
    assert all(at == len(flat[k]) for k in GOLDEN_KEYS)
    return out


@functools.lru_cache(maxsize=None)
def restated_answers():
    """the Python restatement on every case, in the shape parse_reads_answers gives (computed once per process)"""
    out = []
    for c in model_cases():
        m = c["model"]
        per_read = []
        for r in c["reads"]:
            rl = bytes(repeat_length(r["bases"], i) for i in range(len(r["bases"])))
            per_read.append((rl,) + restated_model(r["bases"], r["qual"], r["ins"], r["dele"], r["gcp"], r["mapq"], m["pcr_rate_factor"],
                                                   m["base_quality_threshold"], m["constant_gcp"]))
        out.append((pcr_cache(m["pcr_rate_factor"]) if m["pcr_rate_factor"] else None, per_read))
    return out


# ---- normalise / filter cases ---------------------------------------------------------------------------------------------

NF_MODEL = dict(DEFAULT_MODEL, log10_mismapping_rate=-4.5, max_error_per_base=0.02)
HAP_LEN = 110


def _other(rng, base):
    """a base of ACGT that is not ``base``"""
    return b"ACGT".replace(bytes([base]), b"")[int(rng.randint(3))]


def _mutate(rng, seq, positions):
    s = bytearray(seq)
    for p in positions:
        s[p] = _other(rng, s[p])
    return bytes(s)


def _region(haps, reads, quals, gaps=45, gcp=10):
    """haplotypes and reads (bytes each) as a region dict with the explicit pair list read-major"""
    ro = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    ho = np.concatenate([[0], np.cumsum([len(h) for h in haps])]).astype(np.uint64)
    nb, nr, nh = int(ro[-1]), len(reads), len(haps)
    return dict(read_off=ro, hap_off=ho, bases=_arr(b"".join(reads)).copy(), qual=_arr(b"".join(quals)).copy(),
                ins=np.full(nb, gaps, dtype=np.uint8), dele=np.full(nb, gaps, dtype=np.uint8), gcp=np.full(nb, gcp, dtype=np.uint8),
                hap_bases=_arr(b"".join(haps)).copy(), pair_read=np.repeat(np.arange(nr, dtype=np.uint32), nh),
                pair_hap=np.tile(np.arange(nh, dtype=np.uint32), nr))


def _seam_region(rng, read_len, n_haps=2):
    """reads of one length cut from haplotype 0: verbatim, one and two Q30 mismatches (each twice, at different places); the other
    haplotypes are random"""
    haps = [_letters(rng, HAP_LEN) for _ in range(n_haps)]
    reads = []
    for k in (0, 1, 2, 0, 1, 2):
        at = int(rng.randint(0, HAP_LEN - read_len + 1))
        where = rng.choice(np.arange(5, read_len - 5), k, replace=False)
        reads.append(_mutate(rng, haps[0][at:at + read_len], where))
    return _region(haps, reads, [bytes([30] * read_len)] * len(reads)), np.arange(60, 60 - len(reads), -1).astype(np.uint8)


def _width_region(rng, n_haps, sources, near_q=30, read_quality=30, mapq0=60):
    """one verbatim read per entry of ``sources`` (the index of its haplotype, the best of its row); next to every source a
    haplotype one base away from it, at a base of quality ``near_q`` that every read covers; the others are random"""
    haps = [_letters(rng, HAP_LEN) for _ in range(n_haps)]
    spots = []                                            # within every read's span, a different base per pair of neighbours
    free = [i for i in range(n_haps) if i not in sources]
    if not free:                                          # every haplotype is some read's best: all of them one base from the first
        for k in range(1, n_haps):
            spots.append(30 + 3 * len(spots))
            haps[k] = _mutate(rng, haps[0], [spots[-1]])
    else:
        for p in sorted(set(sources)):
            near = min(free, key=lambda i: abs(i - p))
            free.remove(near)
            spots.append(30 + 3 * len(spots))
            haps[near] = _mutate(rng, haps[p], [spots[-1]])
    reads, quals = [], []
    for r, p in enumerate(sources):
        n = 60 + 9 * r
        at = int(rng.randint(0, min(25, HAP_LEN - n) + 1))
        q = bytearray([read_quality] * n)
        for spot in spots:
            q[spot - at] = near_q
        reads.append(haps[p][at:at + n]); quals.append(bytes(q))
    return _region(haps, reads, quals), (mapq0 - np.arange(len(sources))).astype(np.uint8)


def _subview(d, mapq, rng):
    """the same region as a view into larger arrays: offsets that do not start at 0"""
    jr, jh = int(rng.randint(40, 90)), int(rng.randint(40, 90))
    v = dict(d)
    for k in ("bases", "qual", "ins", "dele", "gcp"):
        v[k] = np.concatenate([rng.randint(33, 90, jr).astype(np.uint8), d[k], rng.randint(33, 90, 17).astype(np.uint8)])
    v["hap_bases"] = np.concatenate([_arr(_letters(rng, jh)), d["hap_bases"], _arr(_letters(rng, 9))])
    v["read_off"] = d["read_off"] + np.uint64(jr)
    v["hap_off"] = d["hap_off"] + np.uint64(jh)
    return v


def _nf(name, regions, mapqs, plain=None, **model):
    """``plain``: per region the same region with offsets from 0 (what the oracle computes on), where it differs"""
    m = dict(NF_MODEL)
    m.update(model)
    return dict(name=name, regions=regions, mapqs=mapqs, plain=plain or regions, model=m)


@functools.lru_cache(maxsize=None)
def nf_cases():
    """Every case: regions whose reads are cut from their haplotypes, their MAPQs and the model."""
    rng = np.random.RandomState(4711)
    cases = []
    # the keep decision where ceil(R * 0.02) goes from 1 to 2, and where min(2, .) takes over
    for R in (49, 50, 51, 100, 101):
        d, mq = _seam_region(rng, R)
        cases.append(_nf("seam_R%d" % R, [d], [mq]))
    d, mq = _seam_region(rng, 50)
    cases.append(_nf("seam_R50_rate_one_ulp_up", [d], [mq], max_error_per_base=float(np.nextafter(0.02, 1.0))))
    # 64 lanes over n_haps
    for n_haps, sources in ((1, [0]), (2, [0, 1]), (63, [0, 62]), (64, [0, 63]), (65, [0, 63, 64]), (128, [0, 63, 64, 127]), (129, [0, 63, 64, 128, 100])):
        d, mq = _width_region(rng, n_haps, sources)
        cases.append(_nf("width_%d" % n_haps, [d], [mq]))
    # four wavefronts per workgroup over n_reads
    for n_reads in (1, 3, 4, 5):
        d, mq = _width_region(rng, 3, [r % 3 for r in range(n_reads)])
        cases.append(_nf("reads_%d" % n_reads, [d], [mq]))
    # the rates
    d, mq = _width_region(rng, 65, [0, 63, 64], near_q=20)
    cases.append(_nf("rate_-3.0", [d], [mq], log10_mismapping_rate=-3.0))
    d, mq = _width_region(rng, 65, [0, 63, 64])
    cases.append(_nf("rate_off", [d], [mq], log10_mismapping_rate=-math.inf))
    # rows of -inf: Q93 throughout, nothing capped or floored by the model
    raw = dict(pcr_rate_factor=0, constant_gcp=-1)
    q93 = bytes([93] * 200)
    d = _region([b"A" * 230, b"G" * 250], [b"C" * 200], [q93], gaps=93, gcp=93)
    cases.append(_nf("all_minus_inf", [d], [np.array([255], dtype=np.uint8)], **raw))
    hap = _letters(rng, 230, b"AC")
    d = _region([hap, _letters(rng, 250, b"GT")], [hap[11:211]], [q93], gaps=93, gcp=93)
    cases.append(_nf("one_minus_inf", [d], [np.array([255], dtype=np.uint8)], **raw))
    # region layout: MAPQ below the base qualities and distinct per read, so a wrong read index shows
    a, mqa = _width_region(rng, 3, [0, 1, 2], read_quality=40, near_q=40, mapq0=35)
    b, mqb = _width_region(rng, 4, [3, 0, 1, 2, 3], read_quality=40, near_q=40, mapq0=32)
    e = _region([_letters(rng, 90), _letters(rng, 95)], [], [])
    s, mqs = _width_region(rng, 9, [8, 2, 0, 5], read_quality=40, near_q=40, mapq0=27)
    cases.append(_nf("layout_empty", [a, e, b], [mqa, np.zeros(0, dtype=np.uint8), mqb]))
    cases.append(_nf("layout_subview", [a, _subview(s, mqs, rng), b], [mqa, mqs, mqb], plain=[a, s, b]))
    return cases
