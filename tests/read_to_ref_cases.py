"""Restatement and cases for the read -> reference step of the realignment (tests/test_read_to_ref_host.py, tests/test_read_to_ref_gpu.py,
tests/golden/make_golden_read_to_ref.py, tools/fuzz.py); not a test.

* ``create_read_aligned_to_ref``: AlignmentUtils::createReadAlignedToRef lines 505-543 (read/AlignmentUtils.cpp) restated sequentially:
  every function it reaches is restated as the reference has it, base by base and element list by element list, exceptions included.
  A CIGAR is a list of (length, operator character).  Where the reference leaves the language's defined behaviour the restatement
  raises ``Undefined``: a negative allocation or a copy from outside the read in createIndelString, and an aligner CIGAR that is one
  element of length 0 (consolidateCigar keeps it, applyCigarToCigar's element counter then never meets the length).
* ``to_ref``: the same as (status, start, elements) with the statuses of include/mgx_realign.h, hard clips and row capacity included.
* ``cases``: the seeded case set of the CPU test;  ``shape_cases``: the kernel's seams for the GPU test;  ``HAND``: the issue's table.
"""
import zlib

import numpy as np

OK, DROPPED, UNCHANGED, THROWS, UNDEFINED, NO_ROOM = range(6)
STATUS_NAMES = ("OK", "DROPPED", "UNCHANGED", "THROWS", "UNDEFINED", "NO_ROOM")
OPS = "MIDNSHP=X"                                       # BAM operator codes 0..8
PAD = 1000
M_CLASS, I_CLASS, D_CLASS = "M=X", "IS", "D"


class Throws(Exception):
    """the reference throws here"""


class Undefined(Exception):
    """the reference would leave defined behaviour here"""


def encode(cigar):
    return np.array([(n << 4) | OPS.index(op) for n, op in cigar], dtype=np.uint32)


def decode(elements):
    return [(int(e) >> 4, OPS[int(e) & 15]) for e in elements]


def parse(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n), ch)); n = ""
    return out


def text_of(cigar):
    return "".join("%d%s" % e for e in cigar)


def validate_arg(cond, msg):
    if not cond:
        raise Throws(msg)


def read_length(c):                                                   # Cigar::getReadLength
    return sum(n for n, op in c if op in "MIS=X")


def reference_length(c):                                              # Cigar::getReferenceLength
    return sum(n for n, op in c if op in "MDN=X")


def needs_consolidation(c):                                           # :101-111
    if len(c) <= 1:
        return False
    last_op = None      # uninitialised in the reference: a spurious "true" consolidates a list that needs none, which changes nothing
    for n, op in c:
        if n == 0 or last_op == op:
            return True
        last_op = op
    return False


def consolidate_cigar(c):                                             # :74-99
    if not needs_consolidation(c):
        return c
    out, sum_length, last = [], 0, None
    for n, op in c:
        if n == 0:
            continue
        if last is not None and last != op:
            out.append((sum_length, last)); sum_length = 0
        sum_length += n
        last = op
    if sum_length > 0:
        out.append((sum_length, last))
    return out


def get_consolidated_padded_cigar(hap_cigar, pad_size):               # Haplotype.cpp:120-127
    ext = list(hap_cigar)
    if pad_size > 0:
        ext.append((pad_size, "M"))
    return consolidate_cigar(ext)


def calc_first_base_matching_reference_in_cigar(cigar, read_start_by_base_of_cigar):      # :550-581
    hap_offset = ref_offset = 0
    for n, op in cigar:
        for _ in range(n):
            if op in M_CLASS:
                if hap_offset >= read_start_by_base_of_cigar:
                    return ref_offset
                hap_offset += 1; ref_offset += 1
            elif op in I_CLASS:
                hap_offset += 1
            elif op == "D":
                ref_offset += 1
            else:
                raise Throws("calcFirstBaseMatchingReferenceInCigar does not support cigar")
    raise Throws("ran off the cigar")


def add_cigar_elements(dest, pos, start, end, elt):                   # :219-224
    length = min(pos + elt[0] - 1, end) - max(pos, start) + 1
    if length > 0:
        dest.append((length, elt[1]))
    return pos + elt[0]


def trim_cigar(cigar, start, end, by_reference):                      # :182-217
    new, pos = [], 0
    for elt in cigar:
        op = elt[1]
        if pos > end and (by_reference or op != "D"):
            break
        if op == "D" and not by_reference:
            if pos >= start:
                new.append(elt)
        elif op in "D=MX":
            pos = add_cigar_elements(new, pos, start, end, elt)
        elif op in "SI":
            if by_reference:
                if pos >= start:
                    new.append(elt)
            else:
                pos = add_cigar_elements(new, pos, start, end, elt)
        else:
            raise Throws("Cannot handle")
    return consolidate_cigar(new)


def trim_cigar_by_bases(cigar, start, end):                           # :243-252
    validate_arg(start >= 0, "start must be >= 0")
    validate_arg(end >= start, "End is < start")
    validate_arg(end <= read_length(cigar), "End is beyond the cigar's read length")
    result = trim_cigar(cigar, start, end, False)
    validate_arg(read_length(result) == end - start + 1, "trimCigarByBases failure")
    return result


TRANSFORMERS = (                                                      # :13-70, op12, op23, op13, advance12, advance23
    (M_CLASS, M_CLASS, "M", 1, 1), (M_CLASS, I_CLASS, "I", 1, 1), (M_CLASS, D_CLASS, "D", 0, 1),
    (D_CLASS, M_CLASS, "D", 1, 1), (D_CLASS, D_CLASS, "D", 0, 1), (D_CLASS, I_CLASS, None, 1, 1),
    (I_CLASS, M_CLASS, "I", 1, 0), (I_CLASS, D_CLASS, "I", 1, 0), (I_CLASS, I_CLASS, "I", 1, 0))


def get_transformer(op12, op23):                                      # :611-619
    for t in TRANSFORMERS:
        if op12 in t[0] and op23 in t[1]:
            return t
    raise Throws("no transformer")


def apply_cigar_to_cigar(first_to_second, second_to_third, trace=None):      # :583-609
    new = []
    cigar12 = cigar23 = elt12 = elt23 = 0
    while cigar12 < len(first_to_second) and cigar23 < len(second_to_third):
        e12, e23 = first_to_second[cigar12], second_to_third[cigar23]
        _, _, op13, advance12, advance23 = get_transformer(e12[1], e23[1])
        if op13 is not None:
            new.append((1, op13))
        elif trace is not None:
            trace["skipped"] = trace.get("skipped", 0) + 1
        elt12 += advance12; elt23 += advance23
        if elt12 == e12[0]:
            cigar12 += 1; elt12 = 0
        if elt23 == e23[0]:
            cigar23 += 1; elt23 = 0
    return consolidate_cigar(new)


def clean_up_cigar(c):                                                # :475-484
    out = []
    for n, op in c:
        if n != 0 and (out or op != "D"):
            out.append((n, op))
    return out


def count_indel_elements(c):                                          # :279-287
    return sum(op in "DI" for _, op in c)


def create_indel_string(cigar, index_of_indel, ref_seq, read_seq, ref_index, read_index):      # :370-424; None = nullptr
    ref_length, read_len = len(ref_seq), len(read_seq)
    indel_length, indel_op = cigar[index_of_indel]
    total_ref_bases = 0
    for i in range(index_of_indel):
        length, op = cigar[i]
        if op in "M=X":
            read_index += length; ref_index += length; total_ref_bases += length
        elif op == "S":
            read_index += length
        elif op == "N":
            ref_index += length; total_ref_bases += length
    if total_ref_bases + indel_length > ref_length:
        indel_length -= total_ref_bases + indel_length - ref_length
    alt_length = ref_length + indel_length * (-1 if indel_op == "D" else 1)
    if alt_length < 0:
        raise Undefined("new uint8_t[%d]" % alt_length)
    alt = bytearray(alt_length)
    if ref_index > alt_length or ref_index > ref_length:
        return None
    alt[0:ref_index] = ref_seq[0:ref_index]
    current_pos = ref_index
    if indel_op == "D":
        ref_index += indel_length
    else:
        if indel_length < 0 or read_index + indel_length > read_len:
            raise Undefined("memcpy of %d read bases from %d" % (indel_length, read_index))
        alt[current_pos:current_pos + indel_length] = read_seq[read_index:read_index + indel_length]
        current_pos += indel_length
    if ref_length - ref_index > alt_length - current_pos:
        return None
    if ref_length - ref_index < 0:
        raise Undefined("memcpy of %d reference bases" % (ref_length - ref_index))
    alt[current_pos:current_pos + ref_length - ref_index] = ref_seq[ref_index:ref_length]
    return bytes(alt)


def move_cigar_left(cigar, index_of_indel):                           # :426-446
    elements = [cigar[i] for i in range(index_of_indel - 1)]
    n, op = cigar[index_of_indel - 1]
    elements.append((max(n - 1, 0), op))
    elements.append(cigar[index_of_indel])
    if index_of_indel + 1 < len(cigar):
        n, op = cigar[index_of_indel + 1]
        elements.append((n + 1, op))
    else:
        elements.append((1, "M"))
    elements.extend(cigar[index_of_indel + 2:])
    return elements


def is_indel_aligned_too_far_left(cigar, leftmost_allowed_alignment):      # :448-459
    location = 0
    for n, op in cigar:
        if op in "DI":
            return location < leftmost_allowed_alignment
        if op in "MDN=X":
            location += n
    return False


def cigar_has_zero_size_element(c):                                   # :461-473
    return any(n == 0 for n, _ in c)


def left_align_single_indel(cigar, ref_seq, read_seq, ref_index, read_index, leftmost_allowed_alignment, cleanup_cigar, trace=None):   # :295-359
    validate_arg(ref_index >= 0 and read_index >= 0, "index less than 0")
    index_of_indel = -1
    for i, (_, op) in enumerate(cigar):
        if op in "DI":
            if index_of_indel != -1:
                raise Throws("more than 1 indel")
            index_of_indel = i
    if index_of_indel == -1:
        raise Throws("no indels")
    if index_of_indel == 0:
        return cigar
    indel_length = cigar[index_of_indel][0]
    alt_string = create_indel_string(cigar, index_of_indel, ref_seq, read_seq, ref_index, read_index)
    if alt_string is None:
        return cigar
    new_cigar = list(cigar)
    i = 0
    while i < indel_length:
        new_cigar = move_cigar_left(new_cigar, index_of_indel)
        if is_indel_aligned_too_far_left(new_cigar, leftmost_allowed_alignment):
            break
        new_alt_string = create_indel_string(new_cigar, index_of_indel, ref_seq, read_seq, ref_index, read_index)
        reached_end_of_read = cigar_has_zero_size_element(new_cigar)
        # a nullptr leaves newAltStringLength at 0: equal only to an empty string
        is_equal = (len(alt_string) == 0) if new_alt_string is None else alt_string == new_alt_string
        if is_equal:
            cigar = new_cigar
            i = -1
            if trace is not None:
                trace["moved"] = True
            if reached_end_of_read:
                cigar = clean_up_cigar(cigar) if cleanup_cigar else cigar
                if trace is not None:
                    trace["to_start"] = True
        if reached_end_of_read:
            break
        i += 1
    return cigar


def left_align_indel(cigar, ref_seq, read_seq, ref_index, read_index, leftmost_allowed_alignment, do_not_throw, trace=None):   # :254-271
    validate_arg(ref_index >= 0 and read_index >= 0, "index less than 0")
    num_indels = count_indel_elements(cigar)
    if trace is not None:
        trace["indels"] = num_indels
    if num_indels == 0:
        return cigar
    if num_indels == 1:
        return left_align_single_indel(cigar, ref_seq, read_seq, ref_index, read_index, leftmost_allowed_alignment, True, trace)
    if do_not_throw:
        return cigar
    raise Throws("more than 1 indel")


def create_read_aligned_to_ref(sw_cigar, sw_offset, hap_cigar, hap_start, ref_bases, read_bases, reference_start, trace=None):
    """-> None (the original read is returned) or (start, read -> reference CIGAR without hard clips)"""
    if sw_offset == -1:                                               # :500
        return None
    if len(sw_cigar) == 1 and sw_cigar[0][0] == 0:
        raise Undefined("an aligner CIGAR of one empty element")
    sw = consolidate_cigar(list(sw_cigar))                            # :505
    extended = get_consolidated_padded_cigar(hap_cigar, PAD)          # :515
    read_start_on_haplotype = calc_first_base_matching_reference_in_cigar(extended, sw_offset)
    read_start_on_reference = reference_start + hap_start + read_start_on_haplotype
    haplotype_to_ref = trim_cigar_by_bases(extended, sw_offset, read_length(extended) - 1)      # :521
    raw = apply_cigar_to_cigar(sw, haplotype_to_ref, trace)
    clean = clean_up_cigar(raw)
    final = left_align_indel(clean, ref_bases, read_bases, read_start_on_haplotype, 0, 0, True, trace)
    leading_deletions = reference_length(clean) - reference_length(final)
    if trace is not None:
        trace["leading"] = leading_deletions
    if read_length(final) != len(read_bases):                         # :543
        raise Throws("read length")
    return read_start_on_reference + leading_deletions, final


def to_ref(case, trace=None):
    """-> (status, start, elements as uint32) for a case dict; start and elements are (0, []) unless OK / NO_ROOM (count only)"""
    none = np.zeros(0, np.uint32)
    try:
        got = create_read_aligned_to_ref(case["sw"], case["offset"], case["hap"], case["hap_start"], case["ref"], case["read"],
                                         case["reference_start"], trace)
    except Throws:
        return THROWS, 0, none
    except Undefined:
        return UNDEFINED, 0, none
    if got is None:
        return UNCHANGED, 0, none
    start, cigar = got
    lead, trail = case.get("hard", (0, 0))
    cigar = ([(lead, "H")] if lead else []) + list(cigar) + ([(trail, "H")] if trail else [])
    if len(cigar) > case.get("stride", 1 << 30):
        return NO_ROOM, start, np.zeros(len(cigar), np.uint32)      # only the count is defined
    return OK, start, encode(cigar)


def case(sw, offset, hap, hap_start, ref, read, reference_start=0, hard=(0, 0), stride=24, name=""):
    sw = parse(sw) if isinstance(sw, str) else list(sw)
    hap = parse(hap) if isinstance(hap, str) else list(hap)
    as_bytes = lambda s: s.encode() if isinstance(s, str) else bytes(s)
    return dict(name=name, sw=sw, offset=int(offset), hap=hap, hap_start=int(hap_start), ref=as_bytes(ref), read=as_bytes(read),
                reference_start=int(reference_start), hard=(int(hard[0]), int(hard[1])), stride=int(stride))


# the issue's table: (case, result text, start), reference_start = 0
HAND = (
    (case("2S6M2S", 3, "20M", 5, "ACGTACGTACGTACGTACGTACGT", "TTACGTACGG"), "2I6M2I", 8),
    (case("4M2I4M", 2, "8M3D12M", 0, "AAAACCCCGGGTTTTACGTACGT", "AACCCCCCGGTT"), "4M2I2M3D2M", 2),
    (case("10M", 4, "6M2D14M", 0, "AC" * 12, "CACACACACA"), "10M", 6),
    (case("10M", 4, "6M2I14M", 0, "AC" * 12, "CACACACACA"), "2M2I6M", 4),
    (case("10M", 0, "6M2I2M", 0, "AC" * 12, "ACACACCCAC"), "5M2I3M", 0),
    (case("10M", 0, "6M2I2M", 0, "AC" * 12, "ACACACACAC"), "2I8M", 0),
    (case("12M", 0, "2M2D20M", 0, "AC" * 12, "AC" * 6), "12M", 2),
)

CATEGORIES = ("moved_left", "moved_to_start", "leading_deletion", "multi_indel", "soft_clips", "d_i_pair", "offset_in_I", "offset_at_D",
              "hard_one", "hard_both")


def categories(c):
    """which of the conditions the CPU test counts this case meets, by the restatement alone"""
    trace = {}
    status, _, _ = to_ref(c, trace)
    out = set()
    if status != OK:
        return status, out
    if trace.get("moved") and not trace.get("to_start"):
        out.add("moved_left")
    if trace.get("to_start"):
        out.add("moved_to_start")
    if trace.get("leading", 0) > 0:
        out.add("leading_deletion")
    if trace.get("indels", 0) >= 2:
        out.add("multi_indel")
    if any(op == "S" and n for n, op in c["sw"]):
        out.add("soft_clips")
    if trace.get("skipped"):
        out.add("d_i_pair")
    pos = 0
    for n, op in get_consolidated_padded_cigar(c["hap"], PAD):
        if op == "I" and pos <= c["offset"] < pos + n:
            out.add("offset_in_I")
        if op == "D" and pos == c["offset"]:
            out.add("offset_at_D")
        if op != "D":
            pos += n
    lead, trail = c["hard"]
    if bool(lead) != bool(trail):
        out.add("hard_one")
    if lead and trail:
        out.add("hard_both")
    return status, out


# ---- generators -----------------------------------------------------------------------------------------------------------------
def _bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(n)).tobytes())


def _apply(ref, cigar, rng):
    """the sequence that `cigar` aligns to ref[0:]: M copies, I inserts new bases, D skips"""
    out, at = bytearray(), 0
    for n, op in cigar:
        if op in "M=X":
            out += ref[at:at + n]; at += n
        elif op in "IS":
            out += _bases(rng, n)
        elif op == "D":
            at += n
    return bytes(out)


def _repeat_ref(rng, period, total, flank):
    unit = _bases(rng, period)
    body = (unit * (total // period + 2))[:total]
    return _bases(rng, flank) + body + _bases(rng, flank)


def repeat_case(rng, period, indel, op, ref_len=None, hard=(0, 0), start_inside=False, extra=None, name="repeat"):
    """a haplotype that is the reference with one indel placed at the right end of a repeat tract, and a read cut from it: the indel
    can move left through the tract, to the read's start when the read begins inside the tract"""
    flank = int(rng.integers(3, 9))
    tract = int(rng.integers(2, 7)) * max(period, 1) + indel + int(rng.integers(0, period + 1))
    ref = _repeat_ref(rng, period, tract, flank)
    if ref_len is not None:
        ref = (ref + _bases(rng, max(ref_len - len(ref), 0)))[:ref_len]
    at = min(flank + tract, len(ref)) - (indel if op == "D" else 0)      # the indel's place on the reference: the tract's right end
    at = max(at, 1)
    tail = len(ref) - at - (indel if op == "D" else 0)
    if tail <= 0:
        hap_cigar = [(len(ref), "M")]
    else:
        hap_cigar = [(at, "M"), (indel, op), (tail, "M")]
    unit_src = ref[flank:flank + max(period, 1)]
    hap, pos = bytearray(), 0
    for n, o in hap_cigar:
        if o == "M":
            hap += ref[pos:pos + n]; pos += n
        elif o == "D":
            pos += n
        else:
            k = (at - flank) % max(period, 1)
            hap += ((unit_src[k:] + unit_src[:k]) * (n // max(period, 1) + 1))[:n]      # the insertion continues the repeat
    hap = bytes(hap)
    lo = int(rng.integers(flank + 1, flank + max(2, tract // 2))) if start_inside else int(rng.integers(0, flank))
    lo = min(lo, max(len(hap) - 1, 0))
    hi = min(len(hap), at + (indel if op == "I" else 0) + int(rng.integers(1, 8)))
    hi = max(hi, lo + 1)
    read = hap[lo:hi]
    sw = [(len(read), "M")] if extra is None else extra(read)
    return case(sw, lo, hap_cigar, int(rng.integers(0, 4)), ref, read, int(rng.integers(0, 1000)), hard, name=name)


def soup_case(rng, name="soup"):
    """small random lists of every kind, most of them consistent in their lengths"""
    ref = _bases(rng, rng.integers(20, 60))
    hap_cigar, left = [], len(ref)
    for _ in range(int(rng.integers(1, 5))):
        op = "MMMIDS=X"[int(rng.integers(0, 8))]
        n = int(rng.integers(0, 7)) if rng.random() < 0.9 else 0
        if op in "MD=X":
            n = min(n, left); left -= n
        hap_cigar.append((n, op))
    hap_cigar.append((left, "M"))
    hap = _apply(ref, hap_cigar, rng)
    offset = int(rng.integers(0, max(len(hap) - 4, 1)))
    sw, budget = [], len(hap) - offset
    for _ in range(int(rng.integers(1, 5))):
        op = "MMMIDS=X"[int(rng.integers(0, 8))]
        n = int(rng.integers(0, 8))
        if op in "MD=X":
            n = min(n, budget); budget -= n
        sw.append((n, op))
    if len(sw) == 1 and sw[0][0] == 0:
        sw.append((1, "M"))
    read = _apply(hap[offset:], sw, rng)
    read = read + _bases(rng, read_length(sw) - len(read))
    hard = ((0, 0), (3, 0), (0, 5), (2, 2))[int(rng.integers(0, 4))]
    return case(sw, offset, hap_cigar, int(rng.integers(0, 5)), ref, read, int(rng.integers(0, 10000)), hard, name=name)


def two_indel_case(rng):
    return repeat_case(rng, int(rng.integers(1, 4)), int(rng.integers(1, 4)), "DI"[int(rng.integers(0, 2))],
                       extra=lambda read: [(len(read) - 3, "M"), (1, "I"), (2, "M")] if len(read) > 4 else [(len(read), "M")], name="two")


def clip_case(rng):
    def clipped(read):
        s = int(rng.integers(1, 3)); t = int(rng.integers(0, 3))
        if len(read) <= s + t:
            return [(len(read), "M")]
        return [(s, "S"), (len(read) - s - t, "M")] + ([(t, "S")] if t else [])
    c = repeat_case(rng, 2, 2, "DI"[int(rng.integers(0, 2))], extra=clipped, name="clips")
    if c["sw"][0][1] == "S":
        c["offset"] += c["sw"][0][0]
    return c


def d_i_case(rng):
    """the aligner deletes exactly the bases the haplotype inserted"""
    ref = _bases(rng, rng.integers(24, 50))
    at, n = int(rng.integers(6, 12)), int(rng.integers(1, 5))
    hap_cigar = [(at, "M"), (n, "I"), (len(ref) - at, "M")]
    lo = int(rng.integers(0, 4))
    pre, post = at - lo, int(rng.integers(3, 9))
    read = ref[lo:at] + ref[at:at + post]
    part = int(rng.integers(1, n + 1))
    sw = [(pre, "M"), (part, "D"), (post, "M")] if part == n else [(pre + n - part, "M"), (part, "D"), (post, "M")]
    if part != n:
        read = ref[lo:at] + _bases(rng, n - part) + ref[at:at + post]
    return case(sw, lo, hap_cigar, 1, ref, read, 17, name="d_i")


def offset_case(rng, inside_i):
    ref = _bases(rng, rng.integers(24, 50))
    at, n = int(rng.integers(4, 12)), int(rng.integers(2, 6))
    length = int(rng.integers(5, 10))
    if inside_i:
        hap_cigar = [(at, "M"), (n, "I"), (len(ref) - at, "M")]
        offset = at + int(rng.integers(0, n))
    else:
        hap_cigar = [(at, "M"), (n, "D"), (len(ref) - at - n, "M")]
        offset = at
    return case([(length, "M")], offset, hap_cigar, 0, ref, _bases(rng, length), 5, name="offset_in_I" if inside_i else "offset_at_D")


def bad_case(rng, kind):
    c = repeat_case(rng, 2, 2, "D", name=kind)
    if kind == "unchanged":
        c["offset"] = -1
    elif kind == "hap_N":
        c["hap"] = c["hap"][:1] + [(3, "NHP"[int(rng.integers(0, 3))])] + c["hap"][1:]
    elif kind == "offset_beyond":
        c["offset"] = read_length(c["hap"]) + PAD + int(rng.integers(0, 3))
    elif kind == "offset_negative":
        c["offset"] = -2 - int(rng.integers(0, 3))
    elif kind == "sw_op":
        c["sw"] = [(2, "M"), (1, "NHP"[int(rng.integers(0, 3))]), (len(c["read"]) - 2, "M")]
    elif kind == "read_length":
        c["read"] = c["read"] + b"A" * int(rng.integers(1, 3))
    elif kind == "empty_element":
        c["sw"] = [(0, "MIDS"[int(rng.integers(0, 4))])]
    elif kind == "outside_read":                       # one insertion whose bases lie behind the read's end
        n = len(c["read"])
        c["hap"] = [(len(c["ref"]), "M")]
        c["sw"] = [(n, "M"), (int(rng.integers(1, 4)), "I")]
    elif kind == "no_room":
        status, _, el = to_ref(c)
        c["hard"] = (1, 0)
        c["stride"] = len(el)                          # one short of the row with the hard clip
    return c


def cases(seed=20240611, n_random=2600):
    """the CPU test's set: HAND, then seeded cases of every kind"""
    rng = np.random.default_rng(seed)
    out = [dict(c, name="hand%d" % i) for i, (c, _, _) in enumerate(HAND)]
    hards = ((0, 0), (0, 0), (4, 0), (0, 7), (3, 9))
    for i in range(n_random):
        kind = i % 13
        hard = hards[int(rng.integers(0, len(hards)))]
        if kind in (0, 1, 2):
            out.append(repeat_case(rng, (1, 2, 3)[kind], int(rng.integers(1, 7)), "DI"[i // 13 % 2], hard=hard))
        elif kind in (3, 4):
            out.append(repeat_case(rng, int(rng.integers(1, 4)), int(rng.integers(1, 5)), "DI"[kind - 3], hard=hard, start_inside=True, name="inside"))
        elif kind == 5:
            out.append(two_indel_case(rng))
        elif kind == 6:
            out.append(clip_case(rng))
        elif kind == 7:
            out.append(d_i_case(rng))
        elif kind == 8:
            out.append(offset_case(rng, i // 13 % 2 == 0))
        elif kind in (9, 10, 11):
            out.append(soup_case(rng))
        else:
            kinds = ("unchanged", "hap_N", "offset_beyond", "offset_negative", "sw_op", "read_length", "empty_element", "outside_read", "no_room")
            out.append(bad_case(rng, kinds[i // 13 % len(kinds)]))
    return out


def shape_cases(seed=77):
    """the kernel's seams: indel lengths and reference lengths around the lanes' stride of 64, repeat periods that divide the indel and
    that do not, a read of one base, a haplotype that is the reference, every status"""
    rng = np.random.default_rng(seed)
    out = []
    for indel in (1, 2, 63, 64, 65):
        for period in (1, 2, 3, 7):
            for op in "DI":
                out.append(repeat_case(rng, period, indel, op, name="indel%d_p%d%s" % (indel, period, op)))
                out.append(repeat_case(rng, period, indel, op, start_inside=True, name="indel%d_p%d%s_inside" % (indel, period, op)))
    for ref_len in (1, 63, 64, 65, 129, 1025):
        for op in "DI":
            for period in (1, 2):
                out.append(repeat_case(rng, period, int(rng.integers(1, 4)), op, ref_len=ref_len, name="ref%d%s" % (ref_len, op)))
        ref = _bases(rng, ref_len)
        out.append(case([(1, "M")], ref_len - 1, [(ref_len, "M")], 0, ref, ref[-1:], 3, name="one_base_ref%d" % ref_len))
        n = min(ref_len, 40)
        out.append(case([(n, "M")], 0, [(ref_len, "M")], 2, ref, ref[:n], 9, hard=(5, 6), name="hap_is_ref%d" % ref_len))
        # a homopolymer as long as the reference: every shift is accepted, the window crosses every lane seam
        homo = b"A" * ref_len
        if ref_len > 4:
            out.append(case([(ref_len - 2, "M")], 0, [(ref_len - 3, "M"), (2, "D"), (1, "M")], 0, homo, b"A" * (ref_len - 2), name="homoD%d" % ref_len))
            out.append(case([(ref_len - 2, "M"), (1, "I"), (1, "M")], 0, [(ref_len, "M")], 0, homo, b"A" * ref_len, name="homoI%d" % ref_len))
    for kind in ("unchanged", "hap_N", "offset_beyond", "offset_negative", "sw_op", "read_length", "empty_element", "outside_read", "no_room"):
        out.append(bad_case(rng, kind))
    out.extend(dict(c, name="hand%d" % i) for i, (c, _, _) in enumerate(HAND))
    return out


def digest(case_list):
    """a checksum of the inputs, so that a fixture is only compared with the cases it was made from"""
    h = 0
    for c in case_list:
        blob = repr((c["sw"], c["offset"], c["hap"], c["hap_start"], c["ref"], c["read"], c["reference_start"])).encode()
        h = zlib.crc32(blob, h)
    return h
