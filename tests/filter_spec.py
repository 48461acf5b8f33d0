"""Specification of filter (Flt) and of the concatenation of batches (Mrg) -- TEST INFRASTRUCTURE ONLY.

A restatement in plain Python, line by line, of
    interval::overlap                     src/interval.h:38-58
    FilterCondition::FilterCondition      src/filter.cpp:24-115   (rsplit: src/util.h:175-185; std::stoi)
    the loop of Filter_module::run        src/filter.cpp:196-212
over the molecule dicts of oracle/mdf_ops_oracle.py (stream_mdf / write_mdf).  Neither draws a random number.  The build takes its
input depth-unrolled (the reference's Flt does not); the predicate reads the record alone, so the build's output is the unrolling of
the reference's: filter_spec is applied to stream_mdf(text, unroll=True).
Refused here (InvalidCondition) beyond what the reference throws on: an unknown kind (it leaves an empty std::function that is called
later), a negative size value (it wraps to unsigned) and a negative coordinate."""
import re

import mdf_ops_oracle as mo

INT_MIN, INT_MAX = -2**31, 2**31 - 1


class InvalidCondition(ValueError):
    def __init__(self, text):
        super().__init__("Invalid condition: " + text)


def overlap(start, end, o_start, o_end):
    """interval(start, end).overlap(interval(o_start, o_end)), src/interval.h:38-58"""
    if o_end <= start:                                              # BEFORE
        return 0
    elif o_start >= end:                                            # AFTER
        return 0
    elif o_start >= start and o_end <= end:                         # IN
        return o_end - o_start
    elif o_start < start and o_end > end:                           # AROUND
        return end - start
    elif o_start < start and o_end < end and o_end > start:         # LEFT OVERLAP
        return o_end - start
    elif o_start > start and o_start < end and o_end > end:         # RIGHT OVERLAP
        return end - o_start
    return 0


def rsplit(s, delim):                                               # src/util.h:175-185: empty pieces are kept
    return s.split(delim)


def stoi(s):
    """std::stoi: white space, a sign, digits, the rest ignored; None where it throws (no digits; outside int)"""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?[0-9]+)", s)
    if not m:
        return None
    v = int(m.group(1))
    return v if INT_MIN <= v <= INT_MAX else None


def condition(text):
    """FilterCondition(text) -> a predicate over a molecule dict (src/filter.cpp:24-115)"""
    fields = rsplit(text, " ")
    if len(fields) != 2:
        raise InvalidCondition(text)
    kind, expr = fields
    if kind == "info":
        def info(md):
            values = md["meta"].get(expr)
            if values is None:
                return False
            if not values:
                return False
            if values[0] == ".":
                return False
            return True
        return info
    if kind == "size":
        if len(expr) < 2:
            raise InvalidCondition(text)
        symb = expr[:2] if expr[1] == "=" else expr[:1]
        val = stoi(expr[len(symb):])
        if val is None or val < 0:
            raise InvalidCondition(text)
        ops = {"<": lambda a: a < val, "<=": lambda a: a <= val, ">": lambda a: a > val, ">=": lambda a: a >= val,
               "==": lambda a: a == val, "!=": lambda a: a != val}
        if symb not in ops:
            raise InvalidCondition(text)
        return lambda md: ops[symb](mo.mol_size(md))                # molecule_descriptor::size, src/interval.h:876
    if kind == "locus":
        rf = rsplit(expr, ":")
        chrom = rf[0]
        if len(rf) == 1:
            return lambda md: any(s["chr"] == chrom for s in md["segments"])
        rng = rsplit(rf[1], "-")
        start = stoi(rng[0])
        end = (start + 1 if start is not None else None) if len(rng) == 1 else stoi(rng[1])
        if start is None or end is None or start < 0 or end < 0:
            raise InvalidCondition(text)
        return lambda md: any(s["chr"] == chrom and overlap(s["start"], s["end"], start, end) > 0 for s in md["segments"])
    raise InvalidCondition(text)


def filter_spec(mols, conditions, negate=False):
    """(true side, false side) of the unrolled molecules `mols`, each in input order (src/filter.cpp:196-212)"""
    preds = [condition(c) for c in conditions]
    sides = ([], [])
    for md in mols:
        flag = True
        for p in preds:
            if not p(md):
                flag = False
                break
        if negate:
            flag = not flag
        sides[0 if flag else 1].append(md)
    return sides


def concat_spec(batches):
    """`cat` of the batches' MDF text, read back: the molecules of batches[0], then batches[1], ..."""
    return [md for b in batches for md in b]
