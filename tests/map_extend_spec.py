"""The rules of `tksm map --extend` (include/tksmseq.h, "map, end extension") in plain Python, written from that text and not from the
kernels: the banded X-drop extension of one end with its tie rules, its stop and its traceback, and the lines of a run with and without
alignment.  Everything else of map comes from tests/map_spec.py and tests/map_align_spec.py, which this file imports and does not edit.
tests/test_map_extend.py pins this file against an independent brute force and hand-worked cases; tests/test_map_extend_gpu.py compares
the device with it byte for byte."""
import functools

import map_align_spec as A
import map_spec as M

DEFAULTS = dict(ext_band=31, ext_drop=40, ext_max=2000)
COUNTERS = ("lines", "ends_moved", "target_gained", "read_gained", "matches", "antidiagonals", "cells", "longest")
MATCH, MISS, GAP = 1, -2, -2


def letters_match(a, b):
    return a == b and a in M.CODE


@functools.lru_cache(maxsize=None)
def extend(T, Q, B=31, Z=40):
    """T and Q: the letters beyond the corner, outward, already cut.  {"ei", "ej", "m", "score", "columns" (from the corner outward, over
    = X I D), "steps" (anti-diagonals computed), "cells" (allowed cells computed)}"""
    Lt, Lq = len(T), len(Q)
    out = dict(ei=0, ej=0, m=0, score=0, columns="", steps=0, cells=0)
    if Lt == 0 or Lq == 0:
        return out
    H, m, how = {(0, 0): 0}, {(0, 0): 0}, {}
    best, cell, before = 0, (0, 0), 0                    # before: mx of the anti-diagonal before this one
    for s in range(1, Lt + Lq + 1):
        row = [(i, s - i) for i in range(max(0, s - Lq), min(Lt, s) + 1) if abs(2 * i - s) <= B]
        if not row:
            break
        for i, j in row:
            options = []                                 # (value, matches, column) in the order of the rule: diagonal, D, I
            if (i - 1, j - 1) in H:
                hit = letters_match(T[i - 1], Q[j - 1])
                options.append((H[i - 1, j - 1] + (MATCH if hit else MISS), m[i - 1, j - 1] + hit, "=" if hit else "X"))
            if (i - 1, j) in H:
                options.append((H[i - 1, j] + GAP, m[i - 1, j], "D"))
            if (i, j - 1) in H:
                options.append((H[i, j - 1] + GAP, m[i, j - 1], "I"))
            top = max(v for v, _, _ in options)
            H[i, j], m[i, j], how[i, j] = next(o for o in options if o[0] == top)
        out["steps"] += 1
        out["cells"] += len(row)
        mx = max(H[c] for c in row)
        if mx > 0 and mx >= best:
            best, cell = mx, min(c for c in row if H[c] == mx)
        if max(mx, before) < best - Z:
            break
        before = mx
    i, j = cell
    columns = []
    while (i, j) != (0, 0):
        columns.append(how[i, j])
        i, j = (i - 1, j - 1) if how[i, j] in "=X" else (i - 1, j) if how[i, j] == "D" else (i, j - 1)
    out.update(ei=cell[0], ej=cell[1], m=m[cell], score=best, columns="".join(reversed(columns)))
    return out


def check_params(ext_band, ext_drop, ext_max):
    if not 1 <= ext_band <= 63 or not 1 <= ext_drop <= 1000 or not 1 <= ext_max <= 32768:
        raise ValueError("map: a parameter out of range")


def ends_of(tseq, strand, c, B, Z, max_ext):
    """(left, right) of chain c on target letters tseq and the read in the strand of rel"""
    right = extend(tseq[c["tend"]:c["tend"] + max_ext], strand[c["qe"]:c["qe"] + max_ext], B, Z)
    left = extend(tseq[max(0, c["tstart"] - max_ext):c["tstart"]][::-1], strand[max(0, c["qs"] - max_ext):c["qs"]][::-1], B, Z)
    return left, right


cigar = functools.lru_cache(maxsize=4096)(A.cigar)       # (the copies of a read share their columns)


def columns_of(text):
    """the columns of a CIGAR written with eqx"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append(ch * int(num))
            num = ""
    return "".join(out)


def map_reads(targets, reads, align=False, band=63, eqx=False, ext_band=31, ext_drop=40, ext_max=2000, memo=None, **params):
    """map_spec.map_reads (align=False) or map_align_spec.map_reads (align=True) with both ends of every line extended (memo: a dict the
    caller keeps between calls with the same targets and parameters): {"paf", "info",
    "align" (with align), "extend": counters, "base": the same run's PAF without extension, "moves": per line (left, right) of extend()}"""
    check_params(ext_band, ext_drop, ext_max)
    if align:
        # (the aligned run gives both spellings at once: it is kept in the caller's memo beside what map_spec keeps there)
        key = ("aligned", band, tuple(sorted(params.items())), tuple(reads))
        aligned = memo[key] if memo is not None and key in memo else A.map_reads(targets, reads, band=band, eqx=True, memo=memo, **params)
        if memo is not None:
            memo[key] = aligned
        base = aligned if eqx else dict(aligned, paf=aligned["other"], other=aligned["paf"])
        spelled = aligned["paf"].splitlines()              # the chain's columns are read from the = X I D spelling
    else:
        base = M.map_reads(targets, reads, memo=memo, **params)
        spelled = None
    rows = base["paf"].splitlines()
    info = dict.fromkeys(COUNTERS, 0)
    out, moves, at = [], [], 0
    for name, seq in reads:
        seq = seq.upper()
        for tname, rel, tp, c in base["lines"].get(name, ()):
            f = rows[at].split("\t")
            at += 1
            assert f[0] == name and f[5] == tname
            tseq = targets[c["t"]][1].upper()
            left, right = ends_of(tseq, seq if rel == 0 else M.revcomp(seq), c, ext_band, ext_drop, ext_max)
            tstart, tend, qs, qe = c["tstart"] - left["ei"], c["tend"] + right["ei"], c["qs"] - left["ej"], c["qe"] + right["ej"]
            assert 0 <= tstart <= tend <= len(tseq) and 0 <= qs <= qe <= len(seq)
            f[2], f[3] = (str(qs), str(qe)) if rel == 0 else (str(len(seq) - qe), str(len(seq) - qs))
            f[7], f[8] = str(tstart), str(tend)
            if align:
                columns = left["columns"][::-1] + columns_of(spelled[at - 1].split("\t")[-1][5:]) + right["columns"]
                n = {op: columns.count(op) for op in "=XID"}
                f[9], f[10] = str(n["="]), str(len(columns))
                f[-2], f[-1] = "NM:i:%d" % (n["X"] + n["I"] + n["D"]), "cg:Z:" + cigar(columns, eqx)
            else:
                f[9], f[10] = str(c["nmatch"] + left["m"] + right["m"]), str(max(tend - tstart, qe - qs))
            out.append("\t".join(f) + "\n")
            moves.append((left, right))
            info["lines"] += 1
            for e in (left, right):
                info["ends_moved"] += e["ei"] + e["ej"] > 0
                info["target_gained"] += e["ei"]
                info["read_gained"] += e["ej"]
                info["matches"] += e["m"]
                info["antidiagonals"] += e["steps"]
                info["cells"] += e["cells"]
                info["longest"] = max(info["longest"], e["ei"] + e["ej"])
    assert at == len(rows)
    result = {"paf": "".join(out), "info": base["info"], "extend": info, "base": base["paf"], "moves": moves, "lines": base["lines"]}
    if align:
        result["align"] = base["align"]
    return result
