"""The rules of `tksm map -c` (include/tksmseq.h, "map, alignment") in plain Python, written from that text and not from the kernels: the
anchors of a written chain as waypoints, the banded unit-cost alignment of a segment with its traceback order, the columns of a line, its
CIGAR and its counters.  Everything else of map comes from tests/map_spec.py.  tests/test_map_align.py pins this file against an
independent Levenshtein and hand-worked cases; tests/test_map_align_gpu.py compares the device with it byte for byte."""
import functools
import os
import random

import numpy as np

import map_spec as M

INF = 1 << 29
COUNTERS = ("lines", "segments", "longest_segment", "cells", "columns", "matches", "mismatches", "inserted", "deleted")
MAX_GAP = 65536


def band_rows(dt, dq, W):
    """[(s, first i, last i)] of the allowed cells of every anti-diagonal of a dt x dq segment (last < first: none)"""
    S = dt + dq
    out = []
    for s in range(S + 1):
        lo = max(0, s - dq, -((W * S - 2 * s * dt) // (2 * S)))      # the smallest i with 2 (i S - s dt) >= -W S
        hi = min(dt, s, (2 * s * dt + W * S) // (2 * S))
        out.append((s, lo, hi))
    return out


def allowed(i, j, dt, dq, W):
    return 2 * abs(i * dq - j * dt) <= W * (dt + dq)


def codes(letters, other):
    """letters as small integers; a letter outside ACGT gets `other`, so that it equals nothing in a sequence coded with another `other`"""
    return np.array([M.CODE.get(c, other) for c in letters], dtype=np.int64)


def align_segment(T, Q, W=63):
    """the columns (a string over = X I D), D[dt][dq] and the number of allowed cells of T against Q"""
    dt, dq = len(T), len(Q)
    assert dt > 0 and dq > 0 and 1 <= W <= 63
    t, q = codes(T, 4), codes(Q, 5)
    rows = band_rows(dt, dq, W)
    cells = 0
    vals, dirs = [], []                                  # per anti-diagonal: (first i, values), (first i, codes 0 = 1 X 2 I 3 D)

    def look(row, idx):
        lo, v = row
        k = idx - lo
        ok = (k >= 0) & (k < len(v))
        return np.where(ok, v[np.clip(k, 0, max(len(v) - 1, 0))] if len(v) else INF, INF)

    empty = (0, np.zeros(0, dtype=np.int64))
    for s, lo, hi in rows:
        if hi < lo:
            vals.append(empty)
            dirs.append(empty)
            continue
        i = np.arange(lo, hi + 1)
        j = s - i
        cells += len(i)
        if s == 0:
            vals.append((0, np.zeros(1, dtype=np.int64)))
            dirs.append((0, np.zeros(1, dtype=np.int64)))
            continue
        one, two = vals[s - 1], vals[s - 2] if s >= 2 else empty
        both = (i > 0) & (j > 0)
        miss = np.where(both, (t[np.clip(i - 1, 0, dt - 1)] != q[np.clip(j - 1, 0, dq - 1)]).astype(np.int64), 1)
        d = np.where(both, look(two, i - 1) + miss, INF)
        u = np.where(i > 0, look(one, i - 1) + 1, INF)
        w = np.where(j > 0, look(one, i) + 1, INF)
        best = np.minimum(np.minimum(d, u), np.minimum(w, INF))
        code = np.where(d == best, miss, np.where(u == best, 3, 2))
        vals.append((lo, best))
        dirs.append((lo, code))
    i, j, out = dt, dq, []
    while i or j:
        lo, code = dirs[i + j]
        c = int(code[i - lo])
        out.append("=XID"[c])
        if c < 2:
            i, j = i - 1, j - 1
        elif c == 3:
            i -= 1
        else:
            j -= 1
        assert i >= 0 and j >= 0
    lo, v = vals[dt + dq]
    return "".join(reversed(out)), int(v[dt - lo]), cells


def cigar(columns, eqx):
    ops = columns if eqx else columns.replace("=", "M").replace("X", "M")
    out, a = [], 0
    while a < len(ops):
        b = a
        while b < len(ops) and ops[b] == ops[a]:
            b += 1
        out.append("%d%s" % (b - a, ops[a]))
        a = b
    return "".join(out)


def groups_of(seq, index, p):
    """{(t, rel): the anchors [(p, qa)] by (p, qa)} of one read, as map_spec.map_read forms them"""
    k, groups = p["k"], {}
    for h, q, sr in M.minimizers(seq, k, p["w"]):
        hits = index.get(h, ())
        if len(hits) > p["max_occ"]:
            continue
        for t, tp, st in hits:
            rel = sr ^ st
            groups.setdefault((t, rel), []).append((tp, q if rel == 0 else len(seq) - k - q))
    return {g: sorted(a) for g, a in groups.items()}


def align_chain(tseq, seq, rel, anchors, k, W=63):
    """the waypoints of a chain -> (columns, NM, [dt + dq of its segments], cells)"""
    strand = seq if rel == 0 else M.revcomp(seq)         # (revcomp leaves a letter outside ACGT as it is: it matches nothing either way)
    points = list(anchors) + [(anchors[-1][0] + k, anchors[-1][1] + k)]
    columns, nm, spans, cells = [], 0, [], 0
    for (p0, q0), (p1, q1) in zip(points, points[1:]):
        assert p1 > p0 and q1 > q0
        col, d, n = align_segment(tseq[p0:p1], strand[q0:q1], W)
        columns.append(col)
        nm += d
        spans.append(p1 - p0 + q1 - q0)
        cells += n
    return "".join(columns), nm, spans, cells


def map_reads(targets, reads, band=63, eqx=False, memo=None, **params):
    """map_spec.map_reads with every line aligned: {"paf", "info", "align": counters, "plain": the same run's plain PAF, "other": the PAF with
    eqx the other way, "nm": {read name: NM of its primary}, "shapes": the (dt, dq) of all segments, "lines": those of the plain run}"""
    p = dict(M.DEFAULTS, **params)
    if not 1 <= band <= 63 or p["max_gap"] > MAX_GAP:
        raise ValueError("map: a parameter out of range")
    plain = M.map_reads(targets, reads, memo=memo, **params)          # (memo: see M.map_reads)
    index, _ = M.build_index([s for _, s in targets], p["k"], p["w"])
    info = dict.fromkeys(COUNTERS, 0)
    rows = plain["paf"].splitlines()
    out, other, at, memo, nms, shapes = [], [], 0, {}, {}, set()
    for name, seq in reads:
        seq = seq.upper()
        if name not in plain["lines"]:
            continue
        if seq not in memo:
            groups = groups_of(seq, index, p)
            memo[seq] = []
            for tname, rel, tp, c in plain["lines"][name]:
                anchors = [groups[(c["t"], rel)][i] for i in c["path"]]
                assert anchors[0] == (c["tstart"], c["qs"]) and anchors[-1] == (c["tend"] - p["k"], c["qe"] - p["k"]) and targets[c["t"]][0] == tname
                shapes.update((b[0] - a[0], b[1] - a[1]) for a, b in zip(anchors, anchors[1:]))
                memo[seq].append(align_chain(targets[c["t"]][1].upper(), seq, rel, anchors, p["k"], band))
        for i, (columns, nm, spans, cells) in enumerate(memo[seq]):
            f = rows[at].split("\t")
            at += 1
            assert f[0] == name
            n = {op: columns.count(op) for op in "=XID"}
            assert nm == n["X"] + n["I"] + n["D"]
            f[9], f[10] = str(n["="]), str(len(columns))
            out.append("\t".join(f + ["NM:i:%d" % nm, "cg:Z:" + cigar(columns, eqx)]) + "\n")
            other.append("\t".join(f + ["NM:i:%d" % nm, "cg:Z:" + cigar(columns, not eqx)]) + "\n")
            if i == 0:
                nms[name] = nm
            info["lines"] += 1
            info["segments"] += len(spans)
            info["longest_segment"] = max(info["longest_segment"], max(spans))
            info["cells"] += cells
            info["columns"] += len(columns)
            info["matches"] += n["="]
            info["mismatches"] += n["X"]
            info["inserted"] += n["I"]
            info["deleted"] += n["D"]
    assert at == len(rows)
    return {"paf": "".join(out), "info": plain["info"], "align": info, "plain": plain["paf"], "other": "".join(other), "nm": nms, "shapes": shapes, "lines": plain["lines"]}


def cigar_spans(text):
    """(target letters, read letters, {op: columns}) a CIGAR consumes"""
    n, num = dict.fromkeys("M=XID", 0), ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            n[ch] += int(num)
            num = ""
    assert not num
    return n["M"] + n["="] + n["X"] + n["D"], n["M"] + n["="] + n["X"] + n["I"], n


def plant(rs, seq, rate):
    """substitutions, insertions and deletions, a third each, at `rate` per base: (letters, edits planted)"""
    out, edits = [], 0
    for c in seq:
        if rs.random() >= rate:
            out.append(c)
            continue
        edits += 1
        kind = rs.randrange(3)
        if kind == 0:
            out.append(rs.choice([x for x in "ACGT" if x != c]))
        elif kind == 1:
            out.append(c + rs.choice("ACGT"))
    return "".join(out), edits


def generate(d, seed, n_targets=8, n_reads=60, lengths=(700, 1500), read_lengths=(200, 600), error=0.08, tag="aln"):
    """random targets, and reads that are substrings of them on alternating strands with planted edits: ref.fa and reads.fq in `d`;
    planted[name] = edits"""
    rs = random.Random(seed)
    targets = [("t%03d" % i, M.random_seq(rs, rs.randint(*lengths))) for i in range(n_targets)]
    reads, planted = [], {}
    for r in range(n_reads):
        name, seq = targets[rs.randrange(n_targets)]
        n = rs.randint(*read_lengths)
        a = rs.randint(0, len(seq) - n)
        piece, edits = plant(rs, seq[a:a + n], error)
        if r % 2:
            piece = M.revcomp(piece)
        reads.append(("r%04d" % r, piece))
        planted["r%04d" % r] = edits
    return {"ref": M.write_fasta(os.path.join(str(d), tag + ".ref.fa"), targets), "reads": M.write_fastq(os.path.join(str(d), tag + ".reads.fq"), reads),
            "targets": targets, "read_list": reads, "planted": planted}


DENSE = {4: 120, 5: 200, 6: 300}                     # k: the length of its target


@functools.lru_cache(maxsize=None)
def dense_case(k):
    """-w 1 with a small k on one random target and six reads with 5 % planted edits on alternating strands: groups of some hundred anchors
    with many admissible predecessors of equal score in the window of every anchor (M.classes_of_lines says which kinds)"""
    rs = random.Random(4600 + k)
    target = M.random_seq(rs, DENSE[k])
    reads = []
    for r in range(6):
        read = plant(rs, target, 0.05)[0]
        reads.append(("d%d_%d" % (k, r), M.revcomp(read) if r % 2 else read))
    return [("dense%d" % k, target)], reads, dict(k=k, w=1, min_score=10, secondary_ratio=0.0)
