"""Crafted molecules and parameter sweeps for the boundary tests of the molecule transforms (TEST INFRASTRUCTURE ONLY; imported by
tests/test_mdf_edges.py, no fixtures in here).

The random corpora of the other test modules draw segment sizes from 1..600 and cut positions from a normal or KDE draw, so whether a
cut meets a segment boundary, an empty segment or the min_val = 100 clamp is left to chance.  Here every such meeting is made on purpose:
  * `crafted_text()`: 49 records (54 molecules once depth is unrolled) built from the segment sizes {0, 1, 2, 30, 50, 64, 65, 101} on both
    strands (total sizes 101..230), plus 130 -- a 5' cut and a 3' cut inside ONE segment need a segment of at least 102 bases, because truncate() never keeps fewer than
    100 -- with empty segments first / in the middle / doubled / last, literals, a single segment, no segment at all, empty segments only,
    depth > 1 and header comments; every non-empty segment carries 0-3 substitutions by a fixed rule (unsorted, duplicate positions,
    position 0 and position size - 1);
  * `kde_model(T, S)`: a truncation model file whose draws are the constants T (truncation length) and S (3' share);
  * `sweep_3p()` / `sweep_kde()`: the specification's outputs over every cut length / every boundary-meeting T, cached, with the classes
    of (molecule, cut) pairs that `coverage()` counts.
Everything is a pure function of constants: two calls give the same text."""
import functools

import numpy as np

import mdf_ops_oracle as mo

SIZES = (0, 1, 2, 30, 50, 64, 65, 101, 130)
LITERAL = "ACGTTGCATGCCATGAACGTTAGCCTAGGA"                              # 30 letters; the k-th segment of a molecule uses it rotated by k
BARCODES = ("ACGTACGTAC", "TTGACCATGA", "GGGCCCAAAT")
MIN_VAL = 100                                                          # truncate()'s default (src/truncate.cpp:23)

# (segments "size strand" with L = the 30-letter literal, depth, header comment)
PATTERNS = [
    ("101+", 1, ""), ("101-", 1, "tid=ENST7;CB=ACGT;"), ("50+ 64-", 1, "z;a=1,2;"), ("65- 50+", 1, ""), ("30+ 50- 30+", 1, ""),
    # empty segments: first, last, in the middle, doubled, around everything
    ("0+ 101+", 1, ""), ("101- 0-", 1, ""), ("50+ 0- 64+", 1, "tid=ENST7;CB=ACGT;"), ("50- 0+ 0- 64-", 1, ""), ("0+ 0+ 50+ 65- 0- 0+", 1, "z;a=1,2;"),
    # ... exactly at the clamp (100 bases before them) and further in, where a cut can land on them
    ("50+ 50- 0+ 30+", 1, ""), ("64+ 30- 2+ 2- 2+ 0- 30+", 1, ""), ("101+ 0+ 30-", 1, ""), ("64+ 50- 0+ 0- 65+", 1, "x=1;"),
    ("101- 0- 1+ 0+ 2-", 1, ""), ("50+ 65- 0+ 50-", 1, ""), ("65- 65+ 0- 0+ 0- 64+", 1, ""), ("30+ 30- 50+ 0+ 101-", 1, ""),
    # one- and two-base segments next to long ones
    ("1+ 101-", 1, ""), ("101+ 1-", 1, ""), ("2- 101+ 2+", 1, ""), ("1+ 2- 30+ 50- 64+", 1, ""), ("2+ 2- 101- 1+ 1-", 1, ""),
    ("50- 1+ 50+ 1- 2+", 1, ""), ("65+ 0+ 1- 0- 65-", 1, ""), ("50+ 50- 1+", 1, ""), ("0- 50+ 0+ 50- 0+ 1+", 1, ""),
    ("64- 65+ 101-", 1, "tid=ENST7;CB=ACGT;"), ("30+ 30- 30+ 30-", 1, ""), ("101- 101+", 1, "z;a=1,2;"), ("30- 64+ 0+ 65+", 1, ""),
    ("65- 65- 65-", 1, ""), ("101+ 30- 50+", 1, ""), ("64+ 64+", 1, ""), ("65- 64+", 1, ""),
    # literals
    ("50+ L+ 30-", 1, ""), ("65- L- 50+", 1, "a=7;"), ("L+ L+ L- 30+", 1, ""),
    # no segments, empty segments only
    ("", 1, "x=1;"), ("", 2, ""), ("0+ 0- 0+", 1, ""), ("0-", 1, "z;"),
    # depth > 1: the copies are named id_0, id_1, ...
    ("50+ 65-", 3, "tid=ENST7;CB=ACGT;"), ("0+ 64- 0- 50+", 2, ""),
    # a segment long enough to hold both cuts of the two-pass truncation
    ("130+", 1, ""), ("130-", 1, "z;"), ("30+ 130- 30+", 1, ""), ("130+ 65-", 1, ""), ("1+ 130+ 1-", 2, ""),
]


def genome():
    rs = np.random.RandomState(21)
    return {f"chr{i + 1}": rs.choice(np.frombuffer(b"ACGT", np.uint8), 70_000).tobytes().decode() for i in range(2)}


def _substitutions(v, sz):
    """0-3 substitutions of a segment of sz > 0 bases: unsorted lists, duplicate positions, position 0 and position sz - 1"""
    return [[], [(0, "A")], [(sz - 1, "C"), (0, "G")], [(sz // 2, "T"), (sz // 2, "A"), (0, "C")], [(sz - 1, "G")],
            [(min(sz - 1, sz // 3 + 1), "A"), (sz // 3, "C"), (sz - 1, "T")]][v % 6]


def crafted_text(cb=False, only=None):
    """the crafted molecules as MDF text; cb: every molecule gets a CB comment (a barcode, or bare `CB;` = no barcode) for scb; only: the
    patterns with these indices alone"""
    lines = []
    for i, (pattern, depth, comment) in enumerate(PATTERNS):
        if only is not None and i not in only:
            continue
        if cb and "CB" not in comment:
            comment += "CB;" if i % 5 == 4 else f"CB={BARCODES[i % 3]};"
        lines.append(f"+e{i}\t{depth}\t{comment}\n")
        for k, tok in enumerate(pattern.split()):
            strand = tok[-1]
            if tok[0] == "L":
                name, start, sz = LITERAL[k:] + LITERAL[:k], 0, len(LITERAL)
            else:
                name, start, sz = f"chr{1 + (i + k) % 2}", 500 + 1400 * i + 150 * k, int(tok[:-1])
                assert sz in SIZES
            mods = ",".join(f"{p}{b}" for p, b in _substitutions(i + k, sz)) if sz else ""
            lines.append(f"{name}\t{start}\t{start + sz}\t{strand}\t{mods}\n")
    return "".join(lines)


@functools.lru_cache(maxsize=None)
def crafted_molecules(cb=False, only=None):
    return tuple(mo.stream_mdf(crafted_text(cb, only), unroll=True))


# a small batch for the runs across molecule index 2^32: 21 molecules, depth 3 and 2 and literals among them
INDEX_PATTERNS = (0, 1, 2, 3, 4, 7, 13, 21, 27, 29, 35, 36, 42, 43, 44, 45, 46, 47)


def pcr_templates_text(n=200):
    """three segments each: plus, EMPTY, minus with a substitution"""
    return "".join(f"+t{u}\t1\t\nchr1\t{300 * u}\t{300 * u + 60 + u % 7}\t+\t\nchr2\t{100 + u}\t{100 + u}\t+\t\n"
                   f"chr2\t{200 * u}\t{200 * u + 40 + u % 5}\t-\t{u % 40}A\n" for u in range(n))


def pcr_long_templates_text(n=12):
    """350 bases in one or two segments, a substitution of their own"""
    return "".join(f"+w{u}\t1\t\n" + (f"chr1\t{1000 * u}\t{1000 * u + 350}\t{'+-'[u & 1]}\t7C\n" if u % 3 else
                                      f"chr1\t{1000 * u}\t{1000 * u + 200}\t-\t199C\nchr2\t{1000 * u}\t{1000 * u + 150}\t+\t\n") for u in range(n))


def pcr_small_text():
    """molecules of 0..5 bases, empty segments among them"""
    pats = ["1+", "1-", "2+", "1+ 1-", "3-", "0+ 2+ 0- 1-", "4+", "2- 2+", "5-", "1+ 0+ 1- 0- 1+ 1- 1+", "", "0+", "0+ 0-", "2+ 0+ 3-"]
    out = []
    for i, p in enumerate(pats):
        out.append(f"+s{i}\t{2 if i == 3 else 1}\t\n")
        for k, tok in enumerate(p.split()):
            st = 40 * i + 6 * k
            out.append(f"chr{1 + (i + k) % 2}\t{st}\t{st + int(tok[:-1])}\t{tok[-1]}\t{'0G' if tok[:-1] != '0' and (i + k) % 2 else ''}\n")
    return "".join(out)


# ------------------------------------------------------------------------------------------------ truncation sweeps
def kde_model(T, S):
    """The JSON parts of a truncation model whose draws are constants.  KDE_mtx: x labels [T, T], y labels [0, 200], weights [[1, 0], [0, 1]]
    -- a molecule of more than 100 bases reads the LAST row (no averaging with a next row), whose only populated bin spans [T, T].
    end_mtx: weights [0, 1] over the labels [S, S]: the populated bin spans [S, S]."""
    return [dict(name="KDE_mtx", shape=[2, 2], data=[1, 0, 0, 1], labels=[T, T, 0, 200]), dict(name="end_mtx", shape=[2], data=[0, 1], labels=[S, S])]


def boundaries(md):
    out, c = [0], 0
    for s in md["segments"]:
        c += mo.seg_size(s)
        out.append(c)
    return out


def max_size():
    return max(mo.mol_size(md) for md in crafted_molecules())


def cut_lengths():
    """3' sweep: every post-truncation length from below the clamp to beyond the largest molecule"""
    return list(range(MIN_VAL - 2, max_size() + 3))


def kde_lengths():
    """truncation lengths that put a 5' cut (S = 0) or a 3' cut (S = 1, or --kde-models-length) on every segment boundary of every
    crafted molecule and one base to either side"""
    ts = {0, 1, 2, max_size()}
    for md in crafted_molecules():
        size = mo.mol_size(md)
        for b in boundaries(md):
            for d in (-1, 0, 1):
                ts.update((b + d, size - b + d))
    return sorted(t for t in ts if 0 <= t <= max_size())


KDE_SIDES = (0.0, 0.25, 0.5, 1.0)
SEED_3P, SEED_KDE, FIRST = 17, 23, 1000


@functools.lru_cache(maxsize=None)
def sweep_3p(L):
    """the specification's molecules for normal=(L, 0): the post-truncation length is L for every molecule"""
    return tuple(mo.trc_spec(md, FIRST + g, SEED_3P, normal=(float(L), 0.0)) for g, md in enumerate(crafted_molecules()))


@functools.lru_cache(maxsize=None)
def sweep_kde(T, S, models_length):
    model = mo.TruncationModel(kde_model(T, S))
    return tuple(mo.trc_spec(md, FIRST + g, SEED_KDE, model=model, models_length=models_length) for g, md in enumerate(crafted_molecules()))


def _unsorted_kept(seg_in, seg_out):
    """the substitutions of seg_in that fall into seg_out, re-based, in their ORIGINAL order"""
    off, n = seg_out["start"] - seg_in["start"], seg_out["end"] - seg_out["start"]
    return [(p - off, b) for p, b in seg_in["errors"] if 0 <= p - off < n]


def classes_3p(md, L, out):
    """classes of one (molecule, cut length) pair of the 3' sweep, read off the specification's output `out`"""
    size, kept = mo.mol_size(md), mo.mol_size(out)
    cls = set()
    if L < MIN_VAL:
        cls.add("length below the clamp")
    if L == size:
        cls.add("length equals the size")
    if L > size:
        cls.add("length above the size")
    if kept == size:
        return cls
    c = 0
    for s in md["segments"]:
        sz = mo.seg_size(s)
        if sz and c < kept < c + sz:
            cls.add("inside a plus segment" if s["plus"] else "inside a minus segment")
        if sz == 0 and c == kept:
            cls.add("at an empty segment")
        c += sz
    if kept in boundaries(md):
        cls.add("on a boundary")
    j = len(out["segments"]) - 1                                       # truncate() drops everything behind the cut segment
    want = _unsorted_kept(md["segments"][j], out["segments"][j])
    if out["segments"][j]["errors"] != want:
        assert out["segments"][j]["errors"] == sorted(want, key=lambda e: e[0])
        cls.add("substitutions re-sorted")
        if kept in boundaries(md):
            cls.add("re-sorted with the cut on the boundary")
    return cls


def both_cuts_in_one_segment(md, out):
    """an output segment that lies strictly inside the input segment it came from: cut at its 5' and at its 3' side"""
    for o in out["segments"]:
        for s in md["segments"]:
            if o["end"] > o["start"] and s["chr"] == o["chr"] and s["plus"] == o["plus"] and s["start"] < o["start"] and o["end"] < s["end"]:
                return True
    return False


CLASSES = ("inside a plus segment", "inside a minus segment", "on a boundary", "at an empty segment", "length below the clamp", "length equals the size",
           "length above the size", "5' and 3' cut in one segment", "substitutions re-sorted",
           # the rule of k_trc_write that the cut segment is THE one whose end reaches the kept length, even when the cut falls on its boundary
           "re-sorted with the cut on the boundary")


def coverage():
    """{class: number of (molecule, cut) pairs}: the 3' sweep for all classes but the two-cut one, which is counted over the KDE sweep at
    S = 0.25 and 0.5 (both ends are cut)"""
    n = dict.fromkeys(CLASSES, 0)
    mols = crafted_molecules()
    for L in cut_lengths():
        for md, out in zip(mols, sweep_3p(L)):
            for c in classes_3p(md, L, out):
                n[c] += 1
    for S in (0.25, 0.5):
        for T in kde_lengths():
            for md, out in zip(mols, sweep_kde(T, S, False)):
                n["5' and 3' cut in one segment"] += both_cuts_in_one_segment(md, out)
    return n
