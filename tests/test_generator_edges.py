"""Boundary sweeps of the two device-side generators (tksm_amd/csrc/mdf_kernels.hip): random-wgs (k_wgs_plan / k_wgs_cut / k_wgs_write) and
tail-noise (k_noise_plan / k_noise_fill / k_pal_count / k_pal_write).

tests/test_wgs.py and tests/test_tail_noise.py compare one six-contig table and randomly drawn corpora with the specifications, which leaves
the branches below to chance or out of reach.  Here the inputs are crafted: contig tables on both sides of the LDS limit of the contig
search (2048 entries), with zero-length contigs, above 2^32 bases, grown between two calls; the stop rule met exactly; hairpins whose
length is pinned (`normal, L + 0.5, 1e-9` draws L for every molecule) on, below and above every partial sum of segment sizes that sit on
the 64-lane stride; substitutions on the window edges and beyond their segment; batches around the four-waves-per-block grid; literal
lengths around the 4-letter Philox block, runs of empty literals, the 2^20 limit.

Every device result is compared text for text with the specification (tests/wgs_spec.py; tests/noise_spec.py + write_mdf), carried state
and error codes included.  CPU part: every crafted input REACHES what it is meant to reach, counted from the specification alone, so
that a later change of a seed or a size cannot quietly empty a case (the counts are tabulated in DESIGN.md)."""
import ctypes as C
import functools

import numpy as np
import pytest

import mdf_ops_oracle as mo
import noise_spec as ns
import wgs_spec as ws

EINVAL, ESTATE, ELIMIT = 1, 5, 6
LDS_CONTIGS = 2048                                                      # WGS_LDS_CONTIGS of tksm_amd/csrc/mdf_kernels.h
N_CAND = 20_000
BIG = 2**31 - 1                                                         # the longest contig random-wgs accepts


# ================================================================================================ random-wgs: the inputs
@functools.lru_cache(None)
def _table(n, pattern):
    """n contigs: "uniform" -- 50 .. 3000 bases; "zeros" -- 5 .. 300 bases with every third contig, the first, the last two and four in a row of length 0;
    "big" -- five contigs of 2^31 - 1 bases among n small ones (more than 2^32 bases; two of them beyond the LDS limit)"""
    rs = np.random.RandomState(1000 + n)
    if pattern == "zeros":
        lens = rs.randint(5, 301, n)
        lens[::3] = 0
        lens[-2:] = 0
        lens[999:1002] = 0
    else:
        lens = rs.randint(50, 3001, n)
        if pattern == "big":
            lens[[100, 700, 1500, 2200, 2900]] = BIG
    return tuple((f"c{i}", int(l)) for i, l in enumerate(lens))


# (table size, pattern, distribution, a, b, stop, seed): seeds found by searching the reach conditions of the CPU tests below
WGS_CASES = [(n, "uniform", ws.UNIFORM, 1.0, 4000.0, ("base_count", 10**12), 66 if n == 2049 else 1) for n in (1, 2047, 2048, 2049, 5000)] + \
            [(n, "zeros", ws.NORMAL, 150.0, 120.0, ("base_count", 10**12), 2) for n in (2047, 2048, 2049, 5000)] + \
            [(2049, "uniform", ws.UNIFORM, 1.0, 4000.0, ("depth", 2.0), 3), (2049, "zeros", ws.NORMAL, 150.0, 120.0, ("depth", 1.5), 4),
             (3000, "big", ws.UNIFORM, 1.0, 4000.0, ("base_count", 10**12), 5), (3000, "big", ws.NORMAL, 3000.0, 2500.0, ("depth", 0.001), 6)]
WGS_IDS = [f"{n}-{pat}-{dist}-{stop[0]}" for n, pat, dist, _, _, stop, _ in WGS_CASES]


def _base_count(stop, table):
    return stop[1] if stop[0] == "base_count" else ws.depth_to_base_count(stop[1], table)


@functools.lru_cache(None)
def _wgs_want(case):
    n, pat, dist, a, b, stop, seed = case
    return ws.wgs_spec(seed, _table(n, pat), dist, a, b, base_count=_base_count(stop, _table(n, pat)), n_candidates=N_CAND)


def _reach(case):
    """what the N_CAND candidates of a case hit, from the specification alone"""
    n, pat, dist, a, b, _, seed = case
    table = _table(n, pat)
    lens = np.array([l for _, l in table], np.int64)
    idx, ref_pos, fl, _ = ws.wgs_candidates_spec(seed, 0, N_CAND, table, dist, a, b)
    begin = np.cumsum(lens) - lens
    at_end = ref_pos == lens[idx]
    nxt = np.minimum(idx + 1, n - 1)
    return {"below": int((idx < LDS_CONTIGS).sum()), "above": int((idx >= LDS_CONTIGS).sum()), "first": int((idx == 0).sum()),
            "last": int((idx == n - 1).sum()), "at_end": int(at_end.sum()), "emitted": int((fl >= 1).sum()), "clipped": int(((fl >= 1) & (fl == lens[idx] - ref_pos)).sum()),
            "tie": int((at_end & (idx + 1 < n) & (lens[nxt] == 0)).sum()), "zero_tables": int((lens == 0).sum()),
            "zero_hit": int((lens[idx] == 0).sum()), "zero_emitted": int(((lens[idx] == 0) & (fl >= 1)).sum()),
            "pos_above_2_32": int((begin[idx] + ref_pos >= 2**32).sum()),
            "small_after_big": int(((lens[idx] < BIG) & (begin[idx] >= BIG)).sum()), "in_big": int((lens[idx] == BIG).sum())}


# the stop rule: the 2049-contig table (global-memory search), uniform lengths
STOP_CASE = (2049, "uniform", ws.UNIFORM, 1.0, 4000.0, 7)
STOP_K = 40                                                             # the emitted candidate whose running sums S' (before) and S (after) are met


@functools.lru_cache(None)
def _stop_sums():
    n, pat, dist, a, b, seed = STOP_CASE
    _, _, fl, _ = ws.wgs_candidates_spec(seed, 0, 2000, _table(n, pat), dist, a, b)
    em = np.flatnonzero(fl >= 1)
    cum = np.cumsum(fl[em])
    return int(cum[STOP_K - 1]), int(cum[STOP_K]), int(em[STOP_K]), int(fl[em[STOP_K]]), int(fl[em[STOP_K + 1]])


def _stop_runs():
    """(name, base_count, first_candidate, (molecules, bases_before))"""
    s_before, s_after, _, _, _ = _stop_sums()
    return [("one base", 1, 0, (0, 0)), ("S'", s_before, 0, (0, 0)), ("S' + 1", s_before + 1, 0, (0, 0)), ("S", s_after, 0, (0, 0)), ("S + 1", s_after + 1, 0, (0, 0)),
            ("carried, one base owed", s_after, 1000, (17, s_after - 1)), ("carried, one base owed at 1", 1, 5, (3, 0)),
            ("carried, nothing owed", s_after, 1000, (17, s_after)), ("carried, more than owed", s_after, 1000, (17, s_after + 5))]


@functools.lru_cache(None)
def _stop_want(base_count, first, state):
    n, pat, dist, a, b, seed = STOP_CASE
    return ws.wgs_spec(seed, _table(n, pat), dist, a, b, base_count=base_count, first_candidate=first, n_candidates=N_CAND, state=state)


# ------------------------------------------------------------------------------------------------ random-wgs: CPU
def test_wgs_tables_are_what_they_are_meant_to_be():
    for n in (2047, 2048, 2049, 5000):
        lens = [l for _, l in _table(n, "zeros")]
        assert lens[0] == lens[-1] == 0 and all(l == 0 for l in lens[::3]) and n // 3 < sum(l == 0 for l in lens) <= n // 3 + 5 and sum(lens) > 0
        assert lens[-2] == 0 and not any(lens[999:1003]) and lens[998] and lens[1003]      # runs of two and of four
        assert min(l for _, l in _table(n, "uniform")) >= 50 and len(_table(n, "uniform")) == n
    big = [l for _, l in _table(3000, "big")]
    assert sum(big) > 2**32 and sum(l == BIG for l in big) == 5 and max(big) < 2**31 and sum(l == BIG for l in big[LDS_CONTIGS:]) == 2
    assert len({c[:2] for c in WGS_CASES}) == 10 and {c[5][0] for c in WGS_CASES} == {"base_count", "depth"} and {c[2] for c in WGS_CASES} == {ws.UNIFORM, ws.NORMAL}


@pytest.mark.parametrize("case", WGS_CASES, ids=WGS_IDS)
def test_wgs_cases_reach_their_branches(case):
    n, pat = case[:2]
    r = _reach(case)
    print(f"{WGS_IDS[WGS_CASES.index(case)]}: {r}")
    assert r["below"] > 0 and r["emitted"] > N_CAND // 4 and r["clipped"] > 0
    assert r["below"] + r["above"] == N_CAND
    assert (r["above"] > 0) == any(l for _, l in _table(n, pat)[LDS_CONTIGS:])          # (2049 "zeros": the table is searched in global memory, its last two contigs are empty)
    if pat == "uniform":
        assert r["first"] > 0 and r["last"] > 0
    if n > 1 and pat != "big":                                          # (above 2^32 bases a draw meets one of 3000 sums once in 10^6 calls)
        assert r["at_end"] > 0                                          # candidates with ref_pos == len: pos sits ON a running sum
    if pat == "zeros":
        assert r["zero_tables"] > n // 3 and r["tie"] > 0               # ... on a running sum that the next contig repeats
        assert r["zero_emitted"] == 0 and r["zero_hit"] == r["first"] and r["last"] == 0       # (pos == 0 lands on the empty first contig)
    if pat == "big":
        assert r["pos_above_2_32"] > N_CAND // 2 and r["small_after_big"] > 0 and r["in_big"] > 0 and r["above"] > 0
    text, st = _wgs_want(case)
    assert st["reached"] == (case[5][0] == "depth") and st["molecules"] == text.count("\n+") + 1 > 100
    if st["reached"]:
        assert 100 < st["next_candidate"] < N_CAND


def test_wgs_stop_rule_cases_meet_the_sums_exactly():
    s_before, s_after, cand, length, next_length = _stop_sums()
    assert s_after - s_before == length >= 2 and next_length >= 2         # S' + 1 and S + 1 lie strictly inside a fragment
    want = {"one base": (1, None, 0), "S'": (STOP_K, s_before, 0), "S' + 1": (STOP_K + 1, s_after, 0), "S": (STOP_K + 1, s_after, 0),
            "S + 1": (STOP_K + 2, s_after + next_length, 0), "carried, one base owed": (18, None, 1000), "carried, one base owed at 1": (4, None, 5),
            "carried, nothing owed": (17, s_after, 1000), "carried, more than owed": (17, s_after + 5, 1000)}
    for name, base_count, first, state in _stop_runs():
        text, st = _stop_want(base_count, first, state)
        mols, bases, first_cand = want[name]
        assert st["reached"] and st["molecules"] == mols and text.count("\n+") + (1 if text else 0) == mols - state[0], name
        assert bases is None or st["bases"] == bases, name
        if mols == state[0]:
            assert text == "" and st["next_candidate"] == first_cand, name      # nothing owed: no candidate taken
        else:
            assert st["next_candidate"] > first_cand and st["bases"] >= base_count, name
    assert _stop_want(s_after, 0, (0, 0))[1]["next_candidate"] == cand + 1
    assert _stop_want(s_after, 0, (0, 0))[1]["bases"] == s_after                # before + len == base_count, met exactly


# ================================================================================================ tail-noise: the inputs
SIZES = (0, 1, 63, 64, 65, 127, 128, 129, 200)
HAIRPIN_L = (1, 63, 64, 65, 128, 129, 193, 257, 10**6)
RATES = (0.0, 0.5, 1.0)
PAL_SEED, PAL_FIRST = 17, 12345


def _roundup64(n):
    return -(-n // 64) * 64


def _edge_errors(size, k, beyond):
    """substitutions on the edges of the 64-lane windows and of the segment, listed unsorted and with one position twice"""
    pos = [size + 1000, 64, 0, _roundup64(size), size - 1, 63, size, size + 1, _roundup64(size) - 1, 64]
    pos = [p for p in pos if p >= 0 and (beyond or p < size)]
    return [(p, "ACGT"[(k + j) & 3]) for j, p in enumerate(pos)]


def _many_errors(size, n, k, beyond):
    """n substitutions of one segment, unsorted, two positions twice; beyond: four of them past the end"""
    perm = [int(p) for p in np.random.RandomState(500 + n + k).permutation(size)]
    pos = perm[:n - 6] + [size, size + 55, size + 56, size + 1000] + perm[:2] if beyond else perm[:n - 2] + perm[:2]
    pos = [pos[i] for i in np.random.RandomState(600 + n + k).permutation(len(pos))]
    return [(p, "ACGT"[(k + j) & 3]) for j, p in enumerate(pos)]


def _literal(size, k):
    if size == 0:
        return "ACGT", 2, 2                                             # a literal segment of no base
    return "".join("ACGT"[int(x)] for x in np.random.RandomState(700 + k).randint(0, 4, size)), 0, size


@functools.lru_cache(None)
def _hairpin_corpus(subs, beyond=True):
    """Molecules whose last three segments have sizes (a, b, c), b and c over SIZES, twice each: once with a chosen so that the molecule
    is exactly as long as the next L of HAIRPIN_L (a zero-size first segment where b + c is one already), once with a = 100 and the
    strands and kinds (contig / literal) of b and c exchanged; a molecule of empty segments only and one without segments; with `subs`
    every segment carries _edge_errors, and four more molecules have a segment with 70 and one with 140 substitutions.  beyond=False
    keeps the substitutions inside their segments (what batch_from_mdf accepts and k_simulate reads)."""
    mols, k = [], 0
    for b in SIZES:
        for c in SIZES:
            for v in (0, 1):
                a = 100 if v else next((L - b - c for L in HAIRPIN_L[:-1] if L >= b + c), 7)
                segs = []
                for j, size in enumerate((a, b, c)):
                    plus = bool(((k >> j) & 1) ^ v)
                    if j and (k // 9 + k % 9 + j + v) % 3 == 0:
                        name, start, end = _literal(size, 3 * k + j)
                    else:
                        name, start = f"chr{1 + ((k + j) & 1)}", 1000 + 37 * k + 300 * j
                        end = start + size
                    segs.append(dict(chr=name, start=start, end=end, plus=plus, errors=_edge_errors(size, k + j, beyond) if subs else []))
                mols.append(dict(id=f"s{a}_{b}_{c}_{v}", depth=1, meta={}, segments=segs))
            k += 1
    mols.append(dict(id="empty_segments", depth=1, meta={}, segments=[dict(chr="chr1", start=5, end=5, plus=True, errors=_edge_errors(0, 1, beyond) if subs else []),
                                                                       dict(chr="chr2", start=9, end=9, plus=False, errors=[]), dict(chr="ACGT", start=1, end=1, plus=True, errors=[])]))
    mols.append(dict(id="no_segment", depth=1, meta={}, segments=[]))
    if subs:
        for v in range(4):                                              # sizes (100, 200, 200): 70 substitutions in b, 140 in c; all strand pairs
            segs = [dict(chr="chr1", start=2000, end=2100, plus=True, errors=_edge_errors(100, v, beyond)),
                    dict(chr="chr2", start=3000 + v, end=3200 + v, plus=bool(v & 1), errors=_many_errors(200, 70, v, beyond)),
                    dict(chr="chr1", start=4000 + v, end=4200 + v, plus=bool(v & 2), errors=_many_errors(200, 140, v, beyond))]
            mols.append(dict(id=f"many_{v}", depth=1, meta={}, segments=segs))
    return mols


def _same_length(L):
    """(mu, sigma) of the normal distribution that draws L for every molecule (|z| of Box-Muller on 32-bit words is below 7)"""
    return float(L) + 0.5, 1e-9


@functools.lru_cache(None)
def _hairpin_want(subs, L, rate):
    mu, sigma = _same_length(L)
    return mo.write_mdf(ns.noise_spec(_hairpin_corpus(subs), PAL_SEED, ns.NORMAL, mu, sigma, True, rate, "AGTC", first=PAL_FIRST))


def _classify(md, L):
    """how the walk of src/append_noise.cpp:93-107 ends for a molecule and a length: the segment that is cut (None: none), and the class"""
    total = 0
    for s in reversed(md["segments"]):
        size = mo.seg_size(s)
        total += size
        if total > L:
            extra = total - L
            return s, extra, "cut to nothing" if extra == size else ("cut, plus original" if s["plus"] else "cut, minus original")
    return None, 0, "uncut, L == molecule" if total == L else "uncut, L above the molecule"


CLASSES = ("cut, plus original", "cut, minus original", "cut to nothing", "uncut, L == molecule", "uncut, L above the molecule")


def _hairpin_reach(subs):
    """per L the molecules of each class; over the sweep the copied substitutions a cut keeps and drops, those beyond their (uncut)
    segment in the last 64-window and past it, and the cut copies that keep more than 64 / 128 -- counted from the walk and checked
    against the specification's own output"""
    mols = _hairpin_corpus(subs)
    per_l = {L: dict.fromkeys(CLASSES, 0) for L in HAIRPIN_L}
    n = dict.fromkeys(("kept by a cut", "dropped by a cut", "beyond, in the last window", "beyond, past the last window", "cut copies with > 64 kept",
                       "cut copies with > 128 kept", "uncut copies with > 64", "uncut copies with > 128", "cut offsets on the stride", "empty segments copied"), 0)
    for L in HAIRPIN_L:
        for md in mols:
            cut, extra, cls = _classify(md, L)
            per_l[L][cls] += 1
            new = ns.hairpin_segments_spec(md, L)
            assert sum(mo.seg_size(s) for s in new) == min(L, mo.mol_size(md))
            n["empty segments copied"] += sum(mo.seg_size(s) == 0 for s in new)
            for s in new[:-1] if cut is not None and cls != "cut to nothing" else new:            # the uncut copies
                size = mo.seg_size(s)
                n["beyond, in the last window"] += sum(size <= p < _roundup64(size) for p, _ in s["errors"])
                n["beyond, past the last window"] += sum(p >= _roundup64(size) for p, _ in s["errors"])
                n["uncut copies with > 64"] += len(s["errors"]) > 64
                n["uncut copies with > 128"] += len(s["errors"]) > 128
            if cut is not None:
                kept = len(new[-1]["errors"]) if cls != "cut to nothing" else 0
                n["kept by a cut"] += kept
                n["dropped by a cut"] += len(cut["errors"]) - kept
                n["cut copies with > 64 kept"] += kept > 64
                n["cut copies with > 128 kept"] += kept > 128
                n["cut offsets on the stride"] += extra in (63, 64, 65, 127, 128, 129) and not cut["plus"]
    return per_l, n


# small batches and odd molecules: 1 - 4 segments, minus strands, literals, substitutions, some molecules without any segment
@functools.lru_cache(None)
def _small_corpus(n=129):
    rs = np.random.RandomState(31)
    mols = []
    for i in range(n):
        segs = []
        for j in range(0 if i % 7 == 3 else int(rs.randint(1, 5))):
            size = int(rs.randint(0, 150))
            if rs.rand() < 0.25:
                name, start, end = _literal(size, 9000 + 5 * i + j)
            else:
                name, start = f"chr{int(rs.randint(1, 3))}", int(rs.randint(0, 50_000))
                end = start + size
            errs = [(int(rs.randint(0, size)), "ACGT"[int(rs.randint(0, 4))]) for _ in range(int(rs.randint(0, 4)))] if size else []
            segs.append(dict(chr=name, start=start, end=end, plus=bool(rs.randint(0, 2)), errors=errs))
        mols.append(dict(id=f"m{i}", depth=1, meta={}, segments=segs))
    return mols


BATCH_SIZES = (1, 3, 4, 5, 127, 128, 129)
SMALL_MODES = {"palindromic": dict(dist=ns.NORMAL, mu=120.0, sigma=90.0, palindromic=True, error_rate=0.5, alphabet="AGTC"),
               "random": dict(dist=ns.NORMAL, mu=20.0, sigma=12.0, palindromic=False, error_rate=0.5, alphabet="AGTC")}


def _noise_want(mols, seed, first, dist, mu, sigma, palindromic, error_rate, alphabet):
    return mo.write_mdf(ns.noise_spec(mols, seed, dist, mu, sigma, palindromic, error_rate, alphabet, first=first))


def _lengths(seed, first, n, mu, sigma):
    return ns.noise_lengths_spec(ns.noise_draws_spec(seed, np.arange(first, first + n, dtype=np.uint64), ns.NORMAL, mu, sigma))


# random mode: pinned (seed, first) found by searching the draws of normal(2, 3)
BLOCK_EDGE = dict(seed=5, first=0, n=1000)                                # lengths 0, 1, 3, 4, 5, 7, 8, 9 all occur
LIMIT = dict(seed=18, first=0, n=5)                                       # normal(2^20 + 1, 0.5): 2^20 or 2^20 + 1 per molecule
ALPHABETS = ("N", "ACG", "AAAGTC")


# ------------------------------------------------------------------------------------------------ tail-noise: CPU
def test_pinned_normal_draws_the_same_length_for_every_molecule():
    for n_mols in {len(_hairpin_corpus(False)), len(_hairpin_corpus(True))}:
        for L in HAIRPIN_L + (2**20,):
            mu, sigma = _same_length(L)
            d = ns.noise_draws_spec(PAL_SEED, np.arange(PAL_FIRST, PAL_FIRST + n_mols, dtype=np.uint64), ns.NORMAL, mu, sigma)
            assert (np.abs(d - mu) <= 1e-8).all() and (ns.noise_lengths_spec(d) == L).all(), L
    for first in (0, 2**32 - 2):
        assert (_lengths(23, first, 8, *_same_length(2**20)) == 2**20).all()


def test_hairpin_corpus_is_what_it_is_meant_to_be():
    plain, subs, inside = _hairpin_corpus(False), _hairpin_corpus(True), _hairpin_corpus(True, False)
    assert len(plain) == 2 * 81 + 2 and len(subs) == len(inside) == len(plain) + 4 and len({m["id"] for m in subs}) == len(subs)
    for corpus in (plain, subs, inside):
        assert mo.stream_mdf(mo.write_mdf(corpus), unroll=True) == corpus                          # the text the device parses says the same
    tails = {(mo.seg_size(m["segments"][1]), mo.seg_size(m["segments"][2])) for m in plain if len(m["segments"]) == 3}
    assert tails >= {(b, c) for b in SIZES for c in SIZES}
    for j in (1, 2):                                                    # b and c: every size on both strands, as a contig and as a literal segment
        seen = {(mo.seg_size(m["segments"][j]), m["segments"][j]["plus"], m["segments"][j]["chr"].startswith("chr")) for m in plain if len(m["segments"]) == 3}
        assert {(size, plus) for size, plus, _ in seen} == {(size, plus) for size in SIZES for plus in (False, True)}
        assert {(size, contig) for size, _, contig in seen} == {(size, contig) for size in SIZES for contig in (False, True)}
    errs = [(mo.seg_size(s), [p for p, _ in s["errors"]]) for m in subs for s in m["segments"]]
    assert all(p != sorted(p) and len(set(p)) < len(p) for _, p in errs if len(p) > 2)                # unsorted, one position twice
    for size, p in errs:
        if size and len(p) < 20:
            assert {0, 63, 64, size - 1, size, size + 1, _roundup64(size) - 1, _roundup64(size), size + 1000} == set(p), size
    assert sorted({len(p) for _, p in errs if len(p) > 20}) == [70, 140]
    assert all(p < mo.seg_size(s) for m in inside for s in m["segments"] for p, _ in s["errors"])
    assert sorted({len(s["errors"]) for m in inside for s in m["segments"] if len(s["errors"]) > 20}) == [70, 140]


@pytest.mark.parametrize("subs", [False, True], ids=["plain", "substitutions"])
def test_hairpin_sweep_reaches_every_class(subs):
    per_l, n = _hairpin_reach(subs)
    for L in HAIRPIN_L:
        print(f"L = {L}: " + ", ".join(f"{c}: {k}" for c, k in per_l[L].items()))
    print("\n".join(f"{c}: {k}" for c, k in n.items()))
    for L in HAIRPIN_L[:-1]:
        for c in CLASSES:
            assert per_l[L][c] > 0, (L, c)
    assert per_l[10**6]["uncut, L above the molecule"] == len(_hairpin_corpus(subs)) and n["cut offsets on the stride"] > 0 and n["empty segments copied"] > 0
    if subs:
        for c, k in n.items():
            assert k > 0, c
    # the specification's text shows the same: an uncut whole-molecule hairpin doubles the segment lines, a cut one does not
    text = _hairpin_want(subs, 10**6, 0.0)
    assert text.count("\n") == len(_hairpin_corpus(subs)) + 2 * sum(len(m["segments"]) for m in _hairpin_corpus(subs))


def test_small_corpus_and_batches():
    mols = _small_corpus()
    assert len(mols) == max(BATCH_SIZES) and sum(not m["segments"] for m in mols) >= 15 and not mols[3]["segments"] and mols[0]["segments"]
    assert any(not s["chr"].startswith("chr") for m in mols for s in m["segments"]) and any(not s["plus"] for m in mols for s in m["segments"])
    assert mo.stream_mdf(mo.write_mdf(mols), unroll=True) == mols
    for name, kw in SMALL_MODES.items():
        for first in (7, 2**32 - 2):
            lens = _lengths(11, first, 5, kw["mu"], kw["sigma"])
            assert (lens[:2] > 0).any() and (lens[2:] > 0).any(), (name, first)      # molecules on both sides of index 2^32 get noise
        # the molecules from 2^32 on do not come out as those at index & 0xffffffff would
        assert _noise_want(mols[2:5], 11, 2**32, **kw) != _noise_want(mols[2:5], 11, 0, **kw)


def _find_first(n, ok, seed=5, span=400_000):
    lens = _lengths(seed, 0, span + n, 2.0, 3.0)
    for f in range(span):
        if ok(lens[f:f + n]):
            return f
    raise AssertionError("no such run of draws")


def _zero_runs_ok(w):
    z = w <= 0
    return z[:3].all() and z[-3:].all() and not z[3] and not z[-4] and any(z[i] and z[i + 1] and not z[i - 1] and not z[i + 2] for i in range(5, len(w) - 6))


def _alternate_ok(w):
    return ((w <= 0) == (np.arange(len(w)) % 2 == 0)).all()


RANDOM_FIRSTS = {"zero runs": 735, "alternate": 1732}                # _find_first(16, _zero_runs_ok), _find_first(10, _alternate_ok)


def test_random_mode_draws_reach_the_block_edges_and_the_empty_runs():
    lens = _lengths(BLOCK_EDGE["seed"], BLOCK_EDGE["first"], BLOCK_EDGE["n"], 2.0, 3.0)
    counts = {L: int((np.maximum(lens, 0) == L).sum()) for L in (0, 1, 3, 4, 5, 7, 8, 9)}
    print(f"normal(2, 3), 1000 molecules: {counts}; non-positive draws: {int((lens <= 0).sum())}")
    assert all(k > 0 for k in counts.values())
    assert _zero_runs_ok(_lengths(5, RANDOM_FIRSTS["zero runs"], 16, 2.0, 3.0)) and _alternate_ok(_lengths(5, RANDOM_FIRSTS["alternate"], 10, 2.0, 3.0))
    lim = _lengths(LIMIT["seed"], LIMIT["first"], LIMIT["n"], 2.0**20 + 1.0, 0.5)
    print(f"normal(2^20 + 1, 0.5): {lim - 2**20}")
    assert set(lim.tolist()) == {2**20, 2**20 + 1} and lim[0] == 2**20 and lim[1] == 2**20 and lim[2] == 2**20 + 1
    with pytest.raises(ns.NoiseLimit) as e:
        ns.noise_spec(_small_corpus()[:5], LIMIT["seed"], ns.NORMAL, 2.0**20 + 1.0, 0.5, first=LIMIT["first"])
    assert e.value.index == 2


# ================================================================================================ GPU
def _first_difference(got, want):
    g, w = got.splitlines(), want.splitlines()
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return f"line {i}: got {a[:300]!r}, want {b[:300]!r}"
    return f"{len(g)} lines against {len(w)}"


def _text_of(s, out):
    try:
        return s.to_mdf_text(out)
    finally:
        out.free()


def _declared(table):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    for name, n in table:
        s.declare_contig(name, n)
    return s


# ------------------------------------------------------------------------------------------------ GPU: random-wgs
@pytest.fixture(scope="module")
def wgs_contexts():
    """one context per contig table, made with declare_contig only"""
    made = {}

    def get(n, pattern):
        if (n, pattern) not in made:
            made[(n, pattern)] = _declared(_table(n, pattern))
        return made[(n, pattern)]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", WGS_CASES, ids=WGS_IDS)
def test_wgs_contig_tables_around_the_lds_limit(wgs_contexts, case):
    """1, 2047, 2048, 2049, 5000 contigs (the search in LDS up to 2048 entries, in global memory above), zero-length contigs (ties in the
    running sums), a reference above 2^32 bases; both stop modes: text and carried state against the specification"""
    n, pat, dist, a, b, stop, seed = case
    s = wgs_contexts(n, pat)
    assert s.reference_info()["total_bases"] == sum(l for _, l in _table(n, pat))
    want, st_want = _wgs_want(case)
    batch, st = s.wgs(dist, a, b, seed=seed, n_candidates=N_CAND, **{stop[0]: stop[1]})
    got = _text_of(s, batch)
    assert st == st_want
    assert got == want, _first_difference(got, want)


@pytest.mark.gpu
def test_wgs_table_of_zero_length_contigs_only_is_refused():
    from tksm_amd.sequence import TksmSeqError
    s = _declared((("c0", 0), ("c1", 0)))
    try:
        with pytest.raises(TksmSeqError) as e:
            s.wgs(ws.UNIFORM, 1.0, 4000.0, base_count=100)
        assert e.value.code == ESTATE
    finally:
        s.close()


@pytest.mark.gpu
def test_wgs_table_grows_across_the_lds_limit_between_calls(wgs_contexts):
    """the device copy of the table is cached by the version of the reference: a context that ran at 2048 contigs (LDS search) and is
    then given one more must search the new table (in global memory) -- the same as a fresh context with 2049"""
    table = _table(2049, "uniform")
    case49 = WGS_CASES[3]
    assert case49[:2] == (2049, "uniform") and case49[5][0] == "base_count"
    s = _declared(table[:2048])
    try:
        _, _, dist, a, b, stop, seed = case49
        want48 = ws.wgs_spec(seed, table[:2048], dist, a, b, base_count=stop[1], n_candidates=N_CAND)
        batch, st = s.wgs(dist, a, b, seed=seed, n_candidates=N_CAND, base_count=stop[1])
        assert (_text_of(s, batch), st) == want48
        s.declare_contig(*table[2048])
        batch, st = s.wgs(dist, a, b, seed=seed, n_candidates=N_CAND, base_count=stop[1])
        got = _text_of(s, batch)
        want, st_want = _wgs_want(case49)
        assert want != want48[0] and f"_{table[2048][0]}:" in want        # the new contig is hit
        assert st == st_want and got == want, _first_difference(got, want)
        fresh = wgs_contexts(2049, "uniform")
        batch, st2 = fresh.wgs(dist, a, b, seed=seed, n_candidates=N_CAND, base_count=stop[1])
        assert _text_of(fresh, batch) == got and st2 == st
    finally:
        s.close()


@pytest.mark.gpu
def test_wgs_stop_rule_met_exactly(wgs_contexts):
    """base_count = 1, S', S' + 1, S, S + 1 for the running sums S' / S before / after an emitted candidate; carried states one base
    below base_count, at it and above it (an empty batch, no candidate taken)"""
    n, pat, dist, a, b, seed = STOP_CASE
    s = wgs_contexts(n, pat)
    for name, base_count, first, state in _stop_runs():
        want, st_want = _stop_want(base_count, first, state)
        batch, st = s.wgs(dist, a, b, seed=seed, base_count=base_count, first_candidate=first, n_candidates=N_CAND, state=state)
        assert batch.n_reads == st_want["molecules"] - state[0], name
        got = _text_of(s, batch)
        assert st == st_want, (name, st, st_want)
        assert got == want, (name, _first_difference(got, want))


# ------------------------------------------------------------------------------------------------ GPU: tail-noise
@pytest.fixture(scope="module")
def gs():
    from tksm_amd.sequence import Sequencer
    rs = np.random.RandomState(21)
    ref = {f"chr{i + 1}": rs.choice(np.frombuffer(b"ACGT", np.uint8), 60_000).tobytes().decode() for i in range(2)}
    s = Sequencer(0)
    for k, v in ref.items():
        s.add_contig(k, v)
    yield s
    s.close()


def _unchecked_batch(s, text):
    """tksmseq_molecules_from_mdf_text, the parser of the `tksm tail-noise` module: it does not compare substitution positions with their
    segments (batch_from_mdf and batch_from_arrays refuse positions beyond the segment)"""
    from tksm_amd.sequence import Batch
    raw = text.encode()
    h = C.c_void_p()
    s._chk(s._lib.tksmseq_molecules_from_mdf_text(s._ctx, raw, len(raw), C.byref(h)))
    return Batch(s, h)


@pytest.fixture(scope="module")
def hairpin_batches(gs):
    made = {subs: _unchecked_batch(gs, mo.write_mdf(_hairpin_corpus(subs))) for subs in (False, True)}
    yield made
    for b in made.values():
        b.free()


@pytest.mark.gpu
def test_only_the_module_parser_takes_positions_beyond_the_segment(gs):
    from tksm_amd.sequence import TksmSeqError
    text = "+m\t1\t\nchr1\t10\t20\t+\t10A\n"
    with pytest.raises(TksmSeqError) as e:
        gs.batch_from_mdf(text)
    assert e.value.code == EINVAL and "outside its interval" in str(e.value)
    with pytest.raises(TksmSeqError) as e:
        gs.batch_from_arrays([[0, 1]], [[0, 10, 20, 0]], mods=[[10, ord("A")]])
    assert e.value.code == EINVAL and "outside its interval" in str(e.value)
    b = _unchecked_batch(gs, text)
    assert _text_of(gs, b) == text


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("subs", [False, True], ids=["plain", "substitutions"])
def test_hairpin_sweep_matches_the_specification(gs, hairpin_batches, subs, rate):
    """segment sizes and hairpin lengths on the 64-lane stride: L below, on and above every partial sum, copies cut on either strand, cut
    to nothing, zero-size segments; with substitutions on the window edges, beyond their segment, 70 and 140 in one segment"""
    b = hairpin_batches[subs]
    for L in HAIRPIN_L:
        mu, sigma = _same_length(L)
        got = _text_of(gs, gs.append_noise(b, ns.NORMAL, mu, sigma, palindromic=True, error_rate=rate, alphabet="AGTC", seed=PAL_SEED, first=PAL_FIRST))
        want = _hairpin_want(subs, L, rate)
        assert got == want, (L, _first_difference(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("L1,rate1", [(10**6, 1.0), (129, 0.5), (257, 0.0)])
def test_hairpin_of_the_sweep_s_hairpins(gs, hairpin_batches, L1, rate1):
    """second pass, other seed: the first pass's output (its own new substitutions merged with copied ones, some beyond their segment)
    as the input; pinned lengths again and drawn ones"""
    mols = _hairpin_corpus(True)
    m1 = ns.noise_spec(mols, PAL_SEED, ns.NORMAL, *_same_length(L1), True, rate1, "AGTC", first=PAL_FIRST)
    b1 = gs.append_noise(hairpin_batches[True], ns.NORMAL, *_same_length(L1), palindromic=True, error_rate=rate1, seed=PAL_SEED, first=PAL_FIRST)
    try:
        for mu, sigma in (_same_length(193), _same_length(10**6), (300.0, 250.0)):
            got = _text_of(gs, gs.append_noise(b1, ns.NORMAL, mu, sigma, palindromic=True, error_rate=0.3, seed=4, first=2**32 - 100))
            want = mo.write_mdf(ns.noise_spec(m1, 4, ns.NORMAL, mu, sigma, True, 0.3, "AGTC", first=2**32 - 100))
            assert got == want, (mu, _first_difference(got, want))
    finally:
        b1.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(SMALL_MODES))
def test_small_batches_and_molecules_without_segments(gs, mode):
    """1, 3, 4, 5, 127, 128, 129 molecules (four waves a block: the spare waves of the last block return early), every seventh molecule
    without any segment; first = 7 and first = 2^32 - 2"""
    kw = SMALL_MODES[mode]
    mols = _small_corpus()
    for n in BATCH_SIZES:
        b = gs.batch_from_mdf(mo.write_mdf(mols[:n]))
        for first in (7, 2**32 - 2):
            out = gs.append_noise(b, kw["dist"], kw["mu"], kw["sigma"], palindromic=kw["palindromic"], error_rate=kw["error_rate"], alphabet=kw["alphabet"], seed=11, first=first)
            assert out.n_reads == n
            got, want = _text_of(gs, out), _noise_want(mols[:n], 11, first, **kw)
            assert got == want, (n, first, _first_difference(got, want))
        b.free()
    # molecules without segments only
    none = [m for m in mols if not m["segments"]][:5]
    b = gs.batch_from_mdf(mo.write_mdf(none))
    got, want = _text_of(gs, gs.append_noise(b, kw["dist"], kw["mu"], kw["sigma"], palindromic=kw["palindromic"], seed=11, first=7)), _noise_want(none, 11, 7, **kw)
    b.free()
    assert got == want and (got.count("\n") == 5) == kw["palindromic"]


@pytest.mark.gpu
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_literal_lengths_around_the_philox_block_and_runs_of_empty_literals(gs, alphabet):
    """normal(2, 3): literal lengths 0 .. 12 (a Philox block holds 4 letters); runs of molecules with L <= 0 at the start, in the middle
    and at the end of a batch, and L <= 0 alternating with L > 0 -- ties in the scan of the block counts the owner search goes through"""
    mols = _small_corpus()
    rounds = [(mols * 8)[:BLOCK_EDGE["n"]], BLOCK_EDGE["seed"], BLOCK_EDGE["first"]], [mols[:16], 5, RANDOM_FIRSTS["zero runs"]], [mols[:10], 5, RANDOM_FIRSTS["alternate"]]
    for batch_mols, seed, first in rounds:
        batch_mols = [dict(m, id=f"{m['id']}_{i}") for i, m in enumerate(batch_mols)]
        b = gs.batch_from_mdf(mo.write_mdf(batch_mols))
        got = _text_of(gs, gs.append_noise(b, ns.NORMAL, 2.0, 3.0, alphabet=alphabet, seed=seed, first=first))
        b.free()
        want = _noise_want(batch_mols, seed, first, ns.NORMAL, 2.0, 3.0, False, 0.5, alphabet)
        assert got == want, (len(batch_mols), first, _first_difference(got, want))


@pytest.mark.gpu
def test_literal_of_exactly_the_longest_length_and_one_letter_more(gs):
    """L = 2^20 on a one-molecule batch succeeds, letter for letter; 2^20 + 1 is refused with the id of the first molecule that drew it,
    which is not the batch's first"""
    from tksm_amd.sequence import TksmSeqError
    mols = _small_corpus()[:5]
    n = 2**20
    for first in (23, 2**32 - 1):
        b = gs.batch_from_mdf(mo.write_mdf(mols[:1]))
        got = _text_of(gs, gs.append_noise(b, ns.NORMAL, *_same_length(n), alphabet="AAAGTC", seed=23, first=first))
        b.free()
        letters = ns.letters_spec(23, first, n, "AAAGTC")
        line = got.splitlines()[-1].split("\t")
        assert len(line[0]) == n and line[1:] == ["0", str(n), "+", ""] and line[0] == letters
        assert got == mo.write_mdf(mols[:1]) + f"{letters}\t0\t{n}\t+\t\n"
    b = gs.batch_from_mdf(mo.write_mdf(mols))
    with pytest.raises(ns.NoiseLimit) as spec:
        ns.noise_spec(mols, LIMIT["seed"], ns.NORMAL, 2.0**20 + 1.0, 0.5, first=LIMIT["first"])
    with pytest.raises(TksmSeqError, match=f"molecule {mols[spec.value.index]['id']} ") as e:
        gs.append_noise(b, ns.NORMAL, 2.0**20 + 1.0, 0.5, seed=LIMIT["seed"], first=LIMIT["first"])
    assert e.value.code == ELIMIT and spec.value.index == 2 and "above 1048576" in str(e.value)
    # the context and the batch still work
    got = _text_of(gs, gs.append_noise(b, ns.NORMAL, 2.0, 3.0, seed=5))
    b.free()
    assert got == _noise_want(mols, 5, 0, ns.NORMAL, 2.0, 3.0, False, 0.5, "AGTC")


def _reads(s, b):
    return [r.split(b"\n")[1].decode() for r in s.run(b, target="perfect", fastq=True, seed=1).records()]


def _revcomp(x):
    return x[::-1].translate(str.maketrans("ACGT", "TGCA"))


@pytest.mark.gpu
@pytest.mark.parametrize("subs", [False, True], ids=["plain", "substitutions"])
def test_perfect_reads_of_the_crafted_hairpins(gs, subs):
    """Not through the specification: with error rate 0 and L above every molecule, the perfect read of an output molecule is the
    input's read followed by its reverse complement.  With L = 129 and 193 it is followed by the reverse complements of the reads of
    its last segments, last one first, while they fit; of the one that does not fit whole, the END of its reverse complement is kept
    (the reference shortens the copy where the original ends: src/append_noise.cpp:100-105).  The substitutions lie inside their
    segments here (k_simulate refuses others)."""
    mols = _hairpin_corpus(subs, False)
    b = gs.batch_from_mdf(mo.write_mdf(mols))
    before = _reads(gs, b)
    assert [len(x) for x in before] == [mo.mol_size(m) for m in mols]
    for L in (10**6, 129, 193):
        out = gs.append_noise(b, ns.NORMAL, *_same_length(L), palindromic=True, error_rate=0.0)
        after = _reads(gs, out)
        out.free()
        assert len(after) == len(before)
        for md, x, y in zip(mols, before, after):
            want, end, left = x, len(x), L
            for size in [mo.seg_size(s) for s in reversed(md["segments"])]:
                piece = _revcomp(x[end - size:end])
                want += piece if size <= left else piece[size - left:]
                end, left = end - size, left - size
                if left < 0:
                    break
            assert y == want and len(y) == len(x) + min(L, len(x)), (L, md["id"])
            if L > len(x):
                assert y == x + _revcomp(x), (L, md["id"])
    b.free()
    assert sum(x != _revcomp(x) for x in before) > 150
