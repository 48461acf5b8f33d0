"""The rules of `tksm map --split` (include/tksmseq.h, "map, split reads") in plain Python, written from that text and not from the kernels:
the rounds of a group over its shrinking anchors, step A (the primary and its secondaries from the round-1 chains, as map_spec chooses them),
step B (the supplementary lines), their mapq and the sn / si tags, with and without alignment and end extension.  The sketch, the index and
chain() come from tests/map_spec.py, the alignment of a chain from tests/map_align_spec.py and the extension of an end from
tests/map_extend_spec.py; this file imports them and edits none.  With split=False it states the same run without the feature, so that
tests/test_map_split.py can hold it against those three files.  tests/test_map_split_gpu.py compares the device with it byte for byte."""
import os
import random

import map_align_spec as A
import map_extend_spec as X
import map_spec as M

DEFAULTS = dict(split_chains=4, split_overlap=30, split_segments=8)
COUNTERS = ("split_reads", "supplementary", "later_chains", "rounds", "rejected_overlap")


def check_params(chains, overlap, segments):
    if not 1 <= chains <= 16 or not 0 <= overlap < 1 << 31 or not 2 <= segments <= 64:
        raise ValueError("map: a parameter out of range")


def rounds_of(anchors, p, chains, window=M.PRED_WINDOW):
    """anchors: a group's [(p, qa)] by (p, qa), at least min_count of them.  ([the kept chains of its rounds, each with "round" and
    "anchors" = its own (p, qa)], the rounds run)"""
    k, remaining, kept, run = p["k"], list(anchors), [], 0
    while run < chains and len(remaining) >= p["min_count"]:
        c = M.chain(remaining, k, p["max_gap"], p["bandwidth"], window)
        c["round"], c["anchors"] = run, [remaining[i] for i in c["path"]]
        run += 1
        if c["cnt"] < p["min_count"] or c["score"] < p["min_score"]:
            break
        kept.append(c)
        remaining = [a for a in remaining if not (a[1] < c["qe"] and a[1] + k > c["qs"])]
    return kept, run


def map_read(seq, index, p, chains, window=M.PRED_WINDOW):
    """what one read's letters give: (read minimizers, anchors, groups, chained groups, rounds run, [kept chains of all rounds by (score
    descending, target, rel, round)])"""
    groups = A.groups_of(seq, index, p)
    n_min = len(M.minimizers(seq, p["k"], p["w"]))
    kept, chained, rounds = [], 0, 0
    for (t, rel), anchors in groups.items():
        if len(anchors) < p["min_count"]:
            continue
        chained += 1
        got, run = rounds_of(anchors, p, chains, window)
        rounds += run
        for c in got:
            c["t"], c["rel"] = t, rel
            kept.append(c)
    kept.sort(key=lambda c: (-c["score"], c["t"], c["rel"], c["round"]))
    return n_min, sum(len(a) for a in groups.values()), len(groups), chained, rounds, kept


def interval(c, qlen):
    """[qstart, qend) of a chain's own corners in the read as it was sequenced"""
    return (c["qs"], c["qe"]) if c["rel"] == 0 else (qlen - c["qe"], qlen - c["qs"])


def shared(a, b):
    return max(0, min(a[1], b[1]) - max(a[0], b[0]))


def select(kept, qlen, p, split, overlap, segments):
    """the lines of a read from its kept chains in sorted order: ([(chain, mapq, kind)], candidates rejected); kind is "primary",
    "secondary" or "supplementary" """
    first = [c for c in kept if c["round"] == 0]
    if not first:
        return [], 0
    P = M.permille(p["secondary_ratio"])
    s1 = first[0]["score"]
    s2 = first[1]["score"] if len(first) > 1 else 0
    out = [(first[0], min(60, 60 * (s1 - s2) // s1), "primary")]
    for c in first[1:]:
        if len(out) > p["max_secondary"] or c["score"] * 1000 < P * s1:
            break
        out.append((c, 0, "secondary"))
    if not split:
        return out, 0
    written = [c for c, _, _ in out]
    accepted, rejected = [], 0
    for c in kept:
        if any(c is w for w in written):
            continue
        if len(accepted) == segments - 1:
            break
        iv = interval(c, qlen)
        if all(shared(iv, interval(x, qlen)) <= overlap for x in [first[0]] + accepted):
            accepted.append(c)
        else:
            rejected += 1
    for c in accepted:
        iv, s = interval(c, qlen), c["score"]
        others = [x["score"] for x in kept if x is not first[0] and not any(x is y for y in accepted) and shared(iv, interval(x, qlen)) > overlap]
        s2 = max(others, default=0)
        out.append((c, 0 if s2 >= s else min(60, 60 * (s - s2) // s), "supplementary"))
    return out, rejected


def generate(d, seed, n_targets=40, n_reads=300, lengths=(600, 2500), min_piece=200, error=0.0, tag="split", shapes=("A", "AB", "AA", "Aa", "ABA")):
    """targets as map_spec.generate makes them; a read is one of `shapes` in turn: a letter is a piece (a random substring of a random
    target on a random strand), the same letter the same piece, a lower-case letter its reverse complement.  `error`: substitutions per
    base, applied to the glued read.  truth[name] = [(target name, strand, start, end)] of its pieces in read order"""
    rs = random.Random(seed)
    targets = [("t%03d" % i, M.random_seq(rs, rs.randint(*lengths))) for i in range(n_targets)]
    reads, truth = [], {}
    for r in range(n_reads):
        shape, pieces = shapes[r % len(shapes)], {}
        for letter in sorted(set(shape.upper())):
            t = rs.randrange(n_targets)
            name, seq = targets[t]
            n = rs.randint(min(min_piece, len(seq)), len(seq))
            a = rs.randint(0, len(seq) - n)
            strand = rs.randrange(2)
            pieces[letter] = (name, strand, a, a + n, M.revcomp(seq[a:a + n]) if strand else seq[a:a + n])
        letters, parts = [], []
        for ch in shape:
            name, strand, a, b, text = pieces[ch.upper()]
            flipped = ch.islower()
            letters.append(M.revcomp(text) if flipped else text)
            parts.append((name, strand ^ flipped, a, b))
        text = "".join(letters)
        if error:
            text = "".join(rs.choice([x for x in "ACGT" if x != c]) if rs.random() < error else c for c in text)
        reads.append(("s%04d" % r, text))
        truth["s%04d" % r] = parts
    return {"ref": M.write_fasta(os.path.join(str(d), tag + ".ref.fa"), targets), "reads": M.write_fastq(os.path.join(str(d), tag + ".reads.fq"), reads),
            "targets": targets, "read_list": reads, "truth": truth}


def map_reads(targets, reads, split=True, split_chains=4, split_overlap=30, split_segments=8, align=False, band=63, eqx=False, extend=False, ext_band=31, ext_drop=40,
              ext_max=2000, pred_window=M.PRED_WINDOW, memo=None, **params):
    """targets, reads: [(name, letters)].  {"paf", "info": map_spec's counters, "split": COUNTERS (with split), "align" (with align) and
    "extend" (with extend): the counters of those specs, "lines": per read name its [(target name, rel, kind, chain)], "estimate": what the
    module logs as the unsegment -p estimate}.  memo: a dict the caller keeps between calls with the same targets and parameters"""
    p = dict(M.DEFAULTS, **params)
    M.check_params(p)
    if split:
        check_params(split_chains, split_overlap, split_segments)
    if align and (not 1 <= band <= 63 or p["max_gap"] > A.MAX_GAP):
        raise ValueError("map: a parameter out of range")
    if extend:
        X.check_params(ext_band, ext_drop, ext_max)
    chains = split_chains if split else 1
    k = p["k"]
    memo = {} if memo is None else memo
    if "index" not in memo:
        memo["index"] = M.build_index([s for _, s in targets], k, p["w"])
    index, n_entries = memo["index"]
    info = dict.fromkeys(M.COUNTERS, 0)
    info.update(reads=len(reads), target_minimizers=n_entries, distinct_hashes=len(index), dropped_hashes=sum(len(v) > p["max_occ"] for v in index.values()))
    sinfo, ainfo, xinfo = dict.fromkeys(COUNTERS, 0), dict.fromkeys(A.COUNTERS, 0), dict.fromkeys(X.COUNTERS, 0)
    paf, lines = [], {}
    for name, seq in reads:
        seq = seq.upper()
        qlen = len(seq)
        key = (seq, chains, pred_window)
        if key not in memo:
            memo[key] = map_read(seq, index, p, chains, pred_window)
        n_min, n_anchors, n_groups, chained, rounds, kept = memo[key]
        info["read_minimizers"] += n_min
        info["anchors"] += n_anchors
        info["groups"] += n_groups
        info["chained_groups"] += chained
        sinfo["rounds"] += rounds
        sinfo["later_chains"] += sum(c["round"] > 0 for c in kept)
        out, rejected = select(kept, qlen, p, split, split_overlap, split_segments)
        sinfo["rejected_overlap"] += rejected
        if not out:
            info["unmapped"] += 1
            continue
        info["mapped"] += 1
        tagged = [i for i, (_, _, kind) in enumerate(out) if kind != "secondary"]
        by_interval = sorted(tagged, key=lambda i: (interval(out[i][0], qlen), i))
        sn = len(tagged)
        sinfo["split_reads"] += sn > 1
        sinfo["supplementary"] += sn - 1
        lines[name] = []
        for i, (c, mapq, kind) in enumerate(out):
            tname, tseq = targets[c["t"]]
            tseq = tseq.upper()
            tstart, tend, qs, qe, nmatch = c["tstart"], c["tend"], c["qs"], c["qe"], c["nmatch"]
            left = right = None
            if extend:
                left, right = X.ends_of(tseq, seq if c["rel"] == 0 else M.revcomp(seq), c, ext_band, ext_drop, ext_max)
                tstart, tend, qs, qe = tstart - left["ei"], tend + right["ei"], qs - left["ej"], qe + right["ej"]
                nmatch += left["m"] + right["m"]
                xinfo["lines"] += 1
                for e in (left, right):
                    xinfo["ends_moved"] += e["ei"] + e["ej"] > 0
                    xinfo["target_gained"] += e["ei"]
                    xinfo["read_gained"] += e["ej"]
                    xinfo["matches"] += e["m"]
                    xinfo["antidiagonals"] += e["steps"]
                    xinfo["cells"] += e["cells"]
                    xinfo["longest"] = max(xinfo["longest"], e["ei"] + e["ej"])
            blen = max(tend - tstart, qe - qs)
            tail = []
            if align:
                akey = ("columns", seq, c["t"], c["rel"], c["round"], band)
                if akey not in memo:
                    memo[akey] = A.align_chain(tseq, seq, c["rel"], c["anchors"], k, band)
                columns, nm, spans, cells = memo[akey]
                n = {op: columns.count(op) for op in "=XID"}
                ainfo["lines"] += 1
                ainfo["segments"] += len(spans)
                ainfo["longest_segment"] = max(ainfo["longest_segment"], max(spans))
                ainfo["cells"] += cells
                ainfo["columns"] += len(columns)
                ainfo["matches"] += n["="]
                ainfo["mismatches"] += n["X"]
                ainfo["inserted"] += n["I"]
                ainfo["deleted"] += n["D"]
                if extend:
                    columns = left["columns"][::-1] + columns + right["columns"]
                    n = {op: columns.count(op) for op in "=XID"}
                nmatch, blen = n["="], len(columns)
                tail = ["NM:i:%d" % (n["X"] + n["I"] + n["D"]), "cg:Z:" + A.cigar(columns, eqx)]
            qstart, qend = (qs, qe) if c["rel"] == 0 else (qlen - qe, qlen - qs)
            tags = ["tp:A:" + ("S" if kind == "secondary" else "P"), "cm:i:%d" % c["cnt"], "s1:i:%d" % c["score"]]
            if sn > 1 and kind != "secondary":
                tags += ["sn:i:%d" % sn, "si:i:%d" % by_interval.index(i)]
            paf.append("\t".join(str(x) for x in [name, qlen, qstart, qend, "+-"[c["rel"]], tname, len(tseq), tstart, tend, nmatch, blen, mapq] + tags + tail) + "\n")
            lines[name].append((tname, c["rel"], kind, c))
            info["lines"] += 1
            info["secondary"] += kind == "secondary"
    J, Mp = sinfo["supplementary"], info["mapped"]
    result = {"paf": "".join(paf), "info": info, "lines": lines, "estimate": J / (Mp + J - 1) if Mp + J > 1 else 0.0}
    if split:
        result["split"] = sinfo
    if align:
        result["align"] = ainfo
    if extend:
        result["extend"] = xinfo
    return result


# ----------------------------------------------------------------------------- inputs that reach one case each
EDGE = dict(k=15, w=1, min_count=3, min_score=0, bandwidth=120)
# anchors of the pieces of one target in target order; the read holds the pieces in the opposite order, so that no two of them chain
# (dt > 0 needs dq > 0).  The group has sum(sizes) anchors in (p, qa) order, piece after piece, and the largest piece (the first of equal
# ones) is the chain of round 1: its positions of the list are what the compaction removes
TILE_SIZES = ((30, 33), (60, 3), (61, 2), (63,),
              (40, 24), (64,),
              (62, 3), (40, 25), (63, 2),
              (63, 33, 32), (64, 32, 32), (65, 32, 31), (31, 32, 65), (128,),
              (63, 33, 33), (64, 33, 32), (65, 32, 32), (32, 32, 65), (129,))
MANY_SIZES = (20, 22, 24, 26, 28, 30)                # six pieces of one target: more rounds than the default `chains`
VARIANTS = {"defaults": {}, "chains_1": dict(split_chains=1), "chains_2": dict(split_chains=2), "segments_2": dict(split_segments=2),
            "segments_3": dict(split_segments=3), "overlap_0": dict(split_overlap=0),
            "limits": dict(split_chains=16, split_overlap=(1 << 31) - 1, split_segments=64)}


def _other_than(rs, c):
    return rs.choice([x for x in "ACGT" if x != c])


def _both(name, read):
    return [(name + "f", read), (name + "r", M.revcomp(read))]


def _pieces(rs, sizes):
    """(target, read): pieces of n + 14 letters for n in sizes side by side in the target between two flanks, and in the opposite order in
    the read.  Drawn again until no piece goes on by a letter in both: the letter before (after) it in the read is not the one before
    (after) it in the target, so that piece i gives exactly sizes[i] anchors"""
    while True:
        left, right = M.random_seq(rs, 40), M.random_seq(rs, 40)
        pieces = [M.random_seq(rs, n + 14) for n in sizes]
        ok = True
        for i in range(len(pieces)):
            before_t, after_t = (pieces[i - 1][-1] if i else left[-1]), (pieces[i + 1][0] if i + 1 < len(pieces) else right[0])
            before_r, after_r = (pieces[i + 1][-1] if i + 1 < len(pieces) else None), (pieces[i - 1][0] if i else None)
            ok = ok and before_r != before_t and after_r != after_t
        if ok:
            return left + "".join(pieces) + right, "".join(reversed(pieces))


def edge_case():
    """(targets, reads, parameters) with w = 1, where every intact 15-mer is an anchor and a piece of n + 14 letters gives n anchors on
    one diagonal, scoring 15 + n - 1.  Read names say what they are for:
    tile_*: TILE_SIZES.  many: MANY_SIZES.
    span: a piece X of 86 anchors that lies, in the target, between the two halves Y1 and Y2 (46 anchors each) of a piece with a
        deletion of 100 letters; in the read X comes first and 200 letters of junk keep it from chaining with Y2.  Round 1 is X; Y2 cannot
        reach Y1 in round 1 (the 64 anchors before it are X's) and does in round 2: a link over 87 original anchors.
    ov30, ov31: U + V + W with U + V on one target and V + W on another, |V| = 30 and 31: read intervals that share exactly |V| letters.
    eq: P + junk + P on two identical targets that hold P and its reverse complement: equal scores over targets, strands and rounds.
    five: five whole targets of different lengths glued: more pieces than --split-segments 2 or 3 accept."""
    rs = random.Random(6464)
    targets, reads = [], []
    for sizes in TILE_SIZES:
        name = "tile_" + "_".join(str(n) for n in sizes)
        target, read = _pieces(rs, sizes)
        targets.append((name, target))
        reads += _both(name, read)
    target, read = _pieces(rs, MANY_SIZES)
    targets.append(("many", target))
    reads += _both("many", read)
    t = M.random_seq(rs, 420)
    targets.append(("span", t))
    reads += _both("span", t[160:260] + M.random_seq(rs, 200) + t[100:160] + t[260:320])
    for v in (30, 31):
        U, V, W = M.random_seq(rs, 100), M.random_seq(rs, v), M.random_seq(rs, 50)
        targets.append(("ov%d_uv" % v, M.random_seq(rs, 40) + U + V + _other_than(rs, W[0]) + M.random_seq(rs, 40)))
        targets.append(("ov%d_vw" % v, M.random_seq(rs, 40) + _other_than(rs, U[-1]) + V + W + M.random_seq(rs, 40)))
        reads += _both("ov%d" % v, U + V + W)
    while True:                                          # (drawn again until no copy of P goes on by a letter in the read and in the target)
        P, junk, F = M.random_seq(rs, 150), M.random_seq(rs, 130), [M.random_seq(rs, n) for n in (40, 60, 40)]
        if junk[0] != F[1][0] and junk[-1] != F[0][-1] and M.COMP[junk[-1]] != F[2][0] and M.COMP[junk[0]] != F[1][-1]:
            break
    t = F[0] + P + F[1] + M.revcomp(P) + F[2]
    targets += [("eq_a", t), ("eq_b", t)]
    reads += _both("eq", P + junk + P)
    five = [("five%d" % i, M.random_seq(rs, 100 + 13 * i)) for i in range(5)]
    targets += five
    reads += _both("five", "".join(seq for _, seq in five))
    return targets, reads, dict(EDGE)
