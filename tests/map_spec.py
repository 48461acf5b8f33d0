"""The rules of `tksm map` (include/tksmseq.h, "map") in plain Python, written from that text and not from the kernels: k-mers and their
hashes, window minimizers, the index with its occurrence filter, anchors, the chain of a (read, target, strand) group, the lines of a read.
Everything is integer.  tests/test_map.py pins this file against brute force and hand-worked cases; tests/test_map_gpu.py compares the
device with it byte for byte."""
import gzip
import math
import os
import random

MASK64 = (1 << 64) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
DEFAULTS = dict(k=15, w=10, max_occ=500, max_gap=5000, bandwidth=500, min_count=3, min_score=40, secondary_ratio=0.8, max_secondary=5)
COUNTERS = ("reads", "mapped", "unmapped", "lines", "secondary", "target_minimizers", "distinct_hashes", "dropped_hashes", "read_minimizers", "anchors",
            "groups", "chained_groups")
PRED_WINDOW = 64


def revcomp(s):
    return "".join(COMP.get(c, c) for c in reversed(s))


def mix(x):
    x ^= x >> 30
    x = x * 0xbf58476d1ce4e5b9 & MASK64
    x ^= x >> 27
    x = x * 0x94d049bb133111eb & MASK64
    x ^= x >> 31
    return x


def kmer(seq, p, k):
    """(h, strand) of the k-mer at p, or None when it is not valid"""
    word = seq[p:p + k]
    if len(word) != k or any(c not in CODE for c in word):
        return None
    fwd = rev = 0
    for c in word:
        fwd = fwd << 2 | CODE[c]
    for c in revcomp(word):
        rev = rev << 2 | CODE[c]
    if fwd == rev:
        return None
    return mix(min(fwd, rev)), 1 if rev < fwd else 0


def minimizers(seq, k, w):
    """[(h, p, strand)] by ascending p"""
    seq = seq.upper()
    n = len(seq) - k + 1
    if n <= 0:
        return []
    km = [kmer(seq, p, k) for p in range(n)]
    chosen = {}
    for j in range(max(0, n - w) + 1):
        best = None
        for p in range(j, min(j + w, n)):
            if km[p] is not None and (best is None or (km[p][0], p) < best):
                best = (km[p][0], p)
        if best is not None:
            chosen[best[1]] = km[best[1]]
    return [(chosen[p][0], p, chosen[p][1]) for p in sorted(chosen)]


def build_index(targets, k, w):
    """{h: [(target, p, strand)] by (target, p)} and the number of entries"""
    index, n = {}, 0
    for t, seq in enumerate(targets):
        for h, p, s in minimizers(seq, k, w):
            index.setdefault(h, []).append((t, p, s))
            n += 1
    return index, n


def cost(g, k):
    return 0 if g == 0 else g * k // 100 + (g.bit_length() - 1) // 2


def chain(anchors, k, max_gap=5000, bandwidth=500):
    """the chain of a group: anchors = [(p, qa)] by (p, qa)"""
    f, pred = [], []
    for i, (p, q) in enumerate(anchors):
        best, who = None, None
        for j in range(max(0, i - PRED_WINDOW), i):
            dt, dq = p - anchors[j][0], q - anchors[j][1]
            if dt <= 0 or dq <= 0 or dt > max_gap or dq > max_gap or abs(dt - dq) > bandwidth:
                continue
            sc = f[j] + min(k, dt, dq) - cost(abs(dt - dq), k)
            if best is None or sc >= best:
                best, who = sc, j
        if best is not None and best > k:
            f.append(best)
            pred.append(who)
        else:
            f.append(k)
            pred.append(None)
    end = max(range(len(f)), key=lambda i: (f[i], -i))
    path = [end]
    while pred[path[-1]] is not None:
        path.append(pred[path[-1]])
    path.reverse()
    nmatch = k
    for a, b in zip(path, path[1:]):
        nmatch += min(k, anchors[b][0] - anchors[a][0], anchors[b][1] - anchors[a][1])
    first, last = anchors[path[0]], anchors[path[-1]]
    out = dict(cnt=len(path), score=f[end], nmatch=nmatch, tstart=first[0], tend=last[0] + k, qs=first[1], qe=last[1] + k, path=path)
    out["blen"] = max(out["tend"] - out["tstart"], out["qe"] - out["qs"])
    return out


def permille(ratio):
    return int(math.floor(ratio * 1000.0 + 0.5))


def check_params(p):
    if not 4 <= p["k"] <= 28 or not 1 <= p["w"] <= 64 or p["max_occ"] < 1 or p["max_gap"] < 0 or p["bandwidth"] < 0 or p["min_count"] < 1 or p["min_score"] < 0 \
            or not 0.0 <= p["secondary_ratio"] <= 1.0 or not 0 <= p["max_secondary"] <= 1000:
        raise ValueError("map: a parameter out of range")


def map_read(seq, index, p):
    """what one read's letters give: (read minimizers, anchors, groups, chained groups, [kept chains in output order])"""
    k = p["k"]
    groups = {}
    mins = minimizers(seq, k, p["w"])
    n_anchors = 0
    for h, q, sr in mins:
        hits = index.get(h, ())
        if len(hits) > p["max_occ"]:
            continue
        for t, tp, st in hits:
            rel = sr ^ st
            groups.setdefault((t, rel), []).append((tp, q if rel == 0 else len(seq) - k - q))
            n_anchors += 1
    kept, chained = [], 0
    for (t, rel), anchors in groups.items():
        if len(anchors) < p["min_count"]:
            continue
        chained += 1
        c = chain(sorted(anchors), k, p["max_gap"], p["bandwidth"])
        if c["cnt"] >= p["min_count"] and c["score"] >= p["min_score"]:
            c["t"], c["rel"] = t, rel
            kept.append(c)
    kept.sort(key=lambda c: (-c["score"], c["t"], c["rel"]))
    return len(mins), n_anchors, len(groups), chained, kept


def map_reads(targets, reads, **params):
    """targets, reads: [(name, letters)].  {"paf": text, "info": counters, "lines": per read name its [(target name, rel, tp, chain)]}"""
    p = dict(DEFAULTS, **params)
    check_params(p)
    index, n_entries = build_index([s for _, s in targets], p["k"], p["w"])
    info = dict.fromkeys(COUNTERS, 0)
    info.update(reads=len(reads), target_minimizers=n_entries, distinct_hashes=len(index), dropped_hashes=sum(len(v) > p["max_occ"] for v in index.values()))
    P = permille(p["secondary_ratio"])
    paf, lines, memo = [], {}, {}
    for name, seq in reads:
        seq = seq.upper()
        if seq not in memo:                     # (a read's result depends on its letters alone)
            memo[seq] = map_read(seq, index, p)
        n_min, n_anchors, n_groups, chained, kept = memo[seq]
        info["read_minimizers"] += n_min
        info["anchors"] += n_anchors
        info["groups"] += n_groups
        info["chained_groups"] += chained
        if not kept:
            info["unmapped"] += 1
            continue
        info["mapped"] += 1
        s1 = kept[0]["score"]
        s2 = kept[1]["score"] if len(kept) > 1 else 0
        out = [(kept[0], min(60, 60 * (s1 - s2) // s1), "P")]
        for c in kept[1:]:
            if len(out) > p["max_secondary"] or c["score"] * 1000 < P * s1:
                break
            out.append((c, 0, "S"))
        lines[name] = []
        for c, mapq, tp in out:
            qlen = len(seq)
            qstart, qend = (c["qs"], c["qe"]) if c["rel"] == 0 else (qlen - c["qe"], qlen - c["qs"])
            tname, tseq = targets[c["t"]]
            paf.append("\t".join(str(x) for x in (name, qlen, qstart, qend, "+-"[c["rel"]], tname, len(tseq), c["tstart"], c["tend"], c["nmatch"], c["blen"], mapq,
                                                 "tp:A:" + tp, "cm:i:%d" % c["cnt"], "s1:i:%d" % c["score"])) + "\n")
            lines[name].append((tname, c["rel"], tp, c))
            info["lines"] += 1
            info["secondary"] += tp == "S"
    return {"paf": "".join(paf), "info": info, "lines": lines}


def _open(path):
    return gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)


def read_fasta(path):
    out = []
    with _open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                out.append([line[1:].split()[0], []])
            elif line:
                out[-1][1].append(line)
    return [(n, "".join(s)) for n, s in out]


def read_fastq(path):
    with _open(path) as f:
        rows = f.read().split("\n")
    return [(rows[i][1:].split()[0], rows[i + 1]) for i in range(0, len(rows) - 3, 4)]


def run(ref, reads, **params):
    """map_reads over files: `ref` and `reads` one path or a list of them"""
    refs = ref if isinstance(ref, (list, tuple)) else [ref]
    fqs = reads if isinstance(reads, (list, tuple)) else [reads]
    return map_reads([t for r in refs for t in read_fasta(r)], [q for r in fqs for q in read_fastq(r)], **params)


def write_fasta(path, targets, width=70):
    with (gzip.open(path, "wt") if str(path).endswith(".gz") else open(path, "w")) as f:
        for name, seq in targets:
            f.write(">%s\n" % name)
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width] + "\n")
            if not seq:
                f.write("\n")
    return str(path)


def write_fastq(path, reads):
    with (gzip.open(path, "wt") if str(path).endswith(".gz") else open(path, "w")) as f:
        for name, seq in reads:
            f.write("@%s\n%s\n+\n%s\n" % (name, seq, "I" * len(seq)))
    return str(path)


def random_seq(rs, n):
    return "".join(rs.choice("ACGT") for _ in range(n))


def mutate(rs, seq, rate):
    """substitutions, insertions and deletions, a third each, at `rate` per base"""
    out = []
    for c in seq:
        if rs.random() >= rate:
            out.append(c)
            continue
        kind = rs.randrange(3)
        if kind == 0:
            out.append(rs.choice([x for x in "ACGT" if x != c]))
        elif kind == 1:
            out.append(c + rs.choice("ACGT"))
    return "".join(out)


def generate(d, seed, n_targets=40, n_reads=300, lengths=(600, 2500), min_read=200, error=0.0, tag="gen"):
    """random targets, and reads that are random substrings of them on a random strand with `error` per base: ref.fa and reads.fq in `d`;
    truth[name] = (target name, strand, start, end)"""
    rs = random.Random(seed)
    targets = [("t%03d" % i, random_seq(rs, rs.randint(*lengths))) for i in range(n_targets)]
    reads, truth = [], {}
    for r in range(n_reads):
        t = rs.randrange(n_targets)
        name, seq = targets[t]
        n = rs.randint(min(min_read, len(seq)), len(seq))
        a = rs.randint(0, len(seq) - n)
        piece, strand = seq[a:a + n], rs.randrange(2)
        if strand:
            piece = revcomp(piece)
        if error:
            piece = mutate(rs, piece, error)
        reads.append(("r%04d" % r, piece))
        truth["r%04d" % r] = (name, strand, a, a + n)
    return {"ref": write_fasta(os.path.join(str(d), tag + ".ref.fa"), targets), "reads": write_fastq(os.path.join(str(d), tag + ".reads.fq"), reads),
            "targets": targets, "read_list": reads, "truth": truth}
