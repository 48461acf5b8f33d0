"""The rules of `tksm map` (include/tksmseq.h, "map") in plain Python, written from that text and not from the kernels: k-mers and their
hashes, window minimizers, the index with its occurrence filter, anchors, the chain of a (read, target, strand) group, the lines of a read.
Everything is integer.  tests/test_map.py pins this file against brute force and hand-worked cases; tests/test_map_gpu.py compares the
device with it byte for byte."""
import functools
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


def window_choices(seq, k, w):
    """(the valid k-mers by position, the position each window selects or None): window j holds the positions j .. j + w - 1"""
    seq = seq.upper()
    n = len(seq) - k + 1
    if n <= 0:
        return [], []
    km = [kmer(seq, p, k) for p in range(n)]
    choice = []
    for j in range(max(0, n - w) + 1):
        best = None
        for p in range(j, min(j + w, n)):
            if km[p] is not None and (best is None or (km[p][0], p) < best):
                best = (km[p][0], p)
        choice.append(None if best is None else best[1])
    return km, choice


def minimizers(seq, k, w):
    """[(h, p, strand)] by ascending p"""
    km, choice = window_choices(seq, k, w)
    return [(km[p][0], p, km[p][1]) for p in sorted({p for p in choice if p is not None})]


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


def chain(anchors, k, max_gap=5000, bandwidth=500, window=PRED_WINDOW):
    """the chain of a group: anchors = [(p, qa)] by (p, qa); `window` predecessors are looked at (None: all of them).  Beside the chain,
    what the one loop that decides it saw: f and pred of every anchor, ties[i] = the candidates of i that reach its best candidate score,
    ascending (the last one is the predecessor when the anchor links), best_is_k[i] = that score was exactly k (no link: the rule is > k)"""
    f, pred, ties, best_is_k = [], [], [], []
    for i, (p, q) in enumerate(anchors):
        best, tied = None, []
        for j in range(0 if window is None else max(0, i - window), i):
            dt, dq = p - anchors[j][0], q - anchors[j][1]
            if dt <= 0 or dq <= 0 or dt > max_gap or dq > max_gap or abs(dt - dq) > bandwidth:
                continue
            sc = f[j] + min(k, dt, dq) - cost(abs(dt - dq), k)
            if best is None or sc > best:
                best, tied = sc, [j]
            elif sc == best:
                tied.append(j)
        ties.append(tied)
        best_is_k.append(best == k)
        if best is not None and best > k:
            f.append(best)
            pred.append(tied[-1])
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
    out.update(f=f, pred=pred, ties=ties, best_is_k=best_is_k)
    return out


CLASSES = ("distance_64", "ties_same_tile", "ties_previous_tile", "ties_both_tiles", "best_is_k", "end_ties")


def classes_of_chain(c):
    """what a group asked of a device that keeps the last 64 anchors in the lanes of a wave and loads the anchors in tiles of 64 (anchor i
    is in tile i // 64), counted from what chain() returned.  distance_64: links to i - 64, the slot that anchor i itself takes over.
    ties_*: anchors i >= 64 that link and had two or more candidates of the best score, by where these lie: all in i's tile, all in the one
    before, some in each.  best_is_k: anchors whose best candidate scored exactly k.  end_ties: 1 when several anchors hold the largest f"""
    out = dict.fromkeys(CLASSES, 0)
    for i, (j, tied) in enumerate(zip(c["pred"], c["ties"])):
        out["distance_64"] += j is not None and i - j == 64
        out["best_is_k"] += c["best_is_k"][i]
        if j is not None and i >= 64 and len(tied) > 1:
            own = sum(t // 64 == i // 64 for t in tied)
            out["ties_same_tile" if own == len(tied) else "ties_both_tiles" if own else "ties_previous_tile"] += 1
    out["end_ties"] = int(c["f"].count(max(c["f"])) > 1)
    return out


def chain_classes(anchors, k, max_gap=5000, bandwidth=500):
    return classes_of_chain(chain(anchors, k, max_gap, bandwidth))


def classes_of_lines(out):
    """the sum of classes_of_chain over the chains that map_reads wrote: what a comparison of the PAF can see"""
    total = dict.fromkeys(CLASSES, 0)
    for lines in out["lines"].values():
        for _, _, _, c in lines:
            for what, n in classes_of_chain(c).items():
                total[what] += n
    return total


def permille(ratio):
    return int(math.floor(ratio * 1000.0 + 0.5))


def check_params(p):
    if not 4 <= p["k"] <= 28 or not 1 <= p["w"] <= 64 or p["max_occ"] < 1 or p["max_gap"] < 0 or p["bandwidth"] < 0 or p["min_count"] < 1 or p["min_score"] < 0 \
            or not 0.0 <= p["secondary_ratio"] <= 1.0 or not 0 <= p["max_secondary"] <= 1000:
        raise ValueError("map: a parameter out of range")


def map_read(seq, index, p, window=PRED_WINDOW):
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
        c = chain(sorted(anchors), k, p["max_gap"], p["bandwidth"], window)
        if c["cnt"] >= p["min_count"] and c["score"] >= p["min_score"]:
            c["t"], c["rel"] = t, rel
            kept.append(c)
    kept.sort(key=lambda c: (-c["score"], c["t"], c["rel"]))
    return len(mins), n_anchors, len(groups), chained, kept


def map_reads(targets, reads, pred_window=PRED_WINDOW, memo=None, **params):
    """targets, reads: [(name, letters)].  {"paf": text, "info": counters, "lines": per read name its [(target name, rel, tp, chain)]}.
    pred_window: the window of chain(), to show what another one would give.  memo: a dict that the caller keeps between calls with the
    same targets and parameters, so that a read's letters are worked on once"""
    p = dict(DEFAULTS, **params)
    check_params(p)
    index, n_entries = build_index([s for _, s in targets], p["k"], p["w"])
    info = dict.fromkeys(COUNTERS, 0)
    info.update(reads=len(reads), target_minimizers=n_entries, distinct_hashes=len(index), dropped_hashes=sum(len(v) > p["max_occ"] for v in index.values()))
    P = permille(p["secondary_ratio"])
    paf, lines = [], {}
    memo = {} if memo is None else memo
    for name, seq in reads:
        seq = seq.upper()
        if (seq, pred_window) not in memo:      # (a read's result depends on its letters alone)
            memo[seq, pred_window] = map_read(seq, index, p, pred_window)
        n_min, n_anchors, n_groups, chained, kept = memo[seq, pred_window]
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


# ----------------------------------------------------------------------------- inputs that reach one case each
TANDEM_REPEATS = (63, 64, 65, 66)
TANDEM = dict(k=15, w=1, min_count=1, min_score=0)


@functools.lru_cache(maxsize=None)
def tandem_case():
    """A target with 3 copies of a 20-base unit, and reads of r copies of it, each with its reverse complement.  With w = 1 the group of a
    read holds, for every position p of the target's repeat, the about r read positions in phase with it: sorted by (p, q), the diagonal
    predecessor (p - 1, q - 1) lies exactly r anchors back.  r = 63 and 64 reach it (64: in the slot that the anchor itself is about to
    take), 65 does not and chains through what the window still holds, 66 links nothing.  "memo" is for map_reads: the tests of three
    files share what the reads gave"""
    rs = random.Random(640)
    unit = random_seq(rs, 20)
    targets = [("tandem", random_seq(rs, 40) + unit * 3 + random_seq(rs, 40))]
    reads = []
    for r in TANDEM_REPEATS:
        reads += [("f%d" % r, unit * r), ("r%d" % r, revcomp(unit * r))]
    return {"targets": targets, "reads": reads, "params": dict(TANDEM), "memo": {}}


SKETCH_WINDOWS = (191, 192, 193, 383, 384, 385)


def sketch_case(k, w):
    """sequences whose numbers of windows lie around one and two tiles of 192: each a target, its copy and its reverse complement the reads"""
    rs = random.Random(192000 + 100 * k + w)
    targets = [("w%d" % n, random_seq(rs, n + k + w - 2)) for n in SKETCH_WINDOWS]
    reads = [("c%d" % n, seq) for (_, seq), n in zip(targets, SKETCH_WINDOWS)] + [("rc%d" % n, revcomp(seq)) for (_, seq), n in zip(targets, SKETCH_WINDOWS)]
    return targets, reads


def tile_boundaries(seq, k, w, tile=192):
    """how the windows of seq meet at the multiples of `tile`: (boundaries where the window before selects the same position as the window
    after, so that the later tile must not write it again; boundaries where it selects another; pairs of consecutive minimizers with a
    boundary above the first and not above the second)"""
    km, choice = window_choices(seq, k, w)
    same = sum(choice[j] is not None and choice[j] == choice[j - 1] for j in range(tile, len(choice), tile))
    other = sum(choice[j] is not None and choice[j - 1] is not None and choice[j] != choice[j - 1] for j in range(tile, len(choice), tile))
    mins = [p for _, p, _ in minimizers(seq, k, w)]
    straddle = sum(1 for a, b in zip(mins, mins[1:]) for j in range(tile, len(choice), tile) if a < j <= b)
    return same, other, straddle


SELECT = dict(k=15, w=1, secondary_ratio=0.8)


@functools.lru_cache(maxsize=None)
def select_case():
    """Reads of 100 bases with w = 1: a target that holds all of a read chains to 100, one that holds its first n bases to n, when the base
    after the prefix differs from the read's (set here) and no 15-mer of a flank matches by chance (asserted where this is used).  `exact`
    has a second chain of 80 = 0.8 * 100, `below` one of 79; `three` and `four` lie on that many identical targets"""
    rs = random.Random(800)
    targets, reads = [], []

    def other_than(c):
        return rs.choice([x for x in "ACGT" if x != c])

    for name, copies in (("three", 3), ("four", 4)):
        read = random_seq(rs, 100)
        target = random_seq(rs, 30) + read + random_seq(rs, 30)
        targets += [("%s%d" % (name, i), target) for i in range(copies)]
        reads.append((name, read))
    for name, n in (("exact", 80), ("below", 79)):
        read = random_seq(rs, 100)
        targets.append((name + "_all", random_seq(rs, 30) + read + random_seq(rs, 30)))
        targets.append((name + "_prefix", random_seq(rs, 30) + read[:n] + other_than(read[n]) + random_seq(rs, 29)))
        reads.append((name, read))
    return targets, reads
