"""Specification of mutate, an independent string model of it, and the reference's own apply_mods restated (TEST INFRASTRUCTURE ONLY;
imported by tests/test_mutate.py and tests/test_mutate_gpu.py, nothing under tksm_amd/).

  * `parse_variants` / `normal_form`: the table reader and the normal form of include/tksmseq.h ("mutate").
  * `mutate_spec`: the transform over the molecule dicts of oracle/mdf_ops_oracle.py, which tksmseq_mutate reproduces text for text.
  * `mutated_contig`: NOT a restatement of the walk -- per position of a contig the text that replaces the base, read off the raw table
    rows (no normal form, no pieces).  A perfect read of a mutated molecule must equal the joined slices of it.
  * `mutate_reference`: read_modifications + apply_mods of src/mutate.cpp:27-181 (with the slicing constructor, src/interval.h:695-703)
    line by line, defects included; the tests state where it and the specification agree and where they part.
  * corpora: `crafted_tables` makes every meeting of a variant with a segment end of tests/mdf_edge_cases.py happen on purpose;
    `random_case` / `random_corpus` draw small mixed cases."""
import copy

import numpy as np

EINVAL, ELIMIT = 1, 6
MAX_POS = 2 ** 31 - 1
MAX_INSERTION = 1 << 20
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a"}


class VariantError(ValueError):
    def __init__(self, code, line, why):
        super().__init__(f"{line}: {why}")
        self.code, self.line = code, line


def _pos(tok):
    if not tok or not all(48 <= b <= 57 for b in tok):
        return None
    v = int(tok)
    return v if v <= MAX_POS else None


def parse_variants(text):
    """[(contig, pos, kind, payload, line)]: kind "del" (payload = the other end), "snv" (the letter), "ins" ((X or None, SEQ))"""
    data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    rows = []
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for ln, line in enumerate(lines, 1):
        f = line.split()                                                # ASCII whitespace
        if not f:
            continue
        if len(f) < 3:
            raise VariantError(EINVAL, ln, "fewer than three fields")
        if len(rows) + 1 >= 2 ** 31:
            raise VariantError(ELIMIT, ln, "2^31 rows")
        pos = _pos(f[1])
        if pos is None:
            raise VariantError(EINVAL, ln, "POS")
        contig, mod = f[0].decode("latin-1"), f[2]
        if all(48 <= b <= 57 for b in mod):
            end = _pos(mod)
            if end is None:
                raise VariantError(EINVAL, ln, "deletion end")
            rows.append((contig, pos, "del", end, ln))
        elif len(mod) == 1:
            if mod == b".":
                raise VariantError(EINVAL, ln, "lone '.'")
            rows.append((contig, pos, "snv", mod.decode("latin-1"), ln))
        else:
            if len(mod) - 1 > MAX_INSERTION:
                raise VariantError(ELIMIT, ln, "insertion longer than 2^20")
            x = mod[:1].decode("latin-1")
            rows.append((contig, pos, "ins", (None if x == "." else x, mod[1:].decode("latin-1")), ln))
    return rows


def normal_form(rows):
    """({contig: {"ranges": [(f, t)], "points": [(pos, line, letter or None, SEQ or None)]}}, counters)"""
    nf = {}
    for contig, pos, kind, payload, ln in rows:
        c = nf.setdefault(contig, {"dels": [], "points": []})
        if kind == "del":
            if payload != pos:
                c["dels"].append((min(pos, payload), max(pos, payload)))
        elif kind == "snv":
            c["points"].append((pos, ln, payload, None))
        else:
            c["points"].append((pos, ln, payload[0], payload[1]))
    dropped = 0
    for c in nf.values():
        ranges = []
        for f, t in sorted(c.pop("dels")):
            if ranges and f <= ranges[-1][1]:
                ranges[-1] = (ranges[-1][0], max(ranges[-1][1], t))
            else:
                ranges.append((f, t))
        kept = [p for p in sorted(c["points"], key=lambda p: (p[0], p[1])) if not any(f <= p[0] < t for f, t in ranges)]
        dropped += len(c["points"]) - len(kept)
        c["ranges"], c["points"] = ranges, kept
    counters = dict(rows=len(rows), snvs=sum(r[2] == "snv" for r in rows), insertions=sum(r[2] == "ins" for r in rows),
                    deletions=sum(r[2] == "del" for r in rows), deleted_ranges=sum(len(c["ranges"]) for c in nf.values()), dropped_points=dropped)
    return nf, counters


def _segment(seg, c):
    s, e = seg["start"], seg["end"]
    if c is None or e <= s:
        return [copy.deepcopy(seg)]
    ranges = [(f, t) for f, t in c["ranges"] if t > s and f < e]
    points = [p for p in c["points"] if s <= p[0] < e]
    subs = [p for p in points if p[2] is not None]
    events = [(f, 0, ("del", f, t)) for f, t in ranges] + [(p[0], p[1], ("ins", p[0], p[3])) for p in points if p[3] is not None]
    if not events:
        out = copy.deepcopy(seg)
        out["errors"] += [(p[0] - s, p[2]) for p in subs]
        return [out]
    out, cur = [], s

    def piece(a, b):
        if b <= a:
            return
        errs = [(q - (a - s), base) for q, base in seg["errors"] if a - s <= q < b - s]
        errs += [(p[0] - a, p[2]) for p in subs if a <= p[0] < b]
        out.append(dict(chr=seg["chr"], start=a, end=b, plus=seg["plus"], errors=errs))

    for _, _, ev in sorted(events, key=lambda x: (x[0], x[1])):
        if ev[0] == "del":
            piece(cur, max(cur, ev[1]))
            cur = min(ev[2], e)
        else:
            piece(cur, ev[1] + 1)
            out.append(dict(chr=ev[2], start=0, end=len(ev[2]), plus=seg["plus"], errors=[]))
            cur = ev[1] + 1
    piece(cur, e)
    return out if seg["plus"] else out[::-1]


def mutate_spec(mols, nf):
    """mols: depth-unrolled molecule dicts (mdf_ops_oracle.stream_mdf(unroll=True)); nf: normal_form(...)[0]"""
    out = []
    for md in mols:
        m = dict(id=md["id"], depth=md["depth"], meta=copy.deepcopy(md["meta"]), segments=[])
        for seg in md["segments"]:
            m["segments"] += _segment(seg, nf.get(seg["chr"]))
        out.append(m)
    return out


# ------------------------------------------------------------------------------------------------ the independent model
def mutated_contig(seq, table, lo=0, hi=None):
    """{position: text} for lo <= position < hi: what stands in the mutated contig in place of base `position` of seq -- "" when a deletion
    covers it, else the base (or the letter of the last SNV / insertion anchor letter at it, in line order) followed by the texts inserted
    behind it, in line order.  table: the raw rows of this contig, [(contig, pos, kind, payload, line)]."""
    hi = len(seq) if hi is None else min(hi, len(seq))
    out = {i: [seq[i], ""] for i in range(max(lo, 0), hi)}
    gone = set()
    for _, pos, kind, payload, _ in sorted(table, key=lambda r: r[4]):
        if kind == "del":
            gone.update(i for i in range(max(min(pos, payload), lo), min(max(pos, payload), hi)))
        elif pos in out:
            if kind == "snv":
                out[pos][0] = payload
            else:
                if payload[0] is not None:
                    out[pos][0] = payload[0]
                out[pos][1] += payload[1]
    return {i: "" if i in gone else v[0] + v[1] for i, v in out.items()}


def revcomp(s):
    return "".join(_COMP.get(ch, ch) for ch in reversed(s))


def splice(mols_or_md, genome):
    """py/sequence.py:303-313 in plain Python: the perfect read of a molecule (a list: of each)"""
    if isinstance(mols_or_md, (list, tuple)):
        return [splice(md, genome) for md in mols_or_md]
    out = []
    for seg in mols_or_md["segments"]:
        contig = genome.get(seg["chr"], seg["chr"])
        t = list(contig[seg["start"]:seg["end"]]) if seg["end"] > seg["start"] else []
        for p, b in seg["errors"]:
            t[p] = b
        t = "".join(t)
        out.append(t if seg["plus"] else revcomp(t))
    return "".join(out)


def expected_read(md, genome, rows):
    """the perfect read of the MUTATED molecule by the string model: per segment of the ORIGINAL molecule, the slice [start, end) of the
    mutated contig -- the contig with the segment's own substitutions put in first, which the table's letters override -- reverse-
    complemented for a minus segment.  A literal is its own contig, named by its text."""
    by_contig = {}
    for r in rows:
        by_contig.setdefault(r[0], []).append(r)
    out = []
    for seg in md["segments"]:
        contig = genome.get(seg["chr"], seg["chr"])
        s, e = seg["start"], min(seg["end"], len(contig))
        if e <= s:
            continue
        own = list(contig[s:e])
        for p, b in seg["errors"]:
            own[p] = b
        if seg["chr"] in by_contig:
            m = mutated_contig(contig[:s] + "".join(own) + contig[e:], by_contig[seg["chr"]], s, e)
            t = "".join(m[i] for i in range(s, e))
        else:
            t = "".join(own)
        out.append(t if seg["plus"] else revcomp(t))
    return "".join(out)


# ------------------------------------------------------------------------------------------------ the reference, restated
def _slice(ei, start, end):                                            # einterval(const einterval&, int, int), src/interval.h:695-703
    return dict(chr=ei["chr"], start=ei["start"] + start, end=ei["start"] + end, plus=ei["plus"],
                errors=[(p - start, b) for p, b in ei["errors"] if not (p < start or p > end)])


def _ref_apply(mod, i):                                                # Mod::operator(), src/mutate.cpp:44-115
    pos, kind, payload = mod
    if kind == "snv":
        if pos < i["start"] or pos > i["end"]:
            return [i]
        i["errors"].append((pos - i["start"], payload))
        return [i]
    if kind == "ins":
        if payload[0] != ".":
            i["errors"].append((pos - i["start"], payload[0]))
        return [_slice(i, 0, pos - i["start"]), dict(chr=payload[1:], start=0, end=len(payload) - 1, plus=True, errors=[]),
                _slice(i, pos + 1 - i["start"], i["end"] - i["start"])]
    a, b = (payload[1], payload[0]) if payload[0] > payload[1] else payload
    if i["start"] > a and i["end"] < b:
        return []
    if i["start"] < a and i["end"] < b:
        return [_slice(i, 0, a - i["start"])]
    if i["start"] > a and i["end"] > b:
        return [_slice(i, a - i["start"], i["end"] - i["start"])]
    if i["start"] < a and i["end"] > b:
        return [_slice(i, 0, a - i["start"]), _slice(i, b - i["start"], i["end"] - i["start"])]
    return []


def mutate_reference(mols, text):
    """read_modifications (src/mutate.cpp:157-181) + apply_mods (:124-156) on well-formed tables.  std::ranges::sort by pos is taken as
    stable (a deletion and its reversed copy, which tie, do the same thing)."""
    forest = {}
    for line in text.split("\n"):
        f = line.split()
        if len(f) < 3:
            continue
        pos, ms = int(f[1]), f[2]
        mods = forest.setdefault(f[0], [])
        if ms.isdigit():
            mods.append((pos, "del", (pos, int(ms))))
            mods.append((pos, "del", (int(ms), pos)))                   # reversed(): the ends swapped, the SAME pos
        elif len(ms) == 1:
            mods.append((pos, "snv", ms))
        else:
            mods.append((pos, "ins", ms))
    for mods in forest.values():
        mods.sort(key=lambda m: m[0])
    out = []
    for md in mols:
        m = dict(id=md["id"], depth=md["depth"], meta=copy.deepcopy(md["meta"]), segments=[])
        for e in md["segments"]:
            if e["chr"] not in forest:
                continue                                               # (:129-131)
            mods = forest[e["chr"]]
            k = 0
            while k < len(mods) and mods[k][0] < e["start"]:
                k += 1
            bin_a = [copy.deepcopy(e)]
            while k < len(mods) and mods[k][0] < e["end"]:
                bin_b = []
                for ee in bin_a:
                    if ee["chr"] != e["chr"] or mods[k][0] < ee["start"] or mods[k][0] > ee["end"]:
                        bin_b.append(ee)
                        continue
                    bin_b += _ref_apply(mods[k], ee)
                bin_a = bin_b
                k += 1
            m["segments"] += bin_a
        out.append(m)
    return out


# ------------------------------------------------------------------------------------------------ corpora
N_SCENARIOS = 12


def _scenario(k, chrom, s, e, nxt):
    """the table lines that make variant kind k meet segment [s, e) of chrom; nxt: (start, end) of a later segment of the same molecule on
    the same contig, or None"""
    sz = e - s
    L = []

    def add(pos, mod):
        if pos >= 0 and (not str(mod).isdigit() or int(mod) >= 0):
            L.append(f"{chrom}\t{pos}\t{mod}\n")
    if k == 0:
        for p, b in ((s - 1, "A"), (s, "C"), (e - 1, "G"), (e, "T")):
            add(p, b)
    elif k == 1:
        add(s, s + max(1, sz // 3))                                      # f == s
    elif k == 2:
        add(e - max(1, sz // 3), e)                                      # t == e
    elif k == 3:
        add(s, e)                                                        # [s, e) exactly
    elif k == 4:
        add(max(s - 1, 0), e + 1)                                        # one base wider on each side
    elif k == 5:
        if sz >= 3:
            add(s + 1, e - 1)                                            # strictly inside
        else:
            add(s, "G")
    elif k == 6:
        add(s, ".ACG")                                                   # anchored at s
    elif k == 7:
        add(e - 1, "TGG")                                                # anchored at e - 1, the anchor replaced
    elif k == 8:
        add(e, ".CC")                                                    # anchored at e: not this segment's
        add(e - 1, "A")
    elif k == 9:
        if nxt is not None and sz >= 2 and nxt[1] - nxt[0] >= 2:
            add(s + sz // 2, nxt[0] + (nxt[1] - nxt[0]) // 2)            # spanning two segments of one molecule
        else:
            add(s + sz // 2, "T")
            add(s + sz // 2, "CAA")
    elif k == 10:
        p = s + sz // 2                                                  # two insertions and an SNV at one anchor; a reversed deletion
        add(p, "GTT")
        add(p, "A")
        add(p, "CGA")
        if sz >= 8:
            add(s + 4, s + 2)
            add(s + 3, "T")                                              # inside it: dropped
    else:
        add(s + 1, s + 2)                                                # overlapping deletions, an insertion in front, one behind
        add(s + 1, s + 3)
        add(s, ".T")
        add(s + 3, "AC")
        add(e - 1, e + 5)
    return L


def crafted_tables(mols):
    """N_SCENARIOS tables over the segments of mols: in table k the j-th segment (over all molecules) meets scenario (j + k) % N_SCENARIOS.
    Literal segments are contigs named by their text."""
    tables = [[] for _ in range(N_SCENARIOS)]
    j = 0
    for md in mols:
        segs = md["segments"]
        for a, seg in enumerate(segs):
            nxt = next(((t["start"], t["end"]) for t in segs[a + 1:] if t["chr"] == seg["chr"] and t["start"] > seg["end"]), None)
            for k in range(N_SCENARIOS):
                tables[k] += _scenario((j + k) % N_SCENARIOS, seg["chr"], seg["start"], seg["end"], nxt)
            j += 1
    return ["".join(t) + "unused_contig\t5\tA\n" for t in tables]


def random_table(rs, contigs, n_rows, max_ins=4):
    """contigs: {name: length}; mixed kinds, shared anchors, overlapping and reversed deletions"""
    names = sorted(contigs)
    lines, anchors = [], []
    for _ in range(n_rows):
        c = names[rs.randint(len(names))]
        n = contigs[c]
        kind = rs.randint(4)
        pos = anchors[rs.randint(len(anchors))][1] if anchors and rs.randint(4) == 0 and anchors[-1][0] == c else int(rs.randint(0, n + 1))
        anchors.append((c, pos))
        if kind == 0:
            lines.append(f"{c}\t{pos}\t{'ACGT'[rs.randint(4)]}\n")
        elif kind == 1:
            lines.append(f"{c}\t{pos}\t{int(np.clip(pos + rs.randint(-4, 5), 0, n + 2))}\n")
        else:
            seq = "".join("ACGT"[x] for x in rs.randint(0, 4, rs.randint(1, max_ins + 1)))
            lines.append(f"{c}\t{pos}\t{'.ACGT'[rs.randint(5)]}{seq}\n")
    return "".join(lines)


def random_molecules(rs, genome, literals, n, prefix="r", with_subs=True):
    """MDF text of n records: 1-3 segments on the contigs of `genome` or on one of `literals`, both strands, 0-2 substitutions of their own,
    now and then an empty segment, no segment, depth 2"""
    names = sorted(genome)
    out = []
    for i in range(n):
        depth = 2 if rs.randint(16) == 0 else 1
        out.append(f"+{prefix}{i}\t{depth}\t{'a=1;' if i % 5 == 0 else ''}\n")
        for _ in range(0 if rs.randint(24) == 0 else rs.randint(1, 4)):
            if literals and rs.randint(5) == 0:
                c = literals[rs.randint(len(literals))]
                n_c = len(c)
            else:
                c = names[rs.randint(len(names))]
                n_c = len(genome[c])
            s = int(rs.randint(0, n_c))
            e = s if rs.randint(12) == 0 else int(rs.randint(s + 1, min(n_c, s + 14) + 1))
            subs = ""
            if with_subs and e > s:
                subs = ",".join(f"{int(rs.randint(0, e - s))}{'ACGT'[rs.randint(4)]}" for _ in range(rs.randint(0, 3)))
            out.append(f"{c}\t{s}\t{e}\t{'+-'[rs.randint(2)]}\t{subs}\n")
    return "".join(out)


def random_genome(rs, n_contigs=3, lo=12, hi=40):
    return {f"c{k}": "".join("ACGT"[x] for x in rs.randint(0, 4, rs.randint(lo, hi + 1))) for k in range(n_contigs)}


RANDOM_LITERALS = ("ACGTTGCAAGGCT", "TTGACCA")


def random_case(seed):
    """one small case: (genome, table text, MDF text)"""
    rs = np.random.RandomState(seed)
    genome = random_genome(rs)
    contigs = {k: len(v) for k, v in genome.items()}
    contigs.update({lit: len(lit) for lit in RANDOM_LITERALS[:rs.randint(0, 3)]})
    return genome, random_table(rs, contigs, rs.randint(0, 9)), random_molecules(rs, genome, list(RANDOM_LITERALS), rs.randint(1, 4))
