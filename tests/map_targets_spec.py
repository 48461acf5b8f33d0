"""map -g in Python: the specification of "map, annotated targets" (include/tksmseq.h).  Which transcripts of a table become targets, their
letters and the image the mapper reads, the FASTA of --targets-out, the projection of a PAF line to genome coordinates (--genome-coords), and
the whole route: map_split_spec.map_reads on the spliced targets, followed by the projection.  Plain Python, letter by letter and column by
column: nothing here shares code with the product."""
import map_split_spec as S

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
COUNTERS = ("transcripts", "targets", "letters", "exons", "skipped_empty", "skipped_unknown_contig", "skipped_bad_exon", "projectable", "image_vwords")
PROJECT_COUNTERS = ("lines", "projected", "unprojected", "junctions")


def parse(gtfs):
    """[(name, text)] or [text] of GTF files, read with skip_non_coding = 0 -> [(transcript id, [(contig, start, end, minus)])] in table order"""
    import tsb_spec
    return [(tid, [(c, a, b, not plus) for c, a, b, plus in exons]) for tid, exons in tsb_spec.read_gtfs(gtfs, 0).items()]


def _minus(x):
    return x in (True, "-", 1)


def revcomp(s):
    return "".join(_COMP.get(c, "N") for c in reversed(s))


def targets(genome, transcripts):
    """genome: {contig: letters} (a contig that is declared only: None); transcripts: [(id, [(contig, start, end, strand)])], 0-based half-open,
    strand '+' / '-' or minus as a bool.  -> dict: names, lengths, voff (n + 1 entries), seqs (the letters, N for a letter outside ACGT),
    codes and valid (the image as lists of 32-bit words), info (COUNTERS), projectable, exons (per target its non-empty exons
    (contig, start, end, minus)), tx (the table index of every target)"""
    out = dict(names=[], lengths=[], voff=[0], seqs=[], projectable=[], exons=[], tx=[])
    info = dict.fromkeys(COUNTERS, 0)
    info["transcripts"] = len(transcripts)
    for t, (tid, exons) in enumerate(transcripts):
        exons = [(c, a, b, _minus(m)) for c, a, b, m in exons]
        if all(a == b for _, a, b, _ in exons):
            info["skipped_empty"] += 1
            continue
        if any(genome.get(c) is None for c, _, _, _ in exons):
            info["skipped_unknown_contig"] += 1
            continue
        if any(b < a or b > len(genome[c]) for c, a, b, _ in exons):
            info["skipped_bad_exon"] += 1
            continue
        kept = [e for e in exons if e[1] != e[2]]
        letters = []
        for c, a, b, minus in kept:
            part = "".join(x if x in _COMP else "N" for x in genome[c][a:b].upper())
            letters.append(revcomp(part) if minus else part)
        seq = "".join(letters)
        if len(out["names"]) + 1 >= 1 << 31 or len(seq) >= 1 << 31 or info["letters"] + len(seq) >= 1 << 36:
            raise OverflowError("map: a limit of the target set")
        proj = len({(c, m) for c, _, _, m in kept}) == 1
        for (_, a0, b0, m), (_, a1, b1, _) in zip(kept, kept[1:]):
            proj = proj and (b1 <= a0 if m else a1 >= b0)
        out["names"].append(tid)
        out["lengths"].append(len(seq))
        out["voff"].append(out["voff"][-1] + (len(seq) + 31) // 32)
        out["seqs"].append(seq)
        out["projectable"].append(proj)
        out["exons"].append(kept)
        out["tx"].append(t)
        info["letters"] += len(seq)
        info["exons"] += len(kept)
        info["projectable"] += proj
    info["targets"] = len(out["names"])
    info["image_vwords"] = out["voff"][-1]
    if not out["names"]:
        raise ValueError("map: no transcript of the table can be a target")
    codes, valid = [0] * (2 * out["voff"][-1]), [0] * out["voff"][-1]
    for v, seq in zip(out["voff"], out["seqs"]):
        for g, x in enumerate(seq):
            if x in _COMP:
                codes[2 * v + (g >> 4)] |= "ACGT".index(x) << (2 * (g & 15))
                valid[v + (g >> 5)] |= 1 << (g & 31)
    out.update(codes=codes, valid=valid, info=info)
    return out


def fasta(t, line_width=60):
    """the bytes of tksmseq_targets_write_fasta for targets() t"""
    out = []
    for name, seq in zip(t["names"], t["seqs"]):
        out.append(">" + name + "\n")
        width = line_width if line_width > 0 else len(seq)
        out += [seq[i:i + width] + "\n" for i in range(0, len(seq), width)]
    return "".join(out).encode()


def genome_position(exons, x):
    """G(x) and the exon that holds transcript position x: exons = the non-empty exons (contig, start, end, minus) of a projectable target"""
    for e, (_, a, b, minus) in enumerate(exons):
        if x < b - a:
            return (b - 1 - x if minus else a + x), e
        x -= b - a
    raise IndexError("a position behind the transcript")


def cigar_runs(text):
    runs, n = [], 0
    for ch in text:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            runs.append((n, ch))
            n = 0
    return runs


def project_line(line, target, exons):
    """line: a PAF line without its end; target = (transcript id, contig length); exons: the non-empty exons of a projectable target.
    -> (the projected line, the junctions it counts)"""
    tid, contig_len = target
    f = line.split("\t")
    a, b = int(f[7]), int(f[8])
    minus = exons[0][3]
    (ga, ea), (gb, eb) = genome_position(exons, a), genome_position(exons, b - 1)
    junctions = eb - ea
    f[4] = "+" if (f[4] == "-") == minus else "-"
    f[5], f[6] = exons[0][0], str(contig_len)
    f[7], f[8] = (str(gb), str(ga + 1)) if minus else (str(ga), str(gb + 1))
    for i in range(12, len(f)):
        if not f[i].startswith("cg:Z:"):
            continue
        columns, x, last, junctions = [], a, None, 0          # last: the genome position and exon of the target-consuming column before
        for n, op in cigar_runs(f[i][5:]):
            for _ in range(n):
                if op != "I":
                    g, e = genome_position(exons, x)
                    if last is not None and e != last[1]:
                        gap = abs(g - last[0]) - 1
                        if gap:
                            columns += ["N"] * gap
                            junctions += 1
                    last = (g, e)
                    x += 1
                columns.append(op)
        if minus:
            columns.reverse()
        runs = []
        for op in columns:
            if runs and runs[-1][1] == op:
                runs[-1][0] += 1
            else:
                runs.append([1, op])
        f[i] = "cg:Z:" + "".join("%d%s" % (n, op) for n, op in runs)
    f.append("tx:Z:" + tid)
    return "\t".join(f), junctions


def map_reads(genome, transcripts, reads, genome_coords=False, split=False, memo=None, **modes):
    """map_split_spec.map_reads on the spliced targets (its modes and parameters), then with genome_coords the projection of every line on a
    projectable target.  Its result with "project": PROJECT_COUNTERS, "first_unprojected": the transcript of the first line left as it was,
    and "targets": targets(genome, transcripts)"""
    t = memo["targets"] if memo is not None and "targets" in memo else targets(genome, transcripts)
    if memo is not None:
        memo["targets"] = t
    out = S.map_reads(list(zip(t["names"], t["seqs"])), reads, split=split, memo=memo, **modes)
    project = dict.fromkeys(PROJECT_COUNTERS, 0)
    first = None
    if genome_coords:
        at = {name: i for i, name in enumerate(t["names"])}           # (ids are unique: the table keeps the first)
        lines = []
        for line in out["paf"].splitlines():
            i = at[line.split("\t")[5]]
            project["lines"] += 1
            if t["projectable"][i]:
                line, j = project_line(line, (t["names"][i], len(genome[t["exons"][i][0][0]])), t["exons"][i])
                project["projected"] += 1
                project["junctions"] += j
            else:
                first = first or t["names"][i]
                project["unprojected"] += 1
            lines.append(line + "\n")
        out["paf"] = "".join(lines)
    out.update(project=project, first_unprojected=first, targets=t)
    return out


# ----------------------------------------------------------------------------- the table tools/sanitize_map_targets_host.cpp walks
def lcg_letters(n, seed):
    out, x = [], seed
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append("N" if i % 23 == 7 else "ACGT"[x >> 30])
    return "".join(out)


HOST_GENOME = {"c1": lcg_letters(100, 1), "c2": lcg_letters(50, 2), "cd": None}      # (cd: declared only)
HOST_TABLE = [
    ("A", [("c1", 10, 30, "+"), ("c1", 40, 45, "+")]),                              # projectable, one junction of 10
    ("B", [("c1", 60, 80, "-"), ("c1", 50, 55, "-")]),                              # descending `-`
    ("C", []),                                                                      # no exon
    ("D", [("c1", 5, 5, "+")]),                                                     # all exons empty
    ("E", [("cX", 0, 10, "+")]),                                                    # unknown contig
    ("F", [("c1", 90, 101, "+")]),                                                  # behind the contig's end
    ("G", [("c1", 0, 10, "+"), ("c2", 40, 50, "-")]),                               # two contigs, two strands: the last base of c2
    ("H", [("c1", 20, 30, "+"), ("c1", 30, 33, "+"), ("c1", 33, 33, "+"), ("c1", 35, 40, "+")]),   # a gap of 0, an empty exon, a gap of 2
    ("I", [("c1", 50, 60, "+"), ("c1", 40, 45, "+")]),                              # turns back
    ("J", [("c1", 30, 20, "+")]),                                                   # end < start
    ("K", [("cX", 0, 10, "+"), ("c1", 90, 101, "+")]),                              # unknown before bad
    ("L", [("cd", 3, 3, "+"), ("c1", 0, 33, "+")]),                                 # declared only
    ("M", [("c2", 0, 1, "-")]),                                                     # one letter
    ("N", [("c2", 0, 32, "+"), ("c2", 32, 50, "-")]),                               # a word's worth, then the rest mirrored
]
