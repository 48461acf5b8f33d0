"""model-sequence in plain Python: the counting rules of include/tksmseq.h ("model-sequence") stated slowly and obviously -- dicts of counts,
'%.6f' % (c / t) -- and a generator of inputs that are consistent by construction (the column string is drawn first; the read follows from
the reference and the columns).  The file formats are those of py/tksm_badread.py's loaders (:91-117, :546-582); Badread's own counting
rules are not in the reference tree, so the rules here are this project's ("model-sequence")."""
import gzip
import os
import random
import re

ACGT = "ACGT"
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")
FORCED = ("=", "X", "I")


def _open(path):
    path = str(path)
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path)


def revcomp(s):
    return s.translate(_COMP)[::-1]


def read_fasta(path):
    """{name up to the first white space: upper-cased sequence}, in file order"""
    out, name = {}, None
    with _open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                name = line[1:].split()[0]
                out[name] = []
            elif name is not None:
                out[name].append(line.upper())
    return {k: "".join(v) for k, v in out.items()}


def read_fastq(paths):
    """{name: (upper-cased bases, [q])}: four lines per record"""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    out = {}
    for path in paths:
        with _open(path) as f:
            lines = [ln.rstrip("\r\n") for ln in f]
        at, rec = 0, 0
        while at < len(lines):
            if lines[at] == "":                             # empty lines between records and at the end are passed over
                at += 1
                continue
            rec += 1
            if at + 4 > len(lines):
                raise ValueError("FASTQ record %d: the file ends inside the record" % rec)
            head, seq, plus, qual = lines[at:at + 4]
            at += 4
            if not head.startswith("@") or not plus.startswith("+") or len(seq) != len(qual):
                raise ValueError("FASTQ record %d" % rec)
            q = [ord(c) - 33 for c in qual]
            if any(v < 0 or v > 93 for v in q):
                raise ValueError("FASTQ record %d: a quality outside '!' .. '~'" % rec)
            name = re.split(r"[ \t]", head[1:])[0]
            if name in out:
                raise ValueError("FASTQ record %d: a read of this name came before" % rec)
            out[name] = (seq.upper(), q)
    return out


def _small_int(text, line_no, col):
    if not re.fullmatch(r"[0-9]{1,10}", text) or int(text) >= 2 ** 31:
        raise ValueError("PAF line %d: column %d is no integer in [0, 2^31)" % (line_no, col + 1))
    return int(text)


def parse_paf(path, reads, ref, max_alignments=0):
    """the used lines, in file order, and the counters; ValueError("PAF line N: ...") for an input error"""
    used = []
    info = dict(lines=0, skipped_no_cigar=0, skipped_supplementary=0, skipped_unknown_read=0, skipped_unknown_target=0, skipped_cigar_op=0)
    with _open(path) as f:
        for line_no, line in enumerate(f, 1):
            if max_alignments and len(used) >= max_alignments:
                break
            line = line.rstrip("\r\n")
            if line == "":
                continue
            info["lines"] += 1
            col = line.split("\t")
            if len(col) < 12:
                raise ValueError("PAF line %d: fewer than 12 columns" % line_no)
            cg = [c[5:] for c in col[12:] if c.startswith("cg:Z:")]
            if not cg:
                info["skipped_no_cigar"] += 1
                continue
            if "tp:A:S" in col[12:]:
                info["skipped_supplementary"] += 1
                continue
            if col[0] not in reads:
                info["skipped_unknown_read"] += 1
                continue
            if col[5] not in ref:
                info["skipped_unknown_target"] += 1
                continue
            cigar = cg[-1]
            ops = re.findall(r"([0-9]+)([A-Za-z=])", cigar)
            if cigar == "" or "".join(n + o for n, o in ops) != cigar:
                raise ValueError("PAF line %d: the cg:Z: tag is no CIGAR" % line_no)
            if any(o not in "M=XID" for _, o in ops):
                info["skipped_cigar_op"] += 1
                continue
            qlen, qstart, qend, tstart, tend = (_small_int(col[c], line_no, c) for c in (1, 2, 3, 7, 8))
            if col[4] not in "+-" or len(col[4]) != 1:
                raise ValueError("PAF line %d: column 5 is neither + nor -" % line_no)
            if qstart > qend or qend > qlen:
                raise ValueError("PAF line %d: the query range is not inside the query" % line_no)
            if tstart > tend or tend > len(ref[col[5]]):
                raise ValueError("PAF line %d: the target range is not inside the reference contig" % line_no)
            if qlen != len(reads[col[0]][0]):
                raise ValueError("PAF line %d: column 2 differs from the length of the FASTQ read" % line_no)
            ops = [(int(n), o) for n, o in ops]
            if sum(n for n, o in ops if o != "D") != qend - qstart or sum(n for n, o in ops if o != "I") != tend - tstart:
                raise ValueError("PAF line %d: the CIGAR does not consume the aligned ranges" % line_no)
            used.append(dict(read=col[0], target=col[5], strand=col[4], qlen=qlen, qstart=qstart, qend=qend, tstart=tstart, tend=tend, ops=ops))
    info["used"] = len(used)
    return used, info


def columns(aln, reads, ref):
    """(letters, read bases per column or None, reference offsets per column or None, aligned bases, their qualities)"""
    seq, qual = reads[aln["read"]]
    if aln["strand"] == "-":
        seq, qual = revcomp(seq), qual[::-1]
        lo, hi = aln["qlen"] - aln["qend"], aln["qlen"] - aln["qstart"]
    else:
        lo, hi = aln["qstart"], aln["qend"]
    bases, quals = seq[lo:hi], qual[lo:hi]
    target = ref[aln["target"]]
    letters, rpos, tpos = [], [], []
    i, t = 0, aln["tstart"]
    for n, op in aln["ops"]:
        for _ in range(n):
            if op in "M=X":
                letters.append("=" if bases[i] == target[t] and bases[i] in ACGT else "X")
                rpos.append(i); tpos.append(t)
                i += 1; t += 1
            elif op == "I":
                letters.append("I"); rpos.append(i); tpos.append(None)
                i += 1
            else:
                letters.append("D"); rpos.append(None); tpos.append(t)
                t += 1
    return "".join(letters), rpos, tpos, bases, quals


def count(ref, reads, used, error_k=7, qscore_k=9, max_del=6):
    """the counts of both models over the used alignments"""
    K = error_k
    total, alts = {}, {}
    qs, overall = {}, {}
    info = dict(counting_positions=0, alternatives_too_long=0, windows_max_del=0, keys_too_long=0, read_positions=0)
    for aln in used:
        letters, rpos, tpos, bases, quals = columns(aln, reads, ref)
        target = ref[aln["target"]]
        col_of_t = {t: c for c, t in enumerate(tpos) if t is not None}
        col_of_i = {i: c for c, i in enumerate(rpos) if i is not None}
        for t in range(aln["tstart"], aln["tend"] - K + 1):
            kmer = target[t:t + K]
            c0, c1 = col_of_t[t], col_of_t[t + K - 1]
            if any(b not in ACGT for b in kmer) or letters[c0] != "=" or letters[c1] != "=":
                continue
            alt = "".join(bases[rpos[c]] for c in range(c0, c1 + 1) if rpos[c] is not None)
            if any(b not in ACGT for b in alt):
                continue
            total[kmer] = total.get(kmer, 0) + 1
            info["counting_positions"] += 1
            if len(alt) <= K + 4:
                alts.setdefault(kmer, {})
                alts[kmer][alt] = alts[kmer].get(alt, 0) + 1
            else:
                info["alternatives_too_long"] += 1
        n = len(bases)
        for i in range(n):
            q = quals[i]
            overall[q] = overall.get(q, 0) + 1
            info["read_positions"] += 1
            for h in range((qscore_k - 1) // 2 + 1):
                if i - h < 0 or i + h > n - 1:
                    continue
                key = letters[col_of_i[i - h]:col_of_i[i + h] + 1]
                if "D" * (max_del + 1) in key:
                    info["windows_max_del"] += 1
                elif len(key) > 29:
                    info["keys_too_long"] += 1
                else:
                    qs.setdefault(key, {})
                    qs[key][q] = qs[key].get(q, 0) + 1
    # distinct counted keys: (k-mer, alternative) pairs, and one per k-mer for its alternatives that are too long
    info["error_keys"] = sum(len(a) for a in alts.values()) + sum(1 for k in total if total[k] > sum(alts.get(k, {}).values()))
    info["qscore_keys"] = len(qs)
    return total, alts, qs, overall, info


def error_model_text(K, total, alts, max_alt=25):
    out = []
    for idx in range(4 ** K):
        kmer = "".join(ACGT[(idx >> (2 * (K - 1 - j))) & 3] for j in range(K))
        t = total.get(kmer, 0)
        if t == 0:
            out.append(kmer + ",1.000000;\n")
            continue
        a = alts.get(kmer, {})
        line = "%s,%s;" % (kmer, "%.6f" % (a.get(kmer, 0) / t))
        others = sorted(((c, alt) for alt, c in a.items() if alt != kmer), key=lambda x: (-x[0], len(x[1]), x[1]))
        for c, alt in others[:max_alt]:
            line += "%s,%s;" % (alt, "%.6f" % (c / t))
        out.append(line + "\n")
    return "".join(out)


def _qline(name, counts):
    n = sum(counts.values())
    return "%s;%d;%s\n" % (name, n, "".join("%d:%s," % (q, ("%.6f" % (counts[q] / n)).rstrip("0")) for q in sorted(counts)))


def qscore_model_text(qs, overall, min_occur=100, max_output=10000):
    for f in FORCED:
        if f not in qs:
            raise ValueError("model-sequence: no '%s' column in any used alignment (the q-score model needs the keys =, X and I)" % f)
    order = lambda key: (-sum(qs[key].values()), len(key), key)      # noqa: E731
    sel = sorted((k for k in qs if sum(qs[k].values()) >= min_occur), key=order)[:max_output]
    for f in FORCED:
        if f in sel:
            continue
        if len(sel) >= max_output:
            for i in range(len(sel) - 1, -1, -1):
                if sel[i] not in FORCED:
                    del sel[i]
                    break
        sel.append(f)
    sel.sort(key=order)
    return _qline("overall", overall) + "".join(_qline(k, qs[k]) for k in sel)


def run(reference, reads_paths, paf, error_k=7, qscore_k=9, max_alignments=0, max_alt=25, max_del=6, min_occur=100, max_output=10000):
    """{"error": text, "qscore": text or the ValueError the q-score rule raises, "info": counters}"""
    ref = {}
    for path in ([reference] if isinstance(reference, (str, os.PathLike)) else reference):
        ref.update(read_fasta(path))
    reads = read_fastq(reads_paths)
    used, info = parse_paf(paf, reads, ref, max_alignments)
    if not used:
        raise ValueError("model-sequence: no alignment can be used")
    total, alts, qs, overall, more = count(ref, reads, used, error_k, qscore_k, max_del)
    info.update(more)
    out = {"error": error_model_text(error_k, total, alts, max_alt), "info": info}
    try:
        out["qscore"] = qscore_model_text(qs, overall, min_occur, max_output)
    except ValueError as e:
        out["qscore"] = e
    return out


# ----------------------------------------------------------------------------- the generator
def _draw_columns(rng, n, p_err=0.12, no_ins=False, max_run=3):
    """n column letters: runs of '=', single X, short I / D runs; never a D (or I) at either end"""
    out = []
    while len(out) < n:
        u = rng.random()
        if u > p_err or len(out) == 0:
            out.append("=")
        elif u < p_err * 0.4:
            out.append("X")
        elif u < p_err * 0.7 and not no_ins:
            out += "I" * min(rng.choice((1, 1, 1, 2, 3)), max_run, n - len(out))
        else:
            out += "D" * min(rng.choice((1, 1, 1, 2, 3)), max_run, n - len(out))
    out = out[:n]
    for at in (0, -1):
        if out[at] in "ID":
            out[at] = "="
    return "".join(out)


def _cigar(cols, style):
    """style 0: M for = and X; 1: = and X"""
    ops = ["M" if (c in "=X" and style == 0) else c for c in cols]
    out, i = [], 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j] == ops[i]:
            j += 1
        out.append("%d%s" % (j - i, ops[i]))
        i = j
    return "".join(out)


def host_ops(cigar):
    """the ops of a CIGAR as the host hands them to the device: M, = and X are one code ('M'), an op of length 0 is dropped, neighbours of
    the same code are joined: [(length, 'M' | 'I' | 'D')]"""
    out = []
    for n, o in re.findall(r"([0-9]+)([A-Za-z=])", cigar):
        n, o = int(n), "M" if o in "M=X" else o
        if not n:
            continue
        if out and out[-1][1] == o:
            out[-1] = (out[-1][0] + n, o)
        else:
            out.append((n, o))
    return out


def pass_columns(cigar, width=64):
    """the columns of every pass of `width` ops over host_ops(cigar)"""
    ops = host_ops(cigar)
    return [sum(n for n, _ in ops[a:a + width]) for a in range(0, len(ops), width)]


def columns_of_ops(n_ops, lengths=None, first="="):
    """a column string of exactly n_ops host ops that ends on '=': `first`, then '=' and an 'I' or a 'D' by turns, with one 'ID' pair
    where the count needs it; op x has lengths.get(x, 1) columns"""
    lengths = lengths or {}
    codes = [first]
    while len(codes) < n_ops:
        left = n_ops - len(codes)
        if codes[-1] != "=":
            codes.append("=")
        elif left % 2 == 0:
            codes.append("ID"[len(codes) // 2 % 2])
        else:                                               # an odd number to go after an '=': two ops that are not '=' in a row
            codes += ["I", "D"]
    assert len(codes) == n_ops and (n_ops == 1 or codes[-1] == "=") and all(a != b for a, b in zip(codes, codes[1:]))
    return "".join(c * lengths.get(x, 1) for x, c in enumerate(codes))


def op_of(n_ops, at, code, length):
    """columns_of_ops(n_ops) with op `at` being `length` columns of `code` ('I' or 'D') between two '=' runs of 12 (none before op 0)"""
    first = "=" if at else code
    was = columns_of_ops(n_ops, first=first)[at]          # (every op has one column there)
    assert was in "ID", (n_ops, at)
    cols = columns_of_ops(n_ops, {at - 1: 12, at: length, at + 1: 12}, first=first)
    return cols if was == code else cols.translate(str.maketrans("ID", "DI"))


def shape_cases(max_del=6):
    """{name: column string}: what k_ms_expand takes another path for.  Op counts around one, two and three passes of 64 ops; a first pass
    of 64 ops whose columns end on, just past and just before a step of 64 columns; one op of many steps; a long deletion (a spliced
    alignment) and a long insertion in the first lane, the last lane and the first lane of the second pass; 'D' runs of max_del and
    max_del + 1 behind a window that is already longer than 29 letters"""
    cases = {}
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 192, 193):
        cases["ops_%d" % n] = "=" * 20 + "I" if n == 2 else columns_of_ops(n)
    for total in (64, 65, 127, 128, 129):
        cases["first_pass_%d_columns" % total] = columns_of_ops(71, {0: total - 63})
    for n in (63, 64, 65, 1000, 5000):
        cases["one_op_%d" % n] = "=" * n
    for code, length in (("D", 3000), ("I", 300)):
        for n_ops, at in ((4, 0), (3, 1), (65, 63), (66, 64)):
            cases["%s%d_as_op_%d" % (code, length, at)] = op_of(n_ops, at, code, length)
    full = ("=" + "D" * max_del) * 5 + "="                 # 6 read positions, 6 + 5 max_del letters
    cases["del_max_del_behind_a_long_window"] = "=" * 12 + full + "D" * max_del + "=" * 12
    cases["del_max_del_plus_1_behind_a_long_window"] = "=" * 12 + full + "D" * (max_del + 1) + "=" * 12
    return cases


def generate_shapes(out_dir, max_del=6):
    """20 ordinary alignments and every case of shape_cases() on both strands, on contigs that a 3 000-base deletion fits in"""
    return generate(out_dir, seed=21, n_alignments=20, extra_columns=(), group=0, contig_len=8000, max_del=max_del, shapes=list(shape_cases(max_del).items()))


def generate(out_dir, seed=1, n_alignments=200, col_lo=60, col_hi=400, K=7, max_del=6, extra_columns=(63, 64, 65), long_columns=0, group=65,
             no_ins=False, contig_len=6000, n_contigs=3, plant=True, p_err=0.12, max_run=3, progress=None, shapes=()):
    """writes ref.fa, reads.fq, aln.paf under out_dir; returns {"reference", "reads", "alignment", "classes": {class: how often planted}}.
    shapes: column strings, or (name, column string) pairs, that are placed as they are, once on either strand, after everything else:
    "shape_reads"[name] = the names of their two reads"""
    rng = random.Random(seed)
    os.makedirs(out_dir, exist_ok=True)
    classes = {}
    note = lambda k: classes.__setitem__(k, classes.get(k, 0) + 1)      # noqa: E731
    contigs = {}
    for c in range(n_contigs):
        n = max(contig_len, long_columns + 200 if c == 0 else 0)
        s = [rng.choice(ACGT) for _ in range(n)]
        for _ in range(3):                                  # N in the reference, away from the ends
            at = rng.randrange(100, n - 100)
            s[at] = "N"
            note("reference_N")
        contigs["ctg%d" % c] = "".join(s)
    shown = {}
    for name, s in contigs.items():                         # lower-case stretches in the file
        at = rng.randrange(0, len(s) - 300)
        shown[name] = s[:at] + s[at:at + 250].lower() + s[at + 250:]
        note("lower_case")
    reads, paf = [], []

    def add_read(name, parts, strand, with_n=True):
        """parts: [(contig, tstart, columns, cigar style)]: the oriented read is flank + part + gap + part + ... + flank"""
        flank = lambda: "".join(rng.choice(ACGT) for _ in range(rng.randrange(0, 12)))      # noqa: E731
        oriented, placed = flank(), []
        for contig, tstart, cols, style in parts:
            target, t, bases = contigs[contig], tstart, []
            for c in cols:
                if c == "=":
                    bases.append(target[t]); t += 1
                elif c == "X":
                    bases.append(rng.choice([b for b in ACGT if b != target[t]])); t += 1
                elif c == "I":
                    bases.append(rng.choice(ACGT))
                else:
                    t += 1
            placed.append((len(oriented), len(bases), contig, tstart, t, cols, style))
            oriented += "".join(bases) + flank()
        oriented = list(oriented)
        if plant and with_n and len(oriented) > 40 and rng.random() < 0.1:
            oriented[rng.randrange(len(oriented))] = "N"
            note("read_N")
        oriented = "".join(oriented)
        quals = [min(93, max(0, int(rng.gauss(20, 9)))) for _ in oriented]
        if plant and rng.random() < 0.05:
            quals[rng.randrange(len(quals))] = rng.choice((0, 93))
        qlen = len(oriented)
        if strand == "-":
            stored, sq = revcomp(oriented), quals[::-1]
        else:
            stored, sq = oriented, quals
        reads.append("@%s some comment\n%s\n+\n%s\n" % (name, stored, "".join(chr(33 + q) for q in sq)))
        note("strand_" + ("minus" if strand == "-" else "plus"))
        for off, n, contig, tstart, tend, cols, style in placed:
            qstart, qend = (off, off + n) if strand == "+" else (qlen - off - n, qlen - off)
            note("ops_M" if style == 0 else "ops_=X")
            paf.append("\t".join([name, str(qlen), str(qstart), str(qend), strand, contig, str(len(contigs[contig])), str(tstart), str(tend),
                                  str(cols.count("=")), str(len(cols)), "60", "tp:A:P", "cg:Z:" + _cigar(cols, style)]))
        if len(placed) > 1:
            note("read_with_several_lines")

    def place(cols, contig=None, at_end=False):
        contig = contig or rng.choice(sorted(contigs))
        m = sum(1 for c in cols if c != "I")
        L = len(contigs[contig])
        return (contig, L - m if at_end else rng.randrange(0, L - m), cols, rng.randrange(2))

    serial = [0]

    def name():
        serial[0] += 1
        return "read%05d" % serial[0]

    for i in range(n_alignments):
        if progress and i % 10000 == 0:
            progress(i)
        add_read(name(), [place(_draw_columns(rng, rng.randrange(col_lo, col_hi + 1), p_err, no_ins, max_run))], "+-"[i % 2])
    for n in extra_columns:
        add_read(name(), [place(_draw_columns(rng, n, no_ins=no_ins))], rng.choice("+-"))
    if long_columns:
        add_read(name(), [place(_draw_columns(rng, long_columns, no_ins=no_ins), contig="ctg0")], "-")
    if group:
        add_read(name(), [place(_draw_columns(rng, 60, no_ins=no_ins)) for _ in range(group)], "+")
    if plant:
        eq = "=" * 12
        cases = {
            "insertion_first_column": "I" + eq * 3, "insertion_last_column": eq * 3 + "I",
            "del_run_max_del": eq + "D" * max_del + eq, "del_run_max_del_plus_1": eq + "D" * (max_del + 1) + eq,
            "alternative_K_plus_4": eq + "IIII" + eq, "alternative_K_plus_5": eq + "IIIII" + eq,
            "alignment_of_K": "=" * K, "alignment_of_K_minus_1": "=" * (K - 1),
            "long_key": eq + "=DDDD" * 8 + eq,
        }
        for what, cols in cases.items():
            if no_ins and "I" in cols:
                continue
            for strand in "+-":
                contig, tstart, cols, style = place(cols)
                # (a planted case is about its columns: keep N out of its reference window)
                while "N" in contigs[contig][tstart:tstart + len(cols)]:
                    contig, tstart, cols, style = place(cols)
                add_read(name(), [(contig, tstart, cols, style)], strand, with_n=False)
                note(what)
        add_read(name(), [place(_draw_columns(rng, 80, no_ins=no_ins), at_end=True)], "+")
        note("ends_at_contig_end")
        add_read(name(), [place(_draw_columns(rng, 70, no_ins=no_ins)), place(_draw_columns(rng, 90, no_ins=no_ins))], "-")
        # lines that are skipped
        first = paf[0].split("\t")
        paf.insert(3, "\t".join(first[:12] + ["tp:A:S", first[13]])); note("tp_A_S")
        paf.insert(5, "\t".join(first[:13])); note("no_cigar")
        paf.insert(7, "\t".join(["nobody"] + first[1:])); note("unknown_read")
        paf.insert(9, "\t".join(first[:5] + ["nowhere"] + first[6:])); note("unknown_target")
        paf.insert(11, "\t".join(first[:13] + ["cg:Z:5S" + first[13][5:]])); note("other_cigar_op")
    shape_reads = {}
    for x, shape in enumerate(shapes):
        what, cols = shape if isinstance(shape, tuple) else ("shape%d" % x, shape)
        for strand in "+-":
            contig, tstart, cols, style = place(cols)
            while "N" in contigs[contig][tstart:tstart + len(cols)]:
                contig, tstart, cols, style = place(cols)
            shape_reads.setdefault(what, []).append("read%05d" % (serial[0] + 1))
            add_read(name(), [(contig, tstart, cols, style)], strand, with_n=False)
            note(what)
    paths = {k: os.path.join(str(out_dir), v) for k, v in (("reference", "ref.fa"), ("reads", "reads.fq"), ("alignment", "aln.paf"))}
    paths["shape_reads"] = shape_reads
    with open(paths["reference"], "w") as f:
        for cname, s in shown.items():
            f.write(">%s generated\n" % cname)
            for a in range(0, len(s), 70):
                f.write(s[a:a + 70] + "\n")
    with open(paths["reads"], "w") as f:
        f.write("".join(reads))
    with open(paths["alignment"], "w") as f:
        f.write("\n".join(paf) + "\n")
    paths["classes"] = classes
    return paths
