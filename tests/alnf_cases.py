"""Crafted inputs that drive the fused aligner (k_alnf / aln_fused, csrc/kernels.hip) into its give-up branches: k-mer error
models written as .gz files, literal-sequence molecules that those models wreck, and the ordinary reads that sit beside them in a
batch.  Everything is a pure function of fixed seeds: no GPU, no state.  DESIGN.md ("give-up branches of k_alnf") lists which
branch each case reaches and the counts one MI355X run showed; tests/test_alnf_fallbacks.py asserts them.

The models change LOW-COMPLEXITY k-mers only (at most two distinct bases: homopolymers, dinucleotide repeats) with a heavy hand;
every other k-mer gets a mild substitution.  So a literal made of polyA blocks and short tandem repeats is wrecked while a read from
a random genome beside it in the batch stays ordinary (4.7 % of its 5-mers are low-complexity ones)."""
import gzip

import numpy as np

K = 5
BASES = "ACGT"


def _kmers(k=K):
    for idx in range(4 ** k):
        yield "".join(BASES[(idx >> (2 * (k - 1 - j))) & 3] for j in range(k))


def low_complexity(kmer):
    return len(set(kmer)) <= 2


def _other(b, step=1):
    return BASES[(BASES.index(b) + step) & 3]


def model_lines(kind):
    """the lines of a k = 5 error model: "ins" inserts 2 - 4 bases behind a middle slot of a low-complexity k-mer (a slot then holds
    up to 5 symbols, the most a slot code has room for); "del" deletes the three middle slots, or the middle one."""
    out = []
    for kmer in _kmers():
        mild = kmer[:2] + _other(kmer[2]) + kmer[3:]
        if not low_complexity(kmer):
            out.append(f"{kmer},0.850000;{mild},0.100000;\n")
        elif kind == "ins":
            x, y, z = _other(kmer[2], 1), _other(kmer[1], 2), _other(kmer[3], 3)
            out.append(f"{kmer},0.050000;{kmer[:3] + x * 4 + kmer[3:]},0.450000;{kmer[:2] + y * 3 + kmer[2:]},0.300000;"
                       f"{kmer[:4] + z * 2 + kmer[4:]},0.150000;\n")
        elif kind == "del":
            out.append(f"{kmer},0.050000;{kmer[0] + kmer[4]},0.600000;{kmer[:2] + kmer[3:]},0.300000;\n")
        else:
            raise ValueError(kind)
    return out


def write_model(path, kind):
    with gzip.open(path, "wt") as f:
        f.writelines(model_lines(kind))
    return str(path)


# identity (mean, max, stdev) that goes with each model: low enough that the error loop runs until most low-complexity slots changed
IDENTITY = {"ins": (55.0, 60.0, 1.0), "del": (30.0, 35.0, 1.0)}


def _rand(rs, n):
    return rs.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes().decode()


def literal(rs, kind, length):
    """a literal of about `length` bases.
    "blocks24": random stretches with homopolymer / dinucleotide blocks of 16 - 30 bases: deleted whole, a block moves the window by
                15 .. 31 rows at once (more than the 14-row entries hold, nothing the 64-row pass cannot do);
    "blocks60": blocks of 40 - 90 bases: a window shift above 31 rows;
    "tail":     a random body and a polyA tail of 60 - 120 bases, the shape of tests/golden/unbanded_reads.json;
    "repeat":   nothing but low-complexity blocks: under the insertion model every slot takes 2 - 4 extra bases."""
    lo, hi = {"blocks24": (16, 31), "blocks60": (40, 91), "repeat": (20, 61)}.get(kind, (0, 0))
    if kind == "tail":
        n_tail = int(rs.randint(60, 121))
        return _rand(rs, max(40, length - n_tail)) + "A" * n_tail
    parts, total = [], 0
    while total < length:
        if kind != "repeat":
            parts.append(_rand(rs, int(rs.randint(30, 61))))
            total += len(parts[-1])
        n = int(rs.randint(lo, hi))
        a, b = BASES[rs.randint(4)], BASES[rs.randint(4)]
        parts.append((a * n) if rs.rand() < 0.5 else ((a + b) * n)[:n])
        total += n
    if kind != "repeat":
        parts.append(_rand(rs, 40))
    return "".join(parts)


def genome(seed=11, size=60_000):
    """one random contig, nothing but ACGT (a read with another byte takes the exact kernel from the start: no neighbour at all)"""
    rs = np.random.RandomState(seed)
    return {"chr1": _rand(rs, size)}


def ordinary(rs, ref, i, mean_len=400):
    ln = max(200, int(rs.normal(mean_len, mean_len * 0.15)))
    st = int(rs.randint(0, len(ref["chr1"]) - ln))
    return (f"ord{i}", [("chr1", st, st + ln, "+-"[rs.randint(2)], "")])


# positions of the crafted reads in a batch of n: first, last lane of the first half wave, last lane of the first wave, first lane of
# the second, last read -- those that exist
def crafted_positions(n):
    return sorted({p for p in (0, 31, 63, 64, n - 1) if 0 <= p < n})


def batch(kind, n, seed, length=600, crafted=True, positions=None):
    """n molecules: literals of `kind` at crafted_positions(n) (or `positions`), ordinary reads of the random genome everywhere else.
    crafted=False: the same ordinary reads, with further ordinary reads where the literals were (the neighbours' control run).
    Returns (reference dict, [(molecule id, intervals)], positions)."""
    ref = genome()
    rs_o, rs_l = np.random.RandomState(seed), np.random.RandomState(seed + 1000)
    pos = crafted_positions(n) if positions is None else sorted(positions)
    mols = []
    for i in range(n):
        o = ordinary(rs_o, ref, i)                                # (drawn for every position: the neighbours do not depend on `pos`)
        if i in pos:
            seq = literal(rs_l, kind, length)
            if crafted:
                o = (f"lit{i}", [(seq, 0, len(seq), "+", "")])
            else:
                o = (f"sub{i}", o[1])
        mols.append(o)
    return ref, mols, pos


def mdf_text(mols):
    return "".join(f"+{m}\t1\t\n" + "".join(f"{c}\t{a}\t{b}\t{st}\t{md}\n" for c, a, b, st, md in ivs) for m, ivs in mols)
