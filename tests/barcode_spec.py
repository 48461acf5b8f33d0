"""The rules of barcode-match (include/tksmseq.h) in plain Python: the (|P| + 1) x (|T| + 1) table, no bit tricks.  `infix` is the
definition; `infix_many` fills the same table for many patterns of one length at once (numpy over the patterns, nothing else changes) and
is checked against `infix` in tests/test_barcode_match.py.  `generate` writes reads and a whitelist with every edge of the rules planted."""
import gzip
import os
import random

import numpy as np

ACGT = "ACGT"
DEFAULT_ADAPTER = "CTACACGACGCTCTTCCGATCT"
DEFAULTS = dict(adapter=DEFAULT_ADAPTER, window=200, max_adapter_errors=5, pad=4, max_errors=2, min_exact=2, revcomp_barcodes=False)
LIST = 8
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    """a byte outside ACGT is its own complement"""
    return "".join(_COMP.get(c, c) for c in reversed(s))


def infix(P, T):
    """(d, e): the minimum Levenshtein distance of P to any substring of T, and the smallest number of consumed letters of T at which it
    is reached.  A letter of T outside ACGT matches nothing."""
    prev = [0] * (len(T) + 1)
    for i in range(1, len(P) + 1):
        cur = [i] + [0] * len(T)
        for j in range(1, len(T) + 1):
            same = P[i - 1] == T[j - 1] and T[j - 1] in ACGT
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if same else 1))
        prev = cur
    d = min(prev)
    return d, prev.index(d)


def infix_many(patterns, T):
    """d of infix(P, T) for every P of `patterns` (all of one length): the same table, one numpy array over the patterns per cell"""
    n, L = len(patterns), len(patterns[0])
    pat = np.array([[ord(c) for c in p] for p in patterns], dtype=np.int32)
    prev = [np.zeros(n, np.int32) for _ in range(len(T) + 1)]
    for i in range(1, L + 1):
        cur = [np.full(n, i, np.int32)]
        for j in range(1, len(T) + 1):
            cost = np.ones(n, np.int32) if T[j - 1] not in ACGT else (pat[:, i - 1] != ord(T[j - 1])).astype(np.int32)
            cur.append(np.minimum(np.minimum(prev[j] + 1, cur[j - 1] + 1), prev[j - 1] + cost))
        prev = cur
    return np.min(np.stack(prev), axis=0)


def _open(path):
    path = str(path)
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path)


def read_fastq(paths):
    """[(name, bases)] over all files in order; ValueError for what the rules refuse"""
    out, seen = [], set()
    for path in paths:
        with _open(path) as f:
            lines = f.read().split("\n")
        i = 0
        while i < len(lines):
            if lines[i].rstrip("\r") == "":
                i += 1
                continue
            rec = [x.rstrip("\r") for x in lines[i:i + 4]]
            if len(rec) < 4:
                raise ValueError("FASTQ: the file ends inside a record")
            i += 4
            if not rec[0].startswith("@") or not rec[2].startswith("+") or len(rec[1]) != len(rec[3]):
                raise ValueError("FASTQ: malformed record")
            if any(not 33 <= ord(c) <= 126 for c in rec[3]):
                raise ValueError("FASTQ: quality out of range")
            name = rec[0][1:].replace("\t", " ").split(" ")[0]
            if name in seen:
                raise ValueError("FASTQ: a read of this name came before")
            seen.add(name)
            out.append((name, "".join(c.upper() if "a" <= c <= "z" else c for c in rec[1])))
    return out


def read_whitelist(path):
    out, lines = [], {}
    with _open(path) as f:
        for no, line in enumerate(f.read().split("\n"), 1):
            line = line.rstrip("\r")
            if not line:
                continue
            if not 4 <= len(line) <= 32 or (out and len(line) != len(out[0])) or any(c not in ACGT for c in line):
                raise ValueError(f"whitelist line {no}: malformed")
            if line in lines:
                raise ValueError(f"whitelist line {no}: the barcode of line {lines[line]} again")
            lines[line] = no
            out.append(line)
    if not out:
        raise ValueError("the whitelist is empty")
    return out


def run(reads, whitelist, **params):
    """reads: a FASTQ path or a list of them; whitelist: a path.  {"matches", "segments", "selected": the files' text, "info": counters}"""
    p = dict(DEFAULTS, **params)
    if p.get("adapter") is None:
        p["adapter"] = DEFAULT_ADAPTER
    adapter, pad = p["adapter"], p["pad"]
    if not isinstance(reads, (list, tuple)):
        reads = [reads]
    if not 4 <= len(adapter) <= 32 or any(c not in ACGT for c in adapter) or p["window"] < len(adapter) or not 0 <= pad <= 16 \
            or not 0 <= p["max_adapter_errors"] < len(adapter) or p["max_errors"] < 0 or p["min_exact"] < 0:
        raise ValueError("a parameter out of range")
    recs = read_fastq(reads)
    if not recs:
        raise ValueError("no reads")
    printed = read_whitelist(whitelist)
    L = len(printed[0])
    if p["max_errors"] >= L:
        raise ValueError("max_errors must be below the barcodes' length")
    matched = [revcomp(b) for b in printed] if p["revcomp_barcodes"] else printed
    index = {b: k for k, b in enumerate(matched)}

    info = dict(reads=len(recs), no_adapter=0, forward=0, reverse=0, whitelist=len(printed), candidates=0, no_barcode=0, unique=0, ambiguous=0, pairs=0)
    segs = []                                        # (name, da, orientation, start, segment)
    for name, bases in recs:
        found = []
        for o in (0, 1):
            T = revcomp(bases) if o else bases
            found.append(infix(adapter, T[:min(p["window"], len(T))]) + (T,))
        o = 0 if found[0][0] <= found[1][0] else 1
        da, ja, T = found[o]
        if da > p["max_adapter_errors"]:
            info["no_adapter"] += 1
            continue
        info["reverse" if o else "forward"] += 1
        start = max(0, ja - pad)
        segs.append((name, da, o, start, T[start:min(len(T), ja + L + pad)]))

    exact = [0] * len(printed)
    for _, _, _, _, seg in segs:
        for k in range(len(seg) - L + 1):
            b = index.get(seg[k:k + L])               # (a window with a byte outside ACGT spells no barcode)
            if b is not None:
                exact[b] += 1
    cand = [b for b in range(len(printed)) if exact[b] >= p["min_exact"]]
    info["candidates"] = len(cand)
    info["pairs"] = len(segs) * len(cand)

    matches = []
    for name, da, _, _, seg in segs:
        d = infix_many([matched[b] for b in cand], seg) if cand else np.zeros(0, np.int32)
        dmin = int(d.min()) if cand else None
        if dmin is None or dmin > p["max_errors"]:
            info["no_barcode"] += 1
            continue
        at = [cand[k] for k in np.nonzero(d == dmin)[0]]
        info["unique" if len(at) == 1 else "ambiguous"] += 1
        matches.append(f"{name}\t{dmin}\t{len(at)}\t{da}\t{','.join(printed[b] for b in at[:LIST])}\n")
    return {"matches": "".join(matches),
            "segments": "".join(f"{n}\t{da}\t{'-' if o else '+'}\t{start}\t{seg}\n" for n, da, o, start, seg in segs),
            "selected": "".join(f"{printed[b]}\t{exact[b]}\n" for b in cand),
            "info": info}


# ---- the generator -------------------------------------------------------------------------------------------------------------------------------
def _rand(rs, n):
    return "".join(rs.choice(ACGT) for _ in range(n))


def _other(rs, c):
    return rs.choice([x for x in ACGT if x != c])


def _substitute(rs, s, positions):
    s = list(s)
    for k in positions:
        s[k] = _other(rs, s[k])
    return "".join(s)


def _spread(n, length):
    """n positions spread over [1, length - 1): substitutions that no shorter edit script replaces"""
    return [1 + (k * (length - 2)) // n for k in range(n)]


def generate(d, seed, L=16, n_barcodes=60, n_seen=40, read_len=(100, 600), gz=False, **params):
    """Writes d/reads.fq[.gz] and d/whitelist.txt[.gz] for the given parameters (DEFAULTS otherwise) and returns their paths with
    `classes`: class name -> the names of the reads (or the barcodes) planted for it.  Every candidate barcode is carried exactly by two
    plain reads, one of them reverse-complemented; what the classes promise is checked from the specification's output by the tests."""
    p = dict(DEFAULTS, **params)
    rs = random.Random(seed)
    adapter, window, pad, m = p["adapter"], p["window"], p["pad"], len(p["adapter"])
    mae, me, mx = p["max_adapter_errors"], p["max_errors"], max(p["min_exact"], 1)
    classes, reads = {}, []
    wl = []
    while len(wl) < n_barcodes:                      # random barcodes, none a homopolymer
        b = _rand(rs, L)
        if b not in wl and len(set(b)) > 1:
            wl.append(b)
    homo = "A" * L
    while True:
        base = _rand(rs, L)                           # its one-substitution variants are in the whitelist, it is not
        variants = []
        for k in range(10):
            pos, c = k % L, ACGT[(ACGT.index(base[k % L]) + 1 + k // L) % 4]
            variants.append(base[:pos] + c + base[pos + 1:])
        tie = _rand(rs, L)
        tie_pair = [tie[:L // 2] + c + tie[L // 2 + 1:] for c in ACGT if c != tie[L // 2]][:2]
        once, never = _rand(rs, L), _rand(rs, L)
        specials = [homo] + variants + tie_pair + [once, never]
        if len(set(specials + [base, tie])) == len(specials) + 2:
            break
    wl = [b for b in wl if b not in specials and b not in (base, tie)]
    # the specials go between the random ones, so that whitelist order is not planting order
    for k, b in enumerate(specials):
        wl.insert((k * 7) % (len(wl) + 1), b)
    spelled = (lambda b: revcomp(b)) if p["revcomp_barcodes"] else (lambda b: b)

    def add(cls, body_forward, reverse=False, lower=False):
        name = f"r{len(reads)}_{cls}"
        s = revcomp(body_forward) if reverse else body_forward
        reads.append((name, s.lower() if lower else s))
        classes.setdefault(cls, []).append(name)
        return name

    def tail():
        return _rand(rs, rs.randint(max(read_len[0] - 60, 20), max(read_len[1] - 260, 40)))

    def plain(b, prefix=None, ad=None, after=None):
        """prefix + adapter + the barcode as it is matched + what follows"""
        if prefix is None:
            prefix = rs.randint(0, max(0, min(40, window - m)))
        return _rand(rs, prefix) + (adapter if ad is None else ad) + spelled(b) + (tail() if after is None else after)

    seen = [b for b in wl if b not in (once, never) and b not in variants and b not in tie_pair and b != homo][:n_seen]
    for b in seen + variants + tie_pair:
        for k in range(mx):
            add("reverse" if k % 2 else "forward", plain(b), reverse=bool(k % 2))
    classes["exact_at_min"] = list(seen[:1])
    add("forward", plain(once))                       # one exact window only: below min_exact when that is 2 or more
    classes["exact_below_min"] = [once]
    classes["never_seen"] = [never]
    # homopolymer: L + 2 equal letters give three windows in one segment
    add("homopolymer", plain(homo, after="AA" + tail()))
    add("homopolymer", plain(homo, after="AA" + tail()), reverse=True)
    b = seen[1 % len(seen)]
    # ---- adapter
    add("adapter_at_max", plain(b, ad=_substitute(rs, adapter, _spread(mae, m)))) if mae else None
    add("adapter_over_max", plain(b, ad=_substitute(rs, adapter, _spread(mae + 1, m)))) if mae + 1 <= m - 2 else None
    add("adapter_ends_at_window", plain(b, prefix=window - m))
    add("adapter_ends_past_window", plain(b, prefix=window - m + 1))
    add("adapter_both_ends", plain(b, prefix=3, after=tail() + revcomp(_rand(rs, 3) + adapter + spelled(seen[2 % len(seen)]))))
    add("shorter_than_adapter", adapter[:m - 2][:10])
    add("ends_inside_barcode", plain(b, after="")[:-(L // 2)])
    add("ends_after_barcode", plain(b, after=""))
    add("adapter_with_n", plain(b, ad=adapter[:m // 2] + "N" + adapter[m // 2 + 1:]))
    # ---- barcode errors (the barcode as matched, edited)
    sb = spelled(b)
    pre = _rand(rs, 12) + adapter
    add("barcode_substitution", pre + _substitute(rs, sb, [L // 2]) + tail())
    add("barcode_insertion", pre + sb[:L // 2] + _other(rs, sb[L // 2]) + sb[L // 2:] + tail(), reverse=True)
    add("barcode_deletion", pre + sb[:L // 2] + sb[L // 2 + 1:] + tail())
    add("barcode_at_max_errors", pre + _substitute(rs, sb, _spread(me, L)) + tail()) if me else None
    add("barcode_over_max_errors", pre + _substitute(rs, sb, _spread(me + 1, L)) + tail(), reverse=True) if me + 1 <= L - 2 else None
    add("barcode_with_n", pre + sb[:L // 2] + "N" + sb[L // 2 + 1:] + tail())
    add("lower_case", plain(b), lower=True)
    # ---- ties
    add("two_tied", pre + spelled(tie) + tail())
    add("more_than_eight_tied", pre + spelled(base) + tail(), reverse=True)
    add("no_adapter", _rand(rs, 300))

    ext = ".gz" if gz else ""
    out = {"reads": os.path.join(str(d), "reads.fq" + ext), "whitelist": os.path.join(str(d), "whitelist.txt" + ext), "classes": classes,
           "barcodes": wl, "params": p, "L": L, "n_reads": len(reads)}
    opener = (lambda path: gzip.open(path, "wt")) if gz else (lambda path: open(path, "w"))
    with opener(out["reads"]) as f:
        for k, (name, s) in enumerate(reads):
            f.write(f"@{name} planted read {k}\n{s}\n+\n{'I' * len(s)}\n")
    with opener(out["whitelist"]) as f:
        f.write("\n".join(wl) + "\n")
    return out
