"""A numpy / plain-Python restatement of `tksm abundance` (include/tksmseq.h, "abundance"), for the tests only: the product must not import it.

It follows the reference's script step by step -- dicts in insertion order, sums left to right in Python floats -- so on the fixtures it
reproduces the files the reference wrote byte for byte; and it states the counter-based cell draws of --cb-count (Philox streams 57 - 60),
which exist nowhere else."""
import gzip
import math

import numpy as np

ST_BC, ST_BC_TXT, ST_WEIGHT, ST_CELL = 57, 58, 59, 60
_M32 = np.uint64(0xFFFFFFFF)
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "K": "GT", "M": "AC", "S": "CG", "W": "AT", "B": "CGT", "D": "AGT", "H": "ACT",
         "V": "ACG", "N": "ACGT"}


def philox_np(seed, g, stream, n):
    """Philox4x32-10 keyed by seed, counter (g low, g high, stream, n): the four words as uint64 arrays over g (and n)"""
    g = np.asarray(g, np.uint64)
    c0, c1 = g & _M32, g >> np.uint64(32)
    c2 = np.broadcast_to(np.uint64(stream), g.shape).copy()
    c3 = np.broadcast_to(np.asarray(n, np.uint64), g.shape).copy()
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _M32, n2, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _open(path):
    return gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)


def parse_paf(path):
    """(transcript names in order of first appearance, {read: [record, ...]} in order of first appearance)"""
    tids, reads = {}, {}
    for no, line in enumerate(open(path), 1):
        f = line.rstrip("\n").split("\t")
        if len(f) < 11:
            raise ValueError(f"PAF line {no}: fewer than 11 columns")
        try:
            rec = {"query_length": int(f[1]), "tid": tids.setdefault(f[5], len(tids)), "target_start": int(f[7]), "num_matches": int(f[9]),
                   "block": int(f[10])}
        except ValueError:
            raise ValueError(f"PAF line {no}: not an integer")
        reads.setdefault(f[0], []).append(rec)
    return list(tids), reads


def compatibility(reads):
    """{surviving read: [(tid, 1 / hits), ...]}; ValueError naming the read where the reference divides by zero"""
    comp = {}
    for rid, recs in reads.items():
        read_length = recs[0]["query_length"]
        best_len, best_m, best_fl = 0, 0, False
        for r in recs:
            fl = r["target_start"] < 20
            if r["num_matches"] > best_m or (r["num_matches"] == best_m and fl):
                best_len, best_m, best_fl = r["block"], r["num_matches"], fl
        if read_length == 0:
            raise ValueError(f"read {rid}: length 0")
        if best_len / float(read_length) < 0.5:
            continue
        if best_m == 0:
            raise ValueError(f"read {rid}: 0 matches")
        hits = [r["tid"] for r in recs if float(r["num_matches"]) / best_m > 0.95 and (r["target_start"] < 20) == best_fl]
        comp[rid] = [(t, 1.0 / len(hits)) for t in hits]
    return comp


def m_step(comp):
    ab, total = {}, 0
    for hits in comp.values():
        for t, w in hits:
            ab[t] = ab.get(t, 0.0) + w
            total += w
    return {t: v / total for t, v in ab.items()}


def e_step(comp, ab):
    for rid, hits in comp.items():
        total = 0
        for t, _ in hits:
            total += ab[t]
        comp[rid] = [(t, ab[t] / total) for t, _ in hits]


def split(comp, cell_of):
    ab, total = {}, 0
    for rid, hits in comp.items():
        for t, w in hits:
            key = (t, cell_of(rid))
            ab[key] = ab.get(key, 0.0) + w
            total += w
    return {k: v / total for k, v in ab.items()}


def rows_of(split_ab, tnames):
    """the rows the writer prints: (name, cell, tpm)"""
    out = []
    for (t, cell), a in split_ab.items():
        tpm = a * 1_000_000
        if tpm < 0.001 or f"{tpm:.3f}" == "0.000":
            continue
        out.append((tnames[t], cell, tpm))
    return out


def tsv_of(rows):
    return "target_id\ttpm\tcell\n" + "".join(f"{n}\t{tpm:.3f}\t{c}\n" for n, c, tpm in rows)


def parse_lr_br(path):
    m = {}
    for line in _open(path):
        rid, _, c, _, bc = line.rstrip("\n").split("\t")
        if c == "1":
            m[rid] = bc
    return m


def barcodes_from_pattern(pattern, count, seed):
    b = np.arange(count, dtype=np.uint64)
    cols = []
    for p, ch in enumerate(pattern):
        letters = np.frombuffer(IUPAC[ch].encode(), np.uint8)
        x = philox_np(seed, b, ST_BC, p)[0]
        cols.append(letters[((x * np.uint64(len(letters))) >> np.uint64(32)).astype(np.int64)])
    return ["".join(chr(c[i]) for c in cols) for i in range(count)]


def barcodes_from_whitelist(lines, count, seed):
    x = philox_np(seed, np.arange(count, dtype=np.uint64), ST_BC_TXT, 0)[0]
    return [lines[int(i)] for i in (x * np.uint64(len(lines))) >> np.uint64(32)]


def cell_cdf(count, seed, mu, sigma, dropout):
    """running sums, left to right, of the count barcode weights and then the dropout entry"""
    x, y, _, _ = philox_np(seed, np.arange(count, dtype=np.uint64), ST_WEIGHT, 0)
    cdf, acc = [], 0.0
    for a, b in zip(x.tolist(), y.tolist()):
        z = math.sqrt(-2.0 * math.log((a + 1.0) * (1.0 / 4294967296.0))) * math.cos(6.283185307179586 * (b * (1.0 / 4294967296.0)))
        acc += 0.0 if dropout >= 1.0 else math.exp(mu + sigma * z)
        cdf.append(acc)
    cdf.append(1.0 if dropout >= 1.0 else acc + acc * dropout / (1.0 - dropout))
    return np.array(cdf)


def draw_cells(n_surviving, seed, cdf):
    """barcode index (len(cdf) - 1: the dropout cell) of the k-th surviving read"""
    u = philox_np(seed, np.arange(n_surviving, dtype=np.uint64), ST_CELL, 0)[0].astype(np.float64) * (1.0 / 4294967296.0)
    return np.minimum(np.searchsorted(cdf, u * cdf[-1], side="right"), len(cdf) - 1)


def run(paf, em_iterations=10, lr_br=None, cb_count=0, cb_lognorm_params=(10.0, 1.0), cb_pattern="NNNNNNNNNNNN", cb_dropout=0.2, cb_txt=None, seed=42):
    tnames, reads = parse_paf(paf)
    comp = compatibility(reads)
    first = {rid: list(h) for rid, h in comp.items()}
    ab = None
    for _ in range(em_iterations):
        ab = m_step(comp)
        e_step(comp, ab)
    if ab is None:
        ab = m_step(comp)
    if cb_count > 0:
        if cb_txt:
            lines = [line.rstrip("\n") for line in _open(cb_txt)]
            assert len(lines) >= cb_count
            barcodes = barcodes_from_whitelist(lines, cb_count, seed)
        else:
            barcodes = barcodes_from_pattern(cb_pattern, cb_count, seed)
        barcodes.append(".")
        cdf = cell_cdf(cb_count, seed, cb_lognorm_params[0], cb_lognorm_params[1], cb_dropout)
        drawn = draw_cells(len(comp), seed, cdf)
        cells = {rid: barcodes[int(k)] for rid, k in zip(comp, drawn)}
        cell_of = cells.__getitem__
        weights = np.diff(np.concatenate([[0.0], cdf]))
    elif lr_br:
        m = parse_lr_br(lr_br)
        cell_of = lambda rid: m.get(rid, ".")      # noqa: E731
        barcodes = weights = None
    else:
        cell_of = lambda rid: "."                  # noqa: E731
        barcodes = weights = None
    rows = rows_of(split(comp, cell_of), tnames)
    vec = np.zeros(len(tnames))
    for t, a in ab.items():
        vec[t] = a
    return {"transcripts": tnames, "reads": list(reads), "kept": [r in comp for r in reads], "surviving": list(comp), "uniform_hits": first, "hits": comp,
            "read_cells": [cell_of(r) for r in comp], "abundance": vec, "rows": rows, "tsv": tsv_of(rows), "barcodes": barcodes, "weights": weights}


# ---- the order of addition (abundance, "The round" and "The split"), restated ------------------------------------------
# `run` above adds left to right, as the reference does.  The device adds in another order, documented as a function of the input alone.
# `ordered_run` performs every addition and division of that document in numpy float64, in that order, so its results can be compared
# with the device's bit for bit.  It is written from the document: chunks of CHUNK positions, WAVE lanes, BLOCK threads.
CHUNK, WAVE, BLOCK = 1024, 64, 256


def _wave_tree(v):
    """v[..., 64] -> what lane 0 holds after the steps 32, 16, 8, 4, 2, 1: at step d, lane l < d adds lane l + d to its own"""
    for d in (32, 16, 8, 4, 2, 1):
        v = v[..., :d] + v[..., d:2 * d]
    return v[..., 0]


def _block_tree(v):
    """v[..., 256] -> the four wave trees, then (0 + 1) + (2 + 3)"""
    w = _wave_tree(v.reshape(v.shape[:-1] + (BLOCK // WAVE, WAVE)))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _strided(x, width):
    """lane l of `width` adds x[l], x[l + width], ... in order, from 0.0; x's last axis is padded with 0.0 (x + 0.0 == x for x >= 0)"""
    rows = max(1, -(-x.shape[-1] // width))
    padded = np.zeros(x.shape[:-1] + (rows * width,))
    padded[..., :x.shape[-1]] = x
    padded = padded.reshape(x.shape[:-1] + (rows, width))
    acc = np.zeros(x.shape[:-1] + (width,))
    for j in range(rows):
        acc = acc + padded[..., j, :]
    return acc


def segment_sums(x, off):
    """x: the weights in segment order; off[segments + 1].  (sum per segment, total): a segment is cut into chunks of CHUNK positions; in
    a chunk lane l adds positions l, l + 64, ... in order, then the wave tree; a segment's chunk partials are added in chunk order; the
    segments' sums fold by blocks of BLOCK (absent segments and the places past the last one count 0.0), and the block results by ONE
    block whose thread t adds parts t, t + 256, ... in order before the same tree"""
    off = np.asarray(off, np.int64)
    n_seg = len(off) - 1
    n_chunks = (np.diff(off) + CHUNK - 1) // CHUNK
    chunk_off = np.concatenate([[0], np.cumsum(n_chunks)])
    chunk_seg = np.repeat(np.arange(n_seg), n_chunks)
    lo = off[chunk_seg] + (np.arange(len(chunk_seg)) - chunk_off[chunk_seg]) * CHUNK
    hi = np.minimum(off[chunk_seg + 1], lo + CHUNK)
    rows = (hi - lo + WAVE - 1) // WAVE
    partial = np.zeros(len(chunk_seg))
    for r in np.unique(rows):                                       # the chunks of r rows of 64 together (most segments are short)
        sel = np.flatnonzero(rows == r)
        at = lo[sel][:, None] + np.arange(r * WAVE)[None, :]
        vals = np.where(at < hi[sel][:, None], x[np.minimum(at, len(x) - 1)], 0.0)
        partial[sel] = _wave_tree(_strided(vals, WAVE))
    sums = np.zeros(n_seg)
    for j in range(int(n_chunks.max()) if n_seg else 0):
        has = np.flatnonzero(n_chunks > j)
        sums[has] = sums[has] + partial[chunk_off[has] + j]
    n_blocks = (n_seg + BLOCK - 1) // BLOCK
    padded = np.zeros(n_blocks * BLOCK)
    padded[:n_seg] = sums
    parts = _block_tree(padded.reshape(n_blocks, BLOCK))
    return sums, float(_block_tree(_strided(parts, BLOCK)))


def _segments(keys):
    """(perm, off, first key of each segment) of a stable sort by key, equal keys forming a segment"""
    perm = np.argsort(keys, kind="stable")
    s = keys[perm]
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    return perm, np.concatenate([start, [len(keys)]]), s[start]


def ordered_run(paf, em_iterations=10, lr_br=None):
    """`run` in the device's documented order of addition: {"abundance", "hit_weights" (flat, surviving reads and their hits in order),
    "uniform_weights", "rows", "tpm"}.  Hits in read and record order; a stable sort by tid; per round the segment sums and their total
    (segment_sums), then per read acc = the sum over its hits, in hit order, of sum[tid] / total and w = (sum[tid] / total) / acc."""
    tnames, reads = parse_paf(paf)
    comp = compatibility(reads)
    T = len(tnames)
    hit_tid = np.array([t for hits in comp.values() for t, _ in hits], np.int64)
    hit_read = np.array([k for k, hits in enumerate(comp.values()) for _ in hits], np.int64)
    w = np.array([x for hits in comp.values() for _, x in hits], np.float64)
    out = {"uniform_weights": w.copy(), "abundance": np.zeros(T), "hit_weights": w, "rows": [], "tpm": np.zeros(0)}
    if not len(w):
        return out
    hit_off = np.concatenate([[0], np.cumsum(np.bincount(hit_read, minlength=len(comp)))])
    nth = np.arange(len(w)) - hit_off[hit_read]                     # a hit's place among its read's hits
    by_place = [np.flatnonzero(nth == j) for j in range(int(nth.max()) + 1)]
    perm = np.argsort(hit_tid, kind="stable")
    off = np.searchsorted(hit_tid[perm], np.arange(T + 1), side="left")
    abundance = None
    for _ in range(em_iterations):
        sums, total = segment_sums(w[perm], off)
        abundance = sums / total
        share = sums[hit_tid] / total
        acc = np.zeros(len(comp))
        for sel in by_place:
            acc[hit_read[sel]] = acc[hit_read[sel]] + share[sel]
        w = share / acc[hit_read]
    # the split: cells are numbered as the reads of the PAF (dropped ones too) first name them, "." is cell 0
    cells, cell_no = ["."], {".": 0}
    named = parse_lr_br(lr_br) if lr_br else {}
    read_cell = {}
    for rid in reads:
        if rid in named:
            read_cell[rid] = cell_no.setdefault(named[rid], len(cell_no))
            if read_cell[rid] == len(cells):
                cells.append(named[rid])
    one_cell = len(cells) == 1
    if one_cell or em_iterations == 0:
        sums, total = segment_sums(w[perm], off)
        if em_iterations == 0:
            abundance = sums / total
        seg_perm, seg_off, seg_key = perm, off, np.arange(T, dtype=np.int64) << 32
    if not one_cell:
        cell = np.array([read_cell.get(rid, 0) for rid in comp], np.int64)
        seg_perm, seg_off, seg_key = _segments((hit_tid << 32) | cell[hit_read])
        sums, total = segment_sums(w[seg_perm], seg_off)
    rows = []
    present = np.flatnonzero(seg_off[1:] > seg_off[:-1])
    for g in present[np.argsort(seg_perm[seg_off[present]], kind="stable")]:      # by the segment's lowest hit index
        tpm = (sums[g] / total) * 1000000.0
        if tpm < 0.001 or f"{tpm:.3f}" == "0.000":
            continue
        rows.append((tnames[int(seg_key[g]) >> 32], cells[int(seg_key[g]) & 0xFFFFFFFF], float(tpm)))
    out.update(abundance=abundance, hit_weights=w, rows=rows, tpm=np.array([t for _, _, t in rows], np.float64))
    return out
