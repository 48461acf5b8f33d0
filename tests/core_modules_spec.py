"""Specification of the segment edits of the single-cell route: polyA, tag, scb and flip (TEST INFRASTRUCTURE ONLY).

  * `*_spec`: the transforms with the build's counter-based RNG (Philox keyed by (seed, molecule index, stream, block)), the
    formulas of the HIP kernels (tksm_amd/csrc/mdf_kernels.hip), which reproduce them bit for bit;
  * `*_reference`: the reference's algorithms line by line (src/polyA.cpp:133-148, src/tag.cpp:93-110, src/scb.cpp:73-81,
    src/strand_man.cpp:37-46) with numpy's generator standing in for mt19937 -- for checking distributions.
Molecules are the dicts of oracle/mdf_ops_oracle.py (stream_mdf / write_mdf)."""
import copy
import math

import numpy as np

import mdf_ops_oracle as mo
import pyoracle as po

ST_PLA_LEN, ST_TAG5, ST_TAG3, ST_FLIP = 26, 27, 28, 29
PLA_MAX_ATTEMPTS = 64
GAMMA, POISSON, WEIBULL, NORMAL = "gamma", "poisson", "weibull", "normal"

# fmt2seq's table (src/util.h:62-80), choices in the reference's order
IUPAC = {"A": "A", "G": "G", "T": "T", "C": "C", "U": "U", "R": "GA", "Y": "TC", "K": "GT", "M": "AC", "S": "GC", "W": "AT",
         "B": "GTC", "D": "GAT", "H": "ACT", "V": "GCA", "N": "AGCT"}

_M32 = np.uint64(0xFFFFFFFF)


def philox_np(seed, g, stream, n):
    """po.philox(seed, g, stream, n) over arrays of g (and n): the 4 words as uint64 arrays"""
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


def _u01(w):
    return w.astype(np.float64) * (1.0 / 4294967296.0)


def _u01o(w):                                                      # (0, 1]
    return (w.astype(np.float64) + 1.0) * (1.0 / 4294967296.0)


def _box_muller(a, b):
    return np.sqrt(-2.0 * np.log(_u01o(a))) * np.cos(6.283185307179586 * _u01(b))


# ------------------------------------------------------------------------------------------------ polyA
def polya_draws_spec(seed, g, dist, a, b=0.0):
    """the kernels' draw for molecules g (array): exact samplers of the named distribution"""
    g = np.asarray(g, np.uint64)
    if dist == NORMAL:
        w = philox_np(seed, g, ST_PLA_LEN, 0)
        return a + b * _box_muller(w[0], w[1])
    if dist == WEIBULL:
        w = philox_np(seed, g, ST_PLA_LEN, 0)
        return b * np.power(-np.log(_u01o(w[0])), 1.0 / a)
    out = np.full(g.shape, np.nan)
    todo = np.ones(g.shape, bool)
    if dist == GAMMA:
        al = a + 1.0 if a < 1.0 else a
        d = al - 1.0 / 3.0
        c = 1.0 / math.sqrt(9.0 * d)
        for n in range(PLA_MAX_ATTEMPTS):
            if not todo.any():
                break
            w = philox_np(seed, g, ST_PLA_LEN, n)
            z = _box_muller(w[0], w[1])
            t = 1.0 + c * z
            with np.errstate(invalid="ignore", divide="ignore"):
                v = t * t * t
                acc = todo & (t > 0.0) & (np.log(_u01o(w[2])) < 0.5 * z * z + d - d * v + d * np.log(v))
            x = d * v
            if a < 1.0:
                x = x * np.power(_u01o(w[3]), 1.0 / a)
            out[acc] = x[acc] * b
            todo &= ~acc
        out[todo] = d * b
        return out
    # Poisson: multiplication below 10 (words of blocks 0, 1, ... in order), PTRS above (one block per attempt)
    lam = a
    if lam < 10.0:
        enlam = math.exp(-lam)
        prod = np.ones(g.shape)
        k = np.zeros(g.shape)
        for n in range(PLA_MAX_ATTEMPTS * 4):
            if not todo.any():
                break
            w = philox_np(seed, g, ST_PLA_LEN, n)
            for j in range(4):
                prod = np.where(todo, prod * _u01(w[j]), prod)
                more = todo & (prod > enlam)
                k[more] += 1.0
                done = todo & ~more
                out[done] = k[done]
                todo &= ~done
        out[todo] = k[todo]
        return out
    slam, loglam = math.sqrt(lam), math.log(lam)
    bb = 0.931 + 2.53 * slam
    aa = -0.059 + 0.02483 * bb
    invalpha = 1.1239 + 1.1328 / (bb - 3.4)
    vr = 0.9277 - 3.6224 / (bb - 2.0)
    for n in range(PLA_MAX_ATTEMPTS):
        if not todo.any():
            break
        w = philox_np(seed, g, ST_PLA_LEN, n)
        U, V = _u01(w[0]) - 0.5, _u01(w[1])
        us = 0.5 - np.abs(U)
        k = np.floor((2.0 * aa / us + bb) * U + lam + 0.43)
        quick = todo & (us >= 0.07) & (V <= vr)
        out[quick] = k[quick]
        todo &= ~quick
        cand = todo & ~((k < 0.0) | ((us < 0.013) & (V > us)))
        for i in np.nonzero(cand)[0]:
            lhs = (math.log(V[i]) if V[i] > 0.0 else -math.inf) + math.log(invalpha) - math.log(aa / (us[i] * us[i]) + bb)
            if lhs <= -lam + k[i] * loglam - math.lgamma(k[i] + 1.0):
                out[i] = k[i]
                todo[i] = False
    out[todo] = math.floor(lam)
    return out


def polya_lengths_spec(draws, min_length, max_length):
    """the kernels' clamp: in double first (NaN -> min), then truncation toward zero"""
    v = np.asarray(draws, np.float64)
    out = np.where(v > max_length, float(max_length), v)
    out = np.where(~(v >= min_length), float(min_length), out)
    return np.trunc(out).astype(np.int64)


def _literal(seq):
    return dict(chr=seq, start=0, end=len(seq), plus=True, errors=[])


def polya_spec(mols, seed, dist, a, b=0.0, min_length=0, max_length=5000, first=0):
    lens = polya_lengths_spec(polya_draws_spec(seed, np.arange(first, first + len(mols), dtype=np.uint64), dist, a, b), min_length, max_length)
    out = []
    for md, n in zip(mols, lens):
        md = copy.deepcopy(md)
        if n > 0:
            md["segments"].append(_literal("A" * int(n)))
        out.append(md)
    return out


def polya_reference(mols, dist, a, b, min_length, max_length, rs):
    """add_polyA (src/polyA.cpp:133-148): int poly_a_len = dist(rand_gen) (toward zero), clamped; std:: parameterisations"""
    out, lens = [], []
    for md in mols:
        if dist == GAMMA:
            v = rs.gamma(a, b)
        elif dist == POISSON:
            v = rs.poisson(a)
        elif dist == WEIBULL:
            v = b * rs.weibull(a)
        else:
            v = rs.normal(a, b)
        n = max(min_length, min(max_length, int(v)))
        md = copy.deepcopy(md)
        if n > 0:
            md["segments"].append(_literal("A" * n))
        out.append(md)
        lens.append(n)
    return out, np.array(lens)


# ------------------------------------------------------------------------------------------------ tag
def tag_format(fmt):
    """the CLI's digit rule (src/tag.cpp:84-91: std::stoi), then fmt2seq's letters only (others add nothing)"""
    if fmt and fmt[0].isdigit():
        n = 0
        for ch in fmt:
            if not ch.isdigit():
                break
            n = 10 * n + int(ch)
        fmt = "N" * n
    return "".join(ch for ch in fmt if ch in IUPAC)


def tag_draws_spec(seed, g, stream, fmt):
    """letter j of the (table-only) format = choice umulhi(word j, k): word j = component j % 4 of block j // 4; g: array"""
    g = np.asarray(g, np.uint64)
    cols = []
    w = None
    for j, ch in enumerate(fmt):
        if j % 4 == 0:
            w = philox_np(seed, g, stream, j // 4)
        k = len(IUPAC[ch])
        pick = (w[j % 4] * np.uint64(k)) >> np.uint64(32)
        cols.append(np.frombuffer(IUPAC[ch].encode(), np.uint8)[pick.astype(np.int64)])
    if not cols:
        return [""] * len(g)
    arr = np.stack(cols, 1)
    return [bytes(r).decode() for r in arr]


def tag_spec(mols, seed, format5="", format3="", first=0):
    f5, f3 = tag_format(format5), tag_format(format3)
    g = np.arange(first, first + len(mols), dtype=np.uint64)
    t5, t3 = tag_draws_spec(seed, g, ST_TAG5, f5), tag_draws_spec(seed, g, ST_TAG3, f3)
    out = []
    for md, a, b in zip(mols, t5, t3):
        md = copy.deepcopy(md)
        if a:
            md["segments"].insert(0, _literal(a))
        if b:
            md["segments"].append(_literal(b))
        out.append(md)
    return out


def tag_reference(mols, format5, format3, rs):
    """TAG_module::run (src/tag.cpp:84-110): fmt2seq draws one choice per letter (std::sample of 1)"""
    f5, f3 = tag_format(format5), tag_format(format3)
    out = []
    for md in mols:
        a = "".join(IUPAC[c][rs.randint(len(IUPAC[c]))] for c in f5)
        b = "".join(IUPAC[c][rs.randint(len(IUPAC[c]))] for c in f3)
        md = copy.deepcopy(md)
        if a:
            md["segments"].insert(0, _literal(a))
        if b:
            md["segments"].append(_literal(b))
        out.append(md)
    return out


# ------------------------------------------------------------------------------------------------ scb
def scb_spec(mols, keep_meta_barcodes=False):
    """SingleCellBarcoder_module::run (src/scb.cpp:73-81): no randomness; a molecule without CB raises (meta.at throws)"""
    out = []
    for md in mols:
        if "CB" not in md["meta"]:
            raise KeyError(md["id"])
        md = copy.deepcopy(md)
        bc = md["meta"]["CB"][0]
        if bc != ".":
            md["segments"].append(_literal(bc))
        if not keep_meta_barcodes:
            del md["meta"]["CB"]
        out.append(md)
    return out


scb_reference = scb_spec


# ------------------------------------------------------------------------------------------------ flip
def flip_bits_spec(seed, g, p):
    return _u01(philox_np(seed, np.asarray(g, np.uint64), ST_FLIP, 0)[0]) < p


def flip_spec(mols, seed, p, first=0):
    bits = flip_bits_spec(seed, np.arange(first, first + len(mols), dtype=np.uint64), p)
    return [mo.flip_molecule(copy.deepcopy(md)) if f else copy.deepcopy(md) for md, f in zip(mols, bits)]


def flip_reference(mols, p, rs):
    """strand_flip_transformer (src/strand_man.cpp:37-46): uniform_real_distribution(0, 1) < p"""
    return [mo.flip_molecule(copy.deepcopy(md)) if rs.random_sample() < p else copy.deepcopy(md) for md in mols]


def philox_matches_oracle(cases):
    """philox_np against the C restatement's philox (pyoracle)"""
    for seed, g, st, n in cases:
        w = philox_np(seed, np.array([g], np.uint64), st, n)
        if [int(x[0]) for x in w] != po.philox(seed, g, st, n):
            return False
    return True
