"""Specification of tail-noise: random and hairpin (palindromic) noise appended to molecules (TEST INFRASTRUCTURE ONLY).

  * `noise_spec`: the transform with the build's counter-based RNG (Philox keyed by (seed, molecule index, stream, block)), the formulas
    of the HIP kernels k_noise_plan / k_noise_fill / k_pal_count / k_pal_write (tksm_amd/csrc/mdf_kernels.hip), which reproduce it bit
    for bit;
  * `noise_reference`: NoiseAdder::operator() line by line (src/append_noise.cpp:83-128) with numpy's generator standing in for
    mt19937 -- the structure of the hairpin exactly, the draws for checking distributions; `reference_with_deviations` applies the two
    deliberate deviations (a) and (b) of DESIGN.md section 7 to its output.
Molecules are the dicts of oracle/mdf_ops_oracle.py (stream_mdf / write_mdf), taken depth-unrolled."""
import copy
import math

import numpy as np

import mdf_ops_oracle as mo
from core_modules_spec import _box_muller, _u01, philox_np
from wgs_spec import to_int

ST_NOISE_LEN, ST_NOISE_SEQ, ST_NOISE_ERR = 40, 41, 42
NORMAL, LOGNORMAL = "normal", "lognormal"
NOISE_MAX_LEN = 1 << 20


class NoiseLimit(Exception):
    """TKSMSEQ_ELIMIT: random mode drew a length above 2^20; .index is the molecule's position in the batch"""
    def __init__(self, index):
        super().__init__(index)
        self.index = index


def check_params(dist, mu, sigma, error_rate, alphabet):
    """what the library refuses with TKSMSEQ_EINVAL (undefined behaviour, or an exit, in the reference)"""
    if dist not in (NORMAL, LOGNORMAL):
        raise ValueError("Distribution not implemented!")
    if not alphabet:
        raise ValueError("empty alphabet")
    if not math.isfinite(mu) or not math.isfinite(sigma) or not sigma > 0.0:
        raise ValueError("mu must be finite, sigma finite and positive")
    if math.isnan(error_rate):
        raise ValueError("the error rate is not a number")


# ------------------------------------------------------------------------------------------------ length
def noise_draws_spec(seed, g, dist, mu, sigma):
    """the continuous draw of molecules g (array): Box-Muller on block 0 of ST_NOISE_LEN (u1 = (x + 1) / 2^32, u2 = y / 2^32), exp of it
    for the lognormal"""
    w = philox_np(seed, np.asarray(g, np.uint64), ST_NOISE_LEN, 0)
    v = mu + sigma * _box_muller(w[0], w[1])
    if dist == LOGNORMAL:
        with np.errstate(over="ignore"):
            return np.exp(v)
    return v


def noise_lengths_spec(draws):
    """the reference's `int operator()` made defined: clamped in double to the int range (NaN -> 0), toward zero"""
    return to_int(draws)


# ------------------------------------------------------------------------------------------------ random mode
def letters_spec(seed, g, n, alphabet, stream=ST_NOISE_SEQ):
    """n letters of molecule g: letter j = alphabet[umulhi(word j, k)], word j = component j % 4 of block j // 4 (the tag rule)"""
    if n <= 0:
        return ""
    nb = (n + 3) // 4
    w = philox_np(seed, np.full(nb, g, np.uint64), stream, np.arange(nb, dtype=np.uint64))
    words = np.stack(w, 1).reshape(-1)[:n]
    pick = (words * np.uint64(len(alphabet))) >> np.uint64(32)
    return bytes(np.frombuffer(alphabet.encode(), np.uint8)[pick.astype(np.int64)]).decode()


# ------------------------------------------------------------------------------------------------ palindromic mode
def hairpin_segments_spec(md, L):
    """the new segments of a hairpin of nominal length L > 0, before the new substitutions (src/append_noise.cpp:90-107 with deviations
    (a) and (b)): copies from the last segment backwards, strand toggled, until the copied bases are strictly above L; the last copy cut
    by extra = total - L (original on the plus strand: end -= extra; on the minus strand: start += extra), its substitutions re-based to
    the kept range and those outside dropped; a copy cut to nothing is not written"""
    out, total = [], 0
    for s in reversed(md["segments"]):
        size = mo.seg_size(s)
        total += size
        c = dict(chr=s["chr"], start=s["start"], end=s["end"], plus=not s["plus"], errors=list(s["errors"]))
        if total > L:
            extra = total - L
            if s["plus"]:
                c["end"] -= extra
                lo = 0
            else:
                c["start"] += extra
                lo = extra
            c["errors"] = [(p - lo, b) for p, b in s["errors"] if 0 <= p - lo < size - extra]
            if size - extra > 0:
                out.append(c)
            break
        out.append(c)
    return out


def hairpin_draws_spec(seed, g, H, error_rate, alphabet):
    """hairpin bases t = 0 .. H - 1 of molecule g: (hit, letter) arrays.  Components (0, 1) of block t // 2 of ST_NOISE_ERR serve even t,
    (2, 3) odd t: u01(first) < error_rate substitutes alphabet[umulhi(second, k)]"""
    if H <= 0:
        return np.zeros(0, bool), np.zeros(0, np.uint8)
    nb = (H + 1) // 2
    w = philox_np(seed, np.full(nb, g, np.uint64), ST_NOISE_ERR, np.arange(nb, dtype=np.uint64))
    first = np.stack([w[0], w[2]], 1).reshape(-1)[:H]
    second = np.stack([w[1], w[3]], 1).reshape(-1)[:H]
    pick = (second * np.uint64(len(alphabet))) >> np.uint64(32)
    return _u01(first) < error_rate, np.frombuffer(alphabet.encode(), np.uint8)[pick.astype(np.int64)]


def hairpin_spec(md, g, L, seed, error_rate, alphabet):
    """the new segments with their substitutions: per segment the copied ones and the new ones in one list sorted by position (stable:
    copied ones keep their order, a copied one comes before a new one at the same position)"""
    segs = hairpin_segments_spec(md, L)
    H = sum(mo.seg_size(s) for s in segs)
    hit, letter = hairpin_draws_spec(seed, g, H, error_rate, alphabet)
    t0 = 0
    for s in segs:
        n = mo.seg_size(s)
        new = [(int(j), chr(letter[t0 + j])) for j in np.flatnonzero(hit[t0:t0 + n])]
        s["errors"] = sorted(s["errors"] + new, key=lambda e: e[0])
        t0 += n
    return segs


# ------------------------------------------------------------------------------------------------ the transform
def noise_spec(mols, seed, dist, mu, sigma, palindromic=False, error_rate=0.5, alphabet="AGTC", first=0):
    check_params(dist, mu, sigma, error_rate, alphabet)
    g = np.arange(first, first + len(mols), dtype=np.uint64)
    lens = noise_lengths_spec(noise_draws_spec(seed, g, dist, mu, sigma)) if len(mols) else []
    if not palindromic:
        over = [i for i, n in enumerate(lens) if n > NOISE_MAX_LEN]
        if over:
            raise NoiseLimit(over[0])
    out = []
    for i, (md, n) in enumerate(zip(mols, lens)):
        md = copy.deepcopy(md)
        n = int(n)
        if n > 0:
            if palindromic:
                md["segments"] += hairpin_spec(md, first + i, n, seed, error_rate, alphabet)
            else:
                seq = letters_spec(seed, first + i, n, alphabet)
                md["segments"].append(dict(chr=seq, start=0, end=n, plus=True, errors=[]))
        out.append(md)
    return out


# ------------------------------------------------------------------------------------------------ the reference, restated
def noise_reference(mols, dist, mu, sigma, palindromic, error_rate, alphabet, rs, lengths=None):
    """NoiseAdder::operator() (src/append_noise.cpp:83-128), rs (numpy RandomState) in place of mt19937; lengths: given noise lengths
    instead of drawn ones (for comparing structures).  Returns (molecules, noise lengths)."""
    out, lens = [], []
    for i, md in enumerate(mols):
        md = copy.deepcopy(md)
        if lengths is not None:
            noise_length = int(lengths[i])
        else:
            v = rs.normal(mu, sigma) if dist == NORMAL else rs.lognormal(mu, sigma)
            noise_length = int(to_int(v))                                # int noise_length = <double>
        lens.append(noise_length)
        if noise_length <= 0:
            pass
        elif palindromic:
            pal_len_so_far = 0
            new_segments = []
            for it in reversed(md["segments"]):
                pal_len_so_far += it["end"] - it["start"]
                new_segments.append(copy.deepcopy(it))
                new_segments[-1]["plus"] = not new_segments[-1]["plus"]
                if pal_len_so_far > noise_length:
                    extra_len = pal_len_so_far - noise_length
                    if it["plus"]:
                        new_segments[-1]["end"] -= extra_len
                    else:
                        new_segments[-1]["start"] += extra_len
                    new_segments[-1]["_cut"] = (extra_len, it["plus"])     # (bookkeeping for reference_with_deviations; not written)
                    break
            for seg in new_segments:
                for j in range(seg["end"] - seg["start"]):
                    if rs.random_sample() < error_rate:
                        seg["errors"].append((j, alphabet[rs.randint(len(alphabet))]))
                md["segments"].append(seg)
        else:
            seq = "".join(alphabet[rs.randint(len(alphabet))] for _ in range(noise_length))
            md["segments"].append(dict(chr=seq, start=0, end=len(seq), plus=True, errors=[]))
        out.append(md)
    return out, np.array(lens, np.int64)


def reference_with_deviations(mols_ref, n_original):
    """deviations (a) and (b) applied to the output of noise_reference run WITHOUT new substitutions (error_rate 0): the copied
    substitutions of the cut copy re-based to the kept range and filtered, a copy cut to length 0 dropped.  n_original[i]: segments
    molecule i had before."""
    out = []
    for md, n0 in zip(mols_ref, n_original):
        md = copy.deepcopy(md)
        segs = md["segments"][:n0]
        for s in md["segments"][n0:]:
            cut = s.pop("_cut", None)
            if cut is not None:
                extra, was_plus = cut
                lo = 0 if was_plus else extra
                size = s["end"] - s["start"]
                s["errors"] = [(p - lo, b) for p, b in s["errors"] if 0 <= p - lo < size]
                if size <= 0:
                    continue
            segs.append(s)
        md["segments"] = segs
        out.append(md)
    return out
