"""Specification of random-wgs: whole-genome fragments (TEST INFRASTRUCTURE ONLY).

  * `wgs_spec`: the generator with the build's counter-based RNG (Philox keyed by (seed, candidate index, stream, 0)), the formulas of
    the HIP kernels k_wgs_plan / k_wgs_cut / k_wgs_write (tksm_amd/csrc/mdf_kernels.hip), which reproduce it bit for bit;
  * `wgs_reference`: the reference's loop line by line (src/random_wgs.cpp:181-207) with numpy's generator standing in for mt19937
    -- for checking distributions.
The contig table is a list of (name, length) in order."""
import numpy as np

from core_modules_spec import _box_muller, philox_np

ST_WGS_POS, ST_WGS_LEN, ST_WGS_STRAND = 32, 33, 34
NORMAL, UNIFORM, LOGNORMAL, EXPONENTIAL = "normal", "uniform", "lognormal", "exponential"
_TWO53 = 1.0 / 9007199254740992.0


def _bits53(hi, lo):
    return ((hi << np.uint64(21)) | (lo >> np.uint64(11))).astype(np.float64)


def wgs_draws_spec(seed, g, dist, a, b=0.0):
    """the raw fragment length of candidates g (array), std:: parameterisation: normal(a, b) by Box-Muller, uniform real on [a, b),
    lognormal(a, b) = exp of the normal, exponential(a) = -ln(u) / a"""
    w = philox_np(seed, np.asarray(g, np.uint64), ST_WGS_LEN, 0)
    if dist == UNIFORM:
        return a + (b - a) * (_bits53(w[0], w[1]) * _TWO53)
    if dist == EXPONENTIAL:
        return -np.log((_bits53(w[0], w[1]) + 1.0) * _TWO53) / a
    v = a + b * _box_muller(w[0], w[1])
    if dist == LOGNORMAL:
        with np.errstate(over="ignore"):
            return np.exp(v)
    return v


def to_int(v):
    """double -> int toward zero, clamped to the int range in double first; NaN gives 0"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        c = np.clip(np.where(np.isnan(v), 0.0, v), -2147483648.0, 2147483647.0)
    return np.trunc(c).astype(np.int64)


def _umul64hi(x, m):
    """high 64 bits of x * m (uint64 array x, python int m < 2^64)"""
    x = np.asarray(x, np.uint64)
    m_lo, m_hi = np.uint64(m & 0xFFFFFFFF), np.uint64(m >> 32)
    x_lo, x_hi = x & np.uint64(0xFFFFFFFF), x >> np.uint64(32)
    ll, lh, hl, hh = x_lo * m_lo, x_lo * m_hi, x_hi * m_lo, x_hi * m_hi
    mid = (ll >> np.uint64(32)) + (lh & np.uint64(0xFFFFFFFF)) + (hl & np.uint64(0xFFFFFFFF))
    return hh + (lh >> np.uint64(32)) + (hl >> np.uint64(32)) + (mid >> np.uint64(32))


def locate(pos, lens):
    """contig and offset as the reference computes them (:190-194): the first i with pos <= so_far[i], ref_pos = pos - so_far[i] + len[i]
    (off-by-one included: ref_pos == len[i] occurs)"""
    lens = np.asarray(lens, np.int64)
    so_far = np.cumsum(lens)
    pos = np.asarray(pos, np.int64)
    idx = np.searchsorted(so_far, pos, side="left")
    return idx, pos - so_far[idx] + lens[idx]


def wgs_candidates_spec(seed, first, n, contigs, dist, a, b=0.0):
    """candidates first .. first + n - 1: (contig index, ref_pos, clipped length, minus strand) as arrays; emitted: clipped length >= 1"""
    lens = np.array([l for _, l in contigs], np.int64)
    ref_length = int(lens.sum())
    g = np.arange(first, first + n, dtype=np.uint64)
    wp = philox_np(seed, g, ST_WGS_POS, 0)
    pos = _umul64hi((wp[0] << np.uint64(32)) | wp[1], ref_length)
    idx, ref_pos = locate(pos, lens)
    fl = np.minimum(to_int(wgs_draws_spec(seed, g, dist, a, b)), lens[idx] - ref_pos)
    minus = (philox_np(seed, g, ST_WGS_STRAND, 0)[0] & np.uint64(1)) != 0
    return idx, ref_pos, fl, minus


def cut_prefix(lengths, base_count, bases_before=0):
    """the stop rule (:188, :205) on the lengths of EMITTED candidates in order: how many are taken -- candidates are taken while the
    bases of the emitted candidates before them are below base_count"""
    if base_count <= 0 or bases_before >= base_count:
        return 0
    before = bases_before + np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))[:-1]])
    return int((before < base_count).sum())


def molecules_text(contigs, index0, idx, ref_pos, fl, minus):
    names = [c for c, _ in contigs]
    out = []
    for k in range(len(idx)):
        nm, p, e, s = names[int(idx[k])], int(ref_pos[k]), int(ref_pos[k]) + int(fl[k]), "-" if minus[k] else "+"
        out.append(f"+{index0 + k}_{nm}:{p}-{e}{s}\t1\t\n{nm}\t{p}\t{e}\t{s}\t\n")
    return "".join(out)


def wgs_spec(seed, contigs, dist, a, b=0.0, base_count=0, first_candidate=0, n_candidates=None, state=(0, 0), block=1 << 18):
    """The generator over candidates [first_candidate, first_candidate + n_candidates) (None: until the stop rule is reached) with the
    carried state (molecules, bases) of the run so far.  Returns (MDF text, {"next_candidate", "molecules", "bases", "reached"})."""
    mols, bases = state
    c, end = first_candidate, None if n_candidates is None else first_candidate + n_candidates
    text = []
    reached = base_count <= 0 or bases >= base_count
    while not reached and (end is None or c < end):
        n = block if end is None else min(block, end - c)
        idx, ref_pos, fl, minus = wgs_candidates_spec(seed, c, n, contigs, dist, a, b)
        em = np.flatnonzero(fl >= 1)
        k = cut_prefix(fl[em], base_count, bases)
        tot = int(fl[em[:k]].sum())
        take = em[:k]
        text.append(molecules_text(contigs, mols, idx[take], ref_pos[take], fl[take], minus[take]))
        mols += k
        bases += tot
        if bases >= base_count:
            reached = True
            c += int(take[-1]) + 1
        else:
            c += n
    return "".join(text), {"next_candidate": c, "molecules": mols, "bases": bases, "reached": reached}


def depth_to_base_count(depth, contigs):
    """--depth D (:173-176): base_count = (int64)(D * ref_length)"""
    return int(float(depth) * float(sum(l for _, l in contigs)))


def wgs_reference(rs, contigs, dist, a, b, base_count):
    """src/random_wgs.cpp:181-207 line by line, rs (numpy RandomState) in place of mt19937.  Returns (contig index, ref_pos, frag_len,
    plus strand) per written molecule, empty and inverted intervals included, as the reference writes them."""
    ref_lens = [l for _, l in contigs]
    ref_lens_so_far = list(np.cumsum(ref_lens))
    ref_length = int(ref_lens_so_far[-1])
    draw = {NORMAL: lambda: rs.normal(a, b), UNIFORM: lambda: rs.uniform(a, b), LOGNORMAL: lambda: rs.lognormal(a, b),
            EXPONENTIAL: lambda: rs.exponential(1.0 / a)}[dist]
    out = []
    generated_bases = 0
    while generated_bases < base_count:
        pos = int(rs.randint(0, ref_length))                         # uniform_int_distribution(0, ref_length - 1)
        ref_index = 0
        while pos > ref_lens_so_far[ref_index]:
            ref_index += 1
        ref_pos = pos - ref_lens_so_far[ref_index] + ref_lens[ref_index]
        frag_len = int(to_int(draw()))                               # int frag_len = <double>
        if frag_len > ref_lens[ref_index] - ref_pos:
            frag_len = ref_lens[ref_index] - ref_pos
        plus_strand = int(rs.randint(0, 2)) == 0                     # uniform_int_distribution(0, 1) == 0
        out.append((ref_index, ref_pos, frag_len, plus_strand))
        generated_bases += frag_len
    return out
