"""random-wgs: whole-genome fragments made on the device (src/random_wgs.cpp), as a C-ABI call, the `tksm random-wgs` module, the
chained `tksm sequence --wgs-*` and Sequencer.wgs.

CPU part: the specification (tests/wgs_spec.py) against scipy (raw length draws) and against the reference's loop restated with numpy's
generator (clipped lengths, molecules per contig, positions, strands); the stop rule, the edges, the id text; the library's exports and
the argument checks of the module and of the chained command.
GPU part (-m gpu): tksmseq_wgs against the specification, text for text; independence of how the candidates are split into calls; a
check that does not go through the specification (--perfect reads are the genome slices their ids name); the module route against the
chained route, byte for byte; the guard against a distribution that never emits."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import wgs_spec as ws

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
KS_GATE = 0.004                          # the flat KS gate of tests/test_core_modules.py for samplers against their named distribution
KS_REF_GATE = 0.02                       # the project's flat gate for comparisons with the reference
N_KS = 300_000
# contigs of very unequal lengths: one shorter than the typical fragment, one of a single base
CONTIGS = [("chrBig", 2_000_000), ("chrMid", 300_000), ("chrSmall", 40_000), ("chrTiny", 3_000), ("chrOne", 1), ("chrEnd", 150_000)]


def _cli(*args, timeout=600, **kw):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout, **kw)


# ------------------------------------------------------------------------------------------------ CPU: specification
@pytest.mark.parametrize("dist,a,b", [(ws.NORMAL, 5000.0, 1500.0), (ws.UNIFORM, 200.0, 9000.0), (ws.LOGNORMAL, 8.0, 0.6),
                                      (ws.EXPONENTIAL, 0.0004, 0.0)])
def test_raw_length_draws_have_the_named_distribution(dist, a, b):
    """std::normal / uniform_real / lognormal / exponential_distribution: one-sample KS on 300 000 draws"""
    from scipy import stats
    d = ws.wgs_draws_spec(77, np.arange(10**6, 10**6 + N_KS, dtype=np.uint64), dist, a, b)
    cdf = {ws.NORMAL: stats.norm(a, b).cdf, ws.UNIFORM: stats.uniform(a, b - a).cdf, ws.LOGNORMAL: stats.lognorm(b, scale=np.exp(a)).cdf,
           ws.EXPONENTIAL: stats.expon(scale=1.0 / a).cdf}[dist]
    D = stats.kstest(d, cdf).statistic
    print(f"{dist}: KS D = {D:.5f}")
    assert D <= KS_GATE


def _summary(idx, ref_pos, fl, plus):
    return {"idx": np.asarray(idx, np.int64), "pos": np.asarray(ref_pos, np.int64), "len": np.asarray(fl, np.int64), "plus": np.asarray(plus, bool)}


def _reference_sample(seed, dist, a, b, base_count):
    m = [r for r in ws.wgs_reference(np.random.RandomState(seed), CONTIGS, dist, a, b, base_count) if r[2] >= 1]     # lengths >= 1 only
    return _summary([r[0] for r in m], [r[1] for r in m], [r[2] for r in m], [r[3] for r in m])


def _spec_sample(seed, dist, a, b, base_count):
    out, c, bases = [], 0, 0
    while bases < base_count:
        idx, ref_pos, fl, minus = ws.wgs_candidates_spec(seed, c, 1 << 16, CONTIGS, dist, a, b)
        em = np.flatnonzero(fl >= 1)
        k = ws.cut_prefix(fl[em], base_count, bases)
        out.append((idx[em[:k]], ref_pos[em[:k]], fl[em[:k]], ~minus[em[:k]]))
        bases += int(fl[em[:k]].sum())
        c += 1 << 16
    return _summary(*[np.concatenate([o[j] for o in out]) for j in range(4)])


def _contingency_p(x, y):
    """chi-square of two count vectors drawn from the same distribution; cells with fewer than 20 counts together are merged"""
    from scipy.stats import chi2_contingency
    x, y = np.asarray(x, float), np.asarray(y, float)
    keep = (x + y) >= 20
    t = np.stack([np.append(x[keep], x[~keep].sum()), np.append(y[keep], y[~keep].sum())])
    t = t[:, t.sum(axis=0) > 0]
    return chi2_contingency(t)[1]


def _same_distribution(A, B, what):
    """the gates of the issue: clipped lengths by two-sample KS (D <= 0.02), molecules per contig and positions in 64 equal bins by
    chi-square, strands binomial (chi2.sf > 1e-3 convention)"""
    from scipy import stats
    starts = np.concatenate([[0], np.cumsum([l for _, l in CONTIGS])[:-1]])
    total = sum(l for _, l in CONTIGS)
    D = stats.ks_2samp(A["len"], B["len"]).statistic
    p_contig = _contingency_p(np.bincount(A["idx"], minlength=len(CONTIGS)), np.bincount(B["idx"], minlength=len(CONTIGS)))
    bins = lambda S: np.bincount(((starts[S["idx"]] + S["pos"]) * 64 // (total + 1)).astype(np.int64), minlength=64)
    p_pos = _contingency_p(bins(A), bins(B))
    p_strand = min(stats.binomtest(int(S["plus"].sum()), len(S["plus"]), 0.5).pvalue for S in (A, B))
    print(f"{what}: n = {len(A['len'])} / {len(B['len'])}, KS D = {D:.5f}, p(contig) = {p_contig:.4f}, p(position) = {p_pos:.4f}, p(strand) = {p_strand:.4f}")
    assert D <= KS_REF_GATE
    assert p_contig > 1e-3 and p_pos > 1e-3 and p_strand > 1e-3


REF_CASES = [(ws.NORMAL, 5000.0, 2500.0), (ws.EXPONENTIAL, 0.0005, 0.0), (ws.LOGNORMAL, 8.0, 0.8), (ws.UNIFORM, 100.0, 8000.0)]
REF_BASES = 250_000_000                   # ~ 60 000 - 120 000 molecules a run: two independent reference runs pass the same gates (below)


@pytest.mark.parametrize("dist,a,b", REF_CASES)
def test_two_runs_of_the_restated_reference_pass_the_gates(dist, a, b):
    """the sample sizes and seeds are such that the reference agrees with itself at these gates"""
    _same_distribution(_reference_sample(101, dist, a, b, REF_BASES), _reference_sample(202, dist, a, b, REF_BASES), f"reference vs reference, {dist}")


@pytest.mark.parametrize("dist,a,b", REF_CASES)
def test_specification_matches_the_restated_reference(dist, a, b):
    """clipped lengths, molecules per contig, positions and strands of the specification against src/random_wgs.cpp:181-207 restated (the
    reference side filtered to lengths >= 1: the one deliberate deviation)"""
    _same_distribution(_spec_sample(42, dist, a, b, REF_BASES), _reference_sample(101, dist, a, b, REF_BASES), f"specification vs reference, {dist}")


def _lengths_of(text):
    return [int(l.split("\t")[2]) - int(l.split("\t")[1]) for l in text.splitlines() if not l.startswith("+")]


@pytest.mark.parametrize("dist,a,b,base_count", [(ws.NORMAL, 5000.0, 2500.0, 1_000_000), (ws.EXPONENTIAL, 0.001, 0.0, 12_345), (ws.UNIFORM, 1.0, 3.0, 7)])
def test_stop_rule_inequalities(dist, a, b, base_count):
    text, st = ws.wgs_spec(5, CONTIGS, dist, a, b, base_count=base_count)
    lens = _lengths_of(text)
    assert st["reached"] and st["molecules"] == len(lens) and st["bases"] == sum(lens)
    assert sum(lens) >= base_count and sum(lens) - lens[-1] < base_count
    assert min(lens) >= 1


def test_nothing_for_a_base_count_that_is_not_positive_and_depth_arithmetic():
    for bc in (0, -5):
        text, st = ws.wgs_spec(5, CONTIGS, ws.NORMAL, 5000.0, 100.0, base_count=bc)
        assert text == "" and st == {"next_candidate": 0, "molecules": 0, "bases": 0, "reached": True}
    total = sum(l for _, l in CONTIGS)
    assert ws.depth_to_base_count(0.37, CONTIGS) == int(0.37 * total) and ws.depth_to_base_count(2, CONTIGS) == 2 * total
    assert ws.depth_to_base_count(1e-9, CONTIGS) == 0


def test_contig_lookup_edges():
    """pos == so_far[i] stays on contig i with ref_pos == len[i] (the reference's off-by-one); a one-base contig is reached by exactly
    one position, at ref_pos 1, where nothing is left of it"""
    lens = [l for _, l in CONTIGS]
    so_far = np.cumsum(lens)
    idx, rp = ws.locate([0, 1, so_far[0] - 1, so_far[0], so_far[0] + 1, so_far[3], so_far[3] + 1, so_far[4] + 1, so_far[-1] - 1], lens)
    assert list(idx) == [0, 0, 0, 0, 1, 3, 4, 5, 5]
    assert list(rp) == [0, 1, lens[0] - 1, lens[0], 1, lens[3], 1, 1, lens[5] - 1]
    # the restated loop computes the same
    for p, i, r in zip([0, so_far[0], so_far[0] + 1, so_far[3] + 1], [0, 0, 1, 4], [0, lens[0], 1, 1]):
        k = 0
        while p > so_far[k]:
            k += 1
        assert (k, p - so_far[k] + lens[k]) == (i, r)
    # nothing of the one-base contig is ever emitted (ref_pos == 1 == its length)
    idx, ref_pos, fl, _ = ws.wgs_candidates_spec(3, 0, 1 << 18, [("a", 5), ("one", 1), ("b", 4)], ws.UNIFORM, 1.0, 4.0)
    assert (idx == 1).any() and (fl[idx == 1] == 0).all() and (ref_pos[idx == 1] == 1).all()
    assert (fl[idx != 1] >= 0).all() and (fl[idx == 0] <= 5 - ref_pos[idx == 0]).all()


def test_huge_and_nan_draws_are_defined():
    assert list(ws.to_int([np.nan, 1e300, -1e300, np.inf, -np.inf, 5.99, -5.99, 2147483646.5])) == [0, 2147483647, -2147483648, 2147483647, -2147483648, 5, -5, 2147483646]
    # exp of a large normal overflows to inf: the clipped length is still the rest of the contig
    idx, ref_pos, fl, _ = ws.wgs_candidates_spec(1, 0, 1000, CONTIGS, ws.LOGNORMAL, 700.0, 50.0)
    lens = np.array([l for _, l in CONTIGS])
    assert ((fl == lens[idx] - ref_pos) | (fl <= 0)).all() and (fl > 0).any()


def test_id_text_and_independence_of_the_split_into_calls():
    text, st = ws.wgs_spec(9, CONTIGS, ws.NORMAL, 4000.0, 3000.0, base_count=3_000_000)
    lines = text.splitlines()
    assert len(lines) == 2 * st["molecules"]
    for k in range(st["molecules"]):
        chrom, start, end, strand, mods = lines[2 * k + 1].split("\t")
        assert lines[2 * k] == f"+{k}_{chrom}:{start}-{end}{strand}\t1\t" and mods == "" and strand in "+-" and int(end) > int(start)
    # the same run in blocks of another size, and as three calls that carry the state
    assert ws.wgs_spec(9, CONTIGS, ws.NORMAL, 4000.0, 3000.0, base_count=3_000_000, block=97)[0] == text
    parts, c, state = [], 0, (0, 0)
    for n in (100, 333, 10**6):
        t, s2 = ws.wgs_spec(9, CONTIGS, ws.NORMAL, 4000.0, 3000.0, base_count=3_000_000, first_candidate=c, n_candidates=n, state=state)
        parts.append(t)
        c, state = s2["next_candidate"], (s2["molecules"], s2["bases"])
    assert "".join(parts) == text and s2 == st


# ------------------------------------------------------------------------------------------------ CPU: exports and argument checks
def test_wgs_symbols_are_exported():
    from tksm_amd import _lib
    lib = _lib.load()
    for s in ("tksmseq_wgs", "tksmseq_random_wgs_main", "tksmseq_reference_declare_contig"):
        assert s in _lib.SYMBOLS and hasattr(lib, s)


def test_random_wgs_argument_checks(tmp_path):
    r = _cli("random-wgs", "--help")
    assert r.returncode == 0 and "random-wgs" in r.stdout
    r = _cli("random-wgs")
    assert r.returncode == 1
    for name in ("reference", "output", "frag-len-dist"):
        assert f"{name} is required!" in r.stderr
    assert "usage: random-wgs" in r.stderr                                    # the help text follows the missing flags
    base = ["random-wgs", "-r", tmp_path / "none.fa", "-o", tmp_path / "o.mdf"]
    r = _cli(*base, "--frag-len-dist", "normal 100 10")
    assert r.returncode == 1 and "Either base-count or depth is required!" in r.stderr
    r = _cli(*base, "--frag-len-dist", "gamma 100 10", "--depth", 1)
    assert r.returncode == 1 and "Invalid fragment length distribution" in r.stderr and "parameters" not in r.stderr
    for bad in ("normal 0 10", "normal -5 10", "normal 100 -1", "uniform 100 50", "exponential", "lognormal nan 1", "normal x"):
        r = _cli(*base, "--frag-len-dist", bad, "--base-count", 100)
        assert r.returncode == 1 and "Invalid fragment length distribution parameters" in r.stderr, bad
    r = _cli(*base, "--frag-len-dist", "normal 100.5 10.25", "--base-count", 100)      # decimals parse; the reference is missing
    assert r.returncode == 1 and "Invalid" not in r.stderr
    assert not (tmp_path / "o.mdf").exists()
    (tmp_path / "dup.fa").write_text(">a\nACGT\n")
    (tmp_path / "dup.fa.fai").write_text("a\t4\t3\t4\t5\na\t4\t11\t4\t5\n")
    r = _cli("random-wgs", "-r", tmp_path / "dup.fa", "-o", tmp_path / "o.mdf", "--frag-len-dist", "normal 3 1", "--base-count", 100)
    assert r.returncode == 1 and "more than once" in r.stderr
    r = _cli("random-wgs", "-r", "x.fa", "-o", "o.mdf", "--frag-len-dist", "normal 3 1", "--depth", 1, "-i", "in.mdf")
    assert r.returncode == 1 and "does not exist" in r.stderr


def test_chained_sequence_argument_checks(tmp_path):
    out = tmp_path / "o.fastq"
    r = _cli("sequence", "-r", "x.fa", "--wgs-frag-len-dist", "normal 100 10", "--wgs-depth", 1, "-i", "in.mdf", "--perfect", out)
    assert r.returncode == 2 and "-i/--input" in r.stderr and "--wgs-" in r.stderr
    r = _cli("sequence", "-r", "x.fa", "--wgs-frag-len-dist", "normal 100 10", "--wgs-depth", 1, "--perfect", out, "--truncate-normal", "100,10")
    assert r.returncode == 2 and "--wgs-*" in r.stderr
    r = _cli("sequence", "-r", "x.fa", "--wgs-frag-len-dist", "normal 100 10", "--wgs-depth", 1, "--perfect", out, "--pcr-cycles", 3)
    assert r.returncode == 2 and "--wgs-*" in r.stderr
    r = _cli("sequence", "-r", "x.fa", "--wgs-frag-len-dist", "normal 100 10", "--perfect", out)
    assert r.returncode == 1 and "Either base-count or depth is required!" in r.stderr
    r = _cli("sequence", "-r", "x.fa", "--wgs-base-count", 100, "--perfect", out)
    assert r.returncode == 1 and "frag-len-dist is required!" in r.stderr
    r = _cli("sequence", "--wgs-frag-len-dist", "normal 100 10", "--wgs-base-count", 100, "--perfect", out)
    assert r.returncode == 1 and "reference is required!" in r.stderr
    r = _cli("sequence", "-r", "x.fa", "--wgs-frag-len-dist", "weibull 100 10", "--wgs-base-count", 100, "--perfect", out)
    assert r.returncode == 1 and "Invalid fragment length distribution" in r.stderr
    r = _cli("sequence", "-r", "x.fa", "--wgs-frag-len-dist", "uniform 100 10", "--wgs-base-count", 100, "--perfect", out)
    assert r.returncode == 1 and "Invalid fragment length distribution parameters" in r.stderr
    r = _cli("sequence", "-r", "x.fa", "--wgs-frag-len-dist", "normal 100 10", "--wgs-base-count", 100, "--wgs-batch-molecules", 0, "--perfect", out)
    assert r.returncode == 2 and "--wgs-batch-molecules" in r.stderr
    # without any --wgs-* option a missing -i is what it was
    r = _cli("sequence", "-r", "x.fa", "--perfect", out)
    assert r.returncode == 2 and "the following arguments are required: -i/--input" in r.stderr
    # the abbreviations the other tests use still resolve
    r = _cli("sequence", "--inp", "missing.mdf", "--perf", out, "--badread-i", "90,99,3")
    assert r.returncode == 1 and "ambiguous" not in r.stderr and "unrecognized" not in r.stderr
    assert not out.exists()
    assert _cli("sequence", "--help").returncode == 0


def test_dispatcher_knows_random_wgs_and_list_is_unchanged():
    r = _cli("list")
    assert r.returncode == 0 and r.stdout == "sequence\npcr\ntruncate\npolyA\ntag\nscb\nflip\n"
    r = _cli("no-such-module")
    assert r.returncode == 1 and "random-wgs" in r.stderr


# ------------------------------------------------------------------------------------------------ GPU
def _genome(seed=11, with_n=False):
    rs = np.random.RandomState(seed)
    ref = {}
    for name, n in CONTIGS:
        b = rs.choice(np.frombuffer(b"ACGT", np.uint8), n)
        if with_n and n > 10_000:
            b[n // 3:n // 3 + 500] = ord("N")
        ref[name] = b.tobytes().decode()
    return ref


def _write_fasta(path, ref, fai=True, width=60):
    off, lines, idx = 0, [], []
    for name, seq in ref.items():
        head = f">{name} test contig\n"
        off += len(head)
        body = "".join(seq[i:i + width] + "\n" for i in range(0, len(seq), width))
        idx.append(f"{name}\t{len(seq)}\t{off}\t{width}\t{width + 1}\n")
        off += len(body)
        lines.append(head + body)
    with open(path, "w") as f:
        f.write("".join(lines))
    if fai:
        with open(str(path) + ".fai", "w") as f:
            f.write("".join(idx))


@pytest.fixture(scope="module")
def declared():
    """a context that knows the contigs by name and length only, as the module does from a .fai"""
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    for name, n in CONTIGS:
        s.declare_contig(name, n)
    yield s
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dist,a,b,stop,start", [
    (ws.NORMAL, 5000.0, 2500.0, ("base_count", 30_000_000), None),
    (ws.UNIFORM, 100.0, 8000.0, ("depth", 7.5), None),
    (ws.LOGNORMAL, 8.0, 0.8, ("base_count", 12_345_678), (1000, 77_001, 3_000_000)),
    (ws.EXPONENTIAL, 0.0005, 0.0, ("depth", 3.25), (5_000_000_000, 4_000_000_123, 1)),
    (ws.EXPONENTIAL, 3.0, 0.0, ("base_count", 500), None),                     # one candidate in twenty emits, one base each
    (ws.NORMAL, 5000.0, 2500.0, ("base_count", 10**15), None),                  # not reached inside the call
])
def test_kernels_match_the_specification(declared, dist, a, b, stop, start):
    """all four distributions, both stop modes, a contig shorter than the typical fragment (and a one-base contig), a starting state
    that is not zero: MDF text and carried state against the specification"""
    base_count = stop[1] if stop[0] == "base_count" else ws.depth_to_base_count(stop[1], CONTIGS)
    first, mols, bases = start if start is not None else (0, 0, 0)
    n = 200_000
    want, st_want = ws.wgs_spec(42, CONTIGS, dist, a, b, base_count=base_count, first_candidate=first, n_candidates=n, state=(mols, bases))
    batch, st = declared.wgs(dist, a, b, seed=42, first_candidate=first, n_candidates=n, state=(mols, bases), **{stop[0]: stop[1]})
    try:
        got = declared.to_mdf_text(batch)
    finally:
        batch.free()
    print(f"{dist}: {st}")
    assert st == st_want
    assert got == want
    assert got.count("\n") == 2 * (st["molecules"] - mols)


@pytest.mark.gpu
def test_one_call_equals_several_calls_with_the_carried_state(declared):
    whole, st_whole = declared.wgs(ws.NORMAL, 3000.0, 2000.0, base_count=40_000_000, seed=7, n_candidates=100_000)
    text = declared.to_mdf_text(whole)
    whole.free()
    assert st_whole["reached"]
    parts, c, state, st = [], 0, (0, 0), None
    for n in (1, 999, 4096, 50_000, 44_904):
        b, st = declared.wgs(ws.NORMAL, 3000.0, 2000.0, base_count=40_000_000, seed=7, first_candidate=c, n_candidates=n, state=state)
        parts.append(declared.to_mdf_text(b))
        b.free()
        c, state = st["next_candidate"], (st["molecules"], st["bases"])
    assert "".join(parts) == text and st == st_whole
    # a call after the run is complete takes nothing
    b, st2 = declared.wgs(ws.NORMAL, 3000.0, 2000.0, base_count=40_000_000, seed=7, first_candidate=c, n_candidates=1000, state=state)
    assert b.n_reads == 0 and st2 == st
    b.free()
    b, st3 = declared.wgs(ws.NORMAL, 3000.0, 2000.0, base_count=0, seed=7, n_candidates=1000)
    assert b.n_reads == 0 and st3 == {"next_candidate": 0, "molecules": 0, "bases": 0, "reached": True}
    b.free()


@pytest.mark.gpu
def test_two_million_candidates_whole_and_in_four_pieces(declared):
    n = 2_000_000
    whole, st_whole = declared.wgs(ws.LOGNORMAL, 7.5, 0.7, base_count=10**14, seed=3, n_candidates=n)
    text = declared.to_mdf_text(whole)
    whole.free()
    assert not st_whole["reached"] and st_whole["next_candidate"] == n
    parts, c, state, st = [], 0, (0, 0), None
    for k in range(4):
        b, st = declared.wgs(ws.LOGNORMAL, 7.5, 0.7, base_count=10**14, seed=3, first_candidate=c, n_candidates=n // 4, state=state)
        parts.append(declared.to_mdf_text(b))
        b.free()
        c, state = st["next_candidate"], (st["molecules"], st["bases"])
    assert st == st_whole
    assert "".join(parts) == text


@pytest.mark.gpu
def test_wgs_errors(declared):
    from tksm_amd.sequence import Sequencer, TksmSeqError
    from tksm_amd import _lib as L
    for dist, a, b in [(ws.NORMAL, 0.0, 1.0), (ws.NORMAL, 10.0, -1.0), (ws.UNIFORM, 10.0, 5.0), (ws.EXPONENTIAL, float("nan"), 0.0), (ws.LOGNORMAL, float("inf"), 1.0)]:
        with pytest.raises(TksmSeqError) as e:
            declared.wgs(dist, a, b, base_count=100)
        assert e.value.code == L.EINVAL
    s = Sequencer(0)
    try:
        with pytest.raises(TksmSeqError) as e:
            s.wgs(ws.NORMAL, 100.0, 10.0, base_count=100)
        assert e.value.code == L.ESTATE
    finally:
        s.close()
    # contigs without bases: sequencing must refuse, not read what is not there
    b, _ = declared.wgs(ws.NORMAL, 100.0, 10.0, base_count=1000)
    try:
        with pytest.raises(TksmSeqError) as e:
            declared.run(b, target="perfect")
        assert e.value.code == L.ESTATE and "without bases" in str(e.value)
    finally:
        b.free()


def _revcomp(s):
    return s.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]


def _check_perfect_fastq(path, ref):
    """every record: the sequence is the genome slice its molecule id names, reverse-complemented for '-'"""
    lines = open(path).read().split("\n")
    n = bases = 0
    for k in range(0, len(lines) - 1, 4):
        rid = lines[k].rsplit("molecule_id=", 1)[1]
        index, rest = rid.split("_", 1)
        chrom, span = rest[:-1].rsplit(":", 1)
        a, b = (int(x) for x in span.split("-"))
        want = ref[chrom][a:b]
        assert int(index) == n and b > a
        assert lines[k + 1] == (want if rid[-1] == "+" else _revcomp(want)), rid
        n += 1
        bases += b - a
    return n, bases


@pytest.mark.gpu
def test_perfect_reads_are_the_genome_slices_their_ids_name(tmp_path):
    ref = _genome(with_n=True)
    _write_fasta(tmp_path / "g.fa", ref)
    out = tmp_path / "p.fastq"
    r = _cli("sequence", "-r", tmp_path / "g.fa", "--wgs-frag-len-dist", "normal 4000 3000", "--wgs-depth", 4, "--perfect", out, "-s", 5,
             "--wgs-batch-molecules", 700)
    assert r.returncode == 0, r.stderr
    n, bases = _check_perfect_fastq(out, ref)
    total = sum(len(v) for v in ref.values())
    assert n > 3 * 700 and 4 * total <= bases < 4 * total + 20_000       # several batches; the stop rule at depth 4


@pytest.mark.gpu
def test_module_route_equals_chained_route(tmp_path):
    """`tksm random-wgs -o x.mdf` then `tksm sequence -i x.mdf` against `tksm sequence --wgs-*`: the same FASTQ byte for byte, perfect and
    Badread with q-scores; the chained output does not change with the batch size, the contexts in flight or the device list; the .fai
    and the FASTA itself give the same MDF"""
    ref = _genome()
    fa = tmp_path / "g.fa"
    _write_fasta(fa, ref)
    dist = "lognormal 6.5 0.5"
    mdf = tmp_path / "x.mdf"
    r = _cli("random-wgs", "-r", fa, "--frag-len-dist", dist, "--depth", 0.4, "-o", mdf, "-s", 21, "--batch-molecules", 500)
    assert r.returncode == 0, r.stderr
    text = open(mdf).read()
    want, st = ws.wgs_spec(21, CONTIGS, ws.LOGNORMAL, 6.5, 0.5, base_count=ws.depth_to_base_count(0.4, CONTIGS))
    assert text == want and st["molecules"] > 1000
    # the batch size, the device list and the way the contig table is found do not matter
    os.makedirs(tmp_path / "nofai")
    _write_fasta(tmp_path / "nofai" / "g.fa", ref, fai=False)
    for extra, fasta in ((["--batch-molecules", 100_000], fa), (["--devices", "0,0", "--batch-molecules", 333], fa), ([], tmp_path / "nofai" / "g.fa")):
        other = tmp_path / "y.mdf"
        r = _cli("random-wgs", "-r", fasta, "--frag-len-dist", dist, "--depth", 0.4, "-o", other, "-s", 21, *extra)
        assert r.returncode == 0, r.stderr
        assert open(other).read() == text, extra
    # --base-count through the module
    r = _cli("random-wgs", "-r", fa, "--frag-len-dist", "uniform 50 900", "--base-count", 200_000, "-o", tmp_path / "u.mdf", "-s", 4)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "u.mdf").read() == ws.wgs_spec(4, CONTIGS, ws.UNIFORM, 50.0, 900.0, base_count=200_000)[0]
    wgs = ["--wgs-frag-len-dist", dist, "--wgs-depth", 0.4]
    for mode in (["--perfect"], ["-o"]):
        via_text, chained = tmp_path / "a.fastq", tmp_path / "b.fastq"
        r = _cli("sequence", "-r", fa, "-i", mdf, *mode, via_text, "-s", 21)
        assert r.returncode == 0, r.stderr
        r = _cli("sequence", "-r", fa, *wgs, *mode, chained, "-s", 21, "--wgs-batch-molecules", 400)
        assert r.returncode == 0, r.stderr
        a = open(via_text, "rb").read()
        assert len(a) > 500_000 and open(chained, "rb").read() == a, mode
        if mode == ["-o"]:
            quals = a.split(b"\n")[3::4]
            assert any(set(q) != {ord("K")} for q in quals[:50])             # q-scores were computed
        for extra in (["--wgs-batch-molecules", 100_000], ["--wgs-batch-molecules", 97, "--in-flight", 1], ["--devices", "0,0", "--wgs-batch-molecules", 250, "--in-flight", 2]):
            r = _cli("sequence", "-r", fa, *wgs, *mode, chained, "-s", 21, *extra)
            assert r.returncode == 0, r.stderr
            assert open(chained, "rb").read() == a, (mode, extra)
    # BGZF made on the device works with the chained route as with -i
    import gzip
    r = _cli("sequence", "-r", fa, *wgs, "--perfect", tmp_path / "c.fastq.gz", "-s", 21, "--gzip", "device")
    assert r.returncode == 0, r.stderr
    r = _cli("sequence", "-r", fa, "-i", mdf, "--perfect", tmp_path / "d.fastq", "-s", 21)
    assert gzip.open(tmp_path / "c.fastq.gz", "rb").read() == open(tmp_path / "d.fastq", "rb").read()


@pytest.mark.gpu
def test_a_distribution_that_never_emits_ends_with_a_message(tmp_path):
    """`exponential 1000`: every draw is below one base.  Both routes stop with exit 1 after a whole batch of candidates without a fragment"""
    ref = _genome()
    fa = tmp_path / "g.fa"
    _write_fasta(fa, ref)
    r = _cli("random-wgs", "-r", fa, "--frag-len-dist", "exponential 1000", "--depth", 1, "-o", tmp_path / "x.mdf", timeout=120)
    assert r.returncode == 1 and "candidate fragments has a base" in r.stderr
    r = _cli("sequence", "-r", fa, "--wgs-frag-len-dist", "exponential 1000", "--wgs-depth", 1, "--perfect", tmp_path / "x.fastq", timeout=120)
    assert r.returncode == 1 and "candidate fragments has a base" in r.stderr
