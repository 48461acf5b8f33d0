"""tail-noise: random and hairpin (palindromic) noise appended on the device (src/append_noise.cpp), as a C-ABI call, the
`tksm tail-noise` module and Sequencer.append_noise.

CPU part: the specification (tests/noise_spec.py) against scipy (continuous length draws) and against NoiseAdder::operator() restated with
numpy's generator (integer lengths, letter frequencies, the structure of the hairpin, substitutions per hairpin); the edges; the library's
exports and the module's argument checks.
GPU part (-m gpu): tksmseq_append_noise against the specification, text for text; independence of batching; a check that does not go
through the specification (--perfect reads: the molecule followed by its reverse complement; by letters of the alphabet); the module
route; the errors."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import mdf_ops_oracle as mo
import noise_spec as ns

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
KS_GATE = 0.004                          # the project's flat KS gate for samplers against their named distribution
KS_REF_GATE = 0.02                       # the project's flat gate for comparisons with the reference
N_KS = 300_000


def _cli(*args, timeout=600, **kw):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout, **kw)


# ------------------------------------------------------------------------------------------------ CPU: lengths
@pytest.mark.parametrize("dist,mu,sigma", [(ns.NORMAL, 500.0, 150.0), (ns.NORMAL, -3.0, 0.5), (ns.LOGNORMAL, 4.0, 0.7), (ns.LOGNORMAL, 0.0, 1.5)])
def test_continuous_length_draws_have_the_named_distribution(dist, mu, sigma):
    """std::normal_distribution / lognormal_distribution: one-sample KS on 300 000 draws"""
    from scipy import stats
    d = ns.noise_draws_spec(77, np.arange(10**6, 10**6 + N_KS, dtype=np.uint64), dist, mu, sigma)
    cdf = stats.norm(mu, sigma).cdf if dist == ns.NORMAL else stats.lognorm(sigma, scale=np.exp(mu)).cdf
    D = stats.kstest(d, cdf).statistic
    print(f"{dist},{mu},{sigma}: KS D = {D:.5f}")
    assert D <= KS_GATE


LEN_CASES = [(ns.NORMAL, 50.0, 10.0), (ns.NORMAL, 2.0, 3.0), (ns.LOGNORMAL, 5.0, 0.8)]
_ONE = [dict(id="m", depth=1, meta={}, segments=[dict(chr="c", start=0, end=10, plus=True, errors=[])])]


_REF_LENGTHS = {}


def _reference_lengths(seed, dist, mu, sigma, n=N_KS):
    """noise lengths of the restated reference, molecule by molecule (molecules without segments: the length is the only draw)"""
    key = (seed, dist, mu, sigma, n)
    if key not in _REF_LENGTHS:
        empty = [dict(id="m", depth=1, meta={}, segments=[])] * n
        _REF_LENGTHS[key] = ns.noise_reference(empty, dist, mu, sigma, True, 0.5, "AGTC", np.random.RandomState(seed))[1]
    return _REF_LENGTHS[key]


@pytest.mark.parametrize("dist,mu,sigma", LEN_CASES)
def test_two_seeds_of_the_restated_reference_pass_the_length_gate(dist, mu, sigma):
    """the sample size suffices: the reference agrees with itself at the gate"""
    from scipy import stats
    D = stats.ks_2samp(_reference_lengths(101, dist, mu, sigma), _reference_lengths(202, dist, mu, sigma)).statistic
    print(f"reference vs reference {dist},{mu},{sigma}: KS D = {D:.5f}")
    assert D <= KS_REF_GATE


@pytest.mark.parametrize("dist,mu,sigma", LEN_CASES)
def test_integer_lengths_match_the_restated_reference(dist, mu, sigma):
    from scipy import stats
    got = ns.noise_lengths_spec(ns.noise_draws_spec(42, np.arange(N_KS, dtype=np.uint64), dist, mu, sigma))
    D = stats.ks_2samp(got, _reference_lengths(101, dist, mu, sigma)).statistic
    print(f"specification vs reference {dist},{mu},{sigma}: KS D = {D:.5f}")
    assert D <= KS_REF_GATE


def test_nan_and_huge_draws_are_defined():
    assert list(ns.noise_lengths_spec([np.nan, 1e300, -1e300, np.inf, -np.inf, 4.99, -4.99, 0.5, 2147483647.5])) == \
        [0, 2147483647, -2147483648, 2147483647, -2147483648, 4, -4, 0, 2147483647]


# ------------------------------------------------------------------------------------------------ CPU: random mode
def _chi2_p(obs, expected):
    from scipy.stats import chisquare
    return chisquare(obs, expected).pvalue


def test_letter_frequencies_follow_the_repeats_of_the_alphabet():
    """--alphabet AAAGTC: A : G : T : C = 3 : 1 : 1 : 1, for the specification and for the restated reference"""
    alphabet = "AAAGTC"
    mols = [dict(id=f"m{i}", depth=1, meta={}, segments=[dict(chr="c", start=0, end=5, plus=True, errors=[])]) for i in range(4000)]
    spec = ns.noise_spec(mols, 3, ns.NORMAL, 50.0, 10.0, alphabet=alphabet)
    ref, _ = ns.noise_reference(mols, ns.NORMAL, 50.0, 10.0, False, 0.5, alphabet, np.random.RandomState(9))
    for name, out in (("specification", spec), ("reference", ref)):
        text = "".join(m["segments"][-1]["chr"] for m in out if len(m["segments"]) == 2)
        assert all(m["segments"][-1]["plus"] and m["segments"][-1]["start"] == 0 and m["segments"][-1]["end"] == len(m["segments"][-1]["chr"])
                   for m in out if len(m["segments"]) == 2)
        obs = np.array([text.count(c) for c in "AGTC"], float)
        assert obs.sum() == len(text) > 150_000
        p = _chi2_p(obs, obs.sum() * np.array([3, 1, 1, 1]) / 6.0)
        print(f"{name}: {obs}, p = {p:.4f}")
        assert p > 1e-3
    # letters depend on (seed, g) only, and a longer literal of the same molecule extends a shorter one
    assert ns.letters_spec(3, 17, 9, "AGTC") == ns.letters_spec(3, 17, 40, "AGTC")[:9]
    assert ns.letters_spec(3, 17, 40, "AGTC") != ns.letters_spec(3, 18, 40, "AGTC")


# ------------------------------------------------------------------------------------------------ CPU: palindromic structure
def _seg(chr_, start, end, plus, errors=()):
    return dict(chr=chr_, start=start, end=end, plus=plus, errors=list(errors))


STRUCT_CORPUS = [
    # single segment, plus and minus, with substitutions on both sides of every cut
    dict(id="one_plus", depth=1, meta={}, segments=[_seg("chr1", 100, 200, True, [(0, "A"), (49, "C"), (50, "G"), (99, "T")])]),
    dict(id="one_minus", depth=1, meta={}, segments=[_seg("chr1", 100, 200, False, [(99, "T"), (0, "A"), (50, "G"), (49, "C")])]),
    # several segments, mixed strands, a literal in the middle and at the end
    dict(id="multi", depth=1, meta={"x": ["1"]}, segments=[_seg("chr1", 10, 70, True, [(5, "A")]), _seg("ACGTACGTAC", 0, 10, True, [(3, "T")]),
                                                            _seg("chr2", 500, 530, False, [(29, "C"), (0, "G"), (15, "A")]), _seg("AAAAAAAA", 0, 8, False, [(0, "C")])]),
    dict(id="two", depth=1, meta={}, segments=[_seg("chr2", 0, 40, False, [(39, "A"), (20, "C")]), _seg("chr1", 7, 27, True, [(19, "G"), (0, "T")])]),
]
# multi: sizes 60, 10, 30, 8 -> partial sums from the end 8, 38, 48, 108; two: 20, 60; one_*: 100
STRUCT_LENGTHS = {"one_plus": [1, 50, 99, 100, 101, 5000], "one_minus": [1, 50, 99, 100, 101, 5000],
                  "multi": [1, 7, 8, 9, 23, 38, 39, 47, 48, 49, 107, 108, 109, 100000], "two": [5, 19, 20, 21, 59, 60, 61]}


def test_hairpin_structure_equals_the_restated_reference():
    """for given lengths the new segments (before new substitutions) are the reference's, deviations (a) and (b) applied to its side:
    single and multi-segment molecules, minus strands, literals, existing substitutions, L equal to a partial sum of the segment sizes,
    to the whole molecule, and beyond it"""
    cases = 0
    for md in STRUCT_CORPUS:
        sizes = [mo.seg_size(s) for s in md["segments"]]
        partial = set(np.cumsum(sizes[::-1]).tolist())
        assert partial & set(STRUCT_LENGTHS[md["id"]]) and sum(sizes) in STRUCT_LENGTHS[md["id"]] and max(STRUCT_LENGTHS[md["id"]]) > sum(sizes)
        for L in STRUCT_LENGTHS[md["id"]]:
            ref, lens = ns.noise_reference([md], ns.NORMAL, 0.0, 1.0, True, 0.0, "AGTC", np.random.RandomState(1), lengths=[L])
            assert lens[0] == L
            want = ns.reference_with_deviations(ref, [len(md["segments"])])[0]["segments"][len(md["segments"]):]
            got = ns.hairpin_segments_spec(md, L)
            assert got == want, (md["id"], L)
            assert sum(mo.seg_size(s) for s in got) == min(L, sum(sizes)), (md["id"], L)
            for s in got:
                assert mo.seg_size(s) > 0 and all(0 <= p < mo.seg_size(s) for p, _ in s["errors"]), (md["id"], L)
            cases += 1
    assert cases == 33
    # the cut rule, spelled out: a total that equals L does not stop the walk, the next copy is cut to nothing (and not written)
    multi = STRUCT_CORPUS[2]
    got = ns.hairpin_segments_spec(multi, 38)
    assert [(s["chr"], s["start"], s["end"], s["plus"]) for s in got] == [("AAAAAAAA", 0, 8, True), ("chr2", 500, 530, True)]
    got = ns.hairpin_segments_spec(multi, 39)
    assert [(s["chr"], s["start"], s["end"], s["plus"], s["errors"]) for s in got][2] == ("ACGTACGTAC", 0, 1, False, [])
    # original on the minus strand: start += extra, substitutions re-based
    got = ns.hairpin_segments_spec(multi, 23)
    assert (got[1]["start"], got[1]["end"], got[1]["plus"], got[1]["errors"]) == (515, 530, True, [(14, "C"), (0, "A")])


@pytest.mark.parametrize("rate", [0.0, 0.1, 0.5, 1.0])
def test_new_substitutions_per_hairpin_are_binomial(rate):
    """new substitutions of a hairpin ~ Binomial(H, error_rate); positions strictly inside their segment and sorted within it; letters
    of the alphabet"""
    from scipy import stats
    rs = np.random.RandomState(12)
    mols = []
    for i in range(1500):
        segs = []
        for _ in range(int(rs.randint(1, 5))):
            ln = int(rs.randint(1, 300))
            st = int(rs.randint(0, 50_000))
            segs.append(_seg(f"chr{int(rs.randint(1, 3))}", st, st + ln, bool(rs.randint(0, 2))))
        mols.append(dict(id=f"m{i}", depth=1, meta={}, segments=segs))
    out = ns.noise_spec(mols, 8, ns.NORMAL, 250.0, 150.0, palindromic=True, error_rate=rate, alphabet="AGTC", first=1000)
    lens = ns.noise_lengths_spec(ns.noise_draws_spec(8, np.arange(1000, 2500, dtype=np.uint64), ns.NORMAL, 250.0, 150.0))
    tot_h = tot_new = 0
    z = []
    for md, o, L in zip(mols, out, lens):
        new = o["segments"][len(md["segments"]):]
        H = sum(mo.seg_size(s) for s in new)
        assert H == max(0, min(int(L), mo.mol_size(md)))
        k = sum(len(s["errors"]) for s in new)
        for s in new:
            pos = [p for p, _ in s["errors"]]
            assert pos == sorted(pos) and len(set(pos)) == len(pos) and all(0 <= p < mo.seg_size(s) for p in pos)
            assert all(b in "AGTC" for _, b in s["errors"])
        if rate in (0.0, 1.0):
            assert k == int(rate * H)
        elif H >= 30:
            z.append((k - H * rate) / np.sqrt(H * rate * (1 - rate)))
        tot_h += H
        tot_new += k
    assert tot_h > 100_000
    if 0.0 < rate < 1.0:
        p = stats.binomtest(tot_new, tot_h, rate).pvalue
        # the counts of the single hairpins scatter as binomials do (not, say, all alike): sum of squared standard scores ~ chi2(n)
        q = stats.chi2(len(z)).cdf(float(np.sum(np.square(z))))
        print(f"rate {rate}: {tot_new} of {tot_h}, p = {p:.4f}; dispersion over {len(z)} hairpins: chi2 cdf = {q:.4f}")
        assert p > 1e-3
        assert 1e-3 < q < 1 - 1e-3


def test_restated_reference_draws_binomial_substitutions_too():
    from scipy import stats
    mols = [dict(id=f"m{i}", depth=1, meta={}, segments=[_seg("chr1", 0, 150, True), _seg("chr1", 300, 450, False)]) for i in range(400)]
    ref, lens = ns.noise_reference(mols, ns.NORMAL, 200.0, 50.0, True, 0.3, "AGTC", np.random.RandomState(4))
    tot_h = sum(min(max(int(L), 0), 300) for L in lens)
    tot_new = sum(len(s["errors"]) for md in ref for s in md["segments"][2:])
    assert stats.binomtest(tot_new, tot_h, 0.3).pvalue > 1e-3


# ------------------------------------------------------------------------------------------------ CPU: edges
def _mdf(rs, n, depth=True):
    """molecules with depth > 1, literal and minus-strand segments, substitutions (unsorted too) and comments"""
    lines = []
    for i in range(n):
        d = 1 if (not depth or rs.rand() < 0.8) else int(rs.randint(2, 4))
        cm = ["tid=ENST7;", "z;a=1,2;", ""][int(rs.randint(0, 3))]
        lines.append(f"+mol{i}\t{d}\t{cm}\n")
        for _ in range(int(rs.randint(1, 7))):
            ln = int(rs.randint(1, 400))
            st = int(rs.randint(0, 59_000))
            md = ",".join(f"{int(rs.randint(0, ln))}{'ACGT'[int(rs.randint(0, 4))]}" for _ in range(int(rs.randint(0, 4))))
            lines.append(f"chr{int(rs.randint(1, 3))}\t{st}\t{st + ln}\t{'+-'[int(rs.randint(0, 2))]}\t{md}\n")
        if rs.rand() < 0.3:
            pa = "".join("ACGT"[int(x)] for x in rs.randint(0, 4, int(rs.randint(1, 30))))
            lines.append(f"{pa}\t0\t{len(pa)}\t{'+-'[int(rs.randint(0, 2))]}\t0C\n")
    return "".join(lines)


def test_non_positive_lengths_leave_the_molecule_text_unchanged():
    text = _mdf(np.random.RandomState(3), 300)
    mols = mo.stream_mdf(text, unroll=True)
    for pal in (False, True):
        out = ns.noise_spec(mols, 5, ns.NORMAL, -50.0, 10.0, palindromic=pal)
        assert mo.write_mdf(out) == mo.write_mdf(mols)
        # mu = 0: about half the molecules draw L <= 0 and are unchanged, the others grow
        out = ns.noise_spec(mols, 5, ns.NORMAL, 0.0, 30.0, palindromic=pal)
        lens = ns.noise_lengths_spec(ns.noise_draws_spec(5, np.arange(len(mols), dtype=np.uint64), ns.NORMAL, 0.0, 30.0))
        same = [mo.write_mdf([a]) == mo.write_mdf([b]) for a, b in zip(mols, out)]
        assert same == [bool(L <= 0) for L in lens] and 0.3 < np.mean(same) < 0.7


def test_results_do_not_depend_on_the_batch_split_or_on_first():
    text = _mdf(np.random.RandomState(4), 400)
    mols = mo.stream_mdf(text, unroll=True)
    for pal in (False, True):
        whole = ns.noise_spec(mols, 6, ns.LOGNORMAL, 4.0, 0.8, palindromic=pal, first=90)
        k = len(mols) // 3
        parts = ns.noise_spec(mols[:k], 6, ns.LOGNORMAL, 4.0, 0.8, palindromic=pal, first=90) + \
            ns.noise_spec(mols[k:], 6, ns.LOGNORMAL, 4.0, 0.8, palindromic=pal, first=90 + k)
        assert mo.write_mdf(parts) == mo.write_mdf(whole)
        assert mo.write_mdf(ns.noise_spec(mols, 6, ns.LOGNORMAL, 4.0, 0.8, palindromic=pal, first=91)) != mo.write_mdf(whole)


def test_refused_parameters():
    for bad in (dict(alphabet=""), dict(mu=float("nan")), dict(mu=float("inf")), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("inf")),
                dict(error_rate=float("nan")), dict(dist="gamma")):
        kw = dict(dist=ns.NORMAL, mu=10.0, sigma=2.0, error_rate=0.5, alphabet="AGTC")
        kw.update(bad)
        with pytest.raises(ValueError):
            ns.noise_spec(_ONE, 1, kw["dist"], kw["mu"], kw["sigma"], error_rate=kw["error_rate"], alphabet=kw["alphabet"])
    with pytest.raises(ns.NoiseLimit):
        ns.noise_spec(_ONE, 1, ns.LOGNORMAL, 20.0, 0.1)
    # palindromic mode has no such limit: the hairpin is the whole molecule
    out = ns.noise_spec(_ONE, 1, ns.LOGNORMAL, 20.0, 0.1, palindromic=True, error_rate=0.0)
    assert [(s["start"], s["end"], s["plus"]) for s in out[0]["segments"]] == [(0, 10, True), (0, 10, False)]


# ------------------------------------------------------------------------------------------------ CPU: library and CLI surface
def test_library_exports_tail_noise():
    import ctypes
    from tksm_amd import _lib
    lib = ctypes.CDLL(os.path.join(ROOT, "tksm_amd", "libtksmseq.so"))
    for s in ("tksmseq_append_noise", "tksmseq_tail_noise_main"):
        assert s in _lib.SYMBOLS and hasattr(lib, s), s


def test_tksm_list_is_unchanged():
    r = _cli("list")
    assert r.returncode == 0 and r.stdout.split() == ["sequence", "pcr", "truncate", "polyA", "tag", "scb", "flip"]


@pytest.mark.parametrize("args,messages", [
    (["tail-noise"], ["input is required!", "output is required!", "length-dist is required!", "usage: tail-noise"]),
    (["tail-noise", "-i", "a", "-o", "b"], ["length-dist is required!", "usage: tail-noise"]),
    (["tail-noise", "-o", "b", "--length-dist", "normal,1,1"], ["input is required!", "usage: tail-noise"]),
    (["tail-noise", "-i", "a", "--length-dist=normal,1,1"], ["output is required!"]),
    (["tail-noise", "-i", "a", "-o", "b", "--length-dist", "gamma,1,1"], ["Distribution not implemented!"]),
    (["tail-noise", "-i", "a", "-o", "b", "--length-dist", "poisson"], ["Distribution not implemented!"]),
    (["tail-noise", "-i", "a", "-o", "b", "--length-dist", "normal,1"], ["length-dist needs NAME,MU,SIGMA"]),
    (["tail-noise", "-i", "a", "-o", "b", "--length-dist", "normal,1,2,3"], ["length-dist needs NAME,MU,SIGMA"]),
    (["tail-noise", "-i", "a", "-o", "b", "--length-dist", "lognormal,x,2"], ["length-dist needs NAME,MU,SIGMA"]),
    (["tail-noise", "-i", "a", "-o", "b", "--length-dist", "normal,1,0"], ["sigma finite and positive"]),
    (["tail-noise", "-i", "a", "-o", "b", "--length-dist", "normal,nan,1"], ["mu must be finite"]),
    (["tail-noise", "-i", "a", "-o", "b", "--length-dist", "normal,1,1", "--alphabet", ""], ["alphabet is empty"]),
    (["tail-noise", "-i", "a", "-o", "b", "--length-dist", "normal,1,1", "--error-rate", "nan"], ["error rate is not a number"]),
    (["tail-noise", "-i", "a", "-o", "b", "--length-dist", "normal,1,1", "--prepend"], ["does not exist"]),
])
def test_module_argument_checks(args, messages):
    r = _cli(*args)
    assert r.returncode == 1, (args, r.stderr)
    for m in messages:
        assert m in r.stderr, (args, m, r.stderr)


def test_module_help_exits_zero():
    r = _cli("tail-noise", "--help")
    assert r.returncode == 0 and "usage" in r.stdout and "--length-dist" in r.stdout


# ------------------------------------------------------------------------------------------------ GPU
def _genome(rs):
    return {f"chr{i + 1}": rs.choice(np.frombuffer(b"ACGT", np.uint8), 60_000).tobytes().decode() for i in range(2)}


@pytest.fixture(scope="module")
def gs():
    from tksm_amd.sequence import Sequencer
    rs = np.random.RandomState(21)
    ref = _genome(rs)
    s = Sequencer(0)
    for k, v in ref.items():
        s.add_contig(k, v)
    yield s, ref
    s.close()


def _no_comments(text):
    return "".join((l.rsplit("\t", 1)[0] + "\t\n") if l.startswith("+") else l for l in text.splitlines(keepends=True))


def _first_difference(got, want):
    g, w = got.splitlines(), want.splitlines()
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return f"line {i}: got {a[:300]!r}, want {b[:300]!r}"
    return f"{len(g)} lines against {len(w)}"


@pytest.mark.gpu
def test_kernels_match_the_spec(gs):
    """both distributions, both modes, error rates 0 / 0.5 / 1, a starting index that is not zero, depth > 1 input, comments on and off"""
    s, _ = gs
    text = _mdf(np.random.RandomState(1), 3000)
    assert "\t2\t" in text or "\t3\t" in text
    mols = mo.stream_mdf(text, unroll=True)
    b = s.batch_from_mdf(text)
    cases = [(ns.NORMAL, 50.0, 10.0, False, 0.5, "AGTC"), (ns.LOGNORMAL, 4.0, 0.9, False, 0.5, "AAAGTC"), (ns.NORMAL, 0.0, 40.0, False, 0.5, "N"),
             (ns.NORMAL, 300.0, 200.0, True, 0.0, "AGTC"), (ns.NORMAL, 300.0, 200.0, True, 0.5, "AGTC"), (ns.NORMAL, 300.0, 200.0, True, 1.0, "AGTC"),
             (ns.LOGNORMAL, 5.5, 1.0, True, 0.5, "AAAGTC"), (ns.LOGNORMAL, 5.5, 1.0, True, 0.05, "ac"), (ns.NORMAL, 2000.0, 1500.0, True, 1.5, "AGTC"),
             (ns.NORMAL, 300.0, 200.0, True, -1.0, "AGTC")]
    for dist, mu, sigma, pal, rate, alphabet in cases:
        out = s.append_noise(b, dist, mu, sigma, palindromic=pal, error_rate=rate, alphabet=alphabet, seed=17, first=12345)
        want = mo.write_mdf(ns.noise_spec(mols, 17, dist, mu, sigma, pal, rate, alphabet, first=12345))
        got = s.to_mdf_text(out)
        assert got == want, ((dist, mu, sigma, pal, rate, alphabet), _first_difference(got, want))
        out.free()
    for pal in (False, True):
        out = s.append_noise(b, ns.NORMAL, 100.0, 50.0, palindromic=pal, seed=17, comments=False)
        assert s.to_mdf_text(out) == _no_comments(mo.write_mdf(ns.noise_spec(mols, 17, ns.NORMAL, 100.0, 50.0, pal)))
        out.free()
    # the hairpin of a hairpin: many copied substitutions merged with the new ones
    b1 = s.append_noise(b, ns.NORMAL, 400.0, 100.0, palindromic=True, error_rate=0.5, seed=3)
    b2 = s.append_noise(b1, ns.NORMAL, 500.0, 200.0, palindromic=True, error_rate=0.3, seed=4)
    m1 = ns.noise_spec(mols, 3, ns.NORMAL, 400.0, 100.0, True, 0.5)
    want = mo.write_mdf(ns.noise_spec(m1, 4, ns.NORMAL, 500.0, 200.0, True, 0.3))
    got = s.to_mdf_text(b2)
    assert got == want, _first_difference(got, want)
    b2.free(); b1.free(); b.free()
    # an empty batch
    e = s.batch_from_mdf("")
    for pal in (False, True):
        out = s.append_noise(e, ns.NORMAL, 50.0, 10.0, palindromic=pal)
        assert s.to_mdf_text(out) == ""
        out.free()
    e.free()


def _big_mdf(n):
    """n molecules of 1 - 6 segments (minus strands, a substitution each, some depth 2), cheap to make"""
    rs = np.random.RandomState(6)
    nseg = rs.randint(1, 7, n)
    st = rs.randint(0, 59_000, n)
    ln = rs.randint(1, 120, n)
    dep = np.where(rs.rand(n) < 0.03, 2, 1)
    out = []
    for i in range(n):
        out.append(f"+m{i}\t{dep[i]}\t\n")
        for k in range(nseg[i]):
            out.append(f"chr{1 + ((i + k) & 1)}\t{st[i] + k}\t{st[i] + k + ln[i]}\t{'+-'[(i >> k) & 1]}\t{(i + k) % ln[i]}G\n")
    return "".join(out)


@pytest.mark.gpu
def test_large_batch_matches_the_spec_whole_and_in_pieces(gs):
    """at least 200 000 molecules with 1 - 6 segments against the specification, and one batch whole equals the same batch in pieces with
    matching first"""
    s, _ = gs
    text = _big_mdf(200_000)
    mols = mo.stream_mdf(text, unroll=True)
    assert len(mols) >= 200_000 and {len(m["segments"]) for m in mols} == {1, 2, 3, 4, 5, 6}
    cuts = [0] + [text.index("\n+", len(text) * q // 4) + 1 for q in (1, 2, 3)] + [len(text)]
    for pal, mu, sigma in ((True, 150.0, 120.0), (False, 20.0, 12.0)):
        b = s.batch_from_mdf(text)
        out = s.append_noise(b, ns.NORMAL, mu, sigma, palindromic=pal, error_rate=0.5, seed=11, first=7)
        whole = s.to_mdf_text(out)
        out.free(); b.free()
        want = mo.write_mdf(ns.noise_spec(mols, 11, ns.NORMAL, mu, sigma, pal, 0.5, first=7))
        assert whole == want, (pal, _first_difference(whole, want))
        parts, first = [], 7
        for i in range(4):
            b = s.batch_from_mdf(text[cuts[i]:cuts[i + 1]])
            out = s.append_noise(b, ns.NORMAL, mu, sigma, palindromic=pal, error_rate=0.5, seed=11, first=first)
            parts.append(s.to_mdf_text(out))
            first += out.n_reads
            out.free(); b.free()
        assert "".join(parts) == whole, pal


def _reads(s, b):
    return [r.split(b"\n")[1].decode() for r in s.run(b, target="perfect", fastq=True, seed=1).records()]


def _revcomp(x):
    return x[::-1].translate(str.maketrans("ACGT", "TGCA"))


@pytest.mark.gpu
def test_perfect_reads_show_the_hairpin_and_the_letters(gs):
    """Not through the specification: with --palindromic --error-rate 0 --length-dist normal,1000000,1 every hairpin is the whole molecule,
    so the perfect read of an output molecule is the input molecule's read followed by its reverse complement (literals, minus strands
    and substitutions in the corpus); in random mode it is the input's read followed by L letters of the alphabet"""
    s, _ = gs
    text = _mdf(np.random.RandomState(9), 2000, depth=False)
    assert "\t-\t" in text and "0C\n" in text
    b = s.batch_from_mdf(text)
    before = _reads(s, b)
    out = s.append_noise(b, ns.NORMAL, 1_000_000.0, 1.0, palindromic=True, error_rate=0.0)
    after = _reads(s, out)
    out.free()
    assert len(after) == len(before) == 2000
    for i, (x, y) in enumerate(zip(before, after)):
        assert y == x + _revcomp(x), i
    out = s.append_noise(b, ns.NORMAL, 40.0, 25.0, alphabet="CCT", seed=5, first=3)
    after = _reads(s, out)
    out.free(); b.free()
    added = 0
    for i, (x, y) in enumerate(zip(before, after)):
        assert y.startswith(x) and set(y[len(x):]) <= set("CT"), i
        added += len(y) - len(x)
    lens = ns.noise_lengths_spec(ns.noise_draws_spec(5, np.arange(3, 2003, dtype=np.uint64), ns.NORMAL, 40.0, 25.0))
    assert added == int(np.maximum(lens, 0).sum()) > 50_000


@pytest.mark.gpu
def test_module_route(gs, tmp_path):
    """`tksm tail-noise` on a file equals the specification's text, whatever --batch-bytes and --devices; its output goes through
    `tksm sequence` with Badread and q-scores"""
    from conftest import ERR_MODEL, QS_MODEL
    _, ref = gs
    env = dict(os.environ, TKSM_MODELS=os.path.join(ROOT, "tksm_amd", "models"))
    text = _mdf(np.random.RandomState(7), 400)
    mols = mo.stream_mdf(text, unroll=True)
    src, fa = tmp_path / "in.mdf", tmp_path / "ref.fa"
    src.write_text(text)
    fa.write_text("".join(f">{k}\n{v}\n" for k, v in ref.items()))
    outs = []
    for k, (flags, kw) in enumerate([(["--length-dist", "normal,50,10"], dict(dist=ns.NORMAL, mu=50.0, sigma=10.0)),
                                     (["--length-dist=lognormal,4,0.5", "--alphabet", "AAAGTC"], dict(dist=ns.LOGNORMAL, mu=4.0, sigma=0.5, alphabet="AAAGTC")),
                                     (["--length-dist", "normal,300,150", "--palindromic"], dict(dist=ns.NORMAL, mu=300.0, sigma=150.0, palindromic=True)),
                                     (["--length-dist", "normal,300,150", "--palindromic", "--error-rate", "0.1"],
                                      dict(dist=ns.NORMAL, mu=300.0, sigma=150.0, palindromic=True, error_rate=0.1))]):
        dst, alt = tmp_path / f"out{k}.mdf", tmp_path / f"alt{k}.mdf"
        r = _cli("tail-noise", "-i", src, "-o", dst, *flags, "-s", 13, env=env)
        assert r.returncode == 0, (flags, r.stderr[-600:])
        want = mo.write_mdf(ns.noise_spec(mols, 13, kw.pop("dist"), kw.pop("mu"), kw.pop("sigma"), **kw))
        assert dst.read_text() == want, (flags, _first_difference(dst.read_text(), want))
        r = _cli("tail-noise", "-i", src, "-o", alt, *flags, "-s", 13, "--batch-bytes", "3000", "--devices", "0,0", env=env)
        assert r.returncode == 0 and alt.read_bytes() == dst.read_bytes(), flags
        outs.append(dst)
    # the default seed is 42
    r = _cli("tail-noise", "-i", src, "-o", tmp_path / "d.mdf", "--length-dist", "normal,50,10", env=env)
    assert r.returncode == 0 and (tmp_path / "d.mdf").read_text() == mo.write_mdf(ns.noise_spec(mols, 42, ns.NORMAL, 50.0, 10.0))
    for k in (0, 3):
        fq = tmp_path / f"r{k}.fastq"
        r = _cli("sequence", "-i", outs[k], "-r", fa, "-o", fq, "-s", 13, "--badread-error-model", ERR_MODEL, "--badread-qscore-model", QS_MODEL,
                 "--badread-identity", "84,99,5.5", env=env)
        assert r.returncode == 0, r.stderr[-600:]
        assert fq.read_bytes().count(b"\n") == 4 * len(mols)


@pytest.mark.gpu
def test_errors(gs, tmp_path):
    from tksm_amd import _lib as L
    from tksm_amd.sequence import TksmSeqError
    s, _ = gs
    b = s.batch_from_mdf("+a\t1\t\nchr1\t0\t50\t+\t\n+deep\t2\t\nchr1\t0\t50\t-\t\n")
    for bad in (dict(alphabet=""), dict(mu=float("nan")), dict(mu=float("-inf")), dict(sigma=0.0), dict(sigma=-2.0), dict(sigma=float("nan")),
                dict(error_rate=float("nan"))):
        kw = dict(mu=10.0, sigma=2.0, error_rate=0.5, alphabet="AGTC")
        kw.update(bad)
        for pal in (False, True):
            with pytest.raises(TksmSeqError) as e:
                s.append_noise(b, "normal", kw["mu"], kw["sigma"], palindromic=pal, error_rate=kw["error_rate"], alphabet=kw["alphabet"])
            assert e.value.code == L.EINVAL, bad
    with pytest.raises(ValueError, match="Distribution not implemented!"):
        s.append_noise(b, "gamma", 1.0, 1.0)
    # the unknown distribution at the C boundary
    import ctypes as C
    p = L.NoiseParams(1, 0, 7, 0, 1.0, 1.0, 0.5, b"AGTC", 0, 0)
    h = C.c_void_p()
    assert s._lib.tksmseq_append_noise(s._ctx, b._h, C.byref(p), C.byref(h)) == L.EINVAL
    # random mode: a drawn length above 2^20 names the molecule; the palindromic mode takes the same draw
    with pytest.raises(TksmSeqError, match="molecule a ") as e:
        s.append_noise(b, "lognormal", 20.0, 0.1)
    assert e.value.code == L.ELIMIT
    out = s.append_noise(b, "lognormal", 20.0, 0.1, palindromic=True, error_rate=0.0)
    assert s.to_mdf_text(out) == ("+a\t1\t\nchr1\t0\t50\t+\t\nchr1\t0\t50\t-\t\n+deep_0\t1\t\nchr1\t0\t50\t-\t\nchr1\t0\t50\t+\t\n"
                                  "+deep_1\t1\t\nchr1\t0\t50\t-\t\nchr1\t0\t50\t+\t\n")
    out.free(); b.free()
    src = tmp_path / "in.mdf"
    src.write_text("+a\t1\t\nchr1\t0\t50\t+\t\n")
    r = _cli("tail-noise", "-i", src, "-o", tmp_path / "o.mdf", "--length-dist", "lognormal,20,0.1")
    assert r.returncode == 1 and "above 1048576" in r.stderr
    r = _cli("tail-noise", "-i", tmp_path / "absent.mdf", "-o", tmp_path / "o.mdf", "--length-dist", "normal,5,1")
    assert r.returncode == 1 and "Could not open file" in r.stderr
