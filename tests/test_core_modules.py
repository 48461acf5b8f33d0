"""polyA, tag, scb and flip: the segment edits of the reference README's single-cell route (plA -> Tag -> SCB -> Tag -> PCR -> Flp ->
Tag -> Seq) as device-side MDF transforms.

CPU part: the specification (tests/core_modules_spec.py) against the reference's algorithms / scipy (distributions), the library's
exports and the `tksm` modules' argument checks.
GPU part (-m gpu): tksmseq_polya / _tag / _scb / _flip against the specification, text for text; independence of batching; the
README route device to device and through files, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import core_modules_spec as cs
import mdf_ops_oracle as mo

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
KS_GATE = 0.004                          # the flat KS gate of tests/test_oracle_golden.py
N_KS = 300_000


def _cli(*args, **kw):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=600, **kw)


def _chi2_p(obs, expected):
    from scipy.stats import chisquare
    return chisquare(obs, expected).pvalue


# ------------------------------------------------------------------------------------------------ CPU: specification
def test_vectorised_philox_is_the_oracles():
    assert cs.philox_matches_oracle([(42, 0, 26, 0), (7, 123456789012, 27, 3), (2**40 + 5, 2**33 + 1, 29, 0), (1, 5, 28, 17)])


@pytest.mark.parametrize("dist,a,b", [(cs.NORMAL, 15.0, 7.5), (cs.NORMAL, -3.0, 0.5), (cs.WEIBULL, 1.5, 20.0), (cs.WEIBULL, 0.6, 3.0),
                                      (cs.GAMMA, 4.0, 5.0), (cs.GAMMA, 0.4, 10.0), (cs.GAMMA, 1.0, 2.0)])
def test_polya_continuous_draws_have_the_named_distribution(dist, a, b):
    """std::normal / weibull / gamma_distribution (a = shape, b = scale for the last two): KS on 300 000 draws"""
    from scipy import stats
    d = cs.polya_draws_spec(99, np.arange(10**6, 10**6 + N_KS, dtype=np.uint64), dist, a, b)
    cdf = {cs.NORMAL: stats.norm(a, b).cdf, cs.WEIBULL: stats.weibull_min(a, scale=b).cdf, cs.GAMMA: stats.gamma(a, scale=b).cdf}[dist]
    assert stats.kstest(d, cdf).statistic <= KS_GATE


@pytest.mark.parametrize("lam", [0.7, 6.5, 10.0, 37.5, 400.0])
def test_polya_poisson_draws_are_poisson(lam):
    """multiplication below lambda = 10, PTRS from 10 on: chi-square against the Poisson pmf"""
    from scipy import stats
    d = cs.polya_draws_spec(5, np.arange(N_KS, dtype=np.uint64), cs.POISSON, lam).astype(np.int64)
    assert (d >= 0).all() and (d == np.floor(d)).all()
    lo, hi = int(stats.poisson.ppf(1e-4, lam)), int(stats.poisson.ppf(1 - 1e-4, lam))
    edges = np.arange(lo, hi + 2)
    obs = np.array([(d < lo).sum()] + [(d == k).sum() for k in edges[:-1]] + [(d > hi).sum()], float)
    pmf = np.array([stats.poisson.cdf(lo - 1, lam)] + [stats.poisson.pmf(k, lam) for k in edges[:-1]] + [stats.poisson.sf(hi, lam)])
    keep = pmf * N_KS >= 5
    obs, exp = np.append(obs[keep], obs[~keep].sum()), np.append(pmf[keep], pmf[~keep].sum()) * N_KS
    obs, exp = obs[exp > 0], exp[exp > 0]
    assert _chi2_p(obs, exp * obs.sum() / exp.sum()) > 1e-3


@pytest.mark.parametrize("dist,a,b,lo,hi", [(cs.NORMAL, 15.0, 7.5, 0, 5000), (cs.NORMAL, 15.0, 7.5, 10, 20), (cs.POISSON, 12.0, 0.0, 8, 14),
                                            (cs.GAMMA, 2.0, 8.0, 5, 30), (cs.WEIBULL, 2.0, 30.0, 0, 25)])
def test_polya_lengths_match_the_reference_algorithm(dist, a, b, lo, hi):
    """lengths (toward zero, clamped to [min, max]) of the spec against add_polyA with numpy's generator: chi-square on the length
    histogram, clamping active in the narrow cases"""
    n = 200_000
    got = cs.polya_lengths_spec(cs.polya_draws_spec(11, np.arange(n, dtype=np.uint64), dist, a, b), lo, hi)
    mols = [dict(id="m", depth=1, meta={}, segments=[])] * 1
    rs = np.random.RandomState(3)
    ref = np.array([cs.polya_reference(mols, dist, a, b, lo, hi, rs)[1][0] for _ in range(n)])
    assert got.min() >= lo and got.max() <= hi
    if hi - lo <= 20:
        assert (got == lo).mean() > 0.01 and (got == hi).mean() > 0.01        # clamping happens on both sides
    cg, cr = np.bincount(got - lo, minlength=hi - lo + 1), np.bincount(ref - lo, minlength=hi - lo + 1)
    keep = (cg + cr) >= 20
    a_, b_ = np.append(cg[keep], cg[~keep].sum()), np.append(cr[keep], cr[~keep].sum())
    keep = (a_ + b_) > 0
    from scipy.stats import chi2
    a_, b_ = a_[keep].astype(float), b_[keep].astype(float)
    assert chi2.sf((((a_ - b_) ** 2) / (a_ + b_)).sum(), len(a_) - 1) > 1e-3


def test_polya_clamp_defines_huge_and_nan_draws():
    assert list(cs.polya_lengths_spec([np.nan, 1e300, -1e300, 4.9, 5.0, 7.99, 8.0, 1e9], 5, 8)) == [5, 8, 5, 5, 5, 7, 8, 8]


def test_tag_iupac_draws_are_uniform_and_unknown_letters_vanish():
    n = 200_000
    fmt = cs.tag_format("NRYKMSWBDHVACGTU-xn*")
    assert fmt == "NRYKMSWBDHVACGTU"                         # lower case and other characters contribute nothing
    tags = cs.tag_draws_spec(8, np.arange(n, dtype=np.uint64), cs.ST_TAG3, fmt)
    arr = np.frombuffer("".join(tags).encode(), np.uint8).reshape(n, len(fmt))
    for j, ch in enumerate(fmt):
        choices = cs.IUPAC[ch]
        col = arr[:, j]
        obs = np.array([(col == ord(c)).sum() for c in choices], float)
        assert obs.sum() == n, ch
        if len(choices) > 1:
            assert _chi2_p(obs, np.full(len(choices), n / len(choices))) > 1e-3, ch
    # the 5' and 3' streams are different draws
    t5 = cs.tag_draws_spec(8, np.arange(1000, dtype=np.uint64), cs.ST_TAG5, "NNNNNNNN")
    t3 = cs.tag_draws_spec(8, np.arange(1000, dtype=np.uint64), cs.ST_TAG3, "NNNNNNNN")
    assert sum(a == b for a, b in zip(t5, t3)) < 5


def test_tag_digit_rule_and_reference_counts():
    assert cs.tag_format("10") == "N" * 10 and cs.tag_format("3ACG") == "NNN" and cs.tag_format("AGATC") == "AGATC"
    assert cs.tag_format("") == "" and cs.tag_format("acgt") == ""
    mols = [dict(id=f"m{i}", depth=1, meta={}, segments=[dict(chr="c", start=0, end=5, plus=True, errors=[])]) for i in range(3000)]
    ref = cs.tag_reference(mols, "4", "ACG", np.random.RandomState(1))
    spec = cs.tag_spec(mols, 1, "4", "ACG")
    for out in (ref, spec):
        assert all(len(m["segments"]) == 3 and len(m["segments"][0]["chr"]) == 4 and m["segments"][2]["chr"] == "ACG" for m in out)
    # base composition of the random 5' tags: spec vs reference
    cnt = [np.array([sum(m["segments"][0]["chr"].count(c) for m in out) for c in "ACGT"], float) for out in (ref, spec)]
    from scipy.stats import chi2_contingency
    assert chi2_contingency(np.stack(cnt))[1] > 1e-3


@pytest.mark.parametrize("p", [0.0, 0.3, 0.5, 1.0, -0.5, 1.5])
def test_flip_count_is_binomial(p):
    from scipy.stats import binom
    n = 200_000
    k = int(cs.flip_bits_spec(4, np.arange(n, dtype=np.uint64), p).sum())
    q = min(1.0, max(0.0, p))
    if q in (0.0, 1.0):
        assert k == int(q * n)
    else:
        assert 1e-4 < binom.cdf(k, n, q) < 1 - 1e-4
    mols = [dict(id="a", depth=1, meta={"x": ["1"]}, segments=[dict(chr="c1", start=0, end=5, plus=True, errors=[(1, "A")]),
                                                                  dict(chr="c2", start=7, end=9, plus=False, errors=[])])] * 200
    ref = cs.flip_reference(mols, q, np.random.RandomState(2))
    spec = cs.flip_spec(mols, 4, q)
    for out in (ref, spec):
        for m in out:
            assert [(s["chr"], s["plus"]) for s in m["segments"]] in ([("c1", True), ("c2", False)], [("c2", True), ("c1", False)])
            assert m["meta"] == {"x": ["1"]} and [s["errors"] for s in m["segments"] if s["chr"] == "c1"] == [[(1, "A")]]


def test_scb_spec_appends_the_first_barcode_and_drops_the_key():
    text = "+a\t1\tCB=ACGT,TTTT;x=1;\nc\t0\t5\t+\t\n+b\t2\tCB;\nc\t0\t5\t-\t1A\n"
    mols = mo.stream_mdf(text, unroll=True)
    out = mo.write_mdf(cs.scb_spec(mols))
    assert out == ("+a\t1\tx=1;\nc\t0\t5\t+\t\nACGT\t0\t4\t+\t\n+b_0\t1\t\nc\t0\t5\t-\t1A\n+b_1\t1\t\nc\t0\t5\t-\t1A\n")
    assert mo.write_mdf(cs.scb_spec(mols, keep_meta_barcodes=True)).startswith("+a\t1\tCB=ACGT,TTTT;x=1;\n")
    with pytest.raises(KeyError):
        cs.scb_spec(mo.stream_mdf("+z\t1\tx=1;\nc\t0\t5\t+\t\n"))


# ------------------------------------------------------------------------------------------------ CPU: library and CLI surface
def test_library_exports_the_segment_edits():
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "tksm_amd", "libtksmseq.so"))
    for s in ("polya", "tag", "scb", "flip"):
        assert hasattr(lib, f"tksmseq_{s}") and hasattr(lib, f"tksmseq_{s}_main"), s


def test_tksm_list_names_all_seven_modules():
    r = _cli("list")
    assert r.returncode == 0 and r.stdout.split() == ["sequence", "pcr", "truncate", "polyA", "tag", "scb", "flip"]


@pytest.mark.parametrize("args,messages", [
    (["polyA", "-i", "a", "-o", "b"], ["No distribution specified"]),
    (["polyA", "-i", "a", "-o", "b", "--gamma", "1,2", "--normal", "1,2"], ["Multiple distributions specified"]),
    (["polyA", "-i", "a", "-o", "b", "--gamma", "1"], ["Gamma distribution requires two parameters"]),
    (["polyA", "-i", "a", "-o", "b", "--poisson", "1,2"], ["Poisson distribution requires one parameter"]),
    (["polyA", "-i", "a", "-o", "b", "--weibull", "1,2,3"], ["Weibull distribution requires two parameters"]),
    (["polyA", "-i", "a", "-o", "b", "--normal=4"], ["Normal distribution requires two parameters"]),
    (["polyA", "--normal", "1,1", "--min-length", "-1", "--max-length", "-3"],
     ["Missing parameter: input", "Missing parameter: output", "Minimum length of polyA cannot be negative",
      "Maximum length of polyA cannot be negative", "Minimum length of polyA cannot be greater than maximum length of polyA"]),
    (["polyA", "-i", "a", "-o", "b", "--gamma", "0,2"], ["must be finite and positive"]),
    (["polyA", "-i", "a", "-o", "b", "--poisson", "-1"], ["must be finite and positive"]),
    (["polyA", "-i", "a", "-o", "b", "--normal", "5,0"], ["must be finite and positive"]),
    (["polyA", "-i", "a", "-o", "b", "--weibull", "nan,1"], ["must be finite and positive"]),
    (["tag", "-i", "a"], ["output is required!", "At least one of the TAG formats must be provided"]),
    (["tag", "-o", "b", "-5", "ACG"], ["input is required!"]),
    (["scb", "-o", "b"], ["Missing parameter: input"]),
    (["flip", "-i", "a", "-o", "b"], ["Missing parameter: flip-probability"]),
    (["polyA", "-i", "a", "-o", "b", "--bogus", "1"], ["does not exist"]),
])
def test_module_argument_checks_follow_the_reference(args, messages):
    r = _cli(*args)
    assert r.returncode == 1, (args, r.stderr)
    for m in messages:
        assert m in r.stderr, (args, m, r.stderr)


@pytest.mark.parametrize("module", ["polyA", "tag", "scb", "flip"])
def test_module_help_exits_zero(module):
    r = _cli(module, "--help")
    assert r.returncode == 0 and "usage" in r.stdout


# ------------------------------------------------------------------------------------------------ GPU
def _genome(rs):
    return {f"chr{i + 1}": rs.choice(np.frombuffer(b"ACGT", np.uint8), 60_000).tobytes().decode() for i in range(2)}


def _mdf(rs, n, cb=True):
    """molecules with depth > 1, literal and minus-strand segments, substitutions and comments (CB among them when cb)"""
    lines = []
    bcs = ["ACGTACGTAC", "TTGACCATGA", "GGGCCCAAAT", "."]
    for i in range(n):
        depth = 1 if rs.rand() < 0.8 else int(rs.randint(2, 4))
        cm = ["tid=ENST7;", "z;a=1,2;", ""][int(rs.randint(0, 3))]
        if cb:
            k = int(rs.randint(0, 6))
            cm += "CB;" if k == 5 else f"CB={bcs[k % 4]};" if k < 4 else f"CB={bcs[0]},{bcs[1]};"
        lines.append(f"+mol{i}\t{depth}\t{cm}\n")
        for _ in range(int(rs.randint(1, 5))):
            ln = int(rs.randint(1, 600))
            st = int(rs.randint(0, 59_000))
            md = ",".join(f"{int(rs.randint(0, ln))}{'ACGT'[int(rs.randint(0, 4))]}" for _ in range(int(rs.randint(0, 3))))
            lines.append(f"chr{int(rs.randint(1, 3))}\t{st}\t{st + ln}\t{'+-'[int(rs.randint(0, 2))]}\t{md}\n")
        if rs.rand() < 0.3:
            pa = "A" * int(rs.randint(1, 30))
            lines.append(f"{pa}\t0\t{len(pa)}\t-\t0C\n")
    return "".join(lines)


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


@pytest.mark.gpu
def test_polya_kernels_match_the_spec(gs):
    s, _ = gs
    text = _mdf(np.random.RandomState(1), 3000)
    mols = mo.stream_mdf(text, unroll=True)
    b = s.batch_from_mdf(text)
    for kw, lo, hi in ((dict(normal=(15.0, 7.5)), 0, 5000), (dict(normal=(15.0, 7.5)), 8, 20), (dict(gamma=(0.5, 30.0)), 0, 5000),
                       (dict(gamma=(3.0, 4.0)), 0, 12), (dict(weibull=(1.5, 20.0)), 2, 5000), (dict(poisson=4.0), 0, 5000),
                       (dict(poisson=60.0), 0, 55)):
        (name, v), = kw.items()
        a, bb = (v, 0.0) if name == "poisson" else v
        out = s.polya(b, **kw, min_length=lo, max_length=hi, seed=17, first_molecule_index=12345)
        want = mo.write_mdf(cs.polya_spec(mols, 17, name, a, bb, lo, hi, first=12345))
        assert s.to_mdf_text(out) == want, kw
        out.free()
    out = s.polya(b, normal=(15.0, 7.5), seed=17, comments=False)
    assert s.to_mdf_text(out) == _no_comments(mo.write_mdf(cs.polya_spec(mols, 17, "normal", 15.0, 7.5)))
    out.free()
    from tksm_amd.sequence import TksmSeqError
    for bad in (dict(gamma=(0.0, 1.0)), dict(normal=(1.0, -1.0)), dict(weibull=(float("inf"), 1.0)), dict(poisson=float("nan"))):
        with pytest.raises(TksmSeqError):
            s.polya(b, **bad)
    b.free()


@pytest.mark.gpu
def test_tag_kernels_match_the_spec(gs):
    s, _ = gs
    text = _mdf(np.random.RandomState(2), 3000)
    mols = mo.stream_mdf(text, unroll=True)
    b = s.batch_from_mdf(text)
    for f5, f3 in (("NNNNNN", ""), ("", "10"), ("AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT"), ("RYKMSWBDHVN", "acgtXN-U"),
                   ("12", "AGATCGGAAGAGCGTCGTGTAG"), ("xyz", "ACG")):
        out = s.tag(b, format5=f5, format3=f3, seed=9, first_molecule_index=777)
        assert s.to_mdf_text(out) == mo.write_mdf(cs.tag_spec(mols, 9, f5, f3, first=777)), (f5, f3)
        out.free()
    out = s.tag(b, format3="10", seed=9, comments=False)
    assert s.to_mdf_text(out) == _no_comments(mo.write_mdf(cs.tag_spec(mols, 9, "", "10")))
    out.free(); b.free()


@pytest.mark.gpu
def test_scb_kernels_match_the_spec(gs):
    from tksm_amd.sequence import TksmSeqError
    s, _ = gs
    text = _mdf(np.random.RandomState(3), 3000)
    mols = mo.stream_mdf(text, unroll=True)
    b = s.batch_from_mdf(text)
    assert "CB=.;" in text and "CB;" in text
    for keep in (False, True):
        out = s.scb(b, keep_meta_barcodes=keep)
        assert s.to_mdf_text(out) == mo.write_mdf(cs.scb_spec(mols, keep)), keep
        out.free()
    out = s.scb(b, comments=False)
    assert s.to_mdf_text(out) == _no_comments(mo.write_mdf(cs.scb_spec(mols)))
    out.free(); b.free()
    # a molecule without CB: the reference's meta.at throws; here an error that names the molecule
    b = s.batch_from_mdf(text + "+lost\t2\tx=1;\nchr1\t5\t50\t+\t\n")
    with pytest.raises(TksmSeqError, match="lost_0"):
        s.scb(b)
    b.free()
    # a batch without comments at all
    b = s.batch_from_arrays(np.array([[0, 1]]), np.array([[0, 0, 10, 0], [0, 0, 0, 0]]), ids=np.array([[0, 1]]), id_pool=b"m")
    with pytest.raises(TksmSeqError):
        s.scb(b)
    b.free()


@pytest.mark.gpu
def test_flip_kernels_match_the_spec(gs):
    s, _ = gs
    text = _mdf(np.random.RandomState(4), 3000)
    mols = mo.stream_mdf(text, unroll=True)
    b = s.batch_from_mdf(text)
    for p in (0.0, 0.3, 1.0):
        out = s.flip(b, p, seed=5, first_molecule_index=4242)
        assert s.to_mdf_text(out) == mo.write_mdf(cs.flip_spec(mols, 5, p, first=4242)), p
        out.free()
    out = s.flip(b, 0.3, seed=5, comments=False)
    assert s.to_mdf_text(out) == _no_comments(mo.write_mdf(cs.flip_spec(mols, 5, 0.3)))
    out.free(); b.free()


def _big_mdf(n):
    """n molecules (some depth 2), cheap to make: what the split-batch test streams"""
    rs = np.random.RandomState(6)
    st = rs.randint(0, 59_000, n)
    ln = rs.randint(50, 900, n)
    dep = np.where(rs.rand(n) < 0.05, 2, 1)
    bc = rs.randint(0, 5000, n)
    strand = np.where(rs.rand(n) < 0.5, "+", "-")
    return "".join(f"+m{i}\t{dep[i]}\tCB=B{bc[i]:05d};\nchr{1 + (i & 1)}\t{st[i]}\t{st[i] + ln[i]}\t{strand[i]}\t{i % 7}G\n" for i in range(n))


@pytest.mark.gpu
def test_split_batches_equal_the_whole(gs):
    """2 M molecules through polyA -> tag -> scb -> flip whole and in four batches with matching first_molecule_index: the same text"""
    s, _ = gs
    text = _big_mdf(1_950_000)
    cuts = [0]
    for q in (1, 2, 3):
        k = text.index("\n+", len(text) * q // 4) + 1
        cuts.append(k)
    cuts.append(len(text))
    pieces = [text[cuts[i]:cuts[i + 1]] for i in range(4)]

    def chain(t, first):
        b0 = s.batch_from_mdf(t)
        b1 = s.polya(b0, gamma=(2.0, 8.0), seed=3, first_molecule_index=first)
        b2 = s.tag(b1, format5="8", format3="ACGTN", seed=3, first_molecule_index=first)
        b3 = s.scb(b2)
        b4 = s.flip(b3, 0.5, seed=3, first_molecule_index=first)
        out = s.to_mdf_text(b4)
        n = b4.n_reads
        for x in (b4, b3, b2, b1, b0):
            x.free()
        return out, n

    whole, n_all = chain(text, 0)
    assert n_all > 2_000_000
    parts, first = [], 0
    for p in pieces:
        t, n = chain(p, first)
        parts.append(t)
        first += n
    assert "".join(parts) == whole


@pytest.mark.gpu
def test_readme_single_cell_route_device_and_files(gs, oracle_models, tmp_path):
    """The README's TKSM_single_cell route (minus Flt / Mrg): polyA -> tag -> scb -> tag -> pcr -> flip -> tag -> Seq, once device to
    device through the C-ABI and once through `tksm` module by module over MDF files: every intermediate MDF equals the spec (PCR:
    the oracle's pcr_spec), the FASTQ of both routes is byte-identical (perfect, and Badread with q-scores); the file modules do not
    depend on --batch-bytes or --devices."""
    from conftest import ERR_MODEL, QS_MODEL
    s, ref = gs
    env = dict(os.environ, TKSM_MODELS=os.path.join(ROOT, "tksm_amd", "models"))
    text = _mdf(np.random.RandomState(7), 400)
    fa = tmp_path / "ref.fa"
    fa.write_text("".join(f">{k}\n{v}\n" for k, v in ref.items()))
    src = tmp_path / "in.mdf"
    src.write_text(text)
    seed = 13
    a5, a3 = "AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT"
    # the spec, step by step (each module reads its input unrolled and numbers molecules from 0)
    m = cs.polya_spec(mo.stream_mdf(text, unroll=True), seed, "normal", 15.0, 7.5)
    want = [mo.write_mdf(m)]
    m = cs.tag_spec(mo.stream_mdf(want[-1]), seed, "", "10"); want.append(mo.write_mdf(m))
    m = cs.scb_spec(mo.stream_mdf(want[-1])); want.append(mo.write_mdf(m))
    m = cs.tag_spec(mo.stream_mdf(want[-1]), seed, "", "AGATCGGAAGAGCGTCGTGTAG"); want.append(mo.write_mdf(m))
    er, ef = mo.PRESETS["Taq-setting1"]
    m = mo.pcr_spec(mo.stream_mdf(want[-1]), 5, ef, er, 3000, seed); want.append(mo.write_mdf(m))
    m = cs.flip_spec(mo.stream_mdf(want[-1]), seed, 0.5); want.append(mo.write_mdf(m))
    m = cs.tag_spec(mo.stream_mdf(want[-1]), seed, a5, a3); want.append(mo.write_mdf(m))
    # device to device
    b = [s.batch_from_mdf(text)]
    b.append(s.polya(b[-1], normal=(15.0, 7.5), seed=seed))
    b.append(s.tag(b[-1], format3="10", seed=seed))
    b.append(s.scb(b[-1]))
    b.append(s.tag(b[-1], format3="AGATCGGAAGAGCGTCGTGTAG", seed=seed))
    b.append(s.pcr(b[-1], 5, 3000, preset="Taq-setting1", seed=seed))
    b.append(s.flip(b[-1], 0.5, seed=seed))
    b.append(s.tag(b[-1], format5=a5, format3=a3, seed=seed))
    for k in range(1, len(b)):
        assert s.to_mdf_text(b[k]) == want[k - 1], k
    s.set_identity(84.0, 99.0, 5.5)
    s.load_error_model(ERR_MODEL)
    s.load_qscore_model(QS_MODEL)
    dev_perfect = b"".join(s.run(b[-1], target="perfect", fastq=True, seed=seed).records())
    dev_bad = b"".join(s.run(b[-1], target="badread", fastq=True, compute_qual=True, seed=seed).records())
    for x in reversed(b):
        x.free()
    # through files, module by module
    steps = [["polyA", "--normal=15,7.5"], ["tag", "--format3", "10"], ["scb"], ["tag", "--format3", "AGATCGGAAGAGCGTCGTGTAG"],
             ["pcr", "--cycles", "5", "--molecule-count", "3000", "-x", "Taq-setting1"], ["flip", "-p", "0.5"],
             ["tag", "--format5", a5, "--format3", a3]]
    cur = src
    for k, st in enumerate(steps):
        nxt = tmp_path / f"step{k}.mdf"
        r = _cli(st[0], "-i", cur, "-o", nxt, *st[1:], "-s", seed, env=env)
        assert r.returncode == 0, (st, r.stderr[-600:])
        assert nxt.read_text() == want[k], st
        if st[0] != "pcr":
            alt = tmp_path / f"step{k}_alt.mdf"
            r = _cli(st[0], "-i", cur, "-o", alt, *st[1:], "-s", seed, "--batch-bytes", "3000", "--devices", "0,0", env=env)
            assert r.returncode == 0 and alt.read_bytes() == nxt.read_bytes(), st
        cur = nxt
    fq_p, fq_b = tmp_path / "p.fastq", tmp_path / "b.fastq"
    r = _cli("sequence", "-i", cur, "-r", fa, "--perfect", fq_p, "-s", seed, env=env)
    assert r.returncode == 0, r.stderr[-600:]
    r = _cli("sequence", "-i", cur, "-r", fa, "-o", fq_b, "-s", seed, "--badread-error-model", ERR_MODEL, "--badread-qscore-model", QS_MODEL,
             "--badread-identity", "84,99,5.5", env=env)
    assert r.returncode == 0, r.stderr[-600:]
    assert fq_p.read_bytes() == dev_perfect
    assert fq_b.read_bytes() == dev_bad
