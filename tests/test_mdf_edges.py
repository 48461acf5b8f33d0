"""Boundary sweeps of the molecule transforms (tksm_amd/csrc/mdf_kernels.hip): truncation at every cut position, PCR beyond 32 cycles and
at its limits, molecule indices across 2^32, the segment edits at their edges.

The corpora of test_mdf_ops.py / test_core_modules.py / test_tail_noise.py are random draws, which leave these meetings to chance.  Here
the molecules are crafted (tests/mdf_edge_cases.py) and the parameters swept.  Every comparison is exact: MDF text against the
specifications (oracle/mdf_ops_oracle.py, tests/core_modules_spec.py, tests/noise_spec.py, tests/wgs_spec.py), read against read; and for
every transform one check that does NOT go through its specification: what the perfect reads of the output must be, said directly.
CPU part: the generator is deterministic, the sweep reaches every class of cut, the PCR refusal threshold."""
import json
import math
import os

import numpy as np
import pytest

from conftest import ERR_MODEL, GOLDEN, QS_MODEL

import core_modules_spec as cs
import mdf_edge_cases as ec
import mdf_ops_oracle as mo
import noise_spec as ns
import wgs_spec as ws

ELIMIT = 6
FIRST32 = 2**32 - 8                                                     # molecule 8 of a batch that starts here has index 2^32


# ------------------------------------------------------------------------------------------------ CPU
def test_case_generator_is_deterministic():
    assert ec.crafted_text() == ec.crafted_text() and ec.crafted_text(cb=True) == ec.crafted_text(cb=True) != ec.crafted_text()
    assert ec.pcr_templates_text() == ec.pcr_templates_text() and ec.pcr_small_text() == ec.pcr_small_text()
    assert ec.genome() == ec.genome() and ec.kde_lengths() == ec.kde_lengths() and ec.cut_lengths() == list(range(98, ec.max_size() + 3))
    mols = ec.crafted_molecules()
    assert 30 <= len(ec.PATTERNS) <= 60 and len({m["id"] for m in mols}) == len(mols)
    sizes = {mo.mol_size(m) for m in mols}
    assert min(sizes - {0}) == 101 and max(sizes) == 230 and 0 in sizes
    shapes = [[mo.seg_size(s) for s in m["segments"]] for m in mols]
    assert [] in shapes and [0, 0, 0] in shapes and any(len(x) == 1 and x[0] for x in shapes)               # no segment; empty only; single
    assert any(x[0] == 0 and sum(x) for x in shapes if x) and any(x[-1] == 0 and sum(x) for x in shapes if x)
    assert any(a == b == 0 and sum(x[:i]) and sum(x[i + 2:]) for x in shapes for i, (a, b) in enumerate(zip(x, x[1:])))      # doubled, inside
    assert any(s["chr"].startswith("ACGT"[:1]) and not s["chr"].startswith("chr") for m in mols for s in m["segments"])      # a literal
    assert any(m["id"].endswith("_2") for m in mols) and any(m["meta"] for m in mols)
    errs = [(mo.seg_size(s), [p for p, _ in s["errors"]]) for m in mols for s in m["segments"] if s["errors"]]
    assert any(p != sorted(p) for _, p in errs) and any(len(set(p)) < len(p) for _, p in errs)
    assert any(0 in p for _, p in errs) and any(sz - 1 in p for sz, p in errs) and all(max(p) < sz for sz, p in errs)
    assert {len(s["errors"]) for m in mols for s in m["segments"] if mo.seg_size(s)} == {0, 1, 2, 3}
    assert not any(s["errors"] for m in mols for s in m["segments"] if not mo.seg_size(s))


def test_truncation_sweep_reaches_every_class_of_cut():
    """Counted from the specification's outputs alone (mdf_edge_cases.coverage): every class of (molecule, cut) pair the kernels treat
    specially has at least 10 members, so a later edit of the generator cannot hollow the sweep out."""
    n = ec.coverage()
    print("\n".join(f"{c}: {k} pairs" for c, k in n.items()))
    assert set(n) == set(ec.CLASSES)
    for c, k in n.items():
        assert k >= 10, (c, k)


def test_deterministic_kde_model_draws_constants():
    """the model of mdf_edge_cases.kde_model gives TR=T,S for every molecule above 100 bases, whatever its index"""
    md = ec.crafted_molecules()[2]
    for T, S in ((37, 0.25), (0, 1.0), (113, 0.0), (64, 0.5)):
        model = mo.TruncationModel(ec.kde_model(T, S))
        assert {tuple(mo.trc_spec(md, g, 23, model=model)["meta"]["TR"]) for g in list(range(100)) + list(range(2**32 - 50, 2**32 + 50))} == \
            {(f"{T},{S:.2f}",)}


def test_pcr_refusal_threshold():
    """The q / A tables stop resolving the drop ratio long before they fail outright (1 - q[cycles - 1] IS the drop ratio, known to
    about 2^-53 / drop of itself): pcr_spec raises where the bound on the relative error of the divisors 1 - q[t], 1 - A[t] is above
    2^-24 (mo.pcr_table_error has the derivation, tksm_amd/csrc/mdf_ops.cpp pcr_tables the same recursion).  The case that used to come
    back empty is refused; BASELINE config 5 (20 cycles, Taq-setting1, 2e8 templates, target 2e8) is far inside."""
    mols = mo.stream_mdf(ec.pcr_templates_text(), unroll=True)
    with pytest.raises(mo.PcrUnresolved, match="56 cycles.*efficiency 1.0.*200 templates"):
        mo.pcr_spec(mols, 56, 1.0, 1e-3, 300, 5)
    er, eff = mo.PRESETS["Taq-setting1"]
    drop5 = 2e8 / (math.pow(1 + eff, 20) * 2e8)
    rel5 = mo.pcr_table_error(20, eff, drop5)
    print(f"config 5: drop ratio {drop5:.3g}, relative error bound {rel5:.3g}, limit {mo.PCR_TABLE_REL_ERR:.3g}")
    assert 2e-6 < drop5 < 5e-6 and rel5 * 100 < mo.PCR_TABLE_REL_ERR == 2.0 ** -24
    # the bound follows (5 / efficiency + 2) u / drop while the tables are far from saturated, and is monotone in the drop ratio
    assert 0.2 < rel5 / ((5 / eff + 2) * 2.0 ** -53 / drop5) < 1.5
    rels = [mo.pcr_table_error(30, 0.9, d) for d in (1e-3, 1e-5, 1e-7, 1e-9, 1e-11, 1e-13, 1e-15, 1e-17)]
    assert rels == sorted(rels) and rels[0] < 1e-11 and rels[-1] == math.inf
    # on the accepted side nothing changes: no cycles, no efficiency, a drop ratio clipped to 1, the tests' own parameters
    assert mo.pcr_table_error(3, 0.8, 0.0) == 0.0 and mo.pcr_spec([], 3, 0.8, 2e-3, 40, 5) == [] and mo.pcr_spec(mols[:5], 3, 0.8, 2e-3, 0, 5) == []
    for cycles, e, n, target in ((0, 0.9, 400, 100), (5, 0.0, 10, 10), (3, 0.56, 4, 700), (20, 0.88, 24_000, 300_000), (56, 0.15, 200, 400)):
        drop = min(1.0, target / (math.pow(1 + e, cycles) * n))
        assert mo.pcr_table_error(cycles, e, drop) < 1e-10, (cycles, e, n, target)


def _tags_fast(seed, g, stream, fmt):
    """cs.tag_draws_spec for a long format: the same rule (letter j = choice umulhi(word j % 4 of block j // 4, k)), one Philox call"""
    n, nb = len(fmt), (len(fmt) + 3) // 4
    w = cs.philox_np(seed, np.repeat(np.asarray(g, np.uint64), nb), stream, np.tile(np.arange(nb, dtype=np.uint64), len(g)))
    words = np.stack(w, 1).reshape(len(g), nb * 4)[:, :n]
    k = np.array([len(cs.IUPAC[c]) for c in fmt], np.uint64)
    table = np.zeros((256, 4), np.uint8)
    for c, opts in cs.IUPAC.items():
        table[ord(c), :len(opts)] = np.frombuffer(opts.encode(), np.uint8)
    pick = ((words * k[None, :]) >> np.uint64(32)).astype(np.int64)
    letters = table[np.frombuffer(fmt.encode(), np.uint8)[None, :], pick]
    return [bytes(r).decode() for r in letters]


def test_fast_tag_helper_is_the_specification():
    g = np.array([0, 7, 2**32 - 1, 2**32, 2**40 + 3], np.uint64)
    for fmt in ("N", "NNN", "NNNN", "NNNNN", "NRYKMSWBDHVACGTU" * 3 + "N"):
        assert _tags_fast(9, g, cs.ST_TAG3, fmt) == cs.tag_draws_spec(9, g, cs.ST_TAG3, fmt), fmt


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def es():
    from tksm_amd.sequence import Sequencer
    ref = ec.genome()
    s = Sequencer(0)
    for k, v in ref.items():
        s.add_contig(k, v)
    s.set_identity(84.0, 99.0, 5.5)
    s.load_error_model(ERR_MODEL)
    s.load_qscore_model(QS_MODEL)
    yield s, ref
    s.close()


def _reads(s, b):
    return [r.split(b"\n")[1].decode() for r in s.run(b, target="perfect", fastq=True, seed=1).records()]


def _revcomp(x):
    return x[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _text_of(s, out):
    try:
        return s.to_mdf_text(out)
    finally:
        out.free()


def _first_difference(got, want):
    g, w = got.splitlines(), want.splitlines()
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return f"line {i}: got {a[:200]!r}, want {b[:200]!r}"
    return f"{len(g)} lines against {len(w)}"


@pytest.fixture(scope="module")
def crafted(es):
    """the crafted batch on the device and the perfect reads of its molecules"""
    s, _ = es
    b = s.batch_from_mdf(ec.crafted_text())
    reads = _reads(s, b)
    assert len(reads) == len(ec.crafted_molecules()) and [len(r) for r in reads] == [mo.mol_size(m) for m in ec.crafted_molecules()]
    yield b, reads
    b.free()


# ---- 1. truncation
@pytest.mark.gpu
def test_truncation_at_every_cut_length(es, crafted):
    """normal=(L, 0): the post-truncation length is exactly L for every molecule; L from 98 (below the clamp) to past the largest
    molecule.  Text for text against the literal truncate() of the specification, `truncated=` comments included."""
    s, _ = es
    b, _ = crafted
    for L in ec.cut_lengths():
        got = _text_of(s, s.truncate(b, normal=(float(L), 0.0), seed=ec.SEED_3P, first_molecule_index=ec.FIRST))
        want = mo.write_mdf(ec.sweep_3p(L))
        assert got == want, (L, _first_difference(got, want))


@pytest.mark.gpu
def test_truncated_reads_are_prefixes_of_the_input_reads(es, crafted):
    """Not through the specification: with K = max(L, 100) the perfect read of a truncated molecule is the first K bases of the input
    molecule's read when the molecule is longer than K, the whole read otherwise (L == size included)."""
    s, _ = es
    b, before = crafted
    for L in ec.cut_lengths():
        out = s.truncate(b, normal=(float(L), 0.0), seed=ec.SEED_3P, first_molecule_index=ec.FIRST)
        after = _reads(s, out)
        out.free()
        K = max(L, 100)
        assert after == [x[:K] if len(x) > K else x for x in before], L


def _window(size, tl, side):
    """the two-pass rule written out: keep the first L1 bases, then -- on the flipped molecule -- the first L2 of what is left, i.e. its
    LAST L2 bases; each pass leaves the molecule alone when the length equals its size, never keeps fewer than 100, and cannot lengthen"""
    def keep(n, length):
        length = int(length)                                            # the double converts toward zero
        if length == n:
            return n
        return min(n, max(length, 100))
    s1 = keep(size, size - tl * side)
    s2 = keep(s1, s1 - tl * (1.0 - side))
    return s1 - s2, s1


@pytest.mark.gpu
@pytest.mark.parametrize("models_length", [False, True])
@pytest.mark.parametrize("side", ec.KDE_SIDES)
def test_truncation_of_both_ends_at_every_boundary(es, crafted, tmp_path, side, models_length):
    """A KDE model whose draws are the constants (T, S): 3' cut, then 5' cut on the flipped molecule, T over every segment boundary +- 1
    from either end.  Against the specification text for text (`truncated=`, `TR=`), and -- not through it -- the perfect read of the
    output is read[w0:w1] of the input with the window of _window()."""
    s, _ = es
    b, before = crafted
    for T in ec.kde_lengths():
        path = tmp_path / f"model_{T}.json"
        path.write_text(json.dumps(ec.kde_model(T, side)))
        out = s.truncate(b, kde_model=path, kde_models_length=models_length, seed=ec.SEED_KDE, first_molecule_index=ec.FIRST)
        after = _reads(s, out)
        got = _text_of(s, out)
        want = mo.write_mdf(ec.sweep_kde(T, side, models_length))
        assert got == want, (T, side, models_length, _first_difference(got, want))
        for x, y in zip(before, after):
            if len(x) > 100:                                            # (shorter ones read the model's first row, whose draw is not a constant)
                w0, w1 = _window(len(x), float(len(x) - T) if models_length else float(T), side)
                assert y == x[w0:w1], (T, side, models_length, len(x), w0, w1)
            else:
                assert y == x == ""


# ---- 2. PCR
def _molecule_table(text):
    """[(id, substitutions)] of MDF text"""
    out = []
    for line in text.splitlines():
        f = line.split("\t")
        if line.startswith("+"):
            out.append([f[0][1:], 0])
        elif f[4]:
            out[-1][1] += f[4].count(",") + 1
    return out


def _check_copies_against_templates(s, b_in, text_in, b_out, text_out):
    """Not through the specification: the perfect read of a copy has the length of its template's read and differs from it in at most as
    many positions as the copy has substitutions; the template is the id before the first '.'"""
    templates = dict(zip([m["id"] for m in mo.stream_mdf(text_in, unroll=True)], zip(_reads(s, b_in), [n for _, n in _molecule_table(s.to_mdf_text(b_in))])))
    copies = _reads(s, b_out)
    table = _molecule_table(text_out)
    assert len(copies) == len(table)
    for (cid, n_subs), y in zip(table, copies):
        x, n_own = templates[cid.split(".")[0]]
        assert len(y) == len(x) and n_subs >= n_own, cid
        assert sum(a != c for a, c in zip(x, y)) <= n_subs, cid


@pytest.mark.gpu
@pytest.mark.parametrize("cycles,eff,min_deep", [(33, 0.3, 32), (40, 0.25, 32), (56, 0.15, 50)])
def test_pcr_beyond_32_cycles(es, cycles, eff, min_deep):
    """Copy steps 32..55: the upper half of the path mask in the Philox stream word, 1ull << t, the id writer.  200 templates (an empty
    segment in the middle, a minus-strand segment with a substitution), target 400; whole and in template slices."""
    s, _ = es
    text = ec.pcr_templates_text()
    mols = mo.stream_mdf(text, unroll=True)
    spec = mo.pcr_spec(mols, cycles, eff, 1e-3, 400, 5)
    steps = [[int(x) for x in m["id"].split(".")[1:]] for m in spec]
    deep = sum(max(p) >= 32 for p in steps)
    print(f"{cycles} cycles: {len(spec)} molecules, {deep} with a copy step >= 32, deepest step {max(max(p) for p in steps)}")
    assert deep >= 100 and max(max(p) for p in steps) >= min_deep and 350 < len(spec) < 450
    b = s.batch_from_mdf(text)
    out = s.pcr(b, cycles, 400, error_rate=1e-3, efficiency=eff, seed=5)
    got, want = s.to_mdf_text(out), mo.write_mdf(spec)
    assert got == want, _first_difference(got, want)
    _check_copies_against_templates(s, b, text, out, got)
    out.free()
    parts = [_text_of(s, s.pcr(b, cycles, 400, error_rate=1e-3, efficiency=eff, seed=5, templates=(lo, min(200, lo + 64)))) for lo in range(0, 200, 64)]
    assert "".join(parts) == got
    counts = s.pcr_template_counts(b, cycles, 400, 1e-3, eff, seed=5)
    assert [int(c) for c in counts] == [sum(m["id"].split(".")[0] == f"t{u}" for m in spec) for u in range(200)]
    b.free()


@pytest.mark.gpu
def test_pcr_refusals_leave_the_context_usable(es):
    """57 cycles; more than 32 substitutions per copy; a drop ratio the tables do not resolve (56 cycles at efficiency 1 on 200
    templates used to come back EMPTY where the reference writes about 300 copies): TKSMSEQ_ELIMIT with a message that says why, from
    tksmseq_pcr and from tksmseq_pcr_template_counts; the same batch then works."""
    from tksm_amd.sequence import TksmSeqError
    s, _ = es
    text = ec.pcr_templates_text()
    b = s.batch_from_mdf(text)
    for call in (lambda **kw: s.pcr(b, seed=5, **kw), lambda cycles, target_count, error_rate, efficiency: s.pcr_template_counts(b, cycles, target_count, error_rate, efficiency, seed=5)):
        with pytest.raises(TksmSeqError, match="between 0 and 56 cycles") as e:
            call(cycles=57, target_count=400, error_rate=1e-3, efficiency=0.15)
        assert e.value.code == ELIMIT
        with pytest.raises(TksmSeqError, match=r"56 cycles at efficiency 1 on 200 templates") as e:
            call(cycles=56, target_count=300, error_rate=1e-3, efficiency=1.0)
        assert e.value.code == ELIMIT and "drop ratio" in str(e.value)
    with pytest.raises(mo.PcrUnresolved):
        mo.pcr_spec(mo.stream_mdf(text, unroll=True), 56, 1.0, 1e-3, 300, 5)
    # the bound's recursion exists twice (pcr_setup, mo.pcr_table_error): on both sides of the threshold the library refuses exactly where
    # the specification raises -- efficiency 1, target 300: the bound is 2/3 of the limit at 27 cycles, 4/3 at 28 -- and an accepted call
    # next to the threshold still equals the specification
    mols = mo.stream_mdf(text, unroll=True)
    verdicts = []
    for cycles in range(24, 32):
        rel = mo.pcr_table_error(cycles, 1.0, 300 / (2.0 ** cycles * 200))
        assert not 0.9 < rel / mo.PCR_TABLE_REL_ERR < 1.1, cycles                          # (no case sits where a last bit could decide)
        try:
            got = _text_of(s, s.pcr(b, cycles, 300, error_rate=1e-3, efficiency=1.0, seed=5))
            verdicts.append(True)
            assert rel <= mo.PCR_TABLE_REL_ERR, cycles
            want = mo.write_mdf(mo.pcr_spec(mols, cycles, 1.0, 1e-3, 300, 5))
            assert got == want and got.count("\n+") > 200, (cycles, _first_difference(got, want))
        except TksmSeqError as e:
            verdicts.append(False)
            assert e.code == ELIMIT and rel > mo.PCR_TABLE_REL_ERR, cycles
            with pytest.raises(mo.PcrUnresolved):
                mo.pcr_spec(mols, cycles, 1.0, 1e-3, 300, 5)
    assert verdicts == [True] * 4 + [False] * 4
    # a drop ratio of 0 -- a molecule count of 0, no templates -- and efficiency 0 are no refusals: nothing is written
    e0 = s.batch_from_mdf("")
    for bb, kw in ((b, dict(cycles=5, target_count=0, efficiency=0.9)), (b, dict(cycles=5, target_count=300, efficiency=0.0)), (e0, dict(cycles=3, target_count=40, efficiency=0.8))):
        assert _text_of(s, s.pcr(bb, error_rate=1e-3, seed=5, **kw)) == ""
    e0.free()
    got = _text_of(s, s.pcr(b, 3, 300, error_rate=1e-3, efficiency=0.9, seed=5))
    assert got == mo.write_mdf(mo.pcr_spec(mo.stream_mdf(text, unroll=True), 3, 0.9, 1e-3, 300, 5)) and got.count("\n+") > 200
    b.free()


@pytest.mark.gpu
def test_pcr_at_the_substitution_cap(es):
    """350-base templates: error rate 0.06 is 28 substitutions per copy event (every copy carries 29 or 57 with its template's own), compared
    exactly; 0.08 would be 37 and is refused, by tksmseq_pcr and by tksmseq_pcr_template_counts, after which 0.06 still works."""
    from tksm_amd.sequence import TksmSeqError
    s, _ = es
    text = ec.pcr_long_templates_text()
    mols = mo.stream_mdf(text, unroll=True)
    b = s.batch_from_mdf(text)
    with pytest.raises(TksmSeqError, match="substitutions per copy") as e:
        s.pcr(b, 2, 30, error_rate=0.08, efficiency=0.9, seed=3)
    assert e.value.code == ELIMIT
    with pytest.raises(TksmSeqError, match="substitutions per copy") as e:
        s.pcr_template_counts(b, 2, 30, 0.08, 0.9, seed=3)
    assert e.value.code == ELIMIT
    spec = mo.pcr_spec(mols, 2, 0.9, 0.06, 30, 3)
    per = [sum(len(x["errors"]) for x in m["segments"]) for m in spec]
    assert set(per) == {29, 57} and len(spec) > 15
    out = s.pcr(b, 2, 30, error_rate=0.06, efficiency=0.9, seed=3)
    got, want = s.to_mdf_text(out), mo.write_mdf(spec)
    assert got == want, _first_difference(got, want)
    _check_copies_against_templates(s, b, text, out, got)
    out.free(); b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("error_rate", [0.75, 0.0])
def test_pcr_of_tiny_molecules(es, error_rate):
    """molecules of 0..5 bases with empty segments: at error rate 0.75 the substitution rate is 1, so every base of every copy is
    substituted (count = size < the draw, the duplicate-rejection loop visits the whole molecule); size 0; add_error over empty segments"""
    s, _ = es
    text = ec.pcr_small_text()
    mols = mo.stream_mdf(text, unroll=True)
    spec = mo.pcr_spec(mols, 3, 0.8, error_rate, 40, 7)
    assert len(spec) > 20 and any(not mo.mol_size(m) for m in spec)
    if error_rate:
        for m in spec:
            own = sum(len(x["errors"]) for x in mols[[t["id"] for t in mols].index(m["id"].split(".")[0])]["segments"])
            assert sum(len(x["errors"]) for x in m["segments"]) == own + mo.mol_size(m) * (m["id"].count("."))
    b = s.batch_from_mdf(text)
    out = s.pcr(b, 3, 40, error_rate=error_rate, efficiency=0.8, seed=7)
    got, want = s.to_mdf_text(out), mo.write_mdf(spec)
    assert got == want, _first_difference(got, want)
    _check_copies_against_templates(s, b, text, out, got)
    out.free(); b.free()


# ---- 4. indices across 2^32
def _halves():
    k = 7                                                              # patterns in the first half: its 7 molecules end below 2^32
    first, second = ec.INDEX_PATTERNS[:k], ec.INDEX_PATTERNS[k:]
    return ec.crafted_text(only=first), ec.crafted_text(only=second)


TRANSFORMS = {
    "truncate normal": (lambda s, b, g: s.truncate(b, normal=(120.0, 40.0), seed=17, first_molecule_index=g),
                        lambda mols, g: [mo.trc_spec(md, g + i, 17, normal=(120.0, 40.0)) for i, md in enumerate(mols)]),
    "truncate kde": (lambda s, b, g: s.truncate(b, kde_model=os.path.join(GOLDEN, "kde_truncation_model.json"), seed=29, first_molecule_index=g),
                     lambda mols, g: [mo.trc_spec(md, g + i, 29, model=_golden_model()) for i, md in enumerate(mols)]),
    "polya": (lambda s, b, g: s.polya(b, normal=(15.0, 7.5), seed=17, first_molecule_index=g), lambda mols, g: cs.polya_spec(mols, 17, "normal", 15.0, 7.5, first=g)),
    "tag": (lambda s, b, g: s.tag(b, format5="NRYKMSWBDHVN", format3="10", seed=9, first_molecule_index=g),
            lambda mols, g: cs.tag_spec(mols, 9, "NRYKMSWBDHVN", "10", first=g)),
    "flip": (lambda s, b, g: s.flip(b, 0.5, seed=5, first_molecule_index=g), lambda mols, g: cs.flip_spec(mols, 5, 0.5, first=g)),
    "noise random": (lambda s, b, g: s.append_noise(b, "normal", 40.0, 25.0, alphabet="AGTC", seed=11, first=g),
                     lambda mols, g: ns.noise_spec(mols, 11, ns.NORMAL, 40.0, 25.0, False, 0.5, "AGTC", first=g)),
    "noise palindromic": (lambda s, b, g: s.append_noise(b, "normal", 150.0, 120.0, palindromic=True, error_rate=0.5, seed=11, first=g),
                          lambda mols, g: ns.noise_spec(mols, 11, ns.NORMAL, 150.0, 120.0, True, 0.5, "AGTC", first=g)),
}


def _golden_model():
    return mo.TruncationModel(json.load(open(os.path.join(GOLDEN, "kde_truncation_model.json"))))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_molecule_indices_across_2_to_the_32(es, name):
    """philox_mol keys on (low word, high word) of the 64-bit molecule index: a batch whose indices run from 2^32 - 8 to 2^32 + 12 against
    the specification, and as two halves with matching first indices.  The specification itself says that the molecules above 2^32
    do not come out as those at index & 0xffffffff would -- a (uint32_t) slipped into the key cannot pass."""
    s, _ = es
    run, spec = TRANSFORMS[name]
    text = ec.crafted_text(only=ec.INDEX_PATTERNS)
    mols = mo.stream_mdf(text, unroll=True)
    assert 16 <= len(mols) <= 32 and any(m["id"].endswith("_1") for m in mols) and any(not x["chr"].startswith("chr") for m in mols for x in m["segments"])
    want = mo.write_mdf(spec(mols, FIRST32))
    assert mo.write_mdf(spec(mols[8:], 2**32)) != mo.write_mdf(spec(mols[8:], 0))
    b = s.batch_from_mdf(text)
    got = _text_of(s, run(s, b, FIRST32))
    b.free()
    assert got == want, _first_difference(got, want)
    parts, g = [], FIRST32
    for half in _halves():
        b = s.batch_from_mdf(half)
        parts.append(_text_of(s, run(s, b, g)))
        g += b.n_reads
        b.free()
    assert g == FIRST32 + len(mols) and "".join(parts) == got


@pytest.mark.gpu
def test_wgs_candidates_across_2_to_the_32(es):
    s, ref = es
    contigs = [(k, len(v)) for k, v in ref.items()]
    first = 2**32 - 100
    want, st_want = ws.wgs_spec(42, contigs, ws.NORMAL, 300.0, 150.0, base_count=10**9, first_candidate=first, n_candidates=200)
    assert want.count("\n+") > 150
    # the candidates from 2^32 on are not those from 0 on
    assert ws.wgs_spec(42, contigs, ws.NORMAL, 300.0, 150.0, base_count=10**9, first_candidate=2**32, n_candidates=100)[0] != \
        ws.wgs_spec(42, contigs, ws.NORMAL, 300.0, 150.0, base_count=10**9, first_candidate=0, n_candidates=100)[0]
    batch, st = s.wgs("normal", 300.0, 150.0, base_count=10**9, seed=42, first_candidate=first, n_candidates=200)
    got = _text_of(s, batch)
    assert got == want, _first_difference(got, want)
    assert st == st_want and st["next_candidate"] == 2**32 + 100


@pytest.mark.gpu
@pytest.mark.parametrize("force_slow", ["0", "1"])
@pytest.mark.parametrize("first,stride", [(2**32 - 5, 3), (2**40 + 1, 2**31)])
def test_read_indices_across_2_to_the_32(po, oracle_models, monkeypatch, first, stride, force_slow):
    """Seq's first_read_index / stride: Badread and perfect records against the oracle at read indices beyond 32 bits, on both kernel
    routes; the oracle's records at those indices are not the ones at index & 0xffffffff.  TKSMSEQ_FORCE_SLOW is read when a context is
    created, so each case makes its own context after setting it; that the Badread run took the other route shows in its diagnostics
    (the fast pipeline counts its rounds, the wave-wide kernel has none), and the perfect run's route hangs on the same flag."""
    from tksm_amd.sequence import Sequencer
    monkeypatch.setenv("TKSMSEQ_FORCE_SLOW", force_slow)
    ref = ec.genome()
    s = Sequencer(0)
    try:
        for k, v in ref.items():
            s.add_contig(k, v)
        s.set_identity(84.0, 99.0, 5.5)
        s.load_error_model(ERR_MODEL)
        s.load_qscore_model(QS_MODEL)
        _read_indices_case(s, ref, po, oracle_models, first, stride, force_slow)
    finally:
        s.close()


def _read_indices_case(s, ref, po, oracle_models, first, stride, force_slow):
    text = ec.crafted_text(only=ec.INDEX_PATTERNS)
    ident = po.Identities(84.0, 5.5, 99.0)
    em, qm = oracle_models["em"], oracle_models["qm"]
    gen = list(po.mdf_generator(text.splitlines(keepends=True)))
    b = s.batch_from_mdf(text)
    bad = s.run(b, target="badread", fastq=True, compute_qual=True, seed=9, first_read_index=first, stride=stride).records()
    rounds = s.run_diagnostics()["rounds"]
    assert (rounds == 0) == (force_slow == "1"), (force_slow, rounds)
    perfect = s.run(b, target="perfect", fastq=True, seed=9, first_read_index=first, stride=stride).records()
    b.free()
    assert len(gen) == len(bad) == len(perfect) >= 16
    differs = 0
    for i, (mid, ivs) in enumerate(gen):
        raw, idx = po.splice(ref, ivs), first + i * stride
        want_bad = po.badread_record(True, 9, idx, raw, ident, em, qm, True, mid)[0]
        want_perfect = po.perfect_record(True, 9, idx, raw, mid)
        assert bad[i] == want_bad, (i, mid, idx)
        assert perfect[i] == want_perfect, (i, mid, idx)
        if idx >= 2**32:
            differs += want_bad != po.badread_record(True, 9, idx & 0xffffffff, raw, ident, em, qm, True, mid)[0]
            differs += want_perfect != po.perfect_record(True, 9, idx & 0xffffffff, raw, mid)
    assert differs >= len(gen)


# ---- 5. segment edits
IUPAC_SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT",
              "V": "ACG", "N": "ACGT"}


@pytest.fixture(scope="module")
def crafted_cb(es):
    s, _ = es
    b = s.batch_from_mdf(ec.crafted_text(cb=True))
    yield b, ec.crafted_molecules(True), _reads(s, b)
    b.free()


@pytest.mark.gpu
def test_segment_edits_of_the_crafted_molecules(es, crafted_cb):
    """molecules without segments, of empty segments only, literals, depth > 1 through polyA, tag, scb and flip"""
    s, _ = es
    b, mols, _ = crafted_cb
    mols = list(mols)
    cases = [(s.polya(b, normal=(15.0, 7.5), seed=17, first_molecule_index=5), cs.polya_spec(mols, 17, "normal", 15.0, 7.5, first=5)),
             (s.tag(b, format5="NNNNN", format3="ACG", seed=9, first_molecule_index=5), cs.tag_spec(mols, 9, "NNNNN", "ACG", first=5)),
             (s.scb(b), cs.scb_spec(mols)), (s.scb(b, keep_meta_barcodes=True), cs.scb_spec(mols, True)),
             (s.flip(b, 0.5, seed=5, first_molecule_index=5), cs.flip_spec(mols, 5, 0.5, first=5)),
             (s.flip(b, 1.0, seed=5), cs.flip_spec(mols, 5, 1.0))]
    for k, (out, want) in enumerate(cases):
        got, want = _text_of(s, out), mo.write_mdf(want)
        assert got == want, (k, _first_difference(got, want))


@pytest.mark.gpu
def test_tag_formats_around_the_philox_block(es, crafted_cb):
    """format lengths 1, 3, 4, 5, 8, 9 (a Philox block is 4 words: tag_draw's j & 3), a format whose unknown letters sit at positions 3, 4
    and 5 (they add nothing, and the word index counts the remaining letters), on both ends.  Not through the specification: the perfect
    read is prefix + input read + suffix, each added letter one its IUPAC format letter allows."""
    s, _ = es
    b, mols, before = crafted_cb
    mols = list(mols)
    mixed = "NRYxz-KMSN"
    assert [j for j, c in enumerate(mixed) if c not in cs.IUPAC] == [3, 4, 5]
    for f5, f3 in [("N" * n, "") for n in (1, 3, 4, 5, 8, 9)] + [("", "N" * n) for n in (1, 3, 4, 5, 8, 9)] + [(mixed, ""), ("NNN", mixed), ("BDHVN", "NNNNNNNNN")]:
        out = s.tag(b, format5=f5, format3=f3, seed=9, first_molecule_index=3)
        after = _reads(s, out)
        got, want = _text_of(s, out), mo.write_mdf(cs.tag_spec(mols, 9, f5, f3, first=3))
        assert got == want, (f5, f3, _first_difference(got, want))
        k5, k3 = [c for c in f5 if c in IUPAC_SETS], [c for c in f3 if c in IUPAC_SETS]
        for x, y in zip(before, after):
            assert len(y) == len(k5) + len(x) + len(k3) and y[len(k5):len(k5) + len(x)] == x, (f5, f3)
            assert all(c in IUPAC_SETS[f] for c, f in zip(y[:len(k5)], k5)) and all(c in IUPAC_SETS[f] for c, f in zip(y[len(k5) + len(x):], k3)), (f5, f3)
    # the draws are not all alike: the 9 letters of one molecule, and the first letter over the molecules
    tags = {l.split("\t")[0] for l in got.splitlines() if l.endswith("\t0\t9\t+\t")}
    assert len(tags) > len(mols) // 2 and all(len(set(t)) > 1 for t in list(tags)[:5])


@pytest.mark.gpu
def test_tag_format_length_limit(es):
    """2^20 letters are accepted (a 2-molecule batch, across molecule index 2^32), 2^20 + 1 refused"""
    from tksm_amd.sequence import TksmSeqError
    s, _ = es
    text = ec.crafted_text(only=(2,)) + "+pair\t1\t\nchr1\t10\t40\t-\t3A\n"
    mols = mo.stream_mdf(text, unroll=True)
    assert len(mols) == 2
    b = s.batch_from_mdf(text)
    n = 1 << 20
    out = s.tag(b, format3="N" * n, seed=4, first_molecule_index=2**32 - 1)
    assert out.n_reads == 2
    got = _text_of(s, out)
    tags = _tags_fast(4, np.array([2**32 - 1, 2**32], np.uint64), cs.ST_TAG3, "N" * n)
    want = "".join(mo.write_mdf([md]) + f"{t}\t0\t{n}\t+\t\n" for md, t in zip(mols, tags))
    assert len(got) == len(want) and got == want
    for kw in (dict(format3="N" * (n + 1)), dict(format5="A" * (n + 1), format3="N")):
        with pytest.raises(TksmSeqError, match="1048576") as e:
            s.tag(b, seed=4, **kw)
        assert e.value.code == ELIMIT
    assert _text_of(s, s.tag(b, format5="ACG", seed=4)) == mo.write_mdf(cs.tag_spec(mols, 4, "ACG", ""))
    b.free()


POLYA_CASES = [(dict(normal=(15.0, 7.5)), 0, 0), (dict(normal=(15.0, 7.5)), 7, 7), (dict(poisson=4.0), 7, 7),
               (dict(poisson=float(np.nextafter(10.0, 0.0))), 0, 5000), (dict(poisson=10.0), 0, 5000), (dict(poisson=10.5), 0, 5000),
               (dict(gamma=(float(np.nextafter(1.0, 0.0)), 12.0)), 0, 5000), (dict(gamma=(1.0, 12.0)), 0, 5000), (dict(gamma=(0.05, 400.0)), 0, 5000),
               (dict(weibull=(0.1, 20.0)), 3, 900), (dict(normal=(15.0, 7.5)), 0, 1 << 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("kw,lo,hi", POLYA_CASES)
def test_polya_at_its_edges(es, crafted_cb, kw, lo, hi):
    """min == max (0 and 7); the Poisson sampler on both sides of its switch at lambda = 10; gamma shapes on both sides of 1 and far
    below; a Weibull shape whose draws are astronomically large (the clamp); --max-length 2^20.  Against the specification, and -- not
    through it -- every perfect read is the input read + 'A' x k with min <= k <= max."""
    s, _ = es
    b, mols, before = crafted_cb
    (name, v), = kw.items()
    a, bb = (v, 0.0) if name == "poisson" else v
    draws = cs.polya_draws_spec(17, np.arange(9, 9 + len(mols), dtype=np.uint64), name, a, bb)
    if name == "weibull":
        assert (draws > 1e4).sum() >= 5 and (draws < lo).sum() >= 5 and np.isfinite(draws).all()      # both sides of the clamp are reached
    out = s.polya(b, **kw, min_length=lo, max_length=hi, seed=17, first_molecule_index=9)
    after = _reads(s, out)
    got, want = _text_of(s, out), mo.write_mdf(cs.polya_spec(list(mols), 17, name, a, bb, lo, hi, first=9))
    assert got == want, (kw, lo, hi, _first_difference(got, want))
    ks = []
    for x, y in zip(before, after):
        assert y.startswith(x) and set(y[len(x):]) <= {"A"} and lo <= len(y) - len(x) <= hi, (kw, lo, hi)
        ks.append(len(y) - len(x))
    assert lo == hi or len(set(ks)) > 3


@pytest.mark.gpu
def test_polya_max_length_limit(es, crafted_cb):
    from tksm_amd.sequence import TksmSeqError
    s, _ = es
    b, _, _ = crafted_cb
    with pytest.raises(TksmSeqError, match="1048576") as e:
        s.polya(b, normal=(15.0, 7.5), max_length=(1 << 20) + 1)
    assert e.value.code == ELIMIT


@pytest.mark.gpu
def test_flipped_reads_are_reverse_complements(es, crafted_cb):
    """Not through the specification: flip with probability 1 reverses the segment order and toggles every strand, so the perfect read of
    every molecule (literals, minus strands, substitutions, empty segments, no segments) is the reverse complement of the input's"""
    s, _ = es
    b, _, before = crafted_cb
    out = s.flip(b, 1.0, seed=5)
    after = _reads(s, out)
    out.free()
    assert after == [_revcomp(x) for x in before] and sum(x != _revcomp(x) for x in before) > 40
    out = s.flip(b, 0.0, seed=5)
    assert _reads(s, out) == before
    out.free()
