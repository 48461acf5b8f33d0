"""mutate on the device (-m gpu): tksmseq_mutate against tests/mutate_spec.py as MDF text, byte for byte; perfect reads of mutated molecules
against the string model of the mutated contig (not through the specification); `tksm mutate` on files against the library's text."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import mdf_edge_cases as ec
import mdf_ops_oracle as mo
import mutate_spec as ms

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
SMALL = ms.random_genome(np.random.RandomState(77), 3, 40, 60)           # c0 .. c2


@pytest.fixture(scope="module")
def genome():
    g = dict(ec.genome())
    g.update(SMALL)
    return g


@pytest.fixture(scope="module")
def dev(genome):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    for k, v in genome.items():
        s.add_contig(k, v)
    yield s
    s.close()


@pytest.fixture(scope="module")
def bare():
    """a context without a reference: every contig name of a parsed batch is a literal"""
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    yield s
    s.close()


def _mutate_text(s, mdf, table, **kw):
    """(a context without contigs parses as the modules do: names stay literals, substitution positions are not checked against them)"""
    b = s.batch_from_mdf(mdf) if s.reference_info()["n_contigs"] else s.molecules_from_mdf(mdf)
    v = s.load_variants(text=table)
    try:
        out = s.mutate(b, v, **kw)
        try:
            return s.to_mdf_text(out)
        finally:
            out.free()
    finally:
        b.free()
        v.close()


def _spec_text(mdf, table):
    return mo.write_mdf(ms.mutate_spec(mo.stream_mdf(mdf, unroll=True), ms.normal_form(ms.parse_variants(table))[0]))


@pytest.fixture(scope="module")
def crafted():
    """the crafted corpus, its generated tables and the specification's text for each: computed once, read by the tests"""
    mdf = ec.crafted_text()
    tables = ms.crafted_tables(ec.crafted_molecules())
    return mdf, tables, [_spec_text(mdf, t) for t in tables]


def test_crafted_corpus_equals_the_spec_with_and_without_a_reference(dev, bare, crafted):
    mdf, tables, want = crafted
    for k, (table, w) in enumerate(zip(tables, want)):
        assert _mutate_text(dev, mdf, table) == w, k
        assert _mutate_text(bare, mdf, table) == w, k
    plain = "".join((l.rsplit("\t", 1)[0] + "\t\n") if l.startswith("+") else l for l in want[0].splitlines(keepends=True))
    assert _mutate_text(dev, mdf, tables[0], comments=False) == plain


def _random_corpus(n, seed):
    rs = np.random.RandomState(seed)
    contigs = {k: len(v) for k, v in SMALL.items()}
    contigs.update({lit: len(lit) for lit in ms.RANDOM_LITERALS})
    return ms.random_molecules(rs, SMALL, list(ms.RANDOM_LITERALS), n), ms.random_table(rs, contigs, 60)


@pytest.mark.parametrize("n", [129, 1000])
def test_random_corpus_equals_the_spec(dev, bare, n):
    mdf, table = _random_corpus(n, n)
    mols = mo.stream_mdf(mdf, unroll=True)
    assert len(mols) % 128 != 0 and len(mols) > 128
    want = _spec_text(mdf, table)
    assert _mutate_text(dev, mdf, table) == want
    assert _mutate_text(bare, mdf, table) == want
    # the same batch given in two halves equals the whole
    records = mdf.split("+")[1:]
    half = ["+" + "+".join(records[:len(records) // 2]), "+" + "+".join(records[len(records) // 2:])]
    assert "".join(half) == mdf
    assert "".join(_mutate_text(dev, h, table) for h in half) == want


def _sweep_mdf():
    """segments of 40 bases every 25 from 900 on, both strands, on chr1 (and a few on chr2, which the small tables do not name)"""
    out = []
    for j in range(28):
        out.append(f"+s{j}\t1\t\nchr1\t{900 + 25 * j}\t{940 + 25 * j}\t{'+-'[j & 1]}\t{'5A,39C' if j % 3 == 0 else ''}\n")
        if j % 7 == 0:
            out.append(f"chr2\t{900 + 25 * j}\t{940 + 25 * j}\t+\t\n")
    return "".join(out)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_tables_of_k_ranges_and_points_per_contig(dev, k):
    """the ends of the binary searches: k deleted ranges and k points on the contig, segments in front of, on, between and behind them"""
    table = "".join(f"chr1\t{1000 + 150 * i}\t{1012 + 150 * i}\nchr1\t{1060 + 150 * i}\t{('G', '.TT', 'CA')[i]}\n" for i in range(k)) or "chr2\t5\t5\n"
    mdf = _sweep_mdf()
    assert _mutate_text(dev, mdf, table) == _spec_text(mdf, table)
    only_ranges = "".join(l for l in table.splitlines(keepends=True) if l.split()[2].isdigit())
    only_points = "".join(l for l in table.splitlines(keepends=True) if not l.split()[2].isdigit())
    for t in (only_ranges, only_points):
        assert _mutate_text(dev, mdf, t) == _spec_text(mdf, t)


def _long_molecules(rs, n, span, subs):
    out = []
    for i in range(n):
        out.append(f"+L{i}\t1\t\n")
        for _ in range(rs.randint(1, 4)):
            s = int(rs.randint(0, span))
            e = s + int(rs.randint(50, 600))
            md = ",".join(f"{int(rs.randint(0, e - s))}{'ACGT'[rs.randint(4)]}" for _ in range(rs.randint(0, 3))) if subs else ""
            out.append(f"chr{rs.randint(1, 3)}\t{s}\t{e}\t{'+-'[rs.randint(2)]}\t{md}\n")
    return "".join(out)


def test_table_of_a_few_thousand_rows(dev):
    rs = np.random.RandomState(9)
    table = ms.random_table(rs, {"chr1": 60_000, "chr2": 60_000}, 4000, max_ins=6)
    mdf = _long_molecules(rs, 150, 59_000, True)
    got = _mutate_text(dev, mdf, table)
    assert got == _spec_text(mdf, table)
    assert got.count("\n") > 2 * mdf.count("\n")                         # (about a variant per 30 bases: most segments are cut)


def test_perfect_reads_equal_the_slices_of_the_mutated_contig(dev, genome):
    """NOT through the specification: single- and multi-segment molecules without substitutions of their own, mutated on the device and
    sequenced --perfect, against mutated_contig's text -- reverse-complemented for minus segments"""
    rs = np.random.RandomState(4)
    table = ms.random_table(rs, {"chr1": 20_000, "chr2": 20_000}, 400, max_ins=8) + open(os.path.join(GOLDEN, "mutate", "variants.tsv")).read()
    mdf = _long_molecules(rs, 120, 19_000, False) + "+g0\t1\t\nchr1\t990\t1310\t+\t\n+g1\t1\t\nchr1\t990\t1310\t-\t\nchr2\t495\t515\t-\t\n"
    rows = ms.parse_variants(table)
    mols = mo.stream_mdf(mdf, unroll=True)
    b, v = dev.batch_from_mdf(mdf), dev.load_variants(text=table)
    out = dev.mutate(b, v)
    got = [r.split(b"\n")[1].decode() for r in dev.run(out, target="perfect", fastq=False, seed=1).records()]
    for x in (out, b):
        x.free()
    v.close()
    want = [ms.expected_read(md, genome, rows) for md in mols]
    assert len(got) == len(want) == 122
    for g, w, md in zip(got, want, mols):
        assert g == w, md["id"]
    assert sum(g != ms.splice(md, genome) for g, md in zip(got, mols)) > 60      # (the table does change them)


def test_empty_table_and_empty_batch(dev):
    mdf = ec.crafted_text()
    assert _mutate_text(dev, mdf, "") == mo.write_mdf(mo.stream_mdf(mdf, unroll=True))
    v = dev.load_variants(text="")
    assert (v.rows, v.snvs, v.insertions, v.deletions, v.deleted_ranges, v.dropped_points) == (0, 0, 0, 0, 0, 0)
    v.close()
    assert _mutate_text(dev, "", "chr1\t5\tA\nchr1\t7\t.ACGT\n") == ""
    v = dev.load_variants(path=os.path.join(GOLDEN, "mutate", "variants.tsv"))
    assert (v.rows, v.snvs, v.insertions, v.deletions, v.deleted_ranges, v.dropped_points) == (20, 6, 6, 8, 5, 2)
    v.close()


def test_a_molecule_deleted_whole_stays_without_segments(dev):
    mdf = "+gone\t1\tx=1;\nchr1\t100\t150\t+\t3A\nchr2\t200\t260\t-\t\n+kept\t1\t\nchr1\t140\t160\t+\t\n"
    table = "chr1\t90\t150\nchr2\t200\t230\nchr2\t260\t225\n"
    text = _mutate_text(dev, mdf, table)
    assert text == "+gone\t1\tx=1;\n+kept\t1\t\nchr1\t150\t160\t+\t\n" == _spec_text(mdf, table)
    b, v = dev.batch_from_mdf(mdf), dev.load_variants(text=table)
    out = dev.mutate(b, v)
    reads = [r.split(b"\n")[1] for r in dev.run(out, target="perfect", fastq=False, seed=1).records()]
    assert reads == [b"", ec.genome()["chr1"][150:160].encode()]
    for x in (out, b):
        x.free()
    v.close()


def test_one_table_on_two_contexts_and_after_the_reference_changed(bare, crafted):
    """a table may be used from several contexts; a context rebuilds its device form when its reference has changed"""
    from tksm_amd.sequence import Sequencer
    mdf, tables, want = crafted
    s = Sequencer(0)
    v = s.load_variants(text=tables[3])
    try:
        for ctx in (s, bare, s):
            b = ctx.molecules_from_mdf(mdf)
            out = ctx.mutate(b, v)
            assert ctx.to_mdf_text(out) == want[3]
            out.free(); b.free()
        for k, seq in ec.genome().items():                               # the names were literals so far; now they are contigs
            s.add_contig(k, seq)
        b = s.batch_from_mdf(mdf)
        out = s.mutate(b, v)
        assert s.to_mdf_text(out) == want[3]
        out.free(); b.free()
    finally:
        v.close()
        s.close()


def test_module_equals_the_library(dev, crafted, tmp_path):
    mdf, tables, want = crafted
    rmdf, rtable = _random_corpus(1000, 1000)
    for name, m, t, w in (("crafted", mdf, tables[10], want[10]), ("random", rmdf, rtable, _mutate_text(dev, rmdf, rtable))):
        (tmp_path / f"{name}.mdf").write_text(m)
        (tmp_path / f"{name}.tsv").write_text(t)
        for extra in ((), ("--batch-bytes", "2000")):
            o = tmp_path / f"{name}{len(extra)}.mdf"
            r = subprocess.run([EXE, "mutate", "-i", str(tmp_path / f"{name}.mdf"), "-o", str(o), "-t", str(tmp_path / f"{name}.tsv"), *extra],
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            assert o.read_text() == w, (name, extra)


def test_an_insertion_above_the_limit_is_refused(dev):
    from tksm_amd import _lib
    from tksm_amd.sequence import TksmSeqError
    with pytest.raises(TksmSeqError) as e:
        dev.load_variants(text="chr1\t5\t." + "A" * ((1 << 20) + 1) + "\n")
    assert e.value.code == _lib.ELIMIT and "<text>:1:" in str(e.value)
    dev.load_variants(text="chr1\t5\t." + "A" * (1 << 20) + "\n").close()
