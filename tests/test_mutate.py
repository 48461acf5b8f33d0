"""CPU tests of mutate: the specification against an independent string model and against the reference's apply_mods restated, the
table reader of the library (no device), the exports and the `tksm mutate` argument handling.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mdf_edge_cases as ec
import mdf_ops_oracle as mo
import mutate_spec as ms
from conftest import GOLDEN, ROOT

GOLDEN_TSV = os.path.join(GOLDEN, "mutate", "variants.tsv")
TKSM = os.path.join(ROOT, "tksm_amd", "tksm")


def _check_against_model(genome, table, mdf):
    rows = ms.parse_variants(table)
    nf, _ = ms.normal_form(rows)
    mols = mo.stream_mdf(mdf, unroll=True)
    out = ms.mutate_spec(mols, nf)
    assert [m["id"] for m in out] == [m["id"] for m in mols]
    for md, got in zip(mols, out):
        assert ms.splice(got, genome) == ms.expected_read(md, genome, rows), (md, got, table)
    return mols, out


def test_spec_equals_the_string_model_on_random_small_cases():
    """3 000 cases: mixed kinds, both strands, shared anchors, overlapping and reversed deletions, literal segments that are table contigs"""
    seen = dict(pieces=0, literals=0, minus_split=0, dropped=0)
    for seed in range(3000):
        genome, table, mdf = ms.random_case(seed)
        mols, out = _check_against_model(genome, table, mdf)
        seen["dropped"] += ms.normal_form(ms.parse_variants(table))[1]["dropped_points"]
        for md, got in zip(mols, out):
            seen["pieces"] += len(got["segments"]) != len(md["segments"])
            seen["literals"] += sum(s["chr"] not in genome and s["chr"] not in ms.RANDOM_LITERALS for s in got["segments"])
            seen["minus_split"] += any(not s["plus"] for s in got["segments"]) and len(got["segments"]) > len(md["segments"])
    assert all(v > 100 for v in seen.values()), seen


def test_spec_equals_the_string_model_on_the_crafted_corpus():
    """every meeting of a variant with a segment end, made on purpose (mutate_spec.crafted_tables): SNVs at s - 1, s, e - 1, e; deletions with
    f == s, t == e, [s, e), one base wider, strictly inside, across two segments; insertions anchored at s, e - 1 and e"""
    genome = ec.genome()
    mols = ec.crafted_molecules()
    changed = whole = 0
    for table in ms.crafted_tables(mols):
        rows = ms.parse_variants(table)
        nf, _ = ms.normal_form(rows)
        out = ms.mutate_spec(mols, nf)
        for md, got in zip(mols, out):
            assert ms.splice(got, genome) == ms.expected_read(md, genome, rows), (md["id"], got)
            changed += got["segments"] != md["segments"]
        whole += sum(not m["segments"] for m, md in zip(out, mols) if mo.mol_size(md))
    assert changed > 300 and whole > 0, (changed, whole)


def _segments_on(mols, contigs):
    return all(s["chr"] in contigs for md in mols for s in md["segments"])


def test_spec_equals_the_reference_on_snv_tables():
    """SNV-only tables with every segment's contig in the table: text for text"""
    rs = np.random.RandomState(5)
    genome = ms.random_genome(rs, 3, 30, 60)
    for trial in range(40):
        mdf = ms.random_molecules(rs, genome, [], 6, with_subs=True)
        taken, lines = set(), [f"{c}\t0\tA\n" for c in genome]
        for _ in range(12):
            c = sorted(genome)[rs.randint(3)]
            p = int(rs.randint(1, len(genome[c])))
            if (c, p) not in taken:
                taken.add((c, p))
                lines.append(f"{c}\t{p}\t{'ACGT'[rs.randint(4)]}\n")
        table = "".join(lines)
        mols = mo.stream_mdf(mdf, unroll=True)
        mols = [md for md in mols if all(s["end"] > s["start"] for s in md["segments"])]
        assert _segments_on(mols, genome)
        nf, _ = ms.normal_form(ms.parse_variants(table))
        assert mo.write_mdf(ms.mutate_spec(mols, nf)) == mo.write_mdf(ms.mutate_reference(mols, table))


def test_spec_equals_the_reference_on_deletions_strictly_inside_plus_segments():
    genome = {"c0": "ACGT" * 30}
    mols = mo.stream_mdf("+a\t1\t\nc0\t10\t40\t+\t3A,25C\nc0\t60\t90\t+\t\n+b\t2\tx=1;\nc0\t50\t58\t+\t0G\n", unroll=True)
    table = "c0\t15\t20\nc0\t70\t71\nc0\t52\t56\n"
    nf, _ = ms.normal_form(ms.parse_variants(table))
    got = ms.mutate_spec(mols, nf)
    assert mo.write_mdf(got) == mo.write_mdf(ms.mutate_reference(mols, table))
    assert [len(m["segments"]) for m in got] == [4, 2, 2]


def _both(mdf, table, genome):
    mols = mo.stream_mdf(mdf, unroll=True)
    rows = ms.parse_variants(table)
    spec = ms.mutate_spec(mols, ms.normal_form(rows)[0])
    ref = ms.mutate_reference(mols, table)
    want = [ms.expected_read(md, genome, rows) for md in mols]
    return ms.splice(spec, genome), ms.splice(ref, genome), want


def test_where_the_reference_is_wrong_the_model_sides_with_the_spec():
    """one case per defect of src/mutate.cpp: the two differ, and the string model agrees with the specification"""
    g = {"c0": "ACGTACGTACGTACGTACGTACGTACGTAC", "c1": "TTTTGGGGCCCCAAAA"}
    cases = {
        "an insertion loses its anchor base (:60-64)": ("+m\t1\t\nc0\t4\t12\t+\t\n", "c0\t6\t.TT\n"),
        "nothing knows about strands": ("+m\t1\t\nc0\t4\t12\t-\t\n", "c0\t6\t.AG\n"),
        "a deletion that shares an end with a segment deletes it whole (:74-89)": ("+m\t1\t\nc0\t4\t12\t+\t\n", "c0\t4\t7\n"),
        "a deletion that starts before a segment does not touch it": ("+m\t1\t\nc0\t4\t12\t+\t\n", "c0\t2\t7\n"),
        "the reversed copy of a deletion keeps the same pos (:117-121)": ("+m\t1\t\nc0\t4\t12\t+\t\n", "c0\t9\t6\n"),
        "the slicing constructor keeps a substitution at position == size (interval.h:695-703)": ("+m\t1\t\nc0\t4\t12\t+\t2T\n", "c0\t6\t8\n"),
        "every segment on a contig without a variant is dropped (:129-131)": ("+m\t1\t\nc0\t4\t12\t+\t\nc1\t2\t9\t+\t\n", "c0\t5\tG\n"),
    }
    for why, (mdf, table) in cases.items():
        try:
            spec, ref, want = _both(mdf, table, g)
        except IndexError:                                              # (the reference's substitution at position == size does not splice at all)
            mols = mo.stream_mdf(mdf, unroll=True)
            rows = ms.parse_variants(table)
            spec, ref, want = ms.splice(ms.mutate_spec(mols, ms.normal_form(rows)[0]), g), None, [ms.expected_read(md, g, rows) for md in mols]
        assert spec == want, why
        assert ref != want, why


# ------------------------------------------------------------------------------------------------ the library's reader (host only)
def _load(text=None, path=None):
    from tksm_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    b = text.encode("latin-1") if isinstance(text, str) else text
    rc = lib.tksmseq_variants_load(None, path.encode() if path else None, b, len(b) if b is not None else 0, C.byref(h))
    if rc:
        return rc, lib.tksmseq_last_error(None).decode(), None
    v = [C.c_uint64() for _ in range(6)]
    assert lib.tksmseq_variants_info(h, *[C.byref(x) for x in v]) == 0
    lib.tksmseq_variants_free(h)
    return 0, "", dict(zip(("rows", "snvs", "insertions", "deletions", "deleted_ranges", "dropped_points"), [x.value for x in v]))


def test_golden_table_counts_and_normal_form():
    text = open(GOLDEN_TSV).read()
    nf, counters = ms.normal_form(ms.parse_variants(text))
    assert counters == dict(rows=20, snvs=6, insertions=6, deletions=8, deleted_ranges=5, dropped_points=2)
    assert nf["chr1"]["ranges"] == [(1020, 1030), (1090, 1100), (1200, 1225)]
    assert [(p[0], p[2], p[3]) for p in nf["chr1"]["points"]] == [(1000, "G", None), (1010, None, "ACGT"), (1300, "T", "AA"), (1300, None, "CC"), (1300, "C", None)]
    assert nf["chr2"]["ranges"] == [] and len(nf["chr2"]["points"]) == 3
    for kw in (dict(text=text), dict(path=GOLDEN_TSV)):
        rc, _, info = _load(**kw)
        assert rc == 0 and info == counters


def test_reader_agrees_with_the_spec_on_random_tables():
    rs = np.random.RandomState(11)
    for _ in range(200):
        table = ms.random_table(rs, {"c0": 30, "c1": 12, "ACGTTGCAAGGCT": 13}, rs.randint(0, 40))
        rc, _, info = _load(text=table)
        assert rc == 0 and info == ms.normal_form(ms.parse_variants(table))[1], table


REFUSED = [
    ("chr1\t5\n", ms.EINVAL, 1), ("chr1\n", ms.EINVAL, 1), ("chr1\t5\tA\n\nchr1 7\n", ms.EINVAL, 3), ("chr1\t-1\tA\n", ms.EINVAL, 1),
    ("chr1\t2147483648\tA\n", ms.EINVAL, 1), ("chr1\t1e3\tA\n", ms.EINVAL, 1), ("chr1\t5x\tA\n", ms.EINVAL, 1),
    ("chr1\t5\t2147483648\n", ms.EINVAL, 1), ("chr1\t5\t99999999999999999999\n", ms.EINVAL, 1), ("chr1\t99999999999999999999\t7\n", ms.EINVAL, 1),
    ("chr1\t5\t.\n", ms.EINVAL, 1), ("chr1\t5\tA\nchr1\t+6\tA", ms.EINVAL, 2),
    ("chr1\t5\t." + "A" * ((1 << 20) + 1) + "\n", ms.ELIMIT, 1),
]
ACCEPTED = ["", "\n\n  \t\n", "chr1\t2147483647\t2147483647", "chr1\t5\t." + "A" * (1 << 20), "chr1 5 A extra fields here\r\n", "\tchr1\v5\f7\r\n",
            "chr1\t5\t-\nchr1\t5\t-3\n", "chr1\t0\t0\n"]


def test_every_refused_line():
    for text, code, line in REFUSED:
        with pytest.raises(ms.VariantError) as e:
            ms.parse_variants(text)
        assert (e.value.code, e.value.line) == (code, line), text[:40]
        rc, msg, _ = _load(text=text)
        assert rc == code and f"<text>:{line}:" in msg, (text[:40], rc, msg)
    for text in ACCEPTED:
        rc, msg, info = _load(text=text)
        assert rc == 0 and info == ms.normal_form(ms.parse_variants(text))[1], (text[:40], msg)
    rc, msg, _ = _load(path="/no/such/dir/variants.tsv")
    assert rc == 2 and "Could not open variant table" in msg


def test_exports():
    from tksm_amd import _lib
    from tksm_amd.sequence import Sequencer, Variants
    lib = _lib.load()
    for s in ("tksmseq_variants_load", "tksmseq_variants_info", "tksmseq_variants_free", "tksmseq_mutate", "tksmseq_mutate_main"):
        assert hasattr(lib, s) and s in _lib.SYMBOLS
    assert callable(Sequencer.load_variants) and callable(Sequencer.mutate) and hasattr(Variants, "close")
    assert C.sizeof(_lib.MutateParams) == 8


# ------------------------------------------------------------------------------------------------ the module's arguments (no device)
def _tksm(*args):
    return subprocess.run([TKSM, "mutate", *args], capture_output=True, text=True)


def test_module_help_and_missing_parameters(tmp_path):
    r = _tksm("-h")
    assert r.returncode == 0 and "usage: mutate -i INPUT -o OUTPUT -t TSV" in r.stdout
    r = _tksm()
    assert r.returncode == 1 and [r.stderr.count(m) for m in ("input is required!", "output is required!", "tsv is required!")] == [1, 1, 1]
    assert "usage: mutate" in r.stderr
    r = _tksm("-i", "x.mdf", "--tsv", "t.tsv")
    assert r.returncode == 1 and "output is required!" in r.stderr and "input is required!" not in r.stderr and "tsv is required!" not in r.stderr
    r = _tksm("-i", "x.mdf", "-o", str(tmp_path / "o.mdf"), "-t", "t.tsv", "--nope")
    assert r.returncode == 1 and "Option '--nope' does not exist" in r.stderr
    r = subprocess.run([TKSM, "list"], capture_output=True, text=True)
    assert "mutate" not in r.stdout.split()


def test_module_refuses_a_bad_table_before_any_device_is_touched(tmp_path):
    bad = tmp_path / "bad.tsv"
    bad.write_text("chr1\t5\tA\nchr1\tfive\tA\n")
    out = tmp_path / "o.mdf"
    r = _tksm("-i", str(tmp_path / "missing.mdf"), "-o", str(out), "-t", str(bad))
    assert r.returncode == 1 and f"{bad}:2:" in r.stderr and "POS" in r.stderr and not out.exists()
    r = _tksm("-i", str(tmp_path / "missing.mdf"), "-o", str(out), "-t", str(tmp_path / "none.tsv"))
    assert r.returncode == 1 and "Could not open variant table" in r.stderr and not out.exists()
