"""filter (Flt) and concat (Mrg), CPU part: the specification (tests/filter_spec.py) pinned against the reference's own text, the
library's exports, the condition parser of the build against the specification, and `tksm filter`'s argument checks.  No GPU: the
module checks its arguments and conditions before it opens a file or a device.  The device side is in tests/test_filter_gpu.py."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

import filter_spec as fs
import mdf_ops_oracle as mo

EXE = os.path.join(ROOT, "tksm_amd", "tksm")


def _cli(*args, **kw):
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=600, **kw)


# ------------------------------------------------------------------------------------------------ specification
# The thirteen relative positions of a range R against the segment S = [10, 20), with seg.overlap(R) read off src/interval.h:38-58
# branch by branch.  Two of them are the reference's defined quirks: a range that shares exactly one end with the segment and sticks
# out on the other side matches none of the six branches and falls through to `return 0`.
OVERLAP_TABLE = [
    ("before", 2, 5, 0),                  # :39  other.end <= start
    ("meets", 5, 10, 0),                  # :39  other.end <= start (equal)
    ("overlaps", 5, 15, 5),               # :51  LEFT OVERLAP: other.end - start
    ("finished-by", 5, 20, 0),            # none: other.start < start && other.end == end  -> :57 return 0   (quirk)
    ("contains", 5, 25, 10),              # :48  AROUND: end - start
    ("starts", 10, 15, 5),                # :45  IN: other.end - other.start
    ("equals", 10, 20, 10),               # :45  IN
    ("started-by", 10, 25, 0),            # none: other.start == start && other.end > end   -> :57 return 0   (quirk)
    ("during", 12, 18, 6),                # :45  IN
    ("finishes", 15, 20, 5),              # :45  IN
    ("overlapped-by", 15, 25, 5),         # :54  RIGHT OVERLAP: end - other.start
    ("met-by", 20, 25, 0),                # :42  other.start >= end (equal)
    ("after", 22, 30, 0),                 # :42  other.start >= end
]


def test_overlap_on_all_thirteen_relative_positions():
    assert len({name for name, *_ in OVERLAP_TABLE}) == 13
    for name, a, b, want in OVERLAP_TABLE:
        assert fs.overlap(10, 20, a, b) == want, name
    # the symmetric picture (the range as `this`) has the same two holes on the other side
    assert fs.overlap(5, 20, 10, 20) == 10 and fs.overlap(10, 25, 10, 20) == 10


def test_conditions_follow_filter_condition():
    text = ("+a\t1\tCB=ACGT;x=1;\nchr1\t10\t20\t+\t\nchr2\t100\t150\t-\t3A\n"
            "+b\t3\tCB=.;\nchr1\t30\t40\t+\t\n"
            "+c\t1\tCB=;\nGATTACA\t0\t7\t+\t\n"
            "+d\t1\t\nchr2\t0\t5\t+\t\n"
            "+e\t1\tCB=.,X;flag;\nchr1\t10\t20\t-\t\n")
    mols = mo.stream_mdf(text, unroll=True)
    ids = lambda side: [m["id"] for m in side]
    t, f = fs.filter_spec(mols, ["info CB"])
    assert ids(t) == ["a"] and ids(f) == ["b_0", "b_1", "b_2", "c", "d", "e"]
    assert ids(fs.filter_spec(mols, ["info flag"])[0]) == []             # a bare key reads as "."
    assert ids(fs.filter_spec(mols, ["info x"])[0]) == ["a"]
    assert ids(fs.filter_spec(mols, ["info CB"], negate=True)[0]) == ids(f)
    for op, v, want in (("<", 10, ["c", "d"]), ("<=", 10, ["b_0", "b_1", "b_2", "c", "d", "e"]), (">", 10, ["a"]), (">=", 60, ["a"]), ("==", 7, ["c"]),
                        ("!=", 10, ["a", "c", "d"])):
        assert ids(fs.filter_spec(mols, [f"size {op}{v}"])[0]) == want, (op, v)
    assert ids(fs.filter_spec(mols, ["locus chr2"])[0]) == ["a", "d"]
    assert ids(fs.filter_spec(mols, ["locus GATTACA"])[0]) == ["c"] and ids(fs.filter_spec(mols, ["locus GATTAC"])[0]) == []
    assert ids(fs.filter_spec(mols, ["locus chr1:15-35"])[0]) == ["a", "b_0", "b_1", "b_2", "e"]
    assert ids(fs.filter_spec(mols, ["locus chr1:5-20"])[0]) == []        # finished-by: the quirk
    assert ids(fs.filter_spec(mols, ["locus chr1:19"])[0]) == ["a", "e"] and ids(fs.filter_spec(mols, ["locus chr1:20"])[0]) == []
    assert ids(fs.filter_spec(mols, ["locus chr1:12-18:junk"])[0]) == ["a", "e"]          # rsplit keeps only the first two pieces
    assert ids(fs.filter_spec(mols, ["locus chr1", "size >10", "info CB"])[0]) == ["a"]
    assert ids(fs.filter_spec(mols, ["locus chr1", "size >10"], negate=True)[0]) == ["b_0", "b_1", "b_2", "c", "d", "e"]
    assert mo.write_mdf(fs.concat_spec([t, f])) == mo.write_mdf([mols[0]] + mols[1:])


INVALID = ["size", "info", "info CB x", "info  CB", "", "bogus x", "Info CB", "size >", "size 5", "size =5", "size =>5", "size >x", "size >=", "size >-3",
           "size >99999999999", "size <>5", "locus chr1:", "locus chr1:-5", "locus chr1:a-5", "locus chr1:5-b", "locus chr1:5-", "locus chr1:99999999999"]
VALID = ["info CB", "info =", "size >5", "size >=5", "size <0", "size <=7", "size ==7", "size !=7", "size >\t5", "size >5x", "size >+5", "size ==2147483647",
         "locus chr1", "locus chr1:5", "locus chr1:5-9", "locus chr1:9-5", "locus chr1:5-9-11", "locus chr1:5:7", "locus :5", "locus chr1:5x-9y"]


def test_spec_refuses_what_the_issue_lists():
    for t in INVALID:
        with pytest.raises(fs.InvalidCondition, match=re.escape("Invalid condition: " + t)):
            fs.condition(t)
    for t in VALID:
        fs.condition(t)


def test_the_builds_parser_agrees_with_the_spec(tmp_path):
    """parse_filter_condition (csrc/filter_host.h), compiled alone: the same texts accepted and refused, and the parsed fields"""
    src = tmp_path / "parse.cpp"
    src.write_text(r'''
#include "filter_host.h"
#include <cstdio>
int main(int argc, char** argv) {
    for (int i = 1; i < argc; i++) {
        tkh::FilterCond c;
        if (!tkh::parse_filter_condition(argv[i], c)) { std::puts("INVALID"); continue; }
        std::printf("%d %d [%s] %lld %d %lld %lld\n", c.kind, c.cmp, c.key.c_str(), c.value, (int)c.ranged, c.start, c.end);
    }
    return 0;
}
''')
    exe = tmp_path / "parse"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "tksm_amd", "csrc"), "-o", str(exe), str(src)], check=True)
    texts = INVALID + VALID
    out = subprocess.run([str(exe), *texts], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(texts)
    for t, line in zip(texts, out):
        assert (line == "INVALID") == (t in INVALID), (t, line)
    got = dict(zip(texts, out))
    assert got["info CB"] == "1 0 [CB] 0 0 0 0"
    assert got["size >=5"] == "2 3 [] 5 0 0 0" and got["size !=7"] == "2 5 [] 7 0 0 0" and got["size >\t5"] == "2 2 [] 5 0 0 0"
    assert got["size >5x"] == "2 2 [] 5 0 0 0" and got["size ==2147483647"] == "2 4 [] 2147483647 0 0 0"
    assert got["locus chr1"] == "3 0 [chr1] 0 0 0 0" and got["locus chr1:5"] == "3 0 [chr1] 0 1 5 6"
    assert got["locus chr1:5-9-11"] == "3 0 [chr1] 0 1 5 9" and got["locus chr1:5:7"] == "3 0 [chr1] 0 1 5 6" and got["locus :5"] == "3 0 [] 0 1 5 6"


# ------------------------------------------------------------------------------------------------ library and CLI surface
def test_library_exports_and_header_declares_filter_and_concat():
    import ctypes
    from tksm_amd import _lib
    lib = ctypes.CDLL(os.path.join(ROOT, "tksm_amd", "libtksmseq.so"))
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    for s in ("tksmseq_filter", "tksmseq_concat", "tksmseq_filter_main"):
        assert hasattr(lib, s), s
        assert re.search(r"\bint " + s + r"\(", header), s
        assert s in _lib.SYMBOLS
    assert "tksmseq_filter_cond" in header and "tksmseq_filter_params" in header
    assert ctypes.sizeof(_lib.FilterCond) == 48 and ctypes.sizeof(_lib.FilterParams) == 24
    from tksm_amd.sequence import Sequencer
    assert callable(Sequencer.filter) and callable(Sequencer.merge)


def test_filter_help_exits_zero_and_list_is_unchanged():
    r = _cli("filter", "--help")
    assert r.returncode == 0 and "usage: filter" in r.stdout and "--negate" in r.stdout
    r = _cli("list")
    assert r.returncode == 0 and r.stdout.split() == ["sequence", "pcr", "truncate", "polyA", "tag", "scb", "flip"]
    assert _cli("merge").returncode == 1                                  # on files Mrg is `cat`: no such module


@pytest.mark.parametrize("args,messages", [
    (["filter"], ["Missing parameter: input", "Missing parameter: true-output", "Missing parameter: condition", "usage: filter"]),
    (["filter", "-t", "t.mdf", "-c", "info CB"], ["Missing parameter: input", "usage: filter"]),
    (["filter", "-i", "a.mdf", "-c", "info CB"], ["Missing parameter: true-output"]),
    (["filter", "-i", "a.mdf", "-t", "t.mdf", "-f", "f.mdf"], ["Missing parameter: condition"]),
    (["filter", "-i", "a.mdf", "-t", "t.mdf", "--negate"], ["Missing parameter: condition"]),
    (["filter", "-i", "a.mdf", "-o", "t.mdf", "-c", "info CB"], ["Option '-o' does not exist"]),
    (["filter", "-i", "a.mdf", "-t", "t.mdf", "-c", "info CB", "--bogus"], ["does not exist"]),
])
def test_filter_argument_checks_follow_the_reference(args, messages):
    r = _cli(*args)
    assert r.returncode == 1, (args, r.stderr)
    for m in messages:
        assert m in r.stderr, (args, m, r.stderr)
    if "condition" not in " ".join(messages):
        assert "Missing parameter: condition" not in r.stderr


@pytest.mark.parametrize("text", [t for t in INVALID if t])
def test_filter_refuses_each_invalid_condition(text, tmp_path):
    t = tmp_path / "t.mdf"
    r = _cli("filter", "-i", tmp_path / "a.mdf", "-t", t, "-c", text)
    assert r.returncode == 1 and "Invalid condition: " + text in r.stderr, r.stderr
    assert not t.exists()                                                 # refused before anything is opened


def test_conditions_are_comma_split_and_repeatable(tmp_path):
    t = tmp_path / "t.mdf"
    r = _cli("filter", "-i", tmp_path / "a.mdf", "-t", t, "-c", "size >5,bogus x")
    assert r.returncode == 1 and "Invalid condition: bogus x" in r.stderr
    r = _cli("filter", "-i", tmp_path / "a.mdf", "-t", t, "-c", "size >5", "--condition=info CB", "-c", "locus chr1:5-")
    assert r.returncode == 1 and "Invalid condition: locus chr1:5-" in r.stderr
    # valid conditions pass the check: the run then stops at the input that is not there (before any device is opened)
    r = _cli("filter", "-i", tmp_path / "a.mdf", "-t", t, "-c", "size >5,info CB", "-c", "locus chr1:5-9", "--negate")
    assert r.returncode == 1 and "Invalid condition" not in r.stderr and f"Could not open file {tmp_path / 'a.mdf'}" in r.stderr
