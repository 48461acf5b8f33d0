"""map --extend on the device against the specification (tests/map_extend_spec.py): the PAF bytes and the integer counters of all info
blocks, no tolerance, without -c, with -c and with -c --eqx.  Shapes, each small and reaching one thing: exact reads on both strands whose
target or read ends first, planted edits with secondary lines, indel runs at the band's edge, mismatch runs at the drop's edge on both
parities, ties of the best score, extensions around 64 and 128 anti-diagonals, --ext-max cutting and binding, N runs, every offset of a
packed word down to position 0, chunk sizes and a chunk over the extension's budget, recycled memory, reuse of a context, the extend-NULL
call, error codes, and the route the option is for: transcribe -> sequence -> map --extend -> model-truncation."""
import ctypes
import gzip
import os
import random
import subprocess

import pytest

from conftest import ERR_MODEL, QS_MODEL, ROOT

import map_align_spec as A
import map_extend_spec as X
import map_spec as M

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
MODES = (dict(align=False), dict(align=True), dict(align=True, eqx=True))


def device(targets, reads, d, tag="dev", sequencer=None, extend=True, **params):
    """the device's PAF and counters for targets and reads given as [(name, letters)]"""
    from tksm_amd.sequence import Sequencer
    fq = M.write_fastq(os.path.join(str(d), tag + ".fq"), reads)
    out = os.path.join(str(d), tag + ".paf")
    s = sequencer or Sequencer(0)
    try:
        if not sequencer:
            for name, seq in targets:
                s.add_contig(name, seq)
        info = s.map(fq, out, extend=extend, **params)
    finally:
        if not sequencer:
            s.close()
    assert not [f for f in os.listdir(str(d)) if f.endswith(".tmp")]
    return {"paf": open(out).read(), "info": info}


def contains(new, old):
    """every line of `new` holds the interval of its line in `old`, and nothing else of columns 1, 2, 5-7, 12 and the tp, cm, s1 tags moved"""
    a, b = new.splitlines(), old.splitlines()
    assert len(a) == len(b)
    for x, y in zip(a, b):
        fx, fy = x.split("\t"), y.split("\t")
        assert fx[:2] == fy[:2] and fx[4:7] == fy[4:7] and fx[11:15] == fy[11:15]
        assert int(fx[2]) <= int(fy[2]) <= int(fy[3]) <= int(fx[3]) <= int(fx[1]) and int(fx[7]) <= int(fy[7]) <= int(fy[8]) <= int(fx[8]) <= int(fx[6])


def same(dev, spec, align, eqx=False):
    assert dev["paf"] == spec["paf"]
    assert {k: dev["info"][k] for k in M.COUNTERS} == spec["info"]
    x = dev["info"]["extend"]
    assert {k: x[k] for k in X.COUNTERS} == spec["extend"] and x["lines"] == dev["info"]["lines"]
    assert x["extend_ms"] > 0 or not x["lines"]
    contains(dev["paf"], spec["base"])
    if not align:
        assert "align" not in dev["info"] and all(len(l.split("\t")) == 15 for l in dev["paf"].splitlines())
        return
    assert {k: dev["info"]["align"][k] for k in A.COUNTERS} == spec["align"]
    for line in dev["paf"].splitlines():
        f = line.split("\t")
        t, q, n = A.cigar_spans(f[-1][5:])
        assert f[-1].startswith("cg:Z:") and t == int(f[8]) - int(f[7]) and q == int(f[3]) - int(f[2])
        assert f[-2].startswith("NM:i:") and int(f[10]) == sum(n.values()) and int(f[-2][5:]) == int(f[10]) - int(f[9])
        assert (not eqx and not n["="] and not n["X"]) or (eqx and not n["M"] and int(f[9]) == n["="] and int(f[-2][5:]) == n["X"] + n["I"] + n["D"])


def check(targets, reads, d, modes=MODES, memo=None, **params):
    """every mode against the spec; the spec of the last mode.  memo: what map_extend_spec.map_reads may keep between calls"""
    memo, spec = {} if memo is None else memo, None
    for n, mode in enumerate(modes):
        spec = X.map_reads(targets, reads, memo=memo, **mode, **params)
        same(device(targets, reads, d, tag="m%d" % n, **mode, **params), spec, mode["align"], mode.get("eqx", False))
    return spec


def noisy(rs, seq, period=10, first=0):
    """seq with a substitution at first, first + period, ...: no 15-mer of it is left when period < 15"""
    out = list(seq)
    for x in range(first, len(out), period):
        out[x] = rs.choice([c for c in "ACGT" if c != seq[x]])
    return "".join(out)


def both(name, read):
    return [(name + "f", read), (name + "r", M.revcomp(read))]


def tailed(target, a, b, left, right):
    """the read target[a:b] with tails: `right` is what follows the core, `left` what precedes it, GIVEN OUTWARD (its first letter is the
    one next to the core), so that one recipe serves both ends"""
    return left[::-1] + target[a:b] + right


W1 = dict(w=1)                                       # every intact 15-mer an anchor: a chain ends where the last intact 15-mer does


def moves_of(spec, name):
    """(left, right) of the first line of read `name`"""
    at = [l.split("\t")[0] for l in spec["paf"].splitlines()].index(name)
    return spec["moves"][at]


# ------------------------------------------------------------------------------------------------ exact reads
def test_exact_reads_whose_target_or_read_ends_first(tmp_path):
    """the default w = 10 leaves up to some ten exact letters between a chain and the end of an exact read: a whole target, junk past both
    ends of the target, a read inside the target, and (w = 1) chains that touch the ends already"""
    rs = random.Random(31)
    targets = [("t%d" % i, M.random_seq(rs, 300 + 7 * i)) for i in range(3)]
    reads = []
    for i, (_, t) in enumerate(targets):
        reads += both("whole%d" % i, t) + both("junk%d" % i, M.random_seq(rs, 30) + t + M.random_seq(rs, 33)) + both("inside%d" % i, t[40 + i:260 - i])
    spec = check(targets, reads, tmp_path)
    rows = {l.split("\t")[0]: l.split("\t") for l in spec["paf"].splitlines()}
    for i, (_, t) in enumerate(targets):
        for s in "fr":
            assert rows["whole%d" % i + s][7:9] == rows["junk%d" % i + s][7:9] == ["0", str(len(t))] and rows["whole%d" % i + s][2:4] == ["0", str(len(t))]
            assert rows["junk%d" % i + s][2:4] == (["30", str(30 + len(t))] if s == "f" else ["33", str(33 + len(t))])
            assert rows["inside%d" % i + s][2:4] == ["0", str(220 - 2 * i)] and rows["inside%d" % i + s][7:9] == [str(40 + i), str(260 - i)]
    assert spec["extend"]["ends_moved"] > len(reads)
    touching = check(targets, reads, tmp_path, **W1)
    assert touching["extend"]["ends_moved"] == 0 and touching["paf"] == touching["base"]


# ------------------------------------------------------------------------------------------------ planted edits, secondary lines
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """24 reads of 200 - 600 bases with 10 % planted edits on both strands, a lightly edited copy of the first target so that its reads
    have a second line, every line written (-p 0.0): the three specs computed once, shared"""
    d = tmp_path_factory.mktemp("map_extend_planted")
    g = M.generate(d, seed=5, n_targets=4, n_reads=24, lengths=(400, 700), min_read=200, error=0.10)
    g["targets"] = g["targets"] + [("copy", A.plant(random.Random(6), g["targets"][0][1], 0.02)[0])]
    g["ref"] = M.write_fasta(os.path.join(str(d), "with_copy.fa"), g["targets"])
    g["memo"] = {}
    g["dir"], g["specs"] = d, [X.map_reads(g["targets"], g["read_list"], memo=g["memo"], secondary_ratio=0.0, **mode) for mode in MODES]
    return g


def test_planted_edits_both_strands_and_secondary_lines(planted):
    g = planted
    for n, (mode, spec) in enumerate(zip(MODES, g["specs"])):
        same(device(g["targets"], g["read_list"], g["dir"], tag="p%d" % n, secondary_ratio=0.0, **mode), spec, mode["align"], mode.get("eqx", False))
    spec = g["specs"][0]
    assert spec["info"]["secondary"] > 0 and {l.split("\t")[4] for l in spec["paf"].splitlines()} == {"+", "-"}
    assert spec["extend"]["ends_moved"] > spec["extend"]["lines"] and spec["extend"]["target_gained"] != spec["extend"]["read_gained"]
    assert any("I" in c or "D" in c for l, r in g["specs"][2]["moves"] for c in (l["columns"], r["columns"]))


def test_ext_drop_1_and_ext_max_1(planted, tmp_path):
    g = planted
    one = check(g["targets"], g["read_list"], tmp_path, memo=g["memo"], secondary_ratio=0.0, ext_drop=1)
    assert 0 < one["extend"]["target_gained"] < g["specs"][0]["extend"]["target_gained"]
    short = check(g["targets"], g["read_list"], tmp_path, memo=g["memo"], secondary_ratio=0.0, ext_max=1)
    assert 0 < short["extend"]["longest"] == 2 and short["extend"]["target_gained"] == short["extend"]["read_gained"] == short["extend"]["ends_moved"]


# ------------------------------------------------------------------------------------------------ the band
@pytest.mark.parametrize("band", [1, 2, 31, 63])
def test_an_indel_run_of_the_band_and_one_more(tmp_path, band):
    """both tails: 30 letters, then `n` letters deleted or inserted, then 260 letters with a substitution every 14th (worth more than the
    gap of 63 costs), with a drop that never binds: the extension crosses a run of n = band and stays before one of band + 1"""
    rs = random.Random(300 + band)
    target = M.random_seq(rs, 800)
    a, b, reads = 370, 430, []
    for n in (band, band + 1):
        for kind in "DI":
            tails = []
            for stretch in (target[:a][::-1], target[b:]):                      # outward
                near, far = noisy(rs, stretch[:30], 14), stretch[30 + n:30 + n + 260] if kind == "D" else stretch[30:290]
                tails.append(near + (M.random_seq(rs, n) if kind == "I" else "") + noisy(rs, far, 14, 6))
            reads += both("%s%d" % (kind, n), tailed(target, a, b, *tails))
    spec = check([("t", target)], reads, tmp_path, ext_band=band, ext_drop=1000, **W1)
    assert all(l.split("\t")[7:9] == ["370", "430"] for l in spec["base"].splitlines())         # (no 15-mer of a tail came back by chance)
    for name, _ in reads:
        for e in moves_of(spec, name):
            assert (e["ei"] + e["ej"] > 500) == (name[1:-1] == str(band)), (name, e["ei"], e["ej"])
            assert name[1:-1] != str(band) or e["columns"].count(name[0]) >= band


# ------------------------------------------------------------------------------------------------ the drop
@pytest.mark.parametrize("shift", [0, 1])
def test_a_penalty_of_the_drop_and_one_more(tmp_path, shift):
    """tails of 20 + shift letters with the 1st and the 12th substituted, 8 N (which match nothing: the diagonal falls 16 below the best),
    then 40 letters with a substitution every 12th.  The stop looks at two anti-diagonals, and the cells beside the diagonal that a gap
    reaches fall a step later, so the drop at which the run is crossed is looked up in the specification: 16, or 15 or 14 when the gap cells
    hold the maximum up.  At that drop the penalty equals it and the extension goes on, at one less it stops; `shift` moves the run to the
    other parity of anti-diagonals"""
    rs = random.Random(200 + shift)
    target = M.random_seq(rs, 500)
    a, b = 200, 260
    tails = []
    for stretch in (target[:a][::-1], target[b:]):
        tails.append(noisy(rs, stretch[:20 + shift], 11) + "N" * 8 + noisy(rs, stretch[28 + shift:68 + shift], 12, 11))
    reads = both("n", tailed(target, a, b, *tails))
    crossed = {z: [e["ei"] for e in X.ends_of(target, reads[0][1], dict(tstart=a, tend=b, qs=len(tails[0]), qe=len(tails[0]) + b - a), 4, z, 2000)] for z in range(12, 19)}
    assert all(set(v) <= {20 + shift, 68 + shift} and len(set(v)) == 1 for v in crossed.values()) and crossed[12][0] == 20 + shift and crossed[18][0] == 68 + shift
    edge = min(z for z, v in crossed.items() if v[0] == 68 + shift)
    assert 14 <= edge <= 16 and all((v[0] == 68 + shift) == (z >= edge) for z, v in crossed.items())
    for drop, far in ((edge, True), (edge - 1, False)):
        spec = check([("t", target)], reads, tmp_path, ext_drop=drop, ext_band=4, **W1)
        assert all(l.split("\t")[7:9] == [str(a), str(b)] for l in spec["base"].splitlines())
        for name, _ in reads:
            for e in moves_of(spec, name):
                assert e["ei"] == e["ej"] == (68 + shift if far else 20 + shift), (drop, e["ei"], e["ej"])


# ------------------------------------------------------------------------------------------------ ties
def test_ties_across_and_within_anti_diagonals(tmp_path):
    """across: a mismatch, 9 matches, 2 mismatches, 4 matches reach the score of 7 twice, the later cell wins.  within: CACACACAC against ACACACACA
    reaches 6 at (9, 8) and at (8, 9), the smaller i wins"""
    rs = random.Random(41)
    cores = [M.random_seq(rs, 60) for _ in range(2)]
    flank = ["G" + M.random_seq(rs, 9) + "GG" + "TTAA", "CACACACAC" + "G"]         # the target beyond the core, outward; the read's first letter differs
    mine = ["C" + flank[0][1:10] + "CC" + "TTAA", "ACACACACA"]
    targets, reads = [], []
    for n in range(2):
        targets.append(("t%d" % n, M.random_seq(rs, 40) + flank[n][::-1] + cores[n] + flank[n] + M.random_seq(rs, 40)))
        reads += both("q%d" % n, mine[n][::-1] + cores[n] + mine[n])
    spec = check(targets, reads, tmp_path, **W1)
    for s in "fr":
        for e in moves_of(spec, "q0" + s):
            assert (e["ei"], e["ej"], e["score"], e["m"]) == (16, 16, 7, 13)
        for e in moves_of(spec, "q1" + s):
            assert (e["ei"], e["ej"], e["score"], e["m"]) == (8, 9, 6, 8)


# ------------------------------------------------------------------------------------------------ lengths around the wave and the store's words
def test_extensions_around_64_and_128_anti_diagonals(tmp_path):
    """tails with a substitution every 10th letter from the first on, an odd count by one deleted letter: the best cell lies on
    anti-diagonal 63 .. 65 and 127 .. 129, where the walk back loads its second batch of 64 store words"""
    rs = random.Random(64)
    target = M.random_seq(rs, 300)
    a, b, reads = 120, 180, []
    for cap in (63, 64, 65, 127, 128, 129):
        n = (cap + 1) // 2
        tails = []
        for stretch in (target[:a][::-1], target[b:]):
            tail = noisy(rs, stretch[:n - 4], 10) + stretch[n - 4:n]                 # (four matches at the end outweigh a substitution just before them)
            tails.append(tail[:n // 2] + tail[n // 2 + 1:] if cap % 2 else tail)
        reads += both("c%d" % cap, tailed(target, a, b, *tails))
    spec = check([("t", target)], reads, tmp_path, **W1)
    for name, _ in reads:
        assert [e["ei"] + e["ej"] for e in moves_of(spec, name)] == [int(name[1:-1])] * 2


def test_ext_max_cuts_an_extension_and_binds(tmp_path):
    rs = random.Random(77)
    target = M.random_seq(rs, 300)
    tails = [noisy(rs, stretch[:60], 10) for stretch in (target[:120][::-1], target[180:])]
    reads = both("x", tailed(target, 120, 180, *tails))
    for ext_max, reach in ((2000, 60), (37, 37), (16, 16)):
        spec = check([("t", target)], reads, tmp_path, ext_max=ext_max, **W1)
        assert all(e["ei"] == e["ej"] == reach for name, _ in reads for e in moves_of(spec, name)), ext_max


def test_n_runs_at_the_ends_of_reads_and_targets(tmp_path):
    rs = random.Random(55)
    t = M.random_seq(rs, 260)
    targets = [("clean", t), ("n_ends", "NNNNN" + t[5:100] + "NNN" + t[103:250] + "N" * 10)]
    reads = both("plain", t[20:240]) + both("n_read", "NNN" + t[23:230] + "NNNNNNN" + t[237:250]) + both("all", t)
    spec = check(targets, reads, tmp_path, secondary_ratio=0.0)
    assert spec["info"]["secondary"] > 0 and spec["extend"]["ends_moved"] > 6


def test_every_offset_of_a_packed_word_down_to_position_0(tmp_path):
    """cores that start and end at every offset of a 32-letter word, with tails that reach position 0 of the target and of the read across
    a word boundary, on both strands"""
    rs = random.Random(32)
    target = M.random_seq(rs, 260)
    reads = []
    for off in range(32):
        a, b = 36 + off, 150 + off
        tails = [noisy(rs, target[4:a][::-1], 10) + target[:4][::-1], noisy(rs, target[b:b + 40 + off // 3], 10)]       # (the last four letters intact)
        reads += both("o%02d" % off, tailed(target, a, b, *tails))
    spec = check([("t", target)], reads, tmp_path, **W1)
    rows = [l.split("\t") for l in spec["paf"].splitlines()]
    assert len(rows) == 64 and all(f[7] == "0" and (f[2] == "0" if f[4] == "+" else f[3] == f[1]) for f in rows)


# ------------------------------------------------------------------------------------------------ chunks, memory, contexts
@pytest.mark.parametrize("chunk_reads", [1, 7, 64])
def test_chunk_sizes_give_the_same_bytes(planted, tmp_path, chunk_reads):
    g = planted
    for n, (mode, spec) in enumerate(zip(MODES, g["specs"])):
        dev = device(g["targets"], g["read_list"], tmp_path, tag="c%d" % n, chunk_reads=chunk_reads, secondary_ratio=0.0, **mode)
        same(dev, spec, mode["align"], mode.get("eqx", False))
        assert dev["info"]["chunks"] == (24 + chunk_reads - 1) // chunk_reads


def test_a_chunk_over_the_extension_budget_is_split(tmp_path):
    """5 000 copies of one read of a core of 60 letters and two tails of 500 with every 4th letter substituted (250 runs of = and X an
    end, 8 bytes a run), on 6 identical targets: the 30 000 lines' alignment fits the device bytes a chunk may take (128 MiB), their
    60 000 extensions with columns and runs do not: the chunk is halved, nothing else changes"""
    rs = random.Random(9)
    t = M.random_seq(rs, 1100)
    tails = [noisy(rs, stretch[:500], 4) for stretch in (t[:520][::-1], t[580:])]
    targets = [("same%02d" % i, t) for i in range(6)]
    reads = [("copy%05d" % i, tailed(t, 520, 580, *tails)) for i in range(5000)]
    spec = X.map_reads(targets, reads, align=True, eqx=True, secondary_ratio=0.0, **W1)
    lines = spec["extend"]["lines"]
    ends = [e for m in spec["moves"][:6] for e in m]
    words, runs = sum((e["ei"] + e["ej"] + 15) // 16 for e in ends), sum(sum(ch in "=XID" for ch in A.cigar(e["columns"], True)) for e in ends)
    per_read = 12 * (24 + 24) + 12 * (24 + 32 + 16 + 8) + 4 * words + 8 * runs                      # the twelve ends of a read's six lines
    aligned = lines * (16 + 32 + 8 + 8) + 8 * spec["align"]["segments"] + 4 * lines * 8 + 8 * lines            # 120 columns' room (8 words) and one run a line
    assert lines == 30000 and all(e["ei"] + e["ej"] > 900 for e in ends) and aligned < 64 << 20
    assert 5000 * per_read > 128 << 20 > 2500 * per_read + (1 << 20)
    dev = device(targets, reads, tmp_path, align=True, eqx=True, secondary_ratio=0.0, **W1)
    # (the bytes and the counters; what same() checks line by line holds for the specification's lines, which these are)
    assert dev["paf"] == spec["paf"] and {k: dev["info"]["extend"][k] for k in X.COUNTERS} == spec["extend"]
    assert {k: dev["info"][k] for k in M.COUNTERS} == spec["info"] and {k: dev["info"]["align"][k] for k in A.COUNTERS} == spec["align"]
    assert dev["info"]["chunks"] == 2


@pytest.mark.parametrize("word", ["00000001", "ffffffff"])
def test_recycled_memory_does_not_reach_the_output(planted, tmp_path, word):
    """the module in a child whose device allocations are filled with a word first (TKSMSEQ_POISON): the same bytes"""
    g = planted
    env = dict(os.environ, TKSMSEQ_POISON=word)
    for flags, spec in (([], g["specs"][0]), (["-c"], g["specs"][1])):
        out = tmp_path / ("poisoned%d.paf" % len(flags))
        r = subprocess.run([EXE, "map", "-r", g["ref"], "--reads", g["reads"], "-o", str(out), "--extend", "-p", "0.0", "--chunk-reads", "10", *flags], capture_output=True,
                           text=True, env=env)
        assert r.returncode == 0, r.stderr[-600:]
        assert f"poison {word}:" in r.stderr and " 0 blocks" not in r.stderr
        assert out.read_text() == spec["paf"]


def test_same_context_twice_after_another_module_and_the_null_call(planted, tmp_path):
    from tksm_amd import _lib
    from tksm_amd.sequence import Sequencer
    g = planted
    s = Sequencer(0)
    try:
        for name, seq in g["targets"]:
            s.add_contig(name, seq)
        first = device(None, g["read_list"], tmp_path, tag="first", sequencer=s, secondary_ratio=0.0, align=True)
        mdf = "".join(f"+m{i}\t1\t\n{name}\t0\t{len(seq)}\t+\t\n" for i, (name, seq) in enumerate(g["targets"]))
        b = s.batch_from_mdf(mdf)
        records = s.run(b, target="perfect", fastq=True).records()
        b.free()
        assert len(records) == len(g["targets"])
        without = device(None, g["read_list"], tmp_path, tag="without", sequencer=s, extend=False, secondary_ratio=0.0, align=True)
        second = device(None, g["read_list"], tmp_path, tag="second", sequencer=s, chunk_reads=5, secondary_ratio=0.0)
        # extend == NULL: the bytes of tksmseq_map_align, with and without align
        lib = _lib.load()
        p = _lib.MapParams(15, 10, 500, 5000, 500, 3, 40, 0, 0.0, 5, 0, 0)
        ap = _lib.AlignParams(63, 0)
        for align, name in ((ctypes.byref(ap), "a"), (None, "n")):
            for call, extra in ((lib.tksmseq_map_extend, (None,)), (lib.tksmseq_map_align, ())):
                info, ainfo = _lib.MapInfo(), _lib.AlignInfo()
                out = tmp_path / f"null_{name}_{len(extra)}.paf"
                rc = call(s._ctx, ctypes.byref(p), align, *extra, g["reads"].encode(), str(out).encode(), ctypes.byref(info), ctypes.byref(ainfo), *extra)
                assert rc == 0 and info.lines == g["specs"][0]["info"]["lines"]
            assert (tmp_path / f"null_{name}_1.paf").read_bytes() == (tmp_path / f"null_{name}_0.paf").read_bytes()
        assert (tmp_path / "null_a_1.paf").read_text() == g["specs"][1]["base"] == without["paf"] and "extend" not in without["info"]
        assert (tmp_path / "null_n_1.paf").read_text() == g["specs"][0]["base"]
    finally:
        s.close()
    same(first, g["specs"][1], True)
    same(second, g["specs"][0], False)


def test_error_codes(planted, tmp_path):
    from tksm_amd import _lib
    from tksm_amd.sequence import Sequencer, TksmSeqError
    g = planted
    s = Sequencer(0)
    try:
        for name, seq in g["targets"]:
            s.add_contig(name, seq)
        for bad in (dict(ext_band=0), dict(ext_band=64), dict(ext_drop=0), dict(ext_drop=1001), dict(ext_max=0), dict(ext_max=32769)):
            with pytest.raises(TksmSeqError) as e:
                s.map(g["reads"], tmp_path / "o.paf", extend=True, **bad)
            assert e.value.code == _lib.EINVAL and "map: extend " in str(e.value), bad
        assert not (tmp_path / "o.paf").exists()
        edge = s.map(g["reads"], tmp_path / "edge.paf", extend=True, align=True, ext_band=63, ext_drop=1000, ext_max=32768)
        assert edge["extend"]["lines"] == edge["lines"] > 0
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ the route this is for
def test_transcribe_sequence_map_extend_model_truncation(tmp_path):
    """about 600 molecules: transcribe -> sequence (Badread, identity 84 / 99 / 5.5) -> tksm map [-c] [--extend] -> model-truncation and
    model-sequence: every --extend line holds its line without --extend, and both consumers read the extended files"""
    from test_map_gpu import transcriptome
    from tksm_amd.sequence import Sequencer
    d = tmp_path
    rs = random.Random(79)
    contigs, gtf, spliced = transcriptome(rs, n=20)
    (d / "ann.gtf").write_text(gtf)
    (d / "ab.tsv").write_text("transcript_id\ttpm\tcell_barcode\n" + "".join(f"{tid}\t{rs.randint(1, 30)}\t.\n" for tid, _ in spliced))
    s = Sequencer(0)
    try:
        for name, seq in contigs:
            s.add_contig(name, seq)
        s.add_gtf(str(d / "ann.gtf"))
        s.set_identity(84.0, 99.0, 5.5); s.load_error_model(ERR_MODEL); s.load_qscore_model(QS_MODEL)
        plan = s.transcribe_plan(str(d / "ab.tsv"), 600, seed=7)
        batch = plan.batch()
        records = s.run(batch, target="badread", fastq=True, compute_qual=True, seed=7).records()
        batch.free()
        plan.close()
    finally:
        s.close()
    (d / "reads.fq").write_bytes(b"".join(records))
    ref = M.write_fasta(d / "tx.fa", spliced)
    pafs = {}
    for name, flags in (("plain", []), ("ext", ["--extend"]), ("c", ["-c"]), ("c_ext", ["-c", "--extend"])):
        r = subprocess.run([EXE, "map", "-r", ref, "--reads", str(d / "reads.fq"), "-o", str(d / (name + ".paf")), "-p", "0.0", "--verbosity", "INFO", *flags],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-600:]
        assert ("lines extended" in r.stderr + r.stdout) == ("--extend" in flags)
        pafs[name] = (d / (name + ".paf")).read_text()
    contains(pafs["ext"], pafs["plain"])
    contains(pafs["c_ext"], pafs["c"])
    assert [l.split("\t")[:9] for l in pafs["ext"].splitlines()] == [l.split("\t")[:9] for l in pafs["c_ext"].splitlines()]
    lines = pafs["ext"].splitlines()
    primary = sum("\ttp:A:P\t" in l for l in lines)
    assert primary > 400

    def lost(paf):
        return sorted(int(f[7]) + int(f[6]) - int(f[8]) for f in (l.split("\t") for l in paf.splitlines()) if f[12] == "tp:A:P")
    before, after = lost(pafs["plain"]), lost(pafs["ext"])
    print("bases lost per primary line (tstart + tlen - tend), median / mean: chains %d / %.1f, extended %d / %.1f" %
          (before[len(before) // 2], sum(before) / len(before), after[len(after) // 2], sum(after) / len(after)))
    s = Sequencer(0)
    try:
        for tid, seq in spliced:
            s.add_contig(tid, seq)
        info = s.model_sequence([str(d / "reads.fq")], d / "c_ext.paf", error_out=d / "e.gz", qscore_out=d / "q.gz")
        assert info["lines"] == len(lines) and info["used"] == primary
        assert info["skipped_no_cigar"] == info["skipped_cigar_op"] == info["skipped_unknown_read"] == info["skipped_unknown_target"] == 0
        s.model_truncation(d / "ext.paf", d / "truncation.json")
        s.model_truncation(d / "c_ext.paf", d / "truncation_c.json")
    finally:
        s.close()
    assert (d / "truncation.json").stat().st_size > 100
