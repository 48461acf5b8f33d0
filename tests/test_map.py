"""map without a device: the specification (tests/map_spec.py) against things that are not the specification -- a second statement of the
window definition, exhaustive search over the chains of small groups, recorded cases small enough to follow by hand -- the proof that
the inputs of the device's tests reach their cases (a predecessor at the edge of the window of 64 and past it, ties across tiles of
anchors, windows around the sketch tiles, a secondary chain on the ratio), the host-only code under ASan / UBSan, the exports, and the
argument checks of `tksm map`."""
import ctypes
import itertools
import json
import os
import random
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

import map_align_spec as A
import map_spec as M

EXE = os.path.join(ROOT, "tksm_amd", "tksm")
KNOWN = json.load(open(os.path.join(GOLDEN, "map_known_answers.json")))["cases"]


def random_with_n(rs, n, p_n=0.03):
    return "".join("N" if rs.random() < p_n else rs.choice("ACGT") for _ in range(n))


@pytest.mark.parametrize("k,w", [(4, 1), (5, 3), (15, 10), (28, 64)])
def test_minimizers_against_a_second_statement_of_the_windows(k, w):
    """position p is a minimizer exactly when some window that holds p has no valid position that is smaller in (h, p)"""
    rs = random.Random(k * 100 + w)
    for trial in range(12):
        seq = random_with_n(rs, rs.choice([k - 1, k, k + w - 2, k + w - 1, k + w, 3 * (k + w), 400]), 0.0 if trial % 3 == 0 else 0.03)
        n = len(seq) - k + 1
        expect = []
        if n > 0:
            key = {p: (M.kmer(seq, p, k)[0], p) for p in range(n) if M.kmer(seq, p, k)}
            last = max(0, n - w)
            for p in sorted(key):
                windows = [j for j in range(max(0, p - w + 1), min(p, last) + 1)]
                if any(all(key[p] <= key[o] for o in range(j, min(j + w, n)) if o in key) for j in windows):
                    expect.append(p)
        got = M.minimizers(seq, k, w)
        assert [p for _, p, _ in got] == expect
        for h, p, s in got:
            assert (h, s) == M.kmer(seq, p, k)
    assert M.minimizers("ACGT" * 20, 4, 3) == [m for m in M.minimizers("acgt" * 20, 4, 3)]


def test_kmer_code_strand_and_palindromes():
    assert M.kmer("ACGT", 0, 4) is None                       # its own reverse complement
    assert M.kmer("ACNT", 0, 4) is None and M.kmer("ACG", 0, 4) is None
    h, s = M.kmer("AAAAC", 0, 5)                              # fwd 0b0000000001 < rev (GTTTT)
    assert s == 0 and h == M.mix(1)
    h2, s2 = M.kmer("GTTTT", 0, 5)
    assert s2 == 1 and h2 == h
    assert M.mix(0) == 0 and M.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF    # the first output of splitmix64 from state 0
    assert M.cost(0, 15) == 0 and M.cost(1, 15) == 0 and M.cost(7, 15) == 1 + 1 and M.cost(100, 15) == 15 + 3


def exhaustive(anchors, k, max_gap, bandwidth):
    """the best score over all chains: every increasing subsequence whose links are all admissible, scored link by link"""
    best = k
    n = len(anchors)
    for size in range(2, n + 1):
        for sub in itertools.combinations(range(n), size):
            sc = k
            for a, b in zip(sub, sub[1:]):
                dt, dq = anchors[b][0] - anchors[a][0], anchors[b][1] - anchors[a][1]
                if dt <= 0 or dq <= 0 or dt > max_gap or dq > max_gap or abs(dt - dq) > bandwidth:
                    sc = None
                    break
                sc += min(k, dt, dq) - M.cost(abs(dt - dq), k)
            if sc is not None:
                best = max(best, sc)
    return best


def test_chain_score_against_exhaustive_search():
    """The recurrence restarts a chain at f = k where a link would not lift it above k, and so does the best subsequence (a prefix worth
    less than nothing is dropped): with at most 10 anchors the 64-predecessor window never binds and the maxima agree (where the window
    binds: test_tandem_repeats_put_the_diagonal_predecessor_at_the_edge_of_the_window)."""
    rs = random.Random(3)
    for trial in range(150):
        k = rs.choice([5, 15])
        n = rs.randint(1, 10)
        anchors = sorted({(rs.randint(0, 60), rs.randint(0, 60)) for _ in range(n)})
        if trial % 3 == 0:                                    # mostly colinear
            anchors = sorted({(p, p + rs.choice([0, 0, 0, 1, -2, 7])) for p, _ in anchors if p >= 2})
            if not anchors:
                continue
        gap, bw = rs.choice([(5000, 500), (20, 3), (8, 0)])
        c = M.chain(anchors, k, gap, bw)
        # the best chain that ends anywhere, prefix scores never below k: a subsequence may start anywhere, so the exhaustive maximum over
        # suffix-restarted sums is the maximum over plain sums of its own suffixes
        assert c["score"] == exhaustive(anchors, k, gap, bw), (anchors, k, gap, bw)
        path = c["path"]
        assert c["cnt"] == len(path) and all(a < b for a, b in zip(path, path[1:]))
        assert c["tstart"] == anchors[path[0]][0] and c["tend"] == anchors[path[-1]][0] + k
        assert c["nmatch"] == k + sum(min(k, anchors[b][0] - anchors[a][0], anchors[b][1] - anchors[a][1]) for a, b in zip(path, path[1:]))


def test_chain_tie_takes_the_later_predecessor_and_the_earlier_end():
    k = 5
    c = M.chain([(0, 0), (1, 1), (10, 10)], k)                # 5, 5 + 1, 6 + 5
    assert c["score"] == 1 + k + k and c["path"] == [0, 1, 2]
    c = M.chain([(0, 0), (0, 2), (10, 10)], k)                # (0, 0): gap 0, score 10; (0, 2): gap 2, cost 0 + 0, score 10: a tie
    assert c["score"] == 10 and c["path"] == [1, 2]
    # two ends with the same f: the smaller index ends the chain
    c = M.chain([(0, 0), (5, 5), (7000, 7000), (7005, 7005)], k, 5000, 500)
    assert c["score"] == 10 and c["path"] == [0, 1]


def test_chain_reports_what_its_loop_decided():
    """f, pred, ties and best_is_k of every anchor against the step stated once more over the f that chain() returned, for the window of
    64, a window of 3 and none; window = 64 is the default, and None is what the exhaustive search knows"""
    rs = random.Random(4)
    for trial in range(60):
        k = rs.choice([5, 15])
        anchors = sorted({(rs.randint(0, 40), rs.randint(0, 40)) for _ in range(rs.randint(1, 12))})
        gap, bw = rs.choice([(5000, 500), (20, 3)])
        assert M.chain(anchors, k, gap, bw) == M.chain(anchors, k, gap, bw, 64)
        if len(anchors) <= 10:
            assert M.chain(anchors, k, gap, bw, None)["score"] == exhaustive(anchors, k, gap, bw)
        for window in (64, 3, None):
            c = M.chain(anchors, k, gap, bw, window)
            for i, (p, q) in enumerate(anchors):
                sc = {}
                for j in range(i):
                    dt, dq = p - anchors[j][0], q - anchors[j][1]
                    if (window is None or i - j <= window) and 0 < dt <= gap and 0 < dq <= gap and abs(dt - dq) <= bw:
                        sc[j] = c["f"][j] + min(k, dt, dq) - M.cost(abs(dt - dq), k)
                top = max(sc.values()) if sc else None
                assert c["ties"][i] == [j for j in sorted(sc) if sc[j] == top] and c["best_is_k"][i] == (top == k)
                linked = top is not None and top > k
                assert c["pred"][i] == (c["ties"][i][-1] if linked else None) and c["f"][i] == (top if linked else k)
            assert all(c["pred"][b] == a for a, b in zip(c["path"], c["path"][1:])) and c["pred"][c["path"][0]] is None


def test_chain_classes_on_groups_made_by_hand():
    k = 5
    none = dict.fromkeys(M.CLASSES, 0)
    # 63 anchors that link to nothing (dt = 0 from the first, dq < 0 to the last) between (0, 0) and (1, 1): the one link spans 64
    group = [(0, 0)] + [(0, 1000 + x) for x in range(63)] + [(1, 1)]
    assert M.chain_classes(group, k, 5000, 500) == dict(none, distance_64=1)
    assert M.chain(group, k)["pred"][64] == 0 and M.chain(group, k, window=63)["pred"][64] is None
    # the tie of test_chain_tie_takes_the_later_predecessor_and_the_earlier_end behind 62, 63 and 64 anchors that link to nothing
    for fill, what in ((62, "ties_previous_tile"), (63, "ties_both_tiles"), (64, "ties_same_tile")):
        group = [(x, 9000 - x) for x in range(fill)] + [(100, 0), (100, 2), (110, 10)]
        c = M.chain(group, k)
        assert c["ties"][fill + 2] == [fill, fill + 1] and c["pred"][fill + 2] == fill + 1
        assert M.chain_classes(group, k, 5000, 500) == dict(none, end_ties=0, **{what: 1}), fill
    assert M.chain_classes([(0, 0), (0, 2), (10, 10)], k, 5000, 500) == none                     # (a tie below anchor 64 is in no class)
    # dt = 1, dq = 5: 5 + min(5, 1, 5) - cost(4) = 5 + 1 - 1 = k exactly, which does not link
    assert M.cost(4, k) == 1 and M.chain_classes([(0, 0), (1, 5)], k, 5000, 500) == dict(none, best_is_k=1, end_ties=1)
    assert M.chain_classes([(0, 0), (5, 5), (7000, 7000), (7005, 7005)], k, 5000, 500) == dict(none, end_ties=1)


def test_tandem_repeats_put_the_diagonal_predecessor_at_the_edge_of_the_window():
    """M.tandem_case: the predecessor that continues the diagonal lies r anchors back.  What each r is there for is shown here from the
    specification alone, so that the device's test can rely on it"""
    case = M.tandem_case()
    targets, reads, params = case["targets"], case["reads"], case["params"]
    out = M.map_reads(targets, reads, memo=case["memo"], **params)
    unbounded = M.map_reads(targets, [r for r in reads if r[0] in ("f65", "r65")], pred_window=None, **params)     # (all predecessors: a second a read)
    assert out["info"]["mapped"] == 8 and out["info"]["lines"] == 8
    chain = {name: lines[0][3] for name, lines in out["lines"].items()}
    free = {name: lines[0][3] for name, lines in unbounded["lines"].items()}
    for s in "fr":
        back = {r: [i - j for i, j in enumerate(chain["%s%d" % (s, r)]["pred"]) if j is not None] for r in M.TANDEM_REPEATS}
        assert back[63].count(63) > 1000 and 64 not in back[63]
        assert back[64].count(64) > 1000 and M.classes_of_chain(chain[s + "64"])["distance_64"] == back[64].count(64)
        path = chain[s + "64"]["path"]
        # (20 r - 14 read positions: the first 6 phases of the unit have 64 of them, the other 14 have 63)
        assert len(path) > 40 and {b - a for a, b in zip(path, path[1:])} == {63, 64} and sum(b - a == 64 for a, b in zip(path, path[1:])) >= 10
        # 65: the diagonal is out of reach; what the window still holds gives a shorter chain than all predecessors would
        assert chain[s + "65"]["cnt"] > 1 and chain[s + "65"]["score"] < free[s + "65"]["score"] == chain[s + "64"]["score"]
        assert chain[s + "66"]["cnt"] == 1 and chain[s + "66"]["score"] == params["k"]
    # a window that is one too small or one too large writes another PAF: 63 loses the links of r = 64 (and changes r = 65), 65 reaches
    # the diagonal of r = 65.  (r = 64 alone cannot tell 65 from 64: every link it has is inside both.)
    both = [r for r in reads if r[0] in ("f64", "r64", "f65", "r65")]
    paf = {w: M.map_reads(targets, both, pred_window=w, **params)["paf"] for w in (63, 64, 65)}
    assert paf[63] != paf[64] != paf[65]
    for name, window, differs in (("f64", 63, True), ("f64", 65, False), ("f65", 63, True), ("f65", 65, True)):
        one = [r for r in reads if r[0] == name]
        assert (M.map_reads(targets, one, pred_window=window, **params)["paf"] != M.map_reads(targets, one, **params)["paf"]) == differs, (name, window)


def test_dense_groups_reach_every_kind_of_tie():
    """A.dense_case: over k = 4, 5 and 6 the written chains hold ties whose candidates lie in the anchor's own tile of 64, in the tile
    before and in both, a best candidate of exactly k, and two ends of the same score.  (Where a count is 0 the seeds of the case change,
    not this condition.)"""
    total = dict.fromkeys(M.CLASSES, 0)
    for k in A.DENSE:
        targets, reads, params = A.dense_case(k)
        out = M.map_reads(targets, reads, **params)
        assert out["info"]["mapped"] == 6 and {lines[0][1] for lines in out["lines"].values()} == {0, 1}
        for what, n in M.classes_of_lines(out).items():
            total[what] += n
    assert all(total[what] >= 1 for what in M.CLASSES if what != "distance_64"), total


SKETCH_KW = [(15, 10), (15, 1), (15, 64), (4, 64), (28, 64)]


@pytest.mark.parametrize("k,w", SKETCH_KW)
def test_sketch_case_has_windows_around_the_tiles_and_minimizers_across_them(k, w):
    targets, reads = M.sketch_case(k, w)
    for (_, seq), n in zip(targets, M.SKETCH_WINDOWS):
        assert max(0, len(seq) - k + 1 - w) + 1 == n
    out = M.map_reads(targets, reads, k=k, w=w, min_count=1, min_score=0)
    assert out["info"]["mapped"] == len(reads) == 12
    same, other, straddle = (sum(x) for x in zip(*[M.tile_boundaries(seq, k, w) for _, seq in targets + reads]))
    # 5 of the 6 lengths have a window 192, 3 of them a window 384: 2 * (5 + 3) boundaries over targets and reads
    assert same + other <= 16 and straddle >= 1
    assert (other >= 1) if w == 1 else (same >= 1)


def test_select_case_scores_lie_on_the_ratio_and_one_below():
    targets, reads = M.select_case()
    every = M.map_reads(targets, reads, max_secondary=10, **dict(M.SELECT, secondary_ratio=0.0))
    score = {name: [(l[0], l[3]["score"]) for l in lines] for name, lines in every["lines"].items()}
    assert score["exact"] == [("exact_all", 100), ("exact_prefix", 80)] and score["below"] == [("below_all", 100), ("below_prefix", 79)]
    assert score["three"] == [("three%d" % i, 100) for i in range(3)] and score["four"] == [("four%d" % i, 100) for i in range(4)]
    assert 80 * 1000 == M.permille(0.8) * 100 > 79 * 1000
    out = M.map_reads(targets, reads, max_secondary=2, **M.SELECT)
    written = {name: [l[0] for l in lines] for name, lines in out["lines"].items()}
    assert written == {"three": ["three0", "three1", "three2"], "four": ["four0", "four1", "four2"], "exact": ["exact_all", "exact_prefix"], "below": ["below_all"]}
    alone = M.map_reads(targets, reads, max_secondary=0, **M.SELECT)
    assert {name: [l[0] for l in lines] for name, lines in alone["lines"].items()} == {"three": ["three0"], "four": ["four0"], "exact": ["exact_all"], "below": ["below_all"]}
    mapq = {l.split("\t")[0]: int(l.split("\t")[11]) for l in alone["paf"].splitlines()}
    assert mapq == {"three": 0, "four": 0, "exact": 60 * 20 // 100, "below": 60 * 21 // 100}      # from the second score, written or not


def test_recorded_cases():
    assert [c["name"] for c in KNOWN] == ["reverse_31", "reverse_30", "tie_of_identical_targets", "secondary_at_the_ratio_exactly", "secondary_one_below_the_ratio",
                                          "one_candidate_more_than_max_secondary"]
    for c in KNOWN:
        out = M.map_reads([tuple(t) for t in c["targets"]], [tuple(r) for r in c["reads"]], **c["params"])
        assert out["paf"] == c["paf"], c["name"]
        assert out["info"] == c["info"], c["name"]
    by = {c["name"]: [l.split("\t") for l in c["paf"].splitlines()] for c in KNOWN}
    for name, n in (("reverse_31", 31), ("reverse_30", 30)):
        (f,) = by[name]
        case = next(c for c in KNOWN if c["name"] == name)
        read, target = case["reads"][0][1], case["targets"][0][1]
        assert f[4] == "-" and int(f[1]) == n
        # the interval is given in the read as sequenced: its reverse complement is the target's interval, letter for letter
        assert M.revcomp(read[int(f[2]):int(f[3])]) == target[int(f[7]):int(f[8])]
    p, s = by["tie_of_identical_targets"]
    assert (p[5], p[11], p[12]) == ("tA", "0", "tp:A:P") and (s[5], s[11], s[12]) == ("tB", "0", "tp:A:S") and p[14] == s[14]
    p, s = by["secondary_at_the_ratio_exactly"]
    assert (p[14], s[14]) == ("s1:i:50", "s1:i:40") and 40 * 1000 == M.permille(0.8) * 50 and p[11] == str(60 * 10 // 50)
    (p,) = by["secondary_one_below_the_ratio"]
    assert p[14] == "s1:i:50" and p[11] == str(60 * 11 // 50)
    case = next(c for c in KNOWN if c["name"] == "one_candidate_more_than_max_secondary")
    assert len(case["targets"]) == case["params"]["max_secondary"] + 2 and [f[5] for f in by[case["name"]]] == ["t0", "t1", "t2"]


def test_specification_maps_generated_reads_to_their_origin(tmp_path):
    g = M.generate(tmp_path, seed=1, n_targets=12, n_reads=40)
    out = M.run(g["ref"], g["reads"])
    assert out["info"]["mapped"] == 40 and out["info"]["secondary"] == 0
    for name, (tname, strand, a, b) in g["truth"].items():
        (line,) = out["lines"][name]
        assert line[0] == tname and line[1] == strand and abs(line[3]["tstart"] - a) <= 9 and abs(line[3]["tend"] - b) <= 9
    with pytest.raises(ValueError):
        M.run(g["ref"], g["reads"], k=3)
    with pytest.raises(ValueError):
        M.run(g["ref"], g["reads"], secondary_ratio=1.5)


def test_paf_through_the_reader_of_abundance(tmp_path):
    """the columns abundance reads (1, 2, 6, 8, 10, 11), through the reader and the compatibility rule of its specification: every exact
    read survives with its own transcript as its only hit"""
    import abundance_spec
    g = M.generate(tmp_path, seed=2, n_targets=6, n_reads=30)
    out = M.run(g["ref"], g["reads"])
    rows = [l.split("\t") for l in out["paf"].splitlines()]
    assert all(len(r) == 15 and int(r[2]) < int(r[3]) <= int(r[1]) and int(r[7]) < int(r[8]) <= int(r[6]) and int(r[9]) <= int(r[10]) for r in rows)
    (tmp_path / "spec.paf").write_text(out["paf"])
    tnames, reads = abundance_spec.parse_paf(str(tmp_path / "spec.paf"))
    comp = abundance_spec.compatibility(reads)
    assert len(comp) == 30
    for name, hits in comp.items():
        assert [(tnames[t], w) for t, w in hits] == [(g["truth"][name][0], 1.0)]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """tools/sanitize_map_host.cpp built with ASan + UBSan and run on reads around the word sizes: {key: [lines]} of what it printed"""
    d = tmp_path_factory.mktemp("map_sanitize")
    exe = d / "sanitize_map_host"
    csrc = os.path.join(ROOT, "tksm_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", csrc, "-o", str(exe),
                    os.path.join(ROOT, "tools", "sanitize_map_host.cpp"), os.path.join(csrc, "map_host.cpp"), os.path.join(csrc, "ms_host.cpp"),
                    os.path.join(csrc, "abund_host.cpp"), "-lz"], check=True)
    rs = random.Random(9)
    reads = [("r%d" % i, random_with_n(rs, n, 0.1)) for i, n in enumerate([0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200])]
    reads.append(("lower", "acgtnACGTRY"))
    fq = M.write_fastq(d / "reads.fq", reads)
    r = subprocess.run([str(exe), fq], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        key, _, rest = line.partition(" ")
        out.setdefault(key, []).append(rest)
    out["reads"], out["raw"] = reads, r.stdout.splitlines()
    return out


def test_host_code_under_sanitizers(sanitized):
    s = sanitized
    ok = {l.split(" ")[0]: l.split(" ")[1] == "1" for l in s["params"]}
    assert [k for k, v in ok.items() if v] == ["defaults", "k4w64"] and len(ok) == 16
    for l in s["params"]:
        label, good, *msg = l.split(" ")
        assert good == "1" or " ".join(msg).startswith("map: ")
    for l in s["permille"]:
        ratio, P = l.split(" ")
        assert int(P) == M.permille(float(ratio))
    assert len(s["tiles"]) == 90
    for l in s["tiles"]:
        k, w, length, windows, tiles, last = (int(x) for x in l.split(" "))
        n = length - k + 1
        expect = 0 if n <= 0 else max(0, n - w) + 1
        assert windows == expect and tiles == (expect + 191) // 192 and last == (0 if not tiles else (tiles - 1) * 192)
    packed = [l.split(" ") for l in s["packed"]]
    reads = s["reads"]
    assert len(packed) == 2 * len(reads)
    voff = 0
    for i, (name, seq) in enumerate(reads):
        want = "".join(c if c in "ACGT" else "N" for c in seq.upper())
        together, alone = packed[i], packed[len(reads) + i]
        assert together[:3] == ["0", str(i), str(len(seq))] and int(together[3]) == voff and (together[4] if len(together) > 4 else "") == want
        assert alone[:4] == ["1", str(i), str(len(seq)), "0"] and (alone[4] if len(alone) > 4 else "") == want
        voff += (len(seq) + 31) // 32
    assert s["pack_words"][0] == "0 0 %d %d" % (2 * voff, voff)
    assert s["paf"][0] == "read/1\t200\t4\t131\t+\ttx\t1000\t10\t140\t101\t130\t60\ttp:A:P\tcm:i:9\ts1:i:120"
    assert s["raw"][-2:] == ["read/1\t200\t69\t196\t-\ttx\t1000\t10\t140\t101\t130\t0\ttp:A:S\tcm:i:9\ts1:i:120", "\t0\t0\t0\t+\t\t0\t0\t0\t0\t0\t0\ttp:A:P\tcm:i:0\ts1:i:0"]


def test_exports_and_header_agree():
    from tksm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    for s in ("tksmseq_map", "tksmseq_map_main"):
        assert s in _lib.SYMBOLS and re.search(rf"\b{s}\s*\(", header) and hasattr(lib, s)
    assert ctypes.sizeof(_lib.MapParams) == 56 and ctypes.sizeof(_lib.MapInfo) == 152
    for struct, cls in (("tksmseq_map_info", _lib.MapInfo), ("tksmseq_map_params", _lib.MapParams)):
        fields = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        names = [n.split("[")[0] for part in re.findall(r"(?:uint64_t|int64_t|int32_t|float|double|const char\*)\s+([^;]+);", fields) for n in re.split(r",\s*", part.strip())]
        assert names == [n for n, _ in cls._fields_], struct
    kernels_h = open(os.path.join(ROOT, "tksm_amd", "csrc", "map_kernels.h")).read()
    host_h = open(os.path.join(ROOT, "tksm_amd", "csrc", "map_host.h")).read()
    assert int(re.search(r"MAP_TILE = (\d+)", kernels_h).group(1)) == int(re.search(r"MAP_TILE_WINDOWS = (\d+)", host_h).group(1)) == 192
    assert int(re.search(r"MAP_PRED_WINDOW = (\d+)", kernels_h).group(1)) == M.PRED_WINDOW
    # the product does not import the specification, and the kernels of this module use no floating point
    for root, _, files in os.walk(os.path.join(ROOT, "tksm_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip")):
                assert "map_spec" not in open(os.path.join(root, f), errors="replace").read(), f
    kernels = open(os.path.join(ROOT, "tksm_amd", "csrc", "map_kernels.hip")).read()
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", kernels))
    import __graft_entry__ as g
    assert "k_map_chain" in g.NO_SPILL_MAP and "k_map_sketch" in g.NO_SPILL_MAP


def _module(*args):
    return subprocess.run([EXE, "map", *[str(a) for a in args]], capture_output=True, text=True)


def test_module_argument_checks_and_exit_codes(tmp_path):
    g = M.generate(tmp_path, seed=3, n_targets=2, n_reads=2)
    out = tmp_path / "o.paf"
    need = ["-r", g["ref"], "--reads", g["reads"], "-o", out]
    r = _module()
    assert r.returncode == 2 and "map: error:" in r.stderr and "-r/--reference, --reads, -o/--output" in r.stderr
    r = _module(*need[2:])
    assert r.returncode == 2 and "-r/--reference" in r.stderr and "--reads" not in r.stderr
    r = _module(*need[:2], *need[4:])
    assert r.returncode == 2 and "--reads" in r.stderr and "-r/--reference" not in r.stderr
    r = _module(*need[:4])
    assert r.returncode == 2 and "-o/--output" in r.stderr and "--reads" not in r.stderr
    r = _module(*need, "--nope")
    assert r.returncode == 2 and "--nope" in r.stderr
    r = _module(*need, "-i", "x")
    assert r.returncode == 2 and "-i" in r.stderr
    for flag, bad in (("-k", "3"), ("-k", "29"), ("-w", "0"), ("-w", "65"), ("-p", "1.5"), ("-p", "-0.1"), ("--max-occ", "0"), ("--max-gap", "-1"), ("--bandwidth", "-1"),
                      ("--min-count", "0"), ("--min-score", "-1"), ("-N", "-1"), ("-N", "1001"), ("--chunk-reads", "-1")):
        r = _module(*need, flag, bad)
        assert r.returncode == 2 and f"map: error: {flag} must" in r.stderr, (flag, bad, r.stderr)
    assert _module(*need, "-k", "four").returncode == 2 and _module(*need, "-p", "0.8x").returncode == 2
    r = _module(*need, "--verbosity", "LOUD")
    assert r.returncode == 1 and "unknown verbosity level" in r.stderr
    assert _module("-h").returncode == 0 and "--max-occ" in _module("--help").stdout
    assert not out.exists() and not os.path.exists(str(out) + ".tmp")
    r = subprocess.run([EXE, "list"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["sequence", "pcr", "truncate", "polyA", "tag", "scb", "flip"]
    r = subprocess.run([EXE, "nonesuch"], capture_output=True, text=True)
    assert r.returncode == 1 and "Unknown kisim" in r.stderr and "and `map`" in r.stderr
