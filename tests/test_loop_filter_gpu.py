"""k_loop with its first-threshold look-ups answered from the bounds table in LDS (tksm_amd/csrc/loop_filter.h): whole records
against the CPU oracle, byte for byte.  Every context here is created with the knobs of test_gpu_parity's "fast" path and without
predicted stragglers, so that the lane-per-read kernel runs every visit of every read.  The cases sit where the table could go wrong:
thresholds on its byte boundaries, the other shipped models, k-mers cut from HBM words, draw positions that no longer fit 16 bits
(they are recomputed in phase 2, not read back from LDS), ranges of one to a few k-mers, and a type-0 model (no table at all)."""
import gzip
import os

import numpy as np
import pytest

from conftest import ERR_MODEL, MODELS, QS_MODEL

pytestmark = pytest.mark.gpu
SEED = 4321
_EM = {}                                                         # parsed oracle error models, by path


def _oracle_em(po, oracle_models, path):
    if path == ERR_MODEL:
        return oracle_models["em"]
    if path not in _EM:
        _EM[path] = po.ErrorModel(path)
    return _EM[path]


@pytest.fixture(scope="module")
def genome():
    rs = np.random.RandomState(17)
    return {f"chr{c + 1}": rs.choice(np.frombuffer(b"ACGT", np.uint8), 150_000).tobytes().decode() for c in range(2)}


def _seqr(genome, err, qs):
    from tksm_amd.sequence import Sequencer
    with pytest.MonkeyPatch.context() as mp:                     # (read when the context is created)
        for k, v in (("TKSMSEQ_FORCE_SLOW", "0"), ("TKSMSEQ_SMALL_ALN", "0"), ("TKSMSEQ_TAIL_CUT", "0"), ("TKSMSEQ_WAVE_LOOP", "0"),
                     ("TKSMSEQ_TAIL_WAVE", "0"), ("TKSMSEQ_EARLY_TAIL", "0")):
            mp.setenv(k, v)
        s = Sequencer(0)
    for name, seq in genome.items():
        s.add_contig(name, seq)
    s.set_identity(84.0, 99.0, 5.5)
    s.load_error_model(err)
    s.load_qscore_model(qs)
    return s


def _molecules(rs, genome, n, lo, hi):
    names = list(genome)
    mols = []
    for i in range(n):
        c = names[i % len(names)]
        ln = int(rs.randint(lo, hi + 1))
        st = int(rs.randint(0, len(genome[c]) - ln))
        mols.append((f"m{i}", [(c, st, st + ln, "+-"[int(rs.randint(2))], "")]))
    return mols


def _check(s, po, genome, mols, em, qm, compute_q, first=11, stride=3):
    text = "".join(f"+{m}\t1\t\n" + "".join(f"{c}\t{a}\t{b}\t{st}\t{md}\n" for c, a, b, st, md in ivs) for m, ivs in mols)
    with pytest.MonkeyPatch.context() as mp:
        for k in ("TKSMSEQ_FORCE_SLOW", "TKSMSEQ_SMALL_ALN", "TKSMSEQ_TAIL_CUT", "TKSMSEQ_WAVE_LOOP", "TKSMSEQ_TAIL_WAVE", "TKSMSEQ_EARLY_TAIL"):
            mp.setenv(k, "0")
        recs = s.run(s.batch_from_mdf(text), target="badread", fastq=True, compute_qual=compute_q, seed=SEED, first_read_index=first,
                     stride=stride).records()
    dg = s.run_diagnostics()
    assert dg["rounds"] > 0 and dg["exact_kernel_reads"] == 0, dg          # the round pipeline did all of it
    ident = po.Identities(84.0, 5.5, 99.0)
    assert len(recs) == len(mols)
    for i, (mid, ivs) in enumerate(mols):
        want, st = po.badread_record(True, SEED, first + stride * i, po.splice(genome, ivs), ident, em, qm, compute_q, mid)
        assert st.band_fail == 0
        assert recs[i] == want, (i, mid)


def _synthetic_model(path, k):
    """every k-mer's no-change probability a multiple of 1/256, so that its first threshold is a multiple of 2^24: steps 0 and 255
    occur, and the four k-mers under one key and one line of the threshold table go step, step + 1, step, step + 1.  One alternative
    (a substitution in the middle) takes 3/4 of the rest; what is left is the random change."""
    steps = set()
    with gzip.open(path, "wt") as f:
        for idx in range(4 ** k):
            kmer = "".join("ACGT"[(idx >> (2 * (k - 1 - j))) & 3] for j in range(k))
            base = (idx >> 2) * 37 % 255                                   # by key: every value 0 .. 254 (37 is coprime to 255)
            m = base + (idx & 1)
            steps.add(m)
            mid = k // 2
            alt = kmer[:mid] + "ACGT"[("ACGT".index(kmer[mid]) + 1 + (idx >> 4) % 3) % 4] + kmer[mid + 1:]
            f.write(f"{kmer},{m / 256:.8f};{alt},{0.75 * (256 - m) / 256:.10f};\n")
    assert 0 in steps and 255 in steps


@pytest.mark.parametrize("k", [5, 7])
def test_thresholds_on_the_byte_boundaries(tmp_path, po, genome, k):
    path = str(tmp_path / f"edges{k}.error.gz")
    _synthetic_model(path, k)
    em, qm = po.ErrorModel(path), po.QScoreModel("random")
    assert em.k == k and em.type == 1
    t0 = em.cdf[:, 0].astype(np.int64)
    assert (t0 % (1 << 24) == 0).all() and t0.min() == 0 and t0.max() == 255 << 24
    assert (np.abs(t0[1::2] - t0[0::2]) == 1 << 24).all()
    s = _seqr(genome, path, "random")
    _check(s, po, genome, _molecules(np.random.RandomState(k), genome, 2048, 150, 400), em, qm, False)
    s.close()


@pytest.mark.parametrize("model", ["nanopore2020", "nanopore2018", "pacbio2016"])
def test_shipped_models(po, oracle_models, genome, model):
    """2 048 reads inside the 64 fragment words of a lane; 64 reads of 1 100 - 1 300 bases: windowed re-estimation, and k-mers beyond
    the words in LDS read from HBM"""
    err = os.path.join(MODELS, f"{model}.error.gz")
    em, qm = _oracle_em(po, oracle_models, err), po.QScoreModel("random")
    s = _seqr(genome, err, "random")
    rs = np.random.RandomState(29)
    _check(s, po, genome, _molecules(rs, genome, 2048, 200, 400), em, qm, False)
    _check(s, po, genome, _molecules(rs, genome, 64, 1100, 1300), em, qm, False, first=5, stride=1)
    s.close()


def test_with_qscores(po, oracle_models, genome):
    s = _seqr(genome, ERR_MODEL, QS_MODEL)
    _check(s, po, genome, _molecules(np.random.RandomState(31), genome, 512, 200, 400), oracle_models["em"], oracle_models["qm"], True)
    s.close()


def test_short_reads_and_positions_beyond_16_bits(po, oracle_models, genome):
    """reads of 1 - 8 bases (a range of k + 1 to k + 8 k-mers; k = 1 with the random model below: 2 to 9); one 70 kb molecule beside
    63 short ones: its draw positions pass 65 535"""
    em, qm = oracle_models["em"], po.QScoreModel("random")
    s = _seqr(genome, ERR_MODEL, "random")
    rs = np.random.RandomState(37)
    _check(s, po, genome, _molecules(rs, genome, 256, 1, 8), em, qm, False)
    mols = _molecules(rs, genome, 63, 1, 8)
    mols.insert(20, ("long70k", [("chr2", 1234, 1234 + 70_000, "-", "")]))
    _check(s, po, genome, mols, em, qm, False, first=0, stride=1)
    s.close()


def test_type_0_model(po, genome):
    """the random error model: every draw changes something, the table is not consulted"""
    em, qm = po.ErrorModel("random"), po.QScoreModel("random")
    s = _seqr(genome, "random", "random")
    rs = np.random.RandomState(41)
    _check(s, po, genome, _molecules(rs, genome, 192, 100, 400) + _molecules(rs, genome, 64, 1, 8), em, qm, False)
    s.close()
