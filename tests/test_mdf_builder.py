"""The output-batch builder that every molecule transform shares (OutBatch and MolPlacement, tksm_amd/csrc/mdf_batch.h; the transforms
themselves are in mdf_ops.cpp, mdf_move.cpp and mdf_make.cpp) where a shared builder can go wrong: a batch without molecules, a batch of one molecule with one segment, a batch with an unrolled
depth-3 molecule, an empty segment and a literal contig -- every transform against its specification, text for text -- and a context
that goes on working after a transform has returned an error half way (what the error exit gave back to the allocation cache is
really free).  GPU only (-m gpu)."""
import pytest

import core_modules_spec as cs
import filter_spec as fs
import glue_shuffle_spec as gss
import mdf_ops_oracle as mo
import mutate_spec as ms
import noise_spec as ns
import wgs_spec as ws

CONTIGS = [("chr1", 60_000), ("chr2", 60_000)]
BATCHES = {
    "empty": "",
    "one": "+solo\t1\tCB=ACGT;\nchr1\t100\t400\t+\t5A\n",
    # five molecules once unrolled: deep_0, deep_1, deep_2, gap (its first segment is empty), lit (its last segment is a literal)
    "three": ("+deep\t3\tCB=ACGTACGTAC;tid=T1;\nchr1\t1000\t1300\t+\t7C,120G\nchr2\t50\t450\t-\t\n"
              "+gap\t1\tCB=.;\nchr1\t500\t500\t+\t\nchr2\t2000\t2350\t-\t3T\n"
              "+lit\t1\tz;CB=TTGACCATGA,ACGT;\nchr1\t10\t260\t+\t\nAAAAAAAAAAAAAAAAAAAAAAAAA\t0\t25\t-\t0C\n"),
}
# SNV, deletion, insertion with and without anchor letter, and a contig that the batch knows as a literal
VARIANTS = "chr1\t1100\tG\nchr1\t1200\t1250\nchr2\t100\tATTT\nchr2\t2100\t.GG\nAAAAAAAAAAAAAAAAAAAAAAAAA\t3\tC\n"
FILTER = ["size >=400", "info CB"]


def _mutate(s, b):
    v = s.load_variants(text=VARIANTS)
    try:
        return s.mutate(b, v)
    finally:
        v.close()


def _filter_side(s, b, true_side):
    t, f = s.filter(b, FILTER)
    (f if true_side else t).free()
    return t if true_side else f


# name: (the transform on the device, its specification on the unrolled molecules)
TRANSFORMS = {
    "pcr": (lambda s, b: s.pcr(b, 3, 40, error_rate=2e-3, efficiency=0.8, seed=5),
            lambda m: mo.pcr_spec(m, 3, 0.8, 2e-3, 40, 5)),
    "truncate": (lambda s, b: s.truncate(b, normal=(250.0, 120.0), seed=17, first_molecule_index=1000),
                 lambda m: [mo.trc_spec(md, 1000 + g, 17, normal=(250.0, 120.0)) for g, md in enumerate(m)]),
    "polyA": (lambda s, b: s.polya(b, normal=(15.0, 7.5), seed=17, first_molecule_index=12345),
              lambda m: cs.polya_spec(m, 17, "normal", 15.0, 7.5, first=12345)),
    "tag": (lambda s, b: s.tag(b, format5="NNNNNN", format3="AGATC", seed=9, first_molecule_index=777),
            lambda m: cs.tag_spec(m, 9, "NNNNNN", "AGATC", first=777)),
    "scb": (lambda s, b: s.scb(b), lambda m: cs.scb_spec(m)),
    "flip": (lambda s, b: s.flip(b, 0.5, seed=5, first_molecule_index=4242),
             lambda m: cs.flip_spec(m, 5, 0.5, first=4242)),
    "tail-noise random": (lambda s, b: s.append_noise(b, ns.NORMAL, 50.0, 10.0, seed=17, first=99),
                          lambda m: ns.noise_spec(m, 17, ns.NORMAL, 50.0, 10.0, first=99)),
    "tail-noise palindromic": (lambda s, b: s.append_noise(b, ns.NORMAL, 300.0, 200.0, palindromic=True, error_rate=0.5, seed=17, first=99),
                               lambda m: ns.noise_spec(m, 17, ns.NORMAL, 300.0, 200.0, True, 0.5, first=99)),
    "glue": (lambda s, b: s.glue(b, 0.5, seed=7, first_molecule_index=31), lambda m: gss.glue_spec(m, 0.5, 7, first=31)),
    "shuffle whole": (lambda s, b: s.shuffle(b, seed=11), lambda m: gss.shuffle_spec(m, 11)),
    "shuffle buffer 2": (lambda s, b: s.shuffle(b, seed=11, buffer_size=2), lambda m: gss.shuffle_spec(m, 11, 2)),
    "mutate": (_mutate, lambda m: ms.mutate_spec(m, ms.normal_form(ms.parse_variants(VARIANTS))[0])),
    "filter true side": (lambda s, b: _filter_side(s, b, True), lambda m: fs.filter_spec(m, FILTER)[0]),
    "filter false side": (lambda s, b: _filter_side(s, b, False), lambda m: fs.filter_spec(m, FILTER)[1]),
    "merge": (lambda s, b: s.merge([b, b]), lambda m: fs.concat_spec([m, m])),
}
_WANT = {}


def _want(transform, batch):
    """the specification's text, computed once per (transform, batch)"""
    if (transform, batch) not in _WANT:
        _WANT[transform, batch] = mo.write_mdf(TRANSFORMS[transform][1](mo.stream_mdf(BATCHES[batch], unroll=True)))
    return _WANT[transform, batch]


@pytest.fixture(scope="module")
def gs():
    import numpy as np
    from tksm_amd.sequence import Sequencer
    rs = np.random.RandomState(21)
    s = Sequencer(0)
    for name, n in CONTIGS:
        s.add_contig(name, rs.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes().decode())
    yield s
    s.close()


def _molecules(text):
    return sum(line.startswith("+") for line in text.splitlines())


def _run(s, transform, batch):
    b = s.batch_from_mdf(BATCHES[batch])
    out = TRANSFORMS[transform][0](s, b)
    try:
        return s.to_mdf_text(out), out.n_reads
    finally:
        out.free()
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_empty_batch(gs, transform):
    assert _run(gs, transform, "empty") == ("", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["one", "three"])
@pytest.mark.parametrize("transform", list(TRANSFORMS))
def test_single_and_unrolled_batches_match_the_specification(gs, transform, batch):
    text, n = _run(gs, transform, batch)
    assert text == _want(transform, batch)
    assert n == _molecules(text)


@pytest.mark.gpu
@pytest.mark.parametrize("what,kw", [
    ("base_count already reached", dict(base_count=1000, n_candidates=100, state=(7, 1000))),
    ("one candidate", dict(base_count=10**9, n_candidates=1)),
    ("one candidate, later in the run", dict(base_count=10**9, first_candidate=12345, n_candidates=1, state=(7, 1000))),
    ("three candidates", dict(base_count=10**9, first_candidate=5, n_candidates=3)),
])
def test_wgs_smallest_ranges(gs, what, kw):
    want, st_want = ws.wgs_spec(42, CONTIGS, ws.NORMAL, 300.0, 50.0, **kw)
    batch, st = gs.wgs(ws.NORMAL, 300.0, 50.0, seed=42, **kw)
    try:
        assert (gs.to_mdf_text(batch), st) == (want, st_want)
        assert batch.n_reads == _molecules(want)
        if what == "base_count already reached":
            assert (want, batch.n_reads, st["reached"]) == ("", 0, True)
    finally:
        batch.free()


@pytest.mark.gpu
def test_error_exits_leave_the_context_usable(gs):
    """scb stops at a molecule without CB when the output batch exists already; random tail-noise stops at a drawn length above 2^20
    after its plan and scan have run.  Both are refused arguments, nothing more; the transforms that follow on the same context take
    blocks out of the same allocation cache and must come out right."""
    from tksm_amd import _lib as L
    from tksm_amd.sequence import TksmSeqError

    def valid_ones():
        for transform in ("flip", "polyA"):
            assert _run(gs, transform, "three")[0] == _want(transform, "three"), transform

    b = gs.batch_from_mdf("+has\t1\tCB=ACGT;\nchr1\t0\t50\t+\t\n+lost\t1\tx=1;\nchr1\t5\t50\t+\t\n")
    with pytest.raises(TksmSeqError, match="lost") as e:
        gs.scb(b)
    assert e.value.code == L.EINVAL
    valid_ones()
    with pytest.raises(TksmSeqError, match="molecule has ") as e:
        gs.append_noise(b, "lognormal", 20.0, 0.1)
    assert e.value.code == L.ELIMIT
    valid_ones()
    b.free()
