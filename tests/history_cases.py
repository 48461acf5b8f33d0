"""The case driver of tests/test_history_gpu.py (a plain script; pytest does not collect it): one case per family of entry points, each on
a context of its own and in the sequence small, large, small -- the large step makes the buffers the context owns grow, the second
small step then runs inside buffers that hold the large step's data -- and the produced bytes of every step written to
`--out DIR` as DIR/<output>.<step>.bin.  The driver itself asserts that the two small steps of every output are equal.  What the bytes
should be is the test's business: it runs this script unset, with TKSMSEQ_POISON=00000000 and with TKSMSEQ_POISON=00000001 (ctx.h) and
compares the three directories, and the first one with the specifications.  The inputs are functions of this module, so that the test
rebuilds them without a GPU.

    python tests/history_cases.py --out DIR [--only CASE ...]

Before every case `case <name>` goes to stderr: the `poison ...` line a context prints as it is destroyed belongs to the case named last."""
import argparse
import functools
import os
import sys
import time

# torch bundles its own ROCm runtime: it is loaded before libtksmseq.so, as in bench.py and tests/conftest.py
import torch  # noqa: F401

import numpy as np

from conftest import ERR_MODEL, GOLDEN, QS_MODEL

import core_modules_spec as cs
import filter_spec as fs
import glue_shuffle_spec as gss
import mdf_ops_oracle as mo
import model_seq_spec as M
import mutate_spec as ms
import noise_spec as ns
import wgs_spec as ws

import test_glue_shuffle_gpu as G
import test_gzip_device as Z
import test_kde_build_gpu as KB
import test_run_reuse as R

STEPS = ("small1", "large", "small2")
SEED = 77


def _size(step, small, large):
    return large if step == "large" else small


# ------------------------------------------------------------------------------------------------ inputs (no GPU)
@functools.lru_cache(None)
def badread_text(step):
    """test_run_reuse's molecules on its genome (N run included): 32 / 600 / 32 of about 300 bases"""
    return R.TEXT["r32"] if step != "large" else R._mdf(4, 600, 300)


TRANSFORM_CONTIGS = {"chr1": 60_000, "chr2": 60_000}
FILTER = ["size >=600", "locus chr1"]


@functools.lru_cache(None)
def transform_genome():
    rs = np.random.RandomState(21)
    return {name: rs.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes().decode() for name, n in TRANSFORM_CONTIGS.items()}


@functools.lru_cache(None)
def transform_text(step):
    """test_glue_shuffle_gpu._mdf: 40 / 700 / 40 records (depth 3, literals, zero-size segments, substitutions on the last interval)"""
    return G._mdf(np.random.RandomState(2), _size(step, 40, 700))


@functools.lru_cache(None)
def variant_table():
    """the golden table and 60 random rows"""
    return open(os.path.join(GOLDEN, "mutate", "variants.tsv")).read() + ms.random_table(np.random.RandomState(5), TRANSFORM_CONTIGS, 60)


def _mutate(s, b):
    v = s.load_variants(text=variant_table())
    try:
        return s.mutate(b, v)
    finally:
        v.close()


def transform_chain(step):
    """[(stage, the transform on the device, its specification on the unrolled molecules)], each stage on the output of the one before;
    the filter and the merge of its two sides follow (FILTER)"""
    target = 2 * len(mo.stream_mdf(transform_text(step), unroll=True))
    return [
        ("pcr", lambda s, b: s.pcr(b, 3, target, error_rate=2e-3, efficiency=0.8, seed=5), lambda m: mo.pcr_spec(m, 3, 0.8, 2e-3, target, 5)),
        ("truncate", lambda s, b: s.truncate(b, lognormal=(5.5, 0.7), seed=17, first_molecule_index=1000),
         lambda m: [mo.trc_spec(md, 1000 + g, 17, lognormal=(5.5, 0.7)) for g, md in enumerate(m)]),
        ("polyA", lambda s, b: s.polya(b, normal=(15.0, 7.5), seed=17, first_molecule_index=12345), lambda m: cs.polya_spec(m, 17, "normal", 15.0, 7.5, first=12345)),
        ("tag", lambda s, b: s.tag(b, format5="NNNNNN", format3="AGATC", seed=9, first_molecule_index=777), lambda m: cs.tag_spec(m, 9, "NNNNNN", "AGATC", first=777)),
        ("flip", lambda s, b: s.flip(b, 0.5, seed=5, first_molecule_index=4242), lambda m: cs.flip_spec(m, 5, 0.5, first=4242)),
        ("glue", lambda s, b: s.glue(b, 0.5, seed=7, first_molecule_index=31), lambda m: gss.glue_spec(m, 0.5, 7, first=31)),
        ("shuffle", lambda s, b: s.shuffle(b, seed=11, buffer_size=64), lambda m: gss.shuffle_spec(m, 11, 64)),
        ("mutate", _mutate, lambda m: ms.mutate_spec(m, ms.normal_form(ms.parse_variants(variant_table()))[0])),
        ("tail-noise random", lambda s, b: s.append_noise(b, ns.NORMAL, 50.0, 10.0, seed=17, first=99), lambda m: ns.noise_spec(m, 17, ns.NORMAL, 50.0, 10.0, first=99)),
        ("tail-noise palindromic", lambda s, b: s.append_noise(b, ns.NORMAL, 300.0, 200.0, palindromic=True, error_rate=0.5, seed=17, first=99),
         lambda m: ns.noise_spec(m, 17, ns.NORMAL, 300.0, 200.0, True, 0.5, first=99)),
    ]


def transform_spec(step):
    """(the text of every stage, the two filter sides and their merge, concatenated; the molecules of the merge) by the specifications"""
    mols = mo.stream_mdf(transform_text(step), unroll=True)
    texts = []
    for _, _, spec in transform_chain(step):
        mols = spec(mols)
        texts.append(mo.write_mdf(mols))
    t, f = fs.filter_spec(mols, FILTER)
    merged = fs.concat_spec([t, f])
    return "".join(texts + [mo.write_mdf(t), mo.write_mdf(f), mo.write_mdf(merged)]), merged


WGS_CONTIGS = [("w1", 50_000), ("w2", 30_000), ("w3", 20_001)]
WGS = dict(seed=42, dist=ws.NORMAL, a=300.0, b=50.0, base_count=10**9)
TSB_CONTIGS = [("c1", 5000), ("c2", 4000), ("c3", 3000)]
TSB_GTF = os.path.join(GOLDEN, "transcribe", "ann.gtf")
TSB_ABUNDANCE = os.path.join(GOLDEN, "transcribe", "abund_exact.tsv")


def wgs_candidates(step):
    return _size(step, 300, 5000)


def transcribe_molecules(step):
    return _size(step, 50, 2000)


def _genome(contigs, seed):
    rs = np.random.RandomState(seed)
    return {name: rs.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes().decode() for name, n in contigs}


@functools.lru_cache(None)
def gzip_raw_plain(step):
    """ACGT-and-newline text of CHUNK + 1 / 3 CHUNK + 17 / CHUNK + 1 bytes"""
    n = _size(step, Z.CHUNK + 1, 3 * Z.CHUNK + 17)
    return np.random.RandomState(6).choice(np.frombuffer(b"ACGT\n", np.uint8), n, p=[0.245, 0.245, 0.245, 0.245, 0.02]).tobytes()


@functools.lru_cache(None)
def gzip_fastq_plain(step):
    return Z._fastq_like(np.random.RandomState(8), _size(step, 20, 200))


KDE_AXIS = KB.centres(17)


def kde_grid_sample(step):
    return KB.sample(_size(step, 5, 4097))


def kde_cv_sample():
    return KB.sample(3000, seed=4)


def kde_cv_samples(step):
    return _size(step, 300, 1501)


KDE_PAF = os.path.join(GOLDEN, "kde_build", "reads.paf")
ABUNDANCE_PAF = os.path.join(GOLDEN, "abundance", "reads.paf")


def model_truncation_args(step):
    """the golden PAF on the 30 x 30 grid, on the default 100 x 100 grid, on the 30 x 30 grid"""
    return dict(bandwidth=120.0, grid_end=_size(step, 3000, 10000))


def abundance_args(step):
    """default settings, then one EM round, then the defaults again"""
    return {} if step != "large" else dict(em_iterations=1)


def model_sequence_data(out_dir, step):
    """model_seq_spec.generate: 20 / 120 / 20 alignments, the large step with one alignment of 5 000 columns.  The contigs come first
    in the generator's draws, so the three steps share their reference."""
    d = os.path.join(str(out_dir), "model_seq_" + ("large" if step == "large" else "small"))
    if not os.path.exists(os.path.join(d, "aln.paf")):
        M.generate(d, seed=11, n_alignments=_size(step, 20, 120), long_columns=_size(step, 0, 5000))
    return {k: os.path.join(d, v) for k, v in (("reference", "ref.fa"), ("reads", "reads.fq"), ("alignment", "aln.paf"))}


def model_sequence_args(step):
    return dict(min_occur=1, **({"chunk_events": 1000} if step == "large" else {}))


# ------------------------------------------------------------------------------------------------ the cases (GPU)
def _badread_context():
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    for name, seq in R.REF.items():
        s.add_contig(name, seq)
    s.set_identity(84.0, 99.0, 5.5)
    s.load_error_model(ERR_MODEL)
    s.load_qscore_model(QS_MODEL)
    return s


def _records(s, step, gz=False, **kw):
    b = s.batch_from_mdf(badread_text(step))
    try:
        r = s.run(b, fastq=True, seed=SEED, **kw)
        return (r.download()[0], r.gzip()) if gz else r.download()[0]
    finally:
        b.free()


def case_badread(emit, work):
    """FASTQ with q-scores, each result through .gzip() as well; then the case `clone`: a clone of this context runs the small batch
    (borrowed buffers, and the first write that replaces one)"""
    from tksm_amd.sequence import Sequencer
    s = _badread_context()
    try:
        for step in STEPS:
            rec, gz = _records(s, step, gz=True, target="badread", compute_qual=True)
            emit("badread", step, rec)
            emit("badread_gzip", step, gz)
        # the counters behind the `poison` lines are the process's: a context made and closed here prints what this case has filled so
        # far, so that the clone's line carries the clone's own blocks
        Sequencer(0).close()
        print("case clone", file=sys.stderr, flush=True)
        c = s.clone()
        try:
            emit("clone", "small1", _records(c, "small1", target="badread", compute_qual=True))
        finally:
            c.close()
        print("case badread", file=sys.stderr, flush=True)
    finally:
        s.close()


def case_perfect(emit, work):
    s = _badread_context()
    try:
        for step in STEPS:
            emit("perfect", step, _records(s, step, target="perfect"))
    finally:
        s.close()


def case_skip_qual(emit, work):
    s = _badread_context()
    try:
        for step in STEPS:
            emit("skip_qual", step, _records(s, step, target="badread", compute_qual=False))
    finally:
        s.close()


def case_transforms(emit, work):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    try:
        for name, seq in transform_genome().items():
            s.add_contig(name, seq)
        for step in STEPS:
            cur, texts = s.batch_from_mdf(transform_text(step)), []
            for _, dev, _ in transform_chain(step):
                nxt = dev(s, cur)
                cur.free()
                cur = nxt
                texts.append(s.to_mdf_text(cur))
            t, f = s.filter(cur, FILTER)
            merged = s.merge([t, f])
            texts += [s.to_mdf_text(t), s.to_mdf_text(f), s.to_mdf_text(merged)]
            reads = s.run(merged, target="perfect", fastq=True, seed=SEED).download()[0]
            for b in (cur, t, f, merged):
                b.free()
            emit("transforms", step, "".join(texts).encode())
            emit("transforms_reads", step, reads)
    finally:
        s.close()


def case_wgs(emit, work):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    try:
        for name, seq in _genome(WGS_CONTIGS, 3).items():
            s.add_contig(name, seq)
        for step in STEPS:
            b, _ = s.wgs(WGS["dist"], WGS["a"], WGS["b"], base_count=WGS["base_count"], seed=WGS["seed"], n_candidates=wgs_candidates(step))
            emit("wgs", step, s.to_mdf_text(b).encode())
            b.free()
    finally:
        s.close()


def case_transcribe(emit, work):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    try:
        for name, seq in _genome(TSB_CONTIGS, 4).items():
            s.add_contig(name, seq)
        s.add_gtf(TSB_GTF)
        for step in STEPS:
            plan = s.transcribe_plan(TSB_ABUNDANCE, transcribe_molecules(step), seed=42)
            b = plan.batch()
            emit("transcribe", step, s.to_mdf_text(b).encode())
            b.free()
            plan.close()
    finally:
        s.close()


def case_gzip(emit, work):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    try:
        for output, plain_of, fmt in (("gzip_raw", gzip_raw_plain, "raw"), ("gzip_fastq", gzip_fastq_plain, "fastq")):
            for step in STEPS:
                t = Z._device_bytes(plain_of(step))
                torch.cuda.synchronize()
                emit(output, step, s.gzip_device(t.data_ptr(), t.numel(), fmt))
    finally:
        s.close()


def case_kde_grid(emit, work):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    try:
        for step in STEPS:
            emit("kde_grid", step, s.kde_grid(kde_grid_sample(step), KDE_AXIS, KDE_AXIS, 120.0).tobytes())
    finally:
        s.close()


def case_kde_cv(emit, work):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    try:
        for step in STEPS:
            bw, scores = s.kde_cv_bandwidth(kde_cv_sample(), seed=7, cv_samples=kde_cv_samples(step))
            emit("kde_cv", step, np.float64(bw).tobytes() + scores.tobytes())
    finally:
        s.close()


def case_model_truncation(emit, work):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    try:
        for step in STEPS:
            out = os.path.join(work, f"model_truncation.{step}.json")
            s.model_truncation(KDE_PAF, out, **model_truncation_args(step))
            emit("model_truncation", step, open(out, "rb").read())
    finally:
        s.close()


def case_abundance(emit, work):
    from tksm_amd.sequence import Sequencer
    s = Sequencer(0)
    try:
        for step in STEPS:
            out = os.path.join(work, f"abundance.{step}.tsv")
            res = s.abundance(ABUNDANCE_PAF, out=out, **abundance_args(step))
            emit("abundance", step, open(out, "rb").read())
            emit("abundance_vector", step, res["abundance"].tobytes())
    finally:
        s.close()


def case_model_sequence(emit, work):
    from tksm_amd.sequence import Sequencer
    data = {step: model_sequence_data(work, step) for step in STEPS}
    assert open(data["small1"]["reference"]).read() == open(data["large"]["reference"]).read()
    s = Sequencer(0)
    try:
        s.get_reference_seqs([data["small1"]["reference"]])
        for step in STEPS:
            e, q = os.path.join(work, f"ms.{step}.error"), os.path.join(work, f"ms.{step}.qscore")
            info = s.model_sequence(data[step]["reads"], data[step]["alignment"], e, q, **model_sequence_args(step))
            if step == "large":
                assert info["chunks"] > 1, info
            emit("model_sequence_error", step, open(e, "rb").read())
            emit("model_sequence_qscore", step, open(q, "rb").read())
    finally:
        s.close()


CASES = {"badread": case_badread, "perfect": case_perfect, "skip_qual": case_skip_qual, "transforms": case_transforms, "wgs": case_wgs,
         "transcribe": case_transcribe, "gzip": case_gzip, "kde_grid": case_kde_grid, "kde_cv": case_kde_cv, "model_truncation": case_model_truncation,
         "abundance": case_abundance, "model_sequence": case_model_sequence}
# the names on the `case` lines of stderr: the clone is closed inside the badread case
CONTEXTS = list(CASES) + ["clone"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", nargs="*", choices=list(CASES))
    a = ap.parse_args(argv)
    os.makedirs(a.out, exist_ok=True)
    work = os.path.join(a.out, "work")
    os.makedirs(work, exist_ok=True)
    t_all = time.time()
    for name in a.only or list(CASES):
        print(f"case {name}", file=sys.stderr, flush=True)
        t0 = time.time()
        got = {}

        def emit(output, step, data):
            got[output, step] = data
            with open(os.path.join(a.out, f"{output}.{step}.bin"), "wb") as f:
                f.write(data)

        CASES[name](emit, work)
        for (output, step), data in got.items():
            assert len(data) > 0, f"{output}.{step} is empty"
            if step == "small2":
                assert data == got[output, "small1"], f"{output}: the second small step differs from the first"
        print(f"{name}: {time.time() - t0:.2f} s, " + ", ".join(f"{o}.{st} {len(d)} B" for (o, st), d in got.items()), flush=True)
    print(f"all cases: {time.time() - t_all:.2f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
