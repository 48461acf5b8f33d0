"""Results must not depend on what recycled device memory held (-m gpu).  DevCache hands device blocks from one call to the next without
clearing them, the buffers a context owns keep the previous call's contents, and every clear in the library covers exactly the bytes one
kernel needs cleared: a read one element too far, a clear one element short or a forgotten sentinel gives the right bytes whenever the
block happens to hold zeros or the tables of the previous, similar call -- which is what it holds in every other suite.

tests/history_cases.py runs one case per family of entry points, each small / large / small on one context.  Here it runs three times,
each time in a fresh child process, one after the other:

    child 1   TKSMSEQ_POISON unset      today's behaviour; its outputs are compared with the specifications
    child 2   TKSMSEQ_POISON=00000000   what fresh memory usually holds
    child 3   TKSMSEQ_POISON=00000001   a flag byte reads as set, a uint32 as 1, a uint64 count as 2^32 + 1, a double as a denormal: different
                                        enough to change any output that depends on it, small enough that a stray 32-bit index stays in its table

and every output file of children 2 and 3 must equal child 1's, with more than zero poisoned blocks reported for every context (the
`poison ...` lines of ctx.h), so that the test cannot pass without having poisoned anything.  A child that ends in any way but exit
status 0 without a HIP error on stderr fails the test there, and no further child is started.

Time limits: child 1 took CHILD1_SECONDS = 2.9 s of wall time on an MI355X (about 1 s in the cases, the rest starting Python and
importing); it gets about three times that, the poisoned children about ten times (every allocation waits for the device in that mode,
which is the only reason for the factor; they took 3.1 s each).

References of child 1: transforms -- the chain of mdf_ops_oracle, core_modules_spec, glue_shuffle_spec, mutate_spec, noise_spec and
filter_spec, text for text, and the --perfect reads of the final batch spliced by the oracle; Badread, perfect, skip-qual and the clone
-- pyoracle, record for record, at the small step (the large step of 600 molecules is pinned by being equal under the three settings
only; test_gpu_parity.py compares such batches with the oracle); gzip -- gzip.decompress and test_gzip_device.check_stream; wgs,
transcribe, model-sequence -- their specifications, text for text; kde_grid, kde_cv_bandwidth and model_truncation -- kde_spec at the
gates of test_kde_build_gpu.py; abundance -- the golden tables byte for byte, the vector against abundance_spec at the gate of
test_abundance_gpu.py.  Every output has a reference at the first small and at the large step, except the Badread records of the large
step."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import history_cases as H

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "history_cases.py")
CHILD1_SECONDS = 2.9
CHILDREN = (None, "00000000", "00000001")
LIMIT = {None: 10, "00000000": 30, "00000001": 30}               # seconds: about 3 x and 10 x CHILD1_SECONDS
HIP_TROUBLE = re.compile(r"illegal memory access|Memory access fault|HSA_STATUS_ERROR|hipError|HIP error", re.I)
POISON_LINE = re.compile(r"^poison ([0-9a-f]{8}): (\d+) blocks, (\d+) bytes$")
_ran = {}


def _child(word, tmp_path_factory):
    """the driver's run under `word` (None: unset), started once, and only after every child before it has ended well:
    {"dir", "stderr", "poison": {context: [blocks, bytes]}}"""
    for w in CHILDREN[:CHILDREN.index(word)]:
        _child(w, tmp_path_factory)
    if word not in _ran:
        out = str(tmp_path_factory.mktemp("history_" + (word or "unset")))
        env = {k: v for k, v in os.environ.items() if k != "TKSMSEQ_POISON"}
        if word is not None:
            env["TKSMSEQ_POISON"] = word
        limit = int(LIMIT[word])
        _ran[word] = "did not end"                               # (a time limit below leaves this behind: nothing is started after it)
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, DRIVER, "--out", out], capture_output=True, text=True, env=env,
                           timeout=limit + 30)
        trouble = HIP_TROUBLE.search(r.stderr)
        if r.returncode != 0 or trouble:
            _ran[word] = (f"child TKSMSEQ_POISON={word}: exit status {r.returncode}" + (f", `{trouble.group(0)}` on stderr" if trouble else "") +
                          f" (time limit {limit} s)\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-6000:]}")
        else:
            poison, cur = {}, None
            for line in r.stderr.splitlines():
                if line.startswith("case "):
                    cur = line[5:].strip()
                m = POISON_LINE.match(line)
                if m:
                    assert m.group(1) == word, line
                    poison.setdefault(cur, [0, 0])
                    poison[cur][0] += int(m.group(2)); poison[cur][1] += int(m.group(3))
            print(f"--- child TKSMSEQ_POISON={word or '(unset)'}\n{r.stdout}")
            _ran[word] = dict(dir=out, stderr=r.stderr, poison=poison)
    if not isinstance(_ran[word], dict):
        pytest.fail(_ran[word], pytrace=False)
    return _ran[word]


def _files(child):
    return sorted(f for f in os.listdir(child["dir"]) if f.endswith(".bin"))


def _read(child, output, step):
    with open(os.path.join(child["dir"], f"{output}.{step}.bin"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def unset(tmp_path_factory):
    return _child(None, tmp_path_factory)


# ------------------------------------------------------------------------------------------------ child 1 against the references
OUTPUTS = ("badread", "badread_gzip", "perfect", "skip_qual", "transforms", "transforms_reads", "wgs", "transcribe", "gzip_raw", "gzip_fastq", "kde_grid",
           "kde_cv", "model_truncation", "abundance", "abundance_vector", "model_sequence_error", "model_sequence_qscore")


def test_unset_run_writes_every_output_and_poisons_nothing(unset):
    assert _files(unset) == sorted([f"{o}.{st}.bin" for o in OUTPUTS for st in H.STEPS] + ["clone.small1.bin"])
    assert unset["poison"] == {} and "poison" not in unset["stderr"]
    for o in OUTPUTS:
        assert _read(unset, o, "small1") == _read(unset, o, "small2"), o
        assert _read(unset, o, "small1") != _read(unset, o, "large"), o


def test_unset_badread_records_equal_the_oracle(unset, po, oracle_models):
    import test_run_reuse as R
    ref = {k: v.decode() for k, v in R.REF.items()}
    ident = po.Identities(84.0, 5.5, 99.0)
    mols = list(po.mdf_generator(H.badread_text("small1").splitlines()))
    want = {"badread": [], "skip_qual": [], "perfect": []}
    for i, (mid, ivs) in enumerate(mols):
        raw = po.splice(ref, ivs)
        want["badread"].append(po.badread_record(True, H.SEED, i, raw, ident, oracle_models["em"], oracle_models["qm"], True, mid)[0])
        want["skip_qual"].append(po.badread_record(True, H.SEED, i, raw, ident, oracle_models["em"], oracle_models["qm"], False, mid)[0])
        want["perfect"].append(po.perfect_record(True, H.SEED, i, raw, mid))
    assert len(mols) == 32
    for output, records in want.items():
        for step in ("small1", "small2"):
            got = _read(unset, output, step)
            at = 0
            for i, w in enumerate(records):                                    # record for record
                assert got[at:at + len(w)] == w, f"{output}.{step}: record {i}"
                at += len(w)
            assert at == len(got)
    assert _read(unset, "clone", "small1") == b"".join(want["badread"])


def test_unset_gzip_streams_inflate_to_their_input(unset):
    import test_gzip_device as Z
    for step in H.STEPS:
        for output, plain in (("gzip_raw", H.gzip_raw_plain(step)), ("gzip_fastq", H.gzip_fastq_plain(step)), ("badread_gzip", _read(unset, "badread", step))):
            out = _read(unset, output, step)
            assert gzip.decompress(out) == plain, f"{output}.{step}"
            members = Z.check_stream(out, plain)
            if output == "gzip_raw":
                assert len(members) == (2 if step != "large" else 4)


def test_unset_transforms_equal_the_chain_of_specifications(unset, po):
    genome = H.transform_genome()
    for step in ("small1", "large"):
        text, merged = H.transform_spec(step)
        assert _read(unset, "transforms", step).decode() == text, step
        want = []
        for i, md in enumerate(merged):
            ivs = [(sg["chr"], sg["start"], sg["end"], "+" if sg["plus"] else "-", ",".join(f"{p}{b}" for p, b in sg["errors"])) for sg in md["segments"]]
            want.append(po.perfect_record(True, H.SEED, i, po.splice(genome, ivs), md["id"]))
        assert _read(unset, "transforms_reads", step) == b"".join(want), step
        assert len(merged) > 20


def test_unset_generators_equal_their_specifications(unset):
    import tsb_spec as ts
    import wgs_spec as ws
    for step in ("small1", "large"):
        want, st = ws.wgs_spec(H.WGS["seed"], H.WGS_CONTIGS, H.WGS["dist"], H.WGS["a"], H.WGS["b"], base_count=H.WGS["base_count"],
                               n_candidates=H.wgs_candidates(step))
        assert _read(unset, "wgs", step).decode() == want and st["molecules"] > 100, step
        plan = ts.tsb_spec(42, [open(H.TSB_GTF).read()], [open(H.TSB_ABUNDANCE).read()], H.transcribe_molecules(step))[0]
        assert _read(unset, "transcribe", step).decode() == plan.unrolled_text(0, plan.molecules), step
        assert plan.molecules > 0.5 * H.transcribe_molecules(step)


def test_unset_model_sequence_equals_the_specification(unset, tmp_path):
    import model_seq_spec as M
    for step in ("small1", "large"):
        d = H.model_sequence_data(tmp_path, step)
        want = M.run(d["reference"], d["reads"], d["alignment"], **{k: v for k, v in H.model_sequence_args(step).items() if k != "chunk_events"})
        assert _read(unset, "model_sequence_error", step).decode() == want["error"], step
        assert _read(unset, "model_sequence_qscore", step).decode() == want["qscore"], step


def test_unset_builders_equal_their_references(unset):
    import abundance_spec as A
    import kde_spec as K
    import test_abundance_gpu as AG
    import test_kde_build_gpu as KB
    for step in ("small1", "large"):
        got = np.frombuffer(_read(unset, "kde_grid", step), np.float64).reshape(len(H.KDE_AXIS), len(H.KDE_AXIS))
        KB.gate(got, K.kde_grid_spec(H.kde_grid_sample(step), H.KDE_AXIS, H.KDE_AXIS, 120.0), f"kde_grid {step}")
        got = np.frombuffer(_read(unset, "kde_cv", step), np.float64)
        want_bw, want = K.cv_bandwidth_spec(H.kde_cv_sample(), 7, H.kde_cv_samples(step))
        rel = np.abs(got[1:].reshape(3, 10) - want) / np.abs(want)
        print(f"kde_cv {step}: bandwidth {got[0]} (spec {want_bw}), worst relative score difference {rel.max():.3g}")
        assert got[0] == want_bw and np.isfinite(got).all() and rel.max() <= 1e-9               # (the gate of test_kde_build_gpu.py)
        name = "default" if step == "small1" else "em1"
        with open(os.path.join(os.path.dirname(H.ABUNDANCE_PAF), f"expected_{name}.tsv"), "rb") as f:
            assert _read(unset, "abundance", step) == f.read(), step
        AG.gate(np.frombuffer(_read(unset, "abundance_vector", step), np.float64), A.run(H.ABUNDANCE_PAF, **H.abundance_args(step))["abundance"],
                f"abundance vector {step}")
        got, want = json.loads(_read(unset, "model_truncation", step)), K.model_spec(H.KDE_PAF, **H.model_truncation_args(step))
        assert [p["name"] for p in got] == ["KDE_mtx", "end_mtx"]
        for a, b in zip(got, want):
            assert a["shape"] == b["shape"] and a["labels"] == b["labels"]
        assert got[1]["data"] == want[1]["data"]
        KB.gate(got[0]["data"], want[0]["data"], f"model_truncation {step}")


# ------------------------------------------------------------------------------------------------ children 2 and 3 against child 1
@pytest.mark.parametrize("word", CHILDREN[1:])
def test_poisoned_run_writes_the_same_bytes(unset, tmp_path_factory, word):
    child = _child(word, tmp_path_factory)
    for name in H.CONTEXTS:
        blocks, nbytes = child["poison"].get(name, (0, 0))
        print(f"TKSMSEQ_POISON={word} {name}: {blocks} blocks, {nbytes} bytes poisoned")
    for name in H.CONTEXTS:
        blocks, nbytes = child["poison"].get(name, (0, 0))
        assert blocks > 0 and nbytes > 0, f"{name}: nothing was poisoned"
    assert _files(child) == _files(unset)
    differ = [f for f in _files(unset) if open(os.path.join(child["dir"], f), "rb").read() != open(os.path.join(unset["dir"], f), "rb").read()]
    assert not differ, f"TKSMSEQ_POISON={word}: these outputs depend on what their memory held before: {differ}"
