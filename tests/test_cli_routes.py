"""`tksm sequence`: the output routes and the empty-batch path that the other CLI tests do not reach (csrc/sequencer_module.cpp: Route).
The reference of every case is the plain regular-file output of the same command line."""
import gzip
import json
import os
import subprocess
import threading

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "splice_corpus")
EXE = os.path.join(ROOT, "tksm_amd", "tksm")
ENV = dict(os.environ, TKSM_MODELS=os.path.join(ROOT, "tksm_amd", "models"))


def _run(mdf, *outputs, env=ENV, timeout=300):
    cmd = [EXE, "sequence", "-i", str(mdf), "-r", os.path.join(GOLDEN, "ref.fa"), "-s", "11", "--batch-bytes", "4096", "--in-flight", "3", *map(str, outputs)]
    return subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout)


def _run_into_fifo(fifo, mdf, *outputs):
    """what a reader of the FIFO got, and the finished process"""
    os.mkfifo(fifo)
    got = []
    rd = threading.Thread(target=lambda: got.append(open(fifo, "rb").read()), daemon=True)
    rd.start()
    r = _run(mdf, *outputs)
    rd.join(timeout=60)
    assert r.returncode == 0, r.stderr
    assert got, "nothing came out of the FIFO"
    return got[0]


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    out = tmp_path_factory.mktemp("routes") / "plain.fastq"
    r = _run(os.path.join(GOLDEN, "mols.mdf"), "-o", out)
    assert r.returncode == 0, r.stderr
    data = out.read_bytes()
    assert data.count(b"\n@") > 100
    return data


def test_host_gzip_into_a_fifo_goes_through_the_ordered_writer(tmp_path, plain):
    """-o pipe.fastq.gz (--gzip host), a FIFO: whole-batch host buffers, one ordered writer"""
    fifo = tmp_path / "pipe.fastq.gz"
    got = _run_into_fifo(fifo, os.path.join(GOLDEN, "mols.mdf"), "-o", fifo)
    assert gzip.decompress(got) == plain


def test_ordered_writer_with_a_regular_plain_file_beside_the_fifo(tmp_path, plain):
    """... with a regular --perfect file next to it: the plain file as with a regular .gz next to it (pwrite at the batches' places)"""
    small = dict(ENV, TKSMSEQ_PIECE_BYTES="4096")
    r = _run(os.path.join(GOLDEN, "mols.mdf"), "-o", tmp_path / "both.fastq.gz", "--perfect", tmp_path / "both_perfect.fasta", env=small)
    assert r.returncode == 0, r.stderr
    assert gzip.decompress((tmp_path / "both.fastq.gz").read_bytes()) == plain
    want = (tmp_path / "both_perfect.fasta").read_bytes()
    assert want.split(b"\n")[1::2] == plain.split(b"\n")[1::4]
    fifo = tmp_path / "pipe.fastq.gz"
    got = _run_into_fifo(fifo, os.path.join(GOLDEN, "mols.mdf"), "-o", fifo, "--perfect", tmp_path / "plain.fasta")
    assert gzip.decompress(got) == plain
    assert (tmp_path / "plain.fasta").read_bytes() == want


def test_a_batch_without_reads_takes_its_empty_place_and_turn(tmp_path):
    """a run of depth-0 molecules longer than --batch-bytes between ordinary ones: at least one batch has no read; a regular file and a
    FIFO both get the output of the input without those molecules"""
    text = open(os.path.join(GOLDEN, "mols.mdf")).read()
    cut = text.index("\n+", len(text) // 2) + 1
    zeros = "".join(f"+zero_{i}\t0\t\nchr1\t{10 + i}\t{40 + i}\t+\t\n" for i in range(600))
    assert len(zeros) > 3 * 4096
    with_zeros, without = tmp_path / "with_zeros.mdf", tmp_path / "without.mdf"
    with_zeros.write_text(text[:cut] + zeros + text[cut:])
    without.write_text(text)
    stats = dict(ENV, TKSMSEQ_STATS_FILE=str(tmp_path / "stats.json"))
    r = _run(without, "-o", tmp_path / "want.fastq", env=stats)
    assert r.returncode == 0, r.stderr
    want = (tmp_path / "want.fastq").read_bytes()
    assert want.count(b"\n@") > 100
    batches = json.load(open(tmp_path / "stats.json"))["batches"]
    r = _run(with_zeros, "-o", tmp_path / "file.fastq", env=stats)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "file.fastq").read_bytes() == want
    # more than 3 x --batch-bytes of depth-0 molecules: at least two more batches, and two batches that hold nothing else
    assert json.load(open(tmp_path / "stats.json"))["batches"] >= batches + 2
    assert _run_into_fifo(tmp_path / "pipe.fastq", with_zeros, "-o", tmp_path / "pipe.fastq") == want


def test_ordered_writer_wakes_everybody_when_a_write_fails(tmp_path):
    """a host-compressed .gz that is /dev/full: exit code 1 with "write failed" instead of workers waiting for the writer for ever"""
    full = tmp_path / "full.fastq.gz"
    os.symlink("/dev/full", full)
    r = _run(os.path.join(GOLDEN, "mols.mdf"), "-o", full, timeout=120)
    assert r.returncode == 1 and "write failed" in r.stderr, r.stderr
