"""BGZF on the device (tksmseq_result_gzip / tksmseq_gzip_device, `tksm sequence --gzip device`).

CPU: the ABI, the flag's validation, the EOF member, a pure-Python BGZF walker that is first tried on files made with zlib by the
same rules (so that it is known to work before it judges the device), and the encoder's serial core (gzip_core.h) run on the host
through tools/gzip_core_check.cpp.  GPU: every case must decompress to its input, pass the walker, and every member must inflate on
its own to its 65 280-byte slice with matching CRC-32 and ISIZE; the size gates compare with zlib level 1 on the same bytes."""
import gzip
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CHUNK = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
EXE = os.path.join(ROOT, "tksm_amd", "tksm")
ENV = dict(os.environ, TKSM_MODELS=os.path.join(ROOT, "tksm_amd", "models"))


# ---- the walker ---------------------------------------------------------------------------------------------------------------
def bgzf_walk(data):
    """Follows BSIZE from member to member.  Returns [(offset, size, payload bytes, crc, isize)]; raises ValueError on anything that
    is not a sequence of well-formed BGZF members."""
    out, at = [], 0
    while at < len(data):
        if len(data) - at < 18 + 8:
            raise ValueError(f"member at {at}: {len(data) - at} bytes left")
        id1, id2, cm, flg, _mtime, _xfl, _os, xlen = struct.unpack_from("<BBBBIBBH", data, at)
        if (id1, id2, cm, flg) != (0x1f, 0x8b, 8, 4):
            raise ValueError(f"member at {at}: ID1 ID2 CM FLG = {id1:#x} {id2:#x} {cm} {flg}")
        if xlen != 6 or data[at + 12:at + 14] != b"BC" or struct.unpack_from("<H", data, at + 14)[0] != 2:
            raise ValueError(f"member at {at}: extra field is not the one BC subfield")
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        if size < 18 + 2 + 8 or at + size > len(data):
            raise ValueError(f"member at {at}: BSIZE + 1 = {size}, {len(data) - at} bytes left")
        if size > 65536:
            raise ValueError(f"member at {at}: {size} bytes")
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        if isize > CHUNK:
            raise ValueError(f"member at {at}: ISIZE {isize}")
        out.append((at, size, data[at + 18:at + size - 8], crc, isize))
        at += size
    return out


def check_stream(out, plain, offsets=None):
    """out: BGZF members of `plain` without the EOF member"""
    assert gzip.decompress(out) == plain if out else plain == b""
    members = bgzf_walk(out)
    assert len(members) == (len(plain) + CHUNK - 1) // CHUNK
    for c, (at, size, payload, crc, isize) in enumerate(members):
        want = plain[c * CHUNK:(c + 1) * CHUNK]
        z = zlib.decompressobj(-15)
        got = z.decompress(payload) + z.flush()
        assert z.eof and not z.unused_data, f"member {c}: deflate stream does not end with the payload"
        assert got == want, f"member {c} does not inflate to its slice"
        assert crc == zlib.crc32(want) and isize == len(want), f"member {c}: CRC-32 / ISIZE"
    if offsets is not None:
        assert [int(x) for x in offsets] == [m[0] for m in members] + [len(out)]
    return members


def zlib_bgzf(plain, level=1):
    out = []
    for at in range(0, len(plain), CHUNK):
        piece = plain[at:at + CHUNK]
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        payload = z.compress(piece) + z.flush()
        out.append(struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 0x42, 0x43, 2, len(payload) + 25) + payload +
                   struct.pack("<II", zlib.crc32(piece), len(piece)))
    return b"".join(out)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def fibonacci_bytes(limit=CHUNK, n_symbols=256):
    """byte values whose counts are 1, 1, 2, 3, 5, ...: an unlimited Huffman code for them is as deep as there are symbols"""
    f = [1, 1]
    while len(f) < n_symbols and sum(f) + f[-1] + f[-2] <= limit:
        f.append(f[-1] + f[-2])
    vals = np.repeat(np.arange(1, len(f) + 1, dtype=np.uint8) * 3, f)          # (x 3: no neighbours in value either)
    np.random.RandomState(4).shuffle(vals)
    return vals.tobytes(), len(f)


def code_length_fibonacci_bytes():
    """a chunk whose literal code lengths occur 1, 1, 2, 3, 5, ... times: byte value groups whose counts fall by halves give code
    lengths 1, 2, 3, ..., and group g holds fib(g) values -- the code-length alphabet of the block header gets Fibonacci weights"""
    out, val, fib = [], 0, [1, 1, 2, 3, 5, 8, 13, 21, 34]
    count = 1 << 12
    for g, k in enumerate(fib):
        for _ in range(k):
            out.append(np.full(max(1, count), val, np.uint8))
            val += 1
        count >>= 1
    rs = np.random.RandomState(5)
    vals = rs.permutation(val).astype(np.uint8)[np.concatenate(out)[:CHUNK]]   # (neighbouring values get unrelated lengths: few repeats to run-length code)
    rs.shuffle(vals)
    return vals.tobytes()


def raw_cases():
    rs = np.random.RandomState(7)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    fib, n_fib = fibonacci_bytes()
    assert n_fib >= 22                                                        # deeper than 15 bits without a limit
    return {
        "one byte": b"x",
        "chunk - 1": rs.choice(acgt, CHUNK - 1).tobytes(),
        "chunk": rs.choice(acgt, CHUNK).tobytes(),
        "chunk + 1": rs.choice(acgt, CHUNK + 1).tobytes(),
        "random 1 MB": rs.randint(0, 256, 1 << 20).astype(np.uint8).tobytes(),
        "all byte values": bytes(range(256)) * 5,
        "one byte repeated": b"A" * (1 << 20),
        "runs 1 - 600": b"".join(bytes([65 + i % 7]) * i for i in range(1, 601)),
        "fibonacci counts": fib,
        "fibonacci code lengths": code_length_fibonacci_bytes(),
    }


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_gzip_symbols_and_the_binding_lists_them():
    from tksm_amd import _lib
    header = open(os.path.join(ROOT, "include", "tksmseq.h")).read()
    declared = set(re.findall(r"\b(tksmseq_[a-z_0-9]+)\s*\(", header))
    want = {"tksmseq_result_gzip", "tksmseq_gzip_device", "tksmseq_gzip_download_range", "tksmseq_gzip_eof"}
    assert want <= declared and want <= set(_lib.SYMBOLS)
    assert declared == set(_lib.SYMBOLS)
    lib = _lib.load()
    for s in want:
        assert hasattr(lib, s)


def test_eof_member_is_the_specifications():
    import ctypes as C
    from tksm_amd import _lib
    from tksm_amd.sequence import BGZF_EOF
    buf = (C.c_uint8 * 28)()
    assert _lib.load().tksmseq_gzip_eof(buf) == 0
    assert bytes(buf) == EOF == BGZF_EOF
    assert gzip.decompress(EOF) == b"" and bgzf_walk(EOF)[0][4] == 0


def test_gzip_flag_is_validated_before_anything_is_created(tmp_path):
    out = tmp_path / "x.fastq.gz"
    r = subprocess.run([EXE, "sequence", "-i", str(tmp_path / "missing.mdf"), "-o", str(out), "--gzip", "bogus"], capture_output=True, text=True,
                       env=ENV, timeout=120)
    assert r.returncode == 1 and "--gzip" in r.stderr and "bogus" in r.stderr
    assert not out.exists()
    keep = tmp_path / "keep.fastq.gz"
    keep.write_bytes(b"precious")
    r = subprocess.run([EXE, "sequence", "-i", str(tmp_path / "missing.mdf"), "-o", str(keep), "--gzip=zlib"], capture_output=True, text=True,
                       env=ENV, timeout=120)
    assert r.returncode == 1 and keep.read_bytes() == b"precious"


def test_walker_accepts_zlib_made_bgzf_and_rejects_damage():
    rs = np.random.RandomState(1)
    plain = rs.choice(np.frombuffer(b"ACGT\n", np.uint8), 3 * CHUNK + 17).tobytes()
    data = zlib_bgzf(plain)
    members = check_stream(data, plain)
    assert len(members) == 4 and members[-1][4] == 17
    assert len(bgzf_walk(data + EOF)) == 5
    with pytest.raises(ValueError):
        bgzf_walk(data[:-1])
    with pytest.raises(ValueError):
        bgzf_walk(data[:members[2][0] + 9])
    bad = bytearray(data)
    bad[members[1][0] + 12] = ord("X")
    with pytest.raises(ValueError):
        bgzf_walk(bytes(bad))
    bad = bytearray(data)
    bad[members[1][0] + 3] = 0
    with pytest.raises(ValueError):
        bgzf_walk(bytes(bad))
    crc = bytearray(data)
    crc[members[0][0] + members[0][1] - 8] ^= 1
    with pytest.raises((AssertionError, gzip.BadGzipFile)):
        check_stream(bytes(crc), plain)


@pytest.fixture(scope="module")
def core_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("gzcore") / "gzip_core_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "tksm_amd", "csrc"), os.path.join(ROOT, "tools", "gzip_core_check.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    return str(exe)


def _fastq_like(rs, n, all_k=False, fasta=False):
    out = []
    for i in range(n):
        ln = int(rs.randint(150, 2500))
        seq = rs.choice(np.frombuffer(b"ACGT", np.uint8), ln).tobytes()
        qual = b"K" * ln if all_k else (33 + np.clip(rs.normal(18, 8, ln), 1, 50).astype(np.uint8)).tobytes()
        head = b"m%d_%d length=%d error_free_length=%d read_identity=%.2f%%" % (i, rs.randint(10 ** 6), ln, ln - 3, rs.rand() * 100)
        out.append(b">" + head + b"\n" + seq + b"\n" if fasta else b"@" + head + b"\n" + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out)


def test_encoder_core_on_the_host(core_check, tmp_path):
    """tokeniser, length limiting, block headers and canonical codes (gzip_core.h, the text the kernels compile) through zlib's inflate"""
    def run(fmt, plain):
        p = tmp_path / "in.bin"
        p.write_bytes(plain)
        r = subprocess.run([core_check, fmt, str(p)], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        check_stream(r.stdout, plain)
        return len(r.stdout)
    for name, plain in raw_cases().items():
        size = run("raw", plain)
        if name == "random 1 MB":
            assert size <= len(plain) + 31 * ((len(plain) + CHUNK - 1) // CHUNK)
        if name == "one byte repeated":
            assert size < len(plain) // 100
    rs = np.random.RandomState(2)
    fq, fq_k, fa = _fastq_like(rs, 300), _fastq_like(rs, 300, all_k=True), _fastq_like(rs, 300, fasta=True)
    assert run("fastq", fq) < run("raw", fq)                                  # tables per line class pay
    assert run("fastq", fq_k) <= 1.05 * len(zlib.compress(fq_k, 1))
    run("fasta", fa)
    run("fastq", fa)                                                          # a wrong format is still a valid stream
    run("fastq", b"\n\n\n\n\n\nAAAAAA\n\n\n\n\n" * 9000)
    run("fasta", raw_cases()["random 1 MB"][:200000])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gz(seqr):
    """a clone of the session's context (its models) with a reference of its own"""
    s = seqr.clone()
    rs = np.random.RandomState(11)
    lens = [400_000, 300_000]
    for c, ln in enumerate(lens):
        s.add_contig(f"g{c + 1}", rs.choice(np.frombuffer(b"ACGT", np.uint8), ln).tobytes())
    s.contig_lens = lens
    yield s
    s.close()


def _device_bytes(plain):
    import torch
    if not plain:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(plain), dtype=torch.uint8).cuda()


@pytest.mark.gpu
def test_gzip_device_raw_edge_cases(gz):
    import torch
    out, off, _ = gz.gzip_device(0, 0, "raw", with_info=True)
    assert out == b"" and [int(x) for x in off] == [0]
    for name, plain in raw_cases().items():
        t = _device_bytes(plain)
        torch.cuda.synchronize()
        out, off, _ = gz.gzip_device(t.data_ptr(), len(plain), "raw", with_info=True)
        members = check_stream(out, plain, off)
        print(f"raw / {name}: {len(plain)} -> {len(out)} bytes in {len(members)} members")
        if name == "random 1 MB":
            assert len(out) <= len(plain) + 31 * len(members)
        if name == "one byte repeated":
            assert len(out) < len(plain) // 100
        # an unaligned source gives the same members
        if len(plain) > 3:
            out2 = gz.gzip_device(t.data_ptr() + 1, len(plain) - 1, "raw")
            check_stream(out2, plain[1:])


@pytest.mark.gpu
def test_gzip_device_line_formats_on_arbitrary_bytes(gz):
    import torch
    rs = np.random.RandomState(3)
    cases = [("fastq", _fastq_like(rs, 200)), ("fasta", _fastq_like(rs, 200, fasta=True)), ("fastq", _fastq_like(rs, 100, fasta=True)),
             ("fastq", b"\n\n\n\n\n\nAAAAAA\n\n\n\n\n" * 9000), ("fasta", rs.randint(0, 256, 200000).astype(np.uint8).tobytes())]
    for fmt, plain in cases:
        t = _device_bytes(plain)
        torch.cuda.synchronize()
        out, off, _ = gz.gzip_device(t.data_ptr(), len(plain), fmt, with_info=True)
        check_stream(out, plain, off)


def _mdf(mols):
    return "".join(f"+{mid}\t1\t\n" + "".join(f"{c}\t{a}\t{b}\t{st}\t\n" for c, a, b, st in ivs) for mid, ivs in mols)


def _mols(rs, lens, n, lo=200, hi=2500):
    out = []
    for i in range(n):
        ln = int(rs.randint(lo, hi))
        c = int(rs.randint(len(lens)))
        st = int(rs.randint(0, lens[c] - ln))
        out.append((f"r{i}", [(f"g{c + 1}", st, st + ln, "+-"[i & 1])]))
    return out


def _run_and_check(s, b, **kw):
    r = s.run(b, **kw)
    plain, _ = r.download()
    out, off, _ = r.gzip(with_info=True)
    check_stream(out, plain, off)
    assert r.gzip() == out, "two calls give different bytes"
    return plain, out


@pytest.mark.gpu
def test_result_gzip_on_every_record_kind(gz):
    rs = np.random.RandomState(21)
    b = gz.batch_from_mdf(_mdf(_mols(rs, gz.contig_lens, 300)))
    for name, kw in [("badread fastq", dict(target="badread", fastq=True, compute_qual=True)),
                     ("badread fasta", dict(target="badread", fastq=False)),
                     ("skip-qual fastq", dict(target="badread", fastq=True, compute_qual=False)),
                     ("perfect fastq", dict(target="perfect", fastq=True))]:
        plain, out = _run_and_check(gz, b, seed=5, **kw)
        print(f"{name}: {len(plain)} -> {len(out)} bytes, zlib level 1: {len(zlib.compress(plain, 1))}")
    # a clone gives the bytes of its source
    plain, out = _run_and_check(gz, b, target="badread", fastq=True, compute_qual=True, seed=5)
    c = gz.clone()
    try:
        r = c.run(b, target="badread", fastq=True, compute_qual=True, seed=5)
        assert r.download()[0] == plain and r.gzip() == out
    finally:
        c.close()
    b.free()
    # a record larger than a chunk, and a single read
    big = gz.batch_from_mdf(_mdf([("long", [("g1", 1000, 61000, "+")])] + _mols(rs, gz.contig_lens, 5)))
    plain, _ = _run_and_check(gz, big, target="badread", fastq=True, compute_qual=True, seed=6)
    assert plain.index(b"\n@", 1) > 2 * CHUNK - 20000
    big.free()
    one = gz.batch_from_mdf(_mdf([("only", [("g2", 10, 310, "-")])]))
    _run_and_check(gz, one, target="badread", fastq=True, compute_qual=True, seed=6)
    one.free()


@pytest.mark.gpu
def test_records_that_end_on_a_chunk_boundary(gz):
    """perfect FASTQ records are '@id ...length=L...\\nSEQ\\n+\\nQUAL\\n': the last read's length is chosen so that the first reads fill
    chunk 0 exactly and the last record fills chunk 1 exactly"""
    def run(mols):
        b = gz.batch_from_mdf(_mdf([(mid, [("g1", 100 + i, 100 + i + ln, "+")]) for i, (mid, ln) in enumerate(mols)]))
        r = gz.run(b, target="perfect", fastq=True, seed=1)
        plain, off = r.download()
        return b, r, plain, [int(x) for x in off]

    def fit(mols, target):
        """one more read after `mols` whose record ends at byte `target`: a record grows by two bytes per base, the length of the id sets
        the parity"""
        b, r, plain, off = run(mols + [("e", 1000)])
        b.free()
        guess = 1000 + (target - off[-1]) // 2
        for mid in ("e", "ee", "eee"):
            for ln in range(guess - 6, guess + 7):
                b, r, plain, off = run(mols + [(mid, ln)])
                if off[-1] == target:
                    return mols + [(mid, ln)], (b, r, plain)
                b.free()
        return None, None
    mols, found = fit([(f"b{i}", 3000) for i in range(10)], CHUNK)
    if found:
        found[0].free()
        mols, found = fit(mols, 2 * CHUNK)
    assert found, "no lengths found that put record ends on chunk boundaries"
    b, r, plain = found
    assert len(plain) == 2 * CHUNK and plain[CHUNK - 1:CHUNK + 1] == b"\n@"
    out, off, _ = r.gzip(with_info=True)
    members = check_stream(out, plain, off)
    assert len(members) == 2 and members[1][4] == CHUNK
    b.free()


@pytest.fixture(scope="module")
def bulk(gz):
    from tksm_amd import synthetic
    rs = np.random.RandomState(31)
    m = synthetic.make_molecules(rs, gz.contig_lens, 20_000, 1000, 200, kind="bulk")
    iv = np.array(m["intervals"], np.uint32).reshape(-1, 4)
    iv[:, 0] += gz.contig_id("g1")             # (the arrays index the context's contig table, which the session's context may have filled)
    b = gz.batch_from_arrays(m["reads"], iv, m["mods"], m["literals"], m["literal_pool"], m["ids"], m["id_pool"])
    yield b
    b.free()


@pytest.mark.gpu
def test_size_gate_fastq_with_qscores(gz, bulk):
    """<= 1.00 x zlib level 1 on the same bytes (tables per line class: 0.88 in the CPU probe; one table per block: 1.02)"""
    r = gz.run(bulk, target="badread", fastq=True, compute_qual=True, seed=3)
    plain, _ = r.download()
    out = r.gzip()
    ref = len(zlib.compress(plain, 1))
    print(f"badread FASTQ with q-scores: {len(plain)} bytes, device {len(out)}, zlib level 1 {ref}, ratio {len(out) / ref:.4f}")
    assert r.n_reads >= 20_000 and gzip.decompress(out) == plain
    assert len(out) <= 1.00 * ref


@pytest.mark.gpu
def test_size_gate_fastq_all_k(gz, bulk):
    """<= 1.05 x zlib level 1 (runs as distance-1 matches on the quality lines: 0.956 in the CPU probe; Huffman alone: 1.53)"""
    r = gz.run(bulk, target="badread", fastq=True, compute_qual=False, seed=3)
    plain, _ = r.download()
    out = r.gzip()
    ref = len(zlib.compress(plain, 1))
    print(f"all-K FASTQ: {len(plain)} bytes, device {len(out)}, zlib level 1 {ref}, ratio {len(out) / ref:.4f}")
    assert r.n_reads >= 20_000 and gzip.decompress(out) == plain
    assert len(out) <= 1.05 * ref


def _cli(args, env=None, **kw):
    return subprocess.run([EXE, "sequence"] + [str(a) for a in args], capture_output=True, env=env or ENV, timeout=300, **kw)


@pytest.mark.gpu
def test_cli_gzip_device(tmp_path):
    d = os.path.join(GOLDEN, "splice_corpus")
    base = ["-i", os.path.join(d, "mols.mdf"), "-r", os.path.join(d, "ref.fa"), "-s", "11", "--batch-bytes", "4096"]
    small = dict(ENV, TKSMSEQ_PIECE_BYTES="4096")
    plain = tmp_path / "plain.fastq"
    r = _cli(base + ["-o", plain, "--in-flight", "3"], env=small)
    assert r.returncode == 0, r.stderr
    want = plain.read_bytes()
    assert want.count(b"\n") >= 4 * 20
    # several batches, small pieces, three contexts in flight
    a = tmp_path / "a.fastq.gz"
    r = _cli(base + ["-o", a, "--gzip", "device", "--in-flight", "3"], env=small)
    assert r.returncode == 0, r.stderr
    data = a.read_bytes()
    assert data.endswith(EOF) and gzip.decompress(data) == want
    members = bgzf_walk(data)
    assert members[-1][4] == 0 and len(members) > 3
    # the same bytes from two device groups
    b = tmp_path / "b.fastq.gz"
    r = _cli(base + ["-o", b, "--gzip", "device", "--devices", "0,0", "--in-flight", "2"], env=small)
    assert r.returncode == 0, r.stderr
    assert b.read_bytes() == data
    # into a pipe
    link = tmp_path / "pipe.fastq.gz"
    os.symlink("/dev/stdout", link)
    p = subprocess.run(f"'{EXE}' sequence " + " ".join(f"'{x}'" for x in base + ["-o", str(link), "--gzip", "device", "--verbosity", "OFF"]) + " | cat",
                       shell=True, capture_output=True, env=small, timeout=300)
    assert p.returncode == 0, p.stderr
    piped = p.stdout[p.stdout.index(b"\x1f\x8b"):]                            # ("Loading reference ..." goes to stdout first)
    assert piped == data
    # next to a plain --perfect output
    g2, pf = tmp_path / "c.fastq.gz", tmp_path / "perfect.fasta"
    r = _cli(base + ["-o", g2, "--perfect", pf, "--gzip", "device"], env=small)
    assert r.returncode == 0, r.stderr
    assert g2.read_bytes() == data and pf.read_bytes().startswith(b">")
    # an input without molecules: the EOF member alone
    empty = tmp_path / "empty.mdf"
    empty.write_text("")
    e = tmp_path / "e.fastq.gz"
    r = _cli(["-i", empty, "-r", os.path.join(d, "ref.fa"), "-o", e, "--gzip", "device"])
    assert r.returncode == 0, r.stderr
    assert e.read_bytes() == EOF
    # an output that cannot be written
    full = tmp_path / "full.fastq.gz"
    os.symlink("/dev/full", full)
    r = _cli(base + ["-o", full, "--gzip", "device"], env=small)
    assert r.returncode == 1
    # --gzip device without a .gz name changes nothing; --gzip host is the default's bytes
    p2 = tmp_path / "plain2.fastq"
    r = _cli(base + ["-o", p2, "--gzip", "device", "--in-flight", "3"], env=small)
    assert r.returncode == 0 and p2.read_bytes() == want
    h1, h2 = tmp_path / "h1.fastq.gz", tmp_path / "h2.fastq.gz"
    assert _cli(base + ["-o", h1, "--gzip", "host"], env=small).returncode == 0
    assert _cli(base + ["-o", h2], env=small).returncode == 0
    assert h1.read_bytes() == h2.read_bytes() and gzip.decompress(h1.read_bytes()) == want and not h1.read_bytes().endswith(EOF)
