#!/usr/bin/env python3
"""map: where the time goes on a generated transcriptome (profiles/map_times.log).

  python tools/map_times.py [--transcripts 20000] [--reads 200000] [--molecules 2000] [--out profiles/map_times.log]
  python tools/map_times.py --align [--out profiles/map_align_times.log]

Makes --transcripts random transcripts of 600 to 2 500 bases; every tenth shares its first half with the one before it (isoforms, so that
secondary chains exist).  --reads reads are substrings of at least 200 bases on a random strand with 5 % substitutions.  Runs Sequencer.map
once at the defaults and records the call's wall time split into reading, packing and uploads, device (HIP events, per stage) and writing.
There is no earlier implementation of these rules to compare a time against.  Then, as an observation: --molecules molecules of 40
transcripts made by transcribe on the device, sequenced as perfect and as Badread reads (nanopore2020, identity 84 / 99 / 5.5), and the
share of them whose primary line names their own transcript.  With --align the same reads are mapped a second time with align=True (map -c)
in place of that observation: the new stage's milliseconds beside the totals of both calls, the lines, segments and allowed cells, cells
per second, and the device bytes the stage may take.  One machine, one run."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RC = bytes.maketrans(b"ACGT", b"TGCA")
STAGES = ("sketch", "index", "seed", "chain", "select")


def transcriptome(rs, acgt, n=40):
    """n transcripts of 600 to 2 500 bases, two exons each on a contig of its own, every other one on the minus strand: (genome contigs,
    GTF text, [(transcript id, spliced letters)])"""
    contigs, gtf, spliced = [], [], []
    for i in range(n):
        total = int(rs.integers(600, 2501))
        e1 = int(rs.integers(100, total - 99))
        flank, intron = 50, 120
        seq = acgt[rs.integers(0, 4, flank + total + intron + flank)].tobytes().decode()
        a1, b1 = flank, flank + e1
        a2, b2 = b1 + intron, b1 + intron + (total - e1)
        strand = "+-"[i % 2]
        name, tid, gid = "g%02d" % i, "TX%02d" % i, "GN%02d" % i
        contigs.append((name, seq))
        attr = f'gene_id "{gid}"; transcript_id "{tid}"; gene_name "{gid}"; gene_biotype "protein_coding";'
        gtf.append(f'{name}\tgen\tgene\t{a1 + 1}\t{b2}\t.\t{strand}\t.\tgene_id "{gid}"; gene_name "{gid}"; gene_biotype "protein_coding";')
        gtf.append(f"{name}\tgen\ttranscript\t{a1 + 1}\t{b2}\t.\t{strand}\t.\t{attr}")
        for a, b in ((a1, b1), (a2, b2)) if strand == "+" else ((a2, b2), (a1, b1)):
            gtf.append(f"{name}\tgen\texon\t{a + 1}\t{b}\t.\t{strand}\t.\t{attr}")
        letters = seq[a1:b1] + seq[a2:b2]
        spliced.append((tid, letters if strand == "+" else letters.encode().translate(RC)[::-1].decode()))
    return contigs, "\n".join(gtf) + "\n", spliced


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transcripts", type=int, default=20000)
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--molecules", type=int, default=2000)
    ap.add_argument("--align", action="store_true", help="a second call with align=True in place of the observation on transcribed molecules")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "map_align_times.log" if a.align else "map_times.log")
    import numpy as np
    import torch  # noqa: F401  (its ROCm runtime has to be loaded before libtksmseq.so)
    from tksm_amd.sequence import Sequencer
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    rs = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        tx = []
        for i in range(a.transcripts):
            seq = acgt[rs.integers(0, 4, int(rs.integers(600, 2501)))].tobytes()
            if i % 10 == 9:
                seq = tx[-1][: len(tx[-1]) // 2] + seq[len(seq) // 2:]
            tx.append(seq)
        fa, fq, paf = os.path.join(d, "tx.fa"), os.path.join(d, "reads.fq"), os.path.join(d, "out.paf")
        with open(fa, "wb") as f:
            for i, seq in enumerate(tx):
                f.write(b">tx%06d\n" % i + seq + b"\n")
        origin = rs.integers(0, a.transcripts, a.reads)
        total = 0
        with open(fq, "wb") as f:
            for r, t in enumerate(origin):
                seq = tx[t]
                n = int(rs.integers(200, len(seq) + 1))
                b = int(rs.integers(0, len(seq) - n + 1))
                piece = np.frombuffer(seq[b:b + n], np.uint8).copy()
                hit = rs.random(n) < 0.05
                piece[hit] = acgt[(np.searchsorted(acgt, piece[hit]) + rs.integers(1, 4, int(hit.sum()))) % 4]
                piece = piece.tobytes()
                if rs.random() < 0.5:
                    piece = piece.translate(RC)[::-1]
                total += n
                f.write(b"@r%07d\n" % r + piece + b"\n+\n" + b"I" * n + b"\n")
        say(f"map: times on the input of tools/map_times.py (seed 1): {a.transcripts} transcripts of 600 to 2500 bases ({sum(map(len, tx))} bases, every tenth an isoform "
            f"of the one before), {a.reads} reads of 200 bases to a whole transcript ({total} bases, 5 % substitutions, both strands), "
            f"{os.path.getsize(fq) >> 20} MB of FASTQ (made in {time.time() - t0:.0f} s).  One machine, one run.")
        say()
        s = Sequencer(0)
        t0 = time.time()
        s.get_reference_seqs([fa])
        t_ref = time.time() - t0
        t0 = time.time()
        i = s.map(fq, paf)
        wall = time.time() - t0
        if a.align:
            t0 = time.time()
            j = s.map(fq, os.path.join(d, "aligned.paf"), align=True)
            wall_c = time.time() - t0
        s.close()
        say("== device (MI355X, 1 GPU; Sequencer.map at the defaults: k 15, w 10) ==")
        say(f"reference read and packed in {t_ref:.2f} s; map wall {wall:.2f} s: reading and parsing {i['read_ms'] / 1e3:.2f} s, packing and uploads {i['upload_ms'] / 1e3:.2f} s, "
            f"device {i['device_ms'] / 1e3:.3f} s, formatting and writing {i['write_ms'] / 1e3:.2f} s")
        say(f"device by HIP events, {i['chunks']} chunk(s): " + ", ".join(f"{n} {ms:.1f} ms" for n, ms in zip(STAGES, i["stage_ms"])))
        say(f"{i['target_minimizers']} target minimizers under {i['distinct_hashes']} hashes ({i['dropped_hashes']} over max_occ); {i['read_minimizers']} read minimizers, "
            f"{i['anchors']} anchors, {i['groups']} groups, {i['chained_groups']} with at least min_count anchors ({i['anchors'] / max(1, i['groups']):.1f} anchors a group)")
        right = primary = 0
        for line in open(paf):
            f = line.split("\t")
            if f[12] == "tp:A:P":
                primary += 1
                right += int(f[5][2:]) == origin[int(f[0][1:])]
        say(f"{i['reads']} reads: {i['mapped']} mapped, {i['unmapped']} unmapped, {i['secondary']} secondary lines; {right} of {primary} primary lines name the read's transcript "
            f"(an isoform's shared half can be either)")
        say(f"{i['reads'] / wall:.3g} reads per second of wall time, {total / (i['device_ms'] / 1e3):.3g} read bases per second of device time")
        say("There is no earlier implementation of these rules to compare a time against.")
        say()
        if a.align:
            al = j["align"]
            say("== the same call with align=True (map -c at the defaults: band 63, M for = and X), after the call above on the same context ==")
            say(f"map wall {wall_c:.2f} s: reading and parsing {j['read_ms'] / 1e3:.2f} s, packing and uploads {j['upload_ms'] / 1e3:.2f} s, device {j['device_ms'] / 1e3:.3f} s "
                f"+ alignment {al['align_ms'] / 1e3:.3f} s, formatting and writing {j['write_ms'] / 1e3:.2f} s")
            say(f"device by HIP events, {j['chunks']} chunk(s): " + ", ".join(f"{n} {ms:.1f} ms" for n, ms in zip(STAGES, j["stage_ms"])) + f", align {al['align_ms']:.1f} ms")
            say(f"(plain call above: wall {wall:.2f} s, device {i['device_ms'] / 1e3:.3f} s in {i['chunks']} chunk(s))")
            say(f"{al['lines']} lines aligned in {al['segments']} segments ({al['segments'] / max(1, al['lines']):.1f} a line, the longest spans {al['longest_segment']} "
                f"anti-diagonals); {al['cells']} allowed cells, {al['cells'] / max(1e-9, al['align_ms'] / 1e3):.3g} cells per second of the stage")
            say(f"{al['columns']} columns: {al['matches']} =, {al['mismatches']} X, {al['inserted']} I, {al['deleted']} D; "
                f"{os.path.getsize(os.path.join(d, 'aligned.paf')) >> 20} MB of PAF against {os.path.getsize(paf) >> 20} MB")
            say("extra device bytes: the stage's anchors, columns, traceback stores and runs take at most 128 MiB in a chunk (MAP_ALN_BYTES_MAX, map_host.h); "
                "the reads of a chunk are sized to that, which is why this call has more chunks than the plain one")
            say("There is no earlier implementation of these rules to compare a time against.")
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
            return

        # ---- observation: molecules made on the device, mapped back
        contigs, gtf, spliced = transcriptome(rs, acgt)
        with open(os.path.join(d, "ann.gtf"), "w") as f:
            f.write(gtf)
        with open(os.path.join(d, "ab.tsv"), "w") as f:
            f.write("transcript_id\ttpm\tcell_barcode\n" + "".join(f"{tid}\t{1 + k % 30}\t.\n" for k, (tid, _) in enumerate(spliced)))
        s = Sequencer(0)
        for name, seq in contigs:
            s.add_contig(name, seq)
        s.add_gtf(os.path.join(d, "ann.gtf"))
        s.set_identity(84.0, 99.0, 5.5)
        models = os.path.join(ROOT, "tksm_amd", "models", "badread")
        s.load_error_model(os.path.join(models, "nanopore2020.error.gz"))
        s.load_qscore_model(os.path.join(models, "nanopore2020.qscore.gz"))
        plan = s.transcribe_plan(os.path.join(d, "ab.tsv"), a.molecules, seed=5)
        truth = []
        for line in plan.mdf_text().splitlines():
            if line.startswith("+"):
                _, depth, comment = line[1:].split("\t")
                truth += [[x[4:] for x in comment.split(";") if x.startswith("tid=")][0]] * int(depth)
        batch = plan.batch()
        m = Sequencer(0)
        for tid, seq in spliced:
            m.add_contig(tid, seq)
        say(f"== observation: {batch.n_reads} molecules of {len(spliced)} transcripts made by transcribe on the device, sequenced, mapped to the spliced transcripts ==")
        for target in ("perfect", "badread"):
            recs = s.run(batch, target=target, fastq=True, seed=9).records()
            with open(os.path.join(d, target + ".fq"), "wb") as f:
                f.write(b"".join(recs))
            names = [r.split(b"\n", 1)[0][1:].split()[0].decode() for r in recs]
            i = m.map(os.path.join(d, target + ".fq"), os.path.join(d, target + ".paf"))
            rows = {l.split("\t")[0]: l.split("\t") for l in open(os.path.join(d, target + ".paf")) if "tp:A:P" in l}
            right = sum(1 for n, tid in zip(names, truth) if n in rows and rows[n][5] == tid)
            say(f"{target}{' (identity 84, 99, 5.5)' if target == 'badread' else ''}: {i['mapped']} of {len(names)} reads mapped, {right} to their own transcript, "
                f"{i['secondary']} secondary lines")
        batch.free()
        plan.close()
        m.close()
        s.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
