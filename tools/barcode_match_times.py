#!/usr/bin/env python3
"""barcode-match: where the time goes on a large synthetic input (profiles/barcode_match_times.log).

  python tools/barcode_match_times.py [--reads 1000000] [--barcodes 10000] [--molecules 2000] [--out profiles/barcode_match_times.log]

Makes --reads reads (0 to 40 random bases, the adapter, one of --barcodes barcodes of 16 letters with 0 to 2 substitutions, 100 to 300
random bases; half of them reverse-complemented), runs Sequencer.barcode_match once at the defaults and records the call's wall time split
into reading, packing and upload, device (HIP events, per stage) and writing, and the pairs per second.  There is no earlier implementation
of these rules to compare a time against.  Then, as an observation: --molecules molecules barcoded on the device (polya -> tag -> scb -> tag ->
flip -> tag), sequenced as perfect and as Badread reads, and the share of them whose own barcode comes back alone.  One machine, one run."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ADAPTER = b"CTACACGACGCTCTTCCGATCT"
RC = bytes.maketrans(b"ACGT", b"TGCA")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--barcodes", type=int, default=10000)
    ap.add_argument("--molecules", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "barcode_match_times.log"))
    a = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (its ROCm runtime has to be loaded before libtksmseq.so)
    from tksm_amd.sequence import Sequencer
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    rs = np.random.default_rng(1)
    letters = np.frombuffer(b"ACGT", np.uint8)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        barcodes = sorted({letters[rs.integers(0, 4, 16)].tobytes() for _ in range(a.barcodes)})
        pool = letters[rs.integers(0, 4, 1 << 24)].tobytes()
        pre, tail, which, at = rs.integers(0, 41, a.reads), rs.integers(100, 301, a.reads), rs.integers(0, len(barcodes), a.reads), rs.integers(0, (1 << 24) - 400, a.reads)
        subs, flip = rs.integers(0, 3, a.reads), rs.integers(0, 2, a.reads)
        with open(os.path.join(d, "reads.fq"), "wb") as f:
            for k in range(a.reads):
                bc = bytearray(barcodes[which[k]])
                for j in range(subs[k]):
                    bc[(5 * j + k) % 16] = pool[(at[k] + j) % len(pool)]
                s = pool[at[k]:at[k] + pre[k]] + ADAPTER + bytes(bc) + pool[at[k] + 50:at[k] + 50 + tail[k]]
                if flip[k]:
                    s = s.translate(RC)[::-1]
                f.write(b"@read%d\n%s\n+\n%s\n" % (k, s, b"I" * len(s)))
                if k % 200000 == 0:
                    print(f"  generated {k} reads", flush=True)
        with open(os.path.join(d, "whitelist.txt"), "wb") as f:
            f.write(b"\n".join(barcodes) + b"\n")
        size = os.path.getsize(os.path.join(d, "reads.fq"))
        say(f"barcode-match: times on the input of tools/barcode_match_times.py (seed 1): {a.reads} reads of 140 to 380 bases, {len(barcodes)} barcodes of 16 letters, "
            f"{size / 1e6:.0f} MB of FASTQ (made in {time.time() - t0:.0f} s).  One machine, one run.")
        say()
        s = Sequencer(0)
        t0 = time.time()
        info = s.barcode_match(os.path.join(d, "reads.fq"), os.path.join(d, "whitelist.txt"), os.path.join(d, "lr_matches.tsv.gz"))
        wall = time.time() - t0
        say("== device (MI355X, 1 GPU; Sequencer.barcode_match at the defaults, the matches file gzipped) ==")
        say(f"wall {wall:.2f} s: reading and parsing {info['read_ms'] / 1e3:.2f} s, packing and uploads {info['upload_ms'] / 1e3:.2f} s, device {info['device_ms'] / 1e3:.3f} s, "
            f"formatting and writing {info['write_ms'] / 1e3:.2f} s")
        st = info["stage_ms"]
        say(f"device by HIP events, {info['chunks']} chunk(s): adapter {st[0]:.1f} ms, selection {st[1]:.1f} ms, match {st[2]:.1f} ms, gather {st[3]:.1f} ms")
        say(f"{info['reads']} reads: {info['no_adapter']} without adapter, {info['forward']} forward, {info['reverse']} reverse; {info['candidates']} of {info['whitelist']} "
            f"barcodes are candidates; {info['unique']} reads with one barcode, {info['ambiguous']} with several, {info['no_barcode']} with none")
        say(f"{info['pairs']} pairs compared: {info['pairs'] / (st[2] / 1e3):.3g} per second of the match kernel, {info['pairs'] / wall:.3g} per second of wall time")
        say("There is no earlier implementation of these rules to compare a time against.")
        say()

        # ---- an observation: molecules barcoded on the device, read back
        comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
        rc = lambda x: "".join(comp[c] for c in reversed(x))
        s.add_contig("chrT", pool[:200000].decode())
        cbs = [b.decode() for b in barcodes[:200]]
        truth = [cbs[k % len(cbs)] for k in range(a.molecules)]
        text = "".join(f"+mol{k}\t1\tCB={cb};\nchrT\t{90 * k % 190000}\t{90 * k % 190000 + 400 + k % 300}\t{'+-'[k % 2]}\t\n" for k, cb in enumerate(truth))
        steps = [s.batch_from_mdf(text)]
        steps.append(s.polya(steps[-1], normal=(30.0, 5.0), seed=3))
        steps.append(s.tag(steps[-1], format3="10", seed=3))
        steps.append(s.scb(steps[-1]))
        steps.append(s.tag(steps[-1], format3=rc(ADAPTER.decode()), seed=4))
        steps.append(s.flip(steps[-1], 0.5, seed=5))
        steps.append(s.tag(steps[-1], format5=pool[300:328].decode(), format3=pool[400:428].decode(), seed=6))
        with open(os.path.join(d, "cbs.txt"), "w") as f:
            f.write("\n".join(cbs) + "\n")
        s.set_identity(84.0, 99.0, 5.5)
        models = os.path.join(ROOT, "tksm_amd", "models", "badread")
        s.load_error_model(os.path.join(models, "nanopore2020.error.gz"))
        s.load_qscore_model(os.path.join(models, "nanopore2020.qscore.gz"))
        say(f"== observation: {a.molecules} molecules barcoded on the device (polya -> tag 10 N -> scb -> tag adapter -> flip 0.5 -> tag outer adapters), "
            f"{len(cbs)} barcodes, --revcomp-barcodes ==")
        for target, extra in (("perfect", {}), ("badread", {}), ("badread", {"min_exact": 0})):
            recs = s.run(steps[-1], target=target, fastq=True, seed=9).records()
            with open(os.path.join(d, target + ".fq"), "wb") as f:
                f.write(b"".join(recs))
            names = [r.split(b"\n", 1)[0][1:].split()[0].decode() for r in recs]
            i = s.barcode_match(os.path.join(d, target + ".fq"), os.path.join(d, "cbs.txt"), os.path.join(d, target + ".tsv"), revcomp_barcodes=True, **extra)
            rows = {l.split("\t")[0]: l.rstrip("\n").split("\t") for l in open(os.path.join(d, target + ".tsv"))}
            right = sum(1 for n, cb in zip(names, truth) if n in rows and rows[n][2] == "1" and rows[n][4] == cb)
            say(f"{target}{' (identity 84, 99, 5.5)' if target == 'badread' else ''}{', min_exact 0' if extra else ''}: {right} of {len(names)} reads come back with their own barcode "
                f"alone at distance <= 2 ({i['no_adapter']} without adapter, {i['no_barcode']} without barcode, {i['ambiguous']} ambiguous, {i['candidates']} candidates)")
        for x in steps:
            x.free()
        s.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
