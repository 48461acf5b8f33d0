"""Times of filter + merge on a synthetic batch: N molecules (seeded; 1 - 4 segments on two contigs, a substitution on some, every second
record with a real CB barcode, the others with `.`, an empty one or none), split by `info CB` and joined again -- the Flt / Flt --negate /
Mrg step of the README's single-cell experiment.

    python tools/filter_times.py [molecules=1000000] [reps=5] [log=profiles/filter_times.log]

(a) on the device: Sequencer.filter (both sides) + Sequencer.merge on a batch that is already there, wall time around the calls (each ends
    with the synchronisation that sizes its output), best of `reps`;
(b) over MDF text: `tksm filter -c "info CB"`, `tksm filter -c "info CB" --negate` and `cat` of the two outputs, wall time of the three
    processes, best of `reps` -- what the route costs when its two halves are split and joined through files.
Nobody promises a ratio: the log records what the run gives."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "tksm_amd", "tksm")


def generate(n, seed=1):
    rs = np.random.RandomState(seed)
    nseg = rs.randint(1, 5, n)
    st = rs.randint(0, 900_000, (n, 4))
    ln = rs.randint(50, 900, (n, 4))
    strand = np.where(rs.rand(n, 4) < 0.5, "+", "-")
    bc = rs.randint(0, 5000, n)
    cm = ["CB=.;", "CB=;", "tid=T1;"]
    out = []
    for i in range(n):
        out.append(f"+m{i}\t1\t{f'CB=B{bc[i]:05d};' if i % 2 == 0 else cm[i % 3]}\n")
        for k in range(nseg[i]):
            out.append(f"chr{1 + (i + k) % 2}\t{st[i, k]}\t{st[i, k] + ln[i, k]}\t{strand[i, k]}\t{'7G' if (i + k) % 4 == 0 else ''}\n")
    return "".join(out)


def main(n=1_000_000, reps=5, log_path=os.path.join(ROOT, "profiles", "filter_times.log")):
    import torch  # noqa: F401  (the ROCm runtime torch bundles, loaded first as everywhere in the project)
    from tksm_amd.sequence import Sequencer
    text = generate(n)
    lines = [f"filter + merge: times on the synthetic batch of tools/filter_times.py (seed 1): {n} molecules, {text.count(chr(10)) - n} segments, "
             f"{len(text) / 1e6:.0f} MB of MDF text; condition `info CB` (every second molecule true)", ""]
    s = Sequencer(0)
    for c in ("chr1", "chr2"):
        s.declare_contig(c, 1_000_000)
    b = s.batch_from_mdf(text)
    best = {"filter": None, "merge": None, "both": None}
    n_true = n_false = 0
    for rep in range(reps + 1):                                    # (the first repetition loads the code objects: not counted)
        s.synchronize()
        t0 = time.perf_counter()
        t, f = s.filter(b, ["info CB"])
        t1 = time.perf_counter()
        m = s.merge([t, f])
        s.synchronize()
        t2 = time.perf_counter()
        n_true, n_false = t.n_reads, f.n_reads
        assert m.n_reads == n
        for x in (t, f, m):
            x.free()
        if rep:
            for k, v in (("filter", t1 - t0), ("merge", t2 - t1), ("both", t2 - t0)):
                best[k] = v if best[k] is None else min(best[k], v)
    b.free()
    s.close()
    lines += ["== (a) on the device: Sequencer.filter (both sides) + Sequencer.merge, the batch already on the device ==",
              f"filter {1e3 * best['filter']:.2f} ms, merge {1e3 * best['merge']:.2f} ms, together {1e3 * best['both']:.2f} ms (wall, best of {reps}; "
              f"{n_true} true, {n_false} false; comments copied on the host, lengths and order of each output computed as for every device-made batch)", ""]
    with tempfile.TemporaryDirectory() as d:
        src, cb, nocb, merged = (os.path.join(d, x) for x in ("in.mdf", "cb.mdf", "nocb.mdf", "merged.mdf"))
        with open(src, "w") as g:
            g.write(text)
        best_files, parts = None, None
        for _ in range(reps):
            t0 = time.perf_counter()
            subprocess.run([EXE, "filter", "-i", src, "-t", cb, "-c", "info CB", "--verbosity", "OFF"], check=True)
            t1 = time.perf_counter()
            subprocess.run([EXE, "filter", "-i", src, "-t", nocb, "-c", "info CB", "--negate", "--verbosity", "OFF"], check=True)
            t2 = time.perf_counter()
            with open(merged, "wb") as out:
                subprocess.run(["cat", cb, nocb], stdout=out, check=True)
            t3 = time.perf_counter()
            if best_files is None or t3 - t0 < best_files:
                best_files, parts = t3 - t0, (t1 - t0, t2 - t1, t3 - t2)
        size = os.path.getsize(merged)
    lines += ["== (b) over MDF text: `tksm filter`, `tksm filter --negate`, `cat` ==",
              f"filter {parts[0]:.2f} s, filter --negate {parts[1]:.2f} s, cat {parts[2]:.2f} s, together {best_files:.2f} s (wall of the three processes, best of {reps}; "
              f"{size / 1e6:.0f} MB joined; each module starts a process, opens the device, parses the text, writes text)", "",
              "== read together ==",
              f"(b) / (a) = {best_files / best['both']:.0f} on this run: one machine, one visit, best of {reps} each.  (a) leaves out what a route pays once anyway "
              "(parsing the head, writing the last MDF or sequencing it); (b) pays parse + write twice in the middle of the route.  No ratio is promised or gated."]
    os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
    with open(log_path, "w") as g:
        g.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 1_000_000, int(a[1]) if len(a) > 1 else 5, a[2] if len(a) > 2 else os.path.join(ROOT, "profiles", "filter_times.log"))
