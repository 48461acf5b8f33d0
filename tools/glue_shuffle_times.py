"""Times of unsegment (glue) and shuffle on a synthetic batch: N molecules (seeded; 1 - 4 segments on two contigs, a substitution on some, a
comment on every second record).

    python tools/glue_shuffle_times.py [molecules=1000000] [reps=5] [log=profiles/glue_shuffle_times.log]

(a) on the device: Sequencer.glue at p = 0.1, Sequencer.shuffle of the whole batch, Sequencer.shuffle with buffer_size 65536, each on a
    batch that is already there; wall time around the call (each ends with the synchronisations that size and finish its output), best of
    `reps`;
(b) over MDF text: `tksm unsegment -p 0.1`, `tksm shuffle`, `tksm shuffle --buffer-size 65536`, wall time of each process, best of `reps`.
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
P, B = 0.1, 65536


def generate(n, seed=1):
    rs = np.random.RandomState(seed)
    nseg = rs.randint(1, 5, n)
    st = rs.randint(0, 900_000, (n, 4))
    ln = rs.randint(50, 900, (n, 4))
    strand = np.where(rs.rand(n, 4) < 0.5, "+", "-")
    bc = rs.randint(0, 5000, n)
    out = []
    for i in range(n):
        out.append(f"+m{i}\t1\t{f'CB=B{bc[i]:05d};' if i % 2 == 0 else ''}\n")
        for k in range(nseg[i]):
            out.append(f"chr{1 + (i + k) % 2}\t{st[i, k]}\t{st[i, k] + ln[i, k]}\t{strand[i, k]}\t{'7G' if (i + k) % 4 == 0 else ''}\n")
    return "".join(out)


def main(n=1_000_000, reps=5, log_path=os.path.join(ROOT, "profiles", "glue_shuffle_times.log")):
    import torch  # noqa: F401  (the ROCm runtime torch bundles, loaded first as everywhere in the project)
    from tksm_amd.sequence import Sequencer
    text = generate(n)
    lines = [f"unsegment + shuffle: times on the synthetic batch of tools/glue_shuffle_times.py (seed 1): {n} molecules, {text.count(chr(10)) - n} segments, "
             f"{len(text) / 1e6:.0f} MB of MDF text; glue at p = {P}, shuffle whole and with buffer_size {B}", ""]
    s = Sequencer(0)
    for c in ("chr1", "chr2"):
        s.declare_contig(c, 1_000_000)
    b = s.batch_from_mdf(text)
    calls = {"glue": lambda: s.glue(b, P, seed=1), "shuffle whole": lambda: s.shuffle(b, seed=1), f"shuffle B = {B}": lambda: s.shuffle(b, seed=1, buffer_size=B)}
    best, sizes = {}, {}
    for name, call in calls.items():
        for rep in range(reps + 1):                                # (the first repetition loads the code objects: not counted)
            s.synchronize()
            t0 = time.perf_counter()
            out = call()
            s.synchronize()
            dt = time.perf_counter() - t0
            sizes[name] = out.n_reads
            out.free()
            if rep:
                best[name] = min(best.get(name, dt), dt)
    b.free()
    s.close()
    lines += ["== (a) on the device: the batch already on the device ==",
              "; ".join(f"{name} {1e3 * best[name]:.2f} ms ({sizes[name]} molecules out)" for name in calls) +
              f" (wall, best of {reps}; comments and, for glue, the joiners' ids handled on the host; lengths and order of each output computed as for every device-made batch)", ""]
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.mdf"), os.path.join(d, "out.mdf")
        with open(src, "w") as g:
            g.write(text)
        cli = {"unsegment": ["unsegment", "-p", str(P)], "shuffle": ["shuffle"], f"shuffle --buffer-size {B}": ["shuffle", "--buffer-size", str(B)]}
        best_cli = {}
        for name, args in cli.items():
            for _ in range(reps):
                t0 = time.perf_counter()
                subprocess.run([EXE, *args, "-i", src, "-o", dst, "-s", "1", "--verbosity", "OFF"], check=True)
                dt = time.perf_counter() - t0
                best_cli[name] = min(best_cli.get(name, dt), dt)
    lines += ["== (b) over MDF text: one `tksm` process each ==",
              "; ".join(f"{name} {best_cli[name]:.2f} s" for name in cli) +
              f" (wall of the process, best of {reps}; each starts a process, opens the device, parses the text, writes text; shuffle holds the whole input as one batch)", "",
              "== read together ==",
              "One machine, one visit, best of " + str(reps) + " each.  (a) leaves out what a route pays once anyway (parsing the head, writing the last MDF or sequencing "
              "it); (b) is what a step costs when the route goes through a file there.  No ratio is promised or gated."]
    os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
    with open(log_path, "w") as g:
        g.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 1_000_000, int(a[1]) if len(a) > 1 else 5, a[2] if len(a) > 2 else os.path.join(ROOT, "profiles", "glue_shuffle_times.log"))
