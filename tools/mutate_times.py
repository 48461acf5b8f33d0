"""Times of mutate on a synthetic batch: N molecules of about 1 kb in 1 - 3 segments (seeded), device to device, next to the project's
yardstick for a segment edit, flip with p = 0, on the same batch in the same run.

    python tools/mutate_times.py [molecules=2000000] [reps=5] [log=profiles/mutate_times.log]

(a) a table of about one variant per kb on two contigs of 70 kb (140 rows), the molecules on those contigs;
(b) a table of a few million rows (3 000 000, one per ~670 bases) on four contigs of 500 Mb that are only declared
    (Sequencer.declare_contig), the molecules spread over them.
Wall time around each call (each ends with the synchronisations that size and finish its output), best of `reps`.  Per scenario the log
gives the meetings of a variant with a segment (counted on the host from the table and the segments) and the output's pieces, per second.
Nobody promises a ratio: the log records what the run gives."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def molecules(rs, n, contigs, length):
    """MDF text, and per contig the (start, end) arrays of its segments"""
    nseg = rs.randint(1, 4, n)
    ctg = rs.randint(0, len(contigs), (n, 3))
    ln = np.maximum(1, (rs.randint(800, 1200, n)[:, None] // nseg[:, None]) + rs.randint(-20, 21, (n, 3)))
    st = (rs.random_sample((n, 3)) * (length - 1300)).astype(np.int64)
    strand = np.where(rs.rand(n, 3) < 0.5, "+", "-")
    out = []
    for i in range(n):
        out.append(f"+m{i}\t1\t\n")
        for k in range(nseg[i]):
            out.append(f"{contigs[ctg[i, k]]}\t{st[i, k]}\t{st[i, k] + ln[i, k]}\t{strand[i, k]}\t{'7G' if (i + k) % 4 == 0 else ''}\n")
    used = np.arange(3)[None, :] < nseg[:, None]
    segs = {c: (st[used & (ctg == j)], (st + ln)[used & (ctg == j)]) for j, c in enumerate(contigs)}
    return "".join(out), segs


def table(rs, contigs, length, rows):
    """rows lines: 60 % SNVs, 20 % insertions of 1 - 6 letters, 20 % deletions of 1 - 8 bases; and the meetings counter's arrays"""
    ctg = rs.randint(0, len(contigs), rows)
    pos = (rs.random_sample(rows) * (length - 10)).astype(np.int64)
    kind = rs.random_sample(rows)
    dl = rs.randint(1, 9, rows)
    il = rs.randint(1, 7, rows)
    letters = rs.randint(0, 4, (rows, 7))
    out = []
    for r in range(rows):
        if kind[r] < 0.6:
            mod = "ACGT"[letters[r, 0]]
        elif kind[r] < 0.8:
            mod = ".ACGT"[letters[r, 0] + (r & 1)] + "".join("ACGT"[x] for x in letters[r, 1:1 + il[r]])
        else:
            mod = str(pos[r] + dl[r])
        out.append(f"{contigs[ctg[r]]}\t{pos[r]}\t{mod}\n")
    arrays = {}
    for j, c in enumerate(contigs):
        pt, de = (ctg == j) & (kind < 0.8), (ctg == j) & (kind >= 0.8)
        arrays[c] = (np.sort(pos[pt]), np.sort(pos[de]), np.sort(pos[de] + dl[de]))
    return "".join(out), arrays


def meetings(segs, arrays):
    n = 0
    for c, (s, e) in segs.items():
        pt, df, dt = arrays[c]
        n += int((np.searchsorted(pt, e, "left") - np.searchsorted(pt, s, "left")).sum())
        n += int((np.searchsorted(df, e, "left") - np.searchsorted(dt, s, "right")).sum())       # ranges with f < e minus those with t <= s
    return n


def scenario(s, name, text, segs, tab, arrays, reps):
    b = s.batch_from_mdf(text)
    v = s.load_variants(text=tab)
    calls = {"mutate": lambda: s.mutate(b, v), "flip p = 0": lambda: s.flip(b, 0.0, seed=1)}
    best, size = {}, {}
    for what, call in calls.items():
        for rep in range(reps + 1):                                    # (the first repetition loads the code objects and the table: not counted)
            s.synchronize()
            t0 = time.perf_counter()
            out = call()
            s.synchronize()
            dt = time.perf_counter() - t0
            size[what] = (out.n_reads, out.n_intervals, out.n_mods)
            out.free()
            if rep:
                best[what] = min(best.get(what, dt), dt)
    m = meetings(segs, arrays)
    line = (f"{name}: {v.rows} rows ({v.snvs} SNVs, {v.insertions} insertions, {v.deletions} deletions in {v.deleted_ranges} ranges, {v.dropped_points} points dropped); "
            f"{b.n_reads} molecules, {b.n_intervals} segments, {b.n_mods} substitutions in; mutate {1e3 * best['mutate']:.2f} ms -> {size['mutate'][1]} pieces, "
            f"{size['mutate'][2]} substitutions; {m} variant-segment meetings: {m / best['mutate'] / 1e6:.1f} M meetings/s, {size['mutate'][1] / best['mutate'] / 1e6:.1f} M pieces/s; "
            f"flip p = 0 on the same batch {1e3 * best['flip p = 0']:.2f} ms")
    b.free()
    v.close()
    return line


def main(n=2_000_000, reps=5, log_path=os.path.join(ROOT, "profiles", "mutate_times.log")):
    import torch  # noqa: F401  (the ROCm runtime torch bundles, loaded first as everywhere in the project)
    from tksm_amd.sequence import Sequencer
    rs = np.random.RandomState(1)
    lines = [f"mutate: times on the synthetic batches of tools/mutate_times.py (seed 1): {n} molecules of about 1 kb in 1 - 3 segments, device to device, wall, best of {reps}", ""]
    s = Sequencer(0)
    small, big = ["chr1", "chr2"], ["big1", "big2", "big3", "big4"]
    for c in small:
        s.declare_contig(c, 70_000)
    for c in big:
        s.declare_contig(c, 500_000_000)
    text, segs = molecules(rs, n, small, 70_000)
    tab, arrays = table(rs, small, 70_000, 140)
    lines.append(scenario(s, "(a) one variant per kb on two 70 kb contigs", text, segs, tab, arrays, reps))
    text, segs = molecules(rs, n, big, 500_000_000)
    tab, arrays = table(rs, big, 500_000_000, 3_000_000)
    lines.append(scenario(s, "(b) 3 000 000 rows on four declared contigs of 500 Mb", text, segs, tab, arrays, reps))
    s.close()
    lines += ["", "One machine, one visit.  Every call ends with what every device-made batch gets: the three scans, the tables, lengths and order of the output.  "
              "No ratio is promised or gated."]
    os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
    with open(log_path, "w") as g:
        g.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 2_000_000, int(a[1]) if len(a) > 1 else 5, a[2] if len(a) > 2 else os.path.join(ROOT, "profiles", "mutate_times.log"))
