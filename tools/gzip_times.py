"""Rates of the device-side BGZF encoder (tksmseq_result_gzip) and of `tksm sequence --gzip device` against `--gzip host`.

    python tools/gzip_times.py [reads=200000] [molecules=2000000] [log=profiles/gzip_times.log]

(a) one Badread FASTQ batch with q-scores of `reads` bulk molecules: tksmseq_result_gzip, best of 5 by HIP events, as GB/s of input and
    as a share of the same batch's tksmseq_run (kernel_ms[4]); the size against zlib level 1 on the same bytes.
(b) `tksm sequence` on `molecules` molecules (the workload of tools/e2e_stream.py) into x.fastq.gz -> a pipe -> /dev/null, three runs
    each of --gzip host (the route without this encoder, unchanged) and --gzip device, interleaved; wall seconds per run.
Every step that uses the GPU is a child process under a time limit of its own; the first failure ends the script.
"""
import json
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch_leg(n):
    import torch  # noqa: F401  (the ROCm runtime torch bundles, loaded first as everywhere in the project)
    from tksm_amd import synthetic
    from tksm_amd.sequence import Sequencer
    models = os.path.join(ROOT, "tksm_amd", "models", "badread")
    rs = np.random.RandomState(1)
    lens = [8_000_000] * 4
    s = Sequencer(0)
    for c, ln in enumerate(lens):
        s.add_contig(f"chr{c + 1}", rs.choice(np.frombuffer(b"ACGT", np.uint8), ln).tobytes())
    s.set_identity(84.0, 99.0, 5.5)
    s.load_error_model(os.path.join(models, "nanopore2020.error.gz"))
    s.load_qscore_model(os.path.join(models, "nanopore2020.qscore.gz"))
    s.set_timing(True)
    m = synthetic.make_molecules(rs, lens, n, 1000, 200, kind="bulk")
    b = s.batch_from_arrays(m["reads"], m["intervals"], m["mods"], m["literals"], m["literal_pool"], m["ids"], m["id_pool"])
    s.run(b, target="badread", fastq=True, compute_qual=True, seed=1)
    r = s.run(b, target="badread", fastq=True, compute_qual=True, seed=1)
    run_ms = r.kernel_ms[4]
    best, out = None, None
    for _ in range(5):
        out, _, ms = r.gzip(with_info=True)
        best = ms if best is None else min(best, ms)
    plain, _ = r.download()
    ref = len(zlib.compress(plain[:64 << 20], 1)) / min(len(plain), 64 << 20) * len(plain)
    print(json.dumps({"leg": "batch", "reads": int(r.n_reads), "record_bytes": len(plain), "gzip_bytes": len(out), "gzip_ms": round(best, 3),
                      "input_GBps": round(len(plain) / best / 1e6, 2), "run_ms": round(run_ms, 3), "share_of_run": round(best / run_ms, 4),
                      "of_zlib_level_1": round(len(out) / ref, 4)}), flush=True)
    b.free()
    s.close()


def main():
    a = sys.argv[1:]
    if a and a[0] == "--batch-leg":
        return batch_leg(int(a[1]))
    n = int(a[0]) if len(a) > 0 else 200_000
    mols = int(a[1]) if len(a) > 1 else 2_000_000
    log_path = a[2] if len(a) > 2 else os.path.join(ROOT, "profiles", "gzip_times.log")
    lines = []

    def say(t):
        print(t, flush=True)
        lines.append(t)

    def finish(rc):
        with open(log_path, "w") as f:
            f.write("\n".join(lines) + "\n")
        sys.exit(rc)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--batch-leg", str(n)], capture_output=True, text=True, timeout=300)
    if r.returncode:
        say(f"batch leg failed (exit {r.returncode}): {r.stderr[-1500:]}")
        finish(1)
    say(r.stdout.strip().splitlines()[-1])
    # (b) the workload of tools/e2e_stream.py
    from tksm_amd import synthetic
    d = os.environ.get("E2E_DIR", "/tmp/gzip_times")
    os.makedirs(d, exist_ok=True)
    rs = np.random.RandomState(1)
    lens = [8_000_000] * 4
    with open(f"{d}/ref.fa", "w") as f:
        for c, ln in enumerate(lens):
            s = rs.choice(np.frombuffer(b"ACGT", np.uint8), ln).tobytes().decode()
            f.write(f">chr{c + 1}\n" + "\n".join(s[i:i + 80] for i in range(0, ln, 80)) + "\n")
    block = min(mols, 250_000)          # (distinct molecules; the file repeats them)
    text = synthetic.mdf_text(synthetic.make_molecules(rs, lens, block, 1000, 200, kind="bulk"), [f"chr{c + 1}" for c in range(4)])
    with open(f"{d}/in.mdf", "w") as f:
        for _ in range(max(1, mols // block)):
            f.write(text)
    link = f"{d}/x.fastq.gz"
    if not os.path.islink(link):
        os.symlink("/dev/stdout", link)
    env = dict(os.environ, TKSM_MODELS=os.path.join(ROOT, "tksm_amd", "models"))
    exe = os.path.join(ROOT, "tksm_amd", "tksm")
    walls = {"host": [], "device": []}
    for rep in range(3):
        for mode in ("host", "device"):
            cmd = f"'{exe}' sequence -i '{d}/in.mdf' -r '{d}/ref.fa' -o '{link}' -t 8 --verbosity ERROR --gzip {mode} | wc -c"
            t0 = time.time()
            r = subprocess.run(["bash", "-o", "pipefail", "-c", cmd], capture_output=True, text=True, env=env, timeout=600)
            wall = time.time() - t0
            if r.returncode:
                say(f"--gzip {mode} run {rep} failed (exit {r.returncode}): {r.stderr[-1500:]}")
                finish(1)
            walls[mode].append(wall)
            say(json.dumps({"leg": "cli", "gzip": mode, "run": rep, "molecules": mols, "wall_s": round(wall, 2), "bytes_out": int(r.stdout.split()[-1]),
                            "M_reads_per_s": round(mols / wall / 1e6, 3)}))
    ok = max(walls["device"]) < min(walls["host"])
    say(json.dumps({"leg": "verdict", "slowest_device_s": round(max(walls["device"]), 2), "fastest_host_s": round(min(walls["host"]), 2),
                    "device_faster_in_every_pairing": ok}))
    finish(0 if ok else 1)


if __name__ == "__main__":
    main()
