"""Writes tests/golden/map_targets_known_answers.json: the specification (tests/map_targets_spec.py) on its hand-made table, the answers
checked by hand against include/tksmseq.h ("map, annotated targets"): which transcripts are kept and why the others are not, the letters of
every target, the layout, and the projection of lines that start, end and have their insertions and deletions at junctions.
    python tests/golden/make_map_targets_known_answers.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import map_targets_spec as T  # noqa: E402

HEAD = "\ttp:A:P\tcm:i:3\ts1:i:25"
LINES = [
    ("A", "r1\t40\t0\t25\t+\tA\t25\t0\t25\t25\t25\t60" + HEAD),
    ("A", "r1\t40\t0\t25\t+\tA\t25\t0\t25\t25\t25\t60" + HEAD + "\tNM:i:0\tcg:Z:25M"),
    ("A", "r2\t40\t2\t30\t-\tA\t25\t1\t24\t20\t29\t60" + HEAD + "\tNM:i:9\tcg:Z:10=2X7=3I1D2=2I1="),
    ("A", "r3\t40\t0\t20\t+\tA\t25\t0\t20\t20\t20\t60" + HEAD + "\tsn:i:2\tsi:i:1\tNM:i:0\tcg:Z:20="),
    ("A", "r4\t40\t0\t18\t+\tA\t25\t18\t25\t13\t18\t60\ttp:A:S\tcm:i:3\ts1:i:25\tNM:i:5\tcg:Z:1=4D5I2="),
    ("B", "r5\t40\t0\t25\t+\tB\t25\t0\t25\t25\t25\t60" + HEAD),
    ("B", "r5\t40\t0\t25\t-\tB\t25\t0\t25\t25\t25\t60" + HEAD + "\tNM:i:0\tcg:Z:25M"),
    ("B", "r6\t40\t5\t31\t+\tB\t25\t3\t23\t15\t28\t7" + HEAD + "\tNM:i:13\tcg:Z:5=6I12=3D2I"),
    ("H", "r7\t40\t0\t18\t+\tH\t18\t0\t18\t18\t18\t60" + HEAD + "\tNM:i:0\tcg:Z:18="),
    ("H", "r8\t40\t0\t9\t+\tH\t18\t9\t14\t3\t9\t60" + HEAD + "\tNM:i:6\tcg:Z:1=4I2D2="),
    ("H", "r9\t40\t0\t4\t+\tH\t18\t9\t13\t4\t4\t60" + HEAD),
    ("M", "r10\t40\t0\t1\t-\tM\t1\t0\t1\t1\t1\t0\ttp:A:P\tcm:i:1\ts1:i:1\tNM:i:0\tcg:Z:1="),
]


def main():
    t = T.targets(T.HOST_GENOME, T.HOST_TABLE)
    out = {"info": t["info"], "names": t["names"], "lengths": t["lengths"], "voff": t["voff"], "projectable": t["projectable"], "seqs": t["seqs"],
           "codes": t["codes"], "valid": t["valid"], "fasta_7": T.fasta(t, 7).decode(), "lines": []}
    for name, line in LINES:
        i = t["names"].index(name)
        projected, junctions = T.project_line(line, (name, len(T.HOST_GENOME[t["exons"][i][0][0]])), t["exons"][i])
        out["lines"].append({"target": name, "line": line, "projected": projected, "junctions": junctions})
    with open(os.path.join(HERE, "map_targets_known_answers.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
