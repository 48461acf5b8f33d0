#!/usr/bin/env python3
"""Writes tests/golden/map_split_known_answers.json: what tests/map_split_spec.py gives for its crafted cases (edge_case) under every
variant of map_split_spec.VARIANTS, without alignment and with -c --eqx --extend.  The answers are this project's own: they record the
specification, so that a later edit of it shows.  Run from the repository root: python tests/golden/make_map_split_known_answers.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import map_split_spec as S  # noqa: E402


def main():
    targets, reads, params = S.edge_case()
    memo, cases = {}, []
    for variant, v in S.VARIANTS.items():
        for mode in ({}, dict(align=True, eqx=True, extend=True)):
            out = S.map_reads(targets, reads, memo=memo, **mode, **v, **params)
            cases.append({"variant": variant, "mode": mode, "paf": out["paf"], "split": out["split"], "info": out["info"]})
    path = os.path.join(HERE, "map_split_known_answers.json")
    with open(path, "w") as f:
        json.dump(cases, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
