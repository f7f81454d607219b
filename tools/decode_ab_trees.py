#!/usr/bin/env python
"""Two-tree A/B of the shared-length decode kernels: ``./ab_old`` (a ``git archive`` of the parent
commit with its own in-tree build, as ``tools/ab_trees.sh`` uses it) against this tree.

Per round each tree's own ``tools/decode_bench.py`` runs once, in a process of its own, old then
new, so the trees' runs interleave in one session. Reported per shape and candidate (``ours``,
``two_launch``, ``ours_fp8``): every repeat's microseconds under both trees, the parent's own
spread across its repeats ``(max - min) / median``, and the new tree's median against the parent's
median. Rows go to ``profiles/ragged_decode/shared_length_ab.jsonl``.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ["8,32,128,512", "8,32,128,8192", "8,8,128,2048", "8,4,128,512", "8,4,128,8192",
        "8,12,64,1024"]
CANDS = ("ours", "two_launch", "ours_fp8")


def run_tree(tree, rows, rounds, timeout):
    with tempfile.NamedTemporaryFile(suffix=".jsonl") as f:
        cmd = [sys.executable, os.path.join(tree, "tools", "decode_bench.py"), "--rows", *rows,
               "--chunks", "256", "--fp8", "--fp8-chunks", "256", "--rounds", str(rounds),
               "--out", f.name]
        r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            raise RuntimeError(f"{tree}: decode_bench exit {r.returncode}\n{r.stderr[-2000:]}")
        return [json.loads(line) for line in open(f.name)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", default=os.path.join(REPO, "ab_old"))
    ap.add_argument("--rows", nargs="*", default=ROWS, metavar="B,H,D,L")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=9, help="decode_bench --rounds")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per decode_bench process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ragged_decode",
                                                  "shared_length_ab.jsonl"))
    args = ap.parse_args(argv)
    trees = {"old": args.old, "new": REPO}
    us = {}                                                  # (row, cand) -> {tree: [us, ...]}
    for i in range(args.repeats):
        for name, tree in trees.items():
            for row in run_tree(tree, args.rows, args.rounds, args.timeout):
                key = (row["B"], row["H"], row["D"], row["L"])
                for c in CANDS:
                    us.setdefault((key, c), {"old": [], "new": []})[name].append(row["us"][c])
            print(f"repeat {i} {name} done", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for (key, c), t in us.items():
            old, new = statistics.median(t["old"]), statistics.median(t["new"])
            rec = {"B": key[0], "H": key[1], "D": key[2], "L": key[3], "candidate": c,
                   "us_old": t["old"], "us_new": t["new"], "median_old": old, "median_new": new,
                   "old_spread": (max(t["old"]) - min(t["old"])) / old,
                   "new_over_old": new / old,
                   "inside_old_spread": min(t["old"]) <= new <= max(t["old"])}
            f.write(json.dumps(rec) + "\n")
            print(f"{key} {c}: old {old:.1f} us (spread {rec['old_spread'] * 100:.1f} %), new "
                  f"{new:.1f} us, new/old {rec['new_over_old']:.3f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
