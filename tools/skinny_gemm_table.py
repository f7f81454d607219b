#!/usr/bin/env python
"""Skinny-M GEMM table: ``mfma_skinny`` (``csrc/gemm_skinny.hip``) against every other candidate
of the ``ops.linear`` dispatch whose contract holds (``mfma``, ``mfma_sk``, ``mfma_split``,
``blas`` = hipBLASLt) on the decode step's shapes, and against a bandwidth floor.

``mfma_skinny_w8`` is the weight-only FP8 form of the skinny kernel (``csrc/gemm_skinny.hip`` too,
``ops.fp8.linear_w8``): not a dispatch candidate (it changes numerics), timed beside the others on
the e4m3 copy of the same weights, with its own floor ``copy_w8`` — the copy of the e4m3 bytes —
and its ratio to ``mfma_skinny`` (the bytes say 0.5).

``mfma_skinny_w4`` is the weight-only MXFP4 form (``ops.mxfp4.linear_w4``), timed the same way on
the MXFP4 copy of the same weights (e2m1 codes + one e8m0 scale per 32 k: 0.266 of the bf16
bytes), with its floor ``copy_w4`` — the copy of exactly the code and scale bytes — and its ratios
to ``mfma_skinny_w8`` (the bytes say 0.53) and to ``mfma_skinny``.

Rows: the sixteen M = 8 shapes of the 7B decode step (four each at world 1 and on rank 0's shard
of a 2-, 4- and 8-way run) plus the shard-8 QKV shape at M = 1 and M = 16. ``--candidates``
restricts what is timed (``mfma_skinny`` and the copies always are).

All candidates of a row are timed in ONE process, each as a HIP graph of ``--inner`` (10)
back-to-back calls, median of ``--rounds`` (9) alternating rounds, twice:

* **cold**: the calls rotate over enough distinct copies of W to exceed the 256 MiB last-level
  cache (``--rotate-mb``; as many 10-call graphs as it takes to walk all copies, replayed in
  turn), as the 32 layers of a decode step do; the e4m3 weights are half the size, so there are
  twice as many of them, and as many MXFP4 ones as exceed the same bytes;
* **warm**: one W, as the autotuner times its candidates.

The floor is ``dst.copy_(src)`` of the same W bytes. The copy moves the bytes twice (read +
write), so its rate is given over 2x the bytes; ``share_of_copy`` is the skinny kernel's W read
rate over that.

Output in ``--out-dir`` (default ``profiles/skinny_gemm``): ``skinny_gemm.jsonl`` (one line per
row) and ``SUMMARY.md``. ``--pmc-loop N`` instead runs N plain launches of ``mfma_skinny`` per
row and nothing else: the form to put under ``rocprofv3 --pmc`` (counters in a run of their
own); ``--pmc-csv FILE...`` turns such runs' counter CSVs (one per counter pass, same
``--pmc-loop``) into ``pmc_skinny.jsonl``.
"""

from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# (label, M, N, K): config/7b_config.yaml, hidden 4096, ffn 16384, batch 8
DEFAULT_ROWS = [("w1 qkv", 8, 12288, 4096), ("w1 out", 8, 4096, 4096),
                ("w1 up", 8, 16384, 4096), ("w1 down", 8, 4096, 16384),
                ("s2 qkv", 8, 6144, 4096), ("s2 out", 8, 4096, 2048),
                ("s2 up", 8, 8192, 4096), ("s2 down", 8, 4096, 8192),
                ("s4 qkv", 8, 3072, 4096), ("s4 out", 8, 4096, 1024),
                ("s4 up", 8, 4096, 4096), ("s4 down", 8, 4096, 4096),
                ("s8 qkv", 8, 1536, 4096), ("s8 out", 8, 4096, 512),
                ("s8 up", 8, 2048, 4096), ("s8 down", 8, 4096, 2048),
                ("s8 qkv M=1", 1, 1536, 4096), ("s8 qkv M=16", 16, 1536, 4096)]


W8 = "mfma_skinny_w8"
W4 = "mfma_skinny_w4"


def candidates(gemm, x, w, out, only=None):
    M, K = x.shape
    N = w.shape[0]
    names = ["mfma_skinny", "mfma"]
    if gemm.streamk_ok(x, w):
        names.append("mfma_sk")
    if gemm.split_plan(M, N, K, gemm._num_cus(x.device)) is not None:
        names.append("mfma_split")
    names.append("blas")
    assert gemm.skinny_ok(x, w, out), "row outside the skinny contract"
    if only is not None:
        names = [n for n in names if n == "mfma_skinny" or n in only]
    return names


def _graphs(torch, fn, nbuf, inner):
    """Graphs of ``inner`` calls that together walk all ``nbuf`` weights (one graph when
    nbuf <= inner)."""
    for i in range(nbuf + 1):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for g0 in range(0, max(nbuf, 1), inner):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for i in range(inner):
                fn(g0 + i)
        gr.replay()
        out.append(gr)
    torch.cuda.synchronize()
    return out


def _time(torch, graph_sets, inner, rounds):
    times = {n: [] for n in graph_sets}
    for _ in range(rounds):                              # alternate the candidates
        for name, graphs in graph_sets.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for gr in graphs:
                gr.replay()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / (inner * len(graphs)))
    return ({n: statistics.median(v) for n, v in times.items()},
            {n: min(v) for n, v in times.items()})


def bench_row(label, M, N, K, args):
    import torch

    from distributed_llm_backend_benchmark_amd.ops import fp8, gemm, mxfp4

    dev = torch.device("cuda", 0)
    w_bytes = N * K * 2
    nbuf = max(1, -(-args.rotate_mb * (1 << 20) // w_bytes))
    g = torch.Generator(device=dev).manual_seed(N + K + M)
    ws = [(torch.rand(N, K, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
          for _ in range(nbuf)]
    x = (torch.rand(M, K, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    sink = torch.empty_like(ws[0])
    names = candidates(gemm, x, ws[0], out, args.candidates)
    with_w8 = args.candidates is None or W8 in args.candidates
    with_w4 = (args.candidates is None or W4 in args.candidates) and K % 128 == 0
    before = gemm.SKINNY_LAUNCHES["count"]
    ref = x.float() @ ws[0].float().t()
    errs = {}
    for n in names:
        gemm._IMPLS[n](x, ws[0], None, None, None, out, None)
        errs[n] = float((out.float() - ref).norm() / ref.norm())
    assert gemm.SKINNY_LAUNCHES["count"] == before + 1
    nbuf8 = 0
    if with_w8:
        # e4m3 copies of the same weights, and as many again to rotate over the same bytes
        nbuf8 = max(1, -(-args.rotate_mb * (1 << 20) // (w_bytes // 2)))
        q8 = [fp8.quantize_rows(ws[i % nbuf]) for i in range(nbuf8)]
        sink8 = torch.empty_like(q8[0][0])
        before = fp8.W8_LAUNCHES["count"]
        fp8.linear_w8(x, q8[0][0], q8[0][1], out=out)
        assert fp8.W8_LAUNCHES["count"] == before + 1
        errs[W8] = float((out.float() - ref).norm() / ref.norm())

    nbuf4, w4_bytes = 0, N * K // 2 + N * K // 32
    if with_w4:
        # MXFP4 copies of the same weights, each one flat buffer (codes, then scales) so that
        # copy_w4 moves exactly the bytes the kernel streams
        nbuf4 = max(1, -(-args.rotate_mb * (1 << 20) // w4_bytes))
        q4 = []
        for i in range(nbuf4):
            if i < nbuf:
                c, sc = mxfp4.quantize_mxfp4(ws[i])
                flat = torch.cat([c.view(-1), sc.view(-1)])
            else:
                flat = q4[i % nbuf][0].clone()
            q4.append((flat, flat[:N * K // 2].view(N, K // 2), flat[N * K // 2:].view(N, K // 32)))
        sink4 = torch.empty_like(q4[0][0])
        before = mxfp4.W4_LAUNCHES["count"]
        mxfp4.linear_w4(x, q4[0][1], q4[0][2], out=out)
        assert mxfp4.W4_LAUNCHES["count"] == before + 1
        errs[W4] = float((out.float() - ref).norm() / ref.norm())

    def call(n):
        f = gemm._IMPLS[n]
        return lambda i: f(x, ws[i % nbuf], None, None, None, out, None)

    fns = {n: call(n) for n in names}
    fns["copy"] = lambda i: sink.copy_(ws[i % nbuf])
    walk = {n: nbuf for n in fns}                        # distinct weights each candidate walks
    if with_w8:
        fns[W8] = lambda i: fp8.linear_w8(x, *q8[i % nbuf8], out=out)
        fns["copy_w8"] = lambda i: sink8.copy_(q8[i % nbuf8][0])
        walk[W8] = walk["copy_w8"] = nbuf8
    if with_w4:
        fns[W4] = lambda i: mxfp4.linear_w4(x, q4[i % nbuf4][1], q4[i % nbuf4][2], out=out)
        fns["copy_w4"] = lambda i: sink4.copy_(q4[i % nbuf4][0])
        walk[W4] = walk["copy_w4"] = nbuf4
    cold = _time(torch, {n: _graphs(torch, f, walk[n], args.inner) for n, f in fns.items()},
                 args.inner, args.rounds)
    warm = _time(torch, {n: _graphs(torch, (lambda i, f=f: f(0)), 1, args.inner)
                         for n, f in fns.items()}, args.inner, args.rounds)
    del ws, sink
    if with_w8:
        del q8, sink8
    if with_w4:
        del q4, sink4
    plan = gemm.skinny_plan(M, N, K, gemm._num_cus(dev))
    row = {"row": label, "M": M, "N": N, "K": K, "w_bytes": w_bytes, "rotated_weights": nbuf,
           "inner": args.inner, "rounds": args.rounds,
           "plan": {"grid": plan[0], "k_split_in_workgroup": plan[1],
                    "k_split_across_workgroups": plan[2], "workspace_bytes": plan[3]},
           "rel_frobenius_err": {n: round(v, 6) for n, v in errs.items()}}
    for tag, (med, mn) in (("cold", cold), ("warm", warm)):
        others = [n for n in names if n != "mfma_skinny"]
        best = min(others, key=lambda n: med[n]) if others else None    # --candidates left none
        row[tag] = {"us": {n: round(t, 2) for n, t in med.items()},
                    "us_min": {n: round(t, 2) for n, t in mn.items()},
                    "best_other": best,
                    "skinny_over_best_other": (round(med["mfma_skinny"] / med[best], 3)
                                               if best else None),
                    "fastest": min(names, key=lambda n: med[n]),
                    "skinny_GBps": round(w_bytes / med["mfma_skinny"] / 1e3, 1),
                    "copy_GBps_2x_bytes": round(2 * w_bytes / med["copy"] / 1e3, 1),
                    "share_of_copy": round(med["copy"] / (2 * med["mfma_skinny"]), 3)}
        if with_w8:
            # the W8 kernel: its e4m3 read rate, the copy of those bytes (moved twice), and its
            # time over the bf16 skinny kernel's in the same alternating rounds
            row[tag].update(
                w8_over_skinny=round(med[W8] / med["mfma_skinny"], 3),
                w8_GBps=round(w_bytes / 2 / med[W8] / 1e3, 1),
                copy_w8_GBps_2x_bytes=round(w_bytes / med["copy_w8"] / 1e3, 1),
                w8_share_of_copy=round(med["copy_w8"] / (2 * med[W8]), 3))
        if with_w4:
            # the W4 kernel: its code + scale read rate, the copy of those bytes (moved twice),
            # and its time over the W8 and the bf16 skinny kernels' in the same rounds
            row[tag].update(
                w4_over_skinny=round(med[W4] / med["mfma_skinny"], 3),
                w4_GBps=round(w4_bytes / med[W4] / 1e3, 1),
                copy_w4_GBps_2x_bytes=round(2 * w4_bytes / med["copy_w4"] / 1e3, 1),
                w4_share_of_copy=round(med["copy_w4"] / (2 * med[W4]), 3))
            if with_w8:
                row[tag]["w4_over_w8"] = round(med[W4] / med[W8], 3)
    if with_w8:
        p8 = fp8.w8_skinny_plan(M, N, K, gemm._num_cus(dev))
        row["w8_bytes"], row["rotated_weights_w8"] = w_bytes // 2, nbuf8
        row["plan_w8"] = {"grid": p8[0], "k_split_in_workgroup": p8[1]}
    if with_w4:
        p4 = mxfp4.w4_skinny_plan(M, N, K, gemm._num_cus(dev))
        row["w4_bytes"], row["rotated_weights_w4"] = w4_bytes, nbuf4
        row["plan_w4"] = {"grid": p4[0], "k_split_in_workgroup": p4[1]}
    return row


def _ratio(t) -> str:
    if t["best_other"] is None:
        return "n/a"
    return f"{t['skinny_over_best_other']:.2f} ({t['best_other']})"


def summary(rows) -> str:
    cols = ["mfma_skinny", W8, W4, "mfma", "mfma_sk", "mfma_split", "blas", "copy", "copy_w8",
            "copy_w4"]
    lines = ["# Skinny-M GEMM table (`tools/skinny_gemm_table.py`)", "",
             "µs per call (HIP graph of 10 calls, median of 9 alternating rounds). cold = calls "
             "rotate over > 256 MiB of distinct weights; warm = one weight. copy = "
             "`dst.copy_(src)` of the W bytes (moves them twice; GB/s over 2x the bytes). "
             "plan = workgroups x waves per workgroup (K-split inside the workgroup). "
             f"{W8} = the weight-only FP8 skinny kernel on the e4m3 copy of W (half the bytes; "
             "copy_w8 = the copy of those); W8 / skinny = its time over mfma_skinny's; W8 share = "
             "its e4m3 read rate over copy_w8's rate. "
             f"{W4} = the weight-only MXFP4 skinny kernel on the MXFP4 copy of W (0.266 of the "
             "bytes: codes + block scales; copy_w4 = the copy of exactly those); W4 / W8 and W4 / "
             "skinny = its time over theirs; W4 share = its read rate over copy_w4's rate.", ""]
    for tag in ("cold", "warm"):
        lines += [f"## {tag}", "",
                  "| row | M, N, K | W | plan | " + " | ".join(cols) +
                  " | skinny / best other | skinny GB/s | copy GB/s | fastest | W8 / skinny | "
                  "W8 GB/s | W8 share | W4 / W8 | W4 / skinny | W4 GB/s | W4 share |",
                  "|" + "---|" * (len(cols) + 15)]
        for r in rows:
            t = r[tag]
            us = " | ".join(f"{t['us'][c]:.1f}" if c in t["us"] else "n/a" for c in cols)
            lines.append(
                f"| {r['row']} | {r['M']}, {r['N']}, {r['K']} | {r['w_bytes'] / 2**20:.0f} MiB | "
                f"{r['plan']['grid']} x {r['plan']['k_split_in_workgroup']} | {us} | "
                f"{_ratio(t)} | {t['skinny_GBps']:.0f} | "
                f"{t['copy_GBps_2x_bytes']:.0f} | {t['fastest']} | " +
                (f"{t['w8_over_skinny']:.2f} | {t['w8_GBps']:.0f} | {t['w8_share_of_copy']:.2f} |"
                 if "w8_over_skinny" in t else "n/a | n/a | n/a |") +
                ((f" {t['w4_over_w8']:.2f} |" if "w4_over_w8" in t else " n/a |") +
                 f" {t['w4_over_skinny']:.2f} | {t['w4_GBps']:.0f} | "
                 f"{t['w4_share_of_copy']:.2f} |"
                 if "w4_over_skinny" in t else " n/a | n/a | n/a | n/a |"))
        lines.append("")
    diff = [r["row"] for r in rows if r["cold"]["fastest"] != r["warm"]["fastest"]]
    lines.append("Rows whose cold and warm rankings name a different fastest candidate: "
                 + (", ".join(diff) if diff else "none") + ".")
    return "\n".join(lines) + "\n"


def pmc_loop(rows, n):
    """Plain launches of the skinny kernel only (the run to put under ``rocprofv3 --pmc``)."""
    import torch

    from distributed_llm_backend_benchmark_amd.ops import gemm

    dev = torch.device("cuda", 0)
    for label, M, N, K in rows:
        g = torch.Generator(device=dev).manual_seed(N + K + M)
        w = (torch.rand(N, K, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
        x = (torch.rand(M, K, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        for _ in range(n):
            gemm._mfma_skinny_linear(x, w, None, None, None, out, None)
        torch.cuda.synchronize()
        print(f"pmc loop {label}: {n} launches, grid {gemm.skinny_plan(M, N, K, 256)}", flush=True)


def pmc_csv_to_jsonl(paths, rows, n, out_path):
    """rocprofv3 counter CSVs (one line per dispatch and counter; one file per counter pass) ->
    one JSON line per row: the mean of every counter over that row's launches of the skinny
    kernel (dispatch order = the order of ``pmc_loop``)."""
    merged = [{} for _ in rows]
    grids = [0 for _ in rows]
    for path in paths:
        per = {}
        with open(path) as f:
            for r in csv.DictReader(f):
                if "skinny" not in r.get("Kernel_Name", ""):
                    continue
                d = per.setdefault(int(r["Dispatch_Id"]), {})
                d[r["Counter_Name"]] = float(r["Counter_Value"])
                d["_grid"] = int(r.get("Grid_Size", 0) or 0)
        ids = sorted(per)
        for i in range(len(rows)):
            mine = [per[d] for d in ids[i * n:(i + 1) * n]]
            if not mine:
                continue
            grids[i] = mine[0]["_grid"]
            for k in sorted(k for k in mine[0] if k != "_grid"):
                merged[i][k] = statistics.mean(m[k] for m in mine if k in m)
    with open(out_path, "w") as f:
        for (label, M, N, K), mean, grid in zip(rows, merged, grids):
            f.write(json.dumps({"row": label, "M": M, "N": N, "K": K, "launches_per_pass": n,
                                "grid_threads": grid, "mean": mean}) + "\n")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", nargs="*", default=None, metavar="M,N,K")
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--rotate-mb", type=int, default=320)
    ap.add_argument("--candidates", nargs="*", default=None, metavar="NAME",
                    help=f"time only these beside mfma_skinny and the copies (e.g. {W8} {W4})")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles", "skinny_gemm"))
    ap.add_argument("--pmc-loop", type=int, default=0, metavar="N")
    ap.add_argument("--pmc-csv", nargs="+", default=None, metavar="FILE")
    args = ap.parse_args(argv)
    rows = ([(r, *(int(v) for v in r.split(","))) for r in args.rows] if args.rows
            else DEFAULT_ROWS)
    os.makedirs(args.out_dir, exist_ok=True)
    if args.pmc_csv:
        pmc_csv_to_jsonl(args.pmc_csv, rows, args.pmc_loop or 5,
                         os.path.join(args.out_dir, "pmc_skinny.jsonl"))
        return 0
    if args.pmc_loop:
        pmc_loop(rows, args.pmc_loop)
        return 0
    done = []
    with open(os.path.join(args.out_dir, "skinny_gemm.jsonl"), "w") as f:
        for label, M, N, K in rows:
            row = bench_row(label, M, N, K, args)
            done.append(row)
            f.write(json.dumps(row) + "\n")
            f.flush()
            for tag in ("cold", "warm"):
                t = row[tag]
                print(f"{label} [{M},{N},{K}] {tag}: " +
                      "  ".join(f"{n} {v:.1f}" for n, v in t["us"].items()) +
                      f" us | skinny {t['skinny_GBps']:.0f} GB/s, copy "
                      f"{t['copy_GBps_2x_bytes']:.0f} GB/s, skinny/best other {_ratio(t)}" +
                      (f", W8/skinny {t['w8_over_skinny']:.2f}, W8 share of its copy "
                       f"{t['w8_share_of_copy']:.2f}" if "w8_over_skinny" in t else "") +
                      (f", W4/W8 {t.get('w4_over_w8', float('nan')):.2f}, W4/skinny "
                       f"{t['w4_over_skinny']:.2f}, W4 share of its copy "
                       f"{t['w4_share_of_copy']:.2f}" if "w4_over_skinny" in t else ""),
                      flush=True)
    with open(os.path.join(args.out_dir, "SUMMARY.md"), "w") as f:
        f.write(summary(done))
    return 0


if __name__ == "__main__":
    sys.exit(main())
