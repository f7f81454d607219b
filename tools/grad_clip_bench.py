"""Rate of the gradient sum-of-squares kernel (csrc/grad_clip.hip, dlbb_grad_sumsq) on bf16
buffers of 1 MiB, 64 MiB and 256 MiB plus GPT-2's 124 M elements, against
``torch.linalg.vector_norm`` on the same buffer and a device copy of the same bytes; with
``--sweep`` also every (loads in flight per lane, most workgroups) pair of dlbb_grad_sumsq_tune —
the table the kernel's two defaults were picked from (profiles/grad_clip/SUMMARY.md).

Device time from HIP events around ``batch`` calls issued back to back, warm, median of the
repeats: buffers up to the 256 MiB Infinity Cache stay resident in it between calls, so those
rows are cache-warm rates; the copy moves twice the bytes (read + write) — ``read_GBps`` is the
source bytes over the time, comparable with the read-only passes. One JSON line per row.

    python tools/grad_clip_bench.py [--sweep] [--dtype bf16|fp32]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_llm_backend_benchmark_amd.ops import _lib, grad_sumsq, sumsq_plan  # noqa: E402

GPT2_ELEMS = 124_439_808      # GPT-2 small, vocabulary padded to 50304


def t_med(fn, batch, iters=15, warm=3):
    """Median seconds per call; ``batch`` calls back to back per event pair."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(batch):
            fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e-3 / batch)
    ts.sort()
    return ts[len(ts) // 2]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    a = ap.parse_args()
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    esz = torch.tensor([], dtype=dtype).element_size()
    lib = _lib.lib()
    plan = sumsq_plan(0)
    sizes = [("1MiB", (1 << 20) // esz), ("64MiB", (64 << 20) // esz),
             ("256MiB", (256 << 20) // esz), ("gpt2_124M", GPT2_ELEMS)]
    part = torch.zeros(2048, device="cuda")
    for name, n in sizes:
        x = (torch.randn(n, device="cuda") * 0.02).to(dtype)
        y = torch.empty_like(x)
        nbytes = n * esz
        batch = max(2, min(200, int(2e9 // nbytes)))

        def row(case, t, **kw):
            print(json.dumps({"case": case, "size": name, "dtype": a.dtype, "n": n,
                              "bytes": nbytes, "batch": batch, "us": round(t * 1e6, 2),
                              "read_GBps": round(nbytes / t / 1e9, 1), **kw}), flush=True)

        row("sumsq", t_med(lambda: grad_sumsq(x, part[:plan["slots"]]), batch),
            unroll=plan["unroll"], grid_cap=plan["slots"], grid=sumsq_plan(n)["grid"])
        row("vector_norm", t_med(lambda: torch.linalg.vector_norm(x), batch))
        row("vector_norm_fp32acc",
            t_med(lambda: torch.linalg.vector_norm(x, dtype=torch.float32), batch))
        row("copy", t_med(lambda: y.copy_(x), batch))
        if a.sweep:
            st = _lib.stream(x.device)
            for unroll in (2, 4, 8):
                for cap in (256, 512, 1024, 2048):
                    def call():
                        _lib.check(lib.dlbb_grad_sumsq_tune(x.data_ptr(), _lib.dt(x), n,
                                                            part.data_ptr(), 2048, unroll, cap,
                                                            st), "grad_sumsq_tune")
                    row("sumsq_tune", t_med(call, batch), unroll=unroll, grid_cap=cap)
        # the result must not depend on the tuning: every pair sums the same values
        grad_sumsq(x, part[:plan["slots"]])
        ref = float(x.double().square().sum())
        got = float(part[:plan["slots"]].double().sum())
        assert abs(got - ref) <= 1e-5 * ref, (name, got, ref)
        del x, y
    return 0


if __name__ == "__main__":
    sys.exit(main())
