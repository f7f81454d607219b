"""FP8 vs bf16 GEMM table of the TP transformer's per-rank shapes (as tools/tp_gemm_table.py:
shapes of models.py:126-144 at P = 1/2/4/8), one process, interleaved rounds, uniform random
operands (CDNA guide §5.4 rules 24/25). Per shape, best of the rounds:

* every bf16 candidate of the ``ops.linear`` dispatch that exists for the shape (``mfma``,
  ``mfma192``, ``mfma192p``, ``mfma_sk``, ``mfma_split``, ``blas`` = hipBLASLt) and the best of them;
* the FP8 GEMM alone (``ops.linear_fp8`` on pre-quantised operands), with the balanced DMA issue
  off / on (``fp8_bal0`` / ``fp8_bal1``) and as shipped (``fp8``);
* the activation quantiser alone (``ops.quantize_rows`` of the [tokens, K] input; like the FP8
  GEMM timed as the bare launch, the cost under HIP-graph replay);
* ``torch._scaled_mm`` with row-wise e4m3fn scales, where this torch / hipBLASLt accepts it (a
  yardstick only: it is on no model path).

One JSON line per shape (``--out`` also appends them to a file).

    python tools/fp8_gemm_table.py [--model 7B] [--ps 1,2,4,8] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_llm_backend_benchmark_amd import ops  # noqa: E402
from distributed_llm_backend_benchmark_amd.ops import _lib, fp8, gemm  # noqa: E402

from tp_gemm_table import tp_shapes, timed  # noqa: E402


def bf16_candidates(x, w, out):
    M, K = x.shape
    N = w.shape[0]
    impls = dict(gemm._IMPLS)
    if not gemm.mfma192_ok(M, N):
        del impls["mfma192"]
    if not gemm.mfma192p_ok(M, N, K, True):
        del impls["mfma192p"]
    if not gemm.streamk_ok(x, w):
        del impls["mfma_sk"]
    if gemm.split_plan(M, N, K, gemm._num_cus(x.device)) is None:
        del impls["mfma_split"]
    return {n: (lambda f=f: f(x, w, None, None, None, out, None)) for n, f in impls.items()}


def scaled_mm_candidate(xq, xs, wq, ws):
    """torch._scaled_mm with row-wise scales, or None when this build refuses it."""
    try:
        fn = lambda: torch._scaled_mm(xq, wq.t(), scale_a=xs.view(-1, 1), scale_b=ws.view(1, -1),  # noqa: E731
                                      out_dtype=torch.bfloat16)
        fn()
        torch.cuda.synchronize()
        return fn
    except Exception as e:  # noqa: BLE001 - recorded, not fatal
        return f"{type(e).__name__}: {e}"[:200]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--ps", default="1,2,4,8")
    ap.add_argument("--tokens", type=int, default=4096, help="B*S (baseline 8 x 512)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default=None, help="comma list of case names to keep")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    shapes = []
    for P in [int(p) for p in args.ps.split(",")]:
        shapes += tp_shapes(args.model, P, args.tokens)
    if args.shapes:
        keep = set(args.shapes.split(","))
        shapes = [s for s in shapes if s[0] in keep]
    for name, M, N, K in shapes:
        g = torch.Generator(device="cuda").manual_seed(0)
        x = (torch.rand(M, K, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
        w = (torch.rand(N, K, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
        ref = x.float() @ w.float().t()
        out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        xq, xs = ops.quantize_rows(x)
        wq, ws = ops.quantize_rows(w)
        qbuf, sbuf = torch.empty_like(xq), torch.empty_like(xs)
        cands = bf16_candidates(x, w, out)
        bf16_names = list(cands)

        ops.linear_fp8(xq, xs, wq, ws, out=out)          # checks the contract once
        lib, stream = _lib.lib(), _lib.stream(x.device)
        fargs = (xq.data_ptr(), K, wq.data_ptr(), K, xs.data_ptr(), ws.data_ptr(),
                 out.data_ptr(), N, M, N, K, None, None, 0, 0, 0, stream)

        def fp8_run(bal):
            # the bare launch, as the bf16 candidates are (no per-call argument checks)
            def run():
                lib.dlbb_gemm_fp8_set_bal(bal)
                _lib.check(lib.dlbb_gemm_fp8_nt(*fargs), "gemm_fp8_nt")
            return run
        cands["fp8_bal0"], cands["fp8_bal1"], cands["fp8"] = fp8_run(0), fp8_run(1), fp8_run(2)
        ops.quantize_rows(x, out_q=qbuf, out_scale=sbuf)          # checks the contract once
        qargs = (x.data_ptr(), x.stride(0), qbuf.data_ptr(), K, sbuf.data_ptr(), M, K, stream)
        cands["quant"] = lambda: _lib.check(lib.dlbb_quant_fp8_rows(*qargs), "quant_fp8_rows")
        smm = scaled_mm_candidate(xq, xs, wq, ws)
        if callable(smm):
            cands["scaled_mm"] = smm
        errs = {}
        for n in list(bf16_names) + ["fp8", "scaled_mm"]:
            if n in cands:
                y = cands[n]()
                y = out if y is None else y
                errs[n] = round(float((y.float() - ref).norm() / ref.norm()), 5)
        best = {n: 1e9 for n in cands}
        for _ in range(args.rounds):
            for n, fn in cands.items():
                best[n] = min(best[n], timed(fn, args.iters))
        fp8.set_bal(2)
        fl = 2.0 * M * N * K
        bf16_best = min(bf16_names, key=lambda n: best[n])
        rec = {"case": name, "M": M, "N": N, "K": K,
               **{f"{n}_ms": round(best[n] * 1e3, 4) for n in cands},
               "bf16_best": bf16_best, "bf16_best_ms": round(best[bf16_best] * 1e3, 4),
               "bf16_best_tflops": round(fl / best[bf16_best] / 1e12, 1),
               "fp8_tflops": round(fl / best["fp8"] / 1e12, 1),
               "fp8_vs_bf16_best": round(best[bf16_best] / best["fp8"], 3),
               "fp8_plus_quant_vs_bf16_best": round(best[bf16_best] / (best["fp8"] + best["quant"]), 3),
               "quant_GBps": round((M * K * 3 + M * 4) / best["quant"] / 1e9, 1),
               "scaled_mm": "timed" if callable(smm) else smm,
               "rel_frobenius_err": errs}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
