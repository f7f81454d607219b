"""Tensor-parallel transformer forward benchmark — ``run_mpi.py`` parity.

Reference: ``run_mpi.py:52-248`` (argparse ``--config``/``--backend``; world-size check;
init timing; warmup loop; timed loop with a barrier before and after each forward; per-rank
forward means gathered to rank 0 with variance / CV; JSON ``{output_dir}/{backend}_{name}.json``
with keys ``experiment, backend, config, system_info, rank_0_summary, rank_statistics,
raw_metrics_rank_0`` (``run_mpi.py:217-225``)).

Launch (one process per GPU)::

    torchrun --nproc-per-node 4 --master-addr 127.0.0.1 -m \
        distributed_llm_backend_benchmark_amd.cli.run_tp --config config/baseline_config.yaml \
        --backend rccl

Differences by design: the forward is device-timed (barrier, then synchronised wall clock and
HIP events); ``--backend`` picks the process-group backend (``rccl`` | ``gloo``) and names the
output file; extra result keys: ``tokens_per_s``, ``tflops_per_rank``, ``allreduce_bytes``.

``--decode N`` adds autoregressive decode: every timed iteration empties a per-rank KV cache,
runs the prefill forward (timed as above) and then N one-token steps over the cache (one captured
step replayed N times where the forward is capturable; ``--eager`` issues them from the host).
The record gets a ``decode`` section (``ms_per_token``, ``achieved_GBps``, ...) and the file name
the suffix ``_decode<N>``. ``--decode-weights fp8`` streams the e4m3 copy of every linear's weight
in those steps (weight-only FP8, bf16 activations): suffix ``_decode<N>_w8``, and the ``decode``
section counts the streamed bytes. ``--decode-weights mxfp4`` streams the MXFP4 copy (e2m1 codes,
one e8m0 scale per 32 k; ``ops.mxfp4``) the same way: suffix ``_decode<N>_w4``. ``--kv-cache fp8`` keeps the KV cache of those steps as e4m3
codes with one fp32 scale per cached row (``ops.decode``): suffix ``_kv8`` (after ``_w8`` / ``_w4``), the
``decode`` section carries ``kv_dtype`` and counts codes + scales in its cache and K / V bytes. It
composes with ``--decode-weights fp8`` / ``mxfp4`` and needs decode tokens and a real attention (not ``slice``).
``--prompt-lens L0,L1,...`` (``execution.prompt_lengths``) makes the batch right-padded prompts of
these lengths over a per-sequence KV cache (``ops.decode``): one value per batch row in ``[1,
sequence_length]``; needs decode tokens and a real attention, composes with ``--kv-cache fp8`` and
``--decode-weights``. The split grid is bounded by ``max + N``, the ``decode`` section carries
``prompt_lengths`` and counts the K / V bytes of the per-row lengths, the suffix ``_ragged`` comes
last. The captured step replays as before: the lengths are device memory.
``--kv-page-size P`` (``execution.kv_page_size``; 16 | 32 | 64 | 128 | 256) keeps the K / V of those
steps in a PAGED cache (``ops.decode``): one pool of ``--kv-pages N`` (``execution.kv_pool_pages``;
default ``sum_b ceil((len_b + N) / P)``, exactly what the run needs) pages per layer, shared by the
rows through a block table. Needs decode tokens and a real attention; composes with
``--prompt-lens`` (absent: every row at ``sequence_length``), ``--kv-cache fp8`` and
``--decode-weights``. Every row's final length is reserved before the first forward, so the table
never changes and the prefill and the step replay from their graphs. The ``decode`` section carries
``kv_page_size``, ``kv_pool_pages`` and ``kv_pages_peak``, ``kv_cache_bytes_per_rank`` is the pools,
and the suffix ``_paged<P>`` comes after ``_ragged``.
"""

from __future__ import annotations

import argparse
import os
import sys
import time


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="TP transformer forward benchmark (run_mpi.py parity)")
    ap.add_argument("--config", required=True, help="YAML config (reference schema)")
    ap.add_argument("--backend", default="rccl", choices=["rccl", "gloo", "nccl"],
                    help="process-group backend; also names the output file")
    ap.add_argument("--allreduce", choices=["auto", "rccl", "custom", "native"], default=None,
                    help="override execution.allreduce")
    ap.add_argument("--device", choices=["auto", "cpu", "cuda"], default="auto",
                    help="tensor device; auto = cuda for rccl, cpu for gloo. gloo + cuda = "
                         "several ranks sharing one GPU over a gloo process group (rehearsal "
                         "of the multi-rank path; RCCL needs one GPU per rank)")
    ap.add_argument("--allreduce-dtype", choices=["bf16", "fp32"], default=None)
    ap.add_argument("--attention", choices=["slice", "sdpa", "flash"], default=None,
                    help="slice = the reference's stub (models.py:162-167, default); sdpa = "
                         "torch causal attention; flash = our causal flash kernel")
    ap.add_argument("--kernels", choices=["hip", "torch"], default=None)
    ap.add_argument("--gemm-dtype", choices=["bf16", "fp8"], default=None,
                    help="GEMM operand type of the TP linears (execution.gemm_dtype): fp8 = e4m3 "
                         "with per-token / per-output-row scales on the FP8 GEMM kernel; output "
                         "file gets the suffix _fp8")
    ap.add_argument("--model-size", default=None, help="override with a MODEL_CONFIGS size")
    ap.add_argument("--num-layers", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--output-dir", default=None)
    ap.add_argument("--graph", action="store_true",
                    help="(default where capturable) capture the forward in a HIP graph and "
                         "replay it: world 1, or all-reduces not issued through "
                         "ProcessGroupNCCL (custom / native / auto)")
    ap.add_argument("--eager", action="store_true",
                    help="time the forward issued eagerly from the host every iteration (the "
                         "reference's host-timed semantics, run_mpi.py:173-188) instead of "
                         "replaying the captured HIP graph")
    ap.add_argument("--trace", action="store_true",
                    help="emit roctx ranges (record with rocprofv3 --marker-trace)")
    ap.add_argument("--torch-profile", default=None, metavar="DIR",
                    help="torch.profiler Chrome trace per rank into DIR")
    ap.add_argument("--ignore-world-size", action="store_true",
                    help="accept any world size (reference exits on mismatch, run_mpi.py:73-77)")
    ap.add_argument("--shard-as", type=int, default=None, metavar="P",
                    help="world 1 only: run rank 0's shard of a P-way TP model (the exact "
                         "per-rank GEMM / LN shapes) with each all-reduce replaced by a local "
                         "stand-in (one rank's one-shot HBM traffic; + link time with "
                         "--emulate-busbw); output <backend>_<name>_shard<P>.json")
    ap.add_argument("--emulate-busbw", type=float, default=None, metavar="GBPS",
                    help="with --shard-as: also hold 32 workgroups for the ring all-reduce time "
                         "bytes*2(P-1)/P / busBW per all-reduce")
    ap.add_argument("--overlap-chunks", type=int, default=None, metavar="N",
                    help="split the batch into N micro-batches and interleave them so each "
                         "row-parallel all-reduce (side comm stream) runs under the next "
                         "micro-batch's GEMMs (execution.overlap_chunks; 1 = blocking, as the "
                         "reference)")
    ap.add_argument("--chunk-streams", action="store_true",
                    help="with --overlap-chunks: each micro-batch on a compute stream of its own "
                         "(verified concurrent, parallel/streams.py)")
    ap.add_argument("--decode", type=int, default=None, metavar="N",
                    help="after the prefill forward of every timed iteration, decode N tokens "
                         "one at a time over a per-rank KV cache (execution.decode_tokens; 0 = "
                         "the prefill forward alone); adds a \"decode\" section to the record "
                         "and the suffix _decode<N> to the output file")
    ap.add_argument("--decode-weights", choices=["bf16", "fp8", "mxfp4"], default=None,
                    help="with --decode: weight type the decode steps stream "
                         "(execution.decode_weight_dtype): fp8 = e4m3 with per-output-row scales "
                         "on the weight-only FP8 skinny GEMM, bf16 activations, batch <= 16; "
                         "output file gets the suffix _w8; mxfp4 = e2m1 codes with one e8m0 "
                         "scale per 32 k on the weight-only MXFP4 skinny GEMM, the same limits, "
                         "suffix _w4")
    ap.add_argument("--kv-cache", choices=["bf16", "fp8"], default=None,
                    help="with --decode: storage of the KV cache (execution.kv_cache_dtype): fp8 = "
                         "e4m3 codes with one fp32 scale per cached row, head_dim + 4 bytes per "
                         "row instead of 2 head_dim; not with attention slice (no cache); output "
                         "file gets the suffix _kv8")
    ap.add_argument("--prompt-lens", default=None, metavar="L0,L1,...",
                    help="with --decode: the batch is right-padded prompts of these lengths "
                         "(execution.prompt_lengths), one per batch row in [1, sequence_length], "
                         "decoded over a per-sequence KV cache; not with attention slice; output "
                         "file gets the suffix _ragged")
    ap.add_argument("--kv-page-size", type=int, default=None, metavar="P",
                    help="with --decode: a PAGED KV cache of pages of P positions "
                         "(execution.kv_page_size; 16|32|64|128|256), shared by the batch rows "
                         "through a block table; not with attention slice; composes with "
                         "--prompt-lens, --kv-cache fp8 and --decode-weights; output file gets the "
                         "suffix _paged<P>")
    ap.add_argument("--kv-pages", type=int, default=None, metavar="N",
                    help="with --kv-page-size: pages of the pool per layer "
                         "(execution.kv_pool_pages; default: exactly what the run needs, "
                         "sum_b ceil((len_b + N) / P))")
    ap.add_argument("--max-len", type=int, default=None, metavar="L",
                    help="with --decode: positions of the KV cache (default sequence_length + N)")
    ap.add_argument("--check-dense", action="store_true",
                    help="after warmup, load the TP shards from a dense world-1 model of the "
                         "same seed (built on every rank) and report the max error of the TP "
                         "output against it (needs world > 1 on real ranks)")
    return ap.parse_args(argv)


def main(argv=None) -> int:
    args = parse_args(argv)
    # config + thread env BEFORE importing torch (reference sets it after: SURVEY §2.8 item 8)
    from ..utils.config import load_config, setup_environment

    config = load_config(args.config)
    setup_environment(config)

    import numpy as np
    import torch

    from ..data import create_dataset_from_config
    from ..models.tp_transformer import MODEL_CONFIGS, create_model_from_config
    from ..parallel.comm import init_distributed
    from ..utils.io import save_results
    from ..utils.metrics import MetricsCollector, print_summary, rank_statistics
    from ..utils.sysinfo import collect_system_info

    ex = config["execution"]
    if args.allreduce:
        ex["allreduce"] = args.allreduce
    if args.allreduce_dtype:
        ex["allreduce_dtype"] = args.allreduce_dtype
    if args.attention:
        ex["attention"] = args.attention
    if args.kernels:
        ex["kernels"] = args.kernels
    if args.gemm_dtype:
        ex["gemm_dtype"] = args.gemm_dtype
    if args.overlap_chunks:
        ex["overlap_chunks"] = args.overlap_chunks
    if args.model_size:
        config["model"].update(MODEL_CONFIGS[args.model_size])
        config["model"]["size"] = args.model_size
    if args.num_layers:
        config["model"]["num_layers"] = args.num_layers
    if args.warmup is not None:
        ex["warmup_iterations"] = args.warmup
    if args.iters is not None:
        ex["benchmark_iterations"] = args.iters
    if args.output_dir:
        config["experiment"]["output_dir"] = args.output_dir
    if args.decode is not None:
        if args.decode < 0:
            print("ERROR: --decode needs N >= 0")
            return 1
        ex["decode_tokens"] = args.decode
    n_dec = int(ex.get("decode_tokens", 0))
    if n_dec and ex.get("gemm_dtype", "bf16") == "fp8":
        # the FP8 GEMM's contract at M = batch rows is not established: refuse, never fall back
        if os.environ.get("RANK", "0") == "0":
            print("ERROR: --decode (execution.decode_tokens) is not supported with gemm_dtype "
                  "fp8: the FP8 GEMM is not specified for the M = batch_size rows of a decode "
                  "step")
        return 1
    if args.decode_weights:
        ex["decode_weight_dtype"] = args.decode_weights
    w8 = ex.get("decode_weight_dtype", "bf16") == "fp8"
    w4 = ex.get("decode_weight_dtype", "bf16") == "mxfp4"
    if args.kv_cache:
        ex["kv_cache_dtype"] = args.kv_cache
    kv8 = ex.get("kv_cache_dtype", "bf16") == "fp8"
    if kv8 and (not n_dec or ex.get("attention", "slice") == "slice"):
        # refused before any process group exists: nothing to quantise, never a silent bf16 run
        if os.environ.get("RANK", "0") == "0":
            print("ERROR: --kv-cache fp8 (execution.kv_cache_dtype) needs " +
                  ("decode tokens (--decode N): only the decode steps keep a KV cache"
                   if not n_dec else
                   "attention sdpa or flash: attention slice keeps no K / V to quantise"))
        return 1
    prompt = int(config["input"]["sequence_length"])
    if args.prompt_lens is not None:
        try:
            ex["prompt_lengths"] = [int(v) for v in args.prompt_lens.split(",")]
        except ValueError:
            print(f"ERROR: --prompt-lens takes integers L0,L1,..., got {args.prompt_lens!r}")
            return 1
    lens = ex.get("prompt_lengths")
    if lens is not None:
        # refused before any process group exists, like --kv-cache fp8
        nb = int(config["input"]["batch_size"])
        why = None
        if not n_dec:
            why = "decode tokens (--decode N): only the decode steps keep a KV cache"
        elif ex.get("attention", "slice") == "slice":
            why = "attention sdpa or flash: attention slice keeps no K / V"
        elif len(lens) != nb:
            why = f"one value per batch row: got {len(lens)} for batch_size {nb}"
        elif any(not 1 <= int(v) <= prompt for v in lens):
            why = f"values in [1, sequence_length {prompt}], got {lens}"
        if why:
            if os.environ.get("RANK", "0") == "0":
                print(f"ERROR: --prompt-lens (execution.prompt_lengths) needs {why}")
            return 1
        lens = [int(v) for v in lens]
    max_len = int(args.max_len) if args.max_len else prompt + n_dec
    if n_dec and max_len < prompt + n_dec:
        print(f"ERROR: --max-len {max_len} < sequence_length {prompt} + {n_dec} decoded tokens")
        return 1
    if args.kv_page_size is not None:
        ex["kv_page_size"] = args.kv_page_size
    if args.kv_pages is not None:
        ex["kv_pool_pages"] = args.kv_pages
    page, pool, row_tokens = ex.get("kv_page_size"), ex.get("kv_pool_pages"), None
    if page is not None or pool is not None:
        # refused before any process group exists, like --prompt-lens
        from ..utils.config import KV_PAGE_SIZES

        why = None
        if page is None:
            why = "--kv-pages (execution.kv_pool_pages) needs --kv-page-size P"
        elif not n_dec:
            why = ("--kv-page-size (execution.kv_page_size) needs decode tokens (--decode N): "
                   "only the decode steps keep a KV cache")
        elif ex.get("attention", "slice") == "slice":
            why = ("--kv-page-size (execution.kv_page_size) needs attention sdpa or flash: "
                   "attention slice keeps no K / V")
        elif page not in KV_PAGE_SIZES:
            why = (f"--kv-page-size (execution.kv_page_size) must be one of {KV_PAGE_SIZES}, "
                   f"got {page}")
        else:
            # positions every row ends at: what the pool has to hold
            row_tokens = [v + n_dec
                          for v in (lens or [prompt] * int(config["input"]["batch_size"]))]
            need = sum((v + page - 1) // page for v in row_tokens)
            if pool is None:
                pool = ex["kv_pool_pages"] = need
            elif pool < need:
                why = (f"--kv-pages (execution.kv_pool_pages) {pool} is too small: the rows "
                       f"need {need} pages of {page} positions")
        if why:
            if os.environ.get("RANK", "0") == "0":
                print(f"ERROR: {why}")
            return 1

    t0 = time.perf_counter()
    cpr = config["parallelism"].get("cores_per_rank")
    # host threads bound to the GPU's NUMA-local cores, cores_per_rank each (reference
    # launch_openmpi.sh:19-23 --bind-to core --map-by socket:PE=14)
    comm = init_distributed(args.backend,
                            device=None if args.device == "auto" else args.device,
                            cores_per_rank=int(cpr) if cpr else None)
    comm.install_tune_agreement()       # GEMM kernel choices agreed on rank-max timings
    comm.barrier()
    init_elapsed = time.perf_counter() - t0
    rank, world = comm.rank, comm.world_size

    expected = config["parallelism"]["world_size"]
    eff_world = args.shard_as or world
    if expected != "auto" and int(expected) != eff_world and not args.ignore_world_size:
        if rank == 0:
            print(f"ERROR: World size mismatch. Expected {expected}, got {eff_world}")
        comm.destroy()
        return 1
    if ex.get("gemm_dtype", "bf16") == "fp8":
        from ..utils.config import ConfigError, check_fp8_shapes

        try:                              # with the TP degree and model overrides now known
            check_fp8_shapes(config, eff_world)
        except ConfigError as e:
            if rank == 0:
                print(f"ERROR: {e}")
            comm.destroy()
            return 1
    if w8 or w4:
        from ..ops import _lib
        from ..utils.config import ConfigError, check_w4_shapes, check_w8_shapes

        wname, wkind, wgemm = ("fp8", "e4m3", "W8") if w8 else ("mxfp4", "MXFP4", "W4")
        hip = comm.is_gpu and ex.get("kernels", "hip") != "torch" and not _lib.force_torch()
        why = None
        if not n_dec:
            why = (f"--decode-weights {wname} (execution.decode_weight_dtype) needs decode "
                   f"tokens (--decode N): only the decode steps stream the {wkind} weights")
        elif hip and int(config["input"]["batch_size"]) > 16:
            why = (f"--decode-weights {wname}: batch_size {config['input']['batch_size']} is "
                   f"larger than the 16 rows of the {wgemm} skinny GEMM; there is no fall-back "
                   "to bf16")
        else:
            try:                          # with the TP degree and model overrides now known
                (check_w8_shapes if w8 else check_w4_shapes)(config, eff_world)
            except ConfigError as e:
                why = str(e)
        if why:
            if rank == 0:
                print(f"ERROR: {why}")
            comm.destroy()
            return 1
    model_comm = comm
    if args.shard_as:
        if world != 1 or args.shard_as < 2:
            if rank == 0:
                print("ERROR: --shard-as P needs world 1 and P >= 2")
            comm.destroy()
            return 1
        from ..parallel.comm import Comm

        # the model sees a P-rank world (shapes, per-rank FLOPs); no process group behind it
        model_comm = Comm(rank=0, world_size=args.shard_as, local_rank=comm.local_rank,
                          backend="emulate", device=comm.device)
        ex["allreduce"] = "emulate"

    if rank == 0:
        si = collect_system_info()
        print(f"\n{'=' * 60}\nExperiment: {config['experiment']['name']}\n"
              f"Backend: {args.backend.upper()} ({comm.backend})\n{'=' * 60}")
        print(f"World size: {world}\nInitialization time: {init_elapsed:.4f}s")
        print(f"Device: {si.get('gpu_name', 'cpu')} arch={si.get('gpu_arch')} "
              f"HIP={si.get('hip_version')} RCCL={si.get('rccl_version')}")
        m = config["model"]
        print(f"Model: {m.get('size')} H={m['hidden_size']} L={m['num_layers']} "
              f"heads={m['num_heads']} F={m['ffn_intermediate']}")
        print(f"Input: B={config['input']['batch_size']} S={config['input']['sequence_length']}")
        print(f"Execution: {ex}")

    model = create_model_from_config(config, model_comm)
    model.chunk_streams = bool(args.chunk_streams)
    if args.shard_as and args.emulate_busbw:
        from ..parallel.tensor_parallel import RowParallelLinear

        for m in model.modules():
            if isinstance(m, RowParallelLinear):
                m.emulate_busbw = float(args.emulate_busbw)
    dataset = create_dataset_from_config(config, comm.device)
    if rank == 0:
        print(f"[Rank 0] Model created: total params {model.get_num_parameters() / 1e9:.2f}B "
              f"(reference formula), {model.num_parameters_exact() / 1e9:.2f}B exact; "
              f"{model.get_memory_footprint() / 1e9:.2f} GB per rank")
    comm.barrier()

    metrics = MetricsCollector(rank, world)
    metrics.record_init_time(init_elapsed)
    gpu = comm.is_gpu

    # --decode: the forward fills a KV cache (emptied before every call) and N one-token steps
    # follow it; without it `forward` is the model itself, as before
    cache = (model.new_kv_cache(int(config["input"]["batch_size"]), max_len,
                                per_sequence=lens is not None, page_size=page, n_pages=pool)
             if n_dec else None)
    if cache is not None:
        # split grid of the decode kernel: final position (of the longest row)
        cache.len_bound = (max(lens) if lens else prompt) + n_dec
        if cache.paged:
            # every page the run will touch, mapped once: the table then never changes, so the
            # prefill and the decode step can be captured
            cache.reserve_all(row_tokens)

    def empty_cache():
        """Every row back to length 0; a paged cache keeps its pages (set_length(0) frees them)."""
        if cache.paged:
            cache.set_length(0, keep_pages=True)
        else:
            cache.set_length(0)

    def forward(x):
        if cache is None:
            return model(x)
        return model(x, kv_cache=cache, prompt_lens=lens)

    fwd_bytes = 0
    for _ in range(int(ex["warmup_iterations"])):
        batch = dataset.get_batch()
        b0 = model.comm_bytes()
        if cache is not None:
            empty_cache()
        t = time.perf_counter()
        forward(batch)
        comm.sync()
        metrics.record_warmup_time(time.perf_counter() - t)
        fwd_bytes = model.comm_bytes() - b0
    comm.barrier()

    dense_check = None
    if args.check_dense and not args.shard_as:
        dense_check = _check_against_dense(config, comm, model, dataset.get_batch())
        if rank == 0:
            print(f"dense check: {dense_check}")

    run_forward = lambda: forward(dataset.get_batch())  # noqa: E731
    # the timed loop replays a captured HIP graph wherever the forward is
    # capturable — the host issue cost of ~10 launches per layer (which made the eager TP
    # forward host-bound and GEMM tuning depend on the caller) is gone; --eager keeps the
    # reference's host-timed semantics
    use_graph = (not args.eager) and bool(ex.get("graph", True)) and gpu
    graph_note = None
    if use_graph and world > 1:
        # a layer whose all-reduce would go through ProcessGroup all_reduce (e.g.
        # allreduce=auto when the native engine could not be created on some rank) cannot be
        # captured; the decision is agreed, so every rank takes the same path
        if not all(comm.all_gather_object(_all_reduces_capturable(model))):
            graph_note = ("an all-reduce path is not capturable on some rank (no native engine "
                          "/ custom kernel)")
            use_graph = False
    if use_graph:
        # HIP graph: one replay launches the whole forward (all GEMM / LN / all-reduce kernels);
        # the autotuned GEMM choices were fixed by the eager warmup above. Any capture failure
        # on any rank -> every rank runs eagerly (agreed over the host side channel BEFORE the
        # first replay, so no rank replays collectives its peers never enqueue)
        static_in = dataset.get_batch()
        graph, err, static_out = None, None, None
        try:
            side = torch.cuda.Stream(comm.device)
            if cache is not None:
                empty_cache()
            side.wait_stream(torch.cuda.current_stream(comm.device))
            with torch.cuda.stream(side):
                forward(static_in)
            torch.cuda.current_stream(comm.device).wait_stream(side)
            comm.sync()
            if cache is not None:
                empty_cache()
                comm.sync()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                y_cap = forward(static_in)
                static_out = y_cap if cache is not None else None   # the decode loop's input
                del y_cap
        except Exception as e:  # noqa: BLE001 - agreed below, then eager
            err = f"{type(e).__name__}: {e}"[:500]
            graph = None
        torch.cuda.synchronize(comm.device)
        errs = _agree_host(comm, err)
        if errs:
            graph_note = f"capture failed on rank(s) {sorted(errs)}: {errs[min(errs)]}"
            use_graph = False
        else:
            graph.replay()
            comm.sync()
            if cache is None:
                run_forward = graph.replay
            else:
                def run_forward():
                    graph.replay()
                    return static_out
    if graph_note and rank == 0:
        print(f"note: HIP graph replay off, running eagerly: {graph_note}")

    dec = None
    if cache is not None:
        dec = _DecodeRunner(model, cache, comm, prompt, n_dec, dataset.get_batch(),
                            use_graph, ex, lens)
        if dec.graph_note and rank == 0:
            print(f"note: decode steps issued eagerly: {dec.graph_note}")

    from ..utils import tracing

    if args.trace:
        tracing.enable()
    prof = tracing.torch_profile(args.torch_profile, rank)
    prof.__enter__()
    ev = []
    for _ in range(int(ex["benchmark_iterations"])):
        comm.barrier()                          # reference run_mpi.py:177
        if cache is not None:
            empty_cache()
        if gpu:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
        t = time.perf_counter()
        with tracing.range("tp_forward"):
            y = run_forward()
        if gpu:
            e.record()
        comm.sync()
        comm.barrier()                          # reference run_mpi.py:183
        metrics.record_forward_time(time.perf_counter() - t)
        if gpu:
            ev.append(s.elapsed_time(e) * 1e-3)
        if dec is not None:
            with tracing.range("tp_decode"):
                dec.timed(y)
    prof.__exit__(None, None, None)
    car = getattr(model, "ipc_allreduce", lambda: None)()
    if car is not None:                 # a timed-out IPC all-reduce must not pass silently
        car.raise_if_error()
    calibration = car.calibration if car is not None else None
    ar_bytes = fwd_bytes
    if ev:
        metrics.metrics["forward_device_times"] = ev

    summary = metrics.get_summary()
    # next to forward_mean: the reference host-times EAGER forwards
    # (run_mpi.py:173-185); a graph-replayed forward is not the same quantity
    summary["timing_mode"] = "hip_graph_replay" if use_graph else "eager"
    means = comm.all_gather_object(summary["forward_mean"])
    affinity = comm.affinity_all_ranks()
    if rank == 0:
        rs = rank_statistics(means)
        B, S = int(config["input"]["batch_size"]), int(config["input"]["sequence_length"])
        fwd = summary["forward_mean"]
        extra = {
            "tokens_per_s": B * S / fwd,
            "tflops_per_rank": model.flops_per_forward(B, S) / fwd / 1e12,
            "allreduce_bytes_per_forward_per_rank": ar_bytes,
            "allreduces_per_forward": 2 * int(config["model"]["num_layers"]),
            "forward_device_mean": float(np.mean(ev)) if ev else None,
            "kernels": ex.get("kernels"),
            "gemm_dtype": ex.get("gemm_dtype", "bf16"),
            "hip_graph": use_graph,
            "hip_graph_note": graph_note,
            "timing_mode": "hip_graph_replay" if use_graph else "eager",
            "gemm_tune_timing": __import__(
                "distributed_llm_backend_benchmark_amd.ops.gemm", fromlist=["x"]).tune_timing(),
            "gemm_fallbacks": __import__(
                "distributed_llm_backend_benchmark_amd.ops.gemm", fromlist=["x"]).FALLBACKS["count"],
            "gemm_kernel_mix": __import__(
                "distributed_llm_backend_benchmark_amd.ops.gemm", fromlist=["x"]).kernel_mix(),
            # node-measured IPC-vs-RCCL crossovers behind allreduce=auto (None: RCCL only)
            "allreduce_calibration": calibration,
            "dense_check": dense_check,
            # micro-batches interleaved so all-reduces run under GEMMs (1 = blocking)
            # (a forward that fills a KV cache runs as one micro-batch)
            "overlap_chunks": 1 if cache is not None else model.overlap_split(
                torch.empty(B, 1, device="meta")),
            "chunk_streams": bool(args.chunk_streams),
        }
        if args.shard_as:
            extra["shard_as"] = {
                "P": args.shard_as, "emulate_busbw_GBps": args.emulate_busbw,
                "what": ("rank 0's shard of a P-way TP forward on ONE GPU: the exact per-rank "
                         "GEMM / LayerNorm shapes; each all-reduce replaced by a stand-in with "
                         "one rank's one-shot HBM traffic" +
                         (" plus the ring time at the assumed bus bandwidth"
                          if args.emulate_busbw else " (no link time)") +
                         "; tokens_per_s is the P-GPU job's (every rank holds all tokens)")}
        results = {
            "experiment": config["experiment"]["name"],
            "backend": args.backend,
            "config": config,
            "system_info": dict(collect_system_info(), host_affinity_per_rank=affinity),
            "rank_0_summary": summary,
            "rank_statistics": rs,
            "raw_metrics_rank_0": metrics.get_raw_metrics(),
            "throughput": extra,
        }
        if dec is not None:
            results["decode"] = dec.record()
        print_summary(summary, args.backend.upper(), rank)
        print(f"\nRank Statistics:\n  Variance across ranks: {rs['variance_across_ranks']:.6g}"
              f"\n  Coefficient of variation: {rs['coefficient_of_variation']:.4f}"
              f"\n  tokens/s: {extra['tokens_per_s']:.1f}  TFLOP/s/rank: "
              f"{extra['tflops_per_rank']:.1f}")
        suffix = f"_shard{args.shard_as}" if args.shard_as else ""
        if extra["overlap_chunks"] > 1:
            suffix += f"_ov{extra['overlap_chunks']}" + ("cs" if args.chunk_streams else "")
        if extra["gemm_dtype"] != "bf16":      # never overwrites the bf16 record
            suffix += f"_{extra['gemm_dtype']}"
        if dec is not None:                    # never overwrites the prefill record
            suffix += f"_decode{n_dec}" + ("_w8" if w8 else "_w4" if w4 else "") + \
                ("_kv8" if kv8 else "") + ("_ragged" if lens else "") + \
                (f"_paged{page}" if page else "")
            d = results["decode"]
            print(f"  decode: {d['ms_per_token_mean']:.4f} ms/token ({d['timing_mode']}, "
                  f"attention {d['attention_path']}), {d['decode_tokens_per_s']:.0f} tokens/s, "
                  f"{d['achieved_GBps']:.0f} GB/s of weights + KV" +
                  (f" ({d['weight_dtype']} weights, {d['w8_launches_per_step']} W8 launches "
                   "per step)" if w8 else "") +
                  (f" ({d['weight_dtype']} weights, {d['w4_launches_per_step']} W4 launches "
                   "per step)" if w4 else "") +
                  (f" ({d['kv_dtype']} KV cache)" if kv8 else ""))
        out = os.path.join(config["experiment"]["output_dir"],
                           f"{args.backend}_{config['experiment']['name']}{suffix}.json")
        save_results(results, out, rank)
    comm.barrier()
    comm.destroy()
    return 0


class _DecodeRunner:
    """The N one-token steps that follow the prefill of every timed iteration (``--decode N``).

    The model has no LM head: the input of step ``i + 1`` is the last-position output of step
    ``i`` (the final LayerNorm keeps the scale), copied into a static ``[B, 1, H]`` input on the
    device. Two eager steps at position ``prompt`` fix the GEMM autotuner's choices for the
    ``M = B`` shapes; then, where the forward was captured (``capturable``) and the attention
    reads the cache length from the device (our kernel, or the stateless stub), ONE step is
    captured at ``len_bound = prompt + N`` and replayed N times; otherwise the host issues the
    steps. The N steps are timed by one device-event pair and by the host clock after a sync.

    ``lens`` (``--prompt-lens``): the prompts are right-padded to ``prompt`` and the cache is a
    per-sequence one; row ``b`` starts at ``lens[b]`` and its first decode input is the output at
    its last real token."""

    def __init__(self, model, cache, comm, prompt: int, n: int, batch, capturable: bool, ex,
                 lens=None):
        import torch

        from ..ops import _lib, fp8, mxfp4
        from ..ops import decode as dec_ops

        self.model, self.cache, self.comm = model, cache, comm
        self.prompt, self.n, self.lens = prompt, n, lens
        # row b's last real token of a padded prefill output (None: the last position)
        self.last = (torch.tensor([v - 1 for v in lens], device=batch.device) if lens else None)
        self.rows = torch.arange(batch.shape[0], device=batch.device) if lens else None
        self.gpu = comm.is_gpu
        attention = ex.get("attention", "slice")
        heads = model.num_heads // model.world_size
        hd = model.hidden_size // model.num_heads
        if attention == "slice":
            self.attention_path = "slice"
        elif (attention == "flash" and ex.get("kernels", "hip") != "torch" and self.gpu
              and not _lib.force_torch() and hd in dec_ops.HEAD_DIMS):
            self.attention_path = "hip"
        else:
            self.attention_path = "torch"
        # bytes of one cached position: K + V rows of hd bf16, or of hd e4m3 codes + an fp32 scale
        row_bytes = hd + 4 if cache.kv_dtype == "fp8" else 2 * hd
        self.kv_per_key = cache.num_layers * cache.batch * heads * row_bytes * 2
        self.x = torch.empty(batch.shape[0], 1, batch.shape[2], dtype=batch.dtype,
                             device=batch.device)
        self.dev_ms, self.host_ms = [], []
        self.graph, self.graph_note = None, None

        # warm: a prefill, then two eager steps at the first decode position (a paged cache was
        # given all its pages by the caller: it is emptied without freeing them)
        if cache.paged:
            cache.set_length(0, keep_pages=True)
        else:
            cache.set_length(0)
        y = model(batch, kv_cache=cache, prompt_lens=lens)
        self.x.copy_(self._last_rows(y))
        b0, l0 = model.comm_bytes(), fp8.W8_LAUNCHES["count"]
        l4 = mxfp4.W4_LAUNCHES["count"]
        for _ in range(2):
            self._rewind()
            self.step()
        comm.sync()
        self.allreduce_bytes_per_step = (model.comm_bytes() - b0) // 2
        self.w8_launches_per_step = (fp8.W8_LAUNCHES["count"] - l0) // 2
        self.w4_launches_per_step = (mxfp4.W4_LAUNCHES["count"] - l4) // 2
        if not capturable:
            return
        if self.attention_path == "torch":
            # the torch form slices the cache by the HOST position: a replay would repeat one
            self.graph_note = "the torch decode attention is not replayable across positions"
            return
        graph, err = None, None
        try:
            side = torch.cuda.Stream(comm.device)
            self._rewind()
            side.wait_stream(torch.cuda.current_stream(comm.device))
            with torch.cuda.stream(side):
                self.step()
            torch.cuda.current_stream(comm.device).wait_stream(side)
            self._rewind()
            comm.sync()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                self.step()
        except Exception as e:  # noqa: BLE001 - agreed below, then eager
            err = f"{type(e).__name__}: {e}"[:500]
            graph = None
        torch.cuda.synchronize(comm.device)
        errs = _agree_host(comm, err)
        if errs:
            self.graph_note = f"capture failed on rank(s) {sorted(errs)}: {errs[min(errs)]}"
            return
        self._rewind()
        graph.replay()
        comm.sync()
        self.graph = graph

    def _rewind(self) -> None:
        """The cache as the prefill leaves it: every row at the prompt, or at its own length."""
        if self.lens:
            self.cache.set_lengths(self.lens)
        else:
            self.cache.set_length(self.prompt)

    def _last_rows(self, y):
        """``[B, 1, H]``: the prefill output at every row's last real token."""
        if self.last is None:
            return y[:, -1:]
        return y[self.rows, self.last][:, None]

    def step(self) -> None:
        y = self.model(self.x, kv_cache=self.cache)
        self.x.copy_(y)

    def timed(self, prefill_out) -> None:
        """N steps from the state the prefill left (cache length = prompt)."""
        import torch

        self.x.copy_(self._last_rows(prefill_out))
        # a replayed prefill advanced the device length only: bring the host mirror along
        self._rewind()
        run = self.graph.replay if self.graph is not None else self.step
        self.comm.sync()
        if self.gpu:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
        t = time.perf_counter()
        for _ in range(self.n):
            run()
        if self.gpu:
            e.record()
        self.comm.sync()
        self.host_ms.append((time.perf_counter() - t) * 1e3 / self.n)
        if self.gpu:
            self.dev_ms.append(s.elapsed_time(e) / self.n)

    def record(self) -> dict:
        import numpy as np

        from ..ops import gemm

        ms = self.dev_ms or self.host_ms
        mean = float(np.mean(ms))
        B = self.x.shape[0]
        # step i reads the K and V of positions [0, prompt + i] in every layer
        kv_mean = self.kv_per_key * (self.prompt + (self.n + 1) / 2.0)
        if self.lens:                           # each row from its own length: the sum over rows
            kv_mean = self.kv_per_key // B * sum(v + (self.n + 1) / 2.0 for v in self.lens)
        weights = self.model.get_memory_footprint()
        w8 = self.model.decode_weight_dtype == "fp8"
        w4 = self.model.decode_weight_dtype == "mxfp4"
        # == weights unless the steps stream e4m3 or MXFP4
        streamed = self.model.decode_weight_bytes()
        tuned = [t for t in gemm.kernel_mix()["linear"]["tuned"] if t["key"][0] == str(B)]
        by_choice = {}
        for t in tuned:
            by_choice[t["choice"]] = by_choice.get(t["choice"], 0) + 1
        rec = {
            "prompt_len": self.prompt, "new_tokens": self.n, "max_len": self.cache.max_len,
            # per timed iteration: (time of the N steps) / N; device events on the GPU
            "ms_per_token": [float(v) for v in ms],
            "ms_per_token_host": [float(v) for v in self.host_ms],
            "ms_per_token_mean": mean, "ms_per_token_p50": float(np.median(ms)),
            "decode_tokens_per_s": B / (mean * 1e-3),
            "kv_cache_bytes_per_rank": self.cache.nbytes,
            "kv_bytes_read_per_step_mean": kv_mean,
            "weight_bytes_per_rank": weights,
            # bytes a step must read from HBM on one rank — every weight once plus the mean K / V
            # read — over the mean step time; activations, partials and all-reduce traffic are
            # not counted
            "achieved_GBps": (streamed + kv_mean) / (mean * 1e-3) / 1e9,
            "allreduce_bytes_per_step": self.allreduce_bytes_per_step,
            "attention_path": self.attention_path,
            "timing_mode": "hip_graph_replay" if self.graph is not None else "eager",
            "hip_graph_note": self.graph_note,
            # the GEMM shapes of a decode step (M = batch rows) and what the autotuner runs there
            "gemm_kernel_mix": {"shapes_by_choice": by_choice, "tuned": tuned},
            "weight_dtype": self.model.decode_weight_dtype,
            "kv_dtype": self.cache.kv_dtype,
        }
        if self.lens:
            rec["prompt_lengths"] = list(self.lens)
        if self.cache.paged:
            # kv_cache_bytes_per_rank above is then the pools
            rec["kv_page_size"] = self.cache.page_size
            rec["kv_pool_pages"] = self.cache.n_pages
            rec["kv_pages_peak"] = self.cache.peak_pages_in_use
        if w8:
            # the e4m3 bytes and row scales of every linear (+ the LayerNorm parameters): what a
            # step streams; weight_bytes_per_rank stays the resident bf16 footprint
            rec["weight_stream_bytes_per_rank"] = streamed
            rec["w8_launches_per_step"] = self.w8_launches_per_step
        if w4:
            # the code and block-scale bytes of every linear (+ the LayerNorm parameters)
            rec["weight_stream_bytes_per_rank"] = streamed
            rec["w4_launches_per_step"] = self.w4_launches_per_step
        return rec


def _all_reduces_capturable(model) -> bool:
    """Every row-parallel layer's all-reduce can be captured in a HIP graph: our native RCCL
    engine exists on the layer, or it is forced to the IPC kernel (``allreduce=custom``);
    ``emulate`` is local work. Otherwise ``RowParallelLinear._all_reduce`` may fall through to
    ProcessGroup ``all_reduce``."""
    from ..parallel.tensor_parallel import RowParallelLinear

    for m in model.modules():
        if isinstance(m, RowParallelLinear):
            if m.allreduce == "emulate":
                continue
            if m._native is None and not (m.allreduce == "custom" and m._car is not None):
                return False
    return True


def _agree_host(comm, err):
    """Every rank's error string (None = ok), gathered over the host side channel (a failed
    capture may leave the device communicator unusable); returns {rank: error} of the failed."""
    import torch.distributed as dist

    if comm.world_size == 1:
        return {0: err} if err else {}
    out = [None] * comm.world_size
    dist.all_gather_object(out, err, group=comm.cpu_group())
    return {r: e for r, e in enumerate(out) if e}


def _check_against_dense(config, comm, model, batch) -> dict:
    """Build the dense (world-1) model of the same seed on every rank, shard its weights into
    the TP model (``LLM.load_from_dense``), run both on ``batch`` and compare: the TP forward,
    all-reduces included, must reproduce the dense output to bf16 accuracy (the test of
    ``run_mpi.py``'s model the reference never runs, models.py:95)."""
    import torch

    from ..models.tp_transformer import create_model_from_config
    from ..parallel.comm import Comm

    solo = Comm(rank=0, world_size=1, local_rank=comm.local_rank, backend=comm.backend,
                device=comm.device)
    dense = create_model_from_config(config, solo)
    with torch.no_grad():
        y_ref = dense(batch).float()
        model.load_from_dense(dense.state_dict())
        del dense
        y = model(batch).float()
    comm.sync()
    scale = float(y_ref.abs().max())
    err = float((y - y_ref).abs().max())
    errs = comm.all_gather_object(err)
    rel = max(errs) / max(scale, 1e-30)
    # fp8: the dense model quantises a row-parallel input with one scale per token, the TP model
    # with one per token and rank, so the two differ by e4m3 rounding (2^-4 per element) carried
    # through every layer, not by bf16 rounding. decode_weight_dtype=fp8 gets the same tolerance:
    # wherever it applies the weights carry the same e4m3 rounding (the forwards compared here
    # have no KV cache, so they run on the bf16 weights and sit far inside it).
    # decode_weight_dtype=mxfp4 keeps the bf16 tolerance of 5e-2 for that very reason: the
    # cache-less forwards compared here never touch the MXFP4 copy
    exe = config["execution"]
    fp8 = "fp8" in (exe.get("gemm_dtype", "bf16"), exe.get("decode_weight_dtype", "bf16"))
    tol = 0.25 if fp8 else 5e-2
    return {"max_abs_err": max(errs), "ref_max_abs": scale, "rel_err": rel, "tolerance": tol,
            "passed": bool(rel < tol and all(e == e for e in errs))}


if __name__ == "__main__":
    sys.exit(main())
