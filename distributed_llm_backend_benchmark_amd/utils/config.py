"""YAML experiment config with the reference schema.

Reference schema: ``config/baseline_config.yaml:1-34`` — sections ``experiment``, ``model``,
``parallelism``, ``input``, ``execution``, ``system``. Keys are read by the reference at
``run_mpi.py:73,82,100-110,154,172,237-238``, ``models.py:323-333``, ``data_gen.py:66-71``
and ``utils.py:163-169``.

Additions (all optional, defaults keep reference behaviour):

* ``parallelism.backend``: ``rccl`` | ``gloo`` | ``auto`` (process-group backend).
* ``parallelism.world_size: auto`` accepts whatever world the launcher created.
* ``parallelism.cores_per_rank`` is accepted and recorded; on GPU it is a no-op.
* ``execution.allreduce``: ``rccl`` (torch ProcessGroupNCCL) | ``native`` (our C++ RCCL engine
  on the compute stream) | ``custom`` (IPC xGMI kernel) | ``auto`` (custom below its crossover,
  native above) — the row-parallel all-reduce path.
* ``execution.allreduce_dtype``: ``bf16`` (on-device, default) | ``fp32`` (reference wire format,
  ``models.py:84``).
* ``execution.attention``: ``slice`` (reference stub ``models.py:162-167``) | ``sdpa`` (torch
  causal attention) | ``flash`` (our causal flash kernel; with decode, our decode kernel).
* ``execution.decode_tokens``: after the prefill forward, decode this many tokens one at a time
  over a KV cache (``run_tp --decode``); 0 (default) = the prefill forward alone.
* ``execution.kernels``: ``hip`` (hand-written gfx950 kernels) | ``torch``.
* ``execution.overlap_chunks``: micro-batches the TP forward interleaves so each row-parallel
  all-reduce runs under another micro-batch's GEMMs (1 = the reference's blocking order).
* ``execution.gemm_dtype``: ``bf16`` (default) | ``fp8`` — the TP linears quantise activations
  per token and weights per output row to e4m3 and run the FP8 GEMM (``ops.fp8``); needs the
  hidden and FFN widths of one rank's shard to be multiples of 128.
* ``execution.decode_weight_dtype``: ``bf16`` (default) | ``fp8`` | ``mxfp4`` — the one-token
  decode steps
  (``decode_tokens``) stream every linear's weight as e4m3 with one scale per output row through
  the weight-only FP8 skinny GEMM (bf16 activations; ``run_tp --decode-weights``); needs the
  hidden size and one rank's hidden and FFN widths to be multiples of 64, a batch of at most 16,
  and keeps both copies of the weights resident (+ 50 % weight memory). ``mxfp4`` streams e2m1
  codes with one e8m0 scale per 32 k through the weight-only MXFP4 skinny GEMM instead
  (``ops.mxfp4``): those widths must be multiples of 128, the batch at most 16, + 26.6 % weight
  memory. Neither with ``gemm_dtype: fp8``.
* ``execution.kv_cache_dtype``: ``bf16`` (default) | ``fp8`` — the KV cache of the decode steps
  holds e4m3 codes with one fp32 scale per cached row of ``head_dim`` values (``ops.decode``;
  ``run_tp --kv-cache``): ``head_dim + 4`` bytes per row instead of ``2 head_dim``. The appends
  quantise, a decode step attends to the quantised rows; the prefill attention is unchanged.
* ``execution.prompt_lengths``: absent (default: every prompt fills ``sequence_length``) | a list
  of ``batch_size`` ints in ``[1, sequence_length]`` — the batch is right-padded prompts of these
  lengths and the decode steps run over a per-sequence KV cache (``ops.decode``;
  ``run_tp --prompt-lens``). Needs ``decode_tokens`` and a real attention.
* ``execution.kv_page_size``: absent (default: contiguous caches) | one of 16, 32, 64, 128, 256 —
  the decode steps run over a PAGED KV cache of pages of this many positions, shared by the batch
  rows through a block table (``ops.decode``; ``run_tp --kv-page-size``). Needs ``decode_tokens``
  and a real attention.
* ``execution.kv_pool_pages``: absent (default: exactly the pages the run needs) | an int >= 1 —
  the pages of that pool, per layer (``run_tp --kv-pages``). Needs ``kv_page_size``.
"""

from __future__ import annotations

import copy
import os
from typing import Any, Dict

import yaml

DEFAULT_CONFIG: Dict[str, Any] = {
    "experiment": {"name": "baseline_7b_world4", "output_dir": "results"},
    "model": {
        "size": "7B",
        "hidden_size": 4096,
        "num_layers": 32,
        "num_heads": 32,
        "ffn_intermediate": 16384,
    },
    "parallelism": {"world_size": 4, "cores_per_rank": 14, "backend": "auto"},
    "input": {"batch_size": 8, "sequence_length": 512, "seed": 42},
    "execution": {
        "warmup_iterations": 5,
        "benchmark_iterations": 10,
        "allreduce": "auto",
        "allreduce_dtype": "bf16",
        "attention": "slice",
        "kernels": "hip",
        "overlap_chunks": 1,
        "gemm_dtype": "bf16",
        "decode_tokens": 0,
        "decode_weight_dtype": "bf16",
        "kv_cache_dtype": "bf16",
    },
    "system": {"omp_num_threads": 14, "mkl_num_threads": 14},
}

# page sizes of the paged KV cache (ops.decode.PAGE_SIZES; not imported: no torch here)
KV_PAGE_SIZES = (16, 32, 64, 128, 256)

REQUIRED_SECTIONS = ("experiment", "model", "parallelism", "input", "execution", "system")

_REQUIRED_KEYS = {
    "experiment": ("name", "output_dir"),
    "model": ("hidden_size", "num_layers", "num_heads", "ffn_intermediate"),
    "parallelism": ("world_size",),
    "input": ("batch_size", "sequence_length", "seed"),
    "execution": ("warmup_iterations", "benchmark_iterations"),
}


class ConfigError(ValueError):
    pass


def _merge(base: Dict[str, Any], over: Dict[str, Any]) -> Dict[str, Any]:
    out = copy.deepcopy(base)
    for k, v in (over or {}).items():
        if isinstance(v, dict) and isinstance(out.get(k), dict):
            out[k] = _merge(out[k], v)
        else:
            out[k] = v
    return out


def validate_config(config: Dict[str, Any]) -> Dict[str, Any]:
    """Check the reference-required keys; fill optional additions with defaults."""
    if not isinstance(config, dict):
        raise ConfigError("config must be a mapping")
    for sec in REQUIRED_SECTIONS[:-1]:
        if sec not in config:
            raise ConfigError(f"missing config section '{sec}'")
        for key in _REQUIRED_KEYS.get(sec, ()):
            if key not in config[sec]:
                raise ConfigError(f"missing config key '{sec}.{key}'")
    cfg = _merge({k: {} for k in REQUIRED_SECTIONS}, config)
    for sec in ("parallelism", "execution"):
        for k, v in DEFAULT_CONFIG[sec].items():
            cfg[sec].setdefault(k, v)
    cfg["model"].setdefault("size", "custom")
    ws = cfg["parallelism"]["world_size"]
    if ws != "auto" and (not isinstance(ws, int) or ws < 1):
        raise ConfigError(f"parallelism.world_size must be a positive int or 'auto', got {ws!r}")
    m = cfg["model"]
    for k in ("hidden_size", "num_layers", "num_heads", "ffn_intermediate"):
        if int(m[k]) <= 0:
            raise ConfigError(f"model.{k} must be positive")
    ex = cfg["execution"]
    if ex["allreduce"] not in ("auto", "rccl", "custom", "native", "torch", "emulate"):
        raise ConfigError("execution.allreduce must be auto|rccl|custom|native|torch, got "
                          f"{ex['allreduce']!r}")
    if ex["allreduce_dtype"] not in ("bf16", "fp32"):
        raise ConfigError("execution.allreduce_dtype must be bf16|fp32")
    if ex["attention"] not in ("slice", "sdpa", "flash"):
        raise ConfigError("execution.attention must be slice|sdpa|flash")
    if not isinstance(ex["decode_tokens"], int) or isinstance(ex["decode_tokens"], bool) \
            or ex["decode_tokens"] < 0:
        raise ConfigError("execution.decode_tokens must be an int >= 0")
    if ex["kernels"] not in ("hip", "torch"):
        raise ConfigError("execution.kernels must be hip|torch")
    if not isinstance(ex["overlap_chunks"], int) or ex["overlap_chunks"] < 1:
        raise ConfigError("execution.overlap_chunks must be a positive int")
    if ex["gemm_dtype"] not in ("bf16", "fp8"):
        raise ConfigError(f"execution.gemm_dtype must be bf16|fp8, got {ex['gemm_dtype']!r}")
    if ex["gemm_dtype"] == "fp8":
        check_fp8_shapes(cfg, ws if isinstance(ws, int) else 1)
    if ex["decode_weight_dtype"] not in ("bf16", "fp8", "mxfp4"):
        raise ConfigError("execution.decode_weight_dtype must be bf16|fp8|mxfp4, got "
                          f"{ex['decode_weight_dtype']!r}")
    if ex["decode_weight_dtype"] == "fp8":
        check_w8_shapes(cfg, ws if isinstance(ws, int) else 1)
    if ex["decode_weight_dtype"] == "mxfp4":
        check_w4_shapes(cfg, ws if isinstance(ws, int) else 1)
    if ex["kv_cache_dtype"] not in ("bf16", "fp8"):
        raise ConfigError("execution.kv_cache_dtype must be bf16|fp8, got "
                          f"{ex['kv_cache_dtype']!r}")
    lens = ex.get("prompt_lengths")             # no default: absent = every prompt is full
    if lens is not None:
        S, B = cfg["input"].get("sequence_length"), cfg["input"].get("batch_size")
        if not isinstance(lens, (list, tuple)) or not lens or any(
                not isinstance(v, int) or isinstance(v, bool) or v < 1 for v in lens):
            raise ConfigError("execution.prompt_lengths must be a list of ints >= 1")
        if isinstance(B, int) and len(lens) != B:
            raise ConfigError(f"execution.prompt_lengths has {len(lens)} values for batch_size "
                              f"{B}")
        if isinstance(S, int) and max(lens) > S:
            raise ConfigError(f"execution.prompt_lengths must lie in [1, sequence_length {S}]")
    page, pool = ex.get("kv_page_size"), ex.get("kv_pool_pages")   # no defaults: absent = contiguous
    if page is not None and (not isinstance(page, int) or isinstance(page, bool)
                             or page not in KV_PAGE_SIZES):
        raise ConfigError(f"execution.kv_page_size must be one of {KV_PAGE_SIZES}, got {page!r}")
    if pool is not None:
        if not isinstance(pool, int) or isinstance(pool, bool) or pool < 1:
            raise ConfigError(f"execution.kv_pool_pages must be an int >= 1, got {pool!r}")
        if page is None:
            raise ConfigError("execution.kv_pool_pages needs execution.kv_page_size")
    return cfg


def check_fp8_shapes(config: Dict[str, Any], world: int) -> None:
    """The FP8 GEMM reduces over K-tiles of 128: the hidden size and the per-rank shard widths
    ``hidden_size / world`` and ``ffn_intermediate / world`` (the row-parallel reductions, also
    the column-parallel output widths) must be multiples of 128. ``world`` is the tensor-parallel
    degree the model is cut for (``run_tp --shard-as`` passes its own)."""
    m = config["model"]
    for key in ("hidden_size", "ffn_intermediate"):
        width = int(m[key])
        if width % world or (width // world) % 128:
            raise ConfigError(f"execution.gemm_dtype=fp8 needs model.{key} / {world} ranks to be "
                              f"a multiple of 128, got {width} / {world}")


def check_w8_shapes(config: Dict[str, Any], world: int) -> None:
    """The weight-only FP8 skinny GEMM of the decode steps reduces over units of 64 and writes
    tiles of 16 output columns: the hidden size (the column-parallel reductions) and the per-rank
    shard widths ``hidden_size / world`` and ``ffn_intermediate / world`` (the row-parallel
    reductions) must be multiples of 64. Every per-rank output width (``3 hidden_size / world``,
    ``ffn_intermediate / world``, ``hidden_size``) is then a multiple of 16 as well. ``world`` as
    in :func:`check_fp8_shapes`."""
    m = config["model"]
    hidden, ffn = int(m["hidden_size"]), int(m["ffn_intermediate"])
    if hidden % 64:
        raise ConfigError("execution.decode_weight_dtype=fp8 needs model.hidden_size to be a "
                          f"multiple of 64, got {hidden}")
    for key, width in (("hidden_size", hidden), ("ffn_intermediate", ffn)):
        if width % world or (width // world) % 64:
            raise ConfigError(f"execution.decode_weight_dtype=fp8 needs model.{key} / {world} "
                              f"ranks to be a multiple of 64, got {width} / {world}")


def check_w4_shapes(config: Dict[str, Any], world: int) -> None:
    """The weight-only MXFP4 skinny GEMM of the decode steps reduces over units of 128 (four MX
    blocks) and writes tiles of 16 output columns: the hidden size and the per-rank shard widths
    ``hidden_size / world`` and ``ffn_intermediate / world`` must be multiples of 128; every
    per-rank output width is then a multiple of 16 as well. ``world`` as in
    :func:`check_fp8_shapes`."""
    m = config["model"]
    hidden, ffn = int(m["hidden_size"]), int(m["ffn_intermediate"])
    if hidden % 128:
        raise ConfigError("execution.decode_weight_dtype=mxfp4 needs model.hidden_size to be a "
                          f"multiple of 128, got {hidden}")
    for key, width in (("hidden_size", hidden), ("ffn_intermediate", ffn)):
        if width % world or (width // world) % 128:
            raise ConfigError(f"execution.decode_weight_dtype=mxfp4 needs model.{key} / {world} "
                              f"ranks to be a multiple of 128, got {width} / {world}")


def load_config(config_path: str) -> Dict[str, Any]:
    """``yaml.safe_load`` + schema validation (reference ``utils.py:90-102``)."""
    with open(config_path, "r") as f:
        raw = yaml.safe_load(f)
    return validate_config(raw)


def setup_environment(config: Dict[str, Any]) -> None:
    """Export OMP/MKL thread counts (reference ``utils.py:154-169``).

    The reference sets these *after* ``import torch``, which is too late
    for the OpenMP runtime; our CLIs call this before importing torch.
    """
    sysc = config.get("system", {}) or {}
    if "omp_num_threads" in sysc:
        os.environ["OMP_NUM_THREADS"] = str(sysc["omp_num_threads"])
    if "mkl_num_threads" in sysc:
        os.environ["MKL_NUM_THREADS"] = str(sysc["mkl_num_threads"])
