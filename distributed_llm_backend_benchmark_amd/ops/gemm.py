"""MFMA bf16 GEMM with fused epilogues (``csrc/gemm.hip``).

``linear(x, w, bias, act, residual, out_dtype)`` computes ``act(x @ w.T + bias) + residual``
with ``w`` stored ``[out_features, in_features]`` (K-contiguous, the MFMA-native layout).
Reference call sites: ``models.py:47`` (column-parallel) and ``models.py:81`` (row-parallel).

Dispatch: see :func:`linear` (per-shape autotune between the fused MFMA kernel and hipBLASLt +
HIP epilogue). Shape contract of the HIP kernel: ``K % 64 == 0``, 16-byte aligned rows; M and N arbitrary.
Shapes outside the contract are routed to ``torch.matmul`` (hipBLASLt) — a plain library GEMM —
and counted in :data:`FALLBACKS` so benchmarks can report it. At M <= 16 (a decode step) the
skinny-M weight-streaming kernel (``csrc/gemm_skinny.hip``) is one more autotune candidate.
"""

from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, use_hip

EPI_BIAS, EPI_GELU_ERF, EPI_GELU_TANH, EPI_RESIDUAL = 1, 2, 4, 8
EPI_DGELU = {"gelu": 16, "gelu_erf": 16, "gelu_tanh": 32}   # dgrad epilogue: * act'(u)
ACTS = {None: 0, "none": 0, "gelu": EPI_GELU_ERF, "gelu_erf": EPI_GELU_ERF,
        "gelu_tanh": EPI_GELU_TANH}

FALLBACKS = {"count": 0}
TUNE_LOG = []         # (kind, key, {impl: median ms}, choice) per autotuned shape


# Collective autotuning: with ranks > 1 every decision must be the same on every rank (TP ranks
# running different kernels for one shape are rank-imbalanced, and the step waits for the
# slowest). ``set_tune_agreement(fn)`` installs ``fn(names, times) -> times``, the element-wise
# MAX of each candidate's time over all ranks (a host side channel,
# ``parallel.comm.Comm.agree_max``); every rank then takes the argmin of the same numbers.
_AGREE = None


def set_tune_agreement(fn) -> None:
    """Install (or with None remove) the cross-rank agreement of autotune timings."""
    global _AGREE
    _AGREE = fn


# env knobs that change which candidates exist or how they run: part of every agreed name, so
# ranks started with different settings fail at the first tuned shape instead of "agreeing" on
# timings of different kernels
_AGREED_ENV = ("DLBB_GEMM", "DLBB_TUNE_TIMING", "DLBB_WGRAD_STREAM")


def _agree_names(kind: str, key, names) -> list:
    """The names every rank must pass identically to the agreement: tuning kind + shape key +
    env signature + candidate, so a shape / call-order / configuration mismatch between ranks
    raises on every rank (``Comm.agree_max``) rather than mixing timings of different GEMMs."""
    env = ",".join(f"{k}={os.environ.get(k, '')}" for k in _AGREED_ENV)
    head = f"{kind}|{'/'.join(str(k) for k in key)}|{env}|{tune_timing()}"
    return [f"{head}|{n}" for n in names]


def library_margin() -> float:
    """Fraction by which the library GEMM (``blas``) must beat the fastest hand-written candidate
    to be chosen (``DLBB_LIB_MARGIN``, default 0.05). The autotuners time device work only; a
    hipBLASLt call also pays ~15 us of host-side setup per call (round-3 measurement, invisible
    to device-time tuning but exposed whenever the host is the bottleneck, e.g. the eager TP
    forward), is a persistent Stream-K grid that stalls beside comm kernels, and keeps the
    kernel mix off our own code. Inside the margin the hand-written kernel runs: at the GPT-2
    LM-head forward (ours 2.8-3.3 % behind by box) that costs ~0.03 ms per step; the A/B against
    ``DLBB_LIB_MARGIN=0`` is recorded in profiles/r04_final. 0 = pure fastest-wins."""
    try:
        return max(0.0, float(os.environ.get("DLBB_LIB_MARGIN", "0.05")))
    except ValueError:
        return 0.05


def _choose(times: dict, kind: str = "", key=()):
    """(best candidate, the timings it was chosen on): rank-max timings when an agreement is
    installed, first-listed candidate on ties; the library candidate only beyond
    :func:`library_margin` of the fastest hand-written one."""
    names = list(times)
    vals = [float(times[n]) for n in names]
    if _AGREE is not None:
        vals = [float(v) for v in _AGREE(_agree_names(kind, key, names), vals)]
    agreed = {n: round(v, 4) for n, v in zip(names, vals)}
    best = min(names, key=lambda n: (agreed[n], names.index(n)))
    ours = [n for n in names if n != "blas"]
    if best == "blas" and ours:
        mine = min(ours, key=lambda n: (agreed[n], names.index(n)))
        if agreed[mine] <= agreed["blas"] * (1.0 + library_margin()):
            best = mine
    return best, agreed


def _log_tune(kind, key, times, best) -> None:
    TUNE_LOG.append((kind, key, times, best))
    if os.environ.get("DLBB_TUNE_LOG") == "1":
        import sys

        print(f"[tune] {kind} {key} {times} -> {best}", file=sys.stderr, flush=True)


_TUNE_TIMING = [None]    # None: DLBB_TUNE_TIMING or "interleaved"; set_tune_timing overrides


def set_tune_timing(mode: str) -> None:
    """How the autotuners time candidates — ONE methodology for every caller (VERDICT r03
    item 7): ``"interleaved"`` (default), the best of interleaved rounds of 3 back-to-back calls,
    i.e. device time with host issue hidden behind the previous call — what a GPU-bound
    training step and a HIP-graph-replayed forward (``cli.run_tp``'s default timed loop) pay.
    ``"single"`` (median of event-bracketed single calls, host issue cost inside the span) is
    kept for A/B only: it favoured our kernels in the eager, host-bound TP forward, a symptom
    graph replay removes (``profiles/r03_lean/tune_ab``)."""
    if mode not in ("single", "interleaved"):
        raise ValueError(mode)
    _TUNE_TIMING[0] = mode


def tune_timing() -> str:
    """The autotune timing mode in effect (recorded in result JSONs)."""
    return _TUNE_TIMING[0] or os.environ.get("DLBB_TUNE_TIMING", "interleaved")


def _time_interleaved(cands: dict, rounds: int = 4, reps: int = 3) -> dict:
    """Per candidate ``name -> fn()``: ms per call under the selected timing (set_tune_timing).
    Interleaved: the best of ``rounds`` rounds of ``reps`` back-to-back calls (one warm-up call
    before each), candidates alternating within every round so clock / thermal drift hits them
    alike. Single: 2 warm-up calls, then the median of 5 event-bracketed single calls."""
    mode = tune_timing()
    if mode == "single":
        out = {}
        for name, fn in cands.items():
            for _ in range(2):
                fn()
            ts = []
            for _ in range(5):
                s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s0.record()
                fn()
                e0.record()
                e0.synchronize()
                ts.append(s0.elapsed_time(e0))
            out[name] = sorted(ts)[len(ts) // 2]
        return out
    best = {n: float("inf") for n in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            fn()
            s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            for _ in range(reps):
                fn()
            e0.record()
            e0.synchronize()
            best[name] = min(best[name], s0.elapsed_time(e0) / reps)
    return best


def set_tile(tile: int) -> None:
    """Force the 128^2 or 256^2 MFMA kernel (0 = size heuristic); for A/B benchmarking."""
    _lib.lib().dlbb_gemm_set_tile(int(tile))


def set_stagger(mode: int) -> None:
    """256^2 NT schedule: 6 = the ping-pong (default; upgraded to its persistent form on
    multi-round grids with a lean epilogue), 10 = the persistent ping-pong wherever its contract
    holds, 3 = the deep-pipeline kernel (the general-contract fallback) forced. The balanced DMA
    issue of the ping-pong is :func:`set_bal`. Other round-1..5 schedules were removed in round 6
    (never the fastest; profiles/r0*_gemm)."""
    _lib.lib().dlbb_gemm_set_stagger(int(mode))


def set_bal(mode: int) -> None:
    """Balanced LDS-DMA issue of the ping-pong kernels (NT forward and NN dgrad): 0 never,
    1 always, 2 = always for NN and for NT when
    K >= 2048 (default, measured: profiles/r02_gemm)."""
    _lib.lib().dlbb_gemm_set_bal(int(mode))


def set_persist_epi(on: bool) -> None:
    """Persistent forms with lean epilogues on multi-round short-K grids: NT bias / bias-GELU
    (+ pre-activation) and NN plain / GELU backward (default on; ``set_persist_epi(False)``
    keeps them on the non-persistent ping-pong; the NT plain form is picked by the autotuner)."""
    _lib.lib().dlbb_gemm_set_persist_epi(int(bool(on)))


def set_wgrad_stages(nb: int) -> None:
    """LDS ring depth of the weight-gradient kernel (2, 3 or 4 stages); for A/B benchmarking."""
    _lib.lib().dlbb_gemm_wgrad_set_stages(int(nb))


def get_stagger() -> int:
    return int(_lib.lib().dlbb_gemm_get_stagger())


def hip_supported(x2: torch.Tensor, w: torch.Tensor) -> bool:
    K = x2.shape[1]
    return (x2.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and K % 64 == 0
            and x2.stride(1) == 1 and w.stride(1) == 1 and x2.stride(0) % 8 == 0
            and w.stride(0) % 8 == 0 and x2.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0)


def _torch_linear(x2, w, bias, act, residual, out_dtype, preact):
    y = torch.matmul(x2.float(), w.float().t()) if x2.device.type == "cpu" else x2 @ w.t()
    y = y.float()
    if bias is not None:
        y = y + bias.float()
    if preact is not None:
        preact.copy_(y.to(preact.dtype))
    if act in ("gelu", "gelu_erf"):
        y = F.gelu(y)
    elif act == "gelu_tanh":
        y = F.gelu(y, approximate="tanh")
    if residual is not None:
        y = y + residual.reshape(y.shape).float()
    return y.to(out_dtype)


def _epi_flags(act, bias, r2) -> int:
    """The C entry points' ``epi`` of ``act(. + bias) + r2``."""
    return (ACTS[act] | (EPI_BIAS if bias is not None else 0)
            | (EPI_RESIDUAL if r2 is not None else 0))


def _mfma_linear(x2, w, bias, act, r2, out, preact, variant: int = 0):
    M, K = x2.shape
    N = w.shape[0]
    epi = _epi_flags(act, bias, r2)
    check(_lib.lib().dlbb_gemm_bf16_nt_v(
        x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), N, M, N, K,
        _lib.ptr(bias), _lib.ptr(r2), r2.stride(0) if r2 is not None else 0,
        _lib.ptr(preact), epi, 1 if out.dtype == torch.float32 else 0, int(variant),
        _lib.stream(x2.device)), "gemm_bf16_nt")
    return out


def _mfma192_linear(x2, w, bias, act, r2, out, preact):
    """256 x 192 output tiles (``csrc/gemm.hip`` ``gemm_bf16_nt_192_pingpong3``): for N % 192 ==
    0 grids whose 256² form ends in a partial round of the CUs (GPT-2 projections N = 768:
    0.75 round -> one full round)."""
    return _mfma_linear(x2, w, bias, act, r2, out, preact, variant=1)


def mfma192_ok(M: int, N: int) -> bool:
    return N % 192 == 0 and M % 8 == 0 and M >= 8


def _mfma192p_linear(x2, w, bias, act, r2, out, preact):
    """Persistent 256 x 192 tiles with the C stores spread under the next tile's K-loop
    (``csrc/gemm.hip`` ``pp192_spread_body``): plain bf16 output on multi-round grids — the GPT-2
    LM-head forward 16384 x 50304 x 768, whose 1.65 GB of logits otherwise drain serially at every
    tile boundary. Outside its contract the library runs variant 1."""
    return _mfma_linear(x2, w, bias, act, r2, out, preact, variant=2)


def mfma192p_ok(M: int, N: int, K: int, plain: bool) -> bool:
    return plain and N % 192 == 0 and M % 16 == 0 and M >= 16 and K // 64 >= 6


_NCU = {}


def _dev_index(device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def _num_cus(device) -> int:
    idx = _dev_index(device)
    if idx not in _NCU:
        _NCU[idx] = torch.cuda.get_device_properties(idx).multi_processor_count
    return _NCU[idx]


def streamk_plan(M: int, N: int, K: int, ncu: int):
    """(grid, L, ws bytes, counters) of the Stream-K NT GEMM (``csrc/gemm.hip``
    ``dlbb_gemm_streamk_plan``) or None outside its contract: 256² tiles below one round of the
    CUs (the 7B TP shard projections: 4096 x 1536 x 4096 = 96 tiles -> 256 workgroups of 24
    K-tiles each), >= 8 K-tiles per tile."""
    out = (ctypes.c_int64 * 4)()
    if not _lib.lib().dlbb_gemm_streamk_plan(M, N, K, ncu, out):
        return None
    return tuple(int(v) for v in out)


def _stream_buffers(cache: dict, device: torch.device, *specs) -> tuple:
    """The buffers of ``cache`` private to (device, current stream), one per spec ``(elements,
    dtype, floor, zero)``: launches on one stream are ordered, so one set serves every call on
    it. A buffer is grown on demand (to at least ``floor`` elements, never shrunk), with no
    per-call allocation or memset. ``zero``: zero-filled when allocated — arrival counters,
    which every launch leaves zero again; partial workspaces stay uninitialised."""
    key = (_dev_index(device), _lib.stream(device))
    bufs = list(cache.get(key, (None,) * len(specs)))
    for i, (n, dtype, floor, zero) in enumerate(specs):
        if bufs[i] is None or bufs[i].numel() < n:
            bufs[i] = (torch.zeros if zero else torch.empty)(max(n, floor), dtype=dtype,
                                                             device=device)
    cache[key] = tuple(bufs)
    return cache[key]


_SK_WS = {}      # (device index, stream handle) -> (fp32 partial workspace, int32 counters)


def _streamk_buffers(device: torch.device, ws_bytes: int, ncnt: int):
    """Partial-block workspace and (tile, wave) arrival counters of the Stream-K GEMM."""
    return _stream_buffers(_SK_WS, device, (-(-ws_bytes // 4), torch.float32, 1 << 20, False),
                           (ncnt, torch.int32, 4096, True))


def _mfma_streamk_linear(x2, w, bias, act, r2, out, preact):
    """Stream-K NT ping-pong (``csrc/gemm.hip`` ``pp_streamk_body``): every CU gets an equal
    contiguous range of the output tiles' K-loops; tiles split between ranges are combined in
    the launch by the last-arriving wave. Outside its contract: the default ping-pong."""
    M, K = x2.shape
    N = w.shape[0]
    ncu = _num_cus(x2.device)
    plan = streamk_plan(M, N, K, ncu)
    if plan is None:
        return _mfma_linear(x2, w, bias, act, r2, out, preact)
    epi = _epi_flags(act, bias, r2)
    ws, cnt = _streamk_buffers(x2.device, plan[2], plan[3])
    check(_lib.lib().dlbb_gemm_bf16_nt_streamk(
        x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0),
        M, N, K, _lib.ptr(bias), _lib.ptr(r2), r2.stride(0) if r2 is not None else 0,
        _lib.ptr(preact), epi, 1 if out.dtype == torch.float32 else 0, ncu, ws.data_ptr(),
        ws.numel() * 4, cnt.data_ptr(), cnt.numel(), _lib.stream(x2.device)),
        "gemm_bf16_nt_streamk")
    return out


def split_plan(M: int, N: int, K: int, ncu: int):
    """(split, tile192) of the split-K NT GEMM (``dlbb_gemm_bf16_nt_split``) or None: grids
    below one round of the CUs, the smallest split (2-4) that fills a round with >= 8 K-tiles
    per slice (else the deepest such split). 256 x 192 tiles when N % 192 == 0."""
    if M % 8 or M < 8 or N % 64 or K % 64:
        return None
    t192 = N % 192 == 0
    tiles = -(-M // 256) * (N // 192 if t192 else -(-N // 256))
    if tiles >= ncu:
        return None
    nkt = K // 64
    for split in (2, 3, 4):
        if tiles * split >= ncu and nkt // split >= 8:
            return split, int(t192)
    split = min(4, nkt // 8)             # no split fills a round: the deepest allowed
    return (split, int(t192)) if split >= 2 else None


_SPLIT_WS = {}   # (device index, stream handle) -> fp32 partial workspace (stream-private)


def _mfma_split_linear(x2, w, bias, act, r2, out, preact):
    """Split-K NT ping-pong + one reduce / cast pass (``csrc/gemm.hip``
    ``dlbb_gemm_bf16_nt_split``): plain bf16 products on grids below one round of the CUs (the
    TP-7B shard projections). The fp32 partial workspace is private to the current stream.
    Outside its contract: the default ping-pong."""
    M, K = x2.shape
    N = w.shape[0]
    plan = split_plan(M, N, K, _num_cus(x2.device))
    if plan is None or bias is not None or act is not None or r2 is not None or \
            preact is not None or out.dtype != torch.bfloat16:   # outside: the default ping-pong
        return _mfma_linear(x2, w, bias, act, r2, out, preact)
    split, t192 = plan
    ws, = _stream_buffers(_SPLIT_WS, x2.device, (split * M * N, torch.float32, 0, False))
    check(_lib.lib().dlbb_gemm_bf16_nt_split(
        x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), N, M, N, K,
        split, t192, ws.data_ptr(), ws.numel() * 4, _lib.stream(x2.device)),
        "gemm_bf16_nt_split")
    return out


SKINNY_LAUNCHES = {"count": 0}    # launches of the skinny-M kernel (never its fallback)


_SKINNY_PLANS = {}


def skinny_plan(M: int, N: int, K: int, ncu: int):
    """(grid, K-split inside a workgroup, K-split across workgroups, workspace bytes) of the
    skinny-M weight-streaming GEMM (``csrc/gemm_skinny.hip`` ``dlbb_gemm_skinny_plan``) or None
    outside its contract: 1 <= M <= 16, N % 16 == 0, K % 64 == 0."""
    key = (int(M), int(N), int(K), int(ncu))
    if key not in _SKINNY_PLANS:
        out = (ctypes.c_int64 * 4)()
        ok = _lib.lib().dlbb_gemm_skinny_plan(*key, out)
        _SKINNY_PLANS[key] = tuple(int(v) for v in out) if ok else None
    return _SKINNY_PLANS[key]


def skinny_ok(x2: torch.Tensor, w: torch.Tensor, out: torch.Tensor, preact=None) -> bool:
    """Host contract of the skinny-M candidate (checked again in C) and a valid plan: bf16
    K-contiguous operands with 16-byte aligned rows, contiguous bf16 / fp32 output, no
    pre-activation output (training only)."""
    if preact is not None or x2.dim() != 2 or w.dim() != 2:
        return False
    M, K = x2.shape
    N = w.shape[0]
    if not (1 <= M <= 16) or N % 16 or K % 64 or K <= 0 or w.shape[1] != K:
        return False
    if not hip_supported(x2, w):
        return False
    if (out.dtype not in (torch.bfloat16, torch.float32) or not out.is_contiguous()
            or tuple(out.shape) != (M, N) or out.data_ptr() % 16):
        return False
    ncu = _num_cus(x2.device) if x2.is_cuda else 256
    return skinny_plan(M, N, K, ncu) is not None


_HIP_INVALID_VALUE = 1


def _mfma_skinny_linear(x2, w, bias, act, r2, out, preact):
    """Skinny-M weight-streaming GEMM (``csrc/gemm_skinny.hip``): the decode step's linears,
    M = batch rows <= 16. W goes straight from global memory to the MFMA operands, K split
    over the waves of a workgroup and summed in a fixed order; no workspace. Outside its
    contract: the default ping-pong (the library where that one's contract fails too).

    A decode step is a chain of ~10 us launches, so the host path is kept short: only what C
    cannot see (dtypes, unit strides, contiguity) is checked here; shape, leading dimensions
    and alignment are checked by the C entry point, which launches nothing and returns
    hipErrorInvalidValue outside the contract (:func:`skinny_ok` is the same contract for
    callers that only ask)."""
    M = x2.shape[0]
    bf16 = torch.bfloat16
    if (preact is None and 1 <= M <= 16 and x2.dtype == bf16 and w.dtype == bf16
            and (out.dtype == bf16 or out.dtype == torch.float32)
            and x2.stride(1) == 1 and w.stride(1) == 1 and w.shape[1] == x2.shape[1]
            and out.is_contiguous()
            and (bias is None or (bias.dtype == bf16 and bias.is_contiguous()))
            and (r2 is None or (r2.dtype == bf16 and r2.stride(1) == 1))):
        epi = _epi_flags(act, bias, r2)
        dev = x2.device
        rc = _lib.lib().dlbb_gemm_bf16_nt_skinny(
            x2.data_ptr(), x2.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), M,
            w.shape[0], x2.shape[1], _lib.ptr(bias), _lib.ptr(r2),
            r2.stride(0) if r2 is not None else 0, epi, 1 if out.dtype == torch.float32 else 0,
            _num_cus(dev), _lib.stream(dev))
        if rc == 0:
            SKINNY_LAUNCHES["count"] += 1
            return out
        if rc != _HIP_INVALID_VALUE:
            check(rc, "gemm_bf16_nt_skinny")
    if hip_supported(x2, w):
        return _mfma_linear(x2, w, bias, act, r2, out, preact)
    # outside every hand-written contract (K % 64, alignment): the library, as `linear`
    return _blas_linear(x2 if x2.stride(1) == 1 else x2.contiguous(), w.contiguous(), bias,
                        act, r2, out, preact)


def streamk_ok(x2: torch.Tensor, w: torch.Tensor) -> bool:
    """Host contract of the Stream-K candidate (checked again in C) and a valid plan."""
    M, K = x2.shape
    N = w.shape[0]
    if N % 64 or M % 8 or M < 8:
        return False
    if (x2.stride(0) * 512 + K * 2) >= 2 ** 31 or (w.stride(0) * 512 + K * 2) >= 2 ** 31:
        return False
    return streamk_plan(M, N, K, _num_cus(x2.device)) is not None


_APPROX = {"gelu": 0, "gelu_erf": 0, "gelu_tanh": 1}


def _blas_linear(x2, w, bias, act, r2, out, preact):
    """hipBLASLt GEMM (bias fused by its epilogue through ``addmm``) followed by our HIP
    elementwise epilogue kernels (GELU, cast) — the plain-library-GEMM path."""
    M, N = x2.shape[0], w.shape[0]
    if act is not None or out.dtype != torch.bfloat16 or r2 is not None:
        u = preact if preact is not None else torch.empty(M, N, dtype=torch.bfloat16,
                                                          device=x2.device)
    else:
        u = out
    if bias is not None:
        torch.addmm(bias, x2, w.t(), out=u)
    else:
        torch.mm(x2, w.t(), out=u)
    if preact is not None and u is not preact:
        preact.copy_(u)
    y = u
    if act is not None:
        y = out if (out.dtype == torch.bfloat16 and r2 is None) else torch.empty_like(u)
        check(_lib.lib().dlbb_bias_gelu_fwd(u.data_ptr(), None, y.data_ptr(), M, N,
                                            _APPROX[act], _lib.stream(x2.device)), "bias_gelu")
    if r2 is not None:
        y = y + r2
    if y is not out:
        if out.dtype == y.dtype:
            out.copy_(y)
        else:
            check(_lib.lib().dlbb_cast(y.data_ptr(), _lib.dt(y), out.data_ptr(), _lib.dt(out),
                                       y.numel(), _lib.stream(x2.device)), "cast")
    return out


CHOICES = {}          # (M, N, K, epi-signature) -> "mfma" | "mfma192" | "mfma_skinny" | ... | "blas"
CALLS = {}            # ("linear" | "wgrad", key) -> calls since import (kernel-mix accounting)
_IMPLS = {"mfma": _mfma_linear, "mfma192": _mfma192_linear, "mfma192p": _mfma192p_linear,
          "mfma_sk": _mfma_streamk_linear, "mfma_split": _mfma_split_linear,
          "mfma_skinny": _mfma_skinny_linear, "blas": _blas_linear}


# > 0 while GEMMs share the chip with communication kernels on another stream (the overlapped
# TP forward). hipBLASLt's bf16 kernels here are persistent Stream-K grids (one workgroup per CU,
# all assumed co-resident): with comm workgroups holding CUs, part of the grid waits for a
# second round and the GEMM takes up to twice as long — measured: 7B shard-8 overlapped forward
# 27.8 ms with one such GEMM vs 17.4 ms on non-persistent grids. Shapes tuned in this state get
# their own keys (suffix "concurrent") and only the hand-written candidates, and our own
# persistent forms (NT bias / bias-GELU, NN plain / dGELU: grid = num_cus) are switched off in
# the library for the duration (dlbb_gemm_set_concurrent) — the same hazard.
_CONCURRENT = [0]


class concurrent_comm:
    """Context: GEMMs issued inside run beside comm kernels (see ``_CONCURRENT``)."""

    def __enter__(self):
        _CONCURRENT[0] += 1
        if _CONCURRENT[0] == 1 and _lib.available():
            _lib.lib().dlbb_gemm_set_concurrent(1)
        return self

    def __exit__(self, *exc):
        _CONCURRENT[0] -= 1
        if _CONCURRENT[0] == 0 and _lib.available():
            _lib.lib().dlbb_gemm_set_concurrent(0)
        return False


def _autotune(key, args) -> str:
    mode = os.environ.get("DLBB_GEMM", "auto").lower()
    if mode in _IMPLS:
        return mode
    if key in CHOICES:
        return CHOICES[key]
    if torch.cuda.is_current_stream_capturing():
        return "mfma"
    impls = dict(_IMPLS)
    if key[-1] == "concurrent":
        del impls["blas"]
    if not mfma192_ok(key[0], key[1]):
        del impls["mfma192"]
    # key: (M, N, K, lda, act, bias, residual, out dtype, preact[, "concurrent"])
    plain = (key[4] is None and not key[5] and not key[6] and key[7] == torch.bfloat16
             and not key[8] and key[-1] != "concurrent")
    if not mfma192p_ok(key[0], key[1], key[2], plain):
        del impls["mfma192p"]
    # Stream-K: grids below one round of the CUs; off beside comm kernels (its ranges assume
    # every CU is free, like the persistent forms)
    if key[-1] == "concurrent" or not streamk_ok(args[0], args[1]):
        del impls["mfma_sk"]
    # split-K (plain bf16 products below one round of the CUs; off beside comm kernels)
    if not plain or split_plan(key[0], key[1], key[2], _num_cus(args[0].device)) is None:
        del impls["mfma_split"]
    # skinny-M weight streaming (M <= 16: the decode step). Its grid never waits on another
    # workgroup and assumes no co-residency, so it stays a candidate beside comm kernels.
    if not skinny_ok(args[0], args[1], args[5], args[6]):
        del impls["mfma_skinny"]
    times = _time_interleaved({n: (lambda f=f: f(*args)) for n, f in impls.items()})
    best, times = _choose(times, "linear", key)
    CHOICES[key] = best
    _log_tune("linear", key, times, best)
    return best


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
           act: Optional[str] = None, residual: Optional[torch.Tensor] = None,
           out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
           preact: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``act(x @ w.T + bias) + residual``; x ``[..., K]``, w ``[N, K]``; returns ``[..., N]``.

    GPU dispatch per shape (measured once, cached in :data:`CHOICES`; ``DLBB_GEMM`` forces):
    ``mfma`` = the hand-written gfx950 kernel with the whole epilogue fused, or ``blas`` =
    hipBLASLt GEMM + our HIP epilogue kernels. Both are native; the faster one runs.
    """
    lead = x.shape[:-1]
    K = x.shape[-1]
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"linear: x[..., {K}] vs w{tuple(w.shape)}")
    x2 = x.reshape(-1, K)
    M = x2.shape[0]
    out_dtype = out_dtype or x.dtype
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    if use_hip(x, w):
        if out is None:
            out = torch.empty(*lead, N, dtype=out_dtype, device=x.device)
        if out.dtype not in (torch.bfloat16, torch.float32) or not out.is_contiguous():
            raise ValueError("linear: out must be contiguous bf16/fp32")
        if bias is not None:
            bias = bias.contiguous()
        r2 = None
        if residual is not None:
            r2 = residual.reshape(M, N)
            if r2.stride(1) != 1 or r2.dtype != torch.bfloat16:
                r2 = r2.contiguous().to(torch.bfloat16)
        o2 = out.view(M, N)
        if not hip_supported(x2, w):
            FALLBACKS["count"] += 1
            _blas_linear(x2 if x2.stride(1) == 1 else x2.contiguous(), w.contiguous(), bias,
                         act, r2, o2, preact)
            return out
        key = (M, N, K, x2.stride(0), act, bias is not None, r2 is not None, out.dtype,
               preact is not None)
        if _CONCURRENT[0]:
            key = key + ("concurrent",)
        args = (x2, w, bias, act, r2, o2, preact)
        _IMPLS[_autotune(key, args)](*args)
        CALLS[("linear", key)] = CALLS.get(("linear", key), 0) + 1
        return out
    y = _torch_linear(x2, w, bias, act, residual, out_dtype, preact)
    return y.reshape(*lead, N) if out is None else out.copy_(y.reshape(out.shape))


def wgrad_supported(dy2: torch.Tensor, x2: torch.Tensor) -> bool:
    M, N = dy2.shape
    K = x2.shape[1]
    return (dy2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16 and x2.shape[0] == M
            and M % 32 == 0 and N % 128 == 0 and K % 128 == 0 and dy2.stride(1) == 1
            and x2.stride(1) == 1 and dy2.stride(0) % 8 == 0 and x2.stride(0) % 8 == 0
            and dy2.data_ptr() % 16 == 0 and x2.data_ptr() % 16 == 0
            # the kernel's buffer offsets (from a split's first row) stay below 2 GiB
            and M * max(dy2.stride(0), x2.stride(0)) * 2 < (1 << 31))


_COUNTERS = {}   # (device index, stream handle) -> int32 tile counters, zero between launches
# In-launch split-K combine of the weight-gradient kernel (each tile's last-arriving workgroup
# sums the fp32 slabs). OFF: measured 1.3-2.3x SLOWER than the separate reduce pass at every
# GPT-2 dW shape (profiles/r05_wgrad): a tile's slabs are split x 64 KiB (0.4-1.4 MB), read
# serially by ONE workgroup at ~0.1 TB/s, far past the "few tens of KB per tile" where an
# in-launch combine pays (CDNA guide §5). Kept as a tested form (set_wgrad_fused) for A/B.
_WGRAD_FUSED = [False]


def set_wgrad_fused(on: bool) -> None:
    _WGRAD_FUSED[0] = bool(on)


def wgrad_fused_reduce() -> bool:
    return _WGRAD_FUSED[0]


def _tile_counters(device: torch.device, n: int) -> torch.Tensor:
    """Arrival counters for ``n`` tiles of the fused weight-gradient reduce."""
    return _stream_buffers(_COUNTERS, device, (n, torch.int32, 4096, True))[0]


# Cap on the default split-K of the weight gradient (None: no cap). The default fills about one
# resident wave when the kernel has the chip; beside the main stream's backward a smaller split
# writes and re-reads fewer fp32 partials — but measured slower in the step at every cap
# (tools/step_ab.py split_cap=N, profiles/r06_step/wgrad_split_cap_ab.jsonl); default no cap.
_WGRAD_SPLIT_CAP = [None]


def set_wgrad_split_cap(cap: Optional[int]) -> None:
    _WGRAD_SPLIT_CAP[0] = None if cap is None else max(1, int(cap))


def _wgrad_hip(dy2, x2, out, accumulate, split=None, bias_out=None, bn=128, bk=128):
    M, N = dy2.shape
    K = x2.shape[1]
    tiles = (N // bn) * (K // bk)
    if split is None:
        # about one resident wave of workgroups (3 per CU x 256 CUs for 128 x 128 tiles, 2 per
        # CU for 256 x 128 and 128 x 256): measured best with the XCD-aware tile order
        # (profiles/r01_gpt2/wgrad_split_xcd.jsonl)
        # (two-per-CU tiles: at most the 512 resident slots — a 2nd partial round costs a
        # whole workgroup time)
        split = max(1, min(M // 256, (-(-768 // tiles)) if bn == bk == 128
                           else max(1, 512 // tiles)))
        if _WGRAD_SPLIT_CAP[0] is not None:
            split = min(split, _WGRAD_SPLIT_CAP[0])
    # one split, plain store, no bias: the kernel stores dW itself (no fp32 partials, no
    # reduce pass — the LM-head dW)
    direct = split == 1 and not accumulate and bias_out is None
    ws = None if direct else torch.empty(split * (N * K + N), dtype=torch.float32,
                                         device=dy2.device)
    if not direct and wgrad_fused_reduce() and out.data_ptr() % 16 == 0:
        # split-K partials combined inside the launch by each tile's last-arriving workgroup
        cnt = _tile_counters(dy2.device, tiles)
        check(_lib.lib().dlbb_gemm_wgrad_fused(
            dy2.data_ptr(), dy2.stride(0), x2.data_ptr(), x2.stride(0), out.data_ptr(),
            _lib.dt(out), int(accumulate), ws.data_ptr(), M, N, K, split, _lib.ptr(bias_out),
            int(bn), int(bk), cnt.data_ptr(), cnt.numel(), _lib.stream(dy2.device)),
            "gemm_wgrad_fused")
        return
    check(_lib.lib().dlbb_gemm_wgrad_tile2(dy2.data_ptr(), dy2.stride(0), x2.data_ptr(),
                                           x2.stride(0), out.data_ptr(), _lib.dt(out),
                                           int(accumulate), _lib.ptr(ws), M, N, K, split,
                                           _lib.ptr(bias_out), int(bn), int(bk),
                                           _lib.stream(dy2.device)),
          "gemm_wgrad")


def _wgrad_hip256(dy2, x2, out, accumulate, split=None, bias_out=None):
    """256 x 128 output tiles (8 waves): 1.33x the MFMA work per L2 byte of the 128^2 tile."""
    _wgrad_hip(dy2, x2, out, accumulate, split, bias_out, bn=256)


def _wgrad_hip_wide(dy2, x2, out, accumulate, split=None, bias_out=None):
    """128 x 256 output tiles, 4 waves of 64 x 128: 25 % fewer LDS fragment bytes per MFMA than
    the 64 x 64-per-wave tiles (the GPT-2 dW shapes are LDS-bound there); needs K % 256."""
    _wgrad_hip(dy2, x2, out, accumulate, split, bias_out, bn=128, bk=256)


def wgrad_pp_supported(dy2, x2, out, accumulate, bias_out=None) -> bool:
    """Contract of the 256^2 ping-pong weight-gradient kernel (``dlbb_gemm_bf16_tn``): accumulate
    only into bf16, output rows N % 128, columns K % 256, reduction M % 64, 32-bit buffer offsets
    over both operands (a bias gradient is a separate column sum, :func:`_wgrad_pp`)."""
    M, N = dy2.shape
    K = x2.shape[1]
    return ((not accumulate or out.dtype == torch.bfloat16)
            and N % 128 == 0 and K % 256 == 0 and M % 64 == 0
            and M * dy2.stride(0) * 2 < 2 ** 31 and M * x2.stride(0) * 2 < 2 ** 31)


def _pp_launch(dy2, x2, out, accumulate, r0, r1, split):
    """TN kernel on output rows [r0, r1) (dY columns r0..r1-1), split-K ``split``."""
    M = dy2.shape[0]
    K = x2.shape[1]
    o = out[r0:r1]
    ws = (torch.empty(split * (r1 - r0) * K, dtype=torch.float32, device=dy2.device)
          if split > 1 else None)
    check(_lib.lib().dlbb_gemm_bf16_tn(
        dy2.data_ptr() + r0 * dy2.element_size(), dy2.stride(0), x2.data_ptr(), x2.stride(0),
        o.data_ptr(), K, r1 - r0, K, M, o.data_ptr() if accumulate else None,
        K if accumulate else 0, EPI_RESIDUAL if accumulate else 0,
        1 if out.dtype == torch.float32 else 0, int(split), _lib.ptr(ws),
        _lib.stream(dy2.device)), "gemm_bf16_tn")


def pp_tail_plan(M: int, N: int, K: int, ncu: int):
    """Row split of the TN grid: (head_rows, tail_split). A grid whose last round is at most half
    full (the LM-head dW: 591 tiles on 256 CUs) runs its whole rounds first, then the tail rows
    with split-K so the tail fills about one round; else (N, 1)."""
    tiles_n = K // 256
    m_tiles = -(-N // 256)
    total = m_tiles * tiles_n
    rounds, rem = divmod(total, ncu)
    nkt = M // 64
    if rounds < 1 or rem == 0 or 2 * rem > ncu:
        return N, 1
    head = (rounds * ncu // tiles_n) * 256
    tail_tiles = -(-(N - head) // 256) * tiles_n
    split = min(ncu // tail_tiles, nkt // 8)
    if split >= 2:                      # no empty trailing slice: as the kernel's launch clamps
        kt = -(-nkt // split)
        split = -(-nkt // kt)
    return (head, split) if split >= 2 else (N, 1)


def _wgrad_pp(dy2, x2, out, accumulate, split=None, bias_out=None):
    """256 x 256 output tiles on the forward's ping-pong schedule, both operands staged as
    transposed-read LDS images (``csrc/gemm.hip`` TN): 4x the MFMA work per staged byte of the
    128^2 tile, whole reduction per workgroup (dW stored directly). A partial last round is run
    as a split-K tail (:func:`pp_tail_plan`; plain stores only). ``split`` is ignored."""
    M, N = dy2.shape
    K = x2.shape[1]
    head, tsplit = (N, 1)
    if not accumulate:
        head, tsplit = pp_tail_plan(M, N, K, _num_cus(dy2.device))
    _pp_launch(dy2, x2, out, accumulate, 0, head, 1)
    if head < N:
        _pp_launch(dy2, x2, out, accumulate, head, N, tsplit)
    if bias_out is not None:            # no fused bias on this kernel: one column-sum pass
        db = dy2.sum(0, dtype=torch.float32)
        if accumulate:                  # fp32 add, one rounding (as the fused kernels)
            bias_out.copy_((bias_out.float() + db).to(bias_out.dtype))
        else:
            bias_out.copy_(db)


def _wgrad_blas(dy2, x2, out, accumulate, split=None, bias_out=None):
    if accumulate and out.dtype == dy2.dtype:
        out.addmm_(dy2.t(), x2)             # the library GEMM accumulates (beta = 1): no add pass
    elif accumulate:
        out.add_(torch.matmul(dy2.t(), x2).to(out.dtype))
    elif out.dtype == dy2.dtype:
        torch.matmul(dy2.t(), x2, out=out)
    else:
        out.copy_(torch.matmul(dy2.t(), x2))
    if bias_out is not None:
        db = dy2.sum(0, dtype=torch.float32)
        if accumulate:
            bias_out.add_(db.to(bias_out.dtype))
        else:
            bias_out.copy_(db)


WGRAD_CHOICES = {}    # (M, N, K, out dtype, fused bias) -> "mfma" | "mfma256" | "pp" | "blas"
_WGRAD_IMPLS = {"mfma": _wgrad_hip, "mfma256": _wgrad_hip256, "mfma_wide": _wgrad_hip_wide,
                "pp": _wgrad_pp, "blas": _wgrad_blas}


def _wgrad_choice(dy2, x2, out, bias_out=None) -> str:
    mode = os.environ.get("DLBB_GEMM", "auto").lower()
    if mode in _WGRAD_IMPLS:
        if mode == "pp" and not wgrad_pp_supported(dy2, x2, out, False, bias_out):
            return "mfma"
        if (mode == "mfma256" and dy2.shape[1] % 256) or (mode == "mfma_wide" and
                                                           x2.shape[1] % 256):
            return "mfma"
        return mode
    key = (dy2.shape[0], dy2.shape[1], x2.shape[1], out.dtype, bias_out is not None)
    if key in WGRAD_CHOICES:
        return WGRAD_CHOICES[key]
    if torch.cuda.is_current_stream_capturing():
        return "mfma"
    scratch = torch.empty_like(out)
    scratch_b = torch.empty_like(bias_out) if bias_out is not None else None
    cands = {}
    for name, fn in _WGRAD_IMPLS.items():
        if name == "mfma256" and dy2.shape[1] % 256:
            continue
        if name == "mfma_wide" and x2.shape[1] % 256:
            continue
        if name == "pp" and not wgrad_pp_supported(dy2, x2, out, False, bias_out):
            continue
        cands[name] = lambda f=fn: f(dy2, x2, scratch, False, None, scratch_b)
    times = _time_interleaved(cands)
    best, times = _choose(times, "wgrad", key)
    WGRAD_CHOICES[key] = best
    _log_tune("wgrad", key, times, best)
    return best


def wgrad(dy2: torch.Tensor, x2: torch.Tensor, out: Optional[torch.Tensor] = None,
          accumulate: bool = False, split: Optional[int] = None,
          bias_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight gradient ``dW = dy2^T @ x2`` ([N, K]) for row-major ``dy2 [M, N]``, ``x2 [M, K]``.

    HIP path (``csrc/gemm_tn.hip``): transposed-read MFMA tiles, split-K over M with fp32
    partials and one reduce/cast pass; ``accumulate=True`` adds into ``out``. ``bias_out``
    ([N], same dtype as ``out``) also receives the bias gradient ``dy2.sum(0)`` — fused into
    the same kernels on the HIP path. Per shape the faster of this kernel and the library GEMM
    is measured once and cached (:data:`WGRAD_CHOICES`; ``DLBB_GEMM=mfma|blas`` forces; an
    explicit ``split`` forces ours)."""
    M, N = dy2.shape
    K = x2.shape[1]
    if out is None:
        out = torch.empty(N, K, dtype=dy2.dtype, device=dy2.device)
    fused_ok = bias_out is None or (bias_out.is_contiguous() and bias_out.dtype == out.dtype
                                    and bias_out.numel() == N)
    if (use_hip(dy2, x2) and wgrad_supported(dy2, x2) and out.is_contiguous() and fused_ok
            and out.dtype in (torch.bfloat16, torch.float32)):
        choice = "mfma" if split is not None else _wgrad_choice(dy2, x2, out, bias_out)
        if choice == "pp" and not wgrad_pp_supported(dy2, x2, out, accumulate, bias_out):
            choice = "mfma"                 # tuned on a plain store; this call accumulates fp32
        _WGRAD_IMPLS[choice](dy2, x2, out, accumulate, split, bias_out)
        if split is None:
            k = (dy2.shape[0], dy2.shape[1], x2.shape[1], out.dtype, bias_out is not None)
            CALLS[("wgrad", k)] = CALLS.get(("wgrad", k), 0) + 1
        return out
    _wgrad_blas(dy2, x2, out, accumulate, None, bias_out)
    return out


def dgrad_supported(dy2: torch.Tensor, w: torch.Tensor) -> bool:
    """Contract of the NN kernel (``dlbb_gemm_bf16_nn``): reduction K % 64, output N % 256,
    M % 8, 16-byte aligned rows, 32-bit buffer offsets over all of W."""
    M, K = dy2.shape
    N = w.shape[1]
    return (dy2.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.shape[0] == K
            and K % 64 == 0 and N % 256 == 0 and M % 8 == 0 and M >= 8
            and dy2.stride(1) == 1 and w.stride(1) == 1 and dy2.stride(0) % 8 == 0
            and w.stride(0) % 8 == 0 and dy2.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
            and K * w.stride(0) * 2 < (1 << 31) and dy2.stride(0) * 512 + K * 2 < (1 << 31))


def dgrad_split(M: int, N: int, K: int) -> int:
    """Split-K factor of the NN kernel: 1 unless the 256^2 grid is below one workgroup per CU
    and K is long (the LM-head dX: 192 tiles x 786 K-tiles), then the smallest split that
    fills whole rounds of the 256 CUs with >= 16 K-tiles per slice."""
    tiles = -(-M // 256) * (N // 256)
    if tiles >= 256 or K < 64 * 64:
        return 1
    for s in range(2, 9):
        if (tiles * s) % 256 == 0 and K // 64 >= 16 * s:
            return s
    return 1


def _dgrad_hip(dy2, w, out, split=None, dgelu=None):
    M, K = dy2.shape
    N = w.shape[1]
    epi, u = 0, None
    if dgelu is not None:
        u, act = dgelu
        epi = EPI_DGELU[act]
        split = 1
    if split is None:
        split = dgrad_split(M, N, K)
    ws = torch.empty(split * M * N, dtype=torch.float32, device=dy2.device) if split > 1 else None
    check(_lib.lib().dlbb_gemm_bf16_nn(
        dy2.data_ptr(), dy2.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), N, M, N, K,
        None, _lib.ptr(u), u.stride(0) if u is not None else 0, None, epi, 0, int(split),
        _lib.ptr(ws), _lib.stream(dy2.device)), "gemm_bf16_nn")
    return out


def _dgrad_blas(dy2, w, out, split=None, dgelu=None):
    if dgelu is None:
        return torch.matmul(dy2, w, out=out)
    u, act = dgelu
    dg = torch.matmul(dy2, w)
    check(_lib.lib().dlbb_bias_gelu_bwd(dg.data_ptr(), u.data_ptr(), None, out.data_ptr(), None,
                                        out.shape[0], out.shape[1], _APPROX[act],
                                        _lib.stream(dy2.device)), "bias_gelu_bwd")
    return out


DGRAD_CHOICES = {}    # (M, N, K, lda, fused GELU-backward act or None) -> "mfma" | "blas"
_DGRAD_IMPLS = {"mfma": _dgrad_hip, "blas": _dgrad_blas}


def _dgrad_choice(dy2, w, out, dgelu=None) -> str:
    mode = os.environ.get("DLBB_GEMM", "auto").lower()
    if mode in ("mfma", "blas"):
        return mode
    key = (dy2.shape[0], w.shape[1], dy2.shape[1], dy2.stride(0),
           dgelu[1] if dgelu is not None else None)
    if key in DGRAD_CHOICES:
        return DGRAD_CHOICES[key]
    if torch.cuda.is_current_stream_capturing():
        return "mfma"
    scratch = torch.empty_like(out)
    times = _time_interleaved({n: (lambda f=f: f(dy2, w, scratch, dgelu=dgelu))
                               for n, f in _DGRAD_IMPLS.items()})
    best, times = _choose(times, "dgrad", key)
    DGRAD_CHOICES[key] = best
    _log_tune("dgrad", key, times, best)
    return best


def dgrad(dy2: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None,
          dgelu=None) -> torch.Tensor:
    """Input gradient ``dX = dY @ W`` for ``dy2 [M, K]`` and a Linear weight ``w [K, N]``
    (``[out_features, in_features]``): an NN GEMM — the reduction runs along W's rows.

    HIP path (``csrc/gemm.hip`` ``gemm_bf16_nn_256_pingpong3``): the forward's ping-pong 256^2
    schedule with W's [64 k][256 n] tiles staged as-is by LDS-DMA and read as MFMA fragments
    with ``ds_read_b64_tr_b16`` — no transposed copy of W. Per shape the faster of this kernel
    and the library GEMM is measured once (:data:`DGRAD_CHOICES`; ``DLBB_GEMM`` forces);
    shapes outside the contract go to the library and are counted as ``dgrad_library_calls``.

    ``dgelu=(u, act)``: the input of this GEMM was ``act(u)`` (GELU), and the result is the
    gradient w.r.t. ``u``: ``(dY @ W) * act'(u)`` — the GELU backward fused into the epilogue
    (``u`` [M, N] bf16, the forward's stored pre-activation)."""
    M, K = dy2.shape
    N = w.shape[1]
    u_ok = dgelu is None or (dgelu[0].dtype == torch.bfloat16 and dgelu[0].stride(1) == 1
                             and dgelu[0].stride(0) % 8 == 0 and dgelu[0].data_ptr() % 16 == 0
                             and tuple(dgelu[0].shape) == (M, N))
    if use_hip(dy2, w) and dgrad_supported(dy2, w) and u_ok and (out is None or (
            out.is_contiguous() and out.dtype == torch.bfloat16)):
        if out is None:
            out = torch.empty(M, N, dtype=dy2.dtype, device=dy2.device)
        choice = _dgrad_choice(dy2, w, out, dgelu)
        _DGRAD_IMPLS[choice](dy2, w, out, dgelu=dgelu)
        key = (M, N, K, dy2.stride(0), dgelu[1] if dgelu is not None else None)
        CALLS[("dgrad", key)] = CALLS.get(("dgrad", key), 0) + 1
        return out
    CALLS[("dgrad", "library")] = CALLS.get(("dgrad", "library"), 0) + 1
    if dgelu is not None:
        u, act = dgelu
        dg = torch.matmul(dy2.float(), w.float())
        uf = u.float()
        if act == "gelu_tanh":
            k0, k1 = 0.7978845608028654, 0.044715
            t = torch.tanh(k0 * (uf + k1 * uf ** 3))
            gp = 0.5 * (1 + t) + 0.5 * uf * (1 - t * t) * k0 * (1 + 3 * k1 * uf * uf)
        else:
            gp = 0.5 * (1 + torch.erf(uf * 0.7071067811865476)) + \
                uf * 0.3989422804014327 * torch.exp(-0.5 * uf * uf)
        r = (dg * gp).to(dy2.dtype)
        return r if out is None else out.copy_(r)
    return torch.matmul(dy2, w) if out is None else torch.matmul(dy2, w, out=out)


def kernel_mix() -> dict:
    """Which implementation each autotuned GEMM shape runs, for result JSONs (the
    kernel choice must be visible next to the throughput it produced). Per kind: shape count by
    choice plus every shape's measured ms per candidate (best of interleaved rounds)."""
    out = {}
    ours = total = 0.0
    for kind, table in (("linear", CHOICES), ("wgrad", WGRAD_CHOICES), ("dgrad", DGRAD_CHOICES)):
        counts = {}
        for v in table.values():
            counts[v] = counts.get(v, 0) + 1
        tuned = []
        for knd, key, times, best in TUNE_LOG:
            if knd != kind:
                continue
            n = CALLS.get((kind, key), 0)
            tuned.append({"key": [str(k) for k in key], "ms": times, "choice": best, "calls": n})
            total += n * times[best]
            ours += n * times[best] if best != "blas" else 0.0
        out[kind] = {"shapes_by_choice": counts, "tuned": tuned}
    # share of the autotuned GEMM time (calls x measured ms of the chosen implementation) that
    # runs on the hand-written kernels; the rest is hipBLASLt
    out["hand_written_time_fraction"] = round(ours / total, 4) if total else None
    out["dgrad_library_calls"] = CALLS.get(("dgrad", "library"), 0)   # not in the fraction
    out["forced"] = os.environ.get("DLBB_GEMM", "auto")
    out["library_margin"] = library_margin()   # blas chosen only when this much faster
    # True: every choice above was made on rank-max timings agreed by all ranks
    out["agreed_across_ranks"] = _AGREE is not None
    out["contract_fallbacks"] = FALLBACKS["count"]
    from .norm_act import LN_FALLBACKS                # LayerNorm backward at unfused widths
    out["layernorm_bwd_fallbacks"] = LN_FALLBACKS["count"]
    from . import fp8                                 # FP8 GEMM launches + distinct shapes
    out["fp8"] = fp8.kernel_mix()
    return out
