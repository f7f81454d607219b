"""FP8 (OCP ``e4m3fn``) GEMM path of the tensor-parallel forward (``csrc/gemm_fp8.hip``).

Per-row dynamic scaling: a bf16 matrix ``x [M, K]`` becomes e4m3 bytes plus one fp32 scale per
row, ``x[m, k] ~= float(q[m, k]) * scale[m]``; a linear layer quantises its activation per token
and its weight per output row, multiplies the bytes on the block-scaled MFMA
(``v_mfma_scale_f32_16x16x128_f8f6f4`` with unit hardware scales, twice the bf16 MFMA rate) and
applies ``scale_x[m] * scale_w[n]`` in the fp32 epilogue, ahead of bias / GELU / residual.

Quantisation semantics (exact; the tests compare bits). For a row with ``amax = max |x|``:

* ``amax == 0``: ``scale = 1`` and every byte is 0;
* otherwise ``inv = 448 / amax`` and ``scale = amax / 448`` (IEEE fp32 divisions) and
  ``q = e4m3fn_rne(float(x) * inv)`` — one fp32 multiply, round to nearest even.

Non-finite inputs (inf / NaN) are outside the contract: their bytes and scale are unspecified.

The path is opt-in (``gemm_dtype="fp8"`` on the TP layers / ``execution.gemm_dtype``); the bf16
GEMMs are untouched. On a GPU tensor the HIP kernels are the only implementation: a shape outside
the kernel contract raises, there is no fall-back to bf16. The torch formulas below serve CPU
tensors, ``DLBB_KERNELS=torch`` and ``kernels="torch"`` (the model-level reference).

Weight-only FP8 for the decode step (``csrc/gemm_skinny.hip``, :func:`linear_w8` /
:func:`w8_linear`): at M = batch rows <= 16 a linear is a pure stream of its weight, so the e4m3
copy of the weight (the same cached ``quantize_weight`` entry) is streamed instead — half the
bytes — widened to bf16 in registers (exact) and multiplied with the bf16 activation as it is;
the row scale is applied to the fp32 accumulator. Opt-in too (``decode_weight_dtype="fp8"``).
"""

from __future__ import annotations

import ctypes
import weakref
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import check, use_hip
from .gemm import ACTS, EPI_BIAS, EPI_RESIDUAL, _HIP_INVALID_VALUE, _num_cus

E4M3 = torch.float8_e4m3fn
E4M3_MAX = 448.0
QUANT_MAX_K = 16384      # the quantiser keeps a whole row in one workgroup's registers

CALLS = {}               # (M, N, K) -> FP8 GEMM launches since import (gemm.kernel_mix()["fp8"])


def _want_hip(kernels: Optional[str], *tensors) -> bool:
    if kernels == "torch":
        return False
    return use_hip(*tensors)


def _quantize_torch(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True)
    zero = amax == 0
    one = torch.ones_like(amax)
    # tensor / tensor: a true fp32 division (`float / tensor` is reciprocal-then-multiply in
    # torch, one rounding too many — it flips round-to-nearest-even ties of x * inv)
    top = torch.full_like(amax, E4M3_MAX)
    inv = torch.where(zero, one, top / amax)
    scale = torch.where(zero, one, amax / top)
    return (xf * inv).to(E4M3), scale.squeeze(-1)


def quantize_rows(x: torch.Tensor, out_q: Optional[torch.Tensor] = None,
                  out_scale: Optional[torch.Tensor] = None,
                  kernels: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``x [..., K]`` -> ``(q, scale)``: ``q`` e4m3fn ``[..., K]``, ``scale`` fp32 ``[...]`` (module
    docstring for the exact semantics; non-finite inputs are out of contract).

    HIP path (bf16 input; one pass, each row read once and held in registers between the amax and
    the convert): rows may be strided (``x[:, :k]`` of a wider matrix is read in place);
    ``K % 8 == 0``, ``K <= 16384``, 16-byte aligned rows. ``out_q`` / ``out_scale`` receive the
    result (``out_q`` 2-D e4m3fn, unit column stride, row stride a multiple of 8)."""
    K = x.shape[-1]
    lead = x.shape[:-1]
    if not _want_hip(kernels, x):
        q, s = _quantize_torch(x)
        if out_q is not None:
            out_q.view(torch.uint8).copy_(q.reshape(out_q.shape).view(torch.uint8))
            q = out_q
        if out_scale is not None:
            s = out_scale.copy_(s.reshape(out_scale.shape))
        return q, s
    if x.dtype != torch.bfloat16:
        raise ValueError(f"quantize_rows: the HIP quantiser takes bf16, got {x.dtype}")
    x2 = x if x.dim() == 2 else x.reshape(-1, K)
    M = x2.shape[0]
    if x2.stride(1) != 1 and M * K:
        x2 = x2.contiguous()
    if K % 8 or K > QUANT_MAX_K or K == 0:
        raise ValueError(f"quantize_rows: K = {K} outside the contract (K % 8 == 0, "
                         f"0 < K <= {QUANT_MAX_K})")
    if M and (x2.data_ptr() % 16 or (M > 1 and x2.stride(0) % 8)):
        raise ValueError("quantize_rows: rows must be 16-byte aligned")
    if out_q is None:
        out_q = torch.empty(M, K, dtype=E4M3, device=x.device)
        q_ret = out_q.view(*lead, K)
    else:
        if (out_q.dtype != E4M3 or out_q.dim() != 2 or tuple(out_q.shape) != (M, K)
                or out_q.stride(1) != 1 or out_q.stride(0) % 8 or out_q.data_ptr() % 8
                or out_q.device != x.device):
            raise ValueError("quantize_rows: out_q must be an [M, K] e4m3fn matrix with 8-byte "
                             "aligned rows on the input's device")
        q_ret = out_q
    if out_scale is None:
        out_scale = torch.empty(M, dtype=torch.float32, device=x.device)
        s_ret = out_scale.view(*lead)
    else:
        if (out_scale.dtype != torch.float32 or out_scale.numel() != M
                or not out_scale.is_contiguous() or out_scale.device != x.device):
            raise ValueError("quantize_rows: out_scale must be contiguous fp32 with one element "
                             "per row")
        s_ret = out_scale
    if M:
        check(_lib.lib().dlbb_quant_fp8_rows(
            x2.data_ptr(), x2.stride(0) if M > 1 else K, out_q.data_ptr(),
            out_q.stride(0) if M > 1 else K, out_scale.data_ptr(), M, K, _lib.stream(x.device)),
            "quant_fp8_rows")
    return q_ret, s_ret


def _epilogue_torch(y, bias, act, residual, out_dtype):
    if bias is not None:
        y = y + bias.float()
    if act in ("gelu", "gelu_erf"):
        y = F.gelu(y)
    elif act == "gelu_tanh":
        y = F.gelu(y, approximate="tanh")
    if residual is not None:
        y = y + residual.reshape(y.shape).float()
    return y.to(out_dtype)


def gemm_contract_error(M: int, N: int, K: int) -> Optional[str]:
    """Why (M, N, K) is outside the FP8 GEMM kernel's shape contract, or None."""
    if M <= 0 or N <= 0 or K <= 0:
        return "empty operand"
    if K % 128:
        return f"K = {K} is not a multiple of 128"
    if M % 8:
        return f"M = {M} is not a multiple of 8"
    if N % 64:
        return f"N = {N} is not a multiple of 64"
    return None


def linear_fp8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor,
               bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
               residual: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.bfloat16,
               out: Optional[torch.Tensor] = None,
               kernels: Optional[str] = None) -> torch.Tensor:
    """``act(((xq @ wq.T) * xs[:, None] * ws[None, :]) + bias) + residual``.

    ``xq [..., K]`` and ``wq [N, K]`` e4m3fn (K-contiguous), ``xs [...]`` and ``ws [N]`` fp32 row
    scales (:func:`quantize_rows`), ``bias [N]`` / ``residual [..., N]`` bf16; fp32 accumulation,
    bf16 or fp32 result ``[..., N]``.

    HIP contract: ``K % 128 == 0``, ``M % 8 == 0`` (M = rows of ``xq``), ``N % 64 == 0``, every
    row 16-byte aligned. Anything else raises ``ValueError`` before any launch."""
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    if xq.dtype != E4M3 or wq.dtype != E4M3:
        raise ValueError(f"linear_fp8: operands must be {E4M3}, got {xq.dtype} / {wq.dtype}")
    K = xq.shape[-1]
    N = wq.shape[0]
    lead = xq.shape[:-1]
    if wq.dim() != 2 or wq.shape[1] != K:
        raise ValueError(f"linear_fp8: xq[..., {K}] vs wq{tuple(wq.shape)}")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("linear_fp8: out_dtype must be bf16 or fp32")
    x2 = xq.reshape(-1, K)
    M = x2.shape[0]
    if xs.numel() != M or ws.numel() != N:
        raise ValueError("linear_fp8: one scale per row of xq and of wq")
    if not _want_hip(kernels, xq, wq):
        y = (x2.float() @ wq.float().t()) * xs.reshape(M, 1).float() * ws.reshape(1, N).float()
        y = _epilogue_torch(y, bias, act, None if residual is None else residual.reshape(M, N),
                            out_dtype).reshape(*lead, N)
        return y if out is None else out.copy_(y.reshape(out.shape))
    why = gemm_contract_error(M, N, K)
    if why:
        raise ValueError(f"linear_fp8: {why} (contract: K % 128 == 0, M % 8 == 0, N % 64 == 0; "
                         "there is no fall-back to bf16)")
    if x2.stride(1) != 1 or wq.stride(1) != 1:
        raise ValueError("linear_fp8: operands must be K-contiguous")
    if (x2.data_ptr() % 16 or wq.data_ptr() % 16 or (M > 1 and x2.stride(0) % 16)
            or (N > 1 and wq.stride(0) % 16)):
        raise ValueError("linear_fp8: operand rows must be 16-byte aligned")
    if xs.dtype != torch.float32 or ws.dtype != torch.float32:
        raise ValueError("linear_fp8: scales must be fp32")
    xs1 = xs.reshape(M)
    ws1 = ws.reshape(N)
    if not xs1.is_contiguous():
        xs1 = xs1.contiguous()
    if not ws1.is_contiguous() or ws1.data_ptr() % 16:
        ws1 = ws1.clone(memory_format=torch.contiguous_format)
    if out is None:
        out = torch.empty(*lead, N, dtype=out_dtype, device=xq.device)
    elif out.dtype not in (torch.bfloat16, torch.float32) or not out.is_contiguous() \
            or out.numel() != M * N or out.data_ptr() % 16:
        raise ValueError("linear_fp8: out must be contiguous, 16-byte aligned bf16/fp32 [..., N]")
    epi = ACTS[act]
    if bias is not None:
        if bias.dtype != torch.bfloat16 or bias.numel() != N:
            raise ValueError("linear_fp8: bias must be bf16 [N]")
        bias = bias.contiguous()
        if bias.data_ptr() % 16:
            bias = bias.clone()
        epi |= EPI_BIAS
    r2 = None
    if residual is not None:
        r2 = residual.reshape(M, N)
        if r2.dtype != torch.bfloat16 or r2.stride(1) != 1 or r2.stride(0) % 8 \
                or r2.data_ptr() % 16:
            r2 = r2.to(torch.bfloat16).contiguous()
        epi |= EPI_RESIDUAL
    check(_lib.lib().dlbb_gemm_fp8_nt(
        x2.data_ptr(), x2.stride(0) if M > 1 else K, wq.data_ptr(), wq.stride(0) if N > 1 else K,
        xs1.data_ptr(), ws1.data_ptr(), out.data_ptr(), N, M, N, K, _lib.ptr(bias),
        _lib.ptr(r2), r2.stride(0) if r2 is not None else 0, epi,
        1 if out.dtype == torch.float32 else 0, _lib.stream(xq.device)), "gemm_fp8_nt")
    CALLS[(M, N, K)] = CALLS.get((M, N, K), 0) + 1
    return out


def set_bal(mode: int) -> None:
    """Balanced LDS-DMA issue of the FP8 ping-pong kernel: 0 never, 1 always, 2 = from 32 K-tiles
    (K >= 4096) on (default); for A/B measurements."""
    _lib.lib().dlbb_gemm_fp8_set_bal(int(mode))


# Quantised weights, one entry per weight storage: data_ptr -> (weak reference to the tensor,
# its _version, device, shape, kernels flavour, wq, ws). An in-place update of the weight
# (``load_from_dense``'s ``copy_``) bumps ``_version`` and the next call requantises; a dead
# tensor's entry is dropped with it.
_WCACHE = {}


def quantize_weight(w: torch.Tensor, kernels: Optional[str] = None):
    """``(wq, ws)`` of a Linear weight ``[N, K]`` (one scale per output row), cached until the
    weight changes (``_version``) or moves (``data_ptr``)."""
    key = w.data_ptr()
    try:
        version = w._version
    except RuntimeError:        # an inference tensor has no version counter: never cached
        return quantize_rows(w.detach(), kernels=kernels)
    ent = _WCACHE.get(key)
    if ent is not None:
        ref, ver, shape, flavour, wq, ws = ent
        if ref() is w and ver == version and shape == tuple(w.shape) and flavour == kernels:
            return wq, ws
    if torch.cuda.is_available() and w.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("fp8: a weight must be quantised before HIP-graph capture (run one "
                           "eager forward first)")
    wq, ws = quantize_rows(w.detach(), kernels=kernels)

    def _drop(ref, key=key):            # the weight died: free its quantised copy
        ent = _WCACHE.get(key)
        if ent is not None and ent[0] is ref:
            del _WCACHE[key]

    _WCACHE[key] = (weakref.ref(w, _drop), version, tuple(w.shape), kernels, wq, ws)
    return wq, ws


def clear_weight_cache() -> None:
    _WCACHE.clear()


def fp8_linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
               act: Optional[str] = None, residual: Optional[torch.Tensor] = None,
               out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
               kernels: Optional[str] = None) -> torch.Tensor:
    """``act(x @ w.T + bias) + residual`` through the FP8 GEMM: ``x [..., K]`` is quantised per
    row (token) on every call, the bf16 weight ``w [N, K]`` once (:func:`quantize_weight`)."""
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in (torch.bfloat16, torch.float32) else torch.bfloat16
    if w.shape[1] != x.shape[-1]:
        raise ValueError(f"fp8_linear: x[..., {x.shape[-1]}] vs w{tuple(w.shape)}")
    if _want_hip(kernels, x, w):            # refuse before the quantiser launches anything
        M = x.numel() // max(x.shape[-1], 1)
        why = gemm_contract_error(M, w.shape[0], x.shape[-1])
        if why:
            raise ValueError(f"fp8_linear: {why} (contract: K % 128 == 0, M % 8 == 0, "
                             "N % 64 == 0; there is no fall-back to bf16)")
    wq, ws = quantize_weight(w, kernels)
    xq, xs = quantize_rows(x, kernels=kernels)
    return linear_fp8(xq, xs, wq, ws, bias, act, residual, out_dtype, out, kernels=kernels)


# ---- weight-only FP8 (W8A16) for the decode step: csrc/gemm_skinny.hip -------------------------

W8_LAUNCHES = {"count": 0}     # launches of the W8 skinny kernel itself

_W8_CONTRACT = "contract: 1 <= M <= 16, N % 16 == 0, K % 64 == 0; there is no fall-back to bf16"
_W8_PLANS = {}


def w8_contract_error(M: int, N: int, K: int) -> Optional[str]:
    """Why (M, N, K) is outside the W8 skinny GEMM's shape contract, or None."""
    if M <= 0 or N <= 0 or K <= 0:
        return "empty operand"
    if M > 16:
        return f"M = {M} is larger than 16"
    if N % 16:
        return f"N = {N} is not a multiple of 16"
    if K % 64:
        return f"K = {K} is not a multiple of 64"
    return None


def w8_skinny_plan(M: int, N: int, K: int, ncu: int):
    """(grid, K-split inside a workgroup, K-split across workgroups, workspace bytes) of the W8
    skinny GEMM (``dlbb_gemm_w8_skinny_plan``), or None outside its shape contract."""
    key = (int(M), int(N), int(K), int(ncu))
    if key not in _W8_PLANS:
        out = (ctypes.c_int64 * 4)()
        ok = _lib.lib().dlbb_gemm_w8_skinny_plan(*key, out)
        _W8_PLANS[key] = tuple(int(v) for v in out) if ok else None
    return _W8_PLANS[key]


def _w8_refusal(x2, wq, ws1, out, M, N, K) -> str:
    """Names the term of the C contract a refused call violated (the slow path of a refusal)."""
    why = w8_contract_error(M, N, K)
    if why:
        return why
    if M > 1 and (x2.stride(0) % 8 or x2.stride(0) < K):
        return f"x row stride {x2.stride(0)} is not a multiple of 8 elements >= K"
    if N > 1 and (wq.stride(0) % 16 or wq.stride(0) < K):
        return f"wq row stride {wq.stride(0)} is not a multiple of 16 bytes >= K"
    for name, t in (("x", x2), ("wq", wq), ("ws", ws1), ("out", out)):
        if t.data_ptr() % 16:
            return f"{name} is not 16-byte aligned"
    return "refused by the kernel's entry point"


def linear_w8(x: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor,
              bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
              residual: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.bfloat16,
              out: Optional[torch.Tensor] = None, kernels: Optional[str] = None) -> torch.Tensor:
    """``act((x @ wq.float().T) * ws[None, :] + bias) + residual``: weight-only FP8 for the
    M = batch rows of a decode step. ``x [..., K]`` bf16, ``wq [N, K]`` e4m3fn (K-contiguous),
    ``ws [N]`` fp32 row scales (:func:`quantize_rows`), ``bias [N]`` / ``residual [..., N]`` bf16;
    fp32 accumulation, bf16 or fp32 result ``[..., N]``.

    HIP contract: ``1 <= M <= 16`` (M = rows of ``x``), ``N % 16 == 0``, ``K % 64 == 0``, 16-byte
    aligned rows of ``x`` and ``wq``. Anything else raises ``ValueError`` before any launch.

    The host path is short (a decode step is a chain of ~10 us launches): dtypes and unit strides
    are checked here, shape, leading dimensions and alignment by the C entry point, which
    launches nothing outside the contract; only then is the violated term worked out."""
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    K = x.shape[-1]
    N = wq.shape[0]
    if wq.dim() != 2 or wq.shape[1] != K:
        raise ValueError(f"linear_w8: x[..., {K}] vs wq{tuple(wq.shape)}")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("linear_w8: out_dtype must be bf16 or fp32")
    lead = x.shape[:-1]
    x2 = x if x.dim() == 2 else x.reshape(-1, K)
    M = x2.shape[0]
    if ws.numel() != N:
        raise ValueError("linear_w8: one scale per row of wq")
    if not _want_hip(kernels, x, wq):
        y = (x2.float() @ wq.float().t()) * ws.reshape(1, N).float()
        y = _epilogue_torch(y, bias, act, None if residual is None else residual.reshape(M, N),
                            out_dtype).reshape(*lead, N)
        return y if out is None else out.copy_(y.reshape(out.shape))
    if x.dtype != torch.bfloat16 or wq.dtype != E4M3 or ws.dtype != torch.float32:
        raise ValueError(f"linear_w8: x must be bf16, wq {E4M3}, ws fp32; got {x.dtype} / "
                         f"{wq.dtype} / {ws.dtype}")
    if x2.stride(1) != 1 or wq.stride(1) != 1:
        raise ValueError("linear_w8: operands must be K-contiguous")
    ws1 = ws if ws.dim() == 1 else ws.reshape(N)
    if not ws1.is_contiguous():
        raise ValueError("linear_w8: ws must be contiguous")
    if out is None:
        out = torch.empty(*lead, N, dtype=out_dtype, device=x.device)
    elif out.dtype not in (torch.bfloat16, torch.float32) or not out.is_contiguous() \
            or out.numel() != M * N:
        raise ValueError("linear_w8: out must be contiguous bf16/fp32 [..., N]")
    epi = ACTS[act]
    if bias is not None:
        if bias.dtype != torch.bfloat16 or bias.numel() != N or not bias.is_contiguous():
            raise ValueError("linear_w8: bias must be contiguous bf16 [N]")
        epi |= EPI_BIAS
    r2 = None
    if residual is not None:
        r2 = residual.reshape(M, N)
        if r2.dtype != torch.bfloat16 or r2.stride(1) != 1:
            r2 = r2.to(torch.bfloat16).contiguous()
        epi |= EPI_RESIDUAL
    dev = x.device
    rc = _lib.lib().dlbb_gemm_w8_nt_skinny(
        x2.data_ptr(), x2.stride(0) if M > 1 else K, wq.data_ptr(),
        wq.stride(0) if N > 1 else K, ws1.data_ptr(), out.data_ptr(), M, N, K, _lib.ptr(bias),
        _lib.ptr(r2), r2.stride(0) if r2 is not None else 0, epi,
        1 if out.dtype == torch.float32 else 0, _num_cus(dev), _lib.stream(dev))
    if rc == 0:
        W8_LAUNCHES["count"] += 1
        return out
    if rc == _HIP_INVALID_VALUE:
        raise ValueError(f"linear_w8: {_w8_refusal(x2, wq, ws1, out, M, N, K)} ({_W8_CONTRACT})")
    check(rc, "gemm_w8_nt_skinny")


def w8_linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
              act: Optional[str] = None, residual: Optional[torch.Tensor] = None,
              out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
              kernels: Optional[str] = None) -> torch.Tensor:
    """``act(x @ w.T + bias) + residual`` with the bf16 weight ``w [N, K]`` streamed as e4m3:
    quantised per output row once (:func:`quantize_weight`, the cache entry :func:`fp8_linear`
    uses; before any graph capture), the bf16 activation ``x [..., K]`` as it is."""
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in (torch.bfloat16, torch.float32) else torch.bfloat16
    if w.shape[1] != x.shape[-1]:
        raise ValueError(f"w8_linear: x[..., {x.shape[-1]}] vs w{tuple(w.shape)}")
    if _want_hip(kernels, x, w):            # refuse before the quantiser launches anything
        M = x.numel() // max(x.shape[-1], 1)
        why = w8_contract_error(M, w.shape[0], x.shape[-1])
        if why:
            raise ValueError(f"w8_linear: {why} ({_W8_CONTRACT})")
    wq, ws = quantize_weight(w, kernels)
    return linear_w8(x, wq, ws, bias, act, residual, out_dtype, out, kernels=kernels)


def kernel_mix() -> dict:
    """FP8 GEMM launches since import and the distinct (M, N, K) they ran at."""
    return {"calls": int(sum(CALLS.values())),
            "shapes": [list(k) for k in sorted(CALLS)]}
