"""Weight-only MXFP4 (W4A16) for the decode step: the OCP MX format gfx950 has in hardware.

A bf16 weight ``W [N, K]`` (``K % 32 == 0``) becomes

* ``codes``: ``uint8 [N, K/2]``, row-major; byte ``j`` of a row holds element ``2j`` in its low
  nibble and element ``2j+1`` in its high nibble. A nibble is an e2m1 code: sign bit, then the
  magnitudes ``0, 0.5, 1, 1.5, 2, 3, 4, 6`` for codes 0..7 (the layout of
  ``torch.float4_e2m1fn_x2``);
* ``scales``: ``uint8 [N, K/32]``, row-major; one e8m0 byte ``b`` per block of 32 consecutive k,
  meaning ``2^(b-127)``;
* value ``= code_value * 2^(b-127)``. There is no per-row fp32 scale: pure MX.

Quantisation semantics (exact; the tests compare bits). Per block of 32, with ``amax`` over the
bf16 values as fp32:

* ``amax == 0``: ``b = 127`` and every code is 0;
* otherwise ``b = clamp(floor(log2(amax)) - 2 + 127, 2, 254)`` (the OCP rule with e2m1's
  emax = 2; ``floor(log2)`` from ``frexp``, never a float ``log2``), ``v = x / 2^(b-127)`` (an
  exact division), clamped to +-6 and rounded to the nearest grid value, ties to the even code
  (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4). Saturation is part
  of the rule: an element in (6, 8) after scaling becomes 6. The sign bit of a code is set
  exactly when ``x < 0`` (a negative element that rounds to zero is ``-0``).

Every emitted scale lies in **[2, 252]**: finite bf16 input has ``floor(log2(amax)) <= 127``,
and the lower clamp keeps the smallest non-zero dequantised value, ``0.5 * 2^-125 = 2^-126``, a
*normal* bf16; the largest is ``6 * 2^125``, finite. So ``code_value * 2^(b-127)`` is exactly
representable in bf16 for every (code, scale) pair the quantiser can emit, and the kernel's
``v_cvt_scalef32_pk_bf16_fp4`` is exact with no reliance on denormal modes. Non-finite inputs
are outside the contract.

``csrc/gemm_skinny.hip`` (:func:`linear_w4` / :func:`w4_linear`) streams the codes and scales —
0.53 of the e4m3 bytes, 0.27 of bf16 — widens them to the exact bf16 values in registers and
multiplies with the bf16 activation as it is. Opt-in (``decode_weight_dtype="mxfp4"``); on a GPU
tensor the HIP kernel is the only implementation and a shape outside its contract raises. The
weight is quantised once, in torch on its own device (there is no HIP quantiser), before any
graph capture.
"""

from __future__ import annotations

import ctypes
import weakref
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check
from .fp8 import _epilogue_torch, _want_hip
from .gemm import ACTS, EPI_BIAS, EPI_RESIDUAL, _HIP_INVALID_VALUE, _num_cus

BLOCK = 32                                # k elements per e8m0 scale
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
SCALE_MIN, SCALE_MAX = 2, 252             # the range of emitted scale bytes (module docstring)
_CHUNK_ELEMS = 1 << 22                    # fp32 temporaries of the quantiser: 16 MiB each

W4_LAUNCHES = {"count": 0}                # launches of the W4 skinny kernel itself

_W4_CONTRACT = ("contract: 1 <= M <= 16, N % 16 == 0, K % 128 == 0; there is no fall-back to "
                "bf16")
_W4_PLANS = {}


def _quantize_rows(xf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 ``[n, K]`` -> (codes ``[n, K/2]``, scales ``[n, K/32]``), both uint8."""
    n, K = xf.shape
    xb = xf.reshape(n, K // BLOCK, BLOCK)
    amax = xb.abs().amax(dim=-1)
    _, e = torch.frexp(amax)                                  # amax = m * 2^e, m in [0.5, 1)
    b = (e.to(torch.int32) - 1 - 2 + 127).clamp_(2, 254)      # floor(log2(amax)) = e - 1
    b = torch.where(amax == 0, torch.full_like(b, 127), b)
    scale = (b << 23).view(torch.float32)                     # 2^(b-127), b >= 1
    a = (xb.abs() / scale.unsqueeze(-1)).clamp_(max=6.0)
    # nearest grid value, ties to the even code: the grid's step is 0.5 below 2, 1 below 4, 2
    # above, and torch.round is round-half-even
    code = torch.where(a < 2, torch.round(a * 2),
                       torch.where(a < 4, torch.round(a) + 2, torch.round(a * 0.5) + 4))
    code = code.to(torch.uint8) | ((xb < 0).to(torch.uint8) << 3)
    code = code.reshape(n, K // 2, 2)
    return code[..., 0] | (code[..., 1] << 4), b.to(torch.uint8)


def quantize_mxfp4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``w [N, K]`` -> ``(codes uint8 [N, K/2], scales uint8 [N, K/32])`` on ``w``'s device
    (module docstring for the exact semantics). ``K % 32 == 0``. Runs in torch, in row chunks
    that bound the fp32 temporaries."""
    if w.dim() != 2 or w.shape[1] % BLOCK or w.shape[1] == 0:
        raise ValueError(f"quantize_mxfp4: a [N, K] matrix with K % {BLOCK} == 0, got "
                         f"{tuple(w.shape)}")
    N, K = w.shape
    codes = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device)
    scales = torch.empty(N, K // BLOCK, dtype=torch.uint8, device=w.device)
    rows = max(1, _CHUNK_ELEMS // K)
    for r0 in range(0, N, rows):
        c, s = _quantize_rows(w[r0:r0 + rows].float())
        codes[r0:r0 + rows] = c
        scales[r0:r0 + rows] = s
    return codes, scales


def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """``(codes [N, K/2], scales [N, K/32])`` -> fp32 ``[N, K]``, exactly."""
    if codes.dtype != torch.uint8:
        codes = codes.view(torch.uint8)
    if scales.dtype != torch.uint8:
        scales = scales.view(torch.uint8)
    N, K = codes.shape[0], codes.shape[1] * 2
    if scales.shape != (N, K // BLOCK) or K % BLOCK:
        raise ValueError(f"dequantize_mxfp4: codes{tuple(codes.shape)} vs "
                         f"scales{tuple(scales.shape)}")
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32,
                       device=codes.device)
    nib = torch.stack((codes & 15, codes >> 4), dim=-1).reshape(N, K // BLOCK, BLOCK)
    v = lut[nib.long()]
    return torch.ldexp(v, (scales.to(torch.int32) - 127).unsqueeze(-1)).reshape(N, K)


# Quantised weights, one entry per weight storage: data_ptr -> (weak reference to the tensor,
# its _version, shape, codes, scales). The rules of fp8._WCACHE, whose entries are e4m3.
_W4CACHE = {}


def quantize_weight_mxfp4(w: torch.Tensor):
    """``(codes, scales)`` of a Linear weight ``[N, K]``, cached until the weight changes
    (``_version``) or moves (``data_ptr``)."""
    key = w.data_ptr()
    try:
        version = w._version
    except RuntimeError:        # an inference tensor has no version counter: never cached
        return quantize_mxfp4(w.detach())
    ent = _W4CACHE.get(key)
    if ent is not None:
        ref, ver, shape, codes, scales = ent
        if ref() is w and ver == version and shape == tuple(w.shape):
            return codes, scales
    if torch.cuda.is_available() and w.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("mxfp4: a weight must be quantised before HIP-graph capture (run one "
                           "eager forward first)")
    codes, scales = quantize_mxfp4(w.detach())

    def _drop(ref, key=key):            # the weight died: free its quantised copy
        ent = _W4CACHE.get(key)
        if ent is not None and ent[0] is ref:
            del _W4CACHE[key]

    _W4CACHE[key] = (weakref.ref(w, _drop), version, tuple(w.shape), codes, scales)
    return codes, scales


def clear_weight_cache() -> None:
    _W4CACHE.clear()


def w4_contract_error(M: int, N: int, K: int) -> Optional[str]:
    """Why (M, N, K) is outside the W4 skinny GEMM's shape contract, or None."""
    if M <= 0 or N <= 0 or K <= 0:
        return "empty operand"
    if M > 16:
        return f"M = {M} is larger than 16"
    if N % 16:
        return f"N = {N} is not a multiple of 16"
    if K % 128:
        return f"K = {K} is not a multiple of 128"
    return None


def w4_skinny_plan(M: int, N: int, K: int, ncu: int):
    """(grid, K-split inside a workgroup, K-split across workgroups, workspace bytes) of the W4
    skinny GEMM (``dlbb_gemm_w4_skinny_plan``), or None outside its shape contract."""
    key = (int(M), int(N), int(K), int(ncu))
    if key not in _W4_PLANS:
        out = (ctypes.c_int64 * 4)()
        ok = _lib.lib().dlbb_gemm_w4_skinny_plan(*key, out)
        _W4_PLANS[key] = tuple(int(v) for v in out) if ok else None
    return _W4_PLANS[key]


def _w4_refusal(x2, codes, scales, out, M, N, K) -> str:
    """Names the term of the C contract a refused call violated (the slow path of a refusal)."""
    why = w4_contract_error(M, N, K)
    if why:
        return why
    if M > 1 and (x2.stride(0) % 8 or x2.stride(0) < K):
        return f"x row stride {x2.stride(0)} is not a multiple of 8 elements >= K"
    if N > 1 and (codes.stride(0) % 16 or codes.stride(0) < K // 2):
        return f"codes row stride {codes.stride(0)} is not a multiple of 16 bytes >= K / 2"
    for name, t in (("x", x2), ("codes", codes), ("out", out)):
        if t.data_ptr() % 16:
            return f"{name} is not 16-byte aligned"
    if scales.data_ptr() % 4:
        return "scales is not 4-byte aligned"
    return "refused by the kernel's entry point"


def linear_w4(x: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor,
              bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
              residual: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.bfloat16,
              out: Optional[torch.Tensor] = None, kernels: Optional[str] = None) -> torch.Tensor:
    """``act(x @ dequantize_mxfp4(codes, scales).T + bias) + residual``: weight-only MXFP4 for
    the M = batch rows of a decode step. ``x [..., K]`` bf16, ``codes [N, K/2]`` uint8 (unit
    column stride; ``torch.float4_e2m1fn_x2`` is taken too), ``scales [N, K/32]`` uint8,
    contiguous, ``bias [N]`` / ``residual [..., N]`` bf16; fp32 accumulation, bf16 or fp32 result
    ``[..., N]``.

    HIP contract: ``1 <= M <= 16`` (M = rows of ``x``), ``N % 16 == 0``, ``K % 128 == 0``,
    16-byte aligned rows of ``x`` and ``codes``. Anything else raises ``ValueError`` before any
    launch. As in :func:`~.fp8.linear_w8`, dtypes and unit strides are checked here, shape,
    leading dimensions and alignment by the C entry point, which launches nothing outside the
    contract; only then is the violated term worked out."""
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    K = x.shape[-1]
    N = codes.shape[0]
    if codes.dtype != torch.uint8 and "float4_e2m1fn_x2" in str(codes.dtype):
        codes = codes.view(torch.uint8)
    if codes.dim() != 2 or codes.shape[1] * 2 != K:
        raise ValueError(f"linear_w4: x[..., {K}] vs codes{tuple(codes.shape)} (two codes per "
                         "byte)")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("linear_w4: out_dtype must be bf16 or fp32")
    lead = x.shape[:-1]
    x2 = x if x.dim() == 2 else x.reshape(-1, K)
    M = x2.shape[0]
    if K % BLOCK or scales.dim() != 2 or tuple(scales.shape) != (N, K // BLOCK):
        raise ValueError(f"linear_w4: scales must be [N, K / {BLOCK}] = [{N}, {K // BLOCK}], "
                         f"got {tuple(scales.shape)}")
    if not _want_hip(kernels, x, codes):
        y = x2.float() @ dequantize_mxfp4(codes, scales).t()
        y = _epilogue_torch(y, bias, act, None if residual is None else residual.reshape(M, N),
                            out_dtype).reshape(*lead, N)
        return y if out is None else out.copy_(y.reshape(out.shape))
    if x.dtype != torch.bfloat16 or codes.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise ValueError(f"linear_w4: x must be bf16, codes and scales uint8; got {x.dtype} / "
                         f"{codes.dtype} / {scales.dtype}")
    if x2.stride(1) != 1 or codes.stride(1) != 1:
        raise ValueError("linear_w4: operands must be K-contiguous")
    if not scales.is_contiguous():
        raise ValueError("linear_w4: scales must be contiguous")
    if out is None:
        out = torch.empty(*lead, N, dtype=out_dtype, device=x.device)
    elif out.dtype not in (torch.bfloat16, torch.float32) or not out.is_contiguous() \
            or out.numel() != M * N:
        raise ValueError("linear_w4: out must be contiguous bf16/fp32 [..., N]")
    epi = ACTS[act]
    if bias is not None:
        if bias.dtype != torch.bfloat16 or bias.numel() != N or not bias.is_contiguous():
            raise ValueError("linear_w4: bias must be contiguous bf16 [N]")
        epi |= EPI_BIAS
    r2 = None
    if residual is not None:
        r2 = residual.reshape(M, N)
        if r2.dtype != torch.bfloat16 or r2.stride(1) != 1:
            r2 = r2.to(torch.bfloat16).contiguous()
        epi |= EPI_RESIDUAL
    dev = x.device
    rc = _lib.lib().dlbb_gemm_w4_nt_skinny(
        x2.data_ptr(), x2.stride(0) if M > 1 else K, codes.data_ptr(),
        codes.stride(0) if N > 1 else K // 2, scales.data_ptr(), out.data_ptr(), M, N, K,
        _lib.ptr(bias), _lib.ptr(r2), r2.stride(0) if r2 is not None else 0, epi,
        1 if out.dtype == torch.float32 else 0, _num_cus(dev), _lib.stream(dev))
    if rc == 0:
        W4_LAUNCHES["count"] += 1
        return out
    if rc == _HIP_INVALID_VALUE:
        raise ValueError(f"linear_w4: {_w4_refusal(x2, codes, scales, out, M, N, K)} "
                         f"({_W4_CONTRACT})")
    check(rc, "gemm_w4_nt_skinny")


def w4_linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
              act: Optional[str] = None, residual: Optional[torch.Tensor] = None,
              out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
              kernels: Optional[str] = None) -> torch.Tensor:
    """``act(x @ w.T + bias) + residual`` with the bf16 weight ``w [N, K]`` streamed as MXFP4:
    quantised once (:func:`quantize_weight_mxfp4`; before any graph capture), the bf16 activation
    ``x [..., K]`` as it is."""
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in (torch.bfloat16, torch.float32) else torch.bfloat16
    if w.shape[1] != x.shape[-1]:
        raise ValueError(f"w4_linear: x[..., {x.shape[-1]}] vs w{tuple(w.shape)}")
    if _want_hip(kernels, x, w):            # refuse before the quantiser launches anything
        M = x.numel() // max(x.shape[-1], 1)
        why = w4_contract_error(M, w.shape[0], x.shape[-1])
        if why:
            raise ValueError(f"w4_linear: {why} ({_W4_CONTRACT})")
    codes, scales = quantize_weight_mxfp4(w)
    return linear_w4(x, codes, scales, bias, act, residual, out_dtype, out, kernels=kernels)
