"""Global gradient-norm clipping on flat gradient buffers (``csrc/grad_clip.hip``).

The reference never clips (DeepSpeed's engine in its smoke tests runs with the default
``gradient_clipping = 0``); every GPT-2 recipe does (llm.c, nanoGPT: global L2 norm at 1.0). Here
the norm is three device-side pieces and no host sync:

* :func:`grad_sumsq` — one read-only pass over a contiguous bf16 / fp32 range, one fp32 partial
  per workgroup in that range's slots (fixed reduction order: bit-identical from run to run);
* :func:`clip_coef` — one workgroup turns the partials into ``[norm, coef, sum]`` in device
  memory, ``coef = min(max_norm / (norm + 1e-6), 1)`` as ``torch.nn.utils.clip_grad_norm_``;
* :class:`~.optim.FlatAdamW` reads ``coef`` on the device (``step(coef_dev=...)``).

CPU tensors and ``DLBB_KERNELS=torch`` use the same formulas in torch.
"""

from __future__ import annotations

import ctypes
from typing import List, Optional

import torch

from . import _lib
from ._lib import check, dt, use_hip

_TORCH_SLOTS = 1     # the torch path keeps a range's whole sum in slot 0


def sumsq_plan(n: int) -> dict:
    """Launch geometry of the sum-of-squares kernel for ``n`` elements (a function of ``n``
    alone): ``grid`` workgroups of ``block`` threads, ``unroll`` 8-element vectors per thread
    and grid sweep, ``slots`` partials per range."""
    out = (ctypes.c_int * 4)()
    check(_lib.lib().dlbb_grad_sumsq_plan(int(n), out), "grad_sumsq_plan")
    return {"grid": out[0], "block": out[1], "unroll": out[2], "slots": out[3]}


def _check_range(g: torch.Tensor) -> None:
    if g.dtype not in (torch.bfloat16, torch.float32) or g.dim() != 1 or not g.is_contiguous():
        raise ValueError("gradient range must be a contiguous 1-D bf16 or fp32 tensor")


@torch.no_grad()
def grad_sumsq(g: torch.Tensor, partials: torch.Tensor) -> torch.Tensor:
    """Sum of squares of ``g`` into the fp32 row ``partials`` (every slot is written; their sum
    is the result), on the current stream."""
    _check_range(g)
    if partials.dtype != torch.float32 or partials.dim() != 1 or not partials.is_contiguous():
        raise ValueError("partials must be a contiguous 1-D fp32 tensor")
    if use_hip(g, partials):
        check(_lib.lib().dlbb_grad_sumsq(g.data_ptr(), dt(g), g.numel(), partials.data_ptr(),
                                         partials.numel(), _lib.stream(g.device)), "grad_sumsq")
    else:
        partials.zero_()
        partials[0] = g.float().square().sum()
    return partials


@torch.no_grad()
def clip_coef(partials: torch.Tensor, pre_scale: float, max_norm: float,
              out: torch.Tensor) -> torch.Tensor:
    """``out[0:3] = [norm, coef, sum]`` from the fp32 ``partials``: ``norm = sqrt(sum) *
    pre_scale``, ``coef = min(max_norm / (norm + 1e-6), 1)``; a non-finite norm gives NaN for
    both. ``partials`` may be ``out[2:3]`` (an already reduced sum)."""
    if (partials.dtype != torch.float32 or out.dtype != torch.float32 or out.numel() < 3
            or not partials.is_contiguous() or not out.is_contiguous() or partials.numel() < 1):
        raise ValueError("clip_coef needs contiguous fp32 partials (>= 1) and out[3]")
    if use_hip(partials, out):
        check(_lib.lib().dlbb_clip_coef(partials.data_ptr(), partials.numel(), float(pre_scale),
                                        float(max_norm), out.data_ptr(),
                                        _lib.stream(out.device)), "clip_coef")
    else:
        total = partials.reshape(-1).sum()
        norm = total.sqrt() * float(pre_scale)
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)       # clamp keeps a NaN
        nan = torch.full_like(norm, float("nan"))
        bad = ~torch.isfinite(norm)
        out[0] = torch.where(bad, nan, norm)
        out[1] = torch.where(bad, nan, coef)
        out[2] = total
    return out


class GradClipper:
    """Global-norm clip state of one trainer: ``partials[n_ranges, slots]`` and ``out[3]``.

    Per step: ``accumulate(i, range_i)`` once for every range (any stream order the caller
    arranges; each call runs on the current stream), then ``finish(pre_scale)`` on a stream
    ordered after all of them. ``finish`` returns the device coefficient (a 1-element fp32
    tensor for ``FlatAdamW.step(coef_dev=...)``); ``norm`` is a device scalar holding the last
    finished step's norm, before clipping. Nothing here synchronises with the host."""

    def __init__(self, n_ranges: int, max_norm: float, device):
        if n_ranges < 1:
            raise ValueError("GradClipper needs at least one range")
        if not max_norm > 0:
            raise ValueError(f"max_norm must be > 0, got {max_norm}")
        dev = torch.device(device)
        self.max_norm = float(max_norm)
        hip = dev.type == "cuda" and not _lib.force_torch()
        self.slots = sumsq_plan(0)["slots"] if hip else _TORCH_SLOTS
        # zeroed once; afterwards every accumulate() rewrites all of its range's slots
        self.partials = torch.zeros(n_ranges, self.slots, dtype=torch.float32, device=dev)
        self.out = torch.zeros(3, dtype=torch.float32, device=dev)
        self.norm = self.out[0]
        self.coef = self.out[1:2]
        self._done: List[bool] = [False] * n_ranges

    def reset(self) -> None:
        """Forget what was accumulated (start of a step; a step that raised leaves flags set)."""
        self._done = [False] * len(self._done)

    def accumulate(self, i: int, grad_range: torch.Tensor) -> None:
        if self._done[i]:
            raise RuntimeError(f"gradient range {i} accumulated twice in one step")
        grad_sumsq(grad_range, self.partials[i])
        self._done[i] = True

    def finish(self, pre_scale: float, group=None) -> torch.Tensor:
        """Norm and coefficient of the accumulated ranges. ``pre_scale`` scales the norm (1/world
        when the buffers hold sums over ranks). ``group``: the ranges are this rank's disjoint
        shard — the sum of squares is all-reduced over the group (one float) first."""
        missing = [i for i, d in enumerate(self._done) if not d]
        if missing:
            raise RuntimeError(f"gradient ranges {missing} were not accumulated this step: the "
                               "norm would silently miss them")
        self._done = [False] * len(self._done)
        flat = self.partials.view(-1)
        if group is None:
            clip_coef(flat, pre_scale, self.max_norm, self.out)
        else:
            import torch.distributed as dist

            clip_coef(flat, 1.0, self.max_norm, self.out)      # out[2] = this rank's sum
            dist.all_reduce(self.out[2:3], group=group)
            clip_coef(self.out[2:3], pre_scale, self.max_norm, self.out)
        return self.coef


def check_coef(coef_dev: Optional[torch.Tensor], like: torch.Tensor) -> None:
    if coef_dev is None:
        return
    if (coef_dev.dtype != torch.float32 or coef_dev.numel() != 1
            or coef_dev.device != like.device):
        raise ValueError("coef_dev must be one fp32 element on the optimizer's device")
