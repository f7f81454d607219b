"""Python entry points of the gfx950 HIP kernel library (``csrc/`` -> ``_dlbb_hip.so``).

* :mod:`.elementwise` — n-way sum-reduce, cast, strided pack, multi-tensor chunk copy
  (flatten/unflatten/all-to-all packing).
* :mod:`.gemm` — MFMA bf16 GEMM with fused bias / GELU / residual epilogues.
* :mod:`.fp8` — e4m3 row quantiser and FP8 GEMM (block-scaled MFMA), the opt-in FP8 TP forward;
  the weight-only FP8 (W8A16) skinny GEMM of the opt-in FP8-weight decode step.
* :mod:`.mxfp4` — MXFP4 (e2m1 codes, e8m0 block scales) weight quantiser and the weight-only
  MXFP4 (W4A16) skinny GEMM of the opt-in MXFP4-weight decode step.
* :mod:`.norm_act` — fused residual+LayerNorm and bias+GELU (fwd + bwd, autograd).
* :mod:`.optim` — flat fused AdamW.
* :mod:`.clip` — global gradient-norm clipping: bucket sum-of-squares, device-side coefficient.
* :mod:`.xent` — fused softmax cross-entropy on bf16 logits; LM-head-fused linear + loss.
* :mod:`.decode` — KV cache (bf16, or opt-in e4m3 codes with one fp32 scale per row), append, and
  single-query (decode) attention split over the keys.
* :mod:`.embedding` — token + position embedding, backward accumulating in place (sinks).
* :mod:`._lib` — loader; ``available()``, ``loaded_path()``.
"""

from . import _lib
from ._lib import available, loaded_path, KernelError
from .elementwise import reduce_sum, cast, pack_rows, ChunkTable, ScaleTable, flatten_into
from .gemm import linear
from .fp8 import quantize_rows, linear_fp8, fp8_linear, linear_w8, w8_linear, W8_LAUNCHES
from .mxfp4 import (quantize_mxfp4, dequantize_mxfp4, quantize_weight_mxfp4, linear_w4,
                    w4_linear, w4_contract_error, w4_skinny_plan, W4_LAUNCHES)
from .norm_act import layernorm, bias_gelu
from .optim import FlatAdamW
from .clip import GradClipper, grad_sumsq, clip_coef, sumsq_plan
from .xent import cross_entropy, linear_cross_entropy
from .attention import causal_attention
from .decode import KVCache, kv_append, decode_attention, CHUNK, CHUNK_FP8, PAGE_SIZE, PAGE_SIZES
from .embedding import embedding

__all__ = ["KVCache", "kv_append", "decode_attention", "CHUNK", "CHUNK_FP8", "PAGE_SIZE", "PAGE_SIZES", "causal_attention", "available", "loaded_path", "KernelError", "reduce_sum", "cast", "pack_rows",
           "ChunkTable", "ScaleTable", "flatten_into", "linear", "layernorm", "bias_gelu",
           "FlatAdamW", "cross_entropy", "linear_cross_entropy", "embedding", "quantize_rows",
           "linear_fp8", "fp8_linear", "linear_w8", "w8_linear", "W8_LAUNCHES",
           "quantize_mxfp4", "dequantize_mxfp4", "quantize_weight_mxfp4", "linear_w4",
           "w4_linear", "w4_contract_error", "w4_skinny_plan", "W4_LAUNCHES", "GradClipper",
           "grad_sumsq", "clip_coef", "sumsq_plan"]
