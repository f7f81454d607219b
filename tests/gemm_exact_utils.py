"""Shared pieces of the exact training-GEMM tests (``test_gemm_exact_gpu.py`` on the GPU,
``test_gemm_exact_cpu.py`` for the pieces themselves): integer operand generators, the exact
comparator, the kernel-id table of ``csrc/gemm.hip`` and the shape table.

Operands are small integers, so every product and every partial sum is an integer below 2^24:
fp32 accumulation is exact in ANY order, the fp32 output must equal the fp64 product bit for bit
and the bf16 output must be its one rounding. Nothing here depends on a GPU."""

import torch

BF16 = torch.bfloat16

# ids of csrc/gemm.hip's GemmKernelId (dlbb_gemm_last_kernel) and the name
# dlbb_gemm_kernel_name gives each
KID = {
    "nt_128": 1, "nt_256_deep": 2, "nt_256_pp": 3, "nt_256_pp_bal": 4, "nt_192_pp": 5,
    "nt_192_pp_bal": 6, "nt_192_spread": 7, "nt_192_spread_bal": 8, "nt_256_streamk": 9,
    "nt_256_streamk_bal": 10, "nn_256_pp": 11, "nn_256_pp_bal": 12, "tn_256_pp": 13,
    "tn_256_pp_bal": 14,
    "nt_256_persist_plain": 16, "nt_256_persist_bias": 17, "nt_256_persist_gelu_tanh": 18,
    "nt_256_persist_gelu_erf": 19,
    "nt_256_persist_bal_plain": 24, "nt_256_persist_bal_bias": 25,
    "nt_256_persist_bal_gelu_tanh": 26, "nt_256_persist_bal_gelu_erf": 27,
    "nn_256_persist_bal_plain": 32, "nn_256_persist_bal_dgelu_tanh": 36,
    "nn_256_persist_bal_dgelu_erf": 37,
    # stamped diagnostic twins of the six ping-pong kernels: the kernel's id + 64
    "nt_256_pp_st": 67, "nt_256_pp_bal_st": 68, "nn_256_pp_st": 75, "nn_256_pp_bal_st": 76,
    "tn_256_pp_st": 77, "tn_256_pp_bal_st": 78,
}
KNAME = {
    1: "gemm_bf16_nt_kernel", 2: "gemm_bf16_nt_256_deep", 3: "gemm_bf16_nt_256_pingpong3",
    4: "gemm_bf16_nt_256_pingpong3_bal", 5: "gemm_bf16_nt_192_pingpong3",
    6: "gemm_bf16_nt_192_pingpong3_bal", 7: "gemm_bf16_nt_192_pp_spread",
    8: "gemm_bf16_nt_192_pp_spread_bal", 9: "gemm_bf16_nt_256_streamk",
    10: "gemm_bf16_nt_256_streamk_bal", 11: "gemm_bf16_nn_256_pingpong3",
    12: "gemm_bf16_nn_256_pingpong3_bal", 13: "gemm_bf16_tn_256_pingpong3",
    14: "gemm_bf16_tn_256_pingpong3_bal",
    16: "gemm_bf16_nt_256_pp_persist<plain>", 17: "gemm_bf16_nt_256_pp_persist<bias>",
    18: "gemm_bf16_nt_256_pp_persist<bias_gelu_tanh>",
    19: "gemm_bf16_nt_256_pp_persist<bias_gelu_erf>",
    24: "gemm_bf16_nt_256_pp_persist_bal<plain>", 25: "gemm_bf16_nt_256_pp_persist_bal<bias>",
    26: "gemm_bf16_nt_256_pp_persist_bal<bias_gelu_tanh>",
    27: "gemm_bf16_nt_256_pp_persist_bal<bias_gelu_erf>",
    32: "gemm_bf16_nn_256_pp_persist_bal<plain>",
    36: "gemm_bf16_nn_256_pp_persist_bal<dgelu_tanh>",
    37: "gemm_bf16_nn_256_pp_persist_bal<dgelu_erf>",
    67: "gemm_bf16_nt_256_pingpong3_st", 68: "gemm_bf16_nt_256_pingpong3_bal_st",
    75: "gemm_bf16_nn_256_pingpong3_st", 76: "gemm_bf16_nn_256_pingpong3_bal_st",
    77: "gemm_bf16_tn_256_pingpong3_st", 78: "gemm_bf16_tn_256_pingpong3_bal_st",
}


# ------------------------------------------------------------------------------- operands

def _idx(R, C, device, r0=0):
    r = torch.arange(r0, r0 + R, device=device, dtype=torch.int64).view(R, 1)
    c = torch.arange(C, device=device, dtype=torch.int64).view(1, C)
    return r, c


def int_a(R, K, device="cpu", r0=0):
    """[R, K] integers in [-3, 4]: varies with (row, k); the ``(row >> (k % 17)) & 1`` term
    carries 17 bits of the row index, so rows stay distinct far past the arithmetic terms'
    common period."""
    m, k = _idx(R, K, device, r0)
    v = (m * 7 + k * 3 + (m * k) % 5 + ((m >> (k % 17)) & 1) * 3 + (m // 40) % 7) % 8 - 3
    return v.to(BF16)


def int_b(R, K, device="cpu", r0=0):
    """[R, K] integers in [-3, 4], asymmetric in (row, k) and unrelated to :func:`int_a`."""
    n, k = _idx(R, K, device, r0)
    v = (n * 5 + k * 11 + n // 3 + (n * k) % 7 + ((n >> (k % 17)) & 1) * 5) % 8 - 3
    return v.to(BF16)


def _no_zero_group(v, r, k):
    """One position per 8-wide k-group (it moves with the row and the group) is made non-zero,
    so no group of any row drops out of the product."""
    g = r + k // 8
    return torch.where((k % 8 == g % 8) & (v == 0), 1 - 2 * (g & 1), v)


def tern_a(R, K, device="cpu", r0=0):
    """[R, K] values in {-1, 0, 1} (the bf16-slab weight-gradient cases)."""
    m, k = _idx(R, K, device, r0)
    v = (m + k * 2 + (m * k) % 5 + ((m >> (k % 17)) & 1) + (m // 15) % 2) % 3 - 1
    return _no_zero_group(v, m, k).to(BF16)


def tern_b(R, K, device="cpu", r0=0):
    n, k = _idx(R, K, device, r0)
    v = (n * 2 + k + n // 3 + (n * k) % 7 + ((n >> (k % 17)) & 1) * 2) % 3 - 1
    return _no_zero_group(v, n, k).to(BF16)


def int_bias(N, device="cpu"):
    """[N] integers in [-8, 8]."""
    n = torch.arange(N, device=device, dtype=torch.int64)
    return ((n * 5 + n // 7) % 17 - 8).to(BF16)


def int_res(M, N, device="cpu", salt=0):
    """[M, N] integers in [-8, 8] (a residual, or the previous value of an accumulated
    output)."""
    m, n = _idx(M, N, device)
    return ((m * 3 + n * 7 + (m * n) % 11 + salt) % 17 - 8).to(BF16)


def rand_bf16(*shape, seed, device="cpu"):
    """Uniform [-1, 1) bf16."""
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.rand(*shape, generator=g, device=device) * 2 - 1).to(BF16)


def exact_ok(amax, bmax, K):
    """Every partial sum of K products |a| <= amax, |b| <= bmax (plus an epilogue term <= 16)
    is an integer below 2^24, i.e. exact in fp32."""
    return amax * bmax * K + 16 < 2 ** 24


def ref_product(a, b, chunk_bytes=1 << 30):
    """fp64 ``a @ b^T`` for a [R, K], b [C, K]; the fp64 copy of ``a`` is made in row chunks
    of at most ``chunk_bytes``."""
    R, K = a.shape
    bd = b.double().t().contiguous()
    rows = max(1, min(R, chunk_bytes // (8 * K)))
    if rows >= R:
        return a.double() @ bd
    out = torch.empty(R, b.shape[0], dtype=torch.float64, device=a.device)
    for r0 in range(0, R, rows):
        out[r0:r0 + rows] = a[r0:r0 + rows].double() @ bd
    return out


# ----------------------------------------------------------------------------- comparator

def mismatch_report(got, want, tile=(256, 256)):
    """None when ``got`` equals ``want`` element for element (as ``torch.equal``: same dtype
    and shape, NaN never equal); else a dict: ``count``, ``first`` = (row, col), ``got``,
    ``want`` at it, and ``tiles`` = ((row tile lo, hi), (col tile lo, hi)), the bounding box
    of the wrong elements in units of ``tile``."""
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    g2 = got.reshape(-1, got.shape[-1]) if got.dim() != 2 else got
    w2 = want.reshape(-1, want.shape[-1]) if want.dim() != 2 else want
    bad = ~(g2 == w2)                                    # NaN != anything
    if not bool(bad.any()):
        return None
    idx = bad.nonzero()
    r, c = int(idx[0, 0]), int(idx[0, 1])
    rows, cols = idx[:, 0], idx[:, 1]
    tm, tn = tile
    return {
        "count": int(idx.shape[0]),
        "first": (r, c),
        "got": float(g2[r, c]),
        "want": float(w2[r, c]),
        "tiles": ((int(rows.min()) // tm, int(rows.max()) // tm),
                  (int(cols.min()) // tn, int(cols.max()) // tn)),
    }


def assert_exact(got, want, tile=(256, 256), what=""):
    rep = mismatch_report(got, want, tile)
    if rep is None:
        return
    (r0, r1), (c0, c1) = rep["tiles"]
    raise AssertionError(
        f"{what}: {rep['count']} of {got.numel()} elements wrong; first at {rep['first']}: got "
        f"{rep['got']!r}, want {rep['want']!r}; wrong elements lie in {tile[0]} x {tile[1]} "
        f"tiles rows {r0}..{r1}, cols {c0}..{c1}")


def assert_within(out, ref, bound, what=""):
    """Every element of |out - ref| within its own ``bound``; prints the worst ratio."""
    err = (out.double() - ref).abs()
    ratio = float((err / bound).max())
    print(f"{what}: max err/bound {ratio:.3f}")
    assert bool((err <= bound).all()), (what, ratio)
    return ratio


# ---------------------------------------------------------------------------- shape table

def persist_shape(ncu):
    """(M, N) of the persistent cases: 17 row blocks (the last one of 8 rows) x enough column
    blocks that the 256^2 tiles exceed the CUs, so workgroups loop."""
    return 256 * 17 - 248, 256 * -(-(ncu + 16) // 17)


def spread_shape(ncu):
    """(M, N) of the looping 192-spread case: M % 16 == 0 with a ragged last row block,
    N = 17 x 192, tiles > ncu."""
    return 256 * -(-(ncu + 16) // 17) - 240, 192 * 17


def wgrad_per(M, split):
    """Rows per split-K slice of the weight-gradient kernel (``wgrad_launch``) and the number
    of slices it really runs."""
    per = max(-(-(M // split) // 32) * 32, 32)
    return per, -(-M // per)


def streamk_contributors(M, N, K, plan):
    """Number of Stream-K ranges that meet each 256^2 tile's K-loop, from (grid, L, ...)."""
    grid, L = plan[0], plan[1]
    tiles = -(-M // 256) * -(-N // 256)
    nk = K // 64
    out = []
    for t in range(tiles):
        lo, hi = t * nk, (t + 1) * nk - 1
        out.append(hi // L - lo // L + 1)
    assert grid == -(-tiles * nk // L)
    return out


def shapes(ncu):
    """The shape table: per path the (M, N, K[, extra]) cases; reduction length last. For the
    weight gradients (tn_*, wgrad*) the tuple is (T, N, K): T tokens reduced, dW is [N, K]."""
    pm, pn = persist_shape(ncu)
    sm, sn = spread_shape(ncu)
    return {
        "nt_128": [(200, 136, 64), (264, 331, 320)],
        "nt_256_deep": [(264, 328, 64), (264, 331, 320)],
        "nt_256_pp": [(8, 64, 64), (264, 320, 192), (520, 576, 2112)],
        "nt_persist": [(pm, pn, 128), (pm, pn, 192)],
        "nt_192": [(8, 192, 64), (264, 384, 320)],
        "nt_192_spread": [(272, 384, 384), (sm, sn, 384), (sm, sn, 448)],
        "nt_streamk": [(520, 256, 704), (2560, 2560, 1536)],
        "nt_split": [(264, 320, 1088), (264, 384, 1088)],
        "nt_split_c": [(264, 320, 448, 3), (264, 384, 448, 3), (264, 320, 640, 7),
                       (264, 384, 640, 7)],
        "nn_256_pp": [(8, 256, 64), (264, 512, 192)],
        "nn_split": [(264, 256, 448, 3), (264, 256, 640, 7)],
        "nn_persist": [(pm, pn, 128)],
        "tn_256_pp": [(64, 128, 256), (192, 384, 512)],
        "tn_split": [(640, 256, 256, 0, 7), (512, 384, 256, 128, 2)],   # (T, N, K, r0, split)
        "tn_tail": [(1024, (ncu + 44) * 256, 256)],
        "wgrad": [(32, 256, 256), (96, 256, 256), (352, 256, 512)],
        "wgrad_fused": [(352, 256, 512, 3)],
    }


WGRAD_SPLITS = (None, 1, 3)
WGRAD_TILES = {"mfma": (128, 128), "mfma256": (256, 128), "mfma_wide": (128, 256)}

# path -> the reduction length's position is always index 2 except the weight gradients (0)
REDUCTION_AT = {k: 2 for k in ("nt_128", "nt_256_deep", "nt_256_pp", "nt_persist", "nt_192",
                               "nt_192_spread", "nt_streamk", "nt_split", "nt_split_c",
                               "nn_256_pp", "nn_split", "nn_persist")}
REDUCTION_AT.update({k: 0 for k in ("tn_256_pp", "tn_split", "tn_tail", "wgrad", "wgrad_fused")})
