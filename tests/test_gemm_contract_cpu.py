"""Out-of-contract calls to the bf16 GEMM entry points of ``csrc/gemm.hip``: every launcher must
refuse them with ``hipErrorInvalidValue`` before its first HIP runtime call, launching nothing
(``dlbb_gemm_last_kernel()`` unchanged). Needs no GPU: the pointers are fake addresses that a
refused call never touches. Each row is one entry point's in-contract call (``BASE``) with the
named fields replaced, so the named violation is the only reason for the refusal; NO row may be
inside a contract, because that call would launch on the fake pointers. Empty problems
(``M == 0`` / ``N == 0``) return success, also without a launch."""

import pytest

from distributed_llm_backend_benchmark_amd.ops import _lib

OK, BAD = 0, 1                       # hipSuccess, hipErrorInvalidValue
P, ODD = 0x10000, 0x10008            # a 16-byte aligned and a misaligned (fake) address
NCU = 256

# argument order of each C entry point (the stream, always null here, is appended)
ARGS = {
    "nt_v": ("A", "lda", "B", "ldb", "C", "ldc", "M", "N", "K", "bias", "residual", "ldr",
             "preact", "epi", "out_f32", "variant"),
    "nt_streamk": ("A", "lda", "B", "ldb", "C", "ldc", "M", "N", "K", "bias", "residual", "ldr",
                   "preact", "epi", "out_f32", "ncu", "ws", "ws_bytes", "cnt", "ncnt"),
    "nn": ("A", "lda", "B", "ldb", "C", "ldc", "M", "N", "K", "bias", "residual", "ldr",
           "preact", "epi", "out_f32", "split", "ws"),
    "nt_split": ("A", "lda", "B", "ldb", "C", "ldc", "M", "N", "K", "split", "tile192", "ws",
                 "ws_bytes"),
    "tn": ("A", "lda", "B", "ldb", "C", "ldc", "M", "N", "K", "residual", "ldr", "epi",
           "out_f32", "split", "ws"),
    "nt_phase_probe": ("A", "lda", "B", "ldb", "C", "M", "N", "K", "nj", "recs"),
}
FN = {"nt_v": "dlbb_gemm_bf16_nt_v", "nt_streamk": "dlbb_gemm_bf16_nt_streamk",
      "nn": "dlbb_gemm_bf16_nn", "nt_split": "dlbb_gemm_bf16_nt_split",
      "tn": "dlbb_gemm_bf16_tn", "nt_phase_probe": "dlbb_gemm_nt_phase_probe"}

_PTRS = dict(A=P, B=P, C=P, bias=None, residual=None, ldr=0, preact=None, epi=0, out_f32=0)
# the in-contract call each row starts from (never made as it stands)
BASE = {
    "nt_v": dict(_PTRS, lda=64, ldb=64, ldc=64, M=64, N=64, K=64, variant=0),
    # one 256² tile x 16 K-tiles: plan = (grid 2, L 8, 1 MiB of partials, 8 counters)
    "nt_streamk": dict(_PTRS, lda=1024, ldb=1024, ldc=256, M=256, N=256, K=1024, ncu=NCU, ws=P,
                       ws_bytes=1 << 30, cnt=P, ncnt=1 << 20),
    "nn": dict(_PTRS, lda=64, ldb=256, ldc=256, M=64, N=256, K=64, split=1, ws=None),
    "nt_split": dict(A=P, B=P, C=P, lda=128, ldb=128, ldc=256, M=64, N=256, K=128, split=2,
                     tile192=0, ws=P, ws_bytes=2 * 64 * 256 * 4),
    "tn": dict(A=P, B=P, C=P, lda=128, ldb=256, ldc=256, M=128, N=256, K=64, residual=None,
               ldr=0, epi=0, out_f32=0, split=1, ws=None),
    "nt_phase_probe": dict(A=P, B=P, C=P, lda=128, ldb=128, M=64, N=256, K=128, nj=4, recs=P),
}
SK_PLAN = (2, 8, 2 * 2 * 8 * 32768, 8)        # of BASE["nt_streamk"], asserted below
NN_SPLIT = dict(split=2, ws=P, K=128, lda=128)
TN_SPLIT = dict(split=2, ws=P, K=128)

ROWS = []                                     # (entry point, what, replaced fields, return code)


def _row(entry, what, expect=BAD, **over):
    ROWS.append((entry, what, over, expect))


for v in (0, 1, 2):
    _row("nt_v", f"v{v} K % 64", variant=v, K=100, lda=104, ldb=104)
    _row("nt_v", f"v{v} K = 0", variant=v, K=0)
    _row("nt_v", f"v{v} lda % 8", variant=v, lda=60)
    _row("nt_v", f"v{v} misaligned A", variant=v, A=ODD)
    _row("nt_v", f"v{v} bias flag, no bias", variant=v, epi=1)
    _row("nt_v", f"v{v} residual flag, no residual", variant=v, epi=8)
    _row("nt_v", f"v{v} dgelu flag, no u", variant=v, epi=16)
    _row("nt_v", f"v{v} M = 0", OK, variant=v, M=0)
    _row("nt_v", f"v{v} N = 0", OK, variant=v, N=0)

_row("nt_streamk", "3 K-tiles", K=192, lda=192, ldb=192)
_row("nt_streamk", "tiles >= CUs", M=8192, N=8192, K=512, lda=512, ldb=512, ldc=8192)
for k, why in ((512, " (K = 512: a grid of one, no plan)"), (1024, "")):
    sk = dict(K=k, lda=k, ldb=k)
    _row("nt_streamk", "ws null" + why, ws=None, **sk)
    _row("nt_streamk", "ws one byte short" + why, ws_bytes=SK_PLAN[2] - 1, **sk)
    _row("nt_streamk", "one counter short" + why, ncnt=SK_PLAN[3] - 1, **sk)
    _row("nt_streamk", "misaligned ws" + why, ws=ODD, **sk)
_row("nt_streamk", "M % 8", M=260)
_row("nt_streamk", "N % 64", N=288, ldc=288)
_row("nt_streamk", "M = 0", OK, M=0)

_row("nn", "K % 64", K=100, lda=104)
_row("nn", "N % 256", N=192, ldc=192)
_row("nn", "M % 8", M=60)
_row("nn", "ldb < N", ldb=128)
_row("nn", "lda < K", lda=32)
_row("nn", "misaligned B", B=ODD)
_row("nn", "K * ldb * 2 = 2^31", K=65536, lda=65536, ldb=16384)
_row("nn", "split, ws null", **dict(NN_SPLIT, ws=None))
_row("nn", "split with an epilogue", residual=P, ldr=256, epi=16, **NN_SPLIT)
_row("nn", "split to fp32", out_f32=1, **NN_SPLIT)
_row("nn", "split, ldc != N", ldc=264, **NN_SPLIT)
_row("nn", "split > K-tiles", **dict(NN_SPLIT, K=64, lda=64))

_row("nt_split", "split = 1", split=1)
_row("nt_split", "ldc != N", ldc=264)
_row("nt_split", "M % 8", M=60)
_row("nt_split", "N % 64", N=96, ldc=96)
_row("nt_split", "tile192, N % 192", tile192=1)
_row("nt_split", "misaligned ws", ws=ODD)
_row("nt_split", "split > K-tiles", K=64, lda=64, ldb=64)
_row("nt_split", "ws one byte short", ws_bytes=2 * 64 * 256 * 4 - 1)

_row("tn", "M % 128", M=64)
_row("tn", "N % 256", N=192, ldc=192)
_row("tn", "lda < M", lda=64)
_row("tn", "ldb < N", ldb=128)
_row("tn", "ldc < N", ldc=128)
_row("tn", "K * lda * 2 = 2^31", K=65536, lda=16384)
_row("tn", "bias flag", epi=1)
_row("tn", "accumulate, no residual", epi=8)
_row("tn", "accumulate to fp32", epi=8, residual=P, ldr=256, out_f32=1)
_row("tn", "split, ws null", **dict(TN_SPLIT, ws=None))
_row("tn", "split, ldc != N", ldc=264, **TN_SPLIT)
_row("tn", "split > K-tiles", **dict(TN_SPLIT, K=64))
_row("tn", "split, misaligned ws", **dict(TN_SPLIT, ws=ODD))

_row("nt_phase_probe", "M % 8", M=60)
_row("nt_phase_probe", "nj = 3, N % 192", nj=3)
_row("nt_phase_probe", "one K-tile", K=64)
_row("nt_phase_probe", "recs null", recs=None)


@pytest.fixture(scope="module")
def lib():
    if not _lib.available():
        pytest.skip("kernel library not built / not loadable here")
    return _lib.lib()


def test_streamk_rows_start_from_a_valid_plan(lib):
    import ctypes

    b = BASE["nt_streamk"]
    out = (ctypes.c_int64 * 4)()
    assert lib.dlbb_gemm_streamk_plan(b["M"], b["N"], b["K"], NCU, out) == 1
    assert tuple(out) == SK_PLAN
    assert b["ws_bytes"] >= SK_PLAN[2] and b["ncnt"] >= SK_PLAN[3]
    for M, N in ((260, 256), (256, 288)):         # the M % 8 / N % 64 rows get past the plan
        assert lib.dlbb_gemm_streamk_plan(M, N, b["K"], NCU, out) == 1
    assert lib.dlbb_gemm_streamk_plan(256, 256, 512, NCU, out) == 0


@pytest.mark.parametrize("entry,what,over,expect", ROWS,
                         ids=[f"{e}-{w}".replace(" ", "_") for e, w, _, _ in ROWS])
def test_out_of_contract_call_is_refused_without_a_launch(lib, entry, what, over, expect):
    assert over and set(over) <= set(ARGS[entry]), (entry, what)
    call = dict(BASE[entry], **over)
    assert call != BASE[entry], (entry, what, "a row inside the contract would launch")
    before = lib.dlbb_gemm_last_kernel()
    rc = getattr(lib, FN[entry])(*[call[k] for k in ARGS[entry]], None)
    assert rc == expect, (entry, what, rc)
    assert lib.dlbb_gemm_last_kernel() == before, (entry, what)
