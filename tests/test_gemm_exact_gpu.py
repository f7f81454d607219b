"""Training GEMMs (``csrc/gemm.hip``, ``csrc/gemm_tn.hip``) held to exact integer products on
every kernel path.

Operands are small integers (``gemm_exact_utils``), so fp32 accumulation is exact in any order:
an fp32 output must equal the fp64 product bit for bit, a bf16 output its one rounding. Every
epilogue works in fp32 in the order acc + bias -> (bf16 pre-activation store) -> act -> +
residual -> one RNE cast, so bias / residual / accumulate forms are exact too; only the values
after a GELU are not (they stay on the tolerance tests). After every call the test asserts
which ``__global__`` the C dispatcher launched (``dlbb_gemm_last_kernel``): a silent fallback
to another kernel fails the case. The implementation functions are called directly, never the
autotuner."""

import contextlib
import functools

import pytest
import torch

import gemm_exact_utils as U

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
BF16 = torch.bfloat16
F32 = torch.float32
CANARY = 777.0


def _gemm():
    from distributed_llm_backend_benchmark_amd.ops import gemm

    return gemm


def _L():
    from distributed_llm_backend_benchmark_amd.ops import _lib

    return _lib


def _ncu():
    return _gemm()._num_cus(DEV)


def _expect(kname):
    """The dispatcher's last launch is the kernel the case is named for."""
    lib = _L().lib()
    got = int(lib.dlbb_gemm_last_kernel())
    assert got == U.KID[kname], (f"expected {U.KNAME[U.KID[kname]]}, the dispatcher launched "
                                 f"{lib.dlbb_gemm_kernel_name(got).decode()}")


@contextlib.contextmanager
def _knobs(tile=0, stagger=6, bal=2, persist_epi=True, stages=2, fused=False, order=1):
    gemm = _gemm()
    lib = _L().lib()
    old = gemm.get_stagger()
    try:
        gemm.set_tile(tile)
        gemm.set_stagger(stagger)
        gemm.set_bal(bal)
        gemm.set_persist_epi(persist_epi)
        gemm.set_wgrad_stages(stages)
        gemm.set_wgrad_fused(fused)
        lib.dlbb_gemm_wgrad_set_order(order)
        yield
    finally:
        gemm.set_tile(0)
        gemm.set_stagger(old)
        gemm.set_bal(2)
        gemm.set_persist_epi(True)
        gemm.set_wgrad_stages(2)
        gemm.set_wgrad_fused(False)
        lib.dlbb_gemm_wgrad_set_order(1)


@functools.lru_cache(maxsize=6)
def _ops(M, N, K, kind="int"):
    """a [M, K], b [N, K] and the fp64 product a b^T [M, N], computed once per shape and shared
    (never written to)."""
    ga, gb = (U.int_a, U.int_b) if kind == "int" else (U.tern_a, U.tern_b)
    amax = 4 if kind == "int" else 1
    assert U.exact_ok(amax, amax, K), (M, N, K)
    a, b = ga(M, K, DEV), gb(N, K, DEV)
    return a, b, U.ref_product(a, b)


@functools.lru_cache(maxsize=6)
def _wops(T, N, K, kind="int"):
    """Weight-gradient operands dy [T, N], x [T, K] and the fp64 dW = dy^T x [N, K]."""
    a, b, ref = _ops(N, K, T, kind)
    return a.t().contiguous(), b.t().contiguous(), ref


@functools.lru_cache(maxsize=6)
def _rops(M, N, K, seed):
    """Uniform [-1, 1) operands with their fp64 product and |a| |b|^T."""
    a, b = U.rand_bf16(M, K, seed=seed, device=DEV), U.rand_bf16(N, K, seed=seed + 1, device=DEV)
    return a, b, U.ref_product(a, b), U.ref_product(a.abs(), b.abs())


def _bounds(K, ref, mag):
    b32 = (K + 8) * 2.0 ** -24 * mag
    return b32, b32 + 2.0 ** -8 * ref.abs()


# ------------------------------------------------------------------------------- NT forward

EPIS = ("plain", "bias", "bias_res", "bias_preact", "bias_gelu_preact")


def _nt(impl, M, N, K, epi, out_dtype, kid, tile=(256, 256), what=""):
    """One NT call of ``impl`` with epilogue ``epi``: the output (and the pre-activation store)
    equal the exact values; the GELU cases check the pre-activation only. Returns the output."""
    a, b, ref = _ops(M, N, K)
    bias = U.int_bias(N, DEV) if epi != "plain" else None
    res = U.int_res(M, N, DEV) if epi == "bias_res" else None
    pre = torch.full((M, N), CANARY, dtype=BF16, device=DEV) if epi.endswith("preact") else None
    act = "gelu_tanh" if "gelu" in epi else None
    out = torch.full((M, N), CANARY, dtype=out_dtype, device=DEV)
    impl(a, b, bias, act, res, out, pre)
    _expect(kid)
    what = f"{what or kid} {M}x{N}x{K} {epi} {out_dtype}"
    u = ref if bias is None else ref + bias.double()
    if pre is not None:
        U.assert_exact(pre, u.to(BF16), tile, what + " (pre-activation)")
    if act is None:
        y = u if res is None else u + res.double()
        U.assert_exact(out, y.to(out_dtype), tile, what)
    else:
        assert bool(torch.isfinite(out.float()).all()), what
    return out


@pytest.mark.parametrize("M,N,K", U.shapes(256)["nt_128"])
def test_nt_128(M, N, K):
    """128^2 tiles: one and five K-tiles, ragged M, N = 331 (odd: the scalar epilogue)."""
    gemm = _gemm()
    with _knobs(tile=128):
        for dt in (F32, BF16):
            for epi in ("plain", "bias_res", "bias_preact", "bias_gelu_preact"):
                _nt(gemm._mfma_linear, M, N, K, epi, dt, "nt_128", (128, 128))


@pytest.mark.parametrize("M,N,K", U.shapes(256)["nt_256_deep"])
def test_nt_256_deep(M, N, K):
    """The deep-pipeline 256^2 kernel (the general contract: any M, N)."""
    gemm = _gemm()
    with _knobs(tile=256, stagger=3):
        for dt in (F32, BF16):
            for epi in ("plain", "bias_res", "bias_preact", "bias_gelu_preact"):
                _nt(gemm._mfma_linear, M, N, K, epi, dt, "nt_256_deep")


@pytest.mark.parametrize("bal", [0, 1])
@pytest.mark.parametrize("M,N,K", U.shapes(256)["nt_256_pp"])
def test_nt_256_pingpong(M, N, K, bal):
    """256^2 ping-pong, plain and balanced DMA issue: 1, 3 and 33 K-tiles."""
    gemm = _gemm()
    assert M % 8 == 0 and N % 64 == 0 and -(-M // 256) * -(-N // 256) <= _ncu()
    kid = "nt_256_pp_bal" if bal else "nt_256_pp"
    with _knobs(tile=256, stagger=6, bal=bal):
        for dt in (F32, BF16):
            for epi in EPIS:
                _nt(gemm._mfma_linear, M, N, K, epi, dt, kid)


@pytest.mark.parametrize("bal", [0, 1])
@pytest.mark.parametrize("K", [128, 192])
def test_nt_persistent(K, bal):
    """Persistent ping-pong: more tiles than CUs (workgroups loop), a ragged last row block, the
    contract's minimum of two K-tiles and three; each lean epilogue kind is its own kernel."""
    gemm = _gemm()
    ncu = _ncu()
    M, N = U.persist_shape(ncu)
    assert -(-M // 256) * (N // 256) > ncu and M % 256 == 8 and K // 64 >= 2
    base = "nt_256_persist_bal_" if bal else "nt_256_persist_"

    def gelu_erf(x2, w, bias, act, r2, out, pre):
        return gemm._mfma_linear(x2, w, bias, "gelu_erf", r2, out, pre)

    with _knobs(tile=256, stagger=10, bal=bal):
        _nt(gemm._mfma_linear, M, N, K, "plain", BF16, base + "plain")
        _nt(gemm._mfma_linear, M, N, K, "bias", BF16, base + "bias")
        _nt(gemm._mfma_linear, M, N, K, "bias_gelu_preact", BF16, base + "gelu_tanh")
        _nt(gelu_erf, M, N, K, "bias_gelu_preact", BF16, base + "gelu_erf")
        _nt(gemm._mfma_linear, M, N, K, "bias_gelu", BF16, base + "gelu_tanh")
        # outside the lean kinds the persistent mode runs the ping-pong: the record says so
        _nt(gemm._mfma_linear, M, N, K, "bias_res", BF16,
            "nt_256_pp_bal" if bal else "nt_256_pp")
    with _knobs(tile=256, stagger=10, bal=bal, persist_epi=False):
        _nt(gemm._mfma_linear, M, N, K, "bias", BF16, "nt_256_pp_bal" if bal else "nt_256_pp")


@pytest.mark.parametrize("bal", [0, 1])
@pytest.mark.parametrize("M,N,K", U.shapes(256)["nt_192"])
def test_nt_192(M, N, K, bal):
    """256 x 192 ping-pong tiles (variant 1)."""
    gemm = _gemm()
    assert gemm.mfma192_ok(M, N)
    kid = "nt_192_pp_bal" if bal else "nt_192_pp"
    with _knobs(bal=bal):
        for dt in (F32, BF16):
            for epi in EPIS:
                _nt(gemm._mfma192_linear, M, N, K, epi, dt, kid, (256, 192))


@pytest.mark.parametrize("bal", [0, 1])
@pytest.mark.parametrize("looping,K", [(False, 384), (True, 384), (True, 448)])
def test_nt_192_spread(looping, K, bal):
    """Persistent 256 x 192 with spread C stores (variant 2): its minimum of 6 K-tiles and 7,
    a grid below the CUs and one where workgroups loop; it must not fall to variant 1."""
    gemm = _gemm()
    ncu = _ncu()
    M, N = U.spread_shape(ncu) if looping else (272, 384)
    tiles = -(-M // 256) * (N // 192)
    assert gemm.mfma192p_ok(M, N, K, True) and (tiles > ncu) == looping
    with _knobs(bal=bal):
        _nt(gemm._mfma192p_linear, M, N, K, "plain", BF16,
            "nt_192_spread_bal" if bal else "nt_192_spread", (256, 192))
        # outside its contract (fp32 output) the library runs variant 1, and says so
        _nt(gemm._mfma192p_linear, M, N, K, "plain", F32,
            "nt_192_pp_bal" if bal else "nt_192_pp", (256, 192))


@pytest.mark.parametrize("bal", [0, 1])
@pytest.mark.parametrize("M,N,K", U.shapes(256)["nt_streamk"])
def test_nt_streamk(M, N, K, bal):
    """Stream-K: every tile of the first shape has 2 contributors, some tile of the second at
    least 3; every epilogue; the arrival counters are zero again afterwards; two calls are
    bit-identical."""
    gemm = _gemm()
    ncu = _ncu()
    plan = gemm.streamk_plan(M, N, K, ncu)
    assert plan is not None, (M, N, K, ncu)
    contrib = U.streamk_contributors(M, N, K, plan)
    if (M, N, K) == (520, 256, 704):
        assert plan[:2] == (4, 9) and contrib == [2, 2, 2], (plan, contrib)
    else:
        assert max(contrib) >= 3, (plan, max(contrib))
    kid = "nt_256_streamk_bal" if bal else "nt_256_streamk"
    with _knobs(bal=bal):
        for dt in (F32, BF16):
            for epi in EPIS:
                first = _nt(gemm._mfma_streamk_linear, M, N, K, epi, dt, kid)
                again = _nt(gemm._mfma_streamk_linear, M, N, K, epi, dt, kid)
                assert torch.equal(first, again)
        _, cnt = gemm._SK_WS[(0, _L().stream(DEV))]
        assert int(cnt.abs().sum()) == 0, "Stream-K arrival counters not re-armed"


def _split_c(a, b, out, split, tile192):
    lib = _L().lib()
    M, K = a.shape
    N = b.shape[0]
    ws = torch.empty(split * M * N, dtype=F32, device=DEV)
    rc = lib.dlbb_gemm_bf16_nt_split(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0),
                                     out.data_ptr(), N, M, N, K, split, tile192, ws.data_ptr(),
                                     ws.numel() * 4, _L().stream(DEV))
    assert rc == 0, rc
    torch.cuda.synchronize()          # ws is freed on return


@pytest.mark.parametrize("bal", [0, 1])
def test_nt_split_k(bal):
    """Split-K NT + reduce: 17 K-tiles in slices of 9 and 8 through ``_mfma_split_linear``
    (256^2 and 256 x 192 tiles); the C entry with 7 K-tiles in 3 slices (3, 3, 1) and 10 K-tiles
    asked in 7 slices, clamped to 5."""
    gemm = _gemm()
    ncu = _ncu()
    with _knobs(bal=bal):
        for M, N, K in U.shapes(ncu)["nt_split"]:
            plan = gemm.split_plan(M, N, K, ncu)
            assert plan == (2, int(N % 192 == 0)), plan
            t192 = plan[1]
            kid = ("nt_192_pp" if t192 else "nt_256_pp") + ("_bal" if bal else "")
            _nt(gemm._mfma_split_linear, M, N, K, "plain", BF16, kid, (256, 192 if t192 else 256))
        for M, N, K, split in U.shapes(ncu)["nt_split_c"]:
            a, b, ref = _ops(M, N, K)
            t192 = int(N % 192 == 0)
            out = torch.full((M, N), CANARY, dtype=BF16, device=DEV)
            _split_c(a, b, out, split, t192)
            _expect(("nt_192_pp" if t192 else "nt_256_pp") + ("_bal" if bal else ""))
            U.assert_exact(out, ref.to(BF16), (256, 192 if t192 else 256),
                           f"nt_split C entry {M}x{N}x{K} split {split} tile192 {t192}")


# ------------------------------------------------------------------------------- NN dgrad

def _nn(M, N, K, kid, split=None):
    """dX [M, N] = dY [M, K] W [K, N] through ``_dgrad_hip``."""
    gemm = _gemm()
    a, b, ref = _ops(M, N, K)
    w = b.t().contiguous()                              # [K, N]
    out = torch.full((M, N), CANARY, dtype=BF16, device=DEV)
    gemm._dgrad_hip(a, w, out, split=split)
    _expect(kid)
    U.assert_exact(out, ref.to(BF16), (256, 256), f"{kid} {M}x{N}x{K} split {split}")


@pytest.mark.parametrize("bal", [0, 1])
def test_nn_dgrad(bal):
    ncu = _ncu()
    kid = "nn_256_pp_bal" if bal else "nn_256_pp"
    with _knobs(bal=bal):
        for M, N, K in U.shapes(ncu)["nn_256_pp"]:
            _nn(M, N, K, kid, split=1)
        for M, N, K, split in U.shapes(ncu)["nn_split"]:          # (3, 3, 1) and 7 -> 5 slices
            _nn(M, N, K, kid, split=split)


@pytest.mark.parametrize("persist", [True, False])
def test_nn_dgrad_persistent(persist):
    """More 256^2 tiles than CUs and a 2-K-tile reduction: the persistent NN form, or with it
    switched off the plain ping-pong, on the same shape."""
    ncu = _ncu()
    (M, N, K), = U.shapes(ncu)["nn_persist"]
    assert -(-M // 256) * (N // 256) > ncu
    with _knobs(persist_epi=persist):
        _nn(M, N, K, "nn_256_persist_bal_plain" if persist else "nn_256_pp_bal", split=1)


# ------------------------------------------------------------------- TN weight gradient

def _prev(N, K, dtype):
    return U.int_res(N, K, DEV, salt=3).to(dtype)


@pytest.mark.parametrize("bal", [0, 1])
@pytest.mark.parametrize("T,N,K", U.shapes(256)["tn_256_pp"])
def test_tn_pingpong(T, N, K, bal):
    """256^2 TN ping-pong: a half tile of output rows and one and a half; bf16, fp32 and
    accumulate-into-bf16 stores."""
    gemm = _gemm()
    dy, x, ref = _wops(T, N, K)
    kid = "tn_256_pp_bal" if bal else "tn_256_pp"
    with _knobs(bal=bal):
        for dt in (BF16, F32):
            assert gemm.wgrad_pp_supported(dy, x, torch.empty(N, K, dtype=dt, device=DEV), False)
            out = torch.full((N, K), CANARY, dtype=dt, device=DEV)
            gemm._pp_launch(dy, x, out, False, 0, N, 1)
            _expect(kid)
            U.assert_exact(out, ref.to(dt), (256, 256), f"{kid} T{T} {N}x{K} {dt}")
        prev = _prev(N, K, BF16)
        out = prev.clone()
        gemm._pp_launch(dy, x, out, True, 0, N, 1)
        _expect(kid)
        U.assert_exact(out, (ref + prev.double()).to(BF16), (256, 256),
                       f"{kid} T{T} {N}x{K} accumulate")


@pytest.mark.parametrize("T,N,K,r0,split", U.shapes(256)["tn_split"])
def test_tn_split_and_row_offset(T, N, K, r0, split):
    """TN split-K (10 K-tiles asked in 7 slices -> 5; 8 in 2) on output rows [r0, N): rows
    below r0 keep their canary."""
    gemm = _gemm()
    dy, x, ref = _wops(T, N, K)
    for dt in (BF16, F32):
        out = torch.full((N, K), CANARY, dtype=dt, device=DEV)
        gemm._pp_launch(dy, x, out, False, r0, N, split)
        _expect("tn_256_pp_bal")
        U.assert_exact(out[r0:], ref[r0:].to(dt), (256, 256),
                       f"tn split {split} r0 {r0} T{T} {N}x{K} {dt}")
        assert bool((out[:r0] == CANARY).all())


def test_tn_tail_plan():
    """A grid of one full round of the CUs plus 44 tiles: ``_wgrad_pp`` runs the tail rows as
    a split-K launch; the whole dW is exact."""
    gemm = _gemm()
    ncu = _ncu()
    (T, N, K), = U.shapes(ncu)["tn_tail"]
    head, tsplit = gemm.pp_tail_plan(T, N, K, ncu)
    assert head < N and tsplit >= 2, (head, tsplit)
    dy, x, ref = _wops(T, N, K)
    for dt in (BF16, F32):
        out = torch.full((N, K), CANARY, dtype=dt, device=DEV)
        gemm._wgrad_pp(dy, x, out, False)
        _expect("tn_256_pp_bal")
        U.assert_exact(out, ref.to(dt), (256, 256), f"tn tail T{T} {N}x{K} {dt}")
    _ops.cache_clear()
    _wops.cache_clear()


@pytest.mark.parametrize("bal", [0, 1])
def test_stamped_pingpong_twins(bal):
    """With per-workgroup stamping on, the six ping-pong kernels run their stamped twins: the
    same exact results, one stamp record per workgroup, and the record names the twin."""
    from distributed_llm_backend_benchmark_amd.utils.stamps import Stamps

    gemm = _gemm()
    sfx = "_bal_st" if bal else "_st"
    M, N, K = 264, 320, 192
    with _knobs(tile=256, stagger=6, bal=bal), Stamps(4096, DEV) as st:
        _nt(gemm._mfma_linear, M, N, K, "bias_res", BF16, "nt_256_pp" + sfx)
        _nt(gemm._mfma_linear, M, N, K, "plain", F32, "nt_256_pp" + sfx)
        _nn(264, 512, 192, "nn_256_pp" + sfx, split=1)
        _nn(264, 256, 448, "nn_256_pp" + sfx, split=3)
        dy, x, ref = _wops(192, 384, 512)
        out = torch.full((384, 512), CANARY, dtype=F32, device=DEV)
        gemm._pp_launch(dy, x, out, False, 0, 384, 1)
        _expect("tn_256_pp" + sfx)
        U.assert_exact(out, ref.float(), (256, 256), "stamped tn")
    recs = st.collect()
    assert [(r["kind"], r["workgroups"]) for r in recs] == [
        ("gemm_nt_pp", 4), ("gemm_nt_pp", 4), ("gemm_nn_pp", 4), ("gemm_nn_pp", 6),
        ("gemm_tn_pp", 4)], [(r["kind"], r["workgroups"]) for r in recs]
    assert all(e >= s for r in recs for s, e in zip(r["start_ns"], r["end_ns"]))
    _nt(gemm._mfma_linear, 8, 64, 64, "plain", BF16, "nt_128")      # stamping is off again


# ------------------------------------------------- 128^2 / 256x128 / 128x256 weight gradient

def _wgrad_fn(impl):
    gemm = _gemm()
    return {"mfma": gemm._wgrad_hip, "mfma256": gemm._wgrad_hip256,
            "mfma_wide": gemm._wgrad_hip_wide}[impl]


def _wgrad_case(impl, T, N, K, split, dt, accumulate, with_bias, what):
    """One weight-gradient call against the exact dW (and db). bf16 outputs that pass through
    bf16 partial slabs (any call that is not a one-slice plain store) use ternary operands, so
    that every slab is an integer of magnitude <= 256 and exact in bf16."""
    fn = _wgrad_fn(impl)
    s = 1 if split is None else split
    assert T < 512 or split is not None            # the default split of these shapes is 1
    per, nsl = U.wgrad_per(T, s)
    direct = nsl == 1 and not accumulate and not with_bias
    kind = "tern" if dt == BF16 and not direct else "int"
    dy, x, ref = _wops(T, N, K, kind)
    if kind == "tern":
        assert per <= 256 if nsl > 1 else float(ref.abs().max()) <= 256, (T, s, per)
    prev = _prev(N, K, dt) if accumulate else None
    out = prev.clone() if accumulate else torch.full((N, K), CANARY, dtype=dt, device=DEV)
    bprev = U.int_bias(N, DEV).to(dt) if accumulate else None
    bout = None
    if with_bias:
        bout = bprev.clone() if accumulate else torch.full((N,), CANARY, dtype=dt, device=DEV)
    fn(dy, x, out, accumulate, split, bout)
    want = ref + prev.double() if accumulate else ref
    U.assert_exact(out, want.to(dt), U.WGRAD_TILES[impl], what)
    if with_bias:
        db = dy.double().sum(0)
        if accumulate:
            db = db + bprev.double()
        U.assert_exact(bout.view(1, N), db.to(dt).view(1, N), (1, U.WGRAD_TILES[impl][0]),
                       what + " (bias gradient)")
    return out, bout


@pytest.mark.parametrize("stages", [2, 3, 4])
@pytest.mark.parametrize("impl", ["mfma", "mfma256", "mfma_wide"])
def test_wgrad_tiles(impl, stages):
    """The three weight-gradient tile forms at every LDS ring depth: 1, 3 and 11 32-row steps;
    one slice, three even slices and 352 rows in slices of 128, 128, 96; plain, accumulate into
    bf16 and into fp32; with and without the fused bias gradient."""
    with _knobs(stages=stages):
        for T, N, K in U.shapes(256)["wgrad"]:
            for split in U.WGRAD_SPLITS:
                for dt in (BF16, F32):
                    for accumulate in (False, True):
                        for with_bias in (False, True):
                            _wgrad_case(impl, T, N, K, split, dt, accumulate, with_bias,
                                        f"wgrad {impl} stages {stages} T{T} {N}x{K} split "
                                        f"{split} {dt} acc {accumulate} bias {with_bias}")


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("impl", ["mfma", "mfma256", "mfma_wide"])
def test_wgrad_in_launch_combine(impl, order):
    """In-launch split-K combine, both workgroup orders: exact, bit-equal to the separate
    reduce pass, tile counters zero afterwards."""
    gemm = _gemm()
    (T, N, K, split), = U.shapes(256)["wgrad_fused"]
    for dt in (BF16, F32):
        for accumulate in (False, True):
            what = f"wgrad {impl} order {order} T{T} {N}x{K} split {split} {dt} acc {accumulate}"
            for with_bias in (True, False):
                with _knobs(fused=False, order=order):
                    sep = _wgrad_case(impl, T, N, K, split, dt, accumulate, with_bias,
                                      what + f" bias {with_bias} separate")
                with _knobs(fused=True, order=order):
                    assert gemm.wgrad_fused_reduce()
                    fus = _wgrad_case(impl, T, N, K, split, dt, accumulate, with_bias,
                                      what + f" bias {with_bias} fused")
                assert torch.equal(sep[0], fus[0])
                assert not with_bias or torch.equal(sep[1], fus[1])
    cnt = gemm._tile_counters(DEV, 1)
    assert int(cnt.abs().sum()) == 0, "wgrad tile counters not re-armed"


# -------------------------------------------------------------------- padding and canaries

def _padded(t, pad_rows=8, pad_cols=64):
    """``t`` as a view into a larger NaN-filled buffer (row stride > columns, NaN rows after)."""
    R, C = t.shape
    buf = torch.full((R + pad_rows, C + pad_cols), float("nan"), dtype=t.dtype, device=DEV)
    buf[:R, :C] = t
    v = buf[:R, :C]
    assert v.stride(0) == C + pad_cols and v.data_ptr() % 16 == 0
    return v


def _canvas(M, N, dtype, col0=0, extra=0):
    """An [M, N] output view at rows 1 .. M, columns col0 .. col0 + N of a canary-filled
    [M + 2, N + extra] buffer, with the mask of everything outside the view."""
    buf = torch.full((M + 2, N + extra), CANARY, dtype=dtype, device=DEV)
    view = buf[1:M + 1, col0:col0 + N]
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[1:M + 1, col0:col0 + N] = False
    return buf, view, outside


def _check_canvas(buf, view, outside, dense, what):
    assert bool(torch.isfinite(view.float()).all()), what
    U.assert_exact(view.contiguous(), dense, (256, 256), what)
    assert bool((buf[outside] == CANARY).all()), what + ": wrote outside the output"


def _nt_v(a, b, c, M, N, K, bias, res, epi, variant=0, pre=None):
    rc = _L().lib().dlbb_gemm_bf16_nt_v(
        a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0), M, N, K,
        _L().ptr(bias), _L().ptr(res), res.stride(0) if res is not None else 0, _L().ptr(pre),
        epi, int(c.dtype == F32), variant, _L().stream(DEV))
    assert rc == 0, rc


def _streamk_c(a, b, c, M, N, K, bias, res, epi):
    gemm = _gemm()
    ncu = _ncu()
    plan = gemm.streamk_plan(M, N, K, ncu)
    assert plan is not None
    ws, cnt = gemm._streamk_buffers(DEV, plan[2], plan[3])
    rc = _L().lib().dlbb_gemm_bf16_nt_streamk(
        a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0), M, N, K,
        _L().ptr(bias), _L().ptr(res), res.stride(0) if res is not None else 0, None, epi,
        int(c.dtype == F32), ncu, ws.data_ptr(), ws.numel() * 4, cnt.data_ptr(), cnt.numel(),
        _L().stream(DEV))
    assert rc == 0, rc


EPI_BIAS, EPI_RESIDUAL = 1, 8


def _epi_consts():
    gemm = _gemm()
    assert (gemm.EPI_BIAS, gemm.EPI_RESIDUAL) == (EPI_BIAS, EPI_RESIDUAL)


@pytest.mark.parametrize("path", ["nt_128", "nt_256_deep", "nt_256_pp", "nt_192_pp",
                                  "nt_256_streamk"])
@pytest.mark.parametrize("layout", ["padded", "misaligned"])
def test_nt_padding_canaries_and_misaligned_epilogue(path, layout):
    """A and B are views into NaN-filled buffers (row strides > K, NaN rows after M / N); C is
    rows 1 .. M and a column slice of a canary buffer (ldc > N). ``padded`` keeps everything
    16-byte aligned (the vector epilogue); ``misaligned`` offsets C, the bias and the residual
    by one element with an odd ldc (vec_ok = 0, the scalar epilogue). The result is finite and
    equals the dense call bit for bit, and nothing outside C is written."""
    _epi_consts()
    M, N, K, knobs, variant = {
        "nt_128": (200, 136, 64, dict(tile=128), 0),
        "nt_256_deep": (264, 328, 64, dict(tile=256, stagger=3), 0),
        "nt_256_pp": (264, 320, 192, dict(tile=256, stagger=6, bal=0), 0),
        "nt_192_pp": (264, 384, 320, dict(bal=0), 1),
        "nt_256_streamk": (520, 256, 704, dict(bal=0), 0),
    }[path]
    a, b, ref = _ops(M, N, K)
    ap, bp = _padded(a), _padded(b)
    col0, extra = (8, 16) if layout == "padded" else (1, 3)
    bias_buf = torch.full((N + 8,), float("nan"), dtype=BF16, device=DEV)
    boff = 0 if layout == "padded" else 1
    bias_buf[boff:boff + N] = U.int_bias(N, DEV)
    bias = bias_buf[boff:boff + N]
    rbuf, res, _ = _canvas(M, N, BF16, col0, extra)
    res.copy_(U.int_res(M, N, DEV))
    want = ref + bias.double() + res.double()
    with _knobs(**knobs):
        for dt in (F32, BF16):
            buf, c, outside = _canvas(M, N, dt, col0, extra)
            if layout == "misaligned":
                assert c.stride(0) % 2 == 1 and bias.data_ptr() % 16 != 0
            else:
                assert c.stride(0) > N and c.stride(0) % 8 == 0 and c.data_ptr() % 16 == 0
            if path == "nt_256_streamk":
                _streamk_c(ap, bp, c, M, N, K, bias, res, EPI_BIAS | EPI_RESIDUAL)
            else:
                _nt_v(ap, bp, c, M, N, K, bias, res, EPI_BIAS | EPI_RESIDUAL, variant)
            _expect(path)
            what = f"{path} {layout} {M}x{N}x{K} {dt}"
            U.assert_exact(c.contiguous(), want.to(dt), (256, 256), what)
            dense = torch.empty(M, N, dtype=dt, device=DEV)
            if path == "nt_256_streamk":
                _streamk_c(a, b, dense, M, N, K, bias.clone(), res.contiguous(),
                           EPI_BIAS | EPI_RESIDUAL)
            else:
                _nt_v(a, b, dense, M, N, K, bias.clone(), res.contiguous(),
                      EPI_BIAS | EPI_RESIDUAL, variant)
            _expect(path)
            _check_canvas(buf, c, outside, dense, what)


def test_nt_split_padding_canaries():
    M, N, K, split = 264, 320, 448, 3
    a, b, ref = _ops(M, N, K)
    ap, bp = _padded(a), _padded(b)
    buf, c, outside = _canvas(M, N, BF16)
    with _knobs(bal=0):
        _split_c(ap, bp, c, split, 0)
        _expect("nt_256_pp")
        dense = torch.empty(M, N, dtype=BF16, device=DEV)
        _split_c(a, b, dense, split, 0)
    U.assert_exact(dense, ref.to(BF16), (256, 256), "nt split dense")
    _check_canvas(buf, c, outside, dense, "nt split padded")


def _nn_c(a, w, c, M, N, K, split=1):
    ws = torch.empty(split * M * N, dtype=F32, device=DEV) if split > 1 else None
    rc = _L().lib().dlbb_gemm_bf16_nn(
        a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), c.data_ptr(), c.stride(0), M, N, K,
        None, None, 0, None, 0, int(c.dtype == F32), split, _L().ptr(ws), _L().stream(DEV))
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", ["padded", "misaligned"])
def test_nn_padding_canaries_and_misaligned_epilogue(layout):
    """NN dgrad: dY and W ([K, N]) inside NaN-filled buffers (lda > K, ldb > N, NaN rows after
    M and after K); the output rows 1 .. M of a canary buffer — ``misaligned``: a column slice
    at an odd offset with an odd ldc (scalar epilogue). fp32 and bf16 outputs."""
    M, N, K = 264, 512, 192
    a, b, ref = _ops(M, N, K)
    w = b.t().contiguous()
    ap, wp = _padded(a), _padded(w)
    col0, extra = (0, 0) if layout == "padded" else (1, 3)
    with _knobs(bal=0):
        for dt in (F32, BF16):
            buf, c, outside = _canvas(M, N, dt, col0, extra)
            _nn_c(ap, wp, c, M, N, K)
            _expect("nn_256_pp")
            dense = torch.empty(M, N, dtype=dt, device=DEV)
            _nn_c(a, w, dense, M, N, K)
            U.assert_exact(dense, ref.to(dt), (256, 256), f"nn dense {dt}")
            _check_canvas(buf, c, outside, dense, f"nn {layout} {dt}")
        if layout == "padded":                   # the split form: ldc == N, bf16
            buf, c, outside = _canvas(M, N, BF16)
            _nn_c(ap, wp, c, M, N, K, split=2)
            _expect("nn_256_pp")
            _check_canvas(buf, c, outside, ref.to(BF16), "nn padded split 2")


def _tn_c(dy, x, c, N, K, T, prev=None, split=1):
    """dW [N, K] = dy[:, :N]^T x[:, :K] over T rows through the C entry."""
    ws = torch.empty(split * N * K, dtype=F32, device=DEV) if split > 1 else None
    rc = _L().lib().dlbb_gemm_bf16_tn(
        dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), c.data_ptr(), c.stride(0), N, K,
        T, _L().ptr(prev), prev.stride(0) if prev is not None else 0,
        EPI_RESIDUAL if prev is not None else 0, int(c.dtype == F32), split, _L().ptr(ws),
        _L().stream(DEV))
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", ["padded", "misaligned"])
def test_tn_padding_canaries_and_misaligned_epilogue(layout):
    """TN weight gradient: dY and X inside NaN-filled buffers (row strides > N / K, NaN rows
    after T); dW rows 1 .. N of a canary buffer — ``misaligned``: a column slice at an odd
    offset with an odd ldc (scalar epilogue)."""
    T, N, K = 64, 128, 256
    dy, x, ref = _wops(T, N, K)
    dyp, xp = _padded(dy), _padded(x)
    col0, extra = (0, 0) if layout == "padded" else (1, 3)
    with _knobs(bal=0):
        for dt in (F32, BF16):
            buf, c, outside = _canvas(N, K, dt, col0, extra)
            _tn_c(dyp, xp, c, N, K, T)
            _expect("tn_256_pp")
            dense = torch.empty(N, K, dtype=dt, device=DEV)
            _tn_c(dy, x, dense, N, K, T)
            U.assert_exact(dense, ref.to(dt), (256, 256), f"tn dense {dt}")
            _check_canvas(buf, c, outside, dense, f"tn {layout} {dt}")
        # accumulate into bf16 with the previous value at the same (mis)alignment
        buf, c, outside = _canvas(N, K, BF16, col0, extra)
        prev = _prev(N, K, BF16)
        c.copy_(prev)
        _tn_c(dyp, xp, c, N, K, T, prev=c)
        _expect("tn_256_pp")
        _check_canvas(buf, c, outside, (ref + prev.double()).to(BF16), f"tn {layout} accumulate")


# ------------------------------------------------------------------------ random operands

def _rand_nt(impl, M, N, K, seed, what, dts=(F32, BF16)):
    a, b, ref, mag = _rops(M, N, K, seed)
    b32, b16 = _bounds(K, ref, mag)
    for dt in dts:
        out = torch.empty(M, N, dtype=dt, device=DEV)
        impl(a, b, None, None, None, out, None)
        U.assert_within(out, ref, b32 if dt == F32 else b16, f"{what} {M}x{N}x{K} {dt}")


def test_random_nt_pingpong():
    gemm = _gemm()
    with _knobs(tile=256, stagger=6):
        for i, (M, N, K) in enumerate([(264, 320, 192), (520, 576, 2112)]):
            _rand_nt(gemm._mfma_linear, M, N, K, 100 + 2 * i, "nt ping-pong")
            assert int(_L().lib().dlbb_gemm_last_kernel()) in (U.KID["nt_256_pp"],
                                                               U.KID["nt_256_pp_bal"])


def test_random_nt_192():
    gemm = _gemm()
    for i, (M, N, K) in enumerate([(264, 384, 320), (264, 384, 2112)]):
        _rand_nt(gemm._mfma192_linear, M, N, K, 110 + 2 * i, "nt 192")
        assert int(_L().lib().dlbb_gemm_last_kernel()) in (U.KID["nt_192_pp"],
                                                           U.KID["nt_192_pp_bal"])


def test_random_nt_streamk():
    gemm = _gemm()
    for i, (M, N, K) in enumerate(U.shapes(256)["nt_streamk"]):
        _rand_nt(gemm._mfma_streamk_linear, M, N, K, 120 + 2 * i, "nt stream-k")
        _expect("nt_256_streamk")


def test_random_nt_split_k():
    gemm = _gemm()
    for i, (M, N, K) in enumerate([(264, 320, 1088), (264, 320, 4160)]):
        assert gemm.split_plan(M, N, K, _ncu()) is not None
        _rand_nt(gemm._mfma_split_linear, M, N, K, 130 + 2 * i, "nt split-k", dts=(BF16,))
        _expect("nt_256_pp")


def test_random_nn_and_nn_split():
    gemm = _gemm()
    for i, (M, N, K, split) in enumerate([(264, 512, 192, 1), (264, 512, 2112, 1),
                                          (264, 256, 448, 3), (264, 256, 4160, 4)]):
        a, b, ref, mag = _rops(M, N, K, 140 + 2 * i)
        w = b.t().contiguous()
        out = torch.empty(M, N, dtype=BF16, device=DEV)
        gemm._dgrad_hip(a, w, out, split=split)
        _expect("nn_256_pp_bal")
        U.assert_within(out, ref, _bounds(K, ref, mag)[1], f"nn {M}x{N}x{K} split {split} bf16")


def test_random_tn():
    gemm = _gemm()
    for i, (T, N, K) in enumerate([(192, 384, 512), (2112, 384, 512)]):
        a, b, ref, mag = _rops(N, K, T, 150 + 2 * i)
        dy, x = a.t().contiguous(), b.t().contiguous()
        b32, b16 = _bounds(T, ref, mag)
        for dt in (F32, BF16):
            out = torch.empty(N, K, dtype=dt, device=DEV)
            gemm._pp_launch(dy, x, out, False, 0, N, 1)
            _expect("tn_256_pp_bal")
            U.assert_within(out, ref, b32 if dt == F32 else b16, f"tn T{T} {N}x{K} {dt}")


def test_random_wgrad_128():
    """fp32 dW: the any-order bound over T; bf16 dW through bf16 partial slabs: each slab's own
    rounding adds at most 2^-8 (|dy|^T |x|) in all."""
    gemm = _gemm()
    for i, (T, N, K, split) in enumerate([(96, 256, 256, 3), (2112, 256, 512, None)]):
        a, b, ref, mag = _rops(N, K, T, 160 + 2 * i)
        dy, x = a.t().contiguous(), b.t().contiguous()
        b32, b16 = _bounds(T, ref, mag)
        out = torch.empty(N, K, dtype=F32, device=DEV)
        gemm._wgrad_hip(dy, x, out, False, split, None)
        U.assert_within(out, ref, b32, f"wgrad T{T} {N}x{K} split {split} fp32")
        outb = torch.empty(N, K, dtype=BF16, device=DEV)
        gemm._wgrad_hip(dy, x, outb, False, split, None)
        U.assert_within(outb, ref, b16 + 2.0 ** -8 * mag, f"wgrad T{T} {N}x{K} split {split} bf16")
