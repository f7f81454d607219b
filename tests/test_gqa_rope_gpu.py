"""``rope=`` on the grouped-query ``ops.kv_append`` / ``ops.decode_attention`` /
``ops.prefill_attention`` against an fp64 reference on the same bf16 bits: Q and K rotated in fp64
with the table and rounded to bf16 (the cache's contract), fp64 softmax. The table has exactly
``L_max`` rows (an index one row too far is outside it); the caches are NaN past the live rows and,
under a window, below the first key the kernels may touch. The bound is the project's GQA bound: a
torch model of the kernel's roundings (fp32 rotation, bf16 Q / K / P) stays within 4.1e-3 of the
unrounded fp64 reference at D 64 / 128, lengths 0 .. 4000, with and without a window."""

import functools

import pytest
import torch

import gqa_rope_utils as U
from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.ops.decode import CHUNK_GQA

pytestmark = pytest.mark.gpu

HKV, NAN, DEV = 2, float("nan"), "cuda"
TOL = dict(rtol=2e-2, atol=2e-2)     # the project's decode and prefill bound: bf16 P, bf16 output


def _case(D, G, lens, T, W=None, tile=1, table=U.table):
    """qkv [B, T, (H_q + 2 H_kv) * D] of the block at [len_b, len_b + T), the table [L_max, D], NaN
    caches holding rows [floor_b, len_b + T) of every live row (written by ``ops.kv_append(rope=)``;
    floor_b: the first key of the row's first token under W, rounded down to ``tile``), the device
    lengths (one element when the rows agree) and the fp64 reference per row (None: empty slot)."""
    B, HQ, top = len(lens), G * HKV, max(lens)
    g = torch.Generator().manual_seed(1000 * D + 10 * G + 7 * T + sum(lens))
    rows = torch.randn(B, top + T, HQ + 2 * HKV, D, generator=g).mul(1.5).bfloat16().to(DEV)
    rope = table(top + T + 5, D).to(DEV)
    k, v = (torch.full((B, HKV, top + T + 5, D), NAN, dtype=torch.bfloat16, device=DEV)
            for _ in "kv")
    seq = len(set(lens)) > 1
    qkv = torch.stack([rows[b, max(n, 0):max(n, 0) + T] for b, n in enumerate(lens)])
    qkv = qkv.reshape(B, T, -1)
    length = torch.tensor(lens if seq else lens[:1], dtype=torch.int32, device=DEV)
    if top > 0:
        start = torch.tensor([0 if n >= 0 else -1 for n in lens] if seq else [0],
                             dtype=torch.int32, device=DEV)
        ops.kv_append(rows[:, :top].reshape(B, top, -1), HQ, k, v, start, n_kv_head=HKV, rope=rope)
    for b, n in enumerate(lens):
        if n >= 0:
            floor = 0 if W is None else max(0, n - W + 1) // tile * tile
            k[b, :, :floor], v[b, :, :floor], k[b, :, n:], v[b, :, n:] = NAN, NAN, NAN, NAN
    ops.kv_append(qkv, HQ, k, v, length, n_kv_head=HKV, rope=rope)
    ref = [None if n < 0 else U.reference(rows[b, :n + T], rope, n, T, G, HKV, W)
           for b, n in enumerate(lens)]
    return qkv, k, v, length, rope, ref


def _check(out, ref):
    for b, r in enumerate(ref):
        if r is None:
            assert not out[b].any()
        else:
            assert torch.isfinite(out[b]).all()
            torch.testing.assert_close(out[b].double().cpu(), r, **TOL)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("lens,L", [((5, 5), 12), ((5, 0, -1, 8), 12), ((10, 10), 12)])
def test_append(D, lens, L, G=4, T=3):
    B, HQ, seq = len(lens), G * HKV, len(set(lens)) > 1
    g = torch.Generator().manual_seed(D + sum(lens))
    x = torch.randn(B, T, HQ + 2 * HKV, D, generator=g).mul(1.5).bfloat16().to(DEV)
    rope = U.table(L, D).to(DEV)
    k, v = (torch.full((B, HKV, L, D), NAN, dtype=torch.bfloat16, device=DEV) for _ in "kv")
    length = torch.tensor(lens if seq else lens[:1], dtype=torch.int32, device=DEV)
    ops.kv_append(x.reshape(B, T, -1), HQ, k, v, length, n_kv_head=HKV, rope=rope)
    for b, n in enumerate(lens):
        m = max(0, min(T, L - n)) if n >= 0 else 0             # tokens of the row that fit
        live = slice(n, n + m)
        assert torch.equal(v[b, :, live], x[b, :m, HQ + HKV:].transpose(0, 1))
        want = U.rotate(x[b, :m, HQ:HQ + HKV].cpu(), rope[live].cpu()).bfloat16().float()
        got = k[b, :, live].transpose(0, 1).float().cpu()
        ulp = torch.ldexp(torch.ones(()), torch.frexp(torch.maximum(want.abs(), got.abs()))[1] - 8)
        assert ((got - want).abs() <= ulp).all()               # fp32 then bf16: one ulp, no more
        rest = torch.ones(L, dtype=torch.bool)
        rest[live] = False
        assert k[b][:, rest].isnan().all() and v[b][:, rest].isnan().all()


@pytest.mark.parametrize("D,G,lens,W", [(D, G, (n, n), None) for D in (64, 128) for G in (2, 16)
                                        for n in (0, 37, CHUNK_GQA + 1)]
                         + [(D, 4, (0, 37, -1, 300), None) for D in (64, 128)]
                         + [(D, 4, (299, 299), 100) for D in (64, 128)])
def test_decode(D, G, lens, W):
    qkv, k, v, length, rope, ref = _case(D, G, lens, 1, W)
    kw = {} if W is None else {"window": W}
    out = ops.decode_attention(qkv, G * HKV, k, v, length, n_kv_head=HKV, rope=rope, **kw)
    _check(out, ref)
    if len(lens) > 2:
        assert k[2].isnan().all() and v[2].isnan().all()       # the empty slot


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [2, 16])
@pytest.mark.parametrize("T,n", [(5, 37), (8, 150)])
@pytest.mark.parametrize("kw", [{}, {"window": 30}, {"key_split": 128}])
def test_prefill(D, G, T, n, kw):
    qkv, k, v, length, rope, ref = _case(D, G, (n, n), T, kw.get("window"), tile=8192 // (2 * D))
    out = ops.prefill_attention(qkv, G * HKV, k, v, length, n_kv_head=HKV, rope=rope, **kw)
    _check(out, ref)


@pytest.mark.parametrize("D,T,n,kw", [(64, 1, CHUNK_GQA + 1, {}), (128, 1, 299, {"window": 100}),
                                      (64, 5, 37, {}), (128, 8, 150, {"key_split": 128}),
                                      (128, 8, 150, {"window": 30})])
def test_identity_table(D, T, n, kw, G=4):
    ident = lambda P, D: torch.cat((torch.ones(P, D // 2), torch.zeros(P, D // 2)), 1)
    qkv, k, v, length, rope, _ = _case(D, G, (n, n), T, kw.get("window"), 8192 // (2 * D), ident)
    fn = functools.partial(ops.decode_attention if T == 1 else ops.prefill_attention, qkv,
                           G * HKV, k, v, length, n_kv_head=HKV, **kw)
    assert torch.equal(fn(rope=rope), fn())
    HQ = G * HKV
    assert torch.equal(k[:, :, n:n + T], qkv.view(2, T, -1, D)[:, :, HQ:HQ + HKV].transpose(1, 2))


@pytest.mark.parametrize("bad", [
    lambda r: dict(rope=r, n_kv_head=None), lambda r: dict(rope=r, n_kv_head=8),
    lambda r: dict(rope=r.double()), lambda r: dict(rope=r.repeat(1, 2)[:, :64]),
    lambda r: dict(rope=r[:, :32]), lambda r: dict(rope=r[:-1]), lambda r: dict(rope=r.cpu())])
def test_argument_errors(bad, HQ=8, D=64, L=8):
    qkv = torch.randn(2, 1, (HQ + 4) * D, device=DEV).bfloat16()
    kw = {"n_kv_head": HKV, **bad(U.table(L, D).to(DEV))}
    if kw["n_kv_head"] in (None, HQ):                          # the ungrouped layout
        qkv = torch.randn(2, 1, 3 * HQ * D, device=DEV).bfloat16()
    k, v = (torch.zeros(2, kw["n_kv_head"] or HQ, L, D, dtype=torch.bfloat16, device=DEV)
            for _ in "kv")
    length = torch.zeros(1, dtype=torch.int32, device=DEV)
    before = qkv.clone()
    for fn in (ops.kv_append, ops.decode_attention, ops.prefill_attention):
        with pytest.raises(ValueError, match="rope"):
            fn(qkv, HQ, k, v, length, **kw)
    assert not k.any() and not v.any() and not length.any() and torch.equal(qkv, before)
