"""The decode attention kernels (csrc/attn_decode.hip) against an fp32 softmax over the bf16
cache contents: every key position, chunk edges, the device-side length, agreement with the
prefill kernel, bit-exact appends, determinism and HIP-graph replay across positions."""

import math

import pytest
import torch

from distributed_llm_backend_benchmark_amd.ops import decode as dec
from distributed_llm_backend_benchmark_amd.ops.attention import attn_fwd
from distributed_llm_backend_benchmark_amd.ops.decode import CHUNK, decode_attention, kv_append

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _ref(q, K, V):
    """fp32 softmax attention of q [B, H, D] over K / V [B, H, L, D] (bf16 values) -> fp32."""
    D = q.shape[-1]
    s = (q.float()[:, :, None, :] * K.float()).sum(-1) / math.sqrt(D)        # [B, H, L]
    p = torch.softmax(s, dim=-1)
    return (p[..., None] * V.float()).sum(2), s


def _pack(q, k_new, v_new):
    """q / k_new / v_new [B, H, D] -> fused qkv [B, 1, 3C]."""
    B, H, D = q.shape
    return torch.cat([t.reshape(B, 1, H * D) for t in (q, k_new, v_new)], dim=2).contiguous()


def _case(B, H, D, L, L_max, seed):
    """Random q / K / V for L keys; a NaN-filled cache holding the first L - 1 of them, the last
    one as the token being decoded; length = L - 1 on the device."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, D, generator=g).to(torch.bfloat16).to(DEV)
    K = torch.randn(B, H, L, D, generator=g).to(torch.bfloat16).to(DEV)
    V = torch.randn(B, H, L, D, generator=g).to(torch.bfloat16).to(DEV)
    kc = torch.full((B, H, L_max, D), NAN, dtype=torch.bfloat16, device=DEV)
    vc = torch.full((B, H, L_max, D), NAN, dtype=torch.bfloat16, device=DEV)
    kc[:, :, :L - 1] = K[:, :, :L - 1]
    vc[:, :, :L - 1] = V[:, :, :L - 1]
    qkv = _pack(q, K[:, :, L - 1], V[:, :, L - 1])
    length = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
    return q, K, V, kc, vc, qkv, length


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("D", [64, 128])
def test_every_key_position_is_seen(D):
    """Batch entry b asks for key b: q_b = 16 k_b makes key b's score lead every other by >= 30
    (asserted from the fp32 reference), so the output must be v_b exactly — the leaked weight
    is < L e^-30, far below half a bf16 ulp. One launch, L = 2 CHUNK + 3 keys, B = L."""
    L = 2 * CHUNK + 3
    g = torch.Generator().manual_seed(11 + D)
    k = torch.randn(L, D, generator=g).to(torch.bfloat16).to(DEV)
    v = torch.randn(L, D, generator=g).to(torch.bfloat16).to(DEV)
    q = (k.float() * 16).to(torch.bfloat16)                      # exact: a power of two
    assert torch.equal(q.float(), k.float() * 16)
    K = k[None, None].expand(L, 1, L, D)
    V = v[None, None].expand(L, 1, L, D)
    want, s = _ref(q[:, None, :], K, V)
    top2 = s[:, 0].topk(2, dim=-1)
    assert torch.equal(top2.indices[:, 0], torch.arange(L, device=DEV))
    lead = float((top2.values[:, 0] - top2.values[:, 1]).min())
    assert lead >= 30, lead
    assert torch.equal(want[:, 0].to(torch.bfloat16), v)         # the reference itself is exact

    kc = torch.full((L, 1, L + 5, D), NAN, dtype=torch.bfloat16, device=DEV)
    vc = torch.full((L, 1, L + 5, D), NAN, dtype=torch.bfloat16, device=DEV)
    kc[:, :, :L - 1] = K[:, :, :L - 1]
    vc[:, :, :L - 1] = V[:, :, :L - 1]
    qkv = _pack(q[:, None, :], K[:, :, L - 1], V[:, :, L - 1])
    length = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
    got = decode_attention(qkv, 1, kc, vc, length)
    torch.cuda.synchronize()
    assert got.shape == (L, 1, D)
    wrong = (_bits(got[:, 0]) != _bits(v)).any(-1).nonzero().flatten().tolist()
    assert not wrong, f"batch entries (= key positions) with a wrong output: {wrong[:20]}"


LENGTHS = [1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17]


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("fused", [True, False])
def test_random_inputs_match_fp32(B, H, D, L, fused):
    """Bound 2^-7 max|want|: one bf16 rounding of the output is <= 2^-9 relative, fp32
    reassociation is orders below; the 4x margin is stated, not tuned. Cache rows >= L hold NaN:
    a read past the live length would show in the output."""
    L_max = L + 37
    q, K, V, kc, vc, qkv, length = _case(B, H, D, L, L_max, seed=1000 * D + 10 * L + B)
    got = decode_attention(qkv, H, kc, vc, length, fused=fused)
    torch.cuda.synchronize()
    want, _ = _ref(q, K, V)
    got = got.view(B, H, D).float()
    assert torch.isfinite(got).all()
    ratio = float((got - want).abs().max() / want.abs().max())
    print(f"decode B={B} H={H} D={D} L={L} fused={fused}: max|got-want|/max|want| = {ratio:.3e}")
    assert ratio <= 2.0 ** -7, f"max|got - want| / max|want| = {ratio:.3e} > 2^-7"
    # the token was appended at position L - 1, bit-exactly, and nothing after it was written
    assert torch.equal(_bits(kc[:, :, :L]), _bits(K)) and torch.equal(_bits(vc[:, :, :L]), _bits(V))
    assert torch.isnan(kc[:, :, L:].float()).all() and torch.isnan(vc[:, :, L:].float()).all()
    assert int(length) == L - 1                                   # not advanced


@pytest.mark.parametrize("D", [64, 128])
def test_length_is_read_on_the_device(D):
    """Same host arguments twice, the device length bumped in between (across a chunk edge):
    the second call appends at the new position and attends over one key more."""
    B, H, n0 = 2, 3, CHUNK - 1
    L_max = CHUNK + 40
    q, K, V, kc, vc, qkv, length = _case(B, H, D, n0 + 1, L_max, seed=77 + D)
    ws = torch.empty(dec.workspace_numel(B, H, D, L_max), dtype=torch.float32, device=DEV)
    outs = []
    for _ in range(2):
        outs.append(decode_attention(qkv, H, kc, vc, length, len_bound=L_max, workspace=ws)
                    .view(B, H, D).float())
        length.add_(1)
    torch.cuda.synchronize()
    assert int(length) == n0 + 2
    for i, got in enumerate(outs):
        Ki = torch.cat([K] + [K[:, :, -1:]] * i, dim=2)          # the token once more per call
        Vi = torch.cat([V] + [V[:, :, -1:]] * i, dim=2)
        want, _ = _ref(q, Ki, Vi)
        ratio = float((got - want).abs().max() / want.abs().max())
        assert ratio <= 2.0 ** -7, (i, ratio)
        assert torch.equal(_bits(kc[:, :, :n0 + 1 + i]), _bits(Ki))
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("T", [65, 200])
@pytest.mark.parametrize("D", [64, 128])
def test_agrees_with_the_prefill_kernel(T, D):
    """attn_fwd(qkv)[:, T - 1] against a decode step on a cache filled by kv_append from
    qkv[:, :T - 1]: two bf16 roundings of the same fp32 value, so 2 x 2^-7 = 2^-6."""
    B, H = 2, 3
    g = torch.Generator().manual_seed(5 * T + D)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(torch.bfloat16).to(DEV)
    full, _ = attn_fwd(qkv, H)
    kc = torch.full((B, H, T + 3, D), NAN, dtype=torch.bfloat16, device=DEV)
    vc = torch.full((B, H, T + 3, D), NAN, dtype=torch.bfloat16, device=DEV)
    length = torch.zeros(1, dtype=torch.int32, device=DEV)
    kv_append(qkv[:, :T - 1].contiguous(), H, kc, vc, length)
    length.fill_(T - 1)
    got = decode_attention(qkv[:, T - 1:].contiguous(), H, kc, vc, length)
    torch.cuda.synchronize()
    want = full[:, T - 1].float()
    ratio = float((got[:, 0].float() - want).abs().max() / want.abs().max())
    print(f"decode vs prefill T={T} D={D}: {ratio:.3e}")
    assert ratio <= 2.0 ** -6, ratio


@pytest.mark.parametrize("at_end", [False, True])
@pytest.mark.parametrize("T", [1, 70])
@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_is_bit_exact_and_writes_nothing_else(D, T, at_end):
    """The caches are contiguous views into larger sentinel-filled allocations: after the
    append every element outside positions [length, length + T) is unchanged — inside the cache
    and in the margins on both sides — and the appended rows equal the K / V rows of qkv."""
    B, H, L_max, margin = 2, 3, 80, 4096
    n = B * H * L_max * D
    start = L_max - T if at_end else 0
    g = torch.Generator().manual_seed(D + T)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(torch.bfloat16).to(DEV)
    bigs = [torch.full((n + 2 * margin,), s, dtype=torch.bfloat16, device=DEV)
            for s in (-12345.0, 54321.0)]
    kc, vc = (b[margin:margin + n].view(B, H, L_max, D) for b in bigs)
    want = [b.clone() for b in bigs]
    for j, w in enumerate(want):
        rows = qkv.view(B, T, 3, H, D)[:, :, 1 + j].permute(0, 2, 1, 3)     # [B, H, T, D]
        w[margin:margin + n].view(B, H, L_max, D)[:, :, start:start + T] = rows
    length = torch.tensor([start], dtype=torch.int32, device=DEV)
    kv_append(qkv, H, kc, vc, length, pos=start)
    torch.cuda.synchronize()
    for b, w in zip(bigs, want):
        assert torch.equal(_bits(b), _bits(w))
    with pytest.raises(ValueError):
        kv_append(qkv, H, kc, vc, length, pos=L_max - T + 1)                 # host overflow check


def test_two_runs_are_bit_identical():
    B, H, D, L = 2, 3, 128, 3 * CHUNK + 17
    outs = []
    for _ in range(2):
        _, _, _, kc, vc, qkv, length = _case(B, H, D, L, L + 37, seed=9)
        outs.append(decode_attention(qkv, H, kc, vc, length))
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize("D", [64, 128])
def test_graph_replay_walks_the_positions(D):
    """One captured decode_attention + length.add_(1), replayed 5 times on fixed inputs (single
    stream, no forked branches): after every replay the output equals the eager result for that
    position bit-exactly and the cache's newest row is the appended token."""
    B, H, p, steps = 2, 3, CHUNK - 2, 5
    L_max = p + steps + 3
    _, K, V, kc, vc, qkv, length = _case(B, H, D, p + 1, L_max, seed=31 + D)
    ws = torch.empty(dec.workspace_numel(B, H, D, L_max), dtype=torch.float32, device=DEV)
    kc2, vc2, len2 = kc.clone(), vc.clone(), length.clone()

    eager = []
    for _ in range(steps):
        eager.append(decode_attention(qkv, H, kc, vc, length, len_bound=L_max, workspace=ws)
                     .clone())
        length.add_(1)
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up: writes row p, the same token
        decode_attention(qkv, H, kc2, vc2, len2, len_bound=L_max, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = decode_attention(qkv, H, kc2, vc2, len2, len_bound=L_max, workspace=ws)
        len2.add_(1)
    assert int(len2) == p                                # the capture ran nothing
    tok_k, tok_v = K[:, :, -1], V[:, :, -1]
    for i in range(steps):
        graph.replay()
        torch.cuda.synchronize()
        assert int(len2) == p + i + 1
        assert torch.equal(_bits(out), _bits(eager[i])), f"replay {i}"
        assert torch.equal(_bits(kc2[:, :, p + i]), _bits(tok_k))
        assert torch.equal(_bits(vc2[:, :, p + i]), _bits(tok_v))
    assert torch.isnan(kc2[:, :, p + steps:].float()).all()
    assert not torch.equal(_bits(eager[0]), _bits(eager[-1]))
