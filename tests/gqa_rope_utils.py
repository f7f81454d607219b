"""The theta-10000 ``cos | sin`` table and the fp64 reference of the ``rope=`` tests (CPU and GPU)."""

import math

import torch


def table(P, D, theta=10000.0):
    """fp32 [P, D]: row p holds cos | sin of the D / 2 angles p * theta^(-i / (D / 2))."""
    inv = theta ** (-torch.arange(D // 2, dtype=torch.float64) / (D // 2))
    ang = torch.arange(P, dtype=torch.float64)[:, None] * inv
    return torch.cat((ang.cos(), ang.sin()), 1).float()


def rotate(x, rows):
    """fp64 rotate-half rotation of ``x [n, heads, D]`` by the table rows ``[n, D]``."""
    x, rows, h = x.double(), rows.double()[:, None], x.shape[-1] // 2
    lo, hi, cos, sin = x[..., :h], x[..., h:], rows[..., :h], rows[..., h:]
    return torch.cat((lo * cos - hi * sin, hi * cos + lo * sin), -1)


def reference(rows, rope, n, T, G, HKV, W=None):
    """fp64 attention of tokens [n, n + T) of ``rows [n + T, H_q + 2 H_kv, D]`` (bf16 bits), Q and
    K rotated in fp64 at their positions and rounded to bf16 (the cache's contract), each token
    over its last W keys (None: all) -> [T, H_q * D] fp64."""
    HQ, D = G * HKV, rows.shape[2]
    x = rows.double().cpu()
    qk = rotate(x[:, :HQ + HKV], rope[:n + T].cpu()).bfloat16().double()
    kv_of = torch.arange(HQ) // G                              # query head h -> KV head h // G
    s = torch.einsum("thd,khd->htk", qk[n:, :HQ], qk[:, HQ + kv_of]) / math.sqrt(D)
    band = torch.ones(T, n + T, dtype=torch.bool).tril(n)
    if W is not None:
        band = band.triu(n - W + 1)
    s.masked_fill_(~band, -math.inf)
    return torch.einsum("htk,khd->thd", s.softmax(-1), x[:, HQ + HKV + kv_of]).reshape(T, HQ * D)
