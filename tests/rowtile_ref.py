"""Test helper for the C = 320 row-tile kernels (sd_xfront_f16, sd_xattn_chain_f16, sd_xtail_f16): plain torch, float64, on the CPU, one
function per kernel, each returning every tensor the kernel writes.

``exact=True``  no intermediate rounding at all: the truth a kernel is measured against.
``exact=False`` the same arithmetic with a round-to-fp16 exactly where the unfused launch graph stores an fp16 tensor (n, h, n1 for the
                front; h1, n2, q2, a2, h2 for the chain; the hidden tensor and h3 for the tail).  Its own distance from the truth is the
                yardstick of the per-row measure in tests/test_sd_rowtile_gpu.py.

All three kernels are local to a token row (the front once the GroupNorm statistics of the sample exist), so every function takes an
optional list of row indices and computes only those.  Inputs are taken as they are handed to the kernel (fp16 tensors); weights in
the diffusers layout (W1 / b1 of the GEGLU NOT interleaved).  Pinned against oracle.sd_oracle.transformer_ref by a CPU test.
Nothing here is product code."""
from __future__ import annotations

import math

import torch

C, HEADS, D = 320, 8, 40
F64 = torch.float64


def _d(t):
    return t.to(F64)


def _store(t, exact):
    """A tensor the unfused graph keeps in memory as fp16."""
    return t if exact else t.half().to(F64)


def _rows(rows, n):
    return torch.arange(n) if rows is None else torch.as_tensor(rows, dtype=torch.long)


def _layernorm(x, gamma, beta, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * _d(gamma) + _d(beta)


def xfront(x, gn_gamma, gn_beta, wpi, bpi, g1, b1, wq, wk, wv, *, rows_per_sample, gn_eps=1e-6, eps=1e-5, groups=32, exact, rows=None):
    """x [M, 320] -> dict(h [R, 320], qk [R, 640], v [R, 320]) for the R selected rows; v is token-major (the kernel writes it
    transposed per sample, keys of every 16 in the PERM16 order).  The GroupNorm statistics are always those of the whole sample."""
    M = x.shape[0]
    B, L = M // rows_per_sample, rows_per_sample
    xs = _d(x).reshape(B, L, groups, C // groups)
    mu = xs.mean((1, 3), keepdim=True)
    var = ((xs - mu) ** 2).mean((1, 3), keepdim=True)
    r = _rows(rows, M)
    b = r // L
    xr = _d(x[r]).reshape(-1, groups, C // groups)
    n = ((xr - mu[b, 0]) / torch.sqrt(var[b, 0] + gn_eps)).reshape(-1, C) * _d(gn_gamma) + _d(gn_beta)
    n = _store(n, exact)
    h = _store(n @ _d(wpi).t() + _d(bpi), exact)
    n1 = _store(_layernorm(h, g1, b1, eps), exact)
    return dict(h=h, qk=torch.cat([n1 @ _d(wq).t(), n1 @ _d(wk).t()], -1), v=n1 @ _d(wv).t())


def cross_attention(q, k, v, sample):
    """q [R, 320], k / v [B, lk, 320], sample [R] -> [R, 320]: softmax(q k^T / sqrt(40)) v per head, every row against its sample's keys."""
    out = torch.empty_like(q)
    for b in torch.unique(sample).tolist():
        m = sample == b
        qh = q[m].reshape(-1, HEADS, D).transpose(0, 1)                          # [H, R_b, d]
        kh, vh = (_d(t[b]).reshape(-1, HEADS, D).transpose(0, 1) for t in (k, v))   # [H, lk, d]
        p = torch.softmax(qh @ kh.transpose(1, 2) * D ** -0.5, -1)
        out[m] = (p @ vh).transpose(0, 1).reshape(-1, C)
    return out


def xchain(a, h, wo1, bo1, g2, b2, wq, k2, v2, wo2, bo2, g3, b3, *, rows_per_sample, eps=1e-5, exact, rows=None):
    """a (attn1 output), h [M, 320]; k2, v2 [B, lk, 320] (V NOT transposed) -> dict(h1, n2, q2, a2, h2, n3), each [R, 320]: the four
    debug stages and the two outputs of sd_xattn_chain_f16."""
    r = _rows(rows, a.shape[0])
    h1 = _store(_d(a[r]) @ _d(wo1).t() + _d(bo1) + _d(h[r]), exact)
    n2 = _store(_layernorm(h1, g2, b2, eps), exact)
    q2 = _store(n2 @ _d(wq).t(), exact)
    a2 = _store(cross_attention(q2, k2, v2, r // rows_per_sample), exact)
    h2 = _store(a2 @ _d(wo2).t() + _d(bo2) + h1, exact)
    return dict(h1=h1, n2=n2, q2=q2, a2=a2, h2=h2, n3=_layernorm(h2, g3, b3, eps))


def xtail(n3, h2, x, w1, b1, w2, b2, wpo, bpo, *, exact, rows=None, block=8192):
    """n3, h2, x [M, 320]; w1 [2560, 320] = [values ; gates], exact erf GELU -> out [R, 320]."""
    r = _rows(rows, n3.shape[0])
    w1d, b1d, w2d, wpod = _d(w1).t().contiguous(), _d(b1), _d(w2).t().contiguous(), _d(wpo).t().contiguous()
    inner = w2.shape[1]
    out = []
    for i in range(0, len(r), block):                    # the hidden tensor of 65536 rows in float64 is 1.3 GB: walk the rows in blocks
        rb = r[i:i + block]
        y = _d(n3[rb]) @ w1d + b1d
        gate = y[:, inner:]
        hid = _store(y[:, :inner] * (0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0)))), exact)
        h3 = _store(hid @ w2d + _d(b2) + _d(h2[rb]), exact)
        out.append(h3 @ wpod + _d(bpo) + _d(x[rb]))
    return torch.cat(out)


def row_error(got, truth):
    """Per row: || got - truth ||_2 / || truth ||_2 over the columns, in float64."""
    return (_d(got) - truth).norm(dim=-1) / truth.norm(dim=-1)
