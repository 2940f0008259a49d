"""Test helper for sd_conv_gemm_f16 (coma_amd/csrc/sd_gemm.hip): plain torch on the CPU, nothing here is product code and nothing here
needs a GPU.

* ``CASES``            the table of launches, shared by tests/test_gemm_ref_host.py (choice record, emulation, coverage) and
                       tests/test_sd_gemm_domain_gpu.py.  Every row names the tile family it is meant to reach (``TILES``) and whether the
                       K loop runs on 16x16x32 MFMAs; sd_conv_gemm_describe is the judge of both.
* ``make_inputs``      fp16 operands of a case, seeded by its name: x, res, bias, bias_bn ~ N(0, 1), w ~ N(0, 1) / sqrt(K).
* ``yardstick``        the float64 reference (an explicit gather of (b, oy * stride - pad + dy, ox * stride - pad + dx) over the optional
                       nearest-x2 source, then a float64 matmul and the epilogue of include/sd_hip.h), the fp16 emulation (exact products,
                       fp32 sums in K index order, per split with split-K, fp32 epilogue with exact exp / erf, one rounding), its distance
                       from the reference e_emu -- each element's error over the largest |ref| of its output row -- the device bound
                       max(4 e_emu, 2^-10), and the emulation's own a-priori bound.
* ``pack``             flat buffers as the kernel sees them: 256 NaN halves in front of and behind every operand, NaN gap columns and
                       inter-problem gaps, a NaN-filled workspace, sentinel-filled outputs with guards (the guard width, the sentinels,
                       the seeds, the device bound and the refusal rows' PTR are tests/domain_kit.py's).
* ``written_mask`` ... which elements of `out` / `out_t` / `colstats` a launch must write; everything else must keep the sentinel.

DESIGN.md section 3c has the numbers."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import torch

from tests import domain_kit as kit
from tests.domain_kit import F16, F32, F64, GUARD, PTR, U32, device_bound, exp32

LIP = 1.13                       # Lipschitz constant of SiLU / quick GELU (1.0999) and of the erf GELU (1.129)
SAMPLE_ABOVE = 2.0e9             # multiply-adds of a launch above which only sampled_rows() are compared
EPI_GEGLU, EPI_SILU, EPI_BIAS_ROWS, EPI_PERM16, EPI_PERM32, EPI_QGELU = 1, 2, 4, 8, 16, 32

# (bm, bn, bk, stages, waves, tm, spread): the 13 launch lines of the dispatch
TILES = {
    "256x320s": (256, 320, 64, 2, 8, 2, 1), "256x320": (256, 320, 64, 2, 8, 2, 0),
    "256x256s": (256, 256, 64, 2, 8, 2, 1), "256x256": (256, 256, 64, 2, 8, 2, 0),
    "256x128w4": (256, 128, 32, 3, 4, 2, 0), "256x128w8": (256, 128, 64, 2, 8, 2, 0),
    "128x320w8": (128, 320, 64, 2, 8, 1, 1), "128x320w4": (128, 320, 32, 3, 4, 2, 0),
    "128x128k64s": (128, 128, 64, 2, 4, 2, 1), "128x128k64": (128, 128, 64, 2, 4, 2, 0), "128x128k32": (128, 128, 32, 4, 4, 2, 0),
    "128x64k64": (128, 64, 64, 2, 4, 2, 0), "128x64k32": (128, 64, 32, 4, 4, 2, 0),
}
# Which (tile, m16) the dispatch can produce.  m16 = (K >= 256).  The four spread lines of a 3x3 cannot run with m16 off: a 3x3 has
# K >= 288 (and the 64-deep ones K >= 576).  BK = 64 outside the 256-row tiles needs K >= 1024 or (128x320, 8 waves) K >= 256; the 8-wave
# 256 x 128 tile is only taken above K = 1152.  Everything else runs both ways: 19 instantiations of the 26 the file compiles.
REACHABLE = ({(t, 1) for t in TILES} | {(t, 0) for t in ("256x320", "256x256", "256x128w4", "128x320w4", "128x128k32", "128x64k32")})


@dataclass(frozen=True)
class Case:
    name: str
    tile: str                   # expected launch line (TILES)
    m16: int                    # expected MFMA shape of the K loop
    B: int
    H: int                      # source image
    W: int
    c0: int
    n: int
    c1: int = 0
    taps: int = 1               # 1 | 9 | 4 (phase)
    stride: int = 1
    pad: int = 1
    up: int = 0
    epi: int = 0
    bias: bool = False
    bias_bn: bool = False
    res: bool = False
    dldo: int = 0               # ldo = width of an `out` row + dldo (0: the descriptor's default, ldo = 0)
    dldr: int = 0
    dldbb: int = 0
    nz: int = 1
    zgap: Tuple[int, int, int] = (0, 0, 0)      # halves between the problems of a z-batched launch: A, W, out (and res)
    ws_slabs: int = 0           # workspace = this many M x N fp32 slabs (0: none, split-K off)
    ksplit: int = 1             # expected split-K factor
    colstats: bool = False
    out_t: Optional[Tuple[int, int, int]] = None    # (n_split, rows_per_sample, ldo_t - rows_per_sample)
    phase: int = 0              # 1..4: one sub-pixel phase launch; 5: all four into one `out`
    family: str = ""            # the pool DESIGN.md reports the case under (default: the tile)

    @property
    def id(self):
        return self.name

    @property
    def pool(self):
        return self.family or self.tile

    # ---- geometry
    def _o(self, size):
        if self.up:
            return 2 * size
        if self.stride == 2:
            return (size - 2) // 2 + 1 if (self.taps == 9 and self.pad == 0) else (size - 1) // 2 + 1
        return size

    @property
    def out_h(self):
        return self._o(self.H)

    @property
    def out_w(self):
        return self._o(self.W)

    @property
    def rpb(self):              # product rows per sample
        return self.out_h * self.out_w

    @property
    def M(self):
        return self.B * self.rpb

    @property
    def Mo(self):               # rows of `out` per problem
        return 4 * self.M if self.phase else self.M

    @property
    def K(self):
        return self.taps * (self.c0 + self.c1)

    @property
    def N(self):                # product columns
        return roundup(self.n, 16) if self.epi & EPI_PERM16 else self.n

    @property
    def ow(self):               # columns of an `out` row the launch writes
        if self.epi & EPI_GEGLU:
            return self.n // 2
        if self.out_t:
            return self.out_t[0]
        return self.N

    @property
    def ldo(self):
        return self.ow + self.dldo

    @property
    def ldr(self):
        return self.n + self.dldr

    @property
    def ldbb(self):
        return self.n + self.dldbb

    @property
    def macs(self):
        return self.nz * self.M * self.N * self.K * max(1, len(self.phases))

    @property
    def phases(self):
        return () if not self.phase else ((1, 2, 3, 4) if self.phase == 5 else (self.phase,))

    def strides(self):
        """Element strides between the problems of a z-batched launch -> (a, w, out, res)."""
        if self.nz == 1:
            return 0, 0, 0, 0
        ga, gw, go = self.zgap
        return self.B * self.H * self.W * self.c0 + ga, self.n * self.K + gw, self.Mo * self.ldo + go, self.M * self.ldr + go

    def ws_floats(self):
        return self.ws_slabs * self.M * self.N


def roundup(n, m):
    return (n + m - 1) // m * m


def kappa16(j):
    """W row held by output position j with SD_EPI_PERM16_N: every group of 16 positions holds rows (0-3, 8-11, 4-7, 12-15)."""
    return (j & ~12) | ((j & 4) << 1) | ((j & 8) >> 1)


def kappa32(p):
    """W row held by output position p = 8g + e of a group of 32 with SD_EPI_PERM32_N: 16 (e >> 2) + 4g + (e & 3)."""
    g, e = (p >> 3) & 3, p & 7
    return (p & ~31) | (16 * (e >> 2) + 4 * g + (e & 3))


def geglu_rows(n):
    """Interleaved weight row of (value j, gate j), j < n / 2: per 32 outputs the product holds [32 value columns | 32 gate columns]."""
    j = torch.arange(n // 2)
    v = (j // 32) * 64 + j % 32
    return v, v + 32


def out_row(c: Case, m, phase):
    """Row of `out` that product row m = (b, y, x) of a phase launch writes: pixel (2y + a, 2x + b) of the [B, 2H, 2W] image."""
    a, b = (phase - 1) >> 1, (phase - 1) & 1
    bi, r = m // (c.H * c.W), m % (c.H * c.W)
    y, x = r // c.W, r % c.W
    return (bi * 2 * c.H + 2 * y + a) * 2 * c.W + 2 * x + b


# ---------------------------------------------------------------------------------------------------------------- inputs
class Inputs(NamedTuple):
    x: torch.Tensor                 # fp16 [nz, B, H, W, c0 + c1]
    w: torch.Tensor                 # fp16 [nz, n, K]; a phase case: the UNSUMMED 3x3 weights [1, n, 9, c]
    bias: Optional[torch.Tensor]    # fp16 [n] ([M] with BIAS_ROWS)
    bias_bn: Optional[torch.Tensor]  # fp16 [B, n]
    res: Optional[torch.Tensor]     # fp16 [nz, M, n]


def make_inputs(c: Case) -> Inputs:
    g = kit.gen(c.name)
    ctot = c.c0 + c.c1
    x = torch.randn(c.nz, c.B, c.H, c.W, ctot, generator=g).to(F16)
    if c.phase:
        # unsummed 3x3 weights on a 2^-12 grid below 2^-3: every sum of up to four of them is exact in fp16, so the four summed-tap
        # products ARE the 3x3 convolution of the upsampled image, with nothing rounded in between
        w = torch.randn(1, c.n, 9, ctot, generator=g) / math.sqrt(9 * ctot)
        w = (torch.round(w * 4096) / 4096).clamp(-0.125 + 2.0 ** -12, 0.125 - 2.0 ** -12).to(F16)
    else:
        w = (torch.randn(c.nz, c.n, c.K, generator=g) / math.sqrt(c.K)).to(F16)
    bias = torch.randn(c.M if c.epi & EPI_BIAS_ROWS else c.n, generator=g).to(F16) if c.bias else None
    bias_bn = torch.randn(c.B, c.n, generator=g).to(F16) if c.bias_bn else None
    res = torch.randn(c.nz, c.M, c.n, generator=g).to(F16) if c.res else None
    return Inputs(x, w, bias, bias_bn, res)


def phase_weights(w3, phase):
    """[n, 9, c] unsummed 3x3 weights -> [n, 4 * c] of one phase: window position (dy, dx) carries the sum of the taps that land on it.
    Row 2y + a - 1 + ky of the upsampled image is source row y + floor((a - 1 + ky) / 2): a = 0 -> (y-1 | y, y), a = 1 -> (y, y | y+1)."""
    a, b = (phase - 1) >> 1, (phase - 1) & 1
    n, _, ctot = w3.shape
    out = torch.zeros(n, 2, 2, ctot, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            out[:, (a - 1 + ky) // 2 + 1 - a, (b - 1 + kx) // 2 + 1 - b] += w3[:, 3 * ky + kx].to(F64)
    h = out.to(F16)
    assert torch.equal(h.to(F64), out), "the summed phase weights must be exact in fp16"
    return h.reshape(n, 4 * ctot)


# ---------------------------------------------------------------------------------------------------------------- gather
def gather(x, rows, *, out_h, out_w, window, stride, pad_y, pad_x, up):
    """x [B, H, W, C] -> A [R, taps, C] (x's dtype): row m = (b, oy, ox) of `rows`, tap (dy, dx) of the window x window stencil, reads pixel
    (oy * stride - pad_y + dy, ox * stride - pad_x + dx) of the image -- of its nearest-x2 upsampling with up -- or zero outside it."""
    B, H, W, C = x.shape
    b, r = rows // (out_h * out_w), rows % (out_h * out_w)
    oy, ox = r // out_w, r % out_w
    lim_h, lim_w = (2 * H, 2 * W) if up else (H, W)
    A = torch.zeros(rows.numel(), window * window, C, dtype=x.dtype)
    for dy in range(window):
        for dx in range(window):
            iy, ix = oy * stride - pad_y + dy, ox * stride - pad_x + dx
            ok = (iy >= 0) & (iy < lim_h) & (ix >= 0) & (ix < lim_w)
            if up:
                iy, ix = iy // 2, ix // 2
            A[ok, dy * window + dx] = x[b[ok], iy[ok], ix[ok]]
    return A


def operands(c: Case, inp: Inputs, z, rows, phase=0):
    """-> (A [R, K], Wm [n, K]) fp16 values of problem z as the launch multiplies them, K = (tap, channel of the concatenation)."""
    xz = inp.x[z]
    if phase:
        a, b = (phase - 1) >> 1, (phase - 1) & 1
        A = gather(xz, rows, out_h=c.H, out_w=c.W, window=2, stride=1, pad_y=1 - a, pad_x=1 - b, up=0)
        return A.reshape(rows.numel(), -1), phase_weights(inp.w[0], phase)
    if c.taps == 9:
        A = gather(xz, rows, out_h=c.out_h, out_w=c.out_w, window=3, stride=c.stride, pad_y=c.pad, pad_x=c.pad, up=c.up)
    else:
        A = gather(xz, rows, out_h=c.out_h, out_w=c.out_w, window=1, stride=c.stride, pad_y=0, pad_x=0, up=0)
    return A.reshape(rows.numel(), -1), inp.w[z]


def sampled_rows(c: Case):
    """Product rows compared with the reference.  All of them, unless the launch has more than SAMPLE_ABOVE multiply-adds: then every row
    of the first and of the last M tile, of the tile(s) at the first sample boundary, every border pixel of the first and last sample, and
    256 rows drawn at random."""
    M = c.M
    if c.macs <= SAMPLE_ABOVE:
        return torch.arange(M)
    bm = TILES[c.tile][0]
    pick = torch.zeros(M, dtype=torch.bool)
    pick[:bm] = True
    pick[(M - 1) // bm * bm:] = True
    if c.B > 1:
        t = c.rpb // bm * bm
        pick[t:t + bm] = True
        if c.rpb % bm == 0:
            pick[t - bm:t] = True
    r = torch.arange(c.rpb)
    edge = (r // c.out_w == 0) | (r // c.out_w == c.out_h - 1) | (r % c.out_w == 0) | (r % c.out_w == c.out_w - 1)
    pick[:c.rpb] |= edge
    pick[M - c.rpb:] |= edge
    g = kit.gen(c.name + "/rows")
    pick[torch.randperm(M, generator=g)[:256]] = True
    return torch.nonzero(pick).flatten()


# ---------------------------------------------------------------------------------------------------------------- arithmetic
def sum_in_order(A, Wm, lo, hi):
    """fp32 sum over k = lo .. hi-1 of A[:, k] * Wm[:, k], added in index order (an fp16 x fp16 product is exact in fp32)."""
    s = torch.zeros(A.shape[0], Wm.shape[0], dtype=F32)
    At, Wt = A.to(F32).t().contiguous(), Wm.to(F32).t().contiguous()
    for k in range(lo, hi):
        s.addcmul_(At[k][:, None], Wt[k][None, :])
    return s


def emulate_product(A, Wm, ksplit, bk):
    """The product as a careful fp16 kernel makes it: exact products, fp32 accumulation in K index order; with split-K every split of
    ceil(K / bk / ksplit) K tiles on its own, the splits then added in fp32 in split order."""
    K = A.shape[1]
    if ksplit <= 1:
        return sum_in_order(A, Wm, 0, K)
    per = -(-(K // bk) // ksplit) * bk
    tot = torch.zeros(A.shape[0], Wm.shape[0], dtype=F32)
    for s in range(ksplit):
        lo, hi = s * per, min((s + 1) * per, K)
        tot += sum_in_order(A, Wm, lo, max(lo, hi))
    return tot


def _act(epi, v):
    """SiLU / quick GELU of fp32 or float64 `v` in its own precision, the exponential exact."""
    if epi & EPI_SILU:
        return v / (1 + (torch.exp(-v) if v.dtype == F64 else exp32(-v)))
    if epi & EPI_QGELU:
        return v / (1 + (torch.exp(-1.702 * v) if v.dtype == F64 else exp32(-(v * 1.702))))
    return v


def _gelu(v):
    """erf GELU, exact: float64, rounded once when v is fp32."""
    return (0.5 * v.to(F64) * (1 + torch.erf(v.to(F64) / math.sqrt(2.0)))).to(v.dtype)


def epilogue(c: Case, acc, inp: Inputs, z, rows, absacc=None):
    """acc [R, n] (fp32: the emulation; float64: the reference) -> the values of the `out` row and of the out_t columns, in acc's precision
    and in the order of include/sd_hip.h: acc + bias (+ per-sample bias) -> SiLU / quick GELU -> + residual; GEGLU = value * gelu(gate).
    absacc (float64 only): sum_k |a_k w_k| per element -> also returns the a-priori bound of the fp32 epilogue's error BEFORE the final
    rounding: the sum's (K + 4) u S, one u (S + |bias| ..) per addition, LIP through an activation, 8 u |f| for the activation's own
    arithmetic (u = 2^-24)."""
    dt = acc.dtype
    pre, mag = acc, absacc
    err = None if mag is None else (c.K + 4) * U32 * mag
    if inp.bias is not None:
        bv = inp.bias[rows][:, None] if c.epi & EPI_BIAS_ROWS else inp.bias[None, :]
        pre = pre + bv.to(dt)
        if mag is not None:
            mag = mag + bv.to(F64).abs()
            err = err + U32 * mag
    if inp.bias_bn is not None:
        bb = inp.bias_bn[rows // c.rpb]
        pre = pre + bb.to(dt)
        if mag is not None:
            mag = mag + bb.to(F64).abs()
            err = err + U32 * mag
    if c.epi & EPI_GEGLU:
        iv, ig = geglu_rows(c.n)
        gl = _gelu(pre[:, ig])
        v = pre[:, iv] * gl
        if err is not None:
            err = gl.abs() * err[:, iv] + (pre[:, iv].abs() + err[:, iv]) * LIP * err[:, ig] + 8 * U32 * v.abs()
    else:
        v = _act(c.epi, pre)
        if err is not None and c.epi & (EPI_SILU | EPI_QGELU):
            err = LIP * err + 8 * U32 * v.abs()
    if inp.res is not None:
        r = inp.res[z][rows]
        if err is not None:
            err = err + U32 * (v.abs() + r.to(F64).abs() + err)
        v = v + r.to(dt)
    if c.epi & EPI_PERM16:
        src = kappa16(torch.arange(c.N)).clamp(max=c.n - 1)          # positions whose row is >= n: "a clamped finite row", not compared
        v = v[:, src]
        err = None if err is None else err[:, src]
    if c.epi & EPI_PERM32:
        src = kappa32(torch.arange(c.n))
        v = v[:, src]
        err = None if err is None else err[:, src]
    return v, err


def compared_columns(c: Case):
    """Columns of the epilogue's value whose content the contract defines (all but the PERM16 positions whose W row is >= n)."""
    if c.epi & EPI_PERM16:
        return kappa16(torch.arange(c.N)) < c.n
    return torch.ones(c.n // 2 if c.epi & EPI_GEGLU else c.n, dtype=torch.bool)


def row_error(got, ref, cols, split=None):
    """max over an output row's compared columns of |got - ref| / max |ref| of that row -> [.., R].  split: out_t cases, where columns
    [0, split) are a row of `out` and [split, n) a row's share of out_t -- each normalised on its own.  (An out_t element's own row is the
    transposed one, over the keys of a sample; a sampled case does not hold whole ones, so its yardstick is the product row's out_t
    columns: values of the same distribution and as many or more of them, 640+ against rows_per_sample.)"""
    if split is not None:
        return torch.maximum(row_error(got[..., :split], ref[..., :split], cols[:split]), row_error(got[..., split:], ref[..., split:], cols[split:]))
    g, r = got.to(F64)[..., cols], ref[..., cols]
    return (g - r).abs().amax(-1) / r.abs().amax(-1)


class Yardstick(NamedTuple):
    rows: torch.Tensor          # product rows compared [R]; a phase case: rows of `out` (pixels of the upsampled image)
    ref: torch.Tensor           # float64 [nz, R, n-or-N-or-n/2]: the epilogue's values, out_t columns included
    cols: torch.Tensor          # bool: columns compared
    e_emu: float
    bound: float
    emu_over_stated: float      # max over elements of |emulation - ref| / a-priori bound of the emulation (must be <= 1)


@functools.lru_cache(maxsize=4)
def yardstick(c: Case) -> Yardstick:
    inp = make_inputs(c)
    ksplit, bk = c.ksplit, TILES[c.tile][2]
    cols = compared_columns(c)
    split = c.out_t[0] if c.out_t else None
    refs, e_emu, worst, rows_out = [], 0.0, 0.0, None
    launches = c.phases or (0,)
    rows = sampled_rows(c)
    for z in range(c.nz):
        ref_z = []
        for ph in launches:
            A, Wm = operands(c, inp, z, rows, ph)
            A64, W64 = A.to(F64), Wm.to(F64)
            ref, err = epilogue(c, A64 @ W64.t(), inp, z, rows, absacc=A64.abs() @ W64.abs().t())
            emu = epilogue(c, emulate_product(A, Wm, ksplit, bk), inp, z, rows)[0].to(F16)
            assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(emu.float()).all())
            # err bounds the fp32 value v before the last rounding to first order.  1.001 covers what that leaves out: the rounding acts on v,
            # not on ref (2^-11 err), and each addition's 2^-24 acts on the computed partial, not the exact one (2^-24 err per term).
            # 2^-25 is half the spacing of fp16 subnormals: below 2^-14 the last rounding is absolute, not relative.
            stated = 1.001 * err + 2.0 ** -11 * ref.abs() + 2.0 ** -25
            worst = max(worst, float(((emu.to(F64) - ref).abs() / stated)[:, cols].max()))
            e_emu = max(e_emu, float(row_error(emu, ref, cols, split).max()))
            ref_z.append(ref)
        refs.append(torch.cat(ref_z))
    if c.phase:
        rows = torch.cat([out_row(c, rows, ph) for ph in launches])
    return Yardstick(rows, torch.stack(refs), cols, e_emu, device_bound(e_emu), worst)


def reference(c: Case, inp: Inputs, z=0, rows=None, phase=0):
    """float64 values of one launch of the case on product rows `rows` (default: all)."""
    rows = torch.arange(c.M) if rows is None else rows
    A, Wm = operands(c, inp, z, rows, phase)
    return epilogue(c, A.to(F64) @ Wm.to(F64).t(), inp, z, rows)[0]


def reference_3x3_upsampled(c: Case, inp: Inputs):
    """A phase case the long way: conv3x3 of the nearest-x2 upsampled image with the UNSUMMED weights (+ bias) -> float64 [4 M, n]."""
    rows = torch.arange(4 * c.M)
    A = gather(inp.x[0], rows, out_h=2 * c.H, out_w=2 * c.W, window=3, stride=1, pad_y=1, pad_x=1, up=1).reshape(4 * c.M, -1)
    ref = A.to(F64) @ inp.w[0].reshape(c.n, -1).to(F64).t()
    return ref + inp.bias.to(F64)[None, :] if inp.bias is not None else ref


# ---------------------------------------------------------------------------------------------------------------- packing
def _nan(n):
    return torch.full((n,), float("nan"), dtype=F16)


def pack_blocks(blocks, ld, width, stride):
    """blocks [Z, rows, width] -> flat fp16: GUARD NaN | problem z at z * stride, rows of ld halves | GUARD NaN; gap columns and the
    space between problems NaN.  The kernel's pointer is buf[GUARD:]."""
    Z, R, _ = blocks.shape
    span = (Z - 1) * stride + R * ld
    buf = _nan(GUARD + span + GUARD)
    for z in range(Z):
        buf[GUARD + z * stride:GUARD + z * stride + R * ld].view(R, ld)[:, :width] = blocks[z]
    return buf


class Packed(NamedTuple):
    a0: torch.Tensor
    a1: Optional[torch.Tensor]
    w: Tuple[torch.Tensor, ...]         # one per launch (four for phase = 5)
    bias: Optional[torch.Tensor]
    bias_bn: Optional[torch.Tensor]
    res: Optional[torch.Tensor]


def pack(c: Case, inp: Inputs) -> Packed:
    sa, sw, _, sr = c.strides()
    npix = c.B * c.H * c.W
    x = inp.x.reshape(c.nz, npix, c.c0 + c.c1)
    a0 = pack_blocks(x[:, :, :c.c0], c.c0, c.c0, sa)
    a1 = pack_blocks(x[:, :, c.c0:], c.c1, c.c1, 0) if c.c1 else None
    if c.phase:
        w = tuple(pack_blocks(phase_weights(inp.w[0], ph)[None], c.K, c.K, 0) for ph in c.phases)
    else:
        w = (pack_blocks(inp.w, c.K, c.K, sw),)
    bias = pack_blocks(inp.bias[None, None], inp.bias.numel(), inp.bias.numel(), 0) if inp.bias is not None else None
    bias_bn = pack_blocks(inp.bias_bn[None], c.ldbb, c.n, 0) if inp.bias_bn is not None else None
    res = pack_blocks(inp.res, c.ldr, c.n, sr) if inp.res is not None else None
    return Packed(a0, a1, w, bias, bias_bn, res)


def out_elems(c: Case):
    return (c.nz - 1) * c.strides()[2] + c.Mo * c.ldo


def out_t_shape(c: Case):
    n_split, rps, d = c.out_t
    return c.M // rps, c.n - n_split, rps + d


def colstats_slots(c: Case):
    return c.Mo // 32


def new_out(c: Case):
    return kit.sentinel(GUARD + out_elems(c) + GUARD, F16)


def new_out_t(c: Case):
    return kit.sentinel(GUARD + math.prod(out_t_shape(c)) + GUARD, F16)


def new_colstats(c: Case):
    return kit.sentinel(GUARD + colstats_slots(c) * 2 * c.n + GUARD, F32)


def new_workspace(c: Case):
    return torch.full((GUARD + c.ws_floats() + GUARD,), float("nan"), dtype=F32)


def written_rows(c: Case):
    """Rows of `out` (per problem) the launch(es) of the case write."""
    if not c.phase:
        return torch.arange(c.M)
    return torch.cat([out_row(c, torch.arange(c.M), ph) for ph in c.phases])


def written_mask(c: Case):
    """bool over the whole `out` buffer (guards included): the elements the case must write."""
    mask = torch.zeros(GUARD + out_elems(c) + GUARD, dtype=torch.bool)
    so, rows = c.strides()[2], written_rows(c)
    for z in range(c.nz):
        body = mask[GUARD + z * so:GUARD + z * so + c.Mo * c.ldo].view(c.Mo, c.ldo)
        body[rows, :c.ow] = True
    return mask


def out_values(c: Case, buf, rows):
    """The `out` rows `rows` of every problem, columns [0, ow) -> fp16 [nz, R, ow]."""
    so = c.strides()[2]
    return torch.stack([buf[GUARD + z * so:GUARD + z * so + c.Mo * c.ldo].view(c.Mo, c.ldo)[rows, :c.ow] for z in range(c.nz)])


def out_t_values(c: Case, buf_t, rows):
    """Product rows `rows`, columns [n_split, n), read back out of out_t [M / rps][n - n_split][ldo_t]: element (b, ch, pos) is product row
    b * rps + key(pos), the keys of every group of 16 positions in the order (0-3, 8-11, 4-7, 12-15)."""
    nb, cv, ldt = out_t_shape(c)
    rps = c.out_t[1]
    body = buf_t[GUARD:GUARD + nb * cv * ldt].view(nb, cv, ldt)
    pos = kappa16(rows % rps)                                        # kappa16 is an involution: key k sits at position kappa16(k)
    return body[rows // rps, :, pos]                                 # [R, cv]


def out_t_written_mask(c: Case):
    nb, cv, ldt = out_t_shape(c)
    mask = torch.zeros(GUARD + nb * cv * ldt + GUARD, dtype=torch.bool)
    mask[GUARD:GUARD + nb * cv * ldt].view(nb, cv, ldt)[:, :, :c.out_t[1]] = True
    return mask


def colstats_expected(c: Case, out_buf):
    """float64 column sums and sums of squares of the device's own stored `out`, per 32-row block -> (slots written [S], sums [S, n],
    squares [S, n], sum |o| [S, n]).  A phase launch: phase p of sample b owns slots [(4 b + p - 1) per, (4 b + p) per), per = H W / 32,
    block j of them being product rows b H W + 32 j .. + 31 of that phase."""
    body = out_buf[GUARD:GUARD + c.Mo * c.ldo].view(c.Mo, c.ldo)[:, :c.n].to(F64)
    if not c.phase:
        blk = body.view(c.M // 32, 32, c.n)
        return torch.arange(c.M // 32), blk.sum(1), (blk * blk).sum(1), blk.abs().sum(1)
    per, slots, vals = c.H * c.W // 32, [], []
    for ph in c.phases:
        o = body[out_row(c, torch.arange(c.M), ph)].view(c.B, per, 32, c.n)
        for b in range(c.B):
            slots.append((4 * b + ph - 1) * per + torch.arange(per))
            vals.append(o[b])
    blk = torch.cat(vals)
    return torch.cat(slots), blk.sum(1), (blk * blk).sum(1), blk.abs().sum(1)


# ---------------------------------------------------------------------------------------------------------------- launch arguments
def launch_kwargs(c: Case, ptr, launch=0):
    """Keyword arguments of coma_amd.sd.ops.conv_gemm / conv_gemm_describe for launch `launch` of the case (a phase = 5 case has four).
    ptr: name -> tensor (or integer address) of a0, a1, w, bias, bias_bn, res, out, workspace, colstats, out_t, each already moved past
    its front guard."""
    sa, sw, so, sr = c.strides()
    kw = dict(batch=c.B, in_h=c.H, in_w=c.W, out_h=c.out_h, out_w=c.out_w, c0=c.c0, c1=c.c1, n=c.n, taps=c.taps, stride=c.stride,
              upsample=c.up, pad=c.pad, epi=c.epi, nbatch_z=c.nz, stride_a=sa, stride_w=sw, stride_out=so, stride_res=sr if c.res else 0,
              phase=c.phases[launch] if c.phase else 0)
    if c.c1:
        kw["a1"] = ptr["a1"]
    for k, on in (("bias", c.bias), ("bias_bn", c.bias_bn), ("res", c.res), ("colstats", c.colstats)):
        if on:
            kw[k] = ptr[k]
    if c.dldo or c.epi & EPI_PERM16 or c.out_t:
        kw["ldo"] = c.ldo
    if c.dldr:
        kw["ldr"] = c.ldr
    if c.dldbb:
        kw["ldbb"] = c.ldbb
    if c.ws_slabs:
        kw.update(workspace=ptr["workspace"], workspace_bytes=c.ws_floats() * 4)
    if c.out_t:
        kw.update(out_t=ptr["out_t"], n_split=c.out_t[0], rows_per_sample=c.out_t[1], ldo_t=c.out_t[1] + c.out_t[2])
    return kw


FAKE = {k: 0x100000000 + 0x10000000 * i for i, k in enumerate(("a0", "a1", "w", "bias", "bias_bn", "res", "out", "workspace", "colstats", "out_t"))}


def describe(ops, c: Case, launch=0):
    """The library's choice for the case's launch, from never-dereferenced addresses: no GPU needed."""
    return ops.conv_gemm_describe(FAKE["a0"], FAKE["w"], FAKE["out"], **launch_kwargs(c, FAKE, launch))


# ---------------------------------------------------------------------------------------------------------------- the case table
def _build_cases():
    cases = []

    def add(name, tile, m16, B, H, W, c0, n, **kw):
        cases.append(Case(name, tile, m16, B, H, W, c0, n, **kw))

    S, Q, R_, P16, P32, G = EPI_SILU, EPI_QGELU, EPI_BIAS_ROWS, EPI_PERM16, EPI_PERM32, EPI_GEGLU
    # ================================================================ the tile families, smallest shapes that reach each
    # ---- 256 x 320, 8 waves: N % 320 == 0 and ceil(M / 256) (N / 320) nz >= 192
    add("big-1x1-k64", "256x320", 0, 3, 128, 128, 64, 320, bias=True)                                   # M = 49152: 192 tiles exactly
    add("big-1x1-k256", "256x320", 1, 3, 128, 128, 256, 320, res=True)
    add("big-3x3-tapminor", "256x320s", 1, 3, 128, 128, 64, 320, taps=9, bias=True, bias_bn=True, epi=S)     # one N tile -> tap-minor
    add("big-3x3-tapmajor-ragged", "256x320s", 1, 1, 363, 67, 64, 640, taps=9, bias=True)                # M = 24321 = 95 * 256 + 1
    add("big-zplain", "256x320", 0, 1, 24, 32, 64, 1280, nz=16, zgap=(64, 128, 8))                       # M = 768: 3 x 4 x 16 = 192 tiles
    add("big-colstats", "256x320", 1, 3, 128, 128, 256, 320, bias_bn=True, colstats=True)
    add("big-ldo", "256x320", 0, 3, 128, 128, 64, 320, bias=True, res=True, dldo=8, dldr=16)
    # ---- 256 x 256: N % 256 == 0, M >= 32768
    add("b256-1x1-k64", "256x256", 0, 2, 128, 128, 64, 256, bias=True, epi=Q)
    add("b256-1x1-k256", "256x256", 1, 2, 128, 128, 256, 256, bias_bn=True, dldbb=8)
    add("b256-3x3", "256x256s", 1, 2, 128, 128, 64, 256, taps=9, res=True, dldr=8)
    add("b256-colstats-res", "256x256", 1, 1, 129, 256, 256, 256, res=True, colstats=True, dldo=8)       # M = 33024 = 129 tiles
    add("b256-ragged", "256x256", 0, 1, 257, 129, 64, 256, bias=True, dldo=8)                            # M = 33153 = 129 * 256 + 129
    # ---- 256 x 256 GEGLU: N % 256 == 0, M >= 4096
    add("geglu256-k64", "256x256", 0, 1, 64, 64, 64, 256, epi=G, bias=True)
    add("geglu256-k320", "256x256", 1, 1, 64, 65, 320, 512, epi=G, bias=True, dldo=8)                    # M = 4160, ragged last tile
    add("geglu256-nobias", "256x256", 1, 2, 48, 48, 320, 256, epi=G)
    # ---- 256 x 128, 4 waves, BK 32, 3 stages: N = 128 / 384, M >= 65536, K <= 1152
    add("tall-1x1-k64", "256x128w4", 0, 1, 256, 256, 64, 128, bias=True, epi=S)
    add("tall-3x3-ragged", "256x128w4", 1, 1, 258, 255, 128, 128, taps=9, bias=True)                     # M = 65790
    add("tall-n384-colstats", "256x128w4", 0, 1, 256, 256, 64, 384, bias=True, colstats=True)
    # ---- 256 x 128, 8 waves: the same N and M, K = 1280
    add("b128-k1280", "256x128w8", 1, 1, 256, 256, 1280, 128, bias=True, res=True)
    # ---- 128 x 320, 8 waves: N in {320, 640}, M >= 8192, K >= 256 (64-deep); and "midsk": split in two along K
    add("mid8-1x1", "128x320w8", 1, 2, 64, 64, 256, 320, bias=True)
    add("mid8-3x3-tapminor", "128x320w8", 1, 2, 64, 65, 64, 320, taps=9, bias=True, bias_bn=True, epi=S)  # in_w = 65: tap offsets cross a row
    add("mid8-n640-ragged", "128x320w8", 1, 1, 91, 91, 256, 640, res=True, dldr=8, dldo=8)               # M = 8281
    add("mid8-colstats", "128x320w8", 1, 2, 64, 64, 256, 320, bias=True, colstats=True)
    add("mid8-midsk", "128x320w8", 1, 2, 32, 64, 8192, 1280, ws_slabs=2, ksplit=2, bias=True)            # M = 4096, workspace = 2 M N fp32 exactly
    add("mid8-splitk4", "128x320w8", 1, 2, 64, 64, 1536, 320, ws_slabs=16, ksplit=4, bias_bn=True, epi=S)
    add("mid8-stride2", "128x320w8", 1, 2, 128, 128, 64, 320, taps=9, stride=2, bias=True)               # 64 x 64 outputs
    # ---- 128 x 320, 4 waves, BK 32: the same N and M with K < 256 or channels that are no multiple of 64
    add("mid4-k64", "128x320w4", 0, 2, 64, 64, 64, 320, bias=True)
    add("mid4-c352", "128x320w4", 1, 2, 64, 64, 352, 320, res=True)
    add("mid4-c96+32", "128x320w4", 0, 2, 64, 64, 96, 640, c1=32, bias=True, bias_bn=True)
    add("mid4-colstats-n640", "128x320w4", 0, 1, 128, 65, 64, 640, colstats=True, res=True)              # M = 8320
    # ---- 128 x 128, BK 64: N % 128 == 0 or N > 256, K >= 1024, 64-deep channels
    add("g128d-1x1", "128x128k64", 1, 2, 8, 9, 1024, 128, bias=True)                                     # M = 144: a 16-row last tile
    add("g128d-3x3", "128x128k64s", 1, 2, 9, 7, 128, 128, taps=9, bias=True, bias_bn=True, epi=S)        # K = 1152; a sample boundary inside a tile
    add("g128d-n328", "128x128k64", 1, 1, 12, 11, 1024, 328, bias=True, res=True)                        # N tile overhang, n % 8 == 0
    # ---- 128 x 128, BK 32, 4 stages: K < 1024 or not 64-deep; GEGLU at N = 128
    add("g128-k64", "128x128k32", 0, 2, 8, 9, 64, 128, bias=True)
    add("g128-c1056", "128x128k32", 1, 1, 5, 7, 1056, 384, res=True)
    add("g128-geglu", "128x128k32", 1, 1, 13, 11, 320, 128, epi=G, bias=True)
    add("g128-geglu-k64", "128x128k32", 0, 1, 13, 11, 64, 256, epi=G, bias=True, dldo=8)
    # ---- 128 x 64: N <= 256 with N % 128 != 0
    for n in (8, 64, 96, 192):
        add(f"g64d-n{n}", "128x64k64", 1, 1, 10, 13, 1024, n, bias=True)
        add(f"g64-n{n}", "128x64k32", 0, 1, 10, 13, 64, n, bias=True)
    # ================================================================ edges
    # ---- rows
    for M in (1, 31, 127, 129):
        add(f"rows-m{M}", "128x128k32", 0, M, 1, 1, 64, 128, bias=True, res=True)
        add(f"rows-m{M}-k1024-n96", "128x64k64", 1, 1, 1, M, 1024, 96, bias=True)
    add("rows-samplesplit-bb", "128x128k32", 1, 3, 5, 9, 320, 128, bias_bn=True, epi=S)                  # 45 rows per sample: the generic path
    add("rows-samplesplit-bb-3x3", "128x64k32", 1, 3, 7, 5, 32, 64, taps=9, bias_bn=True, bias=True)     # 35 rows per sample, non-square
    # ---- columns
    for n in (4, 12, 100):
        add(f"cols-n{n}", "128x64k32", 0, 2, 6, 7, 64, n, bias=True, res=True, bias_bn=True)
        add(f"cols-n{n}-silu", "128x64k64", 1, 1, 9, 5, 1024, n, bias=True, epi=S)
    add("cols-n328-k64", "128x128k32", 0, 1, 12, 11, 64, 328, bias=True, bias_bn=False)
    add("cols-n328-bb", "128x128k32", 1, 2, 8, 8, 320, 328, bias_bn=True, epi=S)                         # fast path, overhanging N tile, last sample
    add("cols-ldo+8", "128x128k32", 1, 2, 8, 9, 320, 128, bias=True, dldo=8)
    add("cols-ldo+3", "128x128k32", 1, 2, 8, 9, 320, 128, bias=True, res=True, dldo=3)
    add("cols-ldr-ldbb", "128x128k32", 1, 2, 8, 8, 320, 128, bias_bn=True, dldbb=16)
    add("cols-ldr+8", "128x128k32", 1, 2, 8, 9, 320, 128, res=True, dldr=8)
    add("cols-ldr+5", "128x128k32", 1, 2, 8, 9, 320, 128, res=True, dldr=5, epi=Q, bias=True)
    add("cols-ldbb+4", "128x128k32", 1, 2, 8, 8, 320, 128, bias_bn=True, dldbb=4)
    add("cols-ldo+8-256", "256x256", 1, 1, 128, 257, 256, 256, bias=True, res=True, dldo=8, dldr=24)
    add("cols-ldo+3-mid", "128x320w8", 1, 1, 128, 65, 256, 320, bias=True, dldo=3)                       # the scalar store loop on the 320-wide tile
    add("cols-ldr+5-256", "256x256", 0, 1, 128, 257, 64, 256, res=True, dldr=5)
    # ---- gather
    add("gather-s2-pad1", "128x128k32", 1, 2, 9, 11, 64, 128, taps=9, stride=2, bias=True)
    add("gather-s2-pad0", "128x128k32", 1, 2, 10, 12, 64, 128, taps=9, stride=2, pad=0, bias=True)
    add("gather-s2-pad0-k64", "128x128k64s", 1, 2, 10, 12, 128, 128, taps=9, stride=2, pad=0)
    add("gather-1x1-s2", "128x128k32", 0, 2, 9, 11, 64, 128, stride=2, bias=True)
    add("gather-1x1-s2-c2", "128x64k32", 0, 2, 10, 11, 32, 64, c1=64, stride=2)
    add("gather-up", "128x128k32", 1, 2, 5, 7, 64, 128, taps=9, up=1, bias=True)
    add("gather-up-k64", "128x128k64s", 1, 2, 5, 7, 128, 128, taps=9, up=1, res=True)
    add("gather-up-2src", "128x128k32", 1, 1, 6, 5, 64, 128, c1=32, taps=9, up=1)
    add("gather-2src-equal", "128x128k64s", 1, 2, 7, 9, 64, 128, c1=64, taps=9, bias=True)
    add("gather-2src-unequal", "128x128k32", 1, 2, 7, 9, 32, 128, c1=96, taps=9, bias=True)
    add("gather-2src-k64", "128x128k64s", 1, 2, 7, 9, 64, 128, c1=128, taps=9)
    add("gather-2src-1x1", "128x128k32", 0, 2, 7, 9, 32, 128, c1=64)
    add("gather-2src-1x1-k64", "128x128k64", 1, 2, 7, 9, 704, 128, c1=320)
    add("gather-1x1img", "128x128k32", 1, 5, 1, 1, 64, 128, taps=9, bias=True)
    add("gather-1x5img", "128x128k32", 1, 3, 1, 5, 64, 128, taps=9, bias=True)
    add("gather-3x2img", "128x64k32", 1, 3, 3, 2, 32, 64, taps=9, res=True)
    add("gather-w65-mid8", "128x320w8", 1, 1, 127, 65, 64, 320, taps=9)                                   # M = 8255, tap-minor, ragged
    add("gather-big-s2", "256x320s", 1, 3, 256, 256, 64, 320, taps=9, stride=2, pad=0, bias=True)        # tap-minor with stride 2, pad 0
    # ---- epilogue: each term alone and the legal pairs, on a 128-row tile, a 256-row tile and the 128 x 320 tile
    epis = (("bias", dict(bias=True)), ("bb", dict(bias_bn=True)), ("res", dict(res=True)), ("silu", dict(epi=S)), ("qgelu", dict(epi=Q)),
            ("bias-silu", dict(bias=True, epi=S)), ("bias-qgelu", dict(bias=True, epi=Q)), ("bias-res", dict(bias=True, res=True)),
            ("bias-bb-silu", dict(bias=True, bias_bn=True, epi=S)), ("silu-res", dict(epi=S, res=True)),
            ("bb-res", dict(bias_bn=True, res=True)), ("bias-bb-silu-res", dict(bias=True, bias_bn=True, epi=S, res=True)),
            ("none", dict()))
    for tag, kw in epis:
        add(f"epi-{tag}", "128x128k32", 1, 2, 8, 8, 320, 128, **kw)
    for tag, kw in epis[:3] + epis[8:12]:
        add(f"epi256-{tag}", "256x256", 0, 1, 128, 256, 64, 256, **kw)
        add(f"epimid-{tag}", "128x320w8", 1, 2, 64, 64, 256, 320, **kw)
    add("epi-biasrows", "128x128k32", 1, 2, 8, 9, 320, 128, bias=True, epi=R_)
    add("epi-biasrows-silu-res", "128x64k32", 0, 2, 8, 9, 64, 96, bias=True, epi=R_ | S, res=True)
    add("epi-biasrows-mid", "128x320w8", 1, 2, 64, 64, 256, 320, bias=True, epi=R_)
    add("epi-biasrows-256", "256x256", 0, 1, 128, 256, 64, 256, bias=True, epi=R_)
    add("epi-perm16-n77", "128x64k32", 1, 2, 5, 9, 320, 77, epi=P16, dldo=16)
    add("epi-perm16-n80", "128x64k32", 1, 2, 5, 9, 320, 80, epi=P16, dldo=16)
    add("epi-perm16-n77-rows", "128x64k32", 0, 150, 1, 1, 64, 77, epi=P16 | R_, bias=True, dldo=16)
    add("epi-perm16-n4096", "128x128k32", 1, 40, 1, 1, 64 * 5, 4096, epi=P16, nz=2, zgap=(8, 0, 16))     # the V^T shape: A = weights, W = activations
    add("epi-perm32", "128x128k32", 1, 2, 8, 9, 512, 128, epi=P32)
    add("epi-perm32-n96-rows", "128x64k32", 0, 2, 8, 9, 64, 96, epi=P32 | R_, bias=True, dldo=8)
    add("epi-perm32-mid", "128x320w8", 1, 2, 64, 64, 256, 320, epi=P32)
    # ---- z-batching with gaps on A, on W and on both
    add("z-gap-a", "128x128k32", 1, 1, 8, 9, 320, 128, nz=3, zgap=(64, 0, 0), bias=True)
    add("z-gap-w", "128x128k32", 1, 1, 8, 9, 320, 128, nz=3, zgap=(0, 40, 0), res=True)
    add("z-gap-both", "128x64k64", 1, 1, 8, 9, 1024, 96, nz=3, zgap=(8, 16, 24), bias=True, epi=S)
    add("z-gap-n100", "128x64k32", 0, 1, 8, 9, 64, 100, nz=2, zgap=(8, 8, 5), bias=True)                 # the scalar store loop, odd out stride
    # ---- split-K: 2 splits, a ragged split, 16 with two empty, a workspace for exactly 3 slabs, none
    splits = (("k1024", 1024, 16, 2), ("k1280", 1280, 16, 3), ("k6208", 6208, 16, 16), ("k6208-ws3", 6208, 3, 3), ("k6208-nows", 6208, 0, 1))
    sepi = (("plain", dict(bias=True)), ("silu-bb", dict(epi=S, bias_bn=True)), ("res", dict(res=True, dldr=8)),
            ("biasrows", dict(epi=R_, bias=True)))
    for stag, K, slabs, ks in splits:
        for etag, kw in sepi:
            add(f"split-{stag}-{etag}", "128x128k64", 1, 2, 5, 9, K, 128, ws_slabs=slabs, ksplit=ks, **kw)
        add(f"split-{stag}-perm16-n77", "128x64k64", 1, 2, 5, 9, K, 77, ws_slabs=slabs, ksplit=ks, epi=P16, dldo=16)
    add("split-3x3", "128x128k64s", 1, 2, 5, 9, 128, 128, taps=9, ws_slabs=16, ksplit=3, bias=True)      # K = 1152: 18 tiles -> 6, 6, 6
    add("split-3x3-2src", "128x128k64s", 1, 2, 5, 9, 128, 256, c1=64, taps=9, ws_slabs=16, ksplit=4, res=True)   # K = 1728: 27 tiles -> 7, 7, 7, 6
    add("split-k32", "128x128k32", 1, 2, 5, 9, 992, 128, ws_slabs=16, ksplit=2, bias=True)               # BK = 32: 31 tiles -> 16, 15
    add("split-n328", "128x128k64", 1, 1, 9, 5, 1024, 328, ws_slabs=16, ksplit=2, bias=True, dldo=8)
    # ---- colstats on each tile family that takes it
    add("cs-g128", "128x128k32", 1, 2, 8, 8, 320, 128, colstats=True, bias=True)
    add("cs-g128-bb", "128x128k32", 1, 3, 8, 8, 320, 128, colstats=True, bias_bn=True, epi=S)
    add("cs-g128-res", "128x128k32", 1, 2, 8, 12, 320, 128, colstats=True, res=True, dldr=8)
    add("cs-n328", "128x128k32", 1, 2, 8, 8, 320, 328, colstats=True, bias=True)
    add("cs-g128d-3x3", "128x128k64s", 1, 2, 8, 12, 128, 128, taps=9, colstats=True, bias=True)
    add("cs-g64", "128x64k32", 0, 2, 8, 12, 64, 96, colstats=True, bias=True, dldo=8)
    add("cs-g64d", "128x64k64", 1, 1, 8, 4, 1024, 64, colstats=True)
    add("cs-g128d", "128x128k64", 1, 1, 8, 20, 1024, 256, colstats=True, ws_slabs=16)                    # colstats switches split-K off
    # ... and on the 256-row and 128 x 320 tiles with M % 32 == 0 but no multiple of the block's rows: the last block holds 32-row tiles
    # beyond M, which own no slot
    add("cs-big-ragged", "256x320", 0, 1, 1537, 32, 64, 320, colstats=True, res=True)                    # M = 49184 = 192 * 256 + 32
    add("cs-b256-ragged", "256x256", 0, 1, 205, 160, 64, 256, colstats=True, bias=True)                  # M = 32800 = 128 * 256 + 32
    add("cs-tall-ragged", "256x128w4", 0, 1, 683, 96, 64, 128, colstats=True, bias_bn=True)              # M = 65568 = 256 * 256 + 32
    add("cs-b128-ragged", "256x128w8", 1, 1, 683, 96, 1280, 128, colstats=True, bias=True)               # the 8-wave 256 x 128 tile
    add("cs-mid8-ragged", "128x320w8", 1, 1, 257, 32, 256, 320, colstats=True, bias_bn=True, epi=EPI_SILU)   # M = 8224 = 64 * 128 + 32
    add("cs-mid4-ragged", "128x320w4", 0, 1, 257, 32, 64, 640, colstats=True, res=True, dldo=8)
    # ---- phase launches
    add("phase-w1", "128x128k32", 0, 2, 5, 1, 32, 128, taps=4, phase=5, bias=True)
    add("phase-w2", "128x128k32", 1, 2, 3, 2, 64, 128, taps=4, phase=5, bias=True)
    for p in (1, 2, 3, 4):
        add(f"phase-w16-p{p}", "128x128k32", 1, 2, 5, 16, 64, 128, taps=4, phase=p, bias=True)
    add("phase-w16-all-ldo", "128x128k32", 1, 2, 5, 16, 64, 128, taps=4, phase=5, dldo=8)
    add("phase-w16-cs", "128x128k32", 1, 2, 4, 16, 64, 128, taps=4, phase=5, bias=True, colstats=True)
    add("phase-w2-cs-p3", "128x64k32", 0, 2, 16, 2, 32, 64, taps=4, phase=3, bias=True, colstats=True, dldo=8)
    add("phase-k64", "128x128k64", 1, 1, 4, 8, 256, 128, taps=4, phase=5, bias=True)
    add("phase-mid8-cs", "128x320w8", 1, 2, 64, 64, 64, 320, taps=4, phase=5, bias=True, colstats=True, dldo=8)
    add("phase-256", "256x256", 1, 2, 128, 128, 64, 256, taps=4, phase=2, bias=True)
    # ---- out_t
    add("out_t-n1280", "128x128k32", 1, 2, 4, 8, 320, 1280, out_t=(640, 32, 0))
    add("out_t-n1920", "128x128k32", 1, 2, 4, 8, 320, 1920, out_t=(1280, 32, 8), dldo=8)                  # M = 64, rows_per_sample = 32, ldo_t = 40
    add("out_t-k1280", "128x128k64", 1, 1, 12, 8, 1280, 1920, out_t=(640, 96, 8))
    add("out_t-big", "256x320", 1, 3, 64, 64, 320, 1280, out_t=(640, 4096, 0))                           # M = 12288: 48 x 4 tiles, the 320-wide tile takes it
    return tuple(cases)


CASES = _build_cases()


# ---------------------------------------------------------------------------------------------------------------- refusals
# (PTR, the kit's placeholder: an integer address in the host test, a small device tensor in the GPU test)
REFUSAL_BASE = dict(batch=1, in_h=8, in_w=8, c0=64, n=64, taps=9)
_OUT_T = dict(taps=1, c0=320, n=1280, batch=2, in_h=4, in_w=8, out_t=PTR, n_split=640, rows_per_sample=32, ldo_t=32, ldo=640)
PHASE_BASE = dict(taps=4, phase=1, in_h=4, in_w=8)
# (text of coma_last_error, changes to REFUSAL_BASE): every refusal of sd_conv_gemm_f16 that a descriptor can reach, each through sizes and
# flags alone.  The one that none can: "out_t: the ..-column tile of this shape does not divide n_split" -- n_split and n are multiples of
# 640, so the tile is 320, 128 or 64 columns wide (the 256-wide tiles lose to the 320-wide one whenever N % 320 == 0); the check guards
# a later change of the thresholds.
REFUSALS = (
    ("epi 0x40 holds bits outside SD_EPI_ALL", dict(epi=64)),
    ("null pointer", dict(a0=None)),
    ("null pointer", dict(w=None)),
    ("null pointer", dict(out=None)),
    ("phase must be 0..4", dict(phase=5, taps=4)),
    ("phase must be 0..4", dict(phase=-1)),
    ("a phase launch needs taps = 4", dict(phase=1)),                                        # taps = 9
    ("a phase launch needs taps = 4", dict(PHASE_BASE, stride=2)),
    ("a phase launch needs taps = 4", dict(PHASE_BASE, in_w=6)),                                 # not a power of two
    ("a phase launch needs taps = 4", dict(PHASE_BASE, out_h=8)),
    ("a phase launch needs taps = 4", dict(PHASE_BASE, n=68)),
    ("a phase launch needs taps = 4", dict(PHASE_BASE, ldo=68)),
    ("a phase launch needs taps = 4", dict(PHASE_BASE, res=PTR)),
    ("a phase launch needs taps = 4", dict(PHASE_BASE, bias_bn=PTR)),
    ("a phase launch needs taps = 4", dict(PHASE_BASE, epi=EPI_SILU)),
    ("a phase launch needs taps = 4", dict(PHASE_BASE, nbatch_z=2)),
    ("the output of a phase launch must stay below 2 GiB", dict(PHASE_BASE, in_h=1024, in_w=1024, n=256)),
    (r"taps must be 1 or 9 \(4 only with a phase\)", dict(taps=4)),
    ("taps must be 1 or 9", dict(taps=3)),
    ("stride must be 1 or 2", dict(stride=3)),
    ("stride must be 1 or 2", dict(stride=0)),
    (r"source channels must be multiples of 32 \(c0=48 c1=0\)", dict(c0=48)),
    ("source channels must be multiples of 32", dict(c0=0)),
    ("source channels must be multiples of 32", dict(c1=16, a1=PTR)),
    ("source channels must be multiples of 32", dict(c1=32)),                                # c1 without a1
    ("bad sizes", dict(batch=0)),
    ("bad sizes", dict(n=0)),
    ("bad sizes", dict(out_w=0)),
    ("pad must be 0 or 1", dict(pad=2)),
    ("pad must be 0 or 1", dict(pad=-1)),
    ("upsample only with 3x3 stride 1", dict(upsample=1, stride=2)),
    ("upsample only with 3x3 stride 1", dict(upsample=1, taps=1)),
    ("M too large", dict(taps=1, batch=65536, in_h=1, in_w=1, out_h=256, out_w=256)),
    ("at most 65536 samples per launch", dict(taps=1, batch=65537, in_h=1, in_w=1)),       # odd: no power of two folds into the image
    ("at most 65536 samples per launch", dict(taps=1, batch=131072, in_h=1, in_w=1, bias_bn=PTR)),
    ("at most 65536 samples per launch", dict(taps=1, batch=131072, in_h=1, in_w=2)),
    ("a 3x3 convolution takes at most 65535 samples", dict(batch=65536, in_h=1, in_w=1)),
    (r"a source tensor \(2147483648 B\) or the weights \(\d+ B\) exceed 2 GiB", dict(taps=1, in_h=1024, in_w=1024, c0=1024, out_h=1, out_w=1)),
    (r"a source tensor \(\d+ B\) or the weights \(2147483648 B\) exceed 2 GiB", dict(taps=1, c0=1024, n=1 << 20)),
    ("SD_EPI_PERM16_N needs ldo >= n rounded up to 16", dict(taps=1, n=77, epi=EPI_PERM16)),
    ("SD_EPI_PERM16_N needs ldo >= n rounded up to 16", dict(taps=1, n=77, epi=EPI_PERM16, ldo=79)),
    ("SD_EPI_PERM16_N takes no GEGLU / residual", dict(taps=1, n=128, epi=EPI_PERM16 | EPI_GEGLU)),
    ("SD_EPI_PERM16_N takes no GEGLU / residual", dict(taps=1, epi=EPI_PERM16, res=PTR)),
    ("SD_EPI_PERM16_N takes no GEGLU / residual", dict(taps=1, epi=EPI_PERM16, bias_bn=PTR)),
    ("SD_EPI_PERM16_N takes no GEGLU / residual", dict(taps=1, epi=EPI_PERM16, colstats=PTR)),
    ("SD_EPI_PERM32_N needs n % 32 == 0", dict(taps=1, n=48, epi=EPI_PERM32)),
    ("SD_EPI_PERM32_N needs n % 32 == 0", dict(taps=1, epi=EPI_PERM32 | EPI_PERM16)),
    ("SD_EPI_PERM32_N needs n % 32 == 0", dict(taps=1, epi=EPI_PERM32, res=PTR)),
    ("SD_EPI_PERM32_N needs n % 32 == 0", dict(taps=1, epi=EPI_PERM32, colstats=PTR)),
    ("take a bias only with SD_EPI_BIAS_ROWS", dict(taps=1, epi=EPI_PERM16, bias=PTR)),
    ("take a bias only with SD_EPI_BIAS_ROWS", dict(taps=1, epi=EPI_PERM32, bias=PTR)),
    ("take a bias only with SD_EPI_BIAS_ROWS", dict(taps=1, n=77, ldo=80, epi=EPI_PERM16 | EPI_SILU, bias=PTR)),
    ("SD_EPI_QUICK_GELU takes no GEGLU / SiLU", dict(epi=EPI_QGELU | EPI_SILU)),
    ("SD_EPI_QUICK_GELU takes no GEGLU / SiLU", dict(n=128, epi=EPI_QGELU | EPI_GEGLU)),
    ("GEGLU needs N % 128 == 0", dict(epi=EPI_GEGLU)),
    ("GEGLU needs N % 128 == 0", dict(n=128, epi=EPI_GEGLU, res=PTR)),
    ("GEGLU needs N % 128 == 0", dict(n=128, epi=EPI_GEGLU, bias_bn=PTR)),
    ("out_t needs a plain linear", dict(_OUT_T, bias=PTR)),
    ("out_t needs a plain linear", dict(_OUT_T, taps=9)),
    ("out_t needs a plain linear", dict(_OUT_T, n_split=320)),
    ("out_t needs a plain linear", dict(_OUT_T, n=1600)),
    ("out_t needs a plain linear", dict(_OUT_T, in_h=5, in_w=5)),                            # M % 32
    ("out_t needs a plain linear", dict(_OUT_T, rows_per_sample=48)),
    ("out_t needs a plain linear", dict(_OUT_T, rows_per_sample=16)),
    ("out_t needs a plain linear", dict(_OUT_T, ldo_t=36)),
    ("out_t needs a plain linear", dict(_OUT_T, ldo_t=24)),
    ("out_t needs a plain linear", dict(_OUT_T, ldo=632)),
    ("out_t needs a plain linear", dict(_OUT_T, ldo=644)),
    ("out_t needs a plain linear", dict(_OUT_T, epi=EPI_SILU)),
    ("out_t needs a plain linear", dict(_OUT_T, nbatch_z=2)),
    ("out_t needs a plain linear", dict(_OUT_T, colstats=PTR)),
    ("colstats needs M % 32 == 0", dict(colstats=PTR, in_h=5, in_w=5)),
    ("colstats needs M % 32 == 0", dict(colstats=PTR, n=100)),
    ("colstats needs M % 32 == 0", dict(colstats=PTR, ldo=68)),
    ("colstats needs M % 32 == 0", dict(colstats=PTR, res=PTR, ldr=68)),
    ("colstats needs M % 32 == 0", dict(colstats=PTR, res=PTR, bias_bn=PTR)),
    ("colstats needs M % 32 == 0", dict(colstats=PTR, bias_bn=PTR, batch=2, in_h=4, in_w=4)),   # 16 rows per sample
    ("colstats needs M % 32 == 0", dict(colstats=PTR, bias_bn=PTR, ldbb=68)),
    ("colstats needs M % 32 == 0", dict(colstats=PTR, bias=PTR, epi=EPI_BIAS_ROWS)),
    ("colstats needs M % 32 == 0", dict(colstats=PTR, n=128, epi=EPI_GEGLU)),
    ("colstats needs M % 32 == 0", dict(colstats=PTR, nbatch_z=2)),
    ("colstats needs M % 32 == 0", dict(colstats=PTR, taps=1, batch=32768, in_h=1, in_w=1, out_h=16, out_w=16, n=128)),   # (M + 512) ldo 2 >= 2 GiB
    (r"colstats of a phase launch needs in_h \* in_w % 32 == 0", dict(PHASE_BASE, colstats=PTR, batch=2, in_h=4, in_w=4)),
    (r"colstats of a phase launch needs in_h \* in_w % 32 == 0", dict(PHASE_BASE, colstats=PTR, batch=2, in_h=12, in_w=4)),
    ("grid too large", dict(taps=1, c0=32, batch=65536, in_h=1, in_w=1, out_h=128, out_w=128, n=1 << 20)),
)
