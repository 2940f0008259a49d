"""Test helper for the direct ("halo-patch") 3x3 convolutions (coma_amd/csrc/sd_haloconv.hip, sd_smallconv.hip): plain torch on the CPU,
nothing here is product code and nothing here needs a GPU.  The buffers (Operand / Out, pack, new_out, masks), the seeds, the exact SiLU
and the row error are tests/domain_kit.py's; tests/norm_ref.py's allowances and tests/gemm_ref.py's in-order fp32 sum are used, not copied.

* ``CASES``            the table of launches, one named tuple type per entry point (HC: sd_conv3x3_halo_f16, SN: sd_conv3x3_small_n_f16,
                       C3: sd_conv3x3_c3_f16, IC: sd_im2col3x3_c3_f16), shared by tests/test_dconv_ref_host.py and
                       tests/test_sd_dconv_domain_gpu.py.
* ``inputs``           fp16 / fp32 operands of a case, seeded by its id; every sample has its own data and its own affine table.
* ``results``          per case: the float64 reference out = conv(act(x scale + shift) -> fp16, zero padding of the ACTIVATED tensor) + bias
                       (+ res) with this file's own index arithmetic (a loop over the nine taps, no F.conv2d), the fp32 emulation of the
                       kernel's formula (fmaf affine, SiLU as f * (1 / (1 + exp(-f))) with the exponential through float64, rounding to fp16,
                       exact fp16 products added in fp32 in index order (chunk, tap, channel), bias and residual added in fp32, one rounding
                       to fp16) and the emulation's own a-priori bound, element by element.
* ``yardstick``        e_emu = the emulation's largest row error, the device bound max(4 e_emu, 2^-10), emulation / a-priori bound.
* ``branches``         a transcript of what a case reaches in the kernels, written beside the table; ``REACHABLE`` is everything they have.
* ``REFUSALS``         per entry point: an accepted base argument list and every change the argument checks refuse, with the text (the
                       kit's PTR; its check_refusals puts the rows to the entry points).

DESIGN.md section 3f has the numbers."""
from __future__ import annotations

import functools
from typing import NamedTuple

import torch

from tests import gemm_ref as gr
from tests import norm_ref as nr
from tests import domain_kit as kit
from tests.domain_kit import F16, F32, F64, PTR, U32, Operand, Out
from tests.norm_ref import LIP, UD, Result, Yardstick

TILE, CHUNK = 16, 64            # pixels per tile edge, input channels staged per pass (sd_haloconv.hip / sd_smallconv.hip)
STRESS = ("exp-overflow", "large-positive", "zero-scale", "negative-scale", "shift-as-large-as-the-interior")


# ------------------------------------------------------------------------------------------------------------------ the table
class HC(NamedTuple):
    """sd_conv3x3_halo_f16"""
    name: str
    B: int
    h: int
    w: int
    c: int
    n: int
    act: int = 2                # 0: no affine, 1: affine, 2: affine + SiLU
    bias: int = 1
    res: int = 1
    cs: int = 1
    ldo: int = 0                # as passed: 0 means n
    ldr: int = 0
    stress: int = 0
    family = "halo"

    @property
    def id(self):
        return f"halo-{self.name}"


class SN(NamedTuple):
    """sd_conv3x3_small_n_f16"""
    name: str
    B: int
    h: int
    w: int
    c: int
    n: int
    act: int = 2
    bias: int = 1
    ldo: int = 8
    stress: int = 0
    family = "small_n"

    @property
    def id(self):
        return f"small_n-{self.name}"


class C3(NamedTuple):
    """sd_conv3x3_c3_f16"""
    name: str
    B: int
    h: int
    w: int
    ldx: int = 4
    ldo: int = 128
    bias: int = 1
    cs: int = 1
    family = "c3"
    n = 128

    @property
    def id(self):
        return f"c3-{self.name}"


class IC(NamedTuple):
    """sd_im2col3x3_c3_f16"""
    name: str
    B: int
    h: int
    w: int
    ldx: int = 4
    family = "im2col"

    @property
    def id(self):
        return f"im2col-{self.name}"


ACT = ("plain", "affine", "affine+silu")


# ---- transcript of what a launch reaches (sd_haloconv.hip: conv3x3_halo_kernel; sd_smallconv.hip: the entry points and kernels)
def halo_tap1_waits(c, res):
    """The wait_vmcnt branches conv3x3_halo_kernel takes at tap 1, over all its chunks: in every chunk but the last the next chunk's 11 patch
    loads stay in flight (vmcnt<11>); in the last chunk the 8 residual loads of the epilogue's first channel half (vmcnt<8>) or nothing
    (vmcnt<0>).  With c = 64 the first chunk is the last: the residual prefetch is issued at tap 0 of the very first pass and vmcnt<8> (with
    a residual) or vmcnt<0> (without) is the ONLY branch tap 1 ever takes."""
    return ({"vmcnt<11>"} if c // CHUNK > 1 else set()) | {"vmcnt<8>" if res else "vmcnt<0>"}


def small_n_instantiation(c):
    return "<128>:unrolled-two-chunks" if c == 128 else "<320>:rolled-five-chunks"


def branches(c):
    if isinstance(c, HC):
        nchunk = c.c // CHUNK
        out = {f"halo:chunks{nchunk}", f"halo:slices{c.n // 128}", "halo:act:" + ACT[c.act], "halo:bias" if c.bias else "halo:no-bias",
               "halo:colstats" if c.cs else "halo:no-colstats",
               "halo:no-res" if not c.res else "halo:res-prefetch:shares-the-first-chunk" if nchunk == 1 else "halo:res-prefetch:last-of-several-chunks"}
        return out | {"halo:tap1:" + b for b in halo_tap1_waits(c.c, c.res)}
    if isinstance(c, SN):
        return {"small_n:" + small_n_instantiation(c.c), "small_n:act:" + ACT[c.act], "small_n:bias" if c.bias else "small_n:no-bias",
                "small_n:ragged-tile" if c.h % TILE or c.w % TILE else "small_n:full-tiles"}
    if isinstance(c, C3):
        return {"c3:colstats" if c.cs else "c3:no-colstats", "c3:bias" if c.bias else "c3:no-bias"}
    return {"im2col:last-block-ragged" if (c.B * c.h * c.w) % 256 else "im2col:full-blocks"}


REACHABLE = ({f"halo:chunks{k}" for k in range(1, 9)} | {f"halo:slices{k}" for k in range(1, 5)} | {"halo:act:" + a for a in ACT}
             | {"halo:bias", "halo:no-bias", "halo:colstats", "halo:no-colstats", "halo:no-res", "halo:res-prefetch:shares-the-first-chunk",
                "halo:res-prefetch:last-of-several-chunks", "halo:tap1:vmcnt<11>", "halo:tap1:vmcnt<8>", "halo:tap1:vmcnt<0>"}
             | {"small_n:<128>:unrolled-two-chunks", "small_n:<320>:rolled-five-chunks", "small_n:bias", "small_n:no-bias", "small_n:ragged-tile",
                "small_n:full-tiles"} | {"small_n:act:" + a for a in ACT}
             | {"c3:colstats", "c3:no-colstats", "c3:bias", "c3:no-bias", "im2col:last-block-ragged", "im2col:full-blocks"})


def _flags(act, bias, res=None, cs=None):
    s = ACT[act] + ("-bias" if bias else "")
    return s + ("-res" if res else "") + ("-cs" if cs else "")


def _build_cases():
    t = []
    # ---- halo: the full cross of chunk counts and slice counts, everything on.  16 x 16: one tile, padding on all four sides
    t += [HC(f"cross-c{c}-n{n}", 2, 16, 16, c, n) for c in range(64, 513, 64) for n in (128, 256, 384, 512)]
    # every combination of {plain, affine, affine + SiLU} x bias x residual x column sums, leading dimensions passed explicitly as n:
    # at c = 128 (two chunks; tap 1: vmcnt<11> in the first chunk, then vmcnt<8> with a residual, vmcnt<0> without)
    # and at c = 64 (the single chunk is the last; tap 1 takes ONLY vmcnt<8> with a residual -- the prefetch was issued at tap 0 of the
    # very first pass --, ONLY vmcnt<0> without).  16 x 32: two tile columns
    for c, B in ((128, 2), (64, 1)):
        t += [HC(f"c{c}-{_flags(a, b, r, s)}", B, 16, 32, c, 128, a, b, r, s, ldo=128, ldr=128) for a in (0, 1, 2) for b in (0, 1) for r in (0, 1) for s in (0, 1)]
    # a tile with neighbours on every side (48 x 48), tile rows before tile columns (32 x 16) at batch 3
    t += [HC("48x48-c192", 1, 48, 48, 192, 128), HC("48x48-c128", 1, 48, 48, 128, 128), HC("32x16-b3-c192", 3, 32, 16, 192, 128),
          HC("32x16-b3-c128", 3, 32, 16, 128, 128)]
    # leading dimensions
    t += [HC("ldo+8", 2, 16, 16, 128, 128, ldo=136), HC("ldo+8-ldr+24", 2, 16, 16, 128, 128, ldo=136, ldr=152),
          HC("n256-ldo+8-ldr+24", 2, 16, 32, 128, 256, ldo=264, ldr=280), HC("n384-ldo+24-ldr+8", 1, 32, 16, 64, 384, ldo=408, ldr=392)]
    # the activation under stress
    t += [HC("stress-affine", 2, 16, 16, 128, 128, act=1, stress=1), HC("stress-silu", 2, 16, 16, 128, 128, stress=1),
          HC("stress-silu-c64", 2, 16, 16, 64, 128, stress=1)]
    # ---- small_n: both instantiations x n x activation x bias on a ragged 17 x 18 image
    t += [SN(f"c{c}-n{n}-{_flags(a, b)}", 2, 17, 18, c, n, a, b, ldo=16) for c in (128, 320) for n in (1, 2, 3, 4) for a in (0, 1, 2) for b in (0, 1)]
    for i, (h, w) in enumerate(((1, 1), (1, 17), (17, 1), (16, 16), (15, 33), (33, 18))):
        t += [SN(f"{h}x{w}-c{c}-b{B}", B, h, w, c, 3 + (i + j) % 2) for j, (c, B) in enumerate(((128, 1 + 2 * (i % 2)), (320, 3 - 2 * (i % 2))))]
    t += [SN(f"ldo{ld}", 2, 17, 18, 128, 3, ldo=ld) for ld in (8, 16, 72)] + [SN("ldo72-c320-n4", 1, 18, 17, 320, 4, ldo=72)]
    t += [SN("stress-affine", 2, 17, 18, 128, 3, act=1, stress=1), SN("stress-silu", 2, 17, 18, 128, 3, stress=1),
          SN("stress-silu-c320", 2, 17, 18, 320, 4, stress=1)]
    # ---- c3: the geometry set x batch, strides and the four (bias, colstats) combinations in rotation
    k = 0
    for h, w in ((16, 16), (16, 32), (32, 16), (48, 48)):
        for B in (1, 2, 3):
            t.append(C3(f"{h}x{w}-b{B}-ldx{(4, 8, 64)[k % 3]}-ldo{(128, 136, 256)[(k // 3 + k) % 3]}-{_flags(0, k & 1, cs=(k >> 1) & 1)[6:] or 'bare'}",
                        B, h, w, (4, 8, 64)[k % 3], (128, 136, 256)[(k // 3 + k) % 3], k & 1, (k >> 1) & 1))
            k += 1
    t += [C3(f"16x32-{_flags(0, b, cs=s)[6:] or 'bare'}", 2, 16, 32, 8, 136, b, s) for b in (0, 1) for s in (0, 1)]
    # ---- im2col
    t += [IC("1x1", 1, 1, 1), IC("1x5", 2, 1, 5, 8), IC("5x1", 3, 5, 1, 64), IC("7x9", 2, 7, 9, 8), IC("16x16", 1, 16, 16, 64), IC("16x16-b3", 3, 16, 16),
          IC("11x13-b2-block-crossings", 2, 11, 13), IC("11x13-b2-ldx8", 2, 11, 13, 8), IC("3x3-b3-ldx64", 3, 3, 3, 64)]
    return tuple(t)


CASES = _build_cases()


# ------------------------------------------------------------------------------------------------------------------ operands
def _table(g, B, c, stress):
    """fp32 (scale, shift) per (sample, channel), every sample its own.  stress: channels 0 .. 3 and c - 1 of every sample get, in the order
    of STRESS: a pre-activation near -100 (fp32 exp(100) overflows: SiLU gives -0), one near +200, scale 0 (the output is act(shift)), a
    negative scale, and a shift whose activation is as large as the interior values (an activated padding pixel is then an error of order
    one; the random shifts of every other case do the same on a smaller scale)."""
    tab = torch.stack([torch.randn(B, c, generator=g) * 0.5 + 1.0, torch.randn(B, c, generator=g) * 0.7], -1).to(F32)
    if stress:
        b = torch.arange(B, dtype=F32)
        tab[:, 0, 0], tab[:, 0, 1] = 0.25, -100.0 - b
        tab[:, 1, 0], tab[:, 1, 1] = 0.25, 200.0 + b
        tab[:, 2, 0], tab[:, 2, 1] = 0.0, 2.0 + 0.125 * b
        tab[:, 3, 0] = -1.5 - 0.25 * b
        tab[:, c - 1, 0], tab[:, c - 1, 1] = 1.0, 2.5 + 0.25 * b
    return tab.reshape(B * c, 2)


@functools.lru_cache(maxsize=2)
def inputs(c):
    """name -> Operand of everything the launch reads"""
    g = kit.gen(c.id)
    M = c.B * c.h * c.w
    if isinstance(c, (HC, SN)):
        d = dict(x=Operand(kit.randn16(g, M, c.c, scale=1.5, shift=0.3), c.c))
        w = kit.randn16(g, c.n, 9 * c.c, scale=(9 * c.c) ** -0.5)
        bias = kit.randn16(g, 1, c.n)
        if isinstance(c, SN):                                   # rows of w and entries of bias at and beyond n are outside the contract: NaN
            w = torch.cat([w, torch.full((16 - c.n, 9 * c.c), float("nan"), dtype=F16)])
            bias = torch.cat([bias, torch.full((1, 8 - c.n), float("nan"), dtype=F16)], 1)
        d["w"] = Operand(w, 9 * c.c)
        if c.act:
            d["gn_affine"] = Operand(_table(g, c.B, c.c, c.stress), 2)
        if c.bias:
            d["bias"] = Operand(bias, bias.shape[1])
        if isinstance(c, HC) and c.res:
            d["res"] = Operand(kit.randn16(g, M, c.n), c.ldr or c.n)
        return d
    x = kit.randn16(g, M, 3)
    if isinstance(c, IC):                                       # signed zeros: the gather moves bits
        z = torch.rand(M, 3, generator=g)
        x = torch.where(z < 0.1, torch.tensor(-0.0, dtype=F16), torch.where(z < 0.2, torch.tensor(0.0, dtype=F16), x))
        return dict(x=Operand(x, c.ldx))
    w32 = torch.zeros(c.n, 32, dtype=F16)                        # the five zero pad columns include/sd_hip.h demands
    w32[:, :27] = kit.randn16(g, c.n, 27, scale=27 ** -0.5)
    d = dict(x=Operand(x, c.ldx), w32=Operand(w32, 32))
    if c.bias:
        d["bias"] = Operand(kit.randn16(g, 1, c.n), c.n)
    return d


def tiles(c):
    return c.B * (c.h // TILE) * (c.w // TILE)


def outputs(c):
    """name -> Out of everything the launch writes"""
    M = c.B * c.h * c.w
    if isinstance(c, HC):
        d = dict(out=Out(M, c.n, c.ldo or c.n, F16))
    elif isinstance(c, SN):
        d = dict(out=Out(M, 8, c.ldo, F16))                     # channels 0 .. 7 of every pixel are written, channels >= 8 left alone
    elif isinstance(c, C3):
        d = dict(out=Out(M, c.n, c.ldo, F16))
    else:
        return dict(out=Out(M, 32, 32, F16))
    if not isinstance(c, SN) and c.cs:
        d["colstats"] = Out(tiles(c) * 2, c.n, c.n, F32)
    return d


def launch(ops, c, p):
    """The launch of a case through coma_amd.sd.ops; p: name -> device tensor starting at the operand's / output's first element."""
    g = p.get
    if isinstance(c, HC):
        return ops.conv3x3_halo(p["x"], p["w"], p["out"], batch=c.B, h=c.h, w_=c.w, c=c.c, n=c.n, bias=g("bias"), res=g("res"),
                                gn_affine=g("gn_affine"), silu=c.act == 2, colstats=g("colstats"), ldo=c.ldo, ldr=c.ldr)
    if isinstance(c, SN):
        return ops.conv3x3_small_n(p["x"], p["w"], p["out"], batch=c.B, h=c.h, w_=c.w, c=c.c, n=c.n, bias=g("bias"), gn_affine=g("gn_affine"),
                                   silu=c.act == 2, ldo=c.ldo)
    if isinstance(c, C3):
        return ops.conv3x3_c3(p["x"], p["w32"], p["out"], batch=c.B, h=c.h, w=c.w, ldx=c.ldx, n=c.n, bias=g("bias"), colstats=g("colstats"), ldo=c.ldo)
    return ops.im2col3x3_c3(p["x"], p["out"], batch=c.B, h=c.h, w=c.w, ldx=c.ldx)


# ------------------------------------------------------------------------------------------------------------------ arithmetic
def activate(x, tab, B, act):
    """act(x scale + shift) BEFORE its rounding to fp16, x fp16 [B hw, C], tab fp32 [B C, 2] -> (float64; the kernel's formula in fp32: one
    fmaf, SiLU as f * (1 / (1 + exp(-f))) with a correctly rounded exponential; the a-priori bound of |fp32 - float64|: u |y| for the fma
    (u = 2^-24); through SiLU the Lipschitz constant LIP, + UD |f| for the reciprocal + 4 u |f| for the exponential, the addition and the
    product).  Without an affine the tensor itself, exact."""
    C = x.shape[-1]
    if not act:
        return x.to(F64), x.to(F32), torch.zeros(x.shape, dtype=F64)
    x64, t = x.to(F64).view(B, -1, C), tab.to(F64).view(B, 1, C, 2)
    y = x64 * t[..., 0] + t[..., 1]
    y32 = y.to(F32)                                             # fmaf of exact inputs: the float64 value rounded once
    err = U32 * y.abs()
    if act == 2:
        y = kit.silu(y)
        y32 = y32 * (1.0 / (1.0 + kit.exp32(-y32)))             # exp(100) = inf in fp32, 1 / inf = 0, f * 0 = -0: finite, as on the device
        err = LIP * err + (UD + 4 * U32) * y.abs()
    return y.view(-1, C), y32.view(-1, C), err.view(-1, C)


def taps(img):
    """img [B, h, w, C] -> [B h w, 9, C]: the 3 x 3 neighbourhood of every pixel, tap = 3 ky + kx, zero padding 1"""
    B, h, w, C = img.shape
    pad = torch.zeros(B, h + 2, w + 2, C, dtype=img.dtype)
    pad[:, 1:-1, 1:-1] = img
    return torch.stack([pad[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 3).reshape(B * h * w, 9, C)


def conv64(img, w):
    """out[b, y, x, n] = sum over ky, kx, ci of img[b, y - 1 + ky, x - 1 + kx, ci] w[n, 3 ky + kx, ci] in float64, zero padding:
    img [B, h, w, C], w [n, 9, C] -> [B h w, n]"""
    B, h, wd, C = img.shape
    pad = torch.zeros(B, h + 2, wd + 2, C, dtype=F64)
    pad[:, 1:-1, 1:-1] = img.to(F64)
    out = torch.zeros(B, h, wd, w.shape[0], dtype=F64)
    for ky in range(3):
        for kx in range(3):
            out += pad[:, ky:ky + h, kx:kx + wd] @ w[:, 3 * ky + kx].to(F64).t()
    return out.reshape(B * h * wd, -1)


def _chunked(t, chunk):
    """[R, 9, C] -> [R, K] in the kernels' accumulation order: chunk of `chunk` channels, tap, channel"""
    R, _, C = t.shape
    return t.view(R, 9, C // chunk, chunk).permute(0, 2, 1, 3).reshape(R, 9 * C)


def convolve(a, a_emu, e_a, w, B, h, wd, chunk, bias=None, res=None):
    """The convolution of the stored fp16 tensor a (reference) / a_emu (emulation; e_a bounds |a_emu - a| element by element), w fp16
    [n, 9, C] -> (float64, the fp32 emulation BEFORE the final rounding, a-priori bound of their difference before the final rounding):
    exact fp16 products added in fp32 in the order (chunk, tap, channel) -- K terms: (K + 4) u of the sum of magnitudes, as
    gemm_ref.epilogue counts it --, |w| e_a for the emulation's own input, then u of the magnitudes per bias / residual addition."""
    C, K = a.shape[-1], 9 * a.shape[-1]
    img = lambda t: t.view(B, h, wd, C)
    ref = conv64(img(a), w)
    mag = conv64(img(a).abs(), w.abs())
    e_in = conv64(img(e_a), w.abs())
    err = e_in + (K + 4) * U32 * (mag + e_in)
    acc = gr.sum_in_order(_chunked(taps(img(a_emu)), chunk), _chunked(w.contiguous(), chunk), 0, K)
    if bias is not None:
        ref, acc, mag = ref + bias.to(F64), acc + bias.to(F32), mag + bias.to(F64).abs()
        err = err + U32 * (mag + err)
    if res is not None:
        err = err + U32 * (ref.abs() + res.to(F64).abs() + err)
        ref, acc = ref + res.to(F64), acc + res.to(F32)
    return ref, acc, err


@functools.lru_cache(maxsize=2)
def activated(c):
    """HC / SN: (the activated tensor as stored: float64 rounded to fp16 -- the storage point include/sd_hip.h names --, the emulation's,
    the bound of their difference: where the two roundings differ, one fp16 ulp)"""
    d = inputs(c)
    y, y32, _ = activate(d["x"].t, d["gn_affine"].t if c.act else None, c.B, c.act)
    a, a_emu = y.to(F16), y32.to(F16)
    return a, a_emu, torch.where(a == a_emu, torch.zeros_like(y), nr.ulp16(y))


@functools.lru_cache(maxsize=2)
def results(c):
    """output name -> Result (the fp16 output; the column sums are held to the device's own stored output, colstats_expected)"""
    d = inputs(c)
    if isinstance(c, IC):
        ref = torch.zeros(c.B * c.h * c.w, 32, dtype=F16)
        ref[:, :27] = taps(d["x"].t.view(c.B, c.h, c.w, 3)).reshape(-1, 27)
        return dict(out=Result(ref.to(F64), ref, torch.full(ref.shape, 2.0 ** -25, dtype=F64)))
    if isinstance(c, C3):
        x = d["x"].t
        w = d["w32"].t[:, :27].reshape(c.n, 9, 3)
        ref, acc, err = convolve(x, x, torch.zeros(x.shape, dtype=F64), w, c.B, c.h, c.w, 3, d["bias"].t if c.bias else None)
        return dict(out=Result(ref, acc.to(F16), nr.final16(ref, err)))
    a, a_emu, e_a = activated(c)
    w = d["w"].t[:c.n].reshape(c.n, 9, c.c)
    bias = d["bias"].t[:, :c.n] if c.bias else None
    ref, acc, err = convolve(a, a_emu, e_a, w, c.B, c.h, c.w, CHUNK, bias, d["res"].t if isinstance(c, HC) and c.res else None)
    if isinstance(c, SN):                                       # channels n .. 7 of every pixel: zeros
        pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], 8 - c.n, dtype=t.dtype)], 1)
        ref, acc, err = pad(ref), pad(acc), pad(err)
    return dict(out=Result(ref, acc.to(F16), nr.final16(ref, err)))


def row_error(c, got, ref):
    """Each element's error over the largest |ref| of its output row -> the largest per row.  A row is a pixel's n channels for the halo and
    the 3-channel kernels (and a packed row of im2col).  A small_n pixel has at most four values, and one of them can cancel to zero: its
    yardstick row is the SAMPLE, the largest |ref| over all pixels and channels of that sample."""
    if isinstance(c, SN):
        return kit.row_error(got.reshape(c.B, -1), ref.reshape(c.B, -1))
    return kit.row_error(got, ref)


def yardstick(c):
    r = results(c)["out"]
    assert bool(torch.isfinite(r.ref).all()) and bool(torch.isfinite(r.emu.to(F64)).all()), c.id
    if isinstance(c, (HC, SN)):                                 # every activated value stays finite in fp16
        a, a_emu, _ = activated(c)
        assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(a_emu.float()).all()), c.id
    worst = float(((r.emu.to(F64) - r.ref).abs() / r.stated).max())
    e_emu = float(row_error(c, r.emu, r.ref).max())
    return Yardstick(e_emu, kit.device_bound(e_emu), worst)


def colstats_expected(c, out_buf):
    """float64 sums, sums of squares and sums of magnitudes per slot and column of the DEVICE's own stored output; a slot is one 16 x 16
    tile, its index (sample, tile row, tile column); with n > 128 the column index is global -> three [slots, n]"""
    v = kit.body(outputs(c)["out"], out_buf).to(F64).view(c.B, c.h // TILE, TILE, c.w // TILE, TILE, c.n).permute(0, 1, 3, 2, 4, 5).reshape(-1, 256, c.n)
    return v.sum(1), (v * v).sum(1), v.abs().sum(1)


# a slot is 256 stored values added in some fixed order: any order of 256 terms costs at most 255 roundings of 2^-24 of the sum of
# magnitudes (< 2^-16), plus one rounding per square in the second row; 1.001 covers the second-order terms
COLSTATS_REL = 1.001 * 2.0 ** -16


# ------------------------------------------------------------------------------------------------------------------ refusals
OUTPUT_ARGS = {"out", "colstats"}

_HALO = dict(x=PTR, c=64, gn_affine=None, silu=0, w=PTR, bias=None, res=None, ldr=0, batch=1, h=16, w_=16, n=128, out=PTR, ldo=0, colstats=None)
_SMALL = dict(x=PTR, gn_affine=None, silu=0, w=PTR, bias=None, batch=1, h=4, w_=4, c=128, n=3, out=PTR, ldo=8)
_C3 = dict(x=PTR, ldx=4, w32=PTR, bias=None, batch=1, h=16, w_=16, n=128, out=PTR, ldo=128, colstats=None)
_IC = dict(x=PTR, ldx=4, batch=1, h=2, w_=2, out=PTR)

# entry point -> (accepted base, [(text of the refusal, change), ...]): every condition the argument checks state.  (The halo entry
# point's "weights too large" cannot be reached: n <= 512 and c <= 512 are checked first.)
REFUSALS = {
    "sd_conv3x3_halo_f16": (_HALO, [
        ("null pointer", dict(x=None)), ("null pointer", dict(w=None)), ("null pointer", dict(out=None)),
        ("n = 0 (built for 128, 256, 384 and 512", dict(n=0)), ("n = 64 (built for", dict(n=64)), ("n = 192 (built for", dict(n=192)),
        ("n = 640 (built for", dict(n=640)), ("n = -128 (built for", dict(n=-128)),
        ("c = 0 (a multiple of 64, at most 512)", dict(c=0)), ("c = 32 (a multiple of 64", dict(c=32)), ("c = 576 (a multiple of 64", dict(c=576)),
        ("c = -64 (a multiple of 64", dict(c=-64)),
        ("(h, w multiples of 16)", dict(batch=0)), ("(h, w multiples of 16)", dict(h=0)), ("(h, w multiples of 16)", dict(w_=0)),
        ("h=24 w=16 (h, w multiples of 16)", dict(h=24)), ("h=16 w=8 (h, w multiples of 16)", dict(w_=8)),
        ("silu is applied with the GroupNorm affine", dict(silu=1)),
        ("ldo = 64, ldr = 128", dict(ldo=64)), ("ldo = 132", dict(ldo=132)), ("ldo = 128, ldr = 64", dict(res=PTR, ldr=64)),
        ("ldr = 132", dict(res=PTR, ldr=132)), ("ldo = 256, ldr = 384", dict(n=384, res=PTR, ldo=256)),
        ("one input sample is 2147483648 bytes (must stay below 2 GiB)", dict(h=4096, w_=4096)),
        ("one input sample is 2415919104 bytes", dict(c=512, h=1536, w_=1536)),
        ("grid too large", dict(batch=65536, h=4080, w_=4080)), ("grid too large", dict(batch=32768, h=4080, w_=4080, n=256))]),
    "sd_conv3x3_small_n_f16": (_SMALL, [
        ("null pointer", dict(x=None)), ("null pointer", dict(w=None)), ("null pointer", dict(out=None)),
        ("c = 64 (built for 128 and 320 input channels)", dict(c=64)), ("c = 0 (built for", dict(c=0)), ("c = 256 (built for", dict(c=256)),
        ("bad shape n=0", dict(n=0)), ("bad shape n=5", dict(n=5)), ("bad shape", dict(batch=0)), ("bad shape", dict(h=0)), ("bad shape", dict(w_=0)),
        ("ldo=0", dict(ldo=0)), ("ldo=4", dict(ldo=4)), ("ldo=12", dict(ldo=12)),
        ("silu is applied with the GroupNorm affine", dict(silu=1)),
        ("batch = 65536 exceeds the grid limit", dict(batch=65536)),
        ("h = 1048561 exceeds the grid limit", dict(h=16 * 65535 + 1)),
        ("tensor too large", dict(batch=65535, h=16 * 65535, w_=1))]),
    "sd_conv3x3_c3_f16": (_C3, [
        ("null pointer", dict(x=None)), ("null pointer", dict(w32=None)), ("null pointer", dict(out=None)),
        ("n = 64 (built for 128 output channels)", dict(n=64)), ("n = 256 (built for", dict(n=256, ldo=256)),
        ("bad shape ldx=3", dict(ldx=3)), ("bad shape ldx=6", dict(ldx=6)), ("bad shape ldx=0", dict(ldx=0)),
        ("bad shape", dict(batch=0)), ("batch=65536", dict(batch=65536)), ("bad shape", dict(h=0)), ("bad shape", dict(w_=0)),
        ("h=8 w=16", dict(h=8)), ("h=16 w=24", dict(w_=24)), ("ldo=64", dict(ldo=64)), ("ldo=132", dict(ldo=132)),
        ("h = 1048576 exceeds the grid limit", dict(h=16 * 65536))]),
    "sd_im2col3x3_c3_f16": (_IC, [
        ("null pointer", dict(x=None)), ("null pointer", dict(out=None)),
        ("bad shape ldx=3", dict(ldx=3)), ("bad shape ldx=6", dict(ldx=6)), ("bad shape ldx=0", dict(ldx=0)),
        ("bad shape", dict(batch=0)), ("bad shape", dict(h=0)), ("bad shape", dict(w_=0)), ("bad shape", dict(h=-2)),
        ("too many pixels", dict(batch=2, h=32768, w_=32768)), ("too many pixels", dict(batch=32768, h=65536, w_=1))]),
}
