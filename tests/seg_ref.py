"""Case tables and references of the domain tests of the person-segmentation kernels (coma_amd/csrc/seg_gemm.hip, seg_ops.hip): what
tests/test_seg_gemm_domain_gpu.py and tests/test_seg_ops_domain_gpu.py launch, and what tests/test_seg_ref_host.py checks on the CPU.  No
GPU is needed to import this module.  The guards (at this suite's width of 64), the sentinels, the seeds and the refusal rows' PTR are
tests/domain_kit.py's.

Every case is one launch (or one short chain) with an id.  make_*_inputs draws the operands from a generator seeded by the id; every
operand element the contract says is not read is NaN (integer buffers: an index no reference could use), every output starts as SENTINEL
and sits between guards.  References are float64, or exact integer / index arithmetic where the operator decides indices; where
oracle/seg_oracle.py restates an operator it is called, with a float64 restatement beside it where a tolerance is derived.

GEMM bound: |got - ref64| <= gamma_t * (sum_k |a_k w_k| + |bias| + |res|), gamma_t = t u / (1 - t u), u = 2^-24,
t = (real k terms) + 3: the forward bound of ANY fp32 summation order with one rounding per product or FMA, the split-K reduce order
included.  The integer family (operands in [-4, 4]) keeps every partial sum below 2^24, so any order is exact: bit for bit."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import seg_oracle as so
from tests import domain_kit as kit
from tests.domain_kit import PTR, U32 as U

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
GUARD = 64                                   # elements in front of and behind every device buffer (a multiple of 16 bytes for every type)
NAN = float("nan")
seed_of, rng_of, gen_of = kit.seed, kit.rng, kit.gen            # (case id, salt) -> the crc32 seed / a numpy / a torch generator
# the kit's guards, at this suite's width: NaN for floats, `fill` (default -1 / 0xA5 for bytes) for integers
guarded, guards_intact = functools.partial(kit.guarded, guard=GUARD), functools.partial(kit.guards_intact, guard=GUARD)


def gamma(t):
    return t * U / (1.0 - t * U)


def sentinel(*shape):
    """An fp32 tensor of the sentinel, a quiet NaN no kernel produces."""
    return kit.sentinel(math.prod(shape), F32).view(shape)


# ====================================================================================================================== the fp32 GEMM
@dataclass(frozen=True)
class GemmCase:
    id: str
    batch: int
    in_h: int
    in_w: int
    c: int
    n: int
    kh: int = 1
    kw: int = 1
    stride: int = 1
    pad: int = 0
    kpad: int = 0                            # 0: kh * kw * c rounded up to 32
    ldx: int = 0
    ldr: int = 0
    ldo: int = 0
    bias: bool = True
    bias_off: int = 0                        # floats between a 16-byte boundary and the bias (the kernel reads an aligned bias as float4)
    relu: bool = False
    res_mode: int = 0
    tile: int = 0
    split_k: int = 0
    ws_slabs: int = 0                        # the workspace holds exactly this many slabs of the expected tile (0: no workspace)
    counts: Optional[Tuple[int, ...]] = None  # m_dev
    rows_per_item: int = 1
    unit_rows: int = 0
    # the launch this case is meant to reach (seg_conv_gemm_describe must agree): tile 1 / 2 / 3, uniform-tap addressing, residual prefetch, slices
    x_tile: int = 0
    x_uni: bool = False
    x_pre: bool = False
    x_splits: int = 1

    @property
    def out_h(self):
        return (self.in_h + 2 * self.pad - self.kh) // self.stride + 1

    @property
    def out_w(self):
        return (self.in_w + 2 * self.pad - self.kw) // self.stride + 1

    @property
    def m(self):
        return self.batch * self.out_h * self.out_w

    @property
    def k(self):
        return self.kh * self.kw * self.c

    @property
    def kp(self):
        return self.kpad or -(-self.k // 32) * 32

    @property
    def nk(self):
        return self.kp // 32

    @property
    def ldx_(self):
        return self.ldx or self.c

    @property
    def ldr_(self):
        return self.ldr or self.n

    @property
    def ldo_(self):
        return self.ldo or self.n

    @property
    def bn(self):
        return {1: 128, 2: 64, 3: 32}[self.x_tile]

    @property
    def slab_elems(self):
        return -(-self.m // 128) * 128 * -(-self.n // self.bn) * self.bn

    @property
    def gated(self):
        return self.counts is not None


def _g(id, batch, in_h, in_w, c, n, x, **kw):
    """x = (tile, splits) the case is meant to reach; uni and pre follow from the definition of the instantiations."""
    case = GemmCase(id=id, batch=batch, in_h=in_h, in_w=in_w, c=c, n=n, x_tile=x[0], x_splits=x[1], x_uni=c % 32 == 0, **kw)
    return replace(case, x_pre=case.res_mode != 0 and x[1] == 1 and case.nk <= 4)


GATE = dict(rows_per_item=49, unit_rows=245)          # two units of 245 rows: the unit boundary falls inside the row tile 128 .. 255
GEMM_CASES = [
    # ---- the six instantiations with the residual prefetch (PRE: residual, unsplit, nk <= 4), nk = 1, 2, 3, 4: both branches of the peeled tail
    _g("pre-t1-uni-nk1-res1-m127-n129", 1, 1, 127, 32, 129, (1, 1), tile=1, res_mode=1, relu=True, ldo=132, ldr=132),
    _g("pre-t2-uni-nk2-res2-m128-n65", 1, 8, 16, 64, 65, (2, 1), tile=2, res_mode=2, ldo=68, ldr=68),
    _g("pre-t3-uni-nk3-res1-m129-n33", 1, 3, 43, 96, 33, (3, 1), tile=3, res_mode=1, relu=True, ldo=36, ldr=36),
    _g("pre-t2-uni-nk4-res2-m300-n250-tail", 3, 10, 10, 128, 250, (2, 1), res_mode=2, ldo=252, ldr=252),      # the rule: 128 x 64; last column piece scalar
    _g("pre-t1-uni-nk4-res1-m300-n250", 3, 10, 10, 128, 250, (1, 1), tile=1, res_mode=1, relu=True, ldo=252, ldr=252),
    _g("pre-t3-c36-nk2-res1-m1-n31", 1, 1, 1, 36, 31, (3, 1), res_mode=1, ldo=32, ldr=32),
    _g("pre-t2-c12-3x3-nk4-res2-n63", 1, 6, 8, 12, 63, (2, 1), kh=3, kw=3, pad=1, res_mode=2, relu=True, ldo=64, ldr=64),
    _g("pre-t1-c36-nk2-res1-m129-n127", 1, 3, 43, 36, 127, (1, 1), tile=1, res_mode=1, ldo=128, ldr=128),
    # ---- the residual in the epilogue (nk >= 5), vector path
    _g("epi-t1-uni-nk5-res1-m300-n128", 3, 10, 10, 160, 128, (1, 1), tile=1, res_mode=1, relu=True),
    _g("epi-t2-uni-nk8-res2-n64", 1, 4, 6, 256, 64, (2, 1), res_mode=2),
    _g("epi-t3-uni-3x3-nk9-res1-n15", 2, 5, 7, 32, 15, (3, 1), kh=3, kw=3, pad=1, res_mode=1, ldo=16, ldr=16),
    # ---- the scalar tail: a leading dimension that is no multiple of 4
    _g("tail-t3-nk2-res1-ldr35-n33", 1, 9, 9, 64, 33, (3, 1), tile=3, res_mode=1, ldr=35, ldo=36),            # PRE instantiation, residual read in the tail
    _g("tail-t2-nk5-res2-ldo67-n65", 1, 6, 10, 160, 65, (2, 1), tile=2, res_mode=2, ldo=67, relu=True),
    _g("tail-t1-nobias-ldo131-n129", 1, 7, 11, 64, 129, (1, 1), tile=1, bias=False, ldo=131),
    # ---- the addressing without uniform taps: c = 4 (the stem), 12, 36, 336 (the point head: kpad 352)
    _g("stem-c4-7x7s2p3-n64", 2, 13, 11, 4, 64, (2, 1), kh=7, kw=7, stride=2, pad=3, relu=True),
    _g("c336-kpad352-ldx340-m300-n256", 300, 1, 1, 336, 256, (2, 1), kpad=352, ldx=340, relu=True),
    _g("t1-c12-3x3-n129", 2, 9, 9, 12, 129, (1, 1), tile=1, kh=3, kw=3, pad=1),
    _g("t3-c36-1x1-n15-nobias", 1, 5, 5, 36, 15, (3, 1), bias=False, ldo=16),
    _g("t2-bias-unaligned-res1-nk2-n63", 1, 10, 10, 64, 63, (2, 1), bias_off=1, res_mode=1, ldo=64, ldr=64),
    _g("t1-bias-unaligned-nk5-n129", 1, 10, 10, 160, 129, (1, 1), tile=1, bias_off=3, relu=True, ldo=132),
    # ---- forced tiles and the rule on one 3 x 3 shape; the longest K
    _g("t1-uni-3x3-nk18-n129", 2, 9, 9, 64, 129, (1, 1), tile=1, kh=3, kw=3, pad=1, relu=True),
    _g("t2-uni-3x3-nk18-n65", 2, 9, 9, 64, 65, (2, 1), tile=2, kh=3, kw=3, pad=1, relu=True),
    _g("t3-uni-3x3-nk18-n33", 2, 9, 9, 64, 33, (3, 1), tile=3, kh=3, kw=3, pad=1, relu=True),
    _g("rule-n15-t3", 1, 10, 10, 64, 15, (3, 1), ldo=16),
    _g("rule-n63-t2", 1, 10, 10, 64, 63, (2, 1), ldo=64),
    _g("rule-n250-t2", 3, 10, 10, 64, 250, (2, 1)),                                                             # ldo = 250: every store scalar
    # the 128 x 64 rule's other outcome needs more than 256 narrow tiles against at most 256 wide ones: 52 row tiles, the one case above M = 600
    _g("rule-n260-m6530-nk13-t1", 6530, 1, 1, 416, 260, (1, 1)),
    _g("t1-uni-3x3-nk72-m25-n129", 1, 5, 5, 256, 129, (1, 1), tile=1, kh=3, kw=3, pad=1, ldo=132),
    # ---- gather forms
    _g("gather-1x1s2-odd-n33", 2, 7, 9, 64, 33, (2, 1), stride=2, ldo=36),
    _g("gather-3x3s2p1-n65", 2, 9, 7, 32, 65, (2, 1), kh=3, kw=3, stride=2, pad=1, ldo=68),
    _g("gather-2x2s2-n127", 3, 6, 6, 64, 127, (2, 1), kh=2, kw=2, stride=2, ldo=128),
    _g("gather-1x3-n31", 1, 5, 7, 32, 31, (3, 1), kh=1, kw=3, ldo=32),
    _g("gather-3x1-c12-n15", 1, 7, 5, 12, 15, (3, 1), kh=3, kw=1, ldo=16),
    _g("gather-3x3-pad2-n63", 1, 5, 6, 32, 63, (2, 1), kh=3, kw=3, pad=2, ldo=64),
    _g("gather-inh1-3x3p1-n129", 1, 1, 9, 64, 129, (2, 1), kh=3, kw=3, pad=1, ldo=132),
    _g("gather-inw1-3x3s2p1-c4-n1", 1, 9, 1, 4, 1, (3, 1), kh=3, kw=3, stride=2, pad=1, ldo=4),
    _g("ldx72-uni-3x3-n250-ldo256", 1, 6, 7, 64, 250, (2, 1), kh=3, kw=3, pad=1, ldx=72, ldo=256),
    # ---- the row gate: counts on the device, gated-out input rows NaN
    _g("gate-partial-n65", 490, 1, 1, 64, 65, (2, 1), counts=(5, 2), relu=True, ldo=68, **GATE),
    _g("gate-zero-n65", 490, 1, 1, 64, 65, (2, 1), counts=(0, 0), ldo=68, **GATE),
    _g("gate-empty-tile-n65", 490, 1, 1, 64, 65, (2, 1), counts=(1, 0), ldo=68, **GATE),
    _g("gate-empty-tile-split2-nk8", 490, 1, 1, 256, 65, (2, 2), counts=(1, 0), split_k=2, ws_slabs=2, ldo=68, **GATE),
    _g("gate-pre-t1-res1-n129", 490, 1, 1, 128, 129, (1, 1), tile=1, counts=(3, 1), res_mode=1, relu=True, ldo=132, ldr=132, **GATE),
    _g("gate-t3-split3-res1-nk8", 490, 1, 1, 256, 33, (3, 3), tile=3, counts=(2, 5), split_k=3, ws_slabs=3, res_mode=1, ldo=36, ldr=36, **GATE),
    _g("gate-c336-n256-ldo336", 490, 1, 1, 336, 256, (2, 1), kpad=352, counts=(2, 5), relu=True, ldo=336, **GATE),
    # ---- split-K
    # 8 narrow tiles x 36 chunks: the cost model takes 8 slices (nk_per = ceil(36 / 8) = 5: 7 slices of 5 chunks and one of 1); a workspace of 3 slabs: 3
    _g("split0-rule-splits8-3x3-res1", 2, 10, 12, 128, 256, (2, 8), kh=3, kw=3, pad=1, res_mode=1, relu=True, ws_slabs=16),
    _g("split0-rule-holds-3-slabs", 2, 10, 12, 128, 256, (2, 3), kh=3, kw=3, pad=1, res_mode=1, relu=True, ws_slabs=3),
    _g("split0-rule-nk7-unsplit", 1, 10, 10, 224, 33, (2, 1), ws_slabs=4, ldo=36),
    _g("split2-nk8-res1-m129-n33", 1, 3, 43, 256, 33, (2, 2), split_k=2, ws_slabs=2, res_mode=1, ldo=36, ldr=36),
    _g("split5-ragged-nk9-res2-n250", 2, 6, 6, 32, 250, (2, 5), kh=3, kw=3, pad=1, split_k=5, ws_slabs=5, res_mode=2, relu=True),
    _g("split7-clamped-nk3-res1", 1, 10, 10, 96, 65, (2, 3), split_k=7, ws_slabs=3, res_mode=1, ldo=68, ldr=68),
    _g("split-never-nk36", 2, 10, 12, 128, 256, (2, 1), kh=3, kw=3, pad=1, split_k=-1, ws_slabs=16),
    _g("split2-c12-3x3-nk4-n31", 1, 6, 8, 12, 31, (3, 2), kh=3, kw=3, pad=1, split_k=2, ws_slabs=2, ldo=32),
    _g("split5-t1-nk72-m25-n129", 1, 5, 5, 256, 129, (1, 5), tile=1, kh=3, kw=3, pad=1, split_k=5, ws_slabs=5, res_mode=1, relu=True, ldo=132, ldr=132),
    _g("split2-stem-c4-nk7", 2, 13, 11, 4, 64, (2, 2), kh=7, kw=7, stride=2, pad=3, split_k=2, ws_slabs=2, relu=True),
]
GEMM_FAMILIES = ("int", "normal")


@dataclass
class GemmInputs:
    x: torch.Tensor                           # [batch, in_h, in_w, ldx]; gap columns and gated-out rows NaN
    w: torch.Tensor                           # [n, kpad], zero beyond k
    bias: Optional[torch.Tensor]
    res: Optional[torch.Tensor]               # [rows, ldr]; gap columns NaN
    m_dev: Optional[torch.Tensor]


def gemm_valid_rows(c):
    """bool [M]: the rows the launch computes."""
    ok = torch.ones(c.m, dtype=torch.bool)
    if c.gated:
        m = torch.arange(c.m)
        ok = (m % c.unit_rows) < torch.tensor(c.counts)[m // c.unit_rows] * c.rows_per_item
    return ok


def make_gemm_inputs(c, family):
    g = torch.Generator().manual_seed(seed_of(c.id, GEMM_FAMILIES.index(family)))
    if family == "int":
        draw = lambda *s: torch.randint(-4, 5, s, generator=g).to(F32)
        wdraw = draw
    else:
        draw = lambda *s: torch.randn(*s, generator=g)
        wdraw = lambda *s: torch.randn(*s, generator=g) / math.sqrt(c.k)
    x = torch.full((c.batch, c.in_h, c.in_w, c.ldx_), NAN)
    x[..., :c.c] = draw(c.batch, c.in_h, c.in_w, c.c)
    if c.gated:
        assert c.kh == c.kw == c.stride == 1 and c.pad == 0 and c.m == c.batch and c.m == len(c.counts) * c.unit_rows
        x[~gemm_valid_rows(c)] = NAN
    w = torch.zeros(c.n, c.kp)
    w[:, :c.k] = wdraw(c.n, c.k)
    bias = draw(c.n) if c.bias else None
    res = None
    if c.res_mode:
        rows = c.m if c.res_mode == 1 else c.batch * (c.out_h // 2) * (c.out_w // 2)
        res = torch.full((rows, c.ldr_), NAN)
        res[:, :c.n] = draw(rows, c.n)
        if c.gated:
            res[~gemm_valid_rows(c)] = NAN
    m_dev = torch.tensor(c.counts, dtype=I32) if c.gated else None
    return GemmInputs(x, w, bias, res, m_dev)


def _res_rows(c, res, dtype):
    """The residual operand as [M, n] in `dtype` (res_mode 2: read at (oy >> 1, ox >> 1))."""
    r = res[:, :c.n].to(dtype)
    if c.res_mode == 2:
        r = r.view(c.batch, c.out_h // 2, c.out_w // 2, c.n)
        r = r.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).reshape(c.m, c.n)
    return r


def _conv(c, x, w, dtype):
    xs = x[..., :c.c].to(dtype).nan_to_num(0.0).permute(0, 3, 1, 2)          # gated-out rows are NaN: not compared, and a 1 x 1 row feeds no other
    ws = w[:, :c.k].to(dtype).view(c.n, c.kh, c.kw, c.c).permute(0, 3, 1, 2)
    return F.conv2d(xs, ws, None, stride=c.stride, padding=c.pad).permute(0, 2, 3, 1).reshape(c.m, c.n), xs, ws


def gemm_reference(c, inp, dtype=F64):
    """-> (out [M, n], mag [M, n]) in `dtype`: the launch's result and sum_k |a_k w_k| + |bias| + |res| (the bound's magnitude)."""
    acc, xs, ws = _conv(c, inp.x, inp.w, dtype)
    mag = F.conv2d(xs.abs(), ws.abs(), None, stride=c.stride, padding=c.pad).permute(0, 2, 3, 1).reshape(c.m, c.n)
    if c.bias:
        acc, mag = acc + inp.bias.to(dtype), mag + inp.bias.to(dtype).abs()
    if c.res_mode:
        r = _res_rows(c, inp.res, dtype).nan_to_num(0.0)
        acc, mag = acc + r, mag + r.abs()
    return (acc.clamp_min(0) if c.relu else acc), mag


def gemm_bound(c, mag):
    """The per-element bound of the module docstring (ReLU does not enlarge a difference)."""
    return gamma(c.k + 3) * mag.to(F64)


def gemm_int_peak(c, inp):
    """The largest magnitude any partial sum of the integer family can reach: sum_k |a_k w_k| + |bias| + |res|."""
    return float(gemm_reference(c, inp)[1].max())


def gemm_written_mask(c):
    """bool [M, ldo]: what the launch has to write."""
    mask = torch.zeros(c.m, c.ldo_, dtype=torch.bool)
    mask[:, :c.n] = gemm_valid_rows(c)[:, None]
    return mask


def gemm_kwargs(c, t):
    """Keywords of coma_amd.seg.ops.conv_gemm / conv_gemm_describe; t: name -> tensor (or address) of x, w, out, bias, res, m_dev, workspace."""
    kw = dict(batch=c.batch, in_h=c.in_h, in_w=c.in_w, c=c.c, n=c.n, kpad=c.kp, kh=c.kh, kw=c.kw, stride=c.stride, pad=c.pad, ldx=c.ldx,
              ldr=c.ldr, ldo=c.ldo, relu=c.relu, res_mode=c.res_mode, tile=c.tile, split_k=c.split_k, bias=t.get("bias"), res=t.get("res"))
    if c.gated:
        kw.update(m_dev=t["m_dev"], rows_per_item=c.rows_per_item, unit_rows=c.unit_rows)
    if c.ws_slabs:
        kw.update(workspace=t["workspace"], workspace_bytes=c.ws_slabs * c.slab_elems * 4)
    return kw


def gemm_fake_tensors(c):
    """Addresses that are never dereferenced: what seg_conv_gemm_describe needs on a machine without a GPU."""
    t = dict(x=4096, w=8192, out=12288, bias=16384 if c.bias else None, res=20480 if c.res_mode else None)
    if c.gated:
        t["m_dev"] = 24576
    if c.ws_slabs:
        t["workspace"] = 28672
    return t


# (text the refusal must contain, changes to GEMM_REFUSAL_BASE); PTR = any valid address
GEMM_REFUSAL_BASE = dict(x=PTR, w=PTR, out=PTR, batch=1, in_h=4, in_w=4, c=32, n=16, kpad=32)
GEMM_REFUSALS = [
    ("null pointer", dict(x=None)),
    ("null pointer", dict(w=None)),
    (r"batch=0", dict(batch=0)),
    (r"n=0", dict(n=0)),
    (r"out=0x4", dict(kh=5, kpad=800)),
    (r"c=30 \(a multiple of 4\)", dict(c=30)),
    (r"stride=0", dict(stride=0, out_h=4, out_w=4)),
    (r"pad=-1", dict(pad=-1)),
    (r"ldx=28", dict(ldx=28)),
    (r"ldx=34", dict(ldx=34)),
    (r"kpad=48 must be a multiple of 32", dict(kpad=48)),
    (r"kpad=32 must be a multiple of 32 covering kh\*kw\*c=288", dict(kh=3, kw=3, pad=1)),
    (r"res_mode=3", dict(res_mode=3, res=PTR)),
    (r"res_mode=1 without a residual", dict(res_mode=1)),
    (r"up-sampled residual needs even out_h, out_w", dict(res_mode=2, res=PTR, in_w=5)),
    (r"rows_per_item=0 unit_rows=16", dict(m_dev=PTR, rows_per_item=0, unit_rows=16)),
    (r"rows_per_item=1 unit_rows=0", dict(m_dev=PTR, rows_per_item=1, unit_rows=0)),
    (r"ldo=12 < n=16", dict(ldo=12)),
    (r"split_k=-2", dict(split_k=-2)),
    (r"workspace_bytes=8", dict(workspace=PTR, workspace_bytes=8)),
    (r"tile=4", dict(tile=4)),
    (r"tile=-1", dict(tile=-1)),
    (r"split_k=2 needs a workspace of 32768 bytes", dict(c=64, kpad=64, split_k=2)),                       # no workspace at all
    # a forced factor means exactly that many slices: a workspace that holds fewer slabs (128 x 32 floats each here) is refused, it used to
    # run with as many slices as fitted
    (r"split_k=2 needs a workspace of 32768 bytes", dict(c=64, kpad=64, split_k=2, workspace=PTR, workspace_bytes=32764)),
    (r"split_k=5 needs a workspace of 32768 bytes", dict(c=64, kpad=64, split_k=5, workspace=PTR, workspace_bytes=16384)),   # clamped to nk = 2 first
]


# ====================================================================================================================== level assignment
# the three cut points of roi_align_kernel (seg_ops.hip): the smallest fp32 v = sqrt(area) / 224 + 1e-8 for which assign_levels' own
# expression floor(4 + log2(v)) reaches level 3, 4, 5
LEVEL_CUTS = (float.fromhex("0x1.fffffcp-2"), float.fromhex("0x1.fffffep-1"), float.fromhex("0x1.fffffap+0"))


def level_by_cuts(v):
    """The kernel's rule on fp32 values v (a NaN compares false: level 0)."""
    v = torch.as_tensor(v, dtype=F32)
    return sum((v >= torch.tensor(cut, dtype=F32)).to(I64) for cut in LEVEL_CUTS)


def level_by_formula(v):
    """assign_levels' expression on fp32 values v = sizes / 224 + 1e-8."""
    v = torch.as_tensor(v, dtype=F32)
    return torch.clamp(torch.floor(so.CANONICAL_LEVEL + torch.log2(v)), min=2, max=5).to(I64) - 2


def floats_around(x, n):
    """The 2 n + 1 fp32 values within n floats of x, ascending."""
    c = np.float32(x)
    lo = c
    for _ in range(n):
        lo = np.nextafter(lo, np.float32(-np.inf))
    out = [lo]
    for _ in range(2 * n):
        out.append(np.nextafter(out[-1], np.float32(np.inf)))
    return np.asarray(out, np.float32)


def level_boundary_boxes():
    """The boxes of the issue: sides on and up to 4 floats either side of 112, 224 and 448, square and 224-based rectangles -> f32 [54, 4]."""
    boxes = []
    for side in (112.0, 224.0, 448.0):
        for s in floats_around(side, 4):
            boxes.append([0.0, 0.0, float(s), float(s)])
            boxes.append([0.0, 0.0, float(s), side])
    return torch.tensor(boxes, dtype=F32)


# ====================================================================================================================== the operators
SENT_I32, SENT_U8 = kit.sentinel_bits(I32), kit.sentinel_bits(U8)     # 0xA5A5A5A5 (as int32: negative), 0xA5


def sentinel_i32(*shape):
    return kit.sentinel(math.prod(shape), I32).view(shape)


def desc_keys(scores, low):
    """The candidate key of include/seg_hip.h: (descending-order bits of the score) << 32 | low word -> int64."""
    s = np.asarray(scores, np.float32).copy()
    s[s == 0] = 0.0
    u = s.view(np.uint32)
    asc = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint64)
    return ((((~asc) & np.uint64(0xffffffff)) << np.uint64(32)) | np.asarray(low, np.uint64)).view(np.int64)


# ------------------------------------------------------------------ seg_memset
MEMSET_CASES = [(n, off) for n in (1, 15, 16, 17, 4096 + 5) for off in (0, 1, 8)]       # offset 0: the aligned 16-byte branch; 1, 8: the scalar one

# ------------------------------------------------------------------ pooling: (h, w, c), batch 3
POOL_CASES = [(1, 1, 4), (1, 2, 68), (2, 7, 4), (7, 8, 68), (8, 1, 4), (8, 8, 68), (7, 2, 4), (2, 1, 68)]


def make_pool_input(h, w, c, batch=3):
    g = gen_of(f"pool-{h}-{w}-{c}")
    x = torch.randn(batch, c, h, w, generator=g)
    x[torch.rand(batch, c, h, w, generator=g) < 0.2] = -math.inf                       # whole windows of -inf included
    return x


# ------------------------------------------------------------------ seg_resize_normalize_u8: (id, h, w, new_h, new_w, pad_h, pad_w, resized?)
RESIZE_CASES = [
    ("up-5x7-to-8x11", 5, 7, 8, 11, 12, 16, True),
    ("down-20x26-to-7x9-ksize7", 20, 26, 7, 9, 8, 12, True),
    ("strip-1x9-to-1x5", 1, 9, 1, 5, 4, 8, True),
    ("down-13x10-to-4x3-no-resized", 13, 10, 4, 3, 4, 4, False),
]
RESIZE_MEAN = so.PIXEL_MEAN


def make_resize_input(cid, h, w, batch=2):
    return rng_of(cid).integers(0, 256, size=(batch, h, w, 3)).astype(np.uint8)


# ------------------------------------------------------------------ seg_rpn_select / seg_rpn_select_levels
@dataclass(frozen=True)
class RpnCase:
    id: str
    dims: Tuple[Tuple[int, int], ...]
    pre_topk: int
    batch: int = 3
    img: Tuple[float, float] = (70.0, 90.0)            # (img_h, img_w)
    ld: int = 16
    slack: int = 7                                      # candidate slots behind the last level's: keep ~0

    @property
    def counts(self):
        return [fh * fw * 3 for fh, fw in self.dims]

    @property
    def takes(self):
        return [min(n, self.pre_topk) for n in self.counts]

    @property
    def cap(self):
        return sum(self.takes) + self.slack


RPN_SIZES = (32, 64, 128, 256, 512, 1024)
RPN_CASES = [
    # n > pre_topk, n == pre_topk, n < pre_topk, a larger level, one pixel, n == pre_topk again: six levels
    RpnCase("six-levels-topk48", ((6, 5), (4, 4), (3, 5), (7, 7), (1, 1), (2, 8)), 48),
    RpnCase("one-level-n-is-topk-plus-1", ((4, 4),), 47),
    RpnCase("one-level-9000-second-strip-round", ((60, 50),), 50, img=(300.0, 260.0)),
]


def make_rpn_preds(c):
    """-> list of f32 [batch, fh * fw, ld] per level: columns 0..2 logits, 3..14 deltas, the rest NaN (never read).  Image b of level 0: a block
    of equal logits straddling the cut; level 1 (or image 1 of a single level): all logits equal; level 2 / image 2: only +0 / -0."""
    g = gen_of(c.id)
    preds = []
    for l, (fh, fw) in enumerate(c.dims):
        p = torch.full((c.batch, fh * fw, c.ld), NAN)
        p[..., :3] = torch.randn(c.batch, fh * fw, 3, generator=g)
        p[..., 3:15] = torch.randn(c.batch, fh * fw, 12, generator=g) * 0.3
        n = fh * fw * 3
        flat = p[..., :3].reshape(c.batch, n).clone()
        for b in range(c.batch):
            kind = (l + b) % 4 if len(c.dims) > 1 else b
            if kind == 0 and n > c.pre_topk:              # a block of equal logits straddling the cut: about half of the places above it are larger
                order = torch.argsort(flat[b], descending=True)
                lo, hi = max(c.pre_topk - 5, 0), min(c.pre_topk + 9, n)
                flat[b, order[lo:hi]] = float(flat[b, order[lo]])
            elif kind == 1:
                flat[b] = 0.75                             # all equal: the first pre_topk anchors
            elif kind == 2:
                flat[b] = torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
        p[..., :3] = flat.view(c.batch, fh * fw, 3)
        if fh * fw >= 4:
            p[0, 1, 0] = math.inf                          # an infinite logit: selected first, then dropped (key ~0)
            p[c.batch - 1, 2, 3 + 4 * 1 + 2] = NAN         # a NaN delta of anchor 1 of pixel 2
            p[c.batch - 1, 2, 1] = 50.0                    # ... which is selected
        preds.append(p)
    return preds


def rpn_reference(c, preds):
    """-> per image, per level: dict(sel = selected anchors (set order: ascending), ok bool per selected, boxes f32 [k, 4] clipped)."""
    out = []
    for b in range(c.batch):
        levels = []
        for l, (fh, fw) in enumerate(c.dims):
            lg = preds[l][b, :, :3].reshape(-1)
            dl = preds[l][b, :, 3:15].reshape(-1, 4)
            anchors = so.grid_anchors(fh, fw, 4 << l, RPN_SIZES[l])
            idx = so.topk_stable(lg, min(lg.numel(), c.pre_topk))
            boxes = so.apply_deltas(dl[idx], anchors[idx], so.RPN_BBOX_WEIGHTS)
            valid = torch.isfinite(boxes).all(dim=1) & torch.isfinite(lg[idx])
            boxes = so.clip_boxes(boxes, *c.img)
            ok = valid & ((boxes[:, 2] - boxes[:, 0]) > 0) & ((boxes[:, 3] - boxes[:, 1]) > 0)
            order = torch.argsort(idx)
            levels.append(dict(sel=idx[order], ok=ok[order], boxes=boxes[order], scores=lg[idx][order]))
        out.append(levels)
    return out


# ------------------------------------------------------------------ seg_sort_candidates: one launch per cap, one image per count variant
SORT_CAPS = (64, 128, 1024, 8192)


def sort_variants(cap):
    """(valid count, where) per image: the counts of the issue, the only valid key in the last slot and in slot 0."""
    v = [(0, "random"), (1, "random"), (63, "random"), (64, "random"), (65, "random"), (cap, "random"), (1, "last"), (1, "first"), (65, "with-last")]
    return [(min(n, cap), where) for n, where in v]


def make_sort_inputs(cap):
    """-> keys i64 [B, cap], boxes f32 [B, cap, 4], group i32 [B, cap], and the reference order (slot indices) per image.  Slots without a
    candidate hold key ~0, NaN boxes and group -7: never read."""
    rng = rng_of(f"sort-{cap}")
    var = sort_variants(cap)
    B = len(var)
    keys = np.full((B, cap), -1, np.int64)
    boxes = np.full((B, cap, 4), np.nan, np.float32)
    group = np.full((B, cap), -7, np.int32)
    scores_all, orders = [], []
    for b, (n, where) in enumerate(var):
        slots = np.sort(rng.permutation(cap)[:n])
        if where == "last":
            slots = np.array([cap - 1])
        elif where == "first":
            slots = np.array([0])
        elif where == "with-last" and cap - 1 not in slots:
            slots[-1] = cap - 1
        sc = rng.normal(0, 2, n).astype(np.float32)
        if n > 3:
            sc[rng.integers(0, n, n // 3)] = sc[0]                                    # equal scores: ascending low word
            sc[1], sc[2] = 0.0, -0.0
        low = slots * 3 + 1                                                           # any distinct 32-bit words, ascending with the slot
        keys[b, slots] = desc_keys(sc, low)
        boxes[b, slots] = rng.uniform(0, 100, (n, 4)).astype(np.float32)
        group[b, slots] = rng.integers(0, 5, n)
        order = slots[torch.sort(torch.from_numpy(sc), descending=True, stable=True)[1].numpy()] if n else slots
        scores = np.zeros(cap, np.float32)
        scores[slots] = np.where(sc == 0, np.float32(0.0), sc)                       # the key maps -0 to +0
        scores_all.append(scores)
        orders.append(order)
    return keys, boxes, group, np.stack(scores_all), orders


# ------------------------------------------------------------------ seg_nms
@dataclass(frozen=True)
class NmsCase:
    id: str
    cap: int
    n: Tuple[int, ...]                               # valid candidates per image
    max_keep: int
    thresh: float
    kind: str = "clusters"                           # "clusters" | "dyadic"
    groups: int = 3


NMS_CASES = [
    NmsCase("cap64-n0-n1", 64, (0, 1), 5, 0.5),
    NmsCase("cap64-n64-keep1", 64, (64, 30), 1, 0.5),
    NmsCase("cap128-n65-keep40-mid-block", 128, (65, 64), 40, 0.7, groups=1),
    NmsCase("cap128-dyadic-thresh-hit-exactly", 128, (96, 65), 200, 0.5, kind="dyadic", groups=2),
    NmsCase("cap8192-n4097-second-register", 8192, (4097, 300), 5000, 0.7),
]


def make_nms_inputs(c):
    """Sorted candidates (scores descending) -> boxes f32 [B, cap, 4], scores, group i32, src i32; slots >= n hold NaN / -7: never read."""
    rng = rng_of(c.id)
    B = len(c.n)
    boxes = np.full((B, c.cap, 4), np.nan, np.float32)
    scores = np.full((B, c.cap), np.nan, np.float32)
    group = np.full((B, c.cap), -7, np.int32)
    src = np.full((B, c.cap), -7, np.int32)
    for b, n in enumerate(c.n):
        if n == 0:
            continue
        if c.kind == "dyadic":
            # integer boxes [0, 0, w, h]: nested boxes have IoU = (w h) / (w' h'), a dyadic rational for these sides -- 0.5 exactly is NOT
            # suppressed (>), 0.75 is; identical boxes (IoU 1), zero-area boxes (IoU 0 or 0 / 0) among them
            sides = np.array([[4, 4], [4, 2], [4, 3], [2, 2], [8, 4], [8, 8], [4, 4], [0, 4], [0, 4], [0, 0], [0, 0], [16, 8]], np.float32)
            bx = np.zeros((n, 4), np.float32)
            pick = rng.integers(0, len(sides), n)
            off = (rng.integers(0, 2, n) * 64).astype(np.float32)                     # two far-apart piles
            bx[:, 0], bx[:, 1], bx[:, 2], bx[:, 3] = off, off, off + sides[pick, 0], off + sides[pick, 1]
        else:
            m = max(n // 6, 1)
            ctr, wh = rng.uniform(0, 400, (m, 2)), rng.uniform(8, 120, (m, 2))
            centres = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1)
            bx = (centres[rng.integers(0, m, n)] + rng.normal(0, 5, (n, 4))).astype(np.float32)
            bx[:, 2:] = np.maximum(bx[:, 2:], bx[:, :2] + 1)
            if n > 8:
                bx[5] = bx[6] = bx[7]                                                  # identical boxes
                bx[8, 2] = bx[8, 0]                                                    # zero area
        sc = np.sort(rng.normal(0, 2, n).astype(np.float32))[::-1].copy()
        if n > 20:
            sc[10:16] = sc[10]                                                         # equal scores keep their order
        boxes[b, :n], scores[b, :n] = bx, sc
        group[b, :n] = rng.integers(0, c.groups, n)
        src[b, :n] = rng.permutation(n) + 100
    return boxes, scores, group, src


def nms_reference(c, boxes, scores, group, b):
    n = c.n[b]
    if n == 0:
        return np.zeros(0, np.int64)
    return so.nms_ref(torch.from_numpy(boxes[b, :n]), torch.from_numpy(scores[b, :n]), group[b, :n], c.thresh)[:c.max_keep].numpy()


# ------------------------------------------------------------------ seg_roi_align_f32
@dataclass(frozen=True)
class RoiCase:
    id: str
    out_size: int
    c: int
    h2: int
    w2: int
    counts: Tuple[int, ...]
    R: int
    kind: str = "mixed"                              # "mixed" | "levels" | "wide" | "tall"


ROI_CASES = [
    RoiCase("out7-c260-16x24-partial", 7, 260, 16, 24, (20, 13), 20),
    RoiCase("out1-c4-8x8-count0", 1, 4, 8, 8, (0, 5), 6),
    RoiCase("out2-c4-16x24", 2, 4, 16, 24, (9, 9), 9),
    RoiCase("out14-c260-8x8", 14, 260, 8, 8, (5, 2), 5),
    RoiCase("out16-c4-16x24", 16, 4, 16, 24, (6, 3), 6),
    RoiCase("out2-c4-level-boundaries", 2, 4, 16, 24, (54,), 54, kind="levels"),
    RoiCase("out7-c4-wide-general-path", 7, 4, 64, 3712, (3,), 4, kind="wide"),
    RoiCase("out7-c4-tall-general-path", 7, 4, 3712, 64, (3,), 4, kind="tall"),
]


def make_roi_inputs(c):
    """-> feats (4 tensors f32 [B, C, h, w] NCHW), boxes f32 [B, R, 4]; rows past the count are NaN (never read)."""
    g, rng = gen_of(c.id), rng_of(c.id)
    B = len(c.counts)
    feats = [torch.randn(B, c.c, c.h2 >> l, c.w2 >> l, generator=g) for l in range(4)]
    W, H = 4.0 * c.w2, 4.0 * c.h2
    boxes = np.full((B, c.R, 4), np.nan, np.float32)
    for b, n in enumerate(c.counts):
        if c.kind == "levels":
            bx = level_boundary_boxes().numpy()
        elif c.kind == "wide":
            bx = np.array([[100, 20, 14500, 84], [300, 40, 420, 150], [10, 0, 14848, 256]], np.float32)      # 65 and 67 samples per bin on x (level p5)
        elif c.kind == "tall":
            bx = np.array([[20, 100, 84, 14500], [40, 300, 150, 420], [0, 10, 256, 14848]], np.float32)
        else:
            ctr = rng.uniform(0, [W, H], (c.R, 2))
            wh = rng.uniform(2, [W, H], (c.R, 2)) * rng.choice([0.2, 0.6, 1.5, 4.0], (c.R, 1))              # every level
            bx = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
            special = [[5, 5, 5, 30],                       # empty on x: no samples
                       [30, 40, 10, 60],                    # inverted on x
                       [30, 40, 10, 20],                    # inverted on both axes: positive area, no samples
                       [-20, -30, 50, 40],                  # partly outside
                       [8, 16, 36, 44]]                     # on cell boundaries of p2 and p3
            for i, s in enumerate(special[:max(n - 1, 0)]):
                bx[i] = s
        boxes[b, :n] = bx[:n]
    return feats, boxes


def roi_levels_reference(boxes):
    """assign_levels; a negative area (a box inverted on one axis) has a NaN size, for which the oracle's integer cast is undefined: the
    kernel's three comparisons are all false there, level 0."""
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    lv = so.assign_levels(torch.where(area[:, None] >= 0, boxes, torch.tensor([0.0, 0.0, 1.0, 1.0])))
    return torch.where(area >= 0, lv, torch.zeros_like(lv))


def _roi_axis(lo, hi, out_size, size, scale):
    """The sample table of one axis as the kernel builds it, in fp32: -> (grid, idx int64 [out * grid, 2], w f32 [out * grid, 2])."""
    f = np.float32
    a, b = f(f(lo) * f(scale)) - f(0.5), f(f(hi) * f(scale)) - f(0.5)
    ext = f(b - a)
    bin_ = f(ext / f(out_size))
    grid = max(int(math.ceil(float(bin_))), 0)
    i = np.arange(out_size * grid)
    p, s = (i // max(grid, 1)).astype(np.float32), (i % max(grid, 1)).astype(np.float32)
    v = (a + p * bin_).astype(np.float32) + ((s + f(0.5)) * bin_).astype(np.float32) / f(max(grid, 1))
    v = v.astype(np.float32)
    inside = ~((v < -1) | (v > size))
    v = np.where(v <= 0, f(0), v)
    v = np.where(inside, v, f(0)).astype(np.float32)
    lo_i = v.astype(np.int64)
    top = lo_i >= size - 1
    lo_i = np.where(top, size - 1, lo_i)
    hi_i = np.where(top, size - 1, lo_i + 1)
    v = np.where(top, lo_i.astype(np.float32), v)
    l = (v - lo_i.astype(np.float32)).astype(np.float32)
    h = (f(1) - l).astype(np.float32)
    w = np.stack([np.where(inside, h, f(0)), np.where(inside, l, f(0))], 1).astype(np.float32)
    return grid, np.stack([lo_i, hi_i], 1), w


def roi_align_reference64(feat, box, out_size, scale):
    """One ROI on feat [C, H, W]: the kernel's fp32 sample geometry and fp32 weight products, the weighted sum in float64.
    -> (out [C, out, out], mag [C, out, out] = sum |w f| / samples, samples per bin)."""
    C, H, W = feat.shape
    gh, yi, yw = _roi_axis(box[1], box[3], out_size, H, scale)
    gw, xi, xw = _roi_axis(box[0], box[2], out_size, W, scale)
    if gh == 0 or gw == 0:
        z = torch.zeros(C, out_size, out_size, dtype=F64)
        return z, z, 0
    w4 = (yw[:, :, None, None] * xw[None, None, :, :]).astype(np.float32)             # [ny, 2, nx, 2], one rounding each as on the device
    f = feat.double()[:, torch.from_numpy(yi)][:, :, :, torch.from_numpy(xi)]          # [C, ny, 2, nx, 2]
    t = f * torch.from_numpy(w4).double()
    shape = (C, out_size, gh, 2, out_size, gw, 2)
    cnt = float(gh * gw)
    return t.view(shape).sum(dim=(2, 3, 5, 6)) / cnt, t.abs().view(shape).sum(dim=(2, 3, 5, 6)) / cnt, gh * gw


def roi_bound(samples, mag):
    """t = 4 * samples + 2 roundings-worth: the products, the sum in any order, the division."""
    return gamma(4 * samples + 2) * mag


# ------------------------------------------------------------------ seg_box_predict
@dataclass(frozen=True)
class BoxPredCase:
    id: str
    ld: int
    R: int
    counts: Tuple[int, ...]
    thresh: float
    cap: int
    img: Tuple[float, float] = (200.0, 180.0)


BOXPRED_CASES = [
    # thresh = fl32(1 / 81): a row of 81 equal logits has every probability exactly AT the threshold -- not taken (the test is >)
    BoxPredCase("ld401-exact-threshold-count0", 401, 7, (7, 0, 4), float(np.float32(1.0) / np.float32(81.0)), 4096),
    BoxPredCase("ld404-cap16-overflow", 404, 9, (9, 5), 0.05, 16),
]


def make_boxpred_inputs(c):
    """-> pred f32 [B * R, ld] (gap columns NaN, rows past the count NaN), proposals f32 [B, R, 4]."""
    g, rng = gen_of(c.id), rng_of(c.id)
    B = len(c.counts)
    pred = torch.full((B * c.R, c.ld), NAN)
    pred[:, :81] = torch.randn(B * c.R, 81, generator=g) * 2.5
    pred[:, 81:401] = torch.randn(B * c.R, 320, generator=g) * 0.5
    pred[0, :81] = 1.25                                    # every probability 1 / 81 exactly
    pred[1, 7] = math.inf                                  # a non-finite logit: no candidate from this row
    pred[2, 80] = -math.inf                                # probability 0 for the background: an ordinary row
    ctr, wh = rng.uniform(0, 180, (B, c.R, 2)), rng.uniform(8, 100, (B, c.R, 2))
    props = np.concatenate([ctr - wh / 2, ctr + wh / 2], 2).astype(np.float32)
    for b, n in enumerate(c.counts):
        pred[b * c.R + n:(b + 1) * c.R] = NAN
        props[b, n:] = np.nan
    return pred, props


def boxpred_reference(c, pred, props, b):
    n = c.counts[b]
    rows = pred[b * c.R:b * c.R + n]
    return so.fast_rcnn_inference(rows[:, :81], rows[:, 81:401], torch.from_numpy(props[b, :n]), c.img, c.thresh)


def boxpred_border(c, ref, exact_rows=()):
    """Flat (roi * 80 + class) positions whose float64 probability lies within 1e-6 of the threshold, rows compared exactly left out."""
    p = ref["probs"][:, :80].double()
    near = (p - c.thresh).abs() < 1e-6
    for r in exact_rows:
        if r < len(near):
            near[r] = False
    return set(torch.nonzero(near.reshape(-1)).reshape(-1).tolist())


# ------------------------------------------------------------------ seg_point_sample_f32
@dataclass(frozen=True)
class SampleCase:
    id: str
    c: int
    P: int
    per_roi: bool
    grid: bool                                       # the regular grid (P = side^2) or explicit coordinates
    fh: int
    fw: int
    counts: Tuple[int, ...]
    R: int
    col0: int = 0
    ldo: int = 0
    n_copies: int = 1
    gap: int = 0                                     # floats between two copies


SAMPLE_CASES = [
    SampleCase("image-c80-grid196", 80, 196, False, True, 10, 12, (3, 1), 3),
    SampleCase("roi-c4-explicit5-col8-3copies", 4, 5, True, False, 7, 7, (2, 3), 3, col0=8, ldo=16, n_copies=3, gap=8),
    SampleCase("image-c4-explicit1-3points", 4, 1, False, False, 9, 5, (3,), 3),
    SampleCase("roi-c80-grid196-col4", 80, 196, True, True, 7, 7, (1, 2), 2, col0=4, ldo=88),
    SampleCase("image-c80-explicit5-3copies", 80, 5, False, False, 6, 11, (2, 0), 2, ldo=84, n_copies=3),
]
SPECIAL_COORDS = (0.0, 1.0, -0.1, 1.1, 0.5)


def make_sample_inputs(c):
    """-> feat f32 NCHW ([B or B * R, C, fh, fw]), boxes f32 [B, R, 4] (per_roi: None), coords f32 [B * R, P, 2] or None."""
    g, rng = gen_of(c.id), rng_of(c.id)
    B = len(c.counts)
    feat = torch.randn(B * c.R if c.per_roi else B, c.c, c.fh, c.fw, generator=g)
    boxes = None
    if not c.per_roi:
        W, H = 4.0 * c.fw, 4.0 * c.fh
        ctr, wh = rng.uniform(0, [W, H], (B, c.R, 2)), rng.uniform(4, [W, H], (B, c.R, 2))
        boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 2).astype(np.float32)
        boxes[0, 0] = [-8, -8, 20, 30]                                                 # samples outside the map: zero padding
    coords = None
    if not c.grid:
        coords = torch.rand(B * c.R, c.P, 2, generator=g)
        sp = torch.tensor(SPECIAL_COORDS)
        for r in range(B * c.R):                                                       # the exact edge values, on x and on y
            coords[r, 0, r % 2] = sp[r % len(sp)]
            if c.P > 1:
                coords[r, 1] = torch.stack([sp[(r + 1) % len(sp)], sp[(r + 2) % len(sp)]])
    for b, n in enumerate(c.counts):
        if boxes is not None:
            boxes[b, n:] = np.nan
        if coords is not None:
            coords[b * c.R + n:(b + 1) * c.R] = NAN
        if c.per_roi:
            feat[b * c.R + n:(b + 1) * c.R] = NAN
    return feat, boxes, coords


def sample_coords(c, coords, rois):
    return so.regular_grid(rois, int(round(math.sqrt(c.P)))) if c.grid else coords


def point_sample_reference64(c, feat, box, xy):
    """One ROI: feat [C, fh, fw], box f32 [4] or None, xy f32 [P, 2] -> (out f64 [P, C], mag [P, C]): the kernel's fp32 geometry and weights
    (four products of fp32 differences), the four taps summed in float64."""
    f = np.float32
    cx, cy = xy[:, 0].numpy().astype(f), xy[:, 1].numpy().astype(f)
    W, H = f(c.fw), f(c.fh)
    if c.per_roi:
        nx, ny = cx, cy
    else:
        bx = np.asarray(box, f)
        px, py = (cx * f(bx[2] - bx[0]) + bx[0]).astype(f), (cy * f(bx[3] - bx[1]) + bx[1]).astype(f)
        nx, ny = (px / f(W / f(0.25))).astype(f), (py / f(H / f(0.25))).astype(f)
    gx, gy = (f(2) * nx - f(1)).astype(f), (f(2) * ny - f(1)).astype(f)
    ix, iy = ((((gx + f(1)) * W).astype(f) - f(1)) / f(2)).astype(f), ((((gy + f(1)) * H).astype(f) - f(1)) / f(2)).astype(f)
    fx, fy = np.floor(ix), np.floor(iy)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1f, y1f = (fx + 1).astype(f), (fy + 1).astype(f)
    wx = [(x1f - ix).astype(f), (ix - fx).astype(f)]
    wy = [(y1f - iy).astype(f), (iy - fy).astype(f)]
    fd = feat.double()
    out = torch.zeros(len(cx), feat.shape[0], dtype=F64)
    mag = torch.zeros_like(out)
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < c.fw) & (yy >= 0) & (yy < c.fh)
            w = torch.from_numpy(np.where(ok, (wx[dx] * wy[dy]).astype(f), f(0))).double()
            v = fd[:, torch.from_numpy(np.clip(yy, 0, c.fh - 1)), torch.from_numpy(np.clip(xx, 0, c.fw - 1))].t()     # [P, C]
            out += v * w[:, None]
            mag += (v * w[:, None]).abs()
    return out, mag


# ------------------------------------------------------------------ seg_upsample2x_f32, seg_topk_points, seg_point_logit_scatter
UPSAMPLE_SIDES = (1, 2, 7, 28)
TOPK_CASES = [(1, 1), (7, 1), (7, 49), (28, 784), (70, 50)]                             # 70^2 = 4900: a second strip round with a ragged tail
TOPK_KINDS = ("random", "all-equal", "plus-minus-pairs", "zeros", "ties-at-the-cut", "past-count")


def make_topk_maps(s, k):
    """-> f32 [6, s, s], one map per TOPK_KINDS; the last one lies past the count."""
    g = gen_of(f"topk-{s}-{k}")
    n = s * s
    m = torch.randn(len(TOPK_KINDS), n, generator=g)
    m[1] = -0.6
    half = torch.randn((n + 1) // 2, generator=g).abs() + 0.01
    m[2] = torch.stack([half, -half], 1).reshape(-1)[:n]                                # |x| equal in pairs: ascending index decides
    m[3] = torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    order = torch.argsort(m[4].abs())
    lo, hi = max(k - 3, 0), min(k + 4, n)
    sign = torch.where(torch.rand(hi - lo, generator=g) < 0.5, -1.0, 1.0)
    m[4, order[lo:hi]] = float(m[4, order[lo]].abs()) * sign                                   # equal |logit| straddling the k-th place
    return m.view(-1, s, s)


def topk_reference(m, k):
    idx = torch.sort(so.topk_stable(-m.reshape(-1).abs(), k))[0]
    s = m.shape[-1]
    return idx, torch.stack((1.0 / (2 * s) + (idx % s).float() / s, 1.0 / (2 * s) + (idx // s).float() / s), dim=1)


LOGIT_CASES = [(3, 4, 7, True), (64, 68, 5, False), (336, 340, 7, False), (336, 352, 4, True)]       # (kdim, ldx, s, idx given)

# ------------------------------------------------------------------ seg_paste_masks
@dataclass(frozen=True)
class PasteCase:
    id: str
    s: int
    R: int
    counts: Tuple[int, ...]
    masks: bool = True
    cat_id: int = 0
    out_h: int = 16
    out_w: int = 24


PASTE_CASES = [
    PasteCase("s7-R5", 7, 5, (5, 3)),
    PasteCase("s28-R5-cat3", 28, 5, (4, 5), cat_id=3),
    PasteCase("s28-R1-no-masks", 28, 1, (1, 0), masks=False),
    PasteCase("s7-R1", 7, 1, (1, 1)),
]


def make_paste_inputs(c):
    """-> logits f32 [B * R, s, s], boxes f32 [B, R, 4], valid i32 [B, R], classes i32 [B, R]; rows past the count NaN / poison."""
    g, rng = gen_of(c.id), rng_of(c.id)
    B = len(c.counts)
    coarse = torch.randn(B * c.R, 1, 4, 4, generator=g) * 4
    logits = F.interpolate(coarse, size=(c.s, c.s), mode="bilinear", align_corners=False)[:, 0].contiguous()
    ctr, wh = rng.uniform(2, [c.out_w - 2, c.out_h - 2], (B, c.R, 2)), rng.uniform(3, [c.out_w, c.out_h], (B, c.R, 2))
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], 2).astype(np.float32)
    boxes = np.clip(boxes, 0, [c.out_w, c.out_h, c.out_w, c.out_h]).astype(np.float32)
    boxes[0, 0] = [2.5, 3.5, 14.5, 12.5]                   # every edge exactly on a pixel centre
    if c.R > 1:
        boxes[0, 1] = [5.0, 6.0, 6.0, 7.0]                 # covers one pixel
        boxes[0, 2] = [3.0, 3.0, 20.0, 3.0]                # an invalid (empty) box: valid = 0
    valid = ((boxes[..., 2] - boxes[..., 0] > 0) & (boxes[..., 3] - boxes[..., 1] > 0)).astype(np.int32)
    classes = rng.choice([0, 0, 3, 7], (B, c.R)).astype(np.int32)
    classes[0, 0] = c.cat_id
    for b, n in enumerate(c.counts):
        logits[b * c.R + n:(b + 1) * c.R] = NAN
        boxes[b, n:] = np.nan
        valid[b, n:] = 1                                   # poison: a kernel that read it would paste NaN boxes
        classes[b, n:] = c.cat_id
    return logits, boxes, valid, classes


def paste_reference(c, logits, boxes, valid, b):
    """-> (masks bool [n, H, W] by the oracle in fp32, float64 blended probability [n, H, W]) of image b's first count rows."""
    n = c.counts[b]
    lg, bb = logits[b * c.R:b * c.R + n], torch.from_numpy(boxes[b, :n])
    ok = torch.from_numpy(valid[b, :n]).bool()
    safe = torch.where(ok[:, None], bb, torch.tensor([0.0, 0.0, 1.0, 1.0]))
    ref = so.paste_masks(lg.sigmoid(), safe, c.out_h, c.out_w) & ok[:, None, None]
    x0, y0, x1, y1 = torch.split(safe.double(), 1, dim=1)
    img_y = (torch.arange(0, c.out_h, dtype=F64) + 0.5 - y0) / (y1 - y0) * 2 - 1
    img_x = (torch.arange(0, c.out_w, dtype=F64) + 0.5 - x0) / (x1 - x0) * 2 - 1
    grid = torch.stack((img_x[:, None, :].expand(n, c.out_h, c.out_w), img_y[:, :, None].expand(n, c.out_h, c.out_w)), dim=3)
    p64 = F.grid_sample(lg.double().sigmoid()[:, None], grid, align_corners=False)[:, 0] if n else torch.zeros(0, c.out_h, c.out_w, dtype=F64)
    return ref, p64


def paste_excluded(p64):
    """Pixels whose float64 blended probability lies within 1e-5 of 0.5: not compared (at most 1 % of a case's pixels)."""
    return (p64 - 0.5).abs() < 1e-5


# ------------------------------------------------------------------ refusals of the operator entry points: (function, text, arguments); P = a valid pointer
P = PTR
OPS_REFUSALS = [
    ("seg_memset", "bad args", (None, 0, 16)), ("seg_memset", "bad args", (P, 0, 0)),
    ("seg_maxpool3x3s2_f32", "bad args", (P, 1, 4, 4, 6, P)), ("seg_maxpool3x3s2_f32", "bad args", (P, 1, 0, 4, 4, P)),
    ("seg_subsample2_f32", "bad args", (P, 1, 4, 4, 2, P)), ("seg_subsample2_f32", "bad args", (P, 0, 4, 4, 4, P)),
    ("seg_resize_normalize_u8", "bad sizes", (P, 1, 4, 4, 8, 8, 7, 8, P, P, 3, P, P, 3, 0.0, 0.0, 0.0, P, None, P)),      # pad_h < new_h
    ("seg_resize_normalize_u8", "null pointer", (P, 1, 4, 4, 8, 8, 8, 8, P, P, 3, P, P, 3, 0.0, 0.0, 0.0, None, None, P)),
    ("seg_rpn_select", "bad sizes", (P, 14, 1, 4, 4, 4, P, 0, 0, 10, 64.0, 64.0, 0, 64, P, P, P)),                        # ld < 15
    ("seg_rpn_select", "bad sizes", (P, 16, 1, 4, 4, 4, P, 0, 0, 10, 64.0, 64.0, 60, 64, P, P, P)),                       # offset + topk > cap
    ("seg_sort_candidates", r"cap=96", (P, P, P, 1, 96, P, P, P, P, P)), ("seg_sort_candidates", r"cap=16384", (P, P, P, 1, 16384, P, P, P, P, P)),
    ("seg_sort_candidates", r"cap=32", (P, P, P, 1, 32, P, P, P, P, P)),
    ("seg_nms", r"cap=100 max_keep=10", (P, P, P, P, P, 1, 100, 0.5, 10, P, P, P, P, P, P, P)),
    ("seg_nms", r"cap=64 max_keep=0", (P, P, P, P, P, 1, 64, 0.5, 0, P, P, P, P, P, P, P)),
    ("seg_roi_align_f32", "bad sizes", (P, P, P, P, 12, 8, 4, P, P, 1, 1, 7, P, None)),                                    # h2 % 8
    ("seg_roi_align_f32", "bad sizes", (P, P, P, P, 8, 8, 6, P, P, 1, 1, 7, P, None)),                                     # c % 4
    ("seg_roi_align_f32", r"out_size=17 > 16", (P, P, P, P, 8, 8, 4, P, P, 1, 1, 17, P, None)),
    ("seg_box_predict", "bad sizes", (P, 400, P, P, 1, 4, 64.0, 64.0, 0.5, 16, P, P, P, P, None)),
    ("seg_box_predict", "bad sizes", (P, 401, P, P, 1, 4, 64.0, 64.0, 0.5, 0, P, P, P, P, None)),
    ("seg_finalize_detections", "bad args", (P, P, 0, 4, 64.0, 64.0, 16, 16, P, P)),
    ("seg_point_sample_f32", "null pointer", (P, 7, 7, 4, 0, 0.25, None, P, 1, 1, None, 4, 2, P, 4, 0, 1, 0)),            # per_roi = 0 without boxes
    ("seg_point_sample_f32", "bad sizes", (P, 7, 7, 4, 1, 1.0, None, P, 1, 1, None, 5, 2, P, 4, 0, 1, 0)),                # grid_side^2 != P
    ("seg_point_sample_f32", "bad sizes", (P, 7, 7, 4, 1, 1.0, None, P, 1, 1, None, 4, 2, P, 8, 8, 1, 0)),                # ldo < col0 + c
    ("seg_point_sample_f32", "bad sizes", (P, 7, 7, 4, 1, 1.0, None, P, 1, 1, None, 4, 2, P, 6, 0, 1, 0)),                # ldo % 4
    ("seg_upsample2x_f32", "bad args", (P, P, 1, 1, 0, P)),
    ("seg_topk_points", "bad args", (P, P, 1, 1, 7, 50, P, P)), ("seg_topk_points", "bad args", (P, P, 1, 1, 7, 0, P, P)),
    ("seg_point_logit_scatter", "bad args", (P, 3, 4, P, P, P, P, 1, 1, 4, None, P, 2)),                                   # ldx < kdim
    ("seg_point_logit_scatter", "bad args", (P, 4, 4, P, P, P, P, 1, 1, 5, None, P, 2)),                                   # no idx and P != s^2
    ("seg_paste_masks", "bad args", (P, 7, P, P, P, P, 1, 1, 0, 8, 0, None, P)), ("seg_paste_masks", "bad args", (P, 7, P, P, P, P, 1, 1, 8, 8, 0, None, None)),
]
