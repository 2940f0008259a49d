"""Test helper for the normalisation and Winograd operators (coma_amd/csrc/sd_norm.hip, sd_winograd.hip): plain torch / numpy on the CPU,
nothing here is product code and nothing here needs a GPU.

* ``CASES``            the table of launches (named tuples, one type per family), shared by tests/test_norm_ref_host.py (references,
                       emulation, coverage, refusals) and tests/test_sd_norm_domain_gpu.py.
* ``inputs``           fp16 / fp32 operands of a case, seeded by its name.
* ``yardstick``        per output: the float64 reference (the operator's formula with this file's own index arithmetic; fp16 rounding only at
                       the storage points include/sd_hip.h names), the fp32 emulation of a careful kernel (one-pass GroupNorm sums with
                       var = max(q / count - mean^2, 0) and an fp32 affine table, two-pass LayerNorm, exp through float64, every sum in index
                       order), e_emu = the emulation's largest row error (each element's error over the largest |ref| of its output row), the
                       device bound max(4 e_emu, 2^-10), and the emulation's own a-priori bound (``stated``; the derivations are at the
                       functions that compute them).
* ``inputs`` / ``outputs``  give tests/domain_kit.py's Operand / Out records; its pack / new_out / masks make of them the flat buffers as the
                       kernels see them: 256 NaN elements in front of and behind every operand, NaN gap columns, outputs filled with a
                       sentinel NaN pattern and guarded exactly where the documented size ends.
* ``groupnorm_route``, ``layernorm_instantiation``, ``gn_wino_vec``, ``wino_output_kernel``  a transcript of the dispatch of the entry points,
                       written beside the table: which kernel a row reaches.  ``REACHABLE`` is every branch the entry points have.
* ``REFUSALS``         per entry point: a base argument list that is accepted, and every change the argument checks refuse, with the text;
                       written with the kit's PTR / Off and put to the entry points by its check_refusals.

DESIGN.md section 3e has the numbers."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

from tests import domain_kit as kit
from tests.domain_kit import (F16, F32, F64, GUARD, PTR, U32, Operand, Out, body, device_bound, exp32, gen, masks, new_out, pack,  # noqa: F401
                              randn16, row_error, sum32)            # (pack / new_out / masks: a case's buffers, also through this module)

UD = 4 * U32                     # allowance for one fp32 division, rsqrt or reciprocal
LIP = 1.1                        # Lipschitz constant of SiLU (1.0999)
GN_MAX_C, GN_SMALL_ITEMS, GN_WINO_MAX_SLICE = 2560, 5120, 20480
# fp32 operators of the oracle against float64: a few hundred fp32 roundings (statistics over up to 16 k elements, summed pairwise or
# by vector lanes, then about ten operations per element) -> 2^-24 * 128 = 2^-17 of (1 + the output's largest value)
ORACLE_LIMIT = 2.0 ** -17

BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=F64)
GM = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=F64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=F64)


def close_to_oracle(ref, theirs):
    return float((ref - theirs.to(F64)).abs().max()) <= ORACLE_LIMIT * (1 + float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------------------------ the table
class GN(NamedTuple):
    """sd_groupnorm_f16 (entry 'gn'), sd_groupnorm_colstats_f16 ('gn_cs'), sd_groupnorm_table_f16 from a statistics pass ('table') or from
    column sums ('table_cs'), sd_groupnorm_table_cat_f16 ('table_cat')."""
    name: str
    entry: str
    B: int
    hw: int
    c0: int
    c1: int
    G: int
    eps: float = 1e-5
    silu: int = 1
    dist: str = "n"             # n: N(0, 1);  shift: 8 + 0.25 N(0, 1) (mean ~ 30 std);  const: 3.0 everywhere
    rps: int = 32               # rows per column-sum slot

    family = "groupnorm"

    @property
    def id(self):
        return f"{self.entry}-{self.name}"

    @property
    def C(self):
        return self.c0 + self.c1

    @property
    def cg(self):
        return self.C // self.G


class LN(NamedTuple):
    name: str
    rows: int
    c: int
    eps: float = 1e-5
    family = "layernorm"

    @property
    def id(self):
        return f"ln-{self.name}"


class SM(NamedTuple):
    name: str
    rows: int
    n: int
    dld: int                    # ld = n + dld
    scale: float
    kind: str = "n"             # n: N(0, 2);  equal: every row constant;  underflow: one value 0, the others -300 .. -200
    family = "softmax"

    @property
    def id(self):
        return f"softmax-{self.name}"


class WI(NamedTuple):
    name: str
    B: int
    h: int
    w: int
    c0: int
    c1: int = 0
    up: int = 0
    affine: int = 0
    silu: int = 0
    vscale: float = 1.0
    family = "winograd-input"

    @property
    def id(self):
        return f"wino_in-{self.name}"


class WW(NamedTuple):
    name: str
    n: int
    c: int
    uscale: float = 1.0
    family = "winograd-weight"

    @property
    def id(self):
        return f"wino_w-{self.name}"


class WO(NamedTuple):
    name: str
    B: int
    h: int
    w: int
    n: int
    dldm: int = 0
    dldo: int = 0
    dldr: int = 0
    dldbb: int = 0
    bias: int = 0
    bias_bn: int = 0
    res: int = 0
    silu: int = 0
    mscale: float = 1.0
    cs: int = 0
    family = "winograd-output"

    @property
    def id(self):
        return f"wino_out-{self.name}"


class GW(NamedTuple):
    name: str
    mode: int
    B: int
    h: int
    w: int
    c0: int
    c1: int
    G: int
    eps: float = 1e-5
    silu: int = 1
    dldm: int = 0
    bias: int = 0
    bias_bn: int = 0
    dldbb: int = 0
    mscale: float = 1.0
    gamma_off: int = 0          # halves the gamma pointer is moved off its 16-byte alignment
    family = "gn-winograd"

    @property
    def id(self):
        return f"gn_wino-{self.name}"

    @property
    def C(self):
        return self.c0 + self.c1

    @property
    def cg(self):
        return self.C // self.G


# ---- transcript of the dispatch (sd_norm.hip / sd_winograd.hip entry points), as attention_ref.generic_instantiation is of sd_attention.hip
def groupnorm_route(c0, c1, hw, groups):
    cg = (c0 + c1) // groups
    return "gn_small_kernel" if cg % 4 == 0 and c0 % 4 == 0 and hw * (cg // 4) <= GN_SMALL_ITEMS else "partial-finalize-apply"


def layernorm_instantiation(rows, c):
    if c == 320:
        return "group<8,2>" if rows >= 32768 else "group<8,1>"
    if c == 640:
        return "group<16,2>" if rows >= 65536 else "group<16,1>"
    if c == 1280 and rows >= 16384:
        return "group<32,2>" if rows >= 32768 else "group<32,1>"
    return "row<4,1>" if c <= 512 else "row<2,2>" if c <= 1024 else "row<1,4>"


def gn_wino_vec(cg, mode, ldm, ldbb, aligned):
    return 8 if cg % 8 == 0 and (not mode or ldm % 8 == 0) and ldbb % 8 == 0 and aligned else 4


def wino_output_kernel(colstats):
    return "winograd_output_cs_kernel" if colstats else "winograd_output_kernel"


def branches(c):
    """The branches of the scope table a case reaches."""
    if isinstance(c, GN):
        out = set()
        if c.entry == "gn":
            out.add("gn:" + groupnorm_route(c.c0, c.c1, c.hw, c.G))
        elif c.entry == "table":
            out.add("table:statistics-pass")
        else:
            out.add(f"{c.entry}:slots{'32' if c.rps == 32 else 'N'}")
            per, slots = 256 // c.cg, c.hw // c.rps
            out.add("finalize_colstats:" + ("one-row-lane" if per == 1 else "row-lanes"))
            out.add("finalize_colstats:" + ("predicated-tail" if slots % (8 * per) else "full-trips"))
        return out
    if isinstance(c, LN):
        return {"ln:" + layernorm_instantiation(c.rows, c.c)}
    if isinstance(c, SM):
        return {"softmax"}
    if isinstance(c, WI):
        return {"wino_in:" + ("affine+silu" if c.silu else "affine" if c.affine else "plain"), "wino_in:up" if c.up else "wino_in:same-size",
                "wino_in:two-sources" if c.c1 else "wino_in:one-source"}
    if isinstance(c, WW):
        return {"wino_w"}
    if isinstance(c, WO):
        return {"wino_out:" + wino_output_kernel(c.cs)}
    ldbb = (c.C + c.dldbb) if c.bias_bn else c.C
    return {f"gn_wino:mode{c.mode}:VEC{gn_wino_vec(c.cg, c.mode, c.C + c.dldm, ldbb, c.gamma_off % 8 == 0)}"}


REACHABLE = ({"gn:gn_small_kernel", "gn:partial-finalize-apply", "gn_cs:slots32", "table:statistics-pass", "table_cs:slots32", "table_cs:slotsN",
              "table_cat:slots32", "finalize_colstats:one-row-lane", "finalize_colstats:row-lanes", "finalize_colstats:predicated-tail",
              "finalize_colstats:full-trips", "softmax", "wino_w", "wino_out:winograd_output_kernel", "wino_out:winograd_output_cs_kernel",
              "wino_in:plain", "wino_in:affine", "wino_in:affine+silu", "wino_in:up", "wino_in:same-size", "wino_in:two-sources",
              "wino_in:one-source"}
             | {f"ln:group<{l},{u}>" for l in (8, 16, 32) for u in (1, 2)} | {"ln:row<4,1>", "ln:row<2,2>", "ln:row<1,4>"}
             | {f"gn_wino:mode{m}:VEC{v}" for m in (0, 1) for v in (4, 8)})


def _build_cases():
    t = []
    # ---- GroupNorm, small route
    t += [GN("hw1-c8-g2", "gn", 2, 1, 8, 0, 2), GN("limit-5120-items-c2560", "gn", 1, 256, 1280, 1280, 32),
          GN("cg12-straddle", "gn", 2, 64, 8, 16, 2, silu=0), GN("small-shift", "gn", 2, 64, 64, 0, 8, dist="shift"),
          GN("small-const", "gn", 1, 16, 32, 0, 4, dist="const"), GN("small-eps1e-6", "gn", 2, 9, 16, 8, 3, eps=1e-6)]
    # ---- GroupNorm, three launches
    t += [GN("hw257-c2560", "gn", 1, 257, 1280, 1280, 32), GN("hw1-cg6", "gn", 2, 1, 24, 0, 4), GN("hw65-c320", "gn", 2, 65, 320, 0, 32),
          GN("hw127-c320", "gn", 1, 127, 320, 0, 32, silu=0), GN("cg1", "gn", 2, 70, 32, 0, 32), GN("g1-c2056", "gn", 1, 64, 2056, 0, 1),
          GN("c2048-hw13", "gn", 1, 13, 2048, 0, 1), GN("c2048-hw14", "gn", 2, 14, 1024, 1024, 1, silu=0), GN("c2048-hw15", "gn", 1, 15, 2048, 0, 1, eps=1e-6),
          GN("two-sources-c0-ne-c1", "gn", 2, 130, 40, 104, 16), GN("three-shift", "gn", 2, 200, 160, 0, 32, dist="shift"),
          GN("three-const", "gn", 2, 100, 40, 0, 4, dist="const")]
    # ---- the column-sum finalize through its three entry points: cg 1, 10, 80, 136, 256; slots 1, 8 per, 8 per + 1; rows_per_slot 32, 64, 256
    t += [GN("cg1-1slot", "gn_cs", 2, 32, 32, 0, 32), GN("cg10-tail", "gn_cs", 2, 32 * (8 * 25 + 1), 320, 0, 32),
          GN("cg80-full", "gn_cs", 2, 32 * 24, 1280, 1280, 32, silu=0), GN("cg80-tail", "gn_cs", 1, 32 * 25, 2560, 0, 32),
          GN("cg136-one-lane", "gn_cs", 2, 32 * 9, 136, 136, 2), GN("cg256-one-lane", "gn_cs", 1, 32 * 8, 512, 0, 2, eps=1e-6),
          GN("c8-c24-g2", "gn_cs", 2, 32, 8, 24, 2),
          GN("cg10-rps32", "table_cs", 2, 32 * 200, 320, 0, 32), GN("cg80-rps64", "table_cs", 2, 64 * 25, 2560, 0, 32, rps=64),
          GN("cg16-rps256", "table_cs", 2, 256 * 3, 512, 0, 32, rps=256), GN("cg256-rps64-tail", "table_cs", 1, 64 * 9, 256, 0, 1, rps=64),
          GN("cg1-hw32", "table_cs", 1, 32, 8, 0, 8),
          GN("c8-c24-g2", "table_cat", 2, 32, 8, 24, 2), GN("cg80-tail", "table_cat", 2, 32 * 25, 640, 1920, 32), GN("cg136", "table_cat", 1, 64, 136, 136, 2),
          GN("one-source", "table_cat", 2, 32 * 8, 64, 0, 32),
          GN("hw65-c320", "table", 2, 65, 320, 0, 32), GN("hw257-c2560", "table", 1, 257, 2560, 0, 32), GN("hw1-cg6", "table", 2, 1, 24, 0, 4),
          GN("cg256-c2304", "table", 1, 64, 2304, 0, 9, eps=1e-6)]
    # ---- LayerNorm: every instantiation at 1 row, one short of a block and one over; both sides of every row threshold
    for c, blk in ((8, 16), (512, 16), (520, 8), (1024, 8), (1032, 4), (2048, 4), (320, 32), (640, 16)):
        t += [LN(f"c{c}-rows{r}", r, c, 1e-6 if c == 520 else 1e-5) for r in (1, blk - 1, blk + 1)]
    t += [LN("c1280-rows5", 5, 1280), LN("c1280-rows16383", 16383, 1280), LN("c1280-rows16385", 16385, 1280), LN("c1280-rows16391", 16391, 1280),
          LN("c1280-rows32767", 32767, 1280), LN("c1280-rows32783", 32768 + 15, 1280), LN("c1280-rows32785", 32768 + 17, 1280),
          LN("c320-rows32767", 32767, 320), LN("c320-rows32768", 32768, 320), LN("c320-rows32831", 32768 + 63, 320), LN("c320-rows32833", 32768 + 65, 320),
          LN("c640-rows65535", 65535, 640), LN("c640-rows65567", 65536 + 31, 640), LN("c640-rows65569", 65536 + 33, 640)]
    # ---- softmax
    for n in (1, 7, 255, 256, 257, 1000):
        t += [SM(f"n{n}", 3, n, 0, 1.0), SM(f"n{n}-ld+3", 2, n, 3, 0.125)]
    t += [SM("negative-scale", 3, 300, 3, -0.7), SM("equal-row", 2, 257, 0, 2.0, "equal"), SM("underflow", 2, 600, 3, 1.0, "underflow")]
    # ---- Winograd input
    t += [WI("2x2", 1, 2, 2, 8), WI("2x6", 2, 2, 6, 16, vscale=0.25), WI("4x2", 3, 4, 2, 8, 24), WI("up-4x2", 2, 4, 2, 16, 8, up=1),
          WI("affine", 2, 4, 6, 8, 16, affine=1), WI("affine-silu", 2, 6, 4, 24, 0, affine=1, silu=1, vscale=0.25),
          WI("up-affine-silu", 1, 8, 4, 8, 8, up=1, affine=1, silu=1), WI("threads-not-256", 3, 10, 6, 40)]
    t += [WW("n1-c1", 1, 1), WW("n3-c5", 3, 5, 0.25), WW("n128-c64", 128, 64, 0.25)]
    # ---- Winograd output: every subset of {bias, bias_bn, res, silu}; n = 8 and 24 with every leading dimension larger than n
    for k in range(16):
        b, bb, r, s = k & 1, (k >> 1) & 1, (k >> 2) & 1, (k >> 3) & 1
        n = 24 if k % 3 == 0 else 8
        t.append(WO(f"n{n}" + ("-bias" if b else "") + ("-bb" if bb else "") + ("-res" if r else "") + ("-silu" if s else "") + ("-ld" if k % 2 else ""),
                    2, 4 if k % 4 else 2, 6 if k % 5 else 2, n, dldm=8 * (k % 2), dldo=16 * (k % 2), dldr=8 * (k % 2), dldbb=24 * (k % 2),
                    bias=b, bias_bn=bb, res=r, silu=s, mscale=16.0 if k in (5, 15) else 1.0))
    t += [WO("cs-b2-h2-n128", 2, 2, 32, 128, cs=1), WO("cs-h4-n256-all", 1, 4, 32, 256, dldm=8, dldo=8, dldr=16, dldbb=8, bias=1, bias_bn=1, res=1, silu=1,
                                                     mscale=4.0, cs=1)]
    # ---- GroupNorm + Winograd input in one launch
    t += [GW("m0-cg8", 0, 2, 4, 6, 16, 16, 4), GW("m0-cg4", 0, 2, 2, 6, 8, 0, 2), GW("m0-cg12", 0, 2, 4, 4, 8, 16, 2, silu=0),
          GW("m0-cg60", 0, 1, 6, 4, 120, 0, 2, eps=1e-6), GW("m0-cg8-gamma+4", 0, 2, 4, 4, 32, 32, 8, gamma_off=4),
          GW("m0-slice-20480", 0, 1, 16, 16, 1280, 1280, 32), GW("m0-2x6", 0, 2, 2, 6, 64, 0, 8),
          GW("m1-cg8", 1, 2, 4, 6, 32, 0, 4, bias=1, bias_bn=1, dldbb=8, mscale=16.0), GW("m1-cg8-plain", 1, 1, 2, 2, 16, 0, 2),
          GW("m1-ldm+4", 1, 2, 4, 4, 32, 0, 4, dldm=4, bias=1), GW("m1-cg12", 1, 2, 2, 6, 24, 0, 2, bias_bn=1, dldbb=4, silu=0),
          GW("m1-cg60", 1, 2, 4, 4, 120, 0, 2, bias=1, bias_bn=1, dldbb=16, mscale=4.0), GW("m1-cg8-gamma+4", 1, 2, 4, 4, 32, 0, 4, bias=1, gamma_off=4),
          GW("m1-slice-20480", 1, 1, 16, 16, 2560, 0, 32, bias=1, bias_bn=1, mscale=16.0)]
    return tuple(t)


CASES = _build_cases()


# ------------------------------------------------------------------------------------------------------------------ operands
def gn_stats_floats(c: GN):
    """the documented size of `stats`: the affine table, then the partial sums"""
    return c.B * c.C * 2 + c.B * -(-c.hw // 64) * c.G * 2


def _colsums(x, rps):
    """fp32 [slots][2][cw] of fp16 x [rows, cw]: float64 sums per slot rounded to fp32 -- the exact input of every column-sum consumer here"""
    x = x.to(F64).view(-1, rps, x.shape[-1])
    return torch.stack([x.sum(1), (x * x).sum(1)], 1).to(F32)


@functools.lru_cache(maxsize=2)
def inputs(c):
    """name -> Operand of everything the launch reads (and `x` of softmax, which it also writes)"""
    g = gen(c.id)
    if isinstance(c, GN):
        if c.dist == "const":
            x = torch.full((c.B * c.hw, c.C), 3.0, dtype=F16)
        else:
            x = randn16(g, c.B * c.hw, c.C, scale=0.25 if c.dist == "shift" else 1.0, shift=8.0 if c.dist == "shift" else 0.0)
        d = dict(gamma=Operand(randn16(g, 1, c.C, shift=1.0, scale=0.5), c.C), beta=Operand(randn16(g, 1, c.C), c.C))
        if c.entry != "table_cat":
            d["x0"] = Operand(x[:, :c.c0].contiguous(), c.c0)
            if c.c1:
                d["x1"] = Operand(x[:, c.c0:].contiguous(), c.c1)
        if c.entry in ("gn_cs", "table_cs", "table_cat"):
            d["colstats0"] = Operand(_colsums(x[:, :c.c0], c.rps).view(-1, c.c0), c.c0)
            if c.c1:
                d["colstats1"] = Operand(_colsums(x[:, c.c0:], c.rps).view(-1, c.c1), c.c1)
        return d
    if isinstance(c, LN):
        base = randn16(g, min(c.rows, 2048), c.c) * randn16(g, min(c.rows, 2048), 1, shift=1.5, scale=0.5) + randn16(g, min(c.rows, 2048), 1)
        x = base.repeat(-(-c.rows // base.shape[0]), 1)[:c.rows].contiguous()
        return dict(x=Operand(x, c.c), gamma=Operand(randn16(g, 1, c.c, shift=1.0, scale=0.5), c.c), beta=Operand(randn16(g, 1, c.c), c.c))
    if isinstance(c, SM):
        x = randn16(g, c.rows, c.n, scale=2.0)
        if c.kind == "equal":
            x = x[:, :1].repeat(1, c.n)
        if c.kind == "underflow":
            x = -(200 + 100 * torch.rand(c.rows, c.n, generator=g)).to(F16)
            x[torch.arange(c.rows), (100 + torch.arange(c.rows) * 7) % c.n] = 0        # the maximum sits outside the first wave's elements
        return dict(x=Operand(x, c.n + c.dld))
    if isinstance(c, WI):
        hs, ws, C = c.h >> c.up, c.w >> c.up, c.c0 + c.c1
        x = randn16(g, c.B * hs * ws, C)
        d = dict(x0=Operand(x[:, :c.c0].contiguous(), c.c0))
        if c.c1:
            d["x1"] = Operand(x[:, c.c0:].contiguous(), c.c1)
        if c.affine:
            tab = torch.stack([torch.randn(c.B * C, generator=g) * 0.5 + 1.0, torch.randn(c.B * C, generator=g)], 1).to(F32)
            d["gn_affine"] = Operand(tab, 2)
        return d
    if isinstance(c, WW):
        return dict(w=Operand(randn16(g, c.n * 9, c.c, scale=0.2), c.c))
    if isinstance(c, WO):
        T = c.B * (c.h // 2) * (c.w // 2)
        d = dict(m=Operand(randn16(g, 16 * T, c.n, scale=1.0 / c.mscale), c.n + c.dldm))
        if c.bias:
            d["bias"] = Operand(randn16(g, 1, c.n), c.n)
        if c.bias_bn:
            d["bias_bn"] = Operand(randn16(g, c.B, c.n), c.n + c.dldbb)
        if c.res:
            d["res"] = Operand(randn16(g, c.B * c.h * c.w, c.n), c.n + c.dldr)
        return d
    C, hw = c.C, c.h * c.w
    d = dict(gamma=Operand(randn16(g, 1, C, shift=1.0, scale=0.5), C, c.gamma_off), beta=Operand(randn16(g, 1, C), C))
    if c.mode == 0:
        x = randn16(g, c.B * hw, C, shift=0.5)
        d["x0"] = Operand(x[:, :c.c0].contiguous(), c.c0)
        if c.c1:
            d["x1"] = Operand(x[:, c.c0:].contiguous(), c.c1)
    else:
        d["m"] = Operand(randn16(g, 16 * c.B * hw // 4, C, scale=1.0 / c.mscale), C + c.dldm)
        if c.bias:
            d["bias"] = Operand(randn16(g, 1, C), C)
        if c.bias_bn:
            d["bias_bn"] = Operand(randn16(g, c.B, C), C + c.dldbb)
    return d


def outputs(c):
    """name -> Out of everything the launch writes"""
    if isinstance(c, GN):
        d = {}
        if c.entry in ("gn", "gn_cs"):
            d["out"] = Out(c.B * c.hw, c.C, c.C, F16)
        table = c.B * c.C * 2
        # the table in `stats`: written by every route but gn_small_kernel (sd_hip.h: unspecified after sd_groupnorm_f16)
        d["stats"] = Out(1, gn_stats_floats(c), gn_stats_floats(c), F32, must=0 if c.entry == "gn" else table)
        return d
    if isinstance(c, LN):
        return dict(out=Out(c.rows, c.c, c.c, F16))
    if isinstance(c, SM):
        return dict(x=Out(c.rows, c.n, c.n + c.dld, F16))
    if isinstance(c, WI):
        return dict(v=Out(16 * c.B * (c.h // 2) * (c.w // 2), c.c0 + c.c1, c.c0 + c.c1, F16))
    if isinstance(c, WW):
        return dict(u=Out(16 * c.n, c.c, c.c, F16))
    if isinstance(c, WO):
        d = dict(out=Out(c.B * c.h * c.w, c.n, c.n + c.dldo, F16))
        if c.cs:
            d["colstats"] = Out(c.B * c.h * c.w // 32 * 2, c.n, c.n, F32)
        return d
    return dict(v=Out(16 * c.B * c.h * c.w // 4, c.C, c.C, F16))


def launch(ops, c, p):
    """The launch of a case through coma_amd.sd.ops; p: name -> device tensor starting at the operand's / output's first element."""
    g = p.get
    if isinstance(c, GN):
        kw = dict(batch=c.B, hw=c.hw, c0=c.c0, groups=c.G, eps=c.eps)
        if c.entry == "gn":
            return ops.groupnorm(p["x0"], p["gamma"], p["beta"], p["out"], p["stats"], x1=g("x1"), c1=c.c1, silu=bool(c.silu), **kw)
        if c.entry == "gn_cs":
            return ops.groupnorm_colstats(p["x0"], p["gamma"], p["beta"], p["out"], p["stats"], p["colstats0"], x1=g("x1"), c1=c.c1,
                                          colstats1=g("colstats1"), silu=bool(c.silu), **kw)
        if c.entry == "table_cat":
            return ops.groupnorm_table_cat(p["gamma"], p["beta"], p["stats"], p["colstats0"], g("colstats1"), c1=c.c1, **kw)
        return ops.groupnorm_table(p["x0"], p["gamma"], p["beta"], p["stats"], colstats0=g("colstats0"), rows_per_slot=c.rps, **kw)
    if isinstance(c, LN):
        return ops.layernorm(p["x"], p["gamma"], p["beta"], p["out"], rows=c.rows, c=c.c, eps=c.eps)
    if isinstance(c, SM):
        return ops.softmax_(p["x"], rows=c.rows, n=c.n, ld=c.n + c.dld, scale=c.scale)
    if isinstance(c, WI):
        return ops.winograd_input(p["x0"], p["v"], batch=c.B, h=c.h, w=c.w, c0=c.c0, x1=g("x1"), c1=c.c1, upsample=bool(c.up),
                                  gn_affine=g("gn_affine"), silu=bool(c.silu), vscale=c.vscale)
    if isinstance(c, WW):
        return ops.winograd_weight(p["w"], p["u"], n=c.n, c=c.c, uscale=c.uscale)
    if isinstance(c, WO):
        return ops.winograd_output(p["m"], p["out"], batch=c.B, h=c.h, w=c.w, n=c.n, ldm=c.n + c.dldm, bias=g("bias"), bias_bn=g("bias_bn"),
                                   ldbb=(c.n + c.dldbb) if c.bias_bn else 0, res=g("res"), ldr=(c.n + c.dldr) if c.res else 0, ldo=c.n + c.dldo,
                                   silu=bool(c.silu), colstats=g("colstats"), mscale=c.mscale)
    return ops.gn_winograd_input(p["v"], p["gamma"], p["beta"], batch=c.B, h=c.h, w=c.w, c0=c.c0, x0=g("x0"), x1=g("x1"), c1=c.c1, m=g("m"),
                                 ldm=c.C + c.dldm, bias=g("bias"), bias_bn=g("bias_bn"), ldbb=(c.C + c.dldbb) if c.bias_bn else 0, groups=c.G,
                                 eps=c.eps, silu=bool(c.silu), mscale=c.mscale)


# ------------------------------------------------------------------------------------------------------------------ arithmetic
class Result(NamedTuple):
    ref: torch.Tensor           # float64 [rows, width]
    emu: torch.Tensor           # the emulation in the output's stored type
    stated: torch.Tensor        # a-priori bound of |emu - ref|, element by element (for fp32 tables also the DEVICE's bound: it holds for
                                # every summation order)


def final16(ref, err):
    """a-priori bound after the last fp16 rounding: `err` bounds the fp32 value to first order, 1.002 covers what first order leaves out
    (the rounding acts on the computed value: 2^-11 err; each 2^-24 acts on a computed partial), 2^-25 = half the fp16 subnormal spacing"""
    return 1.002 * err + 2.0 ** -11 * ref.abs() + 2.0 ** -25


def _gn_sums(c, terms):
    """terms [B, G, n] -> (float64 sum, sum of magnitudes, fp32 sum in index order)"""
    t64 = terms.to(F64)
    return t64.sum(-1), t64.abs().sum(-1), sum32(terms).to(F64)


def gn_statistics(c, d, x=None, e_x=None):
    """Per (sample, group): the GroupNorm statistics of a case as float64 (exact from the exact inputs) and as the emulation's fp32 one-pass
    values, with the a-priori bounds (es, eq) of |fp32 sum - exact sum| for ANY summation order: an n-term sum passes each term through at
    most n - 1 additions, each rounding its partial sum by 2^-24 -> (n - 1) 2^-24 sum |term|.
    Sources: the column sums (entries gn_cs, table_cs, table_cat: the fp32 sums are the exact input; a group adds slots x cg of them) or the
    tensor x [B * hw, C] (hw x cg terms; e_x: a bound of the emulation's own deviation in x, for the fused kernel's mode 1)."""
    B, G, cg, hw = c.B, c.G, c.cg, (c.hw if isinstance(c, GN) else c.h * c.w)
    if isinstance(c, GN) and c.entry in ("gn_cs", "table_cs", "table_cat"):
        cs = torch.cat([d[k].t.view(B, -1, 2, d[k].t.shape[-1]) for k in ("colstats0", "colstats1") if k in d], -1)      # [B, slots, 2, C]
        ts = cs[:, :, 0].reshape(B, -1, G, cg).permute(0, 2, 1, 3).reshape(B, G, -1)
        tq = cs[:, :, 1].reshape(B, -1, G, cg).permute(0, 2, 1, 3).reshape(B, G, -1)
        es_in = eq_in = 0.0
    else:
        xs = x.view(B, hw, G, cg).permute(0, 2, 1, 3).reshape(B, G, -1)
        ts, tq = xs.to(F32), xs.to(F32) ** 2                                          # the square of an fp16 value is exact in fp32
        es_in = 0.0 if e_x is None else e_x.view(B, hw, G, cg).permute(0, 2, 1, 3).reshape(B, G, -1).sum(-1)
        eq_in = 0.0 if e_x is None else ((2 * x.to(F64).abs() + e_x) * e_x).view(B, hw, G, cg).permute(0, 2, 1, 3).reshape(B, G, -1).sum(-1)
    n = ts.shape[-1]
    s, s1, s32 = _gn_sums(c, ts)
    q, q1, q32 = _gn_sums(c, tq)
    return dict(s=s, q=q, s32=s32.to(F32), q32=q32.to(F32), es=(n - 1) * U32 * s1 + es_in, eq=(n - 1) * U32 * q1 + eq_in, count=float(hw) * cg)


def gn_affine(c, st, gamma, beta):
    """The affine table y = x scale + shift of a GroupNorm, per (sample, channel): float64, the fp32 emulation, and the a-priori bound of an
    fp32 evaluation by counting roundings (u = 2^-24; a division / rsqrt is allowed 4 u):
        mean  = s / count                      em  = es / count + 4 u |mean|
        var   = max(q / count - mean^2, 0)     ev  = eq / count + 4 u q / count + (2 |mean| + em) em + 2 u mean^2 + u |q / count - mean^2|
        rstd  = rsqrt(var + eps)               the interval [var + eps - et, var + eps + et], et = ev + u (var + eps), clipped below at
                                               eps (1 - 2 u) as the clamp guarantees, mapped through rsqrt, + 4 u
        scale = rstd gamma                     e_sc = |gamma| e_rstd + u |scale|
        shift = beta - mean scale              e_sh = |scale| em + |mean| e_sc + em e_sc, + u of the product and of the difference
    -> (scale, shift, scale32, shift32, e_sc, e_sh), each [B, C]"""
    G, cg, cnt = c.G, c.cg, st["count"]
    ga, be = gamma.to(F64).view(1, G, cg), beta.to(F64).view(1, G, cg)
    mean = st["s"] / cnt
    qc = st["q"] / cnt
    var = (qc - mean * mean).clamp(min=0)
    rstd = (var + c.eps) ** -0.5
    em = st["es"] / cnt + UD * mean.abs()
    ev = st["eq"] / cnt + UD * qc + (2 * mean.abs() + em) * em + 2 * U32 * mean * mean + U32 * (qc - mean * mean).abs()
    t = var + c.eps
    et = ev + U32 * t
    hi = (t - et).clamp(min=c.eps * (1 - 2 * U32)) ** -0.5
    lo = (t + et) ** -0.5
    e_rstd = torch.maximum(hi - rstd, rstd - lo) + UD * hi
    sc = rstd[..., None] * ga
    sh = be - mean[..., None] * sc
    e_sc = ga.abs() * e_rstd[..., None] + U32 * (sc.abs() + ga.abs() * e_rstd[..., None])
    e_prod = sc.abs() * em[..., None] + mean.abs()[..., None] * e_sc + em[..., None] * e_sc
    e_prod = e_prod + U32 * ((mean[..., None] * sc).abs() + e_prod)
    e_sh = e_prod + U32 * (sh.abs() + e_prod)
    # the emulation: fp32, every operation rounded once
    cnt32 = torch.tensor(cnt, dtype=F32)
    mean32 = st["s32"] / cnt32
    var32 = (st["q32"] / cnt32 - mean32 * mean32).clamp(min=0)
    rstd32 = ((var32 + torch.tensor(c.eps, dtype=F32)).to(F64) ** -0.5).to(F32)
    sc32 = rstd32[..., None] * ga.to(F32)
    sh32 = be.to(F32) - mean32[..., None] * sc32
    B = sc.shape[0]
    return tuple(v.reshape(B, -1) for v in (sc, sh, sc32, sh32, e_sc, e_sh))


def gn_apply(c, x, aff, silu, e_x=None):
    """y = act(x scale + shift) per pixel: float64, the emulation (one fma, SiLU with an exact exp, fp32) and the a-priori bound before the
    final rounding: |x| e_sc + e_sh (+ |scale| e_x) + u |y| for the fma; through SiLU the Lipschitz constant 1.1, + 8 u |f| for its own
    arithmetic.  x [B * hw, C] fp16."""
    sc, sh, sc32, sh32, e_sc, e_sh = aff
    B, C = sc.shape
    x64 = x.to(F64).view(B, -1, C)
    y = x64 * sc[:, None] + sh[:, None]
    err = x64.abs() * e_sc[:, None] + e_sh[:, None]
    if e_x is not None:
        err = err + (sc.abs() + e_sc)[:, None] * e_x.view(B, -1, C)
    err = err + U32 * (y.abs() + err)
    y32 = (x64 * sc32.to(F64)[:, None] + sh32.to(F64)[:, None]).to(F32)                # fmaf: one rounding
    if silu:
        y, y32 = kit.silu(y), kit.silu(y32)
        err = LIP * err + 8 * U32 * y.abs()
    return y.view(-1, C), y32.view(-1, C), err.view(-1, C)


def cat(d):
    return torch.cat([d[k].t for k in ("x0", "x1") if k in d], -1)


def _patches(img):
    """img [B, h, w, C] -> the 4 x 4 input patch of every 2 x 2 output tile, zero padding 1: [B, h/2, w/2, C, 4, 4]"""
    B, h, w, C = img.shape
    pad = torch.zeros(B, h + 2, w + 2, C, dtype=img.dtype)
    pad[:, 1:-1, 1:-1] = img
    return pad.unfold(1, 4, 2).unfold(2, 4, 2)


def wino_input(img, vscale=1.0, e_img=None):
    """V[4 i + j][tile][c] = vscale (B^T d B)[i, j] -> (float64 [16 T, C], the fp32 emulation in the kernel's order -- columns first, rounded
    to fp16 --, a-priori bound: two levels of fp32 additions and the scale, 4 u |B^T| |d| |B|; + |B^T| e_img |B| for a deviation of the
    emulation's own input)."""
    B, h, w, C = img.shape
    P = _patches(img.to(F64))
    V = vscale * torch.einsum("ik,btxckl,jl->ijbtxc", BT, P, BT).reshape(16 * B * (h // 2) * (w // 2), C)
    A = torch.einsum("ik,btxckl,jl->ijbtxc", BT.abs(), P.abs(), BT.abs()).reshape(V.shape)
    err = 4 * U32 * vscale * A
    if e_img is not None:
        err = err + vscale * torch.einsum("ik,btxckl,jl->ijbtxc", BT.abs(), _patches(e_img), BT.abs()).reshape(V.shape)
    return V, A, err


def wino_input32(img, vscale=1.0):
    d = _patches(img.to(F32))                                                          # [..., i, j]
    d0, d1, d2, d3 = d.unbind(-2)
    t = torch.stack([d0 - d2, d1 + d2, d2 - d1, d1 - d3], -2)
    t0, t1, t2, t3 = t.unbind(-1)
    vs = torch.tensor(vscale, dtype=F32)
    V = torch.stack([vs * (t0 - t2), vs * (t1 + t2), vs * (t2 - t1), vs * (t1 - t3)], -1)                                # [B, th, tw, C, i, j]
    B, th, tw, C = V.shape[:4]
    return V.permute(4, 5, 0, 1, 2, 3).reshape(16 * B * th * tw, C).to(F16)


def wino_output(m, B, h, w, mscale, bias, bias_bn, res, silu):
    """out[b, 2 ty + a, 2 tx + bb] = act(mscale (A^T m A)[a, bb] + bias + bias_bn[b]) + res, m [16 T, n] fp16 ->
    (float64 [B h w, n], fp32 emulation before the final rounding, a-priori bound before the final rounding: 8 u over the magnitudes of
    the nine-term sum, its scale and the bias additions; 1.1 through SiLU + 8 u |f|; u per residual addition)."""
    th, tw, n = h // 2, w // 2, m.shape[-1]
    M = m.view(4, 4, B, th, tw, n)
    M64 = M.to(F64)
    Y = mscale * torch.einsum("ai,ijbtxn,cj->btaxcn", AT, M64, AT)                      # [B, th, a, tw, bb, n]
    mag = mscale * torch.einsum("ai,ijbtxn,cj->btaxcn", AT.abs(), M64.abs(), AT.abs())
    M32 = M.to(F32)
    s0 = (M32[0] + M32[1]) + M32[2]                                                     # [j, B, th, tw, n]
    s1 = (M32[1] - M32[2]) - M32[3]
    ms = torch.tensor(mscale, dtype=F32)
    rows = []
    for s in (s0, s1):
        rows.append(torch.stack([ms * ((s[0] + s[1]) + s[2]), ms * ((s[1] - s[2]) - s[3])], -2))                      # [B, th, tw, bb, n]
    Y32 = torch.stack(rows, 2)                                                          # [B, th, a, tw, bb, n]
    add64, add32 = torch.zeros(B, 1, 1, 1, 1, n, dtype=F64), torch.zeros(B, 1, 1, 1, 1, n, dtype=F32)
    for t in (bias, bias_bn):
        if t is not None:
            tv = t.view(-1, 1, 1, 1, 1, n)
            add64, add32 = add64 + tv.to(F64), add32 + tv.to(F32)
            mag = mag + tv.to(F64).abs()
    y, y32 = Y + add64, Y32 + add32
    err = 8 * U32 * mag
    if silu:
        y, y32 = kit.silu(y), kit.silu(y32)
        err = LIP * err + 8 * U32 * y.abs()
    y, y32, err = (v.reshape(B * h * w, n) for v in (y, y32, err))
    if res is not None:
        err = err + U32 * (y.abs() + res.to(F64).abs() + err)
        y, y32 = y + res.to(F64), y32 + res.to(F32)
    return y, y32, err


def ulp16(v):
    """a bound of the distance between the fp16 roundings of two values near v that straddle a rounding boundary: one fp16 ulp"""
    return 2.0 ** -10 * v.abs() + 2.0 ** -24


@functools.lru_cache(maxsize=2)
def results(c):
    """output name -> Result"""
    d = inputs(c)
    if isinstance(c, GN):
        x = None if c.entry == "table_cat" else cat(d) if c.entry != "table_cs" and c.entry != "table" else d["x0"].t
        st = gn_statistics(c, d, x)
        aff = gn_affine(c, st, d["gamma"].t, d["beta"].t)
        sc, sh, sc32, sh32, e_sc, e_sh = aff
        out = {}
        if c.entry in ("gn", "gn_cs"):
            y, y32, err = gn_apply(c, x, aff, c.silu)
            out["out"] = Result(y, y32.to(F16), final16(y, err))
        else:
            tab = lambda a, b: torch.stack([a, b], -1).reshape(-1, 2)
            out["stats"] = Result(tab(sc, sh), tab(sc32, sh32), 1.002 * tab(e_sc, e_sh) + 2.0 ** -126)
        return out
    if isinstance(c, LN):
        return dict(out=layernorm(d["x"].t, d["gamma"].t, d["beta"].t, c.eps))
    if isinstance(c, SM):
        return dict(x=softmax(d["x"].t, c.scale))
    if isinstance(c, WI):
        hs, ws, C = c.h >> c.up, c.w >> c.up, c.c0 + c.c1
        x, e_img = cat(d), None
        img = x.view(c.B, hs, ws, C)
        img32 = img
        if c.affine:                                            # storage point: the activated tensor is rounded to fp16 before the transform
            tab = d["gn_affine"].t.view(c.B, C, 2)
            x64 = img.to(F64)
            y = x64 * tab[:, None, None, :, 0].to(F64) + tab[:, None, None, :, 1].to(F64)
            y32 = y.to(F32)                                     # fmaf of exact inputs: the float64 value rounded once
            e = U32 * y.abs()
            if c.silu:
                y, y32, e = kit.silu(y), kit.silu(y32), LIP * e + 8 * U32 * kit.silu(y).abs()
            img, img32 = y.to(F16), y32.to(F16)
            e_img = ulp16(y)                                   # the two roundings differ by at most one fp16 ulp
        if c.up:
            rep = lambda t: None if t is None else t.repeat_interleave(2, 1).repeat_interleave(2, 2)
            img, img32, e_img = rep(img), rep(img32), rep(e_img)
        V, _, err = wino_input(img, c.vscale, e_img)
        return dict(v=Result(V, wino_input32(img32, c.vscale), final16(V, err)))
    if isinstance(c, WW):
        g = d["w"].t.view(c.n, 3, 3, c.c)
        U = c.uscale * torch.einsum("ak,nklc,bl->abnc", GM, g.to(F64), GM).reshape(16 * c.n, c.c)
        mag = c.uscale * torch.einsum("ak,nklc,bl->abnc", GM.abs(), g.to(F64).abs(), GM.abs()).reshape(16 * c.n, c.c)
        g32 = g.to(F32)
        half = torch.tensor(0.5, dtype=F32)
        t = torch.stack([g32[:, 0], half * ((g32[:, 0] + g32[:, 1]) + g32[:, 2]), half * ((g32[:, 0] - g32[:, 1]) + g32[:, 2]), g32[:, 2]], 1)   # [n, a, b, c]
        us = torch.tensor(c.uscale, dtype=F32)
        u32 = torch.stack([us * t[:, :, 0], us * (half * ((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2])), us * (half * ((t[:, :, 0] - t[:, :, 1]) + t[:, :, 2])),
                           us * t[:, :, 2]], 2)                 # [n, a, b, c]
        # two levels of three-term sums: 4 roundings of partial sums bounded by |G| |g| |G^T| (the halvings and the scale are exact)
        return dict(u=Result(U, u32.permute(1, 2, 0, 3).reshape(16 * c.n, c.c).to(F16), final16(U, 4 * U32 * mag)))
    if isinstance(c, WO):
        get = lambda k: d[k].t if k in d else None
        y, y32, err = wino_output(d["m"].t, c.B, c.h, c.w, c.mscale, get("bias"), get("bias_bn"), get("res"), c.silu)
        return dict(out=Result(y, y32.to(F16), final16(y, err)))
    # ---- GroupNorm + Winograd input in one launch
    e_x = None
    if c.mode == 0:
        x = x_emu = cat(d)
    else:                                                       # storage point: mscale A^T m A + bias + bias_bn is rounded to fp16 before the statistics
        get = lambda k: d[k].t if k in d else None
        y, y32, err = wino_output(d["m"].t, c.B, c.h, c.w, c.mscale, get("bias"), get("bias_bn"), None, 0)
        x, x_emu = y.to(F16), y32.to(F16)
        e_x = torch.where(x == x_emu, torch.zeros_like(y), ulp16(y))
    st_ref = gn_statistics(c, d, x, None)
    aff_ref = gn_affine(c, st_ref, d["gamma"].t, d["beta"].t)
    aff_emu = gn_affine(c, gn_statistics(c, d, x_emu), d["gamma"].t, d["beta"].t)
    y, _, _ = gn_apply(c, x, aff_ref, c.silu)
    # the bound: the emulation's statistics see x_emu; its deviation from x enters the sums (e_x) and the apply pass
    aff_b = gn_affine(c, gn_statistics(c, d, x, e_x), d["gamma"].t, d["beta"].t)
    _, _, err = gn_apply(c, x, aff_b, c.silu, e_x)
    _, y32, _ = gn_apply(c, x_emu, aff_emu, c.silu)
    act, act32 = y.to(F16), y32.to(F16)                         # storage point: the activated tensor
    e_img = (err + ulp16(y)).view(c.B, c.h, c.w, c.C)
    V, _, verr = wino_input(act.view(c.B, c.h, c.w, c.C), 1.0, e_img)
    return dict(v=Result(V, wino_input32(act32.view(c.B, c.h, c.w, c.C)), final16(V, verr)))


def layernorm(x, gamma, beta, eps):
    """float64: (x - mean) / sqrt(var + eps) gamma + beta, var = mean (x - mean)^2.  Emulation: the two-pass form in fp32, sums in index
    order.  A-priori bound (C terms): em = (C - 1) u sum|x| / C + 4 u |mean|;  d = x - mean: ed = em + u |d|;
    q = sum d^2: eq = sum (2 |d| + ed) ed + C u sum d^2;  t = q / C + eps: et = eq / C + 5 u t;  rstd: 0.5 et / (t - et) + 4 u relative;
    y = d rstd gamma + beta: |gamma| (rstd ed + |d| e_rstd) + 3 u (|d rstd gamma| + |y|)."""
    C = x.shape[-1]
    x64, ga, be = x.to(F64), gamma.to(F64), beta.to(F64)
    mean = x64.mean(-1, keepdim=True)
    dd = x64 - mean
    q = (dd * dd).sum(-1, keepdim=True)
    t = q / C + eps
    rstd = t ** -0.5
    y = dd * rstd * ga + be
    em = (C - 1) * U32 * x64.abs().sum(-1, keepdim=True) / C + UD * mean.abs()
    ed = em + U32 * dd.abs()
    eq = ((2 * dd.abs() + ed) * ed).sum(-1, keepdim=True) + C * U32 * q
    et = eq / C + 5 * U32 * t
    e_rstd = rstd * (0.5 * et / (t - et) + UD)
    err = ga.abs() * (rstd * ed + dd.abs() * e_rstd) + 3 * U32 * ((dd * rstd * ga).abs() + y.abs())
    x32, C32 = x.to(F32), torch.tensor(float(C), dtype=F32)
    mean32 = (sum32(x32) / C32)[:, None]
    d32 = x32 - mean32
    var32 = sum32(d32 * d32) / C32
    rstd32 = ((var32 + torch.tensor(eps, dtype=F32)).to(F64) ** -0.5).to(F32)[:, None]
    y32 = d32 * rstd32 * gamma.to(F32) + beta.to(F32)
    return Result(y, y32.to(F16), final16(y, err))


def softmax(x, scale):
    """float64 softmax(scale x) per row.  Emulation: t = fl(x scale), the row maximum, e = exp(t - max) (exact, rounded to fp32), the sum in
    index order, one reciprocal, e * inv rounded to fp16.  A-priori bound: the exponent is off by at most a = u (|t| + |max| + |t - max|), so
    e carries a + u relative; the n-term sum (n - 1) u + max_j (a_j + u); the reciprocal 4 u, the product u."""
    n = x.shape[-1]
    t = x.to(F64) * float(np.float32(scale))
    m = t.amax(-1, keepdim=True)
    e = torch.exp(t - m)
    ref = e / e.sum(-1, keepdim=True)
    a = U32 * (t.abs() + m.abs() + (t - m).abs()) + U32
    rel = a + (n - 1) * U32 + a.amax(-1, keepdim=True) + UD + U32
    t32 = x.to(F32) * torch.tensor(scale, dtype=F32)
    e32 = exp32(t32 - t32.amax(-1, keepdim=True))
    inv = (1.0 / sum32(e32).to(F64)).to(F32)[:, None]
    return Result(ref, (e32 * inv).to(F16), final16(ref, ref * rel))


class Yardstick(NamedTuple):
    e_emu: float                # fp16 outputs: the emulation's largest row error
    bound: float                # max(4 e_emu, 2^-10)
    emu_over_stated: float      # max over every output's elements of |emulation - ref| / a-priori bound (must be <= 1)


SUBSET_ABOVE = 1 << 24           # elements of an output above which only compared_rows() are put to the float64 reference


def compared_rows(c):
    """LayerNorm's large cases: the first and last 300 rows (the ragged last blocks and what the clamped loads of the last wave touch)
    and 256 random ones; everything else is compared whole.  (b), (c) and (d) always cover the whole output."""
    if isinstance(c, LN) and c.rows * c.c > SUBSET_ABOVE:
        pick = torch.zeros(c.rows, dtype=torch.bool)
        pick[:300] = True
        pick[-300:] = True
        pick[torch.randperm(c.rows, generator=gen(c.id + "/rows"))[:256]] = True
        return torch.nonzero(pick).flatten()
    return None


@functools.lru_cache(maxsize=2)
def _results_for_yardstick(c):
    rows = compared_rows(c)
    if rows is None:
        return results(c)
    d = inputs(c)
    return dict(out=layernorm(d["x"].t[rows], d["gamma"].t, d["beta"].t, c.eps))


def yardstick(c):
    res = _results_for_yardstick(c)
    e_emu, worst = 0.0, 0.0
    for name, r in res.items():
        assert bool(torch.isfinite(r.ref).all()) and bool(torch.isfinite(r.emu.to(F64)).all()), (c.id, name)
        worst = max(worst, float(((r.emu.to(F64) - r.ref).abs() / r.stated).max()))
        if r.emu.dtype == F16:
            e_emu = max(e_emu, float(row_error(r.emu, r.ref).max()))
    return Yardstick(e_emu, device_bound(e_emu), worst)


def reference_rows(c):
    """output name -> (rows compared or None, Result)"""
    return compared_rows(c), _results_for_yardstick(c)


def colstats_expected(c: WO, out_buf):
    """float64 sums, sums of squares and sums of magnitudes per 32-row slot and column of the DEVICE's own stored output"""
    o = outputs(c)["out"]
    v = body(o, out_buf).to(F64).view(-1, 32, c.n)
    return v.sum(1), (v * v).sum(1), v.abs().sum(1)


# ------------------------------------------------------------------------------------------------------------------ refusals
OUTPUT_ARGS = {"out", "stats", "v", "u"}        # (softmax's x is written in place)

_GN = dict(x0=PTR, x1=None, c0=16, c1=0, batch=1, hw=32, groups=2, eps=1e-5, gamma=PTR, beta=PTR, silu=1, out=PTR, stats=PTR)
_WO = dict(m=PTR, ldm=8, batch=1, h=2, w=2, n=8, bias=None, bias_bn=None, ldbb=0, res=None, ldr=0, out=PTR, ldo=0, silu=0, mscale=1.0, colstats=None)
_GW = dict(x0=PTR, x1=None, c0=16, c1=0, m=None, ldm=16, bias=None, bias_bn=None, ldbb=0, batch=1, h=2, w=2, groups=2, eps=1e-5, gamma=PTR, beta=PTR,
           silu=1, mscale=1.0, v=PTR)
_GW1 = dict(_GW, x0=None, m=PTR)
_WI = dict(x0=PTR, x1=None, c0=8, c1=0, batch=1, h=2, w=2, upsample=0, gn_affine=None, silu=0, vscale=1.0, v=PTR)

# entry point -> (accepted base, [(text of the refusal, change), ...]): every condition the argument checks state
REFUSALS = {
    "sd_groupnorm_f16": (_GN, [
        ("null pointer", dict(x0=None)), ("null pointer", dict(gamma=None)), ("null pointer", dict(beta=None)), ("null pointer", dict(out=None)),
        ("null pointer", dict(stats=None)), ("x1 missing", dict(c1=16)),
        ("c0 must be positive and c1 non-negative", dict(c0=-8, c1=16, x1=PTR)), ("c0 must be positive and c1 non-negative", dict(c0=0, c1=0)),
        ("c0 must be positive and c1 non-negative", dict(c0=32, c1=-16)), ("c0 must be positive and c1 non-negative", dict(c0=0, c1=16, x1=PTR)),
        ("bad shape", dict(batch=0)), ("bad shape", dict(hw=0)), ("bad shape", dict(groups=0)), ("bad shape", dict(groups=33, c0=264)),
        ("bad shape", dict(groups=3)), ("bad shape", dict(c0=12, groups=1)), ("bad shape", dict(c0=8, c1=12, x1=PTR, groups=1)),
        ("bad shape", dict(c0=2568, groups=1))]),
    "sd_groupnorm_colstats_f16": (dict(_GN, colstats0=PTR, colstats1=None), [
        ("null pointer", dict(x0=None)), ("null pointer", dict(colstats0=None)), ("null pointer", dict(stats=None)),
        ("second source incomplete", dict(c1=16)), ("second source incomplete", dict(c1=16, x1=PTR)),
        ("c0 must be positive and c1 non-negative", dict(c0=-8, c1=16, x1=PTR, colstats1=PTR)),
        ("c0 must be positive and c1 non-negative", dict(c0=0, c1=0)), ("c0 must be positive and c1 non-negative", dict(c0=32, c1=-16)),
        ("bad shape", dict(batch=0)), ("bad shape", dict(hw=0)), ("bad shape", dict(hw=33)), ("bad shape", dict(groups=0)),
        ("bad shape", dict(groups=33, c0=264)), ("bad shape", dict(groups=3)), ("bad shape", dict(c0=12, groups=1)),
        ("bad shape", dict(c0=8, c1=12, x1=PTR, colstats1=PTR, groups=1)),
        ("more than 256 channels per group", dict(c0=264, groups=1))]),
    "sd_groupnorm_table_f16": (dict(x0=PTR, c0=16, batch=1, hw=32, groups=2, eps=1e-5, gamma=PTR, beta=PTR, stats=PTR, colstats0=None, rows_per_slot=0), [
        ("null pointer", dict(x0=None)), ("null pointer", dict(gamma=None)), ("null pointer", dict(stats=None)),
        ("c0 must be positive", dict(c0=-32, groups=32)), ("c0 must be positive", dict(c0=0)),
        ("bad shape", dict(batch=0)), ("bad shape", dict(hw=0)), ("bad shape", dict(groups=0)), ("bad shape", dict(groups=33, c0=264)),
        ("bad shape", dict(groups=3)), ("bad shape", dict(c0=12, groups=1)), ("bad shape", dict(c0=2568, groups=32)), ("bad shape", dict(c0=264, groups=1)),
        ("colstats need hw % rows_per_slot == 0", dict(colstats0=PTR, hw=48)), ("colstats need hw % rows_per_slot == 0", dict(colstats0=PTR, rows_per_slot=16)),
        ("colstats need hw % rows_per_slot == 0", dict(colstats0=PTR, rows_per_slot=-32)), ("colstats need hw % rows_per_slot == 0", dict(colstats0=PTR, hw=64, rows_per_slot=48))]),
    "sd_groupnorm_table_cat_f16": (dict(c0=16, c1=16, batch=1, hw=32, groups=2, eps=1e-5, gamma=PTR, beta=PTR, stats=PTR, colstats0=PTR, colstats1=PTR), [
        ("null pointer", dict(gamma=None)), ("null pointer", dict(beta=None)), ("null pointer", dict(stats=None)), ("null pointer", dict(colstats0=None)),
        ("null pointer", dict(colstats1=None)), ("bad shape", dict(batch=0)), ("bad shape", dict(hw=0)), ("bad shape", dict(hw=48)),
        ("bad shape", dict(groups=0)), ("bad shape", dict(groups=33, c0=264, c1=0)), ("bad shape", dict(c0=0)), ("bad shape", dict(c0=-16, c1=48)),
        ("bad shape", dict(c1=-8, c0=24)), ("bad shape", dict(groups=3)), ("bad shape", dict(c0=12, c1=4)), ("bad shape", dict(c0=16, c1=12, groups=1)), ("bad shape", dict(c0=2560, c1=8, groups=8)),
        ("bad shape", dict(c0=264, c1=0, groups=1))]),
    "sd_layernorm_f16": (dict(x=PTR, rows=4, c=16, eps=1e-5, gamma=PTR, beta=PTR, out=PTR), [
        ("null pointer", dict(x=None)), ("null pointer", dict(gamma=None)), ("null pointer", dict(beta=None)), ("null pointer", dict(out=None)),
        ("bad shape", dict(rows=0)), ("bad shape", dict(rows=-1)), ("bad shape", dict(c=0)), ("bad shape", dict(c=12)), ("bad shape", dict(c=2056))]),
    "sd_softmax_f16": (dict(x=PTR, rows=2, n=8, ld=8, scale=1.0), [
        ("null pointer", dict(x=None)), ("bad shape", dict(rows=0)), ("bad shape", dict(n=0)), ("bad shape", dict(ld=7)),
        ("exceeds the grid limit", dict(rows=1 << 31)), ("exceeds the grid limit", dict(rows=(1 << 32) + 2))]),
    "sd_winograd_input_f16": (_WI, [
        ("upsample must be 0 or 1", dict(upsample=2)), ("null pointer", dict(x0=None)), ("null pointer", dict(v=None)),
        ("vscale must be positive", dict(vscale=0.0)), ("vscale must be positive", dict(vscale=float("nan"))),
        ("channel counts must be multiples of 8", dict(c0=0)), ("channel counts must be multiples of 8", dict(c0=12)),
        ("channel counts must be multiples of 8", dict(c1=-8)), ("channel counts must be multiples of 8", dict(c1=4, x1=PTR)),
        ("channel counts must be multiples of 8", dict(c1=8)), ("even h, w required", dict(batch=0)), ("even h, w required", dict(h=0)),
        ("even h, w required", dict(w=0)), ("even h, w required", dict(h=3)), ("even h, w required", dict(w=5)),
        ("silu needs gn_affine", dict(silu=1))]),
    "sd_winograd_weight_f16": (dict(w=PTR, n=1, c=1, uscale=1.0, u=PTR), [
        ("bad arguments", dict(w=None)), ("bad arguments", dict(u=None)), ("bad arguments", dict(n=0)), ("bad arguments", dict(c=0)),
        ("bad arguments", dict(uscale=0.0))]),
    "sd_winograd_output_f16": (_WO, [
        ("null pointer", dict(m=None)), ("null pointer", dict(out=None)), ("mscale must be positive", dict(mscale=0.0)),
        ("bad shape", dict(n=0)), ("bad shape", dict(n=12, ldm=16)), ("bad shape", dict(ldm=12)), ("bad shape", dict(batch=0)), ("bad shape", dict(h=3)),
        ("bad shape", dict(w=3)),
        ("h and w must be positive", dict(h=0)), ("h and w must be positive", dict(w=0)), ("h and w must be positive", dict(h=-2)),
        ("ldm = 8 is below n = 16", dict(n=16)), ("ldm = 0 is below", dict(ldm=0)),
        ("ldo = 4 must be", dict(ldo=4)), ("ldo = 12 must be", dict(ldo=12)), ("ldo = 8 must be", dict(n=16, ldm=16, ldo=8)),
        ("ldr = 4 must be", dict(res=PTR, ldr=4)), ("ldr = 12 must be", dict(res=PTR, ldr=12)),
        ("ldbb = 4 must be", dict(bias_bn=PTR, ldbb=4)), ("ldbb = 12 must be", dict(bias_bn=PTR, ldbb=12)),
        ("column sums need w = 32", dict(colstats=PTR)), ("column sums need w = 32", dict(colstats=PTR, w=32))]),
    "sd_gn_winograd_input_f16": (_GW, [
        ("null pointer", dict(x0=None)), ("null pointer", dict(gamma=None)), ("null pointer", dict(beta=None)), ("null pointer", dict(v=None)),
        ("mscale must be positive", dict(_GW1, mscale=0.0)), ("either NHWC sources or plane products", dict(m=PTR)),
        ("either NHWC sources or plane products", dict(_GW1, c1=16)), ("channels per group must be a multiple of 4", dict(c0=0)),
        ("channels per group must be a multiple of 4", dict(c0=6)), ("channels per group must be a multiple of 4", dict(c1=-4, c0=20)),
        ("channels per group must be a multiple of 4", dict(c1=16)), ("channels per group must be a multiple of 4", dict(c1=6, x1=PTR, groups=1)),
        ("channels per group must be a multiple of 4", dict(groups=0)),
        ("channels per group must be a multiple of 4", dict(groups=3)), ("channels per group must be a multiple of 4", dict(groups=8)),
        ("even h, w required", dict(batch=0)), ("even h, w required", dict(batch=65536)), ("even h, w required", dict(h=0)),
        ("even h, w required", dict(w=3)), ("exceeds 20480 elements", dict(h=16, w=16, c0=2688, groups=32)),
        ("ldm = 18", dict(_GW1, ldm=18)), ("ldm = 8", dict(_GW1, ldm=8)),
        ("ldbb = 8 must be", dict(_GW1, bias_bn=PTR, ldbb=8)), ("ldbb = 18 must be", dict(_GW1, bias_bn=PTR, ldbb=18))]),
}
