"""Test helper for the elementwise, mask and text kernels (coma_amd/csrc/sd_elementwise.hip, sd_text.hip): plain numpy on the CPU, nothing
here is product code and nothing here needs a GPU.

* ``CASES``       the table of launches (named tuples, one type per entry point), shared by tests/test_elementwise_ref_host.py (references,
                  emulations, coverage, refusals, mutations) and tests/test_sd_elementwise_domain_gpu.py.
* ``plan``        the buffers of a case as the kernel sees them: 256 poison elements in front of and behind every operand (NaN for floats,
                  a value whose reading changes the result for the u8 masks and the ids), NaN gap columns, outputs prefilled with a
                  sentinel and a mask of what the contract says is written.
* ``reference``   float64 (arithmetic kernels) or exact integer / bit arithmetic (everything else), each with its own index arithmetic and
                  rounded only at the storage points include/sd_hip.h names.
* ``emulate``     the kernel's formula in numpy float32 (exponentials, square roots and trigonometry through float64, rounded once): what a
                  careful fp32 kernel stores.  Its error against the float64 reference is e_emu.  ``mut`` breaks it on purpose (the
                  mutation check of the host file).
* ``check``       every assertion of a case on a set of outputs -- the device's, or the emulation's on the CPU.  Exact contracts bit for
                  bit; arithmetic results within max(4 e_emu, floor), the error normalised by the sum of magnitudes of the formula's terms.
* ``branches`` / ``REACHABLE``  what each case reaches, and everything the eleven entry points have.
* ``REFUSALS``    per entry point an accepted base and every change the argument checks refuse, with the text (tests/domain_kit.py's PTR /
                  Off; its check_refusals puts the rows to the entry points).  The guard width, the sentinels, pack_rows and bits are the
                  kit's too.

DESIGN.md section 3g has the numbers."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

from oracle import sd_oracle as so
from tests import domain_kit as kit
from tests.domain_kit import GUARD, PTR, U32, Off, bits

f16, f32, f64 = np.float16, np.float32, np.float64
SEG_GUARD, DFLT_GUARD, ID_GUARD = 255, 1, 0x7FFFFFFF
INT32_MAX = 2 ** 31 - 1
GRID_ELEMS = INT32_MAX * 256    # elements of the largest 1-D launch of 256-thread blocks

# floors of the device bound (the counted rounding of the storage format; the derivations are at `_stated`)
FLOOR_X0, FLOOR_XPREV, FLOOR_NOISE, FLOOR_TEMB, FLOOR_ATT = 12 * U32, 16 * U32, 5 * U32, 2.0 ** -12, 2.0 ** -11


def _sqrt32(v):
    return f32(np.sqrt(f64(v)))


# ------------------------------------------------------------------------------------------------------------------ conversions, by bits
def f32_to_f16_bits(x):
    """IEEE round-to-nearest-even of fp32 `x` to fp16, on the bits (no NaN in the data) -> uint16"""
    b = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.int64)
    sign, a = (b >> 16) & 0x8000, b & 0x7FFFFFFF
    e, m = (a >> 23) - 127 + 15, a & 0x7FFFFF
    # normal results: drop 13 bits
    hn, remn = (np.maximum(e, 0) << 10) | (m >> 13), m & 0x1FFF
    hn = hn + ((remn > 0x1000) | ((remn == 0x1000) & ((hn & 1) == 1)))
    # subnormal results: the implicit one comes back and 14 - e bits go
    sh = np.minimum(14 - e, 40)
    ms = m | 0x800000
    hs, rems, half = ms >> sh, ms & ((1 << sh) - 1), 1 << (sh - 1)
    hs = hs + ((rems > half) | ((rems == half) & ((hs & 1) == 1)))
    h = np.where(e >= 1, hn, np.where(a == 0, 0, hs))
    h = np.where((a >= 0x47800000) | (h > 0x7C00), 0x7C00, h)                           # 65536 and beyond, or rounded up past 65504
    return (sign | h).astype(np.uint16)


def f16_bits_to_f32(h):
    """the exact fp32 value of every fp16 bit pattern (no NaN) -> float32"""
    h = np.asarray(h).astype(np.int64)
    s, e, m = np.where(h & 0x8000, -1.0, 1.0), (h >> 10) & 31, h & 0x3FF
    v = np.where(e == 0, m * 2.0 ** -24, np.where(e == 31, np.inf, (1024 + m) * 2.0 ** (e.astype(f64) - 25)))
    return (s * v).astype(f32)


def _to16(x32):
    return f32_to_f16_bits(x32).view(f16)


# ------------------------------------------------------------------------------------------------------------------ the table
class DD(NamedTuple):
    """sd_cfg_ddim_step"""
    name: str
    B: int
    hw: int
    eps_ld: int = 4
    mode: str = "full"          # full | assemble (eps_uc NULL) | step (unet_in NULL) | no-x0 | keep-latents (write_latents = 0)
    guidance: float = 7.5
    alphas: str = "mid"         # first | mid | last (of the 50-step schedule) | prev1 | prev0 | t1
    entry = "sd_cfg_ddim_step"

    @property
    def id(self):
        return f"ddim-{self.name}"


class TE(NamedTuple):
    name: str
    B: int
    dim: int
    t: tuple
    entry = "sd_timestep_embedding_f16"

    @property
    def id(self):
        return f"temb-{self.name}"


class NC(NamedTuple):
    name: str
    B: int
    c: int
    hw: int
    cpad: int
    entry = "sd_nchw_to_nhwc_f16"

    @property
    def id(self):
        return f"to_nhwc-{self.name}"


class NH(NamedTuple):
    name: str
    B: int
    c: int
    hw: int
    ld: int
    entry = "sd_nhwc_to_nchw_f32"

    @property
    def id(self):
        return f"to_nchw-{self.name}"


class U8(NamedTuple):
    name: str
    ld: int
    round_mode: int
    entry = "sd_image_to_u8"

    @property
    def id(self):
        return f"u8-{self.name}"


class VS(NamedTuple):
    name: str
    npix: int
    ld: int
    noise: int
    outs: str                   # f32 | f16 | both
    entry = "sd_vae_sample"

    @property
    def id(self):
        return f"vae-{self.name}"


class AN(NamedTuple):
    name: str
    n: int
    alpha: float
    entry = "sd_add_noise"

    @property
    def id(self):
        return f"noise-{self.name}"


class MA(NamedTuple):
    """sd_mask_adapt_batched (single = 0), or sd_mask_adapt with a batched launch of the same image beside it (single = 1, B = 1)"""
    name: str
    B: int
    H: int
    W: int
    iters: int
    place: str                  # corners | edges | lastcol | one | empty | full | random | per-image
    segval: str = "1"           # 1 | 255 | mixed
    dval: int = 1               # value of the set pixels of the default mask (0: an empty default mask)
    thres: str = "0"            # 0 | neg | 1e9 | eq | +.5 | -.5 | split
    force: int = 0
    cpad: int = 8
    write_pad: int = 0
    single: int = 0

    @property
    def entry(self):
        return "sd_mask_adapt" if self.single else "sd_mask_adapt_batched"

    @property
    def id(self):
        return ("mask1-" if self.single else "maskB-") + self.name


class TX(NamedTuple):
    name: str
    seqs: int
    len: int
    n_pos: int
    vocab: int
    width: int
    entry = "sd_text_embed_f16"

    @property
    def id(self):
        return f"embed-{self.name}"


class CA(NamedTuple):
    name: str
    seqs: int
    heads: int
    len: int
    layout: str                 # packed | separate
    dldo: int
    sharp: int
    entry = "sd_attention_causal_f16"

    @property
    def id(self):
        return f"causal-{self.name}"


N_F16 = 2 * 31 * 1024 + 2       # every finite fp16 bit pattern and the two infinities


def _build_cases():
    t = []
    t += [DD("n1-ld4-first", 1, 1, 4, "full", 7.5, "first"), DD("n255-ld8-g0-mid", 1, 255, 8, "full", 0.0, "mid"),
          DD("n256-ld64-g1-last", 2, 128, 64, "full", 1.0, "last"), DD("n257-ld72-g11-prev1", 1, 257, 72, "full", 11.0, "prev1"),
          DD("n513-ld64-prev0", 3, 171, 64, "full", 7.5, "prev0"), DD("n256-ld8-t1", 2, 128, 8, "full", 7.5, "t1"),
          DD("n513-assemble", 3, 171, 4, "assemble"), DD("n1-assemble", 1, 1, 4, "assemble"),
          DD("n256-ld64-step", 2, 128, 64, "step", 7.5, "first"), DD("n257-ld4-no-x0", 1, 257, 4, "no-x0", 11.0, "mid"),
          DD("n513-ld72-keep-latents", 3, 171, 72, "keep-latents", 7.5, "mid"), DD("n255-ld4-keep-latents-last", 1, 255, 4, "keep-latents", 1.0, "last")]
    t += [TE("b1-dim2", 1, 2, (1000.0,)), TE("b3-dim4", 3, 4, (0.0, 1.0, 500.5)), TE("b5-dim6", 5, 6, (0.0, 981.0, 999.0, 1000.0, 500.5)),
          TE("b3-dim320", 3, 320, (0.0, 999.0, 1000.0)), TE("b1-dim1280", 1, 1280, (1000.0,)), TE("b5-dim1280", 5, 1280, (0.0, 1.0, 500.5, 981.0, 1000.0)),
          TE("b3-dim258", 3, 258, (999.0, 1000.0, 0.0))]
    shapes = [("c4-pad4-256", 1, 4, 64, 4), ("c3-pad4-256", 1, 3, 64, 4), ("c3-pad3-255", 1, 3, 85, 3), ("c4-pad64-256", 1, 4, 4, 64),
              ("c4-pad64-320", 1, 4, 5, 64), ("c9-pad9-261", 1, 9, 29, 9), ("c9-pad10", 3, 9, 9, 10), ("c9-pad64", 2, 9, 3, 64),
              ("c1-pad1-257", 1, 1, 257, 1), ("c1-pad2", 1, 1, 129, 2), ("c1-pad8", 2, 1, 17, 8), ("c4-pad8-b2-hw1", 2, 4, 1, 8),
              ("c3-pad8", 2, 3, 33, 8)]
    t += [NC(*s) for s in shapes] + [NH(*s) for s in shapes]
    t += [U8(f"ld{ld}-{'round' if r else 'trunc'}", ld, r) for ld in (3, 4, 64) for r in (0, 1)]
    t += [VS("n1-ld8-both", 1, 8, 1, "both"), VS("n63-ld16-f32", 63, 16, 1, "f32"), VS("n64-ld64-f16", 64, 64, 1, "f16"),
          VS("n65-ld8-mode-both", 65, 8, 0, "both"), VS("n257-ld16-both", 257, 16, 1, "both"), VS("n257-ld64-mode-f32", 257, 64, 0, "f32"),
          VS("n64-ld8-mode-f16", 64, 8, 0, "f16")]
    t += [AN("n1-a1", 1, 1.0), AN("n255-a0.9991", 255, 0.9991), AN("n256-a0.0047", 256, 0.0047), AN("n257-a1e-6", 257, 1e-6),
          AN("n1025-a1", 1025, 1.0), AN("n1025-a0.0047", 1025, 0.0047)]
    t += [MA("8x8-k0-corners", 1, 8, 8, 0, "corners"), MA("8x8-k1-corners-255-eq-pad16w", 1, 8, 8, 1, "corners", "255", 255, "eq", 0, 16, 1),
          MA("8x8-k8-one-pad64", 1, 8, 8, 8, "one", cpad=64), MA("8x8-k1-edges-pad8w", 1, 8, 8, 1, "edges", "mixed", 1, "0", 0, 8, 1), MA("8x136-k3-edges-mixed--.5", 1, 8, 136, 3, "edges", "mixed", 1, "-.5"),
          MA("8x136-k1-lastcol-neg", 1, 8, 136, 1, "lastcol", "1", 1, "neg"), MA("8x136-k8-one", 1, 8, 136, 8, "one", "255"),
          MA("16x264-k3-corners-+.5-pad16w", 1, 16, 264, 3, "corners", "mixed", 1, "+.5", 0, 16, 1),
          MA("16x264-k1-lastcol-255-eq", 1, 16, 264, 1, "lastcol", "255", 1, "eq"), MA("16x264-k264-one-pad64w", 1, 16, 264, 264, "one", cpad=64, write_pad=1),
          MA("24x8-k1-edges", 1, 24, 8, 1, "edges"), MA("24x8-k24-one", 1, 24, 8, 24, "one", "mixed", 255),
          MA("64x96-b3-k3-per-image-split", 3, 64, 96, 3, "per-image", "255", 1, "split"), MA("64x96-b3-k0-full-1e9", 3, 64, 96, 0, "full", "255", 1, "1e9"),
          MA("64x96-b3-k1-full-mixed-d255", 3, 64, 96, 1, "full", "mixed", 255), MA("64x96-b3-force-pad64", 3, 64, 96, 2, "random", force=1, cpad=64),
          MA("64x96-b3-k3-empty", 3, 64, 96, 3, "empty"), MA("64x96-b3-k1-random-d0", 3, 64, 96, 1, "random", "mixed", 0),
          MA("64x96-b3-k3-random-eq-pad16", 3, 64, 96, 3, "random", "mixed", 1, "eq", 0, 16, 0),
          MA("64x96-b3-k96-lastcol-pad64w", 3, 64, 96, 96, "lastcol", "1", 1, "0", 0, 64, 1)]
    t += [MA("8x8-k1-corners-pad3", 1, 8, 8, 1, "corners", cpad=3, single=1), MA("8x136-k3-lastcol-pad5", 1, 8, 136, 3, "lastcol", "255", cpad=5, single=1),
          MA("16x264-k264-one-pad8", 1, 16, 264, 264, "one", "mixed", 255, cpad=8, single=1),
          MA("24x8-k1-edges-default-pad64", 1, 24, 8, 1, "edges", "1", 1, "1e9", cpad=64, single=1),
          MA("64x96-k3-random-eq-pad3", 1, 64, 96, 3, "random", "mixed", 1, "eq", cpad=3, single=1),
          MA("16x264-k0-edges-pad5", 1, 16, 264, 0, "edges", cpad=5, single=1), MA("8x136-k8-one-pad8", 1, 8, 136, 8, "one", "255", cpad=8, single=1)]
    t += [TX("w8-len1", 1, 1, 1, 1, 8), TX("w512-len77-pos80-s3", 3, 77, 80, 300, 512), TX("w520-len77", 1, 77, 77, 300, 520),
          TX("w768-len1-pos4-s3", 3, 1, 4, 300, 768), TX("w1032-len77-pos80-vocab1", 1, 77, 80, 1, 1032), TX("w768-len77-s3", 3, 77, 77, 300, 768)]
    t += [CA("len1-h1", 1, 1, 1, "packed", 0, 0), CA("len2-h3-s2-sharp", 2, 3, 2, "separate", 3, 1), CA("len3-h1-sharp", 1, 1, 3, "separate", 0, 1),
          CA("len4-h3", 1, 3, 4, "packed", 3, 0), CA("len5-h12", 1, 12, 5, "separate", 3, 0), CA("len63-h1-s2-sharp", 2, 1, 63, "packed", 0, 1),
          CA("len64-h3-sharp", 1, 3, 64, "separate", 3, 1), CA("len65-h1", 1, 1, 65, "packed", 3, 0), CA("len127-h3-s2", 2, 3, 127, "separate", 0, 0),
          CA("len128-h12-s2-sharp", 2, 12, 128, "packed", 3, 1), CA("len128-h1", 1, 1, 128, "separate", 3, 0), CA("len77-h12-sharp", 1, 12, 77, "packed", 0, 1)]
    return tuple(t)


CASES = _build_cases()


def _blocks(n):
    return {"one-block" if n <= 256 else "blocks", "ragged" if n % 256 else "exact-256"}


def branches(c):
    """What a case reaches, as entry:feature"""
    if isinstance(c, DD):
        return {f"ddim:{c.mode}", f"ddim:alphas-{c.alphas}"} | {"ddim:" + b for b in _blocks(c.B * c.hw)}
    if isinstance(c, TE):
        return {"temb:" + b for b in _blocks(c.B * c.dim)} | ({"temb:odd-half"} if (c.dim // 2) % 2 else {"temb:even-half"}) | ({"temb:t0"} if 0.0 in c.t else set())
    if isinstance(c, (NC, NH)):
        p, ld = ("to_nhwc:", c.cpad) if isinstance(c, NC) else ("to_nchw:", c.ld)
        n = c.B * c.hw * (ld if isinstance(c, NC) else c.c)
        return {p + b for b in _blocks(n)} | {p + ("tight" if ld == c.c else "padded")}
    if isinstance(c, U8):
        return {"u8:" + ("round" if c.round_mode else "truncate"), "u8:" + ("tight" if c.ld == 3 else "padded")}
    if isinstance(c, VS):
        return {"vae:" + ("sample" if c.noise else "mode"), "vae:out-" + c.outs} | {"vae:" + b for b in _blocks(c.npix * 4)}
    if isinstance(c, AN):
        return {"noise:" + b for b in _blocks(c.n)} | ({"noise:alpha1"} if c.alpha == 1.0 else {"noise:mix"})
    if isinstance(c, MA):
        p = "mask1:" if c.single else "maskB:"
        out = {p + ("k0" if c.iters == 0 else "k>=W" if c.iters >= c.W else "k>=H" if c.iters >= c.H else "k"), p + "place-" + c.place,
               p + ("finish-x-blocks" if c.W > 128 else "finish-one-x-block")}
        d = _mask_data(c)
        out |= {p + ("default" if u else "adapted") for u in d["use_default"]}
        if not c.single:
            out |= {p + ("row-loop-twice" if c.W > 256 else "row-loop-once"), p + ("write-pad" if c.write_pad else "keep-pad"), p + f"thres-{c.thres}",
                    p + ("forced" if c.force else "area-test")}
            if len(set(d["use_default"])) > 1:
                out.add(p + "decisions-differ")
        return out
    if isinstance(c, TX):
        w8 = c.width // 8
        return {"embed:" + ("one-pass" if w8 <= 64 else "several-passes"), "embed:" + ("last-pass-ragged" if w8 % 64 else "last-pass-full"),
                "embed:" + ("seqs" if c.seqs > 1 else "one-seq"), "embed:" + ("pos-rows-beyond-len" if c.n_pos > c.len else "pos-tight"),
                "embed:" + ("vocab1" if c.vocab == 1 else "vocab")}
    return {f"causal:len%4={c.len % 4}", "causal:" + ("second-key-register" if c.len > 64 else "first-key-register"), "causal:" + c.layout,
            "causal:" + ("ldo-gap" if c.dldo else "ldo-tight"), "causal:" + ("one-trip" if c.len <= 4 else "trips"),
            "causal:" + ("sharp" if c.sharp else "flat")}


_B4 = ("one-block", "blocks", "ragged", "exact-256")
REACHABLE = (
    {f"ddim:{m}" for m in ("full", "assemble", "step", "no-x0", "keep-latents")} | {f"ddim:alphas-{a}" for a in ("first", "mid", "last", "prev1", "prev0", "t1")}
    | {p + b for p in ("ddim:", "temb:", "to_nhwc:", "to_nchw:", "vae:", "noise:") for b in _B4}
    | {"temb:odd-half", "temb:even-half", "temb:t0", "to_nhwc:tight", "to_nhwc:padded", "to_nchw:tight", "to_nchw:padded"}
    | {"u8:round", "u8:truncate", "u8:tight", "u8:padded", "vae:sample", "vae:mode", "vae:out-f32", "vae:out-f16", "vae:out-both", "noise:alpha1", "noise:mix"}
    | {f"maskB:{k}" for k in ("k0", "k", "k>=W", "k>=H", "finish-x-blocks", "finish-one-x-block", "row-loop-twice", "row-loop-once", "write-pad", "keep-pad",
                              "forced", "area-test", "default", "adapted", "decisions-differ")}
    | {f"maskB:place-{p}" for p in ("corners", "edges", "lastcol", "one", "empty", "full", "random", "per-image")}
    | {f"maskB:thres-{t}" for t in ("0", "neg", "1e9", "eq", "+.5", "-.5", "split")}
    | {f"mask1:{k}" for k in ("k0", "k", "k>=W", "k>=H", "finish-x-blocks", "finish-one-x-block", "default", "adapted")}
    | {f"mask1:place-{p}" for p in ("corners", "edges", "lastcol", "one", "random")}
    | {"embed:one-pass", "embed:several-passes", "embed:last-pass-ragged", "embed:last-pass-full", "embed:seqs", "embed:one-seq", "embed:pos-rows-beyond-len",
       "embed:pos-tight", "embed:vocab1", "embed:vocab"}
    | {f"causal:len%4={r}" for r in range(4)}
    | {"causal:second-key-register", "causal:first-key-register", "causal:packed", "causal:separate", "causal:ldo-gap", "causal:ldo-tight",
       "causal:one-trip", "causal:trips", "causal:sharp", "causal:flat"})


# ------------------------------------------------------------------------------------------------------------------ buffers
class In(NamedTuple):
    buf: torch.Tensor           # flat, guards included
    off: int = 0                # elements between the front guard and the pointer's first element


class Out(NamedTuple):
    buf: torch.Tensor           # flat initial contents, guards included: the sentinel, or the data of an in / out operand
    must: torch.Tensor          # bool over buf: what the contract says the launch writes
    off: int = 0
    finite: bool = True         # float outputs: what is written has to be finite


_TORCH = {f16: torch.float16, f32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32}


def _poison(dtype):
    return np.nan if dtype in (f16, f32) else None


def pack_in(body, ld=None, poison=None, off=0):
    """body [rows, width] -> guard | off | rows x ld, gap columns poisoned | guard"""
    body = np.ascontiguousarray(body)
    return In(torch.from_numpy(kit.pack_rows(body, _poison(body.dtype.type) if poison is None else poison, ld, off)), off)


def _sentinel(n, dt):
    """the kit's sentinel; the one int32 output (`area`) starts as the bits of the fp32 pattern"""
    return kit.sentinel(n, f32).view(np.int32) if dt == np.int32 else kit.sentinel(n, dt)


def new_out(rows, width, ld, dt, off=0, must_cols=None, init=None, written=True, finite=True):
    """an output of rows x ld elements of which columns [0, width) (or the bool [ld] must_cols) of every row are written; init: the body's
    first contents when it is also read; written = False: the launch must leave all of it alone"""
    n = GUARD + off + rows * ld + GUARD
    buf = _sentinel(n, dt)
    if init is not None:
        buf[GUARD + off:GUARD + off + rows * ld].reshape(rows, ld)[:, :init.shape[-1]] = init.reshape(rows, -1)
    must = np.zeros(n, bool)
    if written:
        cols = np.arange(ld) < width if must_cols is None else must_cols
        must[GUARD + off:GUARD + off + rows * ld].reshape(rows, ld)[:, cols] = True
    return Out(torch.from_numpy(buf), torch.from_numpy(must), off, finite)


def body(o, buf, rows, ld):
    """the rows x ld body of a flat output buffer (numpy view)"""
    a = buf.numpy() if isinstance(buf, torch.Tensor) else buf
    return a[GUARD + o.off:GUARD + o.off + rows * ld].reshape(rows, ld)


# ------------------------------------------------------------------------------------------------------------------ data
SPECIAL32 = np.array([0.0, -0.0, 1.0, -1.0, 65504.0, -65504.0, 65519.996, -65519.996, 65520.0, -65520.0, 65536.0, 1e6, -3e38, np.inf, -np.inf,
                      1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -24, 2047.0, 2049.0, 2051.0,
                      2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26, 2.0 ** -24, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, -1.5 * 2.0 ** -24, 2.0 ** -25,
                      -(2.0 ** -25), 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -26, 1e-7, 3e-8, -3e-8, 1e-40, 6.1e-5, 6.0975e-5, 0.1, -0.3333, 3.14159],
                     dtype=f32)


def interesting32(g, n):
    x = (g.standard_normal(n) * np.exp(g.uniform(-12, 6, n))).astype(f32)
    k = min(n, SPECIAL32.size)
    x[g.permutation(n)[:k]] = g.permutation(SPECIAL32)[:k]
    return x


def _alphas(kind):
    """(alpha_t, alpha_prev) as Python floats; the entry point takes them as fp32"""
    a = so.ddim_alphas()
    ts = so.ddim_timesteps()
    pair = lambda t: (float(a[t]), float(a[t - 20] if t >= 20 else a[0]))
    return {"first": pair(ts[0]), "mid": pair(ts[24]), "last": pair(ts[-1]), "prev1": (float(a[1]), 1.0), "prev0": (float(a[500]), 0.0),
            "t1": (1.0, float(a[481]))}[kind]


LOGVARS = np.array([-40, -30.5, -30, 0, 19.5, 20, 25, np.inf, -np.inf, -3.25, 1.5], dtype=f16)


@functools.lru_cache(maxsize=4)
def _mask_data(c: MA):
    g = kit.rng("mask-" + c.name)                     # (not the id: the batched twin of a single-image case has the same data)
    B, H, W = c.B, c.H, c.W
    seg = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        # per-image: the image behind the one whose only pixel is its last is adapted too and has nothing of its own near its first rows' end,
        # so a window running from image b into image b + 1 shows
        kind = c.place if c.place != "per-image" else ("lastpix", "edges", "empty")[b % 3]
        pts = {"corners": [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)], "edges": [(0, W // 2), (H // 2, 0), (H // 2, W - 1), (H - 1, W // 2 + 1)],
               "lastcol": [(H // 2 - 1, W - 1), (H - 1, W - 1)], "lastpix": [(H - 1, W - 1)], "one": [(H // 2, W // 3)], "empty": []}.get(kind)
        if pts is not None:
            for y, x in pts:
                seg[b, y, x] = 1
        elif kind == "full":
            seg[b] = 1
        else:
            seg[b] = g.random((H, W)) > (0.97 + 0.01 * b)
    vals = {"1": 1, "255": 255}.get(c.segval)
    seg = seg * (np.uint8(vals) if vals else g.integers(1, 256, (B, H, W)).astype(np.uint8))
    yy, xx = np.mgrid[0:H, 0:W]
    dflt = np.broadcast_to(np.where((xx + 2 * yy) % 7 == 3, 0, c.dval).astype(np.uint8), (B, H, W)).copy()
    dflt[:, :, W // 4] = 0 if B > 1 else dflt[:, :, W // 4]
    img = g.uniform(-2, 2, (B, 3, H, W)).astype(f32)
    flat = img.reshape(-1)
    sp = np.array([-0.0, 0.0, 1e-7, -1e-7, 3e-8, 2.0 ** -25, 1.5 * 2.0 ** -24, 6.0975e-5, 1 + 2.0 ** -11, -1.9995117], dtype=f32)
    flat[g.permutation(flat.size)[:10 * sp.size]] = np.tile(sp, 10)
    area = seg.reshape(B, -1).astype(np.int64).sum(-1)
    thres = {"0": 0.0, "neg": -3.0, "1e9": 1e9, "eq": float(area[0]), "+.5": area[0] + 0.5, "-.5": area[0] - 0.5, "split": float(sorted(area)[B // 2])}[c.thres]
    use_default = tuple(bool(c.force or a < thres) for a in area)
    return dict(seg=seg, dflt=dflt, img=img, area=area, thres=thres, use_default=use_default)


@functools.lru_cache(maxsize=4)
def data(c):
    """name -> numpy array: the operands of a case without their packing"""
    g = kit.rng(c.id)
    if isinstance(c, DD):
        n = c.B * c.hw
        sp16 = np.array([0.0, -0.0, 1.0, 6e-8, -6e-8, 3e-5, 0.5], dtype=f16)
        mask = sp16[g.integers(0, sp16.size, n)]
        masked = g.standard_normal((n, 4)).astype(f16)
        masked.reshape(-1)[g.permutation(n * 4)[:max(1, n // 2)]] = sp16[g.integers(0, sp16.size, max(1, n // 2))]
        a_t, a_p = _alphas(c.alphas)
        return dict(eps=g.standard_normal((2 * n, 4)).astype(f16), latents=g.standard_normal((n, 4)).astype(f32), mask=mask, masked=masked,
                    alpha_t=a_t, alpha_prev=a_p)
    if isinstance(c, TE):
        return dict(t=np.array(c.t, dtype=f32))
    if isinstance(c, NC):
        return dict(x=interesting32(g, c.B * c.c * c.hw))
    if isinstance(c, NH):
        h = g.integers(0, 1 << 16, c.B * c.hw * c.c).astype(np.uint16)
        h = np.where((h & 0x7FFF) > 0x7C00, h & 0x83FF, h).astype(np.uint16)                    # NaN patterns become subnormals
        h[:min(h.size, 6)] = np.array([0, 0x8000, 1, 0x8001, 0x7C00, 0xFC00], np.uint16)[:min(h.size, 6)]
        return dict(x=h.view(f16).reshape(c.B * c.hw, c.c))
    if isinstance(c, U8):
        h = np.arange(1 << 16, dtype=np.uint16)
        v = h[(h & 0x7FFF) <= 0x7C00].view(f16)
        assert v.size == N_F16
        return dict(x=np.stack([v, np.roll(v, 7919), np.roll(v[::-1], 104729)], -1))             # every value in every channel
    if isinstance(c, VS):
        mom = np.empty((c.npix, 8), f16)
        mom[:, :4] = g.standard_normal((c.npix, 4)).astype(f16)
        mom[:, 4:] = LOGVARS[(np.arange(c.npix * 4) * 5 + 3) % LOGVARS.size].reshape(c.npix, 4) if c.npix > 2 else LOGVARS[[4, 2, 7, 1]]
        mom.reshape(-1)[::37] = f16(-0.0) if c.npix > 8 else mom.reshape(-1)[::37]
        return dict(mom=mom, noise=np.clip(g.standard_normal((c.npix, 4)), -3, 3).astype(f32), scale=0.18215)
    if isinstance(c, AN):
        return dict(x0=g.standard_normal(c.n).astype(f32), noise=g.standard_normal(c.n).astype(f32))
    if isinstance(c, MA):
        return _mask_data(c)
    if isinstance(c, TX):
        ids = g.integers(0, c.vocab, c.seqs * c.len).astype(np.int32)
        ids[0] = -5
        ids[-1] = c.vocab + 7
        if ids.size > 4:
            ids[1], ids[2] = c.vocab - 1, 0
        pos = g.standard_normal((c.n_pos, c.width)).astype(f16)
        pos[c.len:] = np.nan
        return dict(ids=ids, tok=g.standard_normal((c.vocab, c.width)).astype(f16), pos=pos)
    rows, w = c.seqs * c.len, c.heads * 64
    s = 2.5 if c.sharp else 0.25
    return dict(q=(g.standard_normal((rows, w)) * s).astype(f16), k=(g.standard_normal((rows, w)) * s).astype(f16),
                v=g.standard_normal((rows, w)).astype(f16), scale=0.125)


def ca_lds(c):
    w = c.heads * 64
    return (3 * w + 8,) * 3 if c.layout == "packed" else (w + 8, w + 16, w + 24)


@functools.lru_cache(maxsize=2)
def plan(c):
    """(ins: name -> In, outs: name -> Out) of a case"""
    d = data(c)
    if isinstance(c, DD):
        n = c.B * c.hw
        ins, outs = {}, {}
        if c.mode != "assemble":
            ins["eps"] = pack_in(d["eps"], c.eps_ld)
        if c.mode != "step":
            ins["mask"], ins["masked"] = pack_in(d["mask"][None]), pack_in(d["masked"])
            outs["unet_in"] = new_out(2 * n, 64, 64, f16)
        outs["latents"] = new_out(n, 4, 4, f32, init=d["latents"], written=c.mode in ("full", "step", "no-x0"))
        outs["x0"] = new_out(n, 4, 4, f32, written=c.mode in ("full", "step", "keep-latents"))
        return ins, outs
    if isinstance(c, TE):
        return dict(t=pack_in(d["t"][None])), dict(out=new_out(c.B, c.dim, c.dim, f16))
    if isinstance(c, NC):
        return dict(x=pack_in(d["x"][None])), dict(out=new_out(c.B * c.hw, c.cpad, c.cpad, f16, finite=False))
    if isinstance(c, NH):
        return dict(x=pack_in(d["x"], c.ld)), dict(out=new_out(1, c.B * c.c * c.hw, c.B * c.c * c.hw, f32, finite=False))
    if isinstance(c, U8):
        return dict(x=pack_in(d["x"], c.ld)), dict(out=new_out(N_F16, 3, 3, np.uint8))
    if isinstance(c, VS):
        ins = dict(mom=pack_in(d["mom"], c.ld))
        if c.noise:
            ins["noise"] = pack_in(d["noise"])
        outs = {}
        if c.outs in ("f32", "both"):
            outs["lat32"] = new_out(c.npix, 4, 4, f32)
        if c.outs in ("f16", "both"):
            outs["lat16"] = new_out(c.npix, 4, 4, f16)
        return ins, outs
    if isinstance(c, AN):
        return dict(x0=pack_in(d["x0"][None]), noise=pack_in(d["noise"][None])), dict(out=new_out(1, c.n, c.n, f32))
    if isinstance(c, MA):
        B, H, W = c.B, c.H, c.W
        ins = dict(dflt=pack_in(d["dflt"].reshape(1, -1), poison=DFLT_GUARD), img=pack_in(d["img"].reshape(1, -1)))
        if not c.force:
            ins["seg"] = pack_in(d["seg"].reshape(1, -1), poison=SEG_GUARD)
        lat = B * (H // 8) * (W // 8)
        batched = lambda cpad, wp: dict(mask_full=new_out(1, B * H * W, B * H * W, np.uint8), mask_lat=new_out(1, lat, lat, f16),
                                        masked=new_out(B * H * W, cpad if wp else 8, cpad, f16), area=new_out(1, B, B, np.int32))
        if c.single:
            outs = dict(mask_full=new_out(1, H * W, H * W, np.uint8), mask_lat=new_out(1, lat, lat, f16), masked=new_out(H * W, c.cpad, c.cpad, f16))
            outs.update({"b_" + k: v for k, v in batched(8, 0).items()})
            outs["b_scratch"] = new_out(1, H * W, H * W, np.uint8)
        else:
            outs = batched(c.cpad, c.write_pad)
            if not c.force:
                outs["scratch"] = new_out(1, B * H * W, B * H * W, np.uint8)
        return ins, outs
    if isinstance(c, TX):
        return (dict(ids=pack_in(d["ids"][None], poison=ID_GUARD), tok=pack_in(d["tok"]), pos=pack_in(d["pos"])),
                dict(out=new_out(c.seqs * c.len, c.width, c.width, f16)))
    rows, w = c.seqs * c.len, c.heads * 64
    if c.layout == "packed":
        ins = dict(qkv=pack_in(np.concatenate([d["q"], d["k"], d["v"]], -1), 3 * w + 8))
    else:
        ins = {k: pack_in(d[k], ld) for k, ld in zip("qkv", ca_lds(c))}
    return ins, dict(out=new_out(rows, w, w + c.dldo, f16, off=1))           # out sits one half off: 2-byte alignment is all the contract asks


def launch(ops, c, p):
    """The launch(es) of a case through coma_amd.sd.ops; p: name -> device tensor starting at the operand's / output's first element."""
    g = p.get
    d = data(c)
    if isinstance(c, DD):
        ops.cfg_ddim_step(g("eps"), c.eps_ld, p["latents"], None if c.mode == "no-x0" else p["x0"], g("mask"), g("masked"), g("unet_in"), batch=c.B,
                          hw=c.hw, guidance=c.guidance, alpha_t=d["alpha_t"], alpha_prev=d["alpha_prev"], write_latents=c.mode != "keep-latents")
    elif isinstance(c, TE):
        ops.timestep_embedding(p["t"], p["out"], batch=c.B, dim=c.dim)
    elif isinstance(c, NC):
        ops.nchw_to_nhwc(p["x"], p["out"], batch=c.B, c=c.c, hw=c.hw, cpad=c.cpad)
    elif isinstance(c, NH):
        ops.nhwc_to_nchw(p["x"], p["out"], batch=c.B, c=c.c, hw=c.hw, ld=c.ld)
    elif isinstance(c, U8):
        ops.image_to_u8(p["x"], p["out"], batch=2, hw=N_F16 // 2, ld=c.ld, round_mode=c.round_mode)
    elif isinstance(c, VS):
        ops.vae_sample(p["mom"], c.ld, g("noise"), d["scale"], c.npix, g("lat32"), g("lat16"))
    elif isinstance(c, AN):
        ops.add_noise(p["x0"][:c.n], p["noise"][:c.n], c.alpha, p["out"])
    elif isinstance(c, MA):
        kw = dict(H=c.H, W=c.W, dilate_iters=c.iters, cpad=c.cpad)
        if c.single:
            ops.mask_adapt(g("seg"), p["dflt"], p["img"], p["mask_full"], p["mask_lat"], p["masked"], use_default=d["use_default"][0], **kw)
            ops.mask_adapt_batched(g("seg"), p["dflt"], p["img"], p["b_mask_full"], p["b_mask_lat"], p["b_masked"], p["b_area"], p["b_scratch"], batch=1,
                                   force_default=False, area_thres=d["thres"], write_pad=False, **dict(kw, cpad=8))
        else:
            ops.mask_adapt_batched(g("seg"), p["dflt"], p["img"], p["mask_full"], p["mask_lat"], p["masked"], p["area"], g("scratch"), batch=c.B,
                                   force_default=bool(c.force), area_thres=d["thres"], write_pad=bool(c.write_pad), **kw)
    elif isinstance(c, TX):
        ops.text_embed(p["ids"], p["tok"], p["pos"], p["out"], seqs=c.seqs, len_=c.len, vocab=c.vocab, n_pos=c.n_pos, width=c.width)
    else:
        w = c.heads * 64
        ldq, ldk, ldv = ca_lds(c)
        q, k, v = (p["qkv"], p["qkv"][w:], p["qkv"][2 * w:]) if c.layout == "packed" else (p["q"], p["k"], p["v"])
        ops.attention_causal(q, k, v, p["out"], seqs=c.seqs, heads=c.heads, len_=c.len, d=64, ldq=ldq, ldk=ldk, ldv=ldv, ldo=w + c.dldo, scale=d["scale"])


# ------------------------------------------------------------------------------------------------------------------ references
class Ref(NamedTuple):
    ref: np.ndarray             # float64
    norm: np.ndarray            # what the error is divided by (sum of magnitudes of the formula's terms; 1 for absolute errors)
    stated: np.ndarray          # a-priori bound of |fp32 evaluation - ref| / norm
    floor: float                # floor of the device bound


def dilate_loops(seg, k):
    """max over the clipped (2k + 1)^2 window, pixel by pixel: u8 [H, W] -> bool [H, W]"""
    H, W = seg.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        y0, y1 = max(0, y - k), min(H - 1, y + k)
        for x in range(W):
            out[y, x] = seg[y0:y1 + 1, max(0, x - k):min(W - 1, x + k) + 1].any()
    return out


def mask_reference(seg, dflt, iters, use_default):
    """AND(dilate(seg), default), or the default mask where use_default[b]: u8 [B, H, W] x 2 -> u8 [B, H, W] of 0 / 1"""
    mask = np.zeros(seg.shape, np.uint8)
    for b in range(seg.shape[0]):
        dm = dflt[b] != 0
        mask[b] = dm if use_default[b] else (dilate_loops(seg[b], iters) & dm)
    return mask


def causal64(q, k, v, seqs, heads, ln, scale):
    """float64 softmax over keys 0 .. i, loops over sequence, head and query -> [seqs * len, heads * 64]"""
    out = np.zeros((seqs * ln, heads * 64))
    for s in range(seqs):
        for h in range(heads):
            sl = (slice(s * ln, (s + 1) * ln), slice(h * 64, (h + 1) * 64))
            Q, K, V = q[sl].astype(f64), k[sl].astype(f64), v[sl].astype(f64)
            for i in range(ln):
                sc = (K[:i + 1] @ Q[i]) * scale
                pr = np.exp(sc - sc.max())
                out[s * ln + i, h * 64:(h + 1) * 64] = (pr / pr.sum()) @ V[:i + 1]
    return out


def _ddim_coeffs(d, dt):
    a_t, a_p = f32(d["alpha_t"]), f32(d["alpha_prev"])
    if dt == f64:
        return np.sqrt(f64(a_t)), np.sqrt(1.0 - f64(a_t)), np.sqrt(f64(a_p)), np.sqrt(1.0 - f64(a_p))
    return _sqrt32(a_t), _sqrt32(f32(1.0) - a_t), _sqrt32(a_p), _sqrt32(f32(1.0) - a_p)


@functools.lru_cache(maxsize=2)
def reference(c):
    """name -> Ref for the arithmetic outputs, name -> exact numpy array for the exact ones"""
    d = data(c)
    if isinstance(c, DD):
        if c.mode == "assemble":
            return {}
        n = c.B * c.hw
        sa, s1, sap, s1p = _ddim_coeffs(d, f64)
        eu, ec, x, g = d["eps"][:n].astype(f64), d["eps"][n:].astype(f64), d["latents"].astype(f64), f64(f32(c.guidance))
        e, E = eu + g * (ec - eu), np.abs(eu) + abs(g) * (np.abs(ec) + np.abs(eu))
        x0, N0 = (x - s1 * e) / sa, (np.abs(x) + s1 * E) / sa
        xp, Np = sap * x0 + s1p * e, sap * N0 + s1p * E
        # counted, u = 2^-24, relative to the sums of magnitudes N0 / Np: e is three operations (3 u E); sqrt(1 - a) carries the rounding of
        # 1 - a and its own (2 u), the product one: 6 u s E; the difference u; the division by sqrt(a) (1 u) is allowed 4 u: 12 u N0.
        # x_prev: 14 u on sa_p x0, 6 u on s1ma_p e, u for the sum: 16 u Np.  Contraction into fma only removes roundings.
        return dict(x0=Ref(x0, N0, np.full(x0.shape, 12 * U32 * 1.001), FLOOR_X0), latents=Ref(xp, Np, np.full(xp.shape, 16 * U32 * 1.001), FLOOR_XPREV))
    if isinstance(c, TE):
        half = c.dim // 2
        arg = -f64(f32(9.210340371976184)) * np.arange(half) / half
        a = d["t"].astype(f64)[:, None] * np.exp(arg)[None]
        # the angle t f_k in fp32: two roundings in the exponent's argument (2 u |arg|), the exponential and the product (2 u), then the
        # function itself and the fp32 and fp16 roundings of a value <= 1.  The emulation forms exp / cos / sin in float64 and rounds: one u
        # more on the angle and one on the value are allowed for the host library's own error and the second rounding, so that the check
        # does not hang on one numpy build.  (The emulation's largest share, 0.997, is at a small angle: cos = 0.99146 lies 0.998 of half
        # an fp16 ulp from 0.9917, the 2^-12 term alone; the library terms are below 1e-3 of the bound there.)
        ea = np.abs(a) * (2 * U32 * np.abs(arg)[None] + 3 * U32) * 1.001
        st = np.concatenate([ea, ea], -1) + 3 * U32 + 2.0 ** -12
        return dict(out=Ref(np.concatenate([np.cos(a), np.sin(a)], -1), np.ones((c.B, c.dim)), st, FLOOR_TEMB))
    if isinstance(c, NC):
        x = d["x"].reshape(c.B, c.c, c.hw)
        out = np.zeros((c.B, c.hw, c.cpad), np.uint16)
        for b in range(c.B):
            for ch in range(c.c):
                for p in range(c.hw):
                    out[b, p, ch] = f32_to_f16_bits(x[b, ch, p:p + 1])[0]
        return dict(out=out.reshape(c.B * c.hw, c.cpad))
    if isinstance(c, NH):
        x = bits(d["x"]).reshape(c.B, c.hw, c.c)
        out = np.zeros((c.B, c.c, c.hw), f32)
        for b in range(c.B):
            for ch in range(c.c):
                for p in range(c.hw):
                    out[b, ch, p] = f16_bits_to_f32(x[b, p, ch])
        return dict(out=out.reshape(1, -1))
    if isinstance(c, U8):
        return dict(out=emulate(c)["out"])
    if isinstance(c, VS):
        mean, lv, sc = d["mom"][:, :4].astype(f64), np.clip(d["mom"][:, 4:].astype(f64), -30, 20), f64(f32(d["scale"]))
        std = np.exp(0.5 * lv)
        nz = d["noise"].astype(f64) if c.noise else np.zeros_like(mean)
        ref, N = (mean + std * nz) * sc, (np.abs(mean) + std * np.abs(nz)) * abs(sc)
        # exp, product, sum, product: one rounding each, every one relative to at most the sum of magnitudes
        return dict(lat=Ref(ref, np.maximum(N, 1e-300), np.full(ref.shape, 4 * U32 * 1.001), 0.0))
    if isinstance(c, AN):
        a = f32(c.alpha)
        sa, s1 = np.sqrt(f64(a)), np.sqrt(1.0 - f64(a))
        x0, nz = d["x0"].astype(f64), d["noise"].astype(f64)
        # sqrt(a) u, its product u; 1 - a and its square root 2 u, the product u; the sum u: at most 5 u of the magnitudes
        return dict(out=Ref((sa * x0 + s1 * nz)[None], (sa * np.abs(x0) + s1 * np.abs(nz))[None], np.full((1, c.n), 5 * U32 * 1.001), FLOOR_NOISE))
    if isinstance(c, MA):
        B, H, W = c.B, c.H, c.W
        mask = mask_reference(d["seg"], d["dflt"], c.iters, d["use_default"])
        img16 = f32_to_f16_bits(d["img"]).reshape(B, 3, H, W).transpose(0, 2, 3, 1)
        masked = np.where(mask[..., None] != 0, np.uint16(0), img16).reshape(B * H * W, 3)
        lat = np.where(mask[:, ::8, ::8] != 0, np.uint16(0x3C00), np.uint16(0)).reshape(1, -1)
        return dict(mask_full=mask.reshape(1, -1), mask_lat=lat, masked=masked, area=(np.zeros(B, np.int64) if c.force else d["area"])[None])
    if isinstance(c, TX):
        out = np.zeros((c.seqs * c.len, c.width), np.uint16)
        for row in range(c.seqs * c.len):
            i = min(max(int(d["ids"][row]), 0), c.vocab - 1)
            out[row] = f32_to_f16_bits(d["tok"][i].astype(f32) + d["pos"][row % c.len].astype(f32))
        return dict(out=out)
    q, k, v = d["q"], d["k"], d["v"]
    ref = causal64(q, k, v, c.seqs, c.heads, c.len, f64(f32(d["scale"])))
    # counted: a score is 64 fma and the scale, 65 u sum |q| |k| scale = ds; a probability carries 2 max ds of the exponent's argument, the
    # exponential, the i additions of the row sum, the reciprocal (4 u) and its product; the output i + 1 fma more; then the fp16 rounding.
    # Relative to the largest |ref| of the output row (a head's 64 channels of a query), as sections 3b / 3e do.
    st, norm = np.zeros_like(ref), np.zeros_like(ref)
    for s in range(c.seqs):
        for h in range(c.heads):
            sl = (slice(s * c.len, (s + 1) * c.len), slice(h * 64, (h + 1) * 64))
            ds = 65 * U32 * (np.abs(q[sl].astype(f64)) @ np.abs(k[sl].astype(f64)).T) * 0.125
            vmax = np.maximum.accumulate(np.abs(v[sl].astype(f64)).max(-1))                                             # largest |v_j|, j <= i
            i = np.arange(c.len)
            D = np.array([ds[j, :j + 1].max() for j in range(c.len)])
            rel = 2.02 * D + (2 * i + 10) * U32
            nrm = np.abs(ref[sl]).max(-1)
            st[sl] = ((1.002 * rel * vmax + 2.0 ** -25) / nrm + 2.0 ** -11)[:, None]
            norm[sl] = nrm[:, None]
    return dict(out=Ref(ref, norm, st, FLOOR_ATT))


# ------------------------------------------------------------------------------------------------------------------ emulations
MUTATIONS = ("ignore-write-latents", "area-le", "area-count-nonzero", "row-dilation-wraps", "round-mode-truncates", "logvar-clamp-20", "causal-key-i+1",
             "pos-row-not-mod-len")


def _fma32(a, b, acc):
    """fmaf on fp32 arrays whose product is exact in float64 (fp16 x fp16, or fp32 x fp16)"""
    return (a.astype(f64) * b.astype(f64) + acc.astype(f64)).astype(f32)


def emulate(c, mut=None):
    """name -> numpy body of every output the launch writes, as the kernel's formula gives it in fp32.  Outputs the launch leaves alone are
    returned with their first contents.  mut: one of MUTATIONS, a deliberately wrong kernel."""
    d = data(c)
    if isinstance(c, DD):
        n = c.B * c.hw
        out = dict(latents=d["latents"].copy(), x0=_sentinel(n * 4, f32).reshape(n, 4))
        x = d["latents"].copy()
        if c.mode != "assemble":
            sa, s1, sap, s1p = _ddim_coeffs(d, f32)
            eu, ec, g = d["eps"][:n].astype(f32), d["eps"][n:].astype(f32), f32(c.guidance)
            e = eu + g * (ec - eu)
            x0 = (x - s1 * e) / sa
            x = sap * x0 + s1p * e
            if c.mode != "no-x0":
                out["x0"] = x0
            if c.mode != "keep-latents" or mut == "ignore-write-latents":
                out["latents"] = x
        if c.mode != "step":
            u = np.zeros((n, 64), np.uint16)
            u[:, :4], u[:, 4], u[:, 5:9] = f32_to_f16_bits(x).reshape(n, 4), bits(d["mask"]), bits(d["masked"])
            out["unet_in"] = np.concatenate([u, u]).view(f16)
        return out
    if isinstance(c, TE):
        half = c.dim // 2
        arg = (f32(-9.210340371976184) * np.arange(half, dtype=f32)) / f32(half)
        a = d["t"][:, None] * kit.exp32(arg)[None]
        return dict(out=_to16(np.concatenate([np.cos(a.astype(f64)), np.sin(a.astype(f64))], -1).astype(f32)).reshape(c.B, c.dim))
    if isinstance(c, NC):
        out = np.zeros((c.B, c.hw, c.cpad), f16)
        with np.errstate(over="ignore"):
            out[:, :, :c.c] = d["x"].reshape(c.B, c.c, c.hw).transpose(0, 2, 1).astype(f16)
        return dict(out=out.reshape(-1, c.cpad))
    if isinstance(c, NH):
        return dict(out=d["x"].reshape(c.B, c.hw, c.c).transpose(0, 2, 1).astype(f32).reshape(1, -1))
    if isinstance(c, U8):
        with np.errstate(invalid="ignore"):
            v = d["x"].astype(f32) * f32(0.5) + f32(0.5)                # exact: an fma gives the same value
            v = np.minimum(np.maximum(v, f32(0.0)), f32(1.0)) * f32(255.0)
        return dict(out=(np.rint(v) if c.round_mode and mut != "round-mode-truncates" else np.trunc(v)).astype(np.uint8))
    if isinstance(c, VS):
        lo, hi = (-20, 20) if mut == "logvar-clamp-20" else (-30, 20)
        mean, lv = d["mom"][:, :4].astype(f32), np.minimum(np.maximum(d["mom"][:, 4:].astype(f32), f32(lo)), f32(hi))
        nz = d["noise"] if c.noise else np.zeros_like(mean)
        v = (mean + kit.exp32(f32(0.5) * lv) * nz) * f32(d["scale"])
        return {k: val for k, val in (("lat32", v), ("lat16", _to16(v).reshape(v.shape))) if k in plan(c)[1]}
    if isinstance(c, AN):
        a = f32(c.alpha)
        return dict(out=(_sqrt32(a) * d["x0"] + _sqrt32(f32(1.0) - a) * d["noise"])[None])
    if isinstance(c, MA):
        B, H, W, k = c.B, c.H, c.W, c.iters
        seg = d["seg"]
        area = (seg != 0).reshape(B, -1).sum(-1) if mut == "area-count-nonzero" else seg.reshape(B, -1).astype(np.int64).sum(-1)
        area = np.zeros(B, np.int64) if c.force else area
        use = [bool(c.force or (a <= d["thres"] if mut == "area-le" else a < d["thres"])) for a in area]
        mask = np.zeros((B, H, W), np.uint8)
        for b in range(B):
            dm = d["dflt"][b] != 0
            if use[b]:
                mask[b] = dm
                continue
            s = seg[b] != 0
            if mut == "row-dilation-wraps":                             # the row window runs over the flat image
                f = s.reshape(-1)
                idx = np.arange(H * W)
                rows = np.array([f[max(0, i - k):i + k + 1].any() for i in idx]).reshape(H, W)
            else:
                cs = np.concatenate([np.zeros((H, 1), np.int64), np.cumsum(s, 1)], 1)
                xx = np.arange(W)
                rows = (cs[:, np.minimum(W - 1, xx + k) + 1] - cs[:, np.maximum(0, xx - k)]) > 0
            cc = np.concatenate([np.zeros((1, W), np.int64), np.cumsum(rows, 0)], 0)
            yy = np.arange(H)
            mask[b] = ((cc[np.minimum(H - 1, yy + k) + 1] - cc[np.maximum(0, yy - k)]) > 0) & dm
        cp = c.cpad
        ncol = cp if (c.single or c.write_pad) else 8
        m = _sentinel(B * H * W * cp, f16).reshape(-1, cp)
        m[:, :ncol] = 0
        m[:, :3] = np.where(mask.reshape(-1, 1) != 0, f16(0), d["img"].astype(f16).transpose(0, 2, 3, 1).reshape(-1, 3))
        out = dict(mask_full=mask.reshape(1, -1), mask_lat=(mask[:, ::8, ::8] != 0).astype(f16).reshape(1, -1), masked=m)
        if c.single:
            b = emulate(c._replace(single=0, cpad=8, write_pad=0), mut)
            out.update({"b_" + kk: v for kk, v in b.items()})
        else:
            out["area"] = area.astype(np.int32)[None]
            if not c.force:
                out["scratch"] = None                                   # a workspace: written, contents not part of the contract
        return out
    if isinstance(c, TX):
        ids = np.clip(d["ids"], 0, c.vocab - 1)
        rows = np.arange(c.seqs * c.len)
        if mut == "pos-row-not-mod-len":
            flat = np.concatenate([plan(c)[0]["pos"].buf.numpy()[GUARD:], np.full(rows.size * c.width, np.nan, f16)])     # what lies behind is not data
            pos = np.stack([flat[r * c.width:(r + 1) * c.width] for r in rows])
        else:
            pos = d["pos"][rows % c.len]
        with np.errstate(invalid="ignore"):
            return dict(out=(d["tok"][ids].astype(f32) + pos.astype(f32)).astype(f16))
    ln, sc = c.len, f32(d["scale"])
    out = np.zeros((c.seqs * ln, c.heads * 64), f16)
    jj, ii = np.meshgrid(np.arange(ln), np.arange(ln))
    valid = jj <= (np.minimum(ii + 1, ln - 1) if mut == "causal-key-i+1" else ii)
    for s in range(c.seqs):
        for h in range(c.heads):
            sl = (slice(s * ln, (s + 1) * ln), slice(h * 64, (h + 1) * 64))
            Q, K, V = d["q"][sl].astype(f32), d["k"][sl].astype(f32), d["v"][sl].astype(f32)
            S = np.zeros((ln, ln), f32)
            for e in range(64):
                S = _fma32(Q[:, e:e + 1], K[None, :, e], S)
            S = np.where(valid, S * sc, f32(-np.inf))
            E = np.where(valid, kit.exp32(S - S.max(-1, keepdims=True)), f32(0))
            tot = np.zeros(ln, f32)
            for j in range(ln):
                tot = tot + E[:, j]
            P = E * (f32(1.0) / tot)[:, None]
            acc = np.zeros((ln, 64), f32)
            for j in range(ln):
                acc = _fma32(P[:, j:j + 1], V[j][None], acc)
            out[sl] = acc.astype(f16)
    return dict(out=out)


# ------------------------------------------------------------------------------------------------------------------ the yardstick and the checks
class Figure(NamedTuple):
    e_emu: float
    bound: float
    err: float                  # of the outputs given to check()
    emu_over_stated: float


def _err(got, r: Ref):
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(np.asarray(got, dtype=f64).reshape(r.ref.shape) - r.ref) / r.norm
    return np.nan_to_num(e, nan=np.inf)


@functools.lru_cache(maxsize=4)
def yardstick(c):
    """output name -> (e_emu, bound, emulation's largest share of its a-priori bound) for the arithmetic outputs of a case"""
    # (a DDIM case that stores only some of its results is measured on all of them: the arithmetic is the same)
    ref, emu = reference(c), emulate(c._replace(mode="full") if isinstance(c, DD) and c.mode != "assemble" else c)
    out = {}
    for name, r in ref.items():
        if not isinstance(r, Ref):
            continue
        e = _err(emu["lat32" if name == "lat" and "lat32" in emu else "lat16" if name == "lat" else name], r)
        stated = r.stated + ((2.0 ** -11 + 2.0 ** -25 / r.norm) if name == "lat" and "lat32" not in emu else 0.0)
        e_emu = float(e.max())
        out[name] = (e_emu, max(4 * e_emu, r.floor), float((e / stated).max()))
    return out


def _same(a, b, what):
    a, b = bits(np.asarray(a)).reshape(-1), bits(np.asarray(b)).reshape(-1)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} elements differ, first at {int(bad[0])}: {int(a[bad[0]]):#x} != {int(b[bad[0]]):#x}"


def check(c, got):
    """Every assertion of case c on the bodies `got` (name -> numpy array shaped as emulate() returns them) -> name -> Figure."""
    ref, d, y, fig = reference(c), data(c), yardstick(c), {}

    def bounded(name, value, rname=None):
        rname = rname or name
        e_emu, bound, share = y[rname]
        e = _err(value, ref[rname])
        fig[name] = Figure(e_emu, bound, float(e.max()), share)
        assert fig[name].err <= bound, f"{c.id}: `{name}` error {fig[name].err:.3e} > {bound:.3e} (e_emu {e_emu:.3e}) at {int(e.argmax())}"

    if isinstance(c, DD):
        n = c.B * c.hw
        if c.mode in ("full", "step", "no-x0"):
            bounded("latents", got["latents"])
        else:
            _same(got["latents"], d["latents"], "latents must keep their bits")
        if c.mode in ("full", "step", "keep-latents"):
            bounded("x0", got["x0"])
        else:
            _same(got["x0"], _sentinel(n * 4, f32), "x0_out must not be written")
        if c.mode != "step":
            u = bits(got["unet_in"]).reshape(2, n, 64)
            _same(u[0], u[1], "the two halves of unet_in")
            if c.mode == "keep-latents":                                # the fp32 x_prev is not stored: its fp16 rounding against float64
                r = ref["latents"]
                e = np.abs(u[0][:, :4].view(f16).astype(f64) - r.ref)
                lim = y["latents"][1] * r.norm + 2.0 ** -11 * np.abs(r.ref) + 2.0 ** -25
                assert bool((e <= lim).all()), f"{c.id}: channels 0 .. 3 of unet_in are not the new x_prev (worst {float((e / lim).max()):.2f} of the bound)"
            else:
                _same(u[0][:, :4], f32_to_f16_bits(got["latents"]).reshape(n, 4), "channels 0 .. 3 = fp16(device's own fp32 x_prev)")
            _same(u[0][:, 4], bits(d["mask"]), "channel 4 = mask")
            _same(u[0][:, 5:9], bits(d["masked"]), "channels 5 .. 8 = masked_latents")
            assert not u[:, :, 9:].any(), "channels 9 .. 63 must be +0"
    elif isinstance(c, TE):
        bounded("out", got["out"])
        for b, t in enumerate(c.t):
            if t == 0.0:
                _same(got["out"][b], np.concatenate([np.ones(c.dim // 2, f16), np.zeros(c.dim // 2, f16)]), "t = 0 gives [1 .. | 0 ..]")
    elif isinstance(c, (NC, NH, TX)):
        _same(got["out"], ref["out"], "out")
    elif isinstance(c, U8):
        _same(got["out"], ref["out"], "out")
    elif isinstance(c, VS):
        if "lat32" in got:
            if c.noise:
                bounded("lat32", got["lat32"], "lat")
            else:
                _same(got["lat32"], (d["mom"][:, :4].astype(f32) + f32(0)) * f32(d["scale"]), "the mode is one fp32 product")
            if "lat16" in got:
                _same(got["lat16"], f32_to_f16_bits(got["lat32"]), "lat16 = fp16(device's own lat32)")
        else:
            r = ref["lat"]
            e_emu, bound, share = y["lat"]
            # the fp32 value is held to the fp32 bound of the same data (4 e_emu of the fp32 emulation), then rounded once
            e32 = float(_err(emulate(c._replace(outs="f32"))["lat32"], r).max())
            e = np.abs(got["lat16"].astype(f64) - r.ref)
            lim = 4 * e32 * r.norm + 2.0 ** -11 * np.abs(r.ref) * (1 + 4 * e32) + 2.0 ** -25
            fig["lat16"] = Figure(e_emu, float("nan"), float((e / r.norm).max()), share)
            assert bool((e <= lim).all()), f"{c.id}: lat16 at {float((e / lim).max()):.2f} of its bound"
    elif isinstance(c, AN):
        bounded("out", got["out"])
        if c.alpha == 1.0:
            _same(got["out"], d["x0"], "alpha = 1: out = x0")
    elif isinstance(c, MA):
        for p in ("", "b_") if c.single else ("",):
            cp = 8 if p else c.cpad
            _same(got[p + "mask_full"], ref["mask_full"], p + "mask_full")
            _same(got[p + "mask_lat"], ref["mask_lat"], p + "mask_lat")
            m = bits(got[p + "masked"]).reshape(-1, cp)
            _same(m[:, :3], ref["masked"], p + "masked_image channels 0 .. 2")
            full = bool(c.single and not p) or bool(c.write_pad and not p)
            ncol = cp if full else 8
            assert not m[:, 3:ncol].any(), p + "padding channels must be +0"
            assert bool((m[:, ncol:] == kit.sentinel_bits(f16)).all()), p + "channels >= 8 are left alone without write_pad"
            if p or not c.single:
                _same(got[p + "area"].astype(np.int64), ref["area"], p + "area")
    else:
        bounded("out", got["out"])
    return fig


# ------------------------------------------------------------------------------------------------------------------ refusals
OUTPUT_ARGS = {"latents", "x0_out", "unet_in", "out", "latents_f32", "latents_f16", "mask_full", "mask_latent", "masked_image", "area", "scratch"}

_DD = dict(eps_uc=PTR, eps_ld=4, latents=PTR, x0_out=PTR, mask=PTR, masked_latents=PTR, unet_in=PTR, batch=1, hw=4, guidance=7.5, alpha_t=0.5,
           alpha_prev=0.6, write_latents=1)
_M1 = dict(seg=PTR, default_mask=PTR, H=8, W=8, dilate_iters=1, use_default=0, image_nchw=PTR, cpad=8, mask_full=PTR, mask_latent=PTR, masked_image=PTR)
_MB = dict(seg=PTR, default_mask=PTR, batch=1, H=8, W=8, dilate_iters=1, force_default=0, area_thres=1.0, image_nchw=PTR, cpad=8, write_pad=0,
           mask_full=PTR, mask_latent=PTR, masked_image=PTR, area=PTR, scratch=PTR)
_TX = dict(ids=PTR, seqs=1, len=4, tok_emb=PTR, vocab=10, pos_emb=PTR, n_pos=4, width=8, out=PTR)
_CA = dict(q=PTR, k=PTR, v=PTR, out=PTR, seqs=1, heads=2, len=4, d=64, ldq=128, ldk=128, ldv=128, ldo=128, scale=0.125)
_BIG = 1 << 30

# entry point -> (accepted base, [(text of the refusal, change), ...]): every condition the argument checks state
REFUSALS = {
    "sd_cfg_ddim_step": (_DD, [
        ("null latents", dict(latents=None)), ("mask inputs missing", dict(mask=None)), ("mask inputs missing", dict(masked_latents=None)),
        ("bad sizes", dict(batch=0)), ("bad sizes", dict(hw=0)), ("bad sizes", dict(batch=-1)),
        ("alphas out of range", dict(alpha_t=0.0)), ("alphas out of range", dict(alpha_t=1.5)), ("alphas out of range", dict(alpha_t=float("nan"))),
        ("alphas out of range", dict(alpha_prev=-0.1)), ("alphas out of range", dict(alpha_prev=1.5)), ("alphas out of range", dict(alpha_prev=float("nan"))),
        ("eps_ld = 3 is below the 4 channels", dict(eps_ld=3)), ("eps_ld = 0 is below", dict(eps_ld=0)), ("eps_ld = -4 is below", dict(eps_ld=-4)),
        ("unet_in must be 16-byte aligned", dict(unet_in=Off(2))), ("unet_in must be 16-byte aligned", dict(unet_in=Off(8), eps_uc=None)),
        (f"batch * hw = {_BIG * 1024} exceeds the grid limit", dict(batch=_BIG, hw=1024))]),
    "sd_timestep_embedding_f16": (dict(timesteps=PTR, batch=1, dim=4, out=PTR), [
        ("bad args", dict(timesteps=None)), ("bad args", dict(out=None)), ("bad args", dict(batch=0)), ("bad args", dict(dim=0)), ("bad args", dict(dim=5)),
        ("bad args", dict(dim=-2)), (f"batch * dim = {1 << 31} exceeds the int32 limit 2147483647", dict(batch=1 << 20, dim=1 << 11)),
        (f"batch * dim = {65536 * 65536} exceeds", dict(batch=65536, dim=65536))]),
    "sd_nchw_to_nhwc_f16": (dict(x=PTR, batch=1, c=3, hw=4, cpad=8, out=PTR), [
        ("bad args", dict(x=None)), ("bad args", dict(out=None)), ("bad args", dict(batch=0)), ("bad args", dict(c=0)), ("bad args", dict(hw=0)),
        ("bad args", dict(cpad=2)), ("exceeds the grid limit", dict(batch=_BIG, hw=_BIG)), ("exceeds the grid limit", dict(batch=_BIG, hw=64, cpad=9))]),
    "sd_nhwc_to_nchw_f32": (dict(x=PTR, batch=1, c=3, hw=4, ld=8, out=PTR), [
        ("bad args", dict(x=None)), ("bad args", dict(out=None)), ("bad args", dict(batch=0)), ("bad args", dict(c=0)), ("bad args", dict(hw=0)),
        ("bad args", dict(ld=2)), ("exceeds the grid limit", dict(batch=_BIG, hw=_BIG)), ("exceeds the grid limit", dict(batch=_BIG, hw=64, c=9, ld=9))]),
    "sd_image_to_u8": (dict(x=PTR, batch=1, hw=4, ld=3, round_mode=0, out=PTR), [
        ("bad args", dict(x=None)), ("bad args", dict(out=None)), ("bad args", dict(batch=0)), ("bad args", dict(hw=0)), ("bad args", dict(ld=2)),
        ("exceeds the grid limit", dict(batch=_BIG, hw=256)), ("exceeds the grid limit", dict(batch=_BIG, hw=_BIG))]),
    "sd_vae_sample": (dict(moments=PTR, ld=8, noise=PTR, scale=0.18215, npix=4, latents_f32=PTR, latents_f16=PTR), [
        ("bad args", dict(moments=None)), ("bad args", dict(npix=0)), ("bad args", dict(npix=-1)), ("bad args", dict(ld=7)),
        ("bad args", dict(latents_f32=None, latents_f16=None)), ("exceeds the grid limit", dict(npix=1 << 38)), ("exceeds the grid limit", dict(npix=1 << 62))]),
    "sd_add_noise": (dict(x0=PTR, noise=PTR, alpha=0.5, n=4, out=PTR), [
        ("bad args", dict(x0=None)), ("bad args", dict(noise=None)), ("bad args", dict(out=None)), ("bad args", dict(n=0)), ("bad args", dict(alpha=0.0)),
        ("bad args", dict(alpha=1.5)), ("bad args", dict(alpha=float("nan"))), (f"n = {1 << 40} exceeds the grid limit", dict(n=1 << 40))]),
    "sd_mask_adapt": (_M1, [
        ("null pointer", dict(seg=None)), ("null pointer", dict(default_mask=None)), ("null pointer", dict(image_nchw=None)), ("null pointer", dict(mask_full=None)),
        ("null pointer", dict(mask_latent=None)), ("null pointer", dict(masked_image=None)),
        ("bad sizes", dict(H=0)), ("bad sizes", dict(W=0)), ("bad sizes", dict(H=12)), ("bad sizes", dict(W=12)), ("bad sizes", dict(dilate_iters=-1)),
        ("bad sizes", dict(cpad=2)), ("H = 65536 exceeds the grid limit 65535", dict(H=65536)),
        (f"H * W = {65528 * 32776} exceeds the int32 limit", dict(H=65528, W=32776))]),
    "sd_mask_adapt_batched": (_MB, [
        ("null pointer", dict(seg=None)), ("null pointer", dict(scratch=None)), ("null pointer", dict(default_mask=None)), ("null pointer", dict(image_nchw=None)),
        ("null pointer", dict(mask_full=None)), ("null pointer", dict(mask_latent=None)), ("null pointer", dict(masked_image=None)),
        ("null pointer", dict(area=None)), ("null pointer", dict(area=None, force_default=1, seg=None, scratch=None)),
        ("bad sizes", dict(batch=0)), ("bad sizes", dict(batch=65536)), ("bad sizes", dict(H=0)), ("bad sizes", dict(H=65536)), ("bad sizes", dict(W=0)),
        ("bad sizes", dict(W=16392)), ("bad sizes", dict(H=12)), ("bad sizes", dict(W=12)), ("bad sizes", dict(dilate_iters=-1)), ("bad sizes", dict(cpad=0)),
        ("bad sizes", dict(cpad=12)), (f"H * W * 255 = {2064 * 4096 * 255} exceeds the int32 limit 2147483647 of the area sum", dict(H=2064, W=4096)),
        ("exceeds the int32 limit 2147483647 of the area sum", dict(H=65528, W=16384)),
        ("masked_image must be 16-byte aligned", dict(masked_image=Off(2))), ("masked_image must be 16-byte aligned", dict(masked_image=Off(8), force_default=1))]),
    "sd_text_embed_f16": (_TX, [
        ("null pointer", dict(ids=None)), ("null pointer", dict(tok_emb=None)), ("null pointer", dict(pos_emb=None)), ("null pointer", dict(out=None)),
        ("bad sizes", dict(seqs=0)), ("bad sizes", dict(len=0)), ("bad sizes", dict(vocab=0)), ("bad sizes", dict(n_pos=3)), ("bad sizes", dict(width=0)),
        ("bad sizes", dict(width=12)), ("too many rows", dict(seqs=1 << 16, len=1 << 15, n_pos=1 << 15)),
        ("16-byte aligned", dict(tok_emb=Off(8))), ("16-byte aligned", dict(pos_emb=Off(2))), ("16-byte aligned", dict(out=Off(4)))]),
    "sd_attention_causal_f16": (_CA, [
        ("null pointer", dict(q=None)), ("null pointer", dict(k=None)), ("null pointer", dict(v=None)), ("null pointer", dict(out=None)),
        ("head dim must be 64 (got 40)", dict(d=40)), ("sequence length must be 1..128 (got 0)", dict(len=0)), ("sequence length must be 1..128 (got 129)", dict(len=129)),
        ("bad seqs / heads", dict(seqs=0)), ("bad seqs / heads", dict(heads=0)), ("bad seqs / heads", dict(seqs=65536)),
        ("bad seqs / heads", dict(heads=65536, ldq=1 << 22, ldk=1 << 22, ldv=1 << 22, ldo=1 << 22)),
        ("leading dimensions", dict(ldq=120)), ("leading dimensions", dict(ldk=64)), ("leading dimensions", dict(ldv=0)), ("leading dimensions", dict(ldo=127)),
        ("leading dimensions", dict(ldq=132)), ("leading dimensions", dict(ldk=130)), ("leading dimensions", dict(ldv=129)),
        ("q / k / v must be 16-byte aligned", dict(q=Off(2))), ("q / k / v must be 16-byte aligned", dict(k=Off(8))), ("q / k / v must be 16-byte aligned", dict(v=Off(4))),
        ("out must be 2-byte aligned", dict(out=Off(1)))]),
}
