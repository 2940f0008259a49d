"""Test helper for the attention kernels of coma_amd/csrc/sd_attention.hip (sd_attention_f16, its software-pipelined d = 40 form and
sd_attention_wide_f16): plain torch on the CPU, nothing here is product code and nothing here needs a GPU.

* ``attention_f64``             softmax(q k^T scale) v in float64 on the fp16-rounded inputs: the truth a kernel is measured against.
* ``attention_fp16_emulation``  the same arithmetic as a careful fp16 kernel does it (fp32 scores, softmax weights rounded to fp16 before
                                the PV product, fp32 accumulation in index order, fp16 output).  Its distance from the truth, per query and normalised by
                                that query's largest |output|, is ``e_emu``: the yardstick of tests/test_sd_attention_domain_gpu.py, whose
                                bound for the device is ``max(4 * e_emu, 2^-10)`` (``device_bound``).
* ``emulation_bound``           an a-priori, element-wise worst-case bound of the emulation's own error (the emulation's stated bound).
* packing helpers               lay q / k / out / V^T into flat buffers with a leading dimension and a column offset; everything the
                                contract of include/sd_hip.h says is NOT read is NaN, V^T pad columns ("must be finite") are 1e4, `out`
                                is prefilled with a NaN bit pattern, so an element the kernel should have written and did not shows too
                                (the guard width, that pattern, the seed and ``device_bound`` are tests/domain_kit.py's).
* ``CASES``                     the table of launches, shared by the host test (which computes e_emu for every row) and the GPU test.
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional, Tuple

import torch

from tests import domain_kit as kit
from tests.domain_kit import F16, F32, F64, GUARD, device_bound      # (GUARD: NaN halves after the last row of every operand)

LOG2E = 1.4426950408889634
PAD_VALUE = 1.0e4            # V^T pad columns lk .. ldv-1: finite, and large enough that a non-zero weight on one of them shows


# ---------------------------------------------------------------------------------------------------------------- references
def _split(x, heads, dtype):
    B, L, C = x.shape
    return x.to(F16).to(dtype).reshape(B, L, heads, C // heads).transpose(1, 2)          # [B, H, L, d]


def _merge(x):
    B, H, L, d = x.shape
    return x.transpose(1, 2).reshape(B, L, H * d)


def _scale32(scale):
    """The scale as the C ABI receives it (a float)."""
    return float(torch.tensor(scale, dtype=F32))


def attention_f64(q, k, v, heads, scale):
    """q [B, Lq, H*d], k / v [B, Lk, H*d] (rounded to fp16 first) -> [B, Lq, H*d] float64."""
    qh, kh, vh = (_split(t, heads, F64) for t in (q, k, v))
    w = torch.softmax(qh @ kh.transpose(-1, -2) * _scale32(scale), dim=-1)
    return _merge(w @ vh)


def attention_fp16_emulation(q, k, v, heads, scale, round_q=False):
    """A careful fp16 attention kernel in fp32 torch: fp32 scores, exp2 of (score * scale*log2(e) - max), fp32 denominator, weights
    rounded to fp16 before the PV product, fp32 accumulation, one rounding to fp16 at the end.  round_q: Q * scale*log2(e) is rounded
    to fp16 BEFORE the score product, as the software-pipelined d = 40 kernel is documented to do (include/sd_hip.h)."""
    c = torch.tensor(_scale32(scale), dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    qh, kh, vh = (_split(t, heads, F32) for t in (q, k, v))
    if round_q:
        e = _dot_in_order((qh * c).to(F16).to(F32), kh)
        e = e - e.max(-1, keepdim=True).values
    else:
        s = _dot_in_order(qh, kh)
        e = s * c - s.max(-1, keepdim=True).values * c
    p = torch.exp2(e.to(F64)).to(F32)                 # a correctly rounded fp32 exp2, whatever the host's vector library does
    ph = p.to(F16).to(F32)
    l, o = torch.zeros_like(p[..., 0]), torch.zeros(*p.shape[:-1], vh.shape[-1], dtype=F32)
    for j in range(p.shape[-1]):                      # fp32 accumulation in key order
        l += p[..., j]
        o += ph[..., j, None] * vh[..., None, j, :]
    return _merge(o * (1.0 / l)[..., None]).to(F16)


def _dot_in_order(a, b):
    """a [.., Lq, d] . b [.., Lk, d]^T in fp32, the d products added in index order: element-wise IEEE arithmetic only, so the result --
    and with it e_emu -- is the same on every host (a BLAS call picks its own summation order per CPU)."""
    s = torch.zeros(*a.shape[:-1], b.shape[-2], dtype=F32)
    for i in range(a.shape[-1]):
        s += a[..., :, None, i] * b[..., None, :, i]
    return s


def emulation_bound(q, k, v, heads, scale, round_q=False):
    """Element-wise worst-case bound of |attention_fp16_emulation - attention_f64|, from float64 quantities only.  With w the exact
    softmax weights, A = w |v| and T[q, key] = sum_i |q_i k_i| scale*log2(e) (the score's condition, in log2 units):
      * scores: fp32 accumulation of d exact products and the scaling move an exponent by at most u_s T, u_s = (d + 4) 2^-24 (plus
        2^-11 with round_q); every weight then changes by a factor within 2^(+-2 Delta), Delta = max_key u_s T: (2^(2 Delta) - 1) A;
      * weights rounded to fp16: 2^-11 A, and 2^-25 sum|v| for weights below the fp16 normal range;
      * fp32 exp2, denominator sum, PV accumulation (any order), reciprocal: (2 lk + 16) 2^-24 A;
      * output rounded to fp16: 2^-11 |ref| (+ 2^-25 below the normal range)."""
    sc = _scale32(scale)
    qh, kh, vh = (_split(t, heads, F64) for t in (q, k, v))
    d, lk = qh.shape[-1], kh.shape[-2]
    w = torch.softmax(qh @ kh.transpose(-1, -2) * sc, dim=-1)
    ref = w @ vh
    A = w @ vh.abs()
    T = (qh.abs() @ kh.abs().transpose(-1, -2)) * (sc * LOG2E)
    u_s = (d + 4) * 2.0 ** -24 + (2.0 ** -11 if round_q else 0.0)
    delta = u_s * T.max(-1, keepdim=True).values
    rel = torch.exp2(2 * delta) - 1 + 2.0 ** -11 + (2 * lk + 16) * 2.0 ** -24
    bound = 1.001 * rel * A + 2.0 ** -25 * vh.abs().sum(-2, keepdim=True) + 2.0 ** -11 * ref.abs() + 2.0 ** -24
    return _merge(bound)


def query_error(got, ref, heads):
    """Per (batch, head, query): max |got - ref| over the head's d outputs, divided by that query's max |ref| -> [B, H, Lq] float64."""
    B, L, C = ref.shape
    g = got.to(F64).reshape(B, L, heads, C // heads)
    r = ref.to(F64).reshape(B, L, heads, C // heads)
    return ((g - r).abs().amax(-1) / r.abs().amax(-1)).transpose(1, 2)


# ---------------------------------------------------------------------------------------------------------------- packing
def roundup(n, m):
    return (n + m - 1) // m * m


def pack_rows(x, ld, col0=0):
    """x [B, L, C] -> flat fp16 buffer, element (b, l, c) at col0 + (b L + l) ld + c; gap columns C .. ld-1, the col0 halves in front and
    GUARD halves after the last row are NaN.  The kernel's pointer is buf[col0:]."""
    B, L, C = x.shape
    assert ld >= C
    buf = torch.full((col0 + B * L * ld + GUARD,), float("nan"), dtype=F16)
    buf[col0:col0 + B * L * ld].view(B, L, ld)[:, :, :C] = x.to(F16)
    return buf


def pack_fused_qk(q, k):
    """The UNet's fused projection output: one [B, L, 2C] buffer, q in columns 0 .. C-1 and k in C .. 2C-1 (ldq = ldk = 2C, the K
    pointer is buf[C:]); GUARD NaN halves behind it."""
    assert q.shape == k.shape
    return pack_rows(torch.cat([q, k], -1), 2 * q.shape[-1])


def perm16_source(n):
    """Key held by position j of a PERM16 row: every group of 16 positions holds the keys (0-3, 8-11, 4-7, 12-15)."""
    j = torch.arange(n)
    return (j & ~12) | ((j & 4) << 1) | ((j & 8) >> 1)


def perm32_source(n):
    """Key held by position p = 8g + e of a PERM32 row: 16 (e >> 2) + 4g + (e & 3) within every group of 32."""
    p = torch.arange(n)
    return (p & ~28) | (((p >> 3) & 3) << 2) | (((p >> 2) & 1) << 4)


def _pack_vt(v, ldv, src):
    B, lk, C = v.shape
    rows = torch.full((B, C, ldv), PAD_VALUE, dtype=F16)
    real = src < lk                                   # positions whose key exists; all others are pad columns
    pos = torch.arange(src.numel())[real]
    rows[:, :, pos] = v.to(F16).transpose(1, 2)[:, :, src[real]]
    buf = torch.full((B * C * ldv + GUARD,), float("nan"), dtype=F16)
    buf[:B * C * ldv] = rows.reshape(-1)
    return buf


def pack_vt_plain(v, ldv):
    """v [B, lk, H*d] -> V^T [B, H*d, ldv] flat, ldv >= roundup(lk, 8): keys in order, pad columns PAD_VALUE, NaN guard behind."""
    assert ldv % 8 == 0 and ldv >= roundup(v.shape[1], 8)
    return _pack_vt(v, ldv, torch.arange(ldv))


def pack_vt_perm16(v, ldv):
    """... in the SD_EPI_PERM16_N key order (ldv % 16 == 0, ldv >= roundup(lk, 16)); positions whose key is >= lk are pad columns."""
    assert ldv % 16 == 0 and ldv >= roundup(v.shape[1], 16)
    return _pack_vt(v, ldv, perm16_source(ldv))


def pack_vt_perm32(v, ldv):
    """... in the SD_EPI_PERM32_N key order (lk % 32 == 0, ldv >= lk): what sd_attention_wide_f16 reads."""
    lk = v.shape[1]
    assert lk % 32 == 0 and ldv >= lk and ldv % 8 == 0
    src = torch.arange(ldv)
    src[:lk] = perm32_source(lk)
    return _pack_vt(v, ldv, src)


def new_out(B, lq, ldo):
    """`out` [B, lq, ldo] + GUARD, every half the sentinel NaN."""
    return kit.sentinel(B * lq * ldo + GUARD, F16)


def split_out(buf, B, lq, C, ldo):
    """-> (written region [B, lq, C] fp16, bits of everything else as one int16 vector: gap columns C .. ldo-1 and the guard)."""
    bits = buf.cpu().view(torch.int16)
    body = bits[:B * lq * ldo].view(B, lq, ldo)
    rest = torch.cat([body[:, :, C:].reshape(-1), bits[B * lq * ldo:]])
    return body[:, :, :C].contiguous().view(F16), rest


# ---------------------------------------------------------------------------------------------------------------- the case table
class Case(NamedTuple):
    family: str                 # generic | strided | pipelined | qt2 | stress | wide   (the pools DESIGN.md reports)
    kind: str                   # generic: sd_attention_f16, library's own kernel choice; sp: the pipelined kernel forced; wide: sd_attention_wide_f16
    d: int
    B: int
    H: int
    lq: int
    lk: int
    vt: str                     # plain | perm16 | perm32
    ld: str                     # dense | fused (unet.py: q, k in one [B, L, 2C] buffer) | fusedx (fused, ldv one group up, ldo = C + 8)
    #                             | mixed (q at column offset 8 with ldq = C + 16, ldk = C + 8, ldo = C + 8, ldv one group up)
    data: str = "randn"         # randn | jump | nudge | low   (make_inputs)
    slices: Optional[Tuple[Tuple[int, int], ...]] = None       # (batch, head) pairs compared with the reference; None = all

    @property
    def id(self):
        s = f"{self.kind}-d{self.d}-b{self.B}h{self.H}-q{self.lq}k{self.lk}-{self.vt}-{self.ld}"
        return s if self.data == "randn" else f"{s}-{self.data}"

    @property
    def C(self):
        return self.H * self.d

    def leading_dims(self):
        """-> dict(ldq, ldk, ldv, ldo, qcol0)."""
        C, g = self.C, {"plain": 8, "perm16": 16, "perm32": 64}[self.vt]
        ldv_min = self.lk if self.vt == "perm32" else roundup(self.lk, g)
        if self.ld == "dense":
            return dict(ldq=C, ldk=C, ldv=ldv_min, ldo=C, qcol0=0)
        if self.ld == "fused":
            return dict(ldq=2 * C, ldk=2 * C, ldv=ldv_min, ldo=C, qcol0=0)
        if self.ld == "fusedx":
            return dict(ldq=2 * C, ldk=2 * C, ldv=ldv_min + g, ldo=C + 8, qcol0=0)
        assert self.ld == "mixed"
        return dict(ldq=C + 16, ldk=C + 8, ldv=ldv_min + g, ldo=C + 8, qcol0=8)

    def compared(self):
        return self.slices if self.slices is not None else tuple((b, h) for b in range(self.B) for h in range(self.H))


def generic_instantiation(d, B, H, lq, lk):
    """attention_kernel<KS, DVT, QT, ONES> a launch of sd_attention_f16 lands in: a transcript of the dispatch at the end of
    coma_amd/csrc/sd_attention.hip (the pipelined kernel aside), kept beside the table so that the table can be checked to reach all ten."""
    blocks256 = B * H * ((lq + 255) // 256)
    two80 = d == 80 and lq >= 1024 and lk >= 256 and blocks256 >= 512
    two = (lq >= 1024 and d == 40 and lk > 128) or two80
    if d == 40:
        return (3, 2, 2, 40) if two else (3, 2, 1, 40)
    if d <= 48:
        return (3, 2, 1, -1)
    if d <= 64:
        return (4, 2, 1, -1)
    if d == 80:
        return (5, 3, 2, 80) if two80 else (5, 3, 1, 80)
    if d <= 80:
        return (5, 3, 1, -1)
    if d <= 96:
        return (6, 3, 1, -1)
    if d <= 128:
        return (8, 4, 1, -1)
    return (10, 5, 1, -1)


ALL_INSTANTIATIONS = {(3, 2, 1, 40), (3, 2, 2, 40), (3, 2, 1, -1), (4, 2, 1, -1), (5, 3, 1, -1), (5, 3, 1, 80), (5, 3, 2, 80), (6, 3, 1, -1),
                      (8, 4, 1, -1), (10, 5, 1, -1)}

# Query blocks are 128 queries (QT = 1), key tiles 64 keys: (1, 1) and (33, 7) one ragged tile only (lk < 8: a single 16-byte V^T chunk),
# (32, 64) exactly one full tile, (129, 65) full + ragged tile and a second query block holding ONE query, (127, 200) several tiles.
GENERIC_SHAPES = ((1, 1), (33, 7), (32, 64), (129, 65), (127, 200))


def _build_cases():
    cases = []
    # ---- generic kernel, every accepted head dim, both V^T layouts; batch 2 x 3 heads: h * d is no multiple of 64.
    #   d =   8 .. 32, 48   attention_kernel<3, 2, 1, -1>    one K panel, VALU denominator, K chunks 1-5 / V^T rows beyond d out of range
    #   d =  40             attention_kernel<3, 2, 1, 40>    ones row at V^T row 40
    #   d =  56, 64         attention_kernel<4, 2, 1, -1>    one K panel, full at d = 64
    #   d =  72             attention_kernel<5, 3, 1, -1>    two K panels, the second holds one chunk
    #   d =  80             attention_kernel<5, 3, 1, 80>    ones row at V^T row 80
    #   d =  88, 96         attention_kernel<6, 3, 1, -1>    two K panels
    #   d = 104 .. 128      attention_kernel<8, 4, 1, -1>    two K panels, full at d = 128
    #   d = 136 .. 160      attention_kernel<10, 5, 1, -1>   three K panels, the third partly out of range
    # (<3, 2, 2, 40> and <5, 3, 2, 80>: the qt2 family below.)  Every instantiation runs as VPERM = false (plain) and true (perm16).
    for d in range(8, 161, 8):
        for lq, lk in GENERIC_SHAPES:
            for vt in ("plain", "perm16"):
                cases.append(Case("generic", "generic", d, 2, 3, lq, lk, vt, "dense"))
    # ---- strided operands: d = 40 / 80 / 160 (the UNet's) and one d of each instantiation no operator test ran before
    #      (24 -> <3,2,1,-1>, 72 -> <5,3,1,-1>, 96 -> <6,3,1,-1>, 112 -> <8,4,1,-1>).  fused: L = 129 (two full key tiles + one key);
    #      mixed: ldq != ldk, q at a column offset, ldo = C + 8, ldv one group above the minimum.
    for d in (40, 80, 160, 24, 72, 96, 112):
        cases.append(Case("strided", "generic", d, 2, 3, 129, 129, "perm16", "fused"))
        cases.append(Case("strided", "generic", d, 2, 3, 129, 129, "plain", "fused"))
        cases.append(Case("strided", "generic", d, 2, 3, 129, 65, "perm16", "mixed"))
        cases.append(Case("strided", "generic", d, 2, 3, 129, 65, "plain", "mixed"))
    # ---- attention_sp_kernel<1>, forced: 2, 3 and 4 key tiles against its three LDS stages; 256 queries per block
    for L in (128, 192, 256):
        cases.append(Case("pipelined", "sp", 40, 2, 3, L, L, "perm16", "fused"))
    for lk in (128, 192, 256):
        for lq in (77, 256, 300):
            cases.append(Case("pipelined", "sp", 40, 2, 3, lq, lk, "perm16", "mixed"))
    # ---- 64 queries per wave (QT = 2, 256-query blocks), ragged last block of 6 queries
    cases.append(Case("qt2", "generic", 40, 2, 3, 1030, 136, "perm16", "dense"))           # attention_kernel<3, 2, 2, 40, true>
    cases.append(Case("qt2", "generic", 40, 2, 3, 1030, 136, "plain", "dense"))            # attention_kernel<3, 2, 2, 40, false>
    s80 = ((0, 0), (0, 7), (6, 3), (12, 0), (12, 7))
    cases.append(Case("qt2", "generic", 80, 13, 8, 1030, 264, "perm16", "dense", slices=s80))   # <5, 3, 2, 80, true>: 13 * 8 * 5 = 520 >= 512 blocks
    cases.append(Case("qt2", "generic", 80, 13, 8, 1030, 264, "plain", "dense", slices=s80))    # <5, 3, 2, 80, false>
    # ---- softmax state of the generic kernel: ones-row denominator (d = 40) and VALU sum (d = 64); 3 full key tiles + 8 keys
    for d in (40, 64):
        for data in ("jump", "nudge", "low"):
            cases.append(Case("stress", "generic", d, 1, 2, 100, 200, "perm16", "dense", data=data))
    # ---- wide kernel: attention_wide_kernel<4 / 8 / 16, 4> below 256 blocks of 128 queries, <.., 8> from there on
    for d in (128, 256, 512):
        cases.append(Case("wide", "wide", d, 2, 2, 64, 64, "perm32", "fusedx"))                # a single key tile
        for lq in (1, 63, 65, 200):
            cases.append(Case("wide", "wide", d, 2, 2, lq, 128, "perm32", "mixed"))            # lq != lk, NW = 4
        sw = ((0, 0), (0, 3), (31, 2), (63, 0), (63, 3))
        cases.append(Case("wide", "wide", d, 64, 4, 100, 64, "perm32", "dense", slices=sw))    # NW = 8: 64 * 4 * 1 = 256 blocks, 100 of 128 queries
    return tuple(cases)


CASES = _build_cases()


@functools.lru_cache(maxsize=2)
def _inputs(d, B, H, lq, lk, data):
    g = kit.gen(repr((d, B, H, lq, lk, data)))
    C = H * d
    q, k, v = (torch.randn(B, n, C, generator=g).to(F16) for n in (lq, lk, lk))
    scale = d ** -0.5
    if data == "jump":
        # a dominant key arrives in the third key tile: the running maximum jumps by far more than the 6-unit rescale threshold
        for h in range(H):
            cs = slice(h * d, (h + 1) * d)
            k[0, 150, cs] = q[0, 7, cs] * 6.0
            k[0, 160, cs] = q[0, 40, cs] * 9.0
    elif data == "nudge":
        # flat scores, then key 150 (third tile) lifts every query's maximum by ~5.5 log2 units: below the threshold, so the running
        # maximum stays and the weight of that key is ~2^5.5
        q, k = (q.float() * 0.25).to(F16), (k.float() * 0.25).to(F16)
        for h in range(H):
            q[:, :, h * d] = 2.0
            k[:, :, h * d] = 0.0
            k[:, 150, h * d] = 5.5 / (2.0 * scale * LOG2E)
    elif data == "low":
        # every score of every query is near -60: the first tile must set the maximum although nothing is above zero
        for h in range(H):
            q[:, :, h * d] = 4.0
            k[:, :, h * d] = -60.0 / (4.0 * scale)
    else:
        assert data == "randn"
    return q, k, v


def make_inputs(c: Case):
    """q [B, lq, C], k, v [B, lk, C] fp16 on the CPU; a function of the shape and the data kind only (not of layout or strides)."""
    return _inputs(c.d, c.B, c.H, c.lq, c.lk, c.data)


def select(x, pairs, d):
    """x [B, L, H*d] -> [len(pairs), L, d]: the (batch, head) slices as a batch of one-head problems."""
    return torch.stack([x[b, :, h * d:(h + 1) * d] for b, h in pairs])


class Yardstick(NamedTuple):
    ref: torch.Tensor           # float64 [S, lq, d], S = len(case.compared())
    e_emu: float                # max over the compared queries of the emulation's normalised error
    bound: float                # device_bound(e_emu)


@functools.lru_cache(maxsize=2)
def _yardstick(d, B, H, lq, lk, data, pairs, round_q):
    q, k, v = _inputs(d, B, H, lq, lk, data)
    qs, ks, vs = (select(t, pairs, d) for t in (q, k, v))
    ref = attention_f64(qs, ks, vs, 1, d ** -0.5)
    emu = attention_fp16_emulation(qs, ks, vs, 1, d ** -0.5, round_q=round_q)
    e = float(query_error(emu, ref, 1).max())
    return Yardstick(ref, e, device_bound(e))


def yardstick(c: Case) -> Yardstick:
    """Reference, e_emu and the device bound of a case -- computed on the CPU, the same wherever it runs."""
    return _yardstick(c.d, c.B, c.H, c.lq, c.lk, c.data, c.compared(), c.kind == "sp")
