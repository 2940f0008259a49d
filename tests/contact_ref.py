"""coma_contact_accumulate_f32 (coma_amd/csrc/contact.hip, K1 + K2 + K3) over the domain its argument checks accept.  CPU only: the table
of launches (CASES), the operands and the first contents of the in/out state (data), the reference in NumPy written from the reference's
formulas as oracle/coma_oracle.py restates them (reference), the kernel's own arithmetic (emulate), what a case reaches (branches), the
assertions the device is held to (check) and every argument check (REFUSALS).  tests/test_coma_core_domain_gpu.py launches the table;
tests/test_coma_core_ref_host.py checks the table itself.

Reference: distance and threshold test in the reference's f32 sequence (sub, square, (x + y) + z, correctly rounded sqrt); K2 the literal
f32 formula, incomplete skew matrix and `1 + c < eps` mirror branch included; the scores in f64 on the f64 sphere grid, added sample by
sample into the f32 state (f32(f64(state) + score), as an in-place add of an f64 array into an f32 one does).
Emulation: f32 sphere grid; the dot product and the degree-7 interpolant as fused multiply-adds, sqrt(|1 - |x||) standing in for the clip;
exp2 of theta^2 cexp + 64 (results below 2^-126 flushed); f32 accumulation over all samples of the call in sample order; one 2^-64 rescale,
one read-modify-write into the state; nom and cnt as lane partials over the eight sample slots, then the xor butterfly.

The bound.  cnt and den: bit for bit.  nom and the two histograms: max(4 e_emu, floor), e_emu what emulate() loses against reference() on
the same case.  Histograms in two measures: per row relative to the row's largest reference value, and per bin relative for every bin
whose reference value is a normal f32.  The floors are counted roundings times the f32 unit roundoff U32 = 2^-24:
  nom        (S + 6) U32 of |nom0| + sum of the terms: S additions of the partial sums and the butterfly, the division d / size (1), expf (2),
             the final add (1), the reference's own rounding of exp (1), one spare;
  hist, row  (S + 8) U32 of the row's largest value: S additions into the accumulator, the rescale and the read-modify-write (2), exp2 (1),
             the three roundings of x and two of theta seen through d w / d theta <= 1 at the row's largest bins (5);
  hist, bin  (S + 8 + 4 ln2 (E + 64)) U32 of the bin: as above, plus the exponent argument theta^2 cexp + 64 -- magnitude up to E + 64 with
             E = min(213, pi^2 log2(e) / sigma^2), the largest exponent that still gives a non-zero weight -- whose four roundings (theta^2
             twice, the product, the sum) each move w by ln2 (E + 64) U32 relative.
A bin whose reference value is at least 4 x the smallest f32 denormal is non-zero on the device (asserted where the state starts at zero)."""
import functools
import math

import numpy as np

from oracle import coma_oracle as orc
from tests import domain_kit as kit
from tests.domain_kit import PTR, U32

f32, f64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
PT, SC, WAVE, NB = 8, 8, 64, 4          # pairs per wave, sample slots, lanes, bins per lane (contact.hip)
CHUNK = NB * WAVE
TINY, DENORM = float(np.finfo(f32).tiny), 2.0 ** -149
EPS = 1e-8
SIZE, THRES = 0.5, 0.35                 # spatial_grid_size, spatial_grid_thres of every case


class Case:
    def __init__(self, id, H, O, N, S, stride, sigma, p=(0.0, 0.0, 1.0), state="random", special=False, straddle=False):
        self.id, self.H, self.O, self.N, self.S, self.sigma, self.p, self.state = id, H, O, N, S, sigma, p, state
        self.stride, self.special, self.straddle = (3 * O if stride else 0), special, straddle
        self.sp = (0.0, 1.0, 0.0) if p == (0.0, 0.0, 1.0) else (1.0, 0.0, 0.0)

    def __repr__(self):
        return self.id


PQ = (0.0, 0.6, 0.8)
CASES = [
    Case("contact-ho1-n1-s1", 1, 1, 1, 1, 0, 0.2, state="zero"),
    Case("contact-ho7-n63-s7", 7, 1, 63, 7, 1, 0.05),
    Case("contact-ho8-n64-s8-zero", 2, 4, 64, 8, 0, 0.25, state="zero"),
    Case("contact-ho9-n65-s9-special", 3, 3, 65, 9, 1, 2.0, p=PQ, special=True),
    Case("contact-ho31-n255-s17", 31, 1, 255, 17, 0, 0.2),
    Case("contact-ho32-n256-s1-zero", 4, 8, 256, 1, 1, 0.05, state="zero"),
    Case("contact-ho33-n257-s9-special", 11, 3, 257, 9, 0, 0.25, p=PQ, special=True),
    Case("contact-ho63-n513-s8", 9, 7, 513, 8, 0, 2.0),
    Case("contact-ho15-n100-s300", 3, 5, 100, 300, 1, 0.2),
    Case("contact-ho9-n65-s0", 3, 3, 65, 0, 1, 0.2),
    Case("contact-ho20-n64-s8-special-zero", 4, 5, 64, 8, 1, 0.05, special=True, state="zero"),
    Case("contact-ho13-n8-s2-straddle", 13, 1, 8, 2, 0, 0.2, straddle=True),
]
BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------------------------------ f32 pieces (K1, K2)
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def unit(v, eps):
    with np.errstate(all="ignore"):
        return v / (np.sqrt(dot3(v, v)) + f32(eps))[..., None]


def canon(a, b, p, sp, eps):
    """canonicalize_a_wrt_b_to_p for pairs (a, b) [..., 3] f32, the literal f32 formula: the incomplete skew matrix, the mirror branch"""
    assert a.dtype == b.dtype == p.dtype == sp.dtype == f32
    z = f32(0.0)
    with np.errstate(all="ignore"):
        c, ab, ap, asp = dot3(b, p), dot3(a, b), dot3(a, p), dot3(a, sp)
        v = np.stack([(b[..., 0] * p[0] + (-b[..., 2]) * p[1]) + b[..., 1] * p[2], (b[..., 2] * p[0] + z * p[1]) + (-b[..., 0]) * p[2],
                      ((-b[..., 1]) * p[0] + z * p[1]) + z * p[2]], -1)
        av = dot3(a, v)
        opc = f32(1.0) + c
        mirror = (f32(2.0) * asp)[..., None] * sp - a
        gen = (((v * av[..., None]) / opc[..., None] + c[..., None] * a) + ab[..., None] * p) - ap[..., None] * b
        f = np.where((opc < f32(eps))[..., None], mirror, gen)
        return (f / np.sqrt(dot3(f, f))[..., None]).astype(f32), opc


def unit_vec(v, eps=EPS):
    return unit(np.asarray(v, f32), eps)


# ------------------------------------------------------------------------------------------------------------------ operands
def _ulps(x, k):
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(INF if k > 0 else -INF))
    return x


def _perp(p):
    t = np.cross(p, np.array([1.0, 0.0, 0.0]) if abs(p[0]) < 0.9 else np.array([0.0, 1.0, 0.0]))
    return t / np.linalg.norm(t)


@functools.lru_cache(maxsize=None)
def data(cid):
    c = BY_ID[cid]
    rng = kit.rng(c.id)
    S, H, O, N = c.S, c.H, c.O, c.N
    So = S if c.stride else min(S, 1)
    hv = rng.uniform(-0.3, 0.3, (S, H, 3)).astype(f32)
    ov = rng.uniform(-0.3, 0.3, (So, O, 3)).astype(f32)
    nrm = lambda *s: (lambda v: (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32))(rng.normal(size=s + (3,)))
    hn, on = nrm(S, H), nrm(So, O)
    p64 = np.array(c.p) / np.linalg.norm(c.p)
    if c.special and S:
        on[:, 0] = (-unit_vec(c.p)).astype(f32)                                          # exactly antiparallel: the mirror branch (c1)
        for s in range(So):                                                              # 1 + c = a few f32 ulps: tiny, but not below eps
            on[s, 1] = (-p64 + math.sqrt(2.0 * (2 + s % 4)) * 2.0 ** -12 * _perp(p64)).astype(f32)
        hn[:, 0] = (-unit_vec(c.p)).astype(f32)                                          # the mirror branch of c2
        hn[:, 2] *= f32(3.7)                                                             # un-normalised
        on[:, 2] *= f32(0.01)
        hn[0, 1] = 0.0                                                                   # a zero normal: NaN in both histograms of the pairs of h = 1
        hv[0, 2, 1] = INF                                                                # non-finite coordinates: cnt unchanged, nom as the reference
        if H > 3:
            hv[min(1, S - 1), 3, 0] = NAN
    if c.straddle:                                                                       # d = thres + k ulps, k = -6 .. 6: k = 0 is equal, not below
        ov[:] = 0.0
        for h in range(H):
            hv[:, h] = (_ulps(THRES, h - 6), 0.0, 0.0)
            hv[1, h] = (0.0, 0.0, -_ulps(THRES, 6 - h))
    grid64 = orc.fibonacci_sphere(N)
    if c.state == "zero":
        P1, P2 = np.zeros((H * O, N), f32), np.zeros((H * O, N), f32)
        nom, den, cnt = (np.zeros(H * O, f32) for _ in range(3))
    else:
        P1, P2 = rng.uniform(0.0, 2.0, (H * O, N)).astype(f32), rng.uniform(0.0, 2.0, (H * O, N)).astype(f32)
        nom, den, cnt = rng.uniform(0.0, 5.0, H * O).astype(f32), rng.integers(0, 40, H * O).astype(f32), rng.integers(0, 40, H * O).astype(f32)
    return dict(hv=hv, hn=hn, ov=ov, on=on, grid64=grid64, grid=grid64.astype(f32), p=np.array(c.p, f32), sp=np.array(c.sp, f32),
                state=dict(P1=P1, P2=P2, nom=nom, den=den, cnt=cnt))


def _pairs(c, d, tile_h_from_first=False, slots_past_s=False):
    """the per-(sample, pair) scalars of K1 and K2 -> dist [S, M] f32, c1, c2 [S, M, 3] f32, opc1, opc2"""
    M = c.H * c.O
    m = np.arange(M)
    h, o = m // c.O, m % c.O
    if tile_h_from_first:
        h = np.minimum((m // PT * PT) // c.O, c.H - 1)
    so = (np.arange(c.S) if c.stride else np.zeros(c.S, int))
    hv, hn = d["hv"][:, h], d["hn"][:, h]
    ov, on = d["ov"][so][:, o], d["on"][so][:, o]
    with np.errstate(all="ignore"):
        df = hv - ov
        dist = np.sqrt((df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2])
    p, sp = unit_vec(d["p"]), unit_vec(d["sp"])
    a, b = unit(hn, EPS), unit(on, EPS)
    c1, o1 = canon(a, b, p, sp, EPS)
    c2, o2 = canon(b, a, p, sp, EPS)
    return dist, c1, c2, o1, o2


def _terms(dist):
    with np.errstate(all="ignore"):
        return kit.exp32(-dist / f32(SIZE)), (dist < f32(THRES)).astype(f32)


# ------------------------------------------------------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def reference(cid):
    c, d = BY_ID[cid], data(cid)
    st = d["state"]
    dist, c1, c2, _, _ = _pairs(c, d)
    term, below = _terms(dist)
    out = {k: v.copy() for k, v in st.items()}
    norm_nom = np.abs(st["nom"]).astype(f64)
    for s in range(c.S):
        out["cnt"] = out["cnt"] + below[s]
        out["nom"] = out["nom"] + term[s]
        out["den"] = out["den"] + f32(1.0)
        with np.errstate(invalid="ignore"):
            norm_nom = norm_nom + np.abs(term[s].astype(f64))
        for name, cn in (("P1", c1), ("P2", c2)):
            with np.errstate(all="ignore"):
                score = orc.geodesic_gaussian(d["grid64"], cn[s][None], c.sigma, EPS)[0]          # [M, N] f64
                out[name] = (out[name].astype(f64) + score).astype(f32)
    out["norm_nom"] = norm_nom
    return out


# ------------------------------------------------------------------------------------------------------------------ the emulation
MUTATIONS = ("bias-dropped", "ragged-chunk-written-past-n", "tile-h-from-first-pair", "slot-past-s-counted", "nom-by-every-chunk")
COEF = [f32(v) for v in (-0.001211737748235464, 0.006491521373391151, -0.01684105210006237, 0.03072212263941765, -0.05011430382728577,
                         0.08896885067224503, -0.214598149061203, 1.570796251296997)]
PI = f32(3.14159265358979323846)


def fma(a, b, c):
    """a * b + c with one rounding to f32 (through f64: the product is exact there; the second rounding is off by an ulp once in ~2^29)"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def bin_weight(grid, cn, cexp, bias=f32(64.0)):
    """grid [N, 3] f32, cn [..., 3] f32 -> 2^bias w [..., N] f32 as bin_weight2 computes it"""
    g = lambda k: grid[:, k]
    cc = lambda k: cn[..., k, None]
    with np.errstate(all="ignore"):
        x = fma(g(2), cc(2), fma(g(1), cc(1), g(0) * cc(0)))
        ax = np.abs(x)
        t = f32(1.0) - ax
        r = np.broadcast_to(COEF[0], ax.shape)
        for k in COEF[1:]:
            r = fma(r, ax, k)
        s = np.sqrt(np.abs(t))
        u = fma(s, r, f32(-0.5) * PI)
        th = fma(np.copysign(f32(1.0), x), u, f32(0.5) * PI)
        e = fma(th * th, cexp, bias)
        w = np.exp2(e.astype(f64))
        w = np.where(w < TINY, 0.0, w).astype(f32)                       # v_exp_f32 flushes a denormal result
    return w


def emulate(cid, mut=None):
    """-> the five outputs as flat f32 arrays; P1 / P2 carry a tail of CHUNK sentinels behind the last row (what a write past N lands in)"""
    assert mut is None or mut in MUTATIONS
    c, d = BY_ID[cid], data(cid)
    st = d["state"]
    M, N, S = c.H * c.O, c.N, c.S
    out = {k: v.copy() for k, v in st.items()}
    out["P1"], out["P2"] = (np.concatenate([st[k].reshape(-1), kit.sentinel(CHUNK, f32)]) for k in ("P1", "P2"))
    if S == 0:
        return out
    dist, c1, c2, _, _ = _pairs(c, d, tile_h_from_first=mut == "tile-h-from-first-pair")
    term, below = _terms(dist)
    # nom / cnt: lane partials over the eight sample slots (slot = sample % 8), then the xor butterfly over the slot index
    slots = S + (-S % SC) if mut == "slot-past-s-counted" else S                       # a slot past S reads a sample again
    idx = np.arange(slots) % S
    def slot_sum(x):
        part = np.zeros((SC, M), f32)
        for j in range(SC):
            rows = x[idx[j::SC]]
            part[j] = np.add.accumulate(rows, axis=0, dtype=f32)[-1] if len(rows) else f32(0.0)
        for bit in (1, 2, 4):
            part = part + part[np.arange(SC) ^ bit]
        return part[0]
    chunks = -(-N // CHUNK)
    times = chunks if mut == "nom-by-every-chunk" else 1
    with np.errstate(invalid="ignore"):
        for _ in range(times):
            out["nom"] = out["nom"] + slot_sum(term)
            out["cnt"] = out["cnt"] + slot_sum(below)
            out["den"] = out["den"] + f32(S)
    # K3
    cexp = f32(-1.4426950408889634 / (f64(f32(c.sigma)) * f64(f32(c.sigma))))
    bias = f32(0.0) if mut == "bias-dropped" else f32(64.0)
    grid = d["grid"]
    if mut == "ragged-chunk-written-past-n":                                          # the bins of the last chunk past N exist: grid 0, weight of theta = pi / 2
        grid = np.concatenate([grid, np.zeros((chunks * CHUNK - N, 3), f32)])
    NN = len(grid)
    for name, cn in (("P1", c1), ("P2", c2)):
        with np.errstate(all="ignore"):
            acc = np.add.accumulate(bin_weight(grid, cn, cexp, bias), axis=0, dtype=f32)[-1]    # [M, NN], sample order
            add = acc * f32(2.0 ** -64) if mut != "bias-dropped" else acc
        flat = out[name]
        for m in range(M):
            lim = min(NN, len(flat) - m * N)
            with np.errstate(invalid="ignore"):
                keep = kit.bits(flat[m * N:m * N + lim]) == kit.sentinel_bits(f32)
                new = flat[m * N:m * N + lim] + add[m, :lim]
            new[keep & (np.arange(lim) >= N)] = add[m, :lim][keep & (np.arange(lim) >= N)]   # (the sentinel is a NaN: show the write)
            flat[m * N:m * N + lim] = new
    return out


# ------------------------------------------------------------------------------------------------------------------ regimes
REACHABLE = {f"pairs%8={k}" for k in (0, 1, 7)} | {f"pairs%32={k}" for k in (0, 1, 31)} | {"tile-spans-two-h", "one-tile", "second-workgroup"} \
    | {f"N%64={k}" for k in (0, 1, 63)} | {"one-chunk", "two-chunks", "three-chunks", "ragged-last-chunk", "full-chunk"} \
    | {f"S%8={k}" for k in (0, 1, 7)} | {"S=0", "S-one-chunk", "S-many-chunks", "S-hundreds", "stride-0", "stride-3O", "state-zero", "state-random",
                                         "K2-mirror", "K2-general", "K2-tiny-opc", "zero-normal-nan", "nonfinite-vertex", "unnormalised-normal", "p-is-z", "p-not-z",
                                         "denormal-bins", "flushed-weights", "antipodal-bin-significant", "d-equals-thres", "d-within-6-ulps-below", "d-within-6-ulps-above",
                                         "sigma-0.05", "sigma-0.2", "sigma-0.25", "sigma-2"}


@functools.lru_cache(maxsize=None)
def branches(cid):
    c, d = BY_ID[cid], data(cid)
    M, N, S = c.H * c.O, c.N, c.S
    b = {f"sigma-{c.sigma:g}", "stride-3O" if c.stride else "stride-0", f"state-{c.state}", "p-is-z" if c.p == (0.0, 0.0, 1.0) else "p-not-z"}
    if S == 0:
        return b | {"S=0"}
    for mod, ks in ((8, (0, 1, 7)), (32, (0, 1, 31))):
        if M % mod in ks:
            b.add(f"pairs%{mod}={M % mod}")
    if N % 64 in (0, 1, 63):
        b.add(f"N%64={N % 64}")
    if S % 8 in (0, 1, 7):
        b.add(f"S%8={S % 8}")
    if M <= PT:
        b.add("one-tile")
    if M > 4 * PT:
        b.add("second-workgroup")
    if any((t * PT) // c.O != min(t * PT + PT - 1, M - 1) // c.O for t in range(-(-M // PT))):
        b.add("tile-spans-two-h")
    chunks = -(-N // CHUNK)
    b |= {{1: "one-chunk", 2: "two-chunks", 3: "three-chunks"}[chunks], "ragged-last-chunk" if N % CHUNK else "full-chunk"}
    b.add("S-one-chunk" if S <= SC else "S-many-chunks")
    if S >= 200:
        b.add("S-hundreds")
    dist, c1, c2, o1, o2 = _pairs(c, d)
    opc = np.concatenate([o1.reshape(-1), o2.reshape(-1)])
    if (opc < f32(EPS)).any():
        b.add("K2-mirror")
    if (opc >= f32(EPS)).any():
        b.add("K2-general")
    if ((opc >= f32(EPS)) & (opc < 1e-6)).any():
        b.add("K2-tiny-opc")
    if np.isnan(c1).any() and (d["hn"] == 0).all(-1).any():
        b.add("zero-normal-nan")
    if not np.isfinite(d["hv"]).all():
        b.add("nonfinite-vertex")
    n = np.sqrt((d["hn"].astype(f64) ** 2).sum(-1))
    if (np.abs(n[n > 0] - 1) > 0.5).any():
        b.add("unnormalised-normal")
    ref = reference(cid)
    if c.state == "zero":
        for k in ("P1", "P2"):
            r = ref[k]
            if ((r >= 4 * DENORM) & (r < TINY)).any():
                b.add("denormal-bins")
            if (r == 0).any():
                b.add("flushed-weights")
    if c.sigma >= 2.0:
        b.add("antipodal-bin-significant")
    t = f32(THRES)
    for k in range(1, 7):
        if (dist == _ulps(t, -k)).any():
            b.add("d-within-6-ulps-below")
        if (dist == _ulps(t, k)).any():
            b.add("d-within-6-ulps-above")
    if (dist == t).any():
        b.add("d-equals-thres")
    return b


# ------------------------------------------------------------------------------------------------------------------ the bound
class Fig:
    def __init__(self, e_emu, floor, err=None):
        self.e_emu, self.floor, self.bound, self.err = e_emu, floor, max(4 * e_emu, floor), err


def floors(c):
    E = min(213.0, math.pi ** 2 * 1.4426950408889634 / c.sigma ** 2)
    return dict(nom=(c.S + 6) * U32, row=(c.S + 8) * U32, bin=(c.S + 8 + 4 * math.log(2.0) * (E + 64.0)) * U32)


def errors(c, got):
    """the three measured errors of `got` (name -> flat array, tails allowed) against the reference, over what is compared; NaN-ness must agree
    -> dict(nom, row, bin), and the number of elements left out of the comparison / compared"""
    ref = reference(c.id)
    M, N = c.H * c.O, c.N
    out, skipped, total = dict(nom=0.0, row=0.0, bin=0.0), 0, 0
    r, g = ref["nom"].astype(f64), np.asarray(got["nom"][:M]).astype(f64)
    assert np.array_equal(np.isnan(r), np.isnan(g)), f"{c.id}: NaN-ness of nom"
    fin = np.isfinite(r)
    assert np.array_equal(r[~fin & ~np.isnan(r)], g[~fin & ~np.isnan(r)])
    if fin.any():
        out["nom"] = float((np.abs(g[fin] - r[fin]) / np.maximum(ref["norm_nom"][fin], TINY)).max())
    total += M
    for name in ("P1", "P2"):
        r, g = ref[name].astype(f64), np.asarray(got[name][:M * N]).reshape(M, N).astype(f64)
        assert np.array_equal(np.isnan(r), np.isnan(g)), f"{c.id}: NaN-ness of {name}"
        nan_row = np.isnan(r).any(1)
        assert np.array_equal(np.isnan(r).all(1), nan_row)                             # a NaN row is NaN throughout: compared for NaN-ness, not left out
        rr, gg = r[~nan_row], g[~nan_row]
        total += r.size
        if not rr.size:
            continue
        top = np.abs(rr).max(1, keepdims=True)
        zero = top[:, 0] == 0
        assert np.array_equal(gg[zero], rr[zero])
        if (~zero).any():
            out["row"] = max(out["row"], float((np.abs(gg - rr)[~zero] / top[~zero]).max()))
        normal = np.abs(rr) >= TINY
        skipped += int((~normal & (rr != 0)).sum())                                    # denormal bins: held by the row measure and the denormal promise
        if normal.any():
            out["bin"] = max(out["bin"], float((np.abs(gg - rr)[normal] / np.abs(rr)[normal]).max()))
    return out, skipped, total


@functools.lru_cache(maxsize=None)
def yardstick(cid):
    c = BY_ID[cid]
    e, skipped, total = errors(c, emulate(cid))
    return {k: Fig(e[k], floors(c)[k]) for k in e}, skipped, total


def check(c, got, start=None):
    """the assertions the device is held to -> name -> Fig.  got: name -> flat f32 array (a tail behind P1 / P2 is allowed and must still
    hold the sentinel)"""
    ref, d = reference(c.id), data(c.id)
    M, N = c.H * c.O, c.N
    for k in ("cnt", "den"):
        assert np.array_equal(kit.bits(np.asarray(got[k][:M])), kit.bits(ref[k])), f"{c.id}: {k} differs from the reference's bits"
    for k in ("P1", "P2"):
        tail = np.asarray(got[k][M * N:])
        assert bool((kit.bits(tail) == kit.sentinel_bits(f32)).all()), f"{c.id}: {k} written past the last row"
    if c.S == 0:
        for k in ("P1", "P2", "nom"):
            assert np.array_equal(kit.bits(np.asarray(got[k][:d["state"][k].size])), kit.bits(d["state"][k].reshape(-1))), f"{c.id}: S = 0 wrote {k}"
        return {}
    fig, _, _ = yardstick(c.id)
    e, _, _ = errors(c, got)
    out = {}
    for k in ("nom", "row", "bin"):
        f = Fig(fig[k].e_emu, fig[k].floor, e[k])
        out[k] = f
        assert f.err <= f.bound, f"{c.id}: {k} error {f.err:.3e} > bound {f.bound:.3e} (e_emu {f.e_emu:.3e}, floor {f.floor:.3e})"
    if c.state == "zero":                                                              # the denormal promise
        for k in ("P1", "P2"):
            r, g = ref[k].reshape(-1), np.asarray(got[k][:M * N])
            lost = (r >= 4 * DENORM) & (g == 0)
            assert not lost.any(), f"{c.id}: {int(lost.sum())} bins of {k} the reference keeps (>= 4 denormals) are zero"
    return out


# ------------------------------------------------------------------------------------------------------------------ the C ABI
OUTPUT_ARGS = ("prob_h_wrt_o", "prob_o_wrt_h", "nom", "den", "cnt")
HOST_ARGS = ("principle_vec", "sub_principle_vec")
_BASE = dict(human_verts=PTR, human_normals=PTR, obj_verts=PTR, obj_normals=PTR, obj_sample_stride=0, sphere_grid=PTR, S=2, H=3, O=4, N=65,
             principle_vec=PTR, sub_principle_vec=PTR, spatial_grid_size=SIZE, spatial_grid_thres=THRES, normal_gaussian_sigma=0.2, eps=EPS,
             prob_h_wrt_o=PTR, prob_o_wrt_h=PTR, nom=PTR, den=PTR, cnt=PTR)
REFUSALS = {"coma_contact_accumulate_f32": (_BASE, [("null pointer", {k: 0}) for k, v in _BASE.items() if v is PTR] + [
    ("bad sizes", dict(S=-1)), ("bad sizes", dict(H=0)), ("bad sizes", dict(O=0)), ("bad sizes", dict(N=0)), ("bad sizes", dict(H=-3)),
    ("obj_sample_stride must be 0 or 3*O", dict(obj_sample_stride=3)), ("obj_sample_stride must be 0 or 3*O", dict(obj_sample_stride=-12)),
    ("sigma and spatial_grid_size must be > 0", dict(normal_gaussian_sigma=0.0)), ("sigma and spatial_grid_size must be > 0", dict(normal_gaussian_sigma=NAN)),
    ("sigma and spatial_grid_size must be > 0", dict(spatial_grid_size=0.0)), ("sigma and spatial_grid_size must be > 0", dict(spatial_grid_size=-1.0)),
    ("exceeds 16776960 bins", dict(N=65535 * 256 + 1)), ("exceeds 16776960 bins", dict(N=2 ** 31 - 1)),
])}
