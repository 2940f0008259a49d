"""GPU: the C = 320 row-tile kernels (sd_xfront_f16, sd_xattn_chain_f16, sd_xtail_f16) over their whole accepted domain, against the
float64 reference of tests/rowtile_ref.py (pinned to oracle.sd_oracle.transformer_ref in tests/test_host_logic.py).

Two measures per output tensor, both printed as a METRIC line (`pytest -rP`) before anything is asserted:
  * the project's bar (`close`): max |kernel - restatement| <= 4e-3 x max |restatement|, restatement = the reference with a round-to-fp16
    where the unfused launch graph stores fp16 (exact=False) -- comparable with the three one-shape tests in test_sd_ops_gpu.py;
  * per row, so that a bad tile cannot hide in a norm over 65536 rows: e_k(row) = ||kernel - truth||_2 / ||truth||_2 over the columns of
    the row, e_r(row) the same for the restatement, truth = the reference without any rounding (exact=True);
    asserted: max_row e_k <= MARGIN x max_row e_r.

MARGIN = 3: max_row e_k / max_row e_r measured on an MI355X with the kernels as they stood before this module existed, per case
(largest over the outputs of the case; e_r is 2.0e-4 ... 6.0e-4 everywhere except the mean = 10 sigma cases, 2.4e-3 ... 2.6e-3):
  xchain  64 x 24 lk 77: h2 1.00, n3 1.24, stages h1 / n2 / q2 1.00, a2 1.37      4096 x 16 lk 77: h2 0.99, n3 1.28
          192 x 3 lk 1: 1.30     128 x 2, lk 32: 1.20   lk 33: n3 1.20, a2 1.45   lk 64: 1.23   lk 65 peaked: 1.29   lk 80, ldv2 80 / 96: 1.20
          lk 77 / 70 with junk pads: 1.21 / 1.23     256 x 2 eps 1e-3: low variance 1.31, mean = 10 sigma 1.03
  xfront  (the same from both GroupNorm tables) 64 x 24: h 1.00, qk 1.10, v 1.13     4096 x 16: 1.00, 1.09, 1.12     192 x 3, ldv 208 / 256: 1.12
          3072 x 2: 1.11     256 x 2 eps 1e-3: low variance 1.10, mean = 10 sigma 1.00
  xtail   128 rows 1.37     65536 rows 1.36     4224 rows 1.38     512 rows, gate sweep 1.17
Largest 1.45 (the a2 debug stage: the kernel rounds q2 * scale * log2(e) to fp16 once more than the restatement, and the probabilities
to fp16); x 1.5 for another accumulation order and a one-ulp flip of the final fp16 rounding = 2.2, rounded up to one digit: 3.  No case
needs more.  Errors of order 1 are two to three orders of magnitude beyond it: with 81 / 96 keys, which the entry point accepted until
this module (only 80 key positions enter P.V), the same kernels gave ratios 141 / 432 on h2 and 753 / 1556 on a2; a variant that drops
the last weight K-slice of the chain's products gave 915 ... 1355, one that reads sample 0's k2 in every workgroup 636 ... 2711 (at
64 x 24 and at 4096 x 16 alike) -- the first of these two moves the whole-UNet rel-L2 to 1.9e-1, i.e. that one would also be seen there.
The 81 ... 96 key range is now refused by sd_xattn_chain_f16 (test_bad_sizes_are_refused_not_launched) and unet.py sends such contexts
down the unfused path (tests/test_sd_unet_gpu.py::test_context_longer_than_the_chain_kernel_takes_the_unfused_path).
"""
import ctypes
import functools

import pytest
import torch

from tests import domain_kit as kit
from tests import rowtile_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16
C = 320
MARGIN = 3.0
BENCH_B, BENCH_L = 16, 4096           # the benchmark's 64 x 64 level: 65536 rows


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(F16)


def dv(t):
    return t.to(DEV).contiguous()


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.sd import ops
    return ops


class Check:
    """Collects the comparisons of one case: every METRIC line is printed first, the assertions are made together at the end."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def rows(self, name, got, truth, restated, margin=None):
        got = got.detach().cpu()
        e_k, e_r = float(rr.row_error(got, truth).max()), float(rr.row_error(restated, truth).max())
        err = float((got.double() - restated).abs().max())
        lim = 4e-3 * float(restated.abs().max()) + 1e-6
        print(f"METRIC {self.case} {name}: e_k {e_k:.3e} e_r {e_r:.3e} ratio {e_k / max(e_r, 1e-300):.3f} max-abs-err {err:.3e} (bar {lim:.3e})")
        if not err <= lim:
            self.bad.append(f"{name}: max abs err {err:.3e} > {lim:.3e}")
        if not e_k <= (margin or MARGIN) * e_r:
            self.bad.append(f"{name}: per-row error {e_k:.3e} > {margin or MARGIN} x {e_r:.3e}")

    def true(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        assert not self.bad, f"{self.case}: " + "; ".join(self.bad)


# ===================================================================================================================== sd_xattn_chain_f16
def chain_inputs(B, rps, lk, kind="randn", seed=100):
    """The thirteen inputs of the chain as fp16 CPU tensors (k2, v2 [B, lk, 320], V not yet transposed).
    kind: "randn"  as test_xattn_chain_matches_the_unfused_chain_stage_by_stage;
          "lowvar" rows of h1 and h2 with sigma = 0.02 (an eps of 1e-3 decides the LayerNorm results);
          "offset" LayerNorm rows with mean = 10 sigma (h = 3 + 0.3 randn);
          "peaked" k2[b, j] = 8 x the (unit-rms) q2 row of token j: one dominant key for those queries, sharp rows elsewhere."""
    M = B * rps
    sa, sh, sb, sv = dict(randn=(1, 1, 0.1, 1), lowvar=(0.014, 0.014, 0.005, 0.02), offset=(0.1, 0.3, 0.1, 1), peaked=(1, 1, 0.1, 1))[kind]
    a, h = rnd(M, C, seed=seed + 1, scale=sa), rnd(M, C, seed=seed + 2, scale=sh)
    if kind == "offset":
        h = (h.float() + 3.0).half()
    wo1, wq, wo2 = (rnd(C, C, seed=seed + 10 + i, scale=C**-0.5) for i in range(3))
    bo1, bo2 = rnd(C, seed=seed + 20, scale=sb), rnd(C, seed=seed + 21, scale=sb)
    g2, b2, g3, b3 = (1 + rnd(C, seed=seed + 30, scale=0.1)), rnd(C, seed=seed + 31, scale=0.1), (1 + rnd(C, seed=seed + 32, scale=0.1)), \
        rnd(C, seed=seed + 33, scale=0.1)
    k2, v2 = rnd(B, lk, C, seed=seed + 40), rnd(B, lk, C, seed=seed + 41, scale=sv)
    if kind == "peaked":
        idx = (torch.arange(B)[:, None] * rps + torch.arange(lk)[None] % rps).reshape(-1)
        q2 = rr.xchain(a, h, wo1, bo1, g2, b2, wq, k2, v2, wo2, bo2, g3, b3, rows_per_sample=rps, exact=True, rows=idx)["q2"]
        k2 = (8.0 * q2 / q2.pow(2).mean(-1, keepdim=True).sqrt()).reshape(B, lk, C).half()
    return a, h, wo1, bo1, g2, b2, wq, k2, v2, wo2, bo2, g3, b3


def vt_perm16(ops, v2, ldv2):
    """[B, lk, 320] -> V^T [B, 320, ldv2] with the keys of every 16 in the PERM16 order, pad positions zero."""
    p = ops.perm16_columns(v2.transpose(1, 2).contiguous())
    vt = torch.zeros(v2.shape[0], C, ldv2, dtype=F16)
    vt[..., :p.shape[-1]] = p
    return vt


def launch_chain(ops, inp, vt2, *, rps, lk, eps=1e-5, stage=0):
    a, h, wo1, bo1, g2, b2, wq, k2, v2, wo2, bo2, g3, b3 = inp
    M = a.shape[0]
    args = [t if t.is_cuda else dv(t) for t in (a, h, wo1, bo1, g2, b2, wq, k2.reshape(-1, C), vt2, wo2, bo2, g3, b3)]
    o_h2, o_n3 = torch.zeros(M, C, dtype=F16, device=DEV), torch.zeros(M, C, dtype=F16, device=DEV)
    dbg = torch.zeros(M, C, dtype=F16, device=DEV) if stage else None
    ops.xattn_chain(*args, o_h2, o_n3, rows=M, rows_per_sample=rps, lk=lk, ldv2=vt2.shape[-1], eps=eps, debug_out=dbg, debug_stage=stage)
    return o_h2, o_n3, dbg


def run_chain_case(ops, rps, B, lk, ldv2, kind="randn", eps=1e-5, stages=False, junk=False):
    case = f"xchain rps={rps} B={B} lk={lk} ldv2={ldv2} {kind} eps={eps:g}"
    inp = chain_inputs(B, rps, lk, kind)
    truth, rest = (rr.xchain(*inp, rows_per_sample=rps, eps=eps, exact=e) for e in (True, False))
    vt2 = vt_perm16(ops, inp[8], ldv2)
    ck = Check(case)
    with kit.device_guard(case):                                # (the kit's fault policy: a launch error ends the session)
        o_h2, o_n3, _ = launch_chain(ops, inp, vt2, rps=rps, lk=lk, eps=eps)
    ck.rows("h2", o_h2, truth["h2"], rest["h2"])
    ck.rows("n3", o_n3, truth["n3"], rest["n3"])
    if stages:
        for stage, name in ((1, "h1"), (2, "n2"), (3, "q2"), (4, "a2")):
            with kit.device_guard(f"{case} stage {stage}"):
                dbg = launch_chain(ops, inp, vt2, rps=rps, lk=lk, eps=eps, stage=stage)[2]
            ck.rows(name, dbg, truth[name], rest[name])
    if junk:
        # the pad positions of vt2 belong to no key: whatever finite values they hold, the result is the same bits
        j = torch.arange(ldv2)
        pad = ((j & ~12) | ((j & 4) << 1) | ((j & 8) >> 1)) >= lk
        assert int(pad.sum()) == ldv2 - lk
        vj = vt2.clone()
        vj[:, :, pad] = torch.where(torch.arange(int(pad.sum())) % 2 == 0, 1000.0, -1000.0).to(F16)
        with kit.device_guard(case + " (junk pad)"):
            j_h2, j_n3, _ = launch_chain(ops, inp, vj, rps=rps, lk=lk, eps=eps)
        ck.true(torch.equal(j_h2, o_h2) and torch.equal(j_n3, o_n3), "junk in the pad positions of vt2 changed the result")
    ck.done()


CHAIN_CASES = [
    # rows_per_sample, samples, lk, ldv2, kind, eps, debug stages, junk pad
    (64, 24, 77, 80, "randn", 1e-5, True, False),         # a different sample, K2 and V2^T in every workgroup
    (BENCH_L, BENCH_B, 77, 80, "randn", 1e-5, False, False),   # benchmark shape: 1024 workgroups, more than are resident at once
    (192, 3, 1, 80, "randn", 1e-5, False, False),         # single key: the softmax is exactly 1, a2 = the V row
    (128, 2, 32, 80, "randn", 1e-5, False, False),        # key-tile edges
    (128, 2, 33, 80, "randn", 1e-5, True, False),
    (128, 2, 64, 80, "randn", 1e-5, False, False),
    (128, 2, 65, 80, "peaked", 1e-5, False, False),       # ... and one dominant key per query
    (128, 2, 80, 80, "randn", 1e-5, False, False),        # every fetched position live
    (128, 2, 80, 96, "randn", 1e-5, False, False),        # ldv2 above the minimum
    (128, 2, 77, 80, "randn", 1e-5, False, True),         # finite junk in the pad positions of vt2
    (128, 2, 70, 80, "randn", 1e-5, False, True),
    (256, 2, 77, 80, "lowvar", 1e-3, False, False),       # eps decides the result
    (256, 2, 77, 80, "offset", 1e-3, False, False),       # E[x^2] - mean^2 at mean = 10 sigma
]


@pytest.mark.parametrize("rps,B,lk,ldv2,kind,eps,stages,junk", CHAIN_CASES)
def test_xattn_chain_over_the_accepted_domain(ops, rps, B, lk, ldv2, kind, eps, stages, junk):
    run_chain_case(ops, rps, B, lk, ldv2, kind, eps, stages, junk)


# ========================================================================================================================== sd_xfront_f16
def front_inputs(B, L, kind="randn", seed=200):
    """kind "lowvar": rows of h with sigma = 0.02; "offset": rows of h with mean = 10 sigma (bpi = 3, proj_in scaled to 0.3)."""
    sw, sb = dict(randn=(1.0, 0.1), lowvar=(0.02, 0.005), offset=(0.3, 0.03))[kind]
    x = (rnd(B * L, C, seed=seed + 1).float() * 2 + 0.5).half()
    gng, gnb = 1 + rnd(C, seed=seed + 2, scale=0.1), rnd(C, seed=seed + 3, scale=0.1)
    wpi = rnd(C, C, seed=seed + 10, scale=sw * C**-0.5)
    wq, wk, wv = (rnd(C, C, seed=seed + 11 + i, scale=C**-0.5) for i in range(3))
    bpi = rnd(C, seed=seed + 20, scale=sb)
    if kind == "offset":
        bpi = (bpi.float() + 3.0).half()
    g1, b1 = 1 + rnd(C, seed=seed + 21, scale=0.1), rnd(C, seed=seed + 22, scale=0.1)
    return x, gng, gnb, wpi, bpi, g1, b1, wq, wk, wv


SENTINEL = 7.5


def launch_front(ops, dinp, table, *, B, L, ldv, eps):
    x, gng, gnb, wpi, bpi, g1, b1, wqk, wv = dinp
    M = B * L
    o_h, o_qk = torch.zeros(M, C, dtype=F16, device=DEV), torch.zeros(M, 2 * C, dtype=F16, device=DEV)
    o_vt = torch.full((B, C, ldv), SENTINEL, dtype=F16, device=DEV)
    ops.xfront(x, table, wpi, bpi, g1, b1, wqk, wv, o_h, o_qk, o_vt, rows=M, rows_per_sample=L, ldv=ldv, eps=eps)
    return o_h, o_qk, o_vt


def front_tables(ops, x, dx, dgng, dgnb, B, L):
    """The GroupNorm (scale, shift) table two ways: from a statistics pass over x, and from per-32-row column sums of x."""
    t_pass = torch.zeros(ops.gn_scratch_floats(B, L), dtype=torch.float32, device=DEV)
    ops.groupnorm_table(dx, dgng, dgnb, t_pass, batch=B, hw=L, c0=C, eps=1e-6)
    xs = x.double().reshape(B * L // 32, 32, C)
    cs = torch.stack([xs.sum(1), (xs * xs).sum(1)], 1).float()
    t_sums = torch.zeros_like(t_pass)
    ops.groupnorm_table(dx, dgng, dgnb, t_sums, batch=B, hw=L, c0=C, eps=1e-6, colstats0=dv(cs), rows_per_slot=32)
    return (("pass", t_pass), ("sums", t_sums))


def run_front_case(ops, L, B, ldv, kind="randn", eps=1e-5):
    case = f"xfront rps={L} B={B} ldv={ldv} {kind} eps={eps:g}"
    inp = front_inputs(B, L, kind)
    x, gng, gnb, wpi, bpi, g1, b1, wq, wk, wv = inp
    truth, rest = (rr.xfront(*inp, rows_per_sample=L, gn_eps=1e-6, eps=eps, exact=e) for e in (True, False))
    dinp = [dv(t) for t in (x, gng, gnb, wpi, bpi, g1, b1, torch.cat([wq, wk]), wv)]
    ck = Check(case)
    with kit.device_guard(case + " (tables)"):
        tables = front_tables(ops, x, dinp[0], dinp[1], dinp[2], B, L)
    for how, table in tables:
        with kit.device_guard(f"{case} [table from {how}]"):
            o_h, o_qk, o_vt = launch_front(ops, dinp, table, B=B, L=L, ldv=ldv, eps=eps)
        ck.rows(f"[table from {how}] h", o_h, truth["h"], rest["h"])
        ck.rows(f"[table from {how}] qk", o_qk, truth["qk"], rest["qk"])
        v = ops.perm16_columns(o_vt[:, :, :L].cpu()).transpose(1, 2).reshape(B * L, C)       # PERM16 is its own inverse
        ck.rows(f"[table from {how}] v", v, truth["v"], rest["v"])
        ck.true(bool((o_vt[:, :, L:] == SENTINEL).all()), "the pad columns of vt (the caller's) were written")
    ck.done()


FRONT_CASES = [
    # rows_per_sample, samples, ldv, kind, eps
    (64, 24, 64, "randn", 1e-5),          # one tile per sample: table row and V^T slab change every workgroup
    (BENCH_L, BENCH_B, BENCH_L, "randn", 1e-5),
    (192, 3, 208, "randn", 1e-5),         # ldv above the sample: the sentinel in the pad columns survives
    (192, 3, 256, "randn", 1e-5),
    (3072, 2, 3072, "randn", 1e-5),       # a 48 x 64 latent
    (256, 2, 256, "lowvar", 1e-3),        # eps decides the result
    (256, 2, 256, "offset", 1e-3),        # mean = 10 sigma rows
]


@pytest.mark.parametrize("L,B,ldv,kind,eps", FRONT_CASES)
def test_xfront_over_the_accepted_domain(ops, L, B, ldv, kind, eps):
    run_front_case(ops, L, B, ldv, kind, eps)


# =========================================================================================================================== sd_xtail_f16
def tail_inputs(M, seed=300):
    n3, h2, x = rnd(M, C, seed=seed + 1), rnd(M, C, seed=seed + 2), rnd(M, C, seed=seed + 3)
    w1, b1 = rnd(8 * C, C, seed=seed + 4, scale=C**-0.5), rnd(8 * C, seed=seed + 5, scale=0.1)
    w2, b2 = rnd(C, 4 * C, seed=seed + 6, scale=(4 * C)**-0.5), rnd(C, seed=seed + 7, scale=0.1)
    wpo, bpo = rnd(C, C, seed=seed + 8, scale=C**-0.5), rnd(C, seed=seed + 9, scale=0.1)
    return n3, h2, x, w1, b1, w2, b2, wpo, bpo


def tail_device_args(inp):
    from coma_amd.sd.weights import geglu_interleave
    n3, h2, x, w1, b1, w2, b2, wpo, bpo = inp
    w1i, b1i = geglu_interleave(w1, b1)
    return [dv(t) for t in (n3, h2, x, w1i, b1i, w2, b2, wpo, bpo)]


def launch_tail(ops, dargs, M, stats=True):
    out = torch.zeros(M, C, dtype=F16, device=DEV)
    cs = torch.zeros(M // 32, 2, C, dtype=torch.float32, device=DEV) if stats else None
    ops.xtail(*dargs, out, cs, rows=M)
    return out, cs


def check_tail(ops, ck, inp, M):
    truth, rest = (rr.xtail(*inp, exact=e) for e in (True, False))
    dargs = tail_device_args(inp)
    with kit.device_guard(ck.case):
        out, cs = launch_tail(ops, dargs, M)
    ck.rows("out", out, truth, rest)
    o = out.double().cpu().reshape(M // 32, 32, C)              # column sums of the STORED values: 32 fp32 additions of fp16 numbers
    ck.true(torch.allclose(cs[:, 0].double().cpu(), o.sum(1), rtol=1e-5, atol=1e-5), "colstats: sums")
    ck.true(torch.allclose(cs[:, 1].double().cpu(), (o * o).sum(1), rtol=1e-5, atol=1e-5), "colstats: sums of squares")
    with kit.device_guard(ck.case + " (no colstats)"):
        out2, _ = launch_tail(ops, dargs, M, stats=False)
    ck.true(torch.equal(out, out2), "out differs between the launches with and without colstats")
    return out


@pytest.mark.parametrize("M", [128, BENCH_B * BENCH_L, 33 * 128])       # one workgroup; one per CU and a second round; an odd count
def test_xtail_over_the_accepted_domain(ops, M):
    ck = Check(f"xtail rows={M}")
    check_tail(ops, ck, tail_inputs(M), M)
    ck.done()


def test_xtail_gelu_swept_over_the_gate_range(ops):
    """The GELU inside the fused kernel (not the GEMM epilogue's copy of it), as test_geglu_gelu_is_the_erf_form_to_fp16_resolution does
    it: in the first block of 128 hidden columns the value is 1 (bias only) and the gate is the swept number (n3[:, 0]), every other
    hidden column is 0; W2 averages the block (1 / 128: exact), Wpo is the identity, h2 = x = 0 -> out = fp16(fp16(gelu(gate)) + bpo).
    Bound: the polynomial's 3e-6 + 4e-7 |g| (sd_gelu.h, the epilogue test's) + half an fp16 ulp for each of the two roundings."""
    import math
    M, inner = 512, 4 * C
    g = torch.linspace(-9, 9, M).half()
    n3 = torch.zeros(M, C, dtype=F16)
    n3[:, 0] = g
    zero = torch.zeros(M, C, dtype=F16)
    w1, b1 = torch.zeros(2 * inner, C, dtype=F16), torch.zeros(2 * inner, dtype=F16)
    b1[:128] = 1.0
    w1[inner:inner + 128, 0] = 1.0
    w2 = torch.zeros(C, inner, dtype=F16)
    w2[:, :128] = 1.0 / 128
    wpo, bpo, b2 = torch.eye(C, dtype=F16), rnd(C, seed=7, scale=0.1), torch.zeros(C, dtype=F16)
    inp = (n3, zero, zero, w1, b1, w2, b2, wpo, bpo)
    ck = Check("xtail rows=512 gate sweep")
    out = check_tail(ops, ck, inp, M).double().cpu()
    gd = g.double()
    gelu = (0.5 * gd * (1.0 + torch.erf(gd / math.sqrt(2.0))))[:, None]
    ref = gelu + bpo.double()[None]
    tiny = torch.tensor(6.1e-5, dtype=torch.float64)
    lim = 3e-6 + 4e-7 * gd.abs()[:, None] + (torch.maximum(gelu.abs(), tiny) + torch.maximum(ref.abs(), tiny)) * 2.0 ** -11
    bad = (out - ref).abs() > lim
    print(f"METRIC xtail gate sweep: max |out - (gelu + bpo)| {float((out - ref).abs().max()):.3e}, worst err / bound {float(((out - ref).abs() / lim).max()):.3f}")
    ck.true(not bool(bad.any()), f"GELU off the erf form at gates {g[bad.any(1)][:5].tolist()}")
    ck.done()


# ============================================================================================================================ race screen
@functools.lru_cache(maxsize=None)
def _bench_inputs(which):
    return dict(chain=lambda: chain_inputs(BENCH_B, BENCH_L, 77), front=lambda: front_inputs(BENCH_B, BENCH_L),
                tail=lambda: tail_inputs(BENCH_B * BENCH_L))[which]()


def _all_equal(what, launch):
    with kit.device_guard(what):                                # twelve back-to-back launches, one synchronize behind them
        runs = [launch() for _ in range(12)]
    for r in runs[1:]:
        for got, first in zip(r, runs[0]):
            assert torch.equal(got, first)
    assert all(float(t.float().abs().max()) > 0 for t in runs[0])


def test_xattn_chain_race_screen(ops):
    """The row-tile kernels rely on counted vmcnt waits and raw barriers around in-flight LDS-DMA, as the GEMM tiles do
    (test_gemm_race_screen): 12 back-to-back launches at the benchmark shape into 12 output sets must give the same bits."""
    inp = _bench_inputs("chain")
    dinp = [dv(t) for t in inp]
    vt2 = dv(vt_perm16(ops, inp[8], 80))
    _all_equal("xattn_chain race screen", lambda: launch_chain(ops, dinp, vt2, rps=BENCH_L, lk=77)[:2])


def test_xfront_race_screen(ops):
    x, gng, gnb, wpi, bpi, g1, b1, wq, wk, wv = _bench_inputs("front")
    dinp = [dv(t) for t in (x, gng, gnb, wpi, bpi, g1, b1, torch.cat([wq, wk]), wv)]
    table = torch.zeros(ops.gn_scratch_floats(BENCH_B, BENCH_L), dtype=torch.float32, device=DEV)
    ops.groupnorm_table(dinp[0], dinp[1], dinp[2], table, batch=BENCH_B, hw=BENCH_L, c0=C, eps=1e-6)
    _all_equal("xfront race screen", lambda: launch_front(ops, dinp, table, B=BENCH_B, L=BENCH_L, ldv=BENCH_L, eps=1e-5))


def test_xtail_race_screen(ops):
    dargs = tail_device_args(_bench_inputs("tail"))
    _all_equal("xtail race screen", lambda: launch_tail(ops, dargs, BENCH_B * BENCH_L))


# ============================================================================================================================== refusals
def test_bad_sizes_are_refused_not_launched(ops):
    """Sizes only, as test_argument_errors_are_reported_not_launched: every call below is refused before any memory is touched."""
    from coma_amd._lib import ComaHipError
    z = torch.zeros(8 * C, C, dtype=F16, device=DEV)                 # as large as the largest operand (W1) of the sizes below
    tab = torch.zeros(2 * C * 2, dtype=torch.float32, device=DEV)

    def chain(rows=256, rps=128, lk=77, ldv2=80, a=z):
        ops.xattn_chain(a, z, z, z, z, z, z, z, z, z, z, z, z, z, z, rows=rows, rows_per_sample=rps, lk=lk, ldv2=ldv2)

    def front(rows=256, rps=128, ldv=128, x=z):
        ops.xfront(x, tab, z, z, z, z, z, z, z, z, z, rows=rows, rows_per_sample=rps, ldv=ldv)

    def tail(rows=256, n3=z):
        ops.xtail(n3, z, z, z, z, z, z, z, z, z, None, rows=rows)

    for kw in (dict(rows=192, rps=96), dict(rows=200), dict(lk=0), dict(lk=81), dict(lk=96), dict(lk=97), dict(ldv2=72), dict(ldv2=84)):
        with pytest.raises(ComaHipError, match="sd_xattn_chain_f16: bad sizes"):
            chain(**kw)
    for kw in (dict(rows=192, rps=96), dict(rows=200), dict(ldv=120), dict(ldv=132)):
        with pytest.raises(ComaHipError, match="sd_xfront_f16: bad sizes"):
            front(**kw)
    for rows in (192, 0):
        with pytest.raises(ComaHipError, match="sd_xtail_f16: bad sizes"):
            tail(rows=rows)
    for fn, name, kw in ((chain, "sd_xattn_chain_f16", dict(a=None)), (front, "sd_xfront_f16", dict(x=None)), (tail, "sd_xtail_f16", dict(n3=None))):
        with pytest.raises(ComaHipError, match=name + ": null pointer"):
            fn(**kw)


# ====================================================================================================================== record and replay
def test_the_three_kinds_record_replay_save_and_load(ops, tmp_path):
    """One recorded launch of each kind (eps = 1e-3: a dropped or misplaced float argument changes the numbers) run as a list, replayed
    as a hipGraph, saved, loaded into a fresh model and replayed there: the same bits as the direct launches every time."""
    from coma_amd import _lib
    from coma_amd.sd.model import SdModel
    B, L, LK = 2, 128, 77
    M = B * L
    cin = chain_inputs(B, L, LK, "lowvar")
    dchain = [dv(t) for t in cin[:7]] + [dv(cin[7].reshape(-1, C)), dv(vt_perm16(ops, cin[8], 80))] + [dv(t) for t in cin[9:]]
    x, gng, gnb, wpi, bpi, g1, b1, wq, wk, wv = front_inputs(B, L, "lowvar")
    dfront = [dv(t) for t in (x, gng, gnb, wpi, bpi, g1, b1, torch.cat([wq, wk]), wv)]
    table = torch.zeros(ops.gn_scratch_floats(B, L), dtype=torch.float32, device=DEV)
    ops.groupnorm_table(dfront[0], dfront[1], dfront[2], table, batch=B, hw=L, c0=C, eps=1e-6)
    dtail = tail_device_args(tail_inputs(M))
    outs = dict(h2=torch.zeros(M, C, dtype=F16, device=DEV), n3=torch.zeros(M, C, dtype=F16, device=DEV),
                h=torch.zeros(M, C, dtype=F16, device=DEV), qk=torch.zeros(M, 2 * C, dtype=F16, device=DEV),
                vt=torch.zeros(B, C, L, dtype=F16, device=DEV), out=torch.zeros(M, C, dtype=F16, device=DEV),
                cs=torch.zeros(M // 32, 2, C, dtype=torch.float32, device=DEV))

    def launches():
        ops.xfront(dfront[0], table, *dfront[3:], outs["h"], outs["qk"], outs["vt"], rows=M, rows_per_sample=L, ldv=L, eps=1e-3)
        ops.xattn_chain(*dchain, outs["h2"], outs["n3"], rows=M, rows_per_sample=L, lk=LK, ldv2=80, eps=1e-3)
        ops.xtail(*dtail, outs["out"], outs["cs"], rows=M)

    def clear():
        for t in outs.values():
            t.zero_()

    launches()
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in outs.items()}
    assert all(float(v.float().abs().max()) > 0 for v in want.values())
    loose = {k: v.clone() for k, v in outs.items()}                       # the default eps gives other numbers: the float argument matters
    ops.xattn_chain(*dchain, loose["h2"], loose["n3"], rows=M, rows_per_sample=L, lk=LK, ldv2=80)
    assert not torch.equal(loose["n3"], want["n3"])
    m = SdModel(DEV)
    clear()
    m.record("p", launches)
    for k, v in outs.items():
        m.bind(k, v)
    assert m.num_launches("p") == 3
    torch.cuda.synchronize()
    assert all(float(v.float().abs().max()) == 0 for v in outs.values())  # recording launches nothing
    for run in (m.run, m.replay):
        clear()
        run("p")
        torch.cuda.synchronize()
        for k in outs:
            assert torch.equal(outs[k], want[k]), (run.__name__, k)
    clear()
    path = tmp_path / "rowtile.sdm"
    m.save(path)                                                          # the outputs go into the file as zeros
    m2 = SdModel.load(path, DEV)
    assert m2.num_launches("p") == 3
    m2.replay("p")
    for k in outs:
        p, n = m2.binding(k)
        got = torch.empty_like(want[k])
        assert n == got.numel() * got.element_size()
        _lib.check(_lib.lib().sd_copy_d2d(ctypes.c_void_p(got.data_ptr()), ctypes.c_void_p(p), n, _lib.stream_ptr(got.device)), "copy")
        torch.cuda.synchronize()
        assert torch.equal(got, want[k]), ("loaded", k)
