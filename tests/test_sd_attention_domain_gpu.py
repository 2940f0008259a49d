"""The attention kernels of coma_amd/csrc/sd_attention.hip over the whole domain their entry points accept: every head dim of
sd_attention_f16 (all ten attention_kernel instantiations, plain and PERM16 V^T), the UNet's strided operand form, the software-pipelined
d = 40 kernel forced, the 64-queries-per-wave forms with a ragged last block, the softmax state machine of the generic kernel, and
sd_attention_wide_f16 at single tiles, lq != lk, strided operands and both wave counts.  The table is tests/attention_ref.CASES.

Per case: (a) every compared query is within the case's bound of the float64 reference, the error normalised by that query's largest
|output|; the bound is max(4 * e_emu, 2^-10), e_emu being what a careful fp16 kernel emulated on the CPU loses on the same case
(tests/test_attention_ref_host.py prints it; DESIGN.md section "Attention: domain tests" lists it beside the measured device error);
(b) nothing the kernel had to write is NaN / Inf -- `out` starts as NaN, so an unwritten element shows; (c) the gap columns of `out` and
the guard behind it keep the sentinel bit for bit; (d) a second launch gives the same bits.  Every operand element the contract says is
not read is NaN and the V^T pad columns are 1e4, so a read outside the contract poisons (a) or (b)."""
import pytest
import torch

from tests import attention_ref as ar
from tests import domain_kit as kit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.sd import ops
    return ops


def launch(ops, c, q, k, v):
    """Pack the operands of case c as its `ld` / `vt` say, launch twice into fresh sentinel-filled buffers (under the kit's fault policy:
    a launch error ends the session) -> (out1, out2) flat, on the CPU."""
    ld = c.leading_dims()
    C = c.C
    if c.ld in ("fused", "fusedx"):
        qk = ar.pack_fused_qk(q, k).to(DEV)
        qd, kd = qk, qk[C:]
    else:
        qd = ar.pack_rows(q, ld["ldq"], col0=ld["qcol0"]).to(DEV)[ld["qcol0"]:]
        kd = ar.pack_rows(k, ld["ldk"]).to(DEV)
    vt = {"plain": ar.pack_vt_plain, "perm16": ar.pack_vt_perm16, "perm32": ar.pack_vt_perm32}[c.vt](v, ld["ldv"]).to(DEV)
    kw = dict(batch=c.B, heads=c.H, lq=c.lq, lk=c.lk, d=c.d, ldq=ld["ldq"], ldk=ld["ldk"], ldv=ld["ldv"], ldo=ld["ldo"], scale=c.d ** -0.5)
    outs = []
    with kit.device_guard(c.id):
        for _ in range(2):
            out = ar.new_out(c.B, c.lq, ld["ldo"]).to(DEV)
            if c.kind == "wide":
                ops.attention_wide(qd, kd, vt, out, **kw)
            else:
                ops.attention(qd, kd, vt, out, vt_perm16=c.vt == "perm16", pipelined=True if c.kind == "sp" else None, **kw)
            outs.append(out.cpu())
    return outs


@pytest.mark.parametrize("case", ar.CASES, ids=lambda c: c.id)
def test_attention_domain(ops, case):
    c = case
    q, k, v = ar.make_inputs(c)
    y = ar.yardstick(c)
    out1, out2 = launch(ops, c, q, k, v)
    ldo = c.leading_dims()["ldo"]
    got, rest = ar.split_out(out1, c.B, c.lq, c.C, ldo)
    err = ar.query_error(ar.select(got, c.compared(), c.d), y.ref, 1)
    dev = float(err.nan_to_num(nan=float("inf")).max())
    print(f"ATTN_DOMAIN {c.id} family={c.family} e_emu={y.e_emu:.3e} bound={y.bound:.3e} device={dev:.3e}")
    assert bool(torch.isfinite(got.float()).all()), "(b) NaN / Inf (or an unwritten element) in the written region"
    assert bool((rest == kit.sentinel_bits(F16)).all()), "(c) a gap column or the guard of `out` was written"
    assert torch.equal(out1.view(torch.int16), out2.view(torch.int16)), "(d) the second launch differs"
    worst = int(err.flatten().argmax())
    assert dev <= y.bound, f"(a) query error {dev:.3e} > {y.bound:.3e} (e_emu {y.e_emu:.3e}) at compared slice / query {divmod(worst, c.lq)}"


def test_attention_argument_errors_are_reported_not_launched(ops):
    """Every refusal of sd_attention_f16 and sd_attention_wide_f16: an error code and its text, and `out` keeps its sentinel."""
    from coma_amd._lib import ComaHipError
    x = torch.zeros(64 * 512, dtype=F16, device=DEV)
    out = ar.new_out(1, 64, 512).to(DEV)
    ok = dict(batch=1, heads=1, lq=64, lk=64, d=40, ldq=64, ldk=64, ldv=64, ldo=64, scale=1.0)
    wok = dict(batch=1, heads=1, lq=64, lk=64, d=128, ldq=128, ldk=128, ldv=64, ldo=128, scale=1.0)

    def refused(fn, match, base, **change):
        with pytest.raises(ComaHipError, match=match):
            fn(x, x, x, out, **{**base, **change})

    with pytest.raises(ComaHipError, match="sd_attention_f16: null pointer"):
        ops.attention(x, None, x, out, **ok)
    refused(ops.attention, "sd_attention_f16: bad sizes", ok, lq=0)
    refused(ops.attention, "sd_attention_f16: bad sizes", ok, batch=0)
    refused(ops.attention, "head dim 4 unsupported", ok, d=4)
    refused(ops.attention, "head dim 168 unsupported", ok, d=168, ldq=168, ldk=168, ldo=168)
    refused(ops.attention, "head dim 0 unsupported", ok, d=0)
    refused(ops.attention, "sd_attention_f16: bad leading dimensions", ok, ldq=68)             # ldq % 8
    refused(ops.attention, "sd_attention_f16: bad leading dimensions", ok, ldk=68)             # ldk % 8
    refused(ops.attention, "sd_attention_f16: bad leading dimensions", ok, ldo=66)             # ldo % 4
    refused(ops.attention, "sd_attention_f16: bad leading dimensions", ok, ldq=32)             # ldq < heads * d
    refused(ops.attention, "sd_attention_f16: bad leading dimensions", ok, heads=2, ldq=80, ldk=80, ldo=72)    # ldo < heads * d
    refused(ops.attention, "sd_attention_f16: bad leading dimensions", ok, lk=65, ldv=64)      # ldv short of roundup(lk, 8) = 72
    refused(ops.attention, "sd_attention_f16: bad leading dimensions", ok, lk=60, ldv=68)      # ldv % 8
    refused(ops.attention, "vt_perm16 needs ldv a multiple of 16", ok, lk=60, ldv=72, vt_perm16=True)
    refused(ops.attention, "vt_perm16 needs ldv a multiple of 16", ok, lk=65, ldv=72, vt_perm16=True)   # covers roundup(65, 8), not roundup(65, 16)
    # the 2 GiB rule of the 32-bit LDS-DMA offsets, through sizes alone: refused before any memory is touched
    refused(ops.attention, "sd_attention_f16: K / V\\^T slice of one \\(batch, head\\) exceeds 2 GiB", ok, lk=1 << 20, ldk=1024, ldv=1 << 20)
    refused(ops.attention, "sd_attention_f16: K / V\\^T slice of one \\(batch, head\\) exceeds 2 GiB", ok, d=160, ldq=160, ldk=160, ldo=160, ldv=1 << 23)

    with pytest.raises(ComaHipError, match="sd_attention_wide_f16: null pointer"):
        ops.attention_wide(x, x, None, out, **wok)
    refused(ops.attention_wide, "sd_attention_wide_f16: bad sizes", wok, heads=0)
    refused(ops.attention_wide, "lk must be a multiple of 64", wok, lk=96, ldv=96)
    refused(ops.attention_wide, "head dim 64 unsupported \\(128, 256 or 512\\)", wok, d=64)
    refused(ops.attention_wide, "head dim 384 unsupported", wok, d=384, ldq=384, ldk=384, ldo=384)
    refused(ops.attention_wide, "sd_attention_wide_f16: bad leading dimensions", wok, ldq=132)     # ldq % 8
    refused(ops.attention_wide, "sd_attention_wide_f16: bad leading dimensions", wok, ldo=130)     # ldo % 4
    refused(ops.attention_wide, "sd_attention_wide_f16: bad leading dimensions", wok, lk=128, ldv=64)   # ldv < lk
    refused(ops.attention_wide, "sd_attention_wide_f16: bad leading dimensions", wok, ldk=64)      # ldk < heads * d
    refused(ops.attention_wide, "sd_attention_wide_f16: K / V\\^T slice of one \\(batch, head\\) exceeds 2 GiB", wok, lk=1 << 20, ldk=1024, ldv=1 << 20)
    refused(ops.attention_wide, "sd_attention_wide_f16: K / V\\^T slice of one \\(batch, head\\) exceeds 2 GiB", wok, d=512, ldq=512, ldk=512, ldo=512,
            ldv=1 << 21)
    torch.cuda.synchronize()
    assert bool((out.cpu().view(torch.int16) == kit.sentinel_bits(F16)).all())
