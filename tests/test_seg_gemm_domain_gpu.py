"""seg_conv_gemm_f32 (coma_amd/csrc/seg_gemm.hip) over the domain its entry point accepts: the six instantiations with and without the
residual prefetch, every K chunk count around the peeled loop tail, ragged rows and columns, every gather form, leading dimensions with
gaps, both residual forms through all four epilogue paths, the device-side row gate and split-K.  The table is tests/seg_ref.GEMM_CASES;
tests/test_seg_ref_host.py checks on the CPU that each row reaches the launch it names.

Two operand families per case.  "int": integers in [-4, 4], every partial sum below 2^24, so the device equals the float64 reference bit
for bit whatever the summation order.  "normal": |got - ref64| <= gamma_t (sum |a w| + |bias| + |res|) per element, t = k terms + 3
(derived, the measured ratio is printed).  Per case also: (b) nothing that had to be written is NaN / Inf / sentinel; (c)
every gap column, gated-out row and guard of `out` keeps its sentinel bit for bit and the workspace is untouched outside its
workspace_bytes; (d) a second launch into fresh buffers gives the same bits.  Every operand element the contract says is not read is NaN:
guards around every operand, gap columns of x and res, gated-out rows, the whole workspace."""
import pytest
import torch

from coma_amd._lib import ComaHipError
from tests import domain_kit as kit
from tests import seg_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = sr.GUARD


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.seg import ops
    return ops


def run(ops, c, dev):
    """One launch into a fresh sentinel-filled output and a fresh NaN workspace -> (out, workspace) flat on the CPU, guards included."""
    out = sr.guarded(sr.sentinel(c.m, c.ldo_)).to(DEV)
    ws = sr.guarded(torch.full((c.ws_slabs * c.slab_elems,), sr.NAN)).to(DEV) if c.ws_slabs else None
    t = dict(dev, workspace=None if ws is None else ws[G:])
    with kit.device_guard(c.id):
        ops.conv_gemm(dev["x"], dev["w"], out[G:], **sr.gemm_kwargs(c, t))
    return out.cpu(), None if ws is None else ws.cpu()


@pytest.mark.parametrize("family", sr.GEMM_FAMILIES)
@pytest.mark.parametrize("case", sr.GEMM_CASES, ids=lambda c: c.id)
def test_seg_conv_gemm_domain(ops, case, family):
    c = case
    inp = sr.make_gemm_inputs(c, family)
    dev = {k: (None if v is None else sr.guarded(v).to(DEV)[G:-G]) for k, v in vars(inp).items()}
    if c.bias_off:                                                  # the same bias, c.bias_off floats off the 16-byte boundary
        dev["bias"] = sr.guarded(torch.cat([torch.full((c.bias_off,), sr.NAN), inp.bias])).to(DEV)[G + c.bias_off:-G]
    out, ws = run(ops, c, dev)
    out2, _ = run(ops, c, dev)
    ref, mag = sr.gemm_reference(c, inp)
    mask = sr.gemm_written_mask(c)
    body = out[G:-G].view(c.m, c.ldo_)
    got = body[:, :c.n]
    valid = mask[:, :c.n]

    assert bool(torch.isfinite(body[mask]).all()), "(b) NaN / Inf (or an unwritten element) in the written region of `out`"
    assert bool((kit.bits(body)[~mask] == kit.sentinel_bits(torch.float32)).all()), "(c) a gap column or a gated-out row of `out` was written"
    assert sr.guards_intact(out), "(c) a guard of `out` was written"
    assert torch.equal(kit.bits(out), kit.bits(out2)), "(d) the second launch differs"
    if ws is not None:
        assert sr.guards_intact(ws), "(c) the workspace was written outside its workspace_bytes"
    err = (got.double() - ref).abs()[valid]
    if family == "int":
        print(f"SEG_DOMAIN gemm {c.id} family=int mismatches={int((err != 0).sum())} of {int(valid.sum())}")
        assert torch.equal(got[valid], ref.float()[valid]), f"(a) integer operands: {int((err != 0).sum())} elements differ, worst {float(err.max()):g}"
    else:
        bound = sr.gemm_bound(c, mag)[valid]
        ratio = float((err / bound).max()) if err.numel() else 0.0
        print(f"SEG_DOMAIN gemm {c.id} family=normal t={c.k + 3} worst |err| / bound = {ratio:.3f}")
        assert ratio <= 1.0, f"(a) error {ratio:.3f} x the bound"


def test_seg_conv_gemm_refusals_are_reported_not_launched(ops):
    """Every row of seg_ref.GEMM_REFUSALS through the real entry point: the error text, and `out` keeps its sentinel.  Each row is first put
    to seg_conv_gemm_describe, which launches nothing: a row the library accepted would otherwise launch over these small buffers."""
    small = torch.zeros(4096, device=DEV)
    cnt = torch.zeros(16, dtype=torch.int32, device=DEV)
    out = sr.sentinel(4096).to(DEV)
    n = 0
    for text, change in sr.GEMM_REFUSALS:
        kw = {**sr.GEMM_REFUSAL_BASE, **change}
        kw = {k: ((cnt if k == "m_dev" else out if k == "out" else small) if v is kit.PTR else v) for k, v in kw.items()}
        x, w, o = kw.pop("x"), kw.pop("w"), kw.pop("out")
        with pytest.raises(ComaHipError, match=r"seg_conv_gemm_describe failed \(-1\): seg_conv_gemm_f32: .*" + text):
            ops.conv_gemm_describe(x, w, o, **kw)
        with pytest.raises(ComaHipError, match=r"seg_conv_gemm_f32 failed \(-1\): seg_conv_gemm_f32: .*" + text):
            ops.conv_gemm(x, w, o, **kw)
        n += 1
    assert n == len(sr.GEMM_REFUSALS)
    torch.cuda.synchronize()
    assert bool((kit.bits(out.cpu()) == kit.sentinel_bits(torch.float32)).all())
