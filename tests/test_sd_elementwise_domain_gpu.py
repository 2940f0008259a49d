"""The eleven entry points of coma_amd/csrc/sd_elementwise.hip and sd_text.hip (sd_cfg_ddim_step, sd_timestep_embedding_f16,
sd_nchw_to_nhwc_f16, sd_nhwc_to_nchw_f32, sd_image_to_u8, sd_vae_sample, sd_add_noise, sd_mask_adapt, sd_mask_adapt_batched,
sd_text_embed_f16, sd_attention_causal_f16) over the domain their argument checks accept.  The table is tests/elementwise_ref.CASES;
tests/test_elementwise_ref_host.py checks on the CPU that it reaches every branch and that a broken kernel fails it.

Per case: (a) elementwise_ref.check -- the exact contracts (layout conversions, u8 image, every mask output and `area`, the text
embedding, the assembly of unet_in, the fp16 copies of the device's own fp32 results) bit for bit, the arithmetic results within
max(4 * e_emu, floor) of the float64 reference, e_emu being what the kernel's formula in fp32, emulated on the CPU, loses on the same case
(DESIGN.md section 3g lists it beside the measured device error); (b) everything the contract says is written is free of the sentinel
and, where the case keeps its results finite, of NaN / Inf; (c) everything else -- guards, gap columns, channels >= 8 of a masked pixel
without write_pad, latents under write_latents = 0, x0_out without a step -- keeps its first bits; (d) a second launch into fresh buffers
gives the same bits.  Every operand element the contract says is not read is poison (NaN; for the u8 masks and the ids a value that
changes the result), so a read outside the contract fails (a) or (b).  Every case is inside the accepted domain; one synchronize per
case."""
import pytest
import torch

from tests import domain_kit as kit
from tests import elementwise_ref as er

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = kit.GUARD


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.sd import ops
    return ops


@pytest.mark.parametrize("case", er.CASES, ids=lambda c: c.id)
def test_elementwise_domain(ops, case):
    c = case
    ins, outs = er.plan(c)
    dev = {k: i.buf.to(DEV)[G + i.off:] for k, i in ins.items()}
    first, second = kit.launch_twice(lambda: {name: o.buf.to(DEV) for name, o in outs.items()},                 # flat, guards included
                                     lambda bufs: er.launch(ops, c, {**dev, **{name: bufs[name][G + o.off:] for name, o in outs.items()}}), c.id)

    got = {}
    for name, o in outs.items():
        buf = first[name].cpu()
        kit.check_written(name, buf, second[name].cpu(), o.buf, o.must, o.must, o.finite)
        n = buf.numel() - 2 * G - o.off
        got[name] = buf.numpy()[G + o.off:G + o.off + n]
    shaped = {}
    emu = er.emulate(c)
    for name, v in got.items():
        like = emu.get(name)
        shaped[name] = v if like is None else (v.reshape(like.shape) if v.size == like.size else v.reshape(like.shape[0], -1)[:, :like.shape[1]])
    fig = er.check(c, shaped)
    for name, f in fig.items():
        print(f"ELEMENTWISE_DOMAIN {c.id} entry={c.entry} out={name} e_emu={f.e_emu:.3e} bound={f.bound:.3e} device={f.err:.3e}")
    if not fig:
        print(f"ELEMENTWISE_DOMAIN {c.id} entry={c.entry} exact")


def test_refusals_are_reported_not_launched(ops, hip_lib):
    """Every row of elementwise_ref.REFUSALS through the real entry points, with small device buffers where the row wants a pointer: the
    code and the text, and every output buffer keeps its sentinel.  tests/test_elementwise_ref_host.py has put the same rows to the same
    entry points on the CPU, where a wrongly accepted row cannot launch."""
    resolve, outs, small = kit.device_resolver(er.OUTPUT_ARGS)
    assert kit.check_refusals(hip_lib, er.REFUSALS, resolve, expect_control=False) > 120
    kit.refusal_outputs_untouched(outs, small)
