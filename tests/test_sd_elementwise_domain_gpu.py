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
import re

import pytest
import torch

from coma_amd._lib import ComaHipError
from tests import elementwise_ref as er
from tests import norm_ref as nr

COMA_E_INVALID = -1
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = nr.GUARD


@pytest.fixture(scope="module")
def ops(hip_lib):
    assert torch.cuda.is_available()
    from coma_amd.sd import ops
    return ops


def launch_twice(ops, c, dev, outs):
    """Two launches of the case, each into fresh outputs, then ONE synchronize -> two dicts name -> flat device buffer (guards included).
    A refusal by the argument checks fails its own case; any other error ends the session: nothing more is started on the device."""
    both = []
    try:
        for _ in range(2):
            bufs = {name: o.buf.to(DEV) for name, o in outs.items()}
            er.launch(ops, c, {**dev, **{name: bufs[name][G + o.off:] for name, o in outs.items()}})
            both.append(bufs)
        torch.cuda.synchronize()
    except Exception as e:
        if isinstance(e, ComaHipError) and f"failed ({COMA_E_INVALID})" in str(e):
            raise
        pytest.exit(f"{c.id}: {type(e).__name__}: {e}", returncode=3)
    return both


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


@pytest.mark.parametrize("case", er.CASES, ids=lambda c: c.id)
def test_elementwise_domain(ops, case):
    c = case
    ins, outs = er.plan(c)
    dev = {k: i.buf.to(DEV)[G + i.off:] for k, i in ins.items()}
    first, second = launch_twice(ops, c, dev, outs)

    got = {}
    for name, o in outs.items():
        buf = first[name].cpu()
        b, b0 = _bits(buf), _bits(o.buf)
        sent = er.sentinel_of(o.buf.dtype)
        if o.buf.dtype != torch.uint8:                              # (every u8 value is a legitimate result: the exact comparison speaks for those)
            assert not bool((b[o.must] == sent).any()), f"(b) an element the launch owns of `{name}` still holds the sentinel"
        if o.buf.is_floating_point() and o.finite:
            assert bool(torch.isfinite(buf[o.must].float()).all()), f"(b) NaN / Inf in what the launch owns of `{name}`"
        assert torch.equal(b[~o.must], b0[~o.must]), f"(c) `{name}` was written outside what the contract says"
        assert torch.equal(b, _bits(second[name].cpu())), f"(d) the second launch differs in `{name}`"
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
    small = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    outs = {name: nr.sentinel(1 << 16, torch.float32).to(DEV) for name in er.OUTPUT_ARGS}
    resolve = lambda name: (outs[name] if name in outs else small).data_ptr()
    n = 0
    for entry, (base, rows) in sorted(er.REFUSALS.items()):
        for text, change in rows:
            rc = er.call(hip_lib, entry, {**base, **change}, resolve)
            msg = hip_lib.coma_last_error().decode()
            assert rc == COMA_E_INVALID and re.search(re.escape(entry) + ": .*" + re.escape(text), msg), (entry, change, rc, msg)
            n += 1
    assert n == sum(len(rows) for _, rows in er.REFUSALS.values()) and n > 120
    torch.cuda.synchronize()
    for name, buf in outs.items():
        assert bool((nr.bits(buf.cpu()) == nr.SENTINEL_BITS32).all()), name
    assert not bool(small.cpu().any())
