"""GPU: the whole UNet with its Upsample2D convolutions as one launch of the four sub-pixel phase products (sd_conv_gemm_desc.phase = 5,
the rule of coma_amd/sd/unet.py: UNet batch >= 8, source >= 16 x 16) against the same graph with the rule switched off -- the direct 3x3
over the upsampled tensor and the Winograd form, as before the rule existed.  Full widths, batch 8, 32 x 32 latents: the smallest
configuration in which the rule fires (the 16 x 16 -> 32 x 32 upsampler, 640 channels).  Both graphs compute the same convolution with
fp32 accumulation and differ by fp16 rounding of stored activations only, so they must agree within the tolerance
tests/test_sd_unet_gpu.py applies between the graph and the fp32 reference (relative L2 4e-3, cosine 0.99998); the 64 x 64 graph with both
phase launches is held to the fp32 reference itself by test_unet_benchmark_shape_matches_fp32_reference."""
import pytest
import torch

pytestmark = pytest.mark.gpu
REL_L2, COS = 4e-3, 0.99998
DEV = "cuda:0"


def test_unet_with_one_launch_phase_upsampler_agrees_with_the_3x3_form(hip_lib, monkeypatch):
    from coma_amd.sd import unet as U, weights
    state = weights.random_state(weights.unet_shapes(), seed=0)
    B, hw = 8, 32
    g = torch.Generator().manual_seed(3)
    sample, ctx, t = torch.randn(B, 9, hw, hw, generator=g).half().float(), torch.randn(B, 77, 768, generator=g).half().float(), torch.full((B,), 441.0)

    def run():
        unet = U.HipUNet2DConditionModel(state, batch=B, height=hw, width=hw, device=DEV, use_graph=True)
        out = unet(sample.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV))[0].float().cpu()
        tags = [str(x) for x in unet.g.tags]
        del unet
        torch.cuda.empty_cache()
        return out, tags

    out, tags = run()
    assert sum("four phases" in x for x in tags) == 1 and sum("(upsample phase" in x for x in tags) == 0
    monkeypatch.setattr(U, "PHASE_UPSAMPLE_MIN_HW", 1 << 30)
    ref, ref_tags = run()
    assert not any("four phases" in x for x in ref_tags) and len(ref_tags) == len(tags)
    rel = float((out - ref).norm() / ref.norm())
    cos = float(torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0))
    print(f"METRIC rel-L2 {rel:.3e} cos {cos:.6f}")
    assert torch.isfinite(out).all() and rel <= REL_L2 and cos >= COS, (rel, cos)
