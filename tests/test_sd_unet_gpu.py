"""GPU: the whole UNet launch graph against the torch fp32 reference of the same architecture and the same seeded
random weights (oracle/sd_oracle.py: unet_ref).  Full SD-1.5-inpainting widths (320/640/1280/1280, 8 heads, 77x768
context); the latent is 16x16 so that the fp32 reference finishes in seconds on the host (every layer is
resolution-agnostic; the 64x64 case is covered by properties in test_sd_pipeline_gpu.py).
Tolerance: the graph stores every activation in fp16 through ~60 layers; measured (`pytest -rP` prints every METRIC line,
profiles/r04_notes.md 3): relative L2 1.43e-3 ... 1.83e-3, cosine >= 0.999995 over every case of this file -- the bars are 2 x
that (REL_L2 = 4e-3, 1 - COS = 2e-5), so that a kernel regression of 2-3 x fails (an fp16 torch run of the same graph lands at
~5e-3, i.e. would fail: the fp32 accumulation everywhere is part of what is tested)."""
import pytest
import torch

from oracle import sd_oracle as so

pytestmark = pytest.mark.gpu
REL_L2, COS = 4e-3, 0.99998
DEV = "cuda:0"


def _ref_on_device(state, sample, t, ctx, cfg, chunk=4):
    """The fp32 restatement evaluated by torch's own fp32 kernels on the device (nothing of libcoma_hip.so involved) for the large
    cases -- 12 s per forward on the host cores otherwise; the small cases of this file keep the CPU evaluation and
    tests/test_sd_adaptive_gpu.py::test_restatement_on_device_equals_restatement_on_cpu ties the two evaluations (1e-4)."""
    old = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        sd = {k: v.to(DEV, torch.float32) for k, v in state.items()}
        with torch.no_grad():
            out = torch.cat([so.unet_ref(sd, sample[i:i + chunk].to(DEV), t[i:i + chunk].to(DEV), ctx[i:i + chunk].to(DEV), cfg)
                             for i in range(0, sample.shape[0], chunk)])
        return out.cpu()
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = old


@pytest.fixture(scope="module")
def setup(hip_lib):
    from coma_amd.sd import weights
    from coma_amd.sd.unet import HipUNet2DConditionModel
    state = weights.random_state(weights.unet_shapes(), seed=0)
    B, H = 2, 16
    g = torch.Generator().manual_seed(1)
    sample = torch.randn(B, 9, H, H, generator=g).half().float()
    ctx = torch.randn(B, 77, 768, generator=g).half().float()
    t = torch.tensor([961.0, 961.0])
    ref = so.unet_ref(state, sample, t, ctx, weights.UNET_CFG)
    return state, sample, ctx, t, ref, HipUNet2DConditionModel


def _metrics(out, ref):
    out, ref = out.float().cpu(), ref.float().cpu()
    rel = float((out - ref).norm() / ref.norm())
    cos = float(torch.nn.functional.cosine_similarity(out.flatten(), ref.flatten(), dim=0))
    print(f"METRIC rel-L2 {rel:.3e} cos {cos:.6f}")        # pytest -rP shows the measured distances the bars are set from
    return rel, cos


@pytest.mark.parametrize("use_graph", [False, True])
def test_unet_matches_fp32_reference(setup, use_graph):
    state, sample, ctx, t, ref, UNet = setup
    unet = UNet(state, batch=2, height=16, width=16, device=DEV, use_graph=use_graph)
    out = unet(sample.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
    assert tuple(out.shape) == (2, 4, 16, 16)
    rel, cos = _metrics(out, ref)
    assert rel <= REL_L2 and cos >= COS, (rel, cos)
    out2 = unet(sample.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
    assert torch.equal(out, out2), "graph replay must be bitwise reproducible"


def test_unet_responds_to_timestep_and_context(setup):
    state, sample, ctx, t, ref, UNet = setup
    unet = UNet(state, batch=2, height=16, width=16, device=DEV, use_graph=True)
    a = unet(sample.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV))[0].clone()
    b = unet(sample.to(DEV), torch.tensor([1.0, 1.0]).to(DEV), encoder_hidden_states=ctx.to(DEV))[0].clone()
    c = unet(sample.to(DEV), t.to(DEV), encoder_hidden_states=(ctx * 0.5).to(DEV))[0].clone()
    assert not torch.equal(a, b) and not torch.equal(a, c)
    ref_b = so.unet_ref(state, sample, torch.tensor([1.0, 1.0]), ctx, __import__("coma_amd.sd.weights", fromlist=["x"]).UNET_CFG)
    rel, cos = _metrics(b, ref_b)
    assert rel <= REL_L2 and cos >= COS, (rel, cos)


@pytest.mark.parametrize("hw,batch", [(16, 4), (64, 16)])
def test_shared_cfg_prefix_is_bit_identical(setup, hw, batch):
    """Classifier-free guidance feeds the UNet [uncond | cond] with the SAME sample and timestep in both halves
    (utils/adaptive_mask_inpainting.py:990): computing the layers before the first cross-attention once and duplicating
    them must not change a single bit of the output (and the fp32 reference still agrees)."""
    state, _, _, _, _, UNet = setup
    g = torch.Generator().manual_seed(7)
    half = torch.randn(batch // 2, 9, hw, hw, generator=g).half().float()
    sample = torch.cat([half, half])
    ctx = torch.randn(batch, 77, 768, generator=g).half().float()
    t = torch.full((batch,), 441.0)
    outs = []
    for shared in (False, True):
        unet = UNet(state, batch=batch, height=hw, width=hw, device=DEV, use_graph=True, cfg_shared_prefix=shared)
        assert unet.cfg_shared_prefix == shared
        outs.append(unet(sample.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV))[0].clone())
        flops = unet.g.flops
        del unet
        torch.cuda.empty_cache()
        outs.append(flops)
    if batch == 16:
        # benchmark configuration: the half-batch launches pick the same tile families -> not a single bit changes
        assert torch.equal(outs[0], outs[2])
    else:
        # small batches may pick another split-K factor for the half-batch prefix: equal up to fp16 rounding
        assert float((outs[0] - outs[2]).abs().max()) <= 2e-3 * float(outs[0].abs().max())
    assert outs[3] < outs[1]                                    # fewer MFMA flops issued
    assert not torch.equal(outs[0][:batch // 2], outs[0][batch // 2:])   # the halves do differ (context)
    if hw == 16:
        from coma_amd.sd import weights
        rel, cos = _metrics(outs[2], so.unet_ref(state, sample, t, ctx, weights.UNET_CFG))
        assert rel <= REL_L2 and cos >= COS, (rel, cos)


def test_unet_benchmark_shape_matches_fp32_reference(setup):
    """BASELINE config 2's own launch list -- 64x64 latents, UNet batch 16 (8 images x [uncond | cond]) -- against the
    fp32 restatement: this is the forward whose GEMMs pick the 256 x 320 / 128 x 320 / split-K tile families and the
    producer-side GroupNorm statistics (M >= 32768), none of which the 16x16 case reaches.  The host reference takes
    ~1-2 minutes for the batch of 16 on the GPU box's cores.  Same tolerances as the 16x16 case."""
    state, _, _, _, _, UNet = setup
    from coma_amd.sd import weights
    B, hw = 16, 64
    g = torch.Generator().manual_seed(11)
    half = torch.randn(B // 2, 9, hw, hw, generator=g).half().float()
    sample = torch.cat([half, half])                       # CFG layout: both halves see the same latents
    ctx = torch.randn(B, 77, 768, generator=g).half().float()
    t = torch.full((B,), 621.0)
    unet = UNet(state, batch=B, height=hw, width=hw, device=DEV, use_graph=True)
    out = unet(sample.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV), return_dict=False)[0].clone()
    del unet
    torch.cuda.empty_cache()
    ref = _ref_on_device(state, sample, t, ctx, weights.UNET_CFG)
    rel, cos = _metrics(out, ref)
    assert rel <= REL_L2 and cos >= COS, (rel, cos)
    # per-sample: no sample may hide behind the batch average (a wrong tile shows up as one bad image)
    for i in range(B):
        r, c = _metrics(out[i], ref[i])
        assert r <= REL_L2 and c >= COS, (i, r, c)


def test_context_longer_than_the_chain_kernel_takes_the_unfused_path(setup):
    """sd_xattn_chain_f16 multiplies 80 key positions, so its rule in unet.py is Lk <= 80: a UNet built for 96 context tokens has no
    `xchain` launch (the 77-token one has) and matches the fp32 reference at 16 x 16 through sd_attention_f16."""
    state, sample, _, t, _, UNet = setup
    from coma_amd.sd import weights
    assert any(tag.startswith("xchain") for tag, _ in UNet(state, batch=2, height=16, width=16, device=DEV).g.tags)
    ctx = torch.randn(2, 96, 768, generator=torch.Generator().manual_seed(41)).half().float()
    unet = UNet(state, batch=2, height=16, width=16, ctx_len=96, device=DEV, use_graph=True)
    assert not any(tag.startswith("xchain") for tag, _ in unet.g.tags)
    out = unet(sample.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
    ref = so.unet_ref(state, sample, t, ctx, weights.UNET_CFG)
    rel, cos = _metrics(out, ref)
    assert rel <= REL_L2 and cos >= COS, (rel, cos)


def test_row_tile_fusions_agree_with_the_unfused_graph(setup):
    """The C = 320 row-tile kernels (sd_xfront_f16, sd_xattn_chain_f16, sd_xtail_f16) and the one-launch q | k | v projection
    (sd_conv_gemm_desc.out_t) against the SAME network with every one of them switched off, at the 64 x 64 level where they are used
    (batch 4): the two launch lists compute the same products with the same roundings except for accumulation order -> the outputs
    agree far inside the fp32-reference tolerance, and each one matches the reference."""
    state, _, _, _, _, UNet = setup
    from coma_amd.sd import weights
    B, hw = 4, 64
    g = torch.Generator().manual_seed(21)
    sample = torch.randn(B, 9, hw, hw, generator=g).half().float()
    ctx = torch.randn(B, 77, 768, generator=g).half().float()
    t = torch.tensor([981.0, 621.0, 301.0, 21.0])
    outs, n_launch = [], []
    for on in (True, False):
        unet = UNet(state, batch=B, height=hw, width=hw, device=DEV, use_graph=True, fuse_xchain=on, fuse_xfront=on, fuse_xtail=on, fuse_qkv=on,
                    xtail_min_rows=0)       # the rule keeps sd_xtail_f16 for >= 32768 rows; here it runs at 16384
        outs.append(unet(sample.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV), return_dict=False)[0].clone())
        n_launch.append(len(unet.g.launches))
        del unet
        torch.cuda.empty_cache()
    assert n_launch[0] < n_launch[1] - 50, n_launch            # the fused list really is the short one
    rel, cos = _metrics(outs[0], outs[1])
    assert rel <= 5e-3 and cos >= 0.9999, (rel, cos)
    ref = _ref_on_device(state, sample, t, ctx, weights.UNET_CFG)
    for o in outs:
        rel, cos = _metrics(o, ref)
        assert rel <= REL_L2 and cos >= COS, (rel, cos)


@pytest.mark.parametrize("winograd_min_batch", [8, 2])
def test_unet_ragged_resolution_matches_fp32_reference(setup, winograd_min_batch):
    """A latent that is neither square nor a multiple of 64 tokens anywhere (24 x 40 -> 12 x 20 -> 6 x 10 -> 3 x 5: attention over
    960 / 240 / 60 / 15 tokens, GEMMs with M = 30 ... 1920 rows): every ragged-edge path of the kernels (partial tiles, key padding,
    small GroupNorms) and the fall-back of the row-tile fusions, against the fp32 reference.  Second case: the Winograd path of the deep
    ResNet levels forced on at this batch of 2 (the rule keeps it for UNet batches >= 8): odd tile grids (6 x 10, 3 x 5 tiles), the unfused
    GroupNorm chain where a group slice does not fit, the upsampler transform over an odd source."""
    state, _, _, _, _, UNet = setup
    from coma_amd.sd import weights
    B, h, w = 2, 24, 40
    g = torch.Generator().manual_seed(31)
    sample = torch.randn(B, 9, h, w, generator=g).half().float()
    ctx = torch.randn(B, 77, 768, generator=g).half().float()
    t = torch.tensor([741.0, 41.0])
    unet = UNet(state, batch=B, height=h, width=w, device=DEV, use_graph=True, winograd_min_batch=winograd_min_batch)
    assert any("winograd" in tag for tag, _ in unet.g.tags) == (winograd_min_batch == 2)
    out = unet(sample.to(DEV), t.to(DEV), encoder_hidden_states=ctx.to(DEV), return_dict=False)[0]
    assert tuple(out.shape) == (B, 4, h, w)
    ref = so.unet_ref(state, sample, t, ctx, weights.UNET_CFG)
    rel, cos = _metrics(out, ref)
    assert rel <= REL_L2 and cos >= COS, (rel, cos)
