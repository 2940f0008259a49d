#!/usr/bin/env python3
"""Launch listings and output digests of every recorded network, seeded, for comparing two TREES of the host-side builders launch for
launch and bit for bit: per plan one line per launch (tag, flops, executed flops, bytes), the launch count the library recorded, and a
SHA-256 of each output after one call.  It uses only the constructors and `g.tags` / `g.exec_tags` / `g.alg_bytes` /
`g.model.num_launches`, so it runs unchanged on an older tree.  Run it once per tree in separate processes and diff the outputs:

    python scripts/plan_digests.py > a.txt          (in one checkout)
    python scripts/plan_digests.py > b.txt          (in the other)  && diff a.txt b.txt

Shapes are the smallest that reach every rule of sd/gn_stats.py (statistics start at 16 384 output rows): the UNet at batch 16, 64 x 64
with the shared CFG prefix (dup carries statistics, the 32 x 32 Winograd output leaves them, C = 640 takes the table route, xtail leaves
them), at batch 2, 16 x 16 (no statistics anywhere) and at batch 2, 64 x 64 with the Winograd chain (the table route falls back to the
GroupNorm pass); the VAE at batch 1, 512 x 512 (halo layers, implicit-GEMM layers leaving 32-row statistics at 128 x 128, the c3 conv_in,
the fused conv_out); the text tower at capacity 2; the segmentation plan at batch 1 on a 96 x 64 image.
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def emit(name, x):
    a = np.ascontiguousarray(x.detach().cpu().numpy())
    assert a.size, name
    print(f"digest {name} {hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()}", flush=True)


def listing(name, g):
    """After a call: the recorder's launch list and what the library holds for its plan."""
    assert len(g.tags) == len(g.exec_tags) == len(g.alg_bytes)
    for i, ((tag, flops), ex, nbytes) in enumerate(zip(g.tags, g.exec_tags, g.alg_bytes)):
        print(f"launch {name} {i:04d} | {tag} | flops {flops} | executed {ex} | bytes {nbytes}")
    print(f"recorded {name} {g.model.num_launches(g.plan)} launches for {len(g.tags)} closures", flush=True)


def unets():
    from coma_amd.sd import weights
    from coma_amd.sd.unet import HipUNet2DConditionModel
    state = weights.random_state(weights.unet_shapes(), seed=0)
    for name, batch, hw, kw in (("b16_64_shared", 16, 64, dict(cfg_shared_prefix=True)), ("b2_16", 2, 16, {}),
                                ("b2_64_winograd", 2, 64, dict(winograd_min_batch=2))):
        gen = torch.Generator().manual_seed(7)
        half = torch.randn(batch // 2, 9, hw, hw, generator=gen).half().float()
        sample = torch.cat([half, half])                                      # the two CFG halves share sample and timestep
        ctx = torch.randn(batch, 77, 768, generator=gen).half().float()
        unet = HipUNet2DConditionModel(state, batch=batch, height=hw, width=hw, device=DEV, **kw)
        out = unet(sample.to(DEV), torch.full((batch,), 441.0).to(DEV), encoder_hidden_states=ctx.to(DEV))[0]
        listing(f"unet.{name}.step", unet.g)
        listing(f"unet.{name}.context", unet.gc)
        emit(f"unet.{name}.noise_pred", out)
        unet.g.model.close()
        del unet, out
        torch.cuda.empty_cache()


def vae():
    from coma_amd.sd import weights
    from coma_amd.sd.vae import HipAutoencoderKL
    state = weights.random_state(weights.vae_shapes(), seed=3)
    gen = torch.Generator().manual_seed(5)
    vae = HipAutoencoderKL(state, batch=1, height=512, width=512, device=DEV)
    image = vae.decode(torch.randn(1, 4, 64, 64, generator=gen).to(DEV))[0]
    listing("vae.decoder", vae.dec.g)
    emit("vae.decoder.image", image)
    dist = vae.encode((torch.rand(1, 3, 512, 512, generator=gen) * 2 - 1).to(DEV)).latent_dist
    listing("vae.encoder", vae.enc.g)
    emit("vae.encoder.moments", dist.moments)
    emit("vae.encoder.mode", dist.mode())
    vae.dec.g.model.close()
    vae.enc.g.model.close()


def text():
    from coma_amd.sd.text import HipCLIPTextModel
    from coma_amd.sd.weights import TEXT_CFG
    from tests import clip_ref
    cfg = dict(TEXT_CFG)
    enc = HipCLIPTextModel(clip_ref.random_text_state(cfg, seed=11, qk_gain=3.0), cfg, capacity=2, device=DEV)
    gen = torch.Generator().manual_seed(0)
    ids = torch.full((2, 77), 49407, dtype=torch.int64)                       # BOS, words, EOS padding
    for s, n in enumerate((9, 40)):
        ids[s, 0] = 49406
        ids[s, 1:1 + n] = torch.randint(0, 49406, (n,), generator=gen)
    out = enc(ids)[0]
    listing("text", enc.g)
    emit("text.last_hidden_state", out)
    enc.g.model.close()


def segmentation():
    from coma_amd.seg import weights as W
    from coma_amd.seg.model import HipPointRend
    state = W.random_state(seed=1, cls_gain=2.0, delta_gain=0.1, person_bias=3.0)
    image = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(1, 96, 64, 3)).astype(np.uint8))
    plan = HipPointRend(state, 1, 96, 64, DEV, score_thresh=0.2)
    out = plan(image.to(DEV))
    torch.cuda.synchronize()
    listing("seg", plan.g)
    n = int(out["count"][0])
    emit("seg.count", out["count"])
    for key in ("boxes", "scores", "classes", "valid", "masks"):              # rows past the count are never written
        if n:
            emit(f"seg.{key}", out[key][0, :n])
    emit("seg.person", out["person"])
    plan.g.model.close()


def main():
    from coma_amd import _lib
    assert torch.cuda.is_available(), "the digests are of device results"
    print(f"# library: {_lib.LIB_PATH}", file=sys.stderr)
    with torch.no_grad():
        for part in (unets, vae, text, segmentation):
            part()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
