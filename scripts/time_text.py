#!/usr/bin/env python3
"""Per-call time of the CLIP text tower (SD-1.5 size, seeded weights) for 16 sequences of 77 tokens: the device tower (HipCLIPTextModel,
one hipGraph replay + the id / output copies) against transformers' CLIPTextModel in eager fp16 on the same GPU when transformers imports,
and the error of both against the fp32 restatement of tests/clip_ref.py.

    python scripts/time_text.py [--seqs 16] [--reps 50]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from coma_amd.sd.text import HipCLIPTextModel  # noqa: E402
from coma_amd.sd.weights import TEXT_CFG  # noqa: E402
from tests import clip_ref  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = "cuda"
    cfg = dict(TEXT_CFG)
    state = clip_ref.random_text_state(cfg, seed=0)
    g = torch.Generator().manual_seed(1)
    ids = torch.full((a.seqs, 77), 49407, dtype=torch.int64)
    ids[:, 0] = 49406
    ids[:, 1:21] = torch.randint(0, 49406, (a.seqs, 20), generator=g)
    ids_d = ids.to(dev)
    enc = HipCLIPTextModel(state, cfg, capacity=a.seqs, device=dev)
    ref32 = clip_ref.clip_text_ref(state, cfg, ids_d)
    got = enc(ids_d)[0]
    err = (got.float() - ref32).abs()
    ms = timed(lambda: enc(ids_d), a.reps)
    print(f"device tower: {a.seqs} x 77 tokens, {enc.num_launches} launches, {ms:.3f} ms per call; "
          f"error vs fp32 restatement max {float(err.max()):.3e} mean {float(err.mean()):.3e}")
    r16 = (clip_ref.clip_text_ref(state, cfg, ids_d, torch.float16).float() - ref32).abs()
    print(f"torch fp16 restatement: error vs fp32 max {float(r16.max()):.3e} mean {float(r16.mean()):.3e}")
    try:
        import transformers
    except ImportError:
        print("transformers: not importable, no comparison")
        return
    tcfg = transformers.CLIPTextConfig(vocab_size=cfg["vocab_size"], hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                                       num_attention_heads=12, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5)
    with torch.device(dev):
        model = transformers.CLIPTextModel(tcfg).half().eval()
    prefix = "text_model." if any(k.startswith("text_model.") for k in model.state_dict()) else ""      # transformers 5: no prefix
    model.load_state_dict({prefix + k: v.half() for k, v in state.items()}, strict=False)
    with torch.no_grad():
        want = model(input_ids=ids_d).last_hidden_state
        terr = (want.float() - ref32).abs()
        tms = timed(lambda: model(input_ids=ids_d), a.reps)
    print(f"transformers {transformers.__version__} CLIPTextModel fp16 ({model.config._attn_implementation}): {tms:.3f} ms per call; "
          f"error vs fp32 restatement max {float(terr.max()):.3e} mean {float(terr.mean()):.3e}")
    print(f"device tower vs transformers fp16: max |diff| {float((got.float() - want.float()).abs().max()):.3e}; speed ratio {tms / ms:.2f}x")


if __name__ == "__main__":
    main()
