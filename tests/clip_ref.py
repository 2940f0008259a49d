"""Test helpers for the CLIP text tower: a plain-torch restatement of transformers' CLIPTextModel over a state dict (pinned against
transformers in tests/test_text_host.py), seeded weights, and a synthetic tokenizer directory (vocab.json / merges.txt learned by a tiny
BPE loop, tokenizer_config.json).  Nothing here is product code."""
from __future__ import annotations

import collections
import json
import math
import os

import torch

NEGATIVE_PROMPT = "worst quality, normal quality, low quality, bad anatomy, artifacts, blurry, cropped, watermark, greyscale, nsfw"

CORPUS = [
    NEGATIVE_PROMPT,
    "a person sitting on a chair", "a man riding a bicycle in the street", "a woman holding an umbrella in the rain",
    "a child playing with a dog on the grass", "a person lying on a bed, high quality photo", "two people sitting on a bench",
    "a person's hand holding a cup of coffee", "don't look at the camera, realistic photo, 8k, detailed",
    "best quality, masterpiece, ultra detailed, sharp focus", "a person standing next to a motorcycle", "a skateboard and a person",
]


def small_config(layers=2, heads=2, vocab=None, positions=77, intermediate=None):
    c = 64 * heads
    return dict(vocab_size=vocab, hidden_size=c, intermediate_size=intermediate or 4 * c, num_hidden_layers=layers, num_attention_heads=heads,
                max_position_embeddings=positions, hidden_act="quick_gelu", layer_norm_eps=1e-5, architectures=["CLIPTextModel"],
                model_type="clip_text_model")


def random_text_state(cfg, seed=0, qk_gain=3.0):
    """Seeded CLIPTextModel weights (keys without `text_model.`), fp16-representable; q / k projections scaled by qk_gain so that the
    softmax is sharp.  Embeddings ~ 0.5 N(0, 1) (the real tables are O(0.01 .. 1))."""
    from coma_amd.sd.weights import text_shapes
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shp in sorted(text_shapes(cfg).items()):
        if "embedding" in name:
            t = 0.5 * torch.randn(shp, generator=g)
        elif name.endswith("weight") and len(shp) == 2:
            t = torch.randn(shp, generator=g) / math.sqrt(shp[1])
            if "q_proj" in name or "k_proj" in name:
                t = t * qk_gain
        elif name.endswith("weight"):
            t = 1.0 + 0.1 * torch.randn(shp, generator=g)
        else:
            t = 0.05 * torch.randn(shp, generator=g)
        out[name] = t.to(torch.float16).float()
    return out


def clip_text_ref(state, cfg, ids, dtype=torch.float32):
    """last_hidden_state of CLIPTextModel(input_ids=ids) (no attention mask: only the causal one), every op in `dtype`."""
    s = {k: v.to(ids.device, dtype) for k, v in state.items()}
    C, H = cfg["hidden_size"], cfg["num_attention_heads"]
    d, eps = C // H, cfg["layer_norm_eps"]
    S, L = ids.shape
    ln = lambda x, p: torch.nn.functional.layer_norm(x, (C,), s[p + ".weight"], s[p + ".bias"], eps)
    lin = lambda x, p: torch.nn.functional.linear(x, s[p + ".weight"], s[p + ".bias"])
    x = s["embeddings.token_embedding.weight"][ids.long()] + s["embeddings.position_embedding.weight"][:L]
    mask = torch.full((L, L), float("-inf"), device=ids.device).triu(1).to(dtype)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}"
        h = ln(x, p + ".layer_norm1")
        q, k, v = (lin(h, f"{p}.self_attn.{n}").view(S, L, H, d).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        w = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, dim=-1)
        a = (w @ v).transpose(1, 2).reshape(S, L, C)
        x = x + lin(a, p + ".self_attn.out_proj")
        h = lin(ln(x, p + ".layer_norm2"), p + ".mlp.fc1")
        x = x + lin(h * torch.sigmoid(1.702 * h), p + ".mlp.fc2")
    return ln(x, "final_layer_norm")


# ---------------------------------------------------------------------------------------------- synthetic tokenizer
def learn_tokenizer(path, texts=CORPUS, n_merges=300, model_max_length=77):
    """vocab.json (256 byte symbols, their `</w>` forms, the learned merges, BOS, EOS), merges.txt (`#version` header + n_merges pairs
    learned by counting adjacent symbol pairs over the pre-tokenised corpus), tokenizer_config.json (max length 77, pad = EOS)."""
    from coma_amd.sd.tokenizer import bytes_to_unicode, normalize, pre_tokenize
    os.makedirs(path, exist_ok=True)
    be = bytes_to_unicode()
    symbols = [be[b] for b in range(256)]
    vocab = {c: i for i, c in enumerate(symbols)}
    for c in symbols:
        vocab[c + "</w>"] = len(vocab)
    words = collections.Counter()
    for t in texts:
        for piece in pre_tokenize(normalize(t)):
            w = [be[b] for b in piece.encode("utf-8")]
            w[-1] += "</w>"
            words[tuple(w)] += 1
    merges = []
    for _ in range(n_merges):
        pairs = collections.Counter()
        for w, n in words.items():
            for a, b in zip(w, w[1:]):
                pairs[(a, b)] += n
        if not pairs:
            break
        best = max(pairs, key=lambda p: (pairs[p], p))
        merges.append(best)
        if best[0] + best[1] not in vocab:
            vocab[best[0] + best[1]] = len(vocab)
        nw = collections.Counter()
        for w, n in words.items():
            out, k = [], 0
            while k < len(w):
                if k < len(w) - 1 and (w[k], w[k + 1]) == best:
                    out.append(w[k] + w[k + 1])
                    k += 2
                else:
                    out.append(w[k])
                    k += 1
            nw[tuple(out)] += n
        words = nw
    vocab["<|startoftext|>"] = len(vocab)
    vocab["<|endoftext|>"] = len(vocab)
    with open(os.path.join(path, "vocab.json"), "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=False)
    with open(os.path.join(path, "merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in merges))
    with open(os.path.join(path, "tokenizer_config.json"), "w") as f:
        json.dump({"model_max_length": model_max_length, "bos_token": "<|startoftext|>", "eos_token": "<|endoftext|>",
                   "pad_token": "<|endoftext|>", "unk_token": "<|endoftext|>", "tokenizer_class": "CLIPTokenizer"}, f)
    return vocab, merges


def write_text_encoder(path, state, cfg, prefix="text_model.", fmt="safetensors", dtype=torch.float16):
    """A `text_encoder/` directory: config.json + model.safetensors (or pytorch_model.bin) with keys under `prefix`."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    st = {prefix + k: v.to(dtype).contiguous() for k, v in state.items()}
    st[prefix + "embeddings.position_ids"] = torch.arange(cfg["max_position_embeddings"]).unsqueeze(0)
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(st, os.path.join(path, "model.safetensors"))
    else:
        torch.save(st, os.path.join(path, "pytorch_model.bin"))
