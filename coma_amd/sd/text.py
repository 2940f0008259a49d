"""CLIP text tower (SD-1.x: transformers' CLIPTextModel, hidden 768, 12 layers, 12 heads of 64, quick_gelu) on MI355X as one recorded
launch list in a library-owned model (plan "text", bindings "ids" / "text_out"), the fourth network of the inpainting loop.

The reference encodes prompts with ``self.text_encoder(text_input_ids)[0]`` in eager fp16 (utils/adaptive_mask_inpainting.py:459-482,
src/generation/inpaint.py:64).  Per layer: LayerNorm -> one q|k|v product -> causal attention (sd_attention_causal_f16, reading q, k and v
in place) -> out_proj + residual -> LayerNorm -> fc1 + quick_gelu (SD_EPI_QUICK_GELU) -> fc2 + residual; the token + position embedding
before (sd_text_embed_f16) and the final LayerNorm after: 7 launches per layer + 2.
"""
from __future__ import annotations

import os

import torch

from . import ops
from .graph import F16, LaunchGraph
from .weights import TEXT_CFG, check_state, check_text_config, load_text_encoder, strip_text_prefix, text_shapes


class HipCLIPTextModel:
    """Drop-in for what the pipeline's ``_encode_prompt`` calls: ``model(input_ids)`` with int64 / int32 ids [S, L] (L = the tower's
    positions, 77 for SD-1.x) on the host or the device -> ``(last_hidden_state fp16 [S, L, hidden],)``.

    The plan is recorded once at a fixed sequence capacity; a call with any S is padded / chunked to it, so a row's result never depends on
    the other rows of the call.  The returned tensor is a fresh tensor (never a view of the plan's output buffer): two successive calls do
    not alias."""

    def __init__(self, state, config=None, capacity=16, device="cuda"):
        cfg = check_text_config(config if config is not None else TEXT_CFG)
        state = check_state(strip_text_prefix(state), text_shapes(cfg), "CLIP text encoder")
        if capacity <= 0:
            raise ValueError("capacity must be positive")
        self.config = cfg
        self.device = torch.device(device)
        self.dtype = F16
        self.capacity = cap = int(capacity)
        self.seq_len = L = int(cfg["max_position_embeddings"])
        self.vocab = int(cfg["vocab_size"])
        C, I, H = int(cfg["hidden_size"]), int(cfg["intermediate_size"]), int(cfg["num_attention_heads"])
        self.hidden = C
        eps = float(cfg["layer_norm_eps"])
        s = {k: v.to(self.device, F16).contiguous() for k, v in state.items()}
        g = self.g = LaunchGraph(self.device, plan="text")
        rows = cap * L
        self.ids = g.buf(cap, L, dtype=torch.int32, zero=True)
        self.out = g.buf(cap, L, C, zero=True)
        x, h, a, x2 = g.buf(rows, C), g.buf(rows, C), g.buf(rows, C), g.buf(rows, C)
        qkv, f = g.buf(rows, 3 * C), g.buf(rows, I)
        qkv_flat = qkv.view(-1)
        g.text_embed(self.ids, s["embeddings.token_embedding.weight"], s["embeddings.position_embedding.weight"], x, seqs=cap, len_=L)
        for i in range(cfg["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            at = p + "self_attn."
            wqkv = torch.cat([s[at + "q_proj.weight"], s[at + "k_proj.weight"], s[at + "v_proj.weight"]]).contiguous()
            bqkv = torch.cat([s[at + "q_proj.bias"], s[at + "k_proj.bias"], s[at + "v_proj.bias"]]).contiguous()
            g.layernorm(x, s[p + "layer_norm1.weight"], s[p + "layer_norm1.bias"], h, rows=rows, c=C, eps=eps)
            g.conv(h, wqkv, qkv, batch=rows, in_h=1, in_w=1, c0=C, n=3 * C, bias=bqkv)
            # q, k, v: the three column blocks of the fused product, read in place (views starting at columns 0, C, 2C; leading dim 3C)
            g.attention_causal(qkv_flat[0:], qkv_flat[C:], qkv_flat[2 * C:], a, seqs=cap, heads=H, len_=L, d=C // H, ldq=3 * C, ldk=3 * C,
                               ldv=3 * C, ldo=C)
            g.conv(a, s[at + "out_proj.weight"], x2, batch=rows, in_h=1, in_w=1, c0=C, n=C, bias=s[at + "out_proj.bias"], res=x)
            g.layernorm(x2, s[p + "layer_norm2.weight"], s[p + "layer_norm2.bias"], h, rows=rows, c=C, eps=eps)
            g.conv(h, s[p + "mlp.fc1.weight"], f, batch=rows, in_h=1, in_w=1, c0=C, n=I, bias=s[p + "mlp.fc1.bias"], epi=ops.EPI_QUICK_GELU)
            g.conv(f, s[p + "mlp.fc2.weight"], x, batch=rows, in_h=1, in_w=1, c0=I, n=C, bias=s[p + "mlp.fc2.bias"], res=x2)
        g.layernorm(x, s["final_layer_norm.weight"], s["final_layer_norm.bias"], self.out.view(rows, C), rows=rows, c=C, eps=eps)
        g.model.bind("ids", self.ids)
        g.model.bind("text_out", self.out)

    @classmethod
    def from_pretrained(cls, text_dir, capacity=16, device="cuda"):
        """A checkpoint's `text_encoder/` directory (config.json + model.safetensors or pytorch_model.bin)."""
        cfg, state = load_text_encoder(os.fspath(text_dir))
        return cls(state, cfg, capacity=capacity, device=device)

    @property
    def num_launches(self):
        return len(self.g.launches)

    def _check_ids(self, input_ids):
        ids = torch.as_tensor(input_ids)
        if ids.dtype not in (torch.int64, torch.int32):
            raise TypeError(f"input_ids must be int64 or int32 (got {ids.dtype})")
        if ids.dim() != 2 or ids.shape[1] != self.seq_len:
            raise ValueError(f"input_ids must be [S, {self.seq_len}] (got {tuple(ids.shape)})")
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.vocab):
            raise ValueError(f"input_ids out of range [0, {self.vocab}): min {int(ids.min())}, max {int(ids.max())}")
        return ids

    @torch.no_grad()
    def __call__(self, input_ids):
        ids = self._check_ids(input_ids).to(self.device, torch.int32)
        S, L, cap = ids.shape[0], self.seq_len, self.capacity
        out = torch.empty(S, L, self.hidden, dtype=F16, device=self.device)
        with torch.cuda.device(self.device):
            for c0 in range(0, S, cap):
                n = min(cap, S - c0)
                self.ids[:n].copy_(ids[c0:c0 + n])
                if n < cap:
                    self.ids[n:].zero_()                  # padding rows: valid ids, their results are dropped
                self.g.replay()
                out[c0:c0 + n].copy_(self.out[:n])
        return (out,)

    def save(self, path):
        """The model file sd_model_load + sd_text_encode run without Python (ids int32 [capacity, L] -> fp16 [capacity, L, hidden])."""
        self.g.capture()
        self.g.model.save(path)
