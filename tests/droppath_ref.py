"""Reference for stochastic depth (drop path) in the classifier's encoder: the oracle's block loop restated from the oracle's own
pieces, with the two residual adds of every block scaled per image.

  x_mid = x_in + s[2i][b] * attn(LN1(x_in)),      x_out = x_mid + s[2i + 1][b] * mlp(LN2(x_mid))

``scale`` is the engine's table, (2 * depth, B): row 2i the attention branch of block i, row 2i + 1 its MLP branch.  The scale is
applied in fp32 to the branch after the branch's bf16 rounding (the engine multiplies inside the LayerNorm kernel that adds the
stored bf16 branch to the fp32 residual stream).  Differentiable: the tests run it under autograd.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import mae_oracle as O


def _mlp(x, p, pfx, bf16):
    C = x.shape[-1]
    h = F.layer_norm(x, (C,), p[f"{pfx}.norm2.weight"], p[f"{pfx}.norm2.bias"], O.LN_EPS)
    h = O._linear(h, p[f"{pfx}.mlp.fc1.weight"], p[f"{pfx}.mlp.fc1.bias"], bf16)
    h = F.gelu(O._r(h, bf16))
    return O._r(O._linear(h, p[f"{pfx}.mlp.fc2.weight"], p[f"{pfx}.mlp.fc2.bias"], bf16), bf16)


def forward_encoder(p, cfg, images, scale, idx_keep=None, bf16=False):
    """O.forward_encoder with the per-image branch scales; an all-ones table gives O.forward_encoder bit for bit."""
    B = images.shape[0]
    scale = torch.as_tensor(scale, dtype=torch.float32)
    if scale.shape != (2 * cfg.depth, B):
        raise ValueError(f"scale must be ({2 * cfg.depth}, {B}), got {tuple(scale.shape)}")
    tok = O.patch_embed_all(images, p, cfg, bf16)
    tok = torch.cat([p["encoder.vit.cls_token"].expand(B, -1, -1), tok], dim=1)
    tok = tok + p["encoder.vit.pos_embed"]
    if idx_keep is not None:
        tok = torch.gather(tok, 1, idx_keep.unsqueeze(-1).expand(-1, -1, tok.shape[-1]))
    D = cfg.embed_dim
    for i in range(cfg.depth):
        pfx = f"encoder.vit.blocks.{i}"
        h = F.layer_norm(tok, (D,), p[f"{pfx}.norm1.weight"], p[f"{pfx}.norm1.bias"], O.LN_EPS)
        tok = tok + scale[2 * i][:, None, None] * O._attention(h, p, pfx, cfg.num_heads, bf16)
        tok = tok + scale[2 * i + 1][:, None, None] * _mlp(tok, p, pfx, bf16)
    return F.layer_norm(tok, (D,), p["encoder.vit.norm.weight"], p["encoder.vit.norm.bias"], O.LN_EPS)


def embedded_tokens(p, cfg, images, idx_keep=None, bf16=False):
    """[cls | patches] + pos_embed (the rows of idx_keep when given): the encoder's input to block 0."""
    B = images.shape[0]
    tok = O.patch_embed_all(images, p, cfg, bf16)
    tok = torch.cat([p["encoder.vit.cls_token"].expand(B, -1, -1), tok], dim=1) + p["encoder.vit.pos_embed"]
    if idx_keep is not None:
        tok = torch.gather(tok, 1, idx_keep.unsqueeze(-1).expand(-1, -1, tok.shape[-1]))
    return tok
