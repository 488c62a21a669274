"""Functional CPU restatement of ``VAE.encode`` (TEST INFRASTRUCTURE, next to oracle/vae_ref.py whose blocks it reuses).

Follows models/vae3d_dib.py:431-435 -> Encoder.forward (309-327) -> DownBlock (176-184), MidBlock (220-226) on a plain
``state_dict``; fp32.  ``emulate`` rounds to a 16-bit type where the HIP encoder stores: the (normalised) input, and after
every conv / norm / attention op up to norm_out + SiLU.  conv_out's sum and quant_conv stay fp32 (the head kernel
accumulates and finishes in fp32): conv_out's weight and bias are the rounded values, quant_conv's are used unrounded.
``emulate=None`` is the pure-fp32 reference mode (equal to the reference module: tests/test_vae_encode_cpu.py).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle.vae_ref import _gn, _r, resnet_block, volume_attention

Tensor = torch.Tensor


def normalise_payload(x: Tensor) -> Tensor:
    """The inverse of inference.py:345-346: SDF channel * 5, colour + material channels * 2 - 1."""
    return torch.cat([x[:, :1] * 5.0, x[:, 1:] * 2.0 - 1.0], dim=1)


def encoder_features(sd: Dict[str, Tensor], x: Tensor, emulate=None, normalize: bool = False,
                     down_channels: Sequence[int] = (32, 256), layers_per_block: int = 2, heads: int = 8) -> Tensor:
    """x: (P, 6, 8, 8, 8) -> silu(norm_out(...)) (P, 256, 4, 4, 4): the operand of the head."""
    x = x.float()
    if normalize:
        x = normalise_payload(x)
    x = _r(x, emulate)
    e = "encoder."
    x = _r(F.conv3d(x, _r(sd[e + "conv_in.weight"], emulate), _r(sd[e + "conv_in.bias"], emulate), padding=1), emulate)   # :313
    for i in range(len(down_channels)):                                                                                  # :316-317
        d = e + f"down_blocks.{i}."
        for j in range(layers_per_block):
            x = resnet_block(sd, d + f"nets.{j}.", x, emulate)
        if d + "downsample.weight" in sd:                                                      # Conv3d k3 s2 p1 (:168, 181-182)
            x = _r(F.conv3d(x, _r(sd[d + "downsample.weight"], emulate), _r(sd[d + "downsample.bias"], emulate), stride=2,
                            padding=1), emulate)
    m = e + "mid_block."
    x = resnet_block(sd, m + "nets.0.", x, emulate)
    x = volume_attention(sd, m + "attns.0.", x, heads, emulate)
    x = resnet_block(sd, m + "nets.1.", x, emulate)
    return _r(F.silu(_gn(sd, e + "norm_out.", x)), emulate)                                                              # :323-324


def head(sd: Dict[str, Tensor], h: Tensor, emulate=None) -> Tensor:
    """conv_out (:325) + quant_conv (:433) in fp32 on the (rounded) features."""
    y = F.conv3d(h, _r(sd["encoder.conv_out.weight"], emulate), _r(sd["encoder.conv_out.bias"], emulate), padding=1)
    return F.conv3d(y, sd["quant_conv.weight"], sd["quant_conv.bias"])


def vae_encode(sd: Dict[str, Tensor], x: Tensor, emulate: Optional[torch.dtype] = None, normalize: bool = False,
               down_channels: Sequence[int] = (32, 256), layers_per_block: int = 2, heads: int = 8) -> Tensor:
    """x: (P, 6, 8, 8, 8) -> the posterior's parameters (P, 2, 4, 4, 4)."""
    return head(sd, encoder_features(sd, x, emulate, normalize, down_channels, layers_per_block, heads), emulate)
