#!/usr/bin/env python3
"""Generates tests/golden/unet_attn_long.npz by importing the REFERENCE (as make_golden.py does): one UNet
forward of a tiny config whose attention runs over more than 1024 tokens.

Config: inner_channel 32, channel_mults (1, 2), attn_res (64,), image_size 64, res_blocks 1, B = 1, input
68 x 68. Attention covers 68 x 68 = 4624 tokens at C = 32 (full-resolution level, down and up path) and
34 x 34 = 1156 tokens at C = 64 (the mid block); neither count is a multiple of 32. Weights come from the
seed (synth.synth_state_dict), so the fixture holds only x, the noise level, eps and meta.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (reference imports, save / meta helpers)

NAME = "unet_attn_long.npz"


def attn_long_config():
    return mg.graph.UNetConfig(in_channel=6, out_channel=3, inner_channel=32, norm_groups=32, channel_mults=(1, 2),
                               attn_res=(64,), res_blocks=1, dropout=0.0, image_size=64)


if __name__ == "__main__":
    print("unet tiny, attention over 4624 / 1156 tokens (68 x 68)")
    mg.gen_unet(NAME, attn_long_config(), B=1, r=68, seed=21)
