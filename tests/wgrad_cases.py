"""Case table of the weight-gradient dispatch (a plain module shared by tests/test_wgrad_dispatch_cpu.py and tests/test_wgrad_dispatch_gpu.py).

Every case is the smallest layer that reaches one branch of wgrad_plan (csrc/wgrad.hip): kernel family (tiled / halo), tile height, 1x1 forms, reflect padding, and the
layers that take the halo family's split count on the tiled kernel because the split rule sees the shape only.  Layer = (B, H, W, Cout, Cin, k, reflect)."""

CASES = {
    "tile32": (1, 4, 4, 32, 8, 3, 0),
    "tile64": (1, 4, 4, 64, 8, 3, 0),
    "tile64_ragged": (1, 4, 4, 40, 8, 3, 0),
    "tile128": (1, 4, 4, 128, 32, 3, 0),
    "tile128_ragged": (1, 4, 4, 72, 32, 3, 0),
    "1x1_convtranspose": (1, 4, 4, 64, 128, 1, 0),
    "1x1_final": (1, 4, 4, 8, 32, 1, 0),
    "reflect": (2, 6, 6, 64, 64, 3, 1),                     # also a halo-shaped split on the tiled kernel
    "halo_32_32": (1, 2, 16, 32, 32, 3, 0),
    "halo_64_32": (1, 2, 16, 64, 32, 3, 0),
    "halo_32_64": (1, 2, 16, 32, 64, 3, 0),
    "halo_64_64": (1, 2, 16, 64, 64, 3, 0),
    "halo_split_tiled_w8": (1, 8, 8, 32, 32, 3, 0),         # W % 16 != 0
    "halo_split_tiled_1x1_n288": (1, 4, 4, 32, 288, 1, 0),  # N = 288 without nine taps
}

# The (Cout, Cin, k) of the generator's training step (init_features = 32): double convolutions and decoder halves, ConvTranspose2d as its 1x1 form (Cout = the
# layer's input channels, Cin = 4 x its output channels), residual blocks, final 1x1 (8 padded output channels).  The workspace query is pinned for each of them
# at B = 64 and every resolution of the network, whatever stage the layer itself lives at: that is where the caps of the split rule bite.
GENERATOR_LAYERS = [(32, 8, 3), (32, 32, 3), (64, 32, 3), (64, 64, 3), (32, 64, 3), (128, 64, 3), (128, 128, 3), (256, 128, 3), (256, 256, 3), (512, 256, 3),
                    (512, 512, 3), (512, 1024, 1), (256, 512, 1), (128, 256, 1), (64, 128, 1), (8, 32, 1)]
RESOLUTIONS = (224, 112, 56, 28, 14)
LARGE_B = 64

# one pointwise layer per encoder stage (B, H, W, Cout, Cin, 1, 0)
ENCODER_POINTWISE = {
    "enc_112": (64, 112, 112, 16, 16, 1, 0),
    "enc_56": (64, 56, 56, 72, 16, 1, 0),
    "enc_28": (64, 28, 28, 96, 24, 1, 0),
    "enc_14": (64, 14, 14, 144, 48, 1, 0),
    "enc_7": (64, 7, 7, 576, 96, 1, 0),
}

# the three halo-shaped splits on the tiled kernel at a size where the 1536 / 1024 workgroups show
HALO_SPLIT_TILED_LARGE = {
    "halo_split_tiled_w8": (64, 64, 64, 32, 32, 3, 0),
    "halo_split_tiled_1x1_n288": (64, 64, 64, 32, 288, 1, 0),
    "reflect": (64, 64, 64, 64, 64, 3, 1),
}
