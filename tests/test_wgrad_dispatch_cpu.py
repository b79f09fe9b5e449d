"""smirk_conv_wgrad_workspace_bytes pinned, without a GPU (the query is a pure host function of the layer's shape: csrc/wgrad.hip wgrad_plan / wgrad_nsplit).

The bytes are nsplit * Cout * k * k * Cin * 4, so they pin the split count the launch will use — and with it the summation order of the gradient.  Pinned for the tiny
layers of tests/wgrad_cases.py (one per branch of the dispatch) and for the same (Cout, Cin, k) at B = 64 and every resolution of the generator, one pointwise layer per
encoder stage, and the three layers whose shape takes the halo family's split count although the tiled kernel serves them (the query is told neither the padding mode
nor, for a 1x1 layer, that there are no nine taps; a W that is no multiple of 16 it could see, and the recorded rule does not look): there the caps of the split rule
bite and the 1536 / 1024 workgroups show.  Every number was recorded by running these tables on the commit BEFORE the dispatch was rewritten around WgradPlan.
The >= 2 GiB fallback changes the kernel, not the split; tests/test_train_scale_gpu.py keeps covering it on the GPU."""
import pytest

import wgrad_cases as WC
from smirk_amd import _lib as L

# Recorded on the parent commit (see the module docstring): bytes, and for the reader the split count they imply.
EXPECTED_SMALL = {
    '1x1_convtranspose': 32768,  # 1
    '1x1_final': 1024,  # 1
    'halo_32_32': 73728,  # 2
    'halo_32_64': 147456,  # 2
    'halo_64_32': 147456,  # 2
    'halo_64_64': 294912,  # 2
    'halo_split_tiled_1x1_n288': 36864,  # 1
    'halo_split_tiled_w8': 147456,  # 4
    'reflect': 737280,  # 5
    'tile128': 147456,  # 1
    'tile128_ragged': 82944,  # 1
    'tile32': 9216,  # 1
    'tile64': 18432,  # 1
    'tile64_ragged': 11520,  # 1
}
# per generator layer (Cout, Cin, k): bytes at B = 64, H = W = 224, 112, 56, 28, 14
EXPECTED_GENERATOR = {
    (32, 8, 3): [4718592, 4718592, 4718592, 4718592, 4718592],  # 512 512 512 512 512
    (32, 32, 3): [56623104, 56623104, 56623104, 56623104, 28901376],  # 1536 1536 1536 1536 784
    (64, 32, 3): [113246208, 113246208, 113246208, 113246208, 57802752],  # 1536 1536 1536 1536 784
    (64, 64, 3): [150994944, 150994944, 150994944, 150994944, 115605504],  # 1024 1024 1024 1024 784
    (32, 64, 3): [113246208, 113246208, 113246208, 113246208, 57802752],  # 1536 1536 1536 1536 784
    (128, 64, 3): [60162048, 60162048, 60162048, 60162048, 60162048],  # 204 204 204 204 204
    (128, 128, 3): [66650112, 66650112, 66650112, 66650112, 66650112],  # 113 113 113 113 113
    (256, 128, 3): [66060288, 66060288, 66060288, 66060288, 66060288],  # 56 56 56 56 56
    (256, 256, 3): [66060288, 66060288, 66060288, 66060288, 66060288],  # 28 28 28 28 28
    (512, 256, 3): [66060288, 66060288, 66060288, 66060288, 66060288],  # 14 14 14 14 14
    (512, 512, 3): [66060288, 66060288, 66060288, 66060288, 66060288],  # 7 7 7 7 7
    (512, 1024, 1): [67108864, 67108864, 67108864, 67108864, 67108864],  # 32 32 32 32 32
    (256, 512, 1): [67108864, 67108864, 67108864, 67108864, 67108864],  # 128 128 128 128 128
    (128, 256, 1): [67108864, 67108864, 67108864, 67108864, 67108864],  # 512 512 512 512 512
    (64, 128, 1): [16777216, 16777216, 16777216, 16777216, 16777216],  # 512 512 512 512 512
    (8, 32, 1): [524288, 524288, 524288, 524288, 524288],  # 512 512 512 512 512
}
EXPECTED_ENCODER = {
    'enc_112': 524288,  # 512
    'enc_14': 14155776,  # 512
    'enc_28': 4718592,  # 512
    'enc_56': 2359296,  # 512
    'enc_7': 43352064,  # 196
}
EXPECTED_HALO_SPLIT_TILED = {
    'halo_split_tiled_1x1_n288': 56623104,  # 1536
    'halo_split_tiled_w8': 56623104,  # 1536
    'reflect': 150994944,  # 1024
}


def query(shape):
    B, H, W, Cout, Cin, k, _ = shape                               # (no reflect argument: the split rule cannot depend on it)
    return L.lib().smirk_conv_wgrad_workspace_bytes(B, H, W, Cout, Cin, k)


def splits(shape, nbytes):
    _, _, _, Cout, Cin, k, _ = shape
    assert nbytes % (Cout * k * k * Cin * 4) == 0
    return nbytes // (Cout * k * k * Cin * 4)


@pytest.mark.parametrize("case", sorted(WC.CASES))
def test_workspace_of_the_smallest_layer_of_each_branch(case):
    assert query(WC.CASES[case]) == EXPECTED_SMALL[case]


@pytest.mark.parametrize("layer", WC.GENERATOR_LAYERS, ids=lambda l: "%dx%dk%d" % l)
def test_workspace_of_the_generator_layers_at_every_resolution(layer):
    cout, cin, k = layer
    got = [query((WC.LARGE_B, r, r, cout, cin, k, 0)) for r in WC.RESOLUTIONS]
    assert got == EXPECTED_GENERATOR[layer]


@pytest.mark.parametrize("case", sorted(WC.ENCODER_POINTWISE))
def test_workspace_of_one_pointwise_layer_per_encoder_stage(case):
    assert query(WC.ENCODER_POINTWISE[case]) == EXPECTED_ENCODER[case]


@pytest.mark.parametrize("case", sorted(WC.HALO_SPLIT_TILED_LARGE))
def test_halo_split_count_on_layers_the_tiled_kernel_serves(case):
    shape = WC.HALO_SPLIT_TILED_LARGE[case]
    got = query(shape)
    assert got == EXPECTED_HALO_SPLIT_TILED[case]
    assert splits(shape, got) == (1024 if shape[3] == 64 and shape[5] ** 2 * shape[4] == 576 else 1536), "beyond the tiled family's cap of 512"
