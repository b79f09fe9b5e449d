"""Which kernels smirk_backbone_forward launches for every block of the two encoder backbones (csrc/network.hip: backbone_plan).

For every case of tests/backbone_cases.py — both backbones with seeded synthetic weights, B = 2, three input sizes, six settings of the backbone's environment
switches, each set and unset around the single call — one forward runs between profile_start() and profile_stop(); the recorded launch names must equal EXPECTED.
EXPECTED was recorded by running this same table on the commit BEFORE the dispatch was rewritten around backbone_plan: the rewrite must choose what that commit
chose, block by block.  tests/test_backbone_dispatch_cpu.py holds the host-only query smirk_backbone_plan to the same table."""
import os

import pytest
import torch

import backbone_cases as BC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def encoders():
    from oracle import mobilenet_ref as M
    from smirk_amd import SmirkEncoder
    m = SmirkEncoder()
    m.load_state_dict(M.synth_encoder_state_dict(), strict=True)
    m = m.cuda().eval()
    return {"large": (m.shape_encoder.encoder, m.shape_encoder.shape_layers[0]), "small": (m.pose_encoder.encoder, m.pose_encoder.pose_cam_layers[0])}


def observe(encoders, backbone, hw, switches):
    """launch names of one smirk_backbone_forward with the switches set around it"""
    from oracle import assets as A
    from smirk_amd import _lib as L
    bb, head = encoders[backbone]
    img = A.synth_images(BC.B, seed=5)[:, :, :hw[0], :hw[1]].contiguous().cuda()
    env = BC.env_of(switches)
    os.environ.update(env)
    try:
        L.profile_start()
        try:
            with torch.no_grad():
                out, _ = bb.run(img, head)
        finally:
            recs = L.profile_stop()
    finally:
        for k in env:
            del os.environ[k]
    torch.cuda.synchronize()
    assert bb._split and torch.isfinite(out).all()                  # the split-fp16 schedule is the one with fused families
    return [r[0] for r in recs]


@pytest.mark.parametrize("case", sorted(BC.CASES))
def test_forward_launches_the_recorded_kernels(encoders, case):
    got = observe(encoders, *BC.CASES[case])
    assert got == BC.EXPECTED[case]
