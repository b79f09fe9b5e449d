"""BASELINE config 1 ("demo.py single image, plumbing"): a demo-style driver script, executed on top of the drop-in classes through the
`integration/shim` package, makes the calls INTEGRATION.md §2 lists for the reference's demo: `from src... import ...`, the three
constructors with the demo's arguments, the strict `load_state_dict` of a `smirk_encoder.` / `smirk_generator.`-prefixed checkpoint, `.eval()`,
`FLAME().to(...)`, `Renderer().to(...)`, then the first forward of the encoder on a host tensor — which must fail LOUDLY, because the HIP path has no
CPU fallback.  The driver is part of this test, so it runs wherever the repository does."""
import os
import runpy
import sys
import traceback

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the caller's side of INTEGRATION.md §2, written against the reference's module paths (resolved by integration/shim)
DEMO_DRIVER = """\
import argparse
import torch
from src.smirk_encoder import SmirkEncoder
from src.FLAME.FLAME import FLAME
from src.renderer.renderer import Renderer
import src.utils.masking as masking_utils

ap = argparse.ArgumentParser()
ap.add_argument("--device", default="cuda")
ap.add_argument("--checkpoint")
ap.add_argument("--use_smirk_generator", action="store_true")
args = ap.parse_args()

ckpt = torch.load(args.checkpoint)
encoder = SmirkEncoder().to(args.device)
encoder.load_state_dict({k[len("smirk_encoder."):]: v for k, v in ckpt.items() if k.startswith("smirk_encoder.")})
encoder.eval()
if args.use_smirk_generator:
    from src.smirk_generator import SmirkGenerator
    generator = SmirkGenerator(in_channels=6, out_channels=3, init_features=32, res_blocks=5).to(args.device)
    generator.load_state_dict({k[len("smirk_generator."):]: v for k, v in ckpt.items() if k.startswith("smirk_generator.")})
    generator.eval()
flame = FLAME().to(args.device)
renderer = Renderer().to(args.device)
face_probabilities = masking_utils.load_probabilities_per_FLAME_triangle()
image = torch.rand(1, 3, 224, 224, device=args.device)
outputs = encoder(image)   # first device call
"""


def test_demo_driver_runs_on_the_shim_until_the_first_device_call(in_sandbox, monkeypatch, tmp_path):
    from oracle import generator_ref as G, mobilenet_ref as M
    import smirk_amd
    # synthetic checkpoint in the reference's wire format (base_trainer.py:222-231): one flat dict, module-prefixed keys
    ckpt = {"smirk_encoder." + k: v for k, v in M.synth_encoder_state_dict().items()}
    ckpt.update({"smirk_generator." + k: v for k, v in G.synth_state_dict(calibrate=False).items()})
    ckpt_path = str(tmp_path / "SMIRK_em1.pt")
    torch.save(ckpt, ckpt_path)
    driver = str(tmp_path / "demo_driver.py")
    with open(driver, "w") as fh:
        fh.write(DEMO_DRIVER)
    for name in [n for n in sys.modules if n == "src" or n.startswith("src.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(os.path.join(REPO, "integration", "shim"))
    monkeypatch.setattr(sys, "argv", ["demo_driver.py", "--device", "cpu", "--checkpoint", ckpt_path, "--use_smirk_generator"])
    with pytest.raises(smirk_amd.SmirkHipError) as ei:
        runpy.run_path(driver, run_name="__main__")
    assert "no CPU fallback" in str(ei.value)
    frames = [f for f in traceback.extract_tb(ei.tb) if f.filename == driver]
    assert frames and "encoder(image)" in (frames[-1].line or ""), "the driver must have reached its first forward call"


def test_shim_exposes_the_reference_module_paths(monkeypatch):
    """every `from src... import ...` of demo.py:5-10, demo_video.py and smirk_trainer.py:4-8 resolves on the shim"""
    import importlib
    for name in [n for n in sys.modules if n == "src" or n.startswith("src.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(os.path.join(REPO, "integration", "shim"))
    for mod, names in (("src.smirk_encoder", ["SmirkEncoder"]), ("src.FLAME.FLAME", ["FLAME"]), ("src.renderer.renderer", ["Renderer"]),
                       ("src.smirk_generator", ["SmirkGenerator"]),
                       ("src.utils.masking", ["load_probabilities_per_FLAME_triangle", "mesh_based_mask_uniform_faces", "masking", "transfer_pixels",
                                              "point2ind", "triangle_area", "random_barycentric"])):
        m = importlib.import_module(mod)
        for n in names:
            assert hasattr(m, n), (mod, n)
        assert m.__file__.startswith(os.path.join(REPO, "integration", "shim"))


def test_graph_cycle_modules_refuses_eval_mode():
    """smirk_amd.cycle.graph_cycle_modules captures the TRAIN-mode path only (batch-statistics BatchNorm + backward); asking for it in eval mode is an error, raised
    before anything touches a device"""
    import torch
    from smirk_amd.cycle import CYCLE_GRAD_KEYS, _CycleEncoder, graph_cycle_modules

    class Tiny(torch.nn.Module):
        def forward(self, x):
            return {k: x.mean() * (i + 1) for i, k in enumerate(CYCLE_GRAD_KEYS + ("pose_params", "cam"))}

    g, e = torch.nn.Conv2d(6, 3, 1).eval(), Tiny().eval()
    with pytest.raises(ValueError):
        graph_cycle_modules(g, e, torch.zeros(1, 6, 16, 16), torch.zeros(1, 3, 16, 16))
    out = _CycleEncoder(Tiny())(torch.ones(1, 3, 4, 4, requires_grad=True))          # the wrapper detaches what the cycle loss does not differentiate
    assert all(out[k].requires_grad for k in CYCLE_GRAD_KEYS) and not out["pose_params"].requires_grad and not out["cam"].requires_grad
