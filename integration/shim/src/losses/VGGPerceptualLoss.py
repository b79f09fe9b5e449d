from smirk_amd.vgg_loss import VGGPerceptualLoss  # noqa: F401
