"""Import-path shim: ``from spec.losses import HMRCamLoss`` (spec/trainer.py:49 of the reference) resolves to the MI355X build
(the forward value computed on the device by specmi_hmr_loss)."""
from spec_amd.losses import HMRCamLoss, HMRLoss  # noqa: F401
