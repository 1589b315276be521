"""Import-path shim: ``from camcalib.loss import CameraRegressorLoss`` (camcalib/trainer.py:31 of the reference) and its two leaf
criteria resolve to the MI355X build."""
from spec_amd.losses import CameraRegressorLoss, KLDivergence, SoftargmaxClsLoss  # noqa: F401
