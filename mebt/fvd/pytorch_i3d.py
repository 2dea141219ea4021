"""import-name alias: `mebt.fvd.pytorch_i3d` (reference mebt/fvd/pytorch_i3d.py) -> mebt_amd.i3d (the HIP Inception-I3D)"""
from mebt_amd.i3d import InceptionI3d, InceptionModule, Unit3D, MaxPool3dSamePadding  # noqa: F401
