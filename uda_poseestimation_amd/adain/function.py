"""API mirror of the reference's adain/function.py (calc_mean_std, adaptive_instance_normalization) on the AdaIN kernel.

Same semantics as lib/models/Style_net.py's functions of the same names (mean and sqrt(unbiased var + eps) over H*W), which are
the ones used here: NCHW fp32 in and out, the statistics and the blend computed in fp32 on the device.
"""
from ..lib.models.Style_net import adain as adaptive_instance_normalization
from ..lib.models.Style_net import calc_mean_std

__all__ = ["calc_mean_std", "adaptive_instance_normalization"]
