"""Mirror of maskrcnn_benchmark/layers/dcn: the deformable convolutions (the deformable RoI poolers live in layers/__init__.py)."""
from .deform_conv_func import DeformConvFunction, ModulatedDeformConvFunction, deform_conv, modulated_deform_conv
from .deform_conv_module import Conv2d, DeformConv, ModulatedDeformConv, ModulatedDeformConvPack

__all__ = ["DeformConvFunction", "ModulatedDeformConvFunction", "deform_conv", "modulated_deform_conv", "Conv2d", "DeformConv",
           "ModulatedDeformConv", "ModulatedDeformConvPack"]
