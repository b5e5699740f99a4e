"""abr_iod_amd.layers mirrors the names of maskrcnn_benchmark/layers/__init__.py that it carries: code written against the reference's `layers`
package imports them from ours, the poolers' modules have the reference's constructor arguments and __repr__, and the two Pack modules have
the reference's state-dict keys and shapes, so a reference checkpoint loads.  CPU only: nothing here launches a kernel."""
import inspect

import pytest
import torch

# __all__ of the reference's layers/__init__.py:23-46
REFERENCE_ALL = ["nms", "roi_align", "ROIAlign", "roi_pool", "ROIPool", "smooth_l1_loss", "Conv2d", "DFConv2d", "ConvTranspose2d", "interpolate",
                 "BatchNorm2d", "FrozenBatchNorm2d", "SigmoidFocalLoss", "deform_conv", "modulated_deform_conv", "DeformConv", "ModulatedDeformConv",
                 "ModulatedDeformConvPack", "deform_roi_pooling", "DeformRoIPooling", "DeformRoIPoolingPack", "ModulatedDeformRoIPoolingPack"]
# not carried: the generic convolution wrappers (the model's convolutions are modeling/backbone's fused blocks) and the deformable-conv layer
# classes (the body's DCN runs specialised 3x3 kernels)
NOT_CARRIED = {"Conv2d", "DFConv2d", "ConvTranspose2d", "interpolate", "BatchNorm2d", "deform_conv", "modulated_deform_conv", "DeformConv",
               "ModulatedDeformConv", "ModulatedDeformConvPack"}
SIX = ["ROIPool", "roi_pool", "deform_roi_pooling", "DeformRoIPooling", "DeformRoIPoolingPack", "ModulatedDeformRoIPoolingPack"]


def test_the_six_names_import():
    from abr_iod_amd.layers import (DeformRoIPooling, DeformRoIPoolingPack, ModulatedDeformRoIPoolingPack, ROIPool,  # noqa: F401
                                    deform_roi_pooling, roi_pool)
    assert callable(roi_pool) and callable(deform_roi_pooling)
    assert issubclass(DeformRoIPoolingPack, DeformRoIPooling) and issubclass(ModulatedDeformRoIPoolingPack, DeformRoIPooling)


def test_reference_all_is_carried():
    from abr_iod_amd import layers
    want = [n for n in REFERENCE_ALL if n not in NOT_CARRIED]
    assert set(SIX) <= set(want)
    missing = [n for n in want if n not in dir(layers)]
    assert not missing, missing


def test_C_module_carries_the_poolers():
    from abr_iod_amd import _C
    for name in ("roi_pool_forward", "roi_pool_backward", "deform_psroi_pooling_forward", "deform_psroi_pooling_backward"):
        assert callable(getattr(_C, name)), name
    x = torch.zeros(1, 4, 5, 5)
    with pytest.raises(RuntimeError):                      # CPU tensors raise, like the rest of the module
        _C.roi_pool_forward(x, torch.zeros(1, 5), 1.0, 2, 2)
    with pytest.raises(RuntimeError):
        _C.deform_psroi_pooling_forward(x, torch.zeros(1, 5), x.new_empty(0), torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2), True, 1.0, 4, 1, 2, 2, 2, 0.0)


def test_constructor_arguments_and_repr():
    from abr_iod_amd import layers
    assert list(inspect.signature(layers.ROIPool.__init__).parameters)[1:] == ["output_size", "spatial_scale"]
    assert list(inspect.signature(layers.ROIPool.forward).parameters)[1:] == ["input", "rois"]
    assert repr(layers.ROIPool((7, 7), 0.0625)) == "ROIPool(output_size=(7, 7), spatial_scale=0.0625)"
    base = ["spatial_scale", "out_size", "out_channels", "no_trans", "group_size", "part_size", "sample_per_part", "trans_std"]
    sig = inspect.signature(layers.DeformRoIPooling.__init__).parameters
    assert list(sig)[1:] == base
    assert [sig[n].default for n in base[4:]] == [1, None, 4, .0]
    assert list(inspect.signature(layers.DeformRoIPooling.forward).parameters)[1:] == ["data", "rois", "offset"]
    for cls in (layers.DeformRoIPoolingPack, layers.ModulatedDeformRoIPoolingPack):
        sig = inspect.signature(cls.__init__).parameters
        assert list(sig)[1:] == base + ["deform_fc_channels"] and sig["deform_fc_channels"].default == 1024
        assert list(inspect.signature(cls.forward).parameters)[1:] == ["data", "rois"]
    assert layers.DeformRoIPooling(0.0625, 7, 256, True).part_size == 7             # part_size None -> out_size
    assert list(inspect.signature(layers.deform_roi_pooling).parameters)[:11] == ["data", "rois", "offset"] + base


def test_pack_state_dict_is_the_references():
    from abr_iod_amd import layers
    m = layers.DeformRoIPoolingPack(0.0625, 7, 256, False, deform_fc_channels=1024)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert sd == {"offset_fc.0.weight": (1024, 12544), "offset_fc.0.bias": (1024,), "offset_fc.2.weight": (1024, 1024), "offset_fc.2.bias": (1024,),
                  "offset_fc.4.weight": (98, 1024), "offset_fc.4.bias": (98,)}
    mm = layers.ModulatedDeformRoIPoolingPack(0.0625, 7, 256, False, deform_fc_channels=1024)
    sdm = {k: tuple(v.shape) for k, v in mm.state_dict().items()}
    assert sdm == dict(sd, **{"mask_fc.0.weight": (1024, 12544), "mask_fc.0.bias": (1024,), "mask_fc.2.weight": (49, 1024), "mask_fc.2.bias": (49,)})
    assert set(sd) == {n for n, _ in m.named_parameters()} and set(sdm) == {n for n, _ in mm.named_parameters()}
    # the zero initialisations (deform_pool_module.py:63-64,116-117,125-126), and nothing else is zero
    for mod, names in ((m, ["offset_fc.4"]), (mm, ["offset_fc.4", "mask_fc.2"])):
        state = mod.state_dict()
        for k, v in state.items():
            zero = any(k.startswith(n + ".") for n in names)
            assert bool((v == 0).all()) == zero, k
    assert mm.offset_fc[-1].weight is mm.offset_fc[4].weight and mm.mask_fc[2].bias.shape == (49,)
    # indices run over the reference Sequential's slots: linear layers at the even ones, negative indices from the end
    assert mm.offset_fc[-3] is mm.offset_fc[2] and mm.offset_fc[-5] is mm.offset_fc[0] and mm.mask_fc[-1] is mm.mask_fc[2]
    for bad in (-2, 1, 5, -6):
        with pytest.raises(IndexError):
            mm.offset_fc[bad]
    # no_trans: no FC stack at all
    assert not list(layers.DeformRoIPoolingPack(0.0625, 7, 256, True).parameters())
    # a reference-keyed state dict loads strictly, and the values arrive
    ref_sd = {k: torch.randn(s) for k, s in sdm.items()}
    mm.load_state_dict(ref_sd, strict=True)
    for k, v in mm.state_dict().items():
        assert torch.equal(v, ref_sd[k]), k


def test_pack_refuses_channel_counts_it_cannot_contract():
    from abr_iod_amd import layers
    for cls in (layers.DeformRoIPoolingPack, layers.ModulatedDeformRoIPoolingPack):
        with pytest.raises(NotImplementedError, match="out_channels"):
            cls(0.0625, 7, 6, False)
        with pytest.raises(NotImplementedError, match="deform_fc_channels"):
            cls(0.0625, 7, 8, False, deform_fc_channels=30)
        cls(0.0625, 7, 6, True)     # without offsets there is no FC stack to refuse
