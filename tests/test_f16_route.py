"""CPU: the ABR_MATH_F16 arithmetic (cfg.DTYPE "float16") as the host route sees it -- no compute calls.

ABR_MATH_F16 rounds each operand once to fp16 (with f16x3's scales) and contracts with one product.  It never takes Winograd F(4x4,3x3): a
Winograd transform of rounded operands is a different, less accurate function than the mode's definition.  So no Winograd-domain input V is
kept for the weight gradient, on exactly the shapes where every fp32-accurate arithmetic keeps one."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the R50-C4 wide 3x3 convs at B = 4, 600x1000: layer2-4 conv2 (layer4 = the RoI head on 7x7 crops, 96 = 4 x 24 here) and the RPN 3x3
WIDE_3X3 = [((4, 75, 125, 128), (128, 3, 3, 128)), ((4, 38, 63, 256), (256, 3, 3, 256)), ((96, 7, 7, 512), (512, 3, 3, 512)),
            ((4, 38, 63, 1024), (1024, 3, 3, 1024))]


def test_math_f16_constant_matches_the_header():
    from abr_iod_amd import ops
    src = open(os.path.join(ROOT, "include", "abr_iod_hip.h")).read()
    m = re.search(r"#define\s+ABR_MATH_F16\s+(\d+)", src)
    assert m is not None, "ABR_MATH_F16 not defined in include/abr_iod_hip.h"
    assert int(m.group(1)) == ops.MATH_F16 == 4
    assert ops.uses_amax(ops.MATH_F16) and ops.uses_amax(ops.MATH_F16X3)
    assert not any(ops.uses_amax(m) for m in (ops.MATH_F32, ops.MATH_BF16, ops.MATH_BF16X6))


def test_f16_keeps_no_winograd_v():
    from abr_iod_amd import _lib, ops
    L = _lib.lib()

    def v_floats(x_shape, w_shape, math):
        return L.abr_conv_wino_v_floats(C.byref(ops.conv_desc(x_shape, w_shape, 1, 1, math=math)))

    for x_shape, w_shape in WIDE_3X3:
        assert v_floats(x_shape, w_shape, 3) > 0, x_shape           # f16x3 (ABR_MATH_F16X3 = 3) takes Winograd here
        assert v_floats(x_shape, w_shape, 4) == 0, x_shape          # ABR_MATH_F16 = 4 goes direct


def test_float16_dtype_is_accepted_by_the_config():
    """cfg.DTYPE "float16" builds (on CPU the model only records its arithmetic; nothing is launched)"""
    from abr_iod_amd import ops
    from abr_iod_amd.config import cfg as base
    from abr_iod_amd.modeling.backbone.resnet import ResNet
    cfg = base.clone()
    cfg.DTYPE = "float16"
    net = ResNet(cfg)
    maths = {m.math for name, m in net.named_modules() if hasattr(m, "math") and name.startswith("layer")}
    assert maths == {ops.MATH_F16}
