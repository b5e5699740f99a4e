"""CPU: the C-ABI library loads and exports every symbol include/abr_iod_hip.h declares (no compute calls)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "abr_iod_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(abr_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from abr_iod_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/abr_iod_hip.h but not exported"
    # and the Python binding table covers the same set
    assert set(_lib.EXPORTS) == set(names), set(_lib.EXPORTS) ^ set(names)


def test_version_and_error_channel():
    from abr_iod_amd import _lib
    L = _lib.lib()
    assert L.abr_version() >= 100
    # invalid argument -> negative status + message, no launch (works without a GPU)
    rc = L.abr_roi_align_forward(None, None, 4, 1, 8, 4, 4, 1.0, 0, 7, 0, 1, 1, None, None)
    assert rc == -1 and b"roi_align_forward" in L.abr_last_error()
    assert L.abr_nms_workspace_bytes(2, 12000) == 2 * 12000 * 188 * 8


def test_product_path_has_no_cpu_fallback():
    import pytest
    import torch
    from abr_iod_amd import _C
    with pytest.raises(RuntimeError):
        _C.roi_align_forward(torch.zeros(1, 4, 8, 8), torch.zeros(1, 5), 1.0, 7, 7, 0)
    # nothing under abr_iod_amd/ may import the oracle
    for dp, _, fs in os.walk(os.path.join(ROOT, "abr_iod_amd")):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+\.*oracle\b", src, flags=re.M), f
                assert "liboracle" not in src and "oracle/" not in re.sub(r"#.*|\"\"\".*?\"\"\"", "", src, flags=re.S), f


def test_winograd_v_size_follows_the_forward_route():
    """abr_conv_wino_v_floats (host only): V is kept exactly when both the forward pass and the weight gradient take the Winograd path.  The
    R50-C4 Winograd convs (layer2-4 conv2 and their dgrads, the RPN 3x3) keep it in every fp32-accurate arithmetic; the bf16 mode never does;
    a bf16x6 / f16x3 conv with Cout % 32 != 0 runs its forward direct, so there is no V to keep."""
    import ctypes as C
    from abr_iod_amd import _lib, ops
    L = _lib.lib()

    def v_floats(x_shape, w_shape, math):
        return L.abr_conv_wino_v_floats(C.byref(ops.conv_desc(x_shape, w_shape, 1, 1, math=math)))

    convs = [((4, 75, 125, 128), (128, 3, 3, 128)), ((4, 38, 63, 256), (256, 3, 3, 256)), ((96, 7, 7, 512), (512, 3, 3, 512)),
             ((4, 38, 63, 1024), (1024, 3, 3, 1024))]
    for x_shape, w_shape in convs:   # (a 3x3 stride-1 conv with Cin == Cout: its dgrad has the same descriptor)
        B, H, W, Cin = x_shape
        for math in (ops.MATH_F32, ops.MATH_BF16X6, ops.MATH_F16X3):
            assert v_floats(x_shape, w_shape, math) == 36 * B * ((H + 3) // 4) * ((W + 3) // 4) * Cin, (x_shape, math)
        assert v_floats(x_shape, w_shape, ops.MATH_BF16) == 0, x_shape
    for math in (ops.MATH_BF16X6, ops.MATH_F16X3):
        assert v_floats((2, 21, 10, 128), (136, 3, 3, 128), math) == 0, math


def test_conv_route_table():
    """abr_conv_route_info (host only) returns what abr::conv_route decided; this pins the table in conv_route's own comments."""
    from abr_iod_amd import ops
    F32, BF16, X6, H3, F16 = ops.MATH_F32, ops.MATH_BF16, ops.MATH_BF16X6, ops.MATH_F16X3, ops.MATH_F16
    import torch
    res = torch.zeros(4)      # (the route looks at the pointer only)

    def route(x_shape, w_shape, stride=1, pad=1, **kw):
        return ops.conv_route_info(x_shape, w_shape, stride, pad, **kw)

    wide = ((2, 21, 10, 256), (256, 3, 3, 256))
    # wide stride-1 pad-1 3x3: Winograd forward and weight gradient in every full-precision arithmetic ...
    for m in (F32, X6, H3):
        assert route(*wide, math=m) == (m, True, True, m), m
    # ... bf16 and f16 never (a transform of rounded operands is another function than the mode's definition)
    for m in (BF16, F16):
        assert route(*wide, math=m) == (m, False, False, m), m
    # not wide, not stride 1, not pad 1, not 3x3: direct
    for x_shape, w_shape, st, pad in [((2, 21, 10, 64), (256, 3, 3, 64), 1, 1), ((2, 21, 10, 256), (64, 3, 3, 256), 1, 1),
                                      ((2, 21, 10, 256), (256, 3, 3, 256), 2, 1), ((2, 21, 10, 256), (256, 3, 3, 256), 1, 0),
                                      ((2, 21, 10, 256), (256, 1, 1, 256), 1, 0)]:
        for m in (F32, X6, H3):
            assert route(x_shape, w_shape, st, pad, math=m)[1:3] == (False, False), (x_shape, w_shape, st, pad, m)
    # a residual epilogue: forward direct, weight gradient still Winograd
    for m in (F32, X6, H3):
        assert route(*wide, residual=res, math=m) == (m, False, True, m), m
    # Cout % 32 != 0 under the split arithmetics (U's 36 matrices are packed as one whose 32-row blocks must not straddle two): forward direct;
    # fp32 Winograd takes any Cout % 4 == 0
    for cout in (132, 136, 200):
        for m in (X6, H3):
            assert route((2, 21, 10, 128), (cout, 3, 3, 128), math=m) == (m, False, True, m), (cout, m)
        assert route((2, 21, 10, 128), (cout, 3, 3, 128), math=F32) == (F32, True, True, F32), cout
    # Cout % 4 != 0: forward direct in every arithmetic
    for m in (F32, X6, H3):
        assert route((2, 21, 10, 128), (129, 3, 3, 128), math=m)[1] is False, m
    # Cin % 32 != 0: forward direct (and in fp32 under a split arithmetic); the weight gradient asks for Cin % 4 == 0 only and keeps its arithmetic
    assert route((2, 21, 10, 132), (128, 3, 3, 132), math=F32) == (F32, False, True, F32)
    for m in (X6, H3):
        assert route((2, 21, 10, 132), (128, 3, 3, 132), math=m) == (F32, False, True, m), m
    # Cin = 4 (the stem) under a split arithmetic or f16: fp32
    for m in (X6, H3, F16):
        assert route((2, 64, 64, 4), (64, 7, 7, 4), 2, 3, math=m)[0] == F32, m
    # bf16 covers the Cin % 64 == 0 layers: elsewhere forward and weight gradient run in fp32 (and may then take Winograd)
    assert route((2, 21, 10, 128), (128, 3, 3, 128), math=BF16) == (BF16, False, False, BF16)
    assert route((2, 21, 10, 160), (160, 3, 3, 160), math=BF16) == (F32, True, True, F32)
    assert route((2, 21, 10, 96), (64, 1, 1, 96), 1, 0, math=BF16) == (F32, False, False, F32)
    # a scattered output (the input gradient of a strided conv): direct
    for m in (F32, X6, H3):
        assert route(*wide, out_hw=(42, 20), out_stride=(2, 2), math=m)[1] is False, m
