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
