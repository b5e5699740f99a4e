"""GPU: the host side of the conv amax-word protocol is the same on every call path.

Which amax word a conv is handed for each operand, whether its epilogue may write one for the result, and how the result is tagged
afterwards is decided in ops.py (amax_operand, amax_wgrad_operands, conv_out_emits, conv_out_done).  A conv's backward pass reaches those
rules two ways: the per-conv pair (conv_wgrad_async, then conv_forward on the dgrad copy of the weight) and conv_backward's abr_conv_run
table.  Both hand the same descriptors to the same library, so for every state the operands' tags can be in: the gradients are
bit-identical, the result is tagged on one path exactly when it is on the other, the word holds max |dx| bit for bit (tests/amax_words.py),
the scatter marks agree, and the host queued the same number of reductions.  The second pass of a strided scatter (out = residual = the
first pass's tensor) emits only while the tensor still carries the first pass's mark.  (test_gpu_f16x3_admission.py asserts that a consumer
of such a tagged tensor returns the same bits as one that reduces it; here the word's VALUE is read back.)"""
import pytest
import torch

from amax_words import abs_bits, expect

pytestmark = pytest.mark.gpu

# x [B,H,W,Cin], Cout, k, stride, pad, the input gradient's scatter (a stride-2 1x1 conv: rows land on the even pixels of a zeroed [B,H,W,Cin];
# 7 x 5 leaves a ragged last row and column)
GEOMS = {
    "3x3": ((1, 6, 5, 32), 32, 3, 1, 1, {}),
    "1x1s2": ((1, 7, 5, 32), 64, 1, 2, 0, dict(out_hw=(7, 5), out_stride=(2, 2))),
}
STATES = ("both_tagged", "x_untagged", "gy_untagged", "gy_noncontiguous")


class _InBackward(torch.autograd.Function):
    """runs fn() inside an autograd backward pass (the side-stream join is an engine callback)"""

    @staticmethod
    def forward(ctx, a, fn, box):
        ctx.fn, ctx.box = fn, box
        return a.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.box.append(ctx.fn())
        return None, None, None


def _in_backward(fn):
    box = []
    a = torch.zeros(1, device="cuda", requires_grad=True)
    _InBackward.apply(a, fn, box).sum().backward()
    torch.cuda.synchronize()
    return box[0]


def _math(ops, name):
    return {"f16x3": ops.MATH_F16X3, "f16": ops.MATH_F16}[name]


def _setup(monkeypatch):
    from abr_iod_amd import ops
    monkeypatch.setattr(ops, "WGRAD_SIDE_STREAM", True)
    monkeypatch.setattr(ops, "H3_TAGS", True)
    return ops


def _mark(t):
    """the scatter mark without its address, and whether the address is the tensor's"""
    m = getattr(t, "_abr_scatter", None)
    return None if m is None else (m[0] == t.data_ptr(), m[1], m[2])


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("mname", ["f16x3", "f16"])
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_backward_pair_and_table_agree(geom, mname, state, monkeypatch):
    ops = _setup(monkeypatch)
    m = _math(ops, mname)
    x_shape, cout, k, s, p, scatter = GEOMS[geom]
    B, H, W, cin = x_shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = torch.Generator(device="cuda").manual_seed(17)
    x0 = torch.randn(x_shape, device="cuda", generator=g)
    gy0 = torch.randn(B, Ho, Wo, cout, device="cuda", generator=g)
    w = torch.randn(cout, k, k, cin, device="cuda", generator=g) / (k * k * cin) ** 0.5
    wt = ops.conv_dgrad_weights(w)

    def operands():
        """this path's own x, gy objects (a tag rides on the object) in the state asked for"""
        x = x0.clone()
        if state == "gy_noncontiguous":
            gy = gy0.transpose(1, 2).contiguous().transpose(1, 2)
            assert not gy.is_contiguous() and torch.equal(gy, gy0)
        else:
            gy = gy0.clone()
        if state != "x_untagged":
            ops.amax_compute(x)
        if state in ("both_tagged", "x_untagged"):
            ops.amax_compute(gy)
        return x, gy

    def pair(x, gy, dw):
        n0 = ops.amax_reductions[0]
        ops.conv_wgrad_async(x, gy, dw, s, p, math=m)
        dx = ops.conv_forward(gy, wt, 1, k - 1 - p, math=m, **scatter)
        return dx, ops.amax_reductions[0] - n0

    def table(x, gy, dw):
        n0 = ops.amax_reductions[0]
        dx = ops.conv_backward(x, gy, dw, wt, s, p, math=m, **scatter)
        return dx, ops.amax_reductions[0] - n0

    runs = []
    inner = ops._conv_backward_run
    monkeypatch.setattr(ops, "_conv_backward_run", lambda *a: (runs.append(1), inner(*a))[1])
    res = {}
    for name, fn in (("pair", pair), ("table", table)):
        x, gy = operands()
        dw = torch.zeros_like(w)
        dx, n_red = _in_backward(lambda: fn(x, gy, dw))
        res[name] = (dw, dx, n_red)
    (dw_p, dx_p, n_p), (dw_t, dx_t, n_t) = res["pair"], res["table"]
    assert len(runs) == (state != "gy_noncontiguous"), "conv_backward ran its table %d times" % len(runs)
    assert tuple(dx_p.shape) == x_shape and abs_bits(dx_p) != 0 and abs_bits(dw_p) != 0
    assert torch.equal(dw_p, dw_t), float((dw_p - dw_t).abs().max())
    assert torch.equal(dx_p, dx_t), float((dx_p - dx_t).abs().max())
    tag_p, tag_t = ops.amax_of(dx_p), ops.amax_of(dx_t)
    assert (tag_p[0] is None) == (tag_t[0] is None), (tag_p, tag_t)
    assert tag_p[0] is not None, "a fresh result under %s carries its word" % mname
    expect(tag_p[0], tag_p[1], dx_p, "%s %s %s pair" % (geom, mname, state))
    expect(tag_t[0], tag_t[1], dx_t, "%s %s %s table" % (geom, mname, state))
    assert _mark(dx_p) == _mark(dx_t) == ((True, 2, 2) if scatter else None)
    assert n_p == n_t, (n_p, n_t)
    # each contiguous operand without a tag is reduced once (the dgrad finds gy's new tag); a non-contiguous gy is copied, and its copy
    # reduced, by the weight gradient and by the dgrad each
    assert n_p == {"both_tagged": 0, "x_untagged": 1, "gy_untagged": 1, "gy_noncontiguous": 2}[state], n_p
    assert ops.x6_range_flags(reset=True) == 0


@pytest.mark.parametrize("path", ["conv_forward", "conv_backward"])
@pytest.mark.parametrize("mname", ["f16x3", "f16"])
def test_second_pass_into_the_scattered_tensor(mname, path, monkeypatch):
    """the downsample branch's input gradient adds into conv1's scattered one (out = residual = t): it emits while t carries the mark of that
    geometry, and its word is max |t| over the whole tensor; once ops.add_ has filled the holes, or under another out_stride, t ends untagged"""
    ops = _setup(monkeypatch)
    m = _math(ops, mname)
    g = torch.Generator(device="cuda").manual_seed(23)
    g1, g2 = torch.randn(1, 4, 3, 64, device="cuda", generator=g), torch.randn(1, 4, 3, 128, device="cuda", generator=g)
    wt1, wt2 = torch.randn(32, 1, 1, 64, device="cuda", generator=g) / 8, torch.randn(32, 1, 1, 128, device="cuda", generator=g) / 11
    x2 = torch.randn(1, 7, 5, 32, device="cuda", generator=g)      # the branch's input, for its weight gradient on the table path
    ops.amax_compute(g1)

    def first():
        t = ops.conv_forward(g1, wt1, 1, 0, out_hw=(7, 5), out_stride=(2, 2), math=m)
        assert ops.amax_of(t)[0] is not None and _mark(t) == (True, 2, 2)
        return t

    def second(t, out_stride):
        gy = g2.clone()
        ops.amax_compute(gy)
        if path == "conv_forward":
            return ops.conv_forward(gy, wt2, 1, 0, residual=t, out=t, out_hw=(7, 5), out_stride=out_stride, math=m)
        dw = torch.zeros(128, 1, 1, 32, device="cuda")
        return _in_backward(lambda: ops.conv_backward(x2, gy, dw, wt2, 2, 0, math=m, residual=t, out=t, out_hw=(7, 5), out_stride=out_stride))

    t = first()
    first_word = ops.amax_of(t)[0]
    ref = t.clone()
    assert second(t, (2, 2)) is t
    word, epoch = ops.amax_of(t)
    assert word not in (None, first_word)
    assert not torch.equal(t, ref) and bool((t[:, 1::2] == 0).all()) and bool((t[:, :, 1::2] == 0).all())
    expect(word, epoch, t, "second pass, %s, %s" % (mname, path))
    assert _mark(t) == (True, 2, 2)

    t = first()
    ops.add_(t, torch.full_like(t, 0.5))
    assert _mark(t) is None and ops.amax_of(t)[0] is None
    second(t, (2, 2))
    assert ops.amax_of(t)[0] is None and _mark(t) is None

    t = first()
    second(t, (1, 2))          # rows 0..3, columns 0, 2, 4: inside the tensor, but not the pixels the first pass wrote
    assert ops.amax_of(t)[0] is None and _mark(t) is None
    assert ops.x6_range_flags(reset=True) == 0
