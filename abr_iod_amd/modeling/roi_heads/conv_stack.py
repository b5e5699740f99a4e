"""n x relu(conv3x3(pad 1) + bias) over pooled RoI features, forward and hand-scheduled backward: the loop the keypoint head's
KeypointRCNNFeatureExtractor and the FPN mask head's MaskRCNNFPNFeatureExtractor share.  Each extractor is ONE autograd node around it (its
pooler in front); the weight gradients go straight into the flat gradient buffer on the side stream."""
from ... import ops
from ..backbone.resnet import _grad_buf


def conv_stack_forward(convs, x, math, keep=False):
    """x NHWC [P,r,r,C] -> the last activation, or with `keep` (acts = [x, conv1's, ...], vs = the Winograd input transforms the weight
    gradients reuse, None where a conv is frozen)"""
    acts, vs = [x], []
    for c in convs:
        v = ops.wino_v_alloc(x, c.weight, 1, 1, math) if keep and c.weight.requires_grad else None
        x = ops.conv_forward(x, c.weight, 1, 1, bias=c.bias, relu=True, math=math, wino_v=v, w_version=c.version())
        if keep:
            acts.append(x)
            vs.append(v)
    return (acts, vs) if keep else x


def conv_stack_backward(convs, acts, vs, g, math, need_dx):
    """g: the NHWC gradient at the last activation (before its ReLU mask) -> the gradient at acts[0] (None unless need_dx); every trainable
    conv's weight and bias gradient is added to the flat buffer.  A ReLU mask rides in the epilogue of the contraction that produces the
    gradient below it."""
    gz = ops.relu_backward(g if g.is_contiguous() else g.contiguous(), acts[-1])
    gp = None
    for i in range(len(convs) - 1, -1, -1):
        c = convs[i]
        if c.weight.requires_grad:
            ops.conv_wgrad_async(acts[i], gz, _grad_buf(c.weight), 1, 1, math=math, wino_v=vs[i])
            ops.bias_grad(gz, _grad_buf(c.bias))
        if i > 0:
            gz = ops.conv_forward(gz, c.dgrad_weight(), 1, 1, mask=acts[i], math=math, w_version=c.version())
        elif need_dx:
            gp = ops.conv_forward(gz, c.dgrad_weight(), 1, 1, math=math, w_version=c.version())
    return gp
