"""The FPN mask head's feature extractor on the HIP library (MODEL.MASK_ON on an FPN body, SHARE_BOX_FEATURE_EXTRACTOR False).

Mirrors:
    MaskRCNNFPNFeatureExtractor   maskrcnn_benchmark/modeling/roi_heads/mask_head/roi_mask_feature_extractors.py:16-65
    make_conv3x3                  modeling/make_layers.py:47-77 (kaiming_normal_(mode="fan_out", nonlinearity="relu"), bias 0)

Its own 14 x 14, sampling-ratio-2 pooler over P2..P5 and n x relu(conv3x3 + bias); MaskRCNNC4Predictor follows (upstream's FPN configurations
name exactly that predictor).

MI355X-first differences (results identical):
  * training pools only the positives of the box head's sampled set, and it pools them as ROWS of the table that set already is on the device
    (ops.roi_align_pyramid_forward(rows=): the -1-padded list of ops.mask_compact_pos indexes the fused sampler's RoI table): no gathered
    copy of the table, no degenerate box for the padding -- a padding row is zero, never reads the table and takes no gradient.
  * pooler and conv stack are ONE autograd node, the one the FPN keypoint head runs too (roi_heads/pyramid_extractor.py); its backward ends
    in the indexed pyramid backward, which hands every level's map its gradient.
"""
from ..pyramid_extractor import PyramidConvExtractor


class MaskRCNNFPNFeatureExtractor(PyramidConvExtractor):
    """roi_mask_feature_extractors.py:16-65.  forward -> logical [P,CONV_LAYERS[-1],r,r]"""

    def __init__(self, cfg, in_channels):
        m = cfg.MODEL.ROI_MASK_HEAD
        if m.USE_GN or m.DILATION != 1:
            raise NotImplementedError("MODEL.ROI_MASK_HEAD.USE_GN {!r} / DILATION {!r}: the GroupNorm and dilated mask convs are not built".format(
                m.USE_GN, m.DILATION))
        super().__init__(cfg, in_channels, "ROI_MASK_HEAD", "mask_fcn")
