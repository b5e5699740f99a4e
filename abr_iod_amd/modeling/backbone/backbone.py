"""build_backbone (mirror of maskrcnn_benchmark/modeling/backbone/backbone.py): R-50-C4 / R-101-C4 = nn.Sequential(body=ResNet);
R-50-FPN / R-101-FPN / R-152-FPN = body=ResNet (C2..C5) + fpn=FPN with LastLevelMaxPool;
R-50-FPN-RETINANET / R-101-FPN-RETINANET (with MODEL.RETINANET_ON) = the same body + fpn=FPN over C3..C5 with LastLevelP6P7: (P3, .., P7).

One deliberate departure from the reference: its FPN bodies are nn.Sequential(body, fpn), which hands ResNet.forward's PAIR
(outputs, backbone_features) to FPN.forward whole and crashes in the detector.  Here the FPN runs on `outputs` and `backbone_features`
passes through: forward returns ((P2, .., P6), backbone_features), the shape of result every C4 body gives the detector."""
from collections import OrderedDict

from torch import nn

from . import fpn as fpn_module
from . import resnet


class _Body(nn.Sequential):
    def forward(self, x, prefix=None):
        return self.body(x, prefix)

    def frozen_prefix(self, x):
        return self.body.frozen_prefix(x)


class _FPNBody(_Body):
    def forward(self, x, prefix=None):
        outputs, backbone_features = self.body(x, prefix)
        return self.fpn(outputs), backbone_features


def build_resnet_fpn_backbone(cfg, p3p7=False):
    """backbone.py:23-71; p3p7: build_resnet_fpn_p3p7_backbone (:74-97), the skipped first level and LastLevelP6P7 on C5 (USE_C5) or P5"""
    for key in ("USE_GN", "USE_RELU"):
        if getattr(cfg.MODEL.FPN, key):
            raise NotImplementedError("MODEL.FPN.{} = True: the FPN's conv block is a plain conv with bias here (no GroupNorm, no ReLU)".format(key))
    body = resnet.ResNet(cfg)
    in_channels_stage2 = cfg.MODEL.RESNETS.RES2_OUT_CHANNELS
    out_channels = cfg.MODEL.RESNETS.BACKBONE_OUT_CHANNELS
    if p3p7:
        in_channels_p6p7 = in_channels_stage2 * 8 if cfg.MODEL.RETINANET.USE_C5 else out_channels
        fpn = fpn_module.FPN(in_channels_list=[0, in_channels_stage2 * 2, in_channels_stage2 * 4, in_channels_stage2 * 8],
                             out_channels=out_channels, top_blocks=fpn_module.LastLevelP6P7(in_channels_p6p7, out_channels))
    else:
        fpn = fpn_module.FPN(in_channels_list=[in_channels_stage2, in_channels_stage2 * 2, in_channels_stage2 * 4, in_channels_stage2 * 8],
                             out_channels=out_channels, top_blocks=fpn_module.LastLevelMaxPool())
    fpn.math = body.layer1[0].math   # (cfg.DTYPE: the arithmetic ResNet gave its bottlenecks)
    model = _FPNBody(OrderedDict([("body", body), ("fpn", fpn)]))
    model.out_channels = out_channels
    if cfg.MODEL.BACKBONE.ALL_FREEZE:
        for _, param in model.named_parameters():
            param.requires_grad = False
    if cfg.MODEL.BACKBONE.FPN_FREEZE:
        for name, param in model.named_parameters():
            if "fpn" in name:
                param.requires_grad = False
    return model


def build_backbone(cfg):
    resnet.stage_specs(cfg.MODEL.BACKBONE.CONV_BODY, cfg.MODEL.RETINANET_ON)   # NotImplementedError for the bodies this build does not run
    resnet.check_fpn_config(cfg)                       # ... and for an FPN body in front of the single-level RPN
    if cfg.MODEL.RETINANET_ON:
        return build_resnet_fpn_backbone(cfg, p3p7=True)
    if cfg.MODEL.BACKBONE.CONV_BODY in resnet.FPN_BODIES:
        return build_resnet_fpn_backbone(cfg)
    body = resnet.ResNet(cfg)
    model = _Body(OrderedDict([("body", body)]))
    model.out_channels = cfg.MODEL.RESNETS.BACKBONE_OUT_CHANNELS
    return model
