"""CombinedROIHeads (mirror of maskrcnn_benchmark/modeling/roi_heads/roi_heads.py:9-77): the box head and, behind it, the mask head under
MODEL.MASK_ON (mask_head/mask_head.py) and the keypoint head under MODEL.KEYPOINT_ON (keypoint_head/keypoint_head.py; its own extractor on
the backbone features, SHARE_BOX_FEATURE_EXTRACTOR False).

The mask head has two forms.  On a C4 body it shares the box head's extractor and reads the box head's layer4 rows in training.  On an FPN
body it is unshared: MaskRCNNFPNFeatureExtractor (mask_head/fpn_mask_head.py) pools the positives of the box head's sampled set on its own
14 x 14 pooler over P2..P5, as rows of the sampled set's device table, and MaskRCNNC4Predictor follows.  With the unshared head the mask
logits of calculate_soften_label / forward_joint are predictor(extractor(features, proposals)) on the proposals the box soften labels use
(this project's definition: the reference hands the MLP head's [N,1024] rows to the deconvolution and fails).

The keypoint head runs on both kinds of body, always unshared: on a C4 body KeypointRCNNFeatureExtractor pools the body's one map, on an FPN
body it pools P2..P5 on its own pooler (roi_heads/pyramid_extractor.py, the node the FPN mask head runs), again as rows of the sampled set's
device table.  Mask and keypoint heads may run together; the mask head goes first (roi_heads.py:33-62).  The keypoint head adds loss_kp in
training and a "keypoints" field to the detections in eval; it has no distillation term (the reference has none): calculate_soften_label
does not see it."""
import torch

from .box_head.box_head import build_roi_box_head
from .keypoint_head.keypoint_head import build_roi_keypoint_head, check_keypoint_head_cfg
from .mask_head.mask_head import build_roi_mask_head, check_mask_head_cfg


class CombinedROIHeads(torch.nn.ModuleDict):
    def __init__(self, cfg, heads):
        super().__init__(heads)
        self.cfg = cfg.clone()
        if "mask" in self and not self.mask.unshared:
            self.box.keep_joint_head_features = True

    @property
    def joint_supported(self):
        """whether forward_joint can run (an even pooler, e.g. the Mask R-CNN C4 setting 14 -> 7x7, takes the two passes: engine/trainer.py)"""
        return self.box.feature_extractor.joint_supported

    def _mask_train(self, features, x, detections, targets):
        """the shared head reads the box head's output rows `x`, the unshared one pools the backbone's `features` itself"""
        t = getattr(self.box.loss_evaluator, "_fused_targets", None)     # the fused sampler's RoI table and labels, already single device tensors
        return self.mask(features if self.mask.unshared else x, detections, targets, fused=t)

    def _keypoint_train(self, features, detections, targets):
        t = getattr(self.box.loss_evaluator, "_fused_targets", None)
        return self.keypoint(features, detections, targets, fused=t)

    def forward(self, features, proposals, targets=None):
        """training -> (x, detections, soften_results, losses, roi_align_features); eval -> (x, detections, results_background, [])
        (roi_heads.py:23-63)"""
        losses = {}
        mask_on = "mask" in self
        if not self.training:
            x, detections, results_background = self.box(features, proposals, targets)
            if mask_on:     # roi_heads.py:33-45: the mask head runs the shared extractor on the DETECTIONS
                x, detections, _ = self.mask(features, detections, targets)
            if "keypoint" in self:
                x, detections, _ = self.keypoint(features, detections, targets)
            return x, detections, results_background, []
        x, detections, soft_res, loss_box, roi_align_features = self.box(features, proposals, targets)
        losses.update(loss_box)
        if mask_on:         # training, shared head: the box head's layer4 rows of the positives, no second ROIAlign / layer4 pass
            _, detections, loss_mask = self._mask_train(features, x, detections, targets)
            losses.update(loss_mask)
        if "keypoint" in self:     # its own ROIAlign + conv stack on the backbone features, for the sampled positives
            _, detections, loss_kp = self._keypoint_train(features, detections, targets)
            losses.update(loss_kp)
        return x, detections, soft_res, losses, roi_align_features

    def forward_joint(self, features, proposals, targets, soften_proposals):
        """training forward + calculate_soften_label(features, soften_proposals) sharing one head pass"""
        (x, detections, soft_res, loss_box, raf), (s_score, s_bbox, s_raf) = self.box.forward_joint(features, proposals, targets, soften_proposals)
        losses, mask_logits = dict(loss_box), None
        if "mask" in self:
            _, detections, loss_mask = self._mask_train(features, x, detections, targets)       # x: the detection rows of the joint head pass
            losses.update(loss_mask)
            if self.mask.unshared:
                mask_logits = self.mask.calculate_soften_label(features, soften_proposals)
            else:
                mask_logits = self.mask.calculate_soften_label(self.box.last_joint_soft_x)
                self.box.last_joint_soft_x = None
        if "keypoint" in self:
            _, detections, loss_kp = self._keypoint_train(features, detections, targets)
            losses.update(loss_kp)
        return (x, detections, soft_res, losses, raf), (s_score, s_bbox, mask_logits, s_raf)

    def calculate_soften_label(self, features, proposals, targets=None):
        """-> (soften_score, soften_bbox, mask_logits (None without a mask head), roi_align_features)  (roi_heads.py:65-72)"""
        soften_score, soften_bbox, x, roi_align_features = self.box.calculate_soften_label(features, proposals, targets)
        mask_logits = None
        if "mask" in self:
            mask_logits = self.mask.calculate_soften_label(features, proposals) if self.mask.unshared else self.mask.calculate_soften_label(x)
        return soften_score, soften_bbox, mask_logits, roi_align_features


def build_roi_heads(cfg, in_channels):
    if cfg.MODEL.RETINANET_ON:   # roi_heads.py:75-79: RetinaNet has no RoI heads
        from ..backbone.resnet import RETINANET_BODIES
        if cfg.MODEL.BACKBONE.CONV_BODY not in RETINANET_BODIES:
            raise NotImplementedError("MODEL.RETINANET_ON True with MODEL.BACKBONE.CONV_BODY {!r}: RetinaNet runs on its own bodies {} only"
                                      .format(cfg.MODEL.BACKBONE.CONV_BODY, ", ".join(sorted(RETINANET_BODIES))))
        return []
    if cfg.MODEL.MASK_ON:
        check_mask_head_cfg(cfg)
    if cfg.MODEL.KEYPOINT_ON:
        check_keypoint_head_cfg(cfg)
    if cfg.MODEL.RPN_ONLY:
        return []
    heads = [("box", build_roi_box_head(cfg, in_channels))]
    if cfg.MODEL.MASK_ON:
        heads.append(("mask", build_roi_mask_head(cfg, in_channels, heads[0][1].feature_extractor)))
    if cfg.MODEL.KEYPOINT_ON:
        heads.append(("keypoint", build_roi_keypoint_head(cfg, in_channels)))
    return CombinedROIHeads(cfg, heads)
