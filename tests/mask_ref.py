"""Reference-side restatements for the mask head tests (torch on the CPU; no product code): the mask branch for autograd, the float64 paste
the paste test excuses near-threshold pixels with, and the oracle model with a mask branch."""
import torch
import torch.nn.functional as F


def mask_branch(x, w5, b5, wl, bl):
    """MaskRCNNC4Predictor (roi_mask_predictors.py:10-32): x [P,C,h,w], w5 [C,Cm,2,2], wl [K,Cm,1,1] -> logits [P,K,2h,2w]"""
    return F.conv2d(F.relu(F.conv_transpose2d(x, w5, b5, stride=2)), wl, bl)


def mask_loss(logits, labels_pos, targets):
    """mask_head/loss.py:117-128 on the positives' logits [P,K,M,M]"""
    if targets.numel() == 0:
        return logits.sum() * 0
    return F.binary_cross_entropy_with_logits(logits[torch.arange(logits.shape[0]), labels_pos], targets)


def paste_f64(prob, box, im_h, im_w, padding=1):
    """paste_mask_in_image (inference.py:119-159) with the integer box arithmetic in float32 / int32 as there and the INTERPOLATION in float64:
    -> (values float64 [im_h, im_w], written bool [im_h, im_w]); the pasted mask is values > threshold where written, 0 elsewhere"""
    M = prob.shape[-1]
    scale = float(M + 2 * padding) / M
    padded = torch.zeros((M + 2 * padding, M + 2 * padding), dtype=torch.float32)
    padded[padding:-padding, padding:-padding] = prob.float()
    b = box.float()
    w_half, h_half = (b[2] - b[0]) * .5, (b[3] - b[1]) * .5
    x_c, y_c = (b[2] + b[0]) * .5, (b[3] + b[1]) * .5
    w_half = w_half * scale
    h_half = h_half * scale
    bi = torch.stack([x_c - w_half, y_c - h_half, x_c + w_half, y_c + h_half]).to(torch.int32)
    w = max(int(bi[2] - bi[0] + 1), 1)
    h = max(int(bi[3] - bi[1] + 1), 1)
    # float32 source coordinates as torch computes them, float64 taps
    def taps(out, inp):
        sc = torch.tensor(inp, dtype=torch.float32) / torch.tensor(out, dtype=torch.float32)
        s = sc * (torch.arange(out, dtype=torch.float32) + 0.5) - 0.5
        s = s.clamp(min=0)
        i0 = s.floor().long().clamp(max=inp - 1)
        l1 = (s - i0.float()).clamp(0, 1)
        i1 = i0 + (i0 < inp - 1).long()
        return i0, i1, l1.double()
    y0, y1, ly = taps(h, M + 2 * padding)
    x0, x1, lx = taps(w, M + 2 * padding)
    p = padded.double()
    r0 = p[y0][:, x0] * (1 - lx) + p[y0][:, x1] * lx
    r1 = p[y1][:, x0] * (1 - lx) + p[y1][:, x1] * lx
    res = r0 * (1 - ly)[:, None] + r1 * ly[:, None]
    vals = torch.zeros((im_h, im_w), dtype=torch.float64)
    written = torch.zeros((im_h, im_w), dtype=torch.bool)
    bx0, by0, bx2, by3 = (int(v) for v in bi)
    x_0, x_1, y_0, y_1 = max(bx0, 0), min(bx2 + 1, im_w), max(by0, 0), min(by3 + 1, im_h)
    if x_1 > x_0 and y_1 > y_0:
        vals[y_0:y_1, x_0:x_1] = res[y_0 - by0:y_1 - by0, x_0 - bx0:x_1 - bx0]
        written[y_0:y_1, x_0:x_1] = True
    return vals, written


def ref_model_with_mask():
    """oracle.model_ref.RefModel + the mask branch on the box head's layer4 output"""
    from oracle.model_ref import RefModel, _RoiAlignRef

    class MaskRefModel(RefModel):
        def head_features(self, feat, rois, sr=0, res=7, scale=0.0625):
            x = _RoiAlignRef.apply(feat, rois, scale, res, res, sr)
            pooled = x
            for i in range(3):
                x = self._block(x, f"roi_heads.box.feature_extractor.head.layer4.{i}", 2 if i == 0 else 1)
            return pooled, x

        def box_predictor(self, x):
            v = F.adaptive_avg_pool2d(x, 1).flatten(1)
            pr = "roi_heads.box.predictor"
            return (F.linear(v, self.p[f"{pr}.cls_score.weight"], self.p[f"{pr}.cls_score.bias"]),
                    F.linear(v, self.p[f"{pr}.bbox_pred.weight"], self.p[f"{pr}.bbox_pred.bias"]))

        def mask_predictor(self, x):
            pr = "roi_heads.mask.predictor"
            return mask_branch(x, self.p[f"{pr}.conv5_mask.weight"], self.p[f"{pr}.conv5_mask.bias"], self.p[f"{pr}.mask_fcn_logits.weight"],
                               self.p[f"{pr}.mask_fcn_logits.bias"])

    return MaskRefModel
