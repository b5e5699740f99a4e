"""Host restatements of the keypoint head's kernels (abr_iod_amd/csrc/keypoint.hip), the yardsticks of tests/test_gpu_keypoint_kernels.py.

float64 numpy / torch throughout, except the targets: those are index-exact, so select_targets repeats the reference's float32 operations
(structures/keypoint.py:154-188, keypoint_head/loss.py:39-143) in numpy float32, in the same order.  heatmaps_to_keypoints restates
keypoint_head/inference.py:40-94 with cv2.resize(INTER_CUBIC) written out from its definition: Keys' kernel with a = -0.75, source
coordinate (d + 0.5) * src / dst - 0.5, four taps per axis with replicated borders, no antialiasing."""
import numpy as np
import torch

F32 = np.float32


def kp_pad(K):
    return (K + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------------- targets
def box_iou_f32(g, b):
    """structures/boxlist_ops.py:53-88 (TO_REMOVE = 1) for one pair, one float32 rounding per operation"""
    one = F32(1)
    a1 = (g[2] - g[0] + one) * (g[3] - g[1] + one)
    a2 = (b[2] - b[0] + one) * (b[3] - b[1] + one)
    w = max(min(g[2], b[2]) - max(g[0], b[0]) + one, F32(0))
    h = max(min(g[3], b[3]) - max(g[1], b[1]) + one, F32(0))
    inter = w * h
    with np.errstate(all="ignore"):
        return inter / (a1 + a2 - inter)


def match_first_max(gt, b):
    best, bi = F32(-1), 0
    for g in range(gt.shape[0]):
        v = box_iou_f32(gt[g], b)
        if v > best:
            best, bi = v, g
    return bi


def heat_index(v, lo, hi, M):
    """floor((v - lo) * scale) in float32, the v == hi rule; -1 where the index leaves [0, M) (inf and NaN included).  The reference's
    scale, `heatmap_size / (hi - lo)` with a Python number on the left, is torch's reciprocal() * heatmap_size: two roundings"""
    with np.errstate(all="ignore"):
        f = np.floor((F32(v) - F32(lo)) * ((F32(1) / (F32(hi) - F32(lo))) * F32(M)))
    i = int(f) if (f >= 0 and f < M) else -1
    if F32(v) == F32(hi):
        i = M - 1
    return i


def select_targets(rois, labels, gt_boxes, keypoints, M, p_max):
    """-> dict of numpy arrays shaped as ops.kp_select_targets' outputs"""
    rois = np.asarray(rois, F32).reshape(-1, 5)
    labels = np.asarray(labels, np.int64)
    R, K = labels.shape[0], keypoints[0].shape[1]
    pos_rows = np.full((p_max,), -1, np.int64)
    inv = np.full((R,), -1, np.int64)
    tgt = np.zeros((p_max, K), np.int64)
    valid = np.zeros((p_max, K), np.uint8)
    n = 0
    for i in range(R):
        if labels[i] <= 0:
            continue
        img = int(rois[i, 0])
        if img < 0 or img >= len(gt_boxes) or gt_boxes[img].shape[0] == 0:
            continue
        gt, kp, b = np.asarray(gt_boxes[img], F32), np.asarray(keypoints[img], F32), rois[i, 1:]
        gi = match_first_max(gt, b)
        g, pts = gt[gi], kp[gi]
        inside = (pts[:, 0] >= g[0]) & (pts[:, 0] <= g[2]) & (pts[:, 1] >= g[1]) & (pts[:, 1] <= g[3]) & (pts[:, 2] > 0)
        if not inside.any():
            continue
        if n < p_max:
            pos_rows[n], inv[i] = i, n
            for k in range(K):
                xi, yi = heat_index(pts[k, 0], b[0], b[2], M), heat_index(pts[k, 1], b[1], b[3], M)
                ok = xi >= 0 and yi >= 0 and xi < M and yi < M and pts[k, 2] > 0
                tgt[n, k], valid[n, k] = (yi * M + xi if ok else 0), int(ok)
        n += 1
    return dict(pos_rows=pos_rows, inv=inv, n_pos=min(n, p_max), targets=tgt, valid=valid, n_valid=int(valid.sum()))


# ---------------------------------------------------------------------------------------------------- deconvolution
def gemm_columns_to_weight(y_w, K):
    """the GEMM's weight [16*Kp, C] (rows (ky*4+kx)*Kp + k) -> ConvTranspose2d's [C, K, 4, 4]"""
    Kp = kp_pad(K)
    C = y_w.shape[1]
    return y_w.reshape(4, 4, Kp, C)[:, :, :K].permute(3, 2, 0, 1)


def fold(y, bias):
    """y [P,h,w,16*Kp] float64, bias [K] -> [P,Kp,2h,2w]: out[p,k,oy,ox] = bias[k] + sum over taps with oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx"""
    y = torch.as_tensor(y, dtype=torch.float64)
    P, h, w, c = y.shape
    K = bias.numel()
    Kp = kp_pad(K)
    t = y.reshape(P, h, w, 4, 4, Kp)
    out = torch.zeros((P, Kp, 2 * h + 2, 2 * w + 2), dtype=torch.float64)      # (index oy + 1, ox + 1: the taps reach -1 and 2h)
    for ky in range(4):
        for kx in range(4):
            out[:, :, ky:ky + 2 * h:2, kx:kx + 2 * w:2] += t[:, :, :, ky, kx, :].permute(0, 3, 1, 2)
    out = out[:, :, 1:2 * h + 1, 1:2 * w + 1].clone()
    out[:, :K] += torch.as_tensor(bias, dtype=torch.float64).reshape(1, K, 1, 1)
    out[:, K:] = 0
    return out


# ---------------------------------------------------------------------------------------------------- upsample + loss
def upsample2x(x):
    return torch.nn.functional.interpolate(torch.as_tensor(x, dtype=torch.float64), scale_factor=2, mode="bilinear", align_corners=False)


def loss_and_grad(x, K, targets, valid):
    """x [P,Kp,H,W]; targets / valid [P,K] on the upsampled map -> (loss, d loss / d x [P,Kp,H,W], per-row (max |z| + |lse|) [P,K]) in float64:
    upsample, then cross-entropy over the valid rows, mean (keypoint_head/loss.py:145-169; no valid row: 0)"""
    x64 = torch.as_tensor(x, dtype=torch.float64).clone().requires_grad_(True)
    P, Kp, H, W = x64.shape
    z = upsample2x(x64[:, :K]).reshape(P * K, 4 * H * W)
    sel = torch.as_tensor(valid).reshape(-1).bool()
    addends = (z.abs().amax(1) + torch.logsumexp(z, 1).abs()).detach().reshape(P, K) if P else torch.zeros((0, K), dtype=torch.float64)
    if not bool(sel.any()):
        return 0.0, torch.zeros_like(x64), addends
    loss = torch.nn.functional.cross_entropy(z[sel], torch.as_tensor(targets).reshape(-1)[sel])
    loss.backward()
    return loss.item(), x64.grad, addends


# ---------------------------------------------------------------------------------------------------- decode
def cubic_weights(f, A=-0.75):
    c0 = ((A * (f + 1) - 5 * A) * (f + 1) + 8 * A) * (f + 1) - 4 * A
    c1 = ((A + 2) * f - (A + 3)) * f * f + 1
    c2 = ((A + 2) * (1 - f) - (A + 3)) * (1 - f) * (1 - f) + 1
    return np.stack([c0, c1, c2, 1 - c0 - c1 - c2], -1)


def cubic_matrix(src, dst, dtype=np.float64):
    """[dst, src] matrix of the bicubic resize along one axis"""
    s = (np.arange(dst, dtype=dtype) + dtype(0.5)) * (dtype(src) / dtype(dst)) - dtype(0.5)
    fl = np.floor(s)
    c = cubic_weights((s - fl).astype(dtype)).astype(dtype)
    m = np.zeros((dst, src), dtype)
    for j in range(4):
        idx = np.clip(fl.astype(np.int64) - 1 + j, 0, src - 1)
        np.add.at(m, (np.arange(dst), idx), c[:, j])
    return m


def grid_sides(box):
    """(widths, heights, ceil widths, ceil heights) as inference.py:53-58 forms them in float32"""
    box = np.asarray(box, F32)
    w, h = np.maximum(box[2] - box[0], F32(1)), np.maximum(box[3] - box[1], F32(1))
    return w, h, int(np.ceil(w)), int(np.ceil(h))


def resize_map(pl, gw, gh, dtype=np.float64):
    pl = np.asarray(pl, dtype)
    return cubic_matrix(pl.shape[0], gh, dtype) @ pl @ cubic_matrix(pl.shape[1], gw, dtype).T


def xy_at(box, index, gw, gh):
    """inference.py:73-90 in numpy's types: float32 corrections, float64 products and sums, a float32 store"""
    box = np.asarray(box, F32)
    w, h, _, _ = grid_sides(box)
    wc, hc = w / F32(gw), h / F32(gh)
    yi, xi = divmod(int(index), gw)
    return F32((xi + 0.5) * np.float64(wc) + np.float64(box[0])), F32((yi + 0.5) * np.float64(hc) + np.float64(box[1]))


def xy_grid(box, gw, gh):
    """the float32 x of every grid column and y of every grid row (xy_at for a whole axis)"""
    box = np.asarray(box, F32)
    w, h, _, _ = grid_sides(box)
    xs = ((np.arange(gw) + 0.5) * np.float64(w / F32(gw)) + np.float64(box[0])).astype(F32)
    ys = ((np.arange(gh) + 0.5) * np.float64(h / F32(gh)) + np.float64(box[1])).astype(F32)
    return xs, ys


def heatmaps_to_keypoints(maps, boxes, dtype=np.float64):
    """maps [D,K,Hm,Wm], boxes [D,4] -> (index [D,K] of the first maximum of each resized map, resized maps as a list of [K,gh,gw])"""
    maps = np.asarray(maps)
    D, K = maps.shape[:2]
    index, resized = np.zeros((D, K), np.int64), []
    for d in range(D):
        _, _, gw, gh = grid_sides(boxes[d])
        r = np.stack([resize_map(maps[d, k], gw, gh, dtype) for k in range(K)]) if K else np.zeros((0, gh, gw), dtype)
        index[d] = r.reshape(K, -1).argmax(1)
        resized.append(r)
    return index, resized
