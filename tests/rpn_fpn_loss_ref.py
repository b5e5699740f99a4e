"""Restatement of the RPN loss over a feature pyramid (maskrcnn_benchmark/modeling/rpn/loss.py:42-148, rpn/utils.py:10-45, matcher.py:42-112,
box_coder.py:22-50, layers/smooth_l1_loss.py) in plain numpy float64.  Nothing here imports the library or the oracle.

Order of an image's anchors (cat_boxlist over the levels, each level as anchor_generator.py grids it): level-major, then location row-major, then
the anchor of the cell.  The predictions follow the same order (permute_and_flatten per level, cat over the levels).  The fused head output of
level l is [N, nloc_l, Cf]: columns 0 .. A-1 the logits, A + 4a .. A + 4a + 3 the deltas of anchor a, further columns padding.

A flat index g over the batch: image g // n, j = g % n, level l with off_l <= j < off_{l+1}, location (j - off_l) // A, anchor (j - off_l) % A."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)
TOL = 1e-6          # losses: relative to the sum of |addends| over the denominator (tests/test_gpu_loss_kernels.py)
BETA = 1.0 / 9


# ------------------------------------------------------------------------------------------------------------------ order
def level_offsets(nlocs, A):
    """off_l = A * sum_{m<l} nloc_m, with off_L = n appended"""
    return np.concatenate([[0], np.cumsum([int(v) * A for v in nlocs])]).astype(np.int64)


def concat_levels(per_level):
    """list of L per-level arrays [nloc_l * A, ...] -> their concatenation in the reference's order and the L + 1 offsets"""
    offs = np.concatenate([[0], np.cumsum([len(p) for p in per_level])]).astype(np.int64)
    return np.concatenate([np.asarray(p) for p in per_level], 0), offs


def decode_index(g, n, offs, A):
    """flat batch index -> (image, level, location, anchor of the cell)"""
    g = np.asarray(g, np.int64)
    i, j = g // n, g % n
    l = np.searchsorted(np.asarray(offs, np.int64), j, side="right") - 1
    r = j - np.asarray(offs, np.int64)[l]
    return i, l, r // A, r % A


def concat_predictions(ys, A):
    """ys: list of L fused outputs [N, nloc_l, Cf] -> (logits [N, n], deltas [N, n, 4]) in the concatenated order, float64"""
    N = ys[0].shape[0]
    obj = np.concatenate([np.asarray(y, np.float64)[:, :, :A].reshape(N, -1) for y in ys], 1)
    reg = np.concatenate([np.asarray(y, np.float64)[:, :, A:5 * A].reshape(N, -1, 4) for y in ys], 1)
    return obj, reg


# ------------------------------------------------------------------------------------------------------------------ the golden's case
MAPS = ((32, 48), (16, 24), (8, 12), (4, 6), (2, 3))      # tests/rpn_fpn_ref.py's pyramid
IMAGE_SIZES = ((128, 192), (112, 160))
A_GOLDEN = 3
CASES = (("m1", -1), ("0", 0))                            # (tag in rpn_fpn_loss.npz, STRADDLE_THRESH)


def golden_case(g_loss, g_fpn, tag, cf=16):
    """One case of tests/golden/rpn_fpn_loss.npz on the head outputs and anchors of tests/golden/rpn_fpn.npz -> dict: ys (list of L fp32
    [N, nloc_l, cf], pad columns zero), anchors / vis per level (vis per image), boxes [n,4], vis_cat per image, offs, gt, and the golden's
    labels / matched / pos / neg / losses / gradients."""
    assert int(g_loss["seed_rpn_fpn"]) == int(g_fpn["seed"]), "rpn_fpn_loss.npz was written for another rpn_fpn.npz: regenerate it"
    nL, N, A = len(MAPS), len(IMAGE_SIZES), A_GOLDEN
    ys = []
    for l in range(nL):
        obj = g_fpn["obj_%d" % l].astype(np.float32) / np.float32(1024)
        reg = g_fpn["reg_%d" % l].astype(np.float32) / np.float32(16)
        y = np.zeros(obj.shape[:2] + (cf,), np.float32)
        y[:, :, :A] = obj
        y[:, :, A:5 * A] = reg.reshape(obj.shape[0], obj.shape[1], 4 * A)
        ys.append(y)
    anchors = [g_fpn["anchors_%d" % l] for l in range(nL)]
    if tag == "m1":
        vis = [[np.ones(len(a), np.uint8) for a in anchors] for _ in range(N)]
    else:
        vis = [[g_fpn["vis_%d_%d" % (i, l)].astype(np.uint8) for l in range(nL)] for i in range(N)]
    boxes, offs = concat_levels(anchors)
    return dict(ys=ys, A=A, anchors=anchors, vis=vis, boxes=boxes, vis_cat=[np.concatenate(v) for v in vis], offs=offs, n=int(offs[-1]),
                gt=[g_loss["gt_%d" % i] for i in range(N)], labels=g_loss["labels_" + tag].astype(np.float64), matched=g_loss["matched"].astype(np.int64),
                pos=g_loss["pos_" + tag], neg=g_loss["neg_" + tag], samp=np.concatenate([g_loss["pos_" + tag], g_loss["neg_" + tag]]),
                loss_objectness=float(g_loss["loss_objectness_" + tag]), loss_rpn_box_reg=float(g_loss["loss_rpn_box_reg_" + tag]),
                d_obj=g_loss["d_obj_" + tag].astype(np.float64), d_reg=g_loss["d_reg_" + tag].astype(np.float64),
                pos_all=g_loss["pos_all"], tgt_pos_all=g_loss["tgt_pos_all"])


def sampled_grads(grads, A, n, offs, pos, samp):
    """the entries of per-level dense gradients [N, nloc_l, Cf] at the sampled logits (order of samp) and the positives' deltas (order of pos)"""
    i, l, loc, a = decode_index(samp, n, offs, A)
    d_obj = np.array([grads[l[k]][i[k], loc[k], a[k]] for k in range(len(samp))], np.float64)
    i, l, loc, a = decode_index(pos, n, offs, A)
    d_reg = np.array([grads[l[k]][i[k], loc[k], A + 4 * a[k]: A + 4 * a[k] + 4] for k in range(len(pos))], np.float64).reshape(-1, 4)
    return d_obj, d_reg


# ------------------------------------------------------------------------------------------------------------------ targets
def iou64(gt, anchors):
    """boxlist_iou(target, anchor) [G, n] in float64 (boxlist_ops.py:51-87, TO_REMOVE = 1)"""
    g, a = np.asarray(gt, np.float64), np.asarray(anchors, np.float64)
    area_g = (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)
    area_a = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    lt = np.maximum(g[:, None, :2], a[None, :, :2])
    rb = np.minimum(g[:, None, 2:], a[None, :, 2:])
    wh = np.clip(rb - lt + 1, 0, None)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_g[:, None] + area_a[None, :] - inter)


def match(iou, hi, lo, allow_low_quality=True):
    """Matcher.__call__ (matcher.py:42-112): per anchor the ground truth of its largest IoU (the first on ties), -1 below `lo`, -2 between the
    thresholds; with low-quality matches every anchor that attains a ground truth's largest IoU over ALL anchors gets its first choice back"""
    vals, all_matches = iou.max(0), iou.argmax(0).astype(np.int64)
    matches = all_matches.copy()
    matches[vals < lo] = -1
    matches[(vals >= lo) & (vals < hi)] = -2
    if allow_low_quality:
        best = iou.max(1)
        upd = np.nonzero((iou == best[:, None]).any(0))[0]
        matches[upd] = all_matches[upd]
    return matches, vals


def rpn_labels(matches, vis):
    """loss.py:76-90: 1 matched, 0 below the low threshold, -1 not visible or between the thresholds"""
    lab = (matches >= 0).astype(np.float64)
    lab[matches == -1] = 0
    lab[~np.asarray(vis, bool)] = -1
    lab[matches == -2] = -1
    return lab


def encode64(gt, ex, w=(1.0, 1.0, 1.0, 1.0)):
    """float64 BoxCoder.encode of the same fp32 inputs, and 4 fp32 ulps of the magnitude of each output's addends (the bound
    tests/test_gpu_rpn_targets.py gives an fp32 evaluation)"""
    g, e, w = np.asarray(gt, np.float64), np.asarray(ex, np.float64), np.asarray(w, np.float64)
    ew, eh = e[:, 2] - e[:, 0] + 1, e[:, 3] - e[:, 1] + 1
    gw, gh = g[:, 2] - g[:, 0] + 1, g[:, 3] - g[:, 1] + 1
    ecx, ecy = e[:, 0] + 0.5 * ew, e[:, 1] + 0.5 * eh
    gcx, gcy = g[:, 0] + 0.5 * gw, g[:, 1] + 0.5 * gh
    qx, qy = (gcx - ecx) / ew, (gcy - ecy) / eh
    lw, lh = np.log(gw / ew), np.log(gh / eh)
    ref = np.stack([w[0] * qx, w[1] * qy, w[2] * lw, w[3] * lh], 1)
    sx = (np.abs(e[:, 0]) + np.abs(e[:, 2]) + 1) / ew
    sy = (np.abs(e[:, 1]) + np.abs(e[:, 3]) + 1) / eh
    gx = (np.abs(g[:, 0]) + np.abs(g[:, 2]) + 1) / gw
    gy = (np.abs(g[:, 1]) + np.abs(g[:, 3]) + 1) / gh
    mag = np.stack([w[0] * ((np.abs(g[:, 0]) + np.abs(g[:, 2]) + np.abs(e[:, 0]) + np.abs(e[:, 2]) + 2) / ew + np.abs(qx) * (1 + sx)),
                    w[1] * ((np.abs(g[:, 1]) + np.abs(g[:, 3]) + np.abs(e[:, 1]) + np.abs(e[:, 3]) + 2) / eh + np.abs(qy) * (1 + sy)),
                    w[2] * (np.abs(lw) + 1 + sx + gx), w[3] * (np.abs(lh) + 1 + sy + gy)], 1)
    return ref, 4 * EPS * mag


def prepare_targets(anchors, vis, gt, hi=0.7, lo=0.3):
    """one image over the CONCATENATED anchors [n,4]: -> dict(matches, best (largest IoU per anchor), labels, targets [n,4], target_bound)"""
    iou = iou64(gt, anchors)
    matches, best = match(iou, hi, lo, True)
    tgt, bound = encode64(np.asarray(gt, np.float32)[np.clip(matches, 0, None)], anchors)
    return dict(matches=matches, best=best, labels=rpn_labels(matches, vis), targets=tgt, target_bound=bound, iou=iou)


def per_level_low_quality(iou, offs):
    """for every ground truth the level(s) holding its best anchor over all levels, and, per level, that level's own best anchors (what a matcher
    run level by level would promote): -> (set of levels of the global best per gt, list over gt of {level: anchors a per-level matcher promotes})"""
    G = iou.shape[0]
    glob, local = [], []
    for g in range(G):
        at = np.nonzero(iou[g] == iou[g].max())[0]
        glob.append(set((np.searchsorted(offs, at, side="right") - 1).tolist()))
        local.append({l: (offs[l] + np.nonzero(iou[g, offs[l]:offs[l + 1]] == iou[g, offs[l]:offs[l + 1]].max())[0])
                      for l in range(len(offs) - 1)})
    return glob, local


# ------------------------------------------------------------------------------------------------------------------ losses
def sl1(d, beta=BETA):
    a = np.abs(d)
    return np.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta), np.where(a < beta, d / beta, np.sign(d))


def bce(x, y):
    return np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    return np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))


def losses(ys, A, labels, targets, pos_idx, samp_idx, denom=None, g_obj=1.0, g_box=1.0):
    """ys: list of L fused outputs [N, nloc_l, Cf] (fp32 values); labels [N,n] / targets [N,n,4] over the concatenation; pos_idx / samp_idx: flat
    batch indices (entries < 0 are padding).  denom: the normaliser (default max(#sampled, 1)).
    -> dict(obj, box: the two losses; obj_addends, box_addends: the sums of |addends| / denom their bound scales with; grads: list of L float64
    [N, nloc_l, Cf] = d(g_obj * obj + g_box * box) / d ys; obj_scale, box_scale: |g| / denom, what the gradient bounds scale with)"""
    nlocs = [y.shape[1] for y in ys]
    offs = level_offsets(nlocs, A)
    n = int(offs[-1])
    N = ys[0].shape[0]
    x, reg = concat_predictions(ys, A)
    lab, tgt = np.asarray(labels, np.float64).reshape(N * n), np.asarray(targets, np.float64).reshape(N * n, 4)
    pos = np.asarray(pos_idx, np.int64).reshape(-1)
    samp = np.asarray(samp_idx, np.int64).reshape(-1)
    pos, samp = pos[pos >= 0], samp[samp >= 0]
    den = float(max(len(samp), 1)) if denom is None else float(max(denom, 1))
    xs, ys_ = x.reshape(-1)[samp], lab[samp]
    v = bce(xs, ys_)
    d = reg.reshape(-1, 4)[pos] - tgt[pos]
    val, gr = sl1(d)
    out = dict(obj=float(v.sum()) / den, box=float(val.sum()) / den,
               obj_addends=float((v + np.abs(xs) + 1).sum()) / den,
               box_addends=float((val + 9 * np.minimum(np.abs(d), BETA) * (np.abs(reg.reshape(-1, 4)[pos]) + np.abs(tgt[pos]))).sum()) / den,
               obj_scale=abs(g_obj) / den, box_scale=abs(g_box) / den, denom=den)
    grads = [np.zeros(y.shape, np.float64) for y in ys]
    i, l, loc, a = decode_index(samp, n, offs, A)
    go = (sigmoid(xs) - ys_) * g_obj / den
    for k in range(len(samp)):
        grads[l[k]][i[k], loc[k], a[k]] = go[k]
    i, l, loc, a = decode_index(pos, n, offs, A)
    for k in range(len(pos)):
        grads[l[k]][i[k], loc[k], A + 4 * a[k]: A + 4 * a[k] + 4] = gr[k] * g_box / den
    out["grads"] = grads
    return out


def check_losses(got_obj, got_box, ref, what=""):
    assert np.isfinite(got_obj) and np.isfinite(got_box), f"{what}: non-finite loss {got_obj} {got_box}"
    assert abs(got_obj - ref["obj"]) <= TOL * ref["obj_addends"], \
        f"{what}: objectness loss {got_obj!r} vs float64 {ref['obj']!r}: |d| = {abs(got_obj - ref['obj']):.3e} > {TOL * ref['obj_addends']:.3e}"
    assert abs(got_box - ref["box"]) <= TOL * ref["box_addends"], \
        f"{what}: box loss {got_box!r} vs float64 {ref['box']!r}: |d| = {abs(got_box - ref['box']):.3e} > {TOL * ref['box_addends']:.3e}"


def check_grads(got, ref, A, what=""):
    """got: list of L arrays [N, nloc_l, Cf]; the bounds of tests/test_gpu_loss_kernels.py: 8 EPS scale on the logit columns (BCE), 4 EPS scale 10 on
    the delta columns (smooth L1); every element the reference leaves at zero must be exactly zero (pad columns included)"""
    for l, (g, r) in enumerate(zip(got, ref["grads"])):
        g = np.asarray(g, np.float64).reshape(r.shape)
        assert np.isfinite(g).all(), f"{what}: level {l}: non-finite gradient"
        zero = r == 0
        assert np.all(g[zero] == 0), f"{what}: level {l}: {int((g[zero] != 0).sum())} elements outside the sampled entries are not exactly 0"
        err = np.abs(g - r)
        assert np.all(err[:, :, :A] <= 8 * EPS * ref["obj_scale"]), f"{what}: level {l}: BCE gradient off by {err[:, :, :A].max():.3e}"
        assert np.all(err[:, :, A:] <= 4 * EPS * ref["box_scale"] * 10), f"{what}: level {l}: smooth-L1 gradient off by {err[:, :, A:].max():.3e}"
