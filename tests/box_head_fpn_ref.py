"""float64 numpy restatement of the FPN box head behind the pooler (roi_box_feature_extractors.py:93-101, roi_box_predictors.py:92-132 without
the offset layers): pooled [K,C,res,res] -> x.view(K, -1) in (c,h,w) order -> fc6 -> ReLU -> fc7 -> ReLU -> cls_score / bbox_pred, and its
backward for given cotangents on the two outputs.  Weights in the reference's layout ([out, in], fc6's columns in (c,h,w) order).

The golden's settings (tests/golden/make_golden_box_head_fpn.py): the maps and RoI set of tests/golden/pooler_fpn.npz, resolution 7,
MLP_HEAD_DIM 32, NUM_CLASSES 5."""
import numpy as np

RES, DIM, NUM_CLASSES, SAMPLING = 7, 32, 5, 2
PARAMS = ("fc6", "fc7", "cls_score", "bbox_pred")
GOLDEN_SEED = 20261


def _f64(a):
    return np.asarray(a, np.float64)


def params64(g):
    """{"fc6": (w, b), ...} in float64 from a loaded golden (keys w_<name>, b_<name>)"""
    return {n: (_f64(g["w_" + n]), _f64(g["b_" + n])) for n in PARAMS}


def forward(pooled, p):
    """pooled [K,C,res,res] (logical NCHW), p = {"fc6": (w [D, C*res*res], b), "fc7": .., "cls_score": .., "bbox_pred": ..}
    -> dict(flat, h6, h7 = x, cls, bbox), float64"""
    pooled = _f64(pooled)
    flat = pooled.reshape(pooled.shape[0], -1)
    h6 = np.maximum(flat @ _f64(p["fc6"][0]).T + _f64(p["fc6"][1]), 0.0)
    h7 = np.maximum(h6 @ _f64(p["fc7"][0]).T + _f64(p["fc7"][1]), 0.0)
    cls = h7 @ _f64(p["cls_score"][0]).T + _f64(p["cls_score"][1])
    bbox = h7 @ _f64(p["bbox_pred"][0]).T + _f64(p["bbox_pred"][1])
    return dict(flat=flat, h6=h6, h7=h7, cls=cls, bbox=bbox)


def backward(fw, p, g_cls, g_bbox, pooled_shape):
    """cotangents g_cls [K,NC], g_bbox [K,4NC] -> dict: gw_<name> / gb_<name> for the four layers, g_h7 (after fc7's ReLU mask), g_h6 (after
    fc6's), g_pooled [K,C,res,res]; float64"""
    g_cls, g_bbox = _f64(g_cls), _f64(g_bbox)
    out = {"gw_cls_score": g_cls.T @ fw["h7"], "gb_cls_score": g_cls.sum(0), "gw_bbox_pred": g_bbox.T @ fw["h7"], "gb_bbox_pred": g_bbox.sum(0)}
    g_x = g_cls @ _f64(p["cls_score"][0]) + g_bbox @ _f64(p["bbox_pred"][0])
    g7 = g_x * (fw["h7"] > 0)
    out.update(g_x=g_x, g_h7=g7, gw_fc7=g7.T @ fw["h6"], gb_fc7=g7.sum(0))
    g6 = (g7 @ _f64(p["fc7"][0])) * (fw["h6"] > 0)
    out.update(g_h6=g6, gw_fc6=g6.T @ fw["flat"], gb_fc6=g6.sum(0))
    out["g_pooled"] = (g6 @ _f64(p["fc6"][0])).reshape(pooled_shape)
    return out


def fc6_to_ohwi(w, C, res=RES):
    """the reference's fc6 weight [D, C*res*res] -> the stored [D,1,1,res*res*C] (the bytes of an OHWI [D,res,res,C] conv weight)"""
    D = w.shape[0]
    return np.ascontiguousarray(w.reshape(D, C, res, res).transpose(0, 2, 3, 1)).reshape(D, 1, 1, res * res * C)


def fc6_from_ohwi(w, C, res=RES):
    D = w.shape[0]
    return np.ascontiguousarray(w.reshape(D, res, res, C).transpose(0, 3, 1, 2)).reshape(D, C * res * res)


def cotangents(K, seed=GOLDEN_SEED):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, NUM_CLASSES)).astype(np.float32), rng.standard_normal((K, 4 * NUM_CLASSES)).astype(np.float32)
