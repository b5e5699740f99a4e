#!/usr/bin/env python3
"""Feature-pyramid pooler golden FROM THE REFERENCE (in-container only): the reference's own modeling/poolers.py
`Pooler((7, 7), (0.25, 0.125, 0.0625, 0.03125), 2)` and its `map_levels` run on the CPU (its _C built by `make -C oracle ref`) over the
RoI set of tests/pooler_ref.py: B = 2, C = 8, a 128 x 192 image with maps 32 x 48 down to 4 x 6, the level rule's boundary rows, the rows
without a level and random rows (boxes may be larger than the image).
Stored as tests/golden/pooler_fpn.npz: rois [K,5], per_image [B] (rows of each BoxList), levels [K] (the reference's, as it returns them: int64 minus the float k_min, so float32; a
row without a level holds whatever the NaN cast gives), out [K,C,7,7], and seed / B / C / maps to rebuild the feature maps with
pooler_ref.make_feats."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh  # noqa: E402
import pooler_ref as P  # noqa: E402

B, C, IMG_H, IMG_W, SEED = 2, 8, 128, 192, 20240
MAPS = [(32, 48), (16, 24), (8, 12), (4, 6)]


def main():
    rh.setup()
    from maskrcnn_benchmark.modeling.poolers import Pooler
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    rois, _ = P.roi_set(B, IMG_H, IMG_W, MAPS, per_img=30, seed=1)
    rois = rois[np.argsort(rois[:, 0], kind="stable")]          # BoxLists are per image: rows in image order
    per_image = [int((rois[:, 0] == b).sum()) for b in range(B)]
    feats = P.make_feats(SEED, B, C, MAPS)
    pooler = Pooler((7, 7), P.SCALES, 2)
    boxes = [BoxList(torch.from_numpy(rois[rois[:, 0] == b, 1:].copy()), (IMG_W, IMG_H), mode="xyxy") for b in range(B)]
    x = [torch.from_numpy(np.ascontiguousarray(f.transpose(0, 3, 1, 2))) for f in feats]
    with torch.no_grad():
        levels = pooler.map_levels(boxes)
        out = pooler(x, boxes)
    np.savez_compressed(os.path.join(HERE, "pooler_fpn.npz"), rois=rois, per_image=np.array(per_image, np.int64), levels=levels.numpy(),
                        out=out.numpy(), seed=np.int64(SEED), B=np.int64(B), C=np.int64(C), maps=np.array(MAPS, np.int64),
                        image=np.array([IMG_H, IMG_W], np.int64))
    print("rows", len(rois), "per level", np.bincount(np.clip(levels.numpy(), -1, 4).astype(np.int64) + 1).tolist())


if __name__ == "__main__":
    main()
