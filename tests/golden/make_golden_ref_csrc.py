#!/usr/bin/env python3
"""tests/golden/ref_csrc.npz FROM THE REFERENCE'S OWN COMPILED C++ (in-container only: needs `make -C oracle ref`):
what oracle/_ref/_C.so returns for the inputs of tests/test_gpu_vs_reference_csrc.py's case builders.
    python tests/golden/make_golden_ref_csrc.py
ROIAlign outputs are kept as digests plus a seeded sample (tests/test_gpu_vs_reference_csrc.py::assert_equals_stored), NMS keep
lists whole; every case also records the digest of its inputs."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh  # noqa: E402
import test_gpu_vs_reference_csrc as T  # noqa: E402


def roi_align_entry(out, key, ref_C, feat, rois, sr):
    want = ref_C.roi_align_forward(feat, rois, 0.0625, 7, 7, sr)
    flat = want.reshape(-1)
    out[key + "_in_sha256"] = T.digest(feat, rois)
    out[key + "_shape"] = np.array(want.shape, np.int64)
    out[key + "_sample"] = flat[torch.from_numpy(T.sample_index(flat.numel()))].numpy()
    out[key + "_sha256"] = T.digest(want)


def main():
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    ref_C = rh.load_ref_C()
    out = {}
    for sr in (0, 2):
        feat, rois = T.roi_align_full_case(sr)
        roi_align_entry(out, "roi_align_sr%d" % sr, ref_C, feat, rois, sr)
        feat, rois, _ = T.roi_align_f64_case(sr)
        roi_align_entry(out, "roi_align_f64_sr%d" % sr, ref_C, feat, rois, sr)
    feat, rois = T.stub_case()
    roi_align_entry(out, "stub", ref_C, feat, rois, 0)
    for i, (n, thr, b, s) in enumerate(T.nms_cases()):
        out["nms%d_in_sha256" % i] = T.digest(b, s)
        out["nms%d_keep" % i] = ref_C.nms(b, s, thr).numpy()
    scores, boxes, sc, order_ref = T.nms_ties_case()
    n = scores.shape[0]
    out["ties_in_sha256"] = T.digest(boxes, sc)
    out["ties_keep_sorted"] = ref_C.nms(boxes[order_ref], torch.arange(n, 0, -1, dtype=torch.float32), 0.6).numpy()
    out = {k: np.asarray(v) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "ref_csrc.npz"), **out)
    print("wrote ref_csrc.npz: " + ", ".join("{}{}".format(k, list(v.shape)) for k, v in out.items()))


if __name__ == "__main__":
    main()
