"""Keypoints / PersonKeypoints (mirror of maskrcnn_benchmark/structures/keypoint.py:8-150): an [n,K,3] fp32 tensor of (x, y, visibility) on any
device + image size (W,H) + extra fields, with the reference's resize / transpose / to / indexing, so that BoxList carries a "keypoints"
field through its own resize / transpose / __getitem__ / to.  The heat-map targets (keypoints_to_heat_map, :154-188) are not here: they are
one launch for the whole batch, ops.kp_select_targets."""
import torch

FLIP_LEFT_RIGHT = 0
FLIP_TOP_BOTTOM = 1


class Keypoints(object):
    def __init__(self, keypoints, size, mode=None):
        device = keypoints.device if isinstance(keypoints, torch.Tensor) else torch.device("cpu")
        keypoints = torch.as_tensor(keypoints, dtype=torch.float32, device=device)
        num_keypoints = keypoints.shape[0]
        if num_keypoints:
            keypoints = keypoints.view(num_keypoints, -1, 3)
        self.keypoints, self.size, self.mode = keypoints, size, mode
        self.extra_fields = {}

    def crop(self, box):
        raise NotImplementedError()

    def _like(self, data, size):
        out = type(self)(data, size, self.mode)
        for k, v in self.extra_fields.items():
            out.add_field(k, v)
        return out

    def resize(self, size, *args, **kwargs):
        ratio_w, ratio_h = (float(s) / float(o) for s, o in zip(size, self.size))
        data = self.keypoints.clone()
        data[..., 0] *= ratio_w
        data[..., 1] *= ratio_h
        return self._like(data, size)

    def transpose(self, method):
        if method not in (FLIP_LEFT_RIGHT,):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT implemented")
        flip_inds = type(self).FLIP_INDS.to(self.keypoints.device)
        data = self.keypoints[:, flip_inds]
        data[..., 0] = self.size[0] - data[..., 0] - 1        # TO_REMOVE = 1
        data[data[..., 2] == 0] = 0                           # COCO: visibility 0 means x = y = 0
        return self._like(data, self.size)

    def to(self, *args, **kwargs):
        out = type(self)(self.keypoints.to(*args, **kwargs), self.size, self.mode)
        for k, v in self.extra_fields.items():
            out.add_field(k, v.to(*args, **kwargs) if hasattr(v, "to") else v)
        return out

    def __getitem__(self, item):
        out = type(self)(self.keypoints[item], self.size, self.mode)
        for k, v in self.extra_fields.items():
            out.add_field(k, v[item])
        return out

    def __len__(self):
        return self.keypoints.shape[0]

    def add_field(self, field, field_data):
        self.extra_fields[field] = field_data

    def get_field(self, field):
        return self.extra_fields[field]

    def __repr__(self):
        return "{}(num_instances={}, image_width={}, image_height={})".format(type(self).__name__, len(self.keypoints), self.size[0], self.size[1])


def _create_flip_indices(names, flip_map):
    full = dict(flip_map)
    full.update({v: k for k, v in flip_map.items()})
    return torch.tensor([names.index(full.get(n, n)) for n in names])


def kp_connections(keypoints):
    pairs = [("left_eye", "right_eye"), ("left_eye", "nose"), ("right_eye", "nose"), ("right_eye", "right_ear"), ("left_eye", "left_ear"),
             ("right_shoulder", "right_elbow"), ("right_elbow", "right_wrist"), ("left_shoulder", "left_elbow"), ("left_elbow", "left_wrist"),
             ("right_hip", "right_knee"), ("right_knee", "right_ankle"), ("left_hip", "left_knee"), ("left_knee", "left_ankle"),
             ("right_shoulder", "left_shoulder"), ("right_hip", "left_hip")]
    return [[keypoints.index(a), keypoints.index(b)] for a, b in pairs]


class PersonKeypoints(Keypoints):
    NAMES = ["nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow",
             "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle"]
    FLIP_MAP = {"left_eye": "right_eye", "left_ear": "right_ear", "left_shoulder": "right_shoulder", "left_elbow": "right_elbow",
                "left_wrist": "right_wrist", "left_hip": "right_hip", "left_knee": "right_knee", "left_ankle": "right_ankle"}


PersonKeypoints.FLIP_INDS = _create_flip_indices(PersonKeypoints.NAMES, PersonKeypoints.FLIP_MAP)
PersonKeypoints.CONNECTIONS = kp_connections(PersonKeypoints.NAMES)
