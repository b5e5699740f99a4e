from .voc import PascalVOCDataset  # noqa: F401
from .voc2012_instance import PascalVOCDataset2012  # noqa: F401
from .coco import COCODataset  # noqa: F401
