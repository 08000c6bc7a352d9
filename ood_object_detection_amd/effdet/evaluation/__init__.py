from .detection_evaluator import ObjectDetectionEvaluator, PascalDetectionEvaluator  # noqa: F401
from .dataset_evaluator import DatasetDetectionEvaluator  # noqa: F401
from .open_set_evaluator import OpenSetDetectionEvaluator  # noqa: F401
from .coco_evaluator import CocoDetectionEvaluator  # noqa: F401
from .lvis_evaluator import LvisDetectionEvaluator  # noqa: F401
from .openimages_evaluator import (OpenImagesChallengeEvaluator, OpenImagesDetectionEvaluator,  # noqa: F401
                                   WeightedPascalDetectionEvaluator)
from .calibration_evaluator import CalibrationEvaluator  # noqa: F401
