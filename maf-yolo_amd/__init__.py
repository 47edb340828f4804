"""MAF-YOLO hot path, MI355X-native: Model.forward() / non_max_suppression() over hand-written HIP kernels.

See DESIGN.md.  Importing this package does not need a GPU; running it does (no CPU fallback)."""
from . import lib, arch, pack, synth  # noqa: F401
from .lib import MafError  # noqa: F401
from .model import Model, Detect_yaml  # noqa: F401
from .nms import non_max_suppression, non_max_suppression_async, nms_raw  # noqa: F401
from .post import convert_to_coco_format, coco_rows  # noqa: F401
from .letterbox import letterbox, eval_batch, rescale_boxes, detect_frames, resize_area  # noqa: F401
from .augment import TrainAugment, train_batch  # noqa: F401
from . import metrics  # noqa: F401
from .metrics import PrMetric  # noqa: F401
from . import cocoeval  # noqa: F401
from .cocoeval import CocoGt, CocoEval  # noqa: F401
from . import jpeg  # noqa: F401
from .jpeg import JpegUnsupported  # noqa: F401
from . import jpeg_encode  # noqa: F401
from . import png_encode  # noqa: F401
from . import tiff_encode  # noqa: F401
from . import webp_encode  # noqa: F401
from . import bmp_encode  # noqa: F401
from . import png  # noqa: F401
from .png import PngUnsupported  # noqa: F401
from . import webp  # noqa: F401
from .webp import WebpUnsupported  # noqa: F401
from . import webp_lossy  # noqa: F401
from . import tiff  # noqa: F401
from . import bmp  # noqa: F401
from . import frames  # noqa: F401
from .checkpoint import load_checkpoint, reference_state_dict  # noqa: F401
from .loss import ComputeLoss, task_aligned_assign  # noqa: F401
from .streams import concurrent_streams  # noqa: F401
from .eval_loop import EvalLoop  # noqa: F401
from .solver import build_optimizer, ModelEMA, GradScaler  # noqa: F401
from .exchange import GradExchange  # noqa: F401
from .layers import RepVGGBlock, UniRepLKNetBlock  # noqa: F401  (isinstance loops of evaler.py:101-109 stay harmless)


def build_model(cfg, num_classes=80, device="cuda", img_size=640):
    """Counterpart of yolov6/models/yolo.py:290-297."""
    return Model(cfg, channels=3, num_classes=num_classes).to(device)
