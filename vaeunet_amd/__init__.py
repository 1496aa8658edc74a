"""MI355X-native (gfx950 HIP) training path for the tmuird/VAEUNET VAE-U-Net.

Drop-in surface (same names / signatures / state_dict keys as the reference):
  unet.UNet, unet.unet_parts.{DoubleConv, Down, Up, AttentionGate, OutConv},
  unet.unet_resnet.{UNetResNet, DecoderBlock}, utils.loss.*, utils.metrics.{dice_score,
  iou_score, precision_recall, specificity, accuracy, get_all_metrics}, evaluate.evaluate
Calibration / uncertainty metrics (utils/uncertainty_metrics.py's numbers; unpinned):
  calibration.{calib_hist, calib_metrics, CalibrationMeter}
Lesion-level evaluation (unpinned): lesions.{label_components, component_areas,
  remove_small_components, lesion_counts, lesion_metrics, LesionMeter}
Boundary metrics (unpinned): surface.{distance_transform, boundary, surface_stats,
  surface_metrics, SurfaceMeter}
Boundary loss (Kervadec et al.'s definitions): surface.signed_distance,
  loss.{boundary_loss, BoundaryLoss, BoundaryAugmentedLoss}
Sample-set metrics (unpinned): samples.{sample_gram, sample_set_metrics, SampleSetMeter,
  SAMPLESET_METRIC_NAMES}, inference.sample_set_scores
Patch loader with device-side training augmentation (unpinned):
  data.{PatchCache, TrainAugment, augment_patches}
Dispatcher ops: torch.ops.vaeunet.* (vaeunet_amd.ops)
"""
from .unet_model import UNet  # noqa: F401
from .unet_parts import AttentionGate, DoubleConv, Down, Up, OutConv  # noqa: F401
from .unet_resnet import UNetResNet, DecoderBlock  # noqa: F401,E402
from . import ops  # noqa: F401,E402  (registers torch.ops.vaeunet.*)
from .metrics import (dice_score, iou_score, precision_recall, specificity, accuracy,  # noqa: F401,E402
                      get_all_metrics, seg_counts, seg_metrics, SegmentationMeter)
from .evaluate import evaluate, evaluate_with_lesions, evaluate_with_surface  # noqa: F401,E402
from .calibration import calib_hist, calib_metrics, CalibrationMeter, CalibCounts  # noqa: F401,E402
from .lesions import (label_components, component_areas, remove_small_components, lesion_counts,  # noqa: F401,E402
                      lesion_metrics, LesionMeter)
from .surface import (distance_transform, boundary, surface_stats, surface_metrics, SurfaceMeter,  # noqa: F401,E402
                      signed_distance)
from .loss import boundary_loss, BoundaryLoss, BoundaryAugmentedLoss  # noqa: F401,E402
from .samples import sample_gram, sample_set_metrics, SampleSetMeter, SAMPLESET_METRIC_NAMES  # noqa: F401,E402
