"""cosypose_amd: MI355X-native implementation of CosyPose's render-and-compare pose-refinement
hot path (coarse + refiner loop) behind the reference's Python API.  See DESIGN.md."""
from .tensor_collection import TensorCollection, PandasTensorCollection, concatenate  # noqa: F401


def __getattr__(name):  # lazy: importing the package must not require torch.cuda or the built library
    if name in ('PosePredictor',):
        from .pose import PosePredictor
        return PosePredictor
    if name in ('CoarseRefinePosePredictor',):
        from .pose_predictor import CoarseRefinePosePredictor
        return CoarseRefinePosePredictor
    if name in ('create_model_pose', 'create_model_refiner', 'create_model_coarse', 'check_update_config'):
        from . import pose_models_cfg
        return getattr(pose_models_cfg, name)
    if name == 'BatchedMeshes':
        from .mesh_db import BatchedMeshes
        return BatchedMeshes
    if name in ('MeshDataBase', 'make_bop_symmetries'):
        from . import mesh_db
        return getattr(mesh_db, name)
    if name == 'model_info':      # the function and its module share the name, as bop_errors: the module is callable
        import importlib
        return importlib.import_module('.model_info', __name__)
    if name in ('HipBatchRenderer', 'RenderMeshes'):
        from . import rasterizer
        return getattr(rasterizer, name)
    if name in ('HipSceneRenderer', 'scene_visibility'):
        from . import scene_renderer
        return getattr(scene_renderer, name)
    if name == 'MultiviewScenePredictor':
        from .multiview_predictor import MultiviewScenePredictor
        return MultiviewScenePredictor
    if name in ('MultiviewRefinement', 'solve_problems'):
        from . import bundle_adjustment
        return getattr(bundle_adjustment, name)
    if name == 'multiview_candidate_matching':
        from .multiview_matching import multiview_candidate_matching
        return multiview_candidate_matching
    if name == 'PoseErrorMeter':
        from .pose_meters import PoseErrorMeter
        return PoseErrorMeter
    if name == 'BopModels':
        from .bop_errors import BopModels
        return BopModels
    if name == 'bop_errors':      # the function and its module share the name: the module is callable (see its last lines)
        import importlib
        return importlib.import_module('.bop_errors', __name__)
    if name == 'BopScoreMeter':
        from .bop_meters import BopScoreMeter
        return BopScoreMeter
    if name == 'h_pose':
        from .pose_forward_loss import h_pose
        return h_pose
    if name in ('augment_batch', 'draw_sample_params', 'pack_params'):
        from . import augmentations
        return getattr(augmentations, name)
    if name == 'resize_images':
        from .resize import resize_images
        return resize_images
    if name == 'resize_frames':
        from .frames import resize_frames
        return resize_frames
    if name in ('DetectionMeter', 'box_iou', 'box_iou_pairs'):
        from . import detection_meters
        return getattr(detection_meters, name)
    if name in ('mask_instance_stats', 'make_detections_from_segmentation', 'visible_ids', 'instance_masks', 'detection_targets'):
        from . import mask_ops
        return getattr(mask_ops, name)
    if name in ('nms', 'batched_nms', 'postprocess_detections', 'paste_masks', 'detections_from_heads'):
        from . import detector
        return getattr(detector, name)
    if name in ('rpn_anchors', 'rpn_proposals', 'multiscale_roi_align', 'roi_align', 'detections_from_features'):
        from . import detector_rpn
        return getattr(detector_rpn, name)
    if name in ('match_boxes', 'sample_balanced', 'encode_boxes', 'rpn_loss', 'roi_training_samples', 'fastrcnn_loss', 'mask_targets',
                'maskrcnn_loss', 'detector_losses', 'AnchorGrid'):
        from . import detector_train
        return getattr(detector_train, name)
    if name == 'detector_input':  # the function and its module share the name, as model_info: the module is callable
        import importlib
        return importlib.import_module('.detector_input', __name__)
    if name in ('detections_from_frames', 'detector_losses_from_frames', 'DetectorInput'):
        from . import detector_input
        return getattr(detector_input, name)
    if name in ('DetectorHeads', 'HeadLayer', 'conv_layer', 'TrainableLayer', 'layer_backward'):
        from . import detector_heads
        return getattr(detector_heads, name)
    if name in ('DetectorTrunk', 'Detector', 'TrunkLayer', 'trunk_conv_layer'):
        from . import detector_trunk
        return getattr(detector_trunk, name)
    if name in ('TrainableTrunkLayer', 'trunk_dgrad', 'trunk_wgrad', 'layer_dgrad', 'layer_wgrad'):
        from . import detector_trunk_backward
        return getattr(detector_trunk_backward, name)
    if name in ('FlatSGD', 'PackTable'):
        from . import detector_optim
        return getattr(detector_optim, name)
    if name in ('h_maskrcnn', 'train_detector_loop'):
        from . import detector_training
        return getattr(detector_training, name)
    if name in ('gt_info', 'annotate_gt'):
        from . import gt_annotations
        return getattr(gt_annotations, name)
    raise AttributeError(name)
