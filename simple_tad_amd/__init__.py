"""simple_tad_amd -- MI355X-native (gfx950) Video-ViT forward/backward path behind simple-tad's
``modeling_finetune`` operator surface.  Importing the package never touches the GPU; the HIP
shared library is loaded on first use and every op fails loudly if it is missing."""
from . import registry
from .registry import create_model, register_model, list_models
from . import modeling_finetune
from . import internvideo2
from . import internvideo2_pretrain
from .ops import set_precision, get_precision
from .tuning import TuningScope
from . import mixup, loss, random_erasing, rand_augment, transforms, spatial_sampling, frame_targets, grad_norms
from .grad_norms import GradNormCollector
from . import sequencing, frame_store, frame_resize, prefetch
from .prefetch import ClipPrefetcher
from . import explain
from .explain import attention_rollout, attention_received, token_rollout, saliency_to_frames
from .reconstruct import reconstruct, error_to_frames  # (the function takes the module's name in this namespace)
from .engine_pretrain import evaluate_one_epoch
from .frame_resize import PadWideClips, resize_frames
from .frame_store import FrameStore, FrameWindows, StoreViews
from . import stream_bank
from .stream_bank import StreamBank, YuvFrame
from .mixup import Mixup
from .random_erasing import RandomErasing
from .rand_augment import RandAugment, create_random_augment, frames_to_clip, rand_augment_transform
from .transforms import GroupMultiScaleCrop, DataAugmentationForVideoMAE, DataAugmentationForVideoMAE_LightCrop
from .spatial_sampling import SpatialSampling
from .loss import SoftTargetCrossEntropy, LabelSmoothingCrossEntropy
from .loss import FocalLoss, FocalLoss2, SmoothAPLoss, TemporalExponentialLoss, DoubleBCELoss, build_criterion
from .modeling_finetune import (VisionTransformer, PatchEmbed, Block, Attention, Mlp, DropPath,
                                get_sinusoid_encoding_table)

__all__ = ["set_precision", "get_precision", "TuningScope", "create_model", "register_model", "list_models", "modeling_finetune", "VisionTransformer", "PatchEmbed", "Block",
           "Attention", "Mlp", "DropPath", "get_sinusoid_encoding_table", "mixup", "loss", "random_erasing", "rand_augment", "Mixup", "RandomErasing", "RandAugment", "create_random_augment", "rand_augment_transform", "frames_to_clip", "transforms", "GroupMultiScaleCrop", "DataAugmentationForVideoMAE", "DataAugmentationForVideoMAE_LightCrop", "spatial_sampling", "SpatialSampling", "SoftTargetCrossEntropy", "LabelSmoothingCrossEntropy", "FocalLoss", "FocalLoss2", "SmoothAPLoss", "TemporalExponentialLoss", "DoubleBCELoss", "build_criterion", "frame_targets", "grad_norms", "GradNormCollector", "sequencing", "frame_store", "frame_resize", "PadWideClips", "resize_frames", "FrameStore", "FrameWindows", "StoreViews", "prefetch", "ClipPrefetcher", "explain", "attention_rollout", "attention_received", "token_rollout", "saliency_to_frames", "reconstruct", "error_to_frames", "stream_bank", "StreamBank", "YuvFrame",
           "evaluate_one_epoch"]
