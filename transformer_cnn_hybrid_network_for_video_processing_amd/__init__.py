"""MI355X-native (gfx950) CNN backbone + temporal Transformer encoder hot path."""
from .modules import (ConvBNReLUPool, HybridAsymmetricLoss, HybridBCEWithLogitsLoss, HybridCrossEntropyLoss, HybridFocalLoss,  # noqa: F401
                      MixTarget, MultiheadAttention, TransformerCNNHybrid, TransformerEncoder, dense_target)
from .optim import HybridAdamW, HybridLAMB, HybridLARS, HybridSGD  # noqa: F401
from .meter import ClassificationMeter, MultiLabelMeter  # noqa: F401
from .graph import GraphedEval, GraphedPredict, GraphedTrainStep  # noqa: F401
from .fct import FCT, DiceLoss  # noqa: F401
from .encoder32k import Bottleneck, Encoder_32K  # noqa: F401
from .clips import ClipCSVDataset, ClipPipeline, ClipTransform, SyntheticClipSource, collate_clips, t_major  # noqa: F401
from .ops import clip_transform, clip_transform_mix, clip_transform_photo, clip_luma_sums, clip_transform_views, clip_transform_aa, clip_transform_aug  # noqa: F401

__all__ = ["TransformerCNNHybrid", "TransformerEncoder", "MultiheadAttention", "ConvBNReLUPool", "HybridCrossEntropyLoss", "HybridAdamW", "GraphedTrainStep", "GraphedPredict", "FCT", "DiceLoss", "Bottleneck", "Encoder_32K", "ClipCSVDataset", "ClipPipeline", "SyntheticClipSource", "collate_clips", "t_major", "ClipTransform", "clip_transform", "clip_transform_mix", "clip_transform_photo", "clip_luma_sums", "clip_transform_views", "clip_transform_aa", "clip_transform_aug", "MixTarget", "ClassificationMeter", "GraphedEval", "HybridBCEWithLogitsLoss", "dense_target", "HybridFocalLoss", "HybridAsymmetricLoss", "MultiLabelMeter", "HybridLAMB", "HybridSGD", "HybridLARS"]
