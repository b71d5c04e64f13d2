"""Drop-in nn.Modules for the hot path.  Class names, constructor/forward signatures and state-dict
keys follow the reference:

* ``MultiheadAttention(input_dim, num_heads)`` / ``forward(q, k, v, mask=None)``
  and ``TransformerEncoder(input_dim, hidden_dim, num_layers, num_heads, dropout)`` / ``forward(input, mask)``
  -- ``__pycache__/TransformerEncoder.cpython-38.pyc`` src L6-L126.
* the conv stage is the first Conv+BN+ReLU triple of ``UNet._block`` (UNet.py:54-66) + ``MaxPool2d(2,2)``
  (UNet.py:13) with the reference's key names ``encoder{i}.enc{i}conv1.weight``, ``encoder{i}.enc{i}norm1.*``.
* ``TransformerCNNHybrid()`` is zero-argument constructible and is called as ``model(x)`` exactly like the
  reference harnesses call their models (Model.py:27,56 / FCT.py:302,330).

Parameters are ordinary fp32 ``nn.Parameter``s, so stock AdamW, checkpointing and gradient
all-reduce work unchanged.  All compute runs in the HIP library through the ``torch.ops.hybrid.*`` custom operators
(ops.py); CPU tensors raise RuntimeError.
"""
import math
from collections import OrderedDict
from typing import NamedTuple

import torch
import torch.nn as nn

from . import ops


def split_compute_dtype(name):
    """-> (backbone dtype, temporal dtype).  'mixed' = ('bf16', 'bf16x3'): the conv stages (99.7 % of the FLOPs) in bf16, the token projection
    + temporal encoder + head in fp32 storage with split-bf16 MFMA products -- the bf16 mode's logits error comes from the temporal half
    (measured at config 2, eval: 9.0e-3 all bf16, 5.1e-4 with only the backbone in bf16; scripts/exp/logit_error_split.py), so this mode
    keeps north_star's 1e-3 at nearly the bf16 mode's speed.  A pair ('bf16', 'fp32') etc. is taken as given."""
    if isinstance(name, (tuple, list)) and len(name) == 2:
        return name[0], name[1]
    if isinstance(name, str) and name == "mixed":
        return "bf16", "bf16x3"
    return name, name


class _ComputeDtypeMixin:
    def set_compute_dtype(self, name):
        """'bf16' (default: bf16 storage + bf16 MFMA, fp32 accumulate), 'bf16x3' (fp32 storage, three bf16 MFMAs per product) or 'fp32'
        (exact fp32 MFMA; parity gate).  TransformerCNNHybrid also takes 'mixed' / a (backbone, temporal) pair (split_compute_dtype)."""
        code = ops.dtype_code(name)
        for m in self.modules():
            if isinstance(m, _ComputeDtypeMixin):
                m._dt = code
        return self


class ConvBNReLUPool(nn.Sequential, _ComputeDtypeMixin):
    """Conv2d(3x3, pad 1, bias=False) -> BatchNorm2d -> ReLU -> MaxPool2d(2, 2) as ONE fused HIP stage.

    The child modules exist to own the parameters/buffers under the reference's key names
    (``{name}conv1.weight``, ``{name}norm1.{weight,bias,running_mean,running_var,num_batches_tracked}``);
    their own forward()s are never called."""

    def __init__(self, in_channels, features, name, compute_dtype="bf16"):
        super().__init__(OrderedDict([
            (name + "conv1", nn.Conv2d(in_channels, features, kernel_size=3, padding=1, bias=False)),
            (name + "norm1", nn.BatchNorm2d(num_features=features)),
        ]))
        self._conv = name + "conv1"
        self._norm = name + "norm1"
        self.in_channels, self.features = in_channels, features
        self._dt = ops.dtype_code(compute_dtype)

    def forward_nhwc(self, x, first, commit=None):
        """x: NCHW fp32 frames when ``first`` else NHWC compute-dtype activations. Returns NHWC.  ``commit``: see ops.convstage."""
        conv, bn = getattr(self, self._conv), getattr(self, self._norm)
        if bn.momentum is None:
            raise RuntimeError("cumulative-average BatchNorm (momentum=None) is not supported")
        training = self.training or not bn.track_running_stats or bn.running_mean is None
        return ops.convstage(x, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                             training, bn.momentum, bn.eps, self._dt, first, commit)

    def forward(self, x):
        """Standalone use: [N,C,H,W] fp32 in, [N,features,H/2,W/2] fp32 out."""
        if x.dim() != 4:
            raise ValueError("expected [N,C,H,W]")
        if self.in_channels <= 4:
            h = self.forward_nhwc(x.float(), True)
        else:
            h = self.forward_nhwc(ops.nchw_to_nhwc(x, self._dt, ops.pad_channels(self.in_channels)), False)
        return ops.nhwc_to_nchw(h, self._dt, self.features)

    def infer_nhwc(self, x, first):
        """forward_nhwc for inference: BatchNorm from the running statistics whatever ``self.training`` says, nothing saved, and (bf16) the
        conv's epilogue applies BatchNorm + ReLU + MaxPool, so no full-resolution conv output exists.  Call under ``torch.no_grad()``."""
        conv, bn = getattr(self, self._conv), getattr(self, self._norm)
        if not bn.track_running_stats or bn.running_mean is None:
            raise RuntimeError("inference needs BatchNorm running statistics (track_running_stats=True)")
        return ops.convstage_infer(x, conv.weight, bn, self._dt, first)

    @torch.no_grad()
    def infer(self, x):
        """Standalone inference: [N,C,H,W] fp32 in, [N,features,H/2,W/2] fp32 out; eval semantics, ``self.training`` untouched."""
        if x.dim() != 4:
            raise ValueError("expected [N,C,H,W]")
        if not x.is_cuda:
            raise RuntimeError("ConvBNReLUPool runs on the MI355X HIP path only: move the module and input to 'cuda' (there is no CPU fallback)")
        if self.in_channels <= 4:
            h = self.infer_nhwc(x.float(), True)
        else:
            h = self.infer_nhwc(ops.nchw_to_nhwc(x, self._dt, ops.pad_channels(self.in_channels)), False)
        return ops.nhwc_to_nchw(h, self._dt, self.features)


class MultiheadAttention(nn.Module, _ComputeDtypeMixin):
    def __init__(self, input_dim, num_heads, compute_dtype="bf16"):                 # src L7-19
        super().__init__()
        self.input_dim = input_dim
        self.num_heads = num_heads
        self.query_layer = nn.Linear(input_dim, input_dim)
        self.key_layer = nn.Linear(input_dim, input_dim)
        self.value_layer = nn.Linear(input_dim, input_dim)
        self.output_layer = nn.Linear(input_dim, input_dim)
        self.activation = nn.ReLU()
        self.softmax = nn.Softmax(dim=-1)
        self.dropoutLayer = nn.Dropout(0.1)
        self._dt = ops.dtype_code(compute_dtype)

    def _attn_p(self):
        return self.dropoutLayer.p if self.training else 0.0                         # quirk Q5

    def _params(self):
        return [self.query_layer.weight, self.query_layer.bias, self.key_layer.weight, self.key_layer.bias,
                self.value_layer.weight, self.value_layer.bias, self.output_layer.weight, self.output_layer.bias]

    def forward(self, q, k, v, mask=None):                                           # src L67-89
        if self.input_dim % self.num_heads != 0:
            raise ValueError("input_dim must be divisible by num_heads")
        out = ops.mha(ops.to_compute(q, self._dt), ops.to_compute(k, self._dt), ops.to_compute(v, self._dt), mask, self._params(),
                      self._dt, self.num_heads, self._attn_p(), ops.next_seed())
        return ops.to_f32(out, self._dt)


class TransformerEncoder(nn.Module, _ComputeDtypeMixin):
    def __init__(self, input_dim, hidden_dim, num_layers, num_heads, dropout, compute_dtype="bf16"):   # src L94-108
        super().__init__()
        self.input_dim = input_dim
        self.hidden_dim = hidden_dim
        self.num_layers = num_layers
        self.num_heads = num_heads
        self.dropout = dropout
        if input_dim % num_heads != 0:
            raise ValueError(
                f"Input dimension must be divisible by number of heads. Here, Input dimension = {input_dim}"
                f" is not divisible by number of heads = {num_heads}")
        self.attention_layers = nn.ModuleList(
            [MultiheadAttention(input_dim, num_heads, compute_dtype) for _ in range(num_layers)])
        self.feedforward_layers = nn.ModuleList(
            [nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, input_dim))
             for _ in range(num_layers)])
        self.layer_norm = nn.ModuleList([nn.LayerNorm(input_dim) for _ in range(num_layers)])
        self._dt = ops.dtype_code(compute_dtype)

    def _flat_params(self):
        ps = []
        for i in range(self.num_layers):
            ps += self.attention_layers[i]._params()
            ff = self.feedforward_layers[i]
            ps += [ff[0].weight, ff[0].bias, ff[2].weight, ff[2].bias, self.layer_norm[i].weight, self.layer_norm[i].bias]
        return ps

    def forward_compute(self, x, mask):
        """x already in the compute dtype ([B,S,D]); returns the compute dtype."""
        attn_p = self.attention_layers[0]._attn_p() if self.num_layers else 0.0
        return ops.encoder(x, mask, self._flat_params(), self._dt, self.hidden_dim, self.num_layers, self.num_heads, attn_p,
                           float(self.dropout), ops.next_seed())                                  # Q6: the per-layer dropout is always active

    def forward(self, input, mask):                                                  # src L110-126
        return ops.to_f32(self.forward_compute(ops.to_compute(input, self._dt), mask), self._dt)


class MixTarget(NamedTuple):
    """The labels of a Mixup / CutMix batch, all on the device: clip b carries class ``y_a[b]`` with weight ``lam[b]`` and class ``y_b[b]`` with
    weight ``1 - lam[b]`` (int64 [B], int64 [B], fp32 [B]).  ClipPipeline yields one with a mixing ClipTransform; HybridCrossEntropyLoss,
    forward_temporal_loss and GraphedTrainStep take one where they take a class-index tensor."""
    y_a: torch.Tensor
    y_b: torch.Tensor
    lam: torch.Tensor


def _is_dense(target):
    """A dense target: a floating tensor, one row of C numbers per clip (class indices are integer tensors, mixed labels a MixTarget)."""
    return isinstance(target, torch.Tensor) and target.is_floating_point()


def _class_vector(name, v):
    """A per-class vector of a criterion (weight, pos_weight): 1-D fp32, no negative or NaN entry; cloned for the buffer."""
    if v is None:
        return None
    if not isinstance(v, torch.Tensor) or v.dim() != 1 or v.dtype != torch.float32:
        raise ValueError(f"{name} must be a 1-D float32 tensor with one entry per class")
    if bool((v < 0).any()) or bool(torch.isnan(v).any()):
        raise ValueError(f"{name} must not have a negative entry")
    return v.detach().clone()


def _check_dense(target, B, C, logits=None):
    """logits: the stand-alone criterion's; None: the fused loss, whose logits [B, C] do not exist yet."""
    if target.dtype != torch.float32:
        raise TypeError(f"a dense target must be float32, got {target.dtype}")
    if logits is not None and (logits.dim() != 2 or target.dim() != 2 or target.shape != logits.shape):
        raise ValueError(f"a dense target has the shape of the logits [B,C]: got logits {tuple(logits.shape)} and target {tuple(target.shape)}")
    if target.dim() != 2 or tuple(target.shape) != (B, C):
        raise ValueError(f"a dense target has the shape of the logits [B={B},C={C}]: got {tuple(target.shape)}")


def dense_target(y, num_classes, label_smoothing=0.0):
    """Class indices int64 [B], or a ``MixTarget``, as the dense fp32 [B, num_classes] target of the same labels, on their device, with plain
    torch operations: one-hot rows, or ``lam * one_hot(y_a) + (1 - lam) * one_hot(y_b)``; with ``label_smoothing`` e the row is
    ``(1 - e) * row + e / num_classes``.  What a mixing ClipPipeline's labels need in front of HybridBCEWithLogitsLoss."""
    e = float(label_smoothing)
    if not 0.0 <= e <= 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1], got {e}")
    C = int(num_classes)

    def one_hot(t):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
            raise TypeError("dense_target takes class indices int64 [B] or a MixTarget")
        return torch.nn.functional.one_hot(t, C).to(torch.float32)
    if isinstance(y, MixTarget):
        lam = y.lam.to(torch.float32).unsqueeze(1)
        t = lam * one_hot(y.y_a) + (1.0 - lam) * one_hot(y.y_b)
    else:
        t = one_hot(y)
    if e != 0.0:
        t = (1.0 - e) * t + e / C
    return t.contiguous()


def _address(name, t):
    """A criterion's buffer as a captured launch holds it, by address: an in-place update is read, a replaced buffer is not."""
    return _BUFFER_NAME[name], None if t is None else t.data_ptr()


_BUFFER_NAME = {n: f"the {n} buffer (replaced, not updated in place)" for n in ("weight", "pos_weight")}


class _Criterion(nn.Module):
    """What the four criteria share.  Each describes its own call: ``_loss_call(target, B, C, device, logits=None)`` checks the target and
    the per-class vectors against logits [B, C] on ``device`` (``logits`` themselves where they exist: the stand-alone call) and returns
    (family, loss_args) -- the ops.LOSS_FAMILIES row that computes the criterion on that target and the arguments the row's schema lists.
    forward() hands them to the stand-alone operator, forward_temporal_loss to the fused one.  ``_captured()`` -> [(name, value)]: what a
    captured launch carries by value, and the addresses of the buffers it reads."""

    def forward(self, logits, target):
        return ops.cross_entropy_loss(logits, *self._loss_call(target, logits.shape[0], logits.shape[-1], logits.device, logits))


class HybridCrossEntropyLoss(_Criterion):
    """Mean cross-entropy over the batch (the composite's own loss), one HIP kernel each way.

    ``weight`` (one fp32 entry >= 0 per class), ``ignore_index`` and ``label_smoothing`` mean what they mean in ``nn.CrossEntropyLoss``
    with reduction "mean": the kept clips' terms are summed and divided by the sum of their target weights.  Two differences: the default
    ``ignore_index`` is None (no class index is ignored; torch's default is -100), and a target outside [0, C) that is not ``ignore_index``
    makes the loss NaN instead of raising a device assert.  When every clip is ignored or carries zero weight, the loss is NaN and the
    gradient is zero.  With all three at their defaults this is the plain batch mean, through the operators it always used.

    ``weight`` is a registered buffer (``.cuda()`` and ``state_dict()`` carry it) and is read by the kernels when they run: an in-place update
    of the buffer is seen by the next call, and by the next replay of a GraphedTrainStep.  Under data parallelism each rank divides by the
    weight sum of its own clips and the gradients are averaged over the ranks -- exactly what DistributedDataParallel does with
    ``nn.CrossEntropyLoss(weight=...)``; no global weight sum is exchanged.

    ``target`` may be a ``MixTarget(y_a, y_b, lam)``: the loss is sum_b [lam_b term(b, y_a) + (1 - lam_b) term(b, y_b)] over the same mix of
    the target weights (include/hybrid_hip.h, hyb_cross_entropy_mix_*), with any combination of the options, none included; each side keeps
    the rules above on its own, a lam outside [0, 1] makes the loss NaN.  With one lam for the batch, ``y_b`` a permutation of ``y_a`` and
    nothing ignored it is ``lam * CE(logits, y_a) + (1 - lam) * CE(logits, y_b)``.  A plain tensor target takes the path it always took.

    A floating ``target`` [B, C] is a row of class probabilities per clip, torch's own convention: soft-target cross-entropy
    (include/hybrid_hip.h, hyb_cross_entropy_dense_*, kind 0) with ``weight`` and ``label_smoothing``; the sum of the clips' terms is divided
    by B, not by a weight sum (torch's rule for probability targets), rows are used as given (fp32, contiguous; not normalised), and a
    criterion with an ``ignore_index`` raises ValueError, as torch does."""

    def __init__(self, weight=None, ignore_index=None, label_smoothing=0.0):
        super().__init__()
        label_smoothing = float(label_smoothing)
        if not 0.0 <= label_smoothing <= 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing}")
        if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int)):
            raise TypeError(f"ignore_index must be an int or None, got {ignore_index!r}")
        self.register_buffer("weight", _class_vector("weight", weight))
        self.ignore_index, self.label_smoothing = ignore_index, label_smoothing

    def has_options(self):
        return self.weight is not None or self.ignore_index is not None or self.label_smoothing != 0.0

    def options(self):
        """(weight buffer or None, ignore_index or None, label_smoothing): what the option-carrying operators take."""
        return self.weight, self.ignore_index, self.label_smoothing

    def _check_weight(self, C):
        if self.weight is not None and self.weight.shape[0] != C:
            raise ValueError(f"weight has {self.weight.shape[0]} entries but the logits have {C} classes")

    def _refuse_ignore_index(self):
        if self.ignore_index is not None:
            raise ValueError("ignore_index is not supported with a dense (class-probability) target")

    def _loss_call(self, target, B, C, device, logits=None):
        """A dense target: soft-target cross-entropy (dense, kind 0); a MixTarget: mix; class indices: opts, or -- no options -- the plain
        operators it always used."""
        if _is_dense(target):
            self._refuse_ignore_index()
            _check_dense(target, B, C, logits)
            self._check_weight(C)
            return "dense", (target, self.weight, None, 0, float(self.label_smoothing))
        if not isinstance(target, MixTarget) and not self.has_options():
            return "plain", (target,)
        self._check_weight(C)
        opts = (self.weight, *ops.ignore_args(self.ignore_index), float(self.label_smoothing))
        return ("mix", (*target, *opts)) if isinstance(target, MixTarget) else ("opts", (target, *opts))

    def _captured(self):
        return [("ignore_index", self.ignore_index), ("label_smoothing", self.label_smoothing), _address("weight", self.weight)]

    def extra_repr(self):
        return f"ignore_index={self.ignore_index}, label_smoothing={self.label_smoothing}"


class HybridBCEWithLogitsLoss(_Criterion):
    """Mean binary cross-entropy with logits over all B x C entries, ``nn.BCEWithLogitsLoss(weight, pos_weight)`` with per-class vectors, one
    HIP kernel each way (include/hybrid_hip.h, hyb_cross_entropy_dense_*, kind 1; the overflow-safe form).  ``target`` is fp32 [B, C],
    contiguous, on the logits' device: multi-label clips, or ``dense_target(y, C)`` of a mixing ClipPipeline's labels.

    ``weight`` and ``pos_weight`` (one fp32 entry >= 0 per class, or None = all ones) are registered buffers read by the kernels when they
    run: an in-place update is seen by the next call and by the next replay of a GraphedTrainStep."""

    def __init__(self, weight=None, pos_weight=None):
        super().__init__()
        self.register_buffer("weight", _class_vector("weight", weight))
        self.register_buffer("pos_weight", _class_vector("pos_weight", pos_weight))

    def _check_weight(self, C):
        for name in ("weight", "pos_weight"):
            v = getattr(self, name)
            if v is not None and v.shape[0] != C:
                raise ValueError(f"{name} has {v.shape[0]} entries but the logits have {C} classes")

    def _loss_call(self, target, B, C, device, logits=None):
        """Always the dense family, kind 1."""
        if not _is_dense(target):
            raise TypeError("HybridBCEWithLogitsLoss takes a floating target [B,C] (dense_target() makes one from class indices or a MixTarget)")
        _check_dense(target, B, C, logits)
        self._check_weight(C)
        return "dense", (target, self.weight, self.pos_weight, 1, 0.0)

    def _captured(self):
        return [_address("weight", self.weight), _address("pos_weight", self.pos_weight)]


def _gamma(name, g):
    """A focusing exponent: a real number that is 0 or >= 1 (include/hybrid_hip.h says why nothing between)."""
    if isinstance(g, bool) or not isinstance(g, (int, float)):
        raise TypeError(f"{name} must be a number, got {g!r}")
    g = float(g)
    if not (g == 0.0 or 1.0 <= g < float("inf")):
        raise ValueError(f"{name} must be 0 or >= 1, got {g}")
    return g


class HybridFocalLoss(_Criterion):
    """Mean focal loss on class indices int64 [B] (Lin et al. 2017, the softmax form), one HIP kernel each way (include/hybrid_hip.h,
    hyb_cross_entropy_focal_*): every kept clip's cross-entropy term times ``(1 - p_target) ** gamma``, summed and divided by the kept
    clips' target weights -- ``HybridCrossEntropyLoss(weight, ignore_index)``'s rules throughout (an ignored clip adds nothing, all ignored
    gives NaN with a zero gradient, a kept target outside [0, C) gives NaN), and its bits at ``gamma == 0``.  ``gamma`` is 0 or >= 1; there
    is no label smoothing.  A ``MixTarget`` or a dense floating target raises TypeError.

    ``weight`` (one fp32 entry >= 0 per class, or None) is a registered buffer read by the kernels when they run: an in-place update is
    seen by the next call and by the next replay of a GraphedTrainStep; ``gamma`` and ``ignore_index`` travel by value."""

    def __init__(self, gamma=2.0, weight=None, ignore_index=None):
        super().__init__()
        if ignore_index is not None and (isinstance(ignore_index, bool) or not isinstance(ignore_index, int)):
            raise TypeError(f"ignore_index must be an int or None, got {ignore_index!r}")
        self.gamma = _gamma("gamma", gamma)
        self.register_buffer("weight", _class_vector("weight", weight))
        self.ignore_index = ignore_index

    def _check_weight(self, C):
        if self.weight is not None and self.weight.shape[0] != C:
            raise ValueError(f"weight has {self.weight.shape[0]} entries but the logits have {C} classes")

    @staticmethod
    def _check_target(target):
        if isinstance(target, MixTarget) or _is_dense(target):
            raise TypeError("HybridFocalLoss takes class indices int64 [B] (no MixTarget, no dense target)")

    def _loss_call(self, target, B, C, device, logits=None):
        self._check_target(target)
        self._check_weight(C)
        return "focal", (target, self.weight, *ops.ignore_args(self.ignore_index), _gamma("gamma", self.gamma))

    def _captured(self):
        return [("ignore_index", self.ignore_index), ("gamma", self.gamma), _address("weight", self.weight)]

    def extra_repr(self):
        return f"gamma={self.gamma}, ignore_index={self.ignore_index}"


class HybridAsymmetricLoss(_Criterion):
    """Mean asymmetric loss over all B x C entries (Ridnik et al. 2021) on a floating target [B, C], one HIP kernel each way
    (include/hybrid_hip.h, hyb_cross_entropy_asym_*): positives are focused with ``gamma_pos``, negatives with ``gamma_neg`` after their
    probability is shifted down by ``clip`` (a negative below it adds nothing); the gradient includes the focusing factor.  Each exponent
    is 0 or >= 1, ``clip`` in [0, 1).  ``target`` is fp32, contiguous, on the logits' device; soft rows are used as given.

    ``weight`` and ``pos_weight`` (one fp32 entry >= 0 per class, or None = all ones) are registered buffers read by the kernels when they
    run, as in HybridBCEWithLogitsLoss; the exponents and ``clip`` travel by value.  ``sigmoid_focal(gamma, alpha)`` is the sigmoid focal
    loss with reduction "mean" as a special case."""

    def __init__(self, gamma_neg=4.0, gamma_pos=0.0, clip=0.05, weight=None, pos_weight=None):
        super().__init__()
        self.gamma_neg, self.gamma_pos = _gamma("gamma_neg", gamma_neg), _gamma("gamma_pos", gamma_pos)
        self.clip = self._clip(clip)
        self.register_buffer("weight", _class_vector("weight", weight))
        self.register_buffer("pos_weight", _class_vector("pos_weight", pos_weight))

    @staticmethod
    def _clip(clip):
        if isinstance(clip, bool) or not isinstance(clip, (int, float)):
            raise TypeError(f"clip must be a number, got {clip!r}")
        if not 0.0 <= float(clip) < 1.0:
            raise ValueError(f"clip must be in [0, 1), got {clip}")
        return float(clip)

    @classmethod
    def sigmoid_focal(cls, gamma=2.0, alpha=0.25):
        """``mean(alpha_t * (1 - p_t) ** gamma * bce)`` with ``alpha_t = alpha`` on positives and ``1 - alpha`` on negatives: one exponent, no
        clip, a scalar ``weight = 1 - alpha`` and ``pos_weight = alpha / (1 - alpha)`` (kept as 0-d marks until the class count is known:
        ``num_classes`` vectors are made on the first call).  ``alpha`` in (0, 1)."""
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 < float(alpha) < 1.0:
            raise ValueError(f"alpha must be in (0, 1), got {alpha!r}")
        self = cls(gamma_neg=gamma, gamma_pos=gamma, clip=0.0)
        self._alpha = float(alpha)
        return self

    def _scalars(self):
        return _gamma("gamma_pos", self.gamma_pos), _gamma("gamma_neg", self.gamma_neg), self._clip(self.clip)

    def _check_weight(self, C, device=None):
        alpha = getattr(self, "_alpha", None)
        if alpha is not None and self.weight is None and device is not None:       # sigmoid_focal: the two vectors, once the class count is known
            self.weight = torch.full((C,), 1.0 - alpha, dtype=torch.float32, device=device)
            self.pos_weight = torch.full((C,), alpha / (1.0 - alpha), dtype=torch.float32, device=device)
        for name in ("weight", "pos_weight"):
            v = getattr(self, name)
            if v is not None and v.shape[0] != C:
                raise ValueError(f"{name} has {v.shape[0]} entries but the logits have {C} classes")

    def _loss_call(self, target, B, C, device, logits=None):
        """(sigmoid_focal's two vectors are made here, on ``device``)"""
        if not _is_dense(target):
            raise TypeError("HybridAsymmetricLoss takes a floating target [B,C] (dense_target() makes one from class indices or a MixTarget)")
        _check_dense(target, B, C, logits)
        self._check_weight(C, device)
        return "asym", (target, self.weight, self.pos_weight, *self._scalars())

    def _captured(self):
        return [("gamma_pos / gamma_neg / clip", (self.gamma_pos, self.gamma_neg, self.clip)), _address("weight", self.weight),
                _address("pos_weight", self.pos_weight)]

    def extra_repr(self):
        return f"gamma_neg={self.gamma_neg}, gamma_pos={self.gamma_pos}, clip={self.clip}"


_DEFAULT_CRITERION = HybridCrossEntropyLoss()          # forward_temporal_loss(criterion=None)


class TransformerCNNHybrid(nn.Module, _ComputeDtypeMixin):
    """CNN backbone + temporal Transformer encoder over clips [B,T,3,H,W] (or [B,3,H,W] => T=1) -> logits [B,num_classes].

    Defaults are BASELINE config 2: cnn_channels (32,64,128,256) (the UNet(init_features=32) encoder widths,
    UNet.py:8-18), d_model 512, 8 heads, 2 layers, hidden 2048, 8 classes, dropout 0."""

    def __init__(self, in_channels=3, cnn_channels=(32, 64, 128, 256), d_model=512, num_heads=8, num_layers=2, hidden_dim=2048,
                 num_classes=8, dropout=0.0, compute_dtype="bf16"):
        super().__init__()
        chans = (in_channels,) + tuple(cnn_channels)
        if chans[-1] % 8 != 0:
            # the frame-token projection reads 16-byte rows of its [d_model, C] weight and of the pooled features
            raise ValueError(f"TransformerCNNHybrid on the MI355X HIP path needs cnn_channels[-1] to be a multiple of 8 (got {chans[-1]}); "
                             "there is no CPU fallback")
        self.num_stages = len(cnn_channels)
        cb, ct = split_compute_dtype(compute_dtype)
        for i in range(self.num_stages):
            setattr(self, f"encoder{i + 1}", ConvBNReLUPool(chans[i], chans[i + 1], f"enc{i + 1}", cb))
        self.in_channels = in_channels
        self.token_proj = nn.Linear(chans[-1], d_model)
        self.encoder = TransformerEncoder(d_model, hidden_dim, num_layers, num_heads, dropout, ct)
        self.head = nn.Linear(d_model, num_classes)
        self._dt, self._dt_t = ops.dtype_code(cb), ops.dtype_code(ct)            # conv stages / token projection + encoder + head
        self.fuse_model_ops = True        # hybrid::backbone + hybrid::temporal (one C call each way) instead of one operator per stage

    def set_compute_dtype(self, name):
        cb, ct = split_compute_dtype(name)
        for i in range(self.num_stages):
            getattr(self, f"encoder{i + 1}").set_compute_dtype(cb)
        self.encoder.set_compute_dtype(ct)
        self._dt, self._dt_t = ops.dtype_code(cb), ops.dtype_code(ct)
        return self

    def _temporal_dt(self):
        """dtype code of the fused temporal operators: bf16 conv stages in front of an fp32-storage temporal part hand their bf16 map over
        as it is (HYB_H_BF16: the global-average-pool kernels convert, no cast launches)."""
        if ops.torch_dtype(self._dt) == torch.bfloat16 and ops.torch_dtype(self._dt_t) == torch.float32:
            return self._dt_t | ops.HYB_H_BF16
        return self._dt_t

    def _to_temporal(self, h):
        """The last pooled map in the temporal part's storage type (unfused path / other pairs: a cast launch each way)."""
        tb, tt = ops.torch_dtype(self._dt), ops.torch_dtype(self._dt_t)
        if tb == tt:
            return h
        h32 = h if tb == torch.float32 else ops.to_f32(h, self._dt)
        return h32 if tt == torch.float32 else ops.to_compute(h32, self._dt_t)

    def _fused(self):
        """hybrid::backbone / hybrid::temporal apply when the model has the plain reference structure."""
        stages = [getattr(self, f"encoder{i + 1}") for i in range(self.num_stages)]
        bn0 = getattr(stages[0], stages[0]._norm)
        return (self.fuse_model_ops and self.in_channels <= 4 and self.encoder.num_layers > 0 and self.token_proj.bias is not None
                and self.head.bias is not None
                and all(getattr(s, s._norm).track_running_stats and getattr(s, s._norm).running_mean is not None
                        and getattr(s, s._norm).momentum == bn0.momentum and getattr(s, s._norm).eps == bn0.eps
                        and s.training == self.training for s in stages))

    def forward_backbone(self, x):
        """Clips [B,T,C,H,W] (or frames [B,C,H,W] => T=1) -> (last pooled map, NHWC compute dtype [B*T, H/2^S, W/2^S, Cp], B)."""
        if x.dim() == 4:
            x = x.unsqueeze(1)
        if x.dim() != 5:
            raise ValueError("expected a clip tensor [B,T,C,H,W] or a frame batch [B,C,H,W]")
        if not x.is_cuda:
            raise RuntimeError("TransformerCNNHybrid runs on the MI355X HIP path only: move the model and input to 'cuda' "
                               "(there is no CPU fallback)")
        B, T = x.shape[:2]
        f = x.reshape(B * T, *x.shape[2:]).float()                  # frames folded into the batch axis
        stages = [getattr(self, f"encoder{i + 1}") for i in range(self.num_stages)]
        if self._fused():
            # model-level operator: the same kernels as the stage operators below, chained in C (one call)
            return ops.backbone(f, [(getattr(s, s._conv).weight, getattr(s, s._norm)) for s in stages], self.training, self._dt), B
        commit = []                                                  # running-statistics write-back of all stages: one multi-tensor copy
        if self.in_channels <= 4:
            h = self.encoder1.forward_nhwc(f, True, commit)
        else:
            h = self.encoder1.forward_nhwc(ops.nchw_to_nhwc(f, self._dt, ops.pad_channels(self.in_channels)), False, commit)
        for i in range(1, self.num_stages):
            h = stages[i].forward_nhwc(h, False, commit)
        ops.commit_running_stats(commit)
        return h, B

    def forward_temporal(self, h, B, mask=None):
        """Last pooled map -> frame tokens -> temporal encoder -> head: logits [B, num_classes]."""
        enc = self.encoder
        if self._fused():
            tdt = self._temporal_dt()
            return ops.temporal(h if tdt & ops.HYB_H_BF16 else self._to_temporal(h), self.token_proj.weight, self.token_proj.bias, enc._flat_params(),
                                self.head.weight, self.head.bias, mask, B, tdt, enc.hidden_dim, enc.num_layers, enc.num_heads, enc.attention_layers[0]._attn_p(), float(enc.dropout),
                                ops.next_seed())
        h = self._to_temporal(h)
        tok = ops.token(h, self.token_proj.weight, self.token_proj.bias, self._dt_t).reshape(B, h.shape[0] // B, -1)
        return ops.head(enc.forward_compute(tok, mask), self.head.weight, self.head.bias, self._dt_t)

    def forward_temporal_loss(self, h, B, target, mask=None, criterion=None):
        """Last pooled map + class indices [B] -> (mean cross-entropy loss, logits): ``criterion(forward_temporal(h, B, mask), target)``
        with the loss inside the temporal part's own launches (hybrid::temporal_ce, or hybrid::temporal_ce_opts when the criterion carries
        options; same bits, same number of launches).  ``criterion``: a HybridCrossEntropyLoss, None = ``HybridCrossEntropyLoss()``.
        ``target`` may be a MixTarget: hybrid::temporal_ce_mix, again the same launches.  A floating ``target`` [B, num_classes] is a dense
        target: hybrid::temporal_ce_dense, the same launches, as soft-target cross-entropy under a HybridCrossEntropyLoss (or None) and as
        binary cross-entropy under a HybridBCEWithLogitsLoss, which takes nothing else.  Models ``_fused()`` rejects run the criterion behind
        forward_temporal.  A HybridFocalLoss (class indices) and a HybridAsymmetricLoss (a dense target) ride the same way:
        hybrid::temporal_ce_focal / hybrid::temporal_ce_asym.  Which operator, and its loss arguments: the criterion's ``_loss_call``."""
        criterion = _DEFAULT_CRITERION if criterion is None else criterion
        if type(criterion) not in (HybridCrossEntropyLoss, HybridBCEWithLogitsLoss, HybridFocalLoss, HybridAsymmetricLoss):
            raise TypeError("forward_temporal_loss fuses HybridCrossEntropyLoss, HybridBCEWithLogitsLoss, HybridFocalLoss and HybridAsymmetricLoss only")
        family, loss_args = criterion._loss_call(target, B, self.head.weight.shape[0], h.device)
        if not self._fused():              # (the call above then only refused a bad target early; the criterion makes its own behind the logits)
            logits = self.forward_temporal(h, B, mask)
            return criterion(logits, target), logits
        enc, tdt = self.encoder, self._temporal_dt()
        front = (h if tdt & ops.HYB_H_BF16 else self._to_temporal(h), self.token_proj.weight, self.token_proj.bias, enc._flat_params(),
                 self.head.weight, self.head.bias, mask)
        back = (B, tdt, enc.hidden_dim, enc.num_layers, enc.num_heads, enc.attention_layers[0]._attn_p(), float(enc.dropout), ops.next_seed())
        return ops.temporal_loss(front, family, loss_args, back)

    # ---- inference ------------------------------------------------------------------------------------------------------------------
    def _infer_fused(self):
        """hybrid::backbone_infer + hybrid::temporal serve the plain reference structure (what ``_fused()`` asks, minus the train/eval flags:
        inference never looks at them)."""
        stages = [getattr(self, f"encoder{i + 1}") for i in range(self.num_stages)]
        bn0 = getattr(stages[0], stages[0]._norm)
        return (self.fuse_model_ops and self.in_channels <= 4 and self.encoder.num_layers > 0 and self.token_proj.bias is not None
                and self.head.bias is not None
                and all(getattr(s, s._norm).track_running_stats and getattr(s, s._norm).running_mean is not None
                        and getattr(s, s._norm).eps == bn0.eps for s in stages))

    def _frames(self, x):
        if x.dim() == 4:
            x = x.unsqueeze(1)
        if x.dim() != 5:
            raise ValueError("expected a clip tensor [B,T,C,H,W] or a frame batch [B,C,H,W]")
        if not x.is_cuda:
            raise RuntimeError("TransformerCNNHybrid runs on the MI355X HIP path only: move the model and input to 'cuda' "
                               "(there is no CPU fallback)")
        B, T = x.shape[:2]
        return x.reshape(B * T, *x.shape[2:]).float(), B

    def _eval_forward(self, fn, *args):
        """fn(*args) with every submodule in eval mode; the flags are put back afterwards."""
        flags = [(m, m.training) for m in self.modules()]
        try:
            self.eval()
            return fn(*args)
        finally:
            for m, t in flags:
                m.training = t

    @torch.no_grad()
    def forward_backbone_infer(self, x):
        """forward_backbone for inference -> (last pooled map, B): BatchNorm from the running statistics whatever ``self.training`` says,
        nothing kept for a backward, one workspace instead of per-stage buffers, and in bf16 no full-resolution conv output (the conv
        kernels of stages 2.. apply BatchNorm + ReLU + MaxPool in their epilogue).  Models ``_infer_fused()`` rejects take forward_backbone."""
        if not self._infer_fused():
            return self._eval_forward(self.forward_backbone, x)
        f, B = self._frames(x)
        stages = [getattr(self, f"encoder{i + 1}") for i in range(self.num_stages)]
        return ops.backbone_infer(f, [(getattr(s, s._conv).weight, getattr(s, s._norm)) for s in stages], self._dt), B

    @torch.no_grad()
    def predict(self, x, mask=None):
        """Logits [B, num_classes] for inference: what ``model.eval()(x, mask)`` returns under ``torch.no_grad()`` (bf16 conv stages: up to one
        rounding fewer per stage), without looking at or changing ``self.training``: BatchNorm running statistics, attention-weight dropout
        off (quirk Q5), the per-layer dropout as the eval forward applies it (quirk Q6)."""
        if not self._infer_fused():
            return self._eval_forward(self.forward, x, mask)
        h, B = self.forward_backbone_infer(x)
        enc = self.encoder
        tdt = self._temporal_dt()
        return ops.temporal(h if tdt & ops.HYB_H_BF16 else self._to_temporal(h), self.token_proj.weight, self.token_proj.bias, enc._flat_params(),
                            self.head.weight, self.head.bias, mask, B, tdt, enc.hidden_dim, enc.num_layers, enc.num_heads, 0.0, float(enc.dropout),
                            ops.next_seed())

    @torch.no_grad()
    def evaluate(self, x, y, meter, mask=None, views=1):
        """``predict(x, mask)`` followed by ``meter.update(logits, y, views)`` (meter.ClassificationMeter): one more launch behind the forward,
        no synchronisation.  x [B * views, T, 3, H, W] with the views of one video adjacent, y int64 [B]; returns the logits [B * views, C].
        With a meter.MultiLabelMeter y is the fp32 multi-hot target [B, C] and the launch is hyb_eval_multilabel."""
        logits = self.predict(x, mask)
        meter.update(logits, y, views)
        return logits

    def backbone_parameters(self):
        return [p for i in range(self.num_stages) for p in getattr(self, f"encoder{i + 1}").parameters()]

    def temporal_parameters(self):
        return list(self.token_proj.parameters()) + list(self.encoder.parameters()) + list(self.head.parameters())

    def param_groups(self, lr=1e-3, weight_decay=1e-2, layer_decay=1.0, no_decay_1d=True):
        """The usual fine-tuning recipe as a list of parameter-group dicts for HybridAdamW (which serves them all from one AdamW launch,
        merge_groups) or torch.optim.AdamW: no weight decay on biases, BatchNorm and LayerNorm parameters (`no_decay_1d`: every parameter
        with ndim <= 1 gets weight_decay 0.0), and a learning rate that decays layer by layer towards the input,
            lr * layer_decay ** (D - depth)
        with depth i for conv stage encoder{i+1} (i = 0 .. S - 1), S for token_proj, S + 1 + l for encoder layer l (its attention,
        feed-forward and LayerNorm) and D = S + 1 + L for the head, which trains at `lr`.  Every trainable parameter is in exactly one
        group, in depth order; empty groups are dropped; layer_decay=1.0 merges the depths, so the defaults give two groups and
        no_decay_1d=False then one.  Each group also carries "name" ("stage1.decay", "layer0.no_decay", ...) and "lr_scale" (its factor of
        `lr`, for schedulers that set lr = base * lr_scale themselves); "lr" itself is set, so a torch scheduler's initial_lr is right."""
        if lr < 0.0 or weight_decay < 0.0 or not 0.0 < layer_decay <= 1.0:
            raise ValueError("param_groups: lr >= 0, weight_decay >= 0 and 0 < layer_decay <= 1")
        S, L = self.num_stages, self.encoder.num_layers
        depths = [(f"stage{i + 1}", [getattr(self, f"encoder{i + 1}")]) for i in range(S)] + [("token_proj", [self.token_proj])]
        depths += [(f"layer{l}", [self.encoder.attention_layers[l], self.encoder.feedforward_layers[l], self.encoder.layer_norm[l]]) for l in range(L)]
        depths.append(("head", [self.head]))
        D = len(depths) - 1
        groups, seen = {}, set()
        for depth, (name, mods) in enumerate(depths):
            scale = float(layer_decay) ** (D - depth)
            for p in (p for m in mods for p in m.parameters()):
                if not p.requires_grad or id(p) in seen:
                    continue
                seen.add(id(p))
                no_decay = no_decay_1d and p.ndim <= 1
                # one learning rate for all depths: the depth is no part of the key, and the groups are named after what tells them apart
                key = (depth if layer_decay != 1.0 else 0, no_decay)
                if key not in groups:
                    kind = ("no_decay" if no_decay else "decay") if no_decay_1d else None
                    label = ".".join(s for s in (name if layer_decay != 1.0 else None, kind) if s) or "all"
                    groups[key] = {"params": [], "lr": lr * scale, "weight_decay": 0.0 if no_decay else weight_decay, "name": label, "lr_scale": scale}
                groups[key]["params"].append(p)
        if len(seen) != sum(1 for p in self.parameters() if p.requires_grad):
            raise RuntimeError("model has trainable parameters outside its conv stages, token projection, encoder layers and head")
        return [groups[k] for k in sorted(groups)]

    def forward(self, x, mask=None):
        h, B = self.forward_backbone(x)
        return self.forward_temporal(h, B, mask)
