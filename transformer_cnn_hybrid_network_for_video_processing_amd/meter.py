"""Evaluation on the device: an accumulating classification meter whose update is ONE HIP launch behind the logits.

``ClassificationMeter.update(logits, target, views)`` adds one batch into three device tensors -- the loss numerator and denominator
(float64 [2]), five counters (int64 [5]: videos seen, kept, top-1 correct, top-k correct, rows with a NaN score) and, optionally, the
confusion matrix (int64 [C, C], row = target, column = prediction) -- through ``hybrid::eval_metrics_`` (hyb_eval_metrics,
include/hybrid_hip.h).  It never synchronises and can be captured into a prediction graph (graph.GraphedEval); the host reads the numbers
once, in ``compute()``.  The loss is the arithmetic of HybridCrossEntropyLoss -- the same device functions, the same class weights,
``ignore_index`` and label smoothing -- so a validation loss compares exactly with the training loss.  With ``views = V > 1`` a video's
score is the mean of the softmax of its V views (temporal clips x spatial crops), the standard multi-view protocol.

Ties are settled by the library's own rule: the prediction is the lowest index among the maxima, and the target's rank counts the classes
that score higher plus the lower-indexed classes that score the same."""
import torch

from . import ops
from .modules import HybridCrossEntropyLoss


class ClassificationMeter:
    def __init__(self, num_classes, topk=5, confusion=True, criterion=None, device="cuda"):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1:
            raise ValueError(f"num_classes must be an int >= 1, got {num_classes!r}")
        if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= num_classes:
            raise ValueError(f"topk must be an int in [1, num_classes = {num_classes}], got {topk!r}")
        if criterion is not None and not isinstance(criterion, HybridCrossEntropyLoss):
            raise TypeError(f"criterion must be a HybridCrossEntropyLoss or None, got {type(criterion).__name__}")
        if criterion is not None and criterion.weight is not None and criterion.weight.shape[0] != num_classes:
            raise ValueError(f"the criterion's weight has {criterion.weight.shape[0]} entries but the meter has {num_classes} classes")
        device = torch.device(device)
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ClassificationMeter: the meter's state cannot be created under stream capture (it must be zero before the first "
                               "update, and a buffer born in a capture is zeroed by that graph only) -- construct the meter before capturing")
        self.num_classes, self.topk, self.criterion = num_classes, topk, criterion
        # created and zeroed eagerly; update() adds into them in place, so they keep their addresses for the life of the meter
        self.sums = torch.zeros(2, dtype=torch.float64, device=device)
        self.counts = torch.zeros(5, dtype=torch.int64, device=device)
        self.confusion = torch.zeros(num_classes, num_classes, dtype=torch.int64, device=device) if confusion else None

    def _state(self):
        return [t for t in (self.sums, self.counts, self.confusion) if t is not None]

    def loss_options(self):
        """(weight buffer or None, ignore_index, has_ignore, label_smoothing) as the update launch takes them: the weight by address (read
        when the launch runs), the other two by value."""
        c = self.criterion
        if c is None:
            return None, 0, False, 0.0
        return c.weight, 0 if c.ignore_index is None else int(c.ignore_index), c.ignore_index is not None, float(c.label_smoothing)

    def update(self, logits, target, views=1):
        """Add one batch: logits fp32 [B * views, C] contiguous (the views of one video adjacent: row b * views + v), target int64 [B], both on
        the meter's device.  One launch, no synchronisation.  Returns pred (int64 [B]; -1 for a video whose scores hold a NaN), or
        (pred, scores) when views > 1 (scores fp32 [B, C]: the mean of the views' softmax)."""
        if isinstance(views, bool) or not isinstance(views, int) or views < 1:
            raise ValueError(f"views must be an int >= 1, got {views!r}")
        ops._require_cuda(logits, target, *self._state())
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"expected logits [B * views, {self.num_classes}], got {tuple(logits.shape)}")
        weight, ignore_index, has_ignore, smoothing = self.loss_options()
        pred, scores = torch.ops.hybrid.eval_metrics_(logits, target, weight, ignore_index, has_ignore, smoothing, self.topk, views, self.sums,
                                                      self.counts, self.confusion)
        return (pred, scores) if views > 1 else pred

    def reset(self):
        """Zero the state in place.  Eager only: a captured reset would run again at every replay."""
        if self.sums.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ClassificationMeter.reset() under stream capture: it would zero the meter at every replay -- reset it eagerly")
        for t in self._state():
            t.zero_()

    def compute(self):
        """The numbers so far, after ONE device-to-host copy (this is where the host waits): loss = numerator / denominator, top1 and topk
        over the kept videos, videos, kept, nan_rows, and with a confusion matrix per_class_recall (NaN for a class never seen as a target)
        and mean_class_accuracy (over the classes seen).  Nothing kept: NaN loss and NaN accuracies."""
        flat = torch.cat([t.reshape(-1).to(torch.float64) for t in self._state()]).cpu()       # (counts below 2^53 are exact in float64)
        num, den = float(flat[0]), float(flat[1])
        videos, kept, top1, topk, nan_rows = (int(v) for v in flat[2:7].tolist())
        nan = float("nan")
        out = {"loss": num / den if den != 0.0 else nan, "top1": top1 / kept if kept else nan, "topk": topk / kept if kept else nan,
               "videos": videos, "kept": kept, "nan_rows": nan_rows}
        if self.confusion is not None:
            conf = flat[7:].reshape(self.num_classes, self.num_classes)
            rows = conf.sum(1)
            recall = torch.where(rows > 0, conf.diagonal() / rows.clamp(min=1.0), torch.full_like(rows, nan))
            seen = rows > 0
            out["per_class_recall"] = recall.tolist()
            out["mean_class_accuracy"] = float(recall[seen].mean()) if bool(seen.any()) else nan
        return out

    def _check_peer(self, other):
        if not isinstance(other, ClassificationMeter):
            raise TypeError("merge() takes another ClassificationMeter")
        if other.num_classes != self.num_classes or other.topk != self.topk or (other.confusion is None) != (self.confusion is None):
            raise ValueError("merge(): the meters differ in num_classes, topk or in keeping a confusion matrix")

    def merge(self, other):
        """Add another meter's state into this one (plain torch adds; the other meter is left as it is)."""
        self._check_peer(other)
        for mine, theirs in zip(self._state(), other._state()):
            mine.add_(theirs.to(mine.device))
        return self

    def all_reduce(self, group=None):
        """Sum the state over the ranks of `group` (torch.distributed, any backend): every rank ends with the totals."""
        import torch.distributed as dist
        for t in self._state():
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return self

    def __repr__(self):
        return (f"ClassificationMeter(num_classes={self.num_classes}, topk={self.topk}, confusion={self.confusion is not None}, "
                f"criterion={self.criterion!r})")
