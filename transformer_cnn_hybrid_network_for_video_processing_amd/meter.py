"""Evaluation on the device: an accumulating classification meter whose update is ONE HIP launch behind the logits.

``ClassificationMeter.update(logits, target, views)`` adds one batch into three device tensors -- the loss numerator and denominator
(float64 [2]), five counters (int64 [5]: videos seen, kept, top-1 correct, top-k correct, rows with a NaN score) and, optionally, the
confusion matrix (int64 [C, C], row = target, column = prediction) -- through ``hybrid::eval_metrics_`` (hyb_eval_metrics,
include/hybrid_hip.h).  It never synchronises and can be captured into a prediction graph (graph.GraphedEval); the host reads the numbers
once, in ``compute()``.  The loss is the arithmetic of HybridCrossEntropyLoss -- the same device functions, the same class weights,
``ignore_index`` and label smoothing -- so a validation loss compares exactly with the training loss.  With ``views = V > 1`` a video's
score is the mean of the softmax of its V views (temporal clips x spatial crops), the standard multi-view protocol.
The same holds for every criterion the library trains with: a HybridFocalLoss gives the focal validation loss (``hybrid::eval_metrics_focal_``),
a floating [B, C] target the soft-target cross-entropy (``hybrid::eval_metrics_soft_``), and MultiLabelMeter takes a HybridAsymmetricLoss
(``hybrid::eval_multilabel_asym_``).  Each is the same launch with another loss term; everything but the loss sums is computed alike.

Ties are settled by the library's own rule: the prediction is the lowest index among the maxima, and the target's rank counts the classes
that score higher plus the lower-indexed classes that score the same.

``MultiLabelMeter`` is the meter of multi-hot targets (fp32 [B, C]): the same one-launch update through ``hybrid::eval_multilabel_``
(hyb_eval_multilabel), the BCE loss of HybridBCEWithLogitsLoss, per-class tp / fp / fn, and a bank of scores on the device from which
``compute()`` forms the exact average precision."""
import torch

from . import ops
from .modules import HybridAsymmetricLoss, HybridBCEWithLogitsLoss, HybridCrossEntropyLoss, HybridFocalLoss, MixTarget, _gamma, _is_dense


class ClassificationMeter:
    def __init__(self, num_classes, topk=5, confusion=True, criterion=None, device="cuda"):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1:
            raise ValueError(f"num_classes must be an int >= 1, got {num_classes!r}")
        if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= num_classes:
            raise ValueError(f"topk must be an int in [1, num_classes = {num_classes}], got {topk!r}")
        if criterion is not None and not isinstance(criterion, (HybridCrossEntropyLoss, HybridFocalLoss)):
            raise TypeError(f"criterion must be a HybridCrossEntropyLoss, a HybridFocalLoss or None, got {type(criterion).__name__}")
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
        when the launch runs), the other two by value.  Under a HybridFocalLoss the fourth entry is its gamma."""
        c = self.criterion
        if c is None:
            return None, 0, False, 0.0
        if isinstance(c, HybridFocalLoss):                                          # (its fourth scalar is gamma: it has no label smoothing)
            return c.weight, *ops.ignore_args(c.ignore_index), _gamma("gamma", c.gamma)
        return c.weight, 0 if c.ignore_index is None else int(c.ignore_index), c.ignore_index is not None, float(c.label_smoothing)

    def _operator(self, target):
        """Which update launch this target takes under this criterion, after the refusals the criteria themselves make: a floating [B, C]
        target is a row of class probabilities per video (None or a HybridCrossEntropyLoss without ignore_index), class indices go to the
        criterion's own launch.  The scalars are read from the criterion here, at every update, and validated as its own call does."""
        c = self.criterion
        if isinstance(target, MixTarget):
            raise TypeError("ClassificationMeter.update takes class indices int64 [B] or a soft target fp32 [B, C], not a MixTarget: "
                            "validation batches are not mixed")
        if _is_dense(target):
            if isinstance(c, HybridFocalLoss):
                c._check_target(target)                                            # TypeError: focal takes class indices
            if c is not None:
                c._refuse_ignore_index()                                           # ValueError, as the criterion itself
            weight, _, _, smoothing = self.loss_options()
            if not 0.0 <= smoothing <= 1.0:
                raise ValueError(f"label_smoothing must be in [0, 1], got {smoothing}")
            return torch.ops.hybrid.eval_metrics_soft_, (weight, smoothing)
        op = torch.ops.hybrid.eval_metrics_focal_ if isinstance(c, HybridFocalLoss) else torch.ops.hybrid.eval_metrics_
        return op, self.loss_options()

    def update(self, logits, target, views=1):
        """Add one batch: logits fp32 [B * views, C] contiguous (the views of one video adjacent: row b * views + v), target int64 [B], both on
        the meter's device.  One launch, no synchronisation.  Returns pred (int64 [B]; -1 for a video whose scores hold a NaN), or
        (pred, scores) when views > 1 (scores fp32 [B, C]: the mean of the views' softmax).
        A floating target fp32 [B, C] is a row of class probabilities per video (a teacher's soft targets): the loss is the criterion's
        soft-target cross-entropy (criterion None or a HybridCrossEntropyLoss; an ``ignore_index`` raises ValueError as the criterion does, a
        HybridFocalLoss raises TypeError), every video is kept, and its label for the accuracies and the confusion matrix is the lowest
        index among its row's maxima.  A MixTarget raises TypeError: validation batches are not mixed."""
        if isinstance(views, bool) or not isinstance(views, int) or views < 1:
            raise ValueError(f"views must be an int >= 1, got {views!r}")
        op, loss_args = self._operator(target)
        ops._require_cuda(logits, target, *self._state())
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"expected logits [B * views, {self.num_classes}], got {tuple(logits.shape)}")
        pred, scores = op(logits, target, *loss_args, self.topk, views, self.sums, self.counts, self.confusion)
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


def average_precision(scores, labels, valid=None):
    """Exact average precision per class (scikit-learn's definition) of scores [N, C] against 0 / 1 labels [N, C], in float64 on the
    inputs' device: for class c the distinct score values in descending order are the thresholds tau, P(tau) = TP(>= tau) / N(>= tau),
    R(tau) = TP(>= tau) / P_c, AP_c = sum_tau (R(tau) - R(previous tau)) P(tau).  Tied scores form ONE step, so the value depends neither
    on the order of tied rows nor on the order of the rows at all.  NaN for a class without a positive label.  ``valid`` (bool [N], a
    device tensor: no host read) leaves rows out: they weigh nothing in TP and N wherever they sort.  -> float64 [C]."""
    s = scores.to(torch.float64)
    N, C = s.shape
    w = torch.ones(N, 1, dtype=torch.float64, device=s.device) if valid is None else valid.to(torch.float64).reshape(N, 1)
    if N == 0:
        return torch.full((C,), float("nan"), dtype=torch.float64, device=s.device)
    s = torch.where(w > 0, s, torch.full_like(s, float("-inf")))
    vals, idx = s.sort(dim=0, descending=True)
    tp = torch.cumsum(torch.gather(labels.to(torch.float64) * w, 0, idx), 0)      # sums of 0 / 1: exact
    n = torch.cumsum(torch.gather(w.expand(N, C), 0, idx), 0)
    last = torch.ones_like(vals, dtype=torch.bool)                                 # the last row of every run of equal scores
    last[:-1] = vals[:-1] != vals[1:]
    ends = torch.where(last, tp, torch.zeros_like(tp))
    prev = torch.cat([torch.zeros(1, C, dtype=torch.float64, device=s.device), torch.cummax(ends, 0).values[:-1]])   # TP at the previous step
    step = torch.where(last, tp - prev, torch.zeros_like(tp))
    pos = tp[-1]
    ap = torch.where(step > 0, step * tp / n.clamp(min=1.0), torch.zeros_like(tp)).sum(0) / pos
    return torch.where(pos > 0, ap, torch.full_like(ap, float("nan")))


class MultiLabelMeter:
    """The meter of multi-label clips: ``update(logits, target, views)`` adds one batch through ``hybrid::eval_multilabel_``
    (hyb_eval_multilabel, include/hybrid_hip.h) -- ONE launch behind the logits, no synchronisation, capturable (graph.GraphedEval) -- into
    the loss numerator (float64 [1]), five counters (int64 [5]: videos seen, videos with a NaN score, exact matches, rows stored in the bank,
    rows dropped) and the per-class cells (int64 [C, 3]: tp, fp, fn), and appends the video's scores and labels to a bank of ``capacity``
    rows on the device, from which ``compute()`` forms the exact per-class average precision and mAP.

    ``target`` is fp32 [B, C], a label is t >= 0.5; a score is the sigmoid of the logit (the mean over the views' sigmoids with views > 1)
    and a class is predicted when its score reaches its threshold.  ``threshold``: a float or C of them in (0, 1), kept as an fp32 [C]
    device buffer that the launch reads when it runs (an in-place update reaches the next update and the next replay).  ``criterion``: None
    a HybridBCEWithLogitsLoss or a HybridAsymmetricLoss (``sigmoid_focal(...)`` included), whose ``weight`` and ``pos_weight`` buffers are
    read the same way; the loss is that criterion's arithmetic.  The asymmetric loss's exponents and ``clip`` are read at every update.
    ``capacity``: the videos whose scores are kept; 0 = no bank and no AP.  Videos beyond it are counted as dropped, and AP is then NaN."""

    def __init__(self, num_classes, threshold=0.5, criterion=None, capacity=0, device="cuda"):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1:
            raise ValueError(f"num_classes must be an int >= 1, got {num_classes!r}")
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 0:
            raise ValueError(f"capacity must be an int >= 0, got {capacity!r}")
        if criterion is not None and not isinstance(criterion, (HybridBCEWithLogitsLoss, HybridAsymmetricLoss)):
            raise TypeError(f"criterion must be a HybridBCEWithLogitsLoss, a HybridAsymmetricLoss or None, got {type(criterion).__name__}")
        if isinstance(criterion, HybridAsymmetricLoss) and criterion.weight is None and criterion.pos_weight is None:
            criterion._check_weight(num_classes, torch.device(device))             # sigmoid_focal: its two vectors, now that the class count is known
        for name in ("weight", "pos_weight"):
            v = None if criterion is None else getattr(criterion, name)
            if v is not None and v.shape[0] != num_classes:
                raise ValueError(f"the criterion's {name} has {v.shape[0]} entries but the meter has {num_classes} classes")
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, list, tuple, torch.Tensor)):
            raise TypeError(f"threshold must be a float or a sequence / tensor of num_classes floats, got {type(threshold).__name__}")
        thr = torch.as_tensor(threshold, dtype=torch.float32).detach().cpu()
        if thr.dim() == 0:
            thr = thr.repeat(num_classes)
        if thr.dim() != 1 or thr.shape[0] != num_classes:
            raise ValueError(f"threshold must be one float or {num_classes} of them, got shape {tuple(thr.shape)}")
        if not bool(((thr > 0) & (thr < 1)).all()):
            raise ValueError(f"every threshold must lie in (0, 1), got {thr.tolist()}")
        device = torch.device(device)
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("MultiLabelMeter: the meter's state cannot be created under stream capture (it must be zero before the first "
                               "update, and a buffer born in a capture is zeroed by that graph only) -- construct the meter before capturing")
        self.num_classes, self.criterion, self.capacity = num_classes, criterion, capacity
        self.threshold = thr.to(device).contiguous()
        # created and zeroed eagerly; update() adds into them in place, so they keep their addresses for the life of the meter
        self.sums = torch.zeros(1, dtype=torch.float64, device=device)
        self.counts = torch.zeros(5, dtype=torch.int64, device=device)
        self.cells = torch.zeros(num_classes, 3, dtype=torch.int64, device=device)
        self.bank_scores = torch.zeros(capacity, num_classes, dtype=torch.float32, device=device) if capacity else None
        self.bank_labels = torch.zeros(capacity, num_classes, dtype=torch.uint8, device=device) if capacity else None

    def _state(self):
        return [self.sums, self.counts, self.cells]

    def loss_options(self):
        """(weight buffer or None, pos_weight buffer or None), both read by address when the launch runs."""
        c = self.criterion
        return (None, None) if c is None else (c.weight, c.pos_weight)

    def update(self, logits, target, views=1):
        """Add one batch: logits fp32 [B * views, C] contiguous (the views of one video adjacent: row b * views + v), target fp32 [B, C], both
        on the meter's device.  One launch, no synchronisation.  Returns (pred uint8 [B, C], scores fp32 [B, C])."""
        if isinstance(views, bool) or not isinstance(views, int) or views < 1:
            raise ValueError(f"views must be an int >= 1, got {views!r}")
        # the asymmetric loss's exponents and clip: read from the criterion at every update and validated as its own call validates them
        scalars = self.criterion._scalars() if isinstance(self.criterion, HybridAsymmetricLoss) else None
        ops._require_cuda(logits, target, *self._state())
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"expected logits [B * views, {self.num_classes}], got {tuple(logits.shape)}")
        weight, pos_weight = self.loss_options()
        if scalars is not None:
            return torch.ops.hybrid.eval_multilabel_asym_(logits, target, weight, pos_weight, *scalars, self.threshold, views, self.sums,
                                                          self.counts, self.cells, self.bank_scores, self.bank_labels)
        return torch.ops.hybrid.eval_multilabel_(logits, target, weight, pos_weight, self.threshold, views, self.sums, self.counts, self.cells,
                                                 self.bank_scores, self.bank_labels)

    def reset(self):
        """Zero the state in place, the bank's cursor included (the bank's rows stay: nothing reads beyond the cursor).  Eager only: a
        captured reset would run again at every replay."""
        if self.sums.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("MultiLabelMeter.reset() under stream capture: it would zero the meter at every replay -- reset it eagerly")
        for t in self._state():
            t.zero_()

    def compute(self):
        """The numbers so far, after ONE device-to-host copy (this is where the host waits).  loss = sums[0] / (videos C); videos, nan_rows,
        stored, dropped; exact_match; hamming_accuracy = 1 - sum(fp + fn) / (videos C); support = tp + fn per class; per_class_precision /
        recall / f1 (NaN where the denominator is 0); micro_precision / recall / f1; macro_f1 over the classes with support > 0; with a
        bank per_class_ap and mAP (average_precision() above on the stored rows; NaN for a class without a stored positive, mAP over the
        others; all NaN when rows were dropped: a partial bank gives no silent answer).  Nothing seen: NaN."""
        C = self.num_classes
        parts = [t.reshape(-1).to(torch.float64) for t in self._state()]               # (counts below 2^53 are exact in float64)
        if self.bank_scores is not None:
            valid = torch.arange(self.capacity, device=self.counts.device) < self.counts[3]
            parts.append(average_precision(self.bank_scores, self.bank_labels, valid))
        flat = torch.cat(parts).cpu()
        num = float(flat[0])
        videos, nan_rows, exact, stored, dropped = (int(v) for v in flat[1:6].tolist())
        cells = flat[6:6 + 3 * C].reshape(C, 3)
        tp, fp, fn = cells[:, 0], cells[:, 1], cells[:, 2]
        nan = float("nan")

        def ratio(a, b):
            return torch.where(b > 0, a / b.clamp(min=1.0), torch.full_like(b, nan))

        def scalar(a, b):
            return float(a) / float(b) if float(b) > 0 else nan
        support = tp + fn
        f1 = ratio(2 * tp, 2 * tp + fp + fn)
        seen = support > 0
        out = {"loss": num / (videos * C) if videos else nan, "videos": videos, "nan_rows": nan_rows, "stored": stored, "dropped": dropped,
               "exact_match": exact / videos if videos else nan,
               "hamming_accuracy": 1.0 - float((fp + fn).sum()) / (videos * C) if videos else nan,
               "support": [int(v) for v in support.tolist()],
               "per_class_precision": ratio(tp, tp + fp).tolist(), "per_class_recall": ratio(tp, support).tolist(), "per_class_f1": f1.tolist(),
               "micro_precision": scalar(tp.sum(), (tp + fp).sum()), "micro_recall": scalar(tp.sum(), support.sum()),
               "micro_f1": scalar(2 * tp.sum(), (2 * tp + fp + fn).sum()),
               "macro_f1": float(f1[seen].mean()) if bool(seen.any()) else nan}
        if self.bank_scores is not None:
            ap = flat[6 + 3 * C:]
            if dropped > 0:
                ap = torch.full_like(ap, nan)
            have = ~torch.isnan(ap)
            out["per_class_ap"] = ap.tolist()
            out["mAP"] = float(ap[have].mean()) if bool(have.any()) else nan
        return out

    def _check_peer(self, other):
        if not isinstance(other, MultiLabelMeter):
            raise TypeError("merge() takes another MultiLabelMeter")
        if other.num_classes != self.num_classes or (other.bank_scores is None) != (self.bank_scores is None):
            raise ValueError("merge(): the meters differ in num_classes or in keeping a score bank")

    def _append(self, scores, labels, n):
        """Append the first n rows of another bank behind the cursor (host-side bookkeeping: reads the cursor); the rows that do not fit are
        counted as dropped."""
        mine = int(self.counts[3])
        take = max(0, min(n, self.capacity - mine))
        if take:
            self.bank_scores[mine:mine + take].copy_(scores[:take])
            self.bank_labels[mine:mine + take].copy_(labels[:take])
        self.counts[3] = mine + take
        self.counts[4] += n - take

    def merge(self, other):
        """Add another meter's state into this one (plain torch adds; the other meter is left as it is) and append its stored rows behind
        this meter's; rows beyond ``capacity`` are counted as dropped."""
        self._check_peer(other)
        theirs = other.counts.to(self.counts.device)
        self.sums.add_(other.sums.to(self.sums.device))
        self.cells.add_(other.cells.to(self.cells.device))
        self.counts[:3] += theirs[:3]
        self.counts[4] += theirs[4]
        if self.bank_scores is not None:
            self._append(other.bank_scores.to(self.bank_scores.device), other.bank_labels.to(self.bank_labels.device), int(theirs[3]))
        return self

    def all_reduce(self, group=None):
        """Combine the ranks of `group` (torch.distributed, any backend): sums, cells and the counters are summed; the banks are gathered, and
        every rank ends with the stored rows of rank 0, 1, .. in that order, truncated at ``capacity`` (the excess counted as dropped).
        Every rank must have the same ``capacity``."""
        import torch.distributed as dist
        world = dist.get_world_size(group)
        mine = torch.stack([self.counts[3], torch.tensor(self.capacity, dtype=torch.int64, device=self.counts.device)])
        info = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(info, mine, group=group)
        info = torch.stack(info).cpu()
        if any(int(c) != self.capacity for c in info[:, 1]):
            raise ValueError(f"all_reduce(): every rank needs the same capacity, got {info[:, 1].tolist()}")
        totals = self.counts.clone()
        totals[3] = 0                                                               # the cursor is not a sum
        for t in (self.sums, self.cells, totals):
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        self.counts.copy_(totals)
        if self.bank_scores is not None:
            all_scores = [torch.empty_like(self.bank_scores) for _ in range(world)]
            all_labels = [torch.empty_like(self.bank_labels) for _ in range(world)]
            dist.all_gather(all_scores, self.bank_scores, group=group)
            dist.all_gather(all_labels, self.bank_labels, group=group)
            for r in range(world):                                                  # counts[3] starts at 0: rank 0's rows first
                self._append(all_scores[r], all_labels[r], int(info[r, 0]))
        return self

    def __repr__(self):
        return f"MultiLabelMeter(num_classes={self.num_classes}, capacity={self.capacity}, criterion={self.criterion!r})"
