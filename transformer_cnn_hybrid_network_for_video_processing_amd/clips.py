"""Clip input pipeline: the step before the hot path once synthetic data is replaced.

The reference's clip loader exists only as bytecode (``__pycache__/dataset.cpython-38.pyc``: ``CSVDataset.__getitem__`` src
L106-113 turns one CSV row of T frame paths into a list of T ``[3,S,S]`` tensors, ``DataloaderSequential.load_images`` src
L124-127 batches them with ``shuffle=True``, i.e. a T-major list of ``[B,3,S,S]``); its source analogue for single images is
``Dataloader.py:8-46`` (pandas CSV -> ``PIL.Image.open`` -> ``Resize`` -> ``ToTensor``).  torchvision and cv2 are not part of
this image, so the decode/resize leg below uses PIL directly and is "parity unpinned" against those libraries' resamplers; what IS
pinned is ``ToTensor`` (uint8 HWC -> float CHW / 255), done here on the GPU after the PCIe copy.

What is MI355X-specific: frames cross PCIe as uint8 from pinned host memory (19 MB instead of 77 MB per config-2 batch: ~0.3 ms
instead of ~1.2 ms on a 63 GB/s link, against a ~1.6 ms training step), on a dedicated copy stream, two batches deep, and are
expanded to the fp32 ``[B,T,3,H,W]`` clip tensor by ``hyb_frames_u8hwc_to_f32chw`` on that stream -- the training stream only
waits on an event.  No CPU fallback for the device leg.

Augmentation (``ClipTransform``): crop, bilinear resize, horizontal flip, temporal sub-sampling and mean/std normalisation happen in
that same expansion pass (``hyb_clips_u8_transform``), from ONE int32 parameter row per clip drawn on the host -- every frame of a
clip gets the same crop and flip, which per-image host transforms get wrong by default -- so the host never touches a pixel.
Mixup and CutMix (``ClipTransform(mixup_alpha=..., cutmix_alpha=...)``) ride in that pass too (``hyb_clips_u8_transform_mix``): one more
int32 row per clip names its partner and lam or the box, the labels come out as a ``MixTarget`` for the fused two-target loss.
Colour jitter, grayscale, Gaussian noise and random erasing (``ClipTransform(brightness=..., noise_std=..., erase_prob=...)``) are arithmetic on
the value that pass already holds in a register (``hyb_clips_u8_transform_photo``): a third int32 row per clip, no further pass over the clip.
Multi-view evaluation (``ClipTransform(train=False, eval_views=(K, S), eval_crop=..., eval_flip=...)``): K temporal windows x S spatial crops of
every clip come out of ONE launch (``hyb_clips_u8_transform_views``) that reads each source clip in place, V parameter rows per clip -- the bytes
cross PCIe once, and the rows are in the order ``ClassificationMeter.update(..., views=V)`` scores.
The antialiased resize (``ClipTransform(antialias=True)``, ``hyb_clips_u8_transform_aa``): the same rows, training or evaluation, resampled with
torchvision's ``Resize(antialias=True)`` filter -- a separable triangle filter through LDS instead of two taps per axis.
RandAugment and hue jitter (``ClipTransform(randaugment="rand-m7-n4-mstd0.5", hue=0.1)``, ``hyb_clip_aug_u8_transform``): a fourth int32 row per clip
carries the drawn geometric ops folded into ONE affine map, which the kernel composes with the crop's resampling (one gather, not a second
resampling), and the drawn photometric ops as a program of pointwise steps in front of the jitter.
"""
import csv
import os

import numpy as np
import torch

from ._lib import lib
from .modules import MixTarget
from .ops import clip_transform_into


class ClipCSVDataset(torch.utils.data.Dataset):
    """One CSV row = the T frame paths of a clip (dataset.pyc src L86-113; column layout of Datasets/generateDataset.py:4-25: one
    path per cell, no header).  ``__getitem__`` -> (uint8 array [T, size, size, 3], label) -- decoded and resized on the host."""

    def __init__(self, csv_path, size=224, labels=None, root=None):
        with open(csv_path, newline="") as f:
            self.rows = [[c for c in row if c] for row in csv.reader(f) if row]
        if not self.rows:
            raise ValueError(f"{csv_path} holds no clips")
        t = {len(r) for r in self.rows}
        if len(t) != 1:
            raise ValueError(f"clips of different lengths in {csv_path}: {sorted(t)}")
        self.size, self.labels, self.root = int(size), labels, root

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, i):
        from PIL import Image
        frames = []
        for p in self.rows[i]:
            with Image.open(os.path.join(self.root, p) if self.root else p) as im:
                frames.append(np.asarray(im.convert("RGB").resize((self.size, self.size), Image.BILINEAR), dtype=np.uint8))
        return np.stack(frames), (0 if self.labels is None else int(self.labels[i]))


class SyntheticClipSource:
    """Endless seeded uint8 clip batches [B,T,H,W,3] + labels [B] (BASELINE's synthetic data, in the form a decoder produces)."""

    def __init__(self, batch, frames, size, num_classes=8, seed=0, distinct=4):
        g = np.random.default_rng(seed)
        self.batches = [(g.integers(0, 256, (batch, frames, size, size, 3), dtype=np.uint8), g.integers(0, num_classes, (batch,), dtype=np.int64))
                        for _ in range(distinct)]

    def __iter__(self):
        i = 0
        while True:
            yield self.batches[i % len(self.batches)]
            i += 1


def collate_clips(samples):
    """[(uint8 [T,H,W,3], label)] -> (uint8 [B,T,H,W,3], int64 [B]) for torch.utils.data.DataLoader(collate_fn=...)."""
    return np.stack([s[0] for s in samples]), np.asarray([s[1] for s in samples], dtype=np.int64)


def t_major(x):
    """The reference's collated layout: a list of T tensors [B,3,H,W] (views of the [B,T,3,H,W] clip tensor)."""
    return [x[:, t] for t in range(x.shape[1])]


class ClipPipeline:
    """Iterates over ``source`` (any iterable of (uint8 [B,T,H,W,3], labels [B]) host batches -- a DataLoader over ClipCSVDataset
    with ``collate_fn=collate_clips``, or SyntheticClipSource) and yields device tensors (clips fp32 [B,T,3,H,W] in [0,1], labels),
    ``depth`` batches ahead of the consumer: pinned staging buffers, async H2D on its own stream, ToTensor on the device.
    ``transform`` (a ClipTransform): the clips come out augmented instead, fp32 [B,Tout,C,Ho,Wo] -- one parameter row per clip is drawn
    on the host, copied next to the bytes, and hyb_clips_u8_transform takes the ToTensor kernel's place on the copy stream.
    A transform that mixes (``transform.mixing()``): a mix row and a lam per clip travel with the parameter rows, the partners' labels are
    gathered on the host before the copy, hyb_clips_u8_transform_mix is the kernel, and the second item is ``MixTarget(y, y[partner], lam)``.
    A photometric transform (``transform.photometric()``): a photo row per clip travels too and hyb_clips_u8_transform_photo is the one kernel,
    with the mix rows or without; with a contrast range hyb_clips_u8_luma_sums fills a per-slot int64 [B,Tout] buffer in front of it on the copy
    stream.  What is yielded does not change.
    An evaluation transform with ``transform.views`` = V > 1: the source bytes are staged and copied once, [B,Tin,Hin,Win,C]; V parameter rows
    per clip (``transform.sample_views``) travel with them, hyb_clips_u8_transform_views is the one kernel, and what is yielded is
    (x fp32 [B*V,Tout,C,Ho,Wo], y int64 [B]) -- what ``model.evaluate(x, y, meter, views=V)`` and ``GraphedEval(..., views=V)`` take.
    ``pipeline.views`` is V (1 without a transform).
    2-D labels [B, classes] (multi-hot rows, or any dense target): the label slots are fp32 [B, classes], pinned on the host and on the device;
    floating input is used as given, integer / bool input is converted, and ``y`` is yielded as fp32 [B, classes] -- what
    HybridBCEWithLogitsLoss, GraphedTrainStep (dense target) and MultiLabelMeter take.  With a mixing transform the yielded row is
    lam_b y_b + (1 - lam_b) y_partner(b), formed on the host in fp32, in place of a MixTarget.  The first batch decides which kind a pipeline carries.
    A transform with ``antialias=True``: hyb_clips_u8_transform_aa is the one kernel, for the training rows (V = 1) and the evaluation views alike;
    the rows and what is yielded do not change.
    A transform with ``randaugment=`` or ``hue=`` (``transform.augmenting()``): an aug row int32 [B,32] per clip (``transform.sample_aug``) travels in the
    slots' ``host_aug`` / ``dev_aug`` beside the other rows and hyb_clip_aug_u8_transform is the one kernel, with the mix rows and the photo rows or
    without; hyb_clips_u8_luma_sums runs in front of it when a Contrast step or a contrast factor can be drawn.  What is yielded does not change."""

    def __init__(self, source, device="cuda", depth=2, transform=None):
        self.source, self.depth, self.transform = source, max(1, int(depth)), transform
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ClipPipeline feeds the MI355X HIP path: device must be cuda (there is no CPU fallback)")
        self.stream = torch.cuda.Stream(device=self.device)
        self._slots = None

    @property
    def views(self):
        """Output clips per source clip: the ``views=`` of the meter, model.evaluate and GraphedEval behind this pipeline."""
        return 1 if self.transform is None else self.transform.views

    def _make_slots(self, shape, label_shape=()):
        B, T, H, W, C = shape
        # 1-D labels: class indices, int64 [B]; 2-D labels: multi-hot / dense rows, fp32 [B, classes]
        dense = len(label_shape) == 2
        yshape, ydtype = ((B, int(label_shape[1])), torch.float32) if dense else ((B,), torch.int64)
        xshape = (B, T, C, H, W)
        if self.transform is not None:
            Tout, (Ho, Wo) = self.transform.out_frames(T), self.transform.size
            xshape = (B * self.views, Tout, C, Ho, Wo)
            mi = self.transform.mean_invstd(C)
            self._mean_invstd = None if mi is None else torch.from_numpy(mi).to(self.device)
        self._slots = [dict(host=torch.empty(shape, dtype=torch.uint8).pin_memory(), host_y=torch.empty(yshape, dtype=ydtype).pin_memory(),
                            dev_u8=torch.empty(shape, dtype=torch.uint8, device=self.device),
                            x=torch.empty(xshape, dtype=torch.float32, device=self.device),
                            y=torch.empty(yshape, dtype=ydtype, device=self.device), ready=torch.cuda.Event(), free=torch.cuda.Event())
                       for _ in range(self.depth + 1)]
        for s in self._slots:
            s["free"].record(torch.cuda.current_stream(self.device))
        if self.transform is not None:
            # the parameter rows are per slot for the same reason the bytes are: the copy stream writes batch n+2's while batch n's are read
            for s in self._slots:
                s["host_p"] = torch.empty(B * self.views, 8, dtype=torch.int32).pin_memory()
                s["dev_p"] = torch.empty(B * self.views, 8, dtype=torch.int32, device=self.device)
                if self.transform.mixing():
                    s["host_m"] = torch.empty(B, 8, dtype=torch.int32).pin_memory()
                    s["dev_m"] = torch.empty(B, 8, dtype=torch.int32, device=self.device)
                if self.transform.mixing() and not dense:     # dense rows are blended on the host: no second target, no lam
                    s["host_yb"] = torch.empty(B, dtype=torch.int64).pin_memory()
                    s["y_b"] = torch.empty(B, dtype=torch.int64, device=self.device)
                    s["host_lam"] = torch.empty(B, dtype=torch.float32).pin_memory()
                    s["lam"] = torch.empty(B, dtype=torch.float32, device=self.device)
                if self.transform.photometric():
                    s["host_ph"] = torch.empty(B, 16, dtype=torch.int32).pin_memory()
                    s["dev_ph"] = torch.empty(B, 16, dtype=torch.int32, device=self.device)
                if self.transform.augmenting():
                    s["host_aug"] = torch.empty(B, 32, dtype=torch.int32).pin_memory()
                    s["dev_aug"] = torch.empty(B, 32, dtype=torch.int32, device=self.device)
                if self.transform.needs_luma():           # (photometric or augmenting: a contrast factor or a Contrast step can be drawn)
                    s["luma"] = torch.empty(B, xshape[1], dtype=torch.int64, device=self.device)
            self.stream.wait_stream(torch.cuda.current_stream(self.device))      # mean_invstd was uploaded on the consumer's stream

    def _issue(self, slot, batch):
        frames, labels = batch
        frames = np.ascontiguousarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 5:
            raise ValueError("expected uint8 clips [B,T,H,W,C]")
        B, T, H, W, C = frames.shape
        s = self._slots[slot]
        s["free"].synchronize()                               # the consumer has finished with this slot's device tensors
        s["host"].numpy()[...] = frames                       # pageable -> pinned (the decoder could write here directly)
        dense = s["host_y"].dim() == 2
        if dense:
            rows = labels.numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
            if rows.ndim != 2:
                raise ValueError(f"this pipeline's first batch had 2-D labels {tuple(s['host_y'].shape)}; got labels of shape {rows.shape}")
            rows = rows.astype(np.float32, copy=False)        # floating input as given, integer / bool input converted
            s["host_y"].numpy()[...] = rows
        else:
            s["host_y"].numpy()[...] = np.asarray(labels, dtype=np.int64)
        views = self.views
        if self.transform is not None and not self.transform.train:
            # the evaluation rows, V adjacent ones per clip, no draw; with the default views they are sample()'s, and one view per clip
            # (eval_crop alone, say) goes through the plain kernel below
            s["host_p"].numpy()[...] = self.transform.sample_views(B, T, H, W)
        elif self.transform is not None:
            s["host_p"].numpy()[...] = self.transform.sample(B, T, H, W)      # one row per clip: all T frames share crop and flip
        mixing = self.transform is not None and self.transform.mixing()
        if mixing:
            rows, lam, partner = self.transform.sample_mix(B, *self.transform.size)
            s["host_m"].numpy()[...], own = rows, s["host_y"].numpy()
            if dense:                                         # the dense row of the mixed clip, in fp32: two products and a sum
                l = lam.astype(np.float32)[:, None]
                own[...] = l * own + (np.float32(1) - l) * own[partner]
            else:
                s["host_lam"].numpy()[...] = lam
                s["host_yb"].numpy()[...] = own[partner]      # the partners' labels, gathered here: the device only copies
        photo = self.transform is not None and self.transform.photometric()
        if photo:
            s["host_ph"].numpy()[...] = self.transform.sample_photo(B, self.transform.out_frames(T), *self.transform.size)
        augmenting = self.transform is not None and self.transform.augmenting()
        if augmenting:
            s["host_aug"].numpy()[...] = self.transform.sample_aug(B, *self.transform.size)
        with torch.cuda.stream(self.stream):
            s["dev_u8"].copy_(s["host"], non_blocking=True)
            s["y"].copy_(s["host_y"], non_blocking=True)
            if self.transform is None:
                lib.call("hyb_frames_u8hwc_to_f32chw", s["dev_u8"], s["x"], B * T, H, W, C, self.stream.cuda_stream)
            else:
                s["dev_p"].copy_(s["host_p"], non_blocking=True)
                Tout = s["x"].shape[1]
                if mixing:
                    s["dev_m"].copy_(s["host_m"], non_blocking=True)
                if mixing and not dense:
                    s["y_b"].copy_(s["host_yb"], non_blocking=True)
                    s["lam"].copy_(s["host_lam"], non_blocking=True)
                if photo:
                    s["dev_ph"].copy_(s["host_ph"], non_blocking=True)
                if augmenting:
                    s["dev_aug"].copy_(s["host_aug"], non_blocking=True)
                if "luma" in s:
                    lib.call("hyb_clips_u8_luma_sums", s["dev_u8"], s["dev_p"], s["luma"], B, T, H, W, C, Tout, self.stream.cuda_stream)
                # the one transform call: which kernel is ClipTransform.kernel()'s answer, how it is called is the operators' (ops.CLIP_OPS and
                # ops.CLIP_OPS_EXT)
                clip_transform_into(self.transform.kernel(), s["x"], s["dev_u8"], s["dev_p"], self._mean_invstd, views, self.stream.cuda_stream,
                                    mix=s.get("dev_m"), photo=s.get("dev_ph"), luma_sums=s.get("luma"), aug=s.get("dev_aug"))
            s["ready"].record(self.stream)

    def __iter__(self):
        it = iter(self.source)
        pending = []                                          # slots in flight, oldest first
        nxt = 0
        exhausted = False
        while True:
            while not exhausted and len(pending) < self.depth:
                try:
                    batch = next(it)
                except StopIteration:
                    exhausted = True
                    break
                if self._slots is None:
                    self._make_slots(tuple(batch[0].shape), tuple(np.shape(batch[1])))
                self._issue(nxt, batch)
                pending.append(nxt)
                nxt = (nxt + 1) % len(self._slots)
            if not pending:
                return
            slot = pending.pop(0)
            s = self._slots[slot]
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(s["ready"])                        # GPU-side wait only: the host does not block
            yield s["x"], (MixTarget(s["y"], s["y_b"], s["lam"]) if "lam" in s else s["y"])
            s["free"].record(torch.cuda.current_stream(self.device))      # everything the consumer enqueued on x / y so far


class ClipTransform:
    """Per-clip augmentation parameters for the device kernel ``hyb_clips_u8_transform`` (torchvision's ``RandomResizedCrop(size, scale,
    ratio)`` + ``RandomHorizontalFlip(hflip)`` + ``Normalize(mean, std)`` + a temporal window of ``frames`` frames, applied to all frames
    of a clip alike).  The host only draws one row ``{y0, x0, ch, cw, flip, t0, tstride, 0}`` per clip; the pixels are resampled on the
    device with ``F.interpolate(mode="bilinear", align_corners=False, antialias=False)`` arithmetic (``antialias=True`` below: with the filter).

    size          output (Ho, Wo), or one int for a square
    scale, ratio  RandomResizedCrop's area fraction and aspect-ratio (w / h) ranges              (train=True)
    hflip         probability of the horizontal flip                                             (train=True)
    mean, std     per-channel Normalize constants on the [0,1] scale, both or neither; the kernel gets fp32 ``mean`` and fp32 ``1/std``
    frames        output frames per clip (None: all of them, stride 1); frame_stride = (lo, hi): the stride is drawn among lo..hi
    seed          of the numpy Generator that draws the rows; data-parallel ranks pass ``seed + rank`` so that they augment differently
    train=False   the deterministic evaluation transform: largest centred crop of the output's aspect ratio, no flip, the smallest
                  stride, the centred temporal window, no mixing
    mixup_alpha, cutmix_alpha   > 0 switches Mixup / CutMix on (both 0, the default: nothing mixes, ``sample()`` draws what it always drew and
                  the plain kernel runs); lam ~ Beta(alpha, alpha).  The mix rows come from ``sample_mix`` and a SECOND Generator derived
                  from ``seed``: the crop rows of a seed are the same with mixing on and off
    mix_prob      probability that a batch (mix_mode="clip": a clip) is mixed at all
    switch_prob   probability of CutMix when both alphas are > 0
    mix_mode      "batch": one kind and one lam per batch; "clip": every clip draws its own.  The partner is a random permutation either way
    brightness, contrast, saturation   strength s >= 0 of torchvision's ColorJitter: the factor is drawn from U[max(0, 1-s), 1+s] per CLIP and
                  the three ops run in a uniformly drawn order; jitter_prob: probability that a clip is jittered at all.  The contrast pivot is
                  the mean luma of the clip's untouched source crops (one affine map for all frames of a clip), not torchvision's per-frame
                  mean of the jittered image; the hue jitter is ``hue`` below
    grayscale     probability that a clip becomes its luma in every channel (after the jitter)
    noise_std     sigma of additive Gaussian noise on the [0,1] scale, a float or a (lo, hi) range to draw it from; noise_prob: per clip
    erase_prob, erase_scale, erase_ratio   torchvision's RandomErasing: one box per clip in output coordinates, the same for all its frames;
                  erase_mode "zero" (0 after the normalisation), "black" (0 before it) or "pixel" (standard normal values)
                  All of these are drawn by ``sample_photo`` from a THIRD Generator derived from ``seed`` and applied by
                  hyb_clips_u8_transform_photo; with every one at its default (or train=False) nothing changes: the same kernels, draws and bits
    eval_views    (K, S) with train=False: K uniformly spaced temporal windows x S spatial crops per clip (the "clips x crops" protocol video
                  classifiers are reported under); ``views`` = K * S * (2 with eval_flip) rows per clip come from ``sample_views`` and
                  hyb_clips_u8_transform_views writes them in one launch.  (1, 1), the default: today's single centred view.  K > 1 needs ``frames``
    eval_crop     fraction in (0, 1] of the sides of the largest centred crop that each spatial crop takes: 224/256 on a source whose short
                  side is 256 is "resize 256, crop 224" (with ch == Ho bit for bit ToTensor of the crop).  The S crops are spread along the
                  axis with more slack, the first and last touching the borders (S == 3 on a landscape frame: left, centre, right)
    eval_flip     every view is followed by its horizontally flipped twin
                  An axis without slack gives coinciding views (S = 3 of a square source at eval_crop = 1: three times the same crop); that is
                  allowed.  All three are for train=False: a non-default value with train=True raises
    antialias     True: the resize is torchvision's ``Resize(antialias=True)`` -- ``F.interpolate(..., antialias=True)``'s triangle filter, whose
                  support grows with the down-scale -- for training rows and evaluation views alike (``kernel()`` is then "aa"); what to use
                  when the source is more than about 2 x the output ("resize 256, crop 224" from a 720-line decoder).  The rows do not change:
                  ``sample`` / ``sample_views`` of a seed are the same with it on and off.  Not provided together with mixing or the photometric
                  options (raises).  False, the default: the kernels, draws and bits are what they were
    randaugment   None, (n, m) or timm's string form "rand-m7-n4-mstd0.5" (m, n, mstd and inc1 are read; the increasing set is always used; any
                  other field is refused by name): RandAugment per CLIP.  n ops are drawn uniformly WITH replacement from ``ra_ops``, each is applied
                  with probability ``ra_prob`` at the magnitude clip(N(m, mstd), 0, 10); with L = magnitude / 10 the levels are timm's increasing
                  ones: Rotate +-30 L degrees, ShearX / ShearY +-0.3 L, TranslateX / TranslateY +-0.45 L of Wo / Ho, Brightness / Contrast / Color
                  max(0.1, 1 +- 0.9 L), Posterize 4 - int(4 L) bits, Solarize threshold 256 - int(256 L), SolarizeAdd int(110 L); a signed level
                  flips its sign with probability 1/2.  The geometric ops are folded on the host into ONE affine map (timm's PIL matrices, output ->
                  input, Rotate about the frame's centre, op 1 then op 2 = M1 o M2) that the kernel composes with the crop's resampling; the
                  photometric ops run in drawn order as a program of pointwise steps between the resampling and the colour jitter.  All frames of a
                  clip share the row; with Mixup / CutMix the partner goes through its own
    ra_ops        the names to draw from; None: timm's increasing set without AutoContrast, Equalize and Sharpness (``RA_OPS``)
    ra_prob       probability that a drawn op is applied
    fill          the value, on the [0, 1] scale, of pixels the affine map takes from outside the frame: a number or one per channel; None: ``mean``
                  when there is one, else 0.5.  A filled pixel goes through the program, the jitter and the normalisation like any other
    hue           h in [0, 1/2]: a shift from U[-h, h] per clip (torchvision's adjust_hue), drawn under ``jitter_prob`` by a draw of its own and
                  appended as the program's LAST step: it runs in front of the brightness / contrast / saturation steps, not inside their random
                  order as torchvision's ColorJitter would place it
                  These draws come from ``sample_aug`` and a FOURTH Generator derived from ``seed``: the crop, mix and photo rows of a seed do not move.
                  ``kernel()`` is then "aug" (hyb_clip_aug_u8_transform).  With the defaults (or train=False) nothing changes: the same kernels, draws
                  and bits.  Not provided: AutoContrast, Equalize, Sharpness, bicubic interpolation, per-frame programs, the new options together with
                  antialias=True (raises) or on evaluation views
    """

    def __init__(self, size, scale=(0.35, 1.0), ratio=(3 / 4, 4 / 3), hflip=0.5, mean=None, std=None, frames=None, frame_stride=(1, 1), seed=0,
                 train=True, mixup_alpha=0.0, cutmix_alpha=0.0, mix_prob=1.0, switch_prob=0.5, mix_mode="batch", brightness=0.0, contrast=0.0, saturation=0.0, jitter_prob=1.0,
                 grayscale=0.0, noise_std=0.0, noise_prob=1.0, erase_prob=0.0, erase_scale=(0.02, 1 / 3), erase_ratio=(0.3, 3.3), erase_mode="zero",
                 eval_views=(1, 1), eval_crop=1.0, eval_flip=False, antialias=False, randaugment=None, ra_ops=None, ra_prob=0.5, fill=None, hue=0.0):
        self.size = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        if min(self.size) <= 0:
            raise ValueError(f"size must be positive, got {size!r}")
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        if not (0 < self.scale[0] <= self.scale[1]) or not (0 < self.ratio[0] <= self.ratio[1]):
            raise ValueError("scale and ratio are (lo, hi) ranges of positive numbers")
        self.hflip = float(hflip)
        if (mean is None) != (std is None):
            raise ValueError("mean and std go together: give both or neither")
        self.mean = self.invstd = None
        if mean is not None:
            self.mean = np.atleast_1d(np.asarray(mean, dtype=np.float32))
            std32 = np.atleast_1d(np.asarray(std, dtype=np.float32))
            if self.mean.ndim != 1 or self.mean.shape != std32.shape:
                raise ValueError("mean and std must be sequences of the same length (one entry per channel)")
            if not np.all(std32 != 0):
                raise ValueError("std has a zero entry")
            self.invstd = (np.float32(1) / std32).astype(np.float32)          # the fp32 values the kernel multiplies by
        self.frames = None if frames is None else int(frames)
        if self.frames is not None and self.frames <= 0:
            raise ValueError("frames must be positive")
        self.frame_stride = (int(frame_stride[0]), int(frame_stride[1]))
        if not (1 <= self.frame_stride[0] <= self.frame_stride[1]):
            raise ValueError("frame_stride is a (lo, hi) range with 1 <= lo <= hi")
        self.seed, self.train = int(seed), bool(train)
        self.rng = np.random.default_rng(self.seed)
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.mix_prob, self.switch_prob = float(mix_prob), float(switch_prob)
        if self.mixup_alpha < 0 or self.cutmix_alpha < 0:
            raise ValueError("mixup_alpha and cutmix_alpha must be >= 0")
        if not (0.0 <= self.mix_prob <= 1.0 and 0.0 <= self.switch_prob <= 1.0):
            raise ValueError("mix_prob and switch_prob are probabilities")
        if mix_mode not in ("batch", "clip"):
            raise ValueError(f"mix_mode must be 'batch' or 'clip', got {mix_mode!r}")
        self.mix_mode = mix_mode
        self.mix_rng = np.random.default_rng([self.seed, 0x6d6978])          # its own stream: the crop rows do not move when mixing is switched on
        self.brightness, self.contrast, self.saturation = float(brightness), float(contrast), float(saturation)
        if not all(v >= 0 for v in (self.brightness, self.contrast, self.saturation)):
            raise ValueError("brightness, contrast and saturation are strengths >= 0")
        if max(self.brightness, self.contrast, self.saturation) > 15:
            raise ValueError("brightness, contrast and saturation must be <= 15 (the kernel clamps a factor to 16)")
        self.jitter_prob, self.grayscale = float(jitter_prob), float(grayscale)
        self.noise_prob, self.erase_prob = float(noise_prob), float(erase_prob)
        if not all(0.0 <= p <= 1.0 for p in (self.jitter_prob, self.grayscale, self.noise_prob, self.erase_prob)):
            raise ValueError("jitter_prob, grayscale, noise_prob and erase_prob are probabilities")
        self.noise_std = (float(noise_std), float(noise_std)) if np.isscalar(noise_std) else (float(noise_std[0]), float(noise_std[1]))
        if not (0 <= self.noise_std[0] <= self.noise_std[1] <= 1):
            raise ValueError("noise_std is a sigma on the [0,1] scale or a (lo, hi) range with 0 <= lo <= hi <= 1")
        self.erase_scale, self.erase_ratio = (float(erase_scale[0]), float(erase_scale[1])), (float(erase_ratio[0]), float(erase_ratio[1]))
        if not (0 < self.erase_scale[0] <= self.erase_scale[1] <= 1) or not (0 < self.erase_ratio[0] <= self.erase_ratio[1]):
            raise ValueError("erase_scale is a (lo, hi) range inside (0, 1], erase_ratio a (lo, hi) range of positive numbers")
        if erase_mode not in self.ERASE_MODES:
            raise ValueError(f"erase_mode must be one of {self.ERASE_MODES}, got {erase_mode!r}")
        self.erase_mode = erase_mode
        self.photo_rng = np.random.default_rng([self.seed, 0x70686f])        # a third stream: neither the crop rows nor the mix rows move
        self.eval_views, self.eval_crop, self.eval_flip = (int(eval_views[0]), int(eval_views[1])), float(eval_crop), bool(eval_flip)
        if min(self.eval_views) < 1:
            raise ValueError(f"eval_views is (K, S) with K >= 1 temporal windows and S >= 1 spatial crops, got {eval_views!r}")
        if not (0.0 < self.eval_crop <= 1.0):
            raise ValueError(f"eval_crop is a fraction in (0, 1], got {eval_crop!r}")
        if self.train and (self.eval_views != (1, 1) or self.eval_crop != 1.0 or self.eval_flip):
            raise ValueError("eval_views, eval_crop and eval_flip describe the evaluation transform: they need train=False")
        if self.eval_views[0] > 1 and self.frames is None:
            raise ValueError("eval_views with K > 1 temporal windows needs frames=: without it every window is the whole clip")
        self.antialias = bool(antialias)
        if self.antialias and (self.mixing() or self.photometric()):
            raise ValueError("antialias=True together with Mixup / CutMix or the photometric options is not provided: the antialiased resize has "
                             "no mix or photo kernel")
        self.randaugment = None if randaugment is None else self._parse_randaugment(randaugment)
        self.ra_ops = tuple(self.RA_OPS if ra_ops is None else ra_ops)
        unknown = [o for o in self.ra_ops if o not in self.RA_OPS]
        if unknown or not self.ra_ops:
            raise ValueError(f"ra_ops must be a non-empty selection of {self.RA_OPS}, got {unknown or ra_ops!r}")
        self.ra_prob, self.hue = float(ra_prob), float(hue)
        if not 0.0 <= self.ra_prob <= 1.0:
            raise ValueError("ra_prob is a probability")
        if not 0.0 <= self.hue <= 0.5:
            raise ValueError(f"hue is a range h in [0, 1/2] of the shift U[-h, h], got {hue!r}")
        if self.randaugment is not None and self.randaugment[0] + (self.hue > 0) > 8:
            raise ValueError("an aug row's program holds 8 steps: randaugment's n (plus one for hue) must not exceed it")
        if fill is None:
            # the default never refuses: the first three entries of any mean (the aug kernel takes C == 1 or 3), on the [0, 1] scale the row carries
            f = np.clip(self.mean[:3], 0, 1) if self.mean is not None else np.full(1, 0.5, dtype=np.float32)
        else:
            f = np.atleast_1d(np.asarray(fill, dtype=np.float32))
            if f.ndim != 1 or len(f) > 3 or not np.all((f >= 0) & (f <= 1)):
                raise ValueError(f"fill is a value in [0, 1] or one per channel, got {fill!r}")
        self.fill = np.concatenate([f, np.repeat(f[-1:], 3 - len(f))]).astype(np.float32)      # three entries, as the row carries them
        self.aug_rng = np.random.default_rng([self.seed, 0x617567])          # a fourth stream: the crop, mix and photo rows do not move
        if self.antialias and self.augmenting():
            raise ValueError("antialias=True together with randaugment= or hue= is not provided: the antialiased resize has no aug kernel")

    ERASE_MODES = ("zero", "black", "pixel")
    AUG_OPS = ("Identity", "Invert", "Brightness", "Contrast", "Color", "Posterize", "Solarize", "SolarizeAdd", "Hue")      # a program step's op code
    RA_GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateX", "TranslateY")
    # timm's increasing set (rand-...-inc1) without AutoContrast, Equalize and Sharpness
    RA_OPS = ("Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness", "ShearX", "ShearY", "TranslateX", "TranslateY")

    @staticmethod
    def _parse_randaugment(spec):
        """(n, m) or timm's "rand-m7-n4-mstd0.5[-inc1]" -> (n, m, mstd).  timm's defaults for a field left out: m 10, n 2, mstd 0."""
        if isinstance(spec, str):
            parts = spec.split("-")
            if parts[0] != "rand":
                raise ValueError(f"randaugment: {spec!r} does not start with 'rand'")
            n, m, mstd = 2, 10.0, 0.0
            for part in parts[1:]:
                key = part.rstrip("0123456789.")
                val = part[len(key):]
                try:
                    if key not in ("m", "n", "mstd", "inc") or not val:
                        raise ValueError
                    if key == "n":
                        n = int(val)
                    elif key == "m":
                        m = float(val)
                    elif key == "mstd":
                        mstd = float(val)
                    elif int(val) != 1:
                        raise ValueError
                except ValueError:
                    raise ValueError(f"randaugment: the field {part!r} of {spec!r} is not provided (m, n, mstd and inc1 are)") from None
        else:
            (n, m), mstd = spec, 0.0
            n, m = int(n), float(m)
        if not (0 <= n <= 8 and 0.0 <= m <= 10.0 and 0.0 <= mstd < float("inf")):
            raise ValueError(f"randaugment needs 0 <= n <= 8, 0 <= m <= 10 and a finite mstd >= 0, got n = {n}, m = {m}, mstd = {mstd}")
        return n, m, mstd

    def augmenting(self):
        """Whether this transform draws RandAugment ops or a hue shift (``kernel()`` is then "aug" and ClipPipeline carries aug rows)."""
        return self.train and (self.randaugment is not None or self.hue > 0)

    @staticmethod
    def _affine(name, level, Ho, Wo):
        """timm's PIL matrix (a, b, c, d, e, f) of one geometric op at a signed level, output -> input, as a 3 x 3 float64 matrix."""
        M = np.eye(3)
        if name == "Rotate":                                # PIL's Image.rotate(level degrees) about (Wo / 2, Ho / 2)
            a = -np.deg2rad(level)
            M[0, :2], M[1, :2] = (np.cos(a), np.sin(a)), (-np.sin(a), np.cos(a))
            cx, cy = Wo / 2.0, Ho / 2.0
            M[0, 2] = M[0, 0] * -cx + M[0, 1] * -cy + cx
            M[1, 2] = M[1, 0] * -cx + M[1, 1] * -cy + cy
        elif name == "ShearX":
            M[0, 1] = level
        elif name == "ShearY":
            M[1, 0] = level
        elif name == "TranslateX":
            M[0, 2] = level * Wo
        else:
            M[1, 2] = level * Ho
        return M

    def sample_aug(self, B, Ho, Wo):
        """-> int32 [B,32]: one aug row {flags, n, (op, arg) x 8, M[6] as fp32 bits, fill[3] as fp32 bits, 0 x 5} per clip for
        hyb_clip_aug_u8_transform.  A clip that draws nothing gets the identity row: no geometry, an empty program.  Per drawn op four draws
        are made whatever comes of them (the op, applied or not, the magnitude's normal deviate, the sign), then two for the hue."""
        rows = np.zeros((B, 32), dtype=np.int32)
        rows[:, 18:24] = np.asarray([1, 0, 0, 0, 1, 0], dtype=np.float32).view(np.int32)
        rows[:, 24:27] = self.fill.view(np.int32)
        if not self.augmenting():
            return rows
        g = self.aug_rng
        n, m, mstd = self.randaugment if self.randaugment is not None else (0, 0.0, 0.0)
        for b in range(B):
            M, geo, prog = np.eye(3), False, []
            for _ in range(n):
                name = self.ra_ops[int(g.integers(0, len(self.ra_ops)))]
                applied, z, negative = g.random() < self.ra_prob, g.standard_normal(), g.random() < 0.5
                if not applied:
                    continue
                L = min(max(m + mstd * z, 0.0), 10.0) / 10.0
                sign = -1.0 if negative else 1.0
                if name in self.RA_GEOMETRIC:
                    level = sign * L * {"Rotate": 30.0, "ShearX": 0.3, "ShearY": 0.3, "TranslateX": 0.45, "TranslateY": 0.45}[name]
                    M, geo = M @ self._affine(name, level, Ho, Wo), True      # op 1 then op 2: M1 o M2
                elif name in ("Brightness", "Contrast", "Color"):
                    prog.append((self.AUG_OPS.index(name), int(np.float32(max(0.1, 1.0 + sign * 0.9 * L)).view(np.int32))))
                elif name == "Posterize":
                    prog.append((5, 4 - int(4 * L)))
                elif name == "Solarize":
                    prog.append((6, 256 - int(256 * L)))
                elif name == "SolarizeAdd":
                    prog.append((7, int(110 * L)))
                else:
                    prog.append((1, 0))
            if self.hue > 0:
                jitter, u = g.random() < self.jitter_prob, g.uniform(-self.hue, self.hue)
                if jitter:
                    prog.append((8, int(np.float32(u).view(np.int32))))
            rows[b, 0], rows[b, 1] = int(geo), len(prog)
            for i, (op, arg) in enumerate(prog):
                rows[b, 2 + 2 * i], rows[b, 3 + 2 * i] = op, arg
            if geo:
                rows[b, 18:24] = M[:2].reshape(6).astype(np.float32).view(np.int32)
        return rows

    def photometric(self):
        """Whether this transform jitters, grays, adds noise or erases (``kernel()`` says what ClipPipeline then calls)."""
        return self.train and (self.brightness > 0 or self.contrast > 0 or self.saturation > 0 or self.grayscale > 0 or self.noise_std[1] > 0
                               or self.erase_prob > 0)

    def needs_luma(self):
        """Whether a contrast factor other than 1 may be drawn, by the jitter or as a RandAugment Contrast step: the kernel then needs
        hyb_clips_u8_luma_sums for its pivot."""
        return self.train and (self.contrast > 0 or (self.randaugment is not None and self.randaugment[0] > 0 and "Contrast" in self.ra_ops))

    def _erase_box(self, Ho, Wo):
        """torchvision's RandomErasing.get_params: up to 10 tries of area x log-uniform ratio that fit strictly inside, else no box."""
        g, area = self.photo_rng, Ho * Wo
        for _ in range(10):
            target = area * g.uniform(self.erase_scale[0], self.erase_scale[1])
            ar = float(np.exp(g.uniform(np.log(self.erase_ratio[0]), np.log(self.erase_ratio[1]))))
            h, w = int(round(np.sqrt(target * ar))), int(round(np.sqrt(target / ar)))
            if 0 < h < Ho and 0 < w < Wo:
                return int(g.integers(0, Ho - h + 1)), int(g.integers(0, Wo - w + 1)), h, w
        return 0, 0, 0, 0

    def sample_photo(self, B, Tout, Ho, Wo):
        """-> int32 [B,16]: one photo row {brightness, contrast, saturation factor bits, order, gray, sigma bits, seed lo, seed hi, ey0, ex0, eh,
        ew, mode, 0, 0, 0} per clip for hyb_clips_u8_transform_photo.  A clip that draws nothing gets the identity row: factors 1, sigma 0, no
        box.  Every clip draws a seed, so that the noise and the "pixel" erase of two clips never repeat."""
        rows = np.zeros((B, 16), dtype=np.int32)
        one = np.ones(3, dtype=np.float32)
        rows[:, 0:3] = one.view(np.int32)
        rows[:, 12] = self.ERASE_MODES.index(self.erase_mode)
        if not self.photometric():
            return rows
        g = self.photo_rng
        strengths = (self.brightness, self.contrast, self.saturation)
        for b in range(B):
            f = one.copy()
            if max(strengths) > 0 and g.random() < self.jitter_prob:
                for i, s in enumerate(strengths):
                    if s > 0:
                        f[i] = np.float32(g.uniform(max(0.0, 1.0 - s), 1.0 + s))
                rows[b, 3] = int(g.integers(0, 6))
            rows[b, 0:3] = f.view(np.int32)
            if self.grayscale > 0:
                rows[b, 4] = int(g.random() < self.grayscale)
            if self.noise_std[1] > 0 and g.random() < self.noise_prob:
                rows[b, 5] = int(np.float32(g.uniform(self.noise_std[0], self.noise_std[1])).view(np.int32))
            rows[b, 6:8] = np.asarray([g.integers(0, 1 << 64, dtype=np.uint64)], dtype=np.uint64).view(np.int32)
            if self.erase_prob > 0 and g.random() < self.erase_prob:
                rows[b, 8:12] = self._erase_box(Ho, Wo)
        return rows

    def kernel(self):
        """Which device transform ClipPipeline runs for this transform: a key of ops.CLIP_OPS (or, for "aug", ops.CLIP_OPS_EXT).  The first that
        applies of
          "aug"    hyb_clip_aug_u8_transform     randaugment= or hue= is on (``augmenting()``), with mixing and the photometric options or without
          "photo"  hyb_clips_u8_transform_photo  a photometric option is on (``photometric()``), with mixing or without
          "aa"     hyb_clips_u8_transform_aa     antialias=True, for the training rows (V = 1) and the evaluation views alike
          "views"  hyb_clips_u8_transform_views  more than one evaluation view per clip (``views`` > 1)
          "mix"    hyb_clips_u8_transform_mix    Mixup / CutMix (``mixing()``)
          "plain"  hyb_clips_u8_transform        everything else: train=False switches mixing and the photometric options off
        This is the only statement of the rule."""
        if self.augmenting():
            return "aug"
        if self.photometric():
            return "photo"
        if self.antialias:
            return "aa"
        if self.views > 1:
            return "views"
        return "mix" if self.mixing() else "plain"

    @property
    def views(self):
        """Output clips per source clip: K * S * (2 with eval_flip); always 1 with train=True."""
        return 1 if self.train else self.eval_views[0] * self.eval_views[1] * (2 if self.eval_flip else 1)

    def _centre_crop(self, Hin, Win):
        """(h, w) of the largest crop of the output's aspect ratio that fits the frame: the train=False crop."""
        Ho, Wo = self.size
        if Win * Ho >= Hin * Wo:
            return Hin, max(1, Hin * Wo // Ho)
        return max(1, Win * Ho // Wo), Win

    def sample_views(self, B, Tin, Hin, Win):
        """-> int32 [B*V,8]: the V = ``views`` rows {y0, x0, ch, cw, flip, t0, tstride, 0} of every clip for hyb_clips_u8_transform_views, clip-major,
        then temporal window k, then spatial crop s, then flip (fastest).  Deterministic: nothing is drawn.
          crop      (h0, w0) = the train=False crop of ``sample``; eval_crop == 1: (h, w) = (h0, w0), else max(1, round(h0 * eval_crop)), likewise w
          position  slack sy = Hin - h, sx = Win - w; the crops are spread along x if sx >= sy, else along y; the other axis is centred at
                    slack // 2; on the spread axis S == 1 gives slack // 2 and S > 1 gives slack * s // (S - 1): the first and last crops touch the
                    two borders
          time      the smallest fitting stride; span = (Tout - 1) * stride + 1, slack_t = Tin - span; K == 1: t0 = slack_t // 2, K > 1:
                    t0 = slack_t * k // (K - 1)
        No row needs the kernel's clamps.  With the defaults the rows are ``sample``'s."""
        if self.train:
            raise ValueError("sample_views is the evaluation sampler: it needs train=False")
        Tout = self.out_frames(Tin)
        (K, S), F = self.eval_views, 2 if self.eval_flip else 1
        h, w = self._centre_crop(Hin, Win)
        if self.eval_crop != 1.0:
            h, w = max(1, int(round(h * self.eval_crop))), max(1, int(round(w * self.eval_crop)))
        sy, sx = Hin - h, Win - w
        along_x = sx >= sy
        stride, slack_t = 1, 0
        if self.frames is not None:
            stride = self._strides(Tin)[0]
            slack_t = Tin - ((Tout - 1) * stride + 1)
        one = np.zeros((K, S, F, 8), dtype=np.int32)
        for k in range(K):
            t0 = slack_t // 2 if K == 1 else slack_t * k // (K - 1)
            for s in range(S):
                slack = sx if along_x else sy
                at = slack // 2 if S == 1 else slack * s // (S - 1)
                y0, x0 = (sy // 2, at) if along_x else (at, sx // 2)
                for f in range(F):
                    one[k, s, f] = (y0, x0, h, w, f, t0, stride, 0)
        return np.tile(one.reshape(K * S * F, 8), (B, 1))                 # every clip of a batch has the same shape: the same V rows

    def out_frames(self, Tin):
        if self.frames is not None and self.frames > Tin:
            raise ValueError(f"frames={self.frames} exceeds the clip length {Tin}")
        return Tin if self.frames is None else self.frames

    def mean_invstd(self, C):
        """fp32 [2,C] (mean, then 1/std) as the kernel reads it, or None without normalisation."""
        if self.mean is None:
            return None
        if len(self.mean) != C:
            raise ValueError(f"mean/std have {len(self.mean)} entries, the clips have {C} channels")
        return np.stack([self.mean, self.invstd])

    def _strides(self, Tin):
        fit = [s for s in range(self.frame_stride[0], self.frame_stride[1] + 1) if (self.frames - 1) * s < Tin]
        if not fit:
            raise ValueError(f"no stride of frame_stride={self.frame_stride} fits {self.frames} frames into a clip of {Tin}")
        return fit

    def _crop(self, Hin, Win):
        """torchvision's RandomResizedCrop.get_params: up to 10 tries of area x log-uniform ratio that fit, then the largest centred
        crop with the image's ratio clamped into range."""
        g, area = self.rng, Hin * Win
        for _ in range(10):
            target = area * g.uniform(self.scale[0], self.scale[1])
            ar = float(np.exp(g.uniform(np.log(self.ratio[0]), np.log(self.ratio[1]))))
            w, h = int(round(np.sqrt(target * ar))), int(round(np.sqrt(target / ar)))
            if 0 < w <= Win and 0 < h <= Hin:
                return int(g.integers(0, Hin - h + 1)), int(g.integers(0, Win - w + 1)), h, w
        in_ratio = Win / Hin
        if in_ratio < self.ratio[0]:
            w, h = Win, min(Hin, max(1, int(round(Win / self.ratio[0]))))
        elif in_ratio > self.ratio[1]:
            h, w = Hin, min(Win, max(1, int(round(Hin * self.ratio[1]))))
        else:
            w, h = Win, Hin
        return (Hin - h) // 2, (Win - w) // 2, h, w

    def sample(self, B, Tin, Hin, Win):
        """-> int32 [B,8]: one row {y0, x0, ch, cw, flip, t0, tstride, 0} per clip of a [B,Tin,Hin,Win,C] batch."""
        Tout = self.out_frames(Tin)
        rows = np.zeros((B, 8), dtype=np.int32)
        Ho, Wo = self.size
        for b in range(B):
            if self.train:
                y0, x0, h, w = self._crop(Hin, Win)
                flip = int(self.rng.random() < self.hflip)
            else:
                h, w = self._centre_crop(Hin, Win)
                y0, x0, flip = (Hin - h) // 2, (Win - w) // 2, 0
            t0, stride = 0, 1
            if self.frames is not None:
                fit = self._strides(Tin)
                if self.train:
                    stride = fit[int(self.rng.integers(0, len(fit)))]
                    t0 = int(self.rng.integers(0, Tin - (Tout - 1) * stride))
                else:
                    stride = fit[0]
                    t0 = (Tin - ((Tout - 1) * stride + 1)) // 2
            rows[b] = (y0, x0, h, w, flip, t0, stride, 0)
        return rows

    def mixing(self):
        """Whether this transform mixes clips (ClipPipeline then yields MixTargets; ``kernel()`` says what it calls)."""
        return self.train and (self.mixup_alpha > 0 or self.cutmix_alpha > 0)

    def _mix_draw(self, Ho, Wo):
        """One (kind, lam, box) draw: kind 1 Mixup, 2 CutMix (the usual recipe: centre uniform, sides sqrt(1 - lam) of the output's, clipped to the
        frame, lam recomputed from the clipped box), 0 when mix_prob says not this time."""
        g = self.mix_rng
        if g.random() >= self.mix_prob:
            return 0, np.float32(1), (0, 0, 0, 0)
        cut = self.cutmix_alpha > 0 and (self.mixup_alpha <= 0 or g.random() < self.switch_prob)
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(g.beta(alpha, alpha))
        if not cut:
            return 1, np.float32(lam), (0, 0, 0, 0)
        r = np.sqrt(1.0 - lam)
        h, w = int(Ho * r), int(Wo * r)
        cy, cx = int(g.integers(0, Ho)), int(g.integers(0, Wo))
        y0, y1 = min(max(cy - h // 2, 0), Ho), min(max(cy + h // 2, 0), Ho)
        x0, x1 = min(max(cx - w // 2, 0), Wo), min(max(cx + w // 2, 0), Wo)
        bh, bw = y1 - y0, x1 - x0
        return 2, np.float32(1.0 - bh * bw / float(Ho * Wo)), (y0, x0, bh, bw)

    def sample_mix(self, B, Ho, Wo):
        """-> (rows int32 [B,8], lam fp32 [B], partner int64 [B]): one mix row {partner, kind, by0, bx0, bh, bw, lam_bits, 0} per clip for
        hyb_clips_u8_transform_mix, the label weight of each clip's own class (CutMix: 1 - box area / frame area, from the clipped box) and the
        partner permutation.  Un-mixed clips: kind 0, lam 1, partner = self."""
        rows = np.zeros((B, 8), dtype=np.int32)
        lam = np.ones(B, dtype=np.float32)
        partner = np.arange(B, dtype=np.int64)
        rows[:, 0] = partner
        if not self.mixing():
            rows[:, 6] = lam.view(np.int32)
            return rows, lam, partner
        perm = self.mix_rng.permutation(B).astype(np.int64)
        shared = self._mix_draw(Ho, Wo) if self.mix_mode == "batch" else None
        for b in range(B):
            kind, l, (y0, x0, bh, bw) = shared if shared is not None else self._mix_draw(Ho, Wo)
            if kind == 0:
                continue
            partner[b], lam[b] = perm[b], l
            rows[b, :6] = (perm[b], kind, y0, x0, bh, bw)
        rows[:, 6] = lam.view(np.int32)
        return rows, lam, partner
