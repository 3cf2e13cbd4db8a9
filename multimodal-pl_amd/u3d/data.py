"""Training data path on the device.

* ``crop_patch``: AMOSDataSet_newatlas.__getitem__'s tensor work (MOTSDataset.py:355-384): pad to crop + 5 (zeros),
  truncate (:171-186: CT clipped to [-325, 325] / 325 for case ids < 500, MRI z-scored over the padded volume),
  the random crop (offsets drawn with np.random in the reference's order b, c, a) and the (H, W, D) -> (D, H, W)
  transpose — one device pass per tensor (u3d_crop_transpose; the MRI statistics by u3d_volume_stats).
* ``atlas_crop``: the atlas side of the same lines starting from the raw atlas: the nearest resize to the image's shape
  (:357) is taken inside the crop (u3d_atlas_crop), so the image-sized atlas (13 x H x W x D floats) is never formed.
  ``crop_patch(..., atlas=raw)`` uses it.
* ``train_transform``: my_collate's batchgenerators transforms (get_train_transform, :33-52) with their published
  parameters: Gaussian noise (p 0.1), Gaussian blur (sigma U(0.5, 1), per channel p 0.5, p 0.2), multiplicative
  brightness U(0.75, 1.25) (p 0.15), additive brightness N(0, 0.1) (per channel p 0.5, p 0.15), contrast
  (0.75, 1.25), preserve range (p 0.15). Decisions and parameters are drawn on the host with numpy; the kernels apply
  them. batchgenerators is not installed here, so the exact draw sequence is unpinned (each applied operation is
  pinned against numpy / scipy restatements in tests/test_gpu_data.py); the noise uses a counter-based device RNG.
* ``AtlasBuilder`` / ``build_atlas``: the atlas itself (preprocess/atlas_gen_mm.py:100-145): per case one gather of the
  label codes through scipy's zoom(order=0) index tables (``zoom_index``, float64 on the host) into per-label sums
  (u3d_atlas_build_add), then sums / case counts (u3d_atlas_build_normalize) and gaussian_filter(sigma=3) as three
  u3d_aug_blur_axis passes over all planes. ``average_shape``: the atlas shape of :100-111.
* ``label_components`` / ``largest_component`` / ``get_body`` / ``bounding_box`` / ``body_crop``: the body mask and the
  three crops of preprocess/forward_crop.py (:37-82 getmaxcomponent / get_body, :148-207) on 3-D connected components
  labelled on the device (csrc/ccl.hip: a single-pass union-find, scipy.ndimage.label's numbering). get_body queues
  its box-opening fallback behind the component search, gated on the device by the search's record, so a case costs
  three small host reads: the label range and the two body records.
* ``spacing_plan`` / ``GridPlan`` / ``resample_spacing`` / ``preprocess_case``: MONAI's Orientationd + Spacingd as
  preprocess/transforms.py:41-54 applies them (forward_crop.py:121-146), and the way back for predictions
  (``GridPlan.inverse``). With Spacing's defaults the resampling is a permutation and flip of the axes followed by an
  independent scale per axis, so the grid is a few float64 operations on the host (``orientation_of``: nibabel's
  io_orientation) and the sampling a gather through three per-axis tables (csrc/resample.hip: trilinear in fp64 with
  border clamping, or nearest). monai is not installed here: the sampling is pinned to torch's grid_sample on float64
  (the engine MONAI calls) and to scipy's map_coordinates, the output grid to its formulas; bit parity with one MONAI
  release is not pinned, in particular the output size where (n - 1) s / p + 1 is a half-integer (``out_shape=``).
* ``restore_prediction`` / ``GridPlan.restrict_source`` / ``GridPlan.apply_argmax`` / ``keep_largest_per_label``: from
  the network's output on preprocess_case's image_a to a uint8 label map on the case's own voxels. body_crop records
  where its crop sits (``origin``, ``input_shape``); the inverse plan is restricted to that crop and the scores are
  interpolated and decided in one kernel (u3d_grid_resample_argmax: the argmax over the linear kernel's output, bit
  for bit, without the C resampled volumes); the per-organ largest-component cleanup labels all organs at once
  (u3d_ccl_keep_largest: the union-find of csrc/ccl.hip joining only voxels of one code). No host read in either.
"""
import math

import numpy as np
import torch

from . import ops
from ._lib import U3DError, call, query

MODE_COPY, MODE_CT, MODE_MRI = 0, 1, 2


def volume_stats(x, count=None):
    """[mean, population std, min, max] of a device fp32 tensor extended by (count - numel) zeros (fp64, fixed
    order)."""
    x = x.float().contiguous()
    out = torch.empty(4, dtype=torch.float32, device=x.device)
    ws = ops.WS.get(query("u3d_volume_stats_ws_bytes"), x.device, ops.Slot.VOLUME_STATS)
    call("u3d_volume_stats", x.data_ptr(), x.numel(), int(count or x.numel()), out.data_ptr(), ws.data_ptr(),
         ops._stream())
    return out


def crop_transpose(src, offsets, crop, mode=MODE_COPY, stats=None):
    """src [C, H, W, D] (or [H, W, D]) fp32 device; offsets (b, c, a); crop (ch, cw, cd) -> [C, cd, ch, cw]."""
    ops.require_device(src)
    s = src.float().contiguous()
    if s.dim() == 3:
        s = s.unsqueeze(0)
    C, sh, sw, sd = s.shape
    ch, cw, cd = crop
    out = torch.empty((C, cd, ch, cw), dtype=torch.float32, device=s.device)
    call("u3d_crop_transpose", s.data_ptr(), C, sh, sw, sd, int(offsets[0]), int(offsets[1]), int(offsets[2]), ch, cw,
         cd, mode, stats.data_ptr() if stats is not None else None, out.data_ptr(), ops._stream())
    return out


def atlas_crop(atlas, image_shape, offsets, crop):
    """The dataset's atlas path without the image-sized intermediate: atlas [C, Ah, Aw, Ad] device (fp32; a float64
    tensor is cast once, the rounding of the driver's later .float()), image_shape (H, W, D) as the dataset sees the
    image before pad_image, offsets (b, c, a) and crop (ch, cw, cd) as crop_transpose -> [C, cd, ch, cw], equal to
    crop_transpose(F.interpolate(atlas[None], image_shape)[0], offsets, crop) with the nearest resize taken as the
    reference takes it, on a float64 CPU tensor: source index floor(i * in / out) in integers (u3d_atlas_crop). A
    float32 or device interpolate rounds i * (in / out) in float32 and lands one voxel off at some sizes."""
    ops.require_device(atlas)
    if atlas.dim() != 4 or len(image_shape) != 3:
        raise ValueError(f"atlas_crop: atlas {tuple(atlas.shape)} must be [C, Ah, Aw, Ad], image_shape (H, W, D)")
    a = atlas.float().contiguous()
    C, Ah, Aw, Ad = a.shape
    ch, cw, cd = (int(v) for v in crop)
    out = torch.empty((C, cd, ch, cw), dtype=torch.float32, device=a.device)
    call("u3d_atlas_crop", a.data_ptr(), C, Ah, Aw, Ad, int(image_shape[0]), int(image_shape[1]), int(image_shape[2]),
         int(offsets[0]), int(offsets[1]), int(offsets[2]), ch, cw, cd, out.data_ptr(), ops._stream())
    return out


def crop_patch(image, label, catlas, name, crop_size, usage="train", rng=np.random, atlas=None):
    """image / label [H, W, D], catlas [13, H, W, D] device tensors as read (sitk arrays); crop_size = (d, h, w) as
    the dataset's (crop_d, crop_h, crop_w). Returns image [1, D, H, W], label [1, D, H, W], catlas [13, D, H, W].
    ``atlas=``: the raw atlas [13, Ah, Aw, Ad] (device, fp32 or float64) in place of catlas (which must then be None;
    both is a ValueError): the resize of MOTSDataset.py:357 happens inside the crop (atlas_crop), the draws and the
    three outputs are those of the call with catlas = the reference's resized atlas."""
    if atlas is not None and catlas is not None:
        raise ValueError("crop_patch: pass catlas (already at image size) or atlas= (raw, resized in the crop), not both")
    cd, ch, cw = crop_size
    H, W, D = image.shape
    ph, pw, pd = max(H, ch + 5), max(W, cw + 5), max(D, cd + 5)   # pad_image to crop + 5 (zeros)
    mri = float(name) >= 500                                     # truncate(image, name), :177
    stats = None
    if mri:  # z-score over the PADDED volume: the padding zeros count, as np.mean / np.std see them
        stats = volume_stats(image, ph * pw * pd)
    if usage == "train":
        b = rng.randint(ph - ch)
        c = rng.randint(pw - cw)
        a = rng.randint(pd - cd)
        out_hw = (ch, cw, cd)
    else:
        b = c = a = 0
        out_hw = (ph, pw, pd)
    img = crop_transpose(image, (b, c, a), out_hw, MODE_MRI if mri else MODE_CT, stats)
    lab = crop_transpose(label, (b, c, a), out_hw)
    if atlas is not None:
        cat = atlas_crop(atlas, (H, W, D), (b, c, a), out_hw)
    else:
        cat = crop_transpose(catlas, (b, c, a), out_hw) if catlas is not None else None
    return img, lab, cat


def gaussian_kernel1d(sigma, truncate=4.0):
    """scipy.ndimage's 1-D Gaussian (order 0): radius int(truncate * sigma + 0.5), normalised."""
    r = int(truncate * float(sigma) + 0.5)
    xs = np.arange(-r, r + 1, dtype=np.float64)
    k = np.exp(-0.5 / (sigma * sigma) * xs ** 2)
    return (k / k.sum()).astype(np.float32), r


def gaussian_blur(x, sigma):
    """scipy.ndimage.gaussian_filter(x, sigma) (mode 'reflect', truncate 4) of a [D, H, W] device volume, three
    separable passes."""
    w, r = gaussian_kernel1d(sigma)
    wt = torch.from_numpy(w).to(x.device)
    cur = x.float().contiguous()
    D, H, W = cur.shape
    for outer, L, inner in ((1, D, H * W), (D, H, W), (D * H, W, 1)):
        nxt = torch.empty_like(cur)
        call("u3d_aug_blur_axis", cur.data_ptr(), nxt.data_ptr(), outer, L, inner, wt.data_ptr(), r, ops._stream())
        cur = nxt
    return cur


def train_transform(image, rng=np.random, seed=None):
    """my_collate's intensity transforms on a device batch [B, C, D, H, W] (in place where the reference is).
    Returns the batch and a log of the applied operations (for tests / reproducibility)."""
    ops.require_device(image)
    x = image.float().contiguous()
    B, C = x.shape[:2]
    log = []
    base = int(seed if seed is not None else rng.randint(0, 2 ** 31 - 1))
    for b in range(B):                                   # GaussianNoiseTransform(p_per_sample=0.1)
        if rng.uniform() < 0.1:
            var = rng.uniform(0.0, 0.1)
            call("u3d_aug_noise", x[b].data_ptr(), x[b].numel(), float(var), (base * 1000003 + b) & (2 ** 64 - 1),
                 ops._stream())
            log.append(("noise", b, var))
    for b in range(B):                                   # GaussianBlurTransform((0.5, 1), p_ch 0.5, p 0.2)
        if rng.uniform() < 0.2:
            for c in range(C):
                if rng.uniform() < 0.5:
                    sigma = rng.uniform(0.5, 1.0)
                    x[b, c].copy_(gaussian_blur(x[b, c], sigma))
                    log.append(("blur", b, c, sigma))
    for b in range(B):                                   # BrightnessMultiplicativeTransform((0.75, 1.25), p 0.15)
        if rng.uniform() < 0.15:
            for c in range(C):
                m = rng.uniform(0.75, 1.25)
                call("u3d_aug_affine", x[b, c].data_ptr(), x[b, c].numel(), float(m), 0.0, ops._stream())
                log.append(("mul", b, c, m))
    for b in range(B):                                   # BrightnessTransform(0, 0.1, per channel, p_ch 0.5, p 0.15)
        if rng.uniform() < 0.15:
            for c in range(C):
                if rng.uniform() < 0.5:
                    a = rng.normal(0.0, 0.1)
                    call("u3d_aug_affine", x[b, c].data_ptr(), x[b, c].numel(), 1.0, float(a), ops._stream())
                    log.append(("add", b, c, a))
    for b in range(B):                                   # ContrastAugmentationTransform((0.75, 1.25), p 0.15)
        if rng.uniform() < 0.15:
            for c in range(C):
                f = rng.uniform(0.75, 1.0) if rng.uniform() < 0.5 else rng.uniform(1.0, 1.25)
                st = volume_stats(x[b, c])
                call("u3d_aug_contrast", x[b, c].data_ptr(), x[b, c].numel(), float(f), st.data_ptr(), 1,
                     ops._stream())
                log.append(("contrast", b, c, f))
    return x, log


def zoom_index(n_in, n_out):
    """Source index of every output index of scipy.ndimage.zoom(order=0) (mode 'constant', grid_mode False) along an
    axis resized n_in -> n_out, int32 [n_out]; -1 where scipy takes the coordinate as outside the volume and leaves the
    voxel 0. scipy's float64 arithmetic: z = (n_in - 1) / (n_out - 1) (1 when n_out == 1), cc = k * z rounded once,
    floor(cc + 0.5) if cc <= n_in - 1. The "outside" case is real: (n_out - 1) * z rounds to just above n_in - 1 at
    e.g. 8 -> 26, 22 -> 20, 30 -> 8, 26 -> 12, and the whole last plane of that axis receives nothing."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"zoom_index: sizes {n_in} -> {n_out} must be positive")
    z = np.float64(n_in - 1) / np.float64(n_out - 1) if n_out > 1 else np.float64(1.0)
    cc = np.arange(n_out, dtype=np.float64) * z
    src = np.floor(cc + 0.5).astype(np.int64)
    return np.where(cc <= np.float64(n_in - 1), src, -1).astype(np.int32)


def average_shape(shapes):
    """atlas_gen_mm.py:100-111: per axis the integer sum over the cases, divided by their number, np.round (half to
    even), int."""
    shapes = [tuple(int(v) for v in s) for s in shapes]
    if not shapes or any(len(s) != 3 for s in shapes):
        raise ValueError("average_shape: needs at least one (H, W, D) shape")
    total = [sum(s[i] for s in shapes) for i in range(3)]
    return tuple(int(np.round(t / len(shapes))) for t in total)


class AtlasBuilder:
    """The sums of atlas_gen_mm.py:114-136 on the device. ``acc`` fp32 [L, s0, s1, s2] (voxels of label l + 1 after the
    zoom, summed over the cases) and ``counts`` int32 [L] (cases that hold label l + 1 before the zoom) are plain
    sums: partial builders merge by adding them. ``add`` one case at a time, ``finish`` for the atlas."""

    def __init__(self, shape, num_labels=15, device=None):
        shape = tuple(int(v) for v in shape)
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"AtlasBuilder: shape {shape} must be three positive sizes")
        if not 1 <= int(num_labels) <= 31:
            raise ValueError(f"AtlasBuilder: num_labels={num_labels} must be in 1..31 (one presence bit per label)")
        self.shape, self.num_labels = shape, int(num_labels)
        if device is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device) if device is not None else None
        self.acc = self.counts = None
        self._idx = {}
        if self.device is not None:
            if self.device.type != "cuda":
                raise U3DError(f"AtlasBuilder: device {self.device}: the HIP path needs a ROCm device (no CPU fallback)")
            self.acc = torch.zeros((self.num_labels,) + shape, dtype=torch.float32, device=self.device)
            self.counts = torch.zeros(self.num_labels, dtype=torch.int32, device=self.device)
            self._ws = torch.zeros(query("u3d_atlas_build_ws_bytes"), dtype=torch.uint8, device=self.device)

    def _table(self, n_in, n_out):
        key = (int(n_in), int(n_out))
        if key not in self._idx:
            self._idx[key] = torch.from_numpy(zoom_index(*key)).to(self.device)
        return self._idx[key]

    def add(self, label):
        """One case [H, W, D] of label codes (uint8, int16, int32, int64, float32 or float64, on the device). A voxel
        belongs to label l only if its value equals l exactly: anything that is no integer in 0..255 (257, -255, 1.5,
        NaN) counts as background and does not wrap onto a label."""
        if label.dim() != 3 or label.numel() == 0:
            raise ValueError(f"AtlasBuilder.add: label {tuple(label.shape)} must be a non-empty [H, W, D] volume")
        ops.require_device(label)
        if self.acc is None or label.device != self.device:
            raise ValueError(f"AtlasBuilder.add: label on {label.device}, builder on {self.device}")
        if label.dtype == torch.uint8:
            u8 = label.contiguous()
        elif label.dtype in (torch.int16, torch.int32, torch.int64, torch.float32, torch.float64):
            ok = (label >= 0) & (label <= 255)
            if label.is_floating_point():
                ok &= label == label.floor()
            u8 = torch.where(ok, label, torch.zeros((), dtype=label.dtype, device=label.device)).to(torch.uint8)
            u8 = u8.contiguous()
        else:
            raise ValueError(f"AtlasBuilder.add: label dtype {label.dtype} not supported")
        h, w, d = u8.shape
        s0, s1, s2 = self.shape
        i0, i1, i2 = self._table(h, s0), self._table(w, s1), self._table(d, s2)
        with torch.cuda.device(self.device):
            call("u3d_atlas_build_add", u8.data_ptr(), h, w, d, i0.data_ptr(), i1.data_ptr(), i2.data_ptr(),
                 self.num_labels, s0, s1, s2, self.acc.data_ptr(), self.counts.data_ptr(), self._ws.data_ptr(),
                 ops._stream())
        return self

    def finish(self, sigma=3.0):
        """acc / counts per label (a label no case holds: zeros, as the reference leaves it), then
        scipy.ndimage.gaussian_filter(sigma) per label ('reflect', truncate 4; fp32 weights, fp64 accumulation);
        sigma None or 0: no filter. fp32 [L, s0, s1, s2]; the builder stays usable for more add calls."""
        if self.acc is None:
            raise U3DError("AtlasBuilder.finish: no ROCm device (no CPU fallback)")
        L, (s0, s1, s2) = self.num_labels, self.shape
        cur = torch.empty_like(self.acc)
        with torch.cuda.device(self.device):
            call("u3d_atlas_build_normalize", self.acc.data_ptr(), self.counts.data_ptr(), L, s0 * s1 * s2,
                 cur.data_ptr(), ops._stream())
            if sigma:
                w, r = gaussian_kernel1d(sigma)
                wt = torch.from_numpy(w).to(self.device)
                nxt = torch.empty_like(cur)
                for outer, n, inner in ((L, s0, s1 * s2), (L * s0, s1, s2), (L * s0 * s1, s2, 1)):
                    call("u3d_aug_blur_axis", cur.data_ptr(), nxt.data_ptr(), outer, n, inner, wt.data_ptr(), r,
                         ops._stream())
                    cur, nxt = nxt, cur
        return cur


def build_atlas(labels, shape=None, num_labels=15, sigma=3.0):
    """atlas_gen_mm.py:100-145 on an iterable of device label volumes [H, W, D]: shape None takes their
    average_shape (the iterable is then held as a list). Returns the fp32 atlas [num_labels, s0, s1, s2], ready for
    crop_patch(..., atlas=atlas[:13]). Reading the files and choosing the training cases stay with the caller."""
    if shape is None:
        labels = list(labels)
        shape = average_shape([lab.shape for lab in labels])
    builder = None
    for lab in labels:
        ops.require_device(lab)
        if builder is None:
            builder = AtlasBuilder(shape, num_labels, lab.device)
        builder.add(lab)
    if builder is None:
        raise ValueError("build_atlas: no label volumes")
    return builder.finish(sigma)


# ------------------------------------------------------------------------------------------------ body mask and crop
REC_LEN = 12                     # U3D_CCL_RECORD: {found, label, size, lo z y x, hi z y x, n, 0, 0}
ROUTE_COMPONENT, ROUTE_FALLBACK = 0, 1
_BBOX_DTYPES = {torch.uint8: 0, torch.float32: 1, torch.int32: 2}


def ccl_tile():
    """(tz, ty, tx): the tile one workgroup labels in LDS before the seams are joined."""
    import ctypes
    t = [ctypes.c_int(0) for _ in range(3)]
    query("u3d_ccl_tile", *(ctypes.byref(v) for v in t))
    return tuple(v.value for v in t)


def _volume3(x, what):
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError(f"{what}: {tuple(x.shape)} must be a non-empty [Z, Y, X] volume")
    ops.require_device(x)
    if x.numel() >= 2 ** 31:
        raise ValueError(f"{what}: {x.numel()} voxels (the labelling indexes voxels with int32: fewer than 2^31)")


def _mask_u8(mask):
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    return (mask != 0).view(torch.uint8).contiguous()


def _label(m8):
    """labels int32 [Z, Y, X] and the device int n of a uint8 mask; no host read."""
    Z, Y, X = m8.shape
    labels = torch.empty((Z, Y, X), dtype=torch.int32, device=m8.device)
    n = torch.empty(1, dtype=torch.int32, device=m8.device)
    ws = torch.empty(query("u3d_ccl_ws_bytes", m8.numel()), dtype=torch.uint8, device=m8.device)
    call("u3d_ccl_label", m8.data_ptr(), Z, Y, X, labels.data_ptr(), n.data_ptr(), ws.data_ptr(), ops._stream())
    return labels, n


def _select(labels, n, num_limit, min_filter):
    """(mask uint8, record int32[REC_LEN]) of getmaxcomponent on device labels; no host read."""
    if not 1 <= int(num_limit) <= 1024:
        raise ValueError(f"largest_component: num_limit={num_limit} must be in 1..1024")
    Z, Y, X = labels.shape
    out = torch.empty((Z, Y, X), dtype=torch.uint8, device=labels.device)
    rec = torch.empty(REC_LEN, dtype=torch.int32, device=labels.device)
    ws = torch.empty(query("u3d_ccl_select_ws_bytes"), dtype=torch.uint8, device=labels.device)
    call("u3d_ccl_select", labels.data_ptr(), Z, Y, X, n.data_ptr(), int(num_limit), float(min_filter), out.data_ptr(),
         rec.data_ptr(), ws.data_ptr(), ops._stream())
    return out, rec


def label_components(mask):
    """scipy.ndimage.label(mask) on the device: mask [Z, Y, X] of any dtype (nonzero = foreground) -> (labels int32
    [Z, Y, X], n). Face connectivity; components numbered 1..n in the C order of their first voxel. The int n is the
    one host read."""
    _volume3(mask, "label_components")
    with torch.cuda.device(mask.device):
        labels, n = _label(_mask_u8(mask))
        return labels, int(n.item())


def largest_component(mask, num_limit=10, min_filter=1e6):
    """forward_crop.py:37-59 (getmaxcomponent): among the components 1..num_limit-1 with at least min_filter voxels
    the largest, the earliest on a tie, as a uint8 mask; None when none qualifies (one host read of the record)."""
    _volume3(mask, "largest_component")
    with torch.cuda.device(mask.device):
        labels, n = _label(_mask_u8(mask))
        out, rec = _select(labels, n, num_limit, min_filter)
        return out if int(rec[0].item()) else None


def _window3(cur, size, dilate, gate):
    """Box erosion (AND) / dilation (OR) of a uint8 volume, one u3d_mask_window_axis pass per axis."""
    Z, Y, X = cur.shape
    lo, hi = -(size // 2), size - 1 - size // 2
    if dilate:
        lo, hi = -hi, -lo
    for outer, n, inner in ((1, Z, Y * X), (Z, Y, X), (Z * Y, X, 1)):
        nxt = torch.empty_like(cur)
        call("u3d_mask_window_axis", cur.data_ptr(), nxt.data_ptr(), outer, n, inner, lo, hi, 1 if dilate else 0, gate,
             ops._stream())
        cur = nxt
    return cur


def _get_body(volume, threshold_all, min_filter, fallback_threshold):
    """(mask uint8, record): the record's found says which route produced the mask; size, lo, hi describe the mask of
    either route. Everything is queued on the stream; nothing is read."""
    vol = volume.float().contiguous()
    Z, Y, X = vol.shape
    s = ops._stream()
    m = torch.empty((Z, Y, X), dtype=torch.uint8, device=vol.device)
    call("u3d_body_threshold", vol.data_ptr(), Z, Y, X, float(threshold_all), 1, m.data_ptr(), None, s)
    labels, n = _label(m)
    out, rec = _select(labels, n, 100, min_filter)
    # the fallback (:76-80), gated on the device by rec[0] = found: no-ops when a component was chosen
    gate = rec.data_ptr()
    fb = float(threshold_all if fallback_threshold is None else fallback_threshold)
    call("u3d_body_threshold", vol.data_ptr(), Z, Y, X, fb, 0, m.data_ptr(), gate, s)
    opened = _window3(_window3(m, 10, False, gate), 10, True, gate)
    call("u3d_nonzero_bbox", opened.data_ptr(), 0, Z, Y, X, rec.data_ptr(), 1, gate, s)
    return out, opened, rec


def get_body(volume, threshold_all=-200, min_filter=1e6, fallback_threshold=None):
    """forward_crop.py:62-82: volume > threshold_all (strict, fp32, NaN false), eroded by a 2 x 2 x 2 box, then the
    largest of its first 99 components with at least min_filter voxels; when there is none, volume >
    fallback_threshold (default threshold_all; the reference reads its global there, equal in every call it makes)
    opened by a 10^3 box. uint8 [Z, Y, X]."""
    _volume3(volume, "get_body")
    with torch.cuda.device(volume.device):
        out, opened, rec = _get_body(volume, threshold_all, min_filter, fallback_threshold)
        return out if int(rec[0].item()) else opened


def _record(rec):
    r = rec.cpu().tolist()
    return {"found": bool(r[0]), "label": r[1], "size": r[2], "lo": tuple(r[3:6]), "hi": tuple(r[6:9]), "n": r[9]}


def _bbox_record(x):
    _volume3(x, "bounding_box")
    if x.dtype not in _BBOX_DTYPES:
        x = _mask_u8(x)
    x = x.contiguous()
    rec = torch.empty(REC_LEN, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        call("u3d_nonzero_bbox", x.data_ptr(), _BBOX_DTYPES[x.dtype], *x.shape, rec.data_ptr(), 0, None, ops._stream())
    return rec


def bounding_box(x):
    """((z0, y0, x0), (z1, y1, x1)) of the nonzero voxels of a [Z, Y, X] device tensor, max inclusive (one host read);
    ValueError when there is none, as np.min of an empty index list."""
    r = _record(_bbox_record(x))
    if r["size"] == 0:
        raise ValueError("bounding_box: no nonzero voxel")
    return r["lo"], r["hi"]


def body_threshold(cid):
    """forward_crop.py:166-172: 30000 for the case ids 540 and 518, 25 for other ids > 410 (MRI), -200 otherwise (CT)."""
    cid = int(cid)
    if cid in (540, 518):
        return 30000
    return 25 if cid > 410 else -200


def body_crop(image, label, cid, min_filter=1e6, min_filter_up=1e5):
    """forward_crop.py:148-207 on device tensors image / label [Z, Y, X]: label codes >= 14 cleared; image and label
    cropped along x to the label's range (margin 1); the body of the image (get_body at body_threshold(cid)) and its
    bounding box with margin 3; the body of the upper half image[:, :, :w // 2 + 10] (min_filter_up) and its z range
    with margin 5; when the full body is more than 30 planes longer in z than the upper half's and cid > 500 ("find
    hand"), the z slice [zmin_up:zmax_up] of the already cropped arrays, as the reference applies it.
    Returns (image_a, label_a, info): slices of image and of the cleared label; info holds label_range, bbox, bbox_up
    (min, inclusive max), size, size_up, route, route_up (ROUTE_COMPONENT / ROUTE_FALLBACK), inter_all, inter_up,
    found_hand, mask (the body mask as the reference leaves it), label_sum_before / _after (0-dim device tensors: the
    reference's consistency print), origin ((z, y, x) of image_a[0, 0, 0] in the volume passed in: the three nested
    crops added up) and input_shape (that volume's shape): what restore_prediction needs to undo the crop. Three host
    reads: the label range and the two body records. An empty label or an
    empty body raises ValueError."""
    _volume3(image, "body_crop")
    _volume3(label, "body_crop")
    if image.shape != label.shape or image.device != label.device:
        raise ValueError(f"body_crop: image {tuple(image.shape)} on {image.device}, label {tuple(label.shape)} on "
                         f"{label.device}")
    input_shape = tuple(image.shape)
    with torch.cuda.device(image.device):
        label = torch.where(label >= 14, torch.zeros((), dtype=label.dtype, device=label.device), label)
        sum_before = label.double().sum()
        lr = _record(_bbox_record(label))                                            # host read 1
        if lr["size"] == 0:
            raise ValueError("body_crop: the label has no voxel in 1..13")
        xmin, xmax = max(0, lr["lo"][2] - 1), lr["hi"][2] + 1
        image, label = image[:, :, xmin:xmax], label[:, :, xmin:xmax]
        thre = body_threshold(cid)
        comp, opened, rec = _get_body(image, thre, min_filter, None)
        r = _record(rec)                                                             # host read 2
        if r["size"] == 0:
            raise ValueError("body_crop: the body mask is empty")
        mask = comp if r["found"] else opened
        zmin, ymin, x0 = (max(0, v - 3) for v in r["lo"])
        zmax, ymax, x1 = (v + 3 for v in r["hi"])
        image_a, label_a = image[zmin:zmax, ymin:ymax, x0:x1], label[zmin:zmax, ymin:ymax, x0:x1]
        comp_up, opened_up, rec_up = _get_body(image[:, :, :image_a.shape[2] // 2 + 10], thre, min_filter_up, None)
        u = _record(rec_up)                                                          # host read 3
        if u["size"] == 0:
            raise ValueError("body_crop: the body mask of the upper half is empty")
        zmin_up, zmax_up = max(0, u["lo"][0] - 5), u["hi"][0] + 5
        inter_all, inter_up = zmax - zmin, zmax_up - zmin_up
        hand = inter_all - inter_up > 30 and int(cid) > 500
        if hand:
            image_a, label_a, mask = image_a[zmin_up:zmax_up], label_a[zmin_up:zmax_up], mask[zmin_up:zmax_up]
        info = {"label_range": (xmin, xmax), "bbox": (r["lo"], r["hi"]), "bbox_up": (u["lo"], u["hi"]),
                "size": r["size"], "size_up": u["size"],
                "route": ROUTE_COMPONENT if r["found"] else ROUTE_FALLBACK,
                "route_up": ROUTE_COMPONENT if u["found"] else ROUTE_FALLBACK,
                "inter_all": inter_all, "inter_up": inter_up, "found_hand": bool(hand), "mask": mask,
                "origin": (zmin + (zmin_up if hand else 0), ymin, xmin + x0), "input_shape": input_shape,
                "label_sum_before": sum_before, "label_sum_after": label_a.double().sum()}
        return image_a, label_a, info


# ------------------------------------------------------------------------------------- orientation and spacing
AXIS_CODES = (("L", "R"), ("P", "A"), ("I", "S"))        # world axis -> (code of its negative, of its positive end)
RS_U8, RS_I16, RS_I32, RS_F32 = 0, 1, 2, 3               # U3D_RS_* (include/u3d.h)
_RS_DTYPES = {torch.uint8: RS_U8, torch.int16: RS_I16, torch.int32: RS_I32, torch.float32: RS_F32}


def _affine44(affine):
    a = np.array(affine.detach().cpu().numpy() if isinstance(affine, torch.Tensor) else affine, dtype=np.float64)
    if a.shape != (4, 4) or not np.isfinite(a).all():
        raise ValueError(f"affine: a finite 4 x 4 matrix is needed, got shape {a.shape}")
    if np.linalg.matrix_rank(a[:3, :3]) < 3:
        raise ValueError("affine: the 3 x 3 block is singular")
    return a


def orientation_of(affine):
    """nibabel's io_orientation: ((out_axis, sign), ...) per index axis of a 4 x 4 index-to-world affine (RAS+): the
    world axis each index axis runs closest to, and in which direction. Columns divided by their norms (a zero norm
    counts as 1), R = P[:, keep] @ Qs[keep] of their SVD with keep = S > S.max() * 3 * eps, then greedily for the axes
    0, 1, 2: out_axis = argmax |R[:, ax]|, its sign, and row out_axis of R zeroed."""
    a = _affine44(affine)
    rzs = a[:3, :3]
    zooms = np.sqrt(np.sum(rzs * rzs, axis=0))
    zooms[zooms == 0] = 1
    rs = rzs / zooms
    P, S, Qs = np.linalg.svd(rs, full_matrices=False)
    keep = S > S.max() * 3 * np.finfo(S.dtype).eps
    R = np.dot(P[:, keep], Qs[keep])
    out = []
    for ax in range(3):
        col = R[:, ax]
        o = int(np.argmax(np.abs(col)))
        out.append((o, -1 if col[o] < 0 else 1))
        R[o, :] = 0
    if sorted(o for o, _ in out) != [0, 1, 2]:
        raise ValueError("affine: the index axes do not map onto three different world axes")
    return tuple(out)


def axcodes_of(affine):
    """The orientation as axis codes, e.g. "LPS": per index axis the end of the world axis it runs towards."""
    return "".join(AXIS_CODES[o][(s + 1) // 2] for o, s in orientation_of(affine))


def _target_orientation(axcodes):
    codes = tuple(str(axcodes).upper()) if isinstance(axcodes, str) else tuple(str(c).upper() for c in axcodes)
    out = []
    for c in codes:
        hit = [(w, 2 * e - 1) for w, pair in enumerate(AXIS_CODES) for e in (0, 1) if pair[e] == c]
        if not hit:
            raise ValueError(f"axcodes {axcodes!r}: unknown code {c!r} (L R P A I S)")
        out.append(hit[0])
    if len(out) != 3 or sorted(w for w, _ in out) != [0, 1, 2]:
        raise ValueError(f"axcodes {axcodes!r}: three codes, one per world axis, are needed")
    return out


class GridPlan:
    """A separable resampling between two voxel grids: output axis i reads source axis perm[i] at the coordinate
    c(k) = clip(scale[i] * k + offset[i], 0, n - 1) (n = src_shape[perm[i]]), mirrored to n - 1 - c when flip[i].
    ``tables[i]`` = (i0 int32, frac float64, near int32) over the out_shape[i] output indices, in indices of the source
    axis as stored (the flip is inside them). On the reoriented axis the taps are (j0, j1 = min(j0 + 1, n - 1)) with
    j0 = min(floor(c), max(n - 2, 0)) and the weight f = c - j0 on j1, the nearest index rint(c), half to even
    (grid_sample's rule). Stored:
        not flipped   i0 = j0,          frac = f,      near = rint(c)
        flipped       i0 = n - 1 - j1,  frac = 1 - f,  near = n - 1 - rint(c)
    so the kernel's pair (i0, min(i0 + 1, n - 1)) is the same two voxels with the same weights either way
    (the nearest index is rounded before the mirror, as a flip followed by grid_sample rounds it). src_affine /
    out_affine: the index-to-world affines of the two grids. ``apply`` runs the kernels, ``inverse`` gives the way
    back."""

    def __init__(self, src_shape, out_shape, perm, flip, scale, offset, src_affine, out_affine):
        self.src_shape = tuple(int(v) for v in src_shape)
        self.out_shape = tuple(int(v) for v in out_shape)
        self.perm = tuple(int(v) for v in perm)
        self.flip = tuple(bool(v) for v in flip)
        self.scale = tuple(float(v) for v in scale)
        self.offset = tuple(float(v) for v in offset)
        self.src_affine = np.array(src_affine, dtype=np.float64)
        self.out_affine = np.array(out_affine, dtype=np.float64)
        if len(self.src_shape) != 3 or len(self.out_shape) != 3 or min(self.src_shape + self.out_shape) < 1:
            raise ValueError(f"GridPlan: shapes {self.src_shape} -> {self.out_shape} must be three positive sizes each")
        if sorted(self.perm) != [0, 1, 2]:
            raise ValueError(f"GridPlan: perm {self.perm} is no permutation of the axes")
        if not all(np.isfinite(v) for v in self.scale + self.offset) or any(v == 0 for v in self.scale):
            raise ValueError(f"GridPlan: scale {self.scale} / offset {self.offset} must be finite, scale nonzero")
        self.tables = tuple(self._axis_tables(i) for i in range(3))
        self._dev = {}

    def source_coordinate(self, i, k):
        """The clamped coordinate of output indices k of axis i along the (reoriented) source axis, float64."""
        n = self.src_shape[self.perm[i]]
        c = np.float64(self.scale[i]) * np.asarray(k, dtype=np.float64) + np.float64(self.offset[i])
        return np.clip(c, 0.0, np.float64(n - 1))

    def _axis_tables(self, i):
        n = self.src_shape[self.perm[i]]
        c = self.source_coordinate(i, np.arange(self.out_shape[i]))
        i0 = np.minimum(np.floor(c), np.float64(max(n - 2, 0)))
        frac, near = c - i0, np.rint(c)
        if self.flip[i]:                       # the mirrored pair: its lower index is the mirror of the upper tap
            i0 = np.float64(n - 1) - np.minimum(i0 + 1, np.float64(n - 1))
            frac, near = 1.0 - frac, np.float64(n - 1) - near
        return i0.astype(np.int32), frac, near.astype(np.int32)

    @property
    def identity(self):
        return (self.src_shape == self.out_shape and self.perm == (0, 1, 2) and not any(self.flip)
                and self.scale == (1.0, 1.0, 1.0) and self.offset == (0.0, 0.0, 0.0))

    def inverse(self):
        """The plan from this plan's output grid back onto its source grid (out_shape = src_shape): what carries a
        prediction made on the resampled volume to the case's own voxels."""
        perm, scale, offset = [0] * 3, [0.0] * 3, [0.0] * 3
        for i in range(3):
            n = self.src_shape[self.perm[i]]
            se, oe = (-self.scale[i], (n - 1) - self.offset[i]) if self.flip[i] else (self.scale[i], self.offset[i])
            a = self.perm[i]                   # source index j of axis a = se * k + oe  <=>  k = j / se - oe / se
            perm[a], scale[a], offset[a] = i, 1.0 / se, 0.0 - oe / se
        return GridPlan(self.out_shape, self.src_shape, perm, (False,) * 3, scale, offset, self.out_affine,
                        self.src_affine)

    def source_layout(self):
        """(strides, lengths) of the source axis each output axis reads, in elements of a contiguous [C, A0, A1, A2]
        source, and the channel stride: what the entry points take next to the tables."""
        A = self.src_shape
        st = (A[1] * A[2], A[2], 1)
        return tuple(st[p] for p in self.perm), tuple(A[p] for p in self.perm), A[0] * A[1] * A[2]

    def _device_tables(self, device):
        key = (device.type, device.index)
        if key not in self._dev:
            self._dev[key] = tuple(tuple(torch.from_numpy(np.ascontiguousarray(t)).to(device) for t in ax)
                                   for ax in self.tables)
        return self._dev[key]

    def apply(self, x, mode="linear"):
        """x [A0, A1, A2] or [C, A0, A1, A2] on the device (A = src_shape) -> the same with out_shape. mode "linear":
        fp32 or int16 in (anything else is cast to fp32 first), fp32 out, trilinear in fp64 rounded once
        (u3d_grid_resample_linear); mode "nearest": uint8, int16, int32 or fp32, same dtype out
        (u3d_grid_resample_nearest). An identity plan returns x itself."""
        import ctypes
        if mode not in ("linear", "nearest"):
            raise ValueError(f"GridPlan.apply: mode {mode!r} (linear or nearest)")
        if x.dim() not in (3, 4) or tuple(x.shape[-3:]) != self.src_shape or x.numel() == 0:
            raise ValueError(f"GridPlan.apply: x {tuple(x.shape)} must be [A0, A1, A2] or [C, A0, A1, A2] with the "
                             f"plan's source shape {self.src_shape}")
        ops.require_device(x)
        if self.identity:
            return x
        if mode == "linear" and x.dtype not in (torch.float32, torch.int16):
            x = x.float()
        if x.dtype not in _RS_DTYPES:
            raise ValueError(f"GridPlan.apply: dtype {x.dtype} with mode {mode!r} (uint8, int16, int32 or float32)")
        x = x.contiguous()
        C = x.shape[0] if x.dim() == 4 else 1
        st, sn, chan = self.source_layout()
        arr_l, arr_i = ctypes.c_longlong * 3, ctypes.c_int * 3
        strides, src_n, n_out = arr_l(*st), arr_i(*sn), arr_i(*self.out_shape)
        out_shape = ((C,) if x.dim() == 4 else ()) + self.out_shape
        with torch.cuda.device(x.device):
            tabs = self._device_tables(x.device)
            if mode == "linear":
                out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
                call("u3d_grid_resample_linear", x.data_ptr(), _RS_DTYPES[x.dtype], C, strides, chan,
                     src_n, n_out, *(tabs[i][0].data_ptr() for i in range(3)),
                     *(tabs[i][1].data_ptr() for i in range(3)), out.data_ptr(), ops._stream())
            else:
                out = torch.empty(out_shape, dtype=x.dtype, device=x.device)
                call("u3d_grid_resample_nearest", x.data_ptr(), _RS_DTYPES[x.dtype], C, strides, chan,
                     src_n, n_out, *(tabs[i][2].data_ptr() for i in range(3)), out.data_ptr(), ops._stream())
        return out

    def restrict_source(self, origin, shape):
        """(plan_w, valid) for a source of which only the box [origin, origin + shape) exists, as a contiguous crop:
        plan_w reads that crop (src_shape = shape, the same perm and scale, offset[i] - origin[perm[i]]); valid[i] =
        (lo, hi), the output indices of axis i whose nearest source index in THIS plan (the near table: rint of the
        clamped coordinate) lies inside the box; coordinates are monotone, so it is one range, (0, 0) when empty. The
        range is taken from this plan's table, not from plan_w's: rint(c - o) is not rint(c) - o for a half-integer c
        and an odd o (half to even). For a plan without flips (an inverse plan has none); ValueError otherwise, or
        when the box is not inside src_shape."""
        origin, shape = tuple(int(v) for v in origin), tuple(int(v) for v in shape)
        if any(self.flip):
            raise ValueError(f"GridPlan.restrict_source: the plan flips {self.flip}; restrict a plan without flips")
        if len(origin) != 3 or len(shape) != 3 or any(
                o < 0 or s < 1 or o + s > n for o, s, n in zip(origin, shape, self.src_shape)):
            raise ValueError(f"GridPlan.restrict_source: the box at {origin} of shape {shape} is not inside the "
                             f"source {self.src_shape}")
        src_affine = self.src_affine.copy()
        src_affine[:3, 3] += self.src_affine[:3, :3] @ np.array(origin, dtype=np.float64)
        plan_w = GridPlan(shape, self.out_shape, self.perm, self.flip, self.scale,
                          tuple(self.offset[i] - origin[self.perm[i]] for i in range(3)), src_affine, self.out_affine)
        valid = []
        for i in range(3):
            a = self.perm[i]
            near = self.tables[i][2]
            inside = np.flatnonzero((near >= origin[a]) & (near < origin[a] + shape[a]))
            valid.append((int(inside[0]), int(inside[-1]) + 1) if inside.size else (0, 0))
        return plan_w, tuple(valid)

    def apply_argmax(self, x, valid=None):
        """x [C, A0, A1, A2] float on the device (A = src_shape, 1 <= C <= 256) -> uint8 [out_shape]: the argmax over
        the channels of apply(x, "linear"), bit for bit (ties to the lowest channel, a NaN is the maximum, the first
        wins), without forming the C resampled volumes (u3d_grid_resample_argmax). valid: per output axis (lo, hi); a
        voxel with an index outside a range gets 0 (default: everything is valid). x is read through its own strides:
        a permuted view costs no copy (zero strides are made contiguous first); dtypes other than fp32 are cast. An
        identity plan runs the same kernel with all weights 0: the plain channel argmax of finite values."""
        import ctypes
        if x.dim() != 4 or tuple(x.shape[1:]) != self.src_shape or not 1 <= x.shape[0] <= 256:
            raise ValueError(f"GridPlan.apply_argmax: x {tuple(x.shape)} must be [C, A0, A1, A2] with 1 <= C <= 256 and "
                             f"the plan's source shape {self.src_shape}")
        if not x.dtype.is_floating_point:
            raise ValueError(f"GridPlan.apply_argmax: dtype {x.dtype} (a float tensor of scores is needed)")
        ops.require_device(x)
        valid = tuple((0, n) for n in self.out_shape) if valid is None else tuple(
            (int(lo), int(hi)) for lo, hi in valid)
        if len(valid) != 3:
            raise ValueError(f"GridPlan.apply_argmax: valid {valid!r} must hold one (lo, hi) per output axis")
        if x.dtype != torch.float32:
            x = x.float()
        if min(x.stride()) <= 0:
            x = x.contiguous()
        xs = x.stride()
        arr_l, arr_i = ctypes.c_longlong * 3, ctypes.c_int * 3
        strides = arr_l(*(xs[1 + p] for p in self.perm))
        src_n, n_out = arr_i(*(self.src_shape[p] for p in self.perm)), arr_i(*self.out_shape)
        lo, hi = arr_i(*(v[0] for v in valid)), arr_i(*(v[1] for v in valid))
        with torch.cuda.device(x.device):
            tabs = self._device_tables(x.device)
            out = torch.empty(self.out_shape, dtype=torch.uint8, device=x.device)
            call("u3d_grid_resample_argmax", x.data_ptr(), x.shape[0], strides, xs[0], src_n, n_out,
                 *(tabs[i][0].data_ptr() for i in range(3)), *(tabs[i][1].data_ptr() for i in range(3)), lo, hi,
                 out.data_ptr(), ops._stream())
        return out


def spacing_plan(shape, affine, pixdim=(1, 1, 2), axcodes="RAS", out_shape=None):
    """MONAI's Orientationd(axcodes) then Spacingd(pixdim) (defaults: diagonal False, scale_extent False, padding
    "border") of a volume [A0, A1, A2] in file index order with the 4 x 4 index-to-world affine (RAS+), as a GridPlan.
    Orientation: output axis i takes the source axis perm[i] that runs along world axis axcodes[i], reversed (flip[i])
    when it runs the other way; the affine becomes affine @ M, M the index map of that permutation and flip (a flipped
    axis of length n carries the translation n - 1). Spacing, per axis of the reoriented volume: s = the column norm,
    p = pixdim[i] (None keeps s), r = p / s, n_out = int(np.round((n - 1) * s / p + 1)) (half to even; ``out_shape``
    overrides it), source coordinate c(k) = clip(k * r, 0, n - 1), output affine = columns scaled by r, translation kept:
    output voxel 0 sits on reoriented voxel 0. The sampling is pinned to grid_sample's arithmetic, n_out to this closed
    form: MONAI takes it through a matrix inverse, and where (n - 1) * s / p + 1 is a half-integer its rounding follows
    floating-point noise; pass out_shape= to match a file it wrote."""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"spacing_plan: shape {shape} must be three positive sizes")
    a = _affine44(affine)
    pix = tuple(pixdim) if np.ndim(pixdim) else (pixdim,) * 3
    if len(pix) != 3:
        raise ValueError(f"spacing_plan: pixdim {pixdim!r} must be one or three values")
    for p in pix:
        if p is not None and not (np.isfinite(p) and p > 0):
            raise ValueError(f"spacing_plan: pixdim {pixdim!r} must be finite and positive")
    src = orientation_of(a)
    perm, flip = [], []
    for w, sign in _target_orientation(axcodes):
        ax = [i for i, (o, _) in enumerate(src) if o == w][0]
        perm.append(ax)
        flip.append(src[ax][1] != sign)
    M = np.zeros((4, 4), dtype=np.float64)
    M[3, 3] = 1
    for i in range(3):
        M[perm[i], i] = -1.0 if flip[i] else 1.0
        M[perm[i], 3] = shape[perm[i]] - 1 if flip[i] else 0.0
    re = a @ M
    scale, n_out = [], []
    out_affine = re.copy()
    for i in range(3):
        n = shape[perm[i]]
        s = np.sqrt(np.sum(re[:3, i] * re[:3, i]))
        p = s if pix[i] is None else np.float64(pix[i])
        r = p / s
        scale.append(r)
        n_out.append(int(np.round((n - 1) * s / p + 1)))
        out_affine[:3, i] = re[:3, i] * r
    if out_shape is not None:
        n_out = [int(v) for v in out_shape]
        if len(n_out) != 3 or min(n_out) < 1:
            raise ValueError(f"spacing_plan: out_shape {out_shape!r} must be three positive sizes")
    return GridPlan(shape, n_out, perm, flip, scale, (0.0, 0.0, 0.0), a, out_affine)


def resample_spacing(image, label, affine, pixdim=(1, 1, 2), axcodes="RAS"):
    """preprocess/transforms.py:47-52 on device tensors image / label [A0, A1, A2] of one case: to ``axcodes`` and to
    ``pixdim``, the image trilinear (fp32 out, from fp32 or int16), the label nearest (its own dtype). Returns
    (image, label, out_affine, plan); plan.inverse() carries a prediction back."""
    if image.shape != label.shape or image.device != label.device:
        raise ValueError(f"resample_spacing: image {tuple(image.shape)} on {image.device}, label "
                         f"{tuple(label.shape)} on {label.device}")
    ops.require_device(image)
    plan = spacing_plan(image.shape, affine, pixdim, axcodes)
    img = plan.apply(image, "linear")
    return (img if img.dtype == torch.float32 else img.float()), plan.apply(label, "nearest"), plan.out_affine, plan


def preprocess_case(image, label, affine, cid, pixdim=(1, 1, 2), axcodes="RAS", min_filter=1e6, min_filter_up=1e5):
    """preprocess/forward_crop.py:121-207 for one case on the device: resample_spacing, then body_crop (which clears the
    label codes >= 14). Returns body_crop's (image_a, label_a, info); info gains ``affine`` (of the resampled grid,
    before the crops), ``spacing`` (= pixdim) and ``plan``."""
    img, lab, out_affine, plan = resample_spacing(image, label, affine, pixdim, axcodes)
    image_a, label_a, info = body_crop(img, lab, cid, min_filter, min_filter_up)
    info.update(affine=out_affine, spacing=tuple(pixdim) if np.ndim(pixdim) else (pixdim,) * 3, plan=plan)
    return image_a, label_a, info


# ------------------------------------------------------------------------------- predictions on the case's own grid
KEEP_REC = 4                     # U3D_KEEP_RECORD: {components, voxels, kept voxels, first voxel of the kept component}


def keep_largest_per_label(labels, num_labels=13, return_record=False):
    """The per-organ cleanup every AMOS pipeline runs before it writes a label file, in one labelling
    (u3d_ccl_keep_largest): labels [Z, Y, X] uint8, or int16 / int32 / int64 with values in 0..255, on the device. For
    each label 1..num_labels (at most 255) the face-connected component with the most voxels is kept, on a tie the one
    whose first voxel comes first in C order; the label's other voxels become 0; 0 and codes above num_labels stay.
    Returns a tensor of the input's dtype and shape, with return_record also the device int32 [num_labels, 4] of
    {components, voxels, kept voxels, linear index of the kept component's first voxel (-1: label absent)}. No host
    read."""
    if labels.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f"keep_largest_per_label: dtype {labels.dtype} (uint8, int16, int32 or int64)")
    if not 1 <= int(num_labels) <= 255:
        raise ValueError(f"keep_largest_per_label: num_labels={num_labels} must be in 1..255")
    _volume3(labels, "keep_largest_per_label")
    codes = labels.to(torch.uint8).contiguous()
    Z, Y, X = codes.shape
    with torch.cuda.device(codes.device):
        out = torch.empty_like(codes)
        rec = torch.empty((int(num_labels), KEEP_REC), dtype=torch.int32, device=codes.device)
        ws = torch.empty(query("u3d_ccl_keep_largest_ws_bytes", codes.numel()), dtype=torch.uint8, device=codes.device)
        call("u3d_ccl_keep_largest", codes.data_ptr(), Z, Y, X, int(num_labels), out.data_ptr(), rec.data_ptr(),
             ws.data_ptr(), ops._stream())
    out = out if labels.dtype == torch.uint8 else out.to(labels.dtype)
    return (out, rec) if return_record else out


def restore_prediction(pred, info, cleanup=False, num_labels=13):
    """A prediction made on the grid of preprocess_case's image_a, carried to the case's own voxels: uint8
    [info["plan"].src_shape], the file's index order. pred [C, z, y, x] float (logits or probabilities): the crop is
    undone and the resampling inverted in one pass, plan.inverse().restrict_source(info["origin"], image_a's shape) and
    apply_argmax: the scores are interpolated, then decided, and a voxel whose nearest voxel of the resampled grid lies
    outside the crop is 0. pred [z, y, x] integer (a label map, values 0..255): zero-padded to the resampled grid and
    sent through the nearest kernel with the whole inverse plan. cleanup: keep_largest_per_label(result, num_labels)."""
    plan = info["plan"]
    origin = tuple(int(v) for v in info["origin"])
    inv = plan.inverse()
    ops.require_device(pred)
    if pred.dim() == 4 and pred.dtype.is_floating_point:
        plan_w, valid = inv.restrict_source(origin, pred.shape[1:])
        out = plan_w.apply_argmax(pred, valid)
    elif pred.dim() == 3 and not pred.dtype.is_floating_point and pred.dtype != torch.bool:
        if any(o + s > n for o, s, n in zip(origin, pred.shape, plan.out_shape)):
            raise ValueError(f"restore_prediction: pred {tuple(pred.shape)} at {origin} is not inside the resampled grid "
                             f"{plan.out_shape}")
        full = torch.zeros(plan.out_shape, dtype=torch.uint8, device=pred.device)
        full[tuple(slice(o, o + s) for o, s in zip(origin, pred.shape))] = pred.to(torch.uint8)
        out = inv.apply(full, "nearest")
    else:
        raise ValueError(f"restore_prediction: pred {tuple(pred.shape)} {pred.dtype} must be [C, z, y, x] float scores "
                         "or a [z, y, x] integer label map")
    return keep_largest_per_label(out, num_labels) if cleanup else out
