"""The reference's IDRiD patch cache: producer and reader.

Producer (``IDRIDDataset``, ``precompute_all_patches``): the reference's
``utils/data_loading.py:42-446`` in patch mode.  Each image / lesion mask pair
is loaded and scaled with PIL exactly as the reference does (``load_image``
:18-28, ``preprocess`` :580-601: bicubic image, nearest mask, /255, mask > 0),
then every stride-P/2 window is decided in ONE device launch per image
(``vu_patch_stats``: black-pixel and lesion-pixel counts of every window, the
reference's per-window Python loop with ``is_valid_patch`` :287-300 and
``has_lesion`` :381), and the kept windows are written in the reference's
record format and file names (:383-389), with the train split's
positive/negative balancing and deletion of the unselected negatives
(:404-446; ``random.shuffle`` of the global generator, or a given one).
Full-image mode (``patch_size=None``: fundus detection with cv2,
:223-285, 448-578) is not built: cv2 is absent here, so it cannot be pinned.

The reference slices every training image into overlapping patches and
caches each one with ``torch.save({'image': [3,P,P] f32, 'mask': [1,P,P] f32,
'coords': (y, x), 'has_lesion': bool})`` (utils/data_loading.py:302-446); its
``__getitem__`` reads one file (603-616), a 6-worker DataLoader collates a
batch on the host (train.py:111-134, 239-248) and the training loop copies
it to the device as channels_last (train.py:382-383).

``PatchCache`` reads the same files (``torch.load(weights_only=True)``: no
code is unpickled) with a thread pool, stages each batch in pinned host
memory, copies it to the GPU on a side stream (overlapping the step that is
running) and augments it on the device.  ``augment=True`` applies the
flip / rot90 part of the reference's training transform
(utils/data_loading.py:116-120: HorizontalFlip, VerticalFlip, RandomRotate90,
each p = 0.5, applied to image and mask alike) in one integer gather launch
per tensor (``vu_gather_affine``).  ``augment=TrainAugment(...)`` applies the
whole device-side transform in ONE launch per batch (``vu_augment_patch``,
DESIGN.md §4.8): flips, rot90, small-angle affine and grid distortion as one
resampling of image (bilinear) and mask (nearest), then gamma, brightness /
contrast / saturation / hue as one colour matrix, Gaussian noise (Philox) and
the clip to [0, 1].  The reference takes these from albumentations
(:121-178), which is absent here, so the transforms are defined in §4.8 and
their ranges are ``TrainAugment``'s arguments: unpinned vs the reference.
CLAHE (``clahe``: per-tile histograms of an integer luma, then a per-pixel
blend of four lookup tables) and blur (``blur``: a separable symmetric kernel
of radius <= 7, Gaussian or box rows from ``blur_weights``) are launches of
their own ahead of that one, so both see the un-warped patch
and the noise stays white; ``TrainAugment(p_clahe=, p_blur=)`` draws them per
sample.  The median blur (``median_blur``: per channel, window 3, 5 or 7 per
sample, replicated border) is one more launch between the blur
and the warp, bitwise a selection of its inputs; ``TrainAugment(p_median=)``
draws it.  Their definitions are this project's too; the LAB-space CLAHE is
not built.
Normalize(mean=0, std=1) of train.py:37 is the identity.
"""
import logging
import os
import random
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from . import kernels as K
from ._lib import F32, VU_MEDIAN_RMAX

CL = torch.channels_last


# ----------------------------------------------------------------------------
# producer
# ----------------------------------------------------------------------------
def load_image(filename):
    """utils/data_loading.py:18-28: open with PIL and force 3-channel RGB."""
    from PIL import Image
    return Image.open(filename).convert("RGB")


def preprocess(pil_img, scale, is_mask):
    """utils/data_loading.py:580-601: resize to int(scale * size) (nearest for
    masks, bicubic for images); mask -> {0, 1} float32 [H, W], image ->
    float32 [3, H, W] in [0, 1]."""
    from PIL import Image
    w, h = pil_img.size
    nw, nh = int(scale * w), int(scale * h)
    if nw < 1 or nh < 1:
        raise ValueError(f"Image {pil_img} scaled too small => {nw}x{nh}.")
    arr = np.asarray(pil_img.resize((nw, nh), resample=Image.NEAREST if is_mask else Image.BICUBIC))
    if is_mask:
        return ((arr[..., 0] if arr.ndim == 3 else arr) > 0).astype(np.float32)
    if arr.ndim == 2:
        arr = np.stack([arr] * 3, axis=-1)
    return (arr.astype(np.float32) / 255.0).transpose(2, 0, 1)


def window_stats(img, mask, patch, stride, device):
    """(ny, nx, black counts, lesion counts) of every stride-spaced window of
    img [C, H, W] / mask [1 or C', H, W] (CPU float32): one vu_patch_stats
    launch; the counts come back as int64 numpy arrays [ny * nx]."""
    _, h, w = img.shape
    ny = (h - patch) // stride + 1 if h >= patch else 0
    nx = (w - patch) // stride + 1 if w >= patch else 0
    if ny == 0 or nx == 0:
        return ny, nx, np.zeros(0, np.int64), np.zeros(0, np.int64)
    dimg = img.to(device, dtype=torch.float32).contiguous()
    dmsk = mask[0].to(device, dtype=torch.float32).contiguous()
    out = torch.empty(2, ny * nx, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        K.call("vu_patch_stats", K.ptr(dimg), img.shape[0], h, w, K.ptr(dmsk), patch, stride, ny, nx,
               K.ptr(out[0]), K.ptr(out[1]), K.stream())
    cnt = out.cpu().numpy().astype(np.int64)   # one D2H of 8 B per window
    return ny, nx, cnt[0], cnt[1]


def black_ratio_ok(black, patch, threshold):
    """is_valid_patch's test (data_loading.py:296-299): the fp32 mean of the
    per-pixel black flags (count / P^2, rounded to float32) <= threshold."""
    return float(np.float32(black) / np.float32(patch * patch)) <= threshold


def precompute_all_patches(ids, images_dir, masks_dir, patches_dir, split, scale, patch_size, lesion_type,
                           skip_border_check=False, rng=None, device="cuda"):
    """utils/data_loading.py:302-446 (patch mode): writes the cache files into
    ``patches_dir`` and returns the patch index [(img_id, path, has_lesion)]
    in the reference's order (positives in scan order, then the selected
    negatives for 'train'; every patch for 'val' / 'test')."""
    images_dir, masks_dir, patches_dir = Path(images_dir), Path(masks_dir), Path(patches_dir)
    rng = random if rng is None else rng
    threshold = 0.5 if split == "test" else 0.1
    positive_count, negative_paths, patch_index = 0, [], []
    stride = patch_size // 2
    for img_id in ids:
        img_file = images_dir / f"{img_id}.jpg"
        mask_file = masks_dir / lesion_type / f"{img_id}_{lesion_type}.tif"
        img_pil = load_image(img_file).convert("RGB")
        mask_pil = load_image(mask_file).convert("L")
        if img_pil.size != mask_pil.size:
            logging.warning(f"Mismatch in size for {img_file} vs {mask_file}; skipping.")
            continue
        img = torch.as_tensor(preprocess(img_pil, scale, False), dtype=torch.float32)
        msk = torch.as_tensor(preprocess(mask_pil, scale, True), dtype=torch.float32)
        if msk.dim() == 2:
            msk = msk.unsqueeze(0)
        if img.dim() == 2:
            img = img.unsqueeze(0)
        _, h, w = img.shape
        if h < patch_size or w < patch_size:
            logging.warning(f"{img_id}: scaled to {h}x{w} < patch_size={patch_size}; skipping.")
            continue
        ny, nx, black, lesion = window_stats(img, msk, patch_size, stride, device)
        count = 0
        for wi in range(ny * nx):
            y, x = (wi // nx) * stride, (wi % nx) * stride
            if not skip_border_check and img.shape[0] > 0 and not black_ratio_ok(black[wi], patch_size, threshold):
                continue
            has = bool(lesion[wi] > 0)
            path = patches_dir / f"{img_id}_{count}"
            torch.save({"image": img[:, y:y + patch_size, x:x + patch_size].contiguous(),
                        "mask": msk[:, y:y + patch_size, x:x + patch_size].contiguous(),
                        "coords": (y, x),
                        "has_lesion": torch.tensor(has)}, path)
            if has:
                positive_count += 1
                patch_index.append((img_id, str(path), True))
            else:
                negative_paths.append((img_id, str(path)))
            count += 1
    logging.info(f"Found {positive_count} positive patches and {len(negative_paths)} negative patches")
    if split == "train":
        rng.shuffle(negative_paths)
        patch_index += [(i, p, False) for i, p in negative_paths[:positive_count]]
        for _, p in negative_paths[positive_count:]:
            try:
                os.remove(p)
            except OSError as e:
                logging.warning(f"Error removing {p}: {e}")
        return patch_index
    index = patch_index + [(i, p, False) for i, p in negative_paths]
    if split == "test" and not index and positive_count == 0:
        index = [(i, p, False) for i, p in negative_paths[:min(10, len(negative_paths))]]
    return index


class IDRIDDataset(torch.utils.data.Dataset):
    """utils/data_loading.py:42-180 + 603-636 in patch mode: same constructor
    (plus ``ids`` to fix the image order — the reference takes
    ``os.listdir`` order —, ``rng`` for the balancing shuffle and the device
    of the window statistics), same cache directory
    (``base_dir/patches/split/lesion_type``, cleared first), same
    ``patch_indices`` and ``__getitem__`` records.  ``transform`` is None:
    the reference's albumentations pipeline is absent; augmentation runs on
    the device in ``PatchCache(augment=True | TrainAugment(...))``."""

    def __init__(self, base_dir, split="train", scale=0.25, patch_size=None, lesion_type="EX", max_images=None,
                 skip_border_check=False, ids=None, rng=None, device="cuda"):
        super().__init__()
        if patch_size is None:
            raise NotImplementedError("full-image mode needs cv2 fundus detection (data_loading.py:223-285), "
                                      "absent here: use patch_size")
        self.scale, self.split, self.patch_size = scale, split, patch_size
        self.base_dir = Path(base_dir)
        self.images_dir = self.base_dir / "imgs" / split
        self.masks_dir = self.base_dir / "masks" / split
        self.lesion_type = self.class_dir = lesion_type
        self.skip_border_check = skip_border_check
        self.is_full_image = False
        self.transform = None
        if ids is None:
            ids = [os.path.splitext(f)[0] for f in os.listdir(self.images_dir) if f.endswith(".jpg")]
            if max_images is not None:
                ids = ids[:max_images]
        ids = [i for i in ids if (self.masks_dir / lesion_type / f"{i}_{lesion_type}.tif").exists()]
        if not ids:
            raise RuntimeError(f"No valid image-mask pairs found in {self.images_dir} and {self.masks_dir}")
        self.ids = ids
        self.stride = patch_size // 2
        self.patches_dir = self.base_dir / "patches" / split / lesion_type
        if self.patches_dir.exists():
            import shutil
            shutil.rmtree(self.patches_dir)
        self.patches_dir.mkdir(parents=True, exist_ok=True)
        self.patch_indices = precompute_all_patches(ids, self.images_dir, self.masks_dir, self.patches_dir, split,
                                                    scale, patch_size, lesion_type, skip_border_check, rng, device)

    def __len__(self):
        return len(self.patch_indices)

    def __getitem__(self, idx):
        img_id, path, _ = self.patch_indices[idx]
        rec = load_patch(path)
        return {"image": rec["image"], "mask": rec["mask"], "img_id": img_id}

    def paths(self):
        """The cache files in index order (feed to PatchCache)."""
        return [p for _, p, _ in self.patch_indices]


# ----------------------------------------------------------------------------
# reader
# ----------------------------------------------------------------------------


def load_patch(path):
    """One cache record (utils/data_loading.py:605-612)."""
    return torch.load(path, map_location="cpu", weights_only=True)


def _flip_rot_map(P, hflip, vflip, k):
    """Integer map (y, x) of the SOURCE pixel for output (i, j) after
    HorizontalFlip -> VerticalFlip -> rot90(k) (numpy's counter-clockwise
    rot90, as albumentations), square P x P."""
    # start from the identity output->source map and undo the ops last-first
    # rot90 (CCW) once: out[i][j] = in[j][P-1-i]
    ay, by, cy = 1, 0, 0     # y_src = ay*i + by*j + cy
    ax, bx, cx = 0, 1, 0     # x_src = ax*i + bx*j + cx
    for _ in range(k % 4):
        # out[i][j] = prev[j][P-1-i]: substitute (i, j) -> (j, P-1-i) into prev's map
        ay, by, cy, ax, bx, cx = -by, ay, cy + by * (P - 1), -bx, ax, cx + bx * (P - 1)
    if vflip:
        ay, by, cy = -ay, -by, (P - 1) - cy
    if hflip:
        ax, bx, cx = -ax, -bx, (P - 1) - cx
    return [ay, by, cy, ax, bx, cx]


# ----------------------------------------------------------------------------
# training augmentation: host-side parameters, one launch
# ----------------------------------------------------------------------------
NPARAM = 20                       # a0..a5, gamma, M (9), o (3), sigma
MAX_GRID_STEPS = 32
RMAX = 7                          # largest blur radius
NBLUR = 2 + RMAX                  # a blur row: r, w_0..w_RMAX
MAX_TILES = 16                    # CLAHE tiles per axis
MEDIAN_RMAX = VU_MEDIAN_RMAX      # largest median radius: window 7
BORDERS = {"constant": 0, "reflect101": 1}

_GREY = np.array([0.299, 0.587, 0.114])
_YIQ = np.array([[0.299, 0.587, 0.114], [0.5959, -0.2746, -0.3213], [0.2115, -0.5227, 0.3112]])
# generator of the rotation about the grey axis, in RGB: inv(YIQ) [[0,0,0],[0,0,-1],[0,1,0]] YIQ
_HUE_J = np.linalg.inv(_YIQ) @ np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]) @ _YIQ
_ROT90 = np.array([[0.0, -1.0], [1.0, 0.0]])   # one np.rot90 as an output -> source map of centred (x, y)


def affine_matrix(H, W, hflip=False, vflip=False, k=0, angle=0.0, scale=1.0, shift=(0.0, 0.0)):
    """The six fp32 values (a0..a5) of the output -> source map sx = a0 x + a1 y
    + a2, sy = a3 x + a4 y + a5 of: HorizontalFlip, VerticalFlip, rot90(k)
    (numpy's counter-clockwise), then a rotation by ``angle`` degrees, an
    isotropic zoom by ``scale`` and a shift by ``shift`` = (fraction of W,
    fraction of H), everything about the patch centre ((W-1)/2, (H-1)/2).
    The last step reads source = R(angle) (output - shift) / scale in centred
    coordinates, R(t) = [[cos t, -sin t], [sin t, cos t]].  Flips and rot90
    alone give exact integers (square patches for odd k)."""
    if not scale > 0:
        raise ValueError(f"scale must be positive, got {scale}")
    th = np.deg2rad(float(angle))
    L = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) / float(scale)
    t = -L @ np.array([float(shift[0]) * W, float(shift[1]) * H])
    front = np.diag([-1.0 if hflip else 1.0, -1.0 if vflip else 1.0]) @ np.linalg.matrix_power(_ROT90, int(k) % 4)
    L, t = front @ L, front @ t
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    off = c - L @ c + t
    return np.array([L[0, 0], L[0, 1], off[0], L[1, 0], L[1, 1], off[1]], dtype=np.float32)


def colour_matrix(brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0):
    """(M [3, 3], o [3]) fp32 of v <- M v + o for, in this order: v + brightness;
    (1 + contrast) (v - 0.5) + 0.5; grey + (1 + saturation) (v - grey) with
    grey = 0.299 R + 0.587 G + 0.114 B; a rotation by ``hue`` turns about the
    grey axis in YIQ.  All four zero give the identity exactly."""
    b, c, s = float(brightness), float(contrast), float(saturation)
    th = 2.0 * np.pi * float(hue)
    eye, G = np.eye(3), np.tile(_GREY, (3, 1))
    M, o = (1.0 + c) * eye, np.full(3, (1.0 + c) * b + 0.5 * (1.0 - (1.0 + c)))
    Ms = (1.0 + s) * eye + (0.0 - s) * G
    Mh = eye + (np.cos(th) - 1.0) * (eye - G) + np.sin(th) * _HUE_J
    M, o = Mh @ Ms @ M, Mh @ Ms @ o
    return (M + 0.0).astype(np.float32), (o + 0.0).astype(np.float32)


def identity_knots(B, size, S=1):
    """[B, S+1] fp32 knot tables of the identity map over [0, size-1]."""
    k = (np.arange(S + 1, dtype=np.float64) * (size - 1) / S).astype(np.float32)
    k[-1] = size - 1
    return np.tile(k, (B, 1))


def identity_params(B):
    """[B, 20] fp32: identity affine, gamma 1, identity colour, no noise."""
    p = np.zeros((B, NPARAM), np.float32)
    p[:, [0, 4, 6, 7, 11, 15]] = 1.0
    return p


def blur_weights(sigma=None, box=None):
    """One row [9] fp32 = r, w_0..w_7 of the separable blur,
    built in float64, normalised to w_0 + 2 sum w_k = 1 and rounded to fp32.
    ``sigma``: a Gaussian exp(-k^2 / (2 sigma^2)) with r = min(7, ceil(3 sigma));
    taps that are 0 in fp32 are dropped, so sigma -> 0 gives the identity row
    [0, 1, 0, ...].  ``box``: the odd width 2r + 1 <= 15 of a box filter."""
    if (sigma is None) == (box is None):
        raise ValueError("give exactly one of sigma and box")
    if box is not None:
        if int(box) != box or not 1 <= int(box) <= 2 * RMAX + 1 or int(box) % 2 == 0:
            raise ValueError(f"box must be an odd width in [1, {2 * RMAX + 1}], got {box}")
        r = (int(box) - 1) // 2
        w = np.ones(r + 1)
    else:
        sigma = float(sigma)
        if not (np.isfinite(sigma) and sigma >= 0):
            raise ValueError(f"sigma must be finite and non-negative, got {sigma}")
        r = min(RMAX, int(np.ceil(3.0 * sigma)))
        k = np.arange(r + 1, dtype=np.float64)
        w = np.exp(-k * k / (2.0 * sigma * sigma)) if r > 0 else np.ones(1)
    w = (w / (w[0] + 2.0 * w[1:].sum())).astype(np.float32)
    while r > 0 and w[r] == 0:
        r -= 1
    row = np.zeros(NBLUR, np.float32)
    row[0], row[1:r + 2] = r, w[:r + 1]
    return row


def identity_blur(B):
    """[B, 9] fp32: r = 0, w_0 = 1 for every sample."""
    t = np.zeros((B, NBLUR), np.float32)
    t[:, 1] = 1.0
    return t


class TrainAugment:
    """Probabilities and ranges of the device-side training transform
    (``PatchCache(augment=TrainAugment(...))``).  The defaults are this
    project's own choice of a moderate setting, NOT the reference's
    albumentations values (unpinned vs the reference); pass
    the ranges of the run being reproduced.

    geometry   p_hflip, p_vflip, p_rot90 (k uniform in 0..3; square patches);
               p_affine with rotate_limit (degrees), scale_limit (scale in
               [1 - l, 1 + l]), shift_limit (fraction of the size, per axis);
               p_grid with grid_steps (1..32) and grid_limit (< 1)
    photometry p_gamma with gamma_range; p_colour with brightness_limit,
               contrast_limit, saturation_limit, hue_limit (turns);
               p_noise with noise_sigma range
    border     'reflect101' or 'constant'
    filters    (ahead of the warp, image only; off by default)
               p_clahe with the clahe_clip range and clahe_tiles (rows,
               columns); p_blur with the blur_sigma range of a Gaussian;
               p_median with median_limit, the largest odd window (3, 5 or 7;
               DESIGN.md §4.10)"""

    def __init__(self, p_hflip=0.5, p_vflip=0.5, p_rot90=0.5, p_affine=0.5, rotate_limit=15.0, scale_limit=0.1,
                 shift_limit=0.0625, p_grid=0.3, grid_steps=5, grid_limit=0.3, p_gamma=0.3, gamma_range=(0.8, 1.25),
                 p_colour=0.5, brightness_limit=0.2, contrast_limit=0.2, saturation_limit=0.2, hue_limit=0.02,
                 p_noise=0.3, noise_sigma=(0.005, 0.03), border="reflect101", p_clahe=0.0, clahe_clip=(1.0, 4.0),
                 clahe_tiles=(8, 8), p_blur=0.0, blur_sigma=(0.5, 1.5), p_median=0.0, median_limit=7):
        if border not in BORDERS:
            raise ValueError(f"border must be one of {sorted(BORDERS)}, got {border!r}")
        if not 1 <= int(grid_steps) <= MAX_GRID_STEPS:
            raise ValueError(f"grid_steps must be in [1, {MAX_GRID_STEPS}], got {grid_steps}")
        if not 0 <= grid_limit < 1:
            raise ValueError(f"grid_limit must be in [0, 1) (cell widths 1 +- limit stay positive), got {grid_limit}")
        if not 0 <= scale_limit < 1:
            raise ValueError(f"scale_limit must be in [0, 1), got {scale_limit}")
        if not (0 < gamma_range[0] <= gamma_range[1]) or not (0 <= noise_sigma[0] <= noise_sigma[1]):
            raise ValueError("gamma_range must be positive and noise_sigma non-negative, both ascending")
        self.p_hflip, self.p_vflip, self.p_rot90, self.p_affine = p_hflip, p_vflip, p_rot90, p_affine
        self.rotate_limit, self.scale_limit, self.shift_limit = rotate_limit, scale_limit, shift_limit
        self.p_grid, self.grid_steps, self.grid_limit = p_grid, int(grid_steps), grid_limit
        self.p_gamma, self.gamma_range = p_gamma, tuple(gamma_range)
        self.p_colour, self.brightness_limit, self.contrast_limit = p_colour, brightness_limit, contrast_limit
        self.saturation_limit, self.hue_limit = saturation_limit, hue_limit
        self.p_noise, self.noise_sigma = p_noise, tuple(noise_sigma)
        self.border = border
        if not (0 < clahe_clip[0] <= clahe_clip[1] < np.inf) or not (0 <= blur_sigma[0] <= blur_sigma[1] < np.inf):
            raise ValueError("clahe_clip must be positive and blur_sigma non-negative, both finite and ascending")
        self.clahe_tiles = _check_tiles(clahe_tiles)
        self.p_clahe, self.clahe_clip = p_clahe, tuple(clahe_clip)
        self.p_blur, self.blur_sigma = p_blur, tuple(blur_sigma)
        if isinstance(median_limit, bool) or not isinstance(median_limit, (int, np.integer)) \
                or median_limit % 2 == 0 or not 3 <= median_limit <= 2 * MEDIAN_RMAX + 1:
            raise ValueError(f"median_limit must be an odd window in [3, {2 * MEDIAN_RMAX + 1}], got {median_limit!r}")
        self.p_median, self.median_limit = p_median, int(median_limit)

    def _knots(self, size, S, rng):
        w = 1.0 + rng.uniform(-self.grid_limit, self.grid_limit, S)
        cum = np.concatenate([[0.0], np.cumsum(w)])
        k = (cum / cum[-1] * (size - 1)).astype(np.float32)
        k[0], k[-1] = 0.0, size - 1
        return k

    def draw(self, B, H, W, rng):
        """Host arrays (params [B, 20], gx [B, S+1], gy [B, S+1]) fp32 for one
        batch from the numpy Generator ``rng``; a transform whose coin fails
        contributes its identity.  S = grid_steps (1 when p_grid is 0)."""
        if self.p_rot90 > 0 and H != W:
            raise ValueError("rot90 augmentation needs square patches")
        S = self.grid_steps if self.p_grid > 0 else 1
        params = identity_params(B)
        gx, gy = identity_knots(B, W, S), identity_knots(B, H, S)
        for b in range(B):
            hf = rng.random() < self.p_hflip
            vf = rng.random() < self.p_vflip
            k = int(rng.integers(0, 4)) if rng.random() < self.p_rot90 else 0
            angle, scale, shift = 0.0, 1.0, (0.0, 0.0)
            if rng.random() < self.p_affine:
                angle = rng.uniform(-self.rotate_limit, self.rotate_limit)
                scale = 1.0 + rng.uniform(-self.scale_limit, self.scale_limit)
                shift = (rng.uniform(-self.shift_limit, self.shift_limit),
                         rng.uniform(-self.shift_limit, self.shift_limit))
            params[b, 0:6] = affine_matrix(H, W, hf, vf, k, angle, scale, shift)
            if rng.random() < self.p_grid:
                gx[b], gy[b] = self._knots(W, S, rng), self._knots(H, S, rng)
            if rng.random() < self.p_gamma:
                params[b, 6] = rng.uniform(*self.gamma_range)
            if rng.random() < self.p_colour:
                M, o = colour_matrix(rng.uniform(-self.brightness_limit, self.brightness_limit),
                                     rng.uniform(-self.contrast_limit, self.contrast_limit),
                                     rng.uniform(-self.saturation_limit, self.saturation_limit),
                                     rng.uniform(-self.hue_limit, self.hue_limit))
                params[b, 7:16], params[b, 16:19] = M.reshape(9), o
            if rng.random() < self.p_noise:
                params[b, 19] = rng.uniform(*self.noise_sigma)
        return params, gx, gy

    def draw_filters(self, B, rng):
        """Host arrays (clip [B], blur table [B, 9]) fp32 for one batch: a sample
        whose coin fails gets clip 0 (CLAHE off) / the identity blur row.
        PatchCache calls it after ``draw``, and only when p_clahe or p_blur
        is positive, so ``draw``'s sequence is what it was without them."""
        clip, table = np.zeros(B, np.float32), identity_blur(B)
        for b in range(B):
            if rng.random() < self.p_clahe:
                clip[b] = rng.uniform(*self.clahe_clip)
            if rng.random() < self.p_blur:
                table[b] = blur_weights(sigma=rng.uniform(*self.blur_sigma))
        return clip, table

    def draw_median(self, B, rng):
        """Host array radius [B] fp32 of the median blur for one batch: one coin
        per sample; on success the window is uniform over the odd values
        3..median_limit and the radius (window - 1) / 2, else 0 (off).
        PatchCache calls it after ``draw`` and ``draw_filters``, and only when
        p_median is positive, so their sequences are what they were."""
        radius = np.zeros(B, np.float32)
        for b in range(B):
            if rng.random() < self.p_median:
                radius[b] = int(rng.integers(1, (self.median_limit - 1) // 2 + 1))
        return radius


def _check_augment_args(img, msk, params, gx, gy, seed, offset, border):
    """Host validation of one augmentation call; returns (params, gx, gy) as
    contiguous fp32 numpy arrays.  Nothing here touches a device."""
    if border not in BORDERS:
        raise ValueError(f"border must be one of {sorted(BORDERS)}, got {border!r}")
    if img.dim() != 4 or msk.dim() != 4 or img.shape[1] != 3 or msk.shape[1] < 1:
        raise ValueError(f"expected image [B, 3, H, W] and mask [B, Cm >= 1, H, W], got {tuple(img.shape)} and "
                         f"{tuple(msk.shape)}")
    B, _, H, W = img.shape
    if msk.shape[0] != B or tuple(msk.shape[2:]) != (H, W):
        raise ValueError(f"image {tuple(img.shape)} and mask {tuple(msk.shape)} differ in batch or size")
    if img.dtype != torch.float32 or msk.dtype != torch.float32:
        raise ValueError("image and mask must be float32")
    if H < 2 or W < 2:
        raise ValueError(f"patches must be at least 2 x 2, got {H} x {W}")
    params, gx, gy = (np.ascontiguousarray(a, dtype=np.float32) for a in (params, gx, gy))
    if params.shape != (B, NPARAM):
        raise ValueError(f"params must be [{B}, {NPARAM}], got {params.shape}")
    if gx.ndim != 2 or gx.shape != gy.shape or gx.shape[0] != B or not 2 <= gx.shape[1] <= MAX_GRID_STEPS + 1:
        raise ValueError(f"gx and gy must both be [{B}, S + 1] with 1 <= S <= {MAX_GRID_STEPS}, got {gx.shape} "
                         f"and {gy.shape}")
    for name, a in (("params", params), ("gx", gx), ("gy", gy)):
        if not np.isfinite(a).all():
            raise ValueError(f"{name} holds a non-finite value")
    for name, a in (("gx", gx), ("gy", gy)):
        if not (np.diff(a, axis=1) > 0).all():
            raise ValueError(f"{name}: the knots of every sample must be strictly increasing")
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(offset) < 2 ** 32:
        raise ValueError(f"seed must fit 64 bits and offset 32 bits, got {seed} and {offset}")
    return params, gx, gy


def _check_tiles(tiles):
    """(TY, TX) as ints in [1, 16]"""
    try:
        ty, tx = tiles
        ok = int(ty) == ty and int(tx) == tx and 1 <= ty <= MAX_TILES and 1 <= tx <= MAX_TILES
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"tiles must be two integers (rows, columns) in [1, {MAX_TILES}], got {tiles!r}")
    return int(ty), int(tx)


def _check_filter_args(img, clip=None, tiles=(8, 8), table=None):
    """Host validation of a CLAHE and / or blur call on image [B, 3, H, W];
    returns (clip [B] or None, (TY, TX), table [B, 9] or None) as contiguous
    fp32 numpy arrays.  Nothing here touches a device."""
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] < 1 or img.shape[3] < 1:
        raise ValueError(f"expected image [B, 3, H >= 1, W >= 1], got {tuple(img.shape)}")
    if img.dtype != torch.float32:
        raise ValueError("image must be float32")
    B, _, H, W = img.shape
    tiles = _check_tiles(tiles)
    if clip is not None:
        clip = np.asarray(clip, dtype=np.float32)
        clip = np.ascontiguousarray(np.broadcast_to(clip, (B,)) if clip.ndim == 0 else clip)
        if clip.shape != (B,):
            raise ValueError(f"the clip limit must be a scalar or [{B}], got {clip.shape}")
        if not (np.isfinite(clip) & (clip >= 0)).all():
            raise ValueError("every clip limit must be finite and >= 0 (0 switches the sample off)")
        if tiles[0] > H or tiles[1] > W:
            raise ValueError(f"{tiles[0]} x {tiles[1]} tiles do not fit a {H} x {W} image")
    if table is not None:
        table = np.ascontiguousarray(table, dtype=np.float32)
        if table.shape != (B, NBLUR):
            raise ValueError(f"the blur table must be [{B}, {NBLUR}] = r, w_0..w_{RMAX}, got {table.shape}")
        if not np.isfinite(table).all():
            raise ValueError("the blur table holds a non-finite value")
        r = table[:, 0]
        if not ((r == np.round(r)) & (r >= 0) & (r <= RMAX)).all():
            raise ValueError(f"every blur radius must be an integer in [0, {RMAX}]")
    return clip, tiles, table


def _check_median_args(img, radius):
    """Host validation of a median blur call on image [B, 3, H, W]; returns the
    radius as a contiguous fp32 numpy array [B].  Nothing here touches a device."""
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[2] < 1 or img.shape[3] < 1:
        raise ValueError(f"expected image [B, 3, H >= 1, W >= 1], got {tuple(img.shape)}")
    if img.dtype != torch.float32:
        raise ValueError("image must be float32")
    B = img.shape[0]
    try:
        radius = np.asarray(radius, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"the median radius must be a number or [{B}] numbers, got {radius!r}") from None
    radius = np.broadcast_to(radius, (B,)) if radius.ndim == 0 else radius
    if radius.shape != (B,):
        raise ValueError(f"the median radius must be a scalar or [{B}], got {radius.shape}")
    if not (np.isfinite(radius) & (radius == np.round(radius)) & (radius >= 0) & (radius <= MEDIAN_RMAX)).all():
        raise ValueError(f"every median radius must be an integer in [0, {MEDIAN_RMAX}] (0 switches the sample off)")
    return np.ascontiguousarray(radius, dtype=np.float32)


def _launch_clahe(img, dclip, tiles):
    """vu_clahe_luts + vu_clahe_apply on device tensors"""
    img = img.contiguous(memory_format=CL)
    B, _, H, W = img.shape
    luts = torch.empty((B, tiles[0], tiles[1], 256), dtype=torch.uint8, device=img.device)
    out = K.empty_act(B, 3, H, W, torch.float32, img.device)
    with torch.cuda.device(img.device):
        K.call("vu_clahe_luts", K.ptr(img), B, H, W, K.ptr(dclip), tiles[0], tiles[1], K.ptr(luts), K.stream())
        K.call("vu_clahe_apply", K.ptr(img), B, H, W, K.ptr(dclip), tiles[0], tiles[1], K.ptr(luts), K.ptr(out),
               K.stream())
    return out


def _launch_blur(img, dtable):
    """The one vu_blur_sep launch on device tensors"""
    img = img.contiguous(memory_format=CL)
    B, _, H, W = img.shape
    out = K.empty_act(B, 3, H, W, torch.float32, img.device)
    with torch.cuda.device(img.device):
        K.call("vu_blur_sep", K.ptr(img), B, H, W, K.ptr(dtable), K.ptr(out), K.stream())
    return out


def _launch_median(img, dradius):
    """The one vu_median_blur launch on device tensors"""
    img = img.contiguous(memory_format=CL)
    B, _, H, W = img.shape
    out = K.empty_act(B, 3, H, W, torch.float32, img.device)
    with torch.cuda.device(img.device):
        K.call("vu_median_blur", K.ptr(img), B, H, W, K.ptr(dradius), K.ptr(out), K.stream())
    return out


def _need_device(img, what):
    if img.device.type != "cuda":
        raise RuntimeError(f"{what} runs on MI355X (HIP) devices only; got {img.device}")


def clahe(image, clip_limit=2.0, tiles=(8, 8)):
    """CLAHE of image [B, 3, H, W] (fp32 on the device) on an integer luma
    (DESIGN.md §4.9): per-tile clipped histograms -> lookup tables, blended
    per pixel, the luma change added to every channel.  ``clip_limit``: a
    scalar or one value per sample, 0 = off (the sample comes back bitwise);
    ``tiles`` = (rows, columns), each in 1..16 and at most the image size.
    Returns channels_last.  Checked on the host first (ValueError)."""
    clip, tiles, _ = _check_filter_args(image, clip=clip_limit, tiles=tiles)
    _need_device(image, "clahe")
    return _launch_clahe(image, torch.from_numpy(clip).to(image.device), tiles)


def blur(image, table):
    """Separable symmetric blur of image [B, 3, H, W] (fp32 on the device) with
    one row r, w_0..w_7 per sample (``blur_weights``; [B, 9]), reflect101
    border, horizontal then vertical pass in one launch.
    Returns channels_last.  Checked on the host first (ValueError)."""
    _, _, table = _check_filter_args(image, table=table)
    _need_device(image, "blur")
    return _launch_blur(image, torch.from_numpy(table).to(image.device))


def median_blur(image, radius):
    """Median blur of image [B, 3, H, W] (fp32 on the device), per channel, over
    the (2r + 1) x (2r + 1) window with a replicated border.
    ``radius``: an integer in 0..3 or one per sample ([B]); 0 = off (the sample
    comes back bitwise).  Every output value is bitwise one of its window's
    inputs.  Returns channels_last.  Checked on the host first (ValueError)."""
    radius = _check_median_args(image, radius)
    _need_device(image, "median_blur")
    return _launch_median(image, torch.from_numpy(radius).to(image.device))


def _launch_augment(img, msk, dparams, dgx, dgy, seed, offset, border):
    """The one vu_augment_patch launch on device tensors (border: the C code)."""
    img = img.contiguous(memory_format=CL)
    msk = msk.contiguous(memory_format=CL)
    B, _, H, W = img.shape
    Cm, S = msk.shape[1], dgx.shape[1] - 1
    oimg = K.empty_act(B, 3, H, W, torch.float32, img.device)
    omsk = K.empty_act(B, Cm, H, W, torch.float32, img.device)
    with torch.cuda.device(img.device):
        K.call("vu_augment_patch", K.ptr(img), K.ptr(msk), B, H, W, 3, Cm, K.ptr(dparams), K.ptr(dgx), K.ptr(dgy), S,
               border, int(seed), int(offset), K.ptr(oimg), K.ptr(omsk), K.stream())
    return oimg, omsk


def augment_patches(img, msk, params, gx, gy, seed, offset=0, border="reflect101", clahe_clip=None,
                    clahe_tiles=(8, 8), blur=None, median=None):
    """Augment image [B, 3, H, W] and mask [B, Cm, H, W] (fp32 on the device) in
    ONE launch (vu_augment_patch) with the host arrays of
    ``TrainAugment.draw`` (or any of the same layout); returns (image, mask),
    channels_last on the device.  The arrays are checked here before they are
    uploaded (finite, consistent shapes, increasing knots: ValueError); the
    kernel's coordinate clamp is the second line of defence.  The noise is a
    function of (seed, offset, sample, pixel) alone.  ``clahe_clip`` (scalar or
    [B], with ``clahe_tiles``) and ``blur`` ([B, 9]), the arrays of
    ``TrainAugment.draw_filters``, run CLAHE and / or the blur on the image
    ahead of that launch; ``median`` (a radius 0..3, scalar or
    [B], the array of ``TrainAugment.draw_median``) runs the median blur after
    them: CLAHE -> blur -> median -> warp.  Their tables ride
    in the same upload."""
    params, gx, gy = _check_augment_args(img, msk, params, gx, gy, seed, offset, border)
    clip, tiles, table = _check_filter_args(img, clahe_clip, clahe_tiles, blur)
    radius = None if median is None else _check_median_args(img, median)
    if img.device.type != "cuda" or msk.device != img.device:
        raise RuntimeError(f"augment_patches runs on MI355X (HIP) devices only; got {img.device} and {msk.device}")
    B, S1 = params.shape[0], gx.shape[1]
    parts = [params.reshape(-1), gx.reshape(-1), gy.reshape(-1)]
    parts += [a.reshape(-1) for a in (clip, table, radius) if a is not None]
    dev = torch.from_numpy(np.concatenate(parts)).to(img.device)      # one upload for every table
    n0, n1 = B * NPARAM, B * S1
    n2 = n0 + 2 * n1
    if clip is not None:
        img = _launch_clahe(img, dev[n2:n2 + B], tiles)
        n2 += B
    if table is not None:
        img = _launch_blur(img, dev[n2:n2 + B * NBLUR].view(B, NBLUR))
        n2 += B * NBLUR
    if radius is not None:
        img = _launch_median(img, dev[n2:n2 + B])
    return _launch_augment(img, msk, dev[:n0].view(B, NPARAM), dev[n0:n0 + n1].view(B, S1),
                           dev[n0 + n1:n0 + 2 * n1].view(B, S1), seed, offset, BORDERS[border])


class PatchCache:
    """Iterate the cached patches in batches on ``device``.

    paths: cache files (or a directory holding them); yields dicts with
    ``image`` [B, 3, P, P] and ``mask`` [B, 1, P, P] (fp32, channels_last, on
    the device), ``img_id`` and ``coords``.  ``augment``: False; True for the
    flip/rotate augmentation alone (one integer gather per tensor); or a
    ``TrainAugment`` for the full device-side transform (one draw and one
    launch per batch; the Philox key is ``seed``, the offset the number of
    batches augmented so far; the batch gains ``aug_params``, what
    ``augment_patches`` needs to replay it; with ``p_clahe`` / ``p_blur``
    positive the CLAHE and blur launches run first and their drawn arrays
    join ``aug_params``; with ``p_median`` positive the median blur follows
    them and ``aug_params`` gains ``median``).  All draws come from the
    generator seeded with ``seed``."""

    def __init__(self, paths, batch_size, device="cuda", augment=False, shuffle=False, seed=0, workers=6,
                 drop_last=False):
        if isinstance(paths, (str, os.PathLike)) and os.path.isdir(paths):
            paths = sorted(os.path.join(paths, f) for f in os.listdir(paths))
        self.paths = list(paths)
        self.batch_size = batch_size
        self.device = torch.device(device)
        self.augment = augment
        self.shuffle = shuffle
        self.seed = int(seed)
        self.aug_calls = 0                                         # Philox offset of the next TrainAugment batch
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.pool = ThreadPoolExecutor(max_workers=workers)        # file reads
        self.batch_pool = ThreadPoolExecutor(max_workers=1)        # batch assembly (prefetch 1)
        self.drop_last = drop_last
        self.stream = torch.cuda.Stream(device=self.device) if self.device.type == "cuda" else None

    def __len__(self):
        n = len(self.paths)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _host_batch(self, idx):
        recs = list(self.pool.map(lambda i: load_patch(self.paths[i]), idx))
        img = torch.stack([r["image"] for r in recs]).float()
        msk = torch.stack([r["mask"] for r in recs]).float()
        ids = [os.path.basename(self.paths[i]).rsplit("_", 1)[0] for i in idx]
        return img.pin_memory(), msk.pin_memory(), ids, [tuple(r.get("coords", (0, 0))) for r in recs]

    def _to_device(self, host):
        img, msk, ids, coords = host
        with torch.cuda.stream(self.stream):
            dimg = img.to(self.device, non_blocking=True).contiguous(memory_format=CL)
            dmsk = msk.to(self.device, non_blocking=True).contiguous(memory_format=CL)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return dimg, dmsk, ids, coords, ev

    def augment_batch(self, img, msk, flags=None):
        """Flip / rot90 per sample (flags: [(hflip, vflip, k)] or drawn)."""
        B, _, H, W = img.shape
        if H != W:
            raise ValueError("rot90 augmentation needs square patches")
        if flags is None:
            flags = []
            for _ in range(B):
                hf = self.rng.random() < 0.5
                vf = self.rng.random() < 0.5
                k = int(self.rng.integers(0, 4)) if self.rng.random() < 0.5 else 0
                flags.append((hf, vf, k))
        m = torch.tensor([_flip_rot_map(H, *f) for f in flags], dtype=torch.int32).to(img.device)
        outs = []
        for t in (img, msk):
            o = K.empty_act(B, t.shape[1], H, W, torch.float32, t.device)
            K.call("vu_gather_affine", K.ptr(t), B, H, W, t.shape[1], K.ptr(m), K.ptr(o), H, W, F32, K.stream())
            outs.append(o)
        return outs[0], outs[1], flags

    def __iter__(self):
        order = np.arange(len(self.paths))
        if self.shuffle:
            self.rng.shuffle(order)
        batches = [order[i:i + self.batch_size] for i in range(0, len(order), self.batch_size)]
        if self.drop_last and batches and len(batches[-1]) < self.batch_size:
            batches.pop()
        nxt = self.batch_pool.submit(self._host_batch, batches[0]) if batches else None
        for bi in range(len(batches)):
            host = nxt.result()
            nxt = self.batch_pool.submit(self._host_batch, batches[bi + 1]) if bi + 1 < len(batches) else None
            img, msk, ids, coords, ev = self._to_device(host)
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            img.record_stream(cur)   # allocated on the copy stream, used (and freed) on this one
            msk.record_stream(cur)
            extra = {}
            if isinstance(self.augment, TrainAugment):
                params, gx, gy = self.augment.draw(img.shape[0], img.shape[2], img.shape[3], self.rng)
                aug = {"params": params, "gx": gx, "gy": gy, "seed": self.seed & (2 ** 64 - 1),
                       "offset": self.aug_calls & 0xffffffff, "border": self.augment.border}
                if self.augment.p_clahe > 0 or self.augment.p_blur > 0:
                    clip, table = self.augment.draw_filters(img.shape[0], self.rng)
                    if self.augment.p_clahe > 0:
                        aug["clahe_clip"], aug["clahe_tiles"] = clip, self.augment.clahe_tiles
                    if self.augment.p_blur > 0:
                        aug["blur"] = table
                if self.augment.p_median > 0:
                    aug["median"] = self.augment.draw_median(img.shape[0], self.rng)
                img, msk = augment_patches(img, msk, **aug)
                self.aug_calls += 1
                extra["aug_params"] = aug
            elif self.augment:
                img, msk, _ = self.augment_batch(img, msk)
            yield {"image": img, "mask": msk, "img_id": ids, "coords": coords, **extra}
