"""Training-time image augmentation of OpenVLA (`--image_aug`), host restatement and device twin.

In the reference the augmentation runs inside the TF / dlimp ingest (prismatic/vla/datasets/datasets.py:121-136 →
rlds/obs_transforms.py:17-40 → dlimp.transforms.augment_image) with the parameters of datasets.py:123-135, in this order,
each operation followed by `clip(·, 0, 1)` on a float32 image in [0, 1]:

  0. x = u8 · (1/255)                                   tf.image.convert_image_dtype, as eval_preprocess._to_float
  1. random_resized_crop, scale [0.9, 0.9], ratio [1, 1]: side s = sqrt(0.9), offsets y1, x1 ~ U[0, 1 − s), box
     (y1, x1, y1 + s, x1 + s), tf.image.crop_and_resize bilinear back to H×W — the arithmetic of
     eval_preprocess.crop_and_resize_bilinear with a box per image
  2. random_brightness 0.2: x + δ, δ ~ U[−0.2, 0.2)
  3. random_contrast [0.8, 1.2]: (x − mean_c)·f + mean_c, mean_c the per-image, per-channel mean over H×W, defined here as
     fp32(Σ rint(x·2^24) / (H·W·2^24)) with the sum in int64 and the division in fp64: exact in any summation order (so
     the device can reduce in parallel), within 2^-25 of an fp32 mean
  4. random_saturation [0.8, 1.2]: RGB → HSV, S = clip(S·f, 0, 1), HSV → RGB
  5. random_hue 0.05: RGB → HSV, h = h + δ, h = h − floor(h), HSV → RGB, δ ~ U[−0.05, 0.05)
  6. u8 = min(trunc(clip(x, 0, 1)·255.5), 255)          TF's saturating convert, as eval_preprocess._to_uint8_saturate

Every arithmetic step is one IEEE fp32 operation rounded on its own (except the contrast mean above). The HSV conversions
are TF's functors (adjust_saturation / adjust_hue):
  RGB → HSV: V = max, range = V − min, S = V > 0 ? range / V : 0, norm = 1 / (6·range); h = norm·(g − b) if r == V, else
             norm·(b − r) + 2/6 if g == V, else norm·(r − g) + 4/6; h = 0 when range == 0; h += 1 when h < 0
  HSV → RGB: c = S·V, m = V − c, dh = 6h; r = clip(|dh − 3| − 1, 0, 1)·c + m, g = clip(2 − |dh − 2|, 0, 1)·c + m,
             b = clip(2 − |dh − 4|, 0, 1)·c + m

TensorFlow and dlimp are absent here and on the GPU box: dlimp's crop sampling and TF's fused adjust_saturation / adjust_hue
kernels are restated from their documented formulas — PARITY UNPINNED against TF; the tests check the defining properties
(identity parameters, the centre box against the eval-time crop, hue periodicity, parameter ranges).

The randomness is a host table: `draw_params(n, seed, rank, step)` → [n, 8] float32 rows (y1, x1, side_y, side_x,
brightness δ, contrast f, saturation f, hue δ), deterministic per (seed, rank, step) and different across ranks and steps.
`augment_frame` (numpy) is the specification; `augment_frames_gpu` (bl_augment_frames_u8) is bit-identical to it on uint8
frames in HBM and is a pure function of (frames, params)."""
from __future__ import annotations

from typing import Optional

import numpy as np

from .eval_preprocess import _to_float, _to_uint8_saturate, crop_and_resize_bilinear

# datasets.py:123-135
OPENVLA_IMAGE_AUG = dict(random_resized_crop=dict(scale=[0.9, 0.9], ratio=[1.0, 1.0]), random_brightness=[0.2],
                         random_contrast=[0.8, 1.2], random_saturation=[0.8, 1.2], random_hue=[0.05],
                         augment_order=["random_resized_crop", "random_brightness", "random_contrast", "random_saturation",
                                        "random_hue"])
PARAM_COLUMNS = ("y1", "x1", "side_y", "side_x", "brightness", "contrast", "saturation", "hue")
IDENTITY_PARAMS = np.array([0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0], dtype=np.float32)

_f32 = np.float32


def crop_side(aug: dict = OPENVLA_IMAGE_AUG) -> np.float32:
    """Side of the crop box as a fraction of the image side, in fp32 like the eval-time centre crop: scale is one value
    (area fraction) and ratio is 1, so both sides are sqrt(scale)."""
    scale, ratio = aug["random_resized_crop"]["scale"], aug["random_resized_crop"]["ratio"]
    if scale[0] != scale[1] or ratio[0] != 1.0 or ratio[1] != 1.0:
        raise NotImplementedError("only OpenVLA's fixed-scale, square random_resized_crop is restated")
    return np.clip(np.sqrt(_f32(scale[0])), _f32(0.0), _f32(1.0))


def draw_params(n: int, seed: int, rank: int, step: int, aug: dict = OPENVLA_IMAGE_AUG) -> np.ndarray:
    """The augmentation parameters of `n` images, [n, 8] float32 in PARAM_COLUMNS order, from
    np.random.default_rng([seed, rank, step]): the same (seed, rank, step) always gives the same table, another rank or
    another step gives another. Offsets are U[0, 1 − s) so that the fp32 box edge y1 + s never exceeds 1."""
    rng = np.random.default_rng([int(seed), int(rank), int(step)])
    u = rng.random((n, 6), dtype=np.float32)                       # U[0, 1) in fp32
    s = crop_side(aug)
    b, (c0, c1), (s0, s1), h = (aug["random_brightness"][0], aug["random_contrast"], aug["random_saturation"],
                                aug["random_hue"][0])
    out = np.empty((n, 8), dtype=np.float32)
    room = _f32(1.0) - s
    out[:, 0], out[:, 1] = u[:, 0] * room, u[:, 1] * room
    out[:, 2] = out[:, 3] = s
    out[:, 4] = _f32(-b) + u[:, 2] * _f32(2 * b)
    out[:, 5] = _f32(c0) + u[:, 3] * _f32(c1 - c0)
    out[:, 6] = _f32(s0) + u[:, 4] * _f32(s1 - s0)
    out[:, 7] = _f32(-h) + u[:, 5] * _f32(2 * h)
    # fp32 rounding of lo + u·(hi − lo) can land on hi itself: keep every column inside its half-open range
    out[:, 0:2] = np.minimum(out[:, 0:2], np.nextafter(room, _f32(0.0)))
    for col, hi in ((4, b), (5, c1), (6, s1), (7, h)):
        out[:, col] = np.minimum(out[:, col], np.nextafter(_f32(hi), _f32(-np.inf)))
    return out


def _clip01(x: np.ndarray) -> np.ndarray:
    return np.clip(x, _f32(0.0), _f32(1.0))


def channel_means(x: np.ndarray) -> np.ndarray:
    """Per-channel mean of a float32 image [H, W, 3] in [0, 1] as fp32(Σ rint(x·2^24) / (H·W·2^24)): int64 sum, fp64 division."""
    H, W, _ = x.shape
    sums = np.rint(x * _f32(16777216.0)).astype(np.int64).sum(axis=(0, 1))
    return (sums.astype(np.float64) / (np.float64(H * W) * np.float64(16777216.0))).astype(np.float32)


def rgb_to_hsv(x: np.ndarray):
    """TF's RGB → HSV functor on float32 [..., 3]; returns (h, s, v), h in [0, 1)."""
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    rng = v - np.minimum(np.minimum(r, g), b)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(v > 0, rng / v, _f32(0.0)).astype(np.float32)
        norm = _f32(1.0) / (_f32(6.0) * rng)
        h = np.where(r == v, norm * (g - b),
                     np.where(g == v, norm * (b - r) + _f32(2.0) / _f32(6.0), norm * (r - g) + _f32(4.0) / _f32(6.0)))
    h = np.where(rng == 0, _f32(0.0), h).astype(np.float32)
    h = np.where(h < 0, h + _f32(1.0), h).astype(np.float32)
    return h, s, v


def hsv_to_rgb(h: np.ndarray, s: np.ndarray, v: np.ndarray) -> np.ndarray:
    """TF's HSV → RGB functor; float32 [..., 3]."""
    c = s * v
    m = v - c
    dh = _f32(6.0) * h
    r = _clip01(np.abs(dh - _f32(3.0)) - _f32(1.0)) * c + m
    g = _clip01(_f32(2.0) - np.abs(dh - _f32(2.0))) * c + m
    b = _clip01(_f32(2.0) - np.abs(dh - _f32(4.0))) * c + m
    return np.stack([r, g, b], axis=-1).astype(np.float32)


def augment_frame(image_u8: np.ndarray, params: np.ndarray) -> np.ndarray:
    """uint8 [H, W, 3] and one parameter row [8] → the augmented uint8 [H, W, 3] (the specification, op for op)."""
    image_u8 = np.asarray(image_u8)
    if image_u8.dtype != np.uint8 or image_u8.ndim != 3 or image_u8.shape[2] != 3 or min(image_u8.shape[:2]) < 2:
        raise ValueError("augment_frame: expected a uint8 image [H, W, 3] with H, W >= 2")
    y1, x1, sy, sx, bright, contrast, sat, hue = (_f32(v) for v in np.asarray(params, dtype=np.float32).reshape(8))
    H, W, _ = image_u8.shape
    x = _to_float(image_u8)
    x = _clip01(crop_and_resize_bilinear(x, (float(y1), float(x1), float(y1 + sy), float(x1 + sx)), (H, W)))
    x = _clip01(x + bright)
    mean = channel_means(x)
    x = _clip01((x - mean) * contrast + mean)
    h, s, v = rgb_to_hsv(x)
    x = _clip01(hsv_to_rgb(h, _clip01(s * sat), v))
    h, s, v = rgb_to_hsv(x)
    h = h + hue
    x = _clip01(hsv_to_rgb(h - np.floor(h), s, v))
    assert x.dtype == np.float32
    return _to_uint8_saturate(x)


def augment_frames_gpu(frames_u8, params, out=None, workspace=None):
    """`augment_frame` for a batch of uint8 frames [B, H, W, 3] resident on the GPU with params [B, 8] (numpy or tensor) →
    uint8 [B, H, W, 3] (bl_augment_frames_u8); bit-identical to the host function, frame by frame."""
    import torch
    from .. import ops
    if not torch.is_tensor(params):
        params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32))
    params = params.to(frames_u8.device)
    if out is None:
        out = torch.empty_like(frames_u8)
    ops.augment_frames_u8(frames_u8, params, out=out, workspace=workspace)
    return out
