"""CPU: the host restatement of OpenVLA's training-time image augmentation (vla/image_augment.py — the specification its
device twin bl_augment_frames_u8 is held to) and the parameter draw. TensorFlow / dlimp are absent, so these are the
defining properties: identity parameters return the frame, the centre box is the eval-time centre crop, hue has period
1, the draw is deterministic per (seed, rank, step), inside its ranges and different across ranks and steps; and the
training loops refuse `image_aug` when the loader yields float pixel values."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bridgelang_amd.vla import image_augment as A
from bridgelang_amd.vla.eval_preprocess import center_crop_and_resize, center_crop_box


def probe_image(h: int, w: int, seed: int = 0) -> np.ndarray:
    """Random pixels with every grey level, black, white and the six saturated primaries / secondaries written over them."""
    img = np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)
    flat = img.reshape(-1, 3)
    greys = np.arange(256, dtype=np.uint8)[:, None].repeat(3, axis=1)
    colours = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255],
                        [255, 0, 255]], dtype=np.uint8)
    special = np.concatenate([greys, colours])
    flat[::3][:len(special)] = special[:len(flat[::3])]
    assert len(flat[::3]) >= len(special)
    return img


@pytest.mark.parametrize("hw", [(37, 53), (224, 224)])
def test_identity_parameters_return_the_frame(hw):
    img = probe_image(*hw)
    assert (img[..., 0] == img[..., 1]).any() and (img == 255).all(-1).any() and (img == 0).all(-1).any()
    out = A.augment_frame(img, A.IDENTITY_PARAMS)
    assert out.dtype == np.uint8 and np.array_equal(out, img)


@pytest.mark.parametrize("hw", [(37, 53), (224, 224)])
def test_centre_box_is_the_eval_time_centre_crop(hw):
    img = probe_image(*hw, seed=1)
    off, _, _, _ = center_crop_box(0.9)
    s = A.crop_side()
    p = A.IDENTITY_PARAMS.copy()
    p[0] = p[1] = off
    p[2] = p[3] = s
    assert np.float32(off) == (np.float32(1.0) - s) / np.float32(2.0)
    want = center_crop_and_resize(img, 0.9, hw)
    assert np.array_equal(A.augment_frame(img, p), want)
    assert not np.array_equal(want, img)


def test_hue_shift_has_period_one():
    img = probe_image(37, 53, seed=2)
    p = A.IDENTITY_PARAMS.copy()
    for d in (0.0, 0.03125, -0.046875):                            # δ and δ + 1 are both exact in fp32
        p[7] = d
        a = A.augment_frame(img, p)
        p[7] = d + 1.0
        assert np.array_equal(A.augment_frame(img, p), a), d
    p[7] = 0.03125
    assert not np.array_equal(A.augment_frame(img, p), img)


def test_each_operation_moves_the_image_the_right_way():
    img = probe_image(37, 53, seed=3)
    p = A.IDENTITY_PARAMS.copy(); p[4] = 0.2
    up = A.augment_frame(img, p).astype(int)
    assert (up >= img).all() and abs((up - img)[img < 200].mean() - 51) < 0.6       # + 0.2·255, clipped at white
    p = A.IDENTITY_PARAMS.copy(); p[5] = 0.8
    low = A.augment_frame(img, p).astype(float)
    assert low.std() < 0.81 * img.std() and abs(low.mean() - img.mean()) < 0.6      # contrast about the channel means
    p = A.IDENTITY_PARAMS.copy(); p[6] = 0.8
    sat = A.augment_frame(img, p).astype(int)
    spread = lambda x: (x.max(-1) - x.min(-1)).mean()
    assert spread(sat) < 0.82 * spread(img) and np.abs(sat.max(-1) - img.max(-1).astype(int)).max() <= 1   # V is kept
    grey = np.full((5, 7, 3), 93, dtype=np.uint8)
    p = np.array([0, 0, 1, 1, 0, 1.2, 1.2, 0.05], dtype=np.float32)
    assert np.array_equal(A.augment_frame(grey, p), grey)                           # range == 0: no hue, no saturation
    black = np.zeros((5, 7, 3), dtype=np.uint8)
    assert np.array_equal(A.augment_frame(black, p), black)                         # V == 0


def test_draw_params_deterministic_in_range_and_distinct():
    a = A.draw_params(4096, seed=7, rank=0, step=3)
    assert a.dtype == np.float32 and a.shape == (4096, 8)
    assert np.array_equal(a, A.draw_params(4096, seed=7, rank=0, step=3))
    s = A.crop_side()
    assert s == np.sqrt(np.float32(0.9))
    f = np.float32
    assert (a[:, 2] == s).all() and (a[:, 3] == s).all()
    assert (a[:, :2] >= 0).all() and (a[:, :2] < f(1.0) - s).all()
    assert (a[:, 0] + a[:, 2] <= f(1.0)).all() and (a[:, 1] + a[:, 3] <= f(1.0)).all()      # the fp32 box stays inside
    for col, lo, hi in ((4, -0.2, 0.2), (5, 0.8, 1.2), (6, 0.8, 1.2), (7, -0.05, 0.05)):
        assert (a[:, col] >= f(lo)).all() and (a[:, col] < f(hi)).all(), col
        assert a[:, col].min() < f(lo) + f(0.02) * f(hi - lo) and a[:, col].max() > f(hi) - f(0.02) * f(hi - lo), col
    for other in (A.draw_params(4096, 7, 1, 3), A.draw_params(4096, 7, 0, 4), A.draw_params(4096, 8, 0, 3)):
        assert all(not np.array_equal(a[:, c], other[:, c]) for c in (0, 1, 4, 5, 6, 7))
    with pytest.raises(NotImplementedError):
        A.crop_side(dict(A.OPENVLA_IMAGE_AUG, random_resized_crop=dict(scale=[0.5, 0.9], ratio=[1.0, 1.0])))


class Handed(Exception):
    """Raised by the stub once a batch has reached it: the test ends the loop there."""


class StubEngine:
    """What the loops need of a TrainStep up to the point where the batch is handed over."""
    L, B = 64, 2

    def __init__(self, *a, **k):
        self.calls = []
        self.store = None

    def set_batch(self, *a, **k):
        self.calls.append("set_batch")
        raise Handed

    def set_batch_frames(self, ids, mask, frames, labels, aug_params=None):
        self.calls.append(("frames", None if aug_params is None else np.array(aug_params)))
        raise Handed


def _batch(pixel_values):
    ids = torch.ones(2, 8, dtype=torch.int64)
    return dict(input_ids=ids, attention_mask=torch.ones(2, 8, dtype=torch.bool), labels=ids.clone(), pixel_values=pixel_values)


def test_finetune_loop_refuses_image_aug_on_float_pixel_values(monkeypatch):
    from bridgelang_amd.training import finetune as F
    made = []
    monkeypatch.setattr(F, "TrainStep", lambda *a, **k: made.append(StubEngine()) or made[-1])
    vlm = SimpleNamespace(weights=SimpleNamespace(dims=SimpleNamespace(n_patches=256)))
    cfg = F.FinetuneConfig(batch_size=2, use_lora=False, image_aug=True, seed=11)
    with pytest.raises(ValueError, match="uint8 frames"):
        F.finetune(vlm, [_batch(torch.zeros(2, 6, 224, 224))], None, cfg)
    assert made[-1].calls == []
    frames = torch.zeros(2, 224, 224, 3, dtype=torch.uint8)
    with pytest.raises(Handed):                              # uint8 frames: parameters drawn for (seed, rank 0, batch 0)
        F.finetune(vlm, [_batch(frames)], None, cfg)
    assert np.array_equal(made[-1].calls[0][1], A.draw_params(2, 11, 0, 0))
    off = F.FinetuneConfig(batch_size=2, use_lora=False)
    assert off.image_aug is False and off.seed == 7
    with pytest.raises(Handed):                              # image_aug off: frames path without parameters …
        F.finetune(vlm, [_batch(frames)], None, off)
    assert made[-1].calls == [("frames", None)]
    with pytest.raises(Handed):                              # … and float pixel values go through set_batch as before
        F.finetune(vlm, [_batch(torch.zeros(2, 6, 224, 224))], None, off)
    assert made[-1].calls == ["set_batch"]


def test_strategy_loop_refuses_image_aug_on_float_pixel_values(tmp_path):
    from bridgelang_amd.training.strategy import VLAMetrics, get_train_strategy

    class Stream(torch.utils.data.IterableDataset):
        def __init__(self, pv):
            self.pv = pv

        def __iter__(self):
            for _ in range(2):
                yield self.pv

    vlm = SimpleNamespace(weights=SimpleNamespace(dims=SimpleNamespace(n_patches=256)))
    strat = get_train_strategy("fsdp-shard-grad-op", vlm=vlm, device_id=0, stage="vla-train", epochs=1, max_steps=1,
                               global_batch_size=2, per_device_batch_size=2, learning_rate=1e-3, weight_decay=0.0,
                               max_grad_norm=1.0, lr_scheduler_type="constant", warmup_ratio=0.0)
    eng = StubEngine()
    strat._ensure_engine = lambda text_len: eng
    collate = lambda items: _batch(torch.stack(items))
    metrics = VLAMetrics((), "run", tmp_path, {}, resume_step=5)
    with pytest.raises(ValueError, match="uint8 frames"):
        strat.run_vla_training(Stream(torch.zeros(6, 224, 224)), collate, None, metrics, image_aug=True, seed=3)
    assert eng.calls == []
    with pytest.raises(Handed):
        strat.run_vla_training(Stream(torch.zeros(224, 224, 3, dtype=torch.uint8)), collate, None, metrics, image_aug=True, seed=3)
    assert np.array_equal(eng.calls[0][1], A.draw_params(2, 3, 0, 5))      # (seed, rank, global step)
