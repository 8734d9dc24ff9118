"""GPU: bl_augment_frames_u8 (OpenVLA's training-time image augmentation on uint8 frames in HBM) against its host
specification vla/image_augment.py::augment_frame — byte for byte, no tolerance: the kernel is a pure function of
(frames, params) and both sides round every fp32 operation on its own — plus the frames input path of the training step
and of both training loops built on it."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from test_data_cpu import WordTokenizer

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 16, 8), (3, 37, 53), (2, 224, 224)]       # partial waves, 3-byte pixel tails, the model resolution


def edge_cases(H, W):
    """(frames [N, H, W, 3] uint8, params [N, 8] fp32): drawn rows mixed with the hand-picked edges of every operation."""
    from bridgelang_amd.vla import image_augment as A
    rs = np.random.RandomState(H * 1000 + W)
    drawn = A.draw_params(16, seed=5, rank=2, step=H)
    s, f = A.crop_side(), np.float32
    room = f(1.0) - s
    rand = lambda lo=0, hi=256: rs.randint(lo, hi, (H, W, 3), dtype=np.uint8)
    primaries = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 128, 0],
                          [0, 0, 0], [255, 255, 255], [200, 200, 200], [1, 0, 0], [254, 255, 255]], dtype=np.uint8)
    prim = primaries[rs.randint(0, len(primaries), (H, W))]
    solid = lambda rgb: np.broadcast_to(np.array(rgb, dtype=np.uint8), (H, W, 3)).copy()
    ident = A.IDENTITY_PARAMS
    rows = [(rand(), drawn[0]), (rand(), drawn[1]), (rand(), ident)]
    p = drawn[2].copy(); p[0] = p[1] = 0.0                          # the box touches the top / left border
    rows.append((rand(), p))
    p = drawn[3].copy(); p[0] = p[1] = room                         # … the bottom / right border: floor == ceil, y2 rounds to 1
    rows.append((rand(), p))
    p = drawn[4].copy(); p[0], p[1] = 0.0, room
    rows.append((prim, p))
    p = drawn[5].copy(); p[4], p[5] = -0.2, 1.2                     # brightness clips at 0 on a near-black frame
    rows.append((rand(0, 13), p))
    p = drawn[6].copy(); p[4], p[5] = 0.2, 0.8                      # … and at 1 on a near-white one
    rows.append((rand(243, 256), p))
    p = ident.copy(); p[5] = 1.2
    rows.append((rand(), p))
    p = ident.copy(); p[5] = 0.8
    rows.append((prim, p))
    p = ident.copy(); p[6] = 1.2                                    # S·1.2 clips at 1 on the primaries
    rows.append((prim, p))
    p = drawn[7].copy(); p[6] = 1.2
    rows.append((prim, p))
    p = ident.copy(); p[7] = -0.05                                  # red: h = 0, h + δ wraps below 0
    rows.append((solid([255, 0, 0]), p))
    p = drawn[8].copy(); p[7] = -0.05
    rows.append((solid([255, 0, 0]), p))
    p = ident.copy(); p[7] = 0.05
    rows.append((prim, p))
    rows.append((solid([93, 93, 93]), drawn[9]))                    # range == 0
    rows.append((solid([0, 0, 0]), drawn[10]))                      # V == 0
    p = drawn[11].copy(); p[4] = -0.1
    rows.append((solid([0, 0, 0]), p))
    frames = np.stack([r[0] for r in rows])
    params = np.stack([np.asarray(r[1], dtype=np.float32) for r in rows])
    return frames, params


_REF = {}


def reference(H, W):
    """The edge cases of one frame size with their host results, computed once per session and never written to."""
    if (H, W) not in _REF:
        from bridgelang_amd.vla.image_augment import augment_frame
        frames, params = edge_cases(H, W)
        want = np.stack([augment_frame(fr, p) for fr, p in zip(frames, params)])
        for a in (frames, params, want):
            a.setflags(write=False)
        _REF[(H, W)] = (frames, params, want)
    return _REF[(H, W)]


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_device_twin_byte_for_byte(dev, B, H, W):
    from bridgelang_amd.vla.image_augment import augment_frames_gpu
    frames, params, want = reference(H, W)
    n = len(frames)
    assert (want != frames).any()
    idx = np.arange((n + B - 1) // B * B) % n                       # every edge row, in full batches of B
    bad = []
    for k in range(0, len(idx), B):
        sel = idx[k:k + B]
        got = augment_frames_gpu(torch.from_numpy(frames[sel]).to(dev), params[sel]).cpu().numpy()
        assert got.shape == (B, H, W, 3) and got.dtype == np.uint8
        for j, row in enumerate(sel):
            diff = int((got[j] != want[row]).sum())
            if diff:
                bad.append((int(row), diff, int(np.abs(got[j].astype(int) - want[row].astype(int)).max())))
    print("rows", n, "mismatching (row, bytes, max |Δ|):", bad)
    assert not bad, bad


def test_rows_of_a_batch_do_not_leak(dev):
    from bridgelang_amd.vla.image_augment import augment_frames_gpu
    frames, params, want = reference(37, 53)
    sel = np.array([6, 12, 1])                                      # near-black, red, random: very different channel means
    perm = np.array([2, 0, 1])
    a = augment_frames_gpu(torch.from_numpy(frames[sel]).to(dev), params[sel]).cpu().numpy()
    b = augment_frames_gpu(torch.from_numpy(frames[sel[perm]]).to(dev), params[sel[perm]]).cpu().numpy()
    assert np.array_equal(a, want[sel]) and np.array_equal(b, a[perm])
    crossed = augment_frames_gpu(torch.from_numpy(frames[sel]).to(dev), params[sel[perm]]).cpu().numpy()
    assert not np.array_equal(crossed, a)                           # the parameters do act per row


def test_fused_pixel_values_equal_preprocess_of_the_uint8_output(dev):
    from bridgelang_amd import ops
    from bridgelang_amd._lib import BridgeLangHipError
    from bridgelang_amd.extern.hf.processing_prismatic import PrismaticImageProcessor
    frames, params, want = reference(224, 224)
    ip = PrismaticImageProcessor()
    sel = np.array([0, 5])
    F, P = torch.from_numpy(frames[sel]).to(dev), torch.from_numpy(params[sel]).to(dev)
    out = torch.empty_like(F)
    pv_both = torch.zeros(2, 6, 224, 224, dtype=torch.bfloat16, device=dev)
    ops.augment_frames_u8(F, P, out=out, pixel_values=pv_both, mean_std=ip.mean_std(F.device))
    pv_only = torch.zeros_like(pv_both)
    ops.augment_frames_u8(F, P, pixel_values=pv_only, mean_std=ip.mean_std(F.device))
    assert np.array_equal(out.cpu().numpy(), want[sel])
    ref = ip.preprocess_frames_gpu(out)
    assert torch.equal(pv_both, ref) and torch.equal(pv_only, ref)
    with pytest.raises(BridgeLangHipError, match="shape"):          # the fused output needs H·W % 8 == 0
        small = torch.zeros(1, 5, 5, 3, dtype=torch.uint8, device=dev)
        ops.augment_frames_u8(small, P[:1].contiguous(), pixel_values=torch.zeros(1, 6, 5, 5, dtype=torch.bfloat16, device=dev),
                              mean_std=ip.mean_std(F.device))
    with pytest.raises(ValueError):
        ops.augment_frames_u8(torch.zeros(1, 1, 8, 3, dtype=torch.uint8, device=dev), P[:1].contiguous(),
                              out=torch.zeros(1, 1, 8, 3, dtype=torch.uint8, device=dev))


def test_workspace_is_zeroed_inside_the_call(dev):
    from bridgelang_amd import ops
    frames, params, want = reference(37, 53)
    sel = np.array([1, 8, 3])
    F, P = torch.from_numpy(frames[sel]).to(dev), torch.from_numpy(params[sel]).to(dev)
    ws = torch.full((3, 3), 0x1234567890, dtype=torch.int64, device=dev)
    a, b = torch.empty_like(F), torch.empty_like(F)
    op = ops.augment_frames_u8(F, P, out=a, workspace=ws)
    sums = ws.cpu().numpy().copy()
    ops.augment_frames_u8(F, P, out=b, workspace=ws)
    op.run()                                                        # and replayed as a prepared Op
    assert np.array_equal(a.cpu().numpy(), want[sel]) and torch.equal(a, b)
    assert np.array_equal(ws.cpu().numpy(), sums) and (sums > 0).all() and (sums <= 37 * 53 * 2 ** 24).all()


# ---- the training step and loops on the tiny model ----------------------------------------------------------------------
def _tiny(dev, seed=1):
    from bridgelang_amd import weights as W
    from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
    from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
    return OpenVLAForActionPrediction(OpenVLAConfig(norm_stats={}), device=dev, dims=W.tiny_dims()).init_synthetic(seed=seed)


def test_set_batch_frames_fills_pixel_values_like_the_host_transform(dev):
    from PIL import Image
    from bridgelang_amd.extern.hf.processing_prismatic import PrismaticImageProcessor
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.vla.image_augment import augment_frames_gpu, draw_params
    from bridgelang_amd import ops
    vlm = _tiny(dev)
    eng = TrainStep(vlm.weights, "vla-train", 2, 16)
    ip = PrismaticImageProcessor()
    ids = torch.randint(3, 1000, (2, 9), generator=torch.Generator().manual_seed(0))
    mask = torch.ones(2, 9, dtype=torch.bool)
    for H, W in ((224, 224), (100, 300)):                           # at the model resolution, and with the resize in front
        frames = np.random.RandomState(H).randint(0, 256, (2, H, W, 3), dtype=np.uint8)
        host = torch.stack([ip.apply_transform(Image.fromarray(f)) for f in frames])
        eng.set_batch(ids, mask, host, ids)
        want = eng.pixel_values.clone()
        state = [t.clone() for t in (eng.input_ids, eng.key_mask, eng.targets)]
        eng.pixel_values.zero_()
        eng.set_batch_frames(ids, mask, torch.from_numpy(frames), ids)
        assert torch.equal(eng.pixel_values, want)
        assert all(torch.equal(a, b) for a, b in zip(state, (eng.input_ids, eng.key_mask, eng.targets)))
        params = draw_params(2, 7, 0, 0)
        eng.set_batch_frames(ids, mask, torch.from_numpy(frames), ids, aug_params=params)
        resized = ops.resize_bicubic_u8(torch.from_numpy(frames).to(dev), 224, 224) if (H, W) != (224, 224) else torch.from_numpy(frames).to(dev)
        two_step = ip.preprocess_frames_gpu(augment_frames_gpu(resized, params))
        assert torch.equal(eng.pixel_values, two_step) and not torch.equal(eng.pixel_values, want)


def _finetune_losses(dev, tmp_path, tag, image_aug, seed):
    from bridgelang_amd.training.finetune import FinetuneConfig, finetune
    from bridgelang_amd.util.data_utils import PaddedCollatorForActionPrediction
    from bridgelang_amd.vla.action_tokenizer import ActionTokenizer
    from bridgelang_amd.vla.datasets import DummyDataset, raw_frame_transform
    vlm = _tiny(dev)
    tok = WordTokenizer()
    at = ActionTokenizer(tok)
    ds = DummyDataset(at, tok, raw_frame_transform, length=8, seed=0)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, collate_fn=PaddedCollatorForActionPrediction(2048, tok.pad_token_id,
                                                                                                      padding_side="right"))
    cfg = FinetuneConfig(run_root_dir=tmp_path / f"run-{tag}", adapter_tmp_dir=tmp_path / f"adapter-{tag}", batch_size=2,
                         max_steps=2, learning_rate=2e-3, log_every=1, image_aug=image_aug, seed=seed)
    out = finetune(vlm, loader, at, cfg, log_path=tmp_path / f"log-{tag}.jsonl")
    assert out["steps"] == 2
    return [json.loads(l)["train_loss"] for l in open(tmp_path / f"log-{tag}.jsonl")]


def test_finetune_with_image_aug_is_seeded_and_differs_from_plain(dev, tmp_path):
    a = _finetune_losses(dev, tmp_path, "a", True, 7)
    b = _finetune_losses(dev, tmp_path, "b", True, 7)
    plain = _finetune_losses(dev, tmp_path, "plain", False, 7)
    print("losses aug", a, "again", b, "plain", plain)
    assert len(a) == 2 and all(np.isfinite(a)) and a == b
    assert a[0] != plain[0] and a[1] != plain[1]


def test_finetune_script_runs_with_image_aug(dev, tmp_path):
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29589")
    cmd = ["--vla_path", "synthetic:openvla-tiny", "--dataset_name", "dummy", "--run_root_dir", str(tmp_path / "runs"),
           "--adapter_tmp_dir", str(tmp_path / "adapters"), "--batch_size", "2", "--max_steps", "2", "--save_steps", "2",
           "--image_aug", "True", "--dummy_length", "8"]
    p = subprocess.run([sys.executable, str(ROOT / "vla-scripts" / "finetune.py")] + cmd, env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    run = next((tmp_path / "runs").iterdir())
    assert run.name.endswith("--image_aug")
    rows = [json.loads(l) for l in open(run / "train_log.jsonl")]
    assert rows and all(np.isfinite(r["train_loss"]) for r in rows)
    assert (run / "model.safetensors").exists() and json.loads((run / "finetune_config.json").read_text())["image_aug"] == "True"
