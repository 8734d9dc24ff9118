"""training/value_loss.py (the fp64 specification of bl_value_head_f32 / bl_value_head_backward_f32) against a
torch.autograd restatement, its value-row selection and edge cases, `rl.gae` against the direct double sum, the ValueHead
container, and the two C entry points in header, binding table and library."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from bridgelang_amd.training.value_loss import (VALUE_ROW_NAMES, VALUE_STAT_NAMES, ValueLossConfig, value_loss,
                                                value_row_index)

ROOT = Path(__file__).resolve().parents[1]
IGN = -100
D = 24
C = 0.2


def labels_case(kind: str, groups: int = 6, group_rows: int = 9):
    """targets [groups·group_rows] with: a sequence without labels, one with two labelled runs, runs at the first / last row."""
    tg = np.full((groups, group_rows), IGN, dtype=np.int64)
    if kind == "mixed":
        tg[0, 3:6] = 5                      # one run
        tg[1, 0] = 7                        # first row only
        # sequence 2: no labels
        tg[3, 2:4] = 9                      # two runs: the value row of the action level is row 2, not row 6
        tg[3, 6:8] = 9
        tg[4, group_rows - 1] = 11          # last row only
        tg[5, :] = 3                        # all
    elif kind != "none":
        raise ValueError(kind)
    return tg.reshape(-1), group_rows


def draw(tg, level, group_rows, clip, seed=0):
    """hn, w, b, R, vo with v − vo at ±0.5c and ±2c and R on either side of v, cycling over the value rows."""
    rng = np.random.default_rng(seed)
    rows = tg.shape[0]
    hn = rng.standard_normal((rows, D))
    w = rng.standard_normal(D) * 0.3
    b = 0.17
    idx = value_row_index(tg, level, group_rows)
    v = hn @ w + b
    off = np.array([0.5, -0.5, 2.0, -2.0, 2.0, -2.0, 0.5, -0.5])[np.arange(rows) % 8] * (clip if clip is not None else C)
    side = np.array([1.0, 1.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0])[np.arange(rows) % 8]
    vo = v - off
    R = v + side * (0.2 + 0.4 * rng.random(rows))       # |v − R| of many sizes: the sums over rows do not cancel
    other = np.ones(rows, dtype=bool)
    other[idx] = False
    R[other] = np.nan                       # values off the value rows are never read
    vo[other] = np.nan
    hn[other] = np.nan
    return hn, w, b, R, vo, idx


def autograd_loss(hn, w, b, R, vo, idx, cfg):
    """The torch restatement over the value rows: maximum and clamp, gradients by autograd."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64)
    hn_t = t(np.nan_to_num(hn)).requires_grad_(True)
    w_t, b_t = t(w).requires_grad_(True), t(b).requires_grad_(True)
    i = torch.from_numpy(np.asarray(idx, dtype=np.int64))
    h = hn_t.detach()[i] if cfg.detach else hn_t[i]
    v = h @ w_t + b_t
    v.retain_grad()
    e = v - t(R)[i]
    if cfg.clip is None:
        l = 0.5 * e * e
    else:
        vo_t = t(vo)[i]
        ec = vo_t + (v - vo_t).clamp(-cfg.clip, cfg.clip) - t(R)[i]
        l = 0.5 * torch.maximum(e * e, ec * ec)
    n = len(idx)
    vl = l.sum() / n if n else torch.zeros((), dtype=torch.float64)
    if n:
        (cfg.coef * vl).backward()
    z = lambda x, like: x.grad if x.grad is not None else torch.zeros_like(like)
    return vl.item(), v, z(v, v), z(w_t, w_t), z(b_t, b_t), z(hn_t, hn_t)


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    assert np.all(np.abs(got - want) <= 1e-12 * max(scale, 1e-300)), (what, np.abs(got - want).max(), scale)


@pytest.mark.parametrize("level", ["action", "token"])
@pytest.mark.parametrize("clip", [None, C])
def test_definition_matches_autograd(level, clip):
    tg, gr = labels_case("mixed")
    cfg = ValueLossConfig(coef=0.7, clip=clip, level=level)
    hn, w, b, R, vo, idx = draw(tg, level, gr, clip)
    res = value_loss(hn, tg, w, b, R, vo if clip is not None else None, cfg, group_rows=gr, policy_loss=0.25)
    assert np.array_equal(res.index, idx) and res.stats[1] == len(idx)
    if level == "action":                   # no-label sequence has none; the two-run sequence has its first run's first row
        assert list(idx) == [3, 9, 3 * gr + 2, 4 * gr + gr - 1, 5 * gr]
    else:
        assert len(idx) == int((tg != IGN).sum())
    vl, v, dv, dw, db, dhn = autograd_loss(hn, w, b, R, vo, idx, cfg)
    close(res.value_loss, vl, "value_loss")
    close(res.value[idx], v.detach().numpy(), "v")
    close(res.dv[idx], dv.numpy(), "dv")
    close(res.dw, dw.numpy(), "dw")
    close(res.db, db.numpy(), "db")
    close(res.dhn, dhn.numpy(), "dhn")
    assert res.total == pytest.approx(0.25 + 0.7 * vl, rel=1e-14)
    assert np.isfinite(res.rows).all() and np.isfinite(res.stats).all() and np.isfinite(res.dhn).all()
    other = np.ones(len(tg), dtype=bool)
    other[idx] = False
    assert not res.rows[other].any() and not res.dhn[other].any()
    if clip is not None:                    # both branches of the max are selected
        assert 0 < res.stats[2] < 1
        e = res.value[idx] - R[idx]
        assert np.array_equal(res.clipped[idx], res.dl_dv[idx] == 0) and np.array_equal(res.dl_dv[idx][~res.clipped[idx]], e[~res.clipped[idx]])
    else:
        assert res.stats[2] == 0
    # the statistics, from their definitions
    e = res.value[idx] - R[idx]
    want = [res.loss[idx].mean(), len(idx), res.clipped[idx].mean(), res.value[idx].mean(), R[idx].mean(),
            1 - ((e - e.mean()) ** 2).sum() / ((R[idx] - R[idx].mean()) ** 2).sum(), np.abs(e).mean(), res.total]
    close(res.stats, want, "stats")
    assert len(VALUE_STAT_NAMES) == 8 and VALUE_ROW_NAMES == ("value", "loss", "clipped", "dv") and res.rows.shape == (len(tg), 4)


@pytest.mark.parametrize("level", ["action", "token"])
def test_no_value_row_gives_zeros(level):
    tg, gr = labels_case("none")
    hn = np.full((tg.shape[0], D), np.nan)
    res = value_loss(hn, tg, np.ones(D), 0.5, np.full(tg.shape[0], np.nan), np.full(tg.shape[0], np.nan),
                     ValueLossConfig(level=level), group_rows=gr, policy_loss=1.5)
    assert res.index.size == 0 and res.value_loss == 0 and res.total == 1.5 and res.db == 0
    assert not res.dw.any() and not res.dhn.any() and not res.rows.any()
    assert list(res.stats) == [0, 0, 0, 0, 0, 0, 0, 1.5]


def test_detach_zeroes_dhn_only():
    tg, gr = labels_case("mixed")
    hn, w, b, R, vo, idx = draw(tg, "token", gr, C)
    a = value_loss(hn, tg, w, b, R, vo, ValueLossConfig(level="token"), group_rows=gr)
    d = value_loss(hn, tg, w, b, R, vo, ValueLossConfig(level="token", detach=True), group_rows=gr)
    assert a.dhn.any() and not d.dhn.any()
    assert np.array_equal(a.dw, d.dw) and a.db == d.db and np.array_equal(a.rows, d.rows) and np.array_equal(a.stats, d.stats)
    _, _, _, dw, db, dhn = autograd_loss(hn, w, b, R, vo, idx, ValueLossConfig(level="token", detach=True))
    close(d.dw, dw.numpy(), "dw")
    assert not dhn.any()


def test_explained_variance_and_inv_world():
    tg, gr = labels_case("mixed")
    hn, w, b, R, vo, idx = draw(tg, "token", gr, None)
    R[idx] = 2.0                            # constant returns: the denominator is 0
    res = value_loss(hn, tg, w, b, R, None, ValueLossConfig(clip=None, level="token"), group_rows=gr)
    assert res.stats[5] == 0
    half = value_loss(hn, tg, w, b, R, None, ValueLossConfig(clip=None, level="token"), group_rows=gr, inv_world=0.5)
    close(half.dw, 0.5 * res.dw, "dw / world")
    assert half.value_loss == res.value_loss


def test_validation():
    for bad in (dict(level="sequence"), dict(coef=-1.0), dict(coef=float("nan")), dict(clip=0.0), dict(clip=-0.1),
                dict(clip=float("inf")), dict(detach=1)):
        with pytest.raises(ValueError):
            ValueLossConfig(**bad)
    assert ValueLossConfig() == ValueLossConfig(coef=0.5, clip=0.2, level="action", detach=False)
    tg, gr = labels_case("mixed")
    hn, w, b, R, vo, idx = draw(tg, "action", gr, C)
    with pytest.raises(ValueError):
        value_loss(hn, tg, w, b, R, None, ValueLossConfig(), group_rows=gr)              # clip needs old values
    with pytest.raises(ValueError):
        value_loss(hn, tg, w, b, R, vo, ValueLossConfig(), group_rows=None)              # action level needs the sequences
    with pytest.raises(ValueError):
        value_loss(hn, tg, w, b, R, vo, ValueLossConfig(), group_rows=7)
    for which in (0, 1):
        x = [R.copy(), vo.copy()]
        x[which][idx[1]] = np.inf
        with pytest.raises(ValueError):
            value_loss(hn, tg, w, b, x[0], x[1], ValueLossConfig(), group_rows=gr)
    value_loss(hn, tg, w, b, R, None, ValueLossConfig(clip=None), group_rows=gr)


def test_gae_matches_the_double_sum():
    from bridgelang_amd.training.rl import gae
    rng = np.random.default_rng(4)
    N, T = 3, 11
    r, v, last = rng.standard_normal((N, T)), rng.standard_normal((N, T)), rng.standard_normal(N)
    done = np.zeros((N, T), dtype=bool)
    done[0, 4] = done[1, 0] = done[1, 7] = done[2, T - 1] = True
    for gamma, lam in ((0.99, 0.95), (0.9, 0.0), (0.97, 1.0)):
        for dn, lv in ((done, last), (None, last), (done, None), (None, None)):
            adv, ret = gae(r, v, lv, dn, gamma=gamma, lam=lam)
            assert adv.dtype == torch.float32 and tuple(adv.shape) == (N, T) == tuple(ret.shape)
            d = np.zeros((N, T)) if dn is None else dn.astype(np.float64)
            vnext = np.concatenate([v[:, 1:], (np.zeros(N) if lv is None else lv)[:, None]], axis=1)
            delta = r + gamma * vnext * (1 - d) - v
            want = np.zeros((N, T))
            for n in range(N):
                for t in range(T):          # A_t = Σ_{k ≥ t} (γλ)^{k−t} · Π_{t ≤ j < k} (1 − done_j) · δ_k
                    live = 1.0
                    for k in range(t, T):
                        want[n, t] += (gamma * lam) ** (k - t) * live * delta[n, k]
                        live *= 1 - d[n, k]
            assert np.abs(adv.double().numpy() - want).max() <= 2.0 ** -23 * np.abs(want).max()
            assert np.abs(ret.double().numpy() - (want + v)).max() <= 2.0 ** -23 * np.abs(want + v).max()
    a0, _ = gae(r, v, last, done, gamma=0.9, lam=0.0)                                    # λ = 0: the one-step TD error
    vnext = np.concatenate([v[:, 1:], last[:, None]], axis=1)
    assert np.abs(a0.double().numpy() - (r + 0.9 * vnext * (1 - done) - v)).max() <= 2.0 ** -22
    for bad in (dict(values=v[:, :-1]), dict(last_values=last[:-1]), dict(dones=done[:, :-1])):
        kw = dict(rewards=r, values=v, last_values=last, dones=done)
        kw.update(bad)
        with pytest.raises(ValueError):
            gae(**kw)
    nan = r.copy()
    nan[0, 0] = np.nan
    with pytest.raises(ValueError):
        gae(nan, v)
    with pytest.raises(ValueError):
        gae(r, v, np.full(N, np.inf))


def test_value_head_container(tmp_path):
    from bridgelang_amd.training.value_head import ValueHead
    vh = ValueHead(64, "cpu")
    assert vh.weight.dtype == torch.bfloat16 and tuple(vh.weight.shape) == (64,) and tuple(vh.bias.shape) == (1,)
    assert not vh.weight.any() and not vh.bias.any()                                     # a fresh head changes nothing
    units = vh.plain_units()
    assert [(n, d, k) for n, _, d, k in units] == [("value_head.weight", True, "value_head.weight"),
                                                   ("value_head.bias", False, "value_head.bias")]
    assert units[0][1].data_ptr() == vh.weight.data_ptr() and units[1][1].data_ptr() == vh.bias.data_ptr()
    from bridgelang_amd.training.step import no_decay, param_sharded_key
    assert not no_decay("value_head.weight", (1, 64)) and no_decay("value_head.bias", (1,))
    assert not any(param_sharded_key(k) for *_, k in units)
    drawn = ValueHead(64, "cpu", init_std=0.02, seed=5)
    assert drawn.weight.any() and torch.equal(drawn.weight, ValueHead(64, "cpu", init_std=0.02, seed=5).weight)
    drawn.bias.fill_(0.25)
    sd = drawn.state_dict()
    assert tuple(sd["value_head.weight"].shape) == (1, 64) and tuple(sd["value_head.bias"].shape) == (1,)
    assert all(v.dtype == torch.float32 for v in sd.values())
    ptr = vh.weight.data_ptr()
    vh.load_state_dict(sd)
    assert vh.weight.data_ptr() == ptr and torch.equal(vh.weight, drawn.weight) and torch.equal(vh.bias, drawn.bias)
    masters = {"value_head.weight": torch.arange(64, dtype=torch.float32) / 7, "value_head.bias": torch.tensor([1.0 / 3])}
    msd = drawn.state_dict(masters)                                                      # fp32 masters, not the bf16 values
    assert torch.equal(msd["value_head.weight"], masters["value_head.weight"].view(1, 64)) and msd["value_head.bias"].item() == masters["value_head.bias"].item()
    path = drawn.save(tmp_path / "adapter")
    assert path.name == "value_head.safetensors" and path.exists()
    back = ValueHead.load(tmp_path / "adapter", "cpu")
    assert back.dim == 64 and torch.equal(back.weight, drawn.weight) and torch.equal(back.bias, drawn.bias)
    with pytest.raises(ValueError):
        vh.load_state_dict({"value_head.weight": torch.zeros(1, 32), "value_head.bias": torch.zeros(1)})
    with pytest.raises(ValueError):
        ValueHead(12, "cpu")
    with pytest.raises(FileNotFoundError):
        ValueHead.load(tmp_path, "cpu")


def test_entry_points_declared_bound_and_exported():
    from bridgelang_amd import _lib
    header = (ROOT / "include" / "bridgelang_hip.h").read_text()
    declared = set(re.findall(r"\b(bl_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name, n_args in (("bl_value_head_f32", 20), ("bl_value_head_backward_f32", 16)):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(proto.split(",")) == n_args == len(_lib.SIGNATURES[name][1])
    assert "value.hip" in (ROOT / "bridgelang_amd" / "csrc" / "Makefile").read_text()
