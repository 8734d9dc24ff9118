"""training/preference_loss.py (the fp64 specification of bl_preference_loss_f32) against a torch.autograd restatement, its
properties, its error paths, and the batch builders of training/rl.py."""
import dataclasses
import itertools
import math

import numpy as np
import pytest
import torch

from bridgelang_amd.training.policy_loss import IGNORE_INDEX
from bridgelang_amd.training.preference_loss import (KINDS, PAIR_STAT_NAMES, PREF_STAT_NAMES, SEQ_NORMS, SEQ_STAT_NAMES,
                                                     PreferenceLossConfig, check_pairs, preference_loss)

GROUP_ROWS, N = 5, 24
PAIR = np.array([1, -1, 2, 2, -2, 0], dtype=np.int32)          # a 2-vs-1 pair and a labelled sequence in no pair


def make_case(seed=0, n=N, pair=PAIR, scale=1.0):
    g = np.random.default_rng(seed)
    B = len(pair)
    rows = B * GROUP_ROWS
    logits = g.standard_normal((rows, n)) * 2 * scale
    tgt = g.integers(0, n, rows)
    keep = g.random(rows) < 0.7
    keep.reshape(B, GROUP_ROWS)[:, 1] = True                   # every sequence keeps a row
    keep[:GROUP_ROWS] = [False, True, False, False, False]     # one with a single valid row
    keep[GROUP_ROWS:2 * GROUP_ROWS] = True                     # one with all five
    tgt = np.where(keep, tgt, IGNORE_INDEX)
    ref = -np.log(n) + 0.5 * g.standard_normal(rows)
    return logits, tgt, ref


def restated(logits, tgt, pair, ref, cfg, group_rows=GROUP_ROWS):
    """The torch restatement: log_softmax, gather, logsigmoid / square / relu, means — nothing shared with the spec."""
    l = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    first, count = cfg.token_range or (0, l.shape[1])
    t = torch.tensor(tgt)
    valid = t != IGNORE_INDEX
    lsm = torch.log_softmax(l[:, first:first + count] / cfg.temperature, dim=-1)
    logp = lsm.gather(1, (t - first).clamp(min=0)[:, None])[:, 0]
    d = logp - (torch.tensor(ref, dtype=torch.float64) if ref is not None else 0.0)
    B = len(pair)
    P = int(np.abs(pair).max())
    seq = lambda v, b: v[b * group_rows:(b + 1) * group_rows][valid[b * group_rows:(b + 1) * group_rows]]
    delta = [seq(d, b).mean() if cfg.seq_norm == "mean" else seq(d, b).sum() for b in range(B)]
    total, out = 0.0, dict(pref=[], acc=[], margin=[], rc=[], rr=[], nll=[], h=[])
    for k in range(1, P + 1):
        rc = sum(delta[b] for b in range(B) if pair[b] == k)
        rr = sum(delta[b] for b in range(B) if pair[b] == -k)
        h = cfg.beta * (rc - rr) - cfg.margin
        if cfg.kind == "sigmoid":
            lk = -(1 - cfg.label_smoothing) * torch.nn.functional.logsigmoid(h) - cfg.label_smoothing * torch.nn.functional.logsigmoid(-h)
        elif cfg.kind == "ipo":
            lk = (h / cfg.beta - 1 / (2 * cfg.beta)) ** 2
        else:
            lk = torch.relu(1 - h)
        nll = -torch.cat([seq(logp, b) for b in range(B) if pair[b] == k]).mean()
        total = total + lk + cfg.sft_coef * nll
        for key, v in (("pref", lk), ("acc", float(rc - rr > 0)), ("margin", cfg.beta * (rc - rr)), ("rc", cfg.beta * rc),
                       ("rr", cfg.beta * rr), ("nll", nll), ("h", h)):
            out[key].append(float(v.detach()) if torch.is_tensor(v) else float(v))
    loss = total / P
    loss.backward()
    loss = float(loss.detach())
    stats = np.array([loss, P] + [np.mean(out[k]) for k in ("pref", "acc", "margin", "rc", "rr", "nll")])
    return loss, stats, l.grad.numpy(), np.array(out["h"])


def config(kind, norm, ref_free, **kw):
    base = dict(beta=0.3, kind=kind, seq_norm=norm, reference_free=ref_free, sft_coef=0.2, temperature=0.8,
                label_smoothing=0.1 if kind == "sigmoid" else 0.0, margin=0.0 if kind == "ipo" else 0.25)
    base.update(kw)
    return PreferenceLossConfig(**base)


@pytest.mark.parametrize("kind,norm,ref_free", list(itertools.product(KINDS, SEQ_NORMS, (False, True))))
def test_specification_matches_autograd(kind, norm, ref_free):
    cfg = config(kind, norm, ref_free)
    logits, tgt, ref = make_case(seed=3)
    ref = None if ref_free else ref
    loss, stats, grad, h = restated(logits, tgt, PAIR, ref, cfg)
    if kind == "hinge":
        assert (np.abs(h - 1.0) >= 1e-2).all()                 # no pair within reach of the kink
    res = preference_loss(logits, tgt, PAIR, ref, cfg, group_rows=GROUP_ROWS)
    assert res.n_pairs == 2 and len(PREF_STAT_NAMES) == 8 and res.pair_stats.shape == (2, len(PAIR_STAT_NAMES))
    assert res.seq_stats.shape == (len(PAIR), len(SEQ_STAT_NAMES))
    assert abs(res.loss - loss) <= 1e-12 and np.abs(res.stats - stats).max() <= 1e-12
    assert np.abs(res.pair_stats[:, 0] - h).max() <= 1e-12
    assert np.abs(res.dlogits - grad).max() <= 1e-12
    v = tgt != IGNORE_INDEX
    assert (res.dlogits[~v] == 0).all() and (res.dlogits[5 * GROUP_ROWS:] == 0).all() and np.abs(grad).max() > 1e-3


def test_hinge_both_sides_of_the_kink():
    cfg = config("hinge", "sum", True, beta=1.0, margin=0.0, sft_coef=0.0)
    logits, tgt, _ = make_case(seed=3)
    res = preference_loss(logits, tgt, PAIR, None, cfg, group_rows=GROUP_ROWS)
    swapped = preference_loss(logits, tgt, -PAIR, None, cfg, group_rows=GROUP_ROWS)
    h = np.concatenate([res.pair_stats[:, 0], swapped.pair_stats[:, 0]])
    assert (h > 1).any() and (h < 1).any() and (np.abs(h - 1) >= 1e-2).all()
    for r in (res, swapped):
        assert np.array_equal(r.pair_stats[:, 2], -(r.pair_stats[:, 0] < 1).astype(np.float64))


def test_policy_equal_to_reference_gives_log_two():
    cfg = PreferenceLossConfig(beta=0.7)
    logits, tgt, _ = make_case(seed=5)
    free = preference_loss(logits, tgt, PAIR, None, dataclasses.replace(cfg, reference_free=True), group_rows=GROUP_ROWS)
    res = preference_loss(logits, tgt, PAIR, free.logp, cfg, group_rows=GROUP_ROWS)
    st = dict(zip(PREF_STAT_NAMES, res.stats))
    assert abs(st["loss"] - math.log(2)) <= 1e-15 and st["accuracy"] == 0 and st["margin"] == 0 and st["n_pairs"] == 2


def test_swapping_sides_negates_the_margin():
    cfg = config("sigmoid", "mean", False)
    logits, tgt, ref = make_case(seed=6)
    a = preference_loss(logits, tgt, PAIR, ref, cfg, group_rows=GROUP_ROWS)
    b = preference_loss(logits, tgt, -PAIR, ref, cfg, group_rows=GROUP_ROWS)
    assert a.stats[4] == -b.stats[4] and a.stats[5] == b.stats[6] and a.stats[4] != 0


def test_unpaired_sequence_changes_nothing():
    cfg = config("sigmoid", "sum", False)
    logits, tgt, ref = make_case(seed=7)
    a = preference_loss(logits, tgt, PAIR, ref, cfg, group_rows=GROUP_ROWS)
    cut = 5 * GROUP_ROWS
    b = preference_loss(logits[:cut], tgt[:cut], PAIR[:5], ref[:cut], cfg, group_rows=GROUP_ROWS)
    assert np.array_equal(a.stats, b.stats) and np.array_equal(a.dlogits[:cut], b.dlogits) and np.array_equal(a.pair_stats, b.pair_stats)
    moved = logits.copy()
    moved[cut:] = np.nan                                        # an unpaired sequence's logits may hold anything
    c = preference_loss(moved, tgt, PAIR, ref, cfg, group_rows=GROUP_ROWS)
    assert np.array_equal(a.stats, c.stats) and np.array_equal(a.dlogits, c.dlogits)
    assert (a.g[cut:] == 0).all() and a.seq_stats[5, 3] == 0 and a.seq_stats[5, 1] > 0


def test_token_range_is_the_definition_on_sliced_rows():
    first, count = 8, 8
    cfg = config("sigmoid", "sum", False, token_range=(first, count))
    logits, tgt, ref = make_case(seed=8)
    v = tgt != IGNORE_INDEX
    tgt = np.where(v, first + tgt % count, IGNORE_INDEX)
    a = preference_loss(logits, tgt, PAIR, ref, cfg, group_rows=GROUP_ROWS)
    b = preference_loss(logits[:, first:first + count], np.where(v, tgt - first, IGNORE_INDEX), PAIR, ref,
                        dataclasses.replace(cfg, token_range=None), group_rows=GROUP_ROWS)
    assert np.array_equal(a.stats, b.stats) and np.array_equal(a.dlogits[:, first:first + count], b.dlogits)
    assert (a.dlogits[:, :first] == 0).all() and (a.dlogits[:, first + count:] == 0).all()
    outside = logits.copy()
    outside[:, :first], outside[:, first + count:] = np.nan, np.inf
    assert np.array_equal(preference_loss(outside, tgt, PAIR, ref, cfg, group_rows=GROUP_ROWS).dlogits, a.dlogits)
    with pytest.raises(ValueError):
        preference_loss(logits, np.where(v, 0, IGNORE_INDEX), PAIR, ref, cfg, group_rows=GROUP_ROWS)


def test_mean_is_sum_with_beta_over_n():
    pair = np.array([1, -1, -2, 2], dtype=np.int32)
    logits, _, ref = make_case(seed=9, pair=pair)
    g = np.random.default_rng(1)
    tgt = g.integers(0, N, 4 * GROUP_ROWS)
    tgt.reshape(4, GROUP_ROWS)[:, [0, 3]] = IGNORE_INDEX        # n_b = 3 everywhere
    for kind in ("sigmoid", "hinge"):
        mean = config(kind, "mean", False, beta=0.9)
        a = preference_loss(logits, tgt, pair, ref, mean, group_rows=GROUP_ROWS)
        b = preference_loss(logits, tgt, pair, ref, dataclasses.replace(mean, seq_norm="sum", beta=0.3), group_rows=GROUP_ROWS)
        assert np.abs(a.stats - b.stats).max() <= 1e-12 and np.abs(a.dlogits - b.dlogits).max() <= 1e-12


def test_config_errors():
    for kw in (dict(beta=0.0), dict(beta=-1.0), dict(kind="kto"), dict(label_smoothing=0.5), dict(label_smoothing=-0.1),
               dict(margin=-0.1), dict(sft_coef=-1.0), dict(seq_norm="max"), dict(temperature=0.0), dict(token_range=(0, 0)),
               dict(token_range=(-8, 8)), dict(kind="ipo", margin=0.1), dict(kind="ipo", label_smoothing=0.1),
               dict(kind="hinge", label_smoothing=0.1), dict(beta=float("nan"))):
        with pytest.raises(ValueError):
            PreferenceLossConfig(**kw)
    cfg = PreferenceLossConfig(kind="hinge", margin=0.5, token_range=(8, 16), reference_free=True)
    assert cfg.token_range == (8, 16) and cfg.backward_config().entropy_coef == 0.0 and cfg.backward_config().token_range == (8, 16)
    with pytest.raises(dataclasses.FrozenInstanceError):
        cfg.beta = 1.0


def test_precondition_errors():
    cfg = PreferenceLossConfig()
    logits, tgt, ref = make_case(seed=10)
    run = lambda **kw: preference_loss(**{**dict(logits=logits, targets=tgt, pair=PAIR, ref_logprobs=ref, cfg=cfg, group_rows=GROUP_ROWS), **kw})
    run()
    for bad in ([1, -1, 3, 3, -3, 0], [0] * 6, [1, 1, 2, -2, 0, 0], [1, -1, -2, -2, 0, 0], [2, -2, 0, 0, 0, 0]):
        with pytest.raises(ValueError):
            run(pair=np.array(bad, dtype=np.int32))
    with pytest.raises(ValueError):
        run(pair=np.array([1.0, -1, 2, 2, -2, 0]))
    with pytest.raises(ValueError):
        run(pair=PAIR[:5])
    empty = tgt.copy()
    empty[:GROUP_ROWS] = IGNORE_INDEX                            # pair 1 loses its chosen side's only labelled row
    with pytest.raises(ValueError):
        run(targets=empty)
    row = int(np.flatnonzero(tgt[:2 * GROUP_ROWS] != IGNORE_INDEX)[0])
    for name, src in (("logits", logits), ("ref_logprobs", ref)):
        for v in (np.nan, -np.inf):
            moved = src.copy()
            moved[row] = v
            with pytest.raises(ValueError):
                run(**{name: moved})
    with pytest.raises(ValueError):
        run(ref_logprobs=None)                                   # not reference_free: ref needed
    with pytest.raises(ValueError):
        run(cfg=PreferenceLossConfig(reference_free=True))       # … and refused when it is
    with pytest.raises(ValueError):
        run(group_rows=4)
    assert check_pairs(np.array([2, -1, 1, -2]), np.array([1, 1, 1, 1])) == 2


def test_preference_batch_is_policy_batch_interleaved():
    from bridgelang_amd.training.rl import policy_batch, preference_batch
    g = torch.Generator().manual_seed(0)
    B, n = 3, 7
    ids = torch.randint(3, 31000, (B, 9), generator=g)
    mask = torch.ones(B, 9, dtype=torch.bool)
    mask[1, 7:] = False
    ids[0, -1] = 29871
    ch, rj = torch.randint(31744, 32000, (B, n), generator=g), torch.randint(31744, 32000, (B, n), generator=g)
    rc, rr = -torch.rand(B, n, generator=g).double(), -torch.rand(B, n, generator=g).double()
    out = preference_batch(ids, mask, ch, rj, rc, rr, token_range=(31744, 256))
    a = policy_batch(ids, mask, ch, rc, torch.zeros(B), pad_to=out["input_ids"].shape[1])
    b = policy_batch(ids, mask, rj, rr, torch.zeros(B), pad_to=out["input_ids"].shape[1])
    for key, mine in (("input_ids", "input_ids"), ("attention_mask", "attention_mask"), ("labels", "labels"), ("old_logprobs", "ref_logprobs")):
        assert torch.equal(out[mine][0::2], a[key]) and torch.equal(out[mine][1::2], b[key]), key
    assert out["pair"].dtype == torch.int32 and out["pair"].tolist() == [1, -1, 2, -2, 3, -3]
    free = preference_batch(ids, mask, ch, rj, pad_to=24)
    assert free["ref_logprobs"] is None and free["input_ids"].shape == (2 * B, 24) and torch.equal(free["labels"][:, :out["labels"].shape[1]], out["labels"])
    traj = preference_batch(ids, mask, ch, rj, rc, rr, groups=[1, 1, 2])
    assert traj["pair"].tolist() == [1, -1, 1, -1, 2, -2]
    for kw in (dict(groups=[1, 3, 3]), dict(groups=[1, 2]), dict(ref_rejected=None), dict(token_range=(0, 8))):
        with pytest.raises(ValueError):
            preference_batch(ids, mask, ch, rj, **{**dict(ref_chosen=rc, ref_rejected=rr), **kw})
    bad = rc.clone()
    bad[0, 0] = float("-inf")
    with pytest.raises(ValueError):
        preference_batch(ids, mask, ch, rj, bad, rr)


def test_pairs_from_rewards_ties():
    from bridgelang_amd.training.rl import pairs_from_rewards
    r = np.array([[0.0, 2.0, 2.0, -1.0],      # two equal best: the lowest index
                  [1.0, 1.0, 1.0, 1.0],       # all equal: dropped
                  [3.0, 0.5, 0.5, 3.0],       # equal on both sides
                  [0.0, 0.05, 0.0, 0.0]])     # a gap below min_gap
    c, j, keep = pairs_from_rewards(r)
    assert c.tolist() == [1, 0, 0, 1] and j.tolist() == [3, 0, 1, 0] and keep.tolist() == [True, False, True, True]
    assert pairs_from_rewards(r, min_gap=0.1)[2].tolist() == [True, False, True, False]
    assert pairs_from_rewards(r, min_gap=3.0)[2].tolist() == [True, False, False, False]
    for bad in (np.zeros(3), np.array([[np.nan, 1.0]])):
        with pytest.raises(ValueError):
            pairs_from_rewards(bad)
