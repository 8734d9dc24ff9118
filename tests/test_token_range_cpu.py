"""The restricted policy on the host: `vocab=(first, count)` of the sampling specification and `token_range` of the
policy-loss specification are the unrestricted definitions on the sliced row, and the glue (`policy_batch`,
`PolicyLossConfig`) refuses tokens the restricted policy cannot produce."""
import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S
from bridgelang_amd.training.policy_loss import IGNORE_INDEX, PolicyLossConfig, policy_loss

V, ACTIONS = 32064, (31744, 256)
# per-row settings: greedy, temperature only, top-k, top-p, both
SETTINGS = [(0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 8, 1.0), (1.5, 0, 0.9), (2.0, 50, 0.95), (0.5, 3, 0.5)]


def rows_and_settings(rows, n, seed):
    g = torch.Generator().manual_seed(seed)
    l = (torch.randn(rows, n, generator=g) * 3).to(torch.bfloat16).float().numpy()
    T, k, p = (np.array([SETTINGS[r % len(SETTINGS)][c] for r in range(rows)]) for c in range(3))
    seeds = np.random.default_rng(seed).integers(-(1 << 63), (1 << 63) - 1, rows, dtype=np.int64)
    return l, T.astype(np.float32), k.astype(np.int32), p.astype(np.float32), seeds


@pytest.mark.parametrize("n,first,count", [(64, 60, 4), (64, 8, 8), (2056, 1032, 256), (2056, 0, 2056)])
def test_ranged_sampler_is_the_sampler_on_the_slice(n, first, count):
    l, T, k, p, seeds = rows_and_settings(24, n, seed=n + first)
    for t in (0, 5):
        ids, wt = S.sample_rows(l, T, k, p, seeds, t, vocab=(first, count))
        want_ids, want_wt = S.sample_rows(l[:, first:first + count], T, k, p, seeds, t)
        assert np.array_equal(ids, want_ids + first) and np.array_equal(wt, want_wt)
        assert ((ids >= first) & (ids < first + count)).all()
    greedy = T == 0
    assert greedy.any() and np.array_equal(ids[greedy], first + l[greedy, first:first + count].argmax(-1))
    poisoned = l.copy()                                     # nothing outside the range is looked at
    poisoned[:, :first], poisoned[:, first + count:] = np.nan, np.inf
    again = S.sample_rows(poisoned, T, k, p, seeds, 5, vocab=(first, count))
    assert np.array_equal(again[0], ids) and np.array_equal(again[1], wt)


def test_full_range_equals_no_range():
    n = 260
    l, T, k, p, seeds = rows_and_settings(12, n, seed=3)
    a, b = S.sample_rows(l, T, k, p, seeds, 2), S.sample_rows(l, T, k, p, seeds, 2, vocab=(0, n))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    tok = a[0]
    c, d = S.score_rows(l, T, k, p, tok, 4, 16), S.score_rows(l, T, k, p, tok, 4, 16, vocab=(0, n))
    assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1]) and np.array_equal(c[0], a[1])
    for r in range(12):
        assert S.sample_row(l[r], T[r], k[r], p[r], int(seeds[r]), 2, vocab=(0, n)) == S.sample_row(l[r], T[r], k[r], p[r], int(seeds[r]), 2)
        assert S.score_row(l[r], T[r], k[r], p[r], int(tok[r]), vocab=(0, n)) == S.score_row(l[r], T[r], k[r], p[r], int(tok[r]))


def test_scorer_returns_the_ranged_samplers_pair():
    n, first, count = 520, 256, 64
    l, T, k, p, seeds = rows_and_settings(len(SETTINGS), n, seed=9)
    for r in range(len(SETTINGS)):
        args = (l[r], T[r], k[r], p[r])
        drawn = {}
        for s in range(96):                                  # what the sampler draws, over many seeds and steps
            i, w, total = S.sample_row(*args, seed=1000 * r + s, t=s % 7, vocab=(first, count))
            assert first <= i < first + count
            drawn[i] = (w, total)
        for i, pair in drawn.items():
            assert S.score_row(*args, i, vocab=(first, count)) == pair
        if T[r] > 0:                                         # and every token of the support, drawn or not
            kept = S.kept_weights(l[r, first:first + count], T[r], int(k[r]), float(p[r]))
            total = int(kept.sum())
            for j in np.flatnonzero(kept):
                assert S.score_row(*args, first + int(j), vocab=(first, count)) == (int(kept[j]), total)
        for outside in (0, first - 1, first + count, n - 1):
            w, total = S.score_row(*args, outside, vocab=(first, count))
            assert w == 0 and total == S.score_row(*args, first, vocab=(first, count))[1]
    tok = np.array([first + 3, 0, first + count - 1, n - 1, first, first - 1])
    wt, rw = S.score_rows(l, T, k, p, tok, first + 8, 16, vocab=(first, count))
    want_wt, want_rw = S.score_rows(l[:, first:first + count], T, k, p, np.clip(tok - first, 0, count - 1), 8, 16)
    inside = (tok >= first) & (tok < first + count)
    assert np.array_equal(wt[:, 1], want_wt[:, 1]) and np.array_equal(wt[inside, 0], want_wt[inside, 0]) and (wt[~inside, 0] == 0).all()
    assert np.array_equal(rw, want_rw) and rw.dtype == np.int32
    for f, c in ((first - 1, 4), (first + count - 2, 4), (0, 4), (first, count + 1)):
        with pytest.raises(ValueError):
            S.score_rows(l, T, k, p, tok, f, c, vocab=(first, count))
    for bad in ((-4, 8), (n - 4, 8), (8, 0)):
        with pytest.raises(ValueError):
            S.sample_rows(l, T, k, p, seeds, 0, vocab=bad)


def test_unranged_draws_leave_the_action_tokens_and_ranged_draws_do_not():
    """The defect and its repair on one fixed input: temperature draws over the whole 32 064-row vocabulary land on tokens
    that are no action; the same rows and seeds under the restricted policy never do."""
    rows = 8
    g = torch.Generator().manual_seed(2024)
    l = (torch.randn(rows, V, generator=g) * 2).to(torch.bfloat16).float().numpy()
    T, k, p = np.full(rows, 1.0, np.float32), np.zeros(rows, np.int32), np.ones(rows, np.float32)
    seeds = np.arange(500, 500 + rows, dtype=np.int64)
    first, count = ACTIONS
    outside = 0
    for t in range(7):
        free, _ = S.sample_rows(l, T, k, p, seeds, t)
        bound, wt = S.sample_rows(l, T, k, p, seeds, t, vocab=ACTIONS)
        outside += int(((free < first) | (free >= first + count)).sum())
        assert ((bound >= first) & (bound < first + count)).all()
        assert np.isfinite(S.logprob(wt)).all()
    assert outside >= 1


# ---- the policy loss ---------------------------------------------------------------------------------------------------------
def loss_case(n, first, count, seed=0, rows=12):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(rows, n, generator=g) * 2).to(torch.bfloat16).float()
    tgt = first + torch.randint(0, count, (rows,), generator=g)
    tgt[1], tgt[2] = first, first + count - 1
    tgt[::3] = IGNORE_INDEX
    A = torch.randn(rows, generator=g)
    q = -3.0 + 0.4 * torch.randn(rows, generator=g)
    ref = -3.0 + 0.4 * torch.randn(rows, generator=g)
    return logits, tgt, A, q, ref


@pytest.mark.parametrize("n,first,count", [(64, 8, 8), (2056, 1032, 256), (2056, 0, 2056)])
def test_ranged_policy_loss_is_the_loss_on_the_slice(n, first, count):
    logits, tgt, A, q, ref = loss_case(n, first, count)
    base = dict(temperature=0.7, clip_low=0.2, clip_high=0.25, entropy_coef=0.01, kl_coef=0.1)
    got = policy_loss(logits.numpy(), tgt.numpy(), A.numpy(), q.numpy(), ref.numpy(), PolicyLossConfig(token_range=(first, count), **base))
    shifted = torch.where(tgt != IGNORE_INDEX, tgt - first, tgt)
    want = policy_loss(logits[:, first:first + count].numpy(), shifted.numpy(), A.numpy(), q.numpy(), ref.numpy(), PolicyLossConfig(**base))
    for name in ("logp", "entropy", "ratio", "pg", "kl", "row_loss", "clipped", "valid", "g", "stats"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert got.loss == want.loss and got.dlogits.shape == (logits.shape[0], n)
    assert np.array_equal(got.dlogits[:, first:first + count], want.dlogits)
    outside = np.ones(n, bool)
    outside[first:first + count] = False
    assert (got.dlogits[:, outside] == 0).all() and (got.dlogits[~got.valid] == 0).all()
    if count < n:                                            # nothing outside the range is looked at
        poisoned = logits.numpy().copy()
        poisoned[:, outside] = np.nan
        again = policy_loss(poisoned, tgt.numpy(), A.numpy(), q.numpy(), ref.numpy(), PolicyLossConfig(token_range=(first, count), **base))
        assert np.array_equal(again.dlogits, got.dlogits) and again.loss == got.loss


def test_ranged_policy_loss_against_autograd():
    n, first, count = 2056, 1032, 256
    logits, tgt, A, q, ref = loss_case(n, first, count, seed=4)
    cfg = PolicyLossConfig(temperature=0.9, clip_low=0.2, clip_high=0.2, entropy_coef=0.02, kl_coef=0.05, token_range=(first, count))
    got = policy_loss(logits.numpy(), tgt.numpy(), A.numpy(), q.numpy(), ref.numpy(), cfg)
    x = logits.double().requires_grad_(True)
    valid = tgt != IGNORE_INDEX
    lsm = torch.log_softmax(x[:, first:first + count] / cfg.temperature, dim=-1)[valid]
    logp = lsm.gather(1, (tgt[valid] - first)[:, None])[:, 0]
    Ad, qd, rd = A[valid].double(), q[valid].double(), ref[valid].double()
    ratio = torch.exp(logp - qd)
    pg = -torch.minimum(ratio * Ad, ratio.clamp(1 - cfg.clip_low, 1 + cfg.clip_high) * Ad)
    H = -(lsm.exp() * lsm).sum(-1)
    d = rd - logp
    loss = (pg - cfg.entropy_coef * H + cfg.kl_coef * (torch.exp(d) - d - 1)).mean()
    loss.backward()
    assert abs(got.loss - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    assert np.abs(got.dlogits - x.grad.numpy()).max() <= 1e-12 * np.abs(x.grad.numpy()).max()
    assert (x.grad[:, :first] == 0).all() and (x.grad[:, first + count:] == 0).all()
    assert np.abs(got.logp[valid.numpy()] - logp.detach().numpy()).max() <= 1e-12


def test_target_outside_the_range_raises():
    n, first, count = 64, 8, 8
    logits, tgt, A, q, _ = loss_case(n, first, count)
    cfg = PolicyLossConfig(token_range=(first, count))
    for bad in (first - 1, first + count, 0, n - 1):
        t = tgt.clone()
        t[1] = bad
        with pytest.raises(ValueError, match="token_range"):
            policy_loss(logits.numpy(), t.numpy(), A.numpy(), q.numpy(), cfg=cfg)
    t = tgt.clone()
    t[0] = IGNORE_INDEX                                      # an ignored row may hold anything
    policy_loss(logits.numpy(), t.numpy(), A.numpy(), q.numpy(), cfg=cfg)
    with pytest.raises(ValueError, match="token_range"):
        policy_loss(logits.numpy(), tgt.numpy(), A.numpy(), q.numpy(), cfg=PolicyLossConfig(token_range=(60, 8)))


def test_config_validation():
    assert PolicyLossConfig().token_range is None
    assert PolicyLossConfig(token_range=[31744, 256]).token_range == (31744, 256)
    assert PolicyLossConfig(token_range=(np.int64(8), np.int32(8))).token_range == (8, 8)
    for bad in ((-8, 8), (0, 0), (8, -1), (8,), (8, 8, 8), 8, (1.5, 8), "ab"):
        with pytest.raises(ValueError, match="token_range"):
            PolicyLossConfig(token_range=bad)


def test_policy_batch_refuses_tokens_outside_the_range():
    from bridgelang_amd.training.rl import policy_batch
    first, count = ACTIONS
    prompt = torch.randint(3, 31000, (2, 6))
    tok = torch.randint(first, first + count, (2, 7))
    lp, adv = -torch.rand(2, 7), torch.tensor([0.5, -0.5])
    a = policy_batch(prompt, None, tok, lp, adv)
    b = policy_batch(prompt, None, tok, lp, adv, token_range=ACTIONS)
    assert all(torch.equal(a[k], b[k]) for k in a)
    for bad in (first - 1, first + count, 2):
        t = tok.clone()
        t[1, 3] = bad
        policy_batch(prompt, None, t, lp, adv)               # unrestricted: as before
        with pytest.raises(ValueError, match="action_tokens_only=True"):
            policy_batch(prompt, None, t, lp, adv, token_range=ACTIONS)


def test_abi_lists_the_ranged_entry_points():
    from pathlib import Path
    from bridgelang_amd import _lib
    header = (Path(_lib.__file__).resolve().parents[1] / "include" / "bridgelang_hip.h").read_text()
    for name in ("bl_sample_range_f32", "bl_score_range_f32", "bl_policy_loss_range_f32", "bl_policy_loss_backward_range_f32"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header
        base = name.replace("_range", "")
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[base][1]) + 2
