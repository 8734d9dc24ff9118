"""The distillation loss's host specification (training/distill_loss.py) against torch.autograd and central differences in
fp64, its properties and preconditions, the two rl helpers, and the two entry points' declaration / binding / export."""
import math
import pathlib
import re
import subprocess

import numpy as np
import pytest
import torch

from bridgelang_amd.training.distill_loss import (DISTILL_ROW_STAT_NAMES, DISTILL_STAT_NAMES, KINDS, DistillLossConfig, distill_loss)
from bridgelang_amd.training.policy_loss import IGNORE_INDEX, ROW_STAT_NAMES

ROOT = pathlib.Path(__file__).resolve().parents[1]
IGN = IGNORE_INDEX


def softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def make(rows=7, n=24, rng=None, seed=0, zeros=False):
    """Random rows; rows 1 and 4 ignored; a teacher over the range that sums to 1 (with exact zeros when asked)."""
    g = np.random.default_rng(seed)
    first, count = rng or (0, n)
    logits = 2.0 * g.standard_normal((rows, n))
    tgt = first + g.integers(0, count, rows)
    tgt[[1, 4]] = IGN
    q = softmax(1.5 * g.standard_normal((rows, count)))
    if zeros:
        q[:, ::3] = 0.0
        q /= q.sum(axis=1, keepdims=True)
    q[[1, 4]] = np.nan                                   # never looked at
    return logits, tgt.astype(np.int64), q


def torch_loss(logits, tgt, q, cfg):
    """The loss restated with log_softmax, a plain sum and a mean → (loss, dlogits)."""
    n = logits.shape[1]
    first, count = cfg.token_range or (0, n)
    valid = torch.from_numpy(tgt != IGN)
    l = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    lp = torch.log_softmax(l[:, first:first + count] / cfg.temperature, dim=1)[valid]
    p = lp.exp()
    qq = torch.tensor(np.where(np.isnan(q), 0.0, q), dtype=torch.float64)[valid]
    xlogy = torch.special.xlogy
    if cfg.kind == "forward_kl":
        D = (xlogy(qq, qq) - qq * lp).sum(dim=1)
    elif cfg.kind == "reverse_kl":
        D = (p * (lp - qq.log())).sum(dim=1)
    else:
        b = cfg.beta
        mix = b * qq + (1 - b) * p
        D = b * (xlogy(qq, qq) - xlogy(qq, mix)).sum(dim=1) + (1 - b) * (p * (lp - mix.log())).sum(dim=1)
    a = torch.from_numpy(tgt - first)[valid]
    nll = -lp[torch.arange(lp.shape[0]), a]
    loss = (D + cfg.sft_coef * nll).mean()
    loss.backward()
    return float(loss.detach()), l.grad.numpy()


CONFIGS = [DistillLossConfig(kind=k, beta=b, temperature=T, sft_coef=s, token_range=r)
           for k in KINDS for (b, T, s, r) in ((0.5, 1.0, 0.0, None), (0.3, 0.7, 0.3, (8, 8)), (0.8, 1.9, 0.0, (0, 16)), (0.5, 0.7, 0.25, None))]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{c.kind}-b{c.beta}-T{c.temperature}-s{c.sft_coef}-{c.token_range}")
def test_specification_against_autograd(cfg):
    logits, tgt, q = make(rng=cfg.token_range, seed=3, zeros=cfg.kind != "reverse_kl")
    res = distill_loss(logits, tgt, q, cfg)
    loss, grad = torch_loss(logits, tgt, q, cfg)
    assert abs(res.loss - loss) <= 1e-10 * abs(loss)
    assert np.abs(res.dlogits - grad).max() <= 1e-10 * np.abs(grad).max()
    first, count = cfg.token_range or (0, logits.shape[1])
    assert (res.dlogits[:, :first] == 0).all() and (res.dlogits[:, first + count:] == 0).all() and (res.dlogits[tgt == IGN] == 0).all()
    assert res.stats[1] == 5 and res.loss == res.stats[0]


@pytest.mark.parametrize("kind", KINDS)
def test_derivative_against_central_differences_for_an_unnormalised_teacher(kind):
    """∂D/∂z is exact for any q >= 0 (Q = Σ q appears in it): a teacher of mass 1 + 8e-4, inside the precondition."""
    cfg = DistillLossConfig(kind=kind, beta=0.35, temperature=0.8, sft_coef=0.2, token_range=(8, 16))
    logits, tgt, q = make(rows=5, n=32, rng=cfg.token_range, seed=5)
    q = q * (1.0 + 8e-4)
    res = distill_loss(logits, tgt, q, cfg)
    h = 1e-5
    worst = 0.0
    for r in (0, 2, 3):
        for j in range(8, 24):
            up, dn = logits.copy(), logits.copy()
            up[r, j] += h
            dn[r, j] -= h
            fd = (distill_loss(up, tgt, q, cfg).loss - distill_loss(dn, tgt, q, cfg).loss) / (2 * h)
            worst = max(worst, abs(fd - res.dlogits[r, j]))
    assert worst <= 1e-9


@pytest.mark.parametrize("kind", KINDS)
def test_divergence_is_nonnegative_and_zero_with_zero_gradient_at_q_equal_p(kind):
    logits, tgt, q = make(seed=11)
    cfg = DistillLossConfig(kind=kind, temperature=1.3)
    res = distill_loss(logits, tgt, q, cfg)
    v = tgt != IGN
    assert (res.divergence[v] > 0).all()
    same = distill_loss(logits, tgt, softmax(logits / 1.3), cfg)
    assert np.abs(same.divergence).max() <= 1e-15 and np.abs(same.dlogits).max() <= 1e-15
    assert (same.agree[v] == 1).all() and np.abs(same.bin_gap).max() <= 1e-12
    assert np.allclose(same.teacher_entropy[v], same.entropy[v], rtol=1e-12)


def test_jsd_half_is_symmetric_and_at_most_log_two():
    logits, tgt, q = make(seed=13, zeros=True)
    v = tgt != IGN
    cfg = DistillLossConfig(kind="jsd", beta=0.5)
    d_pq = distill_loss(logits, tgt, q, cfg).divergence
    p = softmax(logits)
    with np.errstate(divide="ignore"):
        swapped = np.where(q > 0, np.log(np.where(q > 0, q, 1.0)), -745.0)      # a zero of the teacher: a student bin of e^-745 = 0 in fp64
    d_qp = distill_loss(swapped, tgt, np.where(v[:, None], p, np.nan), cfg).divergence
    assert np.allclose(d_pq[v], d_qp[v], rtol=1e-10)
    assert (d_pq[v] <= math.log(2.0)).all() and (d_pq[v] > 0).all()
    far = np.full((1, 8), -1000.0)
    far[0, 0] = 0.0                                      # the student on bin 0, the teacher on bin 7: disjoint supports
    one = distill_loss(far, np.array([7]), np.eye(8)[[7]], cfg)
    assert abs(one.divergence[0] - math.log(2.0)) <= 1e-12 and one.agree[0] == 0 and abs(one.bin_gap[0] - 7.0) <= 1e-12


def test_forward_kl_to_a_one_hot_teacher_is_cross_entropy():
    logits, tgt, _ = make(seed=17)
    v = tgt != IGN
    onehot = np.zeros_like(logits)
    onehot[np.arange(len(tgt)), np.where(v, tgt, 0)] = 1.0
    res = distill_loss(logits, tgt, onehot, DistillLossConfig(kind="forward_kl"))
    lt = torch.tensor(logits, requires_grad=True)
    ce = torch.nn.functional.cross_entropy(lt, torch.from_numpy(tgt), ignore_index=IGN, reduction="none")
    ce.sum().div(int(v.sum())).backward()
    assert np.allclose(res.row_loss, ce.detach().numpy(), rtol=1e-12, atol=1e-14)
    assert np.allclose(res.dlogits, lt.grad.numpy(), rtol=1e-12, atol=1e-16)
    assert np.allclose(res.divergence, -res.logp) and (res.teacher_entropy == 0).all()


def test_teacher_zeros_are_fine_for_forward_kl_and_jsd_and_refused_for_reverse_kl():
    logits, tgt, q = make(seed=19, zeros=True)
    for kind in ("forward_kl", "jsd"):
        res = distill_loss(logits, tgt, q, DistillLossConfig(kind=kind))
        assert np.isfinite(res.dlogits).all() and np.isfinite(res.stats).all()
    with pytest.raises(ValueError, match="reverse_kl"):
        distill_loss(logits, tgt, q, DistillLossConfig(kind="reverse_kl"))


def test_an_underflowed_student_bin_gives_zero_times_finite():
    logits = np.zeros((1, 8))
    logits[0, 3] = 2000.0                                # every other p_i is exp(-2000) = 0 in fp64
    q = np.full((1, 8), 0.125)
    for kind in KINDS:
        res = distill_loss(logits, np.array([3]), q, DistillLossConfig(kind=kind))
        assert np.isfinite(res.dlogits).all() and np.isfinite(res.stats).all()


def test_result_record_and_all_rows_ignored():
    assert DISTILL_STAT_NAMES == ("loss", "n_valid", "divergence", "entropy", "teacher_entropy", "agreement", "nll", "bin_gap")
    for name in ("logp", "m", "log_s"):                  # token_logprobs() and the backward read these slots
        assert DISTILL_ROW_STAT_NAMES.index(name) == ROW_STAT_NAMES.index(name)
    logits, tgt, q = make(seed=23)
    res = distill_loss(logits, np.full_like(tgt, IGN), q)
    assert (res.stats == 0).all() and (res.dlogits == 0).all() and res.loss == 0
    res = distill_loss(logits, tgt, q, DistillLossConfig(kind="reverse_kl"))
    assert np.array_equal(res.c, res.divergence)
    v = tgt != IGN
    assert np.allclose(distill_loss(logits, tgt, q).c[v], 1.0, atol=1e-12)


def test_config_errors():
    for kw in (dict(kind="kl"), dict(beta=0.0), dict(beta=1.0), dict(beta=float("nan")), dict(temperature=0.0), dict(temperature=float("inf")),
               dict(sft_coef=-0.1), dict(sft_coef=float("nan")), dict(token_range=(8,)), dict(token_range=(-8, 8)), dict(token_range=(0, 0)),
               dict(token_range=(0.5, 8))):
        with pytest.raises(ValueError):
            DistillLossConfig(**kw)
    assert DistillLossConfig(token_range=[8, 16]).token_range == (8, 16)


def test_precondition_errors():
    logits, tgt, q = make(seed=29)
    cfg = DistillLossConfig()
    bad = logits.copy()
    bad[1, 0] = np.inf                                   # even on an ignored row: the logits are the step's
    with pytest.raises(ValueError, match="finite"):
        distill_loss(bad, tgt, q, cfg)
    for what, edit in (("finite", lambda t: t.__setitem__((0, 2), np.nan)), (">= 0", lambda t: t.__setitem__((0, 2), -1e-9)),
                       ("sums to", lambda t: t.__setitem__((2, slice(None)), t[2] * 1.002))):
        t = q.copy()
        edit(t)
        with pytest.raises(ValueError, match=what):
            distill_loss(logits, tgt, t, cfg)
    t = q.copy()
    t[1] = -5.0                                          # an ignored row may hold anything
    distill_loss(logits, tgt, t, cfg)
    with pytest.raises(ValueError, match="shape"):
        distill_loss(logits, tgt, q[:, :-1], cfg)
    low = np.where(tgt == IGN, IGN, tgt % 16)
    with pytest.raises(ValueError, match="shape"):
        distill_loss(logits, low, q, DistillLossConfig(token_range=(0, 16)))
    out = low.copy()
    out[0] = 20
    with pytest.raises(ValueError, match="outside"):
        distill_loss(logits, out, q[:, :16], DistillLossConfig(token_range=(0, 16)))
    with pytest.raises(ValueError, match="leaves"):
        distill_loss(logits, tgt, q, DistillLossConfig(token_range=(16, 16)))


def test_distill_batch_and_gaussian_bin_targets():
    from bridgelang_amd.training import rl
    g = torch.Generator().manual_seed(0)
    B, n, bins, first = 3, 4, 16, 32
    prompt = torch.randint(3, 1000, (B, 6), generator=g)
    mask = torch.ones(B, 6, dtype=torch.bool)
    mask[1, 4:] = False
    tok = first + torch.randint(0, bins, (B, n), generator=g)
    bw = torch.randint(0, 50, (B, n, bins), generator=g)
    bw[..., 5] = 0
    wt = torch.stack([bw.sum(-1) + 7, bw.sum(-1)], dim=-1)
    b = rl.distill_batch(prompt, mask, tok, bw, wt, token_range=(first, bins))
    lab, tp = b["labels"], b["teacher_probs"]
    assert tp.dtype == torch.float32 and tuple(tp.shape) == (B, lab.shape[1], bins) and b["input_ids"].shape == lab.shape
    on = lab != IGN
    assert int(on.sum()) == B * n and torch.equal(lab[on].view(B, n), tok)
    want = (bw.double() / wt[..., 1:].double()).float()
    assert torch.equal(tp[on].view(B, n, bins), want) and (tp[~on] == 0).all()
    assert torch.allclose(tp[on].double().sum(-1), torch.ones(B * n, dtype=torch.float64), atol=1e-6)
    ref = rl.policy_batch(prompt, mask, tok, torch.zeros(B, n), torch.zeros(B), token_range=(first, bins))
    assert all(torch.equal(b[k], ref[k]) for k in ("input_ids", "attention_mask", "labels"))
    sm = rl.distill_batch(prompt, mask, tok, bw, wt, smoothing=0.1, pad_to=20)["teacher_probs"]
    assert sm.shape[1] == 20 and (sm[:, :lab.shape[1]][on] > 0).all()
    assert torch.allclose(sm[:, :lab.shape[1]][on].double(), 0.9 * want.view(-1, bins).double() + 0.1 / bins, atol=1e-7)
    for bad in (dict(bin_wt=bw[:, :2]), dict(wt=wt[..., :1]), dict(smoothing=1.5), dict(token_range=(first, 8)),
                dict(wt=torch.zeros_like(wt)), dict(bin_wt=-bw.double() - 1)):
        with pytest.raises(ValueError):
            rl.distill_batch(**{**dict(prompt_ids=prompt, attention_mask=mask, token_ids=tok, bin_wt=bw, wt=wt), **bad})
    gt = rl.gaussian_bin_targets(tok, 1.5, (first, bins))
    assert gt.dtype == torch.float32 and tuple(gt.shape) == (B, n, bins)
    assert torch.allclose(gt.double().sum(-1), torch.ones(B, n, dtype=torch.float64), atol=1e-6)
    assert torch.equal(gt.argmax(-1), tok - first)
    edge = rl.gaussian_bin_targets(torch.tensor([[first, first + bins - 1]]), 2.0, (first, bins))      # truncated at the ends
    assert edge[0, 0, 0] > 0.3 and edge[0, 1, -1] > 0.3 and torch.allclose(edge[0, 0], edge[0, 1].flip(0))
    onehot = torch.nn.functional.one_hot(tok - first, bins).float()
    assert torch.equal(rl.gaussian_bin_targets(tok, 0.0, (first, bins)), onehot)
    assert torch.allclose(rl.gaussian_bin_targets(tok, 1e-3, (first, bins)), onehot)
    for bad in (lambda: rl.gaussian_bin_targets(tok, -1.0, (first, bins)), lambda: rl.gaussian_bin_targets(tok, 1.0, (0, bins)),
                lambda: rl.gaussian_bin_targets(tok[0], 1.0, (first, bins))):
        with pytest.raises(ValueError):
            bad()
    # the two fit the specification's preconditions as they come
    res = distill_loss(np.zeros((B * n, first + bins)), tok.view(-1).numpy(), gt.view(B * n, bins).numpy(),
                       DistillLossConfig(kind="reverse_kl" if float(gt.min()) > 0 else "jsd", token_range=(first, bins)))
    assert np.isfinite(res.stats).all()


def test_tokens_to_rows_takes_a_trailing_dimension_and_leaves_vectors_alone():
    from bridgelang_amd.training.step import shift_to_rows, tokens_to_rows
    B, l, L, P, C = 2, 5, 6, 3, 4
    g = torch.Generator().manual_seed(1)
    src = torch.rand(B, l, C, generator=g)
    select = torch.zeros(B, L + P, dtype=torch.bool)
    select[0, 4], select[1, 6] = True, True
    dst = torch.full((B * (L + P), C), 7.0)
    tokens_to_rows("teacher", src, dst, l, P, select, "on labelled positions")
    lab = torch.zeros(B, L)
    lab[:, :l] = 1 + torch.arange(l).float()
    where = shift_to_rows(lab, P, 0.0)                   # row → 1 + the token position it predicts
    for b, r in ((0, 4), (1, 6)):
        assert torch.equal(dst.view(B, L + P, C)[b, r], src[b, int(where[b, r]) - 1])
    assert (dst.view(B, L + P, C)[~select] == 0).all()
    vec = torch.full((B * (L + P),), 7.0)
    tokens_to_rows("adv", src[..., 0], vec, l, P, select, "on labelled positions")
    assert torch.equal(vec, dst[:, 0])
    with pytest.raises(ValueError, match="shape"):
        tokens_to_rows("teacher", src[..., :2], dst, l, P, select, "x")
    src[0, int(where[0, 4]) - 1, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        tokens_to_rows("teacher", src, dst, l, P, select, "x")


def test_entry_points_are_declared_bound_and_exported():
    from bridgelang_amd import _lib, train_ops
    header = (ROOT / "include" / "bridgelang_hip.h").read_text()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines()}
    for name, count, tail in (("bl_distill_loss_f32", 17, ["row_stats", "stats", "vocab_first", "vocab_count", "stream"]),
                              ("bl_distill_loss_backward_f32", 19, ["dlogits", "ldd", "vocab_first", "vocab_count", "stream"])):
        proto = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert proto is not None and name in _lib.SIGNATURES and name in exported and hasattr(_lib.load(), name)
        params = [p.strip() for p in proto.group(1).split(",")]
        assert len(params) == len(_lib.SIGNATURES[name][1]) == count
        assert [p.split()[-1].lstrip("*") for p in params[-5:]] == tail
        assert [p.split()[-1].lstrip("*") for p in params[6:8]] == ["teacher", "ldt"]
    assert callable(train_ops.distill_loss) and callable(train_ops.distill_loss_backward)
    assert "distill.hip" in (ROOT / "bridgelang_amd" / "csrc" / "Makefile").read_text()


# ---- tests/distill_ref64.py: the kernels' reference and bounds, checked without a GPU --------------------------------------------
import distill_ref64 as D64      # noqa: E402
import policy_ref64 as P64       # noqa: E402

CASES = D64.cases()
_REF = {}


def ref_of(c):
    if c.name not in _REF:
        _REF[c.name] = D64.reference(c)
    return _REF[c.name]


def test_the_cases_cover_what_they_claim():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    seen = {(c.cfg.kind, c.teacher.shape[1]) for c in CASES}
    assert all((k, n) in seen for k in KINDS for n in (8, 256, 264, 1032))
    assert {len(c.tgt) for c in CASES} >= {1, 5, 37}
    assert {c.cfg.temperature for c in CASES} == {1.0, float(np.float32(0.7))} and {c.cfg.sft_coef > 0 for c in CASES} == {False, True}
    assert any(c.cfg.token_range is None for c in CASES) and any(c.cfg.token_range and c.cfg.token_range[0] == 0 for c in CASES)
    assert any(c.pad for c in CASES) and any(c.tpad for c in CASES) and any(c.dpad for c in CASES)
    peaked = [c for c in CASES if c.name.endswith("-peaked")]
    for c in peaked:                                     # the tail of the student does underflow in fp32
        e = D64.evaluate(c, np.float32)
        assert (e.p == 0).sum() >= 7 * 3 - 3


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_fp64_evaluation_is_the_specification_and_fp32_stays_inside_the_bounds(c):
    ref, extra = ref_of(c)
    got64 = D64.outputs(extra.e)
    for name, (r, _) in ref.items():
        assert np.allclose(got64[name], r, rtol=1e-11, atol=1e-13), name
    before = dict(P64.RATIOS)
    P64.check(D64.outputs(D64.evaluate(c, np.float32)), ref, c.name, rel={}, tag="distill fp32 ")
    P64.RATIOS.clear()
    P64.RATIOS.update(before)
    for name, (r, b) in ref.items():                     # a bound is a bound: finite, and no looser than a part in a thousand
        scale = max(1.0, float(np.abs(r).max())) if r.size else 1.0
        assert np.isfinite(b).all() and float(b.max()) <= 1e-3 * scale, (name, float(b.max()))


def test_the_comparator_rejects_planted_near_misses():
    c = next(c for c in CASES if c.name.startswith("jsd-count256"))
    ref, extra = ref_of(c)
    good = D64.outputs(extra.e)
    v = np.flatnonzero(c.tgt != IGN)[0]
    first = c.cfg.token_range[0]
    for name, at in (("divergence", v), ("row_loss", v), ("c", v), ("logp", v), ("agree", v), ("stats", 2), ("stats", 7), ("dlogits", (v, first))):
        bad = {k: x.copy() for k, x in good.items()}
        bad[name][at] += 4.0 * ref[name][1][at] + (1.0 if ref[name][1][at] == 0 else 0.0)
        with pytest.raises(AssertionError, match=name):
            P64.check(bad, ref, "planted", rel={})
    bad = {k: x.copy() for k, x in good.items()}
    bad["dlogits"][v, 0] = 1e-30                         # outside the range: the bound is 0
    with pytest.raises(AssertionError, match="dlogits"):
        P64.check(bad, ref, "planted", rel={})
