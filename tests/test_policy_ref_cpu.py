"""The bounds and comparators of tests/policy_ref64.py, checked without a GPU, on every case tests/test_policy_ref_gpu.py runs.

* `evaluate_policy` / `evaluate_preference` / `dlogits_from_saved` at float64 ARE the specifications (training/policy_loss.py,
  training/preference_loss.py), to 1e-12.
* The bounds are satisfiable: the same code at float32 (correctly rounded exp / log, numpy's own summation order) stays inside
  every bound, largest err / bound at most 1 — so a GPU failure is never one the CPU already knew.
* The comparators reject near-misses: thirteen planted errors, applied to the reference's own fp64 values, fail by assertion at
  every n used. Zeroing every entry below 1 % of its row's maximum passes the whole-tensor yardstick `max|got − ref| <= 1e-2·max|ref|` of the older tests.
"""
import numpy as np
import pytest
import torch

import glue_ref as G
import policy_ref64 as P64
from policy_ref64 import E, IGN, f32, f64

FWD = P64.forward_cases()
BWD = P64.backward_cases()
PREF = P64.pref_cases()
ids = lambda cs: [c.name for c in cs]
_refs = {}


def ref_of(c):
    """(reference, fwd) of a forward case: computed once, shared, never changed; the 1e-3 threshold condition asserted."""
    if c.name not in _refs:
        if hasattr(c, "pair"):
            _refs[c.name] = P64.preference_reference(c)
            P64.assert_pref_away(c, _refs[c.name][1])
            P64.pref_chain(c, _refs[c.name][1])
        else:
            _refs[c.name] = P64.policy_reference(c)
            P64.assert_policy_away(c, _refs[c.name][1])
    return _refs[c.name]


def rejected(got, ref, what):
    with pytest.raises(AssertionError):
        P64.check(got, ref, what)


def grad_close_accepts(got, ref, tol=1e-2):
    return np.abs(got - ref).max() <= tol * (np.abs(ref).max() + 1e-30)


# ---- float64: the specification -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FWD, ids=ids(FWD))
def test_evaluate_policy_is_the_specification(c):
    ref, fwd = ref_of(c)
    got = P64.policy_outputs(fwd.e)
    for k, (r, _) in ref.items():
        assert np.allclose(got[k], r, rtol=1e-12, atol=1e-300), k
    saved = fwd.e
    dl, _ = P64.dlogits_from_saved(c.logits, c.tgt, saved.r.m, saved.r.logS, saved.r.H, saved.g, saved.nv, c.cfg.temperature,
                                   c.cfg.entropy_coef, c.cfg.token_range)
    # (z − m) − log S against z − (m + log S): fp64 roundings apart, a millionth of the fp32 bound
    assert (np.abs(dl - fwd.dlogits) <= 1e-6 * P64.chained_reference(c, fwd)["dlogits"][1]).all()


@pytest.mark.parametrize("c", PREF, ids=ids(PREF))
def test_evaluate_preference_is_the_specification(c):
    ref, fwd = ref_of(c)
    got = P64.pref_outputs(fwd.e, c.cap)
    for k, (r, _) in ref.items():
        assert np.allclose(got[k], r, rtol=1e-12, atol=1e-300), k


def test_the_cases_hold_what_they_promise():
    seen = dict(clip_hi=0, clip_lo=0, inside=0, trunc=0, mask=0, empty=0, last_only=0)
    for c in FWD:
        e = ref_of(c)[1].e
        v = e.r.valid
        seen["clip_hi"] += int((e.ratio[v] > 1 + c.cfg.clip_high).any())
        seen["clip_lo"] += int((e.ratio[v] < 1 - c.cfg.clip_low).any())
        seen["inside"] += int((~e.clipped[v]).any())
        if c.cfg.rollout_is_cap is not None:
            seen["trunc"] += int(e.truncated.any())
            seen["mask"] += int(e.masked.any())
        if c.group_rows:
            seen["empty"] += int((e.n_g == 0).any())
            vv = v.reshape(-1, c.group_rows)
            seen["last_only"] += int(((vv.sum(axis=1) == 1) & vv[:, -1]).any())
    assert all(seen.values()), seen
    e = ref_of(FWD[0])[1].e
    assert e.r.H[e.r.valid].min() < 1e-20 and np.abs(e.kl[e.r.valid]).min() < 1e-3       # a peaked row; a small d


# ---- float32: the bounds are satisfiable ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FWD, ids=ids(FWD))
def test_fp32_policy_stays_inside_every_bound(c):
    ref, fwd = ref_of(c)
    e32 = P64.evaluate_policy(c, f32)
    P64.check(P64.policy_outputs(e32), ref, c.name)
    dl, _ = P64.dlogits_from_saved(c.logits, c.tgt, e32.r.m, e32.r.logS, e32.r.H, e32.g, e32.nv, c.cfg.temperature, c.cfg.entropy_coef,
                                   c.cfg.token_range, f32)
    P64.check({"dlogits": P64.to_bf16(dl)}, P64.chained_reference(c, fwd), c.name + " chained")


@pytest.mark.parametrize("b", BWD, ids=ids(BWD))
def test_fp32_backward_stays_inside_its_bound(b):
    dl, _ = P64.dlogits_from_saved(b.logits, b.tgt, b.m, b.logS, b.H, b.g, b.nv, b.cfg.temperature, b.cfg.entropy_coef, b.cfg.token_range, f32)
    P64.check({"dlogits": P64.to_bf16(dl)}, P64.backward_reference(b), b.name)


@pytest.mark.parametrize("c", PREF, ids=ids(PREF))
def test_fp32_preference_stays_inside_every_bound(c):
    ref, fwd = ref_of(c)
    e32 = P64.evaluate_preference(c, f32)
    P64.check(P64.pref_outputs(e32, c.cap), ref, c.name)
    cb = c.cfg.backward_config()
    dl, _ = P64.dlogits_from_saved(c.logits, c.tgt, e32.r.m, e32.r.logS, e32.r.H, e32.g, c.P, cb.temperature, 0.0, cb.token_range, f32)
    P64.check({"dlogits": P64.to_bf16(dl)}, P64.chained_reference(c, fwd), c.name + " chained")


def test_largest_ratio_is_recorded():
    P64.check({"x": np.array([1.0 + 2 * E])}, {"x": (np.array([1.0]), np.array([4 * E]))}, "record")
    assert 0.49 < P64.RATIOS["x"] < 0.51


# ---- planted errors on dlogits ------------------------------------------------------------------------------------------------------
ENT = [b for b in BWD if b.cfg.entropy_coef]


def _dl(b, **kw):
    a = dict(m=b.m, logS=b.logS, H=b.H, g=b.g, nv=b.nv, ec=b.cfg.entropy_coef, tgt=b.tgt)
    a.update(kw)
    return P64.dlogits_from_saved(b.logits, a["tgt"], a["m"].astype(f64), a["logS"].astype(f64), a["H"].astype(f64), a["g"].astype(f64), a["nv"],
                                  b.cfg.temperature, a["ec"], b.cfg.token_range)[0]


@pytest.mark.parametrize("b", BWD, ids=ids(BWD))
def test_dlogits_planted_errors_are_rejected(b):
    ref = P64.backward_reference(b)
    good = ref["dlogits"][0]
    P64.check({"dlogits": good}, ref, b.name)
    first, count = b.cfg.token_range or (0, good.shape[1])
    valid = b.tgt != IGN
    if b.cfg.entropy_coef:
        flipped, dropped = _dl(b, ec=-b.cfg.entropy_coef), _dl(b, ec=0.0)
        rejected({"dlogits": flipped}, ref, "entropy term with its sign flipped")
        rejected({"dlogits": dropped}, ref, "entropy term dropped")
    small = np.where(np.abs(good) < 1e-2 * np.abs(good).max(axis=1, keepdims=True), 0.0, good)
    rejected({"dlogits": small}, ref, "every entry below 1 % of the row maximum set to 0")
    assert grad_close_accepts(small, good)
    hole = good.copy()
    r = int(np.flatnonzero(valid)[1])
    c0 = first + (((int(b.tgt[r]) - first) // 8 + 1) % max(count // 8, 1)) * 8
    if count > 8:                                          # an aligned 8-column group away from the target
        hole[r, c0:c0 + 8] = 0.0
        assert not (c0 <= b.tgt[r] < c0 + 8) and np.abs(good[r, c0:c0 + 8]).max() > 0
        rejected({"dlogits": hole}, ref, "one aligned 8-column group set to 0")
    moved = np.where(valid, np.where(b.tgt + 1 < first + count, b.tgt + 1, b.tgt - 1), IGN)
    rejected({"dlogits": _dl(b, tgt=moved)}, ref, "the target's one-hot moved by one column")
    rejected({"dlogits": _dl(b, g=b.g * f32(1 + 2.0 ** -6))}, ref, "g scaled by 1 + 2^-6 (2^-10 is below the bf16 rounding; the fp32 g is held to it)")
    rejected({"dlogits": _dl(b, nv=b.nv + 1)}, ref, "1 / (T·n_valid) taken with n_valid + 1")
    stray = good.copy()
    stray[0, first] = 2.0 ** -100                          # an ignored row is +0 exactly
    rejected({"dlogits": stray}, ref, "a write into an ignored row")
    if first > 0:
        stray = good.copy()
        stray[r, first - 1] = 2.0 ** -100
        rejected({"dlogits": stray}, ref, "a write outside the token range")


def test_g_zero_row_keeps_only_the_entropy_term():
    for b in ENT:
        good = P64.backward_reference(b)["dlogits"][0]
        assert b.g[11] == 0 and np.abs(good[11]).max() > 0
        assert np.array_equal(good[11], _dl(b, g=np.where(np.arange(16) == 11, 0, b.g) * 0)[11])


# ---- planted errors on the forward outputs ----------------------------------------------------------------------------------------
ROWS = P64.row_cases()


def _with(ref, **kw):
    got = {k: r.copy() for k, (r, _) in ref.items()}
    got.update(kw)
    return got


@pytest.mark.parametrize("c", ROWS, ids=ids(ROWS))
def test_row_planted_errors_are_rejected(c):
    ref, fwd = ref_of(c)
    e = fwd.e
    v = e.r.valid
    P64.check(_with(ref), ref, c.name)
    rejected(_with(ref, g=ref["g"][0] * (1 + 2.0 ** -10)), ref, "g scaled by 1 + 2^-10")
    rejected(_with(ref, entropy=ref["entropy"][0] * (1 + 2.0 ** -12)), ref, "H·(1 + 2^-12)")
    if c.cfg.temperature == 1.0:                           # the cases whose every d is small: the mean kl is held to about |d|·e
        assert (np.abs(e.dref[v]) < 0.06).all()
        stats = ref["stats"][0].copy()
        stats[4] = (0.5 * e.dref ** 2 * (1 + 2.0 ** -6))[v].sum() / e.nv
        rejected(_with(ref, stats=stats), ref, "kl = d²/2·(1 + 2^-6) for small d")
    stats = ref["stats"][0].copy()
    stats[0] = stats[0] * e.nv / (e.nv + 1)
    rejected(_with(ref, stats=stats), ref, "the mean over n_valid + 1")
    lp = ref["logp"][0].copy()
    lp[0] = 2.0 ** -100
    rejected(_with(ref, logp=lp), ref, "an ignored row's logp is not 0")


GROUPS = [c for c in P64.group_cases() if c.cfg.ratio_norm == "mean" and c.group_rows > 1]


@pytest.mark.parametrize("c", GROUPS, ids=ids(GROUPS))
def test_group_g_without_its_norm_is_rejected(c):
    ref, fwd = ref_of(c)
    e = fwd.e
    wrong = np.where(e.r.valid, np.repeat(e.gsum, c.group_rows) - c.cfg.kl_coef * e.em1, 0.0)
    assert (np.repeat(e.n_g, c.group_rows)[e.r.valid] > 1).any()
    rejected(_with(ref, g=wrong), ref, "a group's g_r without the factor c")


IS_ACTION = [c for c in P64.is_cases() if c.cfg.ratio_level == "action"]


@pytest.mark.parametrize("c", IS_ACTION, ids=ids(IS_ACTION))
def test_group_weight_per_token_is_rejected(c):
    """w from each token's own λ_r instead of the group's λ_G."""
    ref, fwd = ref_of(c)
    e, cfg = fwd.e, c.cfg
    v, gr = e.r.valid, c.group_rows
    low, high = cfg.rollout_is_mask or (0.0, np.inf)
    rho = np.exp(e.lam_row)
    w = np.where(v, np.where((rho < low) | (rho > high), 0.0, np.minimum(rho, cfg.rollout_is_cap)), 0.0)
    gs = np.where(v, w * e.g0, 0.0).reshape(-1, gr).sum(axis=1)
    g = np.where(v, np.repeat(e.c_g * gs, gr) - cfg.kl_coef * e.em1, 0.0)
    rejected(_with(ref, g=g, is_rows=np.stack([np.where(v, e.lam_row, 0.0), w], axis=1)), ref, "w_G applied per token")


SMOOTHED = [c for c in PREF if c.cfg.kind == "sigmoid" and c.cfg.label_smoothing > 0]


@pytest.mark.parametrize("c", SMOOTHED, ids=ids(SMOOTHED))
def test_pair_dloss_without_label_smoothing_is_rejected(c):
    ref, fwd = ref_of(c)
    ps = ref["pair_stats"][0].copy()
    ps[:c.P, 2] = P64.PF.sigmoid(fwd.e.h) - 1.0
    rejected(_with(ref, pair_stats=ps), ref, "ℓ' with the label-smoothing term dropped")
    ps = ref["pair_stats"][0].copy()
    if c.cap > c.P:
        ps[c.P, 0] = 2.0 ** -100
        rejected(_with(ref, pair_stats=ps), ref, "a pair_stats row beyond P is not 0")


def test_a_write_outside_the_window_is_rejected():
    bf16 = torch.bfloat16
    for where in ("guard below", "guard above", "padding"):
        x = G.Flat((3, 16), "cpu", bf16)
        x.v[:, :8] = 0.5
        P64.window_intact(x, 8, "clean")
        if where == "padding":
            x.v[1, 8] = 0.0
        else:
            x.buf[x.guard - 1 if where == "guard below" else x.guard + 48] = 0.0
        with pytest.raises(AssertionError):
            P64.window_intact(x, 8, where)
    rs = G.Flat((4, 8), "cpu", torch.float32)
    rs.v[:] = 0.0
    rs.buf[-1] = 1.0
    with pytest.raises(AssertionError):
        P64.window_intact(rs, 8, "the last guard element")
