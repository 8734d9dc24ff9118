"""fp64 references, magnitude companions and per-element bounds for the policy and preference loss kernels
(bridgelang_amd/csrc/policy.hip).

A helper module, not a test module: tests import it as `import policy_ref64 as P64`. The VALUES come from the two host
specifications (training/policy_loss.py, training/preference_loss.py; fp64 numpy), called with the fp32 values of the
hyper-parameters the kernels receive (`cfg32`), so no parameter's rounding enters a bound. What the specifications do not
return (m, log S, and the backward from SAVED row statistics) is `evaluate_policy` / `evaluate_preference` /
`dlogits_from_saved` below: the specifications' formulas with the dtype as a parameter. At float64 they must equal the
specifications (tests/test_policy_ref_cpu.py); at float32 they are the "any fp32 evaluation" that has to stay inside every
bound. Every reference is a dict name → (ref, bound), compared by `check`:

    fp32 outputs:  |got − ref| <= bound  (+ FLOOR where bound > 0)         per element, every element
    bf16 dlogits:  |got − ref| <= u·|ref| + bound (+ FLOOR)                u = 2^-8
    bound == 0:    got == ref exactly (ignored rows, the 0/1 outputs, counts, zero columns, spare slots)

A bound is c·e·mag + the error inherited from earlier outputs, e = 2^-24, mag the expression with every term replaced by
its absolute value. First-order worst-case bounds; SECOND = 1 + 2^-10 multiplies every bound for the second-order terms
(every relative first-order error is asserted below 2^-11 in `_rows`). fp32 add / mul / fma / division are 1·e relative
each (no fast-math flag, csrc/Makefile:5); ocml expf, logf, expm1f, log1pf are 1 ulp = 2·e (C_FN).

Row pass (policy_rows_kernel policy.hip:163-205, policy_rows_wave_kernel :209-241, finish_row :125-159)
* z_i = l_i·inv_t, inv_t = 1.0f / T (:658): the division 1, the product 1 (or the fma's single rounding): C_Z = 2.
  m = max(l)·inv_t (:186): the maximum is exact: b_m = C_Z·e·|m|.
* d_i = z_i − m (:192): α_i·e with α_i = C_Z·(|z_i| + |m|) + |d_i|.
* S = Σ expf(d_i) (:193-203): a term is off by ex_i·(α_i + C_FN)·e. The chain: a thread adds ceil(n/1024) groups of 4 in
  sequence, wave_sum 6 butterfly levels (bl_common.h:54-58), red_s[0] + … + red_s[3] 3 adds: K(n) = 4·ceil(n/1024) + 9
  against S itself (every term is positive): mag_S = Σ ex_i·(α_i + C_FN) + K·S.
* log S (:128): an absolute e·mag_S / S from S, logf C_FN·e·|log S|: b_logS.
* W = Σ ex_i·d_i (:195): a term is off by ex_i·(|d_i|·(α_i + C_FN + 1) + α_i)·e (ex's error, the product, d's error), the
  same chain against |W| = Σ ex_i·|d_i| (every d_i <= 0): mag_W.
* H = log S − W/S (:129), both terms >= 0: b_H = b_logS + e·(mag_W/S + (|W|/S)·(mag_S/S) + |W|/S [division] + |H| [sum]).
  On a peaked row S = 1 + tiny and the fp32 sum cannot resolve the tiny part: b_H stays near K·e however small H is.
* logp = z_a − m − log S (:130-131). It cancels on a peaked row, so its companion is |z_a| + |m| + |log S|:
  b_logp = b_m + b_logS + e·(C_Z·|z_a| + |z_a − m| + |logp|).
Surrogate (surrogate_terms :51-62), KL (kl_terms :64-71), row loss (:116-118)
* lr = logp − q: b_lr = b_logp + e·|lr|. Self-proximal (proximal :114): q is the kernel's own logp, lr = 0 and
  ratio = expf(0) = 1 exactly: bound 0.
* ratio = expf(lr): `_exp_b`: ratio·(expm1(b_lr) + C_FN·e·exp(b_lr)).
* pg = −min(ratio·A, clip·A): |A|·(b_ratio + e·hi [1 ± clip is rounded]) + e·|pg|. g0 = −A·ratio: |A|·b_ratio + e·|g0|;
  0 exactly off the active side. `active` is exact: the builders keep ratio 1e-3 (relative) off both limits.
* d = ref − logp: b_d = b_logp + e·|d|. em1 = expm1f(d): `_em1_b` = exp(d + b_d)·b_d + C_FN·e·|em1|.
  kl = em1 − d is about d²/2: the SAME rounded d enters both terms, so d's error moves kl by kl'(d) = em1 only:
  `_k3_b` = (|em1| + exp(d + b_d)·b_d)·b_d + C_FN·e·|em1| + e·|kl| — absolute in |d|·e and in logp's error, not relative to kl.
  The step statistics' expm1f(lr) − lr (:365) and expm1f(λ) − λ (:357) are the same form.
* g = g0 − kl_coef·em1 (:69): b_g0 + |kl_coef|·(b_em1 + e·|em1|) + e·|g|.
* row_loss = pg − ec·H + kc·kl (:117): b_pg + |ec|·(b_H + e·|H|) + |kc|·(b_kl + e·|kl|) + 2·e·(|pg| + |ec·H| + |kc·kl|).
Rollout correction (is_terms :92-100, weight_surrogate :109-112)
* λ = q − μ: e·|λ| (+ b_logp self-proximal). ρ = expf(λ): `_exp_b`. w: 0 exactly when masked, the fp32 cap exactly when
  truncated, else b_ρ; masked / truncated are exact (ρ 1e-3 off the cap and the band). w·x: w·b_x + b_w·|x| + e·|w·x|.
Group level (policy_group_kernel :251-321; preference_seq_kernel :482-509)
* Σ over a sequence's valid rows: lane l adds rows l, l + 64, … (ceil(group_rows/64) adds), then wave_sum: depth_g =
  ceil(group_rows/64) + 6 against Σ|term|, plus every term's own bound; the specification sums in row order.
  s_G = c·Σ δ_r, c = 1.0f / (float)n_G (:284): the division and the product: + 2·e·|s_G|. λ_G likewise.
  g_r = c·[w_G·]Σ_j g0_j − KL share (:286-303): Σ b_g0 + depth_g·e·Σ|g0|, then the weight, then c (2·e), then the KL share.
  group_stats = (s_G, expf(s_G), n_G exact, Σ logp).
Step statistics (stats_body :328-392): a thread adds ceil(rows/256) values, wave_sum 6, the four waves 3, the division 1:
  depth_s = ceil(rows/256) + 10: mean(b_x) + depth_s·e·mean|x|. n_valid is exact; every row ignored: all zeros exactly.
Backward (policy_backward_kernel :422-453), from the fp32 row statistics it is GIVEN (in isolation: the reference's,
  rounded; chained: the forward's bounds b_g, b_H, b_m + b_logS are propagated, `fwd=`)
* off = m + log S (:436): e·|off|. lp_i = z_i − off (:447): b_lp = C_Z·e·|z_i| + b_off + e·|lp_i|. p_i = expf(lp_i): `_exp_b`.
* v = (g·(δ − p) + ec·p·(lp + H))·scale, scale = inv_t / stats[1] (:437, :449): the g term (δ − p) 1 and the product 1;
  the entropy term (lp + H) 1 and two products 2; the sum 1; scale: inv_t 1, the division 1, its product 1; the cross term
  with the bf16 rounding 1: C_BWD = 3 + 1 + 3 + 1 = 8 against mag = scale·(|g|·(δ + p) + |ec|·p·(|lp| + |H|)), plus
  scale·(|g|·b_p + |ec|·(b_p·|lp + H| + p·b_lp)). pack2bf rounds once: u·|ref|. Outside the range, on ignored rows: +0 exactly.
Preference (preference_pair_kernel :516-579, preference_apply_kernel :585-616, softplusf :477)
* rc, rr, lp of a pair are sequential sums over its sequences in ascending b: (number of terms)·e·Σ|term| + Σ b_term.
  nll = −lp/N: + e·|nll|. Δ = rc − rr: + e·|Δ|. h = β·Δ − γ: β·b_Δ + e·|β·Δ| + e·|h|.
* sigmoid: t = expf(−|h|): `_exp_b`. softplus(x) = max(x, 0) + log1pf(t): b_h + b_t/(1 + t) + C_FN·e·log1p(t) + e·softplus.
  ℓ = (1 − ε)·sp(−h) + ε·sp(h): (1 − ε)·b_sp + ε·b_sp + 3·e·ℓ (1 − ε, two products / the sum, all terms >= 0).
  ℓ' = σ − (1 − ε), σ = 1/(1 + t) or t/(1 + t) (|dσ/dt| <= 1): b_t + e·(2·σ + (1 − ε) + |ℓ'|).
* ipo: u = h/β − 1/(2β): b_u = b_h/β + e·(|h/β| + 2/(2β) + |u|); ℓ = u²: 2·|u|·b_u + e·u²; ℓ' = 2u/β: 2·b_u/β + 2·e·|ℓ'|.
* hinge: ℓ = max(0, 1 − h): b_h + e·ℓ; ℓ' = −[h < 1] exact (|h − 1| >= 1e-3 by construction). [Δ > 0] exact likewise.
* the statistics: a thread adds ceil(cap/256) pairs, 6, 3, the division: depth_p = ceil(cap/256) + 10.
* g_seq = ℓ'·β·sign·c_b (:599): β·c_b·b_ℓ' + 3·e·|g_seq|; g = g_seq − α/N (:606): + e·α/N + e·|g|.

FLOOR = 2^-116 (as tests/train_ref64.py): a flushed fp32 denormal times operands below 2^10, and bf16 denormal outputs.
No constant here is fitted to a measured error; a GPU run that exceeds a bound is a finding about the kernel.
"""
from __future__ import annotations

import dataclasses
import math
from types import SimpleNamespace as NS
from typing import Dict, Optional

import numpy as np

from bridgelang_amd.training import policy_loss as PL
from bridgelang_amd.training import preference_loss as PF

E = 2.0 ** -24
U = 2.0 ** -8
FLOOR = 2.0 ** -116
SECOND = 1.0 + 2.0 ** -10
C_Z = 2
C_FN = 2
C_BWD = 8
IGN = PL.IGNORE_INDEX
f64, f32 = np.float64, np.float32

RATIOS: Dict[str, float] = {}      # output name → largest err / bound seen


def cfg32(cfg):
    """The configuration with every float replaced by the fp32 value the kernels receive."""
    kw = {}
    for f in dataclasses.fields(cfg):
        v = getattr(cfg, f.name)
        if isinstance(v, float):
            kw[f.name] = float(f32(v))
        elif f.name == "rollout_is_mask" and v is not None:
            kw[f.name] = tuple(float(f32(x)) for x in v)
    return dataclasses.replace(cfg, **kw)


# ---- the specifications' formulas with the dtype as a parameter ----------------------------------------------------------
def _fn(name, x, dt):
    """exp / log / expm1 / log1p of dt values, correctly rounded to dt (fp64 evaluation, one rounding)."""
    with np.errstate(all="ignore"):
        return getattr(np, name)(np.asarray(x, dtype=dt).astype(f64)).astype(dt)


def _gsum(v, valid, gr, dt):
    """[rows] → [groups]: sums over each group's valid rows in row order, in dt."""
    out = np.zeros(v.shape[0] // gr, dtype=dt)
    for k in range(out.size):
        vk = v[k * gr:(k + 1) * gr][valid[k * gr:(k + 1) * gr]].astype(dt)
        if vk.size:
            out[k] = np.add.accumulate(vk, dtype=dt)[-1]
    return out


def softmax_rows(logits, tgt, T, rng, dt):
    """Row pass over the token range: z, m, d, ex, S, W, log S, H, z_a, logp; 0 on ignored rows (never read)."""
    n = logits.shape[1]
    first, count = rng or (0, n)
    valid = tgt != IGN
    l = np.where(valid[:, None], logits[:, first:first + count], 0).astype(dt)
    z = l / dt(T)
    m = z.max(axis=1)
    d = z - m[:, None]
    ex = _fn("exp", d, dt)
    S = ex.sum(axis=1, dtype=dt)
    W = (ex * d).sum(axis=1, dtype=dt)
    logS = _fn("log", S, dt)
    H = logS - W / S
    a = np.where(valid, tgt - first, 0)
    za = z[np.arange(len(tgt)), a]
    logp = za - m - logS
    zero = lambda v: np.where(valid, v, dt(0))
    return NS(valid=valid, first=first, count=count, z=z, m=zero(m), d=d, ex=ex, S=S, W=W, logS=zero(logS), H=zero(H), za=za,
              logp=zero(logp), a=a, n=n)


def evaluate_policy(c, dt=f64):
    """training/policy_loss.py's definition (token or action level, with or without the rollout correction) in dtype dt."""
    cfg = c.cfg
    r = softmax_rows(c.logits, c.tgt, cfg.temperature, cfg.token_range, dt)
    v, rows = r.valid, len(c.tgt)
    arr = lambda x: np.where(v, np.asarray(x), 0).astype(dt)
    A = arr(c.A)
    q = r.logp if c.q is None else arr(c.q)
    lr = r.logp - q
    corrected, by_action = cfg.rollout_is_cap is not None, cfg.ratio_level == "action"
    lam = q - arr(c.mu) if corrected else None
    gr = c.group_rows if by_action else 1
    n_g = v.reshape(-1, gr).sum(axis=1)
    c_g = (dt(1) / np.maximum(n_g, 1).astype(dt)) if (by_action and cfg.ratio_norm == "mean") else np.ones(n_g.size, dtype=dt)
    rep = lambda x: np.where(v, np.repeat(x, gr), dt(0))
    out = NS(r=r, A=A, q=q, n_g=n_g, c_g=c_g, gr=gr, lr_row=lr, lam_row=lam)
    if by_action:
        out.s_g = c_g * _gsum(lr, v, gr, dt)
        lr = rep(out.s_g)
        out.lp_g = _gsum(r.logp, v, gr, dt)
        if corrected:
            out.lam_g = c_g * _gsum(lam, v, gr, dt)
            lam = rep(out.lam_g)
    ratio = _fn("exp", lr, dt)
    lo, hi = dt(1) - dt(cfg.clip_low), dt(1) + dt(cfg.clip_high)
    pg = -np.minimum(ratio * A, np.clip(ratio, lo, hi) * A)
    active = ((A >= 0) & (ratio <= hi)) | ((A < 0) & (ratio >= lo))
    g0 = np.where(active, -A * ratio, dt(0))
    w = np.ones(rows, dtype=dt)
    if corrected:
        low, high = cfg.rollout_is_mask or (0.0, np.inf)
        rho = _fn("exp", lam, dt)
        masked = v & ((rho < dt(low)) | (rho > dt(high)))
        truncated = v & ~masked & (rho > dt(cfg.rollout_is_cap))
        w = np.where(masked, dt(0), np.minimum(rho, dt(cfg.rollout_is_cap)))
        out.rho, out.masked, out.truncated = rho, masked, truncated
    out.pg0, out.g0 = pg, g0
    if by_action:                        # the kernel's order: Σ_j g0_j, then w_G, then c
        out.gsum = _gsum(g0, v, gr, dt)
        w_g = w.reshape(-1, gr)[np.arange(n_g.size), np.argmax(v.reshape(-1, gr), axis=1)]      # a group's rows share w_G
        g0s = rep(c_g * (w_g * out.gsum))
        pg = w * pg
    else:
        pg, g0s = w * pg, w * g0
    kl, em1, dref = np.zeros(rows, dtype=dt), np.zeros(rows, dtype=dt), np.zeros(rows, dtype=dt)
    g = g0s
    if c.ref is not None:
        dref = arr(c.ref) - r.logp
        em1 = _fn("expm1", dref, dt)
        kl = em1 - dref
        g = g0s - dt(cfg.kl_coef) * em1
    row_loss = pg - dt(cfg.entropy_coef) * r.H + dt(cfg.kl_coef) * kl
    nv = int(v.sum())
    mean = lambda x: dt(np.where(v, x, 0).astype(dt).sum(dtype=dt) / dt(nv)) if nv else dt(0)
    akl = _fn("expm1", lr, dt) - lr
    out.__dict__.update(lr=lr, lam=lam, ratio=np.where(v, ratio, dt(0)), active=active, w=np.where(v, w, dt(0)), pg=pg, g0s=g0s, dref=dref, em1=em1,
                        kl=kl, g=np.where(v, g, dt(0)), row_loss=np.where(v, row_loss, dt(0)), clipped=v & ~active, nv=nv, akl=akl,
                        stats=np.array([mean(row_loss), nv, mean(pg), mean(r.H), mean(kl), mean((~active).astype(dt)), mean(akl),
                                        mean(ratio)], dtype=dt))
    if by_action:
        out.group_stats = np.stack([out.s_g, np.where(n_g > 0, _fn("exp", out.s_g, dt), dt(0)), n_g.astype(dt), out.lp_g], axis=1)
    if corrected:
        rk = _fn("expm1", lam, dt) - lam
        out.rk = rk
        out.is_rows = np.stack([np.where(v, lam, dt(0)), out.w], axis=1)
        out.is_stats = np.array([mean(w), mean(out.rho), mean(out.truncated.astype(dt)), mean(out.masked.astype(dt)), mean(rk),
                                 mean(-lam), 0, 0], dtype=dt)
    return out


def dlogits_from_saved(logits, tgt, m, logS, H, g, nv, T, ec, rng, dt=f64):
    """dlogits of the definition from SAVED row values (what policy_backward_kernel is given) → (dl, parts for the bound)."""
    rows, n = logits.shape
    first, count = rng or (0, n)
    valid = tgt != IGN
    l = np.where(valid[:, None], logits[:, first:first + count], 0).astype(dt)
    z = l / dt(T)
    off = (np.asarray(m, dtype=dt) + np.asarray(logS, dtype=dt))[:, None]
    lp = z - off
    p = _fn("exp", lp, dt)
    oh = np.zeros_like(z)
    oh[np.arange(rows), np.where(valid, tgt - first, 0)] = 1
    g, H = np.asarray(g, dtype=dt)[:, None], np.asarray(H, dtype=dt)[:, None]
    scale = dt(1) / (dt(T) * dt(max(nv, 1)))
    core = np.where(valid[:, None], (g * (oh - p) + dt(ec) * p * (lp + H)) * scale, dt(0))
    dl = np.zeros((rows, n), dtype=dt)
    dl[:, first:first + count] = core
    return dl, NS(z=z, off=off, lp=lp, p=p, oh=oh, g=g, H=H, scale=scale, valid=valid, first=first, count=count, n=n)


def evaluate_preference(c, dt=f64):
    """training/preference_loss.py's definition in dtype dt. P = c.P pairs (ids beyond ±P are no pair)."""
    cfg, gr = c.cfg, c.group_rows
    r = softmax_rows(c.logits, c.tgt, cfg.temperature, cfg.token_range, dt)
    v, rows = r.valid, len(c.tgt)
    B, P = rows // gr, c.P
    pair = np.where(np.abs(c.pair.astype(np.int64)) <= P, c.pair.astype(np.int64), 0)
    ref = np.zeros(rows, dtype=dt) if c.ref is None else np.where(v, c.ref, 0).astype(dt)
    n_b = v.reshape(B, gr).sum(axis=1)
    dlt = r.logp - ref
    d_sum, lp_sum = _gsum(dlt, v, gr, dt), _gsum(r.logp, v, gr, dt)
    c_b = (dt(1) / np.maximum(n_b, 1).astype(dt)) if cfg.seq_norm == "mean" else np.ones(B, dtype=dt)
    delta = c_b * d_sum
    beta, gamma, alpha, eps = dt(cfg.beta), dt(cfg.margin), dt(cfg.sft_coef), dt(cfg.label_smoothing)
    rc, rr, N, lps = (np.zeros(P, dtype=dt) for _ in range(4))
    for b in range(B):
        k = abs(int(pair[b])) - 1
        if pair[b] > 0:
            rc[k] += delta[b]
            N[k] += dt(n_b[b])
            lps[k] += lp_sum[b]
        elif pair[b] < 0:
            rr[k] += delta[b]
    nll = np.where(N > 0, -lps / np.maximum(N, 1), dt(0))
    Delta = rc - rr
    h = beta * Delta - gamma
    if cfg.kind == "sigmoid":
        t = _fn("exp", -np.abs(h), dt)
        sp = lambda x: np.maximum(x, dt(0)) + _fn("log1p", t, dt)
        lk = (dt(1) - eps) * sp(-h) + eps * sp(h)
        dk = np.where(h >= 0, dt(1) / (dt(1) + t), t / (dt(1) + t)) - (dt(1) - eps)
    elif cfg.kind == "ipo":
        u = h / beta - dt(1) / (dt(2) * beta)
        lk, dk = u * u, dt(2) * u / beta
    else:
        lk, dk = np.maximum(dt(0), dt(1) - h), -(h < 1).astype(dt)
    kb = np.abs(pair) - 1
    g_seq = np.where(pair != 0, dk[kb] * beta * np.sign(pair).astype(dt) * c_b, dt(0))
    Nk = np.where(pair > 0, N[kb], dt(1))
    g_b = g_seq - np.where((pair > 0) & (N[kb] > 0) & (alpha != 0), alpha / np.maximum(Nk, 1), dt(0))
    g = np.where(v, np.repeat(g_b, gr), dt(0))
    mean = lambda x: dt(np.asarray(x, dtype=dt).sum(dtype=dt) / dt(P))
    stats = np.array([mean(lk + alpha * nll), P, mean(lk), mean((Delta > 0).astype(dt)), mean(beta * Delta), mean(beta * rc),
                      mean(beta * rr), mean(nll)], dtype=dt)
    return NS(r=r, pair=pair, n_b=n_b, dlt=dlt, d_sum=d_sum, lp_sum=lp_sum, c_b=c_b, delta=delta, rc=rc, rr=rr, N=N, lps=lps, nll=nll,
              Delta=Delta, h=h, lk=lk, dk=dk, g_seq=g_seq, g_b=g_b, g=g, stats=stats, P=P,
              pair_stats=np.stack([h, lk, dk, nll], axis=1), seq_stats=np.stack([delta, n_b.astype(dt), lp_sum, g_seq], axis=1))


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def _exp_b(x, bx):
    """|expf(x') − exp(x)| for |x' − x| <= bx; expf(0) = 1 exactly when x is exact."""
    b = np.exp(x) * (np.expm1(bx) + C_FN * E * np.exp(bx))
    return np.where((bx == 0) & (x == 0), 0.0, b)


def _em1_b(d, bd):
    return np.exp(d + bd) * bd + C_FN * E * np.abs(np.expm1(d))


def _k3_b(d, bd):
    em1 = np.abs(np.expm1(d))
    return np.where((bd == 0) & (d == 0), 0.0, (em1 + np.exp(d + bd) * bd) * bd + C_FN * E * em1 + E * np.abs(np.expm1(d) - d))


def _rows(r):
    """Bounds of the row pass from its fp64 evaluation r: b_m, b_logS, b_H, b_logp (0 on ignored rows)."""
    K = 4 * math.ceil(r.count / 1024) + 9
    am = np.abs(r.z.max(axis=1))
    alpha = C_Z * (np.abs(r.z) + am[:, None]) + np.abs(r.d)
    assert alpha.max() * E < 2.0 ** -11, "a first-order relative error above 2^-11: SECOND does not cover the second order"
    mag_S = (r.ex * (alpha + C_FN)).sum(axis=1) + K * r.S
    aW = np.abs(r.W)
    mag_W = (r.ex * (np.abs(r.d) * (alpha + C_FN + 1) + alpha)).sum(axis=1) + K * aW
    b_m = C_Z * E * am
    b_logS = E * (mag_S / r.S + C_FN * np.abs(r.logS))
    b_H = b_logS + E * (mag_W / r.S + (aW / r.S) * (mag_S / r.S) + aW / r.S + np.abs(r.H))
    b_logp = b_m + b_logS + E * (C_Z * np.abs(r.za) + np.abs(r.za - r.z.max(axis=1)) + np.abs(r.logp))
    z = lambda b: np.where(r.valid, b, 0.0)
    return NS(m=z(b_m), logS=z(b_logS), H=z(b_H), logp=z(b_logp))


def _gb(term_abs, term_b, valid, gr):
    """Bound of a lane-strided sum over each group's valid rows: Σ b_term + depth_g·e·Σ|term|."""
    depth = math.ceil(gr / 64) + 6
    s = lambda x: np.where(valid, x, 0.0).reshape(-1, gr).sum(axis=1)
    return s(term_b) + depth * E * s(term_abs)


def _mean_b(x, bx, valid, depth):
    nv = int(valid.sum())
    if nv == 0:
        return 0.0
    return (np.where(valid, bx, 0.0).sum() + depth * E * np.where(valid, np.abs(x), 0.0).sum()) / nv


def _pack(d):
    return {k: (np.asarray(r, dtype=f64), np.asarray(b, dtype=f64) * SECOND) for k, (r, b) in d.items()}


def policy_reference(c):
    """c: a case with cfg = cfg32(...). → (dict name → (ref, bound), fwd) for row_stats' eight columns, `stats`, and where the
    entry point has them `group_stats`, `is_rows`, `is_stats`; fwd carries what a chained backward inherits."""
    cfg = c.cfg
    spec = PL.policy_loss(c.logits.astype(f64), c.tgt, c.A, c.q, c.ref, cfg, group_rows=c.group_rows, behaviour_logprobs=c.mu)
    e = evaluate_policy(c, f64)
    r, v = e.r, e.r.valid
    rows, gr = len(c.tgt), e.gr
    b = _rows(r)
    corrected, by_action, selfprox = cfg.rollout_is_cap is not None, cfg.ratio_level == "action", c.q is None
    rep = lambda x: np.where(v, np.repeat(x, gr), 0.0)
    ab = np.abs
    # the log-ratio, per row or per group
    b_lr_row = np.zeros(rows) if selfprox else b.logp + E * ab(e.lr_row)
    if by_action:
        b_s = e.c_g * _gb(ab(e.lr_row), b_lr_row, v, gr) + (0.0 if selfprox else 2 * E * ab(e.s_g))
        b_lr = rep(b_s)
    else:
        b_lr = b_lr_row
    b_ratio = _exp_b(e.lr, b_lr)
    hi = 1.0 + cfg.clip_high
    A = ab(e.A)
    b_pg = A * (b_ratio + E * hi) + E * ab(e.pg0)
    b_g0 = np.where(e.active, A * b_ratio + E * ab(e.g0), 0.0)
    out = {}
    b_w = np.zeros(rows)
    if corrected:
        b_lam_row = E * ab(e.lam_row) + (b.logp if selfprox else 0.0)
        if by_action:
            b_lam = rep(e.c_g * _gb(ab(e.lam_row), b_lam_row, v, gr) + 2 * E * ab(e.lam_g))
        else:
            b_lam = b_lam_row
        b_rho = _exp_b(e.lam, b_lam)
        b_w = np.where(e.masked | e.truncated, 0.0, b_rho)
        out["is_rows"] = (np.stack([spec.log_rho, spec.weight], axis=1), np.stack([np.where(v, b_lam, 0), np.where(v, b_w, 0)], axis=1))
    wgt = lambda x, bx: e.w * bx + b_w * ab(x) + E * ab(e.w * x) if corrected else bx
    b_pgw = wgt(e.pg0, b_pg)
    if by_action:
        b_gsum = _gb(ab(e.g0), b_g0, v, gr)
        gsum = rep(e.gsum)
        b_g0s = rep(e.c_g) * wgt(gsum, rep(b_gsum)) + 2 * E * ab(e.g0s)
    else:
        b_g0s = wgt(e.g0, b_g0)
    kc, ec = cfg.kl_coef if c.ref is not None else 0.0, cfg.entropy_coef
    b_d = b.logp + E * ab(e.dref)
    b_kl = _k3_b(e.dref, b_d) if c.ref is not None else np.zeros(rows)
    b_g = b_g0s + (abs(kc) * (_em1_b(e.dref, b_d) + E * ab(e.em1)) if c.ref is not None else 0.0) + E * ab(e.g)
    b_loss = b_pgw + abs(ec) * (b.H + E * ab(r.H)) + abs(kc) * (b_kl + E * ab(e.kl)) + 2 * E * (ab(e.pg) + ab(ec * r.H) + ab(kc * e.kl))
    z = lambda x: np.where(v, x, 0.0)
    out.update(logp=(spec.logp, b.logp), entropy=(spec.entropy, b.H), ratio=(spec.ratio, z(b_ratio)), row_loss=(spec.row_loss, z(b_loss)),
               clipped=(spec.clipped.astype(f64), np.zeros(rows)), m=(e.r.m, b.m), log_s=(e.r.logS, b.logS), g=(spec.g, z(b_g)))
    depth = math.ceil(rows / 256) + 10
    mb = lambda x, bx: _mean_b(x, bx, v, depth)
    zero = np.zeros(rows)
    out["stats"] = (spec.stats, np.array([mb(e.row_loss, b_loss), 0.0, mb(e.pg, b_pgw), mb(r.H, b.H), mb(e.kl, b_kl), mb(e.clipped, zero),
                                          mb(e.akl, _k3_b(e.lr, b_lr)), mb(e.ratio, b_ratio)]))
    if by_action:
        some = e.n_g > 0
        out["group_stats"] = (spec.group_stats, np.stack([np.where(some, b_s, 0), np.where(some, _exp_b(e.s_g, b_s), 0), np.zeros(e.n_g.size),
                                                          _gb(ab(r.logp), b.logp, v, gr)], axis=1))
    if corrected:
        out["is_stats"] = (spec.is_stats, np.array([mb(e.w, b_w), mb(e.rho, b_rho), mb(e.truncated, zero), mb(e.masked, zero),
                                                    mb(e.rk, _k3_b(e.lam, b_lam)), mb(e.lam, b_lam), 0.0, 0.0]))
    fwd = NS(spec=spec, e=e, g=e.g, dlogits=spec.dlogits, b_g=z(b_g), b_H=b.H, b_off=b.m + b.logS, nv=e.nv)
    return _pack(out), fwd


def dlogits_reference(logits, tgt, m, logS, H, g, nv, cfg, fwd_b=None, ref=None):
    """(ref, bound) of the backward from the row values it is given. fwd_b = (b_g, b_H, b_off) per row: the forward's bounds
    (a chained case; `ref` is then the specification's dlogits, otherwise dlogits_from_saved's)."""
    dl, s = dlogits_from_saved(logits, tgt, m, logS, H, g, nv, cfg.temperature, cfg.entropy_coef, cfg.token_range)
    bg, bH, boff = (np.zeros((len(tgt), 1)),) * 3 if fwd_b is None else (np.asarray(x)[:, None] for x in fwd_b)
    ab, ec = np.abs, abs(cfg.entropy_coef)
    b_off = boff + E * ab(s.off)
    b_lp = C_Z * E * ab(s.z) + b_off + E * ab(s.lp)
    b_p = _exp_b(s.lp, b_lp)
    mag = s.scale * (ab(s.g) * (s.oh + s.p) + ec * s.p * (ab(s.lp) + ab(s.H)))
    core = s.scale * (ab(s.g) * b_p + bg * (s.oh + s.p) + ec * (b_p * ab(s.lp + s.H) + s.p * (b_lp + bH))) + C_BWD * E * mag
    bound = np.zeros_like(dl)
    bound[:, s.first:s.first + s.count] = np.where(s.valid[:, None], core, 0.0)
    return {"dlogits": ((dl if ref is None else np.asarray(ref, dtype=f64)), bound * SECOND)}


def preference_reference(c):
    """→ (dict name → (ref, bound), fwd) for logp, entropy, m, log_s, g, the three zero columns, stats, pair_stats (cap rows,
    zeros beyond P) and seq_stats."""
    cfg, gr, P, cap = c.cfg, c.group_rows, c.P, c.cap
    e = evaluate_preference(c, f64)
    r, v, ab = e.r, e.r.valid, np.abs
    rows, B = len(c.tgt), len(c.tgt) // gr
    if c.spec_ok:           # the host preconditions hold (dense ids, both sides labelled): the values are the specification's
        spec = PF.preference_loss(c.logits.astype(f64), c.tgt, c.pair, c.ref, cfg, group_rows=gr)
        val = NS(logp=spec.logp, H=spec.entropy, g=spec.g, stats=spec.stats, pair_stats=spec.pair_stats, seq_stats=spec.seq_stats)
    else:                   # an id beyond ±P: evaluate_preference is the definition with that id read as 0 (policy.hip:472-476)
        val = NS(logp=r.logp, H=r.H, g=e.g, stats=e.stats, pair_stats=e.pair_stats, seq_stats=e.seq_stats)
    b = _rows(r)
    b_dl = b.logp + (E * ab(e.dlt) if c.ref is not None else 0.0)
    b_dsum = _gb(ab(e.dlt), b_dl, v, gr)
    b_delta = e.c_b * b_dsum + 2 * E * ab(e.delta)
    b_lps = _gb(ab(r.logp), b.logp, v, gr)
    b_rc, b_rr, b_lp, cnt_c, cnt_r, a_rc, a_rr, a_lp = (np.zeros(P) for _ in range(8))
    for s in range(B):
        k = abs(int(e.pair[s])) - 1
        if e.pair[s] > 0:
            b_rc[k] += b_delta[s]; a_rc[k] += ab(e.delta[s]); cnt_c[k] += 1
            b_lp[k] += b_lps[s]; a_lp[k] += ab(e.lp_sum[s])
        elif e.pair[s] < 0:
            b_rr[k] += b_delta[s]; a_rr[k] += ab(e.delta[s]); cnt_r[k] += 1
    b_rc, b_rr, b_lp = b_rc + cnt_c * E * a_rc, b_rr + cnt_r * E * a_rr, b_lp + cnt_c * E * a_lp
    Nn = np.maximum(e.N, 1)
    b_nll = b_lp / Nn + E * ab(e.nll)
    b_Delta = b_rc + b_rr + E * ab(e.Delta)
    beta, gamma, alpha, eps = cfg.beta, cfg.margin, cfg.sft_coef, cfg.label_smoothing
    b_h = beta * b_Delta + E * ab(beta * e.Delta) + E * ab(e.h)
    if cfg.kind == "sigmoid":
        t = np.exp(-ab(e.h))
        b_t = _exp_b(-ab(e.h), b_h)
        l1p = np.log1p(t)
        b_sp = lambda x: b_h + b_t / (1 + t) + C_FN * E * l1p + E * (np.maximum(x, 0) + l1p)
        b_l = (1 - eps) * b_sp(-e.h) + eps * b_sp(e.h) + 3 * E * ab(e.lk)
        sig = PF.sigmoid(e.h)
        b_dk = b_t + E * (2 * sig + (1 - eps) + ab(e.dk))
    elif cfg.kind == "ipo":
        u = e.h / beta - 1 / (2 * beta)
        b_u = b_h / beta + E * (ab(e.h / beta) + 2 / (2 * beta) + ab(u))
        b_l, b_dk = 2 * ab(u) * b_u + E * u * u, 2 * b_u / beta + 2 * E * ab(e.dk)
    else:
        b_l, b_dk = b_h + E * ab(e.lk), np.zeros(P)
    kb = np.maximum(ab(e.pair) - 1, 0)
    paired = e.pair != 0
    b_gseq = np.where(paired, beta * e.c_b * b_dk[kb] + 3 * E * ab(e.g_seq), 0.0)
    b_gb = b_gseq + np.where(e.pair > 0, E * alpha / Nn[kb] + E * ab(e.g_b), 0.0) if alpha != 0 else b_gseq
    z = lambda x: np.where(v, x, 0.0)
    zr = np.zeros(rows)
    depth = math.ceil(cap / 256) + 10
    mp = lambda x, bx: (np.sum(bx) + depth * E * np.sum(ab(x))) / P
    tot = e.lk + alpha * e.nll
    b_tot = b_l + alpha * b_nll + 2 * E * (ab(e.lk) + ab(alpha * e.nll))
    bb = lambda x, bx: beta * bx + E * ab(beta * x)
    pad = lambda x: np.concatenate([x, np.zeros((cap - P, 4))], axis=0)
    out = dict(logp=(val.logp, b.logp), entropy=(val.H, b.H), m=(r.m, b.m), log_s=(r.logS, b.logS), ratio=(zr, zr), row_loss=(zr, zr),
               clipped=(zr, zr), g=(val.g, z(np.repeat(b_gb, gr))),
               stats=(val.stats, np.array([mp(tot, b_tot), 0.0, mp(e.lk, b_l), mp((e.Delta > 0) * 1.0, 0.0), mp(beta * e.Delta, bb(e.Delta, b_Delta)),
                                           mp(beta * e.rc, bb(e.rc, b_rc)), mp(beta * e.rr, bb(e.rr, b_rr)), mp(e.nll, b_nll)])),
               pair_stats=(pad(val.pair_stats), pad(np.stack([b_h, b_l, b_dk, b_nll], axis=1))),
               seq_stats=(val.seq_stats, np.stack([b_delta, np.zeros(B), b_lps, b_gseq], axis=1)))
    fwd = NS(e=e, b_g=z(np.repeat(b_gb, gr)), b_H=b.H, b_off=b.m + b.logS, nv=P, h=e.h, Delta=e.Delta, rc=e.rc, rr=e.rr)
    return _pack(out), fwd


# ---- the comparator --------------------------------------------------------------------------------------------------------
def check(got: Dict[str, np.ndarray], ref: Dict[str, tuple], what: str, rel: Optional[Dict[str, float]] = None, tag: str = "") -> None:
    """Every output named in `ref` is in `got`, finite, and within its bound on every element (u·|ref| added for the names in
    `rel`, i.e. the bf16 dlogits). AssertionError names the worst element. RATIOS[tag + name] keeps the largest err / bound."""
    rel = {"dlogits": U} if rel is None else rel
    for name, (r, b) in ref.items():
        g = np.asarray(got[name], dtype=f64)
        assert g.shape == r.shape, f"{what} {name}: shape {g.shape} vs {r.shape}"
        bound = b + rel.get(name, 0.0) * np.abs(r)
        bound = bound + np.where(bound > 0, FLOOR, 0.0)
        err = np.where(np.isfinite(g), np.abs(g - r), np.inf)
        ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1.0))
        ratio = np.where((bound == 0) & (err > 0), np.inf, ratio)
        worst = float(ratio.max()) if ratio.size else 0.0
        if worst > 1.0:
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
            raise AssertionError(f"{what} {name}: {int((ratio > 1).sum())} of {ratio.size} elements out of bound; worst at {tuple(int(j) for j in i)}: "
                                 f"got {g[i]!r}, ref {r[i]!r}, bound {bound[i]:.4g}, err/bound {worst:.4g}")
        RATIOS[tag + name] = max(RATIOS.get(tag + name, 0.0), worst)


def split_row_stats(rs) -> Dict[str, np.ndarray]:
    rs = np.asarray(rs)
    return {name: rs[:, i] for i, name in enumerate(PL.ROW_STAT_NAMES)}


def away(x, limit, what: str) -> None:
    """A deciding quantity keeps a relative 1e-3 off its threshold (a condition on the inputs, asserted on the reference)."""
    x = np.asarray(x, dtype=f64)
    if np.isfinite(limit):
        assert (np.abs(x - limit) >= 1e-3 * max(abs(limit), 1e-30)).all() if limit != 0 else (np.abs(x) >= 1e-3).all(), f"{what}: within 1e-3 of {limit}"


# ---- the cases, shared by the CPU and the GPU test ----------------------------------------------------------------------------
WANT = (0.5, 0.9, 1.0, 1.1, 1.6, 0.7, 1.35)          # ratios: clipped low, inside, exactly 1, inside, clipped high, …
RHO = (0.3, 0.8, 1.0, 2.5, 4.0, 1.5)                 # π_prox / μ: below the band (0.5, 3), inside, above the cap 2, above the band
POLICY = dict(clip_low=0.2, clip_high=0.25, entropy_coef=0.01, kl_coef=0.1)


def _randn(g, shape, scale=2.0):
    """bf16-representable fp32 values (what the step's logits rows hold)."""
    x = (g.standard_normal(shape) * scale).astype(f32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)


def edge_rows(n, seed, trip=1024):
    """16 rows of width n for a kernel whose workgroup strides `trip` columns: where the row maximum and the target sit.
    → (logits fp32 [16, n], targets). Columns are clamped into the row, so a narrow row repeats some placements."""
    g = np.random.default_rng(seed)
    cl = lambda i: min(i, n - 1)
    L = _randn(g, (16, n))
    tgt = g.integers(0, n, 16)
    for r, (mc, tc) in {1: (1, n - 2), 2: (n - 3, 2), 3: (cl(trip // 4 + 4), cl(trip // 2 + 88)), 4: (cl(trip + 2), cl(trip + 6)),
                        5: (n - 1, n - 1)}.items():      # first / last float4, another wave, the second trip, both at the end
        L[r, mc], tgt[r] = 12.0, tc
    L[6] = 1.25                                          # all equal
    L[7], tgt[7] = 0.0, cl(5)
    L[7, tgt[7]] = 60.0                                  # peaked on its target
    L[8], tgt[8] = 0.0, cl(5)
    L[8, (tgt[8] + 1) % n] = 60.0                        # peaked off it
    L[9, 0::2], L[9, 1::2], tgt[9] = 80.0, -80.0, 1      # ±80: exp underflows at T = 0.5, 0·d must be 0
    tgt[0] = tgt[10] = IGN
    return L, tgt.astype(np.int64)


def embed(L, tgt, n, first, seed):
    """The rows as columns [first, first + L.shape[1]) of n-wide random rows, targets shifted."""
    g = np.random.default_rng(seed)
    out = _randn(g, (L.shape[0], n))
    out[:, first:first + L.shape[1]] = L
    return out, np.where(tgt == IGN, IGN, tgt + first)


def policy_case(name, logits, tgt, cfg, seed, group_rows=None, pad=0, selfprox=False, small_d=False):
    cfg = cfg32(cfg)
    rows = len(tgt)
    g = np.random.default_rng(seed)
    valid = tgt != IGN
    vi = np.flatnonzero(valid)
    logp = softmax_rows(logits, tgt, cfg.temperature, cfg.token_range, f64).logp
    A = g.standard_normal(rows).astype(f32)
    if vi.size > 3:
        A[vi[0]], A[vi[1]], A[vi[3]] = abs(A[vi[0]]), -abs(A[vi[1]]), 0.0     # both signs and 0, inside one group where one exists
    by_action, corrected = cfg.ratio_level == "action", cfg.rollout_is_cap is not None
    gr = group_rows if by_action else 1
    groups = rows // gr
    n_g = valid.reshape(groups, gr).sum(axis=1)
    div = np.repeat(np.maximum(n_g, 1), gr) if (by_action and cfg.ratio_norm == "sum") else 1.0
    per_row = lambda vals: np.repeat(np.resize(np.array(vals), groups), gr)
    q = None if selfprox else np.where(valid, logp - np.log(per_row(WANT)) / div, 0).astype(f32)
    d = g.choice([-1.0, 1.0], rows) * g.uniform(0.01, 0.05, rows) if small_d else 0.3 * g.standard_normal(rows)
    ref = np.where(valid, logp + d, 0).astype(f32)       # small_d: kl is about d²/2 <= 1.3e-3 on every row, so the mean shows it
    if vi.size > 2:
        ref[vi[2]] = f32(logp[vi[2]] + 0.02)             # kl = 2e-4
    mu = None
    if corrected:
        qq = logp if selfprox else q.astype(f64)
        jit = np.where(valid, 0.3 * g.standard_normal(rows), 0.0).reshape(groups, gr)     # λ_r differ inside a group; their sum does not move
        jit = np.where(valid.reshape(groups, gr), jit - jit.sum(axis=1, keepdims=True) / np.maximum(n_g, 1)[:, None], 0.0).reshape(-1)
        mu = np.where(valid, qq - np.log(per_row(RHO)) / div - jit, 0).astype(f32)
    A = np.where(valid, A, 0).astype(f32)
    return NS(name=name, logits=logits, tgt=tgt, A=A, q=q, ref=ref if cfg.kl_coef else None, mu=mu, cfg=cfg, group_rows=group_rows if by_action else None,
              pad=pad)


def assert_policy_away(c, fwd) -> None:
    """Every deciding quantity of the case keeps 1e-3 off its threshold; asserted on the reference alone."""
    e, cfg = fwd.e, c.cfg
    v = e.r.valid
    away(e.ratio[v], 1.0 - cfg.clip_low, f"{c.name} ratio")
    away(e.ratio[v], 1.0 + cfg.clip_high, f"{c.name} ratio")
    if cfg.rollout_is_cap is not None:
        low, high = cfg.rollout_is_mask or (0.0, np.inf)
        for lim in (cfg.rollout_is_cap, low, high):
            if lim > 0:
                away(e.rho[v], lim, f"{c.name} rho")


def row_cases():
    """bl_policy_loss_f32 (policy_rows_kernel, stride 1024): n, T, ld − n."""
    out = []
    for i, (n, T) in enumerate([(n, T) for n in (8, 1024, 1032, 2056) for T in (0.5, 1.0, 2.0)]):
        L, tgt = edge_rows(n, 100 + n)
        out.append(policy_case(f"rows-n{n}-T{T}-pad{8 * (i % 2)}", L, tgt, PL.PolicyLossConfig(temperature=T, **POLICY), 7 * n + i, pad=8 * (i % 2),
                               small_d=T == 1.0))
    L, tgt = edge_rows(32064, 5)
    keep = [0, 3, 4, 6, 7, 8, 9, 11]                     # 8 rows: the 32-trip chain
    out.append(policy_case("rows-n32064-T1.0-pad0", L[keep], tgt[keep], PL.PolicyLossConfig(temperature=1.0, **POLICY), 32064, small_d=True))
    return out


N_RANGE = 288


def range_cases():
    """bl_policy_loss_range_f32: count 8, 248, 256 (the wave kernel) and 264 (the workgroup kernel through the same entry)."""
    out = []
    for count in (8, 248, 256, 264):
        for first, rows in zip((0, 8, N_RANGE - count), (1, 4, 5)):
            L, tgt = edge_rows(count, count + first)
            pick = [1, 0, 2, 5, 9][:rows] if rows > 1 else [1]
            Lw, tw = embed(L[pick], tgt[pick], N_RANGE, first, count + rows)
            cfg = PL.PolicyLossConfig(temperature=0.5, token_range=(first, count), **POLICY)
            out.append(policy_case(f"range-first{first}-count{count}-rows{rows}", Lw, tw, cfg, 3 * count + rows, pad=8 * (rows % 2)))
    return out


def _group_targets(gr, groups, n, seed):
    """Targets for `groups` sequences of gr rows: about a third ignored; group 1 empty; group 2 only its last row valid;
    row 0 of group 3 (of group 0 when there are fewer) ignored."""
    g = np.random.default_rng(seed)
    tgt = g.integers(0, n, (groups, gr))
    if gr > 1:
        tgt[g.random((groups, gr)) < 0.3] = IGN
        tgt[:, -1] = np.where(tgt[:, -1] == IGN, 1, tgt[:, -1])
        tgt[min(3, groups - 1), 0] = IGN
        if gr >= 4:
            tgt[0, :4] = [0, n - 1, 1, 2]                # group 0 holds A > 0, A < 0, a valid row, A = 0
    if groups > 1:
        tgt[1] = IGN
    if groups > 2:
        tgt[2, :-1] = IGN
    return tgt.reshape(-1).astype(np.int64)


GROUP_SHAPES = ((1, 4), (7, 5), (64, 1), (65, 4), (65, 5))


def group_cases():
    """bl_policy_loss_grouped_f32 (policy_group_kernel, lane stride 64, four sequences per workgroup), n = 8."""
    out = []
    for gr, groups in GROUP_SHAPES:
        for norm in ("sum", "mean"):
            g = np.random.default_rng(gr * 10 + groups)
            cfg = PL.PolicyLossConfig(temperature=1.0, ratio_level="action", ratio_norm=norm, **POLICY)
            out.append(policy_case(f"group-{gr}x{groups}-{norm}", _randn(g, (gr * groups, 8)), _group_targets(gr, groups, 8, gr + groups), cfg,
                                   gr + 3 * groups, group_rows=gr))
    return out


def is_cases():
    """bl_policy_loss_is_f32 at both levels: proximal given / self, cap finite / inf, no mask / the band (0.5, 3)."""
    out = []
    for level in ("token", "action"):
        for selfprox in (False, True):
            for cap in (2.0, float("inf")):
                for mask in (None, (0.5, 3.0)):
                    gr, groups = (7, 6) if level == "action" else (1, 14)
                    g = np.random.default_rng(len(out))
                    tgt = _group_targets(gr, groups, 8, 40 + len(out)) if level == "action" else np.where(np.arange(14) % 5 == 2, IGN, g.integers(0, 8, 14))
                    cfg = PL.PolicyLossConfig(temperature=1.0, ratio_level=level, ratio_norm="mean" if (level == "action" and selfprox) else "sum",
                                              rollout_is_cap=cap, rollout_is_mask=mask, **POLICY)
                    out.append(policy_case(f"is-{level}-{'self' if selfprox else 'given'}-cap{cap}-{'band' if mask else 'nomask'}",
                                           _randn(g, (gr * groups, 8)), tgt.astype(np.int64), cfg, 60 + len(out), group_rows=gr, selfprox=selfprox))
    return out


def stats_cases():
    """stats_body (stride 256 rows): rows 1, 256, 257 at n = 8; and every row ignored."""
    out = []
    for rows in (1, 256, 257):
        g = np.random.default_rng(rows)
        tgt = np.where((np.arange(rows) % 5 == 3) & (rows > 1), IGN, g.integers(0, 8, rows)).astype(np.int64)
        out.append(policy_case(f"stats-rows{rows}", _randn(g, (rows, 8)), tgt, PL.PolicyLossConfig(temperature=1.0, **POLICY), rows))
    out.append(policy_case("stats-all-ignored", _randn(np.random.default_rng(9), (5, 8)), np.full(5, IGN, dtype=np.int64),
                           PL.PolicyLossConfig(temperature=1.0, **POLICY), 9))
    return out


def forward_cases():
    return row_cases() + range_cases() + group_cases() + is_cases() + stats_cases()


def backward_cases():
    """policy_backward_kernel in isolation (stride 2048 columns): the saved row values are the fp64 reference's, rounded to
    fp32; g = 0 on one row (only the entropy term is left); stats[1] is set directly."""
    out = []
    spec = [(8, None, 0.0, 1, 0), (8, None, 0.01, 16, 8), (2048, None, 0.01, 16, 0), (2056, None, 0.0, 16, 8), (2056, None, 0.01, 1, 0),
            (2056, (8, 2048), 0.01, 16, 8), (2056, (0, 2048), 0.01, 16, 0), (2056, (8, 8), 0.0, 1, 0), (16, (8, 8), 0.01, 16, 8)]
    for n, rng, ec, nv, pad in spec:
        first, count = rng or (0, n)
        L, tgt = edge_rows(count, 7 + n + count, trip=2048)
        L, tgt = embed(L, tgt, n, first, n) if rng else (L, tgt)
        cfg = cfg32(PL.PolicyLossConfig(temperature=0.5 if ec else 2.0, entropy_coef=ec, token_range=rng))
        c = policy_case("bwd", L, tgt, dataclasses.replace(cfg, kl_coef=0.1), n + count)
        e = evaluate_policy(c, f64)
        g = e.g.astype(f32)
        g[11] = 0.0
        out.append(NS(name=f"bwd-n{n}-range{rng}-ec{ec}-nv{nv}-pad{pad}", logits=L, tgt=tgt, m=e.r.m.astype(f32), logS=e.r.logS.astype(f32),
                      H=e.r.H.astype(f32), g=g, nv=nv, cfg=cfg, pad=pad))
    return out


def backward_reference(b):
    return dlogits_reference(b.logits, b.tgt, b.m.astype(f64), b.logS.astype(f64), b.H.astype(f64), b.g.astype(f64), b.nv, b.cfg)


def chained_reference(c, fwd):
    """The backward after the forward kernel, against the specification's dlogits: both bounds."""
    e = fwd.e
    return dlogits_reference(c.logits, c.tgt, e.r.m, e.r.logS, e.r.H, fwd.g, fwd.nv,
                             c.cfg if isinstance(c.cfg, PL.PolicyLossConfig) else c.cfg.backward_config(), fwd_b=(fwd.b_g, fwd.b_H, fwd.b_off),
                             ref=fwd.dlogits)


def pref_case(name, B, gr, n, pair, cfg, seed, cap=None, P=None, pad=0):
    g = np.random.default_rng(seed)
    cfg = cfg32(cfg)
    rows = B * gr
    first, count = cfg.token_range or (0, n)
    L = _randn(g, (rows, n))
    tgt = first + g.integers(0, count, rows)
    keep = g.random(rows) < 0.7
    keep.reshape(B, gr)[:, -1] = True                    # every sequence keeps a row; row 0 of some is ignored
    tgt = np.where(keep, tgt, IGN).astype(np.int64)
    ref = None if cfg.reference_free else (-math.log(count) + 0.5 * g.standard_normal(rows)).astype(f32)
    pair = np.asarray(pair, dtype=np.int32)
    top = int(np.abs(pair.astype(np.int64)).max())
    P = P or top
    return NS(name=name, logits=L, tgt=tgt, pair=pair, ref=ref, cfg=cfg, group_rows=gr, P=P, cap=cap or P, P_dev=P if (cap or P) != P else None,
              spec_ok=top <= P, pad=pad)


def assert_pref_away(c, fwd) -> None:
    away(fwd.Delta, 0.0, f"{c.name} Delta")
    if c.cfg.kind == "hinge":
        away(fwd.h, 1.0, f"{c.name} h")


def pref_cases():
    """bl_preference_loss_f32. (a) 6 sequences of 5 rows, n = 64, range (8, 32), a pair with two chosen sequences and a sequence
    in no pair: every kind x seq_norm x reference; then the pair capacities 1, 256, 257, the device pair count below the capacity,
    an id beyond ±P, and the workgroup row kernel (264 columns)."""
    out = []
    a = [1, -1, 2, 2, -2, 0]
    for kind in PF.KINDS:
        for norm in PF.SEQ_NORMS:
            for ref_free in (False, True):
                cfg = PF.PreferenceLossConfig(beta=0.3, kind=kind, seq_norm=norm, reference_free=ref_free, temperature=0.8, token_range=(8, 32),
                                              label_smoothing=0.1 if (kind == "sigmoid" and not ref_free) else 0.0,
                                              margin=0.0 if kind == "ipo" else 0.25, sft_coef=0.5 if norm == "mean" else 0.0)
                out.append(pref_case(f"pref-{kind}-{norm}-{'free' if ref_free else 'ref'}", 6, 5, 64, a, cfg, len(out), pad=8 * ref_free))
    sig = lambda **kw: PF.PreferenceLossConfig(**{**dict(beta=0.3, kind="sigmoid", seq_norm="sum", label_smoothing=0.1, margin=0.25, sft_coef=0.5,
                                                         temperature=0.8), **kw})
    many = lambda P: [b + 1 for b in range(P)] + [-(b + 1) for b in range(P)] + [0]
    out.append(pref_case("pref-cap1", 2, 1, 8, [1, -1], sig(), 31))
    out.append(pref_case("pref-cap256", 513, 1, 8, many(256), sig(), 32))
    out.append(pref_case("pref-cap257", 515, 1, 8, many(257), sig(seq_norm="mean"), 33))
    out.append(pref_case("pref-cap257-P2", 6, 5, 64, a, sig(token_range=(8, 32)), 34, cap=257, P=2))
    out.append(pref_case("pref-id-beyond-P", 6, 5, 64, [1, -1, 2, 2, -2, 3], sig(token_range=(8, 32)), 35, cap=3, P=2))
    out.append(pref_case("pref-workgroup-264", 4, 3, 264, [1, -1, -2, 2], sig(kind="hinge", label_smoothing=0.0), 36))
    return out


def pref_chain(c, fwd):
    """What chained_reference needs of a preference case: g, the specification's dlogits (the definition's, for an id beyond P)."""
    e = fwd.e
    fwd.g = e.g
    cfgb = c.cfg.backward_config()
    fwd.dlogits = dlogits_from_saved(c.logits, c.tgt, e.r.m, e.r.logS, e.r.H, e.g, c.P, cfgb.temperature, 0.0, cfgb.token_range)[0]
    if c.spec_ok:
        spec = PF.preference_loss(c.logits.astype(f64), c.tgt, c.pair, c.ref, c.cfg, group_rows=c.group_rows)
        assert np.allclose(spec.dlogits, fwd.dlogits, rtol=1e-12, atol=1e-300)
        fwd.dlogits = spec.dlogits
    return fwd


# ---- an evaluation as the kernels' outputs; bf16; the sentinel windows ---------------------------------------------------------
def policy_outputs(e) -> Dict[str, np.ndarray]:
    r = e.r
    out = dict(logp=r.logp, entropy=r.H, ratio=e.ratio, row_loss=e.row_loss, clipped=e.clipped.astype(f64), m=r.m, log_s=r.logS, g=e.g,
               stats=e.stats)
    for k in ("group_stats", "is_rows", "is_stats"):
        if hasattr(e, k):
            out[k] = getattr(e, k)
    return {k: np.array(v, dtype=f64) for k, v in out.items()}


def pref_outputs(e, cap: int) -> Dict[str, np.ndarray]:
    r = e.r
    z = np.zeros(r.logp.shape)
    ps = np.concatenate([e.pair_stats.astype(f64), np.zeros((cap - e.P, 4))], axis=0)
    out = dict(logp=r.logp, entropy=r.H, m=r.m, log_s=r.logS, ratio=z, row_loss=z, clipped=z, g=e.g, stats=e.stats, pair_stats=ps,
               seq_stats=e.seq_stats)
    return {k: np.array(v, dtype=f64) for k, v in out.items()}


def to_bf16(x) -> np.ndarray:
    """fp32 → the nearest bf16 value (ties to even), as fp32."""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)).view(f32)


def window_intact(flat, n: int, what: str) -> None:
    """A glue_ref.Flat whose logical output is the columns [0, n) of its [rows, ld] block (or the whole of a vector): the
    guards on both sides and the ld − n padding columns of every row still hold the sentinel."""
    import glue_ref as G
    G.outside_untouched(flat, what)
    if len(flat.shape) == 2 and flat.shape[1] > n:
        pad = flat.v[:, n:].detach().cpu()
        want = G.Flat((flat.shape[0], flat.shape[1] - n), "cpu", flat.buf.dtype, guard=0).v
        G.assert_bits(pad, want, f"{what}: wrote into the row padding")
