"""fp64 reference, magnitude companions and per-element bounds for the distillation loss kernels
(bridgelang_amd/csrc/distill.hip). A helper module, not a test module: tests import it as `import distill_ref64 as D64`.

The VALUES come from the host specification (training/distill_loss.py, fp64 numpy), called with the fp32 values of the
hyper-parameters the kernels receive (`policy_ref64.cfg32`). `evaluate` is the kernel's own formulas with the dtype as a
parameter: at float64 it must equal the specification, at float32 it is an "any fp32 evaluation" that has to stay inside
every bound (tests/test_distill_loss_cpu.py does not need a GPU for either). Bounds, comparator and conventions are
tests/policy_ref64.py's: first-order worst case, c·e·mag + inherited error, e = 2^-24, SECOND for the second order, ocml
expf / logf 1 ulp = 2·e (C_FN), u = 2^-8 for the bf16 dlogits, FLOOR for flushed denormals, no constant fitted to a
measured error.

Row pass (distill_rows_kernel / distill_rows_wave_kernel, the header comment of distill.hip gives the summation order)
* m, S, W, log S, H, logp are policy.hip's chains to the letter: `policy_ref64._rows` (b_m, b_logS, b_H, b_logp), with its
  per-column α_i (d_i = z_i − m is off by α_i·e).
* Every sum is per thread ceil(n/1024) float4s in sequence, wave_sum 6 levels, 3 adds for the four slots:
  K(n) = 4·ceil(n/1024) + 9 against Σ|term|, plus every term's own bound (`_sum_b`).
* q is an fp32 input: exact. Q = Σ q: K·e·Q. lq = logf(q): C_FN·e·|log q|. E = Σ q·lq: a term q·b_lq + e·|q·lq| (the
  product). IQ = Σ i·q: (float)i is exact (i < 2^24), the product 1: (K + 1)·e·Σ i·q.
* lp_i = d_i − log S: b_lp = α_i·e + b_logS + e·|lp_i|. p_i = expf(lp_i): `_exp_b` + TINY, TINY = 2^-126: an expf result
  below the smallest normal is rounded to a denormal or flushed, an absolute error that no relative bound covers.
  IP = Σ i·p: a term i·b_p + e·i·p. bin gap = |IP − IQ|: b_IP + b_IQ + e·|IP − IQ|.
* forward_kl: t = q·(lq − lp): q·(b_lq + b_lp + e·|lq − lp|) + e·|t|. D = Σ t. c = Q.
* reverse_kl: u = lp − lq: b_u = b_lp + b_lq + e·|u|; t = p·u: b_p·|u| + p·b_u + e·|t|. D = c = Σ t.
* jsd: omb = 1.0f − β on the host: e relative. mi = β·q + omb·p: e·β·q + 2·e·omb·p + omb·b_p + e·mi. lm = logf(mi):
  b_mi / mi + C_FN·e·|log mi|. tq = q·(lq − lm) and tp = p·(omb·(lp − lm)) as above, omb·(…) with 2·e more. D = β·A + C:
  β·b_A + e·|β·A| + b_C + e·(|β·A| + |C|). c = C.
Statistics kernel (distill_stats_kernel): row_loss = D + sft·(−logp): b_D + sft·b_logp + e·|sft·nll| + e·(|D| + |sft·nll|);
  the means are policy_ref64's depth_s = ceil(rows/256) + 10 (`_mean_b`). agree, n_valid: exact.
Backward (distill_backward_kernel), chained after the forward: off = m + log S: b_m + b_logS + e·|off|. lp = z − off:
  C_Z·e·|z| + b_off + e·|lp|. p: `_exp_b` + TINY. forward_kl: dz = p·c − q: b_p·|c| + p·b_c + 2·e·|p·c| + e·q. The others:
  u as in the row pass, w = u − c: b_u + b_c + e·(|u| + |c|), dz = p·w: b_p·|w| + p·b_w + e·|dz|. s = sft·(p − δ):
  sft·(b_p + e·|p − δ|) + e·|s|. v = (dz + s)·scale, scale = inv_t / n_valid: the sum 1, inv_t 1, the division 1, the
  product 1, the cross term with the bf16 rounding 1: 5·e against scale·(|dz| + |s|). pack2bf rounds once: u·|ref|.

Deciding quantities are kept off their boundaries by construction (`case`): both arg-maxes at least 1e-3 above the
runner-up, and no q_i in (0, 2^-100). q > 0 and p > 0 are then exact decisions or decide terms below FLOOR."""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

import policy_ref64 as P64
from bridgelang_amd.training import distill_loss as DL
from policy_ref64 import C_FN, C_Z, E, IGN, SECOND, f32, f64

TINY = 2.0 ** -126
C_SCALE = 5


def _log(x, dt=f64):
    """log of x where x > 0, else 0 (a term with weight 0 is 0), correctly rounded to dt."""
    x = np.asarray(x, dtype=dt)
    with np.errstate(all="ignore"):
        return np.where(x > 0, np.log(np.where(x > 0, x, 1).astype(f64)), 0.0).astype(dt)


def evaluate(c, dt=f64):
    """The kernels' formulas in dtype dt: the row pass, the statistics, and the backward from the row pass's own results."""
    cfg = c.cfg
    r = P64.softmax_rows(c.logits, c.tgt, cfg.temperature, cfg.token_range, dt)
    v = r.valid
    rows, count = len(c.tgt), r.count
    q = np.where(v[:, None], c.teacher, 0).astype(dt)
    lq = _log(q, dt)
    idx = np.arange(count).astype(dt)
    lp = r.d - r.logS[:, None]
    p = P64._fn("exp", lp, dt)
    Q = q.sum(axis=1, dtype=dt)
    te = (q * lq).sum(axis=1, dtype=dt)
    IQ, IP = (idx * q).sum(axis=1, dtype=dt), (idx * p).sum(axis=1, dtype=dt)
    beta, omb, sft = dt(cfg.beta), dt(f32(1) - f32(cfg.beta)) if dt == f32 else dt(1) - dt(cfg.beta), dt(cfg.sft_coef)
    out = NS(r=r, q=q, lq=lq, lp=lp, p=p, Q=Q, te=te, IQ=IQ, IP=IP, omb=omb)
    if cfg.kind == "forward_kl":
        out.t = np.where(q > 0, q * (lq - lp), dt(0))
        D = out.t.sum(axis=1, dtype=dt)
        cc = Q
    elif cfg.kind == "reverse_kl":
        out.u = lp - lq
        out.t = p * out.u
        D = out.t.sum(axis=1, dtype=dt)
        cc = D
    else:
        out.mi = beta * q + omb * p
        out.lm = _log(out.mi, dt)
        out.tq = np.where(q > 0, q * (lq - out.lm), dt(0))
        out.u = omb * (lp - out.lm)
        out.tp = np.where(p > 0, p * out.u, dt(0))
        out.A, out.C = out.tq.sum(axis=1, dtype=dt), out.tp.sum(axis=1, dtype=dt)
        D = beta * out.A + out.C
        cc = out.C
    zero = lambda x: np.where(v, x, dt(0))
    nll = -r.logp
    out.D, out.c, out.nll = zero(D), zero(cc), nll
    out.row_loss = zero(out.D + sft * nll)
    out.agree = zero((np.argmax(np.where(v[:, None], c.logits[:, r.first:r.first + count], 0), axis=1) == np.argmax(q, axis=1)).astype(dt))
    out.te_row, out.gap = zero(-te), zero(np.abs(IP - IQ))
    nv = int(v.sum())
    mean = lambda x: dt(np.where(v, x, 0).astype(dt).sum(dtype=dt) / dt(nv)) if nv else dt(0)
    out.nv = nv
    out.stats = np.array([mean(out.row_loss), nv, mean(out.D), mean(r.H), mean(out.te_row), mean(out.agree), mean(nll), mean(out.gap)], dtype=dt)
    # the backward, from this evaluation's own m, log S and c
    z = r.z
    off = (r.m + r.logS)[:, None]
    blp = z - off
    bp = P64._fn("exp", blp, dt)
    cb = out.c[:, None]
    if cfg.kind == "forward_kl":
        dz = bp * cb - q
    elif cfg.kind == "reverse_kl":
        dz = bp * ((blp - lq) - cb)
    else:
        bmi = beta * q + omb * bp
        dz = np.where(bp > 0, bp * (omb * (blp - _log(bmi, dt)) - cb), dt(0))
    oh = np.zeros((rows, count), dtype=dt)
    oh[np.arange(rows), r.a] = 1
    scale = dt(1) / dt(cfg.temperature) / dt(max(nv, 1))
    core = np.where(v[:, None], (dz + sft * (bp - oh)) * scale, dt(0))
    out.dlogits = np.zeros((rows, r.n), dtype=dt)
    out.dlogits[:, r.first:r.first + count] = core
    out.bwd = NS(z=z, off=off, lp=blp, p=bp, oh=oh, scale=scale)
    return out


def outputs(e):
    """An evaluation as the kernels' outputs, name → fp64 array."""
    r = e.r
    out = dict(logp=r.logp, entropy=r.H, divergence=e.D, row_loss=e.row_loss, agree=e.agree, m=r.m, log_s=r.logS, c=e.c, stats=e.stats,
               dlogits=e.dlogits)
    return {k: np.array(x, dtype=f64) for k, x in out.items()}


def _sum_b(term_abs, term_b, K):
    return term_b.sum(axis=1) + K * E * term_abs.sum(axis=1)


def _mix_b(cfg, e, p, b_p, b_lp, lp):
    """jsd's per-column pieces from a student (p, lp) with bounds: (b_lm, u, b_u, mi > 0)."""
    ab, beta, omb = np.abs, cfg.beta, 1.0 - cfg.beta
    mi = beta * e.q + omb * p
    some = mi > 0
    b_mi = E * beta * e.q + 2 * E * omb * p + omb * b_p + E * mi
    lm = _log(mi)
    b_lm = np.where(some, b_mi / np.where(some, mi, 1.0), 0.0) + C_FN * E * ab(lm)
    u = omb * (lp - lm)
    b_u = omb * (b_lp + b_lm + E * ab(lp - lm)) + 2 * E * ab(u)
    return lm, b_lm, u, b_u


def reference(c):
    """c: a case with cfg = cfg32(...). → dict name → (ref, bound) for row_stats' eight columns, `stats` and the chained
    `dlogits` (the specification's, with the forward's bounds propagated)."""
    cfg = c.cfg
    spec = DL.distill_loss(c.logits.astype(f64), c.tgt, c.teacher.astype(f64), cfg)
    e = evaluate(c, f64)
    r, v, ab = e.r, e.r.valid, np.abs
    rows, count = len(c.tgt), r.count
    b = P64._rows(r)
    K = 4 * math.ceil(count / 1024) + 9
    am = ab(r.z.max(axis=1))
    alpha = C_Z * (ab(r.z) + am[:, None]) + ab(r.d)
    q, lq, lp, p = e.q, e.lq, e.lp, e.p
    idx = np.arange(count, dtype=f64)
    b_lq = C_FN * E * ab(lq)
    b_lp = E * alpha + b.logS[:, None] + E * ab(lp)
    b_p = P64._exp_b(lp, b_lp) + TINY
    b_Q = K * E * e.Q
    b_te = _sum_b(ab(q * lq), q * b_lq + E * ab(q * lq), K)
    b_iq = (K + 1) * E * e.IQ
    b_ip = _sum_b(idx * p, idx * b_p + E * idx * p, K)
    b_gap = b_ip + b_iq + E * ab(e.IP - e.IQ)
    beta, sft = cfg.beta, cfg.sft_coef
    if cfg.kind == "forward_kl":
        b_t = q * (b_lq + b_lp + E * ab(lq - lp)) + E * ab(e.t)
        b_D = _sum_b(ab(e.t), np.where(q > 0, b_t, 0.0), K)
        b_c = b_Q
    elif cfg.kind == "reverse_kl":
        b_u = b_lp + b_lq + E * ab(e.u)
        b_D = _sum_b(ab(e.t), b_p * ab(e.u) + p * b_u + E * ab(e.t), K)
        b_c = b_D
    else:
        lm, b_lm, u, b_u = _mix_b(cfg, e, p, b_p, b_lp, lp)
        b_A = _sum_b(ab(e.tq), np.where(q > 0, q * (b_lq + b_lm + E * ab(lq - lm)) + E * ab(e.tq), 0.0), K)
        b_C = _sum_b(ab(e.tp), np.where(p > 0, b_p * ab(u) + p * b_u + E * ab(e.tp), 0.0), K)
        b_D = beta * b_A + E * ab(beta * e.A) + b_C + E * (ab(beta * e.A) + ab(e.C))
        b_c = b_C
    b_loss = b_D + sft * b.logp + E * ab(sft * e.nll) + E * (ab(e.D) + ab(sft * e.nll))
    z = lambda x: np.where(v, x, 0.0)
    zr = np.zeros(rows)
    out = dict(logp=(spec.logp, b.logp), entropy=(spec.entropy, b.H), divergence=(spec.divergence, z(b_D)), row_loss=(spec.row_loss, z(b_loss)),
               agree=(spec.agree, zr), m=(spec.m, b.m), log_s=(spec.log_s, b.logS), c=(spec.c, z(b_c)))
    depth = math.ceil(rows / 256) + 10
    mb = lambda x, bx: P64._mean_b(x, bx, v, depth)
    out["stats"] = (spec.stats, np.array([mb(e.row_loss, b_loss), 0.0, mb(e.D, b_D), mb(r.H, b.H), mb(e.te_row, b_te), mb(e.agree, zr),
                                          mb(e.nll, b.logp), mb(e.gap, b_gap)]))
    # the backward, chained
    w = e.bwd
    cb, bcb = e.c[:, None], z(b_c)[:, None]
    b_off = (b.m + b.logS)[:, None] + E * ab(w.off)
    b_lp2 = C_Z * E * ab(w.z) + b_off + E * ab(w.lp)
    b_p2 = P64._exp_b(w.lp, b_lp2) + TINY
    if cfg.kind == "forward_kl":
        dz = w.p * cb - q
        b_dz = b_p2 * ab(cb) + w.p * bcb + 2 * E * ab(w.p * cb) + E * q
    else:
        if cfg.kind == "reverse_kl":
            u2 = w.lp - lq
            b_u2 = b_lp2 + b_lq + E * ab(u2)
        else:
            _, _, u2, b_u2 = _mix_b(cfg, e, w.p, b_p2, b_lp2, w.lp)
        ww = u2 - cb
        b_w = b_u2 + bcb + E * (ab(u2) + ab(cb))
        dz = np.where(w.p > 0, w.p * ww, 0.0)
        b_dz = b_p2 * ab(ww) + w.p * b_w + E * ab(dz)
    s = sft * (w.p - w.oh)
    b_s = sft * (b_p2 + E * ab(w.p - w.oh)) + E * ab(s)
    core = w.scale * (b_dz + b_s) + C_SCALE * E * w.scale * (ab(dz) + ab(s))
    bound = np.zeros((rows, r.n))
    if e.nv:
        bound[:, r.first:r.first + count] = np.where(v[:, None], core, 0.0)
    out["dlogits"] = (spec.dlogits, bound)
    return P64._pack(out), NS(spec=spec, e=e)


# ---- the cases, shared by the CPU and the GPU test ---------------------------------------------------------------------------
def _softmax64(x):
    ex = np.exp(x - x.max(axis=1, keepdims=True))
    return ex / ex.sum(axis=1, keepdims=True)


ROW_KINDS = ("dense", "zeros", "ignored", "onehot", "self", "peaked", "peaked-self")
PEAK = 112.0          # exp(−112 / T) is 0 in fp32 for T <= 1: the student's tail underflows, and so does a teacher made from it


def case(name, rows, count, first, n, kind, T=1.0, sft=0.0, beta=0.5, seed=0, pad=0, tpad=0, dpad=0, only=None):
    """`rows` rows of `count` columns at column `first` of n-wide rows. Row j is ROW_KINDS[j % 7] (or `only`): a dense random
    teacher (row 0 with mass 1 + 5e-4), one with exact zeros, an ignored row, a one-hot teacher, the student's own softmax
    rounded to fp32, a student peaked so hard that its tail underflows against a dense teacher / against itself. reverse_kl
    takes a strictly positive stand-in where the row kind has zeros."""
    g = np.random.default_rng(seed)
    cfg = P64.cfg32(DL.DistillLossConfig(kind=kind, beta=beta, temperature=T, sft_coef=sft, token_range=None if (first == 0 and n == count) else (first, count)))
    L = np.minimum(P64._randn(g, (rows, count)), f32(5.0))
    top = g.integers(0, count, rows)
    L[np.arange(rows), top] = 5.5                        # the student's argmax, 0.5 / T above every other logit
    raw = np.exp(1.5 * g.standard_normal((rows, count)))
    qtop = np.where(g.random(rows) < 0.5, top, g.integers(0, count, rows))
    raw[np.arange(rows), qtop] = 2.0 * raw.max(axis=1)   # the teacher's argmax, twice the runner-up
    tgt = g.integers(0, count, rows).astype(np.int64)
    q = raw / raw.sum(axis=1, keepdims=True)
    for j in range(rows):
        rk = only or ROW_KINDS[j % 7]
        if rk.startswith("peaked"):
            L[j] = 0.0
            L[j, top[j]] = PEAK
        if rk == "dense" and j == 0:
            q[j] *= 1.0005
        elif rk == "zeros" and kind != "reverse_kl":
            keep = g.random(count) >= 0.4
            keep[qtop[j]] = True
            q[j] = np.where(keep, raw[j], 0.0) / raw[j][keep].sum()
        elif rk == "ignored":
            tgt[j] = IGN
        elif rk == "onehot":
            q[j] = 0.0 if kind != "reverse_kl" else 0.1 / count
            q[j, qtop[j]] += 1.0 if kind != "reverse_kl" else 0.9
        elif rk in ("self", "peaked-self") and not (rk == "peaked-self" and kind == "reverse_kl"):
            q[j] = _softmax64(L[j:j + 1].astype(f64) / float(f32(T)))[0]
    q = q.astype(f32)
    Lw, tw = P64.embed(L, tgt, n, first, seed + 1) if n != count else (L, tgt)
    c = NS(name=name, logits=Lw, tgt=tw, teacher=q, cfg=cfg, pad=pad, tpad=tpad, dpad=dpad)
    assert_away(c)
    return c


def assert_away(c):
    """Both arg-maxes at least 1e-3 above the runner-up on every valid row, no teacher value in (0, 2^-100), the teacher's
    mass within the precondition: conditions on the inputs, asserted on the fp64 reference."""
    first, count = c.cfg.token_range or (0, c.logits.shape[1])
    v = c.tgt != IGN
    if not v.any():
        return
    p = _softmax64(c.logits[v, first:first + count].astype(f64) / c.cfg.temperature)
    q = c.teacher[v].astype(f64)
    for name, x in (("student", p), ("teacher", q)):
        s = np.sort(x, axis=1)
        assert count == 1 or (s[:, -1] - s[:, -2] >= 1e-3).all(), f"{c.name}: the {name}'s argmax is within 1e-3 of the runner-up"
    assert not ((q > 0) & (q < 2.0 ** -100)).any(), f"{c.name}: a teacher value in (0, 2^-100)"
    assert (np.abs(q.sum(axis=1) - 1) <= 1e-3).all()


def cases():
    """count 8, 256 (the last of the wave form), 264 (the first of the workgroup form), 1032 (a thread loops twice) x the three
    kinds; rows 1, 5, 37; the range at column 0, ending at n, strictly inside; T 1 and 0.7; sft_coef 0 and 0.3; ld > n, ldt >
    count, ldd > n in turn. Then every row ignored, every row of one kind of teacher at 8 columns, and the unranged form."""
    out = []
    for ci, count in enumerate((8, 256, 264, 1032)):
        for ki, kind in enumerate(DL.KINDS):
            i = 3 * ci + ki
            rows = (1, 5, 37)[(ci + ki) % 3]
            first, n = ((0, count + 16), (16, count + 16), (8, count + 24))[i % 3]
            out.append(case(f"{kind}-count{count}-rows{rows}-first{first}", rows, count, first, n, kind, T=0.7 if i % 2 else 1.0,
                            sft=0.3 if (ci + ki) % 2 else 0.0, beta=(0.5, 0.3, 0.8)[ci % 3], seed=100 + i, pad=4 * (i % 3), tpad=4 * ((i + 1) % 2),
                            dpad=8 * (i % 2)))
    out.append(case("all-ignored", 5, 8, 8, 24, "jsd", seed=50, only="ignored", pad=4, tpad=4, dpad=8))
    for ki, kind in enumerate(DL.KINDS):
        for rk in ("zeros", "onehot", "self", "peaked", "peaked-self"):
            out.append(case(f"{kind}-{rk}", 3, 8, 0, 8, kind, T=0.7, sft=0.3 * (ki % 2), beta=0.4, seed=60 + 7 * ki + len(out), only=rk))
    return out
