"""The fp64 training-step comparators (tests/train_ref64.py) tell right from wrong, on the CPU.

Legitimate implementations — autograd over oracle/restate.py where it has the op, and an fp32 torch restatement that
follows the kernel's blocking (fp32 row statistics, 16-row partials summed in a fixed order, erf_as / silu_f written out
op for op) — must pass the per-element bounds with the derived constants. Wrong algorithms, computed in fp64 so that
only the algorithm is wrong, at the shapes the GPU test uses, must fail them. Which of the wrong algorithms the older
whole-tensor check (`grad_close` at 2e-2, tests/test_train_ops_gpu.py) would accept is printed as evidence; it asserts
nothing.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import train_ref64 as T64
from conftest import rand_bf16
from oracle import restate as R

P = R.Prec(True, grad_identity=True)      # roundings are the identity in the backward, as in the kernels
EPS = 1e-6
f32 = torch.float32


def rbf(t):
    return t.to(torch.bfloat16).to(f32)


def _norm_inputs(rows, dim, seed=1):
    x, w = rand_bf16((rows, dim), seed, 2.0), P.rb(rand_bf16((dim,), seed + 1, 0.02) + 1)
    return x, w, rand_bf16((rows, dim), seed + 2), rand_bf16((rows, dim), seed + 3)


def _block_sum(terms, rpb):
    """fp32 column sums the kernels' way: a sequential sum over the rows of each rpb-row block, then the partials in order."""
    parts = []
    for r0 in range(0, terms.shape[0], rpb):
        acc = torch.zeros(terms.shape[1], dtype=f32)
        for r in range(r0, min(terms.shape[0], r0 + rpb)):
            acc = acc + terms[r]
        parts.append(acc)
    out = torch.zeros(terms.shape[1], dtype=f32)
    for p_ in parts:
        out = out + p_
    return out


def _norm_bwd_fp32(x, w, dy, dres, ln, rpb=16):
    """train.hip:136-213 in fp32 torch: one fp32 mean / rstd / dot / gsum per row, dx rounded once, dw from bf16(x̂) (RMSNorm)."""
    inv = torch.tensor(1.0 / x.shape[1], dtype=f32)
    mu = x.sum(-1, keepdim=True) * inv if ln else torch.zeros(x.shape[0], 1)
    xc = x - mu
    rstd = 1.0 / torch.sqrt((xc * xc).sum(-1, keepdim=True) * inv + EPS)
    g = w * dy
    dot = (g * xc * rstd).sum(-1, keepdim=True) * inv
    gsum = g.sum(-1, keepdim=True) * inv if ln else torch.zeros_like(dot)
    xh = xc * rstd
    dx = rstd * (g - gsum - xh * dot)
    if dres is not None:
        dx = dx + dres
    return rbf(dx), _block_sum(dy * (xh if ln else rbf(xh)), rpb), _block_sum(dy, rpb)


@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("rows,dim", [(70, 520), (17, 2056), (5, 8)])
def test_norm_backward_legitimate(ln, rows, dim):
    x, w, dy, dres = _norm_inputs(rows, dim)
    rpb, nblk = T64.norm_bwd_blocking(rows, dim, ((rows + 15) // 16) * dim * 2, ln)
    for use_dres in (False, True):
        ref = T64.norm_backward(x, w, dy, EPS, dres if use_dres else None, ln)
        # 1. autograd over the oracle
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        if ln:
            br = torch.zeros(dim, requires_grad=True)
            (R.layernorm(P, xr, wr, br, EPS) * dy).sum().backward()
        else:
            (R.rmsnorm(P, xr, wr, EPS) * dy).sum().backward()
        dx = rbf(xr.grad + dres) if use_dres else rbf(xr.grad)
        T64.check_norm_backward(f"cpu legit autograd {'ln' if ln else 'rms'}", ref, ln, rpb, nblk, dx, wr.grad, br.grad if ln else None)
        # 2. the fp32 restatement with the kernel's blocking
        dx, dw, db = _norm_bwd_fp32(x, w, dy, dres if use_dres else None, ln, rpb)
        T64.check_norm_backward(f"cpu legit fp32 {'ln' if ln else 'rms'}", ref, ln, rpb, nblk, dx, dw, db if ln else None)


def test_layerscale_colsum_legitimate():
    rows, cols = 300, 520
    dy, u, res = rand_bf16((rows, cols), 3), rand_bf16((rows, cols), 6), rand_bf16((rows, cols), 8)
    ls = P.rb(rand_bf16((cols,), 7, 0.02) + 0.1)
    ur, lr_ = u.clone().requires_grad_(True), ls.clone().requires_grad_(True)
    y = P.rb(P.rb(ur * lr_) + res)
    (y * dy).sum().backward()
    yr, ym = T64.scale_residual(u, ls, res)
    T64.assert_bf16_close(y.detach(), yr, ym, 2, "cpu legit autograd scale_residual")
    assert torch.equal(y.detach().double(), T64.rb64(yr))            # in fact bit for bit
    ref = T64.layerscale_backward(dy, u, ls)
    rpb, nblk = T64.rows_blocking(rows, cols, ((rows + 15) // 16) * cols, 16)
    c = T64.reduce_depth(rpb, nblk)
    for name, du, dsc in (("autograd", rbf(ur.grad), lr_.grad), ("fp32", rbf(dy * ls), _block_sum(dy * u, rpb))):
        T64.assert_bf16_close(du, ref["du"], ref["m_du"], 1, f"cpu legit {name} layerscale du")
        T64.assert_f32_close(dsc, ref["dscale"], ref["m_dscale"], c, f"cpu legit {name} dscale")
    cs, cm = T64.colsum(dy)
    rpb, nblk = T64.rows_blocking(rows, cols, ((rows + 63) // 64) * cols, 64)
    T64.assert_f32_close(_block_sum(dy, rpb), cs, cm, T64.reduce_depth(rpb // 4, nblk), "cpu legit fp32 colsum")
    T64.assert_f32_close(dy.sum(0), cs, cm, T64.reduce_depth(rpb // 4, nblk), "cpu legit torch colsum")


# ---- activations --------------------------------------------------------------------------------------------------------
EDGES = [0.0, 2.0 ** -127, -2.0 ** -127, 2.0 ** -130, -2.0 ** -130, 1.0, -1.0, 8.0, -8.0, 40.0, -40.0, 89.0, -89.0, 100.0,
         -100.0, 1e4, -1e4]


def edge_row(cols, seed):
    """A row of value edges (bf16-representable), padded with N(0, 4) values up to `cols`."""
    r = rand_bf16((cols,), seed, 2.0)
    r[:len(EDGES)] = torch.tensor(EDGES, dtype=f32).to(torch.bfloat16).float()
    return r


def _erf_as32(x):
    """erf_as (bl_common.h:49-55) op for op in fp32 torch (torch.exp for __expf)."""
    ax = x.abs()
    t = 1.0 / torch.addcmul(torch.ones_like(ax), ax, torch.tensor(0.3275911, dtype=f32))
    c = [torch.tensor(v, dtype=f32) for v in (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)]
    poly = c[0]
    for k in c[1:]:
        poly = poly * t + k
    y = 1.0 - (t * poly) * torch.exp(-ax * ax)
    return torch.copysign(y, x)


def _gelu32(x):
    return 0.5 * x * (1.0 + _erf_as32(x * torch.tensor(0.70710678118654752440, dtype=f32)))


def _gelu_grad32(x):
    return 0.5 * (1.0 + _erf_as32(x * torch.tensor(0.70710678118654752440, dtype=f32))) + \
        x * torch.tensor(0.39894228040143267794, dtype=f32) * torch.exp(-0.5 * x * x)


def _act_inputs(rows, cols, seed, scale):
    x = rand_bf16((rows, cols), seed, scale)
    x[0] = edge_row(cols, seed + 50)
    return x


def test_gelu_legitimate():
    x, dy = _act_inputs(40, 832, 3, 2.0), rand_bf16((40, 832), 4)
    # a dense sweep of the far negative tail, where erf_as's absolute error decides
    x[1] = torch.linspace(-9.0, -2.0, 832).to(torch.bfloat16).float()
    fr, br = T64.gelu_forward(x), T64.gelu_backward(x, dy)
    xr = x.clone().requires_grad_(True)
    y = R.gelu(P, xr)
    (y * dy).sum().backward()
    for name, yy, dx in (("autograd", y.detach(), rbf(xr.grad)), ("fp32 erf_as", rbf(_gelu32(x)), rbf(dy * _gelu_grad32(x)))):
        T64.assert_bf16_close(yy, fr["y"], fr["mag"], 4, f"cpu legit {name} gelu fwd", extra=fr["extra"])
        T64.assert_bf16_close(dx, br["dx"], br["mag"], 4, f"cpu legit {name} gelu bwd", extra=br["extra"])
    # erf_as itself stays inside E_ERF = A_S + its fp32 evaluation, over the whole range
    z = torch.linspace(-6.0, 6.0, 200001, dtype=f32)
    err = (_erf_as32(z).double() - torch.erf(z.double())).abs().max().item()
    print(f"erf_as fp32 restatement: max |error| {err:.3g} (A_S {T64.A_S:.3g}, E_ERF {T64.E_ERF:.3g})")
    assert err <= T64.E_ERF


def _silu32(x):
    return x * (1.0 / (1.0 + torch.exp(-x)))


def test_swiglu_legitimate():
    M, I = 37, 1536
    gu, dact = _act_inputs(M, 2 * I, 1, 1.5), rand_bf16((M, I), 2)
    gu[0, 0::2][:len(EDGES)] = torch.tensor(EDGES, dtype=f32).to(torch.bfloat16).float()      # the edges in the gate
    gu[0, 1::2][:len(EDGES)] = rand_bf16((len(EDGES),), 9)
    fr, br = T64.swiglu_forward(gu), T64.swiglu_backward(gu, dact)
    gur = gu.clone().requires_grad_(True)
    act = P.rb(P.rb(F.silu(gur[:, 0::2])) * gur[:, 1::2])
    (act * dact).sum().backward()
    g, up = gu[:, 0::2], gu[:, 1::2]
    sg = 1.0 / (1.0 + torch.exp(-g))
    dgu = torch.empty_like(gu)
    dgu[:, 0::2], dgu[:, 1::2] = dact * up * (sg * (1.0 + g * (1.0 - sg))), dact * rbf(g * sg)
    for name, a, d in (("autograd", act.detach(), rbf(gur.grad)), ("fp32", rbf(rbf(_silu32(g)) * up), rbf(dgu))):
        T64.assert_bf16_close(a, fr["act"], fr["mag"], 2, f"cpu legit {name} swiglu fwd", tie=fr["tie"], extra=fr["extra"])
        T64.check_swiglu_backward(f"cpu legit {name} swiglu bwd", br, d)


def _rope_case(B=2, S=19, H=4, hd=80, pos0=3):
    D = H * hd
    dqkv = rand_bf16((B * S, 3 * D), 6)
    cos, sin = R.rope_tables(hd, 64, 10000.0)
    return B, S, H, hd, pos0, dqkv, cos, sin


def test_rope_backward_legitimate():
    B, S, H, hd, pos0, dqkv, cos, sin = _rope_case()
    ref, mag = T64.rope_backward(dqkv, cos, sin, B, S, H, hd, pos0)
    qr = rand_bf16(dqkv.shape, 5).requires_grad_(True)
    t = qr.view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    out = torch.stack([R.apply_rope(P, t[0], cos, sin, pos0), R.apply_rope(P, t[1], cos, sin, pos0), t[2]])
    (out * dqkv.view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)).sum().backward()
    T64.assert_bf16_close(rbf(qr.grad), ref, mag, 2, "cpu legit autograd rope bwd")
    assert torch.equal(rbf(qr.grad)[:, 2 * H * hd:], dqkv[:, 2 * H * hd:])


# ---- cross-entropy, GEMM, scatter, optimizer ------------------------------------------------------------------------------
def ce_case(rows, n, seed=0):
    """fp32 logits of bf16-representable values and targets: 0 and n − 1, a target 60 above and one 60 below the rest,
    every third row ignored."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(rows, n, generator=g) * 2).to(torch.bfloat16).float()
    tgt = torch.randint(0, n, (rows,), generator=g)
    tgt[1], tgt[2] = 0, n - 1
    logits[4, tgt[4]] = 68.0
    logits[5, tgt[5]] = -68.0
    tgt[::3] = -100
    return logits, tgt


@pytest.mark.parametrize("n", [8, 2056])
def test_cross_entropy_legitimate(n):
    rows = 12
    logits, tgt = ce_case(rows, n)
    ref = T64.cross_entropy(logits, tgt)
    lg = logits.clone().requires_grad_(True)
    loss = F.cross_entropy(lg, tgt, ignore_index=-100)
    loss.backward()
    T64.assert_bf16_close(rbf(lg.grad), ref["dl"], ref["mag"], T64.C_CE, "cpu legit autograd dlogits")
    T64.assert_f32_close(loss.detach(), ref["mean"], ref["m_mean"], T64.C_CE_MEAN, "cpu legit autograd ce mean")
    # fp32 two-pass softmax as in train.hip:41-67
    mx = logits.amax(-1, keepdim=True)
    s = torch.exp(logits - mx).sum(-1, keepdim=True)
    cnt = torch.tensor(float(ref["count"]))
    d = torch.exp(logits - mx) * (1.0 / (s * cnt)) - F.one_hot(tgt.clamp(min=0), n) * (1.0 / cnt)
    d = torch.where((tgt != -100).view(-1, 1), d, torch.zeros(()))
    T64.assert_bf16_close(rbf(d), ref["dl"], ref["mag"], T64.C_CE, "cpu legit fp32 dlogits")
    assert (rbf(d)[::3] == 0).all() and ref["count"] == rows - len(range(0, rows, 3))


def test_gemm_tn_embed_legitimate():
    Tn, Rr, N = 389, 64, 192
    Pm, Q = rand_bf16((Tn, Rr), Tn + Rr), rand_bf16((Tn, N), N)
    ref, mag = T64.gemm_tn(Pm, Q, 0.25)
    acc = torch.zeros(Rr, N)
    for t0 in range(0, Tn, 32):                                   # 32-row steps in order, as the MFMA loop
        acc = acc + Pm[t0:t0 + 32].t() @ Q[t0:t0 + 32]
    T64.assert_f32_close(acc * 0.25, ref, mag, Tn + T64.C_TN_EXTRA, "cpu legit fp32 gemm_tn")
    B, L, D, V, NP = 2, 6, 64, 50, 4
    ids = torch.tensor([[1, 5, 7, 5, 9, 2], [1, 5, 3, 3, 3, 2]])
    dx, dw0 = rand_bf16((B, L + NP, D), 1), rand_bf16((V, D), 2)
    dw, m, hits = T64.embed_backward(ids, dx, dw0, NP)
    got = dw0.clone()
    for b in range(B):
        for j in range(L):
            got[ids[b, j]] += dx[b, 0 if j == 0 else j + NP]
    T64.assert_f32_close(got, dw, m, (hits + 1).view(-1, 1), "cpu legit fp32 embed bwd")


def _adamw32(p, m, v, g, step, lr, b1, b2, eps, wd, coef):
    """adamw_kernel (train.hip:839-853) in fp32 torch."""
    t = lambda a: torch.tensor(a, dtype=f32)
    lr, b1, b2, eps, wd = t(lr), t(b1), t(b2), t(eps), t(wd)
    bc1, bc2s = 1.0 - b1 ** step, torch.sqrt(1.0 - b2 ** step)
    gi = g * t(coef)
    pi = p * (1.0 - lr * wd)
    mi = b1 * m + (1.0 - b1) * gi
    vi = b2 * v + (1.0 - b2) * gi * gi
    return pi - (lr / bc1) * (mi / (torch.sqrt(vi) / bc2s + eps)), mi, vi


def adam_case(n=1000, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01,
            torch.randn(n, generator=g))


ADAM_HP = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.1)


@pytest.mark.parametrize("step", [1, 1000])
def test_optimizer_legitimate(step):
    p, m, v, g = adam_case()
    hp = ADAM_HP
    ref = T64.adamw_step(p, m, v, g, step, coef=0.5, **hp)
    pn, mn, vn = _adamw32(p, m, v, g, step, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], 0.5)
    T64.assert_f32_close(pn, ref["p"], ref["m_p"], T64.C_ADAM_P, "cpu legit fp32 adamw p")
    T64.assert_f32_close(mn, ref["m"], ref["m_m"], T64.C_ADAM_M, "cpu legit fp32 adamw m")
    T64.assert_f32_close(vn, ref["v"], ref["m_v"], T64.C_ADAM_V, "cpu legit fp32 adamw v")
    if step == 1:                                                  # torch.optim.AdamW from zero moments
        pr = p.clone().requires_grad_(True)
        opt = torch.optim.AdamW([pr], lr=hp["lr"], betas=(0.9, 0.999), eps=1e-8, weight_decay=hp["wd"])
        pr.grad = g.clone()
        opt.step()
        r0 = T64.adamw_step(p, torch.zeros_like(p), torch.zeros_like(p), g, 1, **hp)
        T64.assert_f32_close(pr.detach(), r0["p"], r0["m_p"], T64.C_ADAM_P, "cpu legit torch AdamW p")
    ss = (g * g).sum()
    T64.assert_f32_close(ss, T64.sumsq(g), T64.sumsq(g), 1 + 16, "cpu legit fp32 sumsq")
    norm = float(torch.sqrt(ss.double()).float())
    for mx in (0.5, 1e3):
        c32 = torch.minimum(torch.tensor(1.0), torch.tensor(mx) / (torch.tensor(norm) + torch.tensor(1e-6)))
        T64.assert_f32_close(c32, torch.tensor(T64.clip_coef(norm, mx), dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64),
                             4, "cpu legit fp32 clip coef")


# ---- wrong algorithms, each computed in fp64 ------------------------------------------------------------------------------
def _rejected(what, accepts_old, fn):
    """fn() must raise the comparator's AssertionError; print whether grad_close(…, 2e-2) would have accepted the defect."""
    print(f"wrong algorithm: {what}: grad_close(2e-2) {'ACCEPTS' if accepts_old else 'rejects'} it")
    with pytest.raises(AssertionError, match="out of bound"):
        fn()


def _norm64(x, w, dy, dres, ln, *, dim_off=0, drop_row=None, dup_row=None, no_dres_row=None, unrounded=False, no_gsum=False):
    """The norm backward in fp64 with one defect switched on."""
    x, w, dy = x.double(), w.double(), dy.double()
    n = x.shape[1] + dim_off
    xc = x - (x.sum(-1, keepdim=True) / n if ln else 0.0)
    rstd = 1.0 / torch.sqrt((xc * xc).sum(-1, keepdim=True) / n + EPS)
    xh, g = xc * rstd, w * dy
    dot = (g * xh).sum(-1, keepdim=True) / n
    gsum = g.sum(-1, keepdim=True) / n if (ln and not no_gsum) else 0.0
    dx = rstd * (g - gsum - xh * dot)
    if dres is not None:
        add = dres.double().clone()
        if no_dres_row is not None:
            add[no_dres_row] = 0
        dx = dx + add
    wt = torch.ones(x.shape[0], 1, dtype=torch.float64)
    if drop_row is not None:
        wt[drop_row] = 0
    if dup_row is not None:
        wt[dup_row] = 2
    if unrounded:
        terms = w * xh                                               # Σ w ⊙ x̂, unrounded: w in dy's place
    else:
        terms = dy * (xh if ln else T64.rb64(xh))
    return dx, (wt * terms).sum(0), (wt * dy).sum(0)


def test_wrong_norm_backward_rejected():
    rows, dim = 70, 520
    x, w, dy, dres = _norm_inputs(rows, dim)
    for ln in (False, True):
        nm = "ln" if ln else "rms"
        ref = T64.norm_backward(x, w, dy, EPS, dres, ln)
        rpb, nblk = T64.norm_bwd_blocking(rows, dim, ((rows + 15) // 16) * dim * 2, ln)
        chk = lambda dx=None, dw=None, db=None: (lambda: T64.check_norm_backward(f"cpu wrong {nm}", ref, ln, rpb, nblk, dx, dw, db))
        good = _norm64(x, w, dy, dres, ln)
        T64.check_norm_backward(f"cpu fp64 {nm}", ref, ln, rpb, nblk, *good[:2], good[2] if ln else None)
        dx, dw, db = _norm64(x, w, dy, dres, ln, dup_row=rows - 1)
        _rejected(f"{nm} dw: last row of the ragged block twice", T64.grad_close_accepts(dw, ref["dw"]), chk(dw=dw))
        dx, dw, db = _norm64(x, w, dy, dres, ln, no_dres_row=33)
        small = dres.clone(); small[33] *= 2.0 ** -7                 # the same defect on a row whose dres is small
        _rejected(f"{nm} dx: dres not added on one row", T64.grad_close_accepts(dx, ref["dx"]), chk(dx=dx))
        ref_s = T64.norm_backward(x, w, dy, EPS, small, ln)
        dxs = _norm64(x, w, dy, small, ln, no_dres_row=33)[0]
        _rejected(f"{nm} dx: a small dres not added on one row", T64.grad_close_accepts(dxs, ref_s["dx"]),
                  lambda: T64.assert_bf16_close(dxs, ref_s["dx"], ref_s["m_dx"], T64.C_NORM_DX, f"cpu wrong {nm} dx"))
        dx, dw, db = _norm64(x, w, dy, dres, ln, dim_off=8)
        _rejected(f"{nm} dx: mean over dim + 8", T64.grad_close_accepts(dx, ref["dx"]), chk(dx=dx))
        if ln:
            dx, dw, db = _norm64(x, w, dy, dres, ln, no_gsum=True)
            _rejected("ln dx: no mean(g) term", T64.grad_close_accepts(dx, ref["dx"]), chk(dx=dx))
            dx, dw, db = _norm64(x, w, dy, dres, ln, drop_row=41)
            _rejected("ln dw: one row dropped (70 rows)", T64.grad_close_accepts(dw, ref["dw"]), chk(dw=dw))
            _rejected("ln db: one row dropped (70 rows)", T64.grad_close_accepts(db, ref["db"]), chk(db=db))
        else:
            dx, dw, db = _norm64(x, w, dy, dres, ln, unrounded=True)
            _rejected("rms dw: unrounded x̂·w (w and dy swapped)", T64.grad_close_accepts(dw, ref["dw"]), chk(dw=dw))


def test_wrong_one_row_dropped_at_the_largest_row_count_rejected():
    """RMSNorm dw at 8200 x 2560, dscale at 61 blocks of 16 rows, colsum at 300 rows: one row of the sum missing."""
    rows, dim = 8200, 2560
    x, w, dy, _ = _norm_inputs(rows, dim)
    ref = T64.norm_backward(x, w, dy, EPS, None, False)
    rpb, nblk = T64.norm_bwd_blocking(rows, dim, ((rows + 15) // 16) * dim, False)
    assert (rpb, nblk) == (20, 410)
    xs, ds = x[4321:4322].double(), dy[4321:4322].double()
    rstd = 1.0 / torch.sqrt((xs * xs).mean(-1, keepdim=True) + EPS)
    dw = ref["dw"] - (ds * T64.rb64(xs * rstd)).sum(0)
    T64.check_norm_backward("cpu fp64 rms 8200", ref, False, rpb, nblk, dw=ref["dw"])
    _rejected("rms dw: one row of 8200 dropped", T64.grad_close_accepts(dw, ref["dw"]),
              lambda: T64.check_norm_backward("cpu wrong rms 8200", ref, False, rpb, nblk, dw=dw))
    rows, cols = 61 * 16, 64
    dyl, u, ls = rand_bf16((rows, cols), 3), rand_bf16((rows, cols), 6), P.rb(rand_bf16((cols,), 7, 0.02) + 0.1)
    r = T64.layerscale_backward(dyl, u, ls)
    bad = r["dscale"] - (dyl[500] * u[500]).double()
    _rejected("dscale: one row of 976 dropped", T64.grad_close_accepts(bad, r["dscale"]),
              lambda: T64.assert_f32_close(bad, r["dscale"], r["m_dscale"], T64.reduce_depth(16, 61), "cpu wrong dscale"))
    a = rand_bf16((300, 520), 1)
    cs, cm = T64.colsum(a)
    bad_c = cs - a[299].double()
    _rejected("colsum: one row of 300 dropped", T64.grad_close_accepts(bad_c, cs),
              lambda: T64.assert_f32_close(bad_c, cs, cm, T64.reduce_depth(16, 5), "cpu wrong colsum"))


def test_wrong_elementwise_rejected():
    M, I = 37, 1536
    gu, dact = rand_bf16((M, 2 * I), 1, 1.5), rand_bf16((M, I), 2)
    br = T64.swiglu_backward(gu, dact)
    sw = gu.clone()
    sw[:, 0::2], sw[:, 1::2] = gu[:, 1::2], gu[:, 0::2]
    bs = T64.swiglu_backward(sw, dact)["dgu"]
    bad = torch.empty_like(bs)
    bad[:, 0::2], bad[:, 1::2] = bs[:, 1::2], bs[:, 0::2]
    _rejected("swiglu bwd: gate and up swapped", T64.grad_close_accepts(bad, br["dgu"]),
              lambda: T64.check_swiglu_backward("cpu wrong swiglu bwd", br, bad))
    B, S, H, hd, pos0, dqkv, cos, sin = _rope_case()
    ref, mag = T64.rope_backward(dqkv, cos, sin, B, S, H, hd, pos0)
    fwd, _ = T64.rope_backward(dqkv, cos, -sin, B, S, H, hd, pos0)
    _rejected("rope bwd: the forward rotation (sign of sin)", T64.grad_close_accepts(fwd, ref),
              lambda: T64.assert_bf16_close(fwd, ref, mag, 2, "cpu wrong rope bwd"))


def test_wrong_cross_entropy_gemm_adamw_rejected():
    rows, n = 12, 2056
    logits, tgt = ce_case(rows, n)
    ref = T64.cross_entropy(logits, tgt)
    shifted = torch.where(tgt == -100, tgt, (tgt + 1) % n)
    bad = T64.cross_entropy(logits, shifted)["dl"]
    _rejected("ce bwd: one-hot at target + 1", T64.grad_close_accepts(bad, ref["dl"]),
              lambda: T64.assert_bf16_close(bad, ref["dl"], ref["mag"], T64.C_CE, "cpu wrong dlogits"))
    bad = ref["dl"] * ref["count"] / rows
    _rejected("ce bwd: divided by the row count", T64.grad_close_accepts(bad, ref["dl"]),
              lambda: T64.assert_bf16_close(bad, ref["dl"], ref["mag"], T64.C_CE, "cpu wrong dlogits"))
    Tn, Rr, N = 1030, 64, 64
    Pm, Q = rand_bf16((Tn, Rr), Tn + Rr), rand_bf16((Tn, N), N)
    r, m = T64.gemm_tn(Pm, Q, 1.0)
    bad_g, _ = T64.gemm_tn(Pm[:Tn // 32 * 32], Q[:Tn // 32 * 32], 1.0)
    _rejected("gemm_tn_small: last partial 32-row step missing", T64.grad_close_accepts(bad_g, r),
              lambda: T64.assert_f32_close(bad_g, r, m, Tn + T64.C_TN_EXTRA, "cpu wrong gemm_tn"))
    p, mm, v, g = adam_case()
    r = T64.adamw_step(p, mm, v, g, 1000, **ADAM_HP)
    bad_p = T64.adamw_step(p, mm, v, g, 1000, coupled=True, **ADAM_HP)["p"]
    _rejected("adamw: coupled weight decay", T64.grad_close_accepts(bad_p, r["p"]),
              lambda: T64.assert_f32_close(bad_p, r["p"], r["m_p"], T64.C_ADAM_P, "cpu wrong adamw p"))
