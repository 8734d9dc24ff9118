"""bl_value_head_f32 / bl_value_head_backward_f32 (csrc/value.hip) against their fp64 definition (training/value_loss.py),
per element, nothing excluded: every output of both entry points, the index list exactly, rows that are not value rows
poisoned with NaN on the way in and checked for zeros / untouched bits on the way out, canaries behind every output.

Bounds, in the style of tests/train_ref64.py: |got − ref| <= c·e·mag (+ u·|ref| for the bf16 dh), e = 2^-24, u = 2^-8, `mag`
the same expression over absolute values. The constants follow from the kernels' own summation depth (value.hip's header
comment states the orders), each fp32 add / mul / fma / division contributing at most 1·e relative, first order, +1 for the
cross terms:

* v = Σ hn·w + b. A bf16·bf16 product is exact in fp32. A lane adds ceil(dim/512) pieces of 8 in one chain, wave_sum adds
  6 butterfly levels, + b: C_V = 8·ceil(dim/512) + 7 against mag_v = Σ|hn|·|w| + |b|.
* e = v − R, d = v − vo, ec = (vo ± c) − R: at most 3 more roundings, +1: each of e, ec is off by at most
  de = (C_V + 4)·e·M with M = mag_v + |R| + 2|vo| (M also bounds |e| and |ec|).
* l = ½·max(e², ec²): 2·max(|e|, |ec|)·de / 2 for the square, its rounding ½·e·l·2 <= e·M·max/2, +1:
  C_L = C_V + 6 against M·max(|e|, |ec|). Which branch is taken is not within reach of these errors in the test data
  (|v − vo| is 0.5c or 2c, and |e| and |ec| differ by at least 0.2 outside the range).
* dv = (coef·e) / n: de and two roundings, +1: C_DV = C_V + 7 against coef·M / n.
* statistics: a thread adds ceil(n/256) values, the wave 6, the block 3, the product with 1/n and 1/n itself 2:
  K_S = ceil(n/256) + 11 relative to the mean of the absolute values, on top of the mean of the addends' own bounds.
  clip_frac sums 0 / 1 exactly: 2·e. total = p + coef·value_loss: two roundings against |p| + coef·value_loss.
  explained variance 1 − s0 / s1, s0 = Σ(e − ē)², s1 = Σ(R − R̄)²: with δē, δR̄ the bounds of the two means,
  b0 = Σ 2|e_j − ē|·(de_j + δē + e·(|e_j| + |ē|)) + (K_S + 2)·e·s0, b1 alike without de, and
  |Δ| <= (b0 + (s0/s1)·b1) / s1 + 2·e·(s0/s1) + e·|1 − s0/s1|.
* dw[k] = Σ_r (dv_r·inv_world)·hn[r,k]: one thread, n fma steps and the product with inv_world: (n + 1)·e·Σ|dv·hn| on top of
  Σ tol_dv·|hn|. db: a lane adds ceil(n/64) values, the wave 6, the product 1: (ceil(n/64) + 7)·e·Σ|dv| + Σ tol_dv.
* dh = bf16(dh + dv·w): u·|ref| + |w|·tol_dv + 3·e·(|dh| + |dv·w|).
"""
import math

import numpy as np
import pytest
import torch

from bridgelang_amd import _lib, train_ops as T
from bridgelang_amd.training.value_loss import ValueLossConfig, value_loss

pytestmark = pytest.mark.gpu

E, U = 2.0 ** -24, 2.0 ** -8
IGN = -100
CANARY_F, CANARY_I = 1234.5, 0x5A5A5A5

#        id            dim   ld    gr  groups level     clip  pattern     inv_world policy loss
CASES = [("d8",          8,    8,   3,   5,   "action", 0.2,  "mix",      1.0, 0.75),
         ("d512",      512,  512,   3,   5,   "token",  0.2,  "mix",      1.0, None),
         ("d520-ld",   520,  528,  70,   5,   "action", 0.2,  "mix",      1.0, 0.75),
         ("d4096",    4096, 4096,   3,   5,   "token",  None, "mix",      0.5, -0.3),
         ("d5120",    5120, 5120,   3,   1,   "action", 0.2,  "two",      1.0, None),
         ("n300",      512,  512,  70, 300,   "action", 0.2,  "labelled", 1.0, 0.75),
         ("tok-many",    8,    8,  70, 300,   "token",  0.2,  "mix",      1.0, None),
         ("gr1",       512,  512,   1, 300,   "action", None, "mix",      1.0, 0.75),
         ("none",      512,  512,   3,   5,   "token",  0.2,  "none",     1.0, 0.75),
         ("one-row",   512,  512,   1,   1,   "token",  None, "all",      0.5, None),
         ("last-only", 512,  512,  70,   1,   "action", 0.2,  "last",     1.0, None)]


def make_targets(gr: int, groups: int, pattern: str) -> np.ndarray:
    tg = np.full((groups, gr), IGN, dtype=np.int64)
    cycle = {"mix": ("first", "two", "none", "all", "last"), "labelled": ("two", "first", "all", "last")}.get(pattern, (pattern,))
    for g in range(groups):
        p = cycle[g % len(cycle)]
        if p == "first":
            tg[g, 0] = 5
        elif p == "last":
            tg[g, gr - 1] = 5
        elif p == "all":
            tg[g, :] = 5
        elif p == "two":                    # two runs with a gap; the first starts past row 0 where the sequence is long enough
            a = 1 if gr >= 5 else 0
            tg[g, a:a + max(1, min(2, gr // 3))] = 5
            if gr >= 3:
                tg[g, gr - max(1, min(2, gr // 3)):] = 5
        elif p != "none":
            raise ValueError(p)
    return tg.reshape(-1)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16)


class Case:
    """Inputs (host + device), the fp64 reference (computed once) and the derived tolerances of one shape."""

    def __init__(self, spec, dev, seed=0):
        self.name, self.dim, self.ld, self.gr, self.groups, self.level, self.clip, self.pattern, self.inv_world, self.policy = spec
        self.dev = dev
        self.rows = rows = self.gr * self.groups
        self.cfg = ValueLossConfig(coef=0.7, clip=self.clip, level=self.level)
        self.cap = T.value_index_slots(rows, self.level, self.gr)
        g = torch.Generator().manual_seed(100 + seed)
        dim = self.dim
        self.tg = make_targets(self.gr, self.groups, self.pattern)
        hn = bf16_round(torch.randn(rows, dim, generator=g))
        self.w = bf16_round(torch.randn(dim, generator=g) * 0.05)
        self.b = bf16_round(torch.randn(1, generator=g) * 0.3)
        from bridgelang_amd.training.value_loss import value_row_index
        self.idx = idx = value_row_index(self.tg, self.level, self.gr)
        is_v = np.zeros(rows, dtype=bool)
        is_v[idx] = True
        self.is_v = is_v
        v = hn.double().numpy() @ self.w.double().numpy() + float(self.b)
        k = np.zeros(rows, dtype=np.int64)
        k[idx] = np.arange(len(idx)) % 8    # the eight combinations cycle over the value rows
        c = self.clip if self.clip is not None else 0.2
        off = np.array([0.5, -0.5, 2.0, -2.0, 2.0, -2.0, 0.5, -0.5])[k] * c
        side = np.array([1.0, 1.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0])[k]
        m = 0.2 + 0.4 * torch.rand(rows, generator=g).double().numpy()
        R, vo = (v + side * m).astype(np.float32), (v - off).astype(np.float32)
        R[~is_v] = np.nan                   # everything a value row does not own is poison
        vo[~is_v] = np.nan
        hn[torch.from_numpy(~is_v)] = float("nan")
        self.R, self.vo = R, vo
        self.hn_host = hn
        hn_pad = torch.full((rows, self.ld), float("nan"), dtype=torch.bfloat16)
        hn_pad[:, :dim] = hn
        self.hn = hn_pad.to(dev)[:, :dim]
        self.dh0 = bf16_round(torch.randn(rows, self.ld, generator=g))
        self.d_tg = torch.from_numpy(self.tg).to(dev)
        self.d_w, self.d_b = self.w.to(dev), self.b.to(dev)
        self.d_R, self.d_vo = torch.from_numpy(R).to(dev), torch.from_numpy(vo).to(dev)
        self.d_policy = None if self.policy is None else torch.tensor([self.policy] + [float("nan")] * 7, device=dev)
        self.ref = value_loss(hn.double().numpy(), self.tg, self.w.double().numpy(), float(self.b), R.astype(np.float64),
                              vo.astype(np.float64) if self.clip is not None else None, self.cfg, group_rows=self.gr,
                              policy_loss=self.policy or 0.0)

    # ---- device buffers: every output is a view with canaries behind it ----
    def outputs(self):
        dev, rows, dim = self.dev, self.rows, self.dim
        f = lambda n: torch.full((n,), CANARY_F, dtype=torch.float32, device=dev)
        o = dict(index=torch.full((self.cap + 16,), CANARY_I, dtype=torch.int32, device=dev),
                 count=torch.full((16,), CANARY_I, dtype=torch.int32, device=dev),
                 vrows=f(rows * 4 + 16), stats=f(16), dw=f(dim + 16), db=f(16), dh=self.dh0.to(dev).clone())
        return o

    def views(self, o):
        return dict(index=o["index"][:self.cap], count=o["count"][:1], vrows=o["vrows"][:self.rows * 4].view(self.rows, 4),
                    stats=o["stats"][:8], dw=o["dw"][:self.dim], db=o["db"][:1], dh=o["dh"][:, :self.dim])

    def launch(self, o, detach=False, tg=None, R=None, vo=None):
        v = self.views(o)
        vo = (self.d_vo if vo is None else vo) if self.clip is not None else None
        T.value_head(self.hn, self.d_tg if tg is None else tg, self.d_w, self.d_b, self.d_R if R is None else R, vo, self.cfg,
                     v["index"], v["count"], v["vrows"], v["stats"], policy_stats=self.d_policy, group_rows=self.gr, ignore_index=IGN)
        T.value_head_backward(self.hn, self.d_w, v["vrows"], v["index"], v["count"], v["dw"], v["db"], None if detach else v["dh"],
                              self.cfg, group_rows=self.gr, inv_world=self.inv_world)

    def tolerances(self):
        vo = self.vo.astype(np.float64)[self.idx] if self.clip is not None else None
        return value_tolerances(self.hn_host.double().numpy()[self.idx], self.w.double().numpy(), float(self.b),
                                self.R.astype(np.float64)[self.idx], vo, self.ref, self.cfg.coef, self.inv_world, self.policy or 0.0)


def value_tolerances(h, w, b, R, vo, ref, coef: float, inv_world: float = 1.0, policy: float = 0.0):
    """The bounds of the module docstring for one launch: h [n, dim], R, vo [n] (None: unclipped) are the kernel's inputs on
    the value rows, `ref` the definition's result on them. → (dict of per-output bounds, the bound of dv·inv_world per value
    row, |dv·inv_world|)."""
    idx, dim = ref.index, h.shape[1]
    n = len(idx)
    h, w, R_abs = np.abs(h), np.abs(w), np.abs(R)
    vo_abs = np.abs(vo) if vo is not None else np.zeros(n)
    c_v = 8 * math.ceil(dim / 512) + 7
    mag_v = h @ w + abs(b)
    M = mag_v + R_abs + 2 * vo_abs
    e = ref.value[idx] - R
    big = np.sqrt(2 * ref.loss[idx])                           # max(|e|, |ec|)
    de = (c_v + 4) * E * M
    tol = dict(v=c_v * E * mag_v, l=(c_v + 6) * E * M * big, dv=(c_v + 7) * E * coef * M / max(n, 1))
    ks = math.ceil(n / 256) + 11
    mean = lambda x: float(x.sum() / n) if n else 0.0
    t_vl = mean(tol["l"]) + ks * E * mean(ref.loss[idx])
    ev_tol = 0.0
    if n:
        s0, s1 = float(((e - e.mean()) ** 2).sum()), float(((R - R.mean()) ** 2).sum())
        if s1 > 0:
            d_e, d_r = mean(de) + ks * E * mean(np.abs(e)), ks * E * mean(R_abs)
            b0 = float((2 * np.abs(e - e.mean()) * (de + d_e + E * (np.abs(e) + abs(e.mean())))).sum()) + (ks + 2) * E * s0
            b1 = float((2 * np.abs(R - R.mean()) * (d_r + E * (R_abs + abs(R.mean())))).sum()) + (ks + 2) * E * s1
            x = s0 / s1
            ev_tol = (b0 + x * b1) / s1 + 2 * E * x + E * abs(1 - x)
    tol["stats"] = np.array([t_vl, 0.0, 2 * E, mean(tol["v"]) + ks * E * mean(np.abs(ref.value[idx])), ks * E * mean(R_abs), ev_tol,
                             mean(de) + ks * E * mean(np.abs(e)), coef * t_vl + 2 * E * (abs(policy) + coef * ref.value_loss)])
    dv = np.abs(ref.dv[idx]) * inv_world
    tdv = tol["dv"] * inv_world
    tol["dw"] = tdv @ h + (n + 1) * E * (dv @ h)
    tol["db"] = float(tdv.sum()) + (math.ceil(n / 64) + 7) * E * float(dv.sum())
    return tol, tdv, dv


_cases = {}


def get_case(name, dev) -> Case:
    if name not in _cases:
        _cases[name] = Case(next(s for s in CASES if s[0] == name), dev)
    return _cases[name]


def check_outputs(cs: Case, o, detach=False):
    """Every element of every output against the definition; zeros / untouched bits where no value row owns them."""
    ref, idx, rows, dim, n = cs.ref, cs.idx, cs.rows, cs.dim, len(cs.idx)
    tol, tdv, dv = cs.tolerances()
    host = {k: v.cpu() for k, v in o.items()}
    index, count = host["index"].numpy(), host["count"].numpy()
    assert count[0] == n and np.array_equal(index[:n], idx) and (index[n:cs.cap] == -1).all()
    assert (index[cs.cap:] == CANARY_I).all() and (count[1:] == CANARY_I).all()
    vr = host["vrows"][:rows * 4].view(rows, 4).double().numpy()
    assert np.isfinite(vr).all() and not vr[~cs.is_v].any()
    assert (host["vrows"][rows * 4:] == CANARY_F).all() and (host["stats"][8:] == CANARY_F).all()
    worst = {}

    def close(got, want, bound, what):
        err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
        bound = np.asarray(bound, dtype=np.float64) + 2.0 ** -116
        worst[what] = float((err / bound).max()) if err.size else 0.0
        assert (err <= bound).all(), f"{cs.name} {what}: worst error / bound = {worst[what]:.3g}"
    close(vr[idx, 0], ref.value[idx], tol["v"], "value")
    close(vr[idx, 1], ref.loss[idx], tol["l"], "loss")
    assert np.array_equal(vr[idx, 2], ref.clipped[idx].astype(np.float64))
    close(vr[idx, 3], ref.dv[idx], tol["dv"], "dv")
    stats = host["stats"][:8].double().numpy()
    assert np.isfinite(stats).all()
    close(stats, ref.stats, tol["stats"], "stats")
    if cs.clip is not None and n >= 8:
        assert 0 < ref.stats[2] < 1
    dw, db = host["dw"].double().numpy(), host["db"].double().numpy()
    assert (dw[dim:] == CANARY_F).all() and (db[1:] == CANARY_F).all() and np.isfinite(dw).all()
    close(dw[:dim], ref.dw * cs.inv_world, tol["dw"], "dw")
    close(db[0], ref.db * cs.inv_world, tol["db"], "db")
    dh, dh0 = host["dh"], cs.dh0
    other = torch.from_numpy(~cs.is_v)
    assert torch.equal(dh[other].view(torch.int16), dh0[other].view(torch.int16))            # bit-unchanged rows
    assert torch.equal(dh[:, dim:].view(torch.int16), dh0[:, dim:].view(torch.int16))        # … and padding columns
    if detach:
        assert torch.equal(dh.view(torch.int16), dh0.view(torch.int16))
    elif n:
        d0 = dh0[:, :dim].double().numpy()[idx]
        w = cs.w.double().numpy()
        add = (ref.dv[idx] * cs.inv_world)[:, None] * w[None, :]
        want = d0 + add
        bound = U * np.abs(want) + np.abs(w)[None, :] * tdv[:, None] + 3 * E * (np.abs(d0) + np.abs(add))
        close(dh[:, :dim].double().numpy()[idx], want, bound, "dh")
    return worst


@pytest.mark.parametrize("name", [s[0] for s in CASES])
def test_kernels_match_the_definition(dev, name):
    cs = get_case(name, dev)
    o = cs.outputs()
    cs.launch(o)
    torch.cuda.synchronize()
    worst = check_outputs(cs, o)
    print(f"{name}: n_v = {len(cs.idx)}; worst error / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    # a second launch on fresh buffers: the same bits everywhere
    o2 = cs.outputs()
    cs.launch(o2)
    for k in o:
        assert torch.equal(o[k].view(torch.int32 if o[k].element_size() == 4 else torch.int16),
                           o2[k].view(torch.int32 if o2[k].element_size() == 4 else torch.int16)), k
    # detached: dh is not touched, dw and db are the same bits
    o3 = cs.outputs()
    cs.launch(o3, detach=True)
    check_outputs(cs, o3, detach=True)
    assert torch.equal(o3["dw"], o["dw"]) and torch.equal(o3["db"], o["db"]) and torch.equal(o3["vrows"], o["vrows"])


def test_captured_graph_serves_new_labels(dev):
    """One capture; targets, returns and old_values rewritten in place between replays: the replay is the eager result of the
    new inputs, bit for bit (value rows, their number and the statistics are all found on the device)."""
    spec = next(s for s in CASES if s[0] == "d520-ld")
    a = Case(spec, dev)
    b = Case(spec[:7] + ("labelled",) + spec[8:], dev, seed=1)          # other labels, returns and old values; the same shapes
    # the two label sets own different rows of hn: both run over ONE hn without poison (this test compares replay with eager)
    a.hn = b.hn = torch.randn(a.rows, a.dim, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(dev)
    b.d_w, b.d_b = a.d_w, a.d_b
    tg, R, vo = a.d_tg.clone(), a.d_R.clone(), a.d_vo.clone()
    o = a.outputs()
    a.launch(o, tg=tg, R=R, vo=vo)                                      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.launch(o, tg=tg, R=R, vo=vo)
    for cs in (a, b, a):
        tg.copy_(cs.d_tg)
        R.copy_(cs.d_R)
        vo.copy_(cs.d_vo)
        o["dh"].copy_(cs.dh0)
        graph.replay()
        eager = cs.outputs()
        cs.launch(eager)
        torch.cuda.synchronize()
        assert eager["count"][0].item() == len(cs.idx) > 0
        for k in o:
            assert torch.equal(o[k].view(torch.int32 if o[k].element_size() == 4 else torch.int16),
                               eager[k].view(torch.int32 if eager[k].element_size() == 4 else torch.int16)), (cs.pattern, k)
    assert len(a.idx) != len(b.idx)


def test_argument_checks(dev):
    lib = _lib.load()
    rows, dim = 6, 16
    hn = torch.zeros(rows * 32 + 16, dtype=torch.bfloat16, device=dev)
    w, b = torch.zeros(32, dtype=torch.bfloat16, device=dev), torch.zeros(8, dtype=torch.bfloat16, device=dev)
    tg = torch.full((rows,), IGN, dtype=torch.int64, device=dev)
    f = torch.zeros(rows, device=dev)
    idx, cnt = torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    vr, st = torch.zeros(rows * 4 + 4, device=dev), torch.zeros(8, device=dev)
    dw, db = torch.zeros(32 + 4, device=dev), torch.zeros(1, device=dev)
    dh = torch.zeros(rows * 32 + 16, dtype=torch.bfloat16, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def fwd(hp=hn.data_ptr(), ld=16, dim_=dim, gr=3, level=1, clip=0.2, vo=f.data_ptr(), coef=0.5, vrp=vr.data_ptr()):
        return lib.bl_value_head_f32(hp, ld, rows, dim_, tg.data_ptr(), IGN, gr, level, w.data_ptr(), b.data_ptr(), f.data_ptr(), vo,
                                     coef, clip, None, idx.data_ptr(), cnt.data_ptr(), vrp, st.data_ptr(), s)

    def bwd(hp=hn.data_ptr(), ld=16, dim_=dim, gr=3, level=1, inv_world=1.0, dwp=dw.data_ptr(), dhp=dh.data_ptr(), lddh=16):
        return lib.bl_value_head_backward_f32(hp, ld, rows, dim_, gr, level, w.data_ptr(), vr.data_ptr(), idx.data_ptr(),
                                              cnt.data_ptr(), inv_world, dwp, db.data_ptr(), dhp, lddh, s)
    assert fwd() == _lib.BL_OK and fwd(level=0, gr=0) == _lib.BL_OK and fwd(clip=-1.0, vo=None) == _lib.BL_OK
    assert fwd(dim_=12) == _lib.BL_E_SHAPE and fwd(ld=20) == _lib.BL_E_SHAPE and fwd(ld=8) == _lib.BL_E_SHAPE
    assert fwd(gr=4) == _lib.BL_E_SHAPE and fwd(gr=0) == _lib.BL_E_SHAPE and fwd(level=2) == _lib.BL_E_SHAPE
    assert fwd(hp=hn.data_ptr() + 2) == _lib.BL_E_ALIGN and fwd(vrp=vr.data_ptr() + 4) == _lib.BL_E_ALIGN
    assert fwd(hp=None) == _lib.BL_E_ARG and fwd(vo=None) == _lib.BL_E_ARG and fwd(coef=-1.0) == _lib.BL_E_ARG
    assert bwd() == _lib.BL_OK and bwd(dhp=None, lddh=0) == _lib.BL_OK
    assert bwd(dim_=12) == _lib.BL_E_SHAPE and bwd(lddh=20) == _lib.BL_E_SHAPE and bwd(lddh=8) == _lib.BL_E_SHAPE and bwd(gr=4) == _lib.BL_E_SHAPE
    assert bwd(dwp=dw.data_ptr() + 4) == _lib.BL_E_ALIGN and bwd(dhp=dh.data_ptr() + 2) == _lib.BL_E_ALIGN
    assert bwd(dwp=None) == _lib.BL_E_ARG and bwd(inv_world=0.0) == _lib.BL_E_ARG
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        T.value_index_slots(rows, "action", 4)
