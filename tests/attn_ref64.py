"""fp64 reference for the attention kernels (attention.hip, attention_bwd.hip) and a per-element error bound.

A helper module, not a test module: tests import it as `from attn_ref64 import ...`. It is written from the definition of
attention with fp64 torch matmul / exp / sum and deliberately shares nothing with oracle/restate.py, which restates the
kernels' own rounding choices and so cannot catch a kernel that shares one of them by mistake.

Layout: every tensor is [B, H, rows, cols]; q / k / v / o / dO are the bf16 tensors the kernel gets (any float dtype,
converted to fp64 here). Work is done one batch element and a few heads at a time, so the largest case never holds a
B·H × S² fp64 tensor.

Error model and the constants C_O, C_DQ, C_DK, C_DV
----------------------------------------------------
Let u = 2^-8, the unit roundoff of bf16 (8-bit significand, round to nearest even), and e = 2^-24 that of fp32. Each
kernel output element is compared as

    |got - ref| <= c·u·mag + u·|ref| + FLOOR

where `ref` is the fp64 value and `mag` the fp64 "magnitude companion": the same sum with every term replaced by its
absolute value. The u·|ref| term is the final rounding of the output to bf16 (relative error <= u of the value
rounded, which is ref plus an error of order u·mag: the cross term is O(u²) and is absorbed below). The c·u·mag term
bounds everything before that rounding, term by term:

* Forward O (whole-sequence, chunked and decode kernels; attention.hip:14). o_i = Σ_j bf16(ê_ij)·v_j / l̂_i with
  ê_ij = exp2(s'_ij − m) in fp32 and l̂_i the fp32 sum of the UNROUNDED ê (the chunked kernel rescales ê and l̂ by the
  same fp32 alpha, the decode kernel rounds exactly like the others).
  - P rounded to bf16 before the PV product: |bf16(ê) − ê| <= u·ê, so the sum moves by at most u·Σ_j p_ij|v_j| = u·m_o.
    This is the dominant term: 1.
  - fp32 scores: a 128-term fp32 dot of exact bf16 products plus the multiply by fp32(scale·log2e) perturbs s'_ij by
    at most ~130·e·|s'_ij| <= 130·e·64 < 2^-10.9 in the exponent for |s'| <= 64 (the peaked test inputs stay below 40),
    i.e. <= 2^-11.4 ≈ 0.09u relative in each ê; ê appears in numerator and denominator: 0.18u·m_o.
  - v_exp_f32 (1 ulp), fp32 accumulation of <= 2048 PV terms and of l̂ (n·e <= 2^-13 = 0.03u each), the online
    rescale (one fp32 multiply per 64-key chunk, <= 32·e) and 1/l̂: together < 0.07u·m_o.
  Sum 1 + 0.18 + 0.07 = 1.25 → C_O = 1.25.
* dV = Pᵀ·dO (attention_bwd.hip:15): P = exp2(s'·scale·log2e − lse) in fp32 from the forward's fp32 lse, rounded to
  bf16 for the MFMA. Rounding P: 1·u·m_dv. P's fp32 error: the score term (0.09u) plus lse's own error (the l̂ sum
  0.03u, v_log_f32 and the fp32 lse value < 2^-17 absolute: 0.01u) = 0.13u. fp32 accumulation of <= 2048 terms: 0.03u.
  Sum 1.16 → C_DV = 1.25.
* dQ = scale·dS·K and dK = scale·dSᵀ·Q with dS = P∘(dP − δ) rounded to bf16 before its MFMA (attention_bwd.hip:15).
  Rounding dS: u·P|dP − δ| <= u·P(|dP| + |δ|), summed against |k_j| (|q_i|): 1·u·m_dq (m_dk). P's fp32 error as for
  dV: 0.13u. dP and δ are 128-term fp32 dots of exact bf16 products: their error is ~e·√128·Σ|dO||v|, far below
  u·|dP| except where dP itself cancels to ~2^-14 of its terms; allow 0.25u for that tail. fp32 accumulation of
  <= 2048 terms and the fp32 multiply by scale: 0.04u. Sum 1.42 → C_DQ = C_DK = 1.5.

FLOOR = 2^-110 is the fp32 denormal level: an exp2 result below 2^-126 may be flushed to zero, which moves a sum of
<= 2048 terms with operands below 2^4 by at most 2^11·2^-126·2^4 = 2^-111.

lse (base 2, what the kernels store) is checked separately: |got − ref| <= LSE_REL·(1 + |ref| + mag_s), mag_s =
scale·log2e·Σ_j p_ij Σ_d |q_id k_jd| (the p-weighted absolute score, which the fp32 score error scales with).
LSE_REL = 2^-18 is a few fp32 ulps of |ref| (ulp(32) = 2^-18), covers the fp32 score dot (~√128·e·mag_s ≈ 2^-20.5·mag_s),
the fp32 row sum (<= 80 sequential adds per lane in the whole-sequence kernel: 2^-17.7 relative in l̂ worst case, 2^-20
typical, → /ln2 in log2) and v_log_f32's absolute error (~2^-22).

These constants are final: a GPU run that exceeds one is a finding about the kernel, not a reason to widen it.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

U = 2.0 ** -8
FLOOR = 2.0 ** -110
C_O = 1.25
C_DV = 1.25
C_DQ = 1.5
C_DK = 1.5
LSE_REL = 2.0 ** -18
LOG2E = 1.0 / math.log(2.0)

RATIOS: Dict[str, float] = {}      # label → largest err / bound seen (printed by every comparator call)

_CHUNK_ELEMS = 1 << 22              # score elements per fp64 slice (H heads × Sq × Skv) ≈ 32 MiB per tensor


def visible(Sq: int, Skv: int, causal: bool, mask_row: Optional[torch.Tensor]) -> torch.Tensor:
    """[Sq, Skv] bool: key j is visible to query i iff mask_j = 1 and (not causal or j <= i + Skv − Sq)."""
    vis = torch.ones(Sq, Skv, dtype=torch.bool)
    if causal:
        i = torch.arange(Sq).view(-1, 1) + (Skv - Sq)
        vis &= torch.arange(Skv).view(1, -1) <= i
    if mask_row is not None:
        vis &= mask_row.to(torch.bool).cpu().view(1, Skv)
    return vis


def _slices(B: int, H: int, Sq: int, Skv: int):
    hs = max(1, min(H, _CHUNK_ELEMS // max(1, Sq * Skv)))
    for b in range(B):
        for h0 in range(0, H, hs):
            yield b, slice(h0, min(H, h0 + hs))


def _probs(q, k, scale, vis):
    """fp64 [h, Sq, Skv] softmax over the visible keys (0 in empty rows), and the base-2 lse (+inf in empty rows)."""
    s = scale * (q @ k.transpose(-1, -2))
    s = s.masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / torch.where(l > 0, l, torch.ones_like(l))
    lse2 = torch.where(l > 0, (m + torch.log(l)) * LOG2E, torch.full_like(l, float("inf")))
    return p, lse2.squeeze(-1)


def forward(q, k, v, scale: float, causal: bool, key_mask: Optional[torch.Tensor] = None):
    """o, lse2, m_o, mag_s (all fp64) of attention over [B, H, S, hd] inputs; key_mask [B, Skv] (1 = attend)."""
    q, k, v = (t.detach().cpu().double() for t in (q, k, v))
    B, H, Sq, hd = q.shape
    Skv = k.shape[2]
    o = torch.zeros(B, H, Sq, v.shape[-1], dtype=torch.float64)
    m_o = torch.zeros_like(o)
    lse2 = torch.zeros(B, H, Sq, dtype=torch.float64)
    mag_s = torch.zeros_like(lse2)
    for b, hs in _slices(B, H, Sq, Skv):
        vis = visible(Sq, Skv, causal, None if key_mask is None else key_mask[b])
        qb, kb, vb = q[b, hs], k[b, hs], v[b, hs]
        p, lse2[b, hs] = _probs(qb, kb, scale, vis)
        o[b, hs] = p @ vb
        m_o[b, hs] = p @ vb.abs()
        mag_s[b, hs] = (scale * LOG2E) * (p * (qb.abs() @ kb.abs().transpose(-1, -2))).sum(-1)
    return dict(o=o, lse2=lse2, m_o=m_o, mag_s=mag_s)


def backward(q, k, v, o, do, scale: float, causal: bool, key_mask: Optional[torch.Tensor] = None):
    """dq, dk, dv, delta and the magnitude companions m_dq, m_dk, m_dv (all fp64), given dO and the O the kernel got."""
    q, k, v, o, do = (t.detach().cpu().double() for t in (q, k, v, o, do))
    B, H, Sq, hd = q.shape
    Skv = k.shape[2]
    dq, m_dq = torch.zeros_like(q), torch.zeros_like(q)
    dk, m_dk = torch.zeros_like(k), torch.zeros_like(k)
    dv, m_dv = torch.zeros_like(v), torch.zeros_like(v)
    delta = torch.zeros(B, H, Sq, dtype=torch.float64)
    for b, hs in _slices(B, H, Sq, Skv):
        vis = visible(Sq, Skv, causal, None if key_mask is None else key_mask[b])
        qb, kb, vb, ob, gb = q[b, hs], k[b, hs], v[b, hs], o[b, hs], do[b, hs]
        p, _ = _probs(qb, kb, scale, vis)
        dp = gb @ vb.transpose(-1, -2)
        dl = (gb * ob).sum(-1, keepdim=True)
        ds = p * (dp - dl)
        dsm = p * (dp.abs() + dl.abs())
        delta[b, hs] = dl.squeeze(-1)
        dq[b, hs] = scale * (ds @ kb)
        dk[b, hs] = scale * (ds.transpose(-1, -2) @ qb)
        dv[b, hs] = p.transpose(-1, -2) @ gb
        m_dq[b, hs] = scale * (dsm @ kb.abs())
        m_dk[b, hs] = scale * (dsm.transpose(-1, -2) @ qb.abs())
        m_dv[b, hs] = p.transpose(-1, -2) @ gb.abs()
    return dict(dq=dq, dk=dk, dv=dv, delta=delta, m_dq=m_dq, m_dk=m_dk, m_dv=m_dv)


def _log(what: str, ratio: float, n: int) -> None:
    RATIOS[what] = max(RATIOS.get(what, 0.0), ratio)
    print(f"attn_ref64: {what}: max err/bound {ratio:.4f} over {n} elements")


def _worst(ratio, shape):
    idx = int(torch.argmax(ratio).item())
    coords = []
    for dim in reversed(shape):
        coords.append(idx % dim)
        idx //= dim
    return tuple(reversed(coords))


def assert_attn_close(got, ref, mag, c: float, what: str, rows: Optional[torch.Tensor] = None) -> float:
    """Per-element check |got − ref| <= c·u·mag + u·|ref| + FLOOR over [B, H, S, D] tensors. `rows` ([B, S] bool) selects
    the rows that are specified (padded query rows are not); others are ignored. Returns the largest err / bound."""
    got = got.detach().cpu().double()
    ref, mag = ref.double(), mag.double()
    assert got.shape == ref.shape == mag.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    bound = c * U * mag + U * ref.abs() + FLOOR
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    if rows is not None:
        sel = rows.to(torch.bool).cpu().view(rows.shape[0], 1, rows.shape[1], 1).expand_as(err)
        err = torch.where(sel, err, torch.zeros_like(err))
        n = int(sel.sum().item())
    else:
        n = err.numel()
    ratio_t = err / bound
    ratio = float(ratio_t.max().item()) if err.numel() else 0.0
    _log(what, ratio, n)
    bad = ratio_t > 1.0
    if bool(bad.any()):
        b, h, r, col = _worst(ratio_t, tuple(err.shape))
        raise AssertionError(
            f"{what}: {int(bad.sum().item())} of {n} elements out of bound; worst (batch {b}, head {h}, row {r}, col {col}): "
            f"got {got[b, h, r, col].item():.6g}, ref {ref[b, h, r, col].item():.6g}, mag {mag[b, h, r, col].item():.4g}, "
            f"err/bound {ratio:.3g} (c = {c})")
    return ratio


def assert_lse_close(got, ref, mag_s, what: str, rows: Optional[torch.Tensor] = None) -> float:
    """Base-2 lse [B, H, S]: |got − ref| <= LSE_REL·(1 + |ref| + mag_s); +inf (empty rows) must match exactly."""
    got = got.detach().cpu().double()
    ref, mag_s = ref.double(), mag_s.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    sel = torch.ones_like(ref, dtype=torch.bool)
    if rows is not None:
        sel = rows.to(torch.bool).cpu().view(rows.shape[0], 1, rows.shape[1]).expand_as(ref)
    inf_ref = torch.isinf(ref)
    mism = sel & ((inf_ref != torch.isinf(got)) | (inf_ref & (got != ref)))
    assert not bool(mism.any()), f"{what}: {int(mism.sum())} rows disagree on being empty (lse = +inf)"
    fin = sel & ~inf_ref
    bound = LSE_REL * (1.0 + ref.abs() + mag_s)
    err = torch.where(fin, (got - ref).abs(), torch.zeros_like(ref))
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio_t = torch.where(fin, err / torch.where(fin, bound, torch.ones_like(bound)), torch.zeros_like(err))
    ratio = float(ratio_t.max().item()) if ratio_t.numel() else 0.0
    _log(what, ratio, int(fin.sum().item()))
    bad = ratio_t > 1.0
    if bool(bad.any()):
        b, h, r = _worst(ratio_t, tuple(ref.shape))
        raise AssertionError(f"{what}: {int(bad.sum().item())} lse values out of bound; worst (batch {b}, head {h}, row {r}): "
                             f"got {got[b, h, r].item():.9g}, ref {ref[b, h, r].item():.9g}, err/bound {ratio:.3g}")
    return ratio


def peaked_q(q, k, causal: bool, key_mask: Optional[torch.Tensor] = None, gain: float = 1.5):
    """Inputs that stress the online rescale: q scaled ×4, and each row's largest score moved to its LAST visible key
    (q_i += gain·k_last(i)), which sits in the row's last 64-key chunk — so the running max of the chunked forward moves
    in the last chunk, and P of that key is near 1, where P's bf16 rounding matters. Returns bf16-representable fp32."""
    q, k = q.float(), k.float()
    B, H, Sq, _ = q.shape
    Skv = k.shape[2]
    out = 4.0 * q
    for b in range(B):
        vis = visible(Sq, Skv, causal, None if key_mask is None else key_mask[b])
        last = torch.where(vis.any(1), Skv - 1 - vis.flip(1).int().argmax(1), torch.full((Sq,), -1))
        rows = last >= 0
        out[b][:, rows] += gain * k[b][:, last[rows]]
    return out.to(torch.bfloat16).float()
