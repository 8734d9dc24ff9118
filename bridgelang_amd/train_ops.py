"""Torch-tensor front end for the training-step entry points of the C ABI (train.hip, attention_bwd.hip).
Same convention as ops.py: every builder returns a prepared `Op` and (run=True) enqueues it on the current stream."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .ops import Op, _attn_desc, _bf16, _dev, _f32, _op, _rows


def cross_entropy_backward(logits, targets, mean_and_count, dlogits, ignore_index: int = -100, run: bool = True) -> Op:
    rows, n = logits.shape
    return _op("bl_cross_entropy_backward_f32",
               (_f32(logits, "logits").data_ptr(), _rows(logits, "logits"), rows, n, targets.data_ptr(), ignore_index,
                mean_and_count.data_ptr(), _bf16(dlogits, "dlogits").data_ptr(), _rows(dlogits, "dlogits")),
               (logits, targets, mean_and_count, dlogits), run, nbytes=6.0 * rows * n)


def _policy_rows(logits, targets, row_stats, stats, what: str):
    rows, n = logits.shape
    if targets.dtype != torch.int64 or targets.numel() != rows:
        raise TypeError(f"{what}: targets int64 [{rows}]")
    if tuple(_f32(row_stats, "row_stats").shape) != (rows, 8) or not row_stats.is_contiguous() or _f32(stats, "stats").numel() != 8:
        raise ValueError(f"{what}: row_stats fp32 [{rows}, 8] contiguous and stats fp32 [8]")
    return rows, n


def policy_loss(logits, targets, advantages, old_logprob, ref_logprob, row_stats, stats, cfg, ignore_index: int = -100,
                run: bool = True, group_rows: Optional[int] = None, group_stats: Optional[torch.Tensor] = None,
                behaviour_logprob: Optional[torch.Tensor] = None, is_rows: Optional[torch.Tensor] = None,
                is_stats: Optional[torch.Tensor] = None) -> Op:
    """Clipped-surrogate policy-gradient loss over fp32 logits [rows, n] (training/policy_loss.py is the definition; `cfg` a
    PolicyLossConfig). advantages / old_logprob / ref_logprob (None: no KL term) fp32 [rows]; row_stats fp32 [rows, 8] and
    stats fp32 [8] receive policy_loss.ROW_STAT_NAMES / STAT_NAMES. With cfg.token_range the policy is over that token
    range alone (bl_policy_loss_range_f32). With cfg.ratio_level == "action" the ratio is per sequence of `group_rows`
    consecutive rows (bl_policy_loss_grouped_f32) and group_stats fp32 [rows / group_rows, 4] receives
    policy_loss.GROUP_STAT_NAMES; at token level both are ignored. With cfg.rollout_is_cap set it is the rollout correction
    (bl_policy_loss_is_f32, either level): behaviour_logprob fp32 [rows] is what the sampler reported, old_logprob the
    proximal policy's or None (self-proximal: this forward's own logp), and is_rows fp32 [rows, 2] / is_stats fp32 [8]
    receive (λ, w) per row / policy_loss.IS_STAT_NAMES; without it those three must be None and old_logprob given."""
    rows, n = _policy_rows(logits, targets, row_stats, stats, "policy_loss")
    for t, what in ((advantages, "advantages"), (old_logprob, "old_logprob"), (ref_logprob, "ref_logprob"),
                    (behaviour_logprob, "behaviour_logprob")):
        if t is not None and (_f32(t, what).numel() != rows or not t.is_contiguous()):
            raise ValueError(f"policy_loss: {what} fp32 [{rows}] contiguous")
    rng = getattr(cfg, "token_range", None)
    if getattr(cfg, "rollout_is_cap", None) is not None:
        return _policy_loss_is(logits, targets, advantages, old_logprob, ref_logprob, row_stats, stats, cfg, ignore_index, run,
                               group_rows, group_stats, behaviour_logprob, is_rows, is_stats, rows, n)
    if behaviour_logprob is not None or is_rows is not None or is_stats is not None:
        raise ValueError("policy_loss: behaviour_logprob, is_rows and is_stats go with cfg.rollout_is_cap")
    if old_logprob is None:
        raise ValueError("policy_loss: old_logprob=None (self-proximal) needs cfg.rollout_is_cap")
    head = (_f32(logits, "logits").data_ptr(), _rows(logits, "logits"), rows, n, targets.data_ptr(), ignore_index,
            advantages.data_ptr(), old_logprob.data_ptr(), ref_logprob.data_ptr() if ref_logprob is not None else None,
            float(cfg.temperature), float(cfg.clip_low), float(cfg.clip_high), float(cfg.entropy_coef), float(cfg.kl_coef),
            row_stats.data_ptr(), stats.data_ptr())
    keep = (logits, targets, advantages, old_logprob, ref_logprob, row_stats, stats)
    nbytes = 8.0 * rows * (n if rng is None else rng[1])
    if getattr(cfg, "ratio_level", "token") == "action":
        g_rows, norm, group_stats = _group_args(cfg, rows, group_rows, group_stats)
        first, count = (0, n) if rng is None else (int(rng[0]), int(rng[1]))
        return _op("bl_policy_loss_grouped_f32", head + (first, count, g_rows, norm, group_stats.data_ptr()),
                   keep + (group_stats,), run, nbytes=nbytes + 64.0 * rows)
    return _op("bl_policy_loss_f32" if rng is None else "bl_policy_loss_range_f32",
               head + (() if rng is None else (int(rng[0]), int(rng[1]))), keep, run, nbytes=nbytes)


def _group_args(cfg, rows: int, group_rows, group_stats):
    """(group_rows, ratio_norm, group_stats) of an action-level call, checked."""
    if group_rows is None or int(group_rows) != group_rows or group_rows < 1 or rows % int(group_rows):
        raise ValueError(f"policy_loss: ratio_level='action' needs group_rows >= 1 dividing the {rows} rows, got {group_rows!r}")
    groups = rows // int(group_rows)
    if group_stats is None:
        raise ValueError(f"policy_loss: ratio_level='action' needs group_stats fp32 [{groups}, 4]")
    if tuple(_f32(group_stats, "group_stats").shape) != (groups, 4) or not group_stats.is_contiguous():
        raise ValueError(f"policy_loss: group_stats fp32 [{groups}, 4] contiguous")
    return int(group_rows), 1 if cfg.ratio_norm == "mean" else 0, group_stats


def _policy_loss_is(logits, targets, advantages, old_logprob, ref_logprob, row_stats, stats, cfg, ignore_index, run, group_rows,
                    group_stats, behaviour_logprob, is_rows, is_stats, rows: int, n: int) -> Op:
    """`policy_loss` with the rollout correction: one symbol for both levels and both proximal modes."""
    if behaviour_logprob is None or is_rows is None or is_stats is None:
        raise ValueError(f"policy_loss: cfg.rollout_is_cap needs behaviour_logprob fp32 [{rows}], is_rows fp32 [{rows}, 2] and is_stats fp32 [8]")
    if tuple(_f32(is_rows, "is_rows").shape) != (rows, 2) or not is_rows.is_contiguous() or _f32(is_stats, "is_stats").numel() != 8:
        raise ValueError(f"policy_loss: is_rows fp32 [{rows}, 2] contiguous and is_stats fp32 [8]")
    rng = cfg.token_range
    first, count = (0, n) if rng is None else (int(rng[0]), int(rng[1]))
    if cfg.ratio_level == "action":
        g_rows, norm, gs = _group_args(cfg, rows, group_rows, group_stats)
    else:
        g_rows, norm, gs = 0, 0, None
    low, high = cfg.rollout_is_mask or (0.0, float("inf"))
    return _op("bl_policy_loss_is_f32",
               (_f32(logits, "logits").data_ptr(), _rows(logits, "logits"), rows, n, targets.data_ptr(), ignore_index,
                advantages.data_ptr(), old_logprob.data_ptr() if old_logprob is not None else None, behaviour_logprob.data_ptr(),
                ref_logprob.data_ptr() if ref_logprob is not None else None,
                float(cfg.temperature), float(cfg.clip_low), float(cfg.clip_high), float(cfg.entropy_coef), float(cfg.kl_coef),
                row_stats.data_ptr(), stats.data_ptr(), first, count, g_rows, norm, gs.data_ptr() if gs is not None else None,
                float(cfg.rollout_is_cap), float(low), float(high), is_rows.data_ptr(), is_stats.data_ptr()),
               (logits, targets, advantages, old_logprob, behaviour_logprob, ref_logprob, row_stats, stats, gs, is_rows, is_stats),
               run, nbytes=8.0 * rows * count + 80.0 * rows)


def policy_loss_backward(logits, targets, row_stats, stats, dlogits, cfg, ignore_index: int = -100, run: bool = True) -> Op:
    """bf16 dlogits of `policy_loss` from the logits and the row statistics it saved (stats[1] = n_valid); with
    cfg.token_range, zeros outside the range (bl_policy_loss_backward_range_f32)."""
    rows, n = _policy_rows(logits, targets, row_stats, stats, "policy_loss_backward")
    rng = getattr(cfg, "token_range", None)
    return _op("bl_policy_loss_backward_f32" if rng is None else "bl_policy_loss_backward_range_f32",
               (_f32(logits, "logits").data_ptr(), _rows(logits, "logits"), rows, n, targets.data_ptr(), ignore_index,
                row_stats.data_ptr(), stats.data_ptr(), float(cfg.temperature), float(cfg.entropy_coef),
                _bf16(dlogits, "dlogits").data_ptr(), _rows(dlogits, "dlogits")) + (() if rng is None else (int(rng[0]), int(rng[1]))),
               (logits, targets, row_stats, stats, dlogits), run, nbytes=(2.0 * n + 4.0 * (n if rng is None else rng[1])) * rows)


def preference_loss(logits, targets, pair, ref_logprob, row_stats, stats, pair_stats, seq_stats, cfg, group_rows: int,
                    n_pairs: Optional[torch.Tensor] = None, ignore_index: int = -100, run: bool = True) -> Op:
    """Preference-pair loss (DPO family) over fp32 logits [rows, n] (training/preference_loss.py is the definition; `cfg` a
    PreferenceLossConfig). pair int32 [rows / group_rows]: +k / −k / 0 per sequence of `group_rows` rows; ref_logprob fp32
    [rows] (None: reference-free). row_stats fp32 [rows, 8], stats fp32 [8], pair_stats fp32 [cap, 4] and seq_stats fp32
    [rows / group_rows, 4] receive policy_loss.ROW_STAT_NAMES and preference_loss.PREF_STAT_NAMES / PAIR_STAT_NAMES /
    SEQ_STAT_NAMES. The number of pairs P is `cap`, or the int32 device scalar `n_pairs` (read by the kernels, so a captured
    op serves any P <= cap). `policy_loss_backward` with cfg.backward_config() is the gradient."""
    from .training.preference_loss import KINDS, SEQ_NORMS
    rows, n = _policy_rows(logits, targets, row_stats, stats, "preference_loss")
    if int(group_rows) != group_rows or group_rows < 1 or rows % int(group_rows):
        raise ValueError(f"preference_loss: needs group_rows >= 1 dividing the {rows} rows, got {group_rows!r}")
    groups = rows // int(group_rows)
    _dev(pair, torch.int32, groups, "preference_loss: pair")
    if (ref_logprob is None) != bool(cfg.reference_free):
        raise ValueError("preference_loss: ref_logprob is given unless cfg.reference_free")
    if ref_logprob is not None and (_f32(ref_logprob, "ref_logprob").numel() != rows or not ref_logprob.is_contiguous()):
        raise ValueError(f"preference_loss: ref_logprob fp32 [{rows}] contiguous")
    if _f32(pair_stats, "pair_stats").dim() != 2 or pair_stats.shape[0] < 1 or pair_stats.shape[1] != 4 or not pair_stats.is_contiguous():
        raise ValueError("preference_loss: pair_stats fp32 [cap >= 1, 4] contiguous")
    if tuple(_f32(seq_stats, "seq_stats").shape) != (groups, 4) or not seq_stats.is_contiguous():
        raise ValueError(f"preference_loss: seq_stats fp32 [{groups}, 4] contiguous")
    if n_pairs is not None:
        _dev(n_pairs, torch.int32, 1, "preference_loss: n_pairs")
    rng = cfg.token_range
    first, count = (0, n) if rng is None else (int(rng[0]), int(rng[1]))
    return _op("bl_preference_loss_f32",
               (_f32(logits, "logits").data_ptr(), _rows(logits, "logits"), rows, n, targets.data_ptr(), ignore_index,
                pair.data_ptr(), ref_logprob.data_ptr() if ref_logprob is not None else None, int(pair_stats.shape[0]),
                n_pairs.data_ptr() if n_pairs is not None else None, int(group_rows), KINDS.index(cfg.kind),
                SEQ_NORMS.index(cfg.seq_norm), float(cfg.beta), float(cfg.label_smoothing), float(cfg.margin), float(cfg.sft_coef),
                float(cfg.temperature), row_stats.data_ptr(), stats.data_ptr(), pair_stats.data_ptr(), seq_stats.data_ptr(),
                first, count),
               (logits, targets, pair, ref_logprob, row_stats, stats, pair_stats, seq_stats, n_pairs), run,
               nbytes=8.0 * rows * count + 64.0 * rows)


def _distill_args(logits, targets, teacher, row_stats, stats, cfg, ignore_index: int, what: str):
    """The arguments both distillation entry points share up to the teacher's leading dimension, checked → (rows, n, count,
    head tuple, tail tuple)."""
    from .training.distill_loss import KINDS
    rows, n = _policy_rows(logits, targets, row_stats, stats, what)
    rng = getattr(cfg, "token_range", None)
    first, count = (0, n) if rng is None else (int(rng[0]), int(rng[1]))
    if _f32(teacher, "teacher").dim() != 2 or tuple(teacher.shape) != (rows, count) or teacher.stride(1) != 1:
        raise ValueError(f"{what}: teacher fp32 [{rows}, {count}] (one row per logits row, over the range) with unit column stride")
    head = (_f32(logits, "logits").data_ptr(), _rows(logits, "logits"), rows, n, targets.data_ptr(), ignore_index,
            teacher.data_ptr(), _rows(teacher, "teacher"))
    tail = (KINDS.index(cfg.kind), float(cfg.beta), float(cfg.sft_coef), float(cfg.temperature))
    return rows, n, first, count, head, tail


def distill_loss(logits, targets, teacher, row_stats, stats, cfg, ignore_index: int = -100, run: bool = True) -> Op:
    """Distribution-matching loss over fp32 logits [rows, n] (training/distill_loss.py is the definition; `cfg` a
    DistillLossConfig): teacher fp32 [rows, count] in row layout over cfg.token_range (count = n without one), read on valid
    rows only; row_stats fp32 [rows, 8] and stats fp32 [8] receive distill_loss.DISTILL_ROW_STAT_NAMES / DISTILL_STAT_NAMES."""
    rows, n, first, count, head, tail = _distill_args(logits, targets, teacher, row_stats, stats, cfg, ignore_index, "distill_loss")
    return _op("bl_distill_loss_f32", head + tail + (row_stats.data_ptr(), stats.data_ptr(), first, count),
               (logits, targets, teacher, row_stats, stats), run, nbytes=16.0 * rows * count + 64.0 * rows)


def distill_loss_backward(logits, targets, teacher, row_stats, stats, dlogits, cfg, ignore_index: int = -100, run: bool = True) -> Op:
    """bf16 dlogits of `distill_loss` from the logits, the teacher and the row statistics it saved (stats[1] = n_valid); zeros
    outside cfg.token_range and on ignored rows."""
    rows, n, first, count, head, tail = _distill_args(logits, targets, teacher, row_stats, stats, cfg, ignore_index,
                                                      "distill_loss_backward")
    if tuple(_bf16(dlogits, "dlogits").shape) != (rows, n):
        raise ValueError(f"distill_loss_backward: dlogits bf16 [{rows}, {n}]")
    return _op("bl_distill_loss_backward_f32",
               head + (row_stats.data_ptr(), stats.data_ptr()) + tail + (dlogits.data_ptr(), _rows(dlogits, "dlogits"), first, count),
               (logits, targets, teacher, row_stats, stats, dlogits), run, nbytes=(2.0 * n + 8.0 * count) * rows)


def value_index_slots(rows: int, level: str, group_rows: Optional[int]) -> int:
    """Capacity of the value-row list: one slot per row at token level, one per sequence of `group_rows` rows at action level."""
    if level == "token":
        return rows
    if level != "action":
        raise ValueError(f"value head: level is 'action' or 'token', got {level!r}")
    if group_rows is None or int(group_rows) != group_rows or group_rows < 1 or rows % int(group_rows):
        raise ValueError(f"value head: level='action' needs group_rows >= 1 dividing the {rows} rows, got {group_rows!r}")
    return rows // int(group_rows)


def _value_common(hn, w, value_rows, index, count, cfg, group_rows, what: str):
    rows, dim = hn.shape
    cap = value_index_slots(rows, cfg.level, group_rows)
    if _bf16(w, "w").numel() != dim or not w.is_contiguous():
        raise ValueError(f"{what}: w bf16 [{dim}] contiguous")
    if tuple(_f32(value_rows, "value_rows").shape) != (rows, 4) or not value_rows.is_contiguous():
        raise ValueError(f"{what}: value_rows fp32 [{rows}, 4] contiguous")
    _dev(index, torch.int32, cap, f"{what}: index")
    _dev(count, torch.int32, 1, f"{what}: count")
    return rows, dim, cap, (int(group_rows) if cfg.level == "action" else 0), (1 if cfg.level == "action" else 0)


def value_head(hn, targets, w, b, returns, old_values, cfg, index, count, value_rows, stats, policy_stats=None,
               group_rows: Optional[int] = None, ignore_index: int = -100, run: bool = True) -> Op:
    """The value head and PPO's clipped value loss over the bf16 final-norm rows hn [rows, dim] (training/value_loss.py is
    the definition; `cfg` a ValueLossConfig): w bf16 [dim], b bf16 [1], returns / old_values fp32 [rows] (old_values None
    only with cfg.clip None). The value rows are found on the device from `targets`; index int32 [value_index_slots(...)]
    and count int32 [1] receive their ascending list, value_rows fp32 [rows, 4] and stats fp32 [8] receive
    value_loss.VALUE_ROW_NAMES / VALUE_STAT_NAMES. `policy_stats` (the policy loss's stats, or None) supplies the loss that
    `total` adds to."""
    rows, dim, cap, gr, level = _value_common(hn, w, value_rows, index, count, cfg, group_rows, "value_head")
    if targets.dtype != torch.int64 or targets.numel() != rows:
        raise TypeError(f"value_head: targets int64 [{rows}]")
    if _bf16(b, "b").numel() != 1 or _f32(stats, "stats").numel() != 8:
        raise ValueError("value_head: b bf16 [1] and stats fp32 [8]")
    if (old_values is None) != (cfg.clip is None):
        raise ValueError("value_head: old_values is given unless cfg.clip is None")
    for t, what in ((returns, "returns"), (old_values, "old_values")):
        if t is not None and (_f32(t, what).numel() != rows or not t.is_contiguous()):
            raise ValueError(f"value_head: {what} fp32 [{rows}] contiguous")
    return _op("bl_value_head_f32",
               (_bf16(hn, "hn").data_ptr(), _rows(hn, "hn"), rows, dim, targets.data_ptr(), ignore_index, gr, level, w.data_ptr(),
                b.data_ptr(), returns.data_ptr(), old_values.data_ptr() if old_values is not None else None, float(cfg.coef),
                float(cfg.clip) if cfg.clip is not None else -1.0, _f32(policy_stats, "policy_stats").data_ptr() if policy_stats is not None else None,
                index.data_ptr(), count.data_ptr(), value_rows.data_ptr(), stats.data_ptr()),
               (hn, targets, w, b, returns, old_values, policy_stats, index, count, value_rows, stats), run,
               nbytes=8.0 * rows + 2.0 * cap * dim)


def value_head_backward(hn, w, value_rows, index, count, dw, db, dh, cfg, group_rows: Optional[int] = None,
                        inv_world: float = 1.0, run: bool = True) -> Op:
    """Gradient of `value_head` from what it left: dw fp32 [dim] and db fp32 [1] are overwritten, dv_r·w is added into the
    value rows of the bf16 dh [rows, dim] — unless dh is None (cfg.detach). `inv_world` scales dv (the data-parallel mean)."""
    rows, dim, cap, gr, level = _value_common(hn, w, value_rows, index, count, cfg, group_rows, "value_head_backward")
    if _f32(dw, "dw").numel() != dim or not dw.is_contiguous() or _f32(db, "db").numel() != 1:
        raise ValueError(f"value_head_backward: dw fp32 [{dim}] contiguous and db fp32 [1]")
    if dh is not None and tuple(_bf16(dh, "dh").shape) != (rows, dim):
        raise ValueError(f"value_head_backward: dh bf16 [{rows}, {dim}]")
    return _op("bl_value_head_backward_f32",
               (_bf16(hn, "hn").data_ptr(), _rows(hn, "hn"), rows, dim, gr, level, w.data_ptr(), value_rows.data_ptr(),
                index.data_ptr(), count.data_ptr(), float(inv_world), dw.data_ptr(), db.data_ptr(),
                dh.data_ptr() if dh is not None else None, _rows(dh, "dh") if dh is not None else 0),
               (hn, w, value_rows, index, count, dw, db, dh), run, nbytes=(2.0 if dh is None else 6.0) * cap * dim)


def value_predict(x, norm_w, eps: float, w, b, out, run: bool = True) -> Op:
    """V(s) of the residual rows x [rows, dim] (bf16, any row stride that is a multiple of 8) at inference: the final RMSNorm
    (norm_w, eps) and the value head (w bf16 [dim], b bf16 [1]) in one launch, out fp32 [rows] (any stride) — bit for bit
    `ops.rmsnorm` followed by `value_head`'s v, without writing the norm's output. w and b are read when the op runs."""
    rows, dim = _bf16(x, "x").shape
    for t, what in ((norm_w, "norm_w"), (w, "w")):
        if _bf16(t, what).numel() != dim or not t.is_contiguous():
            raise ValueError(f"value_predict: {what} bf16 [{dim}] contiguous")
    if _bf16(b, "b").numel() != 1:
        raise ValueError("value_predict: b bf16 [1]")
    if _f32(out, "out").dim() != 1 or out.shape[0] != rows or (rows > 1 and out.stride(0) < 1):
        raise ValueError(f"value_predict: out fp32 [{rows}] with a positive stride")
    return _op("bl_value_predict_f32",
               (x.data_ptr(), _rows(x, "x"), rows, dim, norm_w.data_ptr(), float(eps), w.data_ptr(), b.data_ptr(), out.data_ptr(),
                out.stride(0) if rows > 1 else 1),
               (x, norm_w, w, b, out), run, nbytes=2.0 * rows * dim + 4.0 * dim + 4.0 * rows, flops=5.0 * rows * dim)


def rmsnorm_backward(x, w, dy, dx, dw, ws, eps: float, dres: Optional[torch.Tensor] = None, run: bool = True) -> Op:
    rows, dim = x.shape
    return _op("bl_rmsnorm_backward_bf16",
               (_bf16(x, "x").data_ptr(), _rows(x, "x"), _bf16(w, "w").data_ptr(), _bf16(dy, "dy").data_ptr(), _rows(dy, "dy"),
                dres.data_ptr() if dres is not None else None, _rows(dres, "dres") if dres is not None else 0,
                _bf16(dx, "dx").data_ptr(), _rows(dx, "dx"), _f32(dw, "dw").data_ptr(), _f32(ws, "ws").data_ptr(), ws.numel(),
                rows, dim, float(eps)), (x, w, dy, dx, dw, ws, dres), run, nbytes=2.0 * rows * dim * (4 if dres is not None else 3))


def colsum(a, out, ws, run: bool = True) -> Op:
    rows, cols = a.shape
    return _op("bl_colsum_bf16", (_bf16(a, "a").data_ptr(), _rows(a, "a"), rows, cols, _f32(out, "out").data_ptr(),
                                  _f32(ws, "ws").data_ptr(), ws.numel()), (a, out, ws), run, nbytes=2.0 * rows * cols)


def swiglu(gu, act, run: bool = True) -> Op:
    rows, two_i = gu.shape
    return _op("bl_swiglu_bf16", (_bf16(gu, "gu").data_ptr(), _rows(gu, "gu"), _bf16(act, "act").data_ptr(), _rows(act, "act"),
                                  rows, two_i // 2), (gu, act), run, nbytes=3.0 * rows * two_i)


def swiglu_backward(gu, dact, dgu, run: bool = True) -> Op:
    rows, two_i = gu.shape
    return _op("bl_swiglu_backward_bf16",
               (_bf16(gu, "gu").data_ptr(), _rows(gu, "gu"), _bf16(dact, "dact").data_ptr(), _rows(dact, "dact"),
                _bf16(dgu, "dgu").data_ptr(), _rows(dgu, "dgu"), rows, two_i // 2), (gu, dact, dgu), run, nbytes=5.0 * rows * two_i)


def gelu(x, y, run: bool = True) -> Op:
    rows, cols = x.shape
    return _op("bl_gelu_bf16", (_bf16(x, "x").data_ptr(), _rows(x, "x"), _bf16(y, "y").data_ptr(), _rows(y, "y"), rows, cols), (x, y), run,
               nbytes=4.0 * rows * cols)


def gelu_backward(x, dy, dx, run: bool = True) -> Op:
    rows, cols = x.shape
    return _op("bl_gelu_backward_bf16", (_bf16(x, "x").data_ptr(), _rows(x, "x"), _bf16(dy, "dy").data_ptr(), _rows(dy, "dy"),
                                         _bf16(dx, "dx").data_ptr(), _rows(dx, "dx"), rows, cols), (x, dy, dx), run, nbytes=6.0 * rows * cols)


def rope(qkv, cos, sin, *, B: int, S: int, H: int, head_dim: int, pos0: int = 0, run: bool = True) -> Op:
    """Rotate the q and k thirds of fused qkv rows [B*S, 3*H*hd] (leading dimension free) in place: no KV cache."""
    return _op("bl_rope_bf16", (_bf16(qkv, "qkv").data_ptr(), _rows(qkv, "qkv"), B, S, H, head_dim, cos.data_ptr(), sin.data_ptr(), pos0),
               (qkv, cos, sin), run, nbytes=8.0 * B * S * H * head_dim)


def rope_backward(dqkv, cos, sin, *, B: int, S: int, H: int, head_dim: int, pos0: int = 0, run: bool = True) -> Op:
    return _op("bl_rope_backward_bf16", (_bf16(dqkv, "dqkv").data_ptr(), _rows(dqkv, "dqkv"), B, S, H, head_dim, cos.data_ptr(),
                                         sin.data_ptr(), pos0), (dqkv, cos, sin), run, nbytes=8.0 * B * S * H * head_dim)


def transpose_pad(a, out, rows_pad: int, run: bool = True) -> Op:
    rows, cols = a.shape
    return _op("bl_transpose_pad_bf16", (_bf16(a, "a").data_ptr(), _rows(a, "a"), rows, cols, _bf16(out, "out").data_ptr(),
                                         _rows(out, "out"), rows_pad), (a, out), run, nbytes=2.0 * cols * (rows + rows_pad))


def colamax(x: torch.Tensor, amax: torch.Tensor, run: bool = True) -> Op:
    """amax[c] = max(amax[c], max_t |x[t, c]|) (fp32): per-channel scales of the e4m3 weight-gradient operands. The kernel
    accumulates into amax with an atomic max over the bits of non-negative floats, so amax must be zeroed first (or hold a
    non-negative running maximum); columns of zeros leave it untouched."""
    rows, cols = x.shape
    assert amax.dtype == torch.float32 and amax.numel() >= cols
    return _op("bl_colamax_bf16", (_bf16(x, "x").data_ptr(), _rows(x, "x"), rows, cols, amax.data_ptr()), (x, amax), run,
               nbytes=2.0 * rows * cols)


def transpose_quantize_fp8(x: torch.Tensor, amax: torch.Tensor, q: torch.Tensor, scales: torch.Tensor, tokens_pad: int, packed: bool,
                           run: bool = True) -> Op:
    """x bf16 [tokens, channels] → e4m3 codes, token-contiguous per channel (tokens zero-padded to tokens_pad) + scales[c] =
    amax[c] / 448 (1, with all-zero codes, for amax[c] < 2^-100): q uint8 [channels, tokens_pad] row-major, or (packed) in bl_gemm_fp8's weight-operand packing
    [channels / 16, tokens_pad / 64, 64, 16]. One pass: 2 B read + 1 B written per element."""
    rows, cols = x.shape
    assert q.dtype == torch.uint8 and q.is_contiguous() and q.numel() == cols * tokens_pad and scales.numel() >= cols
    return _op("bl_transpose_quantize_fp8", (_bf16(x, "x").data_ptr(), _rows(x, "x"), rows, cols, amax.data_ptr(), q.data_ptr(),
                                             tokens_pad, int(packed), scales.data_ptr()), (x, amax, q, scales), run,
               nbytes=3.0 * rows * cols)


def map_rows(src, dst, *, rows: int, group: int, stride: int, offset: int, scatter: bool, run: bool = True) -> Op:
    cols = src.shape[1]
    return _op("bl_map_rows_bf16", (_bf16(src, "src").data_ptr(), _rows(src, "src"), _bf16(dst, "dst").data_ptr(), _rows(dst, "dst"),
                                    rows, cols, group, stride, offset, int(scatter)), (src, dst), run, nbytes=4.0 * rows * cols)


def sumsq_partial(g: torch.Tensor, partial: torch.Tensor, run: bool = True) -> Op:
    return _op("bl_sumsq_partial_f32", (_f32(g, "g").data_ptr(), g.numel(), _f32(partial, "partial").data_ptr(), partial.numel()),
               (g, partial), run, nbytes=4.0 * g.numel())


def clip_coef(partials: torch.Tensor, max_norm: float, out: torch.Tensor, run: bool = True) -> Op:
    return _op("bl_clip_coef_f32", (partials.data_ptr(), partials.numel(), float(max_norm), out.data_ptr()), (partials, out), run)


def adamw(p, m, v, g, step: int, lr: float, *, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
          norm_coef: Optional[torch.Tensor] = None, p_bf16: Optional[torch.Tensor] = None, run: bool = True) -> Op:
    for t in (p, m, v, g):
        assert t.dtype == torch.float32 and t.is_contiguous()
    return _op("bl_adamw_f32", (p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(),
                                norm_coef.data_ptr() if norm_coef is not None else None, p.numel(), float(lr), float(betas[0]),
                                float(betas[1]), float(eps), float(weight_decay), int(step),
                                p_bf16.data_ptr() if p_bf16 is not None else None), (p, m, v, g, norm_coef, p_bf16), run,
               nbytes=(28.0 + (2.0 if p_bf16 is not None else 0.0)) * p.numel())


def embed_backward(ids, dx, dw, n_patches: int, run: bool = True) -> Op:
    B, L = ids.shape
    return _op("bl_embed_backward_bf16", (ids.data_ptr(), B, L, _bf16(dx, "dx").data_ptr(), dx.shape[-1], n_patches,
                                          _f32(dw, "dw").data_ptr()), (ids, dx, dw), run)


def attention_lse(q, k, v, o, lse, *, B, H, Sq, Skv, head_dim, q_strides, k_strides, v_strides, o_strides, causal,
                  scale=None, key_mask=None, run: bool = True) -> Op:
    """Training forward: attention + per-row base-2 log-sum-exp (lse: fp32 [B*H*pad32(Sq)])."""
    assert _f32(lse, "lse").numel() >= B * H * ((Sq + 31) // 32 * 32)
    d = _attn_desc(q, k, v, o, B, H, Sq, Skv, head_dim, q_strides, k_strides, v_strides, o_strides, causal,
                   head_dim ** -0.5 if scale is None else scale, key_mask)
    return _op("bl_attention_lse_bf16", (C.byref(d), lse.data_ptr()), (d, q, k, v, o, lse, key_mask), run,
               flops=4.0 * B * H * Sq * Skv * head_dim * (0.5 if causal else 1.0))


def attention_backward(q, k, v, o, dout, lse, delta, dq, dk, dv, *, B, H, Sq, Skv, head_dim, q_strides, k_strides,
                       v_strides, o_strides, causal, scale=None, key_mask=None, run: bool = True) -> Op:
    for t in (lse, delta):
        assert _f32(t, "lse/delta").numel() >= B * H * ((Sq + 31) // 32 * 32)
    d = _attn_desc(q, k, v, o, B, H, Sq, Skv, head_dim, q_strides, k_strides, v_strides, o_strides, causal,
                   head_dim ** -0.5 if scale is None else scale, key_mask)
    return _op("bl_attention_backward_bf16",
               (C.byref(d), _bf16(dout, "dout").data_ptr(), lse.data_ptr(), delta.data_ptr(), _bf16(dq, "dq").data_ptr(),
                _bf16(dk, "dk").data_ptr(), _bf16(dv, "dv").data_ptr()), (d, q, k, v, o, dout, lse, delta, dq, dk, dv, key_mask), run,
               flops=14.0 * B * H * Sq * Skv * head_dim * (0.5 if causal else 1.0))


def attention_tree_lse(q, k, v, o, lse, *, B, H, S, prefix, branch, head_dim, q_strides, k_strides, v_strides, o_strides,
                       scale=None, key_mask=None, run: bool = True) -> Op:
    """Training forward over the shared-prompt layout (bl_attention_tree_lse_bf16): every batch element is one prompt row
    prefix ‖ G branches of `branch` rows, S = prefix + G·branch; lse fp32 [B*H*pad32(S)]."""
    assert _f32(lse, "lse").numel() >= B * H * ((S + 31) // 32 * 32)
    G = (S - prefix) // branch if branch > 0 else 0      # a bad branch is the library's to refuse
    d = _attn_desc(q, k, v, o, B, H, S, S, head_dim, q_strides, k_strides, v_strides, o_strides, True,
                   head_dim ** -0.5 if scale is None else scale, key_mask)
    return _op("bl_attention_tree_lse_bf16", (C.byref(d), prefix, branch, lse.data_ptr()), (d, q, k, v, o, lse, key_mask), run,
               flops=4.0 * B * H * head_dim * (0.5 * prefix * prefix + G * branch * (prefix + 0.5 * branch)))


def attention_tree_backward(q, k, v, o, dout, lse, delta, dq, dk, dv, *, B, H, S, prefix, branch, head_dim, q_strides, k_strides,
                            v_strides, o_strides, scale=None, key_mask=None, run: bool = True) -> Op:
    for t in (lse, delta):
        assert _f32(t, "lse/delta").numel() >= B * H * ((S + 31) // 32 * 32)
    G = (S - prefix) // branch if branch > 0 else 0      # a bad branch is the library's to refuse
    d = _attn_desc(q, k, v, o, B, H, S, S, head_dim, q_strides, k_strides, v_strides, o_strides, True,
                   head_dim ** -0.5 if scale is None else scale, key_mask)
    return _op("bl_attention_tree_backward_bf16",
               (C.byref(d), prefix, branch, _bf16(dout, "dout").data_ptr(), lse.data_ptr(), delta.data_ptr(),
                _bf16(dq, "dq").data_ptr(), _bf16(dk, "dk").data_ptr(), _bf16(dv, "dv").data_ptr()),
               (d, q, k, v, o, dout, lse, delta, dq, dk, dv, key_mask), run,
               flops=14.0 * B * H * head_dim * (0.5 * prefix * prefix + G * branch * (prefix + 0.5 * branch)))


def _rope_pos_args(qkv, what: str, cos, sin, pos, rows: int, H: int, head_dim: int):
    if pos.dtype != torch.int32 or not pos.is_contiguous() or pos.numel() != rows:
        raise ValueError(f"rope_pos: pos int32 [{rows}] contiguous")
    return (_bf16(qkv, what).data_ptr(), _rows(qkv, what), rows, H, head_dim, cos.data_ptr(), sin.data_ptr(), pos.data_ptr())


def rope_pos(qkv, cos, sin, pos, *, rows: int, H: int, head_dim: int, run: bool = True) -> Op:
    """`rope` with a position per row: pos int32 [rows] on the device (bl_rope_pos_bf16)."""
    return _op("bl_rope_pos_bf16", _rope_pos_args(qkv, "qkv", cos, sin, pos, rows, H, head_dim), (qkv, cos, sin, pos), run,
               nbytes=8.0 * rows * H * head_dim)


def rope_pos_backward(dqkv, cos, sin, pos, *, rows: int, H: int, head_dim: int, run: bool = True) -> Op:
    return _op("bl_rope_pos_backward_bf16", _rope_pos_args(dqkv, "dqkv", cos, sin, pos, rows, H, head_dim), (dqkv, cos, sin, pos),
               run, nbytes=8.0 * rows * H * head_dim)


def pack(w: torch.Tensor, out: torch.Tensor, run: bool = True) -> Op:
    """Row-major [N, K] → fragment-major packed (bl_pack_weight_bf16) as a replayable Op (weights after an optimizer
    step; the transposed activations of a wgrad GEMM)."""
    N, K = w.shape
    assert out.numel() == N * K and N % 16 == 0 and K % 32 == 0
    return _op("bl_pack_weight_bf16", (_bf16(w, "w").data_ptr(), _rows(w, "w"), N, K, _bf16(out, "out").data_ptr()), (w, out), run,
               nbytes=4.0 * N * K)


def layernorm_backward(x, w, dy, dx, dw, db, ws, eps: float, dres: Optional[torch.Tensor] = None, run: bool = True) -> Op:
    rows, dim = x.shape
    return _op("bl_layernorm_backward_bf16",
               (_bf16(x, "x").data_ptr(), _rows(x, "x"), _bf16(w, "w").data_ptr(), _bf16(dy, "dy").data_ptr(), _rows(dy, "dy"),
                dres.data_ptr() if dres is not None else None, _rows(dres, "dres") if dres is not None else 0,
                _bf16(dx, "dx").data_ptr(), _rows(dx, "dx"), _f32(dw, "dw").data_ptr(), _f32(db, "db").data_ptr(),
                _f32(ws, "ws").data_ptr(), ws.numel(), rows, dim, float(eps)), (x, w, dy, dx, dw, db, ws, dres), run,
               nbytes=2.0 * rows * dim * (4 if dres is not None else 3))


def scale_residual(u, scale, res, y, run: bool = True) -> Op:
    rows, cols = u.shape
    return _op("bl_scale_residual_bf16", (_bf16(u, "u").data_ptr(), _rows(u, "u"), _bf16(scale, "scale").data_ptr(),
                                          _bf16(res, "res").data_ptr(), _rows(res, "res"), _bf16(y, "y").data_ptr(), _rows(y, "y"),
                                          rows, cols), (u, scale, res, y), run, nbytes=6.0 * rows * cols)


def layerscale_backward(dy, u, scale, du, dscale, ws, run: bool = True) -> Op:
    rows, cols = dy.shape
    return _op("bl_layerscale_backward_bf16",
               (_bf16(dy, "dy").data_ptr(), _rows(dy, "dy"), _bf16(u, "u").data_ptr(), _rows(u, "u"), _bf16(scale, "scale").data_ptr(),
                _bf16(du, "du").data_ptr(), _rows(du, "du"), _f32(dscale, "dscale").data_ptr(), _f32(ws, "ws").data_ptr(), ws.numel(),
                rows, cols), (dy, u, scale, du, dscale, ws), run, nbytes=6.0 * rows * cols)


def fill_zero(t: torch.Tensor, run: bool = True) -> Op:
    assert t.is_contiguous()
    return _op("bl_memset_zero", (t.data_ptr(), t.numel() * t.element_size()), (t,), run, nbytes=float(t.numel() * t.element_size()))


def copy_f32(src: torch.Tensor, dst: torch.Tensor, run: bool = True) -> Op:
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel() and src.dtype == dst.dtype
    return _op("bl_copy_bytes", (dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size()), (src, dst), run)


def scale(x: torch.Tensor, s: float, out: torch.Tensor, run: bool = True) -> Op:
    assert x.is_contiguous() and out.is_contiguous() and x.numel() == out.numel()
    return _op("bl_scale_bf16", (_bf16(x, "x").data_ptr(), float(s), _bf16(out, "out").data_ptr(), x.numel()), (x, out), run)


def dropout(x: torch.Tensor, out: torch.Tensor, p: float, seed: torch.Tensor, salt: int, run: bool = True) -> Op:
    """out = nn.Dropout(p)(x) in training mode with the counter-based mask of (seed tensor [1] uint32 on the device, salt)."""
    rows, cols = x.shape
    assert seed.dtype in (torch.int32, torch.uint32) and seed.is_cuda and seed.numel() == 1
    return _op("bl_dropout_bf16", (_bf16(x, "x").data_ptr(), _rows(x, "x"), rows, cols, float(p), seed.data_ptr(), int(salt) & 0xFFFFFFFF,
                                   _bf16(out, "out").data_ptr(), _rows(out, "out")), (x, out, seed), run, nbytes=4.0 * rows * cols)


def dropout_grad_fix(u: torch.Tensor, dx: torch.Tensor, p: float, seed: torch.Tensor, salt: int, run: bool = True) -> Op:
    """dx (= dy·W + u) → dy·W + mask/(1-p) ⊙ u with the mask of `dropout(…, seed, salt)`."""
    rows, cols = u.shape
    return _op("bl_dropout_grad_fix_bf16", (_bf16(u, "u").data_ptr(), _rows(u, "u"), rows, cols, float(p), seed.data_ptr(),
                                            int(salt) & 0xFFFFFFFF, _bf16(dx, "dx").data_ptr(), _rows(dx, "dx")), (u, dx, seed), run,
               nbytes=6.0 * rows * cols)


def lora_block_mask(g: torch.Tensor, rp: int, members: int, interleave: bool, run: bool = True) -> Op:
    n, R = g.shape
    assert g.is_contiguous()
    return _op("bl_lora_block_mask_f32", (_f32(g, "g").data_ptr(), n, R, rp, members, int(interleave)), (g,), run)


def transpose_pack(a: torch.Tensor, out_packed: torch.Tensor, rows_pad: int, run: bool = True) -> Op:
    """[rows, cols] → packed [cols/16, rows_pad/32, 64, 8] (the transposed matrix in fragment-major layout)."""
    rows, cols = a.shape
    assert out_packed.numel() == cols * rows_pad and out_packed.is_contiguous()
    return _op("bl_transpose_pack_bf16", (_bf16(a, "a").data_ptr(), _rows(a, "a"), rows, cols, _bf16(out_packed, "out").data_ptr(),
                                          rows_pad), (a, out_packed), run, nbytes=2.0 * cols * (rows + rows_pad))


def gemm_tn(dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor, workspace: Optional[torch.Tensor] = None, run: bool = True) -> Op:
    """out[N, K] (fp32) = dyᵀ·x over the token rows: dy [T, N], x [T, K] row-major bf16 (column-slice views allowed) — the
    weight gradient of y = x·Wᵀ read straight from the buffers the backward pass already holds (bl_gemm_tn_bf16)."""
    from .ops import EPI_F32, GemmDesc
    Tn, N = dy.shape
    K = x.shape[1]
    if x.shape[0] != Tn or tuple(out.shape) != (N, K):
        raise ValueError(f"gemm_tn: dy{tuple(dy.shape)} x{tuple(x.shape)} out{tuple(out.shape)}")
    d = GemmDesc()
    d.A, d.lda = _bf16(dy, "dy").data_ptr(), _rows(dy, "dy")
    d.W, d.ldw = _bf16(x, "x").data_ptr(), _rows(x, "x")
    d.C, d.ldc = _f32(out, "out").data_ptr(), _rows(out, "out")
    d.M, d.N, d.K, d.epilogue = N, K, Tn, EPI_F32
    keep = [d, dy, x, out]
    if workspace is not None:
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
        keep.append(workspace)
    return _op("bl_gemm_tn_bf16", (C.byref(d),), tuple(keep), run, flops=2.0 * Tn * N * K, nbytes=2.0 * Tn * (N + K) + 4.0 * N * K)


def gemm_tn_small(P: torch.Tensor, Q: torch.Tensor, C: torch.Tensor, transpose_out: bool, ws: Optional[torch.Tensor] = None,
                  alpha: float = 1.0, run: bool = True) -> Op:
    """C = alpha · Pᵀ·Q over the rows: P [T, R] (R in 64/128/192), Q [T, N]; C fp32 [R, N] or, transposed, [N, R]."""
    Tn, R = P.shape
    N = Q.shape[1]
    assert Q.shape[0] == Tn and tuple(C.shape) == ((N, R) if transpose_out else (R, N)) and C.is_contiguous()
    return _op("bl_gemm_tn_small_bf16",
               (_bf16(P, "P").data_ptr(), _rows(P, "P"), _bf16(Q, "Q").data_ptr(), _rows(Q, "Q"), Tn, R, N, _f32(C, "C").data_ptr(),
                C.shape[1], int(transpose_out), float(alpha), ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0),
               (P, Q, C, ws), run, flops=2.0 * Tn * R * N, nbytes=2.0 * Tn * (R + N) + 4.0 * R * N)


def pack_into(w: torch.Tensor, out: torch.Tensor, kt_total: int, kb_offset: int, run: bool = True) -> Op:
    """Row-major [N, K] → k-blocks [kb_offset, kb_offset + K/32) of the packed matrix `out` ([N/16, kt_total, 64, 8])."""
    N, K = w.shape
    assert out.numel() == N * kt_total * 32
    return _op("bl_pack_weight_into_bf16", (_bf16(w, "w").data_ptr(), _rows(w, "w"), N, K, _bf16(out, "out").data_ptr(), kt_total,
                                            kb_offset), (w, out), run, nbytes=4.0 * N * K)


def transpose_pack_into(a: torch.Tensor, out: torch.Tensor, rows_pad: int, kt_total: int, kb_offset: int, run: bool = True) -> Op:
    """[rows, cols] → the transposed matrix's k-blocks [kb_offset, …) of packed `out` ([cols/16, kt_total, 64, 8])."""
    rows, cols = a.shape
    assert out.numel() == cols * kt_total * 32
    return _op("bl_transpose_pack_into_bf16", (_bf16(a, "a").data_ptr(), _rows(a, "a"), rows, cols, _bf16(out, "out").data_ptr(),
                                               rows_pad, kt_total, kb_offset), (a, out), run, nbytes=2.0 * cols * (rows + rows_pad))


# ---- batched small ops: one launch for a table of independent copies / (scaled) packs / (scaled) transposing packs -------------
def _grid_for(total: int, block: int = 256) -> int:
    return max(1, min(2048, (total + block - 1) // block))


def be_copy(src: torch.Tensor, dst: torch.Tensor):
    """Table entry: dst ← src (bytes), the work of bl_copy_bytes."""
    from ._lib import BatchOpDesc
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() * src.element_size() == dst.numel() * dst.element_size()
    n = src.numel() * src.element_size()
    vec = ((src.data_ptr() | dst.data_ptr()) & 15) == 0
    d = BatchOpDesc(kind=0, nblocks=_grid_for((n + 15) // 16 if vec else n), n=n, src=src.data_ptr(), dst=dst.data_ptr(), scale=1.0)
    return d, (src, dst)


def be_pack(w: torch.Tensor, out: torch.Tensor, kt_total: Optional[int] = None, kb_offset: int = 0, scale: float = 1.0):
    """Table entry: row-major [N, K] → k-blocks [kb_offset, …) of packed `out` (bl_pack_weight(_into)_bf16), of bf16(scale · w)."""
    from ._lib import BatchOpDesc
    N, K = w.shape
    kt = K // 32 if kt_total is None else kt_total
    assert N % 16 == 0 and K % 32 == 0 and out.numel() == N * kt * 32 and kb_offset + K // 32 <= kt and w.stride(1) == 1
    d = BatchOpDesc(kind=1, nblocks=_grid_for(N * K // 8), rows=N, cols=K, ld=w.stride(0), kt_total=kt, kb_off=kb_offset,
                    src=_bf16(w, "w").data_ptr(), dst=_bf16(out, "out").data_ptr(), scale=float(scale))
    return d, (w, out)


def be_transpose_pack(a: torch.Tensor, out: torch.Tensor, rows_pad: int, kt_total: Optional[int] = None, kb_offset: int = 0,
                      scale: float = 1.0):
    """Table entry: [rows, cols] → the transposed matrix's k-blocks of packed `out` (bl_transpose_pack(_into)_bf16), of bf16(scale · a)."""
    from ._lib import BatchOpDesc
    rows, cols = a.shape
    kt = rows_pad // 32 if kt_total is None else kt_total
    assert cols % 64 == 0 and rows_pad % 32 == 0 and rows_pad >= rows and out.numel() == cols * kt * 32 and a.stride(1) == 1
    bx = cols // 64
    d = BatchOpDesc(kind=2, nblocks=bx * ((rows_pad + 255) // 256), rows=rows, cols=cols, rows_pad=rows_pad, bx_count=bx,
                    ld=a.stride(0), kt_total=kt, kb_off=kb_offset, src=_bf16(a, "a").data_ptr(), dst=_bf16(out, "out").data_ptr(),
                    scale=float(scale))
    return d, (a, out)


def batched(entries, device, run: bool = True) -> Op:
    """ONE launch (bl_batched_ops) for the table entries made by be_copy / be_pack / be_transpose_pack. The entries must be
    independent of each other (no entry reads what another one writes)."""
    import ctypes as C
    import numpy as np
    from ._lib import BatchOpDesc
    descs = [e[0] for e in entries]
    arr = (BatchOpDesc * len(descs))(*descs)
    table = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(device)
    starts, tot = [], 0
    for d in descs:
        starts.append(tot)
        tot += d.nblocks
    block_start = torch.tensor(starts, dtype=torch.int32, device=device)
    keep = tuple(t for e in entries for t in e[1])
    nbytes = float(sum((d.n if d.kind == 0 else 2 * d.rows * d.cols) * 2 for d in descs))
    return _op("bl_batched_ops", (table.data_ptr(), block_start.data_ptr(), len(descs), tot), (table, block_start) + keep, run, nbytes=nbytes)


# ---- LoRA merge: W' = bf16(W + bf16(s·B)·A) on the packed layout (csrc/lora_merge.hip; training/lora.py::merged_reference) ----
LORA_MERGE_MAX_SPAN = 128      # ranks one row may see (LM_MAX_R): two interleaved members of padded rank 64


def lora_merge_items(n: int, k: int, R: int, rp: int, members: int, interleave: bool) -> int:
    """Work items of one group in the merge kernel (lm_shape in csrc/lora_merge.hip): four k-strips x up to 16 row tiles
    each; stacked members that own whole 16-row tiles are walked member by member (their own rank block only)."""
    skip = (not interleave) and members > 1 and n % (16 * members) == 0
    meff = members if skip else 1
    tpm = (n // 16) // meff
    return ((k // 32 + 3) // 4) * meff * ((tpm + 15) // 16)


def _lora_merge_check(w_packed, A, B, out_packed, rp: int, members: int, interleave: bool):
    R, k = A.shape
    n = B.shape[0]
    for t, what in ((w_packed, "w_packed"), (A, "A"), (B, "B"), (out_packed, "out_packed")):
        if not _bf16(t, what).is_contiguous():
            raise ValueError(f"lora_merge: {what} must be contiguous")
    if B.shape[1] != R or R != rp * members or n % 16 or k % 32 or R % 32 or rp % 32 or n % members:
        raise ValueError(f"lora_merge: A{tuple(A.shape)} B{tuple(B.shape)} rp={rp} members={members}")
    if w_packed.numel() != n * k or out_packed.numel() != n * k:
        raise ValueError(f"lora_merge: packed weights of {n} x {k} elements expected")
    skip = (not interleave) and members > 1 and n % (16 * members) == 0
    if (rp if skip else R) > LORA_MERGE_MAX_SPAN:
        raise ValueError(f"lora_merge: a row sees more than {LORA_MERGE_MAX_SPAN} ranks")
    if any(t.data_ptr() & 15 for t in (w_packed, A, B, out_packed)):
        raise ValueError("lora_merge: 16-byte aligned tensors")
    lo, hi = w_packed.data_ptr(), out_packed.data_ptr()
    if lo < hi + 2 * n * k and hi < lo + 2 * n * k:
        raise ValueError("lora_merge: out_packed must not overlap w_packed")
    return n, k, R


def lora_merge(w_packed, A, B, scale: float, out_packed, rp: int, members: int = 1, interleave: bool = False, run: bool = True) -> Op:
    """out_packed = packed bf16(W + bf16(scale·B)·A) from packed W [n/16, k/32, 64, 8], A [R, k], B [n, R] (bl_lora_merge_bf16).
    Shapes are the library's to check (error codes); only dtypes / devices are checked here."""
    R, k = A.shape
    n = B.shape[0]
    return _op("bl_lora_merge_bf16",
               (_bf16(w_packed, "w_packed").data_ptr(), _bf16(A, "A").data_ptr(), _bf16(B, "B").data_ptr(), float(scale),
                _bf16(out_packed, "out_packed").data_ptr(), n, k, R, rp, members, int(interleave)), (w_packed, A, B, out_packed), run,
               nbytes=4.0 * n * k, flops=2.0 * n * k * R)


def be_lora_merge(w_packed, A, B, scale: float, out_packed, rp: int, members: int = 1, interleave: bool = False):
    """Table entry of `lora_merge_batched`: the work of `lora_merge`, validated here (the device table cannot be)."""
    from ._lib import LoraMergeDesc
    n, k, R = _lora_merge_check(w_packed, A, B, out_packed, rp, members, interleave)
    d = LoraMergeDesc(w=w_packed.data_ptr(), A=A.data_ptr(), B=B.data_ptr(), out=out_packed.data_ptr(), scale=float(scale), n=n, k=k,
                      R=R, rp=rp, members=members, interleave=int(interleave),
                      n_items=lora_merge_items(n, k, R, rp, members, interleave), first_item=0)
    return d, (w_packed, A, B, out_packed)


def lora_merge_batched(entries, device, run: bool = False) -> Op:
    """ONE launch (bl_lora_merge_batched_bf16) for the table entries made by be_lora_merge: every adapted group of a model.
    The entries must be independent (no entry reads what another one writes). Bit-identical to one `lora_merge` per entry."""
    import numpy as np
    from ._lib import LoraMergeDesc
    if not entries:
        raise ValueError("lora_merge_batched: no entries")
    descs, tot = [e[0] for e in entries], 0
    for d in descs:
        d.first_item = tot
        tot += d.n_items
    arr = (LoraMergeDesc * len(descs))(*descs)
    table = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(device)
    keep = tuple(t for e in entries for t in e[1])
    return _op("bl_lora_merge_batched_bf16", (table.data_ptr(), len(descs)), (table,) + keep, run,
               nbytes=float(sum(4 * d.n * d.k for d in descs)), flops=float(sum(2 * d.n * d.k * d.R for d in descs)))


# ---- packed bf16 weight → packed e4m3 weight + per-channel scales (csrc/quantize_weight_fp8.hip; ops.quantize_packed_weight_fp8) ----
def quantize_packed_items(n: int, k: int) -> int:
    """Work items of one weight in the packed quantiser: one per 16-row tile (a tile's k columns stay in one workgroup, whose
    threads reduce the sixteen channels' amax among themselves)."""
    return n // 16


def be_quantize_packed(wp, w8, scale):
    """Table entry of `quantize_packed_batched`: the work of `ops.quantize_packed_weight_fp8`, validated here (the device
    table cannot be)."""
    from ._lib import WeightQuantDesc
    if wp.dim() != 4 or tuple(wp.shape[2:]) != (64, 8) or not _bf16(wp, "wp").is_contiguous():
        raise ValueError("quantize_packed: wp must be a packed bf16 weight [n/16, k/32, 64, 8]")
    n, k = wp.shape[0] * 16, wp.shape[1] * 32
    if n <= 0 or k <= 0 or k % 128 or n > 1 << 24 or k > 1 << 24:
        raise ValueError(f"quantize_packed: n = {n}, k = {k}: k % 128 == 0 expected")
    if not w8.is_cuda or not w8.is_contiguous() or w8.numel() * w8.element_size() != n * k:
        raise ValueError(f"quantize_packed: w8 must hold the {n * k} bytes of [n/16, k/64, 64, 16]")
    if _f32(scale, "scale").numel() != n or not scale.is_contiguous():
        raise ValueError(f"quantize_packed: scale fp32 [{n}]")
    if any(t.data_ptr() & 15 for t in (wp, w8, scale)):
        raise ValueError("quantize_packed: 16-byte aligned tensors")
    spans = [(wp.data_ptr(), 2 * n * k), (w8.data_ptr(), n * k), (scale.data_ptr(), 4 * n)]
    for i, (a, an) in enumerate(spans):
        for b, bn in spans[i + 1:]:
            if a < b + bn and b < a + an:
                raise ValueError("quantize_packed: wp, w8 and scale must not overlap")
    d = WeightQuantDesc(w=wp.data_ptr(), w8=w8.data_ptr(), scale=scale.data_ptr(), n=n, k=k, n_items=quantize_packed_items(n, k),
                        pad=0, first_item=0)
    return d, (wp, w8, scale)


def quantize_packed_batched(entries, device, run: bool = False) -> Op:
    """ONE launch (bl_quantize_weight_fp8_packed_batched) for the table entries made by be_quantize_packed: every e4m3 copy of
    a model's adapted weights. Bit-identical to one `ops.quantize_packed_weight_fp8` per entry."""
    import numpy as np
    from ._lib import WeightQuantDesc
    if not entries:
        raise ValueError("quantize_packed_batched: no entries")
    descs, tot = [e[0] for e in entries], 0
    for d in descs:
        d.first_item = tot
        tot += d.n_items
    arr = (WeightQuantDesc * len(descs))(*descs)
    table = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(device)
    keep = tuple(t for e in entries for t in e[1])
    return _op("bl_quantize_weight_fp8_packed_batched", (table.data_ptr(), len(descs)), (table,) + keep, run,
               nbytes=float(sum(3 * d.n * d.k for d in descs)))


def cast(src: torch.Tensor, dst: torch.Tensor, run: bool = True) -> Op:
    """fp32 → bf16 (round to nearest even) or bf16 → fp32 of flat contiguous buffers (gradient wire format)."""
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    name = {(torch.float32, torch.bfloat16): "bl_cast_f32_bf16", (torch.bfloat16, torch.float32): "bl_cast_bf16_f32"}[(src.dtype, dst.dtype)]
    return _op(name, (src.data_ptr(), dst.data_ptr(), src.numel()), (src, dst), run, nbytes=6.0 * src.numel())


def axpy(y: torch.Tensor, x: torch.Tensor, a: float, run: bool = True) -> Op:
    """y += a·x (flat fp32): gradient accumulation."""
    assert y.is_contiguous() and x.is_contiguous() and y.numel() == x.numel()
    return _op("bl_axpy_f32", (_f32(y, "y").data_ptr(), _f32(x, "x").data_ptr(), float(a), y.numel()), (y, x), run, nbytes=12.0 * y.numel())
