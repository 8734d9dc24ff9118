"""References and comparators for the glue kernels (bridgelang_amd/csrc/glue.hip, the greedy rows of sample.hip).

A helper module, not a test module: tests import it as `import glue_ref as G`. Every glue kernel is an exact copy, or
exact bf16 arithmetic that oracle/restate.py already restates (RoPE), so every comparison but the cross-entropy values is
bit for bit. The references are plain index arithmetic in torch:

    rope_          oracle.restate.apply_rope on the q and k thirds; the cache rows by slicing
    embed_splice_  table[ids] into rows 0 and 1 + n_patches …
    write_prefix_  prefix into rows [0, n_prefix) of every batch
    im2col_        oracle.restate.im2col_patch14, the pad columns zero
    pack_into_     the formula above pack_weight_kernel, written as a gather; ops.unpack_weight is its inverse
    argmax         torch.argmax (the first NaN of a row, else the first maximum)
    cross-entropy  train_ref64.cross_entropy (`loss`, `lmag`, `mean`, `m_mean`, `count`)

Sentinels. Every buffer a kernel writes is a `Win` (a column window of a wider allocation, with guard rows above and
below) or a `Flat` (a dense block between guard elements), filled with a sentinel: NaN for floating types, SENT_I64 for
integers. A reference with a trailing underscore works IN PLACE on the CPU copy of such a buffer (`host()`), writing
exactly the logical output; `assert_bits` then compares the WHOLE allocation, sentinels included, so one comparison
checks the values and that nothing outside the logical output was written. tests/test_glue_ref_cpu.py checks every
reference against an independent formulation and shows that the comparison rejects planted near-misses.
"""
from __future__ import annotations

import math

import torch

import train_ref64 as T64
from oracle import restate as R

bf16, f32, i64 = torch.bfloat16, torch.float32, torch.int64
NAN = float("nan")
SENT_I64 = -0x5A5A5A5A5A5A5A5B
PAD = 8
P = R.Prec(True)
GRID_CAP = 2048 * 256                 # grid_for (glue.hip): more work items than this take a second grid-stride trip


def _itype(t: torch.Tensor):
    return {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(_itype(t))


def _sentinel(dtype):
    return NAN if dtype.is_floating_point else (SENT_I64 if dtype == i64 else SENT_I64 >> 32)


class Win:
    """A [rows, cols] window at column PAD of a sentinel-filled [guard + rows + guard, cols + 2·PAD] allocation. `fill`
    replaces the sentinel where a stray READ has to show: a NaN read by mistake may pass for the NaN a rule asks for."""

    def __init__(self, rows, cols, dev, dtype=bf16, data=None, guard=1, fill=None, _buf=None):
        self.rows, self.cols, self.guard = rows, cols, guard
        fill = _sentinel(dtype) if fill is None else fill
        self.buf = _buf if _buf is not None else torch.full((rows + 2 * guard, cols + 2 * PAD), fill, dtype=dtype, device=dev)
        self.v = self.buf[guard:guard + rows, PAD:PAD + cols]
        if data is not None:
            self.v.copy_(data.to(dtype))

    def host(self):
        return Win(self.rows, self.cols, "cpu", guard=self.guard, _buf=self.buf.detach().cpu().clone())


class Flat:
    """A dense block of `shape` between `guard` sentinel elements on each side (guard·itemsize is a multiple of 16)."""

    def __init__(self, shape, dev, dtype=bf16, data=None, guard=64, _buf=None):
        self.shape, self.guard = tuple(shape), guard
        n = math.prod(self.shape)
        self.buf = _buf if _buf is not None else torch.full((n + 2 * guard,), _sentinel(dtype), dtype=dtype, device=dev)
        self.v = self.buf[guard:guard + n].view(self.shape)
        if data is not None:
            self.v.copy_(data.to(dtype).reshape(self.shape))

    def host(self):
        return Flat(self.shape, "cpu", guard=self.guard, _buf=self.buf.detach().cpu().clone())


def assert_bits(got, want, what: str) -> None:
    """The two allocations (Win / Flat / tensors) are equal bit for bit, sentinels included."""
    g = got.buf if hasattr(got, "buf") else got
    w = want.buf if hasattr(want, "buf") else want
    g, w = g.detach().cpu(), w.detach().cpu()
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {tuple(g.shape)} {g.dtype} vs {tuple(w.shape)} {w.dtype}"
    bad = bits(g) != bits(w)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ (sentinels included); first at {idx}: "
                             f"got {g[idx].item()!r}, expected {w[idx].item()!r}")


def outside_untouched(x, what: str) -> None:
    """Everything of the Win / Flat allocation outside its logical block still holds the sentinel."""
    ref = type(x)(x.rows, x.cols, "cpu", x.buf.dtype, guard=x.guard) if isinstance(x, Win) else Flat(x.shape, "cpu", x.buf.dtype, guard=x.guard)
    ref.v.copy_(x.v.detach().cpu())
    assert_bits(x, ref, f"{what}: wrote outside its logical output")


# ---- RoPE + KV-cache append ---------------------------------------------------------------------------------------------
def rope_(qkv, cos, sin, B: int, S: int, H: int, hd: int, pos0: int, k_cache=None, v_cache=None, cache_pos0=None,
          rotate=None) -> None:
    """bl_rope_kvcache_bf16 / bl_rope_bf16 on CPU bf16 views, in place. qkv [B·S, >= 3·H·hd] (the columns beyond are not
    touched): q is rotated in place. With caches [B, H, cache_len, hd]: the rotated k and the v third go to cache rows
    [pos0, pos0 + S) and the k third of qkv is left alone; without: k is rotated in place. The v third never changes.
    `rotate` (default oracle.restate.apply_rope) and `cache_pos0` exist for the planted near-misses of the CPU test."""
    rotate = rotate or (lambda x, p0: R.apply_rope(P, x, cos.float(), sin.float(), p0))
    D = H * hd
    t = qkv[:, :3 * D].float().reshape(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)          # [3, B, H, S, hd]
    q, k = rotate(t[0], pos0), rotate(t[1], pos0)
    back = lambda x: x.permute(0, 2, 1, 3).reshape(B * S, D).to(bf16)
    qkv[:, :D] = back(q)
    if k_cache is None:
        qkv[:, D:2 * D] = back(k)
        return
    c0 = pos0 if cache_pos0 is None else cache_pos0
    k_cache[:, :, c0:c0 + S] = k.to(bf16)
    v_cache[:, :, c0:c0 + S] = t[2].to(bf16)


def rope_inputs(B, S, H, hd, seed):
    """bf16-valued qkv rows; in the first and the last token the first rotation half of q and k is scaled by 2^20, so the
    two products of a pair differ by about 2^20 and the fp32 sum is itself rounded before the bf16 rounding."""
    from conftest import rand_bf16
    qkv = rand_bf16((B * S, 3 * H * hd), seed)
    v = qkv.view(B * S, 3, H, hd)
    for r in {0, B * S - 1}:
        v[r, :2, :, :hd // 2] *= 2.0 ** 20
    return qkv


# ---- copies ------------------------------------------------------------------------------------------------------------------
def embed_splice_(ids, table, dst, n_patches: int) -> None:
    """dst [B, L + n_patches, dim]: row 0 = table[ids[:, 0]], rows 1 + n_patches … = table[ids[:, 1:]]; the patch rows stay."""
    dst[:, 0] = table[ids[:, 0]]
    dst[:, 1 + n_patches:] = table[ids[:, 1:]]


def write_prefix_(prefix, x, B: int, T: int) -> None:
    """x [B·T, dim]: rows [0, n_prefix) of every batch = prefix; the other rows stay."""
    n_prefix, dim = prefix.shape
    x.view(B, T, dim)[:, :n_prefix] = prefix


def im2col_(pv, chan0: int, out) -> None:
    """out [B·256, ld]: columns [0, 588) = the patches of channels chan0 … chan0 + 2 in (c, i, j) order, [588, ld) = 0."""
    B = pv.shape[0]
    out[:, :588] = R.im2col_patch14(pv[:, chan0:chan0 + 3].contiguous()).reshape(B * 256, 588)
    out[:, 588:] = 0


def pack_into_(w, dst, kb_off: int = 0) -> None:
    """The comment above pack_weight_kernel as a gather: dst [N/16, kt_total, 64, 8];
    dst[nt, kb_off + ks, lane, e] = w[16·nt + (lane & 15), 32·ks + 8·(lane >> 4) + e]; the other k-blocks stay."""
    N, K = w.shape
    nt, ks, lane, e = torch.meshgrid(torch.arange(N // 16), torch.arange(K // 32), torch.arange(64), torch.arange(8), indexing="ij")
    dst[:, kb_off:kb_off + K // 32] = w[16 * nt + (lane & 15), 32 * ks + 8 * (lane >> 4) + e]


# ---- argmax and the greedy rows ------------------------------------------------------------------------------------------------
def argmax_rows(n: int, ld: int):
    """(logits [len(names), ld] fp32, names): the value cases of the argmax kernel at width n. Columns [n, ld) hold +inf
    and NaN, which a kernel that reads them would pick. Thread t of the 256 owns columns 4t … 4t + 3 (+ 1024 per pass);
    a wave is 64 threads = 256 columns. Indices are clamped into the row, so a narrow row repeats some cases."""
    g = torch.Generator().manual_seed(n)
    c = lambda i: min(i, n - 1)
    rows, names = [], []

    def add(name, edit, base=None):
        r = (torch.randn(n, generator=g) * 2).to(bf16).float() if base is None else torch.full((n,), float(base))
        edit(r)
        rows.append(r)
        names.append(name)

    def put(idx, val):
        def f(r):
            for i in idx:
                r[c(i)] = val
        return f
    add("random", lambda r: None)
    add("max at 0", put([0], 50.0))
    add("max at n-1", put([n - 1], 50.0))
    add("tie inside one thread", put([5, 6], 50.0))
    add("tie across lanes", put([9, 130], 50.0))
    add("tie across waves", put([300, 700], 50.0))
    add("tie across passes", put([1 + 1024, 1], 50.0) if n > 1025 else put([n - 1, 2], 50.0))
    add("tie across passes, late first", put([7 + 1024, 7 + 2048], 50.0))
    add("all equal", lambda r: None, base=1.5)
    add("all -inf", lambda r: None, base=-math.inf)
    add("-0 then +0", put([2], 0.0), base=-0.0)
    add("+0 then -0", put([2], -0.0), base=0.0)
    add("-0 and +0 above negatives", lambda r: (r.copy_(-r.abs() - 1), put([3], -0.0)(r), put([n - 2], 0.0)(r)))
    add("+inf", put([n // 2], math.inf))
    add("+inf twice", put([n - 1, 1], math.inf))
    add("one NaN", put([n // 2 + 1], NAN))
    add("one NaN behind +inf", lambda r: (put([1], math.inf)(r), put([n - 1], NAN)(r)))
    add("NaN at 0", put([0], NAN))
    add("several NaN", put([n - 1, 3, 700], NAN))
    add("NaN in two passes", put([1024 + 2, 2048 + 2], NAN))
    add("all NaN", lambda r: None, base=NAN)
    add("all NaN but one", put([2], 70.0), base=NAN)
    lg = torch.stack(rows)
    pad = torch.full((len(rows), ld - n), math.inf)
    pad[:, 1::2] = NAN
    return torch.cat([lg, pad], 1), names


def first_nan_else_first_max(row) -> int:
    """The argmax specification as a plain loop: the first NaN, else the first maximum."""
    best, bi = None, -1
    for i, v in enumerate(row.tolist()):
        if v != v:
            return i
        if best is None or v > best:
            best, bi = v, i
    return bi


def check_argmax(got, logits, n: int, what: str, names=None) -> None:
    """got[r] == torch.argmax(logits[r, :n]) for every row, and so lies in [0, n)."""
    got = got.detach().cpu()
    want = torch.argmax(logits[:, :n].detach().cpu(), dim=-1)
    assert got.dtype == i64 and got.shape == want.shape
    bad = (got != want).nonzero().flatten().tolist()
    assert not bad, f"{what}: rows {[(r, names[r] if names else '') for r in bad]}: got {got[bad].tolist()}, torch.argmax {want[bad].tolist()}"
    assert bool(((got >= 0) & (got < n)).all()), f"{what}: an id outside [0, {n})"


# ---- cross-entropy ---------------------------------------------------------------------------------------------------------------
def mean_c(rows: int) -> int:
    """The constant of the mean over `rows` rows: the per-row terms' C_CE_MEAN plus the depth of the fp32 sum in
    masked_mean_kernel: ceil(rows / 256) per-thread adds, six shuffle levels, three LDS adds and the division."""
    return T64.C_CE_MEAN + (rows + 255) // 256 + 10


def check_cross_entropy(what: str, row_loss, mean_and_count, logits, targets, ignore_index: int = -100) -> None:
    """Per row against the fp64 reference (bound C_CE_MEAN·e·lmag[row]); ignored rows exactly +0; the count exact; the mean
    within mean_c(rows)·e·m_mean. All rows ignored: (0, 0) exactly."""
    ref = T64.cross_entropy(logits, targets, ignore_index)
    row_loss, mc = row_loss.detach().cpu(), mean_and_count.detach().cpu()
    ign = targets.detach().cpu() == ignore_index
    assert bool((bits(row_loss)[ign] == 0).all()), f"{what}: an ignored row's loss is not +0"
    T64.assert_f32_close(row_loss, ref["loss"], ref["lmag"], T64.C_CE_MEAN, f"{what} row loss")
    assert mc[1].item() == ref["count"], f"{what}: count {mc[1].item()} vs {ref['count']}"
    if ref["count"] == 0:
        assert bits(mc).tolist() == [0, 0], f"{what}: all rows ignored must give (+0, +0), got {mc.tolist()}"
    else:
        T64.assert_f32_close(mc[0], ref["mean"], ref["m_mean"], mean_c(len(ign)), f"{what} mean")


def check_cross_entropy_outside(what: str, row_loss, mean_and_count, logits, targets, ignore_index: int = -100) -> None:
    """Some targets lie outside [0, n) and are not ignore_index: those rows' losses and the mean are NaN, they count as
    valid, and every other row is what it would be without them."""
    n = logits.shape[1]
    tg = targets.detach().cpu()
    out = (tg != ignore_index) & ((tg < 0) | (tg >= n))
    assert bool(out.any())
    row_loss, mc = row_loss.detach().cpu(), mean_and_count.detach().cpu()
    assert bool(row_loss[out].isnan().all()), f"{what}: rows {out.nonzero().flatten().tolist()} (target outside [0, {n})) have losses {row_loss[out].tolist()}, not NaN"
    assert math.isnan(mc[0].item()), f"{what}: mean {mc[0].item()} with a target outside the vocabulary, not NaN"
    assert mc[1].item() == int((tg != ignore_index).sum()), f"{what}: count {mc[1].item()}"
    rest = torch.where(out, torch.full_like(tg, ignore_index), tg)
    ref = T64.cross_entropy(logits, rest, ignore_index)
    assert bool((bits(row_loss)[tg == ignore_index] == 0).all()), f"{what}: an ignored row's loss is not +0"
    T64.assert_f32_close(row_loss[~out], ref["loss"][~out], ref["lmag"][~out], T64.C_CE_MEAN, f"{what} other rows")
