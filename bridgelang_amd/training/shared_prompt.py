"""The row layout of the shared-prompt training step (`TrainStep(shared_prompt=G, branch_len=nb)`), specified
on the host in numpy / torch. No kernel is involved here: this module says where every token of a batch sits, which rows see
which, and at what rotary position — the definition the step's buffers are filled from and the tests check the kernels
against.

B sequences [B, l] arrive as for the replicated step, in consecutive groups of G that share their prompt. The step works on
P = B / G prompt rows of S = P0 + G·nb positions each:

    prefix (P0 rows)  ‖  branch 0 (nb rows)  ‖  …  ‖  branch G−1 (nb rows)

For a sequence whose labelled tokens are the contiguous run [f, e], the split point is s = f − 1, the token whose row
predicts the first label. The prefix holds BOS, the n_patches patch columns and the tokens [1, s) — 1 + n_patches + (s − 1) =
n_patches + s rows — right-padded to the static capacity P0; the branch holds the tokens [s, e), e − s of them (the number of
labelled tokens), right-padded to nb. The token at e and everything behind it are dropped: in a causal model they influence
no labelled position. Padding rows are hidden by the key mask, as padded positions are in the replicated layout.

Row r of the prefix is at rotary position r; row j of a branch is at n_patches + s + j: where the replicated layout has the
same token. The row of token t (s <= t < e) of sequence b = p·G + g is p·S + P0 + g·nb + (t − s), and it predicts token t + 1:
a per-token value aligned with the labels (index t, f <= t <= e) lives on the row of token t − 1.

P0 = the capacity n_patches + L − nb (a sequence of the planned length L whose branch is full) rounded up to a multiple of nb,
so that the loss kernels' `group_rows = nb` addressing takes every branch as one group and prefix runs hold no labelled row.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

IGNORE_INDEX = -100
PAD_TOKEN = 32000


def tree_visible(prefix: int, branch: int, rows: int, key_mask=None) -> np.ndarray:
    """[rows, rows] bool: key j is visible to query i iff key_mask[j], j <= i, and (j < prefix, or i >= prefix and
    (i − prefix) // branch == (j − prefix) // branch) — the predicate of bl_attention_tree_lse_bf16."""
    if prefix < 1 or branch < 1 or rows < prefix or (rows - prefix) % branch:
        raise ValueError(f"tree_visible: rows {rows} is not prefix {prefix} + G·branch {branch}")
    i = np.arange(rows)[:, None]
    j = np.arange(rows)[None, :]
    vis = (j <= i) & ((j < prefix) | ((i >= prefix) & ((i - prefix) // branch == (j - prefix) // branch)))
    if key_mask is not None:
        vis = vis & (np.asarray(key_mask).reshape(1, rows) != 0)
    return vis


@dataclass(frozen=True)
class SharedPromptLayout:
    """Static shape of the layout: B sequences of up to L text tokens in groups of G, branches of nb rows."""
    B: int
    G: int
    nb: int
    L: int
    n_patches: int

    def __post_init__(self):
        if self.G < 1 or self.nb < 1 or self.B < 1:
            raise ValueError(f"shared_prompt: batch {self.B}, shared_prompt {self.G} and branch_len {self.nb} must be >= 1")
        if self.B % self.G:
            raise ValueError(f"shared_prompt: the batch of {self.B} sequences is not a multiple of the group size {self.G}")
        if self.nb + 1 > self.L:
            raise ValueError(f"shared_prompt: branch_len {self.nb} leaves no prompt in sequences of {self.L} tokens")

    @property
    def P(self) -> int:
        return self.B // self.G

    @property
    def P0(self) -> int:
        cap = self.n_patches + self.L - self.nb
        return (cap + self.nb - 1) // self.nb * self.nb

    @property
    def S(self) -> int:
        """Rows per prompt."""
        return self.P0 + self.G * self.nb

    @property
    def text_len(self) -> int:
        """Length of the step's internal id rows: S minus the patch columns, which embed no token."""
        return self.S - self.n_patches

    def branch_row(self, g: int, j: int = 0) -> int:
        return self.P0 + g * self.nb + j


@dataclass
class SharedBatch:
    """One batch in the layout, on the host. `ids` [P, text_len] int64 (index 0 = BOS = row 0, index j >= 1 = row
    n_patches + j, as the embedding splice places them); `key_mask` [P, S] uint8; `targets` [P·S] int64 (the token each row
    predicts, IGNORE_INDEX elsewhere); `pos` [P·S] int32; `token_row` [B, l] int64: for a labelled token position the flat
    row that predicts it, −1 elsewhere; `split` [B] the split points s; `count` [B] the labelled tokens per sequence."""
    ids: np.ndarray
    key_mask: np.ndarray
    targets: np.ndarray
    pos: np.ndarray
    token_row: np.ndarray
    split: np.ndarray
    count: np.ndarray


def _np(x, dtype) -> np.ndarray:
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x).astype(dtype, copy=False)


def plan_batch(lay: SharedPromptLayout, input_ids, attention_mask, labels) -> SharedBatch:
    """Lay a right-padded batch [B, l] out. ValueError — before anything is produced — when B is not the layout's, the ids
    or the mask of the positions before s differ inside a group, the split points differ inside a group, a sequence's
    labels are not one contiguous run (or start before token 2: the prefix keeps BOS and the branch starts on a text token),
    the run is longer than nb, or the prefix exceeds P0."""
    ids, lab = _np(input_ids, np.int64), _np(labels, np.int64)
    if ids.ndim != 2 or ids.shape != lab.shape:
        raise ValueError(f"shared_prompt: input_ids and labels [B, l], got {ids.shape} and {lab.shape}")
    B, l = ids.shape
    msk = np.ones((B, l), dtype=np.uint8) if attention_mask is None else (_np(attention_mask, np.int64) != 0).astype(np.uint8)
    if msk.shape != ids.shape:
        raise ValueError(f"shared_prompt: attention_mask {msk.shape} does not match input_ids {ids.shape}")
    if B != lay.B or l > lay.L:
        raise ValueError(f"shared_prompt: batch {ids.shape} does not fit the planned step ({lay.B}, <= {lay.L}); the batch must "
                         f"be a multiple of the group size {lay.G}")
    G, nb, P0, S, npat = lay.G, lay.nb, lay.P0, lay.S, lay.n_patches
    split, count = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        at = np.flatnonzero(lab[b] != IGNORE_INDEX)
        if at.size == 0 or at[-1] - at[0] + 1 != at.size:
            raise ValueError(f"shared_prompt: the labels of sequence {b} are not one contiguous run "
                             f"({'none' if at.size == 0 else at.tolist()})")
        if at[0] < 2:
            raise ValueError(f"shared_prompt: sequence {b} is labelled from token {int(at[0])}: the first label must sit at "
                             "token 2 or later")
        if at.size > nb:
            raise ValueError(f"shared_prompt: sequence {b} has {at.size} labelled tokens, more than branch_len {nb}")
        split[b], count[b] = at[0] - 1, at.size
    for p in range(lay.P):
        b0 = p * G
        s = int(split[b0])
        for b in range(b0 + 1, b0 + G):
            if split[b] != s:
                raise ValueError(f"shared_prompt: sequences {b0} and {b} share a group but split at {s} and {int(split[b])}")
            if not np.array_equal(ids[b, :s], ids[b0, :s]) or not np.array_equal(msk[b, :s], msk[b0, :s]):
                raise ValueError(f"shared_prompt: sequences {b0} and {b} share a group but their ids or mask differ before "
                                 f"the split point {s}")
        if npat + s > P0:
            raise ValueError(f"shared_prompt: the prefix of group {p} ({npat} patches + {s} tokens) exceeds the capacity {P0}")
    out_ids = np.full((lay.P, lay.text_len), PAD_TOKEN, dtype=np.int64)
    key_mask = np.zeros((lay.P, S), dtype=np.uint8)
    targets = np.full((lay.P, S), IGNORE_INDEX, dtype=np.int64)
    pos = np.tile(np.arange(S, dtype=np.int32), (lay.P, 1))
    token_row = np.full((B, l), -1, dtype=np.int64)
    for p in range(lay.P):
        b0 = p * G
        s = int(split[b0])
        out_ids[p, :s] = ids[b0, :s]
        key_mask[p, 0] = msk[b0, 0]
        key_mask[p, 1:1 + npat] = 1
        key_mask[p, 1 + npat:npat + s] = msk[b0, 1:s]
        for g in range(G):
            b, n = b0 + g, int(count[b0 + g])
            r0 = lay.branch_row(g)
            out_ids[p, r0 - npat:r0 - npat + n] = ids[b, s:s + n]
            key_mask[p, r0:r0 + n] = msk[b, s:s + n]
            targets[p, r0:r0 + n] = lab[b, s + 1:s + 1 + n]
            pos[p, r0:r0 + nb] = npat + s + np.arange(nb, dtype=np.int32)
            token_row[b, s + 1:s + 1 + n] = p * S + r0 + np.arange(n)
    return SharedBatch(out_ids, key_mask, targets.reshape(-1), pos.reshape(-1), token_row, split, count)


def tokens_to_rows(token_row: np.ndarray, src, rows: int, name: str = "values") -> torch.Tensor:
    """Per-token values [B, l(, C)] aligned with the labels → fp32 [rows(, C)] in row layout: the value of labelled token t
    on the row that predicts it, 0 elsewhere. A non-finite value on a labelled position is a ValueError."""
    src = torch.as_tensor(src).detach().to("cpu", torch.float32)
    if tuple(src.shape[:2]) != token_row.shape:
        raise ValueError(f"{name}: shape {tuple(src.shape)}, expected {token_row.shape} (aligned with the labels of set_batch)")
    sel = torch.from_numpy(token_row >= 0)
    vals = src[sel]
    if not bool(torch.isfinite(vals).all()):
        raise ValueError(f"{name}: {int((~torch.isfinite(vals)).sum())} non-finite value(s) on labelled positions")
    out = torch.zeros((rows,) + tuple(src.shape[2:]), dtype=torch.float32)
    out[torch.from_numpy(token_row[token_row >= 0])] = vals
    return out


def rows_to_tokens(token_row: np.ndarray, rows: torch.Tensor) -> torch.Tensor:
    """Inverse of `tokens_to_rows` on the labelled positions: per-row values [rows] → [B, l] on the rows' device, 0 off the
    labels."""
    idx = torch.from_numpy(np.where(token_row >= 0, token_row, 0)).to(rows.device)
    sel = torch.from_numpy(token_row >= 0).to(rows.device)
    return torch.where(sel, rows.reshape(-1)[idx], torch.zeros((), dtype=rows.dtype, device=rows.device))


def cut_out(lay: SharedPromptLayout, batch: SharedBatch, b: int):
    """The rows of sequence b inside its prompt's tree — the prefix rows and its own branch's — without the masked ones:
    (rows [n] within the prompt, the [n, n] visibility among them, their positions [n])."""
    p, g = divmod(b, lay.G)
    rows = np.concatenate([np.arange(lay.P0), lay.branch_row(g) + np.arange(lay.nb)])
    rows = rows[batch.key_mask[p, rows] != 0]
    vis = tree_visible(lay.P0, lay.nb, lay.S, batch.key_mask[p])
    return rows, vis[np.ix_(rows, rows)], batch.pos.reshape(lay.P, lay.S)[p, rows]
