"""The row layout of the shared-prompt training step (bridgelang_amd/training/shared_prompt.py), without a GPU: where the
tokens of hand-made batches land, the row maps there and back, every refusal, the visibility function cut out per sequence
against the replicated sequence's causal mask and positions, and the new ABI symbols."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from bridgelang_amd.training import shared_prompt as SP

ROOT = Path(__file__).resolve().parents[1]
NPAT = 256


def grouped(prompt_lens, G, n_lab, L, tail=1, seed=0):
    """B = len(prompt_lens)·G sequences: prompt ‖ n_lab labelled tokens ‖ `tail` unlabelled ones (EOS), right-padded to L."""
    g = torch.Generator().manual_seed(seed)
    B = len(prompt_lens) * G
    ids, mask, labels = torch.full((B, L), 32000), torch.zeros(B, L, dtype=torch.int64), torch.full((B, L), -100)
    for p, lp in enumerate(prompt_lens):
        prompt = torch.randint(3, 31000, (lp,), generator=g)
        prompt[0] = 1
        for k in range(G):
            b, n = p * G + k, lp + n_lab + tail
            ids[b, :lp] = prompt
            ids[b, lp:n] = torch.randint(31744, 32000, (n_lab + tail,), generator=g)
            mask[b, :n] = 1
            labels[b, lp:lp + n_lab] = ids[b, lp:lp + n_lab]
    return ids, mask, labels


def check_layout(lay, ids, mask, labels):
    """Everything the layout promises, token by token, against the replicated batch."""
    sb = SP.plan_batch(lay, ids, mask, labels)
    P0, nb, S = lay.P0, lay.nb, lay.S
    assert P0 % nb == 0 and P0 >= NPAT + lay.L - nb and S == P0 + lay.G * nb and lay.text_len == S - NPAT
    assert sb.ids.shape == (lay.P, lay.text_len) and sb.key_mask.shape == (lay.P, S) and sb.targets.shape == (lay.P * S,)
    row_token = lambda r: 0 if r == 0 else r - NPAT            # the embedding splice: ids index j >= 1 sits on row NPAT + j
    tg = sb.targets.reshape(lay.P, S)
    pos = sb.pos.reshape(lay.P, S)
    for b in range(ids.shape[0]):
        p, g = divmod(b, lay.G)
        at = np.flatnonzero(labels[b].numpy() != -100)
        f, e = int(at[0]), int(at[-1])
        s = f - 1
        assert sb.split[b] == s and sb.count[b] == e - s
        # prefix: BOS, the patches, tokens [1, s) at their replicated rows and positions; the rest of the capacity hidden
        assert sb.ids[p, 0] == ids[b, 0] and np.array_equal(sb.ids[p, 1:s], ids[b, 1:s].numpy())
        assert np.array_equal(sb.key_mask[p, :NPAT + s], np.ones(NPAT + s)) and not sb.key_mask[p, NPAT + s:P0].any()
        assert np.array_equal(pos[p, :P0], np.arange(P0)) and (tg[p, :P0] == -100).all()
        # branch: tokens [s, e), each at the position the replicated layout gives it, predicting the next token
        r0 = lay.branch_row(g)
        n = e - s
        assert np.array_equal(sb.ids[p, r0 - NPAT:r0 - NPAT + n], ids[b, s:e].numpy())
        assert (sb.ids[p, r0 - NPAT + n:r0 - NPAT + nb] == 32000).all()
        assert sb.key_mask[p, r0:r0 + n].all() and not sb.key_mask[p, r0 + n:r0 + nb].any()
        assert np.array_equal(tg[p, r0:r0 + n], labels[b, f:e + 1].numpy()) and (tg[p, r0 + n:r0 + nb] == -100).all()
        assert np.array_equal(pos[p, r0:r0 + n], NPAT + np.arange(s, e))
        assert tg[p, r0] != -100 and (row_token(r0) + NPAT == r0)          # the branch starts on the row that predicts label f
        # the rows of the labelled tokens: token t is predicted by the row of token t − 1
        want = np.full(ids.shape[1], -1)
        want[f:e + 1] = p * S + r0 + np.arange(n)
        assert np.array_equal(sb.token_row[b], want)
    assert (sb.targets != -100).sum() == (labels != -100).sum()
    # no labelled row in a prefix run, and the groups of nb rows never straddle a branch boundary
    assert all((tg[:, k * nb:(k + 1) * nb] == -100).all() for k in range(P0 // nb))
    return sb


def test_ragged_prompts_in_one_batch_collator_form():
    """The collator's "last 8" SFT labels (7 action tokens + EOS, nothing behind), prompts of 12, 5 and 19 tokens."""
    L, G = 30, 3
    ids, mask, labels = grouped((12, 5, 19), G, 8, L, tail=0, seed=1)
    lay = SP.SharedPromptLayout(B=9, G=G, nb=8, L=L, n_patches=NPAT)
    assert lay.P == 3 and lay.P0 == 280 and lay.S == 304
    sb = check_layout(lay, ids, mask, labels)
    assert list(sb.split[::G]) == [11, 4, 18] and (sb.count == 8).all()


def test_policy_batch_output_for_three_samples():
    """`rl.policy_batch` for K = 3 samples of each of two prompts: 7 labelled action tokens, an unlabelled EOS behind them
    that the layout drops, branches of 7 rows that start on the empty token."""
    from bridgelang_amd.training.rl import policy_batch
    g = torch.Generator().manual_seed(3)
    K, n = 3, 7
    prompts = torch.randint(3, 31000, (2, 10), generator=g)
    prompts[:, 0], prompts[:, -1] = 1, 29871
    tokens = torch.randint(31744, 32000, (2 * K, n), generator=g)
    batch = policy_batch(prompts.repeat_interleave(K, 0), None, tokens, -torch.rand(2 * K, n, generator=g), torch.randn(2 * K, generator=g))
    l = batch["input_ids"].shape[1]
    assert l == 10 + n + 1
    lay = SP.SharedPromptLayout(B=2 * K, G=K, nb=n, L=l, n_patches=NPAT)
    sb = check_layout(lay, batch["input_ids"], batch["attention_mask"], batch["labels"])
    assert (sb.split == 9).all() and (sb.count == n).all()
    for b in range(2 * K):
        p, k = divmod(b, K)
        assert sb.ids[p, lay.branch_row(k) - NPAT] == 29871 and sb.ids[p, 9] == 32000       # the empty token opens the branch
    # a longer plan than the batch, and branches longer than the run: both pad
    lay2 = SP.SharedPromptLayout(B=2 * K, G=K, nb=8, L=l + 3, n_patches=NPAT)
    check_layout(lay2, batch["input_ids"], batch["attention_mask"], batch["labels"])


def test_row_maps_there_and_back_are_inverse():
    L, G = 24, 2
    ids, mask, labels = grouped((9, 14), G, 5, L, seed=5)
    lay = SP.SharedPromptLayout(B=4, G=G, nb=6, L=L, n_patches=NPAT)
    sb = SP.plan_batch(lay, ids, mask, labels)
    on = labels != -100
    rows_n = lay.P * lay.S
    src = torch.randn(4, L, generator=torch.Generator().manual_seed(1))
    rows = SP.tokens_to_rows(sb.token_row, src, rows_n)
    assert tuple(rows.shape) == (rows_n,) and int((rows != 0).sum()) == int(on.sum())
    assert torch.equal((rows != 0), torch.from_numpy(sb.targets != -100))                    # values sit on the labelled rows
    back = SP.rows_to_tokens(sb.token_row, rows)
    assert torch.equal(back, torch.where(on, src, torch.zeros(())))
    every = torch.arange(rows_n, dtype=torch.float32)                                        # and rows → tokens → rows
    again = SP.tokens_to_rows(sb.token_row, SP.rows_to_tokens(sb.token_row, every), rows_n)
    assert torch.equal(again, torch.where(torch.from_numpy(sb.targets != -100), every, torch.zeros(())))
    vec = torch.randn(4, L, 3, generator=torch.Generator().manual_seed(2))                  # a vector per token rides along
    assert tuple(SP.tokens_to_rows(sb.token_row, vec, rows_n).shape) == (rows_n, 3)
    bad = src.clone()
    bad[0, int(on[0].nonzero()[0])] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        SP.tokens_to_rows(sb.token_row, bad, rows_n, "old_logprobs")
    off = src.clone()
    off[~on] = float("nan")                                                                  # off the labels nothing is read
    assert torch.equal(SP.tokens_to_rows(sb.token_row, off, rows_n), rows)
    with pytest.raises(ValueError, match="shape"):
        SP.tokens_to_rows(sb.token_row, src[:, :-1], rows_n)


def test_every_refusal_fires():
    L, G = 24, 2
    ids, mask, labels = grouped((9, 14), G, 5, L, seed=7)
    lay = SP.SharedPromptLayout(B=4, G=G, nb=6, L=L, n_patches=NPAT)
    SP.plan_batch(lay, ids, mask, labels)
    with pytest.raises(ValueError, match="multiple"):                # B is not a multiple of G
        SP.SharedPromptLayout(B=5, G=2, nb=6, L=L, n_patches=NPAT)
    with pytest.raises(ValueError, match="multiple"):
        SP.plan_batch(lay, ids[:3], mask[:3], labels[:3])
    x = ids.clone()
    x[1, 4] += 1
    with pytest.raises(ValueError, match="ids or mask differ"):      # ids before s differ inside a group
        SP.plan_batch(lay, x, mask, labels)
    m = mask.clone()
    m[3, 2] = 0
    with pytest.raises(ValueError, match="ids or mask differ"):      # mask before s differs inside a group
        SP.plan_batch(lay, ids, m, labels)
    lab = labels.clone()
    lab[0] = torch.roll(lab[0], 1)
    with pytest.raises(ValueError, match="split at"):                # split points differ inside a group
        SP.plan_batch(lay, ids, mask, lab)
    lab = labels.clone()
    lab[2, int((labels[2] != -100).nonzero()[2])] = -100
    with pytest.raises(ValueError, match="contiguous"):              # a hole in the run
        SP.plan_batch(lay, ids, mask, lab)
    lab = labels.clone()
    lab[1] = -100
    with pytest.raises(ValueError, match="contiguous"):              # no label at all
        SP.plan_batch(lay, ids, mask, lab)
    with pytest.raises(ValueError, match="more than branch_len"):    # the run is longer than nb
        SP.plan_batch(SP.SharedPromptLayout(B=4, G=G, nb=4, L=L, n_patches=NPAT), ids, mask, labels)
    # the prefix exceeds P0: a long prompt with a short run, where the capacity assumes full branches
    ids2, mask2, labels2 = grouped((22, 22), G, 1, L, tail=0, seed=8)
    lay2 = SP.SharedPromptLayout(B=4, G=G, nb=8, L=L, n_patches=NPAT)
    assert lay2.P0 == 272
    with pytest.raises(ValueError, match="exceeds the capacity"):
        SP.plan_batch(lay2, ids2, mask2, labels2)
    lab = torch.full_like(labels, -100)
    lab[:, 1:4] = ids[:, 1:4]
    with pytest.raises(ValueError, match="token 2 or later"):        # the branch would start on BOS
        SP.plan_batch(lay, ids, mask, lab)
    with pytest.raises(ValueError, match="tree_visible"):
        SP.tree_visible(10, 4, 21)


@pytest.mark.parametrize("case", ["collator", "policy", "short-runs"])
def test_cut_out_of_the_tree_is_the_replicated_causal_mask(case):
    """Each sequence of a group, cut out of the tree (prefix rows plus its branch) without the masked rows: exactly the causal
    mask of the replicated sequence up to its last labelled token's predecessor, at the replicated positions."""
    L, G = 26, 3
    n_lab, tail, nb = {"collator": (8, 0, 8), "policy": (7, 1, 7), "short-runs": (3, 1, 8)}[case]
    ids, mask, labels = grouped((10, 6), G, n_lab, L, tail=tail, seed=11)
    lay = SP.SharedPromptLayout(B=2 * G, G=G, nb=nb, L=L, n_patches=NPAT)
    sb = SP.plan_batch(lay, ids, mask, labels)
    for b in range(2 * G):
        rows, vis, pos = SP.cut_out(lay, sb, b)
        e = int((labels[b] != -100).nonzero()[-1])
        n = NPAT + e                                               # replicated rows 0 … NPAT + e − 1: BOS, patches, tokens [1, e)
        assert len(rows) == n
        assert np.array_equal(vis, np.tril(np.ones((n, n), dtype=bool)))
        assert np.array_equal(pos, np.arange(n))                   # replicated position = replicated row
        # and the tokens on those rows are the replicated sequence's
        p = b // G
        toks = [int(sb.ids[p, 0])] + [int(sb.ids[p, r - NPAT]) for r in rows if r > NPAT]
        assert toks == ids[b, :e].tolist()
    # across branches nothing is visible, inside the prefix everything causal is
    full = SP.tree_visible(lay.P0, nb, lay.S)
    r0, r1 = lay.branch_row(0), lay.branch_row(1)
    assert not full[r1:r1 + nb, r0:r0 + nb].any() and full[r1, :lay.P0].all() and not full[lay.P0 - 1, lay.P0:].any()
    assert np.array_equal(SP.tree_visible(5, 3, 8), np.tril(np.ones((8, 8), dtype=bool)))   # G = 1: plain causal


def test_entry_points_are_declared_bound_exported_and_wrapped():
    from bridgelang_amd import _lib, train_ops
    header = (ROOT / "include" / "bridgelang_hip.h").read_text()
    declared = set(re.findall(r"\b(bl_[a-z0-9_]+)\s*\(", header))
    i32, i64, vp, desc = C.c_int32, C.c_int64, C.c_void_p, C.POINTER(_lib.AttnDesc)
    want = {"bl_attention_tree_lse_bf16": ([desc, i32, i32, vp, vp], ["d", "prefix", "branch", "lse", "stream"]),
            "bl_attention_tree_backward_bf16": ([desc, i32, i32, vp, vp, vp, vp, vp, vp, vp],
                                                ["d", "prefix", "branch", "dout", "lse", "delta", "dq", "dk", "dv", "stream"]),
            "bl_rope_pos_bf16": ([vp, i64, i64, i32, i32, vp, vp, vp, vp],
                                 ["qkv", "ld", "rows", "H", "head_dim", "cos_tab", "sin_tab", "pos", "stream"]),
            "bl_rope_pos_backward_bf16": ([vp, i64, i64, i32, i32, vp, vp, vp, vp],
                                          ["dqkv", "ld", "rows", "H", "head_dim", "cos_tab", "sin_tab", "pos", "stream"])}
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.fullmatch(r"bl_[a-z0-9_]+", line.split()[-1])}
    lib = _lib.load()
    for name, (args, names) in want.items():
        assert name in declared and f"int {name}(" in header and name in exported and hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == (C.c_int, args), name
        proto = re.search(rf"int {name}\(([^;]*)\);", header).group(1)
        assert [a.split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")] == names, name
    assert declared == set(_lib.SIGNATURES) == exported, (declared ^ exported, declared ^ set(_lib.SIGNATURES))
    for fn in ("attention_tree_lse", "attention_tree_backward", "rope_pos", "rope_pos_backward"):
        assert callable(getattr(train_ops, fn))
    assert "attention_tree.hip" in (ROOT / "bridgelang_amd" / "csrc" / "Makefile").read_text()
    assert "bl_attention_tree_lse_bf16" in (ROOT / "INTEGRATION.md").read_text()
