"""The shared-prompt attention pair (attention_tree.hip) where it SKIPS work, at the shapes tests/test_attention_tree_gpu.py
does not reach: past 512 rows (a dq workgroup drops whole 256-key chunks, the forward drops runs of 64-key chunks, a dkv
workgroup walks three to eight 256-row chunks and starts at chunk 512 and later), branches of 56 to 300 rows (a branch spans
16-row wave tiles, 64-row query tiles, 128-row blocks and a 256-row chunk, so wave_lo / blk_lo / wave_hi / blk_hi are
evaluated for tiles in the middle of a branch), and key masks that hide whole chunks and steps.

Every output element against the fp64 reference of tests/attn_ref64.py under shared_prompt.tree_visible, through the helpers
of tests/test_attention_tree_gpu.py (check_case: fused qkv / dqkv rows, guard rows, sentinels) with its comparators and
constants C_O, C_DV, C_DQ, C_DK, LSE_REL, FLOOR unchanged; B = 2, H = 2, hd = 128, flat and peaked scores, nothing excluded
but masked query rows. The fp64 comparison is the check that a skip bound does not DROP a visible key; the bit comparison
under ±3e4 in every row that must not be read is the check that it does not let a tile SEE a neighbour.

Which path each shape reaches is counted by the host model tests/tree_paths.py (LONG_CASES) and asserted without a GPU in
tests/test_tree_paths_cpu.py, together with the precondition |s'| <= 64 of the error model for the inputs of every check
listed in CHECKS below.
"""
import pytest
import torch

import tree_paths
from conftest import rand_bf16
from test_attention_tree_gpu import B, H, HD, _mask, check_case, run_tree

pytestmark = pytest.mark.gpu

LONG = list(tree_paths.LONG_CASES)

# every check_case call of this file: name → (prefix, branch, G, keywords of _mask (None: key_mask = NULL), seed)
CHECKS = {f"p{p}-nb{nb}-G{g}-{form}": (p, nb, g, {}, 9000 + 20 * i + (5 if form == "peaked" else 0))
          for i, (p, nb, g) in enumerate(LONG) for form in ("flat", "peaked")}
MASKED_CHUNK = (288, 8, 32, dict(hide_prefix=(0, 130)))
SHORT_LONG = (40, 100, 5, dict(hide_prefix=(2, 5), short=37))
CHECKS.update({
    "masked-chunk-flat": MASKED_CHUNK + (9400,), "masked-chunk-peaked": MASKED_CHUNK + (9405,),
    "short-long-branches-flat": SHORT_LONG + (9420,), "short-long-branches-peaked": SHORT_LONG + (9425,),
    "repeat-peaked": (1, 8, 112, {}, 9440),
    "nan-stat-padding-flat": (33, 7, 100, {}, 9460), "nan-stat-padding-peaked": (33, 7, 100, {}, 9465),
    "no-mask-flat": (256, 8, 33, None, 9480), "no-mask-peaked": (256, 8, 33, None, 9485),
})


def check_mask(name):
    prefix, branch, G, mk, _ = CHECKS[name]
    return None if mk is None else _mask(prefix, branch, G, **mk)


def _check(dev, name, **kw):
    prefix, branch, G, _, seed = CHECKS[name]
    return check_case(dev, prefix, branch, G, check_mask(name), seed, name.endswith("peaked"), name, **kw)


@pytest.mark.parametrize("form", ("flat", "peaked"))
@pytest.mark.parametrize("prefix,branch,G", LONG, ids=[f"p{p}-nb{nb}-G{g}" for p, nb, g in LONG])
def test_long_tree_against_fp64(dev, prefix, branch, G, form):
    """The default mask (the last 3 prefix rows of batch element 1 hidden) at every shape of tree_paths.LONG_CASES."""
    if (prefix, branch, G) == (272, 8, 64):          # the numbers of the training step's own layout, taken from it
        from bridgelang_amd.training.shared_prompt import SharedPromptLayout
        lay = SharedPromptLayout(B=64, G=64, nb=8, L=22, n_patches=256)
        assert (lay.P0, lay.nb, lay.G, lay.S) == (prefix, branch, G, 784)
    _check(dev, f"p{prefix}-nb{branch}-G{G}-{form}")


@pytest.mark.parametrize("form", ("flat", "peaked"))
def test_fully_masked_chunk_in_the_middle(dev, form):
    """Batch element 1 hides keys 158..287 of a 288-row prefix: the forward's chunk [192, 256) and four 32-key steps of the
    backward contribute nothing although every branch query sees them by position. Same bounds; the hidden keys get exactly
    zero dk / dv."""
    prefix, branch, G, _, _ = CHECKS[f"masked-chunk-{form}"]
    mask = check_mask(f"masked-chunk-{form}")
    assert not bool(mask[1, 158:288].any()) and bool(mask[1, :158].all()) and bool(mask[0].all())
    n = tree_paths.masked_paths(prefix, branch, G, mask[1].numpy())
    assert n["fwd_chunks"] >= 1 and n["dq_steps"] >= 1, n
    _, _, _, _, got = _check(dev, f"masked-chunk-{form}")
    for t in ("dk", "dv"):
        assert bool((got[t][1, :, 158:288] == 0).all()), f"{t}: hidden prefix keys got gradient"


@pytest.mark.parametrize("form", ("flat", "peaked"))
def test_short_long_branches(dev, form):
    """Branches of 100 rows of which the last 37 are padding, beside a hidden prefix tail: the rows at which a branch ends for
    the mask are not those at which it ends for the skip bounds. check_case holds masked keys to zero gradient."""
    _check(dev, f"short-long-branches-{form}")


@pytest.mark.parametrize("g", (50, 99), ids=("middle-branch", "last-branch"))
def test_rows_that_must_not_be_read(dev, g):
    """(33, 7, 100): the prefix and ONE branch are compared; every other branch's K / V and the masked prefix tail hold ±3e4.
    Not a bit of o / dq / dk / dv of the compared rows may change."""
    prefix, branch, G = 33, 7, 100
    S = prefix + G * branch
    mask = _mask(prefix, branch, G, hide_prefix=(0, 4))
    q, k, v = (rand_bf16((B, H, S, HD), 9500 + 10 * g + i) for i in range(3))
    keep = torch.zeros(B, S, dtype=torch.bool)
    keep[:, :prefix] = True
    keep[:, prefix + g * branch:prefix + (g + 1) * branch] = True
    keep &= mask.bool()
    do = rand_bf16((B, H, S, HD), 9500 + 10 * g + 4) * keep.view(B, 1, S, 1)
    hide = ~keep                                                       # every other branch, and the masked prefix tail
    big = 3.0e4 * (torch.randint(0, 2, k.shape, generator=torch.Generator().manual_seed(2)) * 2 - 1).float()
    sel = hide.view(B, 1, S, 1)
    base = run_tree(dev, q, k, v, mask, prefix, branch, do)
    pert = run_tree(dev, q, torch.where(sel, big, k), torch.where(sel, -big, v), mask, prefix, branch, do)
    rows = keep.view(B, 1, S, 1).expand(B, H, S, HD)
    assert int(hide.sum()) == B * (G - 1) * branch + 4
    for t in ("o", "dq", "dk", "dv"):
        assert bool(torch.isfinite(base[t][rows]).all()) and bool(base[t][rows].abs().sum() > 0), f"{t}: nothing to compare"
        assert torch.equal(base[t][rows], pert[t][rows]), f"{t}: changed when rows that must not be read were overwritten"


def test_repeatability(dev):
    """(1, 8, 112), two skipped dq chunks in one block: a second call over the same inputs gives identical bits."""
    prefix, branch, G, _, _ = CHECKS["repeat-peaked"]
    q, k, v, do, got = _check(dev, "repeat-peaked")
    again = run_tree(dev, q, k, v, check_mask("repeat-peaked"), prefix, branch, do)
    for t in ("o_bits", "lse_bits", "d_bits"):
        assert torch.equal(got[t], again[t]), f"{t}: two calls differ"
    assert torch.equal(got["delta"].view(torch.int32), again["delta"].view(torch.int32)), "delta: two calls differ"


@pytest.mark.parametrize("form", ("flat", "peaked"))
def test_stat_padding_is_never_used(dev, form):
    """S = 733, pad32 = 736: lse and delta hold NaN before the call. The forward and dq write rows < S only, so the three pad
    rows still hold NaN when dkv loads them four at a time; nothing of them may reach an output."""
    prefix, branch, G, _, _ = CHECKS[f"nan-stat-padding-{form}"]
    assert (prefix + G * branch, (prefix + G * branch + 31) // 32 * 32) == (733, 736)
    _, _, _, _, got = _check(dev, f"nan-stat-padding-{form}", stat_fill=float("nan"))
    for t in ("o", "lse", "dq", "dk", "dv", "delta"):
        assert not bool(torch.isnan(got[t]).any()), f"{t}: NaN in an output"
    for t in ("lse_pad", "delta_pad"):
        assert got[t].shape[-1] == 3 and bool(torch.isnan(got[t]).all()), f"{t}: a pad row was written"


@pytest.mark.parametrize("form", ("flat", "peaked"))
def test_no_key_mask(dev, form):
    """key_mask = NULL at (256, 8, 33), the smallest dq block skip."""
    assert check_mask(f"no-mask-{form}") is None
    _check(dev, f"no-mask-{form}")
