"""`rl.policy_batch(values=, returns=)`: the critic's rollout values and GAE's returns ride the training batch as
`old_values` / `returns` for `TrainStep.set_value_batch`; without them the batch is the one it was. And the new entry point
`bl_value_predict_f32` is declared alike in the header, the ctypes table and the ABI table of INTEGRATION.md."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from bridgelang_amd.training.rl import gae, policy_batch

ROOT = Path(__file__).resolve().parent.parent
BASE_KEYS = ["input_ids", "attention_mask", "labels", "advantages", "old_logprobs"]


def rollout(B=3, lp=6, n=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 31000, (B, lp), generator=g)
    ids[:, 0] = 1
    mask = torch.ones(B, lp, dtype=torch.long)
    ids[1, 4:], mask[1, 4:] = 32000, 0
    tok = torch.randint(31744, 32000, (B, n), generator=g)
    return ids, mask, tok, -torch.rand(B, n, generator=g), torch.randn(B, generator=g)


def test_values_and_returns_add_exactly_two_keys():
    ids, mask, tok, lp, adv = rollout()
    v, R = np.array([0.25, -1.5, 3.0], dtype=np.float32), torch.tensor([1.0, 2.0, -0.5], dtype=torch.float64)
    plain = policy_batch(ids, mask, tok, lp, adv)
    both = policy_batch(ids, mask, tok, lp, adv, values=v, returns=R)
    assert list(plain) == BASE_KEYS and list(both) == BASE_KEYS + ["old_values", "returns"]
    for k in BASE_KEYS:
        assert both[k].dtype == plain[k].dtype and torch.equal(both[k], plain[k]), k
    assert both["old_values"].dtype == torch.float32 and torch.equal(both["old_values"], torch.from_numpy(v))
    assert both["returns"].dtype == torch.float32 and torch.equal(both["returns"], R.float())
    assert list(policy_batch(ids, mask, tok, lp, adv, values=v)) == BASE_KEYS + ["old_values"]
    assert list(policy_batch(ids, mask, tok, lp, adv, returns=R)) == BASE_KEYS + ["returns"]


def test_without_them_the_batch_is_todays():
    ids, mask, tok, lp, adv = rollout(seed=1)
    a, b = policy_batch(ids, mask, tok, lp, adv, pad_to=20, token_range=(31744, 256)), \
        policy_batch(ids, mask, tok, lp, adv, pad_to=20, token_range=(31744, 256), values=None, returns=None)
    assert list(a) == list(b) == BASE_KEYS and all(torch.equal(a[k], b[k]) for k in a)
    # the layout itself: prompt | 29871 | n action tokens | EOS, labels on the action tokens alone
    assert a["input_ids"].shape == (3, 20) and int(a["input_ids"][1, 4]) == 29871 and int(a["input_ids"][1, 12]) == 2
    assert torch.equal(a["labels"][1, 5:12], tok[1]) and int((a["labels"][1] != -100).sum()) == 7


@pytest.mark.parametrize("name", ["values", "returns"])
def test_wrong_shape_or_non_finite_is_rejected(name):
    ids, mask, tok, lp, adv = rollout()
    for bad in (torch.zeros(4), torch.zeros(3, 7), torch.zeros(3, 1), torch.tensor(1.0),
                torch.tensor([0.0, float("nan"), 1.0]), torch.tensor([0.0, float("inf"), 1.0])):
        with pytest.raises(ValueError):
            policy_batch(ids, mask, tok, lp, adv, **{name: bad})


def test_rollout_values_feed_gae():
    """The loop the feature closes: V(s_t) from the rollout → gae → the batch's returns / old_values."""
    v = torch.tensor([[0.5, 0.25, -0.125]])
    adv, ret = gae(torch.tensor([[1.0, 0.0, 2.0]]), v, gamma=0.5, lam=1.0)
    assert torch.equal(ret, adv + v)
    ids, mask, tok, lp, _ = rollout()
    batch = policy_batch(ids, mask, tok, lp, adv.reshape(-1), values=v.reshape(-1), returns=ret.reshape(-1))
    assert torch.equal(batch["old_values"], v.reshape(-1)) and torch.equal(batch["returns"], ret.reshape(-1))


def test_value_predict_is_declared_alike_everywhere():
    from bridgelang_amd import _lib
    header = (ROOT / "include" / "bridgelang_hip.h").read_text()
    m = re.search(r"int bl_value_predict_f32\(([^;]*)\);", header)
    assert m, "bl_value_predict_f32 is not declared in include/bridgelang_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    table = next(v for k, v in vars(_lib).items() if isinstance(v, dict) and "bl_value_head_f32" in v)
    restype, argtypes = table["bl_value_predict_f32"]
    assert len(argtypes) == len(params) == 11
    import ctypes as C
    for p, t in zip(params, argtypes):
        want = C.c_void_p if "*" in p else C.c_int64 if p.startswith("int64_t") else C.c_int32 if p.startswith("int32_t") else C.c_float
        assert t is want, (p, t)
    assert "`bl_value_predict_f32`" in (ROOT / "INTEGRATION.md").read_text()
    src = (ROOT / "bridgelang_amd" / "csrc" / "value.hip").read_text()
    assert re.search(r'extern "C" int bl_value_predict_f32\(', src)
