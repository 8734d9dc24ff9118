"""The policy and preference loss kernels (csrc/policy.hip) per element against the fp64 references and derived bounds of
tests/policy_ref64.py, at the smallest shapes at which each loop, switch and reduction can still go wrong. The cases are
policy_ref64's (forward_cases, backward_cases, pref_cases); tests/test_policy_ref_cpu.py shows on the same cases that an fp32
evaluation stays inside every bound and that the comparator rejects thirteen planted near-misses.

Scaffolding. Every buffer a kernel reads or writes is a glue_ref.Flat: a dense block between NaN guard elements. The logits
and dlogits are [rows, ld] blocks whose logical part is the first n columns. After a call the WHOLE allocation of every
output is checked (window_intact: guards and row padding still hold the sentinel), every logical element must be finite
and inside its bound, and an element whose bound is 0 (ignored rows, 0/1 outputs, counts, zero columns, spare slots, the
rows [P, cap) of pair_stats) must be equal. Every case runs twice: with finite filler in everything the header calls never
read (logits of ignored rows, columns outside the token range, the ld padding, adv / old_lp / ref_lp / mu of ignored rows),
and with NaN there; the two runs' allocations must agree bit for bit.

Branch → case
  policy_rows_kernel (stride 1024)   n 8, 1024, 1032, 2056 x T 0.5, 1, 2, ld = n and n + 8; n 32064 x 8 rows. Rows: maximum and
      target in the first / last float4, in another wave, in the second trip; all equal; peaked on / off the target (60);
      ±80 (exp underflows at T 0.5, 0·d = 0)                                                       test_policy_forward[rows-*]
  policy_rows_wave_kernel and the switch   count 8, 248, 256 (wave), 264 (workgroup) x first 0, 8, n − count x rows 1, 4, 5
                                                                                                   test_policy_forward[range-*]
      ranged (0, n) == unranged and wave == workgroup on <= 256 columns, bit for bit              test_range_and_wave_bit_identity
  policy_group_kernel   group_rows 1, 7, 64, 65 x groups 1, 4, 5 x both norms: an empty group, row 0 ignored, only row 64 valid;
      clipped high / low / inside with A of both signs and 0 in one group                          test_policy_forward[group-*]
  bl_policy_loss_is_f32   both levels x proximal given / self x cap 2 / inf x no mask / (0.5, 3)  test_policy_forward[is-*]
  stats_body (stride 256 rows)   rows 1, 256, 257; every row ignored (zeros, and the backward writes zeros)
                                                                                                   test_policy_forward[stats-*]
  policy_backward_kernel (stride 2048)   in isolation from rounded reference row values (the four columns it does not read
      are NaN): n 8, 2048, 2056; ranges ending at n / starting at 0 / one group; ldd = n, n + 8; entropy_coef 0, 0.01; g = 0;
      peaked rows; stats[1] 1, 16                                                                  test_policy_backward
      chained after every forward case, against the sum of both bounds                             test_policy_forward, test_preference
  bl_preference_loss_f32   3 kinds x 2 norms x with / without reference (label_smoothing 0 / 0.1, sft_coef 0 / 0.5); capacity 1,
      256, 257; the device pair count below the capacity; an id beyond ±P; two chosen sequences; a sequence in no pair;
      both row kernels; the backward with stats[1] = P                                             test_preference
  a target inside [0, n) but outside the range: NaN logp, the row's m, log S, H unchanged, sentinels intact
                                                                                                   test_target_outside_the_range

The largest err / bound per output on MI355X is recorded in DESIGN.md (policy_ref64.RATIOS, printed by the last test).
"""
import numpy as np
import pytest
import torch

import glue_ref as G
import policy_ref64 as P64
from glue_ref import Flat
from policy_ref64 import IGN
from test_policy_ref_cpu import BWD, FWD, PREF, ids, ref_of

pytestmark = pytest.mark.gpu
bf16, f32, i32 = torch.bfloat16, torch.float32, torch.int32
NAN = float("nan")


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_error(dev):
    """A HIP error (an illegal access, say) ends the session: no further kernel is launched on a device in that state."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


def logits_block(dev, logits, tgt, rng, pad, poison):
    """[rows, n + pad] between guards; what is never read holds NaN (poison) or a finite filler."""
    rows, n = logits.shape
    first, count = rng or (0, n)
    fill = NAN if poison else 3.0
    block = torch.full((rows, n + pad), fill, dtype=f32)
    block[:, first:first + count] = torch.from_numpy(logits[:, first:first + count])
    block[torch.from_numpy(tgt == IGN)] = fill
    return Flat((rows, n + pad), dev, f32, data=block)


def per_row(dev, x, tgt, poison):
    if x is None:
        return None
    t = torch.from_numpy(np.asarray(x, dtype=np.float32)).clone()
    t[torch.from_numpy(tgt == IGN)] = NAN if poison else 0.25
    return t.to(dev)


def backward_into(dev, L, n, tgt_d, rs, st, cfg, pad):
    from bridgelang_amd import train_ops as T
    dl = Flat((L.shape[0], n + pad), dev, bf16)
    T.policy_loss_backward(L.v[:, :n], tgt_d, rs, st, dl.v[:, :n], cfg)
    return dl


def run_policy(dev, c, poison):
    from bridgelang_amd import train_ops as T
    rows, n = c.logits.shape
    L = logits_block(dev, c.logits, c.tgt, c.cfg.token_range, c.pad, poison)
    tgt_d = torch.from_numpy(c.tgt).to(dev)
    out = dict(rs=Flat((rows, 8), dev, f32), st=Flat((8,), dev, f32))
    kw = {}
    if c.group_rows:
        out["gs"] = Flat((rows // c.group_rows, 4), dev, f32)
        kw.update(group_rows=c.group_rows, group_stats=out["gs"].v)
    if c.mu is not None:
        out["ir"], out["ist"] = Flat((rows, 2), dev, f32), Flat((8,), dev, f32)
        kw.update(behaviour_logprob=per_row(dev, c.mu, c.tgt, poison), is_rows=out["ir"].v, is_stats=out["ist"].v)
    T.policy_loss(L.v[:, :n], tgt_d, per_row(dev, c.A, c.tgt, poison), per_row(dev, c.q, c.tgt, poison), per_row(dev, c.ref, c.tgt, poison),
                  out["rs"].v, out["st"].v, c.cfg, **kw)
    out["dl"] = backward_into(dev, L, n, tgt_d, out["rs"].v, out["st"].v, c.cfg, 8 - c.pad)
    torch.cuda.synchronize()
    return out


def intact(out, n):
    for k, x in out.items():
        P64.window_intact(x, n if k == "dl" else x.shape[-1], k)


def host(x):
    return x.v.detach().float().cpu().numpy().astype(np.float64)


def forward_outputs(out):
    got = P64.split_row_stats(host(out["rs"]))
    got["stats"] = host(out["st"])
    for k, name in (("gs", "group_stats"), ("ir", "is_rows"), ("ist", "is_stats"), ("ps", "pair_stats"), ("ss", "seq_stats")):
        if k in out:
            got[name] = host(out[k])
    return got


def same_bits(a, b, what):
    for k in a:
        G.assert_bits(a[k], b[k], f"{what} {k}: NaN in what is never read changed the output")


@pytest.mark.parametrize("c", FWD, ids=ids(FWD))
def test_policy_forward(dev, c):
    ref, fwd = ref_of(c)
    n = c.logits.shape[1]
    clean, poisoned = run_policy(dev, c, False), run_policy(dev, c, True)
    intact(poisoned, n)
    level = c.name.split("-")[0] + " "
    P64.check(forward_outputs(poisoned), ref, c.name, tag=level)
    dl = host(poisoned["dl"])[:, :n]
    P64.check({"dlogits": dl}, P64.chained_reference(c, fwd), c.name + " chained", tag="chained ")
    same_bits(clean, poisoned, c.name)
    v = c.tgt != IGN
    first, count = c.cfg.token_range or (0, n)
    assert (dl[~v] == 0).all() and (dl[:, :first] == 0).all() and (dl[:, first + count:] == 0).all()
    if c.mu is not None:
        assert (host(poisoned["ir"])[~v] == 0).all() and (host(poisoned["ist"])[6:] == 0).all()
        if c.q is None:                                  # self-proximal: the ratio is 1.0f, every row active
            rs = host(poisoned["rs"])
            assert (rs[v, 2] == 1.0).all() and (rs[:, 4] == 0).all()


@pytest.mark.parametrize("b", BWD, ids=ids(BWD))
def test_policy_backward(dev, b):
    rows, n = b.logits.shape
    for poison in (False, True):
        L = logits_block(dev, b.logits, b.tgt, b.cfg.token_range, 8 - b.pad, poison)
        rs = torch.full((rows, 8), NAN, dtype=f32)       # logp, ratio, row_loss and clipped are not the backward's to read
        for col, x in ((1, b.H), (5, b.m), (6, b.logS), (7, b.g)):
            rs[:, col] = torch.from_numpy(x)
        rs[torch.from_numpy(b.tgt == IGN)] = NAN if poison else 0.0
        st = torch.full((8,), NAN, dtype=f32)
        st[1] = b.nv
        dl = backward_into(dev, L, n, torch.from_numpy(b.tgt).to(dev), rs.to(dev), st.to(dev), b.cfg, b.pad)
        torch.cuda.synchronize()
        P64.window_intact(dl, n, b.name)
        P64.check({"dlogits": host(dl)[:, :n]}, P64.backward_reference(b), b.name, tag="isolated ")
        if poison:
            G.assert_bits(dl, first, f"{b.name}: NaN in what is never read changed dlogits")
        first = dl


def run_preference(dev, c, poison):
    from bridgelang_amd import train_ops as T
    rows, n = c.logits.shape
    L = logits_block(dev, c.logits, c.tgt, c.cfg.token_range, c.pad, poison)
    tgt_d = torch.from_numpy(c.tgt).to(dev)
    out = dict(rs=Flat((rows, 8), dev, f32), st=Flat((8,), dev, f32), ps=Flat((c.cap, 4), dev, f32), ss=Flat((rows // c.group_rows, 4), dev, f32))
    npd = None if c.P_dev is None else torch.tensor([c.P_dev], dtype=i32, device=dev)
    T.preference_loss(L.v[:, :n], tgt_d, torch.from_numpy(c.pair).to(dev), per_row(dev, c.ref, c.tgt, poison), out["rs"].v, out["st"].v,
                      out["ps"].v, out["ss"].v, c.cfg, group_rows=c.group_rows, n_pairs=npd)
    out["dl"] = backward_into(dev, L, n, tgt_d, out["rs"].v, out["st"].v, c.cfg.backward_config(), 8 - c.pad)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("c", PREF, ids=ids(PREF))
def test_preference(dev, c):
    ref, fwd = ref_of(c)
    n = c.logits.shape[1]
    clean, poisoned = run_preference(dev, c, False), run_preference(dev, c, True)
    intact(poisoned, n)
    P64.check(forward_outputs(poisoned), ref, c.name, tag="pref ")
    dl = host(poisoned["dl"])[:, :n]
    P64.check({"dlogits": dl}, P64.chained_reference(c, fwd), c.name + " chained", tag="pref chained ")
    same_bits(clean, poisoned, c.name)
    assert (host(poisoned["ps"])[c.P:] == 0).all() and host(poisoned["st"])[1] == c.P
    unpaired = np.repeat(fwd.e.pair == 0, c.group_rows)
    assert (dl[unpaired] == 0).all() and np.abs(dl[~unpaired]).max() > 0


@pytest.mark.parametrize("n", [8, 256, 264, 1032])
def test_range_and_wave_bit_identity(dev, n):
    """policy.hip:207-208: the ranged entry at (0, n) gives the unranged entry's bits; up to 256 columns that is the wave
    kernel against the workgroup kernel on the same rows."""
    import dataclasses
    L, tgt = P64.edge_rows(n, n)
    c = P64.policy_case(f"ident-{n}", L, tgt, P64.PL.PolicyLossConfig(temperature=0.5, **P64.POLICY), n, pad=8)
    r = dataclasses.replace(c.cfg, token_range=(0, n))
    a = run_policy(dev, c, True)
    b = run_policy(dev, P64.NS(**{**c.__dict__, "cfg": r}), True)
    for k in ("rs", "st", "dl"):
        G.assert_bits(a[k], b[k], f"n = {n}: ranged (0, n) against unranged, {k}")
    assert np.isfinite(host(a["rs"])).all()


def test_target_outside_the_range(dev):
    """A target inside [0, n) but outside the token range: logp is NaN and nothing is read for it — the row's m, log S and H are
    those of the same row with a target inside the range, and no sentinel moves."""
    L, tgt = P64.edge_rows(8, 3)
    Lw, tw = P64.embed(L, tgt, 32, 8, 4)
    c = P64.policy_case("outside", Lw, tw, P64.PL.PolicyLossConfig(temperature=1.0, token_range=(8, 8), **P64.POLICY), 5)
    inside = run_policy(dev, c, True)
    for stray in (7, 16, 0, 31):
        t = c.tgt.copy()
        t[1] = stray
        out = run_policy(dev, P64.NS(**{**c.__dict__, "tgt": t}), True)
        intact(out, 32)
        rs, rs0 = host(out["rs"]), host(inside["rs"])
        assert np.isnan(rs[1, 0]) and np.array_equal(rs[1, [1, 5, 6]], rs0[1, [1, 5, 6]])
        keep = np.arange(16) != 1
        assert np.array_equal(rs[keep], rs0[keep])


def test_report_largest_ratios():
    """Not a check of its own: prints the largest err / bound per output that the tests above recorded (each was <= 1)."""
    for k in sorted(P64.RATIOS):
        print(f"policy_ref64: {k}: largest err/bound {P64.RATIOS[k]:.4f}")
    assert all(v <= 1.0 for v in P64.RATIOS.values())
