"""The sampling specification (bridgelang_amd/sampling.py) on the CPU: Philox known answers, the accuracy of `exp_spec`,
the kept set against transformers' own logits warpers, the drawn distribution, the edge rules, and the server's handling
of per-request settings with a stand-in model. The device kernel is held to this specification bit for bit in
tests/test_sampling_gpu.py."""
import threading

import numpy as np
import pytest
import torch

from bridgelang_amd import sampling as S
from bridgelang_amd import serve

V = 32064
GRID = [(T, k, p) for T in (0.5, 1.0, 2.0) for k in (0, 8, 50) for p in (0.5, 0.9, 0.95, 1.0)]


def bf16_logits(seed, n=V, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(torch.bfloat16).float().numpy()


# ---- RNG ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    """Random123's kat_vectors for philox4x32-10."""
    assert " ".join(f"{int(v):08x}" for v in S.philox4x32_10(counter, key)) == want


def test_draw_uses_seed_words_as_key_and_step_as_counter():
    seed = 0xa99f31d0a4093822
    x = S.philox4x32_10((5, 0, 0, 0), (0xa4093822, 0xa99f31d0))
    assert int(S.draw_u64(seed, 5)) == (int(x[0]) << 32) | int(x[1])
    assert int(S.draw_u64(np.array([seed - (1 << 64)], dtype=np.int64), 5)[0]) == int(S.draw_u64(seed, 5))    # int64 bit pattern
    rng = np.random.default_rng(3)
    for a, b in rng.integers(0, 1 << 63, (200, 2)).tolist() + [[(1 << 64) - 1, (1 << 64) - 1], [0, 5]]:
        assert int(S.mulhi64(a, b)) == (a * b) >> 64


# ---- exp ---------------------------------------------------------------------------------------------------------------
def test_exp_spec_accuracy():
    """Max relative error against fp64 exp over a seeded 2 M-point sweep of [-87, 0]: MEASURED 2.473e-7 (degree-6 Taylor
    after Cody–Waite reduction; the truncation term alone is 0.347^7 / 5040 = 1.2e-7). The bound is that value plus one
    fp32 ulp (1.2e-7)."""
    x = (-87.0 * np.random.default_rng(0).random(2_000_000)).astype(np.float32)
    ref = np.exp(x.astype(np.float64))
    err = float(np.max(np.abs(S.exp_spec(x).astype(np.float64) - ref) / ref))
    print(f"exp_spec max relative error {err:.4e}")
    assert err <= 2.473e-7 + 1.2e-7
    assert S.exp_spec(np.float32(0.0)) == 1.0 and S.weights(np.zeros(4, np.float32), 1.0).tolist() == [S.WEIGHT_ONE] * 4
    assert S.exp_spec(np.float32(-1000.0)) == S.exp_spec(np.float32(-87.0)) > 0          # clamped, still a normal number
    assert np.rint(S.exp_spec(np.float32(-87.0)) * np.float32(S.WEIGHT_ONE)) == 0          # …whose weight is 0


# ---- kept set against transformers ---------------------------------------------------------------------------------------
def test_kept_set_matches_hf_warpers():
    """200 seeded cases over the grid, V = 32 064 bf16-rounded logits. Among the tokens of non-zero weight the kept COUNT
    equals HF's in every case, and the two sets differ only in tokens whose logit equals the lowest kept logit
    (torch.sort is not stable: HF breaks boundary ties arbitrarily, the specification by index)."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    exact = 0
    for case in range(200):
        T, k, p = GRID[case % len(GRID)]
        l = bf16_logits(1000 + case)
        scores = TemperatureLogitsWarper(T)(None, torch.from_numpy(l)[None])
        if k:
            scores = TopKLogitsWarper(k)(None, scores)
        scores = TopPLogitsWarper(p)(None, scores)
        positive = S.weights(l, T) > 0
        hf = np.isfinite(scores[0].numpy()) & positive
        ours = S.kept_weights(l, T, k, p) > 0
        assert not np.any(ours & ~positive)
        assert ours.sum() == hf.sum(), f"case {case} (T={T}, k={k}, p={p}): kept {ours.sum()} tokens, HF {hf.sum()}"
        diff = ours ^ hf
        assert np.all(l[diff] == l[ours].min()), f"case {case} (T={T}, k={k}, p={p}): sets differ away from the boundary ties"
        exact += not diff.any()
    print(f"kept set identical to HF's in {exact} of 200 cases; the rest differ in boundary ties only")


# ---- the drawn distribution ----------------------------------------------------------------------------------------------
def test_empirical_distribution_within_five_sigma():
    l = np.array([1.5, -0.25, 0.0, 3.0, 2.5, -4.0, 1.5, 0.75], dtype=np.float32)
    w = S.kept_weights(l, 1.0)
    n = 200_000
    ids, wd, total = S.pick(w, S.draw_u64(np.arange(n, dtype=np.int64), 0))
    assert total == int(w.sum()) and np.array_equal(wd, w[ids])
    q = w / total
    freq = np.bincount(ids, minlength=8) / n
    sigma = np.sqrt(q * (1 - q) / n)
    assert np.all(np.abs(freq - q) <= 5 * sigma), (freq, q, sigma)
    for s in (0, 1, 77, 199_999):                                  # the vectorised draw is the scalar path's
        assert S.sample_row(l, 1.0, 0, 1.0, s, 0) == (int(ids[s]), int(w[ids[s]]), total)


# ---- edge rules ----------------------------------------------------------------------------------------------------------
def test_temperature_zero_is_argmax_with_lowest_index_ties():
    l = bf16_logits(5, n=512)
    l[[400, 17, 300]] = l.max() + 1
    for seed in (0, 9):
        assert S.sample_row(l, 0.0, 50, 0.5, seed, 3) == (17, 1, 1)


def test_top_k_one_is_greedy_for_any_seed():
    l = bf16_logits(6, n=512)
    for seed in range(50):
        assert S.sample_row(l, 1.0, 1, 1.0, seed, seed % 7) == (int(l.argmax()), S.WEIGHT_ONE, S.WEIGHT_ONE)
    tied = l.copy()
    tied[[30, 40]] = l.max() + 2                                   # HF's rule keeps every tie at the k-th value
    assert np.flatnonzero(S.kept_weights(tied, 1.0, 1, 1.0)).tolist() == [30, 40]


def test_all_equal_logits_draw_uniformly_by_the_integer_rule():
    n = 12
    w = S.kept_weights(np.full(n, -2.5, np.float32), 0.7, 0, 1.0)
    assert w.tolist() == [S.WEIGHT_ONE] * n
    for seed in range(40):
        u = int(S.draw_u64(seed, 1))
        assert S.sample_row(np.full(n, -2.5, np.float32), 0.7, 0, 1.0, seed, 1) == ((u * n) >> 64, S.WEIGHT_ONE, n * S.WEIGHT_ONE)
    # with top-p the index-ordered prefix of the ties stays: ceil(0.5 · 12) = 6 tokens
    assert np.flatnonzero(S.kept_weights(np.full(n, -2.5, np.float32), 0.7, 0, 0.5)).tolist() == list(range(6))


def test_extreme_draws_pick_first_and_last_kept_index():
    l = bf16_logits(7, n=256)
    kept = S.kept_weights(l, 1.0, 8, 1.0)
    idx = np.flatnonzero(kept)
    assert len(idx) == 8
    assert int(S.pick(kept, np.uint64(0))[0]) == idx[0]
    assert int(S.pick(kept, np.uint64((1 << 64) - 1))[0]) == idx[-1]


def test_tiny_top_p_keeps_only_the_first_ranked_token():
    l = bf16_logits(8, n=256)
    l[[100, 200]] = l.max() + 1                                    # two tokens tie for first: index order ranks 100 first
    for p in (1e-9, 1e-6, 0.01):
        assert np.flatnonzero(S.kept_weights(l, 1.0, 0, p)).tolist() == [100]
    assert S.sample_row(l, 1.0, 0, 1e-9, 4, 0) == (100, S.WEIGHT_ONE, S.WEIGHT_ONE)


def test_top_p_boundary_is_strict_and_exact_on_ties():
    """Four tokens at the maximum (weight 2^30 each), the rest far below: p = 0.5 keeps exactly the first two of the four
    (before = 2·2^30 is not below half the total when the tail carries no weight), p just above keeps three."""
    l = np.full(64, -100.0, np.float32)
    l[[5, 9, 33, 60]] = 2.0
    assert np.flatnonzero(S.kept_weights(l, 1.0, 0, 0.5)).tolist() == [5, 9]
    assert np.flatnonzero(S.kept_weights(l, 1.0, 0, 0.51)).tolist() == [5, 9, 33]


def test_sampling_params_resolution():
    T, k, p, seed = S.SamplingParams(0.7, [0, 5, 9], 0.9, seed=-1).resolve(3)
    assert T.dtype == np.float32 and k.dtype == np.int32 and p.dtype == np.float32 and seed.dtype == np.int64
    assert k.tolist() == [0, 5, 9] and seed.tolist() == [-1] * 3 and np.all(T == np.float32(0.7))
    assert S.SamplingParams(seed=(1 << 64) - 1).resolve(2)[3].tolist() == [-1, -1]
    torch.manual_seed(11)
    a = S.SamplingParams().resolve(4)[3]
    torch.manual_seed(11)
    b = S.SamplingParams().resolve(4)[3]
    assert np.array_equal(a, b) and len(set(a.tolist())) == 4          # seed=None honours torch.manual_seed
    for bad in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_k=-2), dict(top_p=0.0), dict(top_k=[1, 2])):
        with pytest.raises(ValueError):
            S.SamplingParams(**bad).resolve(3)
    signed = lambda v: v - (1 << 64) if v >= 1 << 63 else v
    assert S.derive_seed(np.array([-1, 5]), 2).tolist() == [signed((s + 2 * 0x9E3779B97F4A7C15) % (1 << 64)) for s in ((1 << 64) - 1, 5)]
    assert S.derive_seed(7, 0).tolist() == [7]
    assert np.allclose(S.logprob(np.array([[1, 4], [3, 3]])), np.log([0.25, 1.0]))


# ---- server --------------------------------------------------------------------------------------------------------------
class SamplingVLA:
    """Stand-in model: records every call; tokens are a function of each row's own settings."""
    norm_stats = {"robot": {"action": {"q01": [0.0] * 7, "q99": [1.0] * 7}}}

    def __init__(self):
        self.calls = []

    def predict_action(self, input_ids=None, pixel_values=None, unnorm_key=None, do_sample=False, sampling=None,
                       return_weights=False):
        assert do_sample is False
        B = input_ids.shape[0]
        self.calls.append(dict(B=B, sampling=None if sampling is None else sampling.resolve(B), return_weights=return_weights))
        base = input_ids.double().sum(dim=1).numpy()[:, None] + np.arange(7)
        if sampling is None:
            return base[0] if B == 1 else base
        T, k, p, seed = sampling.resolve(B)
        actions = base + 1000.0 * T[:, None] + 10.0 * k[:, None] + (seed % 7)[:, None]
        wt = np.stack([np.full((B, 7), 1, np.int64) * (1 + k[:, None]), np.full((B, 7), 4, np.int64) * (1 + k[:, None])], axis=-1)
        return actions, np.zeros((B, 7), np.int64), wt


class Processor:
    def __call__(self, prompt, image):
        return {"input_ids": torch.tensor([[1, 7, int(np.asarray(image).sum()) % 97, 9]]), "pixel_values": torch.zeros(1, 6, 2, 2)}


def _fire(server, payloads):
    out = [None] * len(payloads)

    def worker(i):
        out[i] = server.predict_action(dict(payloads[i]))
    ts = [threading.Thread(target=worker, args=(i,)) for i in range(len(payloads))]
    [t.start() for t in ts]
    [t.join(timeout=60) for t in ts]
    return out


def _payload(i, **extra):
    img = np.full((4, 4, 3), i, dtype=np.uint8)
    return {"image": serve.encode_ndarray(img), "instruction": "lift", "unnorm_key": "robot", **extra}


def test_server_coalesces_mixed_settings_into_one_call():
    vla = SamplingVLA()
    server = serve.OpenVLAServer(vla, Processor(), max_batch=4, max_wait_ms=10000, sample=True)
    try:
        payloads = [_payload(0, temperature=0.5, top_k=3, seed=10), _payload(1), _payload(2, temperature=2.0, top_p=0.9, seed=11, return_logprob=True),
                    _payload(3, top_k=8, seed=(1 << 64) - 3)]
        out = [serve.decode_tree(o) for o in _fire(server, payloads)]
        assert len(vla.calls) == 1 and vla.calls[0]["B"] == 4 and vla.calls[0]["return_weights"] and server.batch_sizes == [4]
        T, k, p, seed = vla.calls[0]["sampling"]
        rows = {}                                                   # requests arrive in any order: identify rows by their settings
        for r in range(4):
            rows[(float(T[r]), int(k[r]), round(float(p[r]), 4), int(seed[r]))] = r
        assert set(rows) == {(0.5, 3, 1.0, 10), (0.0, 0, 1.0, 0), (2.0, 0, 0.9, 11), (1.0, 8, 1.0, -3)}   # no settings = a greedy row
        for i, (pl, got) in enumerate(zip(payloads, out)):
            ids_sum = 1 + 7 + (i * 48) % 97 + 9
            Ti, ki, si = pl.get("temperature", 1.0 if "top_k" in pl else 0.0), pl.get("top_k", 0), pl.get("seed", 0)
            si = si - (1 << 64) if si >= 1 << 63 else si
            want = ids_sum + np.arange(7) + 1000.0 * Ti + 10.0 * ki + si % 7
            if pl.get("return_logprob"):
                assert set(got) == {"action", "logprob"} and np.allclose(got["action"], want)
                assert np.allclose(got["logprob"], np.log(0.25)) and got["logprob"].shape == (7,)
            else:
                assert isinstance(got, np.ndarray) and np.allclose(got, want), i
    finally:
        server.close()


def test_server_rejects_unknown_and_unserved_sampling_keys():
    vla = SamplingVLA()
    sampled = serve.OpenVLAServer(vla, Processor(), max_batch=1, max_wait_ms=1, sample=True)
    plain = serve.OpenVLAServer(vla, Processor(), max_batch=1, max_wait_ms=1)
    try:
        assert sampled.predict_action(_payload(0, temprature=0.5)) == "error"            # a typo must not become a greedy answer
        assert sampled.predict_action(_payload(0, temperature=-1.0)) == "error"
        assert sampled.predict_action(_payload(0, top_p=0.0)) == "error"
        assert plain.predict_action(_payload(0, temperature=0.5)) == "error"             # nothing is ignored silently
        assert plain.predict_action(_payload(0, return_logprob=True)) == "error"
        assert not vla.calls
        got = serve.decode_tree(plain.predict_action(_payload(0)))                       # the plain server is unchanged
        assert np.allclose(got, 17 + np.arange(7)) and vla.calls[-1]["sampling"] is None
        got = serve.decode_tree(sampled.predict_action(_payload(0, temperature=1.0)))    # a missing seed is drawn
        assert isinstance(got, np.ndarray) and vla.calls[-1]["sampling"][0][0] == 1.0
    finally:
        sampled.close()
        plain.close()
