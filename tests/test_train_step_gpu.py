"""The training step (forward with saved activations → hand-written backward → clip → AdamW) against torch.autograd and
torch.optim.AdamW over the CPU oracle, reduced-width model, reference stage semantics (prismatic.py:129-241)."""
import pytest
import torch

from conftest import rand_bf16
from oracle import restate as R

pytestmark = pytest.mark.gpu


def make_batch(dims, B, L, seed=0, ragged=True):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 31000, (B, L), generator=g)
    ids[:, 0] = 1
    lens = [L - (3 * i if ragged else 0) for i in range(B)]
    mask = torch.zeros(B, L, dtype=torch.bool)
    labels = torch.full((B, L), -100)
    for i, n in enumerate(lens):
        mask[i, :n] = True
        ids[i, n:] = 32000
        ids[i, n - 8:n - 1] = torch.randint(31744, 32000, (7,), generator=g)     # action tokens
        ids[i, n - 1] = 2
        labels[i, n - 8:n] = ids[i, n - 8:n]                                     # datasets.py:63
    pv = rand_bf16((B, 6, 224, 224), seed + 1)
    return ids, mask, labels, pv


def oracle_loss(sd, dims, ids, mask, labels, pv):
    om = R.OracleModel.from_dims(sd, dims)
    logits, _, _ = om.prefill(ids, pv, attention_mask=mask)
    B = ids.shape[0]
    full = torch.cat([labels[:, :1], torch.full((B, 256), -100), labels[:, 1:]], 1)
    return torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, dims.vocab), full[:, 1:].reshape(-1), ignore_index=-100)


def cos(a, b):
    a, b = a.flatten().double(), b.flatten().double()
    return (a @ b / (a.norm() * b.norm() + 1e-300)).item()


@pytest.mark.parametrize("stage", ["vla-train", "vla-last-layer-train", "align", "vla-full-train", "vla-sandwich-train"])
def test_gradients_match_autograd(dev, stage):
    from bridgelang_amd.training.step import TrainStep, trainable_names
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=3)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    B, L = 3, 20
    ids, mask, labels, pv = make_batch(dims, B, L)
    ts = TrainStep(w, stage, B, L + 2)                      # planned longer than the batch: extra right padding
    ts.set_batch(ids, mask, pv, labels)
    loss = ts.forward()
    ts.backward()
    names = trainable_names(w, stage)
    for n in names:
        sd[n].requires_grad_(True)
    ref = oracle_loss(sd, dims, ids, mask, labels, pv)
    ref.backward()
    print(f"[{stage}] loss {loss.item():.5f} vs oracle {ref.item():.5f}; {len(names)} trainable tensors")
    assert abs(loss.item() - ref.item()) <= 2e-3 * abs(ref.item())
    worst = 1.0
    for n in names:
        got, want = ts.store.named_grad(n).float().cpu(), sd[n].grad
        scale = want.abs().max().item()
        assert scale > 0, n
        c = cos(got, want)
        worst = min(worst, c)
        err = (got - want).abs().max().item()
        assert c > 0.99 and err <= 0.06 * scale, f"{n}: cosine {c:.5f}, max err {err:.3g} vs scale {scale:.3g}"
    print(f"[{stage}] worst gradient cosine {worst:.5f}")
    frozen = [n for n in sd if n not in names]
    assert all(not ts.store.trainable(n) for n in frozen)


def test_two_steps_match_torch_adamw(dev):
    """clip_grad_norm(1.0) + AdamW (decay on matrices, none on norms / biases — fsdp.py:200-212) for two steps; the
    second forward runs on the re-packed updated weights, so its loss checks the whole update path."""
    from bridgelang_amd.training.step import TrainStep, trainable_names, no_decay
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=5)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    B, L, lr, wd = 2, 18, 2e-4, 0.1
    ts = TrainStep(w, "vla-train", B, L, max_grad_norm=1.0, weight_decay=wd)
    names = trainable_names(w, "vla-train")
    params = {n: sd[n].clone().requires_grad_(True) for n in names}
    opt = torch.optim.AdamW([{"params": [params[n] for n in names if not no_decay(n, params[n].shape)], "weight_decay": wd},
                             {"params": [params[n] for n in names if no_decay(n, params[n].shape)], "weight_decay": 0.0}], lr=lr)
    for step in range(2):
        ids, mask, labels, pv = make_batch(dims, B, L, seed=10 + step)
        ts.set_batch(ids, mask, pv, labels)
        loss, norm = ts.step(lr, graph=(step == 1))
        # oracle: bf16 compute copy of the fp32 masters (FSDP MixedPrecision param_dtype=bf16, fsdp.py:141-147)
        sd_step = dict(sd)
        bf = {n: params[n].detach().to(torch.bfloat16).float().requires_grad_(True) for n in names}
        sd_step.update(bf)
        ref = oracle_loss(sd_step, dims, ids, mask, labels, pv)
        ref.backward()
        for n in names:
            params[n].grad = bf[n].grad
        ref_norm = torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
        opt.step()
        opt.zero_grad()
        print(f"step {step}: loss {loss.item():.5f} vs {ref.item():.5f}; grad norm {norm.item():.4f} vs {ref_norm.item():.4f}")
        assert abs(loss.item() - ref.item()) <= 3e-3 * abs(ref.item())
        assert abs(norm.item() - ref_norm.item()) <= 2e-2 * ref_norm.item()
    # parameter movement: same direction and size as torch's AdamW
    for n in names:
        got = ts.store.named_master(n).float().cpu() - sd[n]
        want = params[n].detach() - sd[n]
        c = cos(got, want)
        assert c > 0.97, f"{n}: update cosine {c:.4f}"
        assert abs(got.norm().item() - want.norm().item()) <= 0.05 * want.norm().item(), n
    # the live bf16 weights are the rounded masters
    live = w.state_dict()
    for n in names:
        assert torch.equal(live[n].float().cpu(), ts.store.named_master(n).to(torch.bfloat16).float().cpu()), n


@pytest.mark.parametrize("stage", ["vla-train", "vla-full-train"])
def test_graph_replay_equals_eager_over_steps(dev, stage):
    """The three plans replayed as HIP graphs must reproduce the eager step bit for bit, step after step."""
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    out = {}
    for graph in (False, True):
        w = allocate(dims, dev).fill_synthetic(seed=5)
        ts = TrainStep(w, stage, 2, 18, max_grad_norm=1.0, weight_decay=0.1)
        log = []
        for step in range(5):
            ids, mask, labels, pv = make_batch(dims, 2, 18, seed=30 + step)
            ts.set_batch(ids, mask, pv, labels)
            loss, norm = ts.step(1e-3, graph=graph)
            log.append((loss.item(), norm.item()))
        out[graph] = (log, ts.store.full_master().cpu())
    print(out[False][0], out[True][0])
    assert out[False][0] == out[True][0]
    assert torch.equal(out[False][1], out[True][1])


@pytest.mark.parametrize("lora_on", [False, True])
def test_two_stream_vision_towers_equal_one_stream(dev, lora_on, monkeypatch):
    """On one un-sharded GPU the second tower's forward / backward plans run on a side stream (own scratch) inside the
    step's graphs: same kernels on the same data — losses, gradient norms and every master weight must equal the
    single-stream step (BL_TRAIN_VISION_STREAMS=0) bit for bit, for the full fine-tune and for LoRA."""
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    out = {}
    for streams in ("0", "1"):
        monkeypatch.setenv("BL_TRAIN_VISION_STREAMS", streams)
        w = allocate(dims, dev).fill_synthetic(seed=5)
        lora = LoraAdapters(w, r=8, alpha=16, seed=3) if lora_on else None
        ts = TrainStep(w, "lora" if lora_on else "vla-full-train", 2, 18, max_grad_norm=1.0, weight_decay=0.1, lora=lora)
        assert ts._vis2 == (streams == "1")
        log = []
        for step in range(3):
            ids, mask, labels, pv = make_batch(dims, 2, 18, seed=40 + step)
            ts.set_batch(ids, mask, pv, labels)
            loss, norm = ts.step(1e-3, graph=True)
            log.append((loss.item(), norm.item()))
        out[streams] = (log, ts.store.full_master().cpu())
    print(out["0"][0], out["1"][0])
    assert out["0"][0] == out["1"][0]
    assert torch.equal(out["0"][1], out["1"][1])


@pytest.mark.parametrize("stage", ["vla-train", "vla-full-train"])
def test_recompute_equals_saved_activations(dev, stage):
    """Activation recomputation (the reference's checkpointing of the decoder layers, fsdp.py:171-183) replays each
    layer's forward with the same kernels on the same saved input, so losses, norms and masters stay bit-identical while
    the per-layer activation sets collapse into one."""
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    out = {}
    for rc in (False, True):
        w = allocate(dims, dev).fill_synthetic(seed=5)
        ts = TrainStep(w, stage, 2, 18, max_grad_norm=1.0, weight_decay=0.1, recompute=rc)
        log = []
        for step in range(3):
            ids, mask, labels, pv = make_batch(dims, 2, 18, seed=30 + step)
            ts.set_batch(ids, mask, pv, labels)
            loss, norm = ts.step(1e-3, graph=(step == 2))
            log.append((loss.item(), norm.item()))
        out[rc] = (log, ts.store.full_master().cpu(), len({t.data_ptr() for t in ts.gu}), len({t.data_ptr() for t in ts.x}))
    assert out[False][0] == out[True][0]
    assert torch.equal(out[False][1], out[True][1])
    assert out[False][2] == dims.llm_layers and out[True][2] == 1 and out[True][3] == dims.llm_layers + 1


@pytest.mark.parametrize("stage,recompute", [("vla-full-train", False), ("vla-train", True)])
def test_parameter_sharding_equals_replicated_weights(dev, stage, recompute):
    """FSDP FULL_SHARD for the decoder layers (fsdp.py:84-87): the layers' weights leave the model's allocation, each
    layer is gathered into one of two slots ahead of its forward and its backward, AdamW updates the rank's slice. Same
    kernels on the same values → bit-identical losses, norms and masters; `materialize_params()` returns the model."""
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    out = {}
    for sp in (False, True):
        w = allocate(dims, dev).fill_synthetic(seed=5)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        ts = TrainStep(w, stage, 2, 18, max_grad_norm=1.0, weight_decay=0.1, shard_params=sp, recompute=recompute)
        assert w.layers_resident == (not sp)
        log = []
        for step in range(3):
            ids, mask, labels, pv = make_batch(dims, 2, 18, seed=30 + step)
            ts.set_batch(ids, mask, pv, labels)
            loss, norm = ts.step(1e-3, graph=(step == 2))
            log.append((loss.item(), norm.item()))
        if sp:
            slots = ts.pools.slots["layers"]              # qkv_w is the first view carved from the slot's forward layouts
            assert all(w.layers[l].qkv_w.data_ptr() == slots[l % 2]["fwd"].data_ptr() for l in range(dims.llm_layers))
            from bridgelang_amd.engine import OpenVLAEngine
            with pytest.raises(RuntimeError):               # no inference over a model whose layers are sharded out
                OpenVLAEngine(w, 2, 18)
            ts.materialize_params()
            assert w.layers_resident
            with pytest.raises(RuntimeError):
                ts.forward()
        live = {k: v.float().cpu() for k, v in w.state_dict().items()}
        out[sp] = (log, ts.store.full_master().cpu(), live, {n: ts.store.named_master(n).to(torch.bfloat16).float().cpu()
                                                            for n in ts.store.by_name})
    assert out[False][0] == out[True][0]
    assert torch.equal(out[False][1], out[True][1])
    for k, v in out[False][2].items():
        assert torch.equal(v, out[True][2][k]), k
    for n, v in out[True][3].items():                   # the materialised live weights are the rounded masters
        assert torch.equal(out[True][2][n], v), n


def test_parameter_sharding_without_host_syncs_equals_replicated_weights(dev):
    """Steps issued back to back with no host sync in between: the first parameter gathers of step n + 1 run on the
    communication stream and must wait for step n's AdamW (main stream) to have written the rank's slices. Losses, norms
    and masters are read only at the end and must be bit-identical to the replicated run."""
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    ids, mask, labels, pv = make_batch(dims, 2, 18, seed=30)
    out = {}
    for sp in (False, True):
        w = allocate(dims, dev).fill_synthetic(seed=5)
        ts = TrainStep(w, "vla-full-train", 2, 18, max_grad_norm=1.0, weight_decay=0.1, shard_params=sp)
        ts.set_batch(ids, mask, pv, labels)
        log = []
        for step in range(6):                               # nothing below reads a value or synchronises until the loop is over
            loss, norm = ts.step(1e-3)
            log += [loss.clone(), norm.clone()]
        out[sp] = (torch.stack(log).cpu(), ts.store.full_master().cpu())
    assert torch.equal(out[False][0], out[True][0])
    assert torch.equal(out[False][1], out[True][1])


def test_fp8_under_parameter_sharding_equals_fp8_replicated(dev):
    """configs[4]'s combination: full-shard + fp8. The e4m3 copies are produced inside the per-layer gather instead of
    after the optimizer step — same quantisation of the same bf16 values → bit-identical to the replicated fp8 run."""
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    out = {}
    for sp in (False, True):
        w = allocate(dims, dev).fill_synthetic(seed=5)
        ts = TrainStep(w, "vla-full-train", 2, 18, max_grad_norm=1.0, weight_decay=0.1, fp8=True, shard_params=sp, recompute=sp)
        log = []
        for step in range(3):
            ids, mask, labels, pv = make_batch(dims, 2, 18, seed=30 + step)
            ts.set_batch(ids, mask, pv, labels)
            loss, norm = ts.step(1e-3)
            log.append((loss.item(), norm.item()))
        out[sp] = (log, ts.store.full_master().cpu())
    assert out[False][0] == out[True][0]
    assert torch.equal(out[False][1], out[True][1])


def test_fp8_forward_dgrad_close_to_bf16(dev):
    """TrainStep(fp8=True): decoder-layer forward and input-gradient GEMMs W8A8 on the e4m3 MFMA path (BASELINE
    configs[4]); weight gradients, masters and AdamW unchanged. No reference counterpart — the stated bound vs the bf16
    step on the same weights and batches: loss within 2 %, global gradient norm within 5 %, every decoder-layer weight
    gradient at cosine >= 0.97 (measured: loss 0.3 %, norm 1 %, cosine >= 0.99), and the run must still learn."""
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    res = {}
    for fp8 in (False, True):
        w = allocate(dims, dev).fill_synthetic(seed=5)
        ts = TrainStep(w, "vla-train", 2, 18, max_grad_norm=1.0, weight_decay=0.0, fp8=fp8)
        ids, mask, labels, pv = make_batch(dims, 2, 18, seed=30)
        ts.set_batch(ids, mask, pv, labels)
        loss0 = ts.forward().item()
        ts.backward()
        norm0 = ts.clip_grad_norm().item()
        grads = {n: ts.store.named_grad(n).float().cpu().clone() for n in ts.store.by_name if ".layers." in n and n.endswith("proj.weight")}
        losses = []
        for step in range(8):                                   # over-fit the one batch
            loss, _ = ts.step(2e-3)
            losses.append(loss.item())
        res[fp8] = (loss0, norm0, grads, losses)
    (l0, n0, g0, tr0), (l1, n1, g1, tr1) = res[False], res[True]
    worst = min(cos(g0[n], g1[n]) for n in g0)
    print(f"loss {l0:.4f} / {l1:.4f}; grad norm {n0:.4f} / {n1:.4f}; worst layer-weight gradient cosine {worst:.4f}; "
          f"loss after 8 steps {tr0[-1]:.3f} / {tr1[-1]:.3f}")
    assert abs(l1 - l0) <= 2e-2 * abs(l0)
    assert abs(n1 - n0) <= 5e-2 * n0
    assert worst >= 0.97
    assert tr1[-1] < 0.7 * tr1[0] and abs(tr1[-1] - tr0[-1]) <= 0.1 * tr0[0]


def test_fp8_wgrad_close_to_bf16_wgrad(dev):
    """TrainStep(fp8=True, fp8_wgrad=True): the decoder layers' weight-gradient GEMMs on the e4m3 MFMA path as well
    (dyᵀ and xᵀ quantised per output / input channel, fp32 accumulation into the flat gradient buffer) — all three GEMM
    families of BASELINE configs[4] in fp8. Against the fp8 step with bf16 weight gradients on the same weights and batch:
    identical loss (the forward is the same), every decoder-layer weight gradient at cosine >= 0.99 and norm within 3 %
    (per-channel e4m3 has ~2 significant digits; sums over the tokens average the rounding), global norm within 2 %;
    and (exactness of the kernel itself) each fp8 weight gradient equals s_dy[n]·s_x[k]·(dyT8·xT8ᵀ) recomputed in fp64 from
    the quantised operands the step left in its scratch buffers, to the accumulation error of the fp8 MFMA."""
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    res = {}
    for wg in (False, True):
        w = allocate(dims, dev).fill_synthetic(seed=5)
        ts = TrainStep(w, "vla-train", 2, 18, max_grad_norm=1.0, weight_decay=0.0, fp8=True, fp8_wgrad=wg)
        ids, mask, labels, pv = make_batch(dims, 2, 18, seed=30)
        ts.set_batch(ids, mask, pv, labels)
        loss0 = ts.forward().item()
        ts.backward()
        norm0 = ts.clip_grad_norm().item()
        grads = {n: ts.store.named_grad(n).float().cpu().clone() for n in ts.store.by_name if ".layers." in n and n.endswith("proj.weight")}
        losses = [ts.step(2e-3)[0].item() for _ in range(8)]
        res[wg] = (loss0, norm0, grads, losses)
        if wg:   # the LAST weight gradient the backward computed on the fp8 path is layer 0's qkv: its operands are still in scratch
            N, K, Tq = 3 * dims.llm_dim, dims.llm_dim, ts.lin._Tq
            ts.forward(); ts.backward()                           # scratch + gradient of the same (post-update) step
            qa = ts.lin._wg_qA[:N * Tq].view(N, Tq).view(torch.float8_e4m3fn).double().cpu()
            from bridgelang_amd import ops
            pb = ts.lin._wg_pB[:K * Tq].view(torch.bfloat16).view(K // 16, Tq // 64, 64, 8)        # fragment-major packed codes of xᵀ
            qb = ops.unpack_weight(pb).contiguous().view(torch.uint8).view(K, Tq).view(torch.float8_e4m3fn).double().cpu()
            want = (ts.lin._wg_sA[:N].double().cpu()[:, None] * ts.lin._wg_sB[:K].double().cpu()[None, :]) * (qa @ qb.t())
            u = ts.lin.unit_of(w.layers[0].qkv_w)
            got = ts.store.grad_view(u).double().cpu()
            err = ((got - want).abs().max() / want.abs().max()).item()
            print(f"fp8 wgrad of layer 0 qkv vs fp64 on its quantised operands: max rel err {err:.2e}")
            assert err < 1e-3     # measured 1.2e-4 of the largest entry: the block-scaled MFMA's adder tree, not fp32-exact
                                  # (tests/test_fp8_gpu.py bounds the forward GEMM the same way); an indexing slip would be O(1)
    (l0, n0, g0, tr0), (l1, n1, g1, tr1) = res[False], res[True]
    worst = min(cos(g0[n], g1[n]) for n in g0)
    worst_norm = max(abs(g1[n].norm() / g0[n].norm() - 1).item() for n in g0)
    print(f"loss {l0:.4f} / {l1:.4f}; grad norm {n0:.4f} / {n1:.4f}; worst decoder weight-gradient cosine {worst:.4f}, "
          f"worst norm ratio error {worst_norm:.4f}; loss after 8 steps {tr0[-1]:.3f} / {tr1[-1]:.3f}")
    assert l1 == l0
    assert abs(n1 - n0) <= 2e-2 * n0 and worst >= 0.99 and worst_norm <= 3e-2
    assert tr1[-1] < 0.7 * tr1[0] and abs(tr1[-1] - tr0[-1]) <= 0.1 * tr0[0]


def test_recompute_rejected_with_adapters(dev):
    from bridgelang_amd.training.lora import LoraAdapters
    from bridgelang_amd.training.step import TrainStep
    from bridgelang_amd.weights import allocate, tiny_dims
    w = allocate(tiny_dims(), dev).fill_synthetic(seed=5)
    with pytest.raises(ValueError):
        TrainStep(w, "lora", 2, 18, lora=LoraAdapters(w, r=8), recompute=True)


def test_edge_cases_max_length_and_unsupervised_sample(dev):
    """(i) the longest sequence of the whole-sequence attention kernels (S = 320 = 256 patches + 64 text tokens) still matches
    autograd; (ii) a sample with no supervised token contributes nothing (HF ignore_index semantics); (iii) plans beyond the
    model's position table (model_max_length, configuration_prismatic.py:84) are rejected."""
    from bridgelang_amd.training.step import TrainStep, trainable_names
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=8)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    B, L = 2, 64
    ids, mask, labels, pv = make_batch(dims, B, L, seed=3, ragged=False)
    labels[1] = -100                                             # second sample: nothing supervised
    ts = TrainStep(w, "vla-train", B, L)
    assert ts.S == 320
    ts.set_batch(ids, mask, pv, labels)
    loss = ts.forward().item()
    ts.backward()
    names = trainable_names(w, "vla-train")
    for n in names:
        sd[n].requires_grad_(True)
    ref = oracle_loss(sd, dims, ids, mask, labels, pv)
    ref.backward()
    assert abs(loss - ref.item()) <= 2e-3 * abs(ref.item())
    for n in ("language_model.model.layers.0.self_attn.q_proj.weight", "projector.fc1.weight", "language_model.lm_head.weight",
              "language_model.model.embed_tokens.weight"):
        assert cos(ts.store.named_grad(n).float().cpu(), sd[n].grad) > 0.99, n
    # the unsupervised sample's rows of dlogits are exactly zero
    dl = ts.dlogits.view(B, ts.S, -1)
    assert dl[1].abs().max().item() == 0.0 and dl[0].abs().max().item() > 0
    with pytest.raises(ValueError):
        TrainStep(w, "vla-train", B, dims.max_pos - 256 + 1, store=ts.store)


@pytest.mark.parametrize("stage,L", [("vla-train", 150), ("vla-full-train", 344)])
def test_long_prompts_beyond_320_positions(dev, stage, L):
    """The collator pads to the longest sample up to model_max_length = 2048 (data_utils.py:101-142) and run_vla_training
    trains on whatever comes (base_strategy.py:284-366): a 150-token prompt (S = 406) and a 344-token one (S = 600) go
    through the chunked attention kernels — gradients vs autograd over the oracle, then two optimizer steps on the batch."""
    from bridgelang_amd.training.step import TrainStep, trainable_names
    from bridgelang_amd.weights import allocate, tiny_dims
    dims = tiny_dims()
    w = allocate(dims, dev).fill_synthetic(seed=9)
    sd = {k: v.float().cpu() for k, v in w.state_dict().items()}
    B = 2
    ids, mask, labels, pv = make_batch(dims, B, L, seed=5)            # ragged: the second sample is 3 tokens shorter
    ts = TrainStep(w, stage, B, L)
    assert ts.S == L + 256 > 320
    ts.set_batch(ids, mask, pv, labels)
    loss = ts.forward().item()
    ts.backward()
    names = trainable_names(w, stage)
    for n in names:
        sd[n].requires_grad_(True)
    ref = oracle_loss(sd, dims, ids, mask, labels, pv)
    ref.backward()
    assert abs(loss - ref.item()) <= 2e-3 * abs(ref.item())
    worst = 1.0
    for n in names:
        c = cos(ts.store.named_grad(n).float().cpu(), sd[n].grad)
        worst = min(worst, c)
        assert c > 0.99, f"{n}: cosine {c:.5f}"
    print(f"[{stage} S={ts.S}] loss {loss:.5f} vs oracle {ref.item():.5f}; worst gradient cosine {worst:.5f}")
    losses = [ts.step(2e-3)[0].item() for _ in range(3)]
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0], losses
