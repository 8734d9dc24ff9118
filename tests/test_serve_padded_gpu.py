"""/act server with `pad_to` on the HIP path (reduced-width model, character-level stand-in tokenizer): concurrent requests
with instructions of five lengths and two `unnorm_key`s share GPU batches — ONE padded pipeline in throughput mode — and
every answer equals the direct batch-1 `predict_action` of that request with its own key, exactly."""
import numpy as np
import pytest
import torch

from test_serve_gpu import CharTokenizer

pytestmark = pytest.mark.gpu

INSTR = ["lift", "stack it", "open the jar", "push the red block", "put the spoon in the pot"]
KEYS = ["bridge_orig", "other_robot"]
STATS = {"bridge_orig": {"action": {"q01": [-0.5] * 7, "q99": [0.7] * 7, "mask": [True] * 6 + [False]}},
         "other_robot": {"action": {"q01": [-2.0] * 7, "q99": [3.0] * 7, "mask": [True] * 7}}}
_STATE = {}


def _setup(dev):
    """Model, processor, 20 requests and their direct batch-1 answers: built once, shared by both modes."""
    if not _STATE:
        from PIL import Image
        from bridgelang_amd import serve, weights as W
        from bridgelang_amd.extern.hf.configuration_prismatic import OpenVLAConfig
        from bridgelang_amd.extern.hf.modeling_prismatic import OpenVLAForActionPrediction
        from bridgelang_amd.extern.hf.processing_prismatic import PrismaticProcessor
        vla = OpenVLAForActionPrediction(OpenVLAConfig(norm_stats=STATS), device=dev, dims=W.tiny_dims()).init_synthetic(seed=11)
        proc = PrismaticProcessor(tokenizer=CharTokenizer())
        rng = np.random.default_rng(7)
        reqs = [(INSTR[i % 5], KEYS[(i // 5) % 2], rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)) for i in range(20)]

        def direct(instr, key, img):
            x = proc(serve.get_openvla_prompt(instr, "openvla/openvla-7b"), Image.fromarray(img).convert("RGB"))
            return x["input_ids"].shape[1], vla.predict_action(input_ids=x["input_ids"].to(dev), unnorm_key=key, do_sample=False,
                                                               pixel_values=x["pixel_values"].to(dev, torch.bfloat16))
        lens, want = zip(*[direct(*r) for r in reqs])
        long_req = ("put the eggplant in the pot next to the sink", "other_robot", reqs[0][2])
        _STATE.update(vla=vla, proc=proc, reqs=reqs, want=want, pad_to=max(lens) + 1, long_req=long_req,
                      long_want=direct(*long_req)[1])
    return _STATE


def _ask(server, req):
    from bridgelang_amd import serve
    instr, key, img = req
    return serve.decode_tree(server.predict_action({"image": serve.encode_ndarray(img), "instruction": instr, "unnorm_key": key}))


def _queue_all(server, reqs):
    """Concurrent clients whose requests are all waiting when the worker looks: built first, then queued back to back in
    a fixed order, so which requests share a batch does not depend on thread scheduling. Returns the answers in order."""
    made = [server._make_request({"image": img, "instruction": instr, "unnorm_key": key}) for instr, key, img in reqs]
    for r in made:
        server._q.put(r)
    return [r.future.result(timeout=120) for r in made]


@pytest.mark.parametrize("mode", ["pipeline", "plain"])
def test_padded_server_answers_equal_batch1_calls(dev, mode):
    from bridgelang_amd import serve
    st = _setup(dev)
    reqs, want = st["reqs"], st["want"]
    kw = dict(pipeline_batch=2) if mode == "pipeline" else dict(max_batch=4)
    server = serve.OpenVLAServer(st["vla"], st["proc"], max_wait_ms=20, pad_to=st["pad_to"], **kw)
    try:
        out = _queue_all(server, reqs)      # neighbours in the queue differ in length: any batch of two or more mixes lengths
        for i, (o, w) in enumerate(zip(out, want)):
            assert isinstance(o, np.ndarray) and np.array_equal(o, w), f"request {i} {reqs[i][:2]}: {o} != {w}"
        assert sum(server.batch_sizes) == len(reqs)
        assert any(len(set(b)) >= 2 for b in server.batch_lengths), f"no GPU batch mixed prompt lengths: {server.batch_lengths}"
        assert server.pipelines_built == (1 if mode == "pipeline" else 0)
        # a prompt longer than pad_to: answered through the per-length route
        assert np.array_equal(_ask(server, st["long_req"]), st["long_want"])
        assert server.pipelines_built == (2 if mode == "pipeline" else 0)
    finally:
        server.close()


def test_one_pipeline_slot_serves_alternating_lengths(dev):
    """Without pad_to and with max_pipelines=1, a batch of another prompt length arriving while the only pipeline has
    batches in flight: that pipeline is drained first, then replaced — every request is answered, none with an error."""
    from bridgelang_amd import serve
    st = _setup(dev)
    pick = [0, 10, 3, 13, 0, 10]             # two prompt lengths, one unnorm_key, queued back to back
    reqs, want = [st["reqs"][i] for i in pick], [st["want"][i] for i in pick]
    server = serve.OpenVLAServer(st["vla"], st["proc"], max_wait_ms=20, pipeline_batch=2, max_pipelines=1)
    try:
        out = _queue_all(server, reqs)
        for i, (o, w) in enumerate(zip(out, want)):
            assert isinstance(o, np.ndarray) and np.array_equal(o, w), f"request {i} {reqs[i][:2]}: {o} != {w}"
        assert server.batch_sizes == [2, 2, 2] and len({tuple(b) for b in server.batch_lengths}) == 2
        assert server.pipelines_built == 3 and len(server._pipes) == 1
    finally:
        server.close()
