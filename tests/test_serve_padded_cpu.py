"""`OpenVLAServer(pad_to=L)` on CPU with a stand-in model that records its calls: prompts of different lengths and
`unnorm_key`s are right-padded into ONE batch (pad id, mask 1…1 0…0, the empty token 29871 directly behind every
sequence's own last token), each request is un-normalised with its own key, and without `pad_to` the batching stays split
on prompt length and key."""
import threading

import numpy as np
import torch

from bridgelang_amd import serve

PAD, EMPTY = 32000, 29871
SCALE = {"robot_a": 1.0, "robot_b": -2.0}


class RecordingVLA:
    """predict_action = a function of each sequence's real tokens, its mean pixel and ITS key; every call is recorded."""
    pad_token_id = PAD
    norm_stats = {k: {"action": {"q01": [0.0] * 7, "q99": [1.0] * 7}} for k in SCALE}

    def __init__(self):
        self.calls = []

    def get_action_dim(self, unnorm_key=None):
        return len(self.norm_stats[unnorm_key]["action"]["q01"])

    def with_empty_token(self, input_ids):
        if torch.all(input_ids[:, -1] == EMPTY):
            return input_ids
        return torch.cat((input_ids, torch.full((input_ids.shape[0], 1), EMPTY, dtype=torch.long)), dim=1)

    @staticmethod
    def action(real_ids, pixels, key):
        """real_ids: the prompt's own tokens, WITHOUT the empty token."""
        return SCALE[key] * (float(sum(real_ids)) + 1000.0 * len(real_ids) + float(pixels.double().mean()) + np.arange(7))

    def predict_action(self, input_ids=None, pixel_values=None, unnorm_key=None, attention_mask=None, do_sample=False):
        assert do_sample is False
        self.calls.append(dict(ids=input_ids.clone(), mask=None if attention_mask is None else attention_mask.clone(),
                               keys=unnorm_key))
        B = input_ids.shape[0]
        keys = list(unnorm_key) if isinstance(unnorm_key, (list, tuple)) else [unnorm_key] * B
        out = []
        for b in range(B):
            row = input_ids[b] if attention_mask is None else input_ids[b][attention_mask[b].bool()]
            row = [int(t) for t in row if int(t) != EMPTY]
            out.append(self.action(row, pixel_values[b], keys[b]))
        out = np.stack(out)
        return out[0] if B == 1 else out


class WordProcessor:
    """BOS + one id per word of the prompt: the prompt length follows the instruction's word count."""

    def __call__(self, prompt, image):
        ids = torch.tensor([[1] + [3 + sum(map(ord, w)) % 900 for w in prompt.split()]])
        px = torch.from_numpy(np.asarray(image, dtype=np.float32) / 255.0).permute(2, 0, 1)[None]
        return {"input_ids": ids, "pixel_values": px}


INSTR = ["lift", "push the red block", "put the eggplant in the pot next to the sink"]


def _requests():
    rng = np.random.default_rng(5)
    return [(INSTR[i % 3], ("robot_a", "robot_b")[i % 2], rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)) for i in range(6)]


def _expected(proc, instr, key, img):
    x = proc(serve.get_openvla_prompt(instr, "openvla/openvla-7b"), img)
    return RecordingVLA.action(x["input_ids"][0].tolist(), x["pixel_values"][0], key)


def _fire(server, reqs):
    out = [None] * len(reqs)

    def worker(i):
        instr, key, img = reqs[i]
        out[i] = serve.decode_tree(server.predict_action({"image": serve.encode_ndarray(img), "instruction": instr,
                                                          "unnorm_key": key}))
    ts = [threading.Thread(target=worker, args=(i,)) for i in range(len(reqs))]
    [t.start() for t in ts]
    [t.join(timeout=60) for t in ts]
    return out


def test_pad_to_coalesces_lengths_and_keys_into_one_batch():
    vla, proc, reqs = RecordingVLA(), WordProcessor(), _requests()
    lens = {i: proc(serve.get_openvla_prompt(i, "x"), np.zeros((8, 8, 3), np.uint8))["input_ids"].shape[1] + 1 for i in INSTR}
    L = max(lens.values()) + 1
    server = serve.OpenVLAServer(vla, proc, max_batch=len(reqs), max_wait_ms=10000, pad_to=L)
    try:
        out = _fire(server, reqs)
        for (instr, key, img), got in zip(reqs, out):       # each request: its own prompt, its own key's statistics
            assert isinstance(got, np.ndarray) and np.allclose(got, _expected(proc, instr, key, img)), (instr, key)
        assert len(vla.calls) == 1 and server.batch_sizes == [len(reqs)]
        assert sorted(set(server.batch_lengths[0])) == sorted(set(lens.values())) and len(set(lens.values())) == 3
        call = vla.calls[0]
        ids, mask = call["ids"], call["mask"]
        assert tuple(ids.shape) == (8, L) and tuple(mask.shape) == (8, L)         # 6 requests filled up to 8 rows
        assert isinstance(call["keys"], list) and set(call["keys"][:6]) == set(SCALE) and len(call["keys"]) == 8
        for b in range(8):
            n = int(mask[b].sum())
            assert n in lens.values() and torch.equal(mask[b], (torch.arange(L) < n).long()), "mask must be 1…1 0…0"
            assert torch.all(ids[b, n:] == PAD) and not torch.any(ids[b, :n] == PAD), "right-padded with the pad id"
            assert (ids[b] == EMPTY).nonzero().flatten().tolist() == [n - 1], "29871 directly behind the last real token only"
        assert torch.equal(ids[6], ids[5]) and torch.equal(ids[7], ids[5]) and call["keys"][6:] == [call["keys"][5]] * 2
    finally:
        server.close()


def test_pad_to_leaves_long_prompts_and_unknown_keys_on_the_old_route():
    vla, proc = RecordingVLA(), WordProcessor()
    img = np.random.default_rng(6).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    L = 12
    server = serve.OpenVLAServer(vla, proc, max_batch=4, max_wait_ms=1, pad_to=L)
    try:
        long_instr = "move " * (L + 2)
        got = serve.decode_tree(server.predict_action({"image": serve.encode_ndarray(img), "instruction": long_instr,
                                                       "unnorm_key": "robot_b"}))
        assert np.allclose(got, _expected(proc, long_instr, "robot_b", img))
        assert vla.calls[-1]["mask"] is None and vla.calls[-1]["keys"] == "robot_b" and vla.calls[-1]["ids"].shape[1] > L
        assert server.predict_action({"image": serve.encode_ndarray(img), "instruction": "lift", "unnorm_key": "nope"}) == "error"
    finally:
        server.close()


def test_without_pad_to_batches_split_on_length_and_key():
    vla, proc, reqs = RecordingVLA(), WordProcessor(), _requests()
    server = serve.OpenVLAServer(vla, proc, max_batch=len(reqs), max_wait_ms=5)
    try:
        out = _fire(server, reqs)
        for (instr, key, img), got in zip(reqs, out):
            assert np.allclose(got, _expected(proc, instr, key, img)), (instr, key)
        assert sum(server.batch_sizes) == len(reqs)
        # batch_lengths counts the empty token here too, although predict_action appends it
        want_len = {i: proc(serve.get_openvla_prompt(i, "x"), reqs[0][2])["input_ids"].shape[1] + 1 for i in INSTR}
        assert sorted(b[0] for b in server.batch_lengths) == sorted(want_len[r[0]] for r in reqs)
        # six requests = six distinct (length, key) pairs: no two may share a batch, nothing is padded or masked
        assert len(vla.calls) == 6 and server.batch_sizes == [1] * 6
        for call in vla.calls:
            assert call["mask"] is None and call["keys"] in SCALE and not torch.any(call["ids"] == PAD)
            assert not torch.any(call["ids"] == EMPTY), "without pad_to the server leaves the empty token to predict_action"
    finally:
        server.close()


def test_pad_to_with_a_model_that_cannot_pad_keeps_serving():
    """A `vla` without `pad_token_id`: padding fails on the batcher thread, which must survive — the requests take the
    un-padded route and later requests are still answered."""
    class NoPadId(RecordingVLA):
        pad_token_id = property(lambda self: (_ for _ in ()).throw(AttributeError("no pad_token_id")))
    vla, proc = NoPadId(), WordProcessor()
    img = np.random.default_rng(8).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    server = serve.OpenVLAServer(vla, proc, max_batch=2, max_wait_ms=1, pad_to=16)
    try:
        for instr in ("lift", "push the red block"):
            got = serve.decode_tree(server.predict_action({"image": serve.encode_ndarray(img), "instruction": instr,
                                                           "unnorm_key": "robot_a"}))
            assert isinstance(got, np.ndarray) and np.allclose(got, _expected(proc, instr, "robot_a", img))
            assert vla.calls[-1]["mask"] is None and vla.calls[-1]["keys"] == "robot_a"
        assert server._worker.is_alive()
    finally:
        server.close()
