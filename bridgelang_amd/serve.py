"""`/act` REST server over the HIP path — the serving shell of vla-scripts/deploy.py.

Contract kept from the reference (deploy.py:66-123): POST /act with
    {"image": ndarray[H, W, 3] uint8, "instruction": str, "unnorm_key": Optional[str]}      → the action (ndarray[7])
or the "double-encoded" form {"encoded": "<json text of the same dict>"} → a JSON *string* holding the encoded action
(for clients without json-numpy); any failure is logged and answered with the string "error" (deploy.py:112-121).
Prompt templates as `get_openvla_prompt` (deploy.py:56-60).

ndarrays travel in the json-numpy wire format {"__numpy__": base64(bytes), "dtype": descr, "shape": [...]}. The
json-numpy package is not installed in this image, so the codec below is a restatement from its published format
(parity unpinned: no fixture of it exists in the reference).

MI355X-first difference: requests are COALESCED. The reference serves one request per forward (batch 1, ≈ 33 ms here);
one GPU pass over 16 sequences costs 83 ms, so concurrent clients are batched: a worker thread collects up to
`max_batch` requests that share prompt length and `unnorm_key` (waiting at most `max_wait_ms` for company) and runs ONE
batched `predict_action`; per-sample results equal independent batch-1 calls (tests/test_engine_gpu.py).

Throughput mode (`pipeline_batch=B`): under sustained load the worker drives `StaggeredDecodePipeline` instead — every
tick submits one batch of B requests (vision + prefill) while the six older batches advance one decode iteration in a
single merged pass over the weights (pipeline.py; the mode `bench.py` measures, 241 vs 193 action-seqs/s at B = 16). A
request is answered 7 ticks after its batch was submitted; when the queue runs dry the pipeline is drained at once
(`flush`), so a lone request still returns after one prefill + six plain decode steps. Partial batches are padded with
copies of their last request.

Mixed-length traffic (`pad_to=L`, opt-in): instructions differ in length, so batches keyed on the prompt length stay small
and every change of length drains the pipeline. With `pad_to`, every prompt of at most L tokens (its empty token 29871
included) is right-padded to L with an attention mask and shares batches with all the others, whatever its length and
`unnorm_key` (equal action dimension); throughput mode then runs ONE `StaggeredDecodePipeline(padded=True)` for all of
them. Each request still gets the action of its own batch-1 call, bit for bit (tests/test_serve_padded_gpu.py). Longer
prompts take the per-length route above.

Sampled actions (`sample=True`, opt-in): a payload may carry `temperature`, `top_k`, `top_p` and `seed` (the settings of
bridgelang_amd/sampling.py; no seed: one is drawn from torch's default generator), and `return_logprob` to get
{"action": ndarray[7], "logprob": ndarray[7]} back — the log-probability of every drawn token under its warped
distribution. The settings are per-sequence device arrays, so requests with different settings (and requests with none:
greedy rows, temperature 0, the greedy server's action bit for bit) share batches and pipelines. Any other payload key is
answered with "error"; so is a sampling key sent to a server without `sample=True`.

The critic (`value_head=`, opt-in): a payload may carry `"return_value": true`; the answer is then
{"action": ndarray[7], "value": float} (plus "logprob" when that was asked for too): V(s) of the state the action was taken
in, from the same prefill (engine.py, `value="action"`). Requests with and without it share batches. Sent to a server
without a value head it is answered with "error".
"""
from __future__ import annotations

import base64
from collections import OrderedDict
import json
import logging
import queue
import threading
import traceback
from concurrent.futures import Future
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

SYSTEM_PROMPT = (
    "A chat between a curious user and an artificial intelligence assistant. "
    "The assistant gives helpful, detailed, and polite answers to the user's questions."
)


def get_openvla_prompt(instruction: str, openvla_path: Union[str, Path]) -> str:
    """deploy.py:56-60: v01 checkpoints use the Vicuna chat template, everything else the pure `In:/Out:` one."""
    if "v01" in str(openvla_path):
        return f"{SYSTEM_PROMPT} USER: What action should the robot take to {instruction.lower()}? ASSISTANT:"
    return f"In: What action should the robot take to {instruction.lower()}?\nOut:"


# ---- json-numpy wire format ------------------------------------------------------------------------------------------
def encode_ndarray(a: Union[np.ndarray, np.generic]) -> Dict[str, Any]:
    a = np.asarray(a)
    descr = np.lib.format.dtype_to_descr(a.dtype)
    return {"__numpy__": base64.b64encode(np.ascontiguousarray(a).tobytes()).decode("ascii"), "dtype": descr,
            "shape": list(a.shape)}


def _default(o: Any) -> Any:
    if isinstance(o, (np.ndarray, np.generic)):
        return encode_ndarray(o)
    raise TypeError(f"Object of type {type(o).__name__} is not JSON serializable")


def _hook(d: Dict[str, Any]) -> Any:
    if "__numpy__" in d:
        dt = np.lib.format.descr_to_dtype(d["dtype"])
        flat = np.frombuffer(base64.b64decode(d["__numpy__"]), dtype=dt)
        shape = tuple(d.get("shape", ()))
        return flat.reshape(shape).copy() if shape else flat[0]
    return d


def dumps(obj: Any) -> str:
    return json.dumps(obj, default=_default)


def loads(text: Union[str, bytes]) -> Any:
    return json.loads(text, object_hook=_hook)


def decode_tree(obj: Any) -> Any:
    """Apply the ndarray hook to an already-parsed JSON tree (FastAPI hands the handler plain dicts)."""
    if isinstance(obj, dict):
        return _hook({k: decode_tree(v) for k, v in obj.items()})
    if isinstance(obj, list):
        return [decode_tree(v) for v in obj]
    return obj


# ---- server ----------------------------------------------------------------------------------------------------------
class _Request:
    __slots__ = ("input_ids", "pixel_values", "unnorm_key", "future", "mask", "group", "sampling", "want_logprob", "want_value")

    def __init__(self, input_ids, pixel_values, unnorm_key):
        self.input_ids, self.pixel_values, self.unnorm_key = input_ids, pixel_values, unnorm_key
        self.future: Future = Future()
        self.mask: Optional[torch.Tensor] = None      # pad_to: attention mask [1, pad_to] of the right-padded input_ids
        self.group: Optional[tuple] = None            # requests with equal group keys may share a GPU batch
        self.sampling: Tuple[float, int, float, int] = (0.0, 0, 1.0, 0)    # sample=True: temperature (0 = greedy), top_k, top_p, seed
        self.want_logprob = False
        self.want_value = False


class OpenVLAServer:
    """`vla`: OpenVLAForActionPrediction (HIP) — anything with `predict_action(input_ids=, pixel_values=, unnorm_key=,
    do_sample=False) -> ndarray [B, 7] (or [7] at B = 1)`; `processor(prompt, PIL image) -> {input_ids, pixel_values}`.
    `pad_to=L` additionally uses `vla.with_empty_token`, `vla.pad_token_id`, `vla.get_action_dim` and calls
    `predict_action(..., attention_mask=, unnorm_key=[one key per sequence])`. `sample=True` calls
    `predict_action(..., sampling=SamplingParams(per-row arrays), return_weights=True) -> (actions, token ids, wt [B, 7, 2])`.
    `sample=True, action_tokens_only=True` draws (and, for a greedy request, takes the argmax) under the policy restricted
    to `vla.action_token_range()`: every answered action was decoded from action tokens, and a reported log-probability
    is the one under that restricted policy.
    `adapter=` (a directory written by `training.finetune.save_checkpoint`, or a training.lora.LoraAdapters over `vla`'s
    weights) serves the model under those LoRA adapters: they are attached (`vla.load_adapter` / `vla.attach_adapters`)
    before any pipeline is built, and the pipelines read the adapted weights. A learner that refreshes the adapted weights
    while the server runs must let the pipelines drain first (`LoraAdapters.refresh`, ordering contract).
    `value_head=` (a training.value_head.ValueHead, or a directory `ValueHead.save` wrote) attaches the critic
    (`vla.attach_value_head` / `vla.load_value_head`): every batch then also evaluates V(s) of its states (one more launch per
    prefill), `predict_action(..., return_values="action")` on the plain route, and a request with `"return_value": true`
    is answered with it."""

    _BASE_KEYS = ("image", "instruction", "unnorm_key")
    _SAMPLING_KEYS = ("temperature", "top_k", "top_p", "seed", "return_logprob")
    _VALUE_KEYS = ("return_value",)

    def __init__(self, vla: Any, processor: Any, openvla_path: Union[str, Path] = "openvla/openvla-7b",
                 max_batch: int = 16, max_wait_ms: float = 2.0, norm_stats_path: Optional[Union[str, Path]] = None,
                 pipeline_batch: Optional[int] = None, max_pipelines: int = 2, pad_to: Optional[int] = None,
                 sample: bool = False, action_tokens_only: bool = False, adapter: Any = None, attn_taps: Any = None,
                 value_head: Any = None):
        if attn_taps is not None:
            raise ValueError("OpenVLAServer does not return attention: call the model's generate / predict_action with "
                             "return_attention=...")
        self.vla, self.processor, self.openvla_path = vla, processor, str(openvla_path)
        if adapter is not None:
            if isinstance(adapter, (str, Path)):
                vla.load_adapter(adapter)
            else:
                vla.attach_adapters(adapter)
        self.value = None                         # "action" when a value head is attached: what the pipelines / calls are built with
        if value_head is not None:
            if isinstance(value_head, (str, Path)):
                vla.load_value_head(value_head)
            else:
                vla.attach_value_head(value_head)
            self.value = "action"
        self.sample = bool(sample)
        if action_tokens_only and not sample:
            raise ValueError("action_tokens_only goes with sample=True")
        self.vocab_range: Optional[Tuple[int, int]] = tuple(vla.action_token_range()) if action_tokens_only else None
        self.pad_to = int(pad_to) if pad_to else None
        self._pad_pipe: Optional[Tuple[Any, Dict[int, Any]]] = None     # pad_to: the one padded pipeline + its batches in flight
        self.pipelines_built = 0                  # StaggeredDecodePipelines constructed so far (observability / tests)
        self.batch_lengths: List[List[int]] = []  # per GPU batch: its requests' prompt lengths as the model sees them (empty token included)
        self.max_batch, self.max_wait = int(max_batch), float(max_wait_ms) * 1e-3
        self.pipeline_batch = pipeline_batch
        if pipeline_batch:
            self.max_batch = int(pipeline_batch)
        # prompt length → (StaggeredDecodePipeline, {tick: requests}); least recently used first. A pipeline is 7 engines
        # (KV caches + activations, ≈ 3 GB each at B = 16 on 7B) + 7 graphs, and instruction lengths vary per request, so
        # only `max_pipelines` are kept; the plain path's engines are bounded the same way on the model (engine LRU).
        # With `pad_to` the ONE padded pipeline is held in addition to these and is never evicted (7 more engines).
        self._pipes: "OrderedDict[int, Any]" = OrderedDict()
        self.max_pipelines = max(1, int(max_pipelines))
        stats = Path(norm_stats_path) if norm_stats_path else Path(self.openvla_path) / "dataset_statistics.json"
        if stats.is_file():                       # fine-tuned run directory (deploy.py:86-89)
            self.vla.norm_stats = json.loads(stats.read_text())
        self.batch_sizes: List[int] = []          # sizes of the GPU batches run so far (observability / tests)
        self._q: "queue.Queue[Optional[_Request]]" = queue.Queue()
        self._held: Optional[_Request] = None     # a request that did not fit the previous batch
        self._worker = threading.Thread(target=self._serve_loop, name="openvla-batcher", daemon=True)
        self._worker.start()

    # -- request side (any thread) --
    def _make_request(self, payload: Dict[str, Any]) -> _Request:
        from PIL import Image
        image, instruction = payload["image"], payload["instruction"]
        unnorm_key = payload.get("unnorm_key", None)
        sampling_keys = [k for k in self._SAMPLING_KEYS if k in payload]
        if sampling_keys and not self.sample:
            raise ValueError(f"{sampling_keys}: this server was started without sample=True")
        if "return_value" in payload and self.value is None:
            raise ValueError("return_value: this server was started without a value_head")
        unknown = [k for k in payload if k not in self._BASE_KEYS + self._SAMPLING_KEYS + self._VALUE_KEYS] if self.sample else []
        if unknown:
            raise ValueError(f"unknown payload keys {unknown}")
        prompt = get_openvla_prompt(instruction, self.openvla_path)
        inputs = self.processor(prompt, Image.fromarray(np.asarray(image, dtype=np.uint8)).convert("RGB"))
        req = _Request(inputs["input_ids"], inputs["pixel_values"], unnorm_key)
        if any(k in payload for k in ("temperature", "top_k", "top_p", "seed")):
            from .sampling import SamplingParams
            T, k, p, seed = SamplingParams(payload.get("temperature", 1.0), payload.get("top_k", 0), payload.get("top_p", 1.0),
                                           payload.get("seed", None)).resolve(1)        # validates; draws a missing seed
            req.sampling = (float(T[0]), int(k[0]), float(p[0]), int(seed[0]))
        req.want_logprob = bool(payload.get("return_logprob", False))
        req.want_value = bool(payload.get("return_value", False))
        return req

    def _sampling_of(self, rows: List[_Request]):
        from .sampling import SamplingParams
        T, k, p, seed = zip(*(r.sampling for r in rows))
        return SamplingParams(np.array(T, np.float32), np.array(k, np.int64), np.array(p, np.float32), np.array(seed, np.int64))

    def _submit(self, payload: Dict[str, Any]) -> np.ndarray:
        req = self._make_request(payload)
        self._q.put(req)
        return req.future.result()

    def predict_action(self, payload: Dict[str, Any]) -> Any:
        """The /act handler body (deploy.py:91-121), returning the JSON-ready response object."""
        try:
            double_encode = "encoded" in payload
            if double_encode:
                assert len(payload.keys()) == 1, "Only uses encoded payload!"
                payload = loads(payload["encoded"])
            else:
                payload = decode_tree(payload)
            action = self._submit(payload)
            if isinstance(action, dict):      # return_logprob / return_value (a plain float)
                return dumps(action) if double_encode else {k: encode_ndarray(v) if isinstance(v, np.ndarray) else v
                                                            for k, v in action.items()}
            return dumps(action) if double_encode else encode_ndarray(action)
        except Exception:   # noqa: BLE001 — the reference answers every failure with "error"
            logging.error(traceback.format_exc())
            logging.warning(
                "Your request threw an error; make sure your request complies with the expected format:\n"
                "{'image': np.ndarray, 'instruction': str}\n"
                "You can optionally an `unnorm_key: str` to specific the dataset statistics you want to use for "
                "de-normalizing the output actions.")
            return "error"

    # -- GPU side (one thread owns the model) --
    def _take_batch(self) -> Optional[List[_Request]]:
        import time
        first = self._held if self._held is not None else self._q.get()
        self._held = None
        if first is None:
            return None
        batch, key = [first], self._group(first)
        deadline = time.monotonic() + self.max_wait
        while len(batch) < self.max_batch:
            try:
                nxt = self._q.get(timeout=max(0.0, deadline - time.monotonic()))
            except queue.Empty:
                break
            if nxt is None:
                self._q.put(None)
                break
            if self._group(nxt) != key:
                self._held = nxt               # different prompt length / statistics: heads the next batch
                break
            batch.append(nxt)
        return batch

    def _group(self, r: _Request) -> tuple:
        """The key requests must share to ride one GPU batch: prompt shape and `unnorm_key`; with `pad_to`, every prompt
        that fits is first right-padded to it (`_pad`) and then shares a batch with all others of its action dimension."""
        if r.group is None:
            r.group = (tuple(r.input_ids.shape), r.unnorm_key)
            if self.pad_to is not None:
                try:
                    self._pad(r)
                except Exception:   # noqa: BLE001 — this runs on the batcher thread: the request keeps the un-padded route
                    logging.warning("pad_to: request left un-padded:\n%s", traceback.format_exc())
                    r.mask, r.group = None, (tuple(r.input_ids.shape), r.unnorm_key)
        return r.group

    def _pad(self, r: _Request) -> None:
        """pad_to: the empty token goes behind the request's own last token, then pad ids up to `pad_to` columns, hidden
        by the attention mask 1…1 0…0. A prompt that does not fit, or a key without statistics, keeps today's route."""
        ids = self.vla.with_empty_token(r.input_ids)
        n, L = ids.shape[1], self.pad_to
        if ids.shape[0] != 1 or n > L:
            return
        try:
            dim = self.vla.get_action_dim(r.unnorm_key)
        except Exception:   # noqa: BLE001 — unknown unnorm_key: the request fails alone, on the route it takes today
            return
        r.input_ids = torch.cat([ids, torch.full((1, L - n), self.vla.pad_token_id, dtype=ids.dtype, device=ids.device)], dim=1)
        r.mask = (torch.arange(L, device=ids.device)[None, :] < n).long()
        r.group = ("padded", L, dim)

    # -- throughput mode: one pipeline per prompt length (pad_to: ONE padded pipeline for every prompt that fits) --
    def _live(self) -> List[Tuple[Any, Dict[int, Any]]]:
        return ([self._pad_pipe] if self._pad_pipe is not None else []) + list(self._pipes.values())

    def _weights(self):
        """The weights the pipelines read: the adapted ones when adapters are attached to the model."""
        lora = getattr(self.vla, "_adapters", None)
        return lora.adapted_weights() if lora is not None else self.vla.weights

    def _value_kw(self) -> Dict[str, Any]:
        return {} if self.value is None else dict(value=self.value, value_head=self.vla._value_head)

    def _padded_pipe(self):
        from .pipeline import StaggeredDecodePipeline
        if self._pad_pipe is None:
            pipe = StaggeredDecodePipeline(self._weights(), self.pipeline_batch, self.pad_to, padded=True, sample=self.sample,
                                           vocab_range=self.vocab_range, **self._value_kw())
            pipe.capture()
            self.pipelines_built += 1
            self._pad_pipe = (pipe, {})
        return self._pad_pipe

    def _pipe_for(self, L: int):
        from .pipeline import StaggeredDecodePipeline
        if L in self._pipes:
            self._pipes.move_to_end(L)
            return self._pipes[L]
        while len(self._pipes) >= self.max_pipelines:       # evict the least recently used pipeline (always drained:
            old_len, (old, infl) = next(iter(self._pipes.items()))      # _serve_pipelined drains before switching lengths)
            assert not infl, "evicting a pipeline with batches in flight"
            del self._pipes[old_len]
            del old
            torch.cuda.empty_cache()
        pipe = StaggeredDecodePipeline(self._weights(), self.pipeline_batch, L, sample=self.sample, vocab_range=self.vocab_range,
                                       **self._value_kw())
        pipe.capture()
        self.pipelines_built += 1
        self._pipes[L] = (pipe, {})
        return self._pipes[L]

    @staticmethod
    def _answer(r: _Request, action: np.ndarray, wt: Optional[np.ndarray], value: Optional[float] = None) -> Any:
        if not (r.want_logprob or r.want_value):
            return action
        out = {"action": action}
        if r.want_logprob:
            from .sampling import logprob
            out["logprob"] = logprob(wt)
        if r.want_value:
            out["value"] = float(value)
        return out

    def _resolve(self, reqs: List[_Request], out) -> None:
        """`out`: the pipeline's token ids [B, 7], or with sample=True the pair (ids, wt [B, 7, 2]); with a value head the
        values [B] ride last."""
        out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        vals = out[-1].cpu().numpy() if self.value is not None else None
        token_ids, wt = out[0], (out[1] if self.sample else None)
        ids = token_ids.cpu().numpy()
        wt = wt.cpu().numpy() if wt is not None else None
        for i, r in enumerate(reqs):
            try:
                action = np.asarray(self.vla.actions_from_token_ids(ids[i:i + 1], r.unnorm_key)).reshape(-1)
                r.future.set_result(self._answer(r, action, None if wt is None else wt[i], None if vals is None else vals[i]))
            except Exception as e:   # noqa: BLE001 — e.g. an unknown unnorm_key: that request alone fails
                r.future.set_exception(e)

    def _drain(self) -> None:
        for pipe, inflight in self._live():
            if inflight:
                outs = pipe.flush(ticks=set(inflight))    # oldest first; None for slots answered earlier
                for t, out in zip(range(pipe._tick - len(outs), pipe._tick), outs):
                    if out is not None:
                        self._resolve(inflight.pop(t), out)
                inflight.clear()

    def _serve_pipelined(self) -> None:
        dev = self.vla.device
        while True:
            busy = any(inflight for _, inflight in self._live())
            if busy and self._held is None and self._q.empty():
                self._drain()                             # nothing waiting: finish what is in flight right away
                continue
            batch = self._take_batch()
            if batch is None:
                self._drain()
                return
            try:
                if self.vla.get_action_dim(batch[0].unnorm_key) != 7:
                    # the pipelines decode 7 tokens; other action dimensions go through the plain engine
                    self._run_plain(batch)
                    continue
                padded = batch[0].mask is not None
                ids = torch.cat([r.input_ids for r in batch], dim=0).to(dev)
                if not padded:
                    ids = self.vla.with_empty_token(ids)
                pv = torch.cat([r.pixel_values for r in batch], dim=0).to(dev, torch.bfloat16)
                mask = torch.cat([r.mask for r in batch], dim=0).to(dev) if padded else None
                pad = self.pipeline_batch - len(batch)
                if pad:
                    ids = torch.cat([ids, ids[-1:].expand(pad, -1)], dim=0)
                    pv = torch.cat([pv, pv[-1:].expand(pad, -1, -1, -1)], dim=0)
                    mask = torch.cat([mask, mask[-1:].expand(pad, -1)], dim=0) if padded else None
                # one pipeline at a time keeps the tick bookkeeping simple: every OTHER pipeline is drained before this
                # batch's pipeline is fetched (or built: _pipe_for may evict, and evicts drained pipelines only)
                target = self._pad_pipe if padded else self._pipes.get(ids.shape[1])
                if any(e[1] and e is not target for e in self._live()):
                    self._drain()
                pipe, inflight = self._padded_pipe() if padded else self._pipe_for(ids.shape[1])
                tick = pipe._tick
                # the masks were built here, on the host (_pad): 1…1 0…0 by construction, nothing to check on the device
                kw = dict(sampling=self._sampling_of(batch + [batch[-1]] * pad)) if self.sample else {}
                out = pipe.step(ids, pv, mask, mask_checked=True, **kw) if padded else pipe.step(ids, pv, **kw)
                inflight[tick] = batch
                self._record(batch)
                done = tick - (pipe.slots - 1)
                if done in inflight:
                    self._resolve(inflight.pop(done), tuple(o.clone() for o in out) if isinstance(out, tuple) else out.clone())
            except Exception as e:   # noqa: BLE001
                for r in batch:
                    if not r.future.done():
                        r.future.set_exception(e)

    def _serve_loop(self) -> None:
        if self.pipeline_batch:
            return self._serve_pipelined()
        while True:
            batch = self._take_batch()
            if batch is None:
                return
            self._run_plain(batch)

    def _record(self, batch: List[_Request]) -> None:
        self.batch_sizes.append(len(batch))
        self.batch_lengths.append([int(r.mask.sum()) if r.mask is not None else
                                   int(r.input_ids.shape[1]) + int(r.input_ids[0, -1] != 29871) for r in batch])

    def _run_plain(self, batch: List[_Request]) -> None:
        """One predict_action call for the batch. Batch sizes are rounded up to 1 / 2 / 4 / 8 / 16 … with copies of the
        last request, so the model builds (and its engine LRU holds) few distinct engines."""
        try:
            n = len(batch)
            size = 1
            while size < n:
                size *= 2
            rows = batch + [batch[-1]] * (size - n)
            ids = torch.cat([r.input_ids for r in rows], dim=0)
            pv = torch.cat([r.pixel_values for r in rows], dim=0)
            padded = batch[0].mask is not None      # pad_to: lengths and keys are mixed — every sequence un-normalised with its own key
            kw = dict(input_ids=ids, pixel_values=pv, unnorm_key=[r.unnorm_key for r in rows] if padded else batch[0].unnorm_key)
            if padded:
                kw["attention_mask"] = torch.cat([r.mask for r in rows], dim=0)
            if self.sample:                   # per-row settings: mixed requests (greedy ones included) ride one call
                kw.update(sampling=self._sampling_of(rows), return_weights=True)
                if self.vocab_range is not None:
                    kw["action_tokens_only"] = True
            else:
                kw["do_sample"] = False
            if self.value is not None:
                kw["return_values"] = self.value
            res = self.vla.predict_action(**kw)
            wt = None
            if self.sample:
                actions, _, wt, *vals = res
                wt = np.asarray(wt)[:n]
            else:
                actions, *vals = res if self.value is not None else (res,)
            vals = vals[0] if vals else None
            actions = np.asarray(actions).reshape(size, -1)[:n]
            self._record(batch)
            for i, (r, a) in enumerate(zip(batch, actions)):
                r.future.set_result(self._answer(r, a, None if wt is None else wt[i], None if vals is None else vals[i]))
        except Exception as e:   # noqa: BLE001 — delivered to every waiting request
            for r in batch:
                if not r.future.done():
                    r.future.set_exception(e)

    def close(self) -> None:
        self._q.put(None)
        self._worker.join(timeout=10)

    # -- HTTP --
    def build_app(self):
        from fastapi import FastAPI
        from fastapi.responses import JSONResponse
        app = FastAPI()

        def act(payload: Dict[str, Any]):      # sync handler: FastAPI runs it in its thread pool, so requests overlap
            return JSONResponse(self.predict_action(payload))

        app.post("/act")(act)
        self.app = app
        return app

    def run(self, host: str = "0.0.0.0", port: int = 8000) -> None:
        import uvicorn
        uvicorn.run(self.build_app(), host=host, port=port)
