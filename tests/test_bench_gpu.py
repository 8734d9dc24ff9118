"""bench.py on the GPU with the tiny synthetic model: a plain run times exactly --steps steps and prints the headline
alone; --dump-outputs writes what the last timed step returned, the same arrays from run to run, and the staggered
pipeline's arrays equal the one-batch engine's (the bit-identity tests/test_pipeline_gpu.py checks in-process)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _bench(out_dir: Path, *extra: str) -> dict:
    """One bench.py child (a fresh process; this one keeps its GPU state), its single JSON line."""
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--model", "openvla-tiny", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _load(d: Path) -> dict:
    return {k: np.load(d / f"{k}.npy") for k in ("action_ids", "logits_first", "logits_last")}


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(tmp_path, dev):
    line = _bench(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "bf16" and line["higher_is_better"] is True
    assert line["unit"] == "action-seqs/s" and line["ms_per_step"] > 0
    assert abs(line["value"] - 16 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-2 * line["value"]
    assert not {"roofline", "end_to_end", "cpu_baseline"} & set(line)          # a plain run measures the headline only
    a = _load(tmp_path / "a")
    ids, lf, ll = a["action_ids"], a["logits_first"], a["logits_last"]
    assert ids.shape == (16, 7) and lf.shape == ll.shape == (16, 32064)
    assert all(v.dtype == np.float32 for v in a.values()) and np.all(ids == np.round(ids)) and np.all((ids >= 0) & (ids < 32064))
    rows = np.arange(16)
    assert np.all(lf[rows, ids[:, 0].astype(int)] == lf.max(1))                  # greedy: each id is its logits' maximum
    assert np.all(ll[rows, ids[:, -1].astype(int)] == ll.max(1))
    _bench(tmp_path / "b")
    b = _load(tmp_path / "b")
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k}: two runs with the same arguments differ"
    _bench(tmp_path / "c", "--pipeline", "1")
    c = _load(tmp_path / "c")
    for k in a:
        assert np.array_equal(a[k], c[k]), f"{k}: the staggered pipeline differs from the one-batch engine"
