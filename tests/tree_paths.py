"""Host model of the tile schedule of bridgelang_amd/csrc/attention_tree.hip: which K / V chunks and 32-row steps each of the
three kernels visits for a layout prefix ‖ G × branch, and which it skips.

A helper module, not a test module, and a model, not ground truth: it restates the loop bounds and skip predicates of the
kernels in plain Python so that the claim "this shape reaches that path" (tests/test_attention_tree_long_gpu.py) can be checked
without a GPU (tests/test_tree_paths_cpu.py). Every predicate it restates is listed in CITES with the source line it was read
from; test_tree_paths_cpu.py checks that each of those lines still holds that text, so a kernel edit that moves or changes a
predicate fails there until this model is brought along.

What the kernels compute is never taken from here: the GPU tests compare against the fp64 reference under
shared_prompt.tree_visible.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional

import numpy as np

SOURCE = Path(__file__).resolve().parent.parent / "bridgelang_amd" / "csrc" / "attention_tree.hip"

FWD_ROWS, KV_CHUNK = 64, 64                 # tree_fwd_kernel: query rows per workgroup, keys per LDS chunk
BLK, KC, WAVE_ROWS, STEP = 128, 256, 16, 32  # backward pair: rows per workgroup, LDS chunk, rows per wave, rows per step

# line of attention_tree.hip → text that line holds
CITES = {
    40: "return i < prefix ? prefix : prefix + (i - prefix) / branch * branch;",
    44: "return j < prefix ? S : min(S, prefix + ((j - prefix) / branch + 1) * branch);",
    61: "const int blk_lo = branch_lo(q0, p.prefix, p.branch);",
    81: "const int kv_end = min(p.S, q0 + 64);",
    82: "const int nchunk = (kv_end + KV_CHUNK - 1) / KV_CHUNK;",
    90: "if (key0 >= p.prefix && key0 + KV_CHUNK <= blk_lo) continue;",
    257: "const int kv_hi = q0 < p.S ? min(p.S, q0 + 16) : 0;",
    258: "const int block_hi = min(p.S, (int)blockIdx.y * 128 + 128);",
    260: "const int wave_lo = branch_lo(min(q0, p.S - 1), p.prefix, p.branch);",
    261: "const int blk_lo = branch_lo((int)blockIdx.y * 128, p.prefix, p.branch);",
    292: "for (int key0 = 0; key0 < block_hi; key0 += KC) {",
    293: "if (key0 >= p.prefix && key0 + KC <= blk_lo) continue;",
    299: "for (int s2 = 0; s2 < KC / 32 && key0 + s2 * 32 < kv_hi; ++s2) {",
    301: "if (ks0 >= p.prefix && ks0 + 32 <= wave_lo) continue;",
    360: "const int wave_hi = k0 < p.prefix ? p.S : branch_hi(min(k0 + 15, p.S - 1), p.prefix, p.branch, p.S);",
    362: "const int blk_hi = blk_k0 < p.prefix ? p.S : branch_hi(min(blk_k0 + 127, p.S - 1), p.prefix, p.branch, p.S);",
    383: "int s2_wave = k0 >> 5;",
    385: "if (k0 >= p.S) s2_wave = (p.S + 31) >> 5;",
    386: "for (int qc0 = (s2_block * 32) / KC * KC; qc0 < blk_hi; qc0 += KC) {",
    391: "for (int s2 = max(s2_wave, qc0 >> 5); s2 * 32 < min(wave_hi, qc0 + KC); ++s2) {",
}


# The shapes of tests/test_attention_tree_long_gpu.py: (prefix, branch, G) → the counters each is there for.
LONG_CASES = {
    (256, 8, 33): dict(S=520, dq_blk_skips=1, fwd_max=4, dkv_max_chunks=3, dkv_max_start=512),
    (272, 8, 64): dict(S=784, dq_blk_skips=1, fwd_max=7, dkv_max_chunks=4, dkv_max_start=768),
    (33, 7, 100): dict(S=733, fwd_skips=46, fwd_max=9, dq_blk_skips=1),
    (1, 8, 112): dict(S=897, dq_blk_max=2, dq_blk_skips=4, fwd_max=12),
    (1, 1, 700): dict(S=701, dq_blk_skips=2, dq_wave_skips=324),
    (40, 100, 5): dict(S=540, dq_wave_skips=161, fwd_max=5),
    (64, 130, 4): dict(S=584, fwd_max=6),
    (17, 300, 2): dict(S=617, dkv_max_chunks=3),
    (288, 56, 8): dict(S=736, fwd_max=5),
    (520, 8, 0): dict(S=520, fwd_skips=0, dq_blk_skips=0, dq_wave_skips=0, dkv_max_chunks=3),
    (33, 8, 250): dict(S=2033, dkv_max_chunks=8, dq_blk_max=6, fwd_max=29),
}


def branch_lo(i: int, prefix: int, branch: int) -> int:
    """attention_tree.hip:40."""
    return prefix if i < prefix else prefix + (i - prefix) // branch * branch


def branch_hi(j: int, prefix: int, branch: int, S: int) -> int:
    """attention_tree.hip:44."""
    return S if j < prefix else min(S, prefix + ((j - prefix) // branch + 1) * branch)


def fwd_schedule(prefix: int, branch: int, S: int):
    """tree_fwd_kernel: per query tile (q0, visited chunk starts, skipped chunk starts)."""
    for q0 in range(0, S, FWD_ROWS):
        blk_lo = branch_lo(q0, prefix, branch)                                  # :61
        nchunk = (min(S, q0 + 64) + KV_CHUNK - 1) // KV_CHUNK                   # :81, :82
        seen, skipped = [], []
        for c in range(nchunk):
            key0 = c * KV_CHUNK
            (skipped if key0 >= prefix and key0 + KV_CHUNK <= blk_lo else seen).append(key0)   # :90
        yield q0, seen, skipped


def dq_schedule(prefix: int, branch: int, S: int):
    """tree_bwd_dq_kernel: per 128-row block (row0, visited chunk starts, skipped chunk starts, waves), waves being a list of
    (q0, visited step starts, skipped step starts) over the visited chunks."""
    for row0 in range(0, S, BLK):
        block_hi = min(S, row0 + BLK)                                           # :258
        blk_lo = branch_lo(row0, prefix, branch)                                # :261
        seen, skipped = [], []
        for key0 in range(0, block_hi, KC):                                     # :292
            (skipped if key0 >= prefix and key0 + KC <= blk_lo else seen).append(key0)         # :293
        waves = []
        for w in range(BLK // WAVE_ROWS):
            q0 = row0 + w * WAVE_ROWS
            kv_hi = min(S, q0 + 16) if q0 < S else 0                            # :257
            wave_lo = branch_lo(min(q0, S - 1), prefix, branch)                 # :260
            s_seen, s_skipped = [], []
            for key0 in seen:
                for s2 in range(KC // STEP):                                    # :299
                    ks0 = key0 + s2 * STEP
                    if not ks0 < kv_hi:
                        break
                    (s_skipped if ks0 >= prefix and ks0 + STEP <= wave_lo else s_seen).append(ks0)   # :301
            waves.append((q0, s_seen, s_skipped))
        yield row0, seen, skipped, waves


def dkv_schedule(prefix: int, branch: int, S: int):
    """tree_bwd_dkv_kernel: per 128-key block (blk_k0, chunk starts, waves), waves being a list of (k0, query step starts)."""
    for blk_k0 in range(0, S, BLK):
        blk_hi = S if blk_k0 < prefix else branch_hi(min(blk_k0 + 127, S - 1), prefix, branch, S)   # :362
        chunks = list(range(blk_k0 // KC * KC, blk_hi, KC))                     # :386 (s2_block * 32 == blk_k0)
        waves = []
        for w in range(BLK // WAVE_ROWS):
            k0 = blk_k0 + w * WAVE_ROWS
            wave_hi = S if k0 < prefix else branch_hi(min(k0 + 15, S - 1), prefix, branch, S)       # :360
            s2_wave = (S + 31) >> 5 if k0 >= S else k0 >> 5                      # :383, :385
            steps = []
            for qc0 in chunks:
                s2 = max(s2_wave, qc0 >> 5)                                     # :391
                while s2 * STEP < min(wave_hi, qc0 + KC):
                    steps.append(s2 * STEP)
                    s2 += 1
            waves.append((k0, steps))
        yield blk_k0, chunks, waves


def paths(prefix: int, branch: int, G: int) -> Dict[str, int]:
    """Counters of the schedule for one (batch element, head) of the layout prefix + G·branch."""
    S = prefix + G * branch
    fwd = [len(sk) for _, _, sk in fwd_schedule(prefix, branch, S)]     # one tile's skips are one consecutive run (:90)
    dq = list(dq_schedule(prefix, branch, S))
    dkv = list(dkv_schedule(prefix, branch, S))
    return dict(
        S=S,
        fwd_skips=sum(fwd), fwd_max=max(fwd),
        dq_blk_skips=sum(len(sk) for _, _, sk, _ in dq), dq_blk_max=max(len(sk) for _, _, sk, _ in dq),
        dq_wave_skips=sum(len(ss) for _, _, _, waves in dq for _, _, ss in waves),
        dkv_max_chunks=max(len(c) for _, c, _ in dkv), dkv_max_start=max(c[0] for _, c, _ in dkv if c),
    )


def _sees(i: int, lo: int, hi: int, prefix: int, branch: int) -> bool:
    """Query i sees, by position alone, some key of [lo, hi)."""
    hi = min(hi, i + 1)
    return lo < hi and (lo < prefix or hi > branch_lo(i, prefix, branch))


def masked_paths(prefix: int, branch: int, G: int, mask_row) -> Dict[str, int]:
    """For one batch element's key mask [S] (1 = attend): the number of distinct 64-key forward chunks and 32-key dq steps
    whose keys are ALL masked although the kernel visits them for a tile that holds an unmasked query which, by position
    alone, sees one of their keys."""
    S = prefix + G * branch
    m = np.asarray(mask_row).reshape(S) != 0
    live = np.flatnonzero(m)

    def below_visible_query(lo, hi, q0, rows):
        return any(_sees(int(i), lo, hi, prefix, branch) for i in live[(live >= q0) & (live < q0 + rows)])

    chunks, steps = set(), set()
    for q0, seen, _ in fwd_schedule(prefix, branch, S):
        for key0 in seen:
            if not m[key0:key0 + KV_CHUNK].any() and below_visible_query(key0, key0 + KV_CHUNK, q0, FWD_ROWS):
                chunks.add(key0)
    for _, _, _, waves in dq_schedule(prefix, branch, S):
        for q0, s_seen, _ in waves:
            for ks0 in s_seen:
                if not m[ks0:ks0 + STEP].any() and below_visible_query(ks0, ks0 + STEP, q0, WAVE_ROWS):
                    steps.add(ks0)
    return dict(fwd_chunks=len(chunks), dq_steps=len(steps))


def visited(prefix: int, branch: int, G: int) -> Dict[str, np.ndarray]:
    """[S, S] bool per kernel: (query i, key j) lies in a chunk / step the model says the kernel visits. The kernels' per-element
    predicate then decides inside; a visible pair outside `visited` would be a key the schedule drops."""
    S = prefix + G * branch
    out = {n: np.zeros((S, S), dtype=bool) for n in ("fwd", "dq", "dkv")}
    for q0, seen, _ in fwd_schedule(prefix, branch, S):
        for key0 in seen:
            out["fwd"][q0:q0 + FWD_ROWS, key0:key0 + KV_CHUNK] = True
    for _, _, _, waves in dq_schedule(prefix, branch, S):
        for q0, s_seen, _ in waves:
            for ks0 in s_seen:
                out["dq"][q0:q0 + WAVE_ROWS, ks0:ks0 + STEP] = True
    for _, _, waves in dkv_schedule(prefix, branch, S):
        for k0, steps in waves:
            for qs0 in steps:
                out["dkv"][qs0:qs0 + STEP, k0:k0 + WAVE_ROWS] = True
    return out


def cited_lines(source: Optional[Path] = None) -> Dict[int, str]:
    """The cited lines of the kernel source as they stand, stripped of indentation and trailing comments."""
    lines = (source or SOURCE).read_text().splitlines()
    return {n: lines[n - 1].split("//")[0].strip() for n in CITES}
