#!/usr/bin/env python3
"""Timing-only and schedule-variant builds of the staggered GEMM loops (DESIGN §3 "Staggered 288-row tiles", §4 "where the
loop's time goes"). RESULTS OF THE TIMING-ONLY BUILDS ARE INVALID — they drop synchronisation or staging on purpose to
see what a K-tile costs without it.

    python tools/micro/gemm_loop_experiments.py nobar|nowait|noissue|noread|merge288|split333|split225|prio288 [...]

writes a patched COPY of bridgelang_amd/csrc/gemm_bf16.hip under tools/micro/build/<name>/ (the product source holds no
experiment switches), builds the whole library around it as tools/micro/build/<name>/libbridgelang_hip.so and prints the
path; run a bench against it with BRIDGELANG_HIP_LIB=<path> (tools/bench_gemm.py, tools/ab_lib.sh).

256 kernel (timing only): nobar, nowait, noissue, noread.
288 kernel:
  merge288  timing only: the SIX-slot loop the kernel had before its three-phase form (12-MFMA blocks, pieces 1/2/1/2/1/2,
            `vmcnt(2)`) with every second barrier pair dropped, so that two blocks and two slots run back to back. Against
            the six-slot kernel itself it prices a segment: c = (t_six - t_merged) / 6 per K-tile.
  split333  valid results: the nine pieces as 3 / 3 / 3 over the three slots (`vmcnt(3)`) instead of 2 / 3 / 4.
  split225  valid results: 2 / 2 / 5 (`vmcnt(5)`; activation piece 0 moves into slot 2).
  prio288   valid results: no `s_setprio` flips around the phases; one `s_setprio 1` for waves 4-7 before the loop."""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
CSRC = ROOT / "bridgelang_amd" / "csrc"
SRCS = re.search(r"^SRCS := (.*)$", (CSRC / "Makefile").read_text(), re.M).group(1).split()

BAR = ("#define BAR()                                   \\\n  do {                                          \\\n"
       "    __builtin_amdgcn_s_barrier();               \\\n    __builtin_amdgcn_sched_barrier(0);          \\\n  } while (0)\n")
SB = "__builtin_amdgcn_sched_barrier(0);"
SLOT0 = (f"#define SLOT0(SC, T) do {{ READ_X(0, SC); READ_Y(Ya, 0, SC); READ_Y(Yb, 1, SC); {SB} ISSUE_A(0, (T) + 1); "
         "ISSUE_A(1, (T) + 1); WAIT_LGKM(); } while (0)\n")
SLOT1 = (f"#define SLOT1(SC, T) do {{ READ_X(1, SC); {SB} ISSUE_A(2, (T) + 1); ISSUE_A(3, (T) + 1); ISSUE_A(4, (T) + 1); "
         "WAIT_LGKM(); } while (0)\n")
SLOT2 = (f"#define SLOT2(SC, T) do {{ READ_X(2, SC); {SB} ISSUE_W(0, 0, (T) + 2); ISSUE_W(0, 1, (T) + 2); "
         "ISSUE_W(1, 0, (T) + 2); ISSUE_W(1, 1, (T) + 2); WAIT_VM4_LGKM(); } while (0)\n")
VM4 = '#define WAIT_VM4_LGKM() asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory")\n'
PRO_W1 = "  ISSUE_W(0, 0, 1); ISSUE_W(0, 1, 1); ISSUE_W(1, 0, 1); ISSUE_W(1, 1, 1);\n"
PRO_VM4 = '  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");\n'
LOOP_A = """    SLOT0(S0, 0);
    BAR();
    for (int t = 0; t < nk; t += 2) {        // nk is even (launcher: K % 128 == 0)
      PHASE(0); BAR();   SLOT1(S0, t); BAR();
      PHASE(1); BAR();   SLOT2(S0, t); BAR();
      PHASE(2); BAR();   SLOT0(S1, t + 1); BAR();
      PHASE(0); BAR();   SLOT1(S1, t + 1); BAR();
      PHASE(1); BAR();   SLOT2(S1, t + 1); BAR();
      PHASE(2); BAR();   SLOT0(S0, t + 2); BAR();
    }
"""
LOOP_B = """  BAR();
  for (int t = 0; t < nk; t += 2) {
    SLOT0(S0, t); BAR();       PHASE(0); BAR();
    SLOT1(S0, t); BAR();       PHASE(1); BAR();
    SLOT2(S0, t); BAR();       PHASE(2); BAR();
    SLOT0(S1, t + 1); BAR();   PHASE(0); BAR();
    SLOT1(S1, t + 1); BAR();   PHASE(1); BAR();
    SLOT2(S1, t + 1); BAR();   PHASE(2); BAR();
  }
"""
# the six slots and 12-MFMA blocks of the kernel's previous form, for merge288
SIX = VM4 + f"""#define M6(YR, T3, NH) do {{ __builtin_amdgcn_s_setprio(1); MMA(YR, T3, NH) __builtin_amdgcn_s_setprio(0); }} while (0)
#define P1(SC, T) do {{ READ_X(0, SC); READ_Y(Ya, 0, SC); {SB} ISSUE_A(2, (T) + 1); WAIT_LGKM(); }} while (0)
#define P2(SC, T) do {{ READ_Y(Yb, 1, SC); {SB} ISSUE_A(3, (T) + 1); ISSUE_A(4, (T) + 1); WAIT_LGKM(); }} while (0)
#define P3(SC, T) do {{ READ_X(1, SC); {SB} ISSUE_W(0, 0, (T) + 1); WAIT_LGKM(); }} while (0)
#define P4(SC, T) do {{ ISSUE_W(0, 1, (T) + 1); ISSUE_W(1, 0, (T) + 1); }} while (0)
#define P5(SC, T) do {{ READ_X(2, SC); {SB} ISSUE_W(1, 1, (T) + 1); WAIT_LGKM(); }} while (0)
#define P6(SC, T) do {{ ISSUE_A(0, (T) + 2); ISSUE_A(1, (T) + 2); asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory"); }} while (0)
"""
MERGED_A = """    P1(S0, 0);
    BAR();
    for (int t = 0; t < nk; t += 2) {
      M6(Ya, 0, 0); M6(Yb, 0, 1); BAR();   P2(S0, t); P3(S0, t); BAR();
      M6(Yb, 1, 1); M6(Ya, 1, 0); BAR();   P4(S0, t); P5(S0, t); BAR();
      M6(Ya, 2, 0); M6(Yb, 2, 1); BAR();   P6(S0, t); P1(S1, t + 1); BAR();
      M6(Ya, 0, 0); M6(Yb, 0, 1); BAR();   P2(S1, t + 1); P3(S1, t + 1); BAR();
      M6(Yb, 1, 1); M6(Ya, 1, 0); BAR();   P4(S1, t + 1); P5(S1, t + 1); BAR();
      M6(Ya, 2, 0); M6(Yb, 2, 1); BAR();   P6(S1, t + 1); P1(S0, t + 2); BAR();
    }
"""
MERGED_B = """  BAR();
  for (int t = 0; t < nk; t += 2) {
    P1(S0, t); P2(S0, t); BAR();           M6(Ya, 0, 0); M6(Yb, 0, 1); BAR();
    P3(S0, t); P4(S0, t); BAR();           M6(Yb, 1, 1); M6(Ya, 1, 0); BAR();
    P5(S0, t); P6(S0, t); BAR();           M6(Ya, 2, 0); M6(Yb, 2, 1); BAR();
    P1(S1, t + 1); P2(S1, t + 1); BAR();   M6(Ya, 0, 0); M6(Yb, 0, 1); BAR();
    P3(S1, t + 1); P4(S1, t + 1); BAR();   M6(Yb, 1, 1); M6(Ya, 1, 0); BAR();
    P5(S1, t + 1); P6(S1, t + 1); BAR();   M6(Ya, 2, 0); M6(Yb, 2, 1); BAR();
  }
"""
PHASE_FLIPS = ("    __builtin_amdgcn_s_setprio(1);                                                                        \\\n"
               "    MMA(Ya, T3, 0)                                                                                        \\\n"
               "    MMA(Yb, T3, 1)                                                                                        \\\n"
               "    __builtin_amdgcn_s_setprio(0);                                                                        \\\n")

# (old, new): the LAST occurrence is patched (the gemm256s section); (old, new, "288"): the only occurrence, in gemm288s
PATCHES = {
    # every in-loop s_barrier of gemm256s_kernel dropped: how much of the loop is barrier cost
    "nobar": [(BAR, "#define BAR() __builtin_amdgcn_sched_barrier(0)\n")],
    # no vmcnt wait: loop time without waiting for the LDS-DMA
    "nowait": [('#define WAIT_VM8() asm volatile("s_waitcnt vmcnt(8)" ::: "memory")\n',
                '#define WAIT_VM8() asm volatile("" ::: "memory")\n'),
               ('#define WAIT_VM10_LGKM() asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)" ::: "memory")\n',
                '#define WAIT_VM10_LGKM() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")\n')],
    # segment cost without the LDS-DMA issue (stale LDS contents) / without the fragment reads
    "noissue": [("#define ISSUE_READ(I, R) do { R; __builtin_amdgcn_sched_barrier(0); I; } while (0)\n",
                 "#define ISSUE_READ(I, R) do { R; } while (0)\n")],
    "noread": [("#define ISSUE_READ(I, R) do { R; __builtin_amdgcn_sched_barrier(0); I; } while (0)\n",
                "#define ISSUE_READ(I, R) do { I; } while (0)\n")],
    "merge288": [(VM4, SIX, "288"), (PRO_W1, "  ISSUE_A(0, 1); ISSUE_A(1, 1);\n", "288"),
                 (PRO_VM4, '  asm volatile("s_waitcnt vmcnt(2)" ::: "memory");\n', "288"),
                 (LOOP_A, MERGED_A, "288"), (LOOP_B, MERGED_B, "288")],
    "split333": [(SLOT0, SLOT0.replace("ISSUE_A(1, (T) + 1);", "ISSUE_A(1, (T) + 1); ISSUE_A(2, (T) + 1);"), "288"),
                 (SLOT1, SLOT1.replace("ISSUE_A(2, (T) + 1); ", "").replace("WAIT_LGKM();", "ISSUE_W(0, 0, (T) + 1); WAIT_LGKM();"),
                  "288"),
                 (SLOT2, SLOT2.replace("ISSUE_W(0, 0, (T) + 2); ", "").replace("WAIT_VM4_LGKM()", "WAIT_VM3_LGKM()"), "288"),
                 (VM4, VM4 + VM4.replace("VM4", "VM3").replace("vmcnt(4)", "vmcnt(3)"), "288"),
                 (PRO_W1, PRO_W1.replace("ISSUE_W(0, 0, 1); ", ""), "288"), (PRO_VM4, PRO_VM4.replace("(4)", "(3)"), "288")],
    "split225": [(SLOT0, SLOT0.replace("ISSUE_A(0, (T) + 1); ISSUE_A(1, (T) + 1);", "ISSUE_A(1, (T) + 1); ISSUE_A(2, (T) + 1);"),
                  "288"),
                 (SLOT1, SLOT1.replace("ISSUE_A(2, (T) + 1); ", ""), "288"),
                 (SLOT2, SLOT2.replace("ISSUE_W(0, 0, (T) + 2);", "ISSUE_A(0, (T) + 2); ISSUE_W(0, 0, (T) + 2);")
                  .replace("WAIT_VM4_LGKM()", "WAIT_VM5_LGKM()"), "288"),
                 (VM4, VM4 + VM4.replace("VM4", "VM5").replace("vmcnt(4)", "vmcnt(5)"), "288"),
                 (PRO_W1, PRO_W1.replace("  ISSUE_W(0, 0, 1);", "  ISSUE_A(0, 1); ISSUE_W(0, 0, 1);"), "288"),
                 (PRO_VM4, PRO_VM4.replace("(4)", "(5)"), "288")],
    "prio288": [(PHASE_FLIPS, PHASE_FLIPS.replace("__builtin_amdgcn_s_setprio(1);", "                               ")
                 .replace("__builtin_amdgcn_s_setprio(0);", "                               "), "288"),
                (LOOP_B, "  __builtin_amdgcn_s_setprio(1);\n" + LOOP_B, "288")],
}


def build(name: str) -> Path:
    out = Path(__file__).resolve().parent / "build" / name
    out.mkdir(parents=True, exist_ok=True)
    text = (CSRC / "gemm_bf16.hip").read_text()
    for old, new, *where in PATCHES[name]:
        at = text.rfind(old)
        if at < 0 or (where and text.count(old) != 1):
            raise SystemExit(f"{name}: macro text not found in gemm_bf16.hip — update PATCHES")
        text = text[:at] + new + text[at + len(old):]
    (out / "gemm_bf16.hip").write_text(text)
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{ROOT / 'include'}", f"-I{CSRC}"]
    objs = []
    for s in SRCS:
        src = out / s if s == "gemm_bf16.hip" else CSRC / s
        obj = out / (s[:-4] + ".o")
        made = CSRC / "build" / obj.name
        if s != "gemm_bf16.hip" and made.exists() and made.stat().st_mtime > src.stat().st_mtime:
            obj = made                               # the product build's up-to-date object of the same source
        else:
            subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, "-c", str(src), "-o", str(obj)])
        objs.append(str(obj))
    lib = out / "libbridgelang_hip.so"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-shared", "-fPIC", "--offload-arch=gfx950", *objs, "-o", str(lib)])
    return lib


if __name__ == "__main__":
    names = sys.argv[1:] or list(PATCHES)
    for n in names:
        if n not in PATCHES:
            raise SystemExit(f"unknown experiment {n}: choose from {', '.join(PATCHES)}")
        print(n, build(n))
