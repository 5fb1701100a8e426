"""The GEMM tile planner (csrc/gemm_plan.cpp) on a CPU: which kernel every GEMM of the benchmarked launches runs on.

gemm_plan() is the pure host function behind gemm(): shape, epilogue, precision, concurrent stream parts, tuning
knobs and the mmt_gemm_force_config pin in, one tile (plus K slices, super-tile height) or an error out.  The tables
below were recorded from the launch code as it was BEFORE the planner existed (its launches stubbed out and logged,
3.9 million shapes compared equal), so they pin today's choices: a new tile rule shows up here as a small, reviewed
diff.  tests/gemm_plan_print.cpp (built by build() into tests/bin/, or here when absent) prints the plans.

Rows: (launch class, M, N, K, epilogue, other "key=value" words, expected tile, expected K slices).  Epilogues:
0 bf16, 1 GELU bf16, 2 residual fp32, 3 ReLU bf16, 4 fp32, 5 ReLU fp32, 6 position fp32.  Defaults of the printer:
one group, dense A, f16x3 (split=1), conc=1, a split-K workspace, 256 CUs.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "multi-modal-trakcing-bechmark_amd", "csrc")
BIN = os.path.join(REPO, "tests", "bin", "gemm_plan_print")

CONV = "amode=1"
# ViPT-deep, 32 sequences, parity mode: two stream halves of 16 (conc=2); layers of 320 / 244 / 190 / 153 tokens
VIPT_B32 = [
    ("patch", 5120, 768, 768, 4, "groups=2 conc=2", "128x128_4x2_s2_k64", 1),
    ("qkv", 5120, 2304, 768, 0, "conc=2", "gemm256s", 1),
    ("proj", 5120, 768, 768, 2, "conc=2 defer=1", "gemm128w", 1),
    ("fc1", 5120, 3072, 768, 1, "conc=2", "gemm256s", 1),
    ("fc2", 5120, 768, 3072, 2, "conc=2 defer=1", "gemm128w", 1),
    ("fc1", 3904, 3072, 768, 1, "conc=2", "gemm256s", 1),
    ("fc2", 3904, 768, 3072, 2, "conc=2 defer=1", "128x192_4x2_s2_k64", 1),
    ("qkv", 3904, 2304, 768, 0, "conc=2", "gemm256s_320", 1),
    ("proj", 3904, 768, 768, 2, "conc=2 defer=1", "128x192_4x2_s2_k64", 1),
    ("fc1", 3040, 3072, 768, 1, "conc=2", "gemm256s_320", 1),
    ("fc2", 3040, 768, 3072, 2, "conc=2 defer=1", "128x192_4x2_s2_k64", 1),
    ("qkv", 3040, 2304, 768, 0, "conc=2", "128x128_4x2_s2_k32", 1),
    ("proj", 3040, 768, 768, 2, "conc=2 defer=1", "128x192_4x2_s2_k64", 1),
    ("fc1", 2448, 3072, 768, 1, "conc=2", "128x128_4x2_s2_k32", 1),
    ("fc2", 2448, 768, 3072, 2, "conc=2 defer=1", "128x128_4x2_s2_k64", 1),
    ("qkv", 2448, 2304, 768, 0, "conc=2", "128x128_4x2_s2_k32", 1),
    ("proj", 2448, 768, 768, 2, "conc=2 defer=1", "128x128_4x2_s2_k64", 1),
    ("conv1", 4096, 768, 6912, 3, "conc=2 " + CONV, "128x192_4x2_s2_k64", 1),
    ("conv2", 4096, 128, 2304, 3, "groups=3 conc=2 " + CONV, "128x128_4x2_s2_k64", 1),
    ("conv3", 4096, 64, 1152, 3, "groups=3 conc=2 " + CONV, "64x64_4x2_s3_k64", 1),
    ("conv4", 4096, 32, 576, 5, "groups=3 conc=2 " + CONV, "32x32_2x1_s2_k64", 1),
]
# ViPT-deep, one sequence, parity mode: split-K on the residual GEMMs and the head convolutions
VIPT_B1 = [
    ("patch", 320, 768, 768, 4, "groups=2", "64x64_4x2_s3_k64", 1),
    ("qkv", 320, 2304, 768, 0, "", "64x64_4x2_s3_k64", 1),
    ("proj", 320, 768, 768, 2, "defer=1", "64x64_4x2_s3_k64", 3),
    ("fc1", 320, 3072, 768, 1, "", "64x64_4x2_s3_k64", 1),
    ("fc2", 320, 768, 3072, 2, "defer=1", "64x64_4x2_s3_k64", 4),
    ("fc1", 244, 3072, 768, 1, "", "64x64_4x2_s3_k64", 1),
    ("fc2", 244, 768, 3072, 2, "defer=1", "64x64_4x2_s3_k64", 5),
    ("qkv", 244, 2304, 768, 0, "", "64x64_4x2_s3_k64", 1),
    ("proj", 244, 768, 768, 2, "defer=1", "64x64_4x2_s3_k64", 3),
    ("fc1", 190, 3072, 768, 1, "", "64x64_4x2_s3_k64", 1),
    ("fc2", 190, 768, 3072, 2, "defer=1", "64x64_4x2_s3_k64", 7),
    ("qkv", 190, 2304, 768, 0, "", "64x64_4x2_s3_k64", 1),
    ("proj", 190, 768, 768, 2, "defer=1", "64x64_4x2_s3_k64", 3),
    ("fc1", 153, 3072, 768, 1, "", "64x64_4x2_s3_k64", 1),
    ("fc2", 153, 768, 3072, 2, "defer=1", "64x64_4x2_s3_k64", 7),
    ("qkv", 153, 2304, 768, 0, "", "64x64_4x2_s3_k64", 1),
    ("proj", 153, 768, 768, 2, "defer=1", "64x64_4x2_s3_k64", 3),
    ("conv1", 256, 768, 6912, 3, CONV, "64x64_4x2_s3_k64", 5),
    ("conv2", 256, 128, 2304, 3, "groups=3 " + CONV, "64x64_4x2_s3_k64", 8),
    ("conv3", 256, 64, 1152, 3, "groups=3 " + CONV, "64x64_4x2_s3_k64", 4),
    ("conv4", 256, 32, 576, 5, "groups=3 " + CONV, "32x32_2x1_s2_k64", 1),
]
# OSTrack-384, 32 sequences, parity mode (conc=2): layers of 720 / 548 / 427 / 343 tokens
OSTRACK384_B32 = [
    ("patch", 11520, 768, 768, 6, "conc=2", "128x128_4x2_s2_k64", 1),
    ("qkv", 11520, 2304, 768, 0, "conc=2", "gemm256s_320", 1),
    ("proj", 11520, 768, 768, 2, "conc=2 defer=1", "gemm256s", 1),
    ("fc1", 11520, 3072, 768, 1, "conc=2", "gemm256s", 1),
    ("fc2", 11520, 768, 3072, 2, "conc=2 defer=1", "gemm256s", 1),
    ("fc1", 8768, 3072, 768, 1, "conc=2", "gemm256s_320", 1),
    ("fc2", 8768, 768, 3072, 2, "conc=2 defer=1", "gemm256s", 1),
    ("qkv", 8768, 2304, 768, 0, "conc=2", "gemm256s_320", 1),
    ("proj", 8768, 768, 768, 2, "conc=2 defer=1", "gemm256s", 1),
    ("fc1", 6832, 3072, 768, 1, "conc=2", "gemm256s", 1),
    ("fc2", 6832, 768, 3072, 2, "conc=2 defer=1", "128x128_4x2_s2_k64", 1),
    ("qkv", 6832, 2304, 768, 0, "conc=2", "gemm256s", 1),
    ("proj", 6832, 768, 768, 2, "conc=2 defer=1", "128x128_4x2_s2_k64", 1),
    ("fc1", 5488, 3072, 768, 1, "conc=2", "gemm256s_320", 1),
    ("fc2", 5488, 768, 3072, 2, "conc=2 defer=1", "128x128_4x2_s2_k64", 1),
    ("qkv", 5488, 2304, 768, 0, "conc=2", "gemm256s", 1),
    ("proj", 5488, 768, 768, 2, "conc=2 defer=1", "128x128_4x2_s2_k64", 1),
    ("conv1", 9216, 768, 6912, 3, "conc=2 " + CONV, "128x128_4x2_s2_k64", 1),
    ("conv2", 9216, 128, 2304, 3, "groups=3 conc=2 " + CONV, "128x128_4x2_s2_k64", 1),
    ("conv3", 9216, 64, 1152, 3, "groups=3 conc=2 " + CONV, "128x64_2x2_s2_k64", 1),
    ("conv4", 9216, 32, 576, 5, "groups=3 conc=2 " + CONV, "64x32_4x1_s2_k64", 1),
]
# ViPT-deep, 32 sequences, bf16 mode: one stream, no split-K workspace
BF16 = "split=0 ws=0"
VIPT_B32_BF16 = [
    ("patch", 10240, 768, 768, 4, "groups=2 " + BF16, "128x128_4x2_s2_k64", 1),
    ("qkv", 10240, 2304, 768, 0, BF16, "persist", 1),
    ("proj", 10240, 768, 768, 2, BF16, "128x128_4x2_s2_k64", 1),
    ("fc1", 10240, 3072, 768, 1, BF16, "persist", 1),
    ("fc2", 10240, 768, 3072, 2, BF16, "128x128_4x2_s2_k64", 1),
    ("fc1", 7808, 3072, 768, 1, BF16, "persist", 1),
    ("fc2", 7808, 768, 3072, 2, BF16, "128x128_4x2_s2_k64", 1),
    ("qkv", 7808, 2304, 768, 0, BF16, "persist", 1),
    ("proj", 7808, 768, 768, 2, BF16, "128x128_4x2_s2_k64", 1),
    ("fc1", 6080, 3072, 768, 1, BF16, "persist", 1),
    ("fc2", 6080, 768, 3072, 2, BF16, "128x128_4x2_s2_k64", 1),
    ("qkv", 6080, 2304, 768, 0, BF16, "persist", 1),
    ("proj", 6080, 768, 768, 2, BF16, "128x128_4x2_s2_k64", 1),
    ("fc1", 4896, 3072, 768, 1, BF16, "persist", 1),
    ("fc2", 4896, 768, 3072, 2, BF16, "128x64_4x2_s2_k64", 1),
    ("qkv", 4896, 2304, 768, 0, BF16, "persist", 1),
    ("proj", 4896, 768, 768, 2, BF16, "128x64_4x2_s2_k64", 1),
    ("conv1", 8192, 768, 6912, 3, BF16 + " " + CONV, "128x128_4x2_s2_k64", 1),
    ("conv2", 8192, 128, 2304, 3, "groups=3 " + BF16 + " " + CONV, "128x64_2x2_s2_k64", 1),
    ("conv3", 8192, 64, 1152, 3, "groups=3 " + BF16 + " " + CONV, "64x64_4x2_s4_k64", 1),
    ("conv4", 8192, 32, 576, 5, "groups=3 " + BF16 + " " + CONV, "64x32_4x1_s2_k64", 1),
]

# MMT_SPLIT_CFG number -> f16x3 tile, on qkv of 4096 rows (tools/sweep_*.sh, bench_f16x3.py, b1_gemm_study.py)
SPLIT_CFG = ["128x128_4x2_s2_k64", "256x128_4x2_s3_k32", "128x128_2x2_s2_k64", "128x128_2x2_s3_k32", "256x128_4x2_s2_k32",
             "128x256_2x4_s3_k32", "256x256_2x4_s2_k32", "128x128_4x2_s3_k32", "128x64_2x2_s2_k64", "128x128_4x2_s2_k32",
             "128x128_2x2_s2_k32", "128x64_2x2_s2_k32", "128x128_4x2_s4_k32", "128x256_2x4_s2_k32", "gemm256s", "gemm256s",
             "64x64_2x2_s8_k32", "64x64_2x2_s4_k32", "64x64_2x2_s6_k32", "64x64_2x2_s3_k64"]
# mmt_gemm_force_config number -> bf16 tile, on the same shape (tests/test_gpu_kernels.py, tools/bench_gemm.py,
# gemm_stamps.py); 0 pins nothing: the rules' persistent kernel
FORCE_CFG = ["persist", "256x128_4x2_s3_k64", "256x128_4x2_s2_k64", "128x128_2x2_s2_k64", "128x128_2x2_s3_k64",
             "128x128_4x2_s2_k64", "256x256_4x2_s2_k64", "128x256_2x4_s2_k64", "64x128_2x2_s2_k64", "gemm256", "persist",
             "128x128_4x2_s4_k32", "128x128_4x2_s3_k32", "128x64_2x2_s4_k32", "256x128_4x2_s3_k32", "256x128_4x2_s4_k32",
             "ring256x128_4x2_s3_k32", "ring128x128_4x2_s4_k32", "ring128x128_4x2_s2_k64", "ring256x256_4x2_s3_k32",
             "ring256x128_4x2_s2_k64", "128x64_4x2_s2_k64", "64x128_2x4_s2_k64", "128x64_4x2_s3_k64", "64x128_2x4_s3_k64"]
# the f16x3 pins 128 / 256 / 320 (tests/test_gpu_f16x3.py, tools/gemm_stamps_f16x3.py) and the odd cases
PINS = [
    ("pin", 4096, 2304, 768, 0, "force=128", "gemm256s", 1),            # 128 pins fp32 epilogues only
    ("pin", 640, 768, 768, 0, "force=128", "64x64_4x2_s3_k64", 1),
    ("pin", 4096, 2304, 768, 2, "force=128", "gemm128w", 1),
    ("pin", 640, 768, 768, 2, "force=128", "gemm128w", 1),
    ("pin", 4096, 2304, 768, 0, "force=256", "gemm256s", 1),
    ("pin", 640, 768, 768, 0, "force=256", "gemm256s", 1),              # any tile count
    ("pin", 640, 768, 768, 2, "force=256", "gemm256s", 1),
    ("pin", 4096, 2304, 768, 0, "force=320", "gemm256s_320", 1),
    ("pin", 640, 768, 768, 0, "force=320", "gemm256s_320", 1),
    ("pin", 4096, 2304, 768, 2, "force=320", "gemm256s", 1),            # 320 with an fp32 epilogue: the 256-row tile
    ("pin", 640, 768, 768, 2, "force=320", "gemm256s", 1),
    ("odd", 4096, 768, 768, 0, "MMT_SPLIT_CFG=15", "128x128_4x2_s2_k64", 1),   # 15 pins only N >= 2048
    ("odd", 5120, 768, 768, 2, "conc=2 defer=1", "gemm128w", 1),
    # f16x3 with a bf16 pin number: it only switches the gemm128w rule off
    ("odd", 5120, 768, 768, 2, "conc=2 defer=1 force=5", "128x128_4x2_s2_k64", 1),
    ("odd", 5120, 768, 768, 2, "conc=2 defer=1 force=0", "128x128_4x2_s2_k64", 1),
    ("odd", 5120, 768, 768, 2, "conc=2 defer=1 force=24", "128x128_4x2_s2_k64", 1),
    # bf16 with an f16x3 pin number: the rules
    ("odd", 5120, 768, 768, 2, BF16 + " force=128", "128x64_4x2_s2_k64", 1),
    ("odd", 5120, 768, 768, 2, BF16 + " force=256", "128x64_4x2_s2_k64", 1),
    ("odd", 5120, 768, 768, 2, BF16 + " force=320", "128x64_4x2_s2_k64", 1),
    # a dense ReLU epilogue exists as a split-K reduce only
    ("odd", 256, 768, 768, 3, "", "64x64_4x2_s3_k64", 3),
]
# what the launch code used to skip without a word: no kernel has this epilogue / A-mode pair
ERRORS = [
    ("dense ReLU", 4096, 768, 768, 3, ""),
    ("dense ReLU", 4096, 768, 768, 5, BF16),
    ("conv without ReLU", 4096, 768, 6912, 0, CONV),
    ("conv without ReLU", 4096, 768, 6912, 2, BF16 + " " + CONV),
    ("gemm256 ReLU", 4096, 768, 768, 3, BF16 + " force=9"),
    ("pinned tile ReLU", 4096, 768, 768, 3, BF16 + " force=5"),
    ("pinned tile ReLU", 4096, 768, 768, 3, "MMT_SPLIT_CFG=9"),
    ("unknown epilogue", 4096, 768, 768, 7, ""),
]


@pytest.fixture(scope="module")
def printer():
    if not os.path.exists(BIN):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        cxx = os.environ.get("CXX") or shutil.which("c++") or "/opt/rocm/bin/hipcc"   # host-only C++
        subprocess.run([cxx, "-std=c++17", "-O1", "-I" + CSRC, os.path.join(REPO, "tests", "gemm_plan_print.cpp"),
                        os.path.join(CSRC, "gemm_plan.cpp"), "-o", BIN], check=True)

    def plans(rows):
        text = "".join(f"M={r[1]} N={r[2]} K={r[3]} epi={r[4]} {r[5]}\n" for r in rows)
        out = subprocess.run([BIN], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(rows)
        return out
    return plans


def _check(plans, rows):
    got = plans(rows)
    bad = [(r, g) for r, g in zip(rows, got) if g.split()[:2] != [r[6], f"ks={r[7]}"]]
    assert not bad, "\n".join(f"{r}: got {g}" for r, g in bad)


@pytest.mark.parametrize("table", ["VIPT_B32", "VIPT_B1", "OSTRACK384_B32", "VIPT_B32_BF16"])
def test_benchmarked_launches(printer, table):
    _check(printer, globals()[table])


def test_override_numbers(printer):
    qkv = (4096, 2304, 768, 0)
    _check(printer, [("split_cfg", *qkv, f"MMT_SPLIT_CFG={i}", t, 1) for i, t in enumerate(SPLIT_CFG)])
    _check(printer, [("force", *qkv, f"{BF16} force={i}", t, 1) for i, t in enumerate(FORCE_CFG)])
    _check(printer, PINS)


def test_deferred_reduce(printer):
    # the residual GEMMs' K slices stay in the workspace for the consuming row kernel: one group, at most 8 slices
    got = printer([("fc2", 320, 768, 3072, 2, "defer=1"), ("fc2", 320, 768, 3072, 2, ""), ("conv2", 256, 128, 2304, 3, "groups=3 defer=1 " + CONV)])
    assert [g.split()[1:3] for g in got] == [["ks=4", "defer=1"], ["ks=4", "defer=0"], ["ks=8", "defer=0"]]


def test_no_kernel_is_an_error(printer):
    got = printer(ERRORS)
    assert all(g.startswith("error: ") for g in got), got


def test_knobs_from_env(printer):
    # the variable names the tuning tools set (printer: the program exists)
    env = dict(os.environ, MMT_W256="0", MMT_T320="0", MMT_SPLITK_MAX="2")
    text = "M=5120 N=768 K=768 epi=2 conc=2 env=1\nM=3904 N=2304 K=768 conc=2 env=1\nM=320 N=768 K=3072 epi=2 env=1\n"
    out = subprocess.run([BIN], input=text, capture_output=True, text=True, check=True, env=env).stdout.splitlines()
    assert [o.split()[:2] for o in out] == [["128x128_4x2_s2_k64", "ks=1"], ["gemm256s", "ks=1"], ["64x64_4x2_s3_k64", "ks=2"]]
