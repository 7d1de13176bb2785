"""The row split that runs LayerNorm passes beside a residual product's partial last round (csrc/tail_plan.h): its host
arithmetic in a stand-alone program under ASan + UBSan, and the C ABI additions on the host."""
import os
import re
import shutil
import subprocess

import pytest

from aaclip_hip import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "aa-clip-iqm_amd", "csrc")
NEW_SYMBOLS = ("aaclip_set_tail_overlap", "aaclip_set_plan_cus", "aaclip_tail_overlap_count")


def test_tail_plan_header_under_the_sanitizers(tmp_path):
    """r0, tail tile count, engagement rule, slots, LayerNorm worker indices and row disjointness against brute force, as
    gemm256t.hip uses them; no report from either sanitizer"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "tail_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(CSRC, "tail_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime of the host compiler is not installed: " + build.stderr.strip()[-200:])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and not run.stderr, (run.returncode, run.stdout, run.stderr)


def test_symbols_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name + "(" in header
    assert lib.aaclip_version() == _lib.ABI_VERSION == 10                         # additions: the ABI number stays
    assert int(re.search(r"#define\s+AACLIP_ABI_VERSION\s+(\d+)", header).group(1)) == 10


def test_switches_on_the_host():
    lib = _lib.load()
    try:
        for ok in (8, 16, 256, 1024, 0):
            assert lib.aaclip_set_plan_cus(ok) == 0
        for bad in (-8, 1, 4, 12, 1032):
            assert lib.aaclip_set_plan_cus(bad) == -1 and "set_plan_cus" in lib.aaclip_last_error().decode()
        assert lib.aaclip_set_tail_overlap(0) == 0 and lib.aaclip_set_tail_overlap(1) == 0
        assert lib.aaclip_tail_overlap_count() >= 0
        for v in (0, 1, 80, 81, 82):                                              # the accepted variant bits are unchanged
            assert lib.aaclip_set_gemm_variant(v) == 0
        assert lib.aaclip_set_gemm_variant(83) == -1 and lib.aaclip_set_gemm_variant(1 << 18) == -1
    finally:
        lib.aaclip_set_plan_cus(0)
        lib.aaclip_set_tail_overlap(1)
        lib.aaclip_set_gemm_variant(0)
