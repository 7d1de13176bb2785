"""CPU side of the tap / det head backward (aaclip_tap_head_backward): the symbols and the ABI number, the workspace
query, the device-free argument errors (every check precedes the first HIP call), the leaky cases' distance from the
LeakyReLU kink, and the Python surface above the entry point."""
import os
import re

import pytest

import head_backward_cases as HB
from aaclip_hip import _lib, autograd
from conftest import REPO

P = 0x7f0000001000      # plausible, 16-byte aligned device addresses: nothing here may be dereferenced
BIG = 1 << 40
NAMES = ("x", "ln_w", "ln_b", "proj_w", "proj_wt", "d_seg", "det_w", "det_wt", "d_det", "d_x", "d_proj_w", "d_det_w")


def _err(lib):
    return lib.aaclip_last_error()


def call(lib, B=2, L=170, D=1024, E=768, act=0, ws=P, ws_bytes=BIG, **ptrs):
    a = {n: P for n in NAMES}
    a.update(ptrs)
    return lib.aaclip_tap_head_backward(a["x"], a["ln_w"], a["ln_b"], a["proj_w"], a["proj_wt"], act, a["d_seg"],
                                        a["det_w"], a["det_wt"], a["d_det"], a["d_x"], a["d_proj_w"], a["d_det_w"],
                                        B, L, D, E, ws, ws_bytes, None)


def failed(lib, rc, word):
    msg = _err(lib)
    return rc < 0 and msg.startswith(b"tap_head_backward:") and word in msg


def test_symbols_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name in ("aaclip_tap_head_backward_workspace_bytes", "aaclip_tap_head_backward"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert re.search(r"\b%s\(" % name, header)
    in_header = int(re.search(r"#define\s+AACLIP_ABI_VERSION\s+(\d+)", header).group(1))
    assert in_header == 10 and lib.aaclip_version() == 10 and _lib.ABI_VERSION == 10


def test_workspace_query():
    q = _lib.load().aaclip_tap_head_backward_workspace_bytes
    assert q(0, 170, 1024, 768) == 0 and q(2, 0, 1024, 768) == 0 and q(2, 170, 0, 768) == 0 and q(2, 170, 1024, 0) == 0
    assert q(-1, 170, 1024, 768) == 0
    for arg, values in ((0, (1, 2, 3, 16, 64)), (1, (2, 5, 50, 128, 129, 170, 1370, 2049, 2740)),
                        (2, (256, 512, 768, 1024)), (3, (256, 512, 768, 1024))):
        prev = 0
        for v in values:
            shape = [2, 170, 1024, 768]
            shape[arg] = v
            n = q(*shape)
            assert n > prev, (arg, v)
            prev = n
    # at least the LayerNorm'ed rows, the projection rows and one d_ln
    assert q(2, 170, 1024, 768) >= 2 * 170 * (2 * 1024 + 768) * 4


def test_argument_errors():
    lib = _lib.load()
    for name in ("x", "ln_w", "ln_b", "proj_w", "d_proj_w"):
        assert failed(lib, call(lib, **{name: None}), b"null"), name
    assert failed(lib, call(lib, ws=None), b"null")
    assert failed(lib, call(lib, d_seg=None, d_det=None, det_w=None, det_wt=None, d_det_w=None), b"nothing to compute")
    assert failed(lib, call(lib, B=0), b"shape")
    assert failed(lib, call(lib, L=1), b"shape")
    assert failed(lib, call(lib, L=0), b"shape")
    assert call(lib, D=1000) < 0 and b"row width" in _err(lib)
    assert call(lib, E=640) < 0 and b"row width" in _err(lib)
    assert failed(lib, call(lib, act=-1), b"activation")
    assert failed(lib, call(lib, act=3), b"activation")
    # the det arguments: all or none
    for name in ("det_w", "d_det", "d_det_w"):
        assert failed(lib, call(lib, **{name: None}), b"together"), name
    assert failed(lib, call(lib, det_w=None, d_det=None, d_det_w=None), b"together")          # det_wt left over
    # the transposes go with d_x
    assert failed(lib, call(lib, proj_wt=None), b"transposed")
    assert failed(lib, call(lib, det_wt=None), b"transposed")
    for name in NAMES:
        assert failed(lib, call(lib, **{name: P + 4}), b"aligned"), name
    assert failed(lib, call(lib, ws=P + 8), b"aligned")
    assert failed(lib, call(lib, B=1 << 20, L=1 << 10), b"too many rows")
    need = lib.aaclip_tap_head_backward_workspace_bytes(2, 170, 1024, 768)
    assert failed(lib, call(lib, ws_bytes=need - 1), b"workspace too small")


@pytest.mark.parametrize("ptrs", [
    {},                                                                         # seg + det + d_x
    {"det_w": None, "det_wt": None, "d_det": None, "d_det_w": None},            # a level without the det head
    {"d_seg": None},                                                            # the det head alone
    {"d_seg": None, "proj_w": None, "proj_wt": None, "d_proj_w": None},
    {"d_x": None, "proj_wt": None, "det_wt": None},                             # only the projections train
    {"d_x": None},
])
def test_valid_calls_pass_every_check_up_to_the_workspace(ptrs):
    """A fully valid call with a 16-byte workspace fails on the workspace size and on nothing before it: that check is
    the last one in front of the first launch."""
    lib = _lib.load()
    for shape in ((2, 170, 1024, 768), (1, 2, 256, 256), (1, 1370, 256, 256), (2, 50, 768, 1024)):
        for act in (0, 1, 2):
            B, L, D, E = shape
            rc = call(lib, B=B, L=L, D=D, E=E, act=act, ws_bytes=16, **ptrs)
            assert failed(lib, rc, b"workspace too small"), _err(lib)


def test_leaky_cases_stay_off_the_kink():
    """head_case asserts |z| > 1e-5 in fp64 for every patch-row pre-activation of the LeakyReLU cases."""
    leaky = [n for n, c in HB.HEAD_CASES.items() if c[4] == HB.LEAKY]
    assert len(leaky) == 3
    for name in leaky:
        t, want = HB.head_case(name)
        assert want["d_proj_w"] is not None


def test_python_surface():
    import train
    from aaclip_hip import engine
    assert hasattr(autograd, "visual_heads") and hasattr(autograd, "TapHead")
    assert hasattr(engine, "tap_head_backward")
    assert hasattr(train, "stage2_text_loss")
    assert (train.TEXT_WEIGHT, train.CLS_LOSS_SCALE, train.SEG_LOSS_SCALE) == (0.6, 0.5, 0.5)
