"""CPU side of aaclip_cross_rows_backward: the symbols and the ABI number, the Python surface, the workspace size, the
device-free argument errors, the conditioning of the cases (fp32 CPU autograd against fp64) and the kernel's step
sequence in fp64 against autograd."""
import os
import re

import pytest
import torch

import cross_rows_backward_cases as CB
from aaclip_hip import _lib, autograd, engine
from conftest import REPO
from cross_rows_backward_cases import rel

SYMBOLS = ("aaclip_cross_rows_backward_workspace_bytes", "aaclip_cross_rows_backward")
SURFACE = ((engine, "cross_rows_backward"), (autograd, "cross_rows"), (autograd, "iqm_visual_rows"))
P = 0x7f0000001000      # a plausible, 16-byte aligned device address: nothing here may be dereferenced
BIG = 1 << 40
PREFIX = b"cross_rows_backward:"


def test_symbols_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
        assert re.search(r"\b%s\(" % name, header)
    for mod, name in SURFACE:
        assert callable(getattr(mod, name))
    in_header = int(re.search(r"#define\s+AACLIP_ABI_VERSION\s+(\d+)", header).group(1))
    assert in_header == 10 and lib.aaclip_version() == 10 and _lib.ABI_VERSION == 10
    assert engine.CROSS_ROWS_BACKWARD_MAX_SLICES == CB.MAX_SLICES


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.cross_rows_backward(torch.zeros(4, 256), torch.zeros(10, 256), torch.zeros(4, 256), 1, 4, 10, engine.F32)


def test_workspace_bytes():
    ws = _lib.load().aaclip_cross_rows_backward_workspace_bytes
    for args in ((0, 16, 100, 768), (2, 0, 100, 768), (2, 16, 0, 768), (2, 16, 100, 0), (-1, 16, 100, 768)):
        assert ws(*args) == 0, args
    base = (2, 8, 5476, 512)
    assert ws(*base) > 0
    grids = ([1, 2, 3, 64, 65535], [4, 8, 12, 16], [1, 2, 63, 64, 65, 4096, 8191, 8192, 8193, 8256, 8257, 20000, 100000],
             [256, 512, 768, 1024])
    for i, values in enumerate(grids):
        sizes = [ws(*(base[:i] + (v,) + base[i + 1:])) for v in values]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (i, sizes)
        assert sizes[0] > 0
    # what the kernels index: SG [B, Lk, 32], statistics [B, 16, 4] and one partial of d_qt per slice
    for B, R, Lk, Dk in ((2, 16, 5476, 768), (2, 12, 64 * CB.MAX_SLICES + 1, 768), (1, 4, 1, 256)):
        per = 64 * -(-Lk // (64 * CB.MAX_SLICES))
        slices = -(-Lk // per)
        assert slices <= CB.MAX_SLICES
        assert ws(B, R, Lk, Dk) >= 4 * (B * Lk * 32 + B * 16 * 4 + B * slices * R * Dk)


def call(lib, x_dtype=0, qt=P, x=P, d_out=P, d_qt=P, d_x=P, act=0, accumulate=0, B=2, R=16, Lk=5476, Dk=768, ws=P,
         ws_bytes=BIG):
    return lib.aaclip_cross_rows_backward(x_dtype, qt, x, d_out, d_qt, d_x, act, accumulate, B, R, Lk, Dk, ws, ws_bytes,
                                          None)


def test_argument_errors():
    """Every check precedes the first launch: these calls carry addresses that are not memory."""
    lib = _lib.load()

    def failed(rc, word):
        msg = lib.aaclip_last_error()
        return rc < 0 and msg.startswith(PREFIX) and word in msg

    for n in ("qt", "x", "d_out", "ws"):
        assert failed(call(lib, **{n: None}), b"null"), n
    assert failed(call(lib, d_qt=None, d_x=None), b"both NULL")
    for n in ("qt", "x", "d_out", "d_qt", "d_x", "ws"):
        assert failed(call(lib, **{n: P + 4}), b"aligned"), n
    need = lib.aaclip_cross_rows_backward_workspace_bytes(2, 16, 5476, 768)
    assert failed(call(lib, ws_bytes=need - 1), b"workspace too small")
    assert failed(call(lib, ws_bytes=0), b"workspace too small")
    for kw in (dict(B=0), dict(R=0), dict(Lk=0), dict(Dk=0), dict(B=-3)):
        assert failed(call(lib, **kw), b"empty"), kw
    assert failed(call(lib, B=65536), b"grid limit")
    for R in (2, 6, 20):
        assert failed(call(lib, R=R), b"effective queries"), R
    for Dk in (128, 640, 2048):
        assert failed(call(lib, Dk=Dk), b"row width"), Dk
    assert failed(call(lib, x_dtype=3), b"dtype") and failed(call(lib, x_dtype=-1), b"dtype")
    assert failed(call(lib, act=3), b"activation") and failed(call(lib, act=-1), b"activation")


@pytest.mark.parametrize("name", list(CB.CASES))
def test_cases_are_well_conditioned(name):
    """fp32 CPU autograd of the reference stays within 2.5e-5 of fp64 on every case: what makes the GPU bar of 1e-4
    attainable on these inputs."""
    c = CB.CASES[name]
    t, want = CB.case(name)
    d_qt, d_x, _ = CB.autograd_reference(t["qt"], t["x"], t["d_out"], c["B"], c["R"], c["Lk"], c["Dk"], torch.float32)
    got = CB.want_of(name, d_qt, d_x, t)
    errs = {k: rel(got[k], w) for k, w in want.items() if w is not None and float(w.norm()) > 0}
    print(name, errs)
    assert all(v <= 2.5e-5 for v in errs.values()), errs
    if name == "one_key":
        assert not want["d_qt"].any() and not got["d_qt"].any()
    if c.get("act", CB.NONE) != CB.NONE:
        x = t["x"]
        assert (x < 0).any() and (x == 0).any(dim=1).all()
    if c.get("peak") is not None:
        s = t["qt"].double().view(c["B"], c["R"], -1) @ t["x"].double().view(c["B"], c["Lk"], -1).transpose(1, 2)
        assert float(s.max()) > 79 and float(s.min()) < -40
        assert float(torch.softmax(s, -1).amax(-1).median()) > 0.99          # most rows: one key holds the mass


@pytest.mark.parametrize("name", ["one_key", "ragged_tiles", "nearly_one_hot", "widest_rows"])
def test_step_sequence_reproduces_autograd(name):
    c = CB.CASES[name]
    t = CB.case_inputs(name)
    args = (t["qt"], t["x"], t["d_out"], c["B"], c["R"], c["Lk"], c["Dk"])
    d_qt, d_x = CB.step_sequence(*args)
    r_qt, r_x, _ = CB.autograd_reference(*args)
    assert rel(d_x, r_x) <= 1e-12
    assert rel(d_qt, r_qt) <= 1e-12 if float(r_qt.norm()) > 0 else not d_qt.any()


def test_fold_reference_ignores_the_key_bias():
    """The forward folds W_k into the query and drops b_k (one constant per query and head: softmax-invariant)."""
    _, _, d_wk, d_bk = CB.fold_reference()
    assert float(d_bk.norm()) <= 1e-12 * float(d_wk.norm())
