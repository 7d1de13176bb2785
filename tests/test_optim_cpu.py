"""CPU side of the fused optimizer (csrc/optim.hip, aaclip_hip/optim.py): the launch packing of csrc/optim_pack.h as a
host program of its own under AddressSanitizer + UBSan; every refusal of the C entries that returns before touching the
device, and of FusedAdam / FusedAdamW; torch's state_dict layout and the round trip with torch.optim.AdamW; the parsers
of train.py (unchanged) and train_fused.py; FusedAdamW.step() on fp64 stand-ins for the two engine calls against
torch.optim.AdamW in fp64 with a CosineAnnealingLR.

Bound of the stand-in run: parameters and moments are stored in fp32 after every step, one rounding of relative size
2^-24 each, and a rounding of m or v moves p by at most lr / bc1-weighted fractions of the same size; over three steps
the distance from torch in fp64 stays below 3 * 4 * 2^-24 * max |value| per kind of tensor, and 1e-6 * lr-sized updates
on top for p (|update| <= lr * a few)."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

import optim_cases as OC
from aaclip_hip import _lib, engine, optim

REPO = os.path.join(os.path.dirname(__file__), "..")
CSRC = os.path.join(REPO, "aa-clip-iqm_amd", "csrc")
NEW_SYMBOLS = ["aaclip_optim_grad_norm_workspace_bytes", "aaclip_optim_grad_norm", "aaclip_optim_adam_step"]
P, G, M, V, REC, WS = (0x7f0000001000 + 0x100000 * i for i in range(6))     # never dereferenced: refused before a launch


# ----------------------------------------------------------------------------------------------- launch packing
def test_launch_packing_under_the_sanitizers(tmp_path):
    """csrc/optim_pack.h as optim.hip uses it, in a host program with ASan + UBSan over adversarial count lists: every
    element in exactly one chunk, no table overflows, no report from either sanitizer"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "optim_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(CSRC, "optim_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime of the host compiler is not installed: " + build.stderr.strip()[-200:])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "all ok" in run.stdout and "FAIL" not in run.stdout and "runtime error" not in run.stderr
    for name in ("empty", "zeros", "ones", "chunk edges", "larger than a launch", "table + 1 tensors", "many tables"):
        assert name in run.stdout


def test_the_python_constants_are_the_headers():
    pack = open(os.path.join(CSRC, "optim_pack.h")).read()
    assert f"OPTIM_CHUNK = {OC.CHUNK};" in pack and f"OPTIM_TABLE_TENSORS = {OC.TABLE_TENSORS};" in pack
    assert f"OPTIM_TABLE_BLOCKS = {OC.TABLE_BLOCKS};" in pack
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    assert f"#define AACLIP_OPTIM_MAX_GROUPS {_lib.OPTIM_MAX_GROUPS}\n" in header
    assert "#define AACLIP_ABI_VERSION 10 " in header and _lib.ABI_VERSION == 10
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name + "(" in header and getattr(lib, name)
    # the size-tagged struct and its items as the header lays them out (LP64)
    assert ctypes.sizeof(_lib.OptimTensor) == 48 and ctypes.sizeof(_lib.OptimTensors) == 24
    assert ctypes.sizeof(_lib.OptimGroup) == 56


# ------------------------------------------------------------------------------------------- C entry refusals
def _tensors(rows):
    items = (_lib.OptimTensor * max(len(rows), 1))(*rows)
    return _lib.OptimTensors(items=items, count=len(rows)), items


def _groups(*rows):
    rows = rows or ((1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1),)
    return (_lib.OptimGroup * len(rows))(*rows)


def test_c_entries_refuse_bad_arguments():
    lib = _lib.load()

    def no(rc, word):
        assert rc == -1 and word in lib.aaclip_last_error(), (rc, lib.aaclip_last_error())

    good, keep = _tensors([(P, G, M, V, 100, 0)])
    ref = ctypes.byref
    # ---- grad norm
    no(lib.aaclip_optim_grad_norm(None, 1.0, REC, WS, 4096, None), b"tensors is null")
    for size in (0, 16, 32):
        bad, _k = _tensors([(P, G, M, V, 100, 0)])
        bad.struct_bytes = size
        no(lib.aaclip_optim_grad_norm(ref(bad), 1.0, REC, WS, 4096, None), b"struct_bytes")
        no(lib.aaclip_optim_adam_step(ref(bad), _groups(), 1, None, None), b"struct_bytes")
        assert lib.aaclip_optim_grad_norm_workspace_bytes(ref(bad)) == 0
    bad, _k = _tensors([(P, G, M, V, 100, 0)])
    bad.count = -1
    no(lib.aaclip_optim_grad_norm(ref(bad), 1.0, REC, WS, 4096, None), b"count is negative")
    bad = _lib.OptimTensors(items=None, count=3)
    no(lib.aaclip_optim_grad_norm(ref(bad), 1.0, REC, WS, 4096, None), b"items is null")
    no(lib.aaclip_optim_grad_norm(ref(_tensors([(P, G, M, V, -1, 0)])[0]), 1.0, REC, WS, 4096, None), b"n < 0")
    no(lib.aaclip_optim_grad_norm(ref(_tensors([(P, G, M, V, 2 ** 27 * OC.CHUNK, 0)])[0]), 1.0, REC, WS, 4096, None),
       b"more than")
    no(lib.aaclip_optim_grad_norm(ref(_tensors([(P, None, M, V, 5, 0)])[0]), 1.0, REC, WS, 4096, None), b"null pointer")
    no(lib.aaclip_optim_grad_norm(ref(_tensors([(P, G + 2, M, V, 5, 0)])[0]), 1.0, REC, WS, 4096, None), b"4-byte")
    for bad_norm in (0.0, -1.0, float("nan")):
        no(lib.aaclip_optim_grad_norm(ref(good), bad_norm, REC, WS, 4096, None), b"max_norm")
    no(lib.aaclip_optim_grad_norm(ref(good), 1.0, None, WS, 4096, None), b"null pointer")
    no(lib.aaclip_optim_grad_norm(ref(good), 1.0, REC, None, 4096, None), b"null pointer")
    no(lib.aaclip_optim_grad_norm(ref(good), 1.0, REC + 4, WS, 4096, None), b"8-byte")
    no(lib.aaclip_optim_grad_norm(ref(good), 1.0, REC, WS, 8, None), b"too small")
    no(lib.aaclip_optim_grad_norm(ref(good), 1.0, WS + 8, WS, 4096, None), b"overlap")
    # a gradient-less list entry with n == 0 needs no pointer; the workspace size counts chunks and never shrinks
    sizes = [lib.aaclip_optim_grad_norm_workspace_bytes(ref(_tensors([(None, None, None, None, n, 0)] * k)[0]))
             for n, k in ((0, 1), (1, 1), (OC.CHUNK, 1), (OC.CHUNK + 1, 1), (OC.CHUNK + 1, 40), (OC.CHUNK * 1000, 3))]
    assert sizes[0] >= 8 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    assert sizes[4] >= 80 * 8 and sizes[5] >= 3000 * 8
    assert lib.aaclip_optim_grad_norm_workspace_bytes(None) == 0
    assert lib.aaclip_optim_grad_norm_workspace_bytes(ref(_tensors([(None, None, None, None, -1, 0)])[0])) == 0
    # ---- adam step
    no(lib.aaclip_optim_adam_step(None, _groups(), 1, None, None), b"tensors is null")
    no(lib.aaclip_optim_adam_step(ref(good), None, 1, None, None), b"groups is null")
    nine = _groups(*[(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1)] * 9)
    for count in (0, -1, 9):
        no(lib.aaclip_optim_adam_step(ref(good), nine, count, None, None), b"n_groups")
    for group in (-1, 1, 8):
        no(lib.aaclip_optim_adam_step(ref(_tensors([(P, G, M, V, 5, group)])[0]), _groups(), 1, None, None),
           b"group index")
    for row in ((None, G, M, V), (P, None, M, V), (P, G, None, V), (P, G, M, None)):
        no(lib.aaclip_optim_adam_step(ref(_tensors([row + (5, 0)])[0]), _groups(), 1, None, None), b"null pointer")
    for row in ((P + 1, G, M, V), (P, G, M + 2, V), (P, G, M, V + 3)):
        no(lib.aaclip_optim_adam_step(ref(_tensors([row + (5, 0)])[0]), _groups(), 1, None, None), b"4-byte")
    no(lib.aaclip_optim_adam_step(ref(_tensors([(P, G, M, V, -3, 0)])[0]), _groups(), 1, None, None), b"n < 0")
    for step in (0, -5):
        no(lib.aaclip_optim_adam_step(ref(good), _groups((1e-3, 0.9, 0.999, 1e-8, 0.0, 1, step)), 1, None, None),
           b"step must be")
    inf, nan = float("inf"), float("nan")
    for row in ((-1e-3, 0.9, 0.999, 1e-8, 0.0), (inf, 0.9, 0.999, 1e-8, 0.0), (nan, 0.9, 0.999, 1e-8, 0.0),
                (1e-3, 0.9, 0.999, -1e-8, 0.0), (1e-3, 0.9, 0.999, 1e-8, -0.1), (1e-3, 0.9, 0.999, 1e-8, nan)):
        no(lib.aaclip_optim_adam_step(ref(good), _groups(row + (1, 1)), 1, None, None), b"finite and not negative")
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, nan)):
        no(lib.aaclip_optim_adam_step(ref(good), _groups((1e-3, b1, b2, 1e-8, 0.0, 1, 1)), 1, None, None), b"betas")
    no(lib.aaclip_optim_adam_step(ref(good), _groups((1e-3, 0.9, 0.999, 1e-8, 0.0, 2, 1)), 1, None, None), b"decoupled")
    no(lib.aaclip_optim_adam_step(ref(good), _groups(), 1, REC + 4, None), b"8-byte")
    # the second group is checked although no tensor uses it
    no(lib.aaclip_optim_adam_step(ref(good), _groups((1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1),
                                                      (1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0)), 2, None, None), b"step must be")
    del keep


def test_engine_calls_refuse_before_any_launch():
    """CPU tensors, other dtypes, non-contiguous views, unequal lists, too many groups: all raise in Python"""
    t = torch.zeros(8)
    h = {"lr": 1e-3, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "weight_decay": 0.0, "decoupled": True, "step": 1}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.optim_grad_norm([t], 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        engine.optim_adam_step([t], [t], [t], [t], [0], [h])
    with pytest.raises(TypeError):
        engine.optim_grad_norm([None], 1.0)
    with pytest.raises(ValueError, match="equally long"):
        engine.optim_adam_step([t], [t, t], [t], [t], [0], [h])
    with pytest.raises(ValueError, match="groups per call"):
        engine.optim_adam_step([t], [t], [t], [t], [0], [h] * 9)
    with pytest.raises(ValueError, match="groups per call"):
        engine.optim_adam_step([t], [t], [t], [t], [0], [])


def test_engine_calls_refuse_dtype_layout_and_shape(monkeypatch):
    monkeypatch.setattr(engine, "require_gpu", lambda t, what: None)      # reach the checks behind the device check
    t = torch.zeros(4, 4)
    h = {"lr": 1e-3, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "weight_decay": 0.0, "decoupled": True, "step": 1}
    for bad in (t.double(), t.half(), t.bfloat16()):
        with pytest.raises(TypeError, match="fp32"):
            engine.optim_grad_norm([bad], 1.0)
        with pytest.raises(TypeError, match="fp32"):
            engine.optim_adam_step([t], [t], [bad], [t], [0], [h])
    with pytest.raises(ValueError, match="contiguous"):
        engine.optim_grad_norm([t.t()], 1.0)
    with pytest.raises(ValueError, match="contiguous"):
        engine.optim_adam_step([t[:, ::2]], [t[:, ::2]], [t[:, ::2]], [t[:, ::2]], [0], [h])
    with pytest.raises(ValueError, match="does not match"):
        engine.optim_adam_step([t], [torch.zeros(16)], [t], [t], [0], [h])
    with pytest.raises(ValueError, match="group index"):
        engine.optim_adam_step([t], [t], [t], [t], [1], [h])
    for bad_norm in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            engine.optim_grad_norm([t], bad_norm)


# --------------------------------------------------------------------------------------- FusedAdam / FusedAdamW
@pytest.mark.parametrize("cls", [optim.FusedAdam, optim.FusedAdamW])
def test_constructor_refusals(cls):
    p = [torch.nn.Parameter(torch.zeros(3))]
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=flag):
            cls(p, **{flag: True})
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            cls(p, **bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            cls(p, max_grad_norm=bad)
    with pytest.raises(NotImplementedError, match="tensor lr"):
        cls(p, lr=torch.tensor(1e-3))
    assert cls(p).max_grad_norm is None and cls(p, max_grad_norm=2).max_grad_norm == 2.0 and cls(p).grad_norm is None


def test_step_refuses_before_any_launch_and_before_any_state_change(monkeypatch):
    calls = {}
    a = torch.nn.Parameter(torch.zeros(4))               # the real device check: CPU parameters are refused
    a.grad = torch.ones(4)
    opt = optim.FusedAdamW([a])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert len(opt.state) == 0
    OC.install_standins(monkeypatch, calls)

    def refused(good, bad, error, word):
        """a good parameter in front of the bad one: nothing may have been stepped or initialised"""
        opt = optim.FusedAdamW([good, bad], max_grad_norm=1.0)
        before = good.detach().clone()
        with pytest.raises(error, match=word):
            opt.step()
        assert torch.equal(good.detach(), before) and len(opt.state) == 0 and calls == {}

    def param(t, grad):
        p = torch.nn.Parameter(t)
        p.grad = grad
        return p

    good = param(torch.ones(5), torch.ones(5))
    refused(good, param(torch.ones(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)), TypeError, "fp32")
    refused(good, param(torch.ones(3, dtype=torch.float16), torch.ones(3, dtype=torch.float16)), TypeError, "fp32")
    refused(good, param(torch.ones(4, 4).t(), torch.ones(4, 4)), ValueError, "contiguous")
    refused(good, param(torch.ones(4, 4), torch.ones(4, 4).t()), ValueError, "contiguous")
    sparse = param(torch.ones(4), None)
    sparse.grad = torch.sparse_coo_tensor([[1]], [1.0], (4,))
    refused(good, sparse, ValueError, "dense")
    opt = optim.FusedAdamW([good])
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.step()
    assert calls == {}


@pytest.mark.parametrize("case", ["stage1", "stage2"])
def test_state_dict_has_torchs_layout(monkeypatch, case):
    OC.install_standins(monkeypatch)
    sizes = [5, 1, 12, 7]
    monkeypatch.setitem(OC.HYPER, "stage2", ("AdamW", [(0, 5e-4, 1e-4), (2, 5e-5, 1e-3)], (0.9, 0.999)))
    dicts = []
    for cls in (OC.torch_class(case), OC.fused_class(case)):
        params = [torch.nn.Parameter(t) for t in OC.values(4, 0.1, sizes)]
        opt = OC.build(cls, params, case)
        for p, g in zip(params, OC.values(5, 0.1, sizes)):
            p.grad = g
        opt.step()
        dicts.append(opt.state_dict())
    theirs, ours = dicts
    assert set(ours) == set(theirs) == {"state", "param_groups"}
    assert len(ours["param_groups"]) == len(theirs["param_groups"])
    for a, b in zip(ours["param_groups"], theirs["param_groups"]):
        assert a == b                                    # the same keys and the same values, params indices included
    assert set(ours["state"]) == set(theirs["state"]) == set(range(len(sizes)))
    for i in theirs["state"]:
        assert set(ours["state"][i]) == set(theirs["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for k, v in theirs["state"][i].items():
            got = ours["state"][i][k]
            assert got.dtype == v.dtype and got.shape == v.shape and got.device == v.device, (i, k)
        assert ours["state"][i]["step"].dtype == torch.float32 and float(ours["state"][i]["step"]) == 1.0


def _follow(opt, params, steps, first=0):
    for s in range(first, first + steps):
        for p, g in zip(params, OC.values(50 + s, 0.02, [t.numel() for t in params])):
            p.grad = g.to(p.dtype)
        opt.step()


def test_round_trip_with_torchs_adamw(monkeypatch):
    """two steps under one class, the state through state_dict() / load_state_dict(), one more step under the other: the
    same as three steps of torch.optim.AdamW in fp64, both ways"""
    OC.install_standins(monkeypatch)
    sizes = [9, 1, 33]
    start = OC.values(6, 0.1, sizes)
    truth = [torch.nn.Parameter(t.double()) for t in start]
    topt = torch.optim.AdamW(truth, lr=1e-2, weight_decay=1e-2, foreach=False)
    _follow(topt, truth, 3)
    for first, second in ((torch.optim.AdamW, optim.FusedAdamW), (optim.FusedAdamW, torch.optim.AdamW)):
        params = [torch.nn.Parameter(t.clone()) for t in start]
        a = first(params, lr=1e-2, weight_decay=1e-2)
        _follow(a, params, 2)
        saved = a.state_dict()
        b = second(params, lr=1e-2, weight_decay=1e-2)
        b.load_state_dict(saved)
        assert all(float(b.state[p]["step"]) == 2.0 for p in params)
        assert all(b.state[p]["step"].device.type == "cpu" and b.state[p]["step"].dtype == torch.float32 for p in params)
        _follow(b, params, 1, first=2)
        assert all(float(b.state[p]["step"]) == 3.0 for p in params)
        for p, t in zip(params, truth):
            bound = 12 * 2.0 ** -24 * float(t.detach().abs().max()) + 3e-2 * 1e-6
            diff = float((p.detach().double() - t.detach()).abs().max())
            print(first.__name__, "->", second.__name__, "diff", diff, "bound", bound)
            assert diff <= bound
            for k in ("exp_avg", "exp_avg_sq"):
                want = topt.state[t][k]
                assert float((b.state[p][k].double() - want).abs().max()) <= 12 * 2.0 ** -24 * float(want.abs().max())


def test_step_follows_torch_with_a_cosine_schedule(monkeypatch):
    """the two reference groups, three steps, lr from CosineAnnealingLR at every step; a grad-less parameter and an empty
    one are skipped, state untouched; one grad-norm call and one step call per step()"""
    calls = {}
    OC.install_standins(monkeypatch, calls)
    sizes = [17, 4, 0, 40, 6]
    gradless, empty = 1, 2
    start = OC.values(8, 0.1, sizes)

    def make(cls, dtype, **extra):
        params = [torch.nn.Parameter(t.to(dtype)) for t in start]
        opt = cls([{"params": params[:3], "lr": 5e-4, "weight_decay": 1e-4},
                   {"params": params[3:], "lr": 5e-5, "weight_decay": 1e-3}], betas=(0.9, 0.999), **extra)
        return params, opt, torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=3, eta_min=1e-6)

    tp, topt, tsched = make(torch.optim.AdamW, torch.float64, foreach=False)
    fp, fopt, fsched = make(optim.FusedAdamW, torch.float32, max_grad_norm=0.05)
    for s in range(3):
        grads = OC.values(60 + s, 0.02, sizes)
        for plist, dtype in ((tp, torch.float64), (fp, torch.float32)):
            for i, (p, g) in enumerate(zip(plist, grads)):
                p.grad = None if i == gradless else g.to(dtype)
        norm = torch.nn.utils.clip_grad_norm_(tp, 0.05, foreach=False)
        assert float(norm) > 0.05                        # the clipping is active
        topt.step(), tsched.step()
        fopt.step(), fsched.step()
        assert calls == {"optim_grad_norm": s + 1, "optim_adam_step": s + 1}
        assert abs(float(fopt.grad_norm) - float(norm)) <= 2.0 ** -23 * float(norm)
        assert [g["lr"] for g in fopt.param_groups] == [g["lr"] for g in topt.param_groups]
        for i, g in enumerate(grads):                    # unlike clip_grad_norm_, the gradients stay as they are
            assert i == gradless or torch.equal(fp[i].grad, g)
    assert fopt.param_groups[0]["lr"] != 5e-4
    for i, (p, t) in enumerate(zip(fp, tp)):
        if i in (gradless, empty):
            assert p not in fopt.state or len(fopt.state[p]) == 0
            assert torch.equal(p.detach(), start[i])
            continue
        assert float(fopt.state[p]["step"]) == 3.0
        bound = 12 * 2.0 ** -24 * float(t.detach().abs().max()) + 3 * 5e-4 * 1e-6
        diff = float((p.detach().double() - t.detach()).abs().max())
        print("tensor", i, "diff", diff, "bound", bound)
        assert diff <= bound


def test_parameters_at_different_steps_cost_one_call_per_eight_sets(monkeypatch):
    """ten parameters of one group that have taken 1 .. 10 steps: ten hyper-parameter sets, two step calls"""
    calls = {}
    OC.install_standins(monkeypatch, calls)
    params = [torch.nn.Parameter(torch.ones(3)) for _ in range(10)]
    opt = optim.FusedAdam(params, lr=1e-2)
    for s in range(10):
        for i, p in enumerate(params):
            p.grad = torch.full((3,), 0.5) if i <= s else None
        opt.step()
    assert [int(opt.state[p]["step"]) for p in params] == list(range(10, 0, -1))
    assert calls == {"optim_adam_step": 8 + 2 * 2}       # up to eight sets: one call; nine and ten sets: two calls
    ref = [torch.nn.Parameter(torch.ones(3, dtype=torch.float64)) for _ in range(10)]
    ropt = torch.optim.Adam(ref, lr=1e-2, foreach=False)
    for s in range(10):
        for i, p in enumerate(ref):
            p.grad = torch.full((3,), 0.5, dtype=torch.float64) if i <= s else None
        ropt.step()
    for p, r in zip(params, ref):
        assert float((p.detach().double() - r.detach()).abs().max()) <= 10 * 4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------- the parsers
def _actions(parser):
    return {a.dest: (tuple(a.option_strings), a.default, a.type, a.nargs, tuple(a.choices) if a.choices else None,
                     type(a).__name__) for a in parser._actions}


def test_train_fused_parser_is_trains_plus_two(capsys):
    import train
    import train_fused
    base, fused = _actions(train.build_parser()), _actions(train_fused.build_parser())
    assert set(fused) - set(base) == {"fused_optimizer", "clip_grad_norm"}
    assert {k: fused[k] for k in base} == base
    assert fused["fused_optimizer"][1] is False and fused["clip_grad_norm"][1] is None
    # train.build_parser() itself: the reference's arguments plus device_augment, as before
    assert set(base) == set(train.ARGUMENTS) | {"help", "relu", "training_mode", "criterion", "device_augment"}
    args = train_fused.build_parser().parse_args(["--fused_optimizer", "--clip_grad_norm", "1.0"])
    assert args.fused_optimizer is True and args.clip_grad_norm == 1.0
    for argv in (["--clip_grad_norm", "1.0"], ["--fused_optimizer", "--clip_grad_norm", "0"],
                 ["--fused_optimizer", "--clip_grad_norm", "-1"]):
        with pytest.raises(SystemExit):
            train_fused.main(argv)
        assert "clip_grad_norm" in capsys.readouterr().err
    assert callable(train_fused.main) and train_fused.main.__defaults__ == (None,)


def test_train_run_reads_the_two_attributes(monkeypatch, tmp_path):
    """run() builds both optimizers from aaclip_hip.optim when fused_optimizer is set, hands the clipping value to the
    stage-2 one alone, and builds torch's own without the attributes: seen through the constructors, with the run cut
    short where the resume logic begins"""
    import train
    built = []

    class Stop(Exception):
        pass

    def spy(name, cls):
        def make(params, **kw):
            built.append((name, cls, kw.get("max_grad_norm", "absent")))
            return cls([torch.nn.Parameter(torch.zeros(1))], **kw)
        return make

    monkeypatch.setattr(torch.optim, "Adam", spy("Adam", torch.optim.Adam))
    monkeypatch.setattr(torch.optim, "AdamW", spy("AdamW", torch.optim.AdamW))
    monkeypatch.setattr(optim, "FusedAdam", spy("FusedAdam", optim.FusedAdam))
    monkeypatch.setattr(optim, "FusedAdamW", spy("FusedAdamW", optim.FusedAdamW))

    def stop(*a, **kw):
        raise Stop()
    monkeypatch.setattr(torch.optim.lr_scheduler, "CosineAnnealingLR", stop)
    from aaclip_hip import synth
    import visual_backward_cases as VB

    def factory(model_name, img_size, device, pretrained, require_pretrained):
        cfg = synth.tiny_cfg()
        cfg.image_size = img_size
        return VB.build_clip(cfg, "fp32", 7)[1].to(device)

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for extra, want in (({}, [("Adam", "absent"), ("AdamW", "absent")]),
                        ({"fused_optimizer": False}, [("Adam", "absent"), ("AdamW", "absent")]),
                        ({"fused_optimizer": True}, [("FusedAdam", "absent"), ("FusedAdamW", None)]),
                        ({"fused_optimizer": True, "clip_grad_norm": 1.5}, [("FusedAdam", "absent"), ("FusedAdamW", 1.5)])):
        args = train.build_parser().parse_args([])
        vars(args).update(img_size=VB.TAPS_IMAGE, surgery_until_layer=3, save_path=str(tmp_path / "ckpt"),
                          text_adapt_until=1, image_adapt_until=VB.TAPS_UNTIL, iqm_hidden_size=256, **extra)
        built.clear()
        with pytest.raises(Stop):
            train.run(args, model_factory=factory, levels=VB.TAPS_LEVELS)
        assert [(name, clip) for name, _, clip in built] == want, (extra, built)
    args = train.build_parser().parse_args([])
    vars(args).update(img_size=VB.TAPS_IMAGE, surgery_until_layer=3, save_path=str(tmp_path / "ckpt"),
                      text_adapt_until=1, image_adapt_until=VB.TAPS_UNTIL, iqm_hidden_size=256, clip_grad_norm=1.0)
    with pytest.raises(ValueError, match="needs fused_optimizer"):
        train.run(args, model_factory=factory, levels=VB.TAPS_LEVELS)
