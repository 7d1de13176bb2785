"""The fused Adam / AdamW step and its gradient norm on the GPU (csrc/optim.hip, aaclip_hip/optim.py) over the sizes and
hyper-parameters of tests/optim_cases.py.

Error bars (measured against the reference's optimizer, not fixed): the truth is torch.optim.Adam / AdamW(foreach=False)
on the CPU in fp64 started from the same fp32 values; e_ref is the largest absolute error of the same torch optimizer in
fp32 against that truth, taken separately for p, exp_avg and exp_avg_sq over the case; the bar is
max(4 e_ref, 4 * 2^-24 * max |truth|): four for a different order of the same handful of roundings per element, the
floor four half-ulps of the largest element for the cases where torch happens to be exact.  For the norm the truth is
the fp64 norm and e_ref the error of clip_grad_norm_'s returned norm on the CPU in fp32.  Every measured error and bar
goes into conftest.PARITY_ERRORS under optim.* (committed as profiles/optim_parity_errors.json).

Everything else is equality of bits: all tensors in one step() against each tensor alone, two runs, a clipped step whose
coefficient is exactly 1 against the unclipped one, misaligned views against aligned storage, guard elements around
every p, m, v and the record, and the gradients after a clipped step."""
import logging

import numpy as np
import pytest
import torch

import optim_cases as OC
from aaclip_hip import engine, optim
from conftest import PARITY_ERRORS
from test_gpu_augment import _Losses, reduced_clip, run_args, tree  # noqa: F401  (tree is a fixture)

pytestmark = pytest.mark.gpu

GUARD = 4                      # fp32 elements in front of and behind every guarded tensor: 16 bytes keep the alignment
SENTINEL = -7.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the optimizer tests need an MI355X"
    return torch.device("cuda:0")


def guarded(values, dev, offset=0):
    """-> (buffer, view): the fp32 values on the device with GUARD (+ offset) sentinel elements in front and GUARD behind;
    offset 1 puts the view at a 4-byte aligned address"""
    n = values.numel()
    buf = torch.full((n + 2 * GUARD + offset,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[GUARD + offset:GUARD + offset + n]
    view.copy_(values)
    return buf, view


def guards_intact(buf, n, offset=0):
    head, tail = buf[:GUARD + offset], buf[GUARD + offset + n:]
    return bool((head == SENTINEL).all()) and bool((tail == SENTINEL).all()) and tail.numel() == GUARD


class Setup:
    """the case's parameters on the device, every p / g / m / v a view into a guarded buffer (the MISALIGNED tensor's four
    views at a storage offset of one element more), the moments installed as the optimizer's state"""

    def __init__(self, case, dev, loaded=False, misalign=True, lazy_state=False, **extra):
        p0, m0, v0, step0 = OC.initial(loaded)
        self.dev, self.sizes = dev, [t.numel() for t in p0]
        self.off = [1 if (misalign and i == OC.MISALIGNED) else 0 for i in range(len(p0))]
        self.bufs = {k: [] for k in "pgmv"}
        self.views = {k: [] for k in "pgmv"}
        for k, src in (("p", p0), ("m", m0), ("v", v0), ("g", [torch.zeros_like(t) for t in p0])):
            for t, off in zip(src, self.off):
                buf, view = guarded(t, dev, off)
                self.bufs[k].append(buf), self.views[k].append(view)
        self.params = [torch.nn.Parameter(v) for v in self.views["p"]]
        for p, v in zip(self.params, self.views["p"]):
            assert p.data_ptr() == v.data_ptr()
        self.opt = OC.build(OC.fused_class(case), self.params, case, **extra)
        if not lazy_state:
            for p, m, v in zip(self.params, self.views["m"], self.views["v"]):
                self.opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m, "exp_avg_sq": v}

    def set_grads(self, step, scale=0.02, poison=None):
        for i, (p, g) in enumerate(zip(self.params, OC.gradients(step, scale))):
            if g is None:
                p.grad = None
                continue
            self.views["g"][i].copy_(g)
            p.grad = self.views["g"][i]
        if poison is not None:
            self.views["g"][poison[0]][poison[1]] = float("inf")

    def run(self, steps, scale=0.02, poison=None):
        for s in range(steps):
            self.set_grads(s, scale, poison if s == 0 else None)
            self.opt.step()
        torch.cuda.synchronize()
        return self

    def result(self):
        return {"p": [p.detach() for p in self.params], "m": self.views["m"], "v": self.views["v"]}

    def check_guards(self):
        for k in "pgmv":
            for i, buf in enumerate(self.bufs[k]):
                assert guards_intact(buf, self.sizes[i], self.off[i]), (k, i, self.sizes[i])


def check_against_truth(name, got, truth, e_ref, bars, kinds="pmv"):
    """print and record every figure, then assert"""
    entry, failed = {}, []
    for k in kinds:
        err = OC.errors(got[k], truth[k])
        entry[k] = {"error": err, "e_ref": e_ref[k], "bar": bars[k]}
        print(f"{name} {k}: error {err:.3e}  e_ref {e_ref[k]:.3e}  bar {bars[k]:.3e}")
        if not err <= bars[k]:
            failed.append(k)
    PARITY_ERRORS["optim." + name] = entry
    assert not failed, (name, entry)


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# -------------------------------------------------------------------------------------------- against the truth
@pytest.mark.parametrize("loaded", [False, True], ids=["three_steps", "loaded_step_1000"])
@pytest.mark.parametrize("case", list(OC.HYPER))
def test_step_is_torchs_within_the_measured_bar(dev, case, loaded):
    truth, e_ref, bars = OC.reference(case, loaded)
    s = Setup(case, dev, loaded).run(1 if loaded else OC.STEPS)
    s.check_guards()
    assert s.opt.grad_norm is None
    # the grad-less and the empty parameter: values and state untouched, no step counted
    p0, m0, v0, step0 = OC.initial(loaded)
    for i in (OC.GRADLESS, OC.EMPTY):
        assert torch.equal(s.params[i].detach().cpu(), p0[i]) and torch.equal(s.views["m"][i].cpu(), m0[i])
        assert float(s.opt.state[s.params[i]]["step"]) == step0
    want = step0 + (1 if loaded else OC.STEPS)
    assert all(float(s.opt.state[p]["step"]) == want for i, p in enumerate(s.params) if i not in (OC.GRADLESS, OC.EMPTY))
    check_against_truth(f"{case}.{'loaded' if loaded else 'steps3'}", s.result(), truth, e_ref, bars)


def test_lazy_state_is_the_installed_zero_state(dev):
    """state created by step() itself (zeros_like) gives the bits of zero moments installed by hand"""
    a = Setup("stage2", dev).run(OC.STEPS)
    b = Setup("stage2", dev, lazy_state=True).run(OC.STEPS)
    assert same_bits(a.result()["p"], b.result()["p"])
    lazy = [b.opt.state[p] for i, p in enumerate(b.params) if i not in (OC.GRADLESS, OC.EMPTY)]
    assert all(st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and st["exp_avg"].is_cuda
               for st in lazy)
    assert b.params[OC.GRADLESS] not in b.opt.state and b.params[OC.EMPTY] not in b.opt.state


# ------------------------------------------------------------------------------------------------ equality of bits
def test_all_tensors_at_once_equal_each_tensor_alone(dev):
    """catches any chunk or table error: a tensor's result must not depend on its place in a launch"""
    case = "stage2"
    s = Setup(case, dev).run(1)
    groups = OC.param_groups(list(range(len(OC.SIZES))), case)
    alone = Setup(case, dev)
    alone.set_grads(0)
    for group in groups:
        for i in group["params"]:
            p = alone.params[i]
            if p.grad is None:
                continue
            one = optim.FusedAdamW([p], lr=group["lr"], weight_decay=group["weight_decay"], betas=OC.HYPER[case][2])
            one.state[p] = {"step": torch.tensor(0.0), "exp_avg": alone.views["m"][i], "exp_avg_sq": alone.views["v"][i]}
            one.step()
    torch.cuda.synchronize()
    for k in "pmv":
        assert same_bits(s.result()[k], alone.result()[k]), k
    alone.check_guards()


def test_two_runs_give_the_same_bits(dev):
    runs = [Setup("stage2", dev, max_grad_norm=0.01).run(OC.STEPS) for _ in range(2)]
    for k in "pmv":
        assert same_bits(runs[0].result()[k], runs[1].result()[k]), k
    assert same_bits([runs[0].opt._record], [runs[1].opt._record])
    assert float(runs[0].opt._record[1]) < 1.0           # the clipping was active


def test_a_coefficient_of_one_is_the_unclipped_step(dev):
    plain = Setup("stage2", dev).run(OC.STEPS)
    clipped = Setup("stage2", dev, max_grad_norm=1e6).run(OC.STEPS)
    assert float(clipped.opt._record[1]) == 1.0 and 0.0 < float(clipped.opt.grad_norm) < 1e6
    for k in "pmv":
        assert same_bits(plain.result()[k], clipped.result()[k]), k


def test_misaligned_views_equal_aligned_storage(dev):
    """the scalar path (p, g, m, v at a storage offset of one element) against the 16-byte path on the same values, in
    the same list and alone, with the clipping active"""
    for extra in ({}, {"max_grad_norm": 0.01}):
        a = Setup("coupled", dev, misalign=True, **extra).run(OC.STEPS)
        b = Setup("coupled", dev, misalign=False, **extra).run(OC.STEPS)
        i = OC.MISALIGNED
        assert a.params[i].data_ptr() % 16 == 4 and a.views["g"][i].data_ptr() % 16 == 4
        assert a.views["m"][i].data_ptr() % 16 == 4 and a.views["v"][i].data_ptr() % 16 == 4
        assert b.params[i].data_ptr() % 16 == 0
        for k in "pmv":
            assert same_bits(a.result()[k], b.result()[k]), (k, extra)
        a.check_guards()


def test_one_misaligned_pointer_is_enough_for_the_scalar_path(dev):
    """a tensor larger than a chunk whose gradient alone sits at a 4-byte aligned address"""
    n = 2 * OC.CHUNK + 5
    vals = OC.values(9, 0.05, [n] * 4)
    results = []
    for off in (0, 1):
        bufs, views = zip(*[guarded(t.abs() if j == 3 else t, dev, off if j == 1 else 0) for j, t in enumerate(vals)])
        p, g, m, v = views
        record = engine.optim_grad_norm([g], 0.5)
        engine.optim_adam_step([p], [g], [m], [v], [0], [{"lr": 1e-2, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8,
                                                           "weight_decay": 1e-2, "decoupled": False, "step": 7}], record)
        torch.cuda.synchronize()
        assert all(guards_intact(b, n, off if j == 1 else 0) for j, b in enumerate(bufs))
        assert torch.equal(g.cpu(), vals[1])
        results.append([p, m, v, record])
    assert results[1][0].data_ptr() % 16 == 0
    for x, y in zip(*results):
        assert same_bits([x], [y])


# ------------------------------------------------------------------------------------------------------ clipping
def test_grad_norm_record_and_guards(dev):
    """the raw call: norm and coefficient against fp64 with the bar of clip_grad_norm_'s own fp32 error; guard elements
    around the record and behind the workspace; the gradients unchanged; the same bits twice"""
    grads_cpu = [g for g in OC.gradients(0, 3.0) if g is not None]
    truth = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads_cpu)))
    ref32 = float(torch.nn.utils.clip_grad_norm_([_with_grad(g) for g in grads_cpu], 1.0, foreach=False))
    e_ref = abs(ref32 - truth)
    bar = max(4 * e_ref, 4 * 2.0 ** -24 * truth)
    grads = [g.to(dev) for g in grads_cpu]
    need = engine.OptimPack(None, grads).norm_workspace_bytes
    chunks = sum(-(-g.numel() // OC.CHUNK) for g in grads)
    assert need >= 8 * chunks and need % 256 == 0
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=dev)
    rec_buf = torch.full((6,), SENTINEL, dtype=torch.float32, device=dev)
    bits = []
    for max_norm in (1.0, 1.0, 1e9):
        record = engine.optim_grad_norm(grads, max_norm, rec_buf[2:4], ws[:need])
        torch.cuda.synchronize()
        norm, coef = float(record[0]), float(record[1])
        assert rec_buf[:2].tolist() == [SENTINEL] * 2 and rec_buf[4:].tolist() == [SENTINEL] * 2
        assert bool((ws[need:] == 0x5A).all())
        bits.append(record.clone().view(torch.int32).tolist())
        err = abs(norm - truth)
        print(f"grad norm: got {norm!r} truth {truth!r} error {err:.3e} e_ref {e_ref:.3e} bar {bar:.3e} coef {coef!r}")
        assert err <= bar
        want = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
        assert coef == (1.0 if want > 1 else float(want))
    PARITY_ERRORS["optim.grad_norm.raw"] = {"error": abs(float(rec_buf[2]) - truth), "e_ref": e_ref, "bar": bar,
                                            "truth": truth}
    assert bits[0] == bits[1] and bits[0][0] == bits[2][0] and truth > 50
    for g, c in zip(grads, grads_cpu):
        assert torch.equal(g.cpu(), c)
    # no gradients at all: norm 0, coefficient 1
    record = engine.optim_grad_norm([], 1.0, rec_buf[2:4], ws[:need])
    assert record.tolist() == [0.0, 1.0]


def _with_grad(g):
    p = torch.nn.Parameter(torch.zeros_like(g))
    p.grad = g.clone()
    return p


@pytest.mark.parametrize("case", ["stage2", "coupled"])
def test_active_clipping_is_clip_grad_norm_then_step(dev, case):
    """gradients scaled so that the norm is about 50 x max_norm; the truth clips with torch's formula (clip_grad_norm_
    in fp64), then steps"""
    max_norm, scale = 1.0, 0.17
    truth, e_ref, bars = OC.reference(case, False, scale, max_norm)
    assert 40 < float(truth["norms"][0]) / max_norm < 60
    s = Setup(case, dev, max_grad_norm=max_norm)
    norms = []
    for step in range(OC.STEPS):
        s.set_grads(step, scale)
        s.opt.step()
        norms.append(s.opt.grad_norm.clone())
        for i, g in enumerate(OC.gradients(step, scale)):           # the gradients in memory are not rescaled
            assert g is None or torch.equal(s.views["g"][i].cpu(), g)
    torch.cuda.synchronize()
    s.check_guards()
    got = dict(s.result(), norms=norms)
    check_against_truth(f"{case}.clipped", got, truth, e_ref, bars, kinds=["p", "m", "v", "norms"])


def test_one_inf_gradient_propagates_like_torchs(dev):
    """nothing faults, the norm is inf, and every stepped parameter has torch's finite-or-not pattern and, where finite,
    torch's values within the bar"""
    case, poison = "stage2", (9, OC.CHUNK + 1)                        # in the second chunk of the largest tensor
    truth, e_ref, bars = OC.reference(case, False, 0.02, 1.0, poison)
    assert torch.isinf(truth["norms"][0]) and torch.isfinite(truth["norms"][1])
    s = Setup(case, dev, max_grad_norm=1.0)
    s.set_grads(0, poison=poison)
    s.opt.step()
    assert torch.isinf(s.opt.grad_norm).item() and torch.isnan(s.opt._record[1]).item() is False
    assert float(s.opt._record[1]) == 0.0
    for step in (1, 2):
        s.set_grads(step)
        s.opt.step()
    torch.cuda.synchronize()
    s.check_guards()
    got = s.result()
    for k in "pmv":
        for i, (a, t) in enumerate(zip(got[k], truth[k])):
            assert torch.equal(torch.isfinite(a.cpu()), torch.isfinite(t)), (k, i)
            assert torch.equal(torch.isnan(a.cpu()), torch.isnan(t)), (k, i)
    assert not torch.isfinite(got["p"][poison[0]][poison[1]]) and int(sum((~torch.isfinite(p)).sum() for p in got["p"])) == 1
    check_against_truth("stage2.one_inf", got, truth, e_ref, bars)


# ---------------------------------------------------------------------------------------------------- end to end
def _fused_args(save, image_epoch=1, **extra):
    args = run_args(save, False)
    vars(args).update(image_epoch=image_epoch, **extra)
    return args


def _trained(model):
    """{name: clone} of the parameters of the two stage-2 groups' first modules and of the text adapters"""
    return {part: {k: v.detach().clone() for k, v in getattr(model, part).named_parameters()}
            for part in ("image_adapter", "iqm", "text_adapter")}


def _moved(a, b):
    return any(not torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


FUSED = dict(fused_optimizer=True, clip_grad_norm=1.0)
HOW = dict(model_factory=reduced_clip, levels=[2, 3])


@pytest.fixture()
def train_log():
    seen = _Losses()
    logger = logging.getLogger("train")
    logger.setLevel(logging.INFO)
    logger.addHandler(seen)
    yield seen
    logger.removeHandler(seen)


def test_train_run_with_the_fused_optimizer(dev, tree, tmp_path, monkeypatch, train_log):  # noqa: F811
    """1 + 1 epochs with fused_optimizer and clip_grad_norm set on the namespace: finite losses, a parameter of each
    group moves, the checkpoint has torch's layout, and the run resumes from it to the same bits"""
    import train
    starts, stage1 = [], train.train_text_adapter

    def spy(adapted_model, **kw):                        # the weights before anything trains
        starts.append(_trained(adapted_model))
        return stage1(adapted_model=adapted_model, **kw)
    monkeypatch.setattr(train, "train_text_adapter", spy)
    monkeypatch.setattr(train, "NUM_WORKERS", 0)         # the optimizer is under test: no loader processes to fork
    save = tmp_path / "fused"
    model = train.run(_fused_args(save, **FUSED), **HOW)
    losses, first = list(train_log.values), _trained(model)
    ckpt = torch.load(save / "image_adapter.pth")
    text_ckpt = torch.load(save / "text_adapter.pth")
    again = train.run(_fused_args(save, **FUSED), **HOW)                # resumes: nothing is left to train
    print("fused losses", losses)
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses) and train_log.values == losses
    for part in first:                                   # a parameter of each group (and of stage 1) moved
        assert _moved(first[part], starts[0][part]), part
        assert all(bool(torch.isfinite(v).all()) for v in first[part].values())
    for name, state, groups in (("image", ckpt["image_optimizer"], 2), ("text", text_ckpt["text_optimizer"], 1)):
        assert set(state) == {"state", "param_groups"} and len(state["param_groups"]) == groups, name
        # torch's keys; CosineAnnealingLR adds "initial_lr" to the groups of the optimizer it schedules
        assert set(state["param_groups"][0]) - {"initial_lr"} == set(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))])
                                                    .state_dict()["param_groups"][0]), name
        assert set(state["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(state["state"][0]["step"]) >= 1
        assert state["state"][0]["step"].dtype == torch.float32 and state["state"][0]["exp_avg"].dtype == torch.float32
    for k, v in ckpt["image_adapter"].items():
        assert torch.equal(again.image_adapter.state_dict()[k].cpu(), v.cpu()), k
        assert torch.equal(model.image_adapter.state_dict()[k].cpu(), v.cpu()), k
    for k, v in ckpt["iqm_branch"]["iqm"].items():
        assert torch.equal(again.iqm.state_dict()[k].cpu(), v.cpu()), k
    for k, v in text_ckpt["text_adapter"].items():
        assert torch.equal(again.text_adapter.state_dict()[k].cpu(), v.cpu()), k


def test_fused_run_resumes_from_torchs_checkpoint(dev, tree, tmp_path, train_log, monkeypatch):  # noqa: F811
    """a run without the attributes (torch.optim.AdamW) writes the checkpoint; a second epoch with them loads that
    optimizer state into FusedAdamW and goes on from its step counts"""
    import train
    monkeypatch.setattr(train, "NUM_WORKERS", 0)         # the optimizer is under test: no loader processes to fork
    save = tmp_path / "torch"
    few = dict(text_batch_size=6, image_batch_size=6)               # two steps per epoch: the state is what matters
    train.run(_fused_args(save, **few), **HOW)
    torch_ckpt = torch.load(save / "image_adapter.pth")
    steps = float(torch_ckpt["image_optimizer"]["state"][0]["step"])
    before = len(train_log.values)
    crossed = train.run(_fused_args(save, 2, **few, **FUSED), **HOW)
    ckpt = torch.load(save / "image_adapter.pth")
    losses = train_log.values[before:]
    print("torch losses", train_log.values[:before], "then fused", losses)
    assert steps >= 1 and ckpt["epoch"] == 2 and len(losses) == 1 and np.isfinite(losses[0])
    assert float(ckpt["image_optimizer"]["state"][0]["step"]) == 2 * steps
    assert set(ckpt["image_optimizer"]["state"]) == set(torch_ckpt["image_optimizer"]["state"])
    moved = _trained(crossed)
    assert _moved(moved["image_adapter"], {k: torch_ckpt["image_adapter"][k] for k in moved["image_adapter"]})
    assert _moved(moved["iqm"], {k: torch_ckpt["iqm_branch"]["iqm"][k] for k in moved["iqm"]})
    assert all(bool(torch.isfinite(v).all()) for part in moved.values() for v in part.values())
