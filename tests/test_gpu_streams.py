"""The stream contract of include/aaclip.h -- "`stream` is a hipStream_t passed as void*; every call only enqueues work
on it" -- exercised for every case of tests/stream_cases.py: on the default stream, on a side stream, under capture
(recording must execute nothing) and as a graph replayed on new data.  The library's sums are fixed-order, so every
comparison is on the raw bytes.  What a numerical test cannot see shows here: a memset or a stage enqueued on another
stream than the caller's, a host-side decision that reads device data, work left outside the stream, a call that relies
on what its previous run left in the workspace.

One stream per capture, no fork or join inside it (the graph is a linear chain), at most one graph alive per test.
The engine-level test captures the tiny CLIP's encode_image the way tools/graph_probe.py does."""
import gc

import pytest
import torch

import stream_cases as SC
from aaclip_hip import _lib, engine, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def raw(t):
    return t.contiguous().view(torch.uint8)


def same(a, b):
    return torch.equal(raw(a), raw(b))


def err(lib):
    m = lib.aaclip_last_error()
    return m.decode() if m else ""


def run_stream_case(case, dev, what):
    lib = _lib.load()
    default = torch.cuda.current_stream(dev)
    differ, fixed = case.results()
    everything = differ + fixed

    def snapshot():
        return [t.clone() for t in everything]

    def assert_results(ref, step):
        for i, (t, r) in enumerate(zip(everything, ref)):
            assert same(t, r), f"{what}: result {i} after {step} differs from the default-stream run"

    def assert_poison(step):
        for i, t in enumerate(case.outputs + case.fixed + case.scratch):
            assert bool((raw(t) == SC.POISON).all()), f"{what}: {step} wrote output / scratch buffer {i}"
        for i, (t, v) in enumerate(case.state):
            assert same(t.cpu(), v), f"{what}: {step} changed state tensor {i}"

    # 1. default stream, X then Y
    refs = []
    for which in (0, 1):
        case.poison()
        case.load(which)
        rc = case.call(default.cuda_stream)
        assert rc == 0, f"{what}: rc {rc}: {err(lib)}"
        torch.cuda.synchronize(dev)
        refs.append(snapshot())
    for i in range(len(differ)):
        assert not same(refs[0][i], refs[1][i]), f"{what}: result {i} is the same for X and Y: fix the case's inputs"

    # 2. side stream (also the warm-up that loads the code objects before any capture)
    s = torch.cuda.Stream(dev)
    s.wait_stream(default)
    with torch.cuda.stream(s):
        case.poison()
        case.load(0)
        rc = case.call(s.cuda_stream)
    assert rc == 0, f"{what}: side stream: rc {rc}: {err(lib)}"
    s.synchronize()
    assert_results(refs[0], "the side-stream run")

    # 3. capture: recording executes nothing
    with torch.cuda.stream(s):
        case.poison()
        case.load(0)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=s):
            rc = case.call(s.cuda_stream)
        assert rc == 0, f"{what}: under capture: rc {rc}: {err(lib)}"
        torch.cuda.synchronize(dev)
        assert_poison("the capture")

        # 4. replay with new data, twice; the second time over poisoned scratch and outputs
        for step in ("the first replay", "the second replay"):
            with torch.cuda.stream(s):
                case.poison()
                case.load(1)
            s.synchronize()
            g.replay()
            torch.cuda.synchronize(dev)
            assert_results(refs[1], step)
    finally:
        del g
        gc.collect()


@pytest.mark.parametrize("entry,name", SC.case_ids(), ids=[f"{e}-{n}" for e, n in SC.case_ids()])
def test_entry_on_side_stream_capture_and_replay(dev, entry, name):
    lib = _lib.load()
    try:
        case = SC.CASES[entry][name](dev)
        run_stream_case(case, dev, f"{entry}[{name}]")
    finally:
        lib.aaclip_set_gemm_variant(0)


# ----------------------------------------------------------------------------------------------------------------
# engine level: encode_image of the tiny CLIP as a graph on a side stream
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "fp16x2"])
def test_encode_image_graph_on_side_stream(dev, precision):
    """Built as test_tiny_clip_vs_reference_golden builds it; warm-up on the side stream, then capture
    (tools/graph_probe.py's order); the image buffer is overwritten in place with a second image and the replay must
    give, byte for byte, the eager result for that image on the default stream.  The side stream has a scratch buffer
    of its own (engine.Workspace: one per (device, stream))."""
    from model.model import CLIP
    cfg = synth.tiny_cfg()
    sd = synth.synth_clip_state_dict(cfg, seed=7)
    clip = CLIP(cfg.embed_dim,
                dict(image_size=cfg.image_size, layers=cfg.vision.layers, width=cfg.vision.width,
                     patch_size=cfg.patch_size),
                dict(context_length=77, vocab_size=cfg.vocab_size, width=cfg.text.width,
                     heads=cfg.text.heads, layers=cfg.text.layers), precision=precision)
    clip.load_state_dict(sd, strict=True)
    clip = clip.to(dev).eval()
    layers = [1, 3]
    img1 = synth.synth_images(2, cfg.image_size, seed=7).to(dev)
    img2 = synth.synth_images(2, cfg.image_size, seed=8).to(dev)
    default = torch.cuda.current_stream(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.no_grad():
        eager = []
        for img in (img1, img2):
            pooled, taps = clip.encode_image(img, layers)
            torch.cuda.synchronize(dev)
            eager.append([pooled.clone()] + [t.clone() for t in taps])
        assert not same(eager[0][0], eager[1][0])
        ws_default = engine.Workspace._bufs[(idx, default.cuda_stream)]
        buf = img1.clone()
        s = torch.cuda.Stream(dev)
        s.wait_stream(default)
        with torch.cuda.stream(s):
            clip.encode_image(buf, layers)
        s.synchronize()
        ws_side = engine.Workspace._bufs[(idx, s.cuda_stream)]
        assert ws_side is not ws_default and ws_side.data_ptr() != ws_default.data_ptr()
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=s):
                pooled, taps = clip.encode_image(buf, layers)
            assert engine.Workspace._bufs[(idx, s.cuda_stream)] is ws_side
            with torch.cuda.stream(s):
                buf.copy_(img2)
            s.synchronize()
            g.replay()
            torch.cuda.synchronize(dev)
            got = [pooled] + list(taps)
            assert len(got) == len(eager[1])
            for i, (a, b) in enumerate(zip(got, eager[1])):
                assert same(a, b), f"{precision}: output {i} of the replayed graph differs from the eager run"
        finally:
            del g
            gc.collect()
