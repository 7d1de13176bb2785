"""Split fp16 blocks with the LayerNorm passes run beside the residual products' partial last round (csrc/tail_plan.h,
aaclip_set_tail_overlap): every output buffer is bit-identical with the overlap on and off -- through aaclip_blocks_taps
and aaclip_blocks_to, in a captured graph and on a side stream.  The split is planned with 8 CUs (aaclip_set_plan_cus)
so that a tail exists at a few thousand rows: 4097 and 4225 rows are 17 row tiles (the last one partial, and neither row
count is a multiple of the LayerNorm kernel's 4 rows per workgroup); at D = 256 that is two rounds and ONE tail tile, at
D = 1024 eight rounds and a tail of 4 tiles = grid / 2; 4096 rows are an exact number of rounds, where the split must not
engage.  aaclip_tail_overlap_count tells an engaged split from a single launch."""
import ctypes
import functools

import pytest
import torch

from aaclip_hip import _lib, engine
from model.transformer import ResidualAttentionBlock

pytestmark = pytest.mark.gpu

F16X2 = _lib.F16X2
FULL, CAUSAL = 0, 1
N_BLOCKS = 3
# (D, B, L, attention, weights exact in fp16, tail launches expected of one call with the overlap on)
#   a call of three blocks splits three out_proj (-> ln_2) and two c_proj (-> the next block's ln_1) products
CASES = {
    "one_tail_tile": (256, 17, 241, FULL, False, 5),
    "one_tail_tile_causal_exact": (256, 65, 65, CAUSAL, True, 5),
    "tail_of_half_the_grid_exact": (1024, 17, 241, FULL, True, 5),
    "tail_of_half_the_grid": (1024, 65, 65, FULL, False, 5),
    "exact_rounds_do_not_engage": (256, 64, 64, FULL, False, 0),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _plan_with_8_cus():
    lib = _lib.load()
    assert lib.aaclip_set_plan_cus(8) == 0
    yield
    assert lib.aaclip_set_plan_cus(0) == 0 and lib.aaclip_set_tail_overlap(1) == 0


@functools.lru_cache(maxsize=None)
def setup(name):
    """blocks, packed weights, the input rows and the workspace of a case: built once, the inputs never written"""
    D, B, L, attn, exact, launches = CASES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1234 + D + B)
    blocks, keep = [], []
    arr = (_lib.BlockWeights * N_BLOCKS)()
    for i in range(N_BLOCKS):
        blk = ResidualAttentionBlock(D, D // 64)
        with torch.no_grad():
            for p in blk.parameters():
                if p.dim() == 1:     # LayerNorm weights / biases and product biases: not the constructor's ones and zeros
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if p is blk.ln_1.weight or p is blk.ln_2.weight else 0.0))
                elif exact:
                    p.copy_(p.half().float())
        blk.to(dev)
        w, refs = engine.pack_block(blk, F16X2, None)
        assert w.exact16 == (15 if exact else 0)
        arr[i] = w
        blocks.append(blk)
        keep.append(refs)
    rows = B * L
    x_in = torch.randn(rows, D, generator=g).to(dev)
    lib = _lib.load()
    need = lib.aaclip_workspace_bytes(F16X2, rows, D, 4 * D, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    return dict(D=D, B=B, L=L, attn=attn, arr=arr, keep=(blocks, keep), x_in=x_in, ws=ws, rows=rows, launches=launches)


def run(c, entry, on, stream=None):
    """one call of three blocks -> (every output buffer, cloned; tail launches it issued)"""
    lib = _lib.load()
    D, B, L = c["D"], c["B"], c["L"]
    assert lib.aaclip_set_tail_overlap(1 if on else 0) == 0
    st = stream if stream is not None else torch.cuda.current_stream()
    c["ws"].fill_(0x5A)          # nothing may depend on what an earlier call left in the workspace
    tail = (B, L, D, D // 64, 4 * D, c["attn"], F16X2, c["ws"].data_ptr(), c["ws"].numel(), st.cuda_stream)
    before = lib.aaclip_tail_overlap_count()
    if entry == "taps":          # a tap after the second block: blocks 0 and 1 write `tap`, block 2 continues in `last`
        tap, last = torch.full_like(c["x_in"], float("nan")), torch.full_like(c["x_in"], float("nan"))
        outs = (ctypes.c_void_p * N_BLOCKS)(tap.data_ptr(), tap.data_ptr(), last.data_ptr())
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            rc = lib.aaclip_blocks_taps(c["x_in"].data_ptr(), outs, c["arr"], N_BLOCKS, 0.1, *tail)
        bufs = [tap, last]
    else:
        x = torch.full_like(c["x_in"], float("nan"))
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            rc = lib.aaclip_blocks_to(c["x_in"].data_ptr(), x.data_ptr(), c["arr"], N_BLOCKS, 0.1, *tail)
        bufs = [x]
    assert rc == 0, lib.aaclip_last_error().decode()
    issued = lib.aaclip_tail_overlap_count() - before
    st.synchronize()
    return bufs, issued


@functools.lru_cache(maxsize=None)
def reference(name, entry):
    """the overlap OFF: computed once per case and entry"""
    bufs, issued = run(setup(name), entry, on=False)
    assert issued == 0
    assert all(torch.isfinite(b).all() for b in bufs)
    return bufs


def same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"{what}: output buffer {i} differs in {(a != b).sum().item()} elements"


@pytest.mark.parametrize("entry", ["taps", "to"])
@pytest.mark.parametrize("name", list(CASES))
def test_overlap_on_is_bit_identical_to_off(dev, name, entry):
    c = setup(name)
    want = reference(name, entry)
    got, issued = run(c, entry, on=True)
    assert issued == c["launches"], (name, issued)
    same(got, want, f"{name} / {entry}")
    if entry == "taps":
        assert not torch.equal(got[0], got[1])          # the tap and the last block's rows are different streams


def test_the_input_rows_are_left_alone(dev):
    c = setup("one_tail_tile")
    before = c["x_in"].clone()
    run(c, "to", on=True)
    assert torch.equal(c["x_in"], before)


@pytest.mark.parametrize("name", ["one_tail_tile", "tail_of_half_the_grid_exact"])
def test_captured_in_a_graph_and_replayed(dev, name):
    lib = _lib.load()
    c = setup(name)
    want = reference(name, "to")
    D, B, L = c["D"], c["B"], c["L"]
    x = torch.full_like(c["x_in"], float("nan"))
    assert lib.aaclip_set_tail_overlap(1) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rc = lib.aaclip_blocks_to(c["x_in"].data_ptr(), x.data_ptr(), c["arr"], N_BLOCKS, 0.1, B, L, D, D // 64, 4 * D,
                                      c["attn"], F16X2, c["ws"].data_ptr(), c["ws"].numel(), side.cuda_stream)
        assert rc == 0, lib.aaclip_last_error().decode()
    torch.cuda.synchronize()
    for _ in range(2):
        x.fill_(float("nan"))
        c["ws"].fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        same([x], want, f"{name} / graph replay")


@pytest.mark.parametrize("name", ["one_tail_tile_causal_exact", "tail_of_half_the_grid"])
def test_on_a_side_stream(dev, name):
    c = setup(name)
    want = reference(name, "taps")
    got, issued = run(c, "taps", on=True, stream=torch.cuda.Stream())
    assert issued == c["launches"]
    same(got, want, f"{name} / side stream")


def test_switches(dev):
    lib = _lib.load()
    for bad in (-8, 4, 12, 2048):
        assert lib.aaclip_set_plan_cus(bad) == -1 and b"set_plan_cus" in lib.aaclip_last_error()
    c = setup("one_tail_tile")
    assert lib.aaclip_set_plan_cus(0) == 0          # the device's CU count: 17 tiles are no two rounds of it
    _, issued = run(c, "to", on=True)
    assert issued == 0
