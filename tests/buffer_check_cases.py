"""One table per C ABI entry that checks its buffers through csrc/buffers.h (tests/test_buffer_checks_cpu.py): a valid
argument list on stand-in addresses and, for each pointer argument, its byte length, alignment and whether the call
writes it.  The rule under test (include/aaclip.h, "Buffers of a call"): a written buffer overlaps no other buffer.

Nothing here touches memory: every call is refused before a launch, so plausible device addresses stand in.  The
workspace sizes come from the library's own *_workspace_bytes."""
import ctypes as C

from aaclip_hip import _lib

BASE, SLOT = 0x7f0000000000, 1 << 30       # buffer k of a call lies at BASE + k * SLOT: a GiB apart, far from both ends


class Buf:
    def __init__(self, name, nbytes, align, written):
        self.name, self.bytes, self.align, self.written = name, nbytes, align, written


class Entry:
    """name: the id; fn: the symbol; prefix: what its messages start with; bufs: the table; call(lib, addr, ws_bytes) ->
    rc with addr = {buffer name: address}; ws: the workspace's name or None; ws_last: the entry checks the workspace size
    AFTER the overlaps (then every case passes it one byte short, so that a pair nobody checks is still a refusal)"""
    def __init__(self, name, fn, prefix, bufs, call, ws=None, ws_last=False):
        self.name, self.fn, self.prefix, self.bufs, self.call, self.ws, self.ws_last = name, fn, prefix, bufs, call, ws, ws_last
        assert len({b.name for b in bufs}) == len(bufs) and all(b.bytes < SLOT // 4 for b in bufs)
        assert (ws is None and not ws_last) or self.buf(ws).written

    def buf(self, name):
        return next(b for b in self.bufs if b.name == name)

    def addresses(self):
        return {b.name: BASE + k * SLOT for k, b in enumerate(self.bufs)}

    def ws_need(self):
        return self.buf(self.ws).bytes if self.ws else 0

    def pairs(self):
        """(written, other) names: every buffer the call writes against every other buffer, each unordered pair once"""
        out = []
        for i, w in enumerate(self.bufs):
            for j, o in enumerate(self.bufs):
                if i != j and w.written and not (o.written and j < i):
                    out.append((w.name, o.name))
        return out


def R(name, nbytes, align=1):
    return Buf(name, nbytes, align, False)


def W(name, nbytes, align=1):
    return Buf(name, nbytes, align, True)


def placements(entry, written, other):
    """-> {kind: address of `other`}; every shift is a whole multiple of other's alignment (the addresses of the table are
    multiples of 2^30), so the alignment check never answers.  'last' / 'first': other starts on written's last aligned
    unit / ends on its first -- one unit shared; 'after' / 'before': just adjacent, no byte shared."""
    w, o = entry.buf(written), entry.buf(other)
    at, a = entry.addresses()[written], o.align
    up = lambda v: (v + a - 1) // a * a
    return {"last": at + (w.bytes - 1) // a * a, "first": at - (o.bytes - 1) // a * a,
            "after": at + up(w.bytes), "before": at - up(o.bytes)}


def entries(lib):
    n, per, n4 = 12, 4, 48                 # twelve scores in three images
    N, E, M = 5, 64, 3                     # support / coreset rows
    out = []

    def add(name, bufs, call, ws=None, ws_last=False, fn=None, prefix=None):
        out.append(Entry(name, fn or "aaclip_" + name, (prefix or name) + ":", bufs, call, ws, ws_last))

    need = lib.aaclip_color_jitter_workspace_bytes(2, 5, 7)
    add("color_jitter", [W("dst", 210), R("src", 210), R("factors", 24, 4), R("apply", 8, 4), W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_color_jitter(a["src"], a["dst"], 2, 5, 7, a["factors"], a["apply"], a["ws"], ws, None),
        "ws")                              # the workspace size is checked before the table, after dst x src
    add("augment_geometric", [R("image", 600, 4), R("mask", 200, 4), R("angle_deg", 8, 4), R("shift", 16, 4), R("flags", 8, 4),
                              W("image_out", 600, 4), W("mask_out", 200, 4)],
        lambda lib, a, ws: lib.aaclip_augment_geometric(a["image"], a["mask"], 2, 5, a["angle_deg"], a["shift"], a["flags"],
                                                        a["image_out"], a["mask_out"], None))
    need = lib.aaclip_metrics_range_workspace_bytes(n, per)
    add("metrics_range", [R("scores", n4, 4), R("labels", n), W("image_max", n // per * 4, 4), W("record", 24, 8), W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_metrics_range(a["scores"], a["labels"], n, per, a["image_max"], a["record"], a["ws"], ws, None),
        "ws", True)
    add("metrics_normalise", [R("scores", n4, 4), W("out", n4, 4), R("range_record", 24, 8)],
        lambda lib, a, ws: lib.aaclip_metrics_normalise(a["scores"], a["out"], n, a["range_record"], None))
    need = lib.aaclip_metrics_sort_workspace_bytes(n)
    add("metrics_sort", [R("scores", n4, 4), R("labels", n), W("keys", n4, 4), W("labels_sorted", n), W("out_of_range", 8, 8),
                         W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_metrics_sort(a["scores"], a["labels"], n, 0, a["keys"], a["labels_sorted"],
                                                   a["out_of_range"], a["ws"], ws, None), "ws", True)
    for name, rec in (("metrics_curve", 40), ("metrics_f1max", 56)):
        need = getattr(lib, f"aaclip_{name}_workspace_bytes")(n)
        add(name, [R("keys", n4, 4), R("labels_sorted", n), W("record", rec, 8), W("ws", need, 8)],
            lambda lib, a, ws, name=name: getattr(lib, "aaclip_" + name)(a["keys"], a["labels_sorted"], n, 0, a["record"],
                                                                         a["ws"], ws, None), "ws", True)
    need = lib.aaclip_metrics_threshold_workspace_bytes(n, per)
    add("metrics_threshold", [R("scores", n4, 4), R("labels", n), R("range_record", 24, 8), R("f1max_record", 56, 8), W("mask", n),
                              W("image_counts", n // per * 16, 4), W("totals", 32, 8), W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_metrics_threshold(a["scores"], a["labels"], n, per, a["range_record"], a["f1max_record"],
                                                        a["mask"], a["image_counts"], a["totals"], a["ws"], ws, None), "ws", True)

    def bootstrap(lib, a, ws):
        plan = _lib.BootstrapPlan()
        plan.n, plan.images, plan.replicates = n, 3, 4
        return lib.aaclip_bootstrap_curves(C.byref(plan), a["keys"], a["payload"], a["counts"], a["records"], a["ws"], ws)
    need = lib.aaclip_bootstrap_workspace_bytes(n, 3, 4)
    add("bootstrap_curves", [R("keys", n4, 4), R("payload", n4, 4), R("counts", 12), W("records", 128, 8), W("ws", need, 8)],
        bootstrap, "ws", True)

    def tensors(a):
        items = (_lib.OptimTensor * 2)()
        items[0].g, items[0].n, items[1].g, items[1].n = a["grad0"], 5, a["grad1"], 3
        t = _lib.OptimTensors()
        t.items, t.count = items, 2
        return t, items
    need = lib.aaclip_optim_grad_norm_workspace_bytes(C.byref(tensors({"grad0": BASE, "grad1": BASE + SLOT})[0]))
    add("optim_grad_norm", [R("grad0", 20, 4), R("grad1", 12, 4), W("record", 8, 8), W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_optim_grad_norm(C.byref(tensors(a)[0]), 1.0, a["record"], a["ws"], ws, None), "ws")
    need = lib.aaclip_metrics_regions_workspace_bytes(2, 3, 2)
    add("metrics_regions", [R("mask", n), W("region", n4, 4), W("area", n4, 4), W("record", 24, 8), W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_metrics_regions(a["mask"], 2, 3, 2, 8, a["region"], a["area"], a["record"], a["ws"], ws,
                                                      None), "ws", True)
    need = lib.aaclip_metrics_sort_pairs_workspace_bytes(n)
    add("metrics_sort_pairs", [R("scores", n4, 4), R("values", n4, 4), W("keys", n4, 4), W("values_sorted", n4, 4), W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_metrics_sort_pairs(a["scores"], a["values"], n, a["keys"], a["values_sorted"], a["ws"],
                                                         ws, None), "ws", True)
    need = lib.aaclip_metrics_pro_curve_workspace_bytes(n)
    add("metrics_pro_curve", [R("keys", n4, 4), R("areas_sorted", n4, 4), R("regions_record", 24, 8), W("record", 40, 8),
                              W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_metrics_pro_curve(a["keys"], a["areas_sorted"], n, a["regions_record"], 0.3, a["record"],
                                                        a["ws"], ws, None), "ws", True)
    need = lib.aaclip_region_table_workspace_bytes(2, 3, 2)
    add("region_table", [R("region", n4, 4), R("area", n4, 4), R("scores", n4, 4), R("range_record", 24, 8), R("other", n),
                         W("rows", 4 * 48, 8), W("image_offsets", 12, 4), W("kept_mask", n), W("record", 32, 8), W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_region_table(a["region"], a["area"], a["scores"], a["range_record"], a["other"], 2, 3, 2, 1,
                                                   4, a["rows"], a["image_offsets"], a["kept_mask"], a["record"], a["ws"], ws,
                                                   None), "ws", True)
    need = lib.aaclip_support_nearest_workspace_bytes(M, N, E, 0)
    add("support_nearest", [R("q", M * E * 4, 16), R("bank", N * E * 2, 16), W("best_cos", M * 4, 4), W("best_idx", M * 4, 4),
                            W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_support_nearest(a["q"], M, a["bank"], N, E, 0, a["best_cos"], a["best_idx"], a["ws"], ws,
                                                      None), "ws")
    add("support_bank_rows", [R("rows", N * E * 4, 16), W("bank", N * E * 2, 16)],
        lambda lib, a, ws: lib.aaclip_support_bank_rows(a["rows"], N, E, 0, a["bank"], None))

    def support_map(lib, a, ws):           # B = 1, grid 2, S = 4: levels of 4 floats, maps of 16
        levels = (C.c_void_p * 2)(a["level0"], a["level1"])
        return lib.aaclip_support_map(levels, 2, a["base"], 0.5, a["out"], 1, 2, 4, 1, 1.0, a["ws"], ws, None)
    add("support_map", [R("level0", 16, 4), R("level1", 16, 4), R("base", 64, 4), W("out", 64, 4), W("ws", 32, 4)], support_map, "ws")
    add("coreset_rows", [R("rows", N * E * 4, 16), W("q", N * E * 2, 16), W("norm2", N * 4, 4)],
        lambda lib, a, ws: lib.aaclip_coreset_rows(a["rows"], N, E, a["q"], a["norm2"], None))
    add("coreset_unit_rows", [R("rows", N * E * 4, 16), W("out", N * E * 4, 16)],
        lambda lib, a, ws: lib.aaclip_coreset_unit_rows(a["rows"], N, E, a["out"], None))
    need = lib.aaclip_coreset_select_workspace_bytes(N, E, 2)
    add("coreset_select", [R("q", N * E * 2, 16), R("norm2", N * 4, 4), W("picks", 8, 4), W("radius2", 12, 4), W("min_d2", N * 4, 4),
                           W("ws", need, 8)],
        lambda lib, a, ws: lib.aaclip_coreset_select(a["q"], a["norm2"], N, E, 2, 0, a["picks"], a["radius2"], a["min_d2"],
                                                     a["ws"], ws, None), "ws")

    def tile_plan():                       # tile 4, grid 2, overlap 1: a canvas of 7 x 7, four tiles of 4 x 4
        p = _lib.TilePlan()
        p.images, p.channels, p.tile, p.grid, p.overlap = 1, 1, 4, 2, 1
        return p
    add("tile_gather", [R("canvas", 196, 4), W("tiles", 256, 4)], prefix="aaclip_tile_gather",
        call=lambda lib, a, ws: lib.aaclip_tile_gather(C.byref(tile_plan()), a["canvas"], a["tiles"]))
    add("tile_stitch", [R("tiles", 256, 4), W("canvas", 196, 4)], prefix="aaclip_tile_stitch",
        call=lambda lib, a, ws: lib.aaclip_tile_stitch(C.byref(tile_plan()), a["tiles"], a["canvas"]))

    def overlay(lib, a, ws):               # one frame of 3 x 4 pixels, three panels
        p = _lib.OverlayPlan()
        p.images, p.height, p.width, p.panels, p.alpha256, p.thickness = 1, 3, 4, 7, 128, 1
        for c in range(3):
            p.mean[c], p.std[c] = 0.5, 0.25
        return lib.aaclip_overlay_render(C.byref(p), a["frames"], a["maps"], a["range_record"], a["pred"], a["truth"], a["lut"],
                                         a["out"])
    add("overlay_render", [R("frames", 144, 4), R("maps", 48, 4), R("range_record", 24, 8), R("pred", 12), R("truth", 12),
                           R("lut", 768), W("out", 108)], overlay, prefix="aaclip_overlay_render")

    def png_plan():
        p = _lib.PngPlan()
        p.images, p.height, p.width, p.channels = 1, 3, 4, 3
        return p
    need, cap = lib.aaclip_png_workspace_bytes(C.byref(png_plan())), lib.aaclip_png_capacity_bytes(C.byref(png_plan()))
    add("png_encode", [R("pixels", 36), W("ws", need, 16), W("payload", cap), W("offsets", 16, 8)], prefix="aaclip_png_encode",
        call=lambda lib, a, ws: lib.aaclip_png_encode(C.byref(png_plan()), a["pixels"], a["ws"], ws, a["payload"], cap, a["offsets"]),
        ws="ws")
    assert all(e.ws_need() > 0 for e in out if e.ws), [e.name for e in out if e.ws and e.ws_need() == 0]
    return out


# The pairs that no check named before every entry declared its table (include/aaclip.h names each of them): entry ->
# (written, other).  The first six were found by calling the library; the rest by reading its checks.
NEW_PAIRS = {
    "metrics_sort": [("keys", "labels"), ("labels_sorted", "scores"), ("out_of_range", "scores"), ("out_of_range", "labels")],
    "metrics_range": [("image_max", "labels"), ("record", "labels")],
    "metrics_normalise": [("out", "range_record")],
    "png_encode": [("ws", "pixels"), ("ws", "payload"), ("ws", "offsets"), ("payload", "offsets")],
    "augment_geometric": [(o, i) for o in ("image_out", "mask_out") for i in ("angle_deg", "shift", "flags")],
    "color_jitter": [("ws", "dst"), ("ws", "src"), ("ws", "factors"), ("ws", "apply"), ("dst", "factors"), ("dst", "apply")],
    "support_map": [("ws", "level0"), ("ws", "level1"), ("ws", "base"), ("ws", "out"), ("out", "level0"), ("out", "level1")],
    "optim_grad_norm": [(w, g) for w in ("record", "ws") for g in ("grad0", "grad1")],
}
