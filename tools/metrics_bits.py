"""One sha256 per output of the evaluation-side entries (csrc/metrics.hip, regions.hip, region_table.hip, overlay.hip)
on the inputs of the test cases (tests/metrics_device_cases.py, pro_cases.py, defects_cases.py, overlay_cases.py), and
the workspace size of every metrics entry at those n: the pin for a change that must not move a bit.  Outputs only,
never workspace contents.  Run it once per library, one fresh process each (AACLIP_LIB selects the library), each GPU
step under a time limit of its own (a run takes a few seconds), and chained so that a failed step ends the job; then compare:

    AACLIP_LIB=/path/to/parent/libaaclip_hip.so timeout -k 10 240 python tools/metrics_bits.py --out parent.json &&
    timeout -k 10 240 python tools/metrics_bits.py --out new.json &&
    python tools/metrics_bits.py --compare parent.json new.json --out profiles/metrics_skeleton_bits.json

--compare exits 1 unless the two runs hold the same keys with the same hashes and the same workspace sizes."""
import argparse
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "aa-clip-iqm_amd"), os.path.join(REPO, "tests"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

WORKSPACES = ("range", "sort", "sort_pairs", "curve", "f1max", "threshold", "pro_curve")


def write(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write("\n")


def compare(a_path, b_path, out):
    a, b = (json.load(open(p)) for p in (a_path, b_path))
    differing = []
    for part in ("sha256", "workspace_bytes"):
        differing += sorted(f"{part}:{k}" for k in set(a[part]) | set(b[part]) if a[part].get(k) != b[part].get(k))
    result = {"device": a["device"], "outputs": len(a["sha256"]), "equal": not differing, "differing": differing,
              "sha256": a["sha256"], "workspace_bytes": a["workspace_bytes"]}
    print(json.dumps({k: v for k, v in result.items() if k not in ("sha256", "workspace_bytes")}, sort_keys=True))
    if out:
        write(out, result)
    return 0 if a["sha256"] and not differing else 1


def a_divisor(n):
    """a per_image that divides n: the divisor nearest below sqrt(n), n itself for a prime"""
    for d in range(int(n ** 0.5), 1, -1):
        if n % d == 0:
            return d
    return n


def hashes():
    import numpy as np
    import torch

    import defects_cases as DC
    import metrics_device_cases as MD
    import overlay_cases as OC
    import pro_cases as PC
    from aaclip_hip import _lib, engine

    dev = torch.device("cuda:0")
    lib = _lib.load()
    out, sizes = {}, {}

    def put(key, t):
        if t is not None:
            assert key not in out, key
            out[key] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()

    def up(a):
        return None if a is None else torch.from_numpy(np.array(a)).to(dev)

    # ---- range, normalise, sort, curve, F1-max, threshold
    for n in MD.sort_sizes(lib.aaclip_metrics_sort_group_items()):
        for name in WORKSPACES:
            fn = getattr(lib, f"aaclip_metrics_{name}_workspace_bytes")
            sizes[f"{name}.n{n}"] = int(fn(n, 0) if name in ("range", "threshold") else fn(n))
        for kind in ("plain", "coarse", "passthrough"):
            key = f"metrics.n{n}.{kind}"
            scores, labels = (up(v) for v in MD.inputs(n, kind))
            rng, _ = engine.metrics_range(scores, labels)
            norm = engine.metrics_normalise(scores, rng)
            packed = bool(norm.min() >= 0 and norm.max() <= 1)
            keys, labels_sorted, _ = engine.metrics_sort(norm, labels, packed)
            f1 = engine.metrics_f1max(keys, labels_sorted, packed)
            put(f"{key}.range", rng)
            put(f"{key}.normalised", norm)
            put(f"{key}.keys", keys)
            put(f"{key}.labels_sorted", labels_sorted)
            put(f"{key}.curve", engine.metrics_curve(keys, labels_sorted, packed)[:5])     # the sixth word is the sort's
            put(f"{key}.f1max", f1)
            for per_image in (0, a_divisor(n)):
                mask, counts, totals = engine.metrics_threshold(scores, f1, labels=labels, per_image=per_image,
                                                                range_record=rng)
                put(f"{key}.threshold.per{per_image}.mask", mask)
                put(f"{key}.threshold.per{per_image}.image_counts", counts)
                put(f"{key}.threshold.per{per_image}.totals", totals)

    # ---- regions, pair sort, PRO curve
    for shape in PC.SHAPES:
        tag = "x".join(str(v) for v in shape)
        region, area, regions = engine.metrics_regions(up(PC.mask("blobs", shape)))      # the mask of every curve case
        put(f"pro.{tag}.region", region)
        put(f"pro.{tag}.area", area)
        put(f"pro.{tag}.regions_record", regions)
        for levels in PC.LEVELS:
            key = f"pro.{tag}.levels{levels}"
            scores = up(PC.curve_case(shape, levels)[1])
            rng, _ = engine.metrics_range(scores)
            keys, areas_sorted = engine.metrics_sort_pairs(engine.metrics_normalise(scores, rng), area)
            put(f"{key}.keys", keys)
            put(f"{key}.areas_sorted", areas_sorted)
            for limit in (0.05, 0.3, 1.0):
                put(f"{key}.pro_record.limit{limit}", engine.metrics_pro_curve(keys, areas_sorted, regions, limit))

    # ---- region table, with and without a range record (with one where the scores have a range to normalise by)
    labelled = {}
    for case in [c for shape in DC.SHAPES for c in DC.cases(shape)] + [DC.BIG_CASE]:
        where = (case.shape, case.pattern, case.connectivity)
        if where not in labelled:
            labelled[where] = engine.metrics_regions(up(PC.mask(case.pattern, case.shape)), case.connectivity)
        region, area, regions = labelled[where]
        _, raw, _, second = DC.inputs(case)
        for with_range in (False, True) if isinstance(case.scores, int) else (False,):
            key = "table." + ".".join(str(v) for v in case).replace(" ", "") + f".range{int(with_range)}"
            if f"{key}.rows" in out:          # a shape whose minimum areas repeat lists a case twice
                continue
            table = engine.region_table(region, area, up(raw), other=up(second),
                                        range_record=up(DC.range_record(raw)) if with_range else None,
                                        min_area=case.min_area, kept_mask=True, regions=regions)
            put(f"{key}.rows", table.rows)
            put(f"{key}.image_offsets", table.image_offsets)
            put(f"{key}.kept_mask", table.kept_mask)
            put(f"{key}.record", table.record)

    # ---- one overlay with a range record
    case = {"B": 3, "H": 70, "W": 70, "T": 2, "pred": True, "truth": True, "alpha256": 77, "panels": OC.PANELS,
            "lut": "jet", "special": None}
    frames, maps, kw = OC.arguments(case)
    put("overlay.70x70", engine.overlay_render(up(frames), up(maps), up(kw["range_record"]), up(kw["pred"]),
                                               up(kw["truth"]), alpha=77 / 256, lut=up(kw["lut"]), thickness=2))
    torch.cuda.synchronize()
    return {"device": torch.cuda.get_device_name(0), "sha256": out, "workspace_bytes": sizes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, a.out))
    result = hashes()
    print(len(result["sha256"]), "outputs hashed,", len(result["workspace_bytes"]), "workspace sizes")
    if a.out:
        write(a.out, result)


if __name__ == "__main__":
    main()
