"""tools/metrics_bits.py --compare on two small runs: equal runs pass, a moved hash, a missing key and a moved workspace
size are each named and fail.  No GPU: the comparison reads two JSON files."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import metrics_bits as MB  # noqa: E402

RUN = {"device": "x", "sha256": {"a.keys": "00", "a.record": "11"}, "workspace_bytes": {"curve.n2": 768}}


def compared(tmp_path, other):
    paths = []
    for name, run in (("a", RUN), ("b", other)):
        paths.append(str(tmp_path / f"{name}.json"))
        MB.write(paths[-1], run)
    out = str(tmp_path / "sub" / "out.json")
    rc = MB.compare(paths[0], paths[1], out)
    return rc, json.load(open(out))


def test_equal_runs_compare_equal(tmp_path):
    rc, result = compared(tmp_path, RUN)
    assert rc == 0 and result["equal"] is True and result["differing"] == [] and result["outputs"] == 2
    assert result["sha256"] == RUN["sha256"] and result["workspace_bytes"] == RUN["workspace_bytes"]


def test_every_kind_of_difference_is_named_and_fails(tmp_path):
    moved = {**RUN, "sha256": {"a.keys": "00", "a.record": "12"}}
    missing = {**RUN, "sha256": {"a.keys": "00"}}
    extra = {**RUN, "sha256": {**RUN["sha256"], "b.keys": "22"}}
    size = {**RUN, "workspace_bytes": {"curve.n2": 1024}}
    for other, want in ((moved, ["sha256:a.record"]), (missing, ["sha256:a.record"]), (extra, ["sha256:b.keys"]),
                        (size, ["workspace_bytes:curve.n2"])):
        rc, result = compared(tmp_path, other)
        assert rc == 1 and result["equal"] is False and result["differing"] == want


def test_two_empty_runs_do_not_pass(tmp_path):
    empty = {"device": "x", "sha256": {}, "workspace_bytes": {}}
    paths = [str(tmp_path / n) for n in ("a.json", "b.json")]
    for p in paths:
        MB.write(p, empty)
    assert MB.compare(paths[0], paths[1], None) == 1
