"""The parts that the ten evaluation scripts share, without a GPU and without weights:

  eval_last.open_session           the set-up sequence of every run(), against stand-ins for the model, the datasets and
                                   the checkpoint loader: sizes, the text embeddings' source, the lines of test.log
  the with-flag run() paths        eval_tiled --tiles, eval_overlay --overlay, eval_png --masks_png and eval_bootstrap
                                   --bootstrap, with the session and the module's evaluate entry replaced: the canvas size
                                   and the keywords, written out from the run() bodies these paths had when each of them
                                   carried its own copy of the set-up
  eval_defects.evaluate_details    the one evaluate body: what eval_support, eval_coreset, eval_overlay, eval_png and
                                   eval_bootstrap .evaluate hand to eval_last.evaluate_rows, support_banks and
                                   write_defects, and the shape of what they return, against a table
"""
import contextlib
import inspect
import logging
import os

import pytest
import torch

import eval_bootstrap as EB
import eval_coreset as EC
import eval_defects as ED
import eval_last as EL
import eval_overlay as EO
import eval_png as EP
import eval_support as ES
import eval_tiled as ET

ROWS = [{"class name": "bottle", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0},
        {"class name": "Average", "pixel AUC": 91.0, "pixel AP": 50.0, "image AUC": 80.0, "image AP": 70.0}]


# ------------------------------------------------------------------------------------------------- the session
@contextlib.contextmanager
def root_logging():
    """logging.basicConfig configures a root logger without handlers only, and pytest hangs its own on it for the length
    of a test's body: they step aside here, and the file that basicConfig opens is closed on the way out"""
    root = logging.getLogger()
    kept, level = root.handlers[:], root.level
    root.handlers[:] = []
    try:
        yield root
    finally:
        for handler in root.handlers:
            handler.close()
        root.handlers[:] = kept
        root.setLevel(level)


@pytest.fixture
def stand_ins(monkeypatch):
    """-> the calls that open_session makes, by name; load_adapters answers calls["adapt_text"]"""
    import dataset
    import forward_utils
    import model.adapter
    import model.clip
    import test_last as TL
    calls = {"adapt_text": False, "order": []}

    class Clip:
        evaluated = False

        def eval(self):
            self.evaluated = True

    class Adapted(Clip):
        def __init__(self, **kwargs):
            calls["AdaptedCLIP"] = kwargs
            calls["order"].append("AdaptedCLIP")

        def to(self, device):
            calls["to"] = device
            return self

    def create_model(**kwargs):
        calls["create_model"] = kwargs
        calls["order"].append("create_model")
        return Clip()

    def load_adapters(model, save_path, logger=None):
        calls["load_adapters"] = (model, save_path, logger)
        calls["order"].append("load_adapters")
        logger.info("load model from epoch %s", 7)
        return calls["adapt_text"]

    def get_dataset(*args, **kwargs):
        calls["get_dataset"] = (args, kwargs)
        calls["order"].append("get_dataset")
        return {"bottle": "test set of bottle", "grid": "test set of grid"}

    def text_embedding(model, dataset_name, device):
        calls["text"] = (model, dataset_name, device)
        calls["order"].append("text")
        return {"bottle": "anchors of bottle", "grid": "anchors of grid"}

    def single_class(*args, **kwargs):
        calls.setdefault("BaseSingleClassDataset", []).append((args, kwargs))
        return ("support set", args[3])

    monkeypatch.setattr(model.clip, "create_model", create_model)
    monkeypatch.setattr(model.adapter, "AdaptedCLIP", Adapted)
    monkeypatch.setattr(dataset, "get_dataset", get_dataset)
    monkeypatch.setattr(dataset, "BaseSingleClassDataset", single_class)
    monkeypatch.setattr(forward_utils, "get_adapted_text_embedding", text_embedding)
    monkeypatch.setattr(EL, "load_adapters", load_adapters)
    monkeypatch.setattr(TL, "setup_seed", lambda seed: calls.update(seed=seed))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda device: calls.update(set_device=device))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("LOCAL_RANK", raising=False)
    return calls


@pytest.mark.parametrize("adapt_text", [False, True])
def test_open_session(tmp_path, stand_ins, adapt_text):
    import dataset
    calls = stand_ins
    calls["adapt_text"] = adapt_text
    save = tmp_path / "ckpt"
    args = ET.build_parser().parse_args(["--save_path", str(save), "--img_size", "70", "--seed", "5", "--precision", "fp32",
                                         "--support", "2", "--support_meta", "train_good.jsonl", "--device_preprocess",
                                         "--relu", "--shot", "3"])
    with root_logging():
        session = EL.open_session(args, "eval_tiled", 126, ["tiled inference: first extra line", "second extra line"])
    assert session._fields == ("logger", "device", "clip_model", "model", "adapt_text", "image_datasets", "text_embeddings",
                               "support_datasets")
    assert calls["seed"] == 5 and session.device == torch.device("cuda", 0) == calls["set_device"] == calls["to"]
    assert session.logger is logging.getLogger("eval_tiled") and session.adapt_text is adapt_text
    # the model at --img_size; the datasets and the support datasets at the canvas size
    assert calls["create_model"] == dict(model_name="ViT-L-14-336", img_size=70, device=session.device, pretrained="openai",
                                         require_pretrained=True, precision="fp32")
    assert calls["AdaptedCLIP"] == dict(clip_model=session.clip_model, text_adapt_weight=0.1, image_adapt_weight=0.1,
                                        text_adapt_until=3, image_adapt_until=6, relu=True, iqm_hidden_size=768,
                                        iqm_num_layers=2, iqm_num_heads=8)
    assert session.clip_model.evaluated and session.model.evaluated and session.model is not session.clip_model
    assert calls["load_adapters"] == (session.model, str(save), session.logger)
    assert calls["get_dataset"] == (("MVTec", 126, None, 3, "test"), dict(logger=session.logger, device_preprocess=True))
    assert session.image_datasets == {"bottle": "test set of bottle", "grid": "test set of grid"}
    assert calls["BaseSingleClassDataset"] == [((dataset.DATA_PATH["MVTec"], "train_good.jsonl", 126, c),
                                                dict(device_preprocess=True)) for c in ("bottle", "grid")]
    assert session.support_datasets == {"bottle": ("support set", "bottle"), "grid": ("support set", "grid")}
    # the text embeddings come from the adapted model exactly when a text adapter was loaded
    assert calls["text"] == (session.model if adapt_text else session.clip_model, "MVTec", session.device)
    assert session.text_embeddings == {"bottle": "anchors of bottle", "grid": "anchors of grid"}
    assert calls["order"] == ["create_model", "AdaptedCLIP", "load_adapters", "get_dataset", "text"]
    # test.log: the caller's logger name in every line, the extra lines directly after `args:`, before the model's lines
    lines = (save / "test.log").read_text(encoding="utf-8").splitlines()
    assert lines[0].startswith("INFO:eval_tiled:args: {") and "'img_size': 70" in lines[0]
    assert lines[1:] == ["INFO:eval_tiled:tiled inference: first extra line", "INFO:eval_tiled:second extra line",
                         "INFO:eval_tiled:load model from epoch 7"]


def test_open_session_defaults_and_arguments_of_the_lower_parsers(tmp_path, stand_ins, monkeypatch):
    calls = stand_ins
    # eval_last's own parser has no support arguments: the canvas is --img_size, no support datasets, no extra lines
    args = EL.build_parser().parse_args(["--save_path", str(tmp_path / "a"), "--img_size", "84"])
    with root_logging():
        session = EL.open_session(args, "eval_last")
    assert calls["create_model"]["img_size"] == 84 and calls["get_dataset"][0][1] == 84
    assert session.support_datasets is None and "BaseSingleClassDataset" not in calls
    lines = (tmp_path / "a" / "test.log").read_text(encoding="utf-8").splitlines()
    assert len(lines) == 2 and lines[0].startswith("INFO:eval_last:args: ") and lines[1].startswith("INFO:eval_last:load model")
    # --support without --support_meta, and --support_meta's datasets only with --support
    args = ES.build_parser().parse_args(["--save_path", str(tmp_path / "a"), "--support", "2"])
    assert EL.open_session(args, "eval_support").support_datasets is None and "BaseSingleClassDataset" not in calls
    args.support, args.support_meta = None, "m.jsonl"
    assert EL.open_session(args, "eval_support").support_datasets is None and "BaseSingleClassDataset" not in calls
    # no GPU, no session: nothing is built
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    del calls["create_model"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EL.open_session(args, "eval_support")
    assert "create_model" not in calls


# ------------------------------------------------------------------------------------- the with-flag run() paths
LOADER = {"num_workers": 4, "pin_memory": True}
COMMON_ARGV = ["--img_size", "70", "--image_batch_size", "8", "--device_metrics", "--iqm", "off", "--aupro", "0.2",
               "--support", "2", "--support_weight", "20", "--support_form", "fp32", "--support_meta", "m.jsonl",
               "--support_coreset", "0.5", "--support_coreset_dim", "256", "--defects", "3"]


@pytest.fixture
def fake_session(monkeypatch):
    opened = []
    session = EL.Session(logging.getLogger("fake session"), "device", "clip model", "model", True, "image datasets",
                         "text embeddings", "support datasets")

    def open_session(args, name, canvas=None, log_lines=()):
        opened.append((name, canvas, list(log_lines)))
        return session

    monkeypatch.setattr(EL, "open_session", open_session)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return session, opened


def common_keywords(session, save_path):
    """what every run() body above eval_coreset.py passed for COMMON_ARGV, keyword by keyword"""
    return dict(batch_size=8, loader_kwargs=LOADER, logger=session.logger, use_iqm=False, device_metrics=True,
                aupro_limit=0.2, defects=3, save_path=save_path, support=2, support_weight=20.0, support_form="fp32",
                support_datasets="support datasets", coreset=0.5, coreset_dim=256)


def details_of(*classes):
    return {c: {"pixel threshold": 0.5, "image threshold": None} for c in classes}


@pytest.mark.parametrize("tiles", [None, 2])
def test_run_paths_with_their_flags(monkeypatch, capsys, fake_session, tiles):
    session, opened = fake_session
    where = ("model", "image datasets", "text embeddings", "device", 70, "MVTec")
    tile_argv = [] if tiles is None else ["--tiles", str(tiles), "--tile_overlap", "14"]
    canvas = 70 if tiles is None else ET.tile_geometry(70, tiles, 14)[3]
    assert canvas == (70 if tiles is None else 126)
    argv = COMMON_ARGV + tile_argv + ["--save_path", "out"]
    tile_keywords = dict(tiles=tiles, tile_overlap=14 if tiles else 112)
    seen = []

    def entry(result):
        def fake(*a, **k):
            seen.append((a, {key: (type(v)(v) if key.endswith("_written") else v) for key, v in k.items()}))
            return result
        return fake

    # eval_tiled --tiles
    if tiles is not None:
        monkeypatch.setattr(ET, "evaluate_details", entry((ROWS, details_of("bottle"))))
        assert ET.main(list(argv)) == ROWS
        assert opened.pop() == ("eval_tiled", 126, ["tiled inference: S 70, G 2, O 14, C 126 (4 tiles per frame)"])
        (a, k), = seen
        assert a == where + ((2, 14),) and k == dict(common_keywords(session, "out"), f1_max=True)
        assert capsys.readouterr().out == ED.format_table(ROWS) + "\n"
        del seen[:]
    # eval_overlay --overlay
    overlay_keywords = dict(overlay=0.25, overlay_limit=3, overlay_thickness=2, overlay_colormap="gray")
    overlay_argv = ["--overlay", "0.25", "--overlay_limit", "3", "--overlay_thickness", "2", "--overlay_colormap", "gray"]
    monkeypatch.setattr(EO, "evaluate", entry((ROWS, details_of("bottle"))))
    assert EO.main(argv + overlay_argv) == ROWS
    assert opened.pop() == ("eval_overlay", canvas, [])
    (a, k), = seen
    assert a == where and k == dict(common_keywords(session, "out"), f1_max=True, return_masks=True, **tile_keywords,
                                    **overlay_keywords, overlay_written={})
    assert capsys.readouterr().out == ED.format_table(ROWS) + "\n"
    del seen[:]
    # eval_png --masks_png, without --overlay
    monkeypatch.undo()
    monkeypatch.setattr(EL, "open_session", lambda args, name, canvas=None, log_lines=():
                        opened.append((name, canvas, list(log_lines))) or session)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(EP, "evaluate", entry((ROWS, details_of("bottle"))))
    assert EP.main(argv + ["--masks_png", "--overlay_encoder", "device"]) == ROWS
    assert opened.pop() == ("eval_png", canvas, [])
    (a, k), = seen
    assert a == where and k == dict(common_keywords(session, "out"), f1_max=True, return_masks=True, **tile_keywords,
                                    overlay=None, overlay_limit=None, overlay_thickness=1, overlay_colormap="jet",
                                    overlay_written={}, overlay_encoder="device", masks_png=True, masks_written={})
    capsys.readouterr()
    del seen[:]
    # eval_bootstrap --bootstrap: rows only, f1_max from the flags (--defects here), no return_masks and no *_written but its own
    monkeypatch.setattr(EB, "evaluate", entry(ROWS))
    assert EB.main(argv + overlay_argv + ["--bootstrap", "10", "--bootstrap_seed", "4", "--bootstrap_level", "0.9",
                                          "--bootstrap_stratified"]) == ROWS
    assert opened.pop() == ("eval_bootstrap", canvas, []) and not opened
    (a, k), = seen
    assert a == where and k == dict(common_keywords(session, "out"), f1_max=True, **tile_keywords, **overlay_keywords,
                                    overlay_encoder="pillow", masks_png=False,
                                    bootstrap={"R": 10, "seed": 4, "level": 0.9, "stratified": True}, bootstrap_written=[])
    assert capsys.readouterr().out == ED.format_table(ROWS) + "\n"


def test_run_paths_with_few_flags(monkeypatch, capsys, fake_session):
    """the defaults: no support datasets are asked for, f1_max follows the flags in eval_tiled and eval_bootstrap"""
    session, opened = fake_session
    session = session._replace(support_datasets=None)
    monkeypatch.setattr(EL, "open_session", lambda args, name, canvas=None, log_lines=():
                        opened.append((name, canvas, list(log_lines))) or session)
    seen = []
    plain = dict(batch_size=32, loader_kwargs=LOADER, logger=session.logger, use_iqm=True, device_metrics=False,
                 aupro_limit=None, defects=None, save_path="ckpt/baseline", support=None, support_weight=50.0,
                 support_form=None, support_datasets=None, coreset=None, coreset_dim=128)
    monkeypatch.setattr(ET, "evaluate_details", lambda *a, **k: seen.append((a, k)) or (ROWS, None))
    assert ET.main(["--tiles", "3"]) == ROWS
    assert opened.pop()[1] == ET.tile_geometry(518, 3, 112)[3] == 1330
    assert seen.pop() == (("model", "image datasets", "text embeddings", "device", 518, "MVTec", (3, 112)),
                          dict(plain, f1_max=False))
    monkeypatch.setattr(EB, "evaluate", lambda *a, **k: seen.append((a, k)) or ROWS)
    assert EB.main(["--bootstrap", "10"]) == ROWS
    assert opened.pop() == ("eval_bootstrap", 518, [])
    a, k = seen.pop()
    assert a == ("model", "image datasets", "text embeddings", "device", 518, "MVTec")
    assert k == dict(plain, f1_max=False, tiles=None, tile_overlap=112, overlay=None, overlay_limit=None, overlay_thickness=1,
                     overlay_colormap="jet", overlay_encoder="pillow", masks_png=False,
                     bootstrap={"R": 10, "seed": 0, "level": 0.95, "stratified": False}, bootstrap_written=[])
    assert EB.main(["--bootstrap", "10", "--masks_png"]) == ROWS and seen.pop()[1]["f1_max"] is True
    capsys.readouterr()


def test_checks_fire_in_the_order_of_the_layers(monkeypatch, capsys, fake_session):
    """a command line with two faults reports the upper layer's first; the with-flag paths state the lower layers' checks
    through those layers' functions"""
    session, opened = fake_session

    def message(main, argv):
        with pytest.raises(SystemExit):
            main(argv)
        return capsys.readouterr().err.strip().splitlines()[-1].split("error: ")[1]

    assert message(ET.main, ["--tiles", "0", "--aupro", "2"]) == "--tiles takes at least 1 tile per side"
    assert message(ET.main, ["--tiles", "2", "--aupro", "2", "--defects", "0"]) == "--aupro takes a false-positive rate in (0, 1]"
    assert message(ET.main, ["--tiles", "2", "--iqm_hidden_size", "512", "--aupro", "2"]).startswith("--iqm_hidden_size must be 768")
    assert message(ET.main, ["--tiles", "2", "--defects", "0", "--support", "0"]) == "--defects takes a minimum area of at least 1 pixel"
    assert message(ET.main, ["--tiles", "2", "--support_meta", "m", "--support_coreset", "2"]) == \
        "--support_meta and --support_coreset need --support K"
    assert message(ET.main, ["--tiles", "2", "--support", "0", "--support_coreset", "2"]) == "--support takes at least 1 shot"
    assert message(ET.main, ["--tiles", "2", "--support", "1", "--support_coreset", "2", "--support_coreset_dim", "5"]) == \
        "--support_coreset takes a share in (0, 1]"
    assert message(ET.main, ["--tiles", "2", "--support", "1", "--support_coreset", "1", "--support_coreset_dim", "5"]) == \
        "--support_coreset_dim takes 0 or a multiple of 128"
    assert message(EO.main, ["--overlay", "2", "--tiles", "0"]) == "--overlay takes the frame's weight in 0 .. 1"
    assert message(EO.main, ["--overlay", "--overlay_limit", "-1", "--overlay_thickness", "9"]) == "--overlay_limit takes a number of images"
    assert message(EO.main, ["--overlay", "--overlay_thickness", "9", "--tiles", "0"]) == "--overlay_thickness takes 0 .. 8 pixels"
    assert message(EO.main, ["--overlay", "--tiles", "0", "--aupro", "2"]) == "--tiles takes at least 1 tile per side"
    assert message(EO.main, ["--overlay", "--aupro", "2"]) == "--aupro takes a false-positive rate in (0, 1]"
    assert message(EP.main, ["--masks_png", "--overlay_thickness", "9", "--support", "0"]) == "--overlay_thickness takes 0 .. 8 pixels"
    assert message(EP.main, ["--masks_png", "--support", "0"]) == "--support takes at least 1 shot"
    assert message(EB.main, ["--bootstrap", "0", "--overlay", "2"]) == "--bootstrap takes at least 1 replicate"
    assert message(EB.main, ["--bootstrap", "5", "--bootstrap_level", "1", "--overlay", "2"]) == "--bootstrap_level takes a level in (0, 1)"
    assert message(EB.main, ["--bootstrap", "5", "--overlay_limit", "-1"]) == "--overlay_limit takes a number of images"
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert message(ET.main, ["--tiles", "2", "--aupro", "2"]).startswith("--tiles runs in one process")
    assert message(EO.main, ["--overlay", "--tiles", "2"]).startswith("--overlay runs in one process")
    assert message(EP.main, ["--masks_png"]).startswith("--overlay runs in one process")
    assert message(EB.main, ["--bootstrap", "5", "--overlay"]).startswith("--bootstrap runs in one process")
    # the lower scripts, which reach eval_last.run: theirs first, top down
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setattr(EL, "run", lambda *a, **k: pytest.fail("a refused command line reached eval_last.run"))
    assert message(EC.main, ["--support_coreset", "2"]) == "--support_coreset needs --support K"
    assert message(EC.main, ["--support", "0", "--support_coreset", "2"]) == "--support_coreset takes a share in (0, 1]"
    assert message(ES.main, ["--support_meta", "m", "--defects", "0"]) == "--support_meta needs --support K"
    assert message(ES.main, ["--support", "0", "--defects", "0"]) == "--support takes at least 1 shot"
    assert message(ED.main, ["--defects", "0", "--aupro", "2"]) == "--defects takes a minimum area of at least 1 pixel"
    assert not opened


# ------------------------------------------------------------------------------------------ the one evaluate body
WHERE = ("model", "image datasets", "text embeddings", "device", 70, "MVTec")
BOOT = {"R": 10, "seed": 1, "level": 0.9, "stratified": False}
# caller, its keywords -> f1_max, return_masks and an after_class as evaluate_rows receives them; does it return a tuple
TABLE = [
    (ES, dict(support=2), False, False, False, False),
    (ES, dict(support=2, return_masks=True), False, True, False, False),
    (ES, dict(support=2, f1_max=True), True, False, False, False),
    (ES, dict(support=2, f1_max=True, return_masks=True, save_path="out"), True, True, False, True),
    (ES, dict(support=2, defects=3), True, False, False, False),
    (ES, dict(support=2, defects=3, save_path="out", return_masks=True), True, True, False, True),
    (EC, dict(support=2, coreset=0.5), False, False, False, False),
    (EC, dict(support=2, coreset=0.5, coreset_dim=256, f1_max=True, return_masks=True), True, True, False, True),
    (EC, dict(support=2, coreset=0.5, defects=3, save_path="out"), True, False, False, False),
    (EC, dict(support=2, coreset=0.5, defects=3), True, False, False, False),
    (EO, dict(overlay=0.5, save_path="out"), True, True, True, False),
    (EO, dict(overlay=0.5, save_path="out", f1_max=True, return_masks=True), True, True, True, True),
    (EO, dict(overlay=0.5, save_path="out", defects=3), True, True, True, False),
    (EO, dict(overlay=0.5, save_path="out", support=2), True, True, True, False),
    (EO, dict(overlay=0.5, save_path="out", support=2, coreset=0.5, coreset_dim=256, return_masks=True), True, True, True, True),
    (EP, dict(masks_png=True, save_path="out"), True, True, True, False),
    (EP, dict(masks_png=True, save_path="out", return_masks=True), True, True, True, True),
    (EP, dict(overlay=0.5, overlay_encoder="device", save_path="out", defects=3), True, True, True, False),
    (EP, dict(masks_png=True, overlay=0.5, save_path="out", support=2, defects=3, return_masks=True), True, True, True, True),
    (EP, dict(masks_png=True, save_path="out", support=2, coreset=0.5), True, True, True, False),
    (EB, dict(bootstrap=BOOT), False, False, False, False),
    (EB, dict(bootstrap=BOOT, save_path="out"), False, False, False, False),
    (EB, dict(bootstrap=BOOT, f1_max=True), True, False, False, False),
    (EB, dict(bootstrap=BOOT, f1_max=True, return_masks=True, save_path="out"), True, True, False, True),
    (EB, dict(bootstrap=BOOT, defects=3), True, False, False, False),
    (EB, dict(bootstrap=BOOT, defects=3, save_path="out"), True, False, False, False),
    (EB, dict(bootstrap=BOOT, support=2), False, False, False, False),
    (EB, dict(bootstrap=BOOT, support=2, coreset=0.5, save_path="out", return_masks=True, f1_max=True), True, True, False, True),
    (EB, dict(bootstrap=BOOT, masks_png=True, save_path="out"), True, True, True, False),
    (EB, dict(bootstrap=BOOT, overlay=0.5, save_path="out", defects=3, return_masks=True), True, True, True, True),
]


@pytest.mark.parametrize("caller,keywords,f1,masks,after,returns_tuple", TABLE,
                         ids=[f"{c.__name__}-{'-'.join(k)}" for c, k, *_ in TABLE])
def test_one_evaluate_body(monkeypatch, caller, keywords, f1, masks, after, returns_tuple):
    """Every keyword of evaluate_rows is compared after its defaults are filled in, so a caller that passes a default and
    one that leaves it out count as the same call -- which they are."""
    signature = inspect.signature(EL.evaluate_rows)
    seen = {}

    def evaluate_rows(*a, **k):
        seen["rows"] = signature.bind(*a, **k)
        seen["rows"].apply_defaults()
        return ROWS

    def support_banks(*a, **k):
        seen["banks"] = (a, k)
        return {"bottle": "bank"}, "evaluated datasets"

    monkeypatch.setattr(EL, "evaluate_rows", evaluate_rows)
    monkeypatch.setattr(EL, "support_banks", support_banks)
    monkeypatch.setattr(EL, "log_coreset", lambda logger, banks: seen.update(logged=banks))
    monkeypatch.setattr(ED, "write_defects", lambda *a: seen.update(defects=a))
    monkeypatch.setattr(EB, "write_bootstrap", lambda *a: seen.update(bootstrap=a) or ["a.npz"])
    monkeypatch.delenv("RANK", raising=False)
    logger = logging.getLogger("one evaluate body")
    got = caller.evaluate(*WHERE, batch_size=4, loader_kwargs={"num_workers": 0}, logger=logger, use_iqm=False,
                          device_metrics=True, aupro_limit=0.3, support_weight=20.0, support_form="fp32",
                          support_datasets="support datasets", **keywords)
    passed = dict(seen["rows"].arguments)
    details, after_class = passed.pop("details"), passed.pop("after_class")
    support, coreset = keywords.get("support"), keywords.get("coreset")
    assert passed == dict(
        model="model", image_datasets="evaluated datasets" if support else "image datasets", text_embeddings="text embeddings",
        device="device", img_size=70, dataset="MVTec", batch_size=4, loader_kwargs={"num_workers": 0}, logger=logger,
        use_iqm=False, device_metrics=True, fpr_limit=0.3, f1_max=f1, return_masks=masks, defects=keywords.get("defects"),
        support={"bottle": "bank"} if support else None, support_weight=20.0 if support else passed["support_weight"],
        bootstrap=keywords.get("bootstrap"))
    assert passed["support_weight"] in (20.0, 50.0)               # without banks the weight is not read
    assert details == {} if f1 or "bootstrap" in keywords else details is None
    assert callable(after_class) if after else after_class is None
    # the banks: eval_last.support_banks' keywords, the coreset's only where one is asked for
    if support:
        core = {"coreset": coreset, "coreset_dim": keywords.get("coreset_dim", 128)} if coreset else {}
        assert seen["banks"] == (("model", "image datasets", 2, "device", 70),
                                 dict(form="fp32", support_datasets="support datasets", batch_size=4, **core))
    assert ("banks" in seen) == bool(support) and ("logged" in seen) == bool(coreset)
    # the .jsonl files: defects and a save_path, rank 0 or no rank
    if "defects" in keywords and "save_path" in keywords:
        assert seen["defects"] == ("out", "MVTec", details)
    else:
        assert "defects" not in seen
    assert ("bootstrap" in seen) == ("bootstrap" in keywords and "save_path" in keywords)
    assert (got == (ROWS, details)) if returns_tuple else (got == ROWS)


def test_one_evaluate_body_edges(monkeypatch):
    calls = []
    monkeypatch.setattr(EL, "evaluate_rows", lambda *a, **k: calls.append(k) or ROWS)
    monkeypatch.setattr(EL, "support_banks", lambda *a, **k: pytest.fail("no banks without support"))
    monkeypatch.setattr(ED, "write_defects", lambda *a: calls.append(a))
    for fn in (ED.evaluate_details, lambda *a, **k: ET.evaluate_details(*a, None, **k), EC.evaluate, EO.evaluate):
        extra = {"overlay": 0.5, "save_path": "out"} if fn is EO.evaluate else {}
        with pytest.raises(ValueError, match="coreset needs support=K"):
            fn(*WHERE, coreset=0.5, **extra)
    assert not calls
    # eval_tiled.evaluate_details(tiles=None) is the untiled body, keyword for keyword
    seen, names = [], list(inspect.signature(ED.evaluate_details).parameters)
    keywords = {name: f"value of {name}" for name in names[6:]}
    assert list(inspect.signature(ET.evaluate_details).parameters) == names[:6] + ["tiles"] + names[6:]
    monkeypatch.setattr(ED, "evaluate_details", lambda *a, **k: seen.append((a, k)) or "untiled")
    assert ET.evaluate_details(*WHERE, None, **keywords) == "untiled" and seen == [(WHERE, keywords)]
    monkeypatch.undo()
    # write_defects: rank 0 or no rank, defects and a save_path
    monkeypatch.setattr(EL, "evaluate_rows", lambda *a, **k: ROWS)
    monkeypatch.setattr(ED, "write_defects", lambda *a: calls.append(a))
    for rank, defects, save_path, written in ((None, 3, "out", True), ("0", 3, "out", True), ("1", 3, "out", False),
                                              (None, None, "out", False), (None, 3, None, False)):
        monkeypatch.delenv("RANK", raising=False) if rank is None else monkeypatch.setenv("RANK", rank)
        del calls[:]
        rows, details = ED.evaluate_details(*WHERE, f1_max=True, defects=defects, save_path=save_path)
        assert rows == ROWS and details == {} and calls == ([("out", "MVTec", details)] if written else [])
    # the masks asked for on the files' behalf leave the details; the caller's own stay
    details = {"bottle": {"masks": 1, "kept masks": 2, "support nearest": 3, "pixel threshold": 0.5}}
    assert EO.own_masks_only(ROWS, details, True) == (ROWS, details) and "masks" in details["bottle"]
    assert EO.own_masks_only(ROWS, details, False) == ROWS and details == {"bottle": {"pixel threshold": 0.5}}


def test_callbacks_pick_the_predicted_masks_once(monkeypatch):
    seen = []
    monkeypatch.setattr(EO, "write_overlays", lambda folder, ds, masks, preds, names, pred_masks, device, **k:
                        seen.append(("EO overlays", folder, pred_masks, k)) or ["o.png"])
    monkeypatch.setattr(EP, "write_overlays", lambda folder, ds, masks, preds, names, pred_masks, device, **k:
                        seen.append(("EP overlays", folder, pred_masks, k)) or ["p.png"])
    monkeypatch.setattr(EP, "write_masks", lambda folder, names, pred_masks, device, **k:
                        seen.append(("EP masks", folder, pred_masks, k)) or ["m.png"])
    details = {"masks": "at the threshold", "kept masks": "after the area filter"}
    call = ("bottle", "ds", "truth", "labels", "maps", "scores", ["a/good/0.png"], details)
    written, masks_written = {}, {}
    EO.overlay_callback("out", "MVTec", "dev", 0.25, limit=3, thickness=2, colormap="gray", batch_size=4, written=written)(*call)
    EO.overlay_callback("out", "MVTec", "dev", 0.25, defects=1)(*call)
    folder = os.path.join("out", "overlays", "MVTec", "bottle")
    assert seen == [("EO overlays", folder, "at the threshold", dict(alpha=0.25, limit=3, thickness=2, colormap="gray",
                                                                    batch_size=4, loader_kwargs=None)),
                    ("EO overlays", folder, "after the area filter", dict(alpha=0.25, limit=None, thickness=1, colormap="jet",
                                                                         batch_size=32, loader_kwargs=None))]
    assert written == {"bottle": ["o.png"]}
    del seen[:]
    EP.png_callback("out", "MVTec", "dev", overlay=0.5, encoder="device", masks_png=True, defects=2, written=written,
                    masks_written=masks_written)(*call)
    EP.png_callback("out", "MVTec", "dev", masks_png=True)(*call)
    EP.png_callback("out", "MVTec", "dev", overlay=0.5)(*call)
    assert [(s[0], s[2]) for s in seen] == [("EP overlays", "after the area filter"), ("EP masks", "after the area filter"),
                                           ("EP masks", "at the threshold"), ("EP overlays", "at the threshold")]
    assert seen[0][3]["encoder"] == "device" and seen[1][3] == dict(encoder="device", batch_size=32)
    assert seen[1][1] == os.path.join("out", "masks", "MVTec", "bottle")
    assert written == {"bottle": ["p.png"]} and masks_written == {"bottle": ["m.png"]}
    for make, what in ((lambda: EO.overlay_callback("out", "MVTec", "dev", 0.5), "overlays need the masks"),
                       (lambda: EP.png_callback("out", "MVTec", "dev", masks_png=True), "overlays and masks need the masks")):
        for bad in (None, {"pixel threshold": 0.5}):
            with pytest.raises(ValueError, match=what):
                make()(*call[:-1], bad)
