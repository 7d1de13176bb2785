"""Coverage of tests/stream_cases.py, proven from include/aaclip.h: every entry point that takes a stream has a stream
case or a stated exemption, and an entry point with a workspace is never exempt.  A new entry point without a stream
case fails here."""
import os
import re

import stream_cases as SC
from aaclip_hip import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS_PARAM = re.compile(r"\bvoid\s*\*\s*(ws|workspace)\b")
STREAM_PARAM = re.compile(r"\bvoid\s*\*\s*stream\b")


def prototypes():
    """name -> parameter list text of every function include/aaclip.h declares"""
    text = open(os.path.join(REPO, "include", "aaclip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(aaclip_\w+)\s*\(([^()]*)\)\s*;", text)}


def stream_entries():
    return {n: a for n, a in prototypes().items() if STREAM_PARAM.search(a) and not n.startswith("aaclip_profile_")}


def test_header_parse_sees_the_whole_interface():
    protos = prototypes()
    assert set(protos) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.SIGNATURES)
    for name, args in protos.items():      # the binding's argument count is the header's
        n = 0 if args.strip() in ("", "void") else args.count(",") + 1
        assert n == len(_lib.SIGNATURES[name][1]), name
    entries = stream_entries()
    assert len(entries) >= 70 and "aaclip_gemm" in entries and "aaclip_optim_grad_norm" in entries
    assert "aaclip_resample_table" not in entries and "aaclip_profile_begin" not in entries


def test_every_stream_entry_has_a_case_or_an_exemption():
    entries = stream_entries()
    missing = sorted(n for n in entries if n not in SC.CASES and n not in SC.EXEMPT)
    assert not missing, f"no stream case and no exemption: {missing}"
    both = sorted(set(SC.CASES) & set(SC.EXEMPT))
    assert not both, f"both a case and an exemption: {both}"
    for name in list(SC.CASES) + list(SC.EXEMPT):
        assert name in entries, f"{name}: not an entry point with a stream in include/aaclip.h"
        assert name in _lib.SIGNATURES, name


def test_no_entry_with_a_workspace_is_exempt():
    entries = stream_entries()
    with_ws = sorted(n for n, a in entries.items() if WS_PARAM.search(a))
    assert len(with_ws) >= 40
    for name in with_ws:
        assert name not in SC.EXEMPT, f"{name} takes a workspace: it needs a stream case"
        assert SC.CASES.get(name), name
    for name, reason in SC.EXEMPT.items():
        assert isinstance(reason, str) and len(reason) > 10, name


def test_the_named_entries_without_a_workspace_have_their_cases():
    for name in ("aaclip_row_head_backward", "aaclip_optim_adam_step", "aaclip_text_embed", "aaclip_adapter_mix_fold",
                 "aaclip_layernorm_split", "aaclip_attention_backward", "aaclip_gemm", "aaclip_attention",
                 "aaclip_attention_split"):
        assert SC.CASES.get(name), name
    assert {"fp32_m4100", "fp16_m4100", "fp16x2_m4100", "fp16_m200"} <= set(SC.CASES["aaclip_gemm"])
    assert {f"{d}_l{L}" for d in ("fp32", "fp16", "bf16") for L in (130, 600)} <= set(SC.CASES["aaclip_attention"])
    assert {"l130", "l600"} <= set(SC.CASES["aaclip_attention_split"])
    ids = SC.case_ids()
    assert len(ids) == len(set(ids)) == sum(len(v) for v in SC.CASES.values())
