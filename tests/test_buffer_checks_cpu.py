"""The buffer rule of the C ABI (include/aaclip.h, "Buffers of a call") without a GPU: csrc/buffers.h in a host program
under ASan + UBSan against a set-of-bytes model; then, for every entry that declares a table (tests/buffer_check_cases.py)
and every (written, other) pair of it, the other buffer laid on the written one's last and first aligned unit -- each call
refused with the entry's name and "overlap" -- and, where the entry checks the workspace size last, every call with the
workspace one byte short, so that a pair nobody checks would still be refused, and the just-adjacent placements reporting
"workspace too small".  The pairs that were not checked before the tables are named in NEW_PAIRS and must be among them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import buffer_check_cases as BC
from aaclip_hip import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "aa-clip-iqm_amd", "csrc")
NAMES = [e.name for e in BC.entries(_lib.load())]


def err():
    return _lib.load().aaclip_last_error().decode()


@pytest.fixture(scope="module")
def table():
    return {e.name: e for e in BC.entries(_lib.load())}


def test_buffers_header_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "buffers_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", CSRC, os.path.join(CSRC, "buffers_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("the sanitizer runtime of the host compiler is not installed: " + build.stderr.strip()[-200:])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok ") and not run.stderr, (run.returncode, run.stdout, run.stderr)
    assert int(run.stdout.split()[1]) > 10 ** 7


def test_the_tables_cover_the_entries_and_name_the_new_pairs(table):
    """one table per converted entry of csrc/capi.hip (each declares `const Buf b[]`; tile_entry_check serves two entries,
    optim_grad_norm's gradients are rows of its table); valid as they stand; the named pairs exist"""
    src = open(os.path.join(CSRC, "capi.hip")).read()
    assert len(re.findall(r"const Buf b\[\] = ", src)) == len(table) - 1 == 23
    assert "ranges_overlap" not in src and "clash = clash" not in src
    for name, (written, other) in ((n, p) for n, ps in BC.NEW_PAIRS.items() for p in ps):
        assert (written, other) in table[name].pairs() or (other, written) in table[name].pairs(), (name, written, other)
    header = open(os.path.join(REPO, "include", "aaclip.h")).read()
    assert "Buffers of a call" in header
    for e in table.values():
        for b in e.bufs:
            assert b.bytes > 0 and b.align in (1, 4, 8, 16)
        if torch.cuda.is_available():
            continue                       # a valid call on stand-in addresses would be enqueued
        rc = e.call(_lib.load(), e.addresses(), e.ws_need())
        assert rc in (-2, -4), (e.name, rc, err())   # past every check: only the launch fails


@pytest.mark.parametrize("name", NAMES)
def test_a_written_buffer_overlaps_no_other(table, name):
    e = table[name]
    if not e.ws_last and torch.cuda.is_available():
        pytest.skip("no check follows the overlaps of this entry: a hole would enqueue a kernel on stand-in addresses")
    lib = _lib.load()
    ws = e.ws_need() - 1 if e.ws_last else e.ws_need()
    pairs = e.pairs()
    assert set(BC.NEW_PAIRS.get(name, [])) <= set(pairs) | {(o, w) for w, o in pairs}
    for written, other in pairs:
        place = BC.placements(e, written, other)
        for kind in ("last", "first"):
            addr = dict(e.addresses())
            addr[other] = place[kind]
            assert addr[other] % e.buf(other).align == 0
            assert e.call(lib, addr, ws) == -1, (name, written, other, kind)
            assert err().startswith(e.prefix) and "overlap" in err(), (name, written, other, kind, err())
        if e.ws_last:
            for kind in ("after", "before"):
                addr = dict(e.addresses())
                addr[other] = place[kind]
                assert e.call(lib, addr, ws) == -1, (name, written, other, kind)
                assert err().startswith(e.prefix) and "workspace too small" in err(), (name, written, other, kind, err())


def test_the_top_of_the_address_space_and_empty_buffers(table):
    """a workspace that ends on the last byte of the address space still overlaps the record inside it (`p + bytes` wraps
    to 0 there); a call of no images has empty buffers, and an empty out inside the colour table is no overlap"""
    lib, e = _lib.load(), table["metrics_curve"]
    addr = dict(e.addresses())
    addr["ws"], addr["record"] = (1 << 64) - e.ws_need(), (1 << 64) - 40
    assert addr["ws"] % 8 == 0 and e.call(lib, addr, e.ws_need() - 1) == -1
    assert err().startswith(e.prefix) and "overlap" in err(), err()
    plan = _lib.OverlayPlan()
    plan.images, plan.height, plan.width, plan.panels, plan.alpha256, plan.thickness = 0, 3, 4, 7, 128, 1
    for c in range(3):
        plan.mean[c], plan.std[c] = 0.5, 0.25
    lut = BC.BASE + 5 * BC.SLOT
    args = (BC.BASE, BC.BASE + BC.SLOT, None, None, BC.BASE + 2 * BC.SLOT, lut, lut + 16)
    assert lib.aaclip_overlay_render(C.byref(plan), *args) == 0                     # nothing to do: no launch, no error


def test_the_in_place_forms_stay_allowed(table):
    """color_jitter with dst == src and metrics_normalise with out == scores pass every check (the launch then fails for
    want of a device); one element further they are a partial overlap"""
    if torch.cuda.is_available():
        pytest.skip("a valid call on stand-in addresses would be enqueued")
    lib = _lib.load()
    for name, out, src, step in (("color_jitter", "dst", "src", 3), ("metrics_normalise", "out", "scores", 4)):
        e = table[name]
        addr = dict(e.addresses())
        addr[src] = addr[out]
        assert e.call(lib, addr, e.ws_need()) in (-2, -4), (name, err())
        for shift in (step, -step):
            addr[src] = addr[out] + shift
            assert e.call(lib, addr, e.ws_need()) == -1 and "in place" in err() and "overlap" in err(), (name, shift, err())
