"""CPU-only: every workspace / size / path query still returns what the parent of the layout refactor returned (tests/golden/
workspace_queries.json, recorded from a build of that parent by tests/golden/make_workspace_golden.py -- never from the tree under test),
and csrc/hyb_internal.h is the one place an internal function is declared."""
import glob
import importlib.util
import json
import os
import re

import pytest

from transformer_cnn_hybrid_network_for_video_processing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "transformer_cnn_hybrid_network_for_video_processing_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_queries.json")


def _maker():
    spec = importlib.util.spec_from_file_location("make_workspace_golden", os.path.join(ROOT, "tests", "golden", "make_workspace_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def built():
    from transformer_cnn_hybrid_network_for_video_processing_amd import build
    build.build()
    return _lib.lib


def test_golden_file_covers_the_grid():
    """The committed file holds exactly the rows the generator asks for (a grid change without a regeneration from the parent shows here)."""
    golden = json.load(open(GOLDEN))
    want = {}
    for fn, which, args in _maker().grid():
        want.setdefault(fn, []).append([which] + args)
    assert sorted(golden) == sorted(want)
    for fn in want:
        assert [r[:-1] for r in golden[fn]] == want[fn], fn
    for fn in ("hyb_convstage_fwd_workspace", "hyb_convstage_infer_workspace", "hyb_convstage_bwd_workspace", "hyb_backbone_fwd_workspace",
               "hyb_backbone_bwd_workspace", "hyb_backbone_infer_workspace", "hyb_encoder_workspace_bytes", "hyb_encoder_saved_bytes",
               "hyb_temporal_bwd_workspace", "hyb_convstage_route_elems", "hyb_convstage_packed_bwd_elems", "hyb_conv3x3_pool_fused",
               "hyb_conv3x3_wgrad_workspace", "hyb_conv_stats_rows"):
        assert fn in golden and any(r[-1] > 0 for r in golden[fn]), fn


def test_every_query_equals_the_parents_value(built, monkeypatch):
    for k in [k for k in os.environ if k.startswith("HYB_")]:
        monkeypatch.delenv(k)
    maker = _maker()
    golden = json.load(open(GOLDEN))
    bad = []
    for fn, rows in golden.items():
        for which, *args, value in rows:
            got = maker.ask(built, fn, which, args)
            if got != value:
                bad.append((fn, which, args, value, got))
    assert not bad, f"{len(bad)} of {sum(len(v) for v in golden.values())} query values differ from the parent's, first: {bad[:5]}"


def test_bad_arguments_return_zero(built):
    assert built.query("hyb_backbone_fwd_workspace", 1, 0, None) == 0
    assert built.query("hyb_backbone_bwd_workspace", 1, 1, None, 2, 16, 16) == 0
    assert built.query("hyb_convstage_infer_workspace", 1, 0, 2, 16, 16, 33, 64) == 0
    assert built.query("hyb_encoder_workspace_bytes", 1, 2, 4, 64, 128, 0, 2) == 0
    assert built.query("hyb_temporal_bwd_workspace", 1, 0, 4, 16, 32, 64, 128, 1, 2) == 0


def _strip(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


# a function named hyb_* at the start of a line, its parameter list, then `;` (a declaration) -- not `{` (a definition)
_DECL = re.compile(r'^(?!\s)(?:extern "C" )?[A-Za-z_][\w \*&]*?\b(hyb_\w+)\s*\(([^;{}]*)\)\s*;', re.M)


def test_internal_functions_are_declared_in_one_header_only():
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        found = [m.group(1) for m in _DECL.finditer(_strip(open(path).read())) if not m.group(0).lstrip().startswith("return")]
        assert not found, f"{os.path.basename(path)} redeclares {found}: prototypes of internal functions live in csrc/hyb_internal.h"
    header = _strip(open(os.path.join(CSRC, "hyb_internal.h")).read())
    names = [m.group(1) for m in _DECL.finditer(header)]
    assert len(names) >= 40 and len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    for want in ("hyb_gemm_nt", "hyb_conv_v2", "hyb_stage1_fwd", "hyb_encoder_bwd_impl", "hyb_convstage_bwd_impl"):
        assert want in names
    # every file that defines or calls one of them sees the prototype: a changed signature fails to compile in the defining file
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        src = _strip(open(path).read())
        if any(re.search(r"\b%s\s*\(" % n, src) for n in names):
            assert '#include "hyb_internal.h"' in src, os.path.basename(path)


def test_one_helper_reads_the_environment_and_one_rounds_to_256():
    getenv, al = [], []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        for i, line in enumerate(open(path).read().split("\n"), 1):
            if "getenv" in _strip(line):
                getenv.append((os.path.basename(path), i))
            if re.search(r"inline size_t al\w*\(", line):
                al.append((os.path.basename(path), i))
    assert [f for f, _ in getenv] == ["hyb_internal.h"], getenv
    assert [f for f, _ in al] == ["hyb_internal.h"], al
