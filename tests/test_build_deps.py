"""What build.py takes a translation unit to be made of: `unit_deps`, read from the #include lines.

The kernel units (csrc/jtp_k_*.h) are cut so that an edit to one family's bodies recompiles that family alone and the engine
depends on the kernels' face only (csrc/jtp_kernels.hip.h has the map).  These tests hold the edges of that map; they compile nothing.
"""
import os
import shutil

import pytest

import build as jt_build

JTPROP_H = os.path.join("..", "..", "include", "jtprop.h")
FACE = "jtp_kernels.hip.h"


def kernel_units(deps):
    return set(d for d in deps if d.startswith("jtp_k_"))


def inst(family):
    units = [s for s in jt_build.INST if s.startswith("jtp_inst_%s_" % family)]
    assert len(units) == 2, units                      # (f32 and f64)
    return units


def test_multi_units_reach_reduce_and_not_pass_or_lean():
    for src in inst("multi"):
        deps = jt_build.unit_deps(src)
        assert "jtp_k_multi.h" in deps and "jtp_k_reduce.h" in deps
        assert "jtp_k_pass.h" not in deps and "jtp_k_lean.h" not in deps


def test_shape_units_reach_pass_and_not_lean_or_multi():
    for src in inst("shape"):
        deps = jt_build.unit_deps(src)
        assert "jtp_k_pass.h" in deps
        assert "jtp_k_lean.h" not in deps and "jtp_k_multi.h" not in deps


def test_every_family_unit_sees_the_face():
    for src in jt_build.INST:
        assert FACE in jt_build.unit_deps(src), src


def test_engine_reaches_the_face_of_the_kernels_only():
    deps = jt_build.unit_deps("jtp_propagate.hip")
    assert FACE in deps
    assert not kernel_units(deps)
    others = [s for s in jt_build.ENGINE if s != "jtp_propagate.hip"]
    assert len(others) == 8
    for src in others:
        deps = jt_build.unit_deps(src)
        assert FACE not in deps and not kernel_units(deps), src


def test_max_product_units_alone_reach_their_header():
    units = ["jtp_map.hip", "jtp_max.hip", "jtp_mbest.hip"]
    for src in units:
        assert src in jt_build.SOURCES
        assert "jtp_maxprod.h" in jt_build.unit_deps(src), src
    for src in jt_build.SOURCES:
        if src not in units:
            assert "jtp_maxprod.h" not in jt_build.unit_deps(src), src


def test_planner_does_not_reach_the_engine():
    for src in jt_build.PLANNER:
        assert "jtp_engine.h" not in jt_build.unit_deps(src), src


def test_every_header_is_reached():
    reached = set().union(*(jt_build.unit_deps(src) for src in jt_build.SOURCES))
    headers = set(f for f in os.listdir(jt_build.CSRC) if f.endswith(".h"))
    assert headers and headers <= reached, sorted(headers - reached)
    assert JTPROP_H in reached


@pytest.fixture(scope="module")
def tree_copy(tmp_path_factory):
    """csrc/ and include/jtprop.h, laid out as in the repository"""
    root = tmp_path_factory.mktemp("deps")
    csrc = root / "junction-tree_amd" / "csrc"
    shutil.copytree(jt_build.CSRC, str(csrc))
    os.makedirs(str(root / "include"))
    shutil.copy(os.path.join(jt_build.CSRC, JTPROP_H), str(root / "include" / "jtprop.h"))
    return str(csrc)


def test_source_id_moves_with_every_file(tree_copy):
    base = jt_build.source_id(tree_copy)
    assert base == jt_build.source_id()                # (a copy of the same text: the same id)
    reached = set().union(*(jt_build.unit_deps(src, tree_copy) for src in jt_build.SOURCES))
    files = sorted(reached | set(jt_build.SOURCES))
    assert JTPROP_H in files
    for name in files:
        path = os.path.join(tree_copy, name)
        with open(path, "rb") as fh:
            text = fh.read()
        with open(path, "ab") as fh:
            fh.write(b"// one more line\n")
        assert jt_build.source_id(tree_copy) != base, name
        with open(path, "wb") as fh:
            fh.write(text)
    assert jt_build.source_id(tree_copy) == base
