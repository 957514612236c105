"""Pin the oracle's restatement of the reference (oracle/beam_oracle.c: kd build + march) to what the
reference's OWN code computes, pixel by pixel.

tests/golden/ref holds frames traced by the reference's CPU-emulation path (`#define CUDA 0`), compiled
unmodified from its sources and driven through its public API (oracle/ref_frame.cpp, oracle/Makefile
target ref_frame, tests/golden/make_ref_frames.py): packed colour from a pass with the real normals,
triangle id from bit-plane passes. The survey views and small designed scenes (tests/ref_scenes.py)
aimed at what aggregates cannot see: exact-t ties, the faces the 256-face cap drops, the leaf the
first-hit-leaf early-out stops in, zero direction components, eyes on split planes, the world box,
the camera's ray recurrence, global ids over several meshes.

The reference has no output for t: t stays pinned through the glm primitive pin
(tests/test_oracle_glm_pin.py) only. NaN and out-of-range inputs stay pinned to the oracle only.
"""
import importlib.util
import os
import subprocess
import zipfile

import numpy as np
import pytest

import ref_scenes
from golden_io import GOLDEN, ref_frame, ref_manifest, ref_scene

SCENES = ("bunny_256", "suzanne_256", "f16_500", "bunny_sweep_96") + ref_scenes.DESIGNED
REF_PRESENT = os.path.isdir("/root/reference/Raytracer")


def test_manifest_lists_every_scene_and_nothing_was_left_out():
    m = ref_manifest()
    assert set(m["scenes"]) == set(SCENES)
    assert m["left_out"] == {}
    assert "-ffp-contract=off" in m["flags"] and "-march" not in m["flags"] and "NDEBUG" not in m["flags"]


@pytest.mark.parametrize("name", ref_scenes.DESIGNED)
def test_designed_scene_in_fixture_is_the_one_built_here(name):
    """The fixture stores its own inputs; they are what ref_scenes builds today (meshes, camera, views)."""
    s, b = ref_scene(name), ref_scenes.build(name)
    assert len(s["meshes"]) == len(b["meshes"]) and (s["w"], s["h"]) == (b["w"], b["h"])
    for ms, mb in zip(s["meshes"], b["meshes"]):
        for k in ("pos", "nrm", "idx"):
            assert ms[k].dtype == mb[k].dtype and np.array_equal(ms[k], mb[k]), k
    assert np.array_equal(s["cam"], np.asarray(b["cam"], np.float32))
    assert np.array_equal(s["eyes"], np.asarray([e for e, _ in b["views"]], np.float32))
    assert np.array_equal(s["orients"], np.asarray([q for _, q in b["views"]], np.float32))


@pytest.mark.parametrize("name", SCENES)
def test_kd_restatement_equals_reference_on_every_pixel(oracle, name):
    """oracle.kd_render's packed colour and triangle id == the reference's, on every pixel of every view."""
    s = ref_scene(name)
    err, rays = oracle.camera_rays(s["w"], s["h"], *s["cam"])
    assert err == 0
    kd = oracle.kd_build(s["meshes"])
    mv = ref_manifest()["scenes"][name]["views"]
    for k, (eye, orient) in enumerate(s["views"]):
        packed, tri, _ = kd.render(rays, eye, orient)
        rp, rt = ref_frame(s, k)
        bad = np.flatnonzero((tri != rt) | (packed != rp))
        assert bad.size == 0, (f"{name} view {k}: {bad.size} pixels differ, first {bad[:5]}: ids {tri[bad[:5]]} vs "
                               f"reference {rt[bad[:5]]}, colours {packed[bad[:5]]} vs {rp[bad[:5]]}")
        hit = rt != 0xFFFFFFFF
        assert int(hit.sum()) == mv[k]["hits"] and int(rp.astype(np.uint64).sum()) == mv[k]["checksum"]
        assert np.unique(rt[hit]).size == mv[k]["distinct_ids"]
        assert s[f"div_pixels_{k}"].size == mv[k]["closest_hit_differs"]


@pytest.mark.parametrize("name", SCENES)
def test_kd_statistics_equal_the_reference_build_report(oracle, name):
    """The reference prints, after inserting each mesh, a walk of the tree so far (BuildTree.cu:307-360):
    one line per childless node, then MaxDepth, NumLeafs (childless nodes) and numFaces (the sum of the
    leaves' insert counters, which run past the cap); while inserting, one `Num faces` line per face
    beyond a leaf's 256 slots. Mapping to orc_kd_stats of the tree over meshes[0..i]:
      NumLeafs == stats[1] (leaves), MaxDepth == stats[5], numFaces == stats[2] + stats[3] (stored +
      dropped), `Num faces` lines up to and including insertion i == stats[3], and the printed leaves at
      MaxDepth == the leaves that hold faces (orc_kd_leaves)."""
    s = ref_scene(name)
    rep = s["build_report"].astype(np.int64)
    assert rep.shape == (len(s["meshes"]), 5)
    dropped = np.cumsum(rep[:, 4])
    for i in range(len(s["meshes"])):
        kd = oracle.kd_build(s["meshes"][: i + 1])
        st = kd.stats().astype(np.int64)
        keys, counts, faces, depth = kd.leaves()
        if rep[i, 2] == 0:  # nothing of it lies inside the world box
            assert st[2] == st[3] == 0 and keys.size == 0
            continue
        assert (st[5], st[1], st[2] + st[3], st[3]) == (rep[i, 0], rep[i, 1], rep[i, 2], dropped[i]), (name, i, st, rep[i])
        assert keys.size == rep[i, 3] and depth == rep[i, 0]
        assert int(counts.sum()) == rep[i, 2] and faces.size == rep[i, 2] - dropped[i]


def test_cap_scene_drops_the_nearest_faces():
    """What the scene is for: 44 + 344 faces dropped, and on most hit pixels the closest hit is one of them."""
    s = ref_scene("cap")
    assert s["build_report"][0, 4] == 388
    dropped = np.r_[256:300, 300 + 256:900]
    assert np.isin(s["div_tri_0"], dropped).sum() >= 200
    assert not np.isin(s["hit_tri_0"], dropped).any()


def test_early_out_scene_has_pixels_where_the_first_hit_leaf_is_not_the_closest_hit():
    s = ref_scene("early_out")
    assert sum(s[f"div_pixels_{k}"].size for k in range(len(s["views"]))) >= 100


@pytest.mark.skipif(not REF_PRESENT, reason="needs /root/reference (the build container)")
def test_fixture_is_what_the_reference_computes(oracle, tmp_path):
    """Rebuild oracle/_ref/ref_frame from the reference's sources, trace two small scenes again and
    require the committed fixtures byte for byte."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-s", "-B", "-C", os.path.join(repo, "oracle"), "ref_frame"], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    spec = importlib.util.spec_from_file_location("make_ref_frames", os.path.join(GOLDEN, "make_ref_frames.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    todo = gen.all_scenes()
    for name in ("ties", "cap"):
        arrays, _ = gen.make_scene(oracle, name, todo[name])
        path = str(tmp_path / (name + ".npz"))
        gen.write_npz(path, arrays)
        with zipfile.ZipFile(path) as new, zipfile.ZipFile(os.path.join(GOLDEN, "ref", name + ".npz")) as old:
            assert new.namelist() == old.namelist(), name
            for member in old.namelist():  # each array file (header, dtype, shape, data), byte for byte
                assert new.read(member) == old.read(member), (name, member)
