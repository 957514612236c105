"""Helpers to read tests/golden fixtures (shared by CPU and GPU tests)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def manifest():
    return json.load(open(os.path.join(GOLDEN, "manifest.json")))


def view(name):
    with np.load(os.path.join(GOLDEN, "views", name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def sweep():
    with np.load(os.path.join(GOLDEN, "views", "bunny_sweep.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def ref_manifest():
    return json.load(open(os.path.join(GOLDEN, "ref", "manifest.json")))


def ref_scene(name):
    """A fixture of tests/golden/ref (make_ref_frames.py): the arrays of <name>.npz plus "meshes" (from the
    fixture itself, or the tests/golden/meshes file its manifest entry names), "w", "h" and "views"."""
    from raytracercuda_amd import scenes
    with np.load(os.path.join(GOLDEN, "ref", name + ".npz"), allow_pickle=False) as z:
        s = {k: z[k] for k in z.files}
    mesh = ref_manifest()["scenes"][name]["mesh"]
    if mesh is not None:
        s["meshes"] = scenes.load_mesh(mesh)
    else:
        s["meshes"] = [{"pos": s[f"pos{i}"], "nrm": s[f"nrm{i}"], "idx": s[f"idx{i}"]}
                       for i in range(int(s["num_meshes"]))]
    s["w"], s["h"] = int(s["wh"][0]), int(s["wh"][1])
    s["views"] = list(zip(s["eyes"], s["orients"]))
    return s


def ref_frame(s, k):
    """View k of a ref_scene as dense (packed, tri) frames: what the reference's own CPU path computed."""
    n = s["w"] * s["h"]
    packed = np.full(n, 0x0000FF00, np.uint32)
    tri = np.full(n, 0xFFFFFFFF, np.uint32)
    px = s[f"hit_pixels_{k}"]
    packed[px] = s[f"hit_packed_{k}"]
    tri[px] = s[f"hit_tri_{k}"]
    return packed, tri


def ref_closest_frame(s, k):
    """ref_frame with the recorded pixels where the exhaustive closest hit differs replaced by that hit."""
    packed, tri = ref_frame(s, k)
    px = s[f"div_pixels_{k}"]
    packed[px] = s[f"div_packed_{k}"]
    tri[px] = s[f"div_tri_{k}"]
    return packed, tri


def dense(n, rec, prefix="hit"):
    """Expand a sparse reference frame (hits only) to dense (packed, tri, t) arrays of n pixels."""
    packed = np.full(n, 0x0000FF00, np.uint32)
    tri = np.full(n, 0xFFFFFFFF, np.uint32)
    t = np.full(n, np.inf, np.float32)
    px = rec[f"{prefix}_pixels"]
    packed[px] = rec[f"{prefix}_packed"]
    tri[px] = rec[f"{prefix}_tri"]
    t[px] = rec[f"{prefix}_t"]
    return packed, tri, t


def closest_hit_expected(n, rec):
    """Reference frame with the early-out divergent pixels replaced by the closest-hit answer."""
    packed, tri, t = dense(n, rec)
    px = rec["div_pixels"]
    packed[px] = rec["div_packed"]
    tri[px] = rec["div_tri"]
    t[px] = rec["div_t"]
    return packed, tri, t
