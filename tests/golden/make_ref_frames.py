#!/usr/bin/env python3
"""Regenerate tests/golden/ref/ with the reference's own CPU path (run in the build container only:
it needs /root/reference and oracle/_ref/ref_frame, which `make -C oracle ref_frame` compiles from the
reference's sources with `#define CUDA 0`; SURVEY.md Appendix A. Nothing at test time needs either).

Outputs : tests/golden/ref/<scene>.npz   — per scene: camera, views, the reference's frames (sparse),
                                           its build report, and for the designed scenes the meshes
          tests/golden/ref/manifest.json — compiler, flags, hashes of the reference files compiled,
                                           run time, per-view counts

Per view the fixture holds the hit pixels, their packed colour (real-normal pass) and their triangle
id (bit-plane passes, Appendix A.3), and the pixels where the exhaustive closest hit
(oracle.brute_render) differs from the reference's answer, with the closest hit's id and colour: the
set within which the default (closest-hit) mode may differ from the reference. The reference has no
output for t.

Scenes  : the survey views bunny_256, suzanne_256, f16_500 (checked here against the SURVEY §8(c)
          known answers first), views 0, 5, 11 of scenes.sweep_views() at 96x96, and the designed
          scenes of tests/ref_scenes.py.

  make_ref_frames.py [scene ...]     (no argument: all scenes, and the manifest is rewritten whole)
"""
from __future__ import annotations

import hashlib
import io
import json
import os
import re
import subprocess
import sys
import tempfile
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))

import ref_scenes  # noqa: E402
from oracle import Oracle, OrcMeshes  # noqa: E402
from raytracercuda_amd import scenes  # noqa: E402

OUT = os.path.join(HERE, "ref")
REF_BIN = os.path.join(REPO, "oracle", "_ref", "ref_frame")
REF_DIR = "/root/reference/Raytracer"
MISS = 0x0000FF00
NO_TRI = 0xFFFFFFFF

# hits, sum of packed u32; distinct ids; hits on mesh 1 of f16 (tests/test_oracle_golden.py)
SURVEY_KNOWN = {"bunny_256": (8481, 113250083072), "suzanne_256": (6264, 53525903360),
                "f16_500": (8560, 126828994560)}
SURVEY_DISTINCT_IDS = {"bunny_256": 8262, "f16_500": 756}
SURVEY_F16_MESH1_HITS = 352

SURVEY_VIEWS = {
    "bunny_256": ("bunny", 256, 256, scenes.RAYS_SQUARE, scenes.BUNNY_EYE),
    "suzanne_256": ("suzanne", 256, 256, scenes.RAYS_SQUARE, (0.0, 0.0, -3.0)),
    "f16_500": ("f16", 500, 500, scenes.RAYS_SQUARE, (0.0, 0.0, -2.1)),
}
SWEEP_VIEWS = (0, 5, 11)


def all_scenes():
    """name -> scene dict (ref_scenes layout) plus "mesh": the tests/golden/meshes name, or None."""
    out = {}
    for name, (mesh, w, h, cam, eye) in SURVEY_VIEWS.items():
        out[name] = {"mesh": mesh, "meshes": scenes.load_mesh(mesh), "w": w, "h": h, "cam": tuple(cam),
                     "views": [(tuple(eye), tuple(scenes.IDENTITY.tolist()))]}
    eyes, orients = scenes.sweep_views()
    out["bunny_sweep_96"] = {"mesh": "bunny", "meshes": scenes.load_mesh("bunny"), "w": 96, "h": 96,
                             "cam": tuple(scenes.RAYS_SQUARE),
                             "views": [(tuple(eyes[k].tolist()), tuple(np.asarray(orients[k]).reshape(9).tolist()))
                                       for k in SWEEP_VIEWS]}
    for name in ref_scenes.DESIGNED:
        out[name] = dict(ref_scenes.build(name), mesh=None)
    return out


def write_scene(path, s):
    with open(path, "wb") as f:
        f.write(b"BMREFSC1")
        f.write(np.uint32(len(s["meshes"])).tobytes())
        for m in s["meshes"]:
            pos = np.ascontiguousarray(m["pos"], np.float32).reshape(-1, 3)
            nrm = np.ascontiguousarray(m["nrm"], np.float32).reshape(-1, 3)
            idx = np.ascontiguousarray(m["idx"], np.uint32).reshape(-1)
            assert nrm.shape == pos.shape
            f.write(np.array([pos.shape[0], idx.size], np.uint32).tobytes())
            f.write(pos.tobytes())
            f.write(nrm.tobytes())
            f.write(idx.tobytes())
        f.write(np.array([s["w"], s["h"]], np.uint32).tobytes())
        f.write(np.asarray(s["cam"], np.float32).tobytes())
        f.write(np.uint32(len(s["views"])).tobytes())
        for eye, orient in s["views"]:
            f.write(np.asarray(eye, np.float32).tobytes())
            f.write(np.asarray(orient, np.float32).tobytes())


_RE_LEAF = re.compile(r"^Leaf-> Depth (\d+) ")
_RE_SUMMARY = re.compile(r"^MaxDepth: (\d+), AvgDepth \d+, NumLeafs (\d+), numFaces (\d+),")
_RE_DROP = re.compile(r"^Num faces (\d+)$")


def parse_report(text):
    """The reference's stdout of one pass -> per mesh insertion (the tree is cumulative): MaxDepth,
    NumLeafs, numFaces of its summary line, the printed leaves at MaxDepth, and the `Num faces` lines
    printed while that mesh was inserted (one per face beyond the 256-face cap)."""
    rows, depths, drops = [], [], 0
    for line in text.splitlines():
        m = _RE_LEAF.match(line)
        if m:
            depths.append(int(m.group(1)))
            continue
        if _RE_DROP.match(line):
            drops += 1
            continue
        m = _RE_SUMMARY.match(line)
        if m:
            md, nl, nf = (int(x) for x in m.groups())
            assert len(depths) == nl, (len(depths), nl)
            rows.append((md, nl, nf, sum(1 for d in depths if d == md), drops))
            depths, drops = [], 0
    return np.asarray(rows, np.uint64).reshape(-1, 5)


def run_reference(s):
    """Trace scene s with the reference's binary: (colour frames [V, n], id frames [V, n], report)."""
    ntri = sum(m["idx"].size // 3 for m in s["meshes"])
    with tempfile.TemporaryDirectory() as tmp:
        sp, fp = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "frames.bin")
        write_scene(sp, s)
        r = subprocess.run([REF_BIN, sp, fp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"ref_frame exit {r.returncode}: {r.stderr[-2000:]}")
        raw = np.fromfile(fp, np.uint32)
    passes, nviews, w, h = (int(x) for x in raw[:4])
    assert (nviews, w, h) == (len(s["views"]), s["w"], s["h"]) and (1 << (passes - 1)) >= ntri
    frames = raw[4:].reshape(passes, nviews, w * h)
    chunks = r.stdout.split("== ref_frame pass ")[1:]
    assert len(chunks) == passes and "== ref_frame done" in chunks[-1]
    reports = [parse_report(c) for c in chunks]
    for rep in reports[1:]:  # the tree depends on positions and face order alone
        assert np.array_equal(rep, reports[0]), "the build report differs between passes"
    assert reports[0].shape[0] == len(s["meshes"])
    colour = frames[0]
    hit = colour != MISS
    assert not (frames == 0xDEADBEEF).any(), "a pixel was never written"
    ids = np.zeros(colour.shape, np.uint32)
    for b in range(passes - 1):
        plane = frames[1 + b]
        assert np.array_equal(plane != MISS, hit), f"hit mask of bit-plane {b} differs"  # every miss is 0xFF00
        red = plane >> 16
        assert (plane[hit] & 0xFFFF == 0).all() and np.isin(red[hit], (0, 255)).all(), f"bit-plane {b} red not 0/255"
        ids |= ((red == 255) & hit).astype(np.uint32) << np.uint32(b)
    ids[~hit] = NO_TRI
    assert (ids[hit] < ntri).all()
    assert (colour[hit] & 0xFF00FFFF == 0).all()  # a hit is red only (and never 0xFF00)
    return colour, ids, reports[0]


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same file, byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def make_scene(o, name, s):
    """-> (arrays of the scene's npz, its manifest entry)."""
    t0 = time.time()
    colour, ids, report = run_reference(s)
    t_ref = time.time() - t0
    n = s["w"] * s["h"]
    err, rays = o.camera_rays(s["w"], s["h"], *s["cam"])
    assert err == 0
    om = OrcMeshes(s["meshes"])
    arrays = {"wh": np.array([s["w"], s["h"]], np.uint32), "cam": np.asarray(s["cam"], np.float32),
              "eyes": np.asarray([e for e, _ in s["views"]], np.float32),
              "orients": np.asarray([q for _, q in s["views"]], np.float32), "build_report": report}
    if s["mesh"] is None:
        arrays["num_meshes"] = np.int32(len(s["meshes"]))
        for i, m in enumerate(s["meshes"]):
            arrays[f"pos{i}"] = np.asarray(m["pos"], np.float32)
            arrays[f"nrm{i}"] = np.asarray(m["nrm"], np.float32)
            arrays[f"idx{i}"] = np.asarray(m["idx"], np.uint32)
    views = []
    for k, (eye, orient) in enumerate(s["views"]):
        hit = np.flatnonzero(ids[k] != NO_TRI).astype(np.uint32)
        bp, bt, _ = o.brute_render(om, rays, eye, orient)
        div = np.flatnonzero((bt != ids[k]) | (bp != colour[k])).astype(np.uint32)
        arrays.update({f"hit_pixels_{k}": hit, f"hit_packed_{k}": colour[k][hit], f"hit_tri_{k}": ids[k][hit],
                       f"div_pixels_{k}": div, f"div_tri_{k}": bt[div], f"div_packed_{k}": bp[div]})
        views.append({"eye": list(eye), "orient": list(orient), "hits": int(hit.size),
                      "checksum": int(colour[k].astype(np.uint64).sum()),
                      "distinct_ids": int(np.unique(ids[k][hit]).size),
                      "closest_hit_differs": int(div.size),
                      "closest_hit_differs_id_only": int((bt != ids[k]).sum())})
    if name in SURVEY_KNOWN:  # the survey's aggregates first
        v = views[0]
        assert (v["hits"], v["checksum"]) == SURVEY_KNOWN[name], (name, v)
        if name in SURVEY_DISTINCT_IDS:
            assert v["distinct_ids"] == SURVEY_DISTINCT_IDS[name]
        if name == "f16_500":
            assert int((arrays["hit_tri_0"] >= 3704).sum()) == SURVEY_F16_MESH1_HITS
    entry = {"mesh": s["mesh"], "w": s["w"], "h": s["h"], "cam": list(s["cam"]),
             "tris": [int(m["idx"].size // 3) for m in s["meshes"]], "mesh_digest": scenes.mesh_digest(s["meshes"]),
             "build_report": {"columns": ["MaxDepth", "NumLeafs", "numFaces", "leaves_at_MaxDepth", "Num_faces_lines"],
                              "per_insertion": report.tolist()},
             "views": views, "reference_seconds": round(t_ref, 1)}
    return arrays, entry


def toolchain():
    flags = subprocess.run(["make", "-s", "-C", os.path.join(REPO, "oracle"), "-pn", "ref_frame"],
                           stdout=subprocess.PIPE, text=True).stdout
    flags = re.search(r"^REF_FLAGS := (.*)$", flags, re.M).group(1)
    src = re.search(r"^REF_SRC\s*:= (.*)$", open(os.path.join(REPO, "oracle", "Makefile")).read(), re.M).group(1).split()
    files = sorted(src + [f for f in os.listdir(REF_DIR) if f.endswith((".h", ".cuh"))])
    return {"compiler": subprocess.run(["g++", "--version"], stdout=subprocess.PIPE, text=True).stdout.splitlines()[0],
            "flags": flags, "substitution": "Types.h: `#define CUDA 1` -> `#define CUDA 0`",
            "reference_sha256": {f: hashlib.sha256(open(os.path.join(REF_DIR, f), "rb").read()).hexdigest()
                                 for f in files}}


# Scenes the reference's binary could not trace (it asserted or crashed): name -> why. None so far.
LEFT_OUT = {}


def main(argv):
    subprocess.run(["make", "-s", "-C", os.path.join(REPO, "oracle"), "ref_frame"], check=True)
    os.makedirs(OUT, exist_ok=True)
    o = Oracle()
    todo = all_scenes()
    mpath = os.path.join(OUT, "manifest.json")
    if argv:
        todo = {k: todo[k] for k in argv}
        manifest = json.load(open(mpath))
    else:
        manifest = {"generator": "tests/golden/make_ref_frames.py", "driver": "oracle/ref_frame.cpp", "scenes": {}}
    t0 = time.time()
    for name, s in todo.items():
        arrays, entry = make_scene(o, name, s)
        path = os.path.join(OUT, name + ".npz")
        write_npz(path, arrays)
        entry["bytes"] = os.path.getsize(path)
        assert entry["bytes"] < (1 << 20), (name, entry["bytes"])
        manifest["scenes"][name] = entry
        print(name, entry["bytes"], "bytes", entry["reference_seconds"], "s",
              [(v["hits"], v["closest_hit_differs"]) for v in entry["views"]], entry["build_report"]["per_insertion"])
    manifest.update(toolchain())
    manifest["left_out"] = LEFT_OUT
    if not argv:
        manifest["run_seconds"] = round(time.time() - t0)
    json.dump(manifest, open(mpath, "w"), indent=1)
    print("done in", round(time.time() - t0), "s")


if __name__ == "__main__":
    main(sys.argv[1:])
