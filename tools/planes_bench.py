#!/usr/bin/env python3
"""Plane section query throughput (bm_scene_section_planes) on the C3 scene.

    python tools/planes_bench.py [iters] [processes] [--json PATH]

  a slicer stack: 1,024 planes along the longest axis of the scene's bounding box, evenly spaced over it, in
  BM_PLANES_COUNT, BM_PLANES_ANY, and the BM_PLANES_LIST pass writing ids and segments at the exclusive prefix sum
  of the counts ("count + list" is the sum of the two passes' medians);
  a large batch: 262,144 planes with random orientations through random points of the box, COUNT and ANY;
  one plane through the centroid of the vertices (COUNT and LIST): the worst case, one quad walking the whole
  section serially while the rest of the GPU idles (the median of 5 timings after 2 warm-up calls).
Each figure is the median of `iters` (30) HIP-event timings on the library's stream after 10 warm-up calls, with
planes per second and, from the counting build, node records, triangle tests and segments per plane. The
measurement runs in `processes` (3) fresh child processes one after the other; the parent, which never opens the
GPU, prints each and the median over them. No threshold.
"""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STACK, BATCH = 1024, 262144


def child(iters):
    import torch

    from raytracercuda_amd import _lib, beam, scenes
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = beam.Context(device=0, stream=stream.cuda_stream)
    meshes = scenes.scene("armadillo_proxy")
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    ntri = scene.updateGPUScene(stats=True)["num_tris"]
    pos = np.concatenate([np.asarray(m["pos"], np.float32).reshape(-1, 3) for m in meshes])
    lo, hi = pos.min(0), pos.max(0)

    def timed(fn, warm=10, reps=iters):
        for _ in range(warm):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record(stream)
            fn()
            b.record(stream)
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(b) for a, b in ev]))

    def planes_of(pts, nrm):
        p = np.zeros((pts.shape[0], 8), np.float32)
        p[:, 0:3], p[:, 4:7] = pts, nrm
        return torch.from_numpy(p).to(dev)

    rows = []

    def run(name, planes, mode, out, off=0, ids=0, segs=0, **how):
        n = planes.shape[0]
        cnt = np.zeros(4, np.uint64)
        ctx._check(scene.sectionPlanesDevice(planes.data_ptr(), n, mode, out, off, ids, segs, 0, cnt))
        ms = timed(lambda: ctx._check(scene.sectionPlanesDevice(planes.data_ptr(), n, mode, out, off, ids, segs)), **how)
        rows.append({"query": name, "planes": n, "ms": ms, "nodes_per_plane": int(cnt[0]) / n,
                     "tests_per_plane": int(cnt[1]) / n, "segments_per_plane": int(cnt[2]) / n,
                     "deepest_stack": int(cnt[3])})

    def with_list(name, planes, count, **how):
        n = planes.shape[0]
        offsets = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
        torch.cumsum(count, 0, dtype=torch.int32, out=offsets[1:])
        total = max(int(offsets[-1].item()), 1)
        ids = torch.empty((total,), dtype=torch.int32, device=dev)
        segs = torch.empty((total, 8), dtype=torch.float32, device=dev)
        run(name, planes, _lib.PLANES_LIST, 0, offsets.data_ptr(), ids.data_ptr(), segs.data_ptr(), **how)

    axis = int(np.argmax(hi - lo))
    normal = np.zeros(3, np.float32)
    normal[axis] = 1
    pts = np.tile((lo + hi) * np.float32(0.5), (STACK, 1))
    pts[:, axis] = lo[axis] + (np.arange(STACK, dtype=np.float32) + np.float32(0.5)) * ((hi[axis] - lo[axis]) / np.float32(STACK))
    stack = planes_of(pts, np.tile(normal, (STACK, 1)))
    count = torch.empty((STACK,), dtype=torch.int32, device=dev)
    flag = torch.empty((STACK,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    run("stack 1024 count", stack, _lib.PLANES_COUNT, count.data_ptr())
    run("stack 1024 any", stack, _lib.PLANES_ANY, flag.data_ptr())
    with_list("stack 1024 list", stack, count)

    rng = np.random.default_rng(1)
    batch = planes_of(rng.uniform(lo, hi, (BATCH, 3)), rng.normal(size=(BATCH, 3)))
    count = torch.empty((BATCH,), dtype=torch.int32, device=dev)
    flag = torch.empty((BATCH,), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    run("batch 262144 count", batch, _lib.PLANES_COUNT, count.data_ptr())
    run("batch 262144 any", batch, _lib.PLANES_ANY, flag.data_ptr())
    del batch, count, flag

    one = planes_of(pos.mean(0, dtype=np.float64)[None], np.float32([[0.3, 0.5, 0.8]]))
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    run("one plane count", one, _lib.PLANES_COUNT, count.data_ptr(), warm=2, reps=5)
    with_list("one plane list", one, count, warm=2, reps=5)
    scene.destroy()
    del keep
    ctx.close()
    print("PLANES_BENCH " + json.dumps({"num_tris": int(ntri), "iters": iters, "rows": rows}), flush=True)


def main():
    if "--child" in sys.argv:
        child(int(sys.argv[sys.argv.index("--child") + 1]))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--json" in sys.argv:
        args.remove(sys.argv[sys.argv.index("--json") + 1])
    iters = int(args[0]) if args else 30
    procs = int(args[1]) if len(args) > 1 else 3
    out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    runs = []
    for k in range(procs):  # fresh processes, one at a time; a failed one ends the measurement
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(iters)], capture_output=True,
                           text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("PLANES_BENCH ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"process {k} failed with exit status {r.returncode}")
        runs.append(json.loads(line[0][len("PLANES_BENCH "):]))
        for row in runs[-1]["rows"]:
            print(f"process {k}: {row['query']:20s} {row['ms'] * 1e3:10.1f} us  {row['nodes_per_plane']:9.2f} nodes "
                  f"{row['tests_per_plane']:9.2f} tests {row['segments_per_plane']:9.2f} segments per plane  deepest "
                  f"stack {row['deepest_stack']:3d}", flush=True)
    summary = []
    for i, row in enumerate(runs[0]["rows"]):
        ms = [r["rows"][i]["ms"] for r in runs]
        med = float(np.median(ms))
        summary.append({"query": row["query"], "planes": row["planes"], "ms": med, "ms_range": [min(ms), max(ms)],
                        "mplanes_per_s": row["planes"] / med * 1e-3, "nodes_per_plane": row["nodes_per_plane"],
                        "tests_per_plane": row["tests_per_plane"], "segments_per_plane": row["segments_per_plane"]})
        print(f"median of {procs}: {row['query']:20s} {med * 1e3:10.1f} us ({min(ms) * 1e3:.1f}-{max(ms) * 1e3:.1f})  "
              f"{summary[-1]['mplanes_per_s']:9.4f} Mplanes/s  {row['nodes_per_plane']:.2f} nodes "
              f"{row['tests_per_plane']:.2f} tests {row['segments_per_plane']:.2f} segments per plane", flush=True)
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump({"num_tris": runs[0]["num_tris"], "iters": iters, "processes": procs, "summary": summary,
                       "runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
