#!/usr/bin/env python3
"""Multi-result point query throughput (bm_scene_closest_points_multi) on the C3 scene.

    python tools/points_multi_bench.py [iters] [processes] [--json PATH]

The surface and box point sets of tools/points_bench.py at 150,000 points (fixed seed). For each:
  closestPoints in the same process, for scale;
  the k nearest triangles with rmax = +inf at k = 1, 4 and 16;
  the pure count (k = 0, BM_MULTI_COUNT_ALL) with rmax at 0.5 %, 1 % and 2 % of the scene box's diagonal.
Each figure is the median of `iters` (30) HIP-event timings on the library's stream after 10 warm-up calls, with
the ratio to closestPoints and, from the counting build, node records, triangle evaluations and the count per
point. The measurement runs in `processes` (3) fresh child processes one after the other; the parent, which
never opens the GPU, prints each and the median over them. No threshold.
"""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.points_bench import point_sets  # noqa: E402

N = 150_000
KINDS = ("surface", "box")
KS = (1, 4, 16)
RADII = (0.005, 0.01, 0.02)  # of the scene box's diagonal


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
    pos = np.concatenate([np.asarray(m["pos"], np.float32).reshape(-1, 3) for m in meshes]).astype(np.float64)
    diag = float(np.linalg.norm(pos.max(0) - pos.min(0)))

    def timed(fn):
        for _ in range(10):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, b in ev:
            a.record(stream)
            fn()
            b.record(stream)
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(b) for a, b in ev]))

    rows = []
    sets, _ = point_sets(meshes, N, np.random.default_rng(2026))
    out = torch.empty((N * 16, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    for kind in KINDS:
        p = sets[kind]

        def packed(rmax):
            return torch.from_numpy(np.concatenate([p, np.full((N, 1), rmax, np.float32)], axis=1)).to(dev)

        pts = packed(np.inf)
        torch.cuda.synchronize()
        cnt = np.zeros(4, np.uint64)
        ctx._check(scene.closestPointsDevice(pts.data_ptr(), N, out.data_ptr(), cnt))
        base = timed(lambda: ctx._check(scene.closestPointsDevice(pts.data_ptr(), N, out.data_ptr())))
        rows.append({"set": kind, "query": "closestPoints", "ms": base, "ratio": 1.0,
                     "nodes_per_point": int(cnt[0]) / N, "tris_per_point": int(cnt[1]) / N,
                     "count_per_point": int(cnt[2]) / N, "deepest_stack": int(cnt[3])})
        for k in KS:
            cnt = np.zeros(4, np.uint64)
            ctx._check(scene.closestPointsMultiDevice(pts.data_ptr(), N, k, out.data_ptr(), counts.data_ptr(), 0, cnt))
            ms = timed(lambda: ctx._check(scene.closestPointsMultiDevice(pts.data_ptr(), N, k, out.data_ptr(),
                                                                         counts.data_ptr())))
            rows.append({"set": kind, "query": f"k = {k}", "ms": ms, "ratio": ms / base,
                         "nodes_per_point": int(cnt[0]) / N, "tris_per_point": int(cnt[1]) / N,
                         "count_per_point": int(cnt[2]) / N, "deepest_stack": int(cnt[3])})
        for frac in RADII:
            near = packed(np.float32(frac * diag))
            torch.cuda.synchronize()
            cnt = np.zeros(4, np.uint64)
            flag = _lib.MULTI_COUNT_ALL
            ctx._check(scene.closestPointsMultiDevice(near.data_ptr(), N, 0, 0, counts.data_ptr(), flag, cnt))
            ms = timed(lambda: ctx._check(scene.closestPointsMultiDevice(near.data_ptr(), N, 0, 0, counts.data_ptr(),
                                                                         flag)))
            rows.append({"set": kind, "query": f"count, r = {100 * frac:g} %", "ms": ms, "ratio": ms / base,
                         "nodes_per_point": int(cnt[0]) / N, "tris_per_point": int(cnt[1]) / N,
                         "count_per_point": int(cnt[2]) / N, "deepest_stack": int(cnt[3])})
    scene.destroy()
    del keep
    ctx.close()
    print("POINTS_MULTI_BENCH " + json.dumps({"num_tris": int(ntri), "iters": iters, "points": N, "rows": rows}),
          flush=True)


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
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("POINTS_MULTI_BENCH ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"process {k} failed with exit status {r.returncode}")
        runs.append(json.loads(line[0][len("POINTS_MULTI_BENCH "):]))
        for row in runs[-1]["rows"]:
            print(f"process {k}: {row['set']:8s} {row['query']:18s} {row['ms'] * 1e3:9.1f} us  x{row['ratio']:5.2f}  "
                  f"{row['nodes_per_point']:7.1f} nodes {row['tris_per_point']:7.1f} tris {row['count_per_point']:7.2f} "
                  f"counted per point  deepest stack {row['deepest_stack']:3d}", flush=True)
    summary = []
    for i, row in enumerate(runs[0]["rows"]):
        ms = [r["rows"][i]["ms"] for r in runs]
        ratio = [r["rows"][i]["ratio"] for r in runs]
        summary.append({"set": row["set"], "query": row["query"], "ms": float(np.median(ms)), "ms_range": [min(ms), max(ms)],
                        "ratio": float(np.median(ratio)), "mpoints_per_s": N / float(np.median(ms)) * 1e-3,
                        "nodes_per_point": row["nodes_per_point"], "tris_per_point": row["tris_per_point"],
                        "count_per_point": row["count_per_point"]})
        print(f"median of {procs}: {row['set']:8s} {row['query']:18s} {summary[-1]['ms'] * 1e3:9.1f} us "
              f"({min(ms) * 1e3:.1f}-{max(ms) * 1e3:.1f})  x{summary[-1]['ratio']:5.2f}  "
              f"{summary[-1]['mpoints_per_s']:7.1f} Mpoints/s  {row['nodes_per_point']:.1f} nodes "
              f"{row['tris_per_point']:.1f} tris {row['count_per_point']:.2f} counted per point", flush=True)
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump({"num_tris": runs[0]["num_tris"], "iters": iters, "processes": procs, "points": N,
                       "summary": summary, "runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
