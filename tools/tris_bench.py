#!/usr/bin/env python3
"""Triangle overlap query throughput (bm_scene_overlap_triangles) on the C3 scene.

    python tools/tris_bench.py [iters] [processes] [--json PATH]

Three query sets, each every triangle of a second copy of the scene's mesh:
  "through":  the copy turned by 0.3 rad about the z axis through the scene's centre and shifted by 5 % of the
              scene's extent on every axis, so that the two meshes interpenetrate;
  "close":    the copy turned by 0.02 rad and shifted by 0.02 % of the extent: the two surfaces cross nearly
              everywhere, the narrow phase's heaviest load;
  "beside":   the turned copy of "through" shifted by half the extent along x: it mostly misses.
Each in BM_TRIS_ANY, BM_TRIS_COUNT and BM_TRIS_LIST (offsets: the exclusive prefix sum of the count pass).
Each figure is the median of `iters` (30) HIP-event timings on the library's stream after 10 warm-up calls, with
queries per second and, from the counting build, node records, triangle tests and ids per query. The measurement
runs in `processes` (3) fresh child processes one after the other; the parent, which never opens the GPU,
prints each and the median over them. No threshold.
"""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def query_sets(meshes):
    pos = [np.asarray(m["pos"], np.float32).reshape(-1, 3) for m in meshes]
    verts = np.concatenate([p[np.asarray(m["idx"]).reshape(-1, 3)] for p, m in zip(pos, meshes)]).astype(np.float64)
    allp = np.concatenate(pos)
    lo, hi = allp.min(0).astype(np.float64), allp.max(0).astype(np.float64)
    ctr, ext = (lo + hi) * 0.5, hi - lo
    c, s = np.cos(0.3), np.sin(0.3)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    turned = (verts - ctr) @ rot.T + ctr
    c, s = np.cos(0.02), np.sin(0.02)
    near = (verts - ctr) @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]).T + ctr + 0.0002 * ext
    return {"through": np.float32(turned + 0.05 * ext), "close": np.float32(near),
            "beside": np.float32(turned + np.array([0.5 * ext[0], 0.0, 0.0]))}


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

    rows = []

    def run(name, tris, mode, out, off=0, ids=0):
        n = tris.shape[0]
        cnt = np.zeros(4, np.uint64)
        ctx._check(scene.overlapTrianglesDevice(tris.data_ptr(), n, mode, out, off, ids, 0, cnt))
        ms = timed(lambda: ctx._check(scene.overlapTrianglesDevice(tris.data_ptr(), n, mode, out, off, ids)))
        rows.append({"query": name, "queries": n, "ms": ms, "nodes_per_query": int(cnt[0]) / n,
                     "tests_per_query": int(cnt[1]) / n, "ids_per_query": int(cnt[2]) / n, "deepest_stack": int(cnt[3])})

    for name, q in query_sets(meshes).items():
        n = q.shape[0]
        packed = np.zeros((n, 12), np.float32)
        packed.reshape(n, 3, 4)[:, :, 0:3] = q
        tris = torch.from_numpy(packed).to(dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        flag = torch.empty((n,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        run(f"{name} any", tris, _lib.TRIS_ANY, flag.data_ptr())
        run(f"{name} count", tris, _lib.TRIS_COUNT, count.data_ptr())
        offsets = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
        torch.cumsum(count, 0, dtype=torch.int32, out=offsets[1:])
        ids = torch.empty((max(int(offsets[-1].item()), 1),), dtype=torch.int32, device=dev)
        run(f"{name} list", tris, _lib.TRIS_LIST, 0, offsets.data_ptr(), ids.data_ptr())
        del tris, count, flag, offsets, ids
    scene.destroy()
    del keep
    ctx.close()
    print("TRIS_BENCH " + json.dumps({"num_tris": int(ntri), "iters": iters, "rows": rows}), flush=True)


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
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("TRIS_BENCH ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"process {k} failed with exit status {r.returncode}")
        runs.append(json.loads(line[0][len("TRIS_BENCH "):]))
        for row in runs[-1]["rows"]:
            print(f"process {k}: {row['query']:16s} {row['ms'] * 1e3:10.1f} us  {row['nodes_per_query']:8.2f} nodes "
                  f"{row['tests_per_query']:8.2f} tests {row['ids_per_query']:8.3f} ids per query  deepest stack "
                  f"{row['deepest_stack']:3d}", flush=True)
    summary = []
    for i, row in enumerate(runs[0]["rows"]):
        ms = [r["rows"][i]["ms"] for r in runs]
        med = float(np.median(ms))
        summary.append({"query": row["query"], "queries": row["queries"], "ms": med, "ms_range": [min(ms), max(ms)],
                        "mqueries_per_s": row["queries"] / med * 1e-3, "nodes_per_query": row["nodes_per_query"],
                        "tests_per_query": row["tests_per_query"], "ids_per_query": row["ids_per_query"]})
        print(f"median of {procs}: {row['query']:16s} {med * 1e3:10.1f} us ({min(ms) * 1e3:.1f}-{max(ms) * 1e3:.1f})  "
              f"{summary[-1]['mqueries_per_s']:9.2f} Mqueries/s  {row['nodes_per_query']:.2f} nodes "
              f"{row['tests_per_query']:.2f} tests {row['ids_per_query']:.3f} ids per query", flush=True)
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump({"num_tris": runs[0]["num_tris"], "iters": iters, "processes": procs, "summary": summary,
                       "runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
