#!/usr/bin/env python3
"""Multi-hit ray-query throughput (bm_scene_trace_rays_multi) on the C3 scene, beside the closest-hit query
(bm_scene_trace_rays) on the same rays in the same process.

    python tools/multihit_bench.py [iters] [processes] [--json PATH] [--lib PATH ...]

Every process is a fresh child (its own HIP context); every figure in it is the median of `iters` HIP-event
timings on the library's stream after 10 warm-up calls; the table shows the median over the processes and
their spread. No threshold: nothing here passes or fails.

(a) the camera's 1920x1080 primary rays as a batch, row-major.
(b) one cosine-weighted bounce ray per primary hit (fixed seed), in the order of the hits.
For each: closest (bm_scene_trace_rays), multi-hit k = 1 (with and without counts_dev), 4, 16, and
BM_MULTI_COUNT_ALL with k = 0; the counting builds' node records and triangle tests per ray alongside.
--lib: further builds of the library (tools/build_ab.py, e.g. BM_MULTI_LAYOUT=1) measured the same way.
"""
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080
# (name, k (None: bm_scene_trace_rays), BM_MULTI_COUNT_ALL, counts_dev given)
MODES = [("closest", None, False, False), ("multi k=1", 1, False, True), ("multi k=1, no counts", 1, False, False),
         ("multi k=4", 4, False, True), ("multi k=16", 16, False, True), ("count all, k=0", 0, True, True)]


def child(iters):
    import torch

    from oracle import Oracle
    from raytracercuda_amd import _lib, beam, scenes
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = beam.Context(device=0, stream=stream.cuda_stream)
    meshes = scenes.scene("armadillo_proxy")
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    eye = np.float32(scenes.BUNNY_EYE)

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

    err, table = Oracle().camera_rays(W, H, *scenes.RAYS_1080)
    assert err == 0
    packed = np.zeros((W * H, 8), np.float32)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7] = eye, np.inf, table
    primary = torch.from_numpy(packed).to(dev)
    hits = scene.traceRays(primary)["hits"]
    # the bounce rays of tools/rays_bench.py (b)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    verts = torch.from_numpy(np.concatenate([m["pos"][np.asarray(m["idx"]).reshape(-1, 3).astype(np.int64)]
                                             for m in meshes]).astype(np.float32)).to(dev)
    ids = hits.view(torch.int32)[:, 3]
    sel = torch.nonzero(ids >= 0).reshape(-1)
    d0 = primary[sel, 4:7]
    p = primary[sel, 0:3] + d0 * (hits[sel, 0] * 0.9999)[:, None]
    tv = verts[ids[sel].long()]
    nrm = torch.linalg.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    nrm = nrm / torch.linalg.norm(nrm, dim=1, keepdim=True)
    nrm = torch.where((nrm * d0).sum(1, keepdim=True) > 0, -nrm, nrm)
    n = sel.numel()
    r1 = torch.rand(n, generator=gen, device=dev)
    r2 = torch.rand(n, generator=gen, device=dev) * (2 * np.pi)
    helper = torch.where(nrm[:, 0:1].abs() < 0.9, torch.tensor([1.0, 0.0, 0.0], device=dev),
                         torch.tensor([0.0, 1.0, 0.0], device=dev))
    tx = torch.linalg.cross(helper, nrm)
    tx = tx / torch.linalg.norm(tx, dim=1, keepdim=True)
    ty = torch.linalg.cross(nrm, tx)
    rad = torch.sqrt(r1)
    bounce_d = tx * (rad * torch.cos(r2))[:, None] + ty * (rad * torch.sin(r2))[:, None] + nrm * torch.sqrt(1 - r1)[:, None]
    bounce = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    bounce[:, 0:3], bounce[:, 3], bounce[:, 4:7] = p, float("inf"), bounce_d
    torch.cuda.synchronize()

    out = torch.empty((W * H * _lib.MULTI_MAX_HITS, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((W * H,), dtype=torch.int32, device=dev)
    rows = []
    for wname, rays in (("(a) primary rays, row-major", primary), ("(b) bounce rays, hit order", bounce)):
        nr = rays.shape[0]
        for mname, k, count_all, with_counts in MODES:
            if k is None:
                def call(cnt=None):
                    ctx._check(scene.traceRaysDevice(rays.data_ptr(), nr, out.data_ptr(), counters=cnt))
            else:
                def call(cnt=None, k=k, flags=_lib.MULTI_COUNT_ALL if count_all else 0,
                         cp=counts.data_ptr() if with_counts else 0):
                    ctx._check(scene.traceRaysMultiDevice(rays.data_ptr(), nr, k, out.data_ptr() if k else 0, cp, flags,
                                                          cnt))
            ms = timed(call)
            cnt = np.zeros(3, np.uint64)
            call(cnt)
            rows.append({"workload": wname, "mode": mname, "rays": int(nr), "ms": ms, "nodes_per_ray": float(cnt[0]) / nr,
                         "tris_per_ray": float(cnt[1]) / nr, "hits_per_ray": float(cnt[2]) / nr})
    print("ROWS " + json.dumps(rows), flush=True)
    scene.destroy()
    del keep
    ctx.close()


def main():
    if "--child" in sys.argv:
        return child(int(sys.argv[sys.argv.index("--child") + 1]))
    args, libs, out_json = [], [None], None
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--json":
            out_json = next(it)
        elif a == "--lib":
            libs.append(os.path.abspath(next(it)))
        else:
            args.append(a)
    iters = int(args[0]) if args else 30
    procs = int(args[1]) if len(args) > 1 else 3
    report = []
    for lib in libs:
        env = dict(os.environ)
        if lib:
            env["BEAM_HIP_LIB"] = lib
        runs = []
        for _ in range(procs):  # one fresh process after the other
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(iters)], env=env,
                               capture_output=True, text=True, timeout=600)
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")), None)
            if r.returncode or line is None:
                sys.stderr.write(r.stdout + r.stderr)
                return 1
            runs.append(json.loads(line[5:]))
        print(f"library: {lib or 'in-tree'} — medians of {iters} timings, {procs} processes", flush=True)
        base = {}
        for i, row in enumerate(runs[0]):
            ms = [run[i]["ms"] for run in runs]
            med = float(np.median(ms))
            if row["mode"] == "closest":
                base[row["workload"]] = med
            rel = med / base[row["workload"]]
            spread = (max(ms) - min(ms)) / med
            report.append(dict(row, library=lib or "in-tree", ms=med, ms_runs=ms, vs_closest=rel, spread=spread))
            print(f"{row['workload']:30s} {row['mode']:22s} {row['rays']:8d} rays {med * 1e3:9.1f} us "
                  f"({min(ms) * 1e3:.1f}-{max(ms) * 1e3:.1f}, spread {spread * 100:.1f} %) {row['rays'] / med * 1e-6:6.3f} Grays/s "
                  f"{rel:5.2f}x closest | per ray: nodes {row['nodes_per_ray']:.2f} tris {row['tris_per_ray']:.2f} "
                  f"hits {row['hits_per_ray']:.2f}", flush=True)
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump({"iters": iters, "processes": procs, "rows": report}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
