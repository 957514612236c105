#!/usr/bin/env python3
"""Instance transforms on the C3 mesh (armadillo proxy): the transform kernel, and a frame of rigid animation
against the only way there was before (host transform + synchronous re-upload + refit).

    python tools/instances_bench.py [iters] [processes] [--json PATH]

(a) k_instance_xform for 1, 8 and 64 instances, of as many uploaded copies of the mesh and of one. The C ABI runs
    the kernel only inside a build or refit, so the scene holds the C3 mesh's vertices WITHOUT triangles: its
    refit is the kernel plus the empty build (one memset, one single-thread launch), timed by the library's own
    HIP events (build_ms). The same refit of a scene whose entries are plain is that empty build alone; "net" is
    the difference of the two medians.
    Bytes that must move: 48 per vertex (12 + 12 read, 12 + 12 written) plus the 132-byte table row per entry.
    "sources" is the number of distinct vertex buffers the instances read: k instances of k uploaded copies
    stream everything; k instances of one mesh read the same 3.3 MB again and again, from the caches.
(b) A frame of rigid animation over 8 placements of the C3 mesh with its triangles (2.2 M triangles): new, 8 x
    setInstanceTransform + refitGPUScene + sync; old, per placement a numpy float32 transform of positions and
    normals, two setVertexData uploads, then the same refit + sync. Wall time per frame (time.perf_counter), the
    host part included.
Every figure is the median of `iters` timings after 10 warm-ups; the whole measurement runs in `processes`
fresh processes one after the other, and the table gives the median of their medians with the spread (min-max).
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8e12
WARMUP = 10
F = np.float32


def rigid(k, frame):
    """Placement k at animation frame `frame`: a turn about y plus a spot on a 4 x 2 grid, (3,4) float32."""
    a = 0.05 * frame + 0.7 * k
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s, 4.0 * (k % 4) - 6.0], [0, 1, 0, 3.0 * (k // 4) - 1.5], [-s, 0, c, 2.0]], F)


def child(iters):
    from raytracercuda_amd import beam, scenes
    ctx = beam.Context(device=0)
    mesh = scenes.scene("armadillo_proxy")[0]
    pos, nrm = np.ascontiguousarray(mesh["pos"], F), np.ascontiguousarray(mesh["nrm"], F)
    nv = pos.shape[0]
    out = {"vertices": nv, "triangles": int(np.asarray(mesh["idx"]).size // 3), "kernel": [], "frame": {}}

    # ---- (a) the kernel: vertices without triangles ----------------------------------------------------
    bare = {"pos": pos, "nrm": nrm, "idx": np.zeros(0, np.uint32)}
    tmp = beam.IScene.create(ctx)
    bare_meshes = beam.upload_meshes(ctx, tmp, [bare] * 64)  # 64 copies of the vertices, each in buffers of its own
    tmp.destroy()
    for k, sources in ((1, 1), (8, 8), (64, 64), (8, 1), (64, 1)):
        med = {}
        for kind in ("instances", "plain"):
            scene = beam.IScene.create(ctx)
            for i in range(k):
                if kind == "instances":
                    scene.addInstance(bare_meshes[i % sources], rigid(i, 0))
                else:
                    scene.addMesh(bare_meshes[i % sources])
            scene.updateGPUScene(stats=True)
            ms = [scene.refitGPUScene(stats=True)["build_ms"] for _ in range(WARMUP + iters)][WARMUP:]
            med[kind] = float(np.median(ms)) * 1e3
            scene.destroy()
        out["kernel"].append({"instances": k, "sources": sources, "us": med["instances"], "empty_us": med["plain"],
                              "bytes": k * (48 * nv + 132)})

    # ---- (b) a frame of rigid animation, 8 placements with triangles -----------------------------------
    k = 8
    tmp = beam.IScene.create(ctx)
    full_mesh = beam.upload_meshes(ctx, tmp, [mesh])[0]
    tmp.destroy()
    new = beam.IScene.create(ctx)
    for i in range(k):
        new.addInstance(full_mesh, rigid(i, 0))
    st = new.updateGPUScene(stats=True)
    out["frame"]["triangles"] = st["num_tris"]

    def new_frame(f):
        for i in range(k):
            new.setInstanceTransform(i, rigid(i, f))
        new.refitGPUScene()
        ctx.sync()

    def host_xform(x):
        lin, c9 = x[:, :3], beam.normal_matrix(x)
        return (pos @ lin.T + x[:, 3]).astype(F), (nrm @ c9.T).astype(F)

    old = beam.IScene.create(ctx)
    copies = beam.upload_meshes(ctx, old, [dict(mesh, pos=host_xform(rigid(i, 0))[0], nrm=host_xform(rigid(i, 0))[1])
                                           for i in range(k)])
    old.updateGPUScene(stats=True)

    def old_frame(f):
        for i in range(k):
            p, n = host_xform(rigid(i, f))
            ctx._check(copies[i].setVertexData(p, nv, 3, beam.VERTEX_DATA_POSITION))
            ctx._check(copies[i].setVertexData(n, nv, 3, beam.VERTEX_DATA_NORMAL))
        old.refitGPUScene()
        ctx.sync()

    for name, fn in (("new_ms", new_frame), ("old_ms", old_frame)):
        t = []
        for f in range(1, WARMUP + iters + 1):
            t0 = time.perf_counter()
            fn(f)
            t.append((time.perf_counter() - t0) * 1e3)
        out["frame"][name] = float(np.median(t[WARMUP:]))
    out["frame"]["refit_ms"] = float(np.median([new.refitGPUScene(stats=True)["build_ms"]
                                                for _ in range(WARMUP + iters)][WARMUP:]))
    out["frame"]["plain_refit_ms"] = float(np.median([old.refitGPUScene(stats=True)["build_ms"]
                                                      for _ in range(WARMUP + iters)][WARMUP:]))
    print("INSTANCES_BENCH " + json.dumps(out), flush=True)
    new.destroy()
    old.destroy()
    ctx.close()


def spread(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def main():
    out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    args = [a for a in sys.argv[1:] if not a.startswith("--") and a != out_json]
    if "--child" in sys.argv:
        return child(int(args[0]))
    iters = int(args[0]) if args else 30
    procs = int(args[1]) if len(args) > 1 else 3
    runs = []
    for _ in range(procs):  # one after the other: never two processes on the GPU at once
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(iters), "--child"], capture_output=True,
                           text=True, timeout=900)
        if r.returncode:
            sys.exit(f"child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
        runs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("INSTANCES_BENCH ")][-1][16:]))
    report = {"iters": iters, "processes": procs, "vertices": runs[0]["vertices"], "kernel": [], "frame": {}}
    print(f"(a) k_instance_xform, {runs[0]['vertices']} vertices per instance (refit of a scene without triangles)")
    print(f"{'instances':>9s} {'sources':>7s} {'us':>8s} {'spread us':>15s} {'empty us':>9s} {'net us':>8s} {'MB':>8s} "
          f"{'TB/s net':>9s} {'of 8 TB/s':>9s}")
    for i, row in enumerate(runs[0]["kernel"]):
        us, lo, hi = spread([r["kernel"][i]["us"] for r in runs])
        empty, _, _ = spread([r["kernel"][i]["empty_us"] for r in runs])
        net, nlo, nhi = spread([r["kernel"][i]["us"] - r["kernel"][i]["empty_us"] for r in runs])
        rate = row["bytes"] / (net * 1e-6) if net > 0 else float("nan")
        report["kernel"].append({"instances": row["instances"], "sources": row["sources"], "us": us, "us_min": lo,
                                 "us_max": hi, "empty_us": empty, "net_us": net, "net_us_min": nlo, "net_us_max": nhi,
                                 "bytes": row["bytes"],
                                 "tb_per_s": rate * 1e-12, "of_peak": rate / HBM_BYTES_PER_S})
        print(f"{row['instances']:9d} {row['sources']:7d} {us:8.1f} {lo:7.1f}-{hi:<7.1f} {empty:9.1f} {net:8.1f} "
              f"{row['bytes'] * 1e-6:8.2f} "
              f"{rate * 1e-12:9.3f} {rate / HBM_BYTES_PER_S:9.1%}")
    fr = {k: spread([r["frame"][k] for r in runs]) for k in ("new_ms", "old_ms", "refit_ms", "plain_refit_ms")}
    ratio = spread([r["frame"]["old_ms"] / r["frame"]["new_ms"] for r in runs])
    report["frame"] = {"placements": 8, "triangles": runs[0]["frame"]["triangles"],
                       **{k: {"median": v[0], "min": v[1], "max": v[2]} for k, v in fr.items()},
                       "old_over_new": {"median": ratio[0], "min": ratio[1], "max": ratio[2]}}
    print(f"(b) one frame of rigid animation, 8 placements, {runs[0]['frame']['triangles']} triangles, wall ms")
    for k, label in (("new_ms", "8 x setInstanceTransform + refit"), ("old_ms", "host transform + 16 uploads + refit"),
                     ("refit_ms", "  device time of the instanced refit"),
                     ("plain_refit_ms", "  device time of the plain refit")):
        print(f"  {label:40s} {fr[k][0]:9.3f}  ({fr[k][1]:.3f}-{fr[k][2]:.3f})")
    print(f"  old / new = {ratio[0]:.1f}x  ({ratio[1]:.1f}-{ratio[2]:.1f})")
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
