#!/usr/bin/env python3
"""One animation step of a deforming mesh, through the host path and through the device path.

    python tools/deform_bench.py [iters] [processes] [--host-only] [--lib PATH] [--json PATH]

Scenes: C3 (armadillo_proxy, 278,520 triangles) and the C5 proxy (merged_proxy, 1.1M triangles, two meshes). Every
mesh of the scene moves every step. Per scene and step:
  (a) host path   bm_mesh_set_vertex_data for positions and for normals (host arrays, synchronous) plus
                  bm_scene_refit, then a wait: wall time, since this path waits. Only calls an older library
                  has: --host-only --lib PATH measures the same steps against another build of the library
                  (BEAM_HIP_LIB), e.g. the parent commit's.
  (b) device path bm_mesh_set_vertex_data_device (positions, from a torch tensor), bm_mesh_compute_normals and
                  bm_scene_refit on one stream without a wait: HIP-event times of the upload, of the normals and
                  of the whole step, with the refit's own build_ms beside them.
  (c) effective bytes  the compulsory traffic of the normals (indices and positions read, the vertex -> corner
                  table read, normals written) over their time, as a fraction of 8 TB/s.
Medians of `iters` (30) timings after 10 warm-up steps, in `processes` (3) fresh child processes one after the
other; the parent, which never opens the GPU, prints each and the median and range over them. No threshold.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SCENES = (("C3", "armadillo_proxy"), ("C5 proxy", "merged_proxy"))
HBM_BYTES_PER_S = 8e12  # the README's roofline


def child(iters, host_only):
    import torch

    from raytracercuda_amd import beam, scenes
    POS, NRM = beam.VERTEX_DATA_POSITION, beam.VERTEX_DATA_NORMAL
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = beam.Context(device=0, stream=stream.cuda_stream)
    rows = []
    for label, name in SCENES:
        meshes = scenes.scene(name)
        scene = beam.IScene.create(ctx)
        keep = beam.upload_meshes(ctx, scene, meshes)
        ntri = scene.updateGPUScene(stats=True)["num_tris"]
        pos = [np.asarray(m["pos"], np.float32).reshape(-1, 3) for m in meshes]
        nrm = [np.ascontiguousarray(m["nrm"], np.float32).reshape(-1, 3) for m in meshes]
        # two poses to alternate between: the values do not matter to the copies, the refit sees real motion
        poses = [[np.ascontiguousarray(p + np.float32(0.002 * k) * np.sin(40 * p[:, [1, 2, 0]])) for p in pos]
                 for k in (1, 2)]

        def host_step(k):
            for m, p, n in zip(keep, poses[k & 1], nrm):
                ctx._check(m.setVertexData(p, p.shape[0], 3, POS))
                ctx._check(m.setVertexData(n, n.shape[0], 3, NRM))
            scene.refitGPUScene()
            ctx.sync()

        for k in range(10):
            host_step(k)
        wall = []
        for k in range(iters):
            t0 = time.perf_counter()
            host_step(k)
            wall.append((time.perf_counter() - t0) * 1e3)
        row = {"scene": label, "num_tris": int(ntri), "num_vertices": int(sum(p.shape[0] for p in pos)),
               "host_ms": float(np.median(wall))}
        if not host_only:
            dposes = [[torch.from_numpy(p).to(dev) for p in pose] for pose in poses]
            torch.cuda.synchronize()

            def upload(k):
                for m, t in zip(keep, dposes[k & 1]):
                    m.setVertexData(t, t.shape[0], 3, POS)

            def normals():
                for m in keep:
                    m.computeNormals()

            for k in range(10):  # the first computeNormals builds the tables
                upload(k)
                normals()
                scene.refitGPUScene()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(iters)]
            for k, e in enumerate(ev):
                e[0].record(stream)
                upload(k)
                e[1].record(stream)
                normals()
                e[2].record(stream)
                scene.refitGPUScene()
                e[3].record(stream)
            torch.cuda.synchronize()
            row["upload_ms"] = float(np.median([e[0].elapsed_time(e[1]) for e in ev]))
            row["normals_ms"] = float(np.median([e[1].elapsed_time(e[2]) for e in ev]))
            row["device_ms"] = float(np.median([e[0].elapsed_time(e[3]) for e in ev]))
            row["refit_build_ms"] = float(np.median([scene.refitGPUScene(stats=True)["build_ms"] for _ in range(iters)]))
            nv = sum(p.shape[0] for p in pos)
            ni = sum(np.asarray(m["idx"]).size for m in meshes)
            traffic = 4 * ni + 12 * nv + 4 * (nv + len(meshes) + ni) + 12 * nv
            row["normals_bytes"] = int(traffic)
            row["normals_hbm_fraction"] = traffic / (row["normals_ms"] * 1e-3) / HBM_BYTES_PER_S
        rows.append(row)
        scene.destroy()
        for m in keep:
            m.destroy()
    ctx.close()
    print("DEFORM_BENCH " + json.dumps({"iters": iters, "rows": rows}), flush=True)


def main():
    flags = {"--host-only"}
    valued = {"--lib", "--json", "--child"}
    opts, args, argv = {}, [], sys.argv[1:]
    while argv:
        a = argv.pop(0)
        if a in valued:
            opts[a] = argv.pop(0)
        elif a in flags:
            opts[a] = True
        else:
            args.append(a)
    host_only = bool(opts.get("--host-only"))
    if "--child" in opts:
        child(int(opts["--child"]), host_only)
        return
    iters = int(args[0]) if args else 30
    procs = int(args[1]) if len(args) > 1 else 3
    env = dict(os.environ)
    if "--lib" in opts:
        env["BEAM_HIP_LIB"] = os.path.abspath(opts["--lib"])
    runs = []
    for k in range(procs):  # fresh processes, one at a time; a failed one ends the measurement
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(iters)] + (["--host-only"] if host_only else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEFORM_BENCH ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"process {k} failed with exit status {r.returncode}")
        runs.append(json.loads(line[0][len("DEFORM_BENCH "):]))
        for row in runs[-1]["rows"]:
            print(f"process {k}: " + fmt(row), flush=True)
    summary = []
    for i, row in enumerate(runs[0]["rows"]):
        s = {"scene": row["scene"], "num_tris": row["num_tris"], "num_vertices": row["num_vertices"]}
        for key in ("host_ms", "upload_ms", "normals_ms", "device_ms", "refit_build_ms", "normals_hbm_fraction"):
            if key in row:
                v = [r["rows"][i][key] for r in runs]
                s[key] = float(np.median(v))
                s[key + "_range"] = [min(v), max(v)]
        if "normals_bytes" in row:
            s["normals_bytes"] = row["normals_bytes"]
        summary.append(s)
        print(f"median of {procs}: " + fmt(s, ranges=True), flush=True)
    if "--json" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["--json"])), exist_ok=True)
        with open(opts["--json"], "w") as f:
            json.dump({"iters": iters, "processes": procs, "lib": env.get("BEAM_HIP_LIB"), "summary": summary,
                       "runs": runs}, f, indent=1)


def fmt(row, ranges=False):
    def one(key, unit="ms", scale=1.0, digits=4):
        if key not in row:
            return ""
        s = f"{row[key] * scale:.{digits}f}"
        if ranges:
            lo, hi = row[key + "_range"]
            s += f" ({lo * scale:.{digits}f}-{hi * scale:.{digits}f})"
        return f"{key.rsplit('_', 1)[0]} {s} {unit}  "

    out = f"{row['scene']:8s} {row['num_tris']:8d} tris {row['num_vertices']:7d} vertices | " + one("host_ms", digits=3)
    if "device_ms" in row:
        out += ("| " + one("device_ms") + one("upload_ms") + one("normals_ms") + one("refit_build_ms") +
                f"| normals move {row['normals_bytes'] / 1e6:.2f} MB: " + one("normals_hbm_fraction", "of 8 TB/s", digits=4))
    return out


if __name__ == "__main__":
    main()
