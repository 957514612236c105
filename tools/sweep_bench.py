#!/usr/bin/env python3
"""Sphere-cast query throughput (bm_scene_sweep_spheres) on the C3 scene.

    python tools/sweep_bench.py [iters] [processes] [--json PATH]

Two origin sets of about 150 K and about 2 M sweeps each (fixed seed), each towards a random point of the
scene box (dir not normalised, tmax = +inf):
  near  origins near the surface: barycentric samples of random faces moved along the face normal by 0.06-0.2
        of the scene box's diagonal
  far   origins at 1-3 box diagonals from the scene's centre
each with radii of 0.1 % and of 5 % of the diagonal. For each, the median of `iters` (30) HIP-event timings on
the library's stream after 10 warm-up calls, as sweeps/s, with the counting build's node records and triangle
evaluations per sweep. The closest-hit ray query (bm_scene_trace_rays) over the same origins and directions
goes beside them for scale. The measurement runs in `processes` (3) fresh child processes one after the
other; the parent, which never opens the GPU, prints each and the median over them. No threshold.
"""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = (150_000, 2_000_000)
KINDS = ("near", "far")
RADII = (0.001, 0.05)  # of the scene box's diagonal


def origin_sets(meshes, n, rng):
    verts = np.concatenate([np.asarray(m["pos"], np.float32).reshape(-1, 3)[np.asarray(m["idx"]).reshape(-1, 3)]
                            for m in meshes]).astype(np.float64)
    lo, hi = verts.reshape(-1, 3).min(0), verts.reshape(-1, 3).max(0)
    c, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    f = rng.integers(0, verts.shape[0], n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    v0, v1, v2 = verts[f, 0], verts[f, 1], verts[f, 2]
    nrm = np.cross(v1 - v0, v2 - v0)
    with np.errstate(all="ignore"):
        nrm = np.nan_to_num(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    off = rng.uniform(0.06, 0.2, n) * diag
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sets = {"near": v0 * (1 - a - b)[:, None] + v1 * a[:, None] + v2 * b[:, None] + nrm * off[:, None],
            "far": c + d * rng.uniform(1.0, 3.0, (n, 1)) * diag}
    targets = lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)
    return {k: np.float32(v) for k, v in sets.items()}, np.float32(targets), diag


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
    rng = np.random.default_rng(2027)
    for n in SIZES:
        sets, targets, diag = origin_sets(meshes, n, rng)
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        flags = torch.empty((n,), dtype=torch.uint8, device=dev)
        for kind in KINDS:
            o = sets[kind]
            rec = np.zeros((n, 8), np.float32)
            rec[:, 0:3], rec[:, 3], rec[:, 4:7] = o, np.inf, targets - o
            rays = torch.from_numpy(rec).to(dev)  # pad = 0: a plain ray
            torch.cuda.synchronize()
            ray_ms = timed(lambda: ctx._check(scene.traceRaysDevice(rays.data_ptr(), n, out.data_ptr())))
            for frac in RADII:
                rec[:, 7] = frac * diag
                sw = torch.from_numpy(rec).to(dev)
                torch.cuda.synchronize()
                cnt = np.zeros(4, np.uint64)
                ctx._check(scene.sweepSpheresDevice(sw, n, out, counters=cnt))
                ms = timed(lambda: ctx._check(scene.sweepSpheresDevice(sw, n, out)))
                any_ms = timed(lambda: ctx._check(scene.sweepSpheresDevice(sw, n, flags, mode=_lib.SWEEP_ANY)))
                rows.append({"set": kind, "radius": frac, "sweeps": n, "ms": ms, "msweeps_per_s": n / ms * 1e-3,
                             "any_ms": any_ms, "nodes_per_sweep": int(cnt[0]) / n, "tris_per_sweep": int(cnt[1]) / n,
                             "found": int(cnt[2]), "deepest_stack": int(cnt[3]),
                             "rays_ms": ray_ms, "mrays_per_s": n / ray_ms * 1e-3})
    scene.destroy()
    del keep
    ctx.close()
    print("SWEEP_BENCH " + json.dumps({"num_tris": int(ntri), "iters": iters, "rows": rows}), flush=True)


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
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("SWEEP_BENCH ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"process {k} failed with exit status {r.returncode}")
        runs.append(json.loads(line[0][len("SWEEP_BENCH "):]))
        for row in runs[-1]["rows"]:
            print(f"process {k}: {row['set']:5s} r {row['radius']:.3f} {row['sweeps']:8d} sweeps {row['ms'] * 1e3:9.1f} us "
                  f"{row['msweeps_per_s']:8.1f} Msweeps/s (any {row['any_ms'] * 1e3:9.1f} us)  {row['nodes_per_sweep']:6.1f} "
                  f"nodes {row['tris_per_sweep']:6.1f} tris per sweep  hits {row['found']:8d}  deepest stack "
                  f"{row['deepest_stack']:3d} | closest-hit rays {row['rays_ms'] * 1e3:9.1f} us "
                  f"{row['mrays_per_s']:8.1f} Mrays/s", flush=True)
    summary = []
    for i, row in enumerate(runs[0]["rows"]):
        rates = [r["rows"][i]["msweeps_per_s"] for r in runs]
        rays = [r["rows"][i]["mrays_per_s"] for r in runs]
        anys = [r["rows"][i]["any_ms"] for r in runs]
        summary.append({"set": row["set"], "radius": row["radius"], "sweeps": row["sweeps"],
                        "msweeps_per_s": float(np.median(rates)), "msweeps_per_s_range": [min(rates), max(rates)],
                        "any_ms": float(np.median(anys)), "nodes_per_sweep": row["nodes_per_sweep"],
                        "tris_per_sweep": row["tris_per_sweep"], "mrays_per_s": float(np.median(rays))})
        print(f"median of {procs}: {row['set']:5s} r {row['radius']:.3f} {row['sweeps']:8d} sweeps "
              f"{summary[-1]['msweeps_per_s']:8.1f} Msweeps/s ({min(rates):.1f}-{max(rates):.1f})  any "
              f"{summary[-1]['any_ms'] * 1e3:.1f} us  {row['nodes_per_sweep']:.1f} nodes {row['tris_per_sweep']:.1f} tris "
              f"per sweep | closest-hit rays {summary[-1]['mrays_per_s']:.1f} Mrays/s", flush=True)
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump({"num_tris": runs[0]["num_tris"], "iters": iters, "processes": procs, "summary": summary,
                       "runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
