#!/usr/bin/env python3
"""Signed-distance and occupancy query throughput (bm_scene_signed_distances) on the C3 scene, beside the
hand-made chain it replaces.

    python tools/signed_bench.py [iters] [processes] [--chain-lib PATH] [--json PATH]

Two point sets of about 150 K and about 2 M points each (fixed seed, rmax = +inf):
  near  barycentric samples of random faces moved along the face normal by -5 % .. +5 % of the scene box's diagonal
  box   uniform in the scene box
each in both modes with one vote and with three. For each, the median of `iters` (30) HIP-event timings on the
library's stream after 10 warm-up calls, as points/s, with the counting build's node records and triangle
evaluations (nearest phase) and node records and triangle tests (parity phase) per point.
The chain: bm_scene_closest_points (distance mode), then per direction the ray records packed on the device
and bm_scene_trace_rays_multi with k = 0 and BM_MULTI_COUNT_ALL, then the parities summed and the sign merged
into the records (or the byte written) by torch operations on the same stream. --chain-lib names the library
the chain runs on (an older build, through BEAM_HIP_LIB); default: this one.
The measurement runs in `processes` (3) pairs of fresh child processes, the chain first, then the fused call,
one after the other; the parent, which never opens the GPU, prints each and the medians. No threshold.
"""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = (150_000, 2_000_000)
KINDS = ("near", "box")
TAG = "SIGNED_BENCH "


def point_sets(meshes, n, rng):
    verts = np.concatenate([np.asarray(m["pos"], np.float32).reshape(-1, 3)[np.asarray(m["idx"]).reshape(-1, 3)]
                            for m in meshes]).astype(np.float64)
    lo, hi = verts.reshape(-1, 3).min(0), verts.reshape(-1, 3).max(0)
    diag = float(np.linalg.norm(hi - lo))
    f = rng.integers(0, verts.shape[0], n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    v0, v1, v2 = verts[f, 0], verts[f, 1], verts[f, 2]
    nrm = np.cross(v1 - v0, v2 - v0)
    with np.errstate(all="ignore"):
        nrm = np.nan_to_num(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
    off = rng.uniform(-0.05, 0.05, n) * diag
    sets = {"near": v0 * (1 - a - b)[:, None] + v1 * a[:, None] + v2 * b[:, None] + nrm * off[:, None],
            "box": lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)}
    return {k: np.float32(v) for k, v in sets.items()}


def child(what, iters):
    import torch

    from raytracercuda_amd import _lib, beam, scenes
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = beam.Context(device=0, stream=stream.cuda_stream)
    meshes = scenes.scene("armadillo_proxy")
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    ntri = scene.updateGPUScene(stats=True)["num_tris"]
    dirs = [(_lib.SIGNED_DA, _lib.SIGNED_DB, _lib.SIGNED_DC), (-_lib.SIGNED_DB, _lib.SIGNED_DC, _lib.SIGNED_DA),
            (_lib.SIGNED_DC, -_lib.SIGNED_DA, _lib.SIGNED_DB)]

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
    rng = np.random.default_rng(2029)
    for n in SIZES:
        sets = point_sets(meshes, n, rng)
        hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
        byte = torch.empty((n,), dtype=torch.uint8, device=dev)
        votes = torch.empty((n,), dtype=torch.uint8, device=dev)
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        counts = torch.empty((n,), dtype=torch.int32, device=dev)
        for kind in KINDS:
            rec = np.zeros((n, 4), np.float32)
            rec[:, 0:3], rec[:, 3] = sets[kind], np.inf
            pts = torch.from_numpy(rec).to(dev)
            torch.cuda.synchronize()
            for vote3 in (False, True):
                for dist in (True, False):
                    row = {"set": kind, "points": n, "vote3": vote3, "mode": "distance" if dist else "occupancy"}
                    if what == "fused":
                        mode = _lib.SIGNED_DISTANCE if dist else _lib.SIGNED_OCCUPANCY
                        flags = _lib.SIGNED_VOTE3 if vote3 else 0
                        out = hits if dist else byte
                        cnt = np.zeros(4, np.uint64)
                        ctx._check(scene.signedDistancesDevice(pts, n, out, mode, flags, votes, cnt))
                        row["ms"] = timed(lambda: ctx._check(scene.signedDistancesDevice(pts, n, out, mode, flags, votes)))
                        row.update(near_nodes=int(cnt[0]) / n, near_tris=int(cnt[1]) / n, parity_nodes=int(cnt[2]) / n,
                                   parity_tris=int(cnt[3]) / n, inside=int(votes.ge(2 if vote3 else 1).sum()))
                    else:
                        def chain():
                            if dist:
                                ctx._check(scene.closestPointsDevice(pts.data_ptr(), n, hits.data_ptr()))
                            votes.zero_()
                            for d in dirs[:3 if vote3 else 1]:
                                rays[:, 0:4] = pts  # (p, tmax = rmax = +inf)
                                rays[:, 4], rays[:, 5], rays[:, 6], rays[:, 7] = d[0], d[1], d[2], 0.0
                                ctx._check(scene.traceRaysMultiDevice(rays.data_ptr(), n, 0, 0, counts.data_ptr(),
                                                                      _lib.MULTI_COUNT_ALL))
                                votes.add_(counts.bitwise_and(1).to(torch.uint8))
                            inside = votes.ge(2 if vote3 else 1)
                            if dist:
                                hits[:, 0] = torch.where(inside, -hits[:, 0], hits[:, 0])
                            else:
                                byte.copy_(inside)
                        cp = np.zeros(4, np.uint64)
                        if dist:
                            ctx._check(scene.closestPointsDevice(pts.data_ptr(), n, hits.data_ptr(), cp))
                        mh = np.zeros(2)
                        for d in dirs[:3 if vote3 else 1]:
                            rays[:, 0:4] = pts
                            rays[:, 4], rays[:, 5], rays[:, 6], rays[:, 7] = d[0], d[1], d[2], 0.0
                            torch.cuda.synchronize()
                            c3 = np.zeros(3, np.uint64)
                            ctx._check(scene.traceRaysMultiDevice(rays.data_ptr(), n, 0, 0, counts.data_ptr(),
                                                                  _lib.MULTI_COUNT_ALL, c3))
                            mh += [int(c3[0]), int(c3[1])]
                        row["ms"] = timed(chain)
                        row.update(near_nodes=int(cp[0]) / n, near_tris=int(cp[1]) / n, parity_nodes=mh[0] / n,
                                   parity_tris=mh[1] / n, inside=int(votes.ge(2 if vote3 else 1).sum()))
                    row["mpoints_per_s"] = n / row["ms"] * 1e-3
                    rows.append(row)
    scene.destroy()
    del keep
    ctx.close()
    print(TAG + json.dumps({"what": what, "num_tris": int(ntri), "iters": iters, "rows": rows}), flush=True)


def main():
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        child(sys.argv[i + 1], int(sys.argv[i + 2]))
        return
    named = {}
    args = sys.argv[1:]
    for opt in ("--chain-lib", "--json"):
        if opt in args:
            i = args.index(opt)
            named[opt] = args[i + 1]
            del args[i:i + 2]
    iters = int(args[0]) if args else 30
    procs = int(args[1]) if len(args) > 1 else 3
    runs = {"chain": [], "fused": []}
    for k in range(procs):  # fresh processes, one at a time, the chain first; a failed one ends the measurement
        for what in ("chain", "fused"):
            env = dict(os.environ)
            if what == "chain" and "--chain-lib" in named:
                env["BEAM_HIP_LIB"] = os.path.abspath(named["--chain-lib"])
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(iters)],
                               capture_output=True, text=True, timeout=600, env=env)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"process {k} ({what}) failed with exit status {r.returncode}")
            runs[what].append(json.loads(line[0][len(TAG):]))
            for row in runs[what][-1]["rows"]:
                print(f"process {k} {what:5s}: {row['set']:4s} {row['points']:8d} points {row['mode']:9s} "
                      f"{3 if row['vote3'] else 1} vote(s) {row['ms'] * 1e3:9.1f} us {row['mpoints_per_s']:8.1f} Mpoints/s  "
                      f"nearest {row['near_nodes']:5.1f} nodes {row['near_tris']:5.1f} tris, parity "
                      f"{row['parity_nodes']:5.1f} nodes {row['parity_tris']:5.1f} tris per point  inside {row['inside']}",
                      flush=True)
    summary = []
    for i, row in enumerate(runs["fused"][0]["rows"]):
        s = {k: row[k] for k in ("set", "points", "mode", "vote3", "near_nodes", "near_tris", "parity_nodes",
                                 "parity_tris", "inside")}
        for what in ("chain", "fused"):
            ms = [r["rows"][i]["ms"] for r in runs[what]]
            s[what + "_ms"], s[what + "_ms_range"] = float(np.median(ms)), [min(ms), max(ms)]
            assert runs[what][0]["rows"][i]["inside"] == row["inside"], (what, i)  # both give the same answer
        s["speedup"] = s["chain_ms"] / s["fused_ms"]
        summary.append(s)
        print(f"median of {procs}: {s['set']:4s} {s['points']:8d} points {s['mode']:9s} {3 if s['vote3'] else 1} vote(s)  "
              f"fused {s['fused_ms']:8.3f} ms ({s['fused_ms_range'][0]:.3f}-{s['fused_ms_range'][1]:.3f})  chain "
              f"{s['chain_ms']:8.3f} ms ({s['chain_ms_range'][0]:.3f}-{s['chain_ms_range'][1]:.3f})  x{s['speedup']:.2f}  "
              f"nearest {s['near_nodes']:.1f} / {s['near_tris']:.1f}, parity {s['parity_nodes']:.1f} / "
              f"{s['parity_tris']:.1f} nodes / triangles per point", flush=True)
    if "--json" in named:
        os.makedirs(os.path.dirname(os.path.abspath(named["--json"])), exist_ok=True)
        with open(named["--json"], "w") as f:
            json.dump({"num_tris": runs["fused"][0]["num_tris"], "iters": iters, "processes": procs,
                       "chain_lib": named.get("--chain-lib"), "summary": summary, "runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
