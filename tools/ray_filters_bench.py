#!/usr/bin/env python3
"""What the ray query filters cost (bm_scene_trace_rays / bm_scene_trace_rays_multi with BM_RAYS_CULL_* and
BM_RAYS_PAD_* flags), and whether the unfiltered queries moved against another build of the library.

    python tools/ray_filters_bench.py [iters] [processes] [--json PATH] [--lib PATH ...]

The batch: tests/test_gpu_rays.py's make_batch scheme scaled up — 1,024 eyes around the armadillo proxy, 1,024
rays each into its box, 1,048,576 rays, traced in that order. Every process is a fresh child (its own HIP
context); every figure in it is the median of `iters` HIP-event timings on the library's stream after 10 warm-up
calls. The builds (this tree's and every --lib, e.g. the parent commit's library) take turns process by process,
so that they share whatever else the machine is doing; the table shows each build's median over its processes
and their spread (min .. max). No threshold: nothing here passes or fails.

(a) flags = 0: closest, any hit, multi-hit k = 4 — per build.
(b) each filter on the same rays beside flags = 0 in the same process, as a ratio (builds that have the filters):
    cull back, cull front; skip_tri = the ray's own closest hit (the ray goes on to the next surface); tmin = 0
    (rejects nothing) and tmin = half the closest t; ray_mask = all ones over default masks (rejects nothing: the
    owner search alone) and over masks 1, 2, 4, ... per entry with ray masks cycling 1..7.
"""
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GROUPS = PER = 1024
QUERIES = [("closest", None), ("any hit", "any"), ("multi k=4", 4)]


def make_batch(meshes, groups=GROUPS, per=PER, seed=7):
    """`groups` eyes on a sphere around the meshes' box, `per` rays each to uniform targets inside 1.5 x the box."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([np.asarray(m["pos"], np.float32).reshape(-1, 3) for m in meshes]).astype(np.float64)
    lo, hi = pos.min(0), pos.max(0)
    c, ext = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    u = rng.normal(size=(groups, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    eyes = np.float32(c + 0.9 * ext * u)
    targets = np.float32(c + rng.uniform(-0.75, 0.75, (groups, per, 3)) * (hi - lo))
    o = np.repeat(eyes, per, axis=0)
    return o, (targets - eyes[:, None, :]).reshape(-1, 3) + np.float32(0.0)


def child(iters):
    import torch

    from raytracercuda_amd import _lib, beam, scenes
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = beam.Context(device=0, stream=stream.cuda_stream)
    meshes = scenes.scene("armadillo_proxy")
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    has_filters = hasattr(ctx.lib, "bm_scene_set_entry_mask")

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

    o, d = make_batch(meshes)
    n = o.shape[0]
    packed = np.zeros((n, 8), np.float32)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7] = o, np.inf, d
    base = torch.from_numpy(packed).to(dev)
    first = scene.traceRays(base)["hits"].clone()
    torch.cuda.synchronize()

    def with_pad(words):  # a copy of the batch with this int32 pad column
        r = base.clone()
        r.view(torch.int32)[:, 7] = words
        return r

    ones = torch.full((n,), -1, dtype=torch.int32, device=dev)
    cases = [("flags = 0", 0, base, None)]
    if has_filters:
        cycle = (torch.arange(n, device=dev, dtype=torch.int32) % 7) + 1
        entry_bits = [1 << (i % 3) for i in range(len(meshes))]
        cases += [
            ("cull back", _lib.RAYS_CULL_BACK, base, None),
            ("cull front", _lib.RAYS_CULL_FRONT, base, None),
            ("skip_tri = closest hit", _lib.RAYS_PAD_SKIP_TRI, with_pad(first.view(torch.int32)[:, 3]), None),
            ("tmin = 0", _lib.RAYS_PAD_TMIN, with_pad(torch.zeros((n,), dtype=torch.int32, device=dev)), None),
            ("tmin = t / 2", _lib.RAYS_PAD_TMIN,
             with_pad(torch.where(torch.isfinite(first[:, 0]), first[:, 0] * 0.5, torch.zeros_like(first[:, 0]))
                      .view(torch.int32)), None),
            ("ray_mask = all ones, default masks", _lib.RAYS_PAD_MASK, with_pad(ones), [0xFFFFFFFF] * len(meshes)),
            ("ray_mask 1..7, entry masks 1, 2, 4", _lib.RAYS_PAD_MASK, with_pad(cycle), entry_bits),
        ]
    out = torch.empty((n * 4, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rows = []
    for cname, flags, rays, masks in cases:
        if masks is not None:
            for i, m in enumerate(masks):
                scene.setEntryMask(i, m)
        for qname, q in QUERIES:
            if q is None or q == "any":
                def call(cnt=None, q=q):
                    ctx._check(scene.traceRaysDevice(rays.data_ptr(), n, out.data_ptr(), any_hit=q == "any", counters=cnt,
                                                     flags=flags))
            else:
                def call(cnt=None, q=q):
                    ctx._check(scene.traceRaysMultiDevice(rays.data_ptr(), n, q, out.data_ptr(), counts.data_ptr(), flags, cnt))
            ms = timed(call)
            cnt = np.zeros(3, np.uint64)
            call(cnt)
            rows.append({"filter": cname, "query": qname, "rays": int(n), "ms": ms, "nodes_per_ray": float(cnt[0]) / n,
                         "tris_per_ray": float(cnt[1]) / n, "hits_per_ray": float(cnt[2]) / n})
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
    iters = int(args[0]) if args else 50
    procs = int(args[1]) if len(args) > 1 else 3
    runs = {lib: [] for lib in libs}
    for _ in range(procs):  # the builds take turns, one fresh process after the other
        for lib in libs:
            env = dict(os.environ)
            if lib:
                env["BEAM_HIP_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(iters)], env=env,
                               capture_output=True, text=True, timeout=600)
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("ROWS ")), None)
            if r.returncode or line is None:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"child failed ({lib or 'this tree'}): exit {r.returncode}")
            runs[lib].append(json.loads(line[5:]))
    report = []
    for lib in libs:
        name = lib or "this tree"
        print(f"\n== {name}: {procs} processes x median of {iters} calls, {GROUPS * PER} rays ==")
        print(f"{'filter':38s} {'query':10s} {'ms median':>10s} {'min .. max':>19s} {'Mrays/s':>8s} {'vs flags=0':>11s} "
              f"{'nodes/ray':>9s} {'tris/ray':>8s} {'hits/ray':>8s}")
        plain = {}
        for i, row in enumerate(runs[lib][0]):
            ms = [r[i]["ms"] for r in runs[lib]]
            med = float(np.median(ms))
            if row["filter"] == "flags = 0":
                plain[row["query"]] = ms
            # the ratio within each process, then its median: both sides saw the same machine
            ratio = [a / b for a, b in zip(ms, plain[row["query"]])]
            print(f"{row['filter']:38s} {row['query']:10s} {med:10.4f} {min(ms):9.4f} .. {max(ms):7.4f} "
                  f"{row['rays'] / med / 1e3:8.1f} {float(np.median(ratio)):11.3f} {row['nodes_per_ray']:9.2f} "
                  f"{row['tris_per_ray']:8.2f} {row['hits_per_ray']:8.3f}")
            report.append(dict(row, lib=name, ms=med, ms_runs=ms, ratio_runs=ratio))
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"iters": iters, "processes": procs, "rows": report}, f, indent=1)


if __name__ == "__main__":
    main()
