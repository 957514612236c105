#!/usr/bin/env python3
"""Ray-query throughput (bm_scene_trace_rays) on the C3 scene, against the camera trace of the same rays.

    python tools/rays_bench.py [iters] [repeats] [--json PATH]

One process, one GPU visit; every figure is a median of `iters` HIP-event timings on the library's
stream (torch's current stream handed to the context) after 10 warm-up calls, as tools/ab_trace.py
measures; the incoherent workloads are measured `repeats` times and the spread of those medians is
printed beside them.

(a) coherent: the camera's own 1920x1080 primary rays as a batch, in row-major order and in the order
    of 4x4 pixel tiles (a wave's 16 rays then are the quad kernel's tile), closest mode, against
    bm_camera_trace with the quad kernel (wave packets off).
(b) incoherent, generated with torch on the device from the primary hits (fixed seed): one
    cosine-weighted bounce ray per hit (closest mode) and one segment per hit to a random point of a
    sphere of radius ext (the scene box's diagonal) around the scene (any-hit mode), in the order of the
    hits and in a random order.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080


def main():
    import torch

    from oracle import Oracle
    from raytracercuda_amd import beam, scenes
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    iters = int(args[0]) if args else 30
    repeats = int(args[1]) if len(args) > 1 else 5
    out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ctx = beam.Context(device=0, stream=stream.cuda_stream, params={"trace_auto_packet": 0})
    meshes = scenes.scene("armadillo_proxy")
    scene = beam.IScene.create(ctx)
    keep = beam.upload_meshes(ctx, scene, meshes)
    scene.updateGPUScene()
    cam = beam.ICamera.create(ctx)
    ctx._check(cam.setInitialRays(W, H, *scenes.RAYS_1080))
    rt = beam.IRenderTarget.createOffscreen(ctx, W, H)
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

    rows = []
    out_hits = torch.empty((W * H, 4), dtype=torch.float32, device=dev)
    out_occ = torch.empty((W * H,), dtype=torch.uint8, device=dev)

    def query(r, any_hit=False):  # the bare entry point: results into preallocated buffers
        ctx._check(scene.traceRaysDevice(r.data_ptr(), r.shape[0], (out_occ if any_hit else out_hits).data_ptr(),
                                         any_hit))

    def report(name, n, ms, note=""):
        rows.append({"workload": name, "rays": int(n), "ms": ms, "grays_per_s": n / ms * 1e-6, "note": note})
        print(f"{name:44s} {n:9d} rays {ms * 1e3:9.1f} us {n / ms * 1e-6:7.3f} Grays/s  {note}", flush=True)

    # ---- (a) the camera's rays ------------------------------------------------------------------
    cam_ms = timed(lambda: ctx._check(cam.trace(eye, scenes.IDENTITY, scene, rt)))
    frame = rt.read()
    report("camera trace (quad kernel, " + rt.traceKind() + ")", W * H, cam_ms, "baseline")
    err, table = Oracle().camera_rays(W, H, *scenes.RAYS_1080)
    assert err == 0
    packed = np.zeros((W * H, 8), np.float32)
    packed[:, 0:3], packed[:, 3], packed[:, 4:7] = eye, np.inf, table
    y, x = np.divmod(np.arange(W * H), W)
    tile_order = np.lexsort((x % 4, y % 4, x // 4, y // 4))  # 4x4 tiles, row-major inside and across
    orders = {"row-major": np.arange(W * H), "4x4 tiles": tile_order}
    prim = None
    for oname, order in orders.items():
        rays = torch.from_numpy(packed[order]).to(dev)
        res = scene.traceRays(rays)
        torch.cuda.synchronize()
        tri = res["tri_id"].cpu().numpy().view(np.uint32)
        diff = int((tri != frame["tri_id"].reshape(-1)[order]).sum())
        ms = timed(lambda: query(rays))
        report(f"(a) primary rays as a batch, {oname}", W * H, ms, f"{ms / cam_ms:.2f}x the camera trace; "
               f"{diff} ids differ from its frame")
        if oname == "4x4 tiles":
            prim = (rays, res["hits"].clone())
        cnt = scene.traceRays(rays, counters=True)["counters"]
        print(f"    counters {oname}: nodes {int(cnt[0])} tris {int(cnt[1])} hits {int(cnt[2])}", flush=True)
    print(f"    counters camera trace: {list(map(int, cam.traceCounters(eye, scenes.IDENTITY, scene, rt)))}", flush=True)

    # ---- (b) one bounce ray and one segment per primary hit --------------------------------------
    rays, hits = prim
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    verts = torch.from_numpy(np.concatenate([m["pos"][np.asarray(m["idx"]).reshape(-1, 3).astype(np.int64)]
                                             for m in meshes]).astype(np.float32)).to(dev)
    ids = hits.view(torch.int32)[:, 3]
    sel = torch.nonzero(ids >= 0).reshape(-1)
    d0 = rays[sel, 4:7]
    p = rays[sel, 0:3] + d0 * (hits[sel, 0] * 0.9999)[:, None]
    tv = verts[ids[sel].long()]
    nrm = torch.linalg.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    nrm = nrm / torch.linalg.norm(nrm, dim=1, keepdim=True)
    nrm = torch.where((nrm * d0).sum(1, keepdim=True) > 0, -nrm, nrm)  # facing the incoming ray
    n = sel.numel()
    r1 = torch.rand(n, generator=gen, device=dev)
    r2 = torch.rand(n, generator=gen, device=dev) * (2 * np.pi)
    helper = torch.where(nrm[:, 0:1].abs() < 0.9, torch.tensor([1.0, 0.0, 0.0], device=dev),
                         torch.tensor([0.0, 1.0, 0.0], device=dev))
    tx = torch.linalg.cross(helper, nrm)
    tx = tx / torch.linalg.norm(tx, dim=1, keepdim=True)
    ty = torch.linalg.cross(nrm, tx)
    rad = torch.sqrt(r1)
    bounce_d = (tx * (rad * torch.cos(r2))[:, None] + ty * (rad * torch.sin(r2))[:, None] +
                nrm * torch.sqrt(1 - r1)[:, None])
    pos = np.concatenate([m["pos"] for m in meshes]).astype(np.float64)
    lo, hi = pos.min(0), pos.max(0)
    centre = torch.tensor((lo + hi) / 2, dtype=torch.float32, device=dev)
    ext = float(np.linalg.norm(hi - lo))
    sph = torch.randn((n, 3), generator=gen, device=dev)
    sph = centre + ext * sph / torch.linalg.norm(sph, dim=1, keepdim=True)

    def pack(o, d):
        r = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        r[:, 0:3], r[:, 3], r[:, 4:7] = o, float("inf"), d
        return r

    shuffle = torch.randperm(n, generator=gen, device=dev)
    work = {"(b) bounce rays, closest, hit order": (pack(p, bounce_d), False),
            "(b) segments to the sphere, any hit, hit order": (pack(p, sph - p), True),
            "(b') bounce rays, closest, random order": (pack(p, bounce_d)[shuffle].contiguous(), False),
            "(b') segments, any hit, random order": (pack(p, sph - p)[shuffle].contiguous(), True)}
    for name, (r, any_hit) in work.items():
        a = scene.traceRays(r, any_hit=any_hit)
        torch.cuda.synchronize()
        frac = float((a["occluded"] != 0).float().mean()) if any_hit else float((a["tri_id"] >= 0).float().mean())
        runs = [timed(lambda: query(r, any_hit)) for _ in range(repeats)]
        report(name, n, float(np.median(runs)), f"medians of {repeats} runs spread {min(runs) * 1e3:.1f}-"
               f"{max(runs) * 1e3:.1f} us; {'occluded' if any_hit else 'hit'} fraction {frac:.3f}")
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump({"iters": iters, "repeats": repeats, "rows": rows}, f, indent=1)
    rt.destroy()
    cam.destroy()
    scene.destroy()
    del keep
    ctx.close()


if __name__ == "__main__":
    main()
