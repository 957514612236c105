#!/usr/bin/env python3
"""Ray-queue size of the compacted trace per bench config and cull depth: the rays that survive k_cull
(the sum of rayq_count, read back with bm_rt_ray_queue_counts) and the 16-ray batches k_trace_rays
walks, with BM_PARAM_CULL_DEPTH 1 and 2, as the frames-in-flight path traces the config (a target on
its own stream; configs whose view is not sparse take another kernel and are reported as such).

    python tools/cull_counts.py [c2,c3,c5]
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raytracercuda_amd import beam, scenes  # noqa: E402

names = (sys.argv[1] if len(sys.argv) > 1 else "c2,c3,c5").split(",")
for name in names:
    cfg = scenes.CONFIGS[name]
    meshes = scenes.scene(cfg["scene"])
    row = {"config": name, "scene": cfg["scene"], "rays": cfg["width"] * cfg["height"]}
    for depth in (1, 2):
        ctx = beam.Context(device=0, params={"cull_depth": depth})
        scene = beam.IScene.create(ctx)
        keep = beam.upload_meshes(ctx, scene, meshes)
        scene.updateGPUScene()
        cam = beam.ICamera.create(ctx)
        ctx._check(cam.setInitialRays(cfg["width"], cfg["height"], *cfg["rays"]))
        rt = beam.IRenderTarget.createOffscreen(ctx, cfg["width"], cfg["height"])
        stream = torch.cuda.Stream()
        rt.setStream(stream.cuda_stream)
        if cfg["light"]:
            ctx._check(cam.traceShadow(cfg["eye"], scenes.IDENTITY, scene, rt, cfg["light"]))
        else:
            ctx._check(cam.trace(cfg["eye"], scenes.IDENTITY, scene, rt))
        ctx.sync()
        row["kind"] = rt.traceKind()
        if row["kind"] == "cull+quads":
            counts = rt.rayQueueCounts()
            hits = int((rt.read(packed=False, t=False)["tri_id"] != 0xFFFFFFFF).sum())
            row[f"depth{depth}"] = {"survivors": int(counts.sum()), "batches": int((int(counts.sum()) + 15) // 16),
                                    "regions": int(counts.size), "largest_region": int(counts.max()), "hits": hits}
        rt.destroy()
        cam.destroy()
        scene.destroy()
        del keep
        ctx.close()
    print(json.dumps(row))
