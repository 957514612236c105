#!/usr/bin/env python3
"""Box overlap query throughput (bm_scene_overlap_boxes) on the C3 scene.

    python tools/boxes_bench.py [iters] [processes] [--json PATH]

Voxel grids over the scene's bounding box (IScene.voxelize's cells, made on the device):
  64^3 and 256^3 cells in BM_BOXES_ANY and BM_BOXES_COUNT;
  a BM_BOXES_LIST pass over 64^3 with the exclusive prefix sum of its counts as offsets;
  one box that holds the whole scene (BM_BOXES_COUNT): the price of the worst single box, one quad walking
  every record (the median of 5 timings after 2 warm-up calls: it is long).
Each figure is the median of `iters` (30) HIP-event timings on the library's stream after 10 warm-up calls, with
boxes per second and, from the counting build, node records, triangle tests and ids per box. The measurement
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

GRIDS = (64, 256)


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
    pos = np.concatenate([np.asarray(m["pos"], np.float32).reshape(-1, 3) for m in meshes])
    lo, hi = pos.min(0), pos.max(0)

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

    def grid(d):  # voxelize's cells
        cell = (hi - lo) / np.float32(d)
        boxes = torch.zeros((d, d, d, 8), dtype=torch.float32, device=dev)
        for a in range(3):
            shape = [1, 1, 1]
            shape[a] = d
            axis = float(lo[a]) + (torch.arange(d, dtype=torch.float32, device=dev) + 0.5) * float(cell[a])
            boxes[..., a] = axis.view(shape)
            boxes[..., 4 + a] = float(np.float32(0.5) * cell[a])
        return boxes.view(-1, 8)

    rows = []

    def run(name, boxes, mode, out, off=0, ids=0, **how):
        n = boxes.shape[0]
        cnt = np.zeros(4, np.uint64)
        ctx._check(scene.overlapBoxesDevice(boxes.data_ptr(), n, mode, out, off, ids, 0, cnt))
        ms = timed(lambda: ctx._check(scene.overlapBoxesDevice(boxes.data_ptr(), n, mode, out, off, ids)), **how)
        rows.append({"query": name, "boxes": n, "ms": ms, "nodes_per_box": int(cnt[0]) / n, "tests_per_box": int(cnt[1]) / n,
                     "ids_per_box": int(cnt[2]) / n, "deepest_stack": int(cnt[3])})

    for d in GRIDS:
        boxes = grid(d)
        n = boxes.shape[0]
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        flag = torch.empty((n,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        run(f"{d}^3 any", boxes, _lib.BOXES_ANY, flag.data_ptr())
        run(f"{d}^3 count", boxes, _lib.BOXES_COUNT, count.data_ptr())
        if d == GRIDS[0]:
            offsets = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
            torch.cumsum(count, 0, dtype=torch.int32, out=offsets[1:])
            ids = torch.empty((max(int(offsets[-1].item()), 1),), dtype=torch.int32, device=dev)
            run(f"{d}^3 list", boxes, _lib.BOXES_LIST, 0, offsets.data_ptr(), ids.data_ptr())
        del boxes, count, flag
    whole = torch.zeros((1, 8), dtype=torch.float32, device=dev)
    whole[0, 0:3] = torch.from_numpy((lo + hi) * np.float32(0.5)).to(dev)
    whole[0, 4:7] = torch.from_numpy((hi - lo) * np.float32(0.5) + np.float32(1)).to(dev)
    one = torch.empty((1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    run("one scene-sized box", whole, _lib.BOXES_COUNT, one.data_ptr(), warm=2, reps=5)
    assert int(one.item()) == int(ntri)
    scene.destroy()
    del keep
    ctx.close()
    print("BOXES_BENCH " + json.dumps({"num_tris": int(ntri), "iters": iters, "rows": rows}), flush=True)


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
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("BOXES_BENCH ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"process {k} failed with exit status {r.returncode}")
        runs.append(json.loads(line[0][len("BOXES_BENCH "):]))
        for row in runs[-1]["rows"]:
            print(f"process {k}: {row['query']:20s} {row['ms'] * 1e3:10.1f} us  {row['nodes_per_box']:8.2f} nodes "
                  f"{row['tests_per_box']:8.2f} tests {row['ids_per_box']:8.3f} ids per box  deepest stack "
                  f"{row['deepest_stack']:3d}", flush=True)
    summary = []
    for i, row in enumerate(runs[0]["rows"]):
        ms = [r["rows"][i]["ms"] for r in runs]
        med = float(np.median(ms))
        summary.append({"query": row["query"], "boxes": row["boxes"], "ms": med, "ms_range": [min(ms), max(ms)],
                        "mboxes_per_s": row["boxes"] / med * 1e-3, "nodes_per_box": row["nodes_per_box"],
                        "tests_per_box": row["tests_per_box"], "ids_per_box": row["ids_per_box"]})
        print(f"median of {procs}: {row['query']:20s} {med * 1e3:10.1f} us ({min(ms) * 1e3:.1f}-{max(ms) * 1e3:.1f})  "
              f"{summary[-1]['mboxes_per_s']:9.2f} Mboxes/s  {row['nodes_per_box']:.2f} nodes "
              f"{row['tests_per_box']:.2f} tests {row['ids_per_box']:.3f} ids per box", flush=True)
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, "w") as f:
            json.dump({"num_tris": runs[0]["num_tris"], "iters": iters, "processes": procs, "summary": summary,
                       "runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
