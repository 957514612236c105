"""The GPU kernels against frames traced by the reference's OWN code, pixel by pixel (fixtures only).

tests/golden/ref holds what the reference's CPU-emulation path computes (compiled from its sources,
driven through its public API; tests/golden/make_ref_frames.py) on the survey views and on small
designed scenes (tests/ref_scenes.py): exact-t ties, the 256-face cap, the first-hit-leaf early-out,
zero direction components and eyes on split planes, the world box, the camera's ray recurrence,
several meshes. Neither the reference nor its binary is needed here.

Reference mode (bm_kd.hip) must give the reference's packed colour and triangle id on every pixel,
the early-out pixels included, and its tree the reference's own build report. The default mode (LBVH,
closest hit) must give the reference's frame except on the pixels the fixture lists, where the
exhaustive closest hit computed on the CPU (oracle.brute_render) differs from the reference's answer;
there it must give that closest hit. The list is a condition, not a tolerance.

The reference has no output for t: t stays pinned through the glm primitive pin
(tests/test_gpu_glm_pin.py) and the oracle's frames (tests/test_gpu_reference_mode.py).
"""
import numpy as np
import pytest

import ref_scenes
from golden_io import ref_closest_frame, ref_frame, ref_scene
from gpu_util import gpu_build, gpu_frame
from raytracercuda_amd import beam

pytestmark = pytest.mark.gpu

SCENES = ("bunny_256", "suzanne_256", "f16_500", "bunny_sweep_96") + ref_scenes.DESIGNED
COMPACT, PACKET = 12, 14  # bm_internal.h TraceVariant (tests/test_gpu_variants.py)


@pytest.fixture(scope="module")
def fixtures():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ref_scene(name)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def kctx():
    """Reference-mode contexts by march variant (None: the default march), made on first use."""
    made = {}

    def get(march):
        if march not in made:
            made[march] = beam.Context(device=0, reference_kd=True, params={} if march is None else {"kd_march": march})
        return made[march]

    yield get
    for c in made.values():
        c.close()


def _frames(ctx, s, kd_stats=False):
    """Build the fixture's scene once and trace every view: ([(packed, tri_id)], scene statistics)."""
    scene, keep, _ = gpu_build(ctx, s["meshes"])
    out = []
    for eye, orient in s["views"]:
        f = gpu_frame(ctx, scene, s["w"], s["h"], tuple(float(x) for x in s["cam"]), eye, orient)
        out.append((f["packed"], f["tri_id"]))
    kd = scene.kdStats() if kd_stats else None
    scene.destroy()
    del keep
    return out, kd


def _assert_equal(name, k, got, want, what):
    (packed, tri), (rp, rt) = got, want
    bad = np.flatnonzero((tri != rt) | (packed != rp))
    assert bad.size == 0, (f"{name} view {k}: {bad.size} pixels differ from {what}, first {bad[:5]}: ids "
                           f"{tri[bad[:5]]} vs {rt[bad[:5]]}, colours {packed[bad[:5]]} vs {rp[bad[:5]]}")


# every fixture with the default march; the designed scenes also with one-box steps (2) and lane-per-ray leaves (1)
KD_CASES = [(None, n) for n in SCENES] + [(m, n) for m in (2, 1) for n in ref_scenes.DESIGNED]


@pytest.mark.parametrize("march,name", KD_CASES, ids=[f"march{'' if m is None else m}-{n}" for m, n in KD_CASES])
def test_reference_mode_equals_reference_on_every_pixel(kctx, fixtures, march, name):
    """Every fixture view with the default march; the designed scenes also with kd_march 2 and 1. The
    tree: kdStats() == [the reference's printed leaves at MaxDepth (the leaves that hold faces),
    numFaces - `Num faces` lines (references stored), `Num faces` lines (faces dropped by the cap)]."""
    s = fixtures(name)
    frames, kd = _frames(kctx(march), s, kd_stats=True)
    for k, got in enumerate(frames):
        _assert_equal(name, k, got, ref_frame(s, k), "the reference")
    rep = s["build_report"].astype(np.int64)
    dropped = int(rep[:, 4].sum())
    assert [int(x) for x in kd[:3]] == [int(rep[-1, 3]), int(rep[-1, 2]) - dropped, dropped]


@pytest.fixture(scope="module")
def lctx():
    c = beam.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("name", SCENES)
def test_default_mode_equals_reference_outside_the_recorded_closest_hit_set(lctx, fixtures, name):
    """LBVH closest hit == the reference on every pixel outside the fixture's set, == the exhaustive
    closest hit stored beside it inside."""
    s = fixtures(name)
    frames, _ = _frames(lctx, s)
    for k, got in enumerate(frames):
        _assert_equal(name, k, got, ref_closest_frame(s, k), "the reference (closest hit on the recorded set)")


@pytest.mark.parametrize("variant", [PACKET, COMPACT], ids=["packet", "compact"])
def test_default_mode_trace_variants_on_the_early_out_scene(fixtures, variant):
    ctx = beam.Context(device=0, params={"trace_variant": variant})
    try:
        s = fixtures("early_out")
        frames, _ = _frames(ctx, s)
        for k, got in enumerate(frames):
            _assert_equal("early_out", k, got, ref_closest_frame(s, k), "the reference (closest hit on the set)")
    finally:
        ctx.close()
