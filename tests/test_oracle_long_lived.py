"""What the walks of tests/long_lived_scenes.py must put in front of the library, asserted without a GPU from the
oracle's builds and frames and a host restatement of the build's regime predicates.

A walk that rebuilt the same box, or traced the same pixels twice, would pass over state left behind by the call
before: a bound replica that was not cleared changes a key only if the next scene's box is another one, and a
pixel that a kernel forgot to write shows only if the frame before held something else there. So: every regime
is entered from a larger and from a smaller scene; into every regime one step at least halves the box along every
axis, inside the previous one; for that step, and for one step after every regime, the keys computed over the
box a stale replica would leave differ on more than half the triangles; consecutive frames into a target differ
on a quarter of the pixels they write, consecutive shadow planes on 5 %; and a compacted shadow frame culls
pixels that the shadow frame before it left shadowed.
"""
import numpy as np
import pytest

import long_lived_scenes as L
from test_gpu_ray_queue import layout, survivor_bounds

NO_TRI = 0xFFFFFFFF


def test_regime_predicate_and_sizes():
    for r, n in L.SMALLEST.items():
        assert L.regime(n) == r
        assert n == 0 or L.regime(n - 1) != r  # the smallest n inside the regime
    assert [L.regime(n) for n in (512, 16383, 131072, 1 << 19)] == ["chunk", "lsd", "table", "span"]
    for s in L.WALK + L.SHORT_WALK:
        if s.kind == "soup":
            assert s.n == L.SMALLEST[L.regime(s.n)]
    assert sum(s.n > L.MSD_WIDE_N for s in L.WALK) == 1  # the one large build
    # every kernel that clears the bound replicas for the next build ends some step of the walk
    assert set(L.LAST_READER) == set(L.REGIMES) - {"empty"}
    assert {L.LAST_READER[L.regime(s.n)] for s in L.WALK if s.n} == set(L.LAST_READER.values())


def test_every_regime_is_entered_from_both_sides():
    above, below = set(), set()
    for prev, s in zip(L.WALK, L.WALK[1:]):
        (above if prev.n > s.n else below).add(L.regime(s.n))
    # the empty scene has nothing below it; the one step above 2^19 is the largest of the walk
    assert above == set(L.REGIMES) - {"wide"}
    assert below == set(L.REGIMES) - {"empty"}
    refit = {L.regime(s.n) for s in L.WALK if s.refit}
    assert refit == set(L.REGIMES) - {"empty"}
    for walk in (L.WALK, L.SHORT_WALK):
        for prev, s in zip(walk, walk[1:]):
            if s.kind in ("skew", "equal"):
                assert prev.kind == "soup" and prev.n >= L.MSD_MIN_N and prev.scale == 1.0  # a well-spread scene
    assert {s.kind for s in L.WALK} == {"soup", "skew", "equal"}
    assert {L.regime(s.n) for s in L.SHORT_WALK} == {"empty", "one", "two", "chunk", "lsd", "table"}


def halves_inside(prev, meshes):
    """This scene's box at most half the previous one's along every axis and inside it: the vertices' box and
    the box of the triangle centres, over which the keys are quantised."""
    for box in (L.vertex_box, L.centre_box):
        (plo, phi), (lo, hi) = box(prev), box(meshes)
        if not (np.all(hi - lo <= (phi - plo) / 2) and np.all(lo >= plo) and np.all(hi <= phi)):
            return False
    return True


@pytest.mark.parametrize("walk", ["full", "short"])
def test_boxes_shrink_and_keys_change(oracle, walk):
    steps = L.WALKS[walk][0]
    shrunk, left = set(), set()
    for i in range(1, len(steps)):
        prev, meshes = L.final_meshes(walk, i - 1), L.step_meshes(walk, i)
        if not prev or not meshes:
            continue
        own = L.own_keys(oracle, meshes)
        stale = L.stale_keys(oracle, prev, meshes)
        changed = float((own != stale).mean())
        inside = halves_inside(prev, meshes)
        print(f"{walk} step {i}: n {steps[i].n} {L.regime(steps[i].n)} after {L.regime(steps[i - 1].n)}: "
              f"{changed:.3f} of the keys change, box halved inside the previous: {inside}")
        # every build after a non-empty one: a replica left uncleared by the step before changes its keys
        assert changed > 0.5, (i, changed)
        left.add(L.regime(steps[i - 1].n))
        if inside:
            shrunk.add(L.regime(steps[i].n))
    if walk == "full":
        assert shrunk == set(L.REGIMES) - {"empty"}
        assert left == set(L.REGIMES) - {"empty"}
    else:
        assert shrunk >= {"two", "chunk", "lsd"} and left >= {"one", "chunk", "lsd", "table"}


def test_refits_move_the_box():
    """A refit step's second position is a sixteenth of its first along every axis: the second refit's bounds
    are well inside what the first one gathered, and the next build's inside neither."""
    for walk, (steps, _) in L.WALKS.items():
        for i, s in enumerate(steps):
            if not s.refit:
                continue
            m = L.step_meshes(walk, i)
            (alo, ahi), (blo, bhi) = L.vertex_box(L.moved(m, 4.0)), L.vertex_box(L.moved(m, 0.25))
            assert np.all(bhi - blo <= (ahi - alo) / 8) and np.all(blo >= alo) and np.all(bhi <= ahi)


def simulate(oracle, frames):
    """Walk a sequence on the oracle's planes: per step the fraction of the pixels it writes whose tri_id (and
    shadow byte, between shadow steps) differs from what its target held, and for compacted shadow steps the
    culled pixels that were shadowed."""
    held = {}
    out = []
    for fr in frames:
        exp, _ = L.frame_planes(oracle, fr)
        tri = exp["tri_id"].reshape(fr.h, fr.w)
        sh = exp["shadow"].reshape(fr.h, fr.w) if fr.light else None
        if fr.mode == "bands":
            rows = L.band_rows(fr.h, *L.BANDS)
            local = np.concatenate([np.arange(a, a + r.stop - r.start) for a, r in rows])
            glob = np.concatenate([np.arange(r.start, r.stop) for a, r in rows])
        else:
            local = glob = np.arange(fr.h)
        rec = {"tri": None, "shadow": None, "culled_shadowed": None}
        t = held.setdefault(fr.target, {})
        if "tri" in t:
            rec["tri"] = float((t["tri"][local] != tri[glob]).mean())
        else:
            t["tri"] = np.full((fr.h, fr.w), NO_TRI, np.uint32)
        t["tri"][local] = tri[glob]
        if fr.light:
            if "shadow" in t:
                rec["shadow"] = float((t["shadow"][local] != sh[glob]).mean())
                if fr.kind == "cull+quads" and fr.mode != "bands":
                    sure, maybe = survivor_bounds(oracle, fr.scene, fr.w, fr.h, eye=fr.eye, cam=L.WINDOWS[fr.window])
                    rec["culled_shadowed"] = int((~maybe & (t["shadow"] == 1)).sum())
            else:
                t["shadow"] = np.zeros((fr.h, fr.w), np.uint8)
            t["shadow"][local] = sh[glob]
        out.append(rec)
    return out


def test_sequence_visits_every_kind_twice():
    seq = L.SEQUENCE

    def visits(pred):
        at = [i for i, fr in enumerate(seq) if pred(fr)]
        return len(at) >= 2 and any(b - a > 1 for a, b in zip(at, at[1:]))  # twice, not in a block

    assert visits(lambda f: f.kind == "quads" and f.sched == 1)
    assert visits(lambda f: f.kind == "quads" and f.sched == 2)
    assert visits(lambda f: f.kind == "cull+quads")
    assert visits(lambda f: f.kind == "packets" and f.variant == L.PACKET and f.mode == "trace" and not f.light)
    assert visits(lambda f: f.kind == "lanes" and f.variant == L.LANES)
    assert visits(lambda f: f.light is not None and f.kind != "lanes")  # fused shadows
    assert visits(lambda f: f.mode == "count")
    assert visits(lambda f: f.mode == "bands")
    assert visits(lambda f: f.cost is not None)
    assert {f.cost for f in seq} == {None, "descending", "constant"}
    # the ray queue's layout changes on one buffer: 4, then 36, then 4 tiles per region
    tiles = [f.tiles for f in seq if f.kind == "cull+quads" and f.mode == "trace"]
    assert tiles[:3] == [4, 36, 4]
    assert layout(L.W, L.H, 4) == (39, 4) and layout(L.W, L.H, 36) == (5, 36)
    # a full frame follows every band frame into the same target; the window and the size change mid-sequence
    for i, f in enumerate(seq):
        if f.mode == "bands":
            assert seq[i + 1].mode != "bands" and seq[i + 1].target == f.target
            assert sum(r.stop - r.start for _, r in L.band_rows(f.h, *L.BANDS)) < f.h
    assert [f.window for f in seq].count("other") >= 2 and seq[-1].window == "square"
    small = [i for i, f in enumerate(seq) if f.target == "small"]
    assert small and 0 < small[0] < len(seq) - 1 and all((f.w, f.h) == (64, 64) for f in seq if f.target == "small")


@pytest.mark.parametrize("name", ["sequence", "queue"])
def test_consecutive_frames_differ(oracle, name):
    frames = L.SEQUENCE if name == "sequence" else L.QUEUE_SEQUENCE
    recs = simulate(oracle, frames)
    for i, (fr, r) in enumerate(zip(frames, recs)):
        print(f"{name} step {i}: {fr.scene} {fr.kind} {fr.mode}: {r}")
    for i, (fr, r) in enumerate(zip(frames, recs)):
        assert r["tri"] is None or r["tri"] >= 0.25, (i, r)
        assert r["shadow"] is None or r["shadow"] >= 0.05, (i, r)
    assert sum(r["shadow"] is not None for r in recs) >= (3 if name == "sequence" else 1)
    if name == "sequence":
        # k_cull's shadow = 0 store: culled pixels that the shadow step before left shadowed
        assert max(r["culled_shadowed"] or 0 for r in recs) >= 64
        # every hit pixel of the dense views is lit or shadowed by its own geometry, none by the sentinel
        for fr in frames:
            exp, _ = L.frame_planes(oracle, fr)
            assert not (exp["packed"] == L.SENTINEL).any()


def test_frames_in_flight_differ(oracle):
    from test_gpu_ray_queue import SCENES, expected
    from test_gpu_variants import expect
    from raytracercuda_amd import scenes

    for k in range(3):
        d, _ = expected(oracle, "dense", L.W, L.H, eye=L.FLIGHT_EYES["dense"][k])
        w, _ = expected(oracle, "wire", L.W, L.H, eye=L.FLIGHT_EYES["wire"][k])
        m, _ = expect(oracle, L.dense_moved(), L.W, L.H, scenes.RAYS_SQUARE, L.FLIGHT_EYES["dense"][k], scenes.IDENTITY)
        assert (d["tri_id"] != w["tri_id"]).mean() >= 0.25 and (m["tri_id"] != w["tri_id"]).mean() >= 0.25
        # the refit shows: a quarter of the pixels change their t
        assert (d["t"].view(np.uint32) != m["t"].view(np.uint32)).mean() >= 0.25
    assert L.flight_scene(6) == "dense" and L.flight_scene(L.FLIGHT_FRAMES) == "dense"
    assert len(SCENES["dense"]) == 1
