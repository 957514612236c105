"""The oracle's BVH trace against its exhaustive trace over the range grid of tests/range_scenes.py, without
a GPU: far eyes, large world offsets, tiny and huge scales, four eye directions, BVH4 and BVH2.

The GPU tests compare kernels with the oracle's BVH trace; this file checks that trace where nobody had:
  * inside the envelope (any offset, scales 2^-30 .. 2^30, the eye within D_OK scene extents) it equals
    brute force on every pixel: ids, packed colours, t bits and the shadow plane;
  * D_OK is the largest such distance of the grid: at the next one some pixel differs;
  * outside (D > D_OK) nothing is asserted about equality; the counts are printed (DESIGN.md §2 has them);
  * no frame is trivially equal: a quarter of the pixels hit, a tenth miss, and lit and shadowed pixels
    both occur among the hits;
  * at every scale a pixel carries a triangle id exactly when its t is finite and positive, for the BVH as
    for brute force (a candidate whose t overflowed to +inf used to win the tie against "no hit yet"), and
    above 2^30, where triangle tests overflow, the BVH frame still equals the exhaustive one.

Lit and shadowed pixels: the cube is convex, so each of its faces is lit or shadowed as a whole. Three of the
four directions show a lit and a shadowed face. The "axial" one shows a single, lit face, so no light can put
both values into that view of the cube (a few border pixels apart, where a side face's triangle ties for the
hit): it is the one (scene, direction) pair left out of that assertion. The soup and suzanne carry both
values from every direction.
"""
import numpy as np
import pytest

import range_scenes as rs

WIDTHS = (4, 2)
NAN_OCCLUDERS_FROM = 44  # the scale 2^k from which the exhaustive shadow plane carries NaN-made occluders
CASES = [(s, v) for s in rs.SCENES for v in rs.views_of(s)]
IDS = [f"{s}-{v.id}" for s, v in CASES]


@pytest.fixture(scope="module")
def brute(oracle):
    rs.warm(oracle, CASES, WIDTHS)
    yield lambda s, v: rs.brute_expected(oracle, s, v)
    rs.clear()


def subset(keep):
    return {"argvalues": [c for c in CASES if keep(c[1])], "ids": [i for i, c in zip(IDS, CASES) if keep(c[1])]}


@pytest.mark.parametrize("case", **subset(rs.inside))
def test_inside_the_envelope_the_bvh_equals_brute_force(oracle, brute, case):
    scene, v = case
    b = brute(scene, v)
    for width in WIDTHS:
        diff = rs.compare(rs.bvh_expected(oracle, scene, v, width).frame, b)
        assert not any(diff.values()), f"BVH{width}: pixels that differ from brute force: {diff}"


def far_table(oracle, brute, D):
    """{scene: differing ids / lost hits / differing t / differing shadow bytes} at eye distance D, summed
    over the four directions and both widths."""
    out = {}
    for scene in rs.SCENES:
        tot = {"ids": 0, "lost": 0, "t": 0, "shadow": 0}
        views = [v for v in rs.views_of(scene) if v.D == D and not v.T and not v.s_exp]
        if not views:
            continue
        for v in views:
            for width in WIDTHS:
                d = rs.compare(rs.bvh_expected(oracle, scene, v, width).frame, brute(scene, v))
                for k in tot:
                    tot[k] += d[k]
        out[scene] = tot
    return out


def test_the_library_takes_its_envelope_from_the_measured_d_ok():
    """BM_ENVELOPE_EXTENTS (include/beam_c.h) decides where wave packets may run: it is D_OK."""
    import os
    import re
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "beam_c.h")
    with open(header) as f:
        m = re.search(r"^#define BM_ENVELOPE_EXTENTS (\d+)$", f.read(), re.M)
    assert m and int(m.group(1)) == rs.D_OK


def test_d_ok_is_the_largest_distance_of_the_grid_that_is_exact(oracle, brute):
    """Equality up to D_OK is the test above; here: the next distance of the grid is not exact, so D_OK is
    measured and not merely safe."""
    assert rs.D_OK in rs.D_GRID
    nxt = rs.D_GRID[rs.D_GRID.index(rs.D_OK) + 1]
    tab = far_table(oracle, brute, nxt)
    print(f"D = {nxt}: {tab}")
    assert sum(sum(t.values()) for t in tab.values()) > 0, f"D = {nxt} is exact too: raise D_OK"


def test_outside_the_envelope_is_reported_not_asserted(oracle, brute):
    """Printed, not asserted: per (scene, D > D_OK) the pixels of 4 directions x 2 widths x 192^2 on which the
    BVH differs from brute force."""
    for D in rs.D_GRID:
        if D > rs.D_OK:
            for scene, t in far_table(oracle, brute, D).items():
                print(f"D = {D:6d} {scene:8s} ids {t['ids']:6d}  lost {t['lost']:6d}  t {t['t']:6d}  shadow {t['shadow']:6d}")


@pytest.mark.parametrize("case", **subset(lambda v: rs.S_OK[0] <= v.s_exp <= rs.S_OK[1]))
def test_no_view_is_trivially_equal(brute, case):
    scene, v = case
    b = brute(scene, v)
    hit = b["tri_id"] != rs.MISS
    share = float(hit.mean())
    print(f"{scene}-{v.id}: hit share {share:.3f}, {int(b['shadow'][hit].sum())} of {int(hit.sum())} hits shadowed")
    assert share >= 0.25 and 1.0 - share >= 0.10, share
    assert np.unique(b["tri_id"][hit]).size >= 50
    if rs.inside(v):
        if not (scene == "cube" and v.dir == "axial"):  # one lit face: see the module docstring
            assert np.unique(b["shadow"][hit]).size == 2, "the hit pixels are all lit or all shadowed"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_triangle_id_means_a_finite_t(oracle, brute, case):
    scene, v = case
    assert rs.hit_is_finite_t(brute(scene, v)), "brute force"
    for width in WIDTHS:
        f = rs.bvh_expected(oracle, scene, v, width).frame
        bad = int(((f["tri_id"] != rs.MISS) & ~np.isfinite(f["t"])).sum())
        assert rs.hit_is_finite_t(f), f"BVH{width}: {bad} pixels carry a triangle id and a non-finite t"


@pytest.mark.parametrize("case", **subset(lambda v: v.s_exp > rs.S_OK[1]))
def test_above_the_envelope_s_scales_still_equal_brute_force(oracle, brute, case):
    """Where products of coordinates overflow, the triangle tests of both sides fail alike and no box test
    loses a hit that brute force keeps: ids, colours and t are equal up to 2^60, the shadow plane up to 2^42.

    From 2^44 on the exhaustive shadow plane has more shadowed pixels than the BVH's, and they are its own
    artefacts: a shadow ray's direction is the unnormalised segment to the light (2^46 long there), so for
    triangles away from the ray the sums behind u and v reach inf - inf = NaN, the triangle test's rejects
    (u < 0 || u > 1, v < 0 || u + v > 1, as in the reference) let NaN pass, and a t in (0, 1) then makes an
    occluder of a triangle whose box the ray never enters. There the test asserts that the BVH shadows no
    pixel that brute force leaves lit, and prints the count of the others."""
    scene, v = case
    b = brute(scene, v)
    for width in WIDTHS:
        f = rs.bvh_expected(oracle, scene, v, width).frame
        diff = rs.compare(f, b)
        if v.s_exp >= NAN_OCCLUDERS_FROM:
            extra = int(((f["shadow"] == 1) & (b["shadow"] == 0)).sum())
            print(f"{scene}-{v.id} BVH{width}: brute force shadows {diff['shadow'] - extra} pixels more")
            assert extra == 0, f"BVH{width} shadows {extra} pixels that brute force leaves lit"
            diff["shadow"] = 0
        assert not any(diff.values()), f"BVH{width}: pixels that differ from brute force: {diff}"


def test_some_huge_view_mixes_finite_hits_and_overflowing_triangles(oracle, brute):
    mixed = []
    for scene, v in CASES:
        if v.s_exp >= 40:
            hits = int((brute(scene, v)["tri_id"] != rs.MISS).sum())
            over, of = rs.overflowing(oracle, scene, v)
            print(f"{scene}-{v.id}: {hits} finite hits; {over} of the {of} hits of S = 1 now give a non-finite t")
            if hits and over:
                mixed.append((scene, v.id))
    assert mixed, "no view with S >= 2^40 has finite hits next to overflowing triangles: add powers of two"
