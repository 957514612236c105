"""The build's radix sort (csrc/bm_sort.h, launch_build) on scenes whose Morton keys are dictated key by key.

tests/test_gpu_build_sizes.py walks the sort's regimes in n, on uniform soups or copies of one triangle: the
1,024 top-digit buckets then hold about n / 1024 keys each, or one holds all. The cases here (tests/key_scenes.py)
put chosen numbers of chosen keys at chosen input positions, so that the branches that depend on a bucket's
size, on a digit's histogram or on which tile holds which digit are run at the values where they decide
something. tests/test_oracle_sort_keys.py asserts, without a GPU, that every case has the histogram it is
named after, and that the oracle orders it as numpy's stable sort does.

Every case builds in a fresh context with the case's parameters and asserts
  * num_tris and sort_path as the case states them (a threshold that moved in the code shows here);
  * exported keys and permutation equal numpy's stable sort of the designed keys;
  * records, triangle records, keys and permutation equal the oracle's (compare of test_gpu_build_sizes).
No kernel is mutated to show that a case bites; each docstring names the lines the case guards.
"""
import numpy as np
import pytest

import key_scenes as ks
from gpu_util import assert_frame_equal, gpu_build, gpu_frame, oracle_frame
from raytracercuda_amd import beam, scenes
from test_gpu_build_sizes import compare, soup

pytestmark = pytest.mark.gpu


def names(prefix):
    return sorted(n for n in ks.CASES if n.startswith(prefix))


def build_and_check(oracle, name):
    keys, e = ks.case(name)
    meshes, full = ks.scene_from_keys(keys)
    ctx = beam.Context(device=0, params=e["params"])
    try:
        scene, keep, stats = gpu_build(ctx, meshes)
        assert stats["num_tris"] == e["n"]
        assert stats["sort_path"] == getattr(beam, e["sort_path"])
        rec, tris, gkeys, gperm = scene.export()
        skeys, perm = ks.expected_order(full)
        assert np.array_equal(gkeys, skeys)
        assert np.array_equal(gperm, perm), f"{int((gperm != perm).sum())} positions differ from the stable order"
        compare(rec, tris, gkeys, gperm, oracle.bvh_build(meshes, 4, 4))
        scene.destroy()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", names("a-") + names("b-"))
def test_items_per_lane_of_the_bucket_sort(oracle, name):
    """k_bucket_sort<256> (a) and <1024> (b, msd_wide_n lowered): buckets of k * BS_BLOCK - 1, k * BS_BLOCK and
    k * BS_BLOCK + 1 keys, up to BS_CAP = 8 * BS_BLOCK exactly. Guards ie = ceil(c / BS_BLOCK) and every
    `it >= ie` / `i < c` bound of the load, rank (bs_rank), LDS scatter and store loops: one key short of,
    on and past a full row of lanes, and the last index of L.k / L.v. The low 20 bits cycle through random,
    all equal, descending in input order, two alternating values, one lower digit constant, and digits 0 and
    1023 in both lower passes: stability inside a bucket (wave-local rank plus bs_bases' wave bases) and the
    first and last digit of the scans. The -skew cases add one bucket of BS_CAP + 1 keys, the first that must
    not reach the LDS arrays: `c >= skew_cap` in k_onesweep_wide and in bucket_plan, and PLAN_FLAG in
    k_bucket_sort (SORT_MSD_SKEW; off by one the wrong way it would report SORT_MSD)."""
    build_and_check(oracle, name)


@pytest.mark.parametrize("name", names("c-"))
def test_cap_inside_the_lds_arrays(oracle, name):
    """bucket_lds_cap = 300: sixty buckets of 290..300 keys sort in LDS (SORT_MSD), and with one of them
    at 301 the same scene takes the LSD fallback (SORT_MSD_SKEW). Guards skew_cap = cap + 1 in launch_build
    and the `>=` of both device-side tests at a cap that is not the kernel's capacity."""
    build_and_check(oracle, name)


def test_size_classes_of_the_bucket_plan(oracle):
    """bucket_plan: bucket sizes in 22 of the 127 classes of 64 keys, on both sides of class 63 (the
    second wave of the class scan, `cls >= 64 ? wsum[0] : 0`), the clamped class of c >= 8,064, buckets of
    0, 1 and 2 keys (the single-key/empty class is ordered last and skipped by `d == ~0u`), each edge size
    in two digits of different waves (the per-wave class counts), sizes not monotone in the digit. A wrong
    plan position drops or repeats a bucket in PLAN_ORDER: that bucket stays unsorted or another is missed.
    4-key tiles of the top-digit pass, 1,024-lane bucket workgroups."""
    build_and_check(oracle, "d-classes")


@pytest.mark.parametrize("name", names("e-"))
def test_one_pass_with_a_shared_digit(oracle, name):
    """Digit p of every designed key is one value while the other two digits vary. "const": n - 2 keys share
    it (the anchors hold 0 and 1023); "butone": n - 1 keys share digit 0 with the first anchor, g == n - 1,
    the nearest a scene comes to ow_tile's identity shortcut (`g == n`) without taking it. No scene can make
    one pass constant and another not: an axis with an extent quantises to 0 and to 1023 (key_scenes), so
    g == n in one pass means all keys equal, which test_build_constant_digits covers. Guards the `==` of
    that shortcut (a `>= n - 1` or a per-tile test would copy unsorted keys through), the one-digit
    histograms in the look-back (one digit carries every tile's whole count) and, for p = 2 under default
    parameters, a bucket of n - 2 or n - 1 keys: the fallback whose last pass k_bucket_sort runs with on_tile.
    plain: n = 5,000 (three plain passes); lsd: msd_max_n = 0; msd: default parameters, where p = 0 and 1
    give every bucket workgroup a pass with one digit."""
    build_and_check(oracle, name)


@pytest.mark.parametrize("name", names("f-"))
def test_plain_lsd_passes_on_varied_keys(oracle, name):
    """msd_max_n = 0 with random keys (2 % copies, both extremes): launch_build's pass loop (C = false, the
    ping-pong of keys/vals) ranks 1-, 4- and 8-key-per-lane tiles of k_onesweep_wide above 2^14 keys, which
    the suite ran on constant keys only. Guards ow_rank's item loops (`w * 64 * ITEMS + it * 64 + lane`),
    the digit-ordered tile in LDS over wc (2 * OS_BLOCK * ITEMS words) and its runs of output slots."""
    build_and_check(oracle, name)


@pytest.mark.parametrize("name", names("g-"))
def test_digits_absent_from_the_middle_tiles(oracle, name):
    """n = 40 * 1024 + 1: 41 tiles in the first pass run (the top digit under default parameters, the low digit
    with msd_max_n = 0), more than one OS_LB_WIN window. The digit values 512..1023 occur in tile 0, in tile 39
    and in tile 40 (the last anchor alone) and nowhere else; 0..511 occur in tiles 1..39 (and once in tile 0,
    the first anchor). What this makes certain: the 38 tiles 1..38 each publish LB_AGG | 0 for half of the
    digits, so tiles 39 and 40 sum flagged zeros across two windows until they meet a prefix, and a look-back
    that took a flagged zero for an unpublished word (`y == 0u` tested after masking the flag) would never
    end; tiles 39 and 40 publish flagged zeros for most or all of the other half. How far a tile really walks
    back depends on when its predecessors publish their inclusive prefixes: that is timing, and the test
    cannot force a long walk."""
    build_and_check(oracle, name)


H_N, H_W, H_H, H_EYE = 20000, 96, 64, (0.0, 0.0, -1.05)  # just outside the soup: 1,474 triangles of ~220 meshes seen


@pytest.fixture(scope="module")
def table_soup(oracle):
    mesh = soup(H_N, seed=257)[0]
    packed, tri, t = oracle_frame(oracle, [mesh], H_W, H_H, scenes.RAYS_SQUARE, H_EYE, scenes.IDENTITY)
    assert 0.1 < (tri != 0xFFFFFFFF).mean() and np.unique(tri).size > 500  # no degenerate frame
    for a in (packed, tri, t):
        a.setflags(write=False)
    return mesh, (packed, tri, t)


@pytest.mark.parametrize("parts", [ks.CODE["RJ_LDS_MESHES"], ks.CODE["RJ_LDS_MESHES"] + 1])
def test_mesh_table_of_the_deferred_records(oracle, table_soup, parts):
    """gather_records (the records and corner normals gathered beside the top-digit pass, n >= 2^14): 20,000
    triangles in 256 meshes, the last table copied to LDS, and in 257, the first searched in global memory
    (`j.nm <= RJ_LDS_MESHES`, the copy loop and the static_assert's room after the staging area); unequal
    sizes, the first, a middle and the last mesh empty (equal tri_offsets: the search must take the last).
    A wrong mesh gives wrong corner normals, so wrong packed colours in the frame, and wrong original-order
    records, from which the root of a two-device context reshades every plane."""
    mesh, (packed, tri, t) = table_soup
    meshes = ks.split_meshes(mesh, ks.mesh_counts(H_N, parts, seed=parts))
    assert len(meshes) == parts
    ctx = beam.Context(device=0)
    scene, keep, stats = gpu_build(ctx, meshes)
    assert stats["num_tris"] == H_N and stats["sort_path"] == beam.SORT_MSD
    compare(*scene.export(), oracle.bvh_build(meshes, 4, 4))
    one = gpu_frame(ctx, scene, H_W, H_H, scenes.RAYS_SQUARE, H_EYE, scenes.IDENTITY, rgb=True)
    assert_frame_equal(one, packed, tri, t)
    scene.destroy()
    ctx.close()
    ctx = beam.Context(device=0, devices=[0, 0])
    scene, keep, stats = gpu_build(ctx, meshes)
    assert stats["num_tris"] == H_N
    two = gpu_frame(ctx, scene, H_W, H_H, scenes.RAYS_SQUARE, H_EYE, scenes.IDENTITY, rgb=True)
    for k in ("packed", "tri_id", "t", "rgb"):
        assert np.array_equal(two[k], one[k]), k
    scene.destroy()
    ctx.close()
