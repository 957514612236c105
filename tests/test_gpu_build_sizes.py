"""BVH build across the size regimes of bm_build.hip, against the oracle bit for bit.

The build grows the radix tree per 512-leaf chunk in LDS and finds the nodes whose leaf range
crosses a chunk edge ("spanning" nodes) with Karras's searches; BVH4 records come from the chunk
kernel for chunk-local nodes and from k_pack4_span for spanning ones; the chunk table switches from
LDS to global levels above 3072 chunks; the radix sort switches tile size at 2^17 and 2^19 keys, and
from 2^14 to 2^22 keys sorts the top digit first and then each bucket in one workgroup (in LDS up to
2048 keys, 8192 above 2^19 keys with 1024-lane workgroups; a larger bucket switches the same build to
the three LSD passes, decided on the device: the skewed scene and the forced fallback below).
Each regime edge is built here and compared with orc_bvh_build (records a traversal reaches, triangle
records, Morton keys, permutation), then refit with moved vertices against orc_bvh_refit. Equal
Morton keys straddling chunk edges exercise the position tiebreak of the tree (32 + clz(i ^ j)).
"""
import numpy as np
import pytest

from gpu_util import gpu_build
from raytracercuda_amd import beam

pytestmark = pytest.mark.gpu


def soup(n, seed, dup=0):
    """n random triangles in [-1, 1]^3 (small ones, like a tessellated surface); `dup` of them are
    copies of one triangle (identical Morton keys), spread through the index range."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, size=(n, 1, 3)).astype(np.float32)
    tri = (c + rng.normal(scale=0.01, size=(n, 3, 3))).astype(np.float32)
    if dup:
        at = rng.choice(n, size=dup, replace=False)
        tri[at] = tri[at[0]]
    pos = tri.reshape(-1, 3)
    nrm = rng.normal(size=pos.shape).astype(np.float32)
    return [{"pos": pos, "nrm": nrm, "idx": np.arange(3 * n, dtype=np.uint32)}]


def compare(rec, tris, keys, perm, orc):
    orec, otris, okeys, operm = orc.export()
    assert np.array_equal(keys, okeys)
    assert np.array_equal(perm, operm)
    assert np.array_equal(tris, otris)
    assert rec.shape == orec.shape
    if rec.shape[1] == 16:
        assert np.array_equal(rec, orec), f"{int((rec != orec).any(1).sum())} records differ"
    else:
        reach = beam.reachable_records(orec)
        assert np.array_equal(reach, beam.reachable_records(rec))
        assert np.array_equal(rec[reach], orec[reach]), f"{int((rec[reach] != orec[reach]).any(1).sum())} differ"


@pytest.mark.parametrize("n,dup", [(2, 0), (511, 0), (512, 0), (513, 0), (1024, 300), (1025, 0), (4097, 2000),
                                   (16384, 0), (70000, 0), (131072, 0), (131073, 0), (140000, 5000),
                                   (300000, 3000), (524289, 0), (600000, 20000)])
@pytest.mark.parametrize("width", [4, 2])
def test_build_and_refit_at_regime_edges(oracle, n, dup, width):
    meshes = soup(n, seed=n + width, dup=dup)
    ctx = beam.Context(device=0, bvh_width=width)
    scene, keep, stats = gpu_build(ctx, meshes)
    assert stats["num_tris"] == n
    compare(*scene.export(), oracle.bvh_build(meshes, 4, width))
    # refit: every vertex moved a little, same topology
    moved = [dict(m, pos=(m["pos"] + np.float32(0.003) * np.sin(np.float32(7) * m["pos"])).astype(np.float32))
             for m in meshes]
    for m, d in zip(keep, moved):
        assert m.setVertexData(d["pos"], d["pos"].shape[0], 3, beam.VERTEX_DATA_POSITION) == 0
    scene.refitGPUScene()
    obvh = oracle.bvh_build(meshes, 4, width)
    obvh.refit(moved)
    compare(*scene.export(), obvh)
    scene.destroy()
    ctx.close()


def test_build_skewed_top_digit(oracle):
    """A dense cluster plus one far triangle: the scene bounds grow ~100x, so nearly every Morton key
    shares its top digit, a bucket far beyond k_bucket_sort's LDS. The device sees it in k_morton's
    top-digit histogram and the same build sorts with the three LSD passes (k_onesweep_wide passes 0
    and 1, k_bucket_sort pass 2): the first build already reports that path, and every build gives
    the oracle's records (no host-side memory of the skew: VERDICT r3)."""
    meshes = soup(40000, seed=11, dup=0)
    meshes[0]["pos"] = (meshes[0]["pos"] * np.float32(0.01)).astype(np.float32)
    far = np.array([[100, 100, 100], [101, 100, 100], [100, 101, 100]], np.float32)
    meshes.append({"pos": far, "nrm": np.ones_like(far), "idx": np.arange(3, dtype=np.uint32)})
    ctx = beam.Context(device=0)
    scene, keep, stats = gpu_build(ctx, meshes)
    assert stats["num_tris"] == 40001
    assert stats["sort_path"] == beam.SORT_MSD_SKEW  # decided on the device, on the first build
    obvh = oracle.bvh_build(meshes, 4, 4)
    compare(*scene.export(), obvh)
    for _ in range(2):
        assert scene.updateGPUScene(stats=True)["sort_path"] == beam.SORT_MSD_SKEW
        compare(*scene.export(), obvh)
    # the same scene without the far triangle: the next build goes back to the bucket sort
    scene.removeMesh(keep[1])
    st = scene.updateGPUScene(stats=True)
    assert st["num_tris"] == 40000 and st["sort_path"] == beam.SORT_MSD
    compare(*scene.export(), oracle.bvh_build(meshes[:1], 4, 4))
    scene.destroy()
    ctx.close()


@pytest.mark.parametrize("n,wide", [(20000, False), (140000, False), (300000, False), (300000, True),
                                    (600000, True)])
def test_build_lsd_fallback_forced(oracle, n, wide):
    """BM_PARAM_BUCKET_LDS_CAP 0 sends every top-digit-first build down the device-side LSD fallback:
    256-lane (one-key and four-key tiles) and 1,024-lane bucket kernels (msd_wide_n lowered for the
    300,000-triangle case). Records equal the oracle's; the build reports the fallback."""
    meshes = soup(n, seed=n + 5, dup=n // 50)
    params = {"bucket_lds_cap": 0}
    if wide:
        params["msd_wide_n"] = 1 << 14
    ctx = beam.Context(device=0, params=params)
    scene, keep, stats = gpu_build(ctx, meshes)
    assert stats["num_tris"] == n and stats["sort_path"] == beam.SORT_MSD_SKEW
    compare(*scene.export(), oracle.bvh_build(meshes, 4, 4))
    scene.destroy()
    ctx.close()


@pytest.mark.parametrize("n,params", [(20000, {}), (300000, {}), (50000, {"msd_max_n": 0}),
                                      (700000, {"msd_max_n": 0})])
def test_build_constant_digits(oracle, n, params):
    """Every triangle a copy of one: all Morton keys equal, so every pass's histogram has one digit
    holding all n keys and the one-sweep tiles take their identity copy (the top-digit-first sort's
    device-side LSD fallback, and the plain LSD passes with msd_max_n 0). Records equal the
    oracle's (ties broken by triangle index)."""
    meshes = soup(n, seed=n + 9, dup=n)
    ctx = beam.Context(device=0, params=params)
    scene, keep, stats = gpu_build(ctx, meshes)
    assert stats["num_tris"] == n
    assert stats["sort_path"] == (beam.SORT_LSD if params else beam.SORT_MSD_SKEW)
    compare(*scene.export(), oracle.bvh_build(meshes, 4, 4))
    scene.destroy()
    ctx.close()


def test_build_above_the_lds_chunk_table(oracle):
    """1.7M triangles: 3,321 chunks, beyond the LDS chunk table (3,072): global table levels."""
    n = 1_700_000
    meshes = soup(n, seed=7, dup=1000)
    ctx = beam.Context(device=0)
    scene, keep, stats = gpu_build(ctx, meshes)
    assert stats["num_tris"] == n
    compare(*scene.export(), oracle.bvh_build(meshes, 4, 4))
    scene.destroy()
    ctx.close()


def test_msd_max_n_is_capped(oracle):
    """BM_PARAM_MSD_MAX_N above 2^22 is refused (the device-side LSD fallback of a top-digit-first sort
    covers at most 1,024 tiles); 2^22 itself is accepted and a build under it sorts top digit
    first with the oracle's records."""
    ctx = beam.Context(device=0)
    for bad in ((1 << 22) + 1, 1 << 23):
        with pytest.raises(beam.BeamError):
            ctx.set_param("msd_max_n", bad)
    ctx.set_param("msd_max_n", 1 << 22)
    meshes = soup(70000, seed=31)
    scene, keep, stats = gpu_build(ctx, meshes)
    assert stats["sort_path"] == beam.SORT_MSD
    compare(*scene.export(), oracle.bvh_build(meshes, 4, 4))
    scene.destroy()
    ctx.close()


def test_front_launch_parameter_refused():
    """k_front (gather, keys and top-digit pass in one launch, measured slower in round 4: DESIGN.md §8)
    was removed in round 5 (the gather computes the Morton keys itself now); BM_PARAM_FRONT_MAX_N > 0 is
    refused and no build reports a fused front."""
    ctx = beam.Context(device=0)
    with pytest.raises(beam.BeamError):
        ctx.set_param("front_max_n", 1 << 19)
    ctx.set_param("front_max_n", 0)
    ctx.set_param("front_max_n", -1)
    scene, keep, stats = gpu_build(ctx, soup(16384, seed=5))
    assert stats["fused_front"] == 0
    scene.destroy()
    ctx.close()
