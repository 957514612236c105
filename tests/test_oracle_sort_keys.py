"""The designed-key scenes (tests/key_scenes.py) and the oracle on them, without a GPU.

tests/test_gpu_sort_keys.py builds every named case on the GPU and compares it with numpy's stable sort
and with the oracle. This file proves, for each case, that
  * its keys really sit on the edge the case is named after: exact bucket sizes, size classes, shared
    digits and tile patterns, asserted on the histograms of the designed keys (anchors included), and the
    sort path a model of launch_build's decisions gives for them is the one the case states;
  * the oracle's build of the scene exports exactly the designed keys, sorted, and numpy's stable
    permutation: the scene construction dictates the keys, and the oracle the GPU is compared with was
    itself compared with something that is no radix sort.
The constants the cases are designed around are read back from csrc/bm_sort.h, so that a threshold that
moves fails here and not as a silently vacuous GPU test.
"""
import os
import re

import numpy as np
import pytest

import key_scenes as ks

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracercuda_amd", "csrc")


def check_order(full, okeys, operm):
    """The checker both files rest on: exported keys and permutation against numpy's stable sort."""
    keys, perm = ks.expected_order(full)
    assert np.array_equal(okeys, keys)
    assert np.array_equal(operm, perm), f"{int((operm != perm).sum())} positions differ from the stable order"


def test_constants_are_the_sources():
    text = open(os.path.join(CSRC, "bm_sort.h")).read()
    for name, value in ks.CODE.items():
        m = re.search(r"\b%s = ([0-9u <]+);" % name, text)
        assert m, name
        assert eval(m.group(1).replace("u", "")) == value, name
    # the two one-sweep thresholds coincide: onesweep_items never returns 2 (no test can reach 2-key tiles)
    assert ks.CODE["OSW_TINY_N"] == ks.CODE["OSW_SMALL_N"]
    assert {ks.onesweep_items(n) for n in (1, 1 << 17, (1 << 17) + 1, 1 << 19, (1 << 19) + 1, 1 << 22)} == {1, 4, 8}
    build = open(os.path.join(CSRC, "bm_build.hip")).read()
    assert "(wide ? 1024 : 256) * BS_ITEMS" in build and "cap + 1, plan" in build  # bucket_cap's model


def test_interleave_round_trip():
    rng = np.random.default_rng(1)
    x, y, z = rng.integers(0, 1024, (3, 5000), dtype=np.uint32)
    ext = np.array([0, 1, 2, 511, 512, 1022, 1023], np.uint32)
    x[:7], y[7:14], z[14:21] = ext, ext, ext
    key = ks.interleave(x, y, z)
    assert int(key.max()) <= ks.KEY_MAX
    for a, b in zip(ks.deinterleave(key), (x, y, z)):
        assert np.array_equal(a, b)
    keys = np.concatenate([rng.integers(0, 1 << 30, 5000, dtype=np.uint32), np.uint32([0, ks.KEY_MAX, 1, 1 << 29])])
    assert np.array_equal(ks.interleave(*ks.deinterleave(keys)), keys)
    assert ks.interleave(1, 0, 0) == 4 and ks.interleave(0, 1, 0) == 2 and ks.interleave(0, 0, 1) == 1
    assert ks.interleave(1023, 0, 0) == 0x24924924 and ks.interleave(1023, 1023, 1023) == ks.KEY_MAX


def test_interleave_is_the_oracles_key(oracle):
    v = np.array([0, 1, 511, 512, 1023], np.uint32)
    x, y, z = (a.reshape(-1) for a in np.meshgrid(v, v, v, indexing="ij"))
    keys = ks.interleave(x, y, z)
    meshes, full = ks.scene_from_keys(keys)
    _, _, okeys, operm = oracle.bvh_build(meshes, 4, 4).export()
    assert np.array_equal(okeys[np.argsort(operm)], full)  # triangle i has key full[i]
    check_order(full, okeys, operm)


def test_the_checker_bites():
    """An unstable order of the same keys (equal keys swapped) and a wrong key are both refused."""
    keys, _ = ks.case("a-items256")
    full = np.concatenate([[0], keys, [ks.KEY_MAX]]).astype(np.uint32)
    skeys, perm = ks.expected_order(full)
    check_order(full, skeys, perm)
    i = int(np.flatnonzero(skeys[1:] == skeys[:-1])[0])
    bad = perm.copy()
    bad[[i, i + 1]] = bad[[i + 1, i]]
    assert np.array_equal(full[bad], skeys)  # still sorted: only stability is lost
    with pytest.raises(AssertionError):
        check_order(full, skeys, bad)
    wrong = skeys.copy()
    wrong[5] ^= 1
    with pytest.raises(AssertionError):
        check_order(full, wrong, perm)


# ---- preconditions, per family ---------------------------------------------------------------------------
def only_these_buckets(e):
    """Top-digit histogram = the case's sizes, one key per anchor, nothing else."""
    want = np.zeros(ks.RADIX, np.int64)
    want[0] = want[ks.RADIX - 1] = 1
    for d, c in e["sizes"].items():
        assert 0 < d < ks.RADIX - 1
        want[d] = c
    assert np.array_equal(e["buckets"], want)


def pre_items(name, keys, e):
    block = 256 if name.startswith("a") else 1024
    sizes = list(ks.SIZES_256 if block == 256 else ks.SIZES_1024)
    wide, cap = ks.bucket_cap(e["n"], e["params"])
    assert wide == (block == 1024) and cap == block * ks.CODE["BS_ITEMS"] == max(sizes)
    if name.endswith("skew"):
        sizes.append(cap + 1)
    only_these_buckets(e)
    assert sorted(e["sizes"].values()) == sorted(sizes)
    assert sorted(e["sizes"]) == list(range(1, len(sizes) + 1))
    assert int(e["buckets"].max()) == (cap + 1 if name.endswith("skew") else cap)
    ie = {-(-c // block) for c in sizes if c <= cap}
    assert ie == (set(range(1, 9)) if block == 256 else {1, 2, 3, 5, 6, 8})
    if block == 256:
        assert sorted(sizes)[:23] == sorted([256 * k + o for k in range(1, 8) for o in (-1, 0, 1)] + [2047, 2048])
    else:
        assert sorted(sizes)[:11] == [1023, 1024, 1025, 2047, 2048, 2049, 5119, 5120, 5121, 8191, 8192]
    assert ks.CODE["MSD_MIN_N"] <= e["n"] <= ks.CODE["OSW_TINY_N"] and ks.onesweep_items(e["n"]) == 1
    # every kind of low bits is there, as stated, and the buckets are interleaved in input order
    assert set(e["kinds"].values()) == set(ks.KINDS)
    top = keys >> np.uint32(20)
    for d, kind in e["kinds"].items():
        assert ks.kind_holds(kind, keys[top == d] & np.uint32((1 << 20) - 1)), (d, kind)
    assert int((np.diff(top.astype(np.int64)) != 0).sum()) > keys.size // 2


def pre_cap(name, keys, e):
    only_these_buckets(e)
    wide, cap = ks.bucket_cap(e["n"], e["params"])
    assert not wide and cap == 300 and e["n"] >= ks.CODE["MSD_MIN_N"]
    c = np.array(sorted(e["sizes"].values()))
    assert c.size == 60 and c.min() == 290
    if name.endswith("skew"):
        assert c.max() == 301 and int((c > 300).sum()) == 1
    else:
        assert c.max() == 300
    assert set(range(290, 301)) <= set(c.tolist())


def pre_classes(name, keys, e):
    only_these_buckets(e)
    wide, cap = ks.bucket_cap(e["n"], e["params"])
    assert wide and cap == 8192 == int(e["buckets"].max())
    assert ks.CODE["OSW_TINY_N"] < e["n"] <= ks.CODE["OSW_MID_N"] and ks.onesweep_items(e["n"]) == 4
    want = {0, 1, 2, 63, 64, 65, 127, 128, 8127, 8128, 8191, 8192} | {
        64 * j for j in (3, 7, 15, 31, 47, 63, 64, 65, 95, 125, 126, 127)}
    by_size = {}
    for d, c in e["all_sizes"].items():
        by_size.setdefault(c, []).append(d)
        assert int(e["buckets"][d]) == c
    assert want <= set(by_size)
    two_groups = [c for c, ds in by_size.items() if len(ds) == 2 and ds[0] >> 6 != ds[1] >> 6]
    assert len(two_groups) >= 8 and set(two_groups) == want
    in_digit_order = [c for _, c in sorted(e["all_sizes"].items())]
    assert in_digit_order != sorted(in_digit_order) and in_digit_order != sorted(in_digit_order, reverse=True)
    # bucket_plan: class of a bucket with more than one key = min(c >> 6, 126); at most one key: its own class
    c = e["buckets"]
    cls = set(np.minimum(c[c > 1] >> 6, ks.NCLS - 2).tolist())
    assert len(cls) >= 20 and 63 in cls and min(cls) == 0 and max(cls) == ks.NCLS - 2
    assert any(v < 63 for v in cls) and any(v > 63 for v in cls)
    assert int((c == 0).sum()) > 0 and int((c == 1).sum()) >= 3  # the single-key/empty class, anchors included
    assert len({d >> 6 for d in e["sizes"]}) >= 12  # per-wave class counts: the buckets lie in most of the 16 waves


def pre_constant_pass(name, keys, e):
    _, form, p, mode = name.split("-")
    p, n = int(p[1]), e["n"]
    assert p == e["p"] and n == ks.E_MODES[mode][0]
    h = e["hist"][p]
    if form == "const":
        assert h[ks.E_CONST] == n - 2 and h[0] == 1 and h[ks.RADIX - 1] == 1
    else:
        assert h[0] == n - 1 and h[ks.RADIX - 1] == 1
    assert int(h.max()) == e["shared"] and int((h > 0).sum()) == (3 if form == "const" else 2)
    for q in range(3):
        if q != p:
            # "vary": most of the 1,024 values occur and none holds a hundredth of the keys
            assert int((e["hist"][q] > 0).sum()) > ks.RADIX * 3 // 4 and int(e["hist"][q].max()) < n // 100
    if mode == "plain":
        assert n < ks.CODE["MSD_MIN_N"]
    if mode == "msd":
        assert int(e["buckets"].max()) == (e["shared"] if p == 2 else int(e["hist"][2].max()))
        assert (int(e["buckets"].max()) > 2048) == (p == 2)


def pre_lsd(name, keys, e):
    n = e["n"]
    assert n == int(name.split("-")[2]) and e["items"] == {20000: 1, 140000: 4, 530000: 8}[n]
    full_min, full_max = 0, ks.KEY_MAX  # the anchors are the extremes
    assert int(e["hist"][0][0]) >= 1 and int(e["hist"][2][ks.RADIX - 1]) >= 1 and full_min == 0 and full_max == ks.KEY_MAX
    dup = 1.0 - np.unique(keys).size / keys.size
    assert 0.019 <= dup <= 0.021, dup
    for p in range(3):
        assert int((e["hist"][p] > 0).sum()) == ks.RADIX


def pre_absent(name, keys, e):
    n, p, tile = e["n"], e["p"], e["tile"]
    assert n == 40 * 1024 + 1 and tile == 1024 and p == (2 if name.endswith("msd") else 0)
    full = np.concatenate([[0], keys, [ks.KEY_MAX]]).astype(np.uint32)
    d = ks.digits(full, p)
    high = d >= 512
    ntiles = -(-n // tile)
    assert ntiles == 41 > ks.CODE["OS_LB_WIN"] > ks.CODE["LB_WIN"]
    per_tile = np.array([int(high[t * tile:(t + 1) * tile].sum()) for t in range(ntiles)])
    # tile 0: the anchor (digit 0) and 1,023 high keys; tiles 1..38: no high key; the last 1,024 positions are
    # tile 39 but its first key, and tile 40's only key
    assert per_tile.tolist() == [1023] + [0] * 38 + [1023, 1]
    assert not high[0] and high[1:1024].all() and high[n - 1024:].all() and not high[1024:n - 1024].any()
    for block in (d[1:1024], d[n - 1024:]):
        assert set(block.tolist()) == set(range(512, 1024))
    assert set(d[1024:n - 1024].tolist()) == set(range(512))
    if name.endswith("msd"):
        assert int(e["buckets"].max()) <= 2048


PRE = {"a": pre_items, "b": pre_items, "c": pre_cap, "d": pre_classes, "e": pre_constant_pass, "f": pre_lsd,
       "g": pre_absent}


@pytest.mark.parametrize("name", sorted(ks.CASES))
def test_case_preconditions_and_oracle_order(oracle, name):
    keys, e = ks.case(name)
    meshes, full = ks.scene_from_keys(keys)
    assert e["n"] == full.size == keys.size + 2
    assert np.array_equal(e["buckets"], np.bincount(full >> np.uint32(20), minlength=ks.RADIX))
    assert np.array_equal(e["buckets"], e["hist"][2]) and (e["hist"].sum(1) == e["n"]).all()
    PRE[name[0]](name, keys, e)
    assert ks.model_sort_path(e["n"], e["buckets"], e["params"]) == e["sort_path"]
    _, _, okeys, operm = oracle.bvh_build(meshes, 4, 4).export()
    check_order(full, okeys, operm)


def test_case_builders_are_deterministic():
    for name in ("a-items256", "d-classes", "g-absent-lsd"):
        assert np.array_equal(ks.CASES[name]()[0], ks.case(name)[0])


def test_split_meshes_keeps_every_triangle(oracle):
    """split_meshes and mesh_counts (case h of the GPU file): 256 and 257 unequal parts with the first, the
    middle and the last empty; the oracle's build of the parts equals its build of the one mesh."""
    rng = np.random.default_rng(3)
    n = 2000
    pos = rng.normal(size=(3 * n, 3)).astype(np.float32)
    mesh = {"pos": pos, "nrm": rng.normal(size=pos.shape).astype(np.float32), "idx": np.arange(3 * n, dtype=np.uint32)}
    whole = oracle.bvh_build([mesh], 4, 4).export()
    for parts in (ks.CODE["RJ_LDS_MESHES"], ks.CODE["RJ_LDS_MESHES"] + 1):
        counts = ks.mesh_counts(n, parts, seed=parts)
        assert len(counts) == parts and sum(counts) == n and len(set(counts)) > 8  # unequal sizes
        assert [i for i, c in enumerate(counts) if c == 0] == [0, parts // 2, parts - 1]
        cut = ks.split_meshes(mesh, counts)
        assert [m["idx"].size // 3 for m in cut] == counts
        for a, b in zip(whole, oracle.bvh_build(cut, 4, 4).export()):
            assert np.array_equal(a, b)
