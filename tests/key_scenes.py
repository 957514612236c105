"""Scenes whose Morton keys are dictated key by key, for the build's radix sort. Shared by
tests/test_oracle_sort_keys.py (the cases' preconditions and the oracle against numpy's stable sort, without
a GPU) and tests/test_gpu_sort_keys.py (the GPU build of every case). Test infrastructure only.

The build quantises the centre of each triangle's box over the bounds of all centres: scale = 1024 / extent
and quant10 (csrc/bm_common.h). Two anchor triangles with centres (0, 0, 0) and (1024, 1024, 1024) pin the
lower bound to 0 and the scale to 1, so a triangle whose box is centred on (x + 1/2, y + 1/2, z + 1/2), x, y, z
integers in 0..1023, gets exactly the key interleave(x, y, z); its corners are the centre +-1/4 per axis,
all exact in float32. The anchors are triangles 0 and n - 1 with the keys 0 and 2^30 - 1: they count, one
key each in digits 0 and 1023 of every pass. (That also means no scene has a digit that holds every key
unless all keys are equal: on any axis with an extent the smallest centre quantises to 0 and the largest to
1023. A pass whose digit is constant while the others vary exists for the designed keys only, n - 2 of n.)

The expected order of a case is numpy's stable argsort of its keys: not a restatement of a radix sort.

The named cases (CASES) are built around constants of csrc/bm_sort.h and bm_build.hip, repeated in CODE
below; test_oracle_sort_keys.py reads them back from the sources, so a moved threshold fails there.
"""
from functools import lru_cache

import numpy as np

RADIX_BITS, RADIX = 10, 1024
KEY_MAX = (1 << 30) - 1
# constants of the sort the cases are designed around (name in the sources: value)
CODE = {"BS_ITEMS": 8, "MSD_MIN_N": 1 << 14, "MSD_WIDE_N": 1 << 19, "MSD_MAX_N": 1 << 22, "OSW_TINY_N": 1 << 17,
        "OSW_SMALL_N": 1 << 17, "OSW_MID_N": 1 << 19, "OS_BLOCK_N": 1024, "OS_LB_WIN": 32, "LB_WIN": 8,
        "RJ_LDS_MESHES": 256, "NCLS": 128}
NCLS = CODE["NCLS"]  # bucket_plan's size classes (64 keys each)


def interleave(x, y, z):
    """The 30-bit Morton key of 10-bit x, y, z: bit b of x, y, z lands in key bit 3b + 2, 3b + 1, 3b."""
    x, y, z = (np.asarray(a, np.uint32) for a in (x, y, z))
    key = np.zeros(np.broadcast(x, y, z).shape, np.uint32)
    for b in range(RADIX_BITS):
        key |= ((x >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + 2)
        key |= ((y >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + 1)
        key |= ((z >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return key


def deinterleave(key):
    key = np.asarray(key, np.uint32)
    x, y, z = (np.zeros(key.shape, np.uint32) for _ in range(3))
    for b in range(RADIX_BITS):
        x |= ((key >> np.uint32(3 * b + 2)) & np.uint32(1)) << np.uint32(b)
        y |= ((key >> np.uint32(3 * b + 1)) & np.uint32(1)) << np.uint32(b)
        z |= ((key >> np.uint32(3 * b)) & np.uint32(1)) << np.uint32(b)
    return x, y, z


_CORNERS = np.array([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]], np.float32) * np.float32(0.25)


def scene_from_keys(keys, seed=0):
    """([mesh], full keys): triangle 0 the anchor with key 0, then one triangle per key in input order, then
    the anchor with key 2^30 - 1. Every vertex has its own random normal, so a record gathered from the wrong
    triangle shows in the packed colour."""
    keys = np.asarray(keys, np.uint32)
    assert keys.ndim == 1 and (keys.size == 0 or int(keys.max()) <= KEY_MAX)
    x, y, z = deinterleave(keys)
    cen = np.stack([x, y, z], 1).astype(np.float32) + np.float32(0.5)
    cen = np.concatenate([np.zeros((1, 3), np.float32), cen, np.full((1, 3), 1024, np.float32)])
    pos = (cen[:, None, :] + _CORNERS[None]).reshape(-1, 3)
    nrm = np.random.default_rng(seed).normal(size=pos.shape).astype(np.float32)
    full = np.concatenate([[0], keys, [KEY_MAX]]).astype(np.uint32)
    return [{"pos": pos, "nrm": nrm, "idx": np.arange(pos.shape[0], dtype=np.uint32)}], full


def split_meshes(mesh, counts):
    """The mesh cut into consecutive meshes of the given triangle counts (zeros allowed: such a mesh keeps
    one vertex, which the API asks of every mesh, and no index)."""
    idx = np.asarray(mesh["idx"], np.uint32).reshape(-1, 3)
    assert sum(counts) == idx.shape[0]
    out, a = [], 0
    for c in counts:
        used, inv = np.unique(idx[a:a + c].reshape(-1), return_inverse=True)
        if c == 0:
            used = np.zeros(1, np.int64)
        out.append({"pos": np.ascontiguousarray(mesh["pos"][used]), "nrm": np.ascontiguousarray(mesh["nrm"][used]),
                    "idx": inv.astype(np.uint32).reshape(-1)})
        a += c
    return out


def mesh_counts(n, parts, seed):
    """`parts` unequal triangle counts summing to n; the first, the middle and the last are 0."""
    rng = np.random.default_rng(seed)
    empty = (0, parts // 2, parts - 1)
    cuts = np.sort(rng.choice(np.arange(1, n), parts - len(empty) - 1, replace=False))
    sizes = np.diff(np.concatenate([[0], cuts, [n]])).tolist()
    for e in empty:
        sizes.insert(e, 0)
    return sizes


def onesweep_items(n):
    """Keys per lane of a one-sweep tile of 1,024 lanes (onesweep_items in bm_sort.h)."""
    return 1 if n <= CODE["OSW_TINY_N"] else 2 if n <= CODE["OSW_SMALL_N"] else 4 if n <= CODE["OSW_MID_N"] else 8


def bucket_cap(n, params):
    """(1,024-lane bucket kernel?, largest bucket sorted in LDS) as launch_build works them out."""
    wide = n > min(params.get("msd_wide_n", CODE["MSD_WIDE_N"]), CODE["MSD_WIDE_N"])
    return wide, min(params.get("bucket_lds_cap", 1 << 32), (1024 if wide else 256) * CODE["BS_ITEMS"])


def model_sort_path(n, buckets, params):
    """The sort path launch_build and the device-side skew test take for n keys with this top-digit histogram."""
    if n < CODE["MSD_MIN_N"] or n > min(params.get("msd_max_n", CODE["MSD_MAX_N"]), CODE["MSD_MAX_N"]):
        return "SORT_LSD"
    return "SORT_MSD_SKEW" if int(buckets.max()) > bucket_cap(n, params)[1] else "SORT_MSD"


def digits(keys, p):
    return (np.asarray(keys, np.uint32) >> np.uint32(RADIX_BITS * p)) & np.uint32(RADIX - 1)


def _expect(keys, path, params, **more):
    full = np.concatenate([[0], keys, [KEY_MAX]]).astype(np.uint32)
    e = {"n": int(full.size), "sort_path": path, "params": params,
         "buckets": np.bincount(full >> np.uint32(20), minlength=RADIX),
         "hist": np.stack([np.bincount(digits(full, p), minlength=RADIX) for p in range(3)])}
    e.update(more)
    return keys.astype(np.uint32), e


# ---- the low 20 bits of a bucket's keys, in input order -------------------------------------------------
KINDS = ("random", "equal", "descending", "alternating", "low-constant", "mid-constant", "edge-digits")


def _low20(rng, kind, c):
    r10 = lambda: rng.integers(0, RADIX, c, dtype=np.uint32)
    if kind == "random":
        return rng.integers(0, 1 << 20, c, dtype=np.uint32)
    if kind == "equal":
        return np.full(c, rng.integers(0, 1 << 20), np.uint32)
    if kind == "descending":
        return np.sort(rng.choice(1 << 20, c, replace=False))[::-1].astype(np.uint32)
    if kind == "alternating":  # equal keys every second position: their runs cross every wave boundary
        a, b = np.sort(rng.choice(1 << 20, 2, replace=False))[::-1]
        return np.where(np.arange(c) % 2 == 0, a, b).astype(np.uint32)
    if kind == "low-constant":
        return (r10() << np.uint32(10)) | np.uint32(rng.integers(0, RADIX))
    if kind == "mid-constant":
        return (np.uint32(rng.integers(0, RADIX)) << np.uint32(10)) | r10()
    assert kind == "edge-digits"  # digits 0 and 1023 in both lower passes, a third of the keys each
    lo = np.where(rng.integers(0, 3, c) == 0, 0, np.where(rng.integers(0, 2, c) == 0, 1023, r10()))
    mid = np.where(rng.integers(0, 3, c) == 0, 0, np.where(rng.integers(0, 2, c) == 0, 1023, r10()))
    lo[:4], mid[:4] = (0, 1023, 0, 1023), (0, 1023, 1023, 0)
    return (mid.astype(np.uint32) << np.uint32(10)) | lo.astype(np.uint32)


def kind_holds(kind, low):
    """Whether the low 20 bits `low` (input order) are of the kind _low20 was asked for."""
    lo, mid = digits(low, 0), digits(low, 1)
    d = np.diff(low.astype(np.int64))
    return {"random": np.unique(low).size > low.size // 2,
            "equal": np.unique(low).size == 1,
            "descending": bool((d < 0).all()),
            "alternating": np.unique(low).size == 2 and bool((d != 0).all()),
            "low-constant": np.unique(lo).size == 1 and np.unique(mid).size > 64,
            "mid-constant": np.unique(mid).size == 1 and np.unique(lo).size > 64,
            "edge-digits": all(v in dd for dd in (lo, mid) for v in (0, 1023)) and np.unique(low).size > 64}[kind]


def _weave(rng, per_bucket):
    """The buckets' keys interleaved by a shuffle of their labels; each bucket keeps its own input order."""
    labels = rng.permutation(np.repeat(np.arange(len(per_bucket)), [k.size for k in per_bucket]))
    out = np.empty(labels.size, np.uint32)
    for b, k in enumerate(per_bucket):
        out[labels == b] = k
    return out


def _sized_buckets(seed, digit_sizes, kinds, path, params, **more):
    """digit_sizes: [(top digit, keys)]; bucket i takes kinds[i % len(kinds)]."""
    rng = np.random.default_rng(seed)
    per, kind_of = [], {}
    for i, (d, c) in enumerate(digit_sizes):
        kind_of[d] = kinds[i % len(kinds)]
        per.append((np.uint32(d) << np.uint32(20)) | _low20(rng, kind_of[d], c))
    return _expect(_weave(rng, per), path, params, sizes=dict(digit_sizes), kinds=kind_of, **more)


# ---- a, b: items per lane of k_bucket_sort ------------------------------------------------------------------
SIZES_256 = [256 * k + o for k in range(1, 8) for o in (-1, 0, 1)] + [2047, 2048]
SIZES_1024 = [1023, 1024, 1025, 2047, 2048, 2049, 5119, 5120, 5121, 8191, 8192]


def _items_case(sizes, extra, params, seed):
    order = np.random.default_rng(seed).permutation(len(sizes))
    ds = [(1 + i, sizes[j]) for i, j in enumerate(order)]
    if extra:
        ds.append((1 + len(sizes), extra))
    return _sized_buckets(seed + 1, ds, KINDS, "SORT_MSD_SKEW" if extra else "SORT_MSD", params)


# ---- c: a cap inside the LDS arrays ------------------------------------------------------------------------
def _cap_case(over):
    rng = np.random.default_rng(300)
    ds = rng.choice(np.arange(1, RADIX - 1), 60, replace=False)
    sizes = rng.permutation(290 + np.arange(60) % 11)
    if over:
        sizes[np.flatnonzero(sizes == 300)[0]] = 301
    return _sized_buckets(301, list(zip(ds.tolist(), sizes.tolist())), ("random",),
                          "SORT_MSD_SKEW" if over else "SORT_MSD", {"bucket_lds_cap": 300})


# ---- d: bucket_plan's size classes -------------------------------------------------------------------------
SIZES_D = sorted({0, 1, 2, 63, 64, 65, 127, 128, 8127, 8128, 8191, 8192} |
                 {64 * j for j in (3, 7, 15, 31, 47, 63, 64, 65, 95, 125, 126, 127)})
FILL_D = [64 * j + 17 for j in (5, 10, 20, 40, 50, 70, 80, 110)]  # eight more classes, one bucket each


def _classes_case():
    """Every size of SIZES_D twice, in digits of different 64-digit groups (the waves of bucket_plan), the
    fillers once; which digit holds which size is a shuffle, so sizes are not monotone in the digit."""
    rng = np.random.default_rng(64)
    free = rng.permutation(np.arange(1, RADIX - 1)).tolist()
    ds = []
    for c in rng.permutation(SIZES_D).tolist():
        a = free.pop()
        b = next(d for d in reversed(free) if d >> 6 != a >> 6)
        free.remove(b)
        ds += [(a, c), (b, c)]
    ds += [(free.pop(), c) for c in FILL_D]
    ds = [ds[i] for i in rng.permutation(len(ds))]
    return _sized_buckets(65, [x for x in ds if x[1]], ("random", "equal", "descending"), "SORT_MSD",
                          {"msd_wide_n": 1 << 14}, all_sizes=dict(ds))


# ---- e: one pass whose digit is constant ---------------------------------------------------------------------
E_MODES = {"plain": (5000, {}), "lsd": (20000, {"msd_max_n": 0}), "msd": (20000, {})}
E_CONST = 517  # neither anchor's digit


def _constant_pass_case(form, p, mode):
    """form "const": every designed key has digit p = E_CONST (n - 2 of the n keys; the anchors hold 0 and
    1023). form "butone": every designed key has digit p = 0, the first anchor's: n - 1 of n share it. The
    other two digits are random."""
    n, params = E_MODES[mode]
    rng = np.random.default_rng(1000 + 10 * p + (form == "const") + n)
    d = [rng.integers(0, RADIX, n - 2, dtype=np.uint32) for _ in range(3)]
    d[p][:] = E_CONST if form == "const" else 0
    keys = d[0] | (d[1] << np.uint32(10)) | (d[2] << np.uint32(20))
    path = "SORT_LSD" if mode != "msd" else "SORT_MSD_SKEW" if p == 2 else "SORT_MSD"
    return _expect(keys, path, params, p=p, shared=n - 2 if form == "const" else n - 1,
                   value=E_CONST if form == "const" else 0)


# ---- f: plain LSD passes on varied keys ----------------------------------------------------------------------
def _lsd_case(n):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 30, n - 2, dtype=np.uint32)
    at = rng.choice(n - 2, (n - 2) // 50, replace=False)
    keys[at] = keys[rng.integers(0, n - 2, at.size)]  # about 2 % copies of other keys
    return _expect(keys, "SORT_LSD", {"msd_max_n": 0}, items=onesweep_items(n))


# ---- g: digits absent from the middle tiles ------------------------------------------------------------------
G_N = 40 * 1024 + 1


def _absent_case(p, params, path):
    """Digit p (the digit of the first pass run): input positions 1..1023 (position 0 is the anchor with
    digit 0) and the last 1,024 input positions (the last of them the other anchor, digit 1023) carry the
    values 512..1023, each of them at least once in either block; every other position a value in 0..511."""
    rng = np.random.default_rng(4100 + p)
    m = G_N - 2
    d = [rng.integers(0, RADIX, m, dtype=np.uint32) for _ in range(3)]
    d[p] = rng.integers(0, 512, m, dtype=np.uint32)
    d[p][:1023] = 512 + rng.permutation(1023) % 512
    d[p][m - 1023:] = 512 + rng.permutation(1023) % 512
    keys = d[0] | (d[1] << np.uint32(10)) | (d[2] << np.uint32(20))
    return _expect(keys, path, params, p=p, tile=1024 * onesweep_items(G_N))


CASES = {
    "a-items256": lambda: _items_case(SIZES_256, 0, {}, 256),
    "a-items256-skew": lambda: _items_case(SIZES_256, 2049, {}, 256),
    "b-items1024": lambda: _items_case(SIZES_1024, 0, {"msd_wide_n": 1 << 14}, 1024),
    "b-items1024-skew": lambda: _items_case(SIZES_1024, 8193, {"msd_wide_n": 1 << 14}, 1024),
    "c-cap300": lambda: _cap_case(False),
    "c-cap300-skew": lambda: _cap_case(True),
    "d-classes": _classes_case,
    "g-absent-msd": lambda: _absent_case(2, {}, "SORT_MSD"),
    "g-absent-lsd": lambda: _absent_case(0, {"msd_max_n": 0}, "SORT_LSD"),
}
for _form in ("const", "butone"):
    for _p in range(3):
        for _mode in E_MODES:
            CASES[f"e-{_form}-p{_p}-{_mode}"] = lambda f=_form, p=_p, m=_mode: _constant_pass_case(f, p, m)
for _n in (20000, 140000, 530000):
    CASES[f"f-lsd-{_n}"] = lambda n=_n: _lsd_case(n)


@lru_cache(maxsize=None)
def case(name):
    """(keys, expect) of a named case; the arrays are shared and read-only."""
    keys, e = CASES[name]()
    for a in (keys, e["buckets"], e["hist"]):
        a.setflags(write=False)
    return keys, e


def expected_order(full):
    """(sorted keys, permutation) by numpy's stable sort."""
    perm = np.argsort(full, kind="stable")
    return full[perm], perm.astype(np.uint32)
