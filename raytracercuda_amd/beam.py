"""Python mirror of the reference's Beam host API (Raytracer/Beam.h:32-72) over the C ABI.

Same class and method names, argument meaning and u32 error codes as the reference:

    ctx    = Context(device=0)                       # new: explicit device/stream context
    mesh   = IMesh.create(ctx)
    mesh.setIndices(idx, len(idx)); mesh.setVertexData(pos, nv, 3, VERTEX_DATA_POSITION)
    scene  = IScene.create(ctx); scene.addMesh(mesh); scene.updateGPUScene()
    cam    = ICamera.create(ctx); cam.setInitialRays(W, H, -1, 1, -1, 1, 1)
    rt     = IRenderTarget.createOffscreen(ctx, W, H)   # replaces registerGLTBO
    rt.lock(); cam.traceScene(eye3, orient3x3, scene); rt.unlock()

As in the reference (RenderTarget.cpp:53-88), lock() makes the target the process-wide current
render target that traceScene()/clear() use. Device work is asynchronous on the context stream;
ctx.sync() or a read waits.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (ERROR_ALL_FINE, ERROR_DEVICE, ERROR_GPU_ALLOC_FAIL, ERROR_INVALID_FORMAT,  # noqa: F401
                   ERROR_INVALID_PARAMETER, ERROR_LOCK_FIRST, ERROR_NO_RENDER_TARGET, ERROR_NO_VERTICES,
                   ERROR_NOT_BUILT, ERROR_RT_CAM_MISMATCH, ERROR_UNLOCK_FIRST, MISS_PACKED, NO_TRIANGLE,
                   VERTEX_DATA_COUNT, VERTEX_DATA_NORMAL, VERTEX_DATA_POSITION, BeamError, BuildStats, Options,
                   SORT_LSD, SORT_MSD, SORT_MSD_SKEW, SORT_KD_RANKED,
                   VERTEX_DATA_UV1, VERTEX_DATA_UV2, VERTEX_DATA_TANGENT, VERTEX_DATA_BITANGENT, VERTEX_DATA_EXTRA1,
                   VERTEX_DATA_EXTRA2, VERTEX_DATA_EXTRA3, VERTEX_DATA_EXTRA4,
                   ATTR_GEOM_NORMAL, ATTR_MESH_FACE, ATTR_NORMALIZE, ATTR_MAX_REQS,
                   NORMALS_NORMALIZE)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def ray_filter_flags(cull=None, skip_tri=None, tmin=None, ray_mask=None) -> int:
    """The filter flag bits of a ray query: cull None, "back" or "front", and at most one meaning for the
    rays' pad word — skip_tri (a global triangle id never accepted), tmin (accept t > tmin) or ray_mask
    (accept entries whose mask shares a bit with it)."""
    culls = {None: 0, "back": _lib.RAYS_CULL_BACK, "front": _lib.RAYS_CULL_FRONT}
    if cull not in culls:
        raise BeamError(ERROR_INVALID_PARAMETER, 'cull: None, "back" or "front"')
    given = [f for v, f in ((skip_tri, _lib.RAYS_PAD_SKIP_TRI), (tmin, _lib.RAYS_PAD_TMIN),
                            (ray_mask, _lib.RAYS_PAD_MASK)) if v is not None]
    if len(given) > 1:
        raise BeamError(ERROR_INVALID_PARAMETER, "at most one of skip_tri, tmin and ray_mask: the pad word has one meaning")
    return culls[cull] | (given[0] if given else 0)


def ray_pad_words(n: int, skip_tri=None, tmin=None, ray_mask=None):
    """The pad column of n bm_ray records as uint32 for one of skip_tri (ids; -1 is NO_TRIANGLE), tmin (float32
    bits) and ray_mask, each a scalar or n values; None when none is given."""
    if tmin is not None:
        return np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, np.float32), (n,))).view(np.uint32)
    v = skip_tri if skip_tri is not None else ray_mask
    if v is None:
        return None
    a = np.asarray(v)
    if a.dtype.kind not in "iu":
        raise BeamError(ERROR_INVALID_PARAMETER, "skip_tri and ray_mask are integers")
    return np.ascontiguousarray(np.broadcast_to((a.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32), (n,)))


def _write_pad(rays, skip_tri=None, tmin=None, ray_mask=None) -> None:
    """Write the pad column of a packed (n,8) float32 torch tensor from torch tensors or host values, on the
    device and with the right bit pattern."""
    import torch
    n = rays.shape[0]
    col = rays.view(torch.int32)[:, 7]
    v = tmin if tmin is not None else skip_tri if skip_tri is not None else ray_mask
    if v is None:
        return
    if isinstance(v, torch.Tensor):
        if tmin is not None:
            rays[:, 7] = v.to(torch.float32)
        elif v.dtype == torch.int32:
            col[:] = v
        else:  # wider integers: the low 32 bits
            col[:] = (((v.to(torch.int64) & 0xFFFFFFFF) + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)
    else:
        words = ray_pad_words(n, skip_tri, tmin, ray_mask)
        col[:] = torch.from_numpy(words.view(np.int32).copy()).to(rays.device)


def _xform12(xform) -> np.ndarray:
    """An instance transform as 12 contiguous float32, row-major 3x4: from 12 floats, a (3,4) array, or a
    (4,4) array whose last row is exactly [0,0,0,1]. Anything else is a ValueError."""
    a = np.asarray(xform, dtype=np.float32)
    if a.shape == (4, 4):
        if not np.array_equal(a[3], np.array([0, 0, 0, 1], np.float32)):
            raise ValueError("xform: the last row of a (4,4) transform must be exactly [0,0,0,1]")
        a = a[:3]
    elif a.shape not in ((12,), (3, 4)):
        raise ValueError(f"xform: expected 12 floats, a (3,4) or a (4,4) array, got shape {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32).reshape(12)


def normal_matrix(xform) -> np.ndarray:
    """bm_xform_normal_matrix: the (3,3) cofactor matrix of the transform's linear part, the map an instance's
    normals go through (host only; include/beam_c.h has the formula)."""
    x = _xform12(xform)
    out = np.zeros(9, np.float32)
    err = _lib.load().bm_xform_normal_matrix(_fp(x), _fp(out))
    if err:
        raise BeamError(err, "bm_xform_normal_matrix")
    return out.reshape(3, 3)


def comm_unique_id() -> bytes:
    """Rank 0 of a multi-process context makes the RCCL unique id every rank passes as comm_id."""
    lib = _lib.load()
    buf = (C.c_uint8 * _lib.COMM_ID_BYTES)()
    err = lib.bm_comm_unique_id(buf)
    if err:
        raise BeamError(err, "bm_comm_unique_id: RCCL unavailable")
    return bytes(buf)


def ab_build() -> bool:
    """Whether the loaded library is an A/B build (tools/build_ab.py ... BM_TRACE_AB=1): the trace
    variants measured slower than the product kernels and BVH8 are compiled in (bm_version "+ab")."""
    return _lib.load().bm_version().decode().endswith("+ab")


def comm_available() -> None:
    """Raises BeamError unless RCCL resolves in this process (bm_comm_available): what every rank
    checks before any rank starts the communicator (multigpu.start_comm)."""
    err = _lib.load().bm_comm_available()
    if err:
        raise BeamError(err, "bm_comm_available: RCCL (librccl.so.1) unavailable")


_GATHER = {"auto": _lib.GATHER_AUTO, "peer": _lib.GATHER_PEER, "rccl": _lib.GATHER_RCCL}
_PLANES = {"packed": _lib.PLANE_PACKED, "tri_id": _lib.PLANE_TRI_ID, "t": _lib.PLANE_T, "nz": _lib.PLANE_NZ,
           "shadow": _lib.PLANE_SHADOW}


class Context:
    """One device + one HIP stream (bm_context), or a multi-GPU context:

    * devices=[d0, d1, ...] (one process): objects are replicated on every listed device and a trace
      deals 16-row screen bands round-robin to them, gathered into the render target on d0
      (gather "peer": xGMI writes from each device; "rccl": one RCCL communicator). Repeating a device
      rehearses the n-way path on one GPU.
    * comm=(rank, size, unique_id) (one process per GPU): this rank's bands, gathered into rank 0's
      render target over RCCL.
    planes: which planes the gather carries ("packed", "tri_id", "t", "nz", "shadow"; None = all).
    params: tuning parameters {name: value} (bm_context_set_param; names in _lib.PARAMS), set right
    after creation: measurement and test hooks, the defaults being the measured-best schedules."""

    def __init__(self, device: int = 0, stream: int | None = None, leaf_size: int = 4, shadow_queue: bool = False,
                 bvh_width: int = 4, reference_kd: bool = False, reference_hash: bool = False, devices=None,
                 band_height: int = 0, gather: str = "auto", planes=None, comm=None, params=None):
        self.lib = _lib.load()
        h = C.c_void_p()
        # stream=None: the context owns a stream; an int (0 = the null stream) is used as given
        flags = _lib.OPT_NULL_STREAM if stream == 0 else 0
        if shadow_queue:  # shadow rays as a separate wavefront pass (compaction study)
            flags |= _lib.OPT_SHADOW_QUEUE
        if bvh_width == 2:  # binary BVH (64-B records) instead of BVH4
            flags |= _lib.OPT_BVH2
        if bvh_width == 8:  # BVH8 (256-B records, three binary levels per node; quad kernel only)
            flags |= _lib.OPT_BVH8
        if reference_kd:  # the reference's own kd-tree + march: frames equal to the reference's
            flags |= _lib.OPT_REFERENCE_KD
        if reference_hash:  # the reference's hashed uniform grid (Hash.cu) + its cell march
            flags |= _lib.OPT_REFERENCE_HASH
        opts = Options(device, C.c_void_p(stream) if stream else None, leaf_size, flags)
        if devices:
            devices = list(devices)
            if len(devices) > _lib.MAX_DEVICES:
                raise BeamError(ERROR_INVALID_PARAMETER, f"at most {_lib.MAX_DEVICES} devices")
            opts.num_devices = len(devices)
            for i, d in enumerate(devices):
                opts.devices[i] = d
            device = devices[0]
        opts.band_height = band_height
        opts.gather = _GATHER[gather]
        opts.gather_planes = sum(_PLANES[p] for p in planes) if planes else 0
        if comm is not None:
            rank, size, uid = comm
            opts.comm_rank, opts.comm_size = rank, size
            C.memmove(opts.comm_id, bytes(uid), _lib.COMM_ID_BYTES)
        err = self.lib.bm_context_create(C.byref(opts), C.byref(h))
        if err:
            raise BeamError(err, f"bm_context_create(device={device}, devices={devices}, comm="
                                 f"{None if comm is None else comm[:2]}) failed")
        self.h = h
        self.device = device
        self.num_devices = int(self.lib.bm_context_num_devices(h))
        # the transport the library resolved: "peer", "rccl", "rccl-loopback" (a repeated device
        # list over one single-rank communicator) or None (one device)
        self.gather = {1: "peer", 2: "rccl", 3: "rccl-loopback"}.get(int(self.lib.bm_context_gather(h)))
        self.bvh_width = bvh_width if bvh_width in (2, 8) else 4
        for k, v in (params or {}).items():
            self.set_param(k, v)

    def set_param(self, name: str, value: int) -> None:
        """bm_context_set_param by name (_lib.PARAMS); -1 restores the library default."""
        if name not in _lib.PARAMS:
            raise BeamError(ERROR_INVALID_PARAMETER, f"unknown parameter {name!r}")
        self._check(self.lib.bm_context_set_param(self.h, _lib.PARAMS[name], int(value)))

    def get_param(self, name: str) -> int:
        """The value set for a parameter, -1 while the library default is in effect."""
        return int(self.lib.bm_context_get_param(self.h, _lib.PARAMS[name]))

    def start_comm(self, rank: int, size: int, unique_id: bytes) -> None:
        """Join the multi-process RCCL communicator (bm_context_start_comm) on a context created
        without one: the collective ncclCommInitRank, entered only after every rank's device context
        exists (multigpu.start_comm)."""
        uid = (C.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(bytes(unique_id)[:_lib.COMM_ID_BYTES])
        self._check(self.lib.bm_context_start_comm(self.h, rank, size, uid))
        self.num_devices = int(self.lib.bm_context_num_devices(self.h))
        self.gather = {1: "peer", 2: "rccl", 3: "rccl-loopback"}.get(int(self.lib.bm_context_gather(self.h)))

    def sync(self):
        self._check(self.lib.bm_sync(self.h))

    def debug_primitives(self, records):
        """bm_debug_primitives: the trace kernels' scalar primitives on float32 records [n, 36] ->
        [n, 12] (layouts in include/beam_c.h; tests/test_gpu_glm_pin.py)."""
        inp = np.ascontiguousarray(records, np.float32).reshape(-1, 36)
        out = np.zeros((inp.shape[0], 12), np.float32)
        self._check(self.lib.bm_debug_primitives(self.h, inp.shape[0], inp.ctypes.data, out.ctypes.data))
        return out

    @property
    def stream(self) -> int:
        return self.lib.bm_context_stream(self.h) or 0

    def last_error(self) -> str:
        return (self.lib.bm_last_error_string(self.h) or b"").decode()

    def _check(self, err):
        if err:
            raise BeamError(err, self.last_error())
        return err

    def close(self):
        if getattr(self, "h", None):
            self.lib.bm_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class IMesh:
    """Raytracer/Beam.h:47-54, Mesh.cpp."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.bm_mesh_create(ctx.h, C.byref(h)))
        self.h = h
        self._slot_comp = {}     # slot -> components, as uploaded (vertexData sizes its tensor by them)
        self._num_vertices = 0
        self._upload_keep = None

    @staticmethod
    def create(ctx: Context) -> "IMesh":
        return IMesh(ctx)

    def setVertexData(self, vertices, numVertices: int, numComponents: int, slotId: int, asyncCopy: bool = False):
        """A slot's values for every vertex (bm_mesh_set_vertex_data): host values, copied synchronously; returns
        the error code.

        A torch tensor on the context's device takes the device path (bm_mesh_set_vertex_data_device): the copy
        is enqueued on the context stream and nothing waits (unless the slot has to grow). The tensor is
        contiguous float32, shaped (numVertices, numComponents) or flat; anything else about it, and any error
        of the call, raises BeamError. Make the context on torch's stream
        (Context(stream=torch.cuda.current_stream().cuda_stream)) so that the simulation that wrote the tensor,
        this upload, computeNormals, refitGPUScene and the queries after it are ordered; the tensor may then be
        rewritten right after the call. The two forms may be mixed on one mesh."""
        import sys
        torch = sys.modules.get("torch")
        if torch is not None and isinstance(vertices, torch.Tensor):
            t = vertices
            dev = torch.device("cuda", self.ctx.device)
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"setVertexData: the tensor must be contiguous float32 on {dev} (the context's device)")
            if tuple(t.shape) not in ((numVertices, numComponents), (numVertices * numComponents,)):
                raise BeamError(ERROR_INVALID_PARAMETER,
                                "setVertexData: the tensor is (numVertices, numComponents) or flat")
            self.ctx._check(self.ctx.lib.bm_mesh_set_vertex_data_device(self.h, t.data_ptr(), numVertices,
                                                                        numComponents, slotId))
            self._upload_keep = t  # until the next upload: the copy may not have read it yet
            self._slot_comp[slotId] = numComponents
            self._num_vertices = numVertices
            return ERROR_ALL_FINE
        a = _f32(vertices).reshape(-1)
        if a.size < numVertices * numComponents:
            return ERROR_INVALID_PARAMETER
        err = self.ctx.lib.bm_mesh_set_vertex_data(self.h, _fp(a), numVertices, numComponents, slotId)
        if not err:
            self._slot_comp[slotId] = numComponents
            self._num_vertices = numVertices
        return err

    def computeNormals(self, normalize: bool = True) -> None:
        """bm_mesh_compute_normals: rewrites the NORMAL slot (creating it when absent) from the POSITION slot and
        the indices, on the context stream: smooth, area-weighted vertex normals, defined to the bit
        (include/beam_c.h). The first call after setIndices builds the vertex -> corner table and waits; later
        calls enqueue one launch. With the context on torch's stream the loop setVertexData(tensor),
        computeNormals(), refitGPUScene(), queries needs no synchronisation."""
        self.ctx._check(self.ctx.lib.bm_mesh_compute_normals(self.h, NORMALS_NORMALIZE if normalize else 0))
        self._slot_comp[VERTEX_DATA_NORMAL] = 3

    def vertexData(self, slotId: int):
        """The slot's current contents as a fresh (numVertices, numComponents) float32 torch tensor on the
        context's device (bm_mesh_copy_vertex_data_device): a device-to-device copy on the context stream, no
        host wait. Read it on the context's stream (or after ctx.sync())."""
        import torch
        if not 0 <= slotId < VERTEX_DATA_COUNT:
            raise BeamError(ERROR_INVALID_PARAMETER, "vertexData: unknown slot")
        comp = self._slot_comp.get(slotId, 0)  # as set through this object
        if not comp or not self._num_vertices:
            raise BeamError(ERROR_NO_VERTICES, "vertexData: the slot is empty")
        dev = torch.device("cuda", self.ctx.device)
        out = torch.empty((self._num_vertices, comp), dtype=torch.float32, device=dev)
        self.ctx._check(self.ctx.lib.bm_mesh_copy_vertex_data_device(self.h, slotId, out.data_ptr(),
                                                                     self._num_vertices, comp))
        return out

    def setIndices(self, indices, numIndices: int, asyncCopy: bool = False):
        a = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        if a.size < numIndices:
            return ERROR_INVALID_PARAMETER
        return self.ctx.lib.bm_mesh_set_indices(self.h, _up(a), numIndices)

    def destroy(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.bm_mesh_destroy(self.h)
        self.h = None


class IScene:
    """Raytracer/Beam.h:56-63, Scene.cpp / SceneTree.cpp (acceleration structure = LBVH)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.bm_scene_create(ctx.h, C.byref(h)))
        self.h = h
        self.meshes = []  # keep meshes alive (sptr semantics)
        self.last_stats = None

    @staticmethod
    def create(ctx: Context) -> "IScene":
        return IScene(ctx)

    def addMesh(self, mesh: IMesh):
        self.ctx._check(self.ctx.lib.bm_scene_add_mesh(self.h, mesh.h))
        self.meshes.append(mesh)

    def removeMesh(self, mesh: IMesh):
        self.ctx._check(self.ctx.lib.bm_scene_remove_mesh(self.h, mesh.h))
        self.meshes = [m for m in self.meshes if m is not mesh]

    def addInstance(self, mesh: IMesh, xform) -> int:
        """bm_scene_add_instance: the mesh placed by a 3x4 transform (12 floats, (3,4), or (4,4) with last row
        [0,0,0,1]) as one more entry of the scene; returns the entry's index (what ATTR_MESH_FACE reports)."""
        x = _xform12(xform)
        idx = C.c_uint32(0)
        self.ctx._check(self.ctx.lib.bm_scene_add_instance(self.h, mesh.h, _fp(x), C.byref(idx)))
        self.meshes.append(mesh)
        return int(idx.value)

    def setInstanceTransform(self, index: int, xform) -> None:
        """Replace an instance entry's matrix; it takes effect at the next updateGPUScene or refitGPUScene."""
        x = _xform12(xform)
        self.ctx._check(self.ctx.lib.bm_scene_set_instance_transform(self.h, index, _fp(x)))

    def instanceTransform(self, index: int) -> np.ndarray:
        """The matrix last set for an instance entry, (3,4) float32."""
        out = np.zeros(12, np.float32)
        self.ctx._check(self.ctx.lib.bm_scene_get_instance_transform(self.h, index, _fp(out)))
        return out.reshape(3, 4)

    def removeInstance(self, index: int) -> None:
        """Erase the entry at index (plain or instance); later entries move down by one."""
        self.ctx._check(self.ctx.lib.bm_scene_remove_instance(self.h, index))

    def setEntryMask(self, index: int, mask: int) -> None:
        """bm_scene_set_entry_mask: the 32-bit visibility mask of the entry at index, plain or instance (default
        0xFFFFFFFF). No rebuild: ray queries with ray_mask= enqueued after the call see it."""
        self.ctx._check(self.ctx.lib.bm_scene_set_entry_mask(self.h, index, mask & 0xFFFFFFFF))

    def getEntryMask(self, index: int) -> int:
        out = C.c_uint32(0)
        self.ctx._check(self.ctx.lib.bm_scene_get_entry_mask(self.h, index, C.byref(out)))
        return int(out.value)

    def updateGPUScene(self, stats: bool = False):
        """Rebuild the BVH from the current meshes (asynchronous unless stats=True)."""
        st = BuildStats()
        self.ctx._check(self.ctx.lib.bm_scene_build(self.h, C.byref(st) if stats else None))
        if stats:
            self.last_stats = {f: getattr(st, f) for f, _ in BuildStats._fields_}
            return self.last_stats
        return None

    def kdStats(self):
        """Reference mode: [leaves with faces, face refs stored, faces dropped (cap 256), largest leaf]."""
        out = np.zeros(4, np.uint64)
        self.ctx._check(self.ctx.lib.bm_scene_kd_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def kdExport(self):
        """Reference mode, for tests (bm_scene_kd_export): a dict of uint32 arrays — leaf_key, leaf_start,
        leaf_count [leaves] (count before the 256 cap), faces [pairs], and the radix tree lch, rch, first,
        last [leaves - 1] (a child with bit 31 set is a leaf index)."""
        lib, u32 = self.ctx.lib, C.POINTER(C.c_uint32)
        nl = int(self.kdStats()[0])
        m = C.c_uint64(0)
        self.ctx._check(lib.bm_scene_kd_export(self.h, C.byref(m), *([None] * 8)))
        sizes = {"leaf_key": nl, "leaf_start": nl, "leaf_count": nl, "faces": int(m.value),
                 "lch": max(nl - 1, 0), "rch": max(nl - 1, 0), "first": max(nl - 1, 0), "last": max(nl - 1, 0)}
        out = {k: np.zeros(max(1, n), np.uint32) for k, n in sizes.items()}
        self.ctx._check(lib.bm_scene_kd_export(self.h, None, *(out[k].ctypes.data_as(u32) for k in sizes)))
        return {k: out[k][:n] for k, n in sizes.items()}

    def gridStats(self):
        """Hashed-grid mode: [(cell, face) pairs, non-empty buckets, largest bucket, faces beyond
        the 256 cap]."""
        out = np.zeros(4, np.uint64)
        self.ctx._check(self.ctx.lib.bm_scene_grid_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def gridExport(self):
        """Hashed-grid mode: (bucket_start[65536], bucket_end[65536], faces[pairs])."""
        pairs = int(self.gridStats()[0])
        b0 = np.zeros(65536, np.uint32)
        b1 = np.zeros(65536, np.uint32)
        faces = np.zeros(max(1, pairs), np.uint32)
        u32 = C.POINTER(C.c_uint32)
        self.ctx._check(self.ctx.lib.bm_scene_grid_export(self.h, b0.ctypes.data_as(u32), b1.ctypes.data_as(u32),
                                                          faces.ctypes.data_as(u32)))
        return b0, b1, faces[:pairs]

    def refitGPUScene(self, stats: bool = False):
        """Refit-only update after vertex data changed (bm_scene_refit): same meshes and triangle
        counts as the last updateGPUScene; raises BeamError otherwise."""
        st = BuildStats()
        self.ctx._check(self.ctx.lib.bm_scene_refit(self.h, C.byref(st) if stats else None))
        if stats:
            self.last_stats = {f: getattr(st, f) for f, _ in BuildStats._fields_}
            return self.last_stats
        return None

    def traceRaysDevice(self, rays_ptr: int, n: int, out_ptr: int, any_hit: bool = False, counters=None,
                        mode=None, flags=0) -> int:
        """bm_scene_trace_rays on device pointers (n bm_ray records of 32 bytes in, n bm_hit records of
        16 bytes or n bytes out, both 16-byte aligned); returns the error code. Asynchronous on the
        context stream unless `counters` (a uint64[3] numpy array to fill) is given. mode overrides
        any_hit with a raw value; flags: 0 or filter bits (RAYS_CULL_*, RAYS_PAD_*: the records' pad words)."""
        mode = (_lib.RAYS_ANY_HIT if any_hit else _lib.RAYS_CLOSEST) if mode is None else mode
        rp, op = C.c_void_p(rays_ptr or None), C.c_void_p(out_ptr or None)
        if counters is None:
            return self.ctx.lib.bm_scene_trace_rays(self.h, rp, n, mode, flags, op)
        return self.ctx.lib.bm_scene_trace_rays_counters(self.h, rp, n, mode, flags, op,
                                                         counters.ctypes.data_as(C.POINTER(C.c_uint64)))

    def traceRays(self, origins, dirs=None, tmax=None, any_hit: bool = False, counters: bool = False, cull=None,
                  skip_tri=None, tmin=None, ray_mask=None, flags: int = 0):
        """Closest hit (or, any_hit, occlusion of the segment origin -> origin + dir) of n rays of the
        caller's own (bm_scene_trace_rays). tmax: None (unbounded), a scalar or n values; closest mode only.

        numpy (n,3) float32 origins and dirs: packs, uploads, traces and waits; returns numpy arrays
        {"t", "u", "v", "tri_id"} (a miss: t = inf, tri_id = NO_TRIANGLE) or {"occluded"}.
        torch tensors on the context's device — origins and dirs (n,3), or one packed (n,8) float32
        tensor (origin, tmax, dir, pad) as `origins` with dirs=None: everything stays on the device and
        nothing waits. Returns {"hits": (n,4) float32, "t", "u", "v", "tri_id"} (views of hits; tri_id its
        last column as int32, -1 on a miss) or {"occluded": (n,) uint8}. Make the context on torch's
        stream (Context(stream=torch.cuda.current_stream().cuda_stream)) so the query is ordered with
        the torch work around it.
        Filters: cull="back" / "front" accepts front-facing (back-facing) hits only; one of skip_tri (a global
        triangle id the ray never hits, e.g. the tri_id it starts on; -1 skips nothing), tmin (accept
        t > tmin, finite and >= 0) and ray_mask (accept entries whose setEntryMask mask shares a bit with it),
        each a scalar or n values (numpy, or torch on the device), goes into the rays' pad words. The packed
        (n,8) form carries its own pad column: pass the bits as flags= (RAYS_CULL_*, RAYS_PAD_*).
        counters=True adds "counters": [node records, triangle tests, hits or occluded rays] (waits)."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        on_device = isinstance(origins, torch.Tensor)
        packed_in = on_device and dirs is None
        if packed_in:
            if cull is not None or skip_tri is not None or tmin is not None or ray_mask is not None:
                raise BeamError(ERROR_INVALID_PARAMETER, "traceRays: packed rays carry their pad column; pass flags=")
        else:
            if flags:
                raise BeamError(ERROR_INVALID_PARAMETER, "traceRays: flags= goes with packed (n, 8) rays")
            flags = ray_filter_flags(cull, skip_tri, tmin, ray_mask)
        if on_device:
            if dirs is None:
                rays = origins
                if rays.dim() != 2 or rays.shape[1] != 8:
                    raise BeamError(ERROR_INVALID_PARAMETER, "traceRays: packed rays are (n, 8) float32")
            else:
                n = origins.shape[0]
                rays = torch.zeros((n, 8), dtype=torch.float32, device=origins.device)
                rays[:, 0:3] = origins
                rays[:, 3] = float("inf") if tmax is None else tmax
                rays[:, 4:7] = dirs
                _write_pad(rays, skip_tri, tmin, ray_mask)
            if rays.device != dev or rays.dtype != torch.float32 or not rays.is_contiguous():
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"traceRays: rays must be contiguous float32 on {dev} (the context's device)")
        else:
            o = _f32(origins).reshape(-1, 3)
            packed = np.zeros((o.shape[0], 8), np.float32)
            packed[:, 0:3] = o
            packed[:, 3] = np.inf if tmax is None else tmax
            packed[:, 4:7] = _f32(dirs).reshape(-1, 3)
            pad = ray_pad_words(o.shape[0], skip_tri, tmin, ray_mask)
            if pad is not None:
                packed.view(np.uint32)[:, 7] = pad
            rays = torch.from_numpy(packed).to(dev)
            torch.cuda.current_stream(dev).synchronize()  # the upload, before the context stream reads it
        n = rays.shape[0]
        out = (torch.empty((n,), dtype=torch.uint8, device=dev) if any_hit
               else torch.empty((n, 4), dtype=torch.float32, device=dev))
        cnt = np.zeros(3, np.uint64) if counters else None
        self.ctx._check(self.traceRaysDevice(rays.data_ptr() if n else 0, n, out.data_ptr() if n else 0, any_hit,
                                             cnt, flags=flags))
        self._rays_keep = rays  # until the next query: the kernel may not have read them yet
        if on_device:
            res = ({"occluded": out} if any_hit else
                   {"hits": out, "t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "tri_id": out.view(torch.int32)[:, 3]})
        else:
            self.ctx.sync()
            h = out.cpu().numpy()
            res = ({"occluded": h} if any_hit else
                   {"t": h[:, 0].copy(), "u": h[:, 1].copy(), "v": h[:, 2].copy(),
                    "tri_id": h.view(np.uint32)[:, 3].copy()})
        if counters:
            res["counters"] = cnt
        return res

    def traceRaysMultiDevice(self, rays_ptr: int, n: int, k: int, hits_ptr: int, counts_ptr: int = 0, flags: int = 0,
                             counters=None) -> int:
        """bm_scene_trace_rays_multi on device pointers (n bm_ray records of 32 bytes in, n * k bm_hit records
        of 16 bytes out, both 16-byte aligned; counts_ptr: n uint32, or 0); returns the error code.
        Asynchronous on the context stream unless `counters` (a uint64[3] numpy array to fill) is given.
        flags: MULTI_COUNT_ALL and the filter bits of traceRaysDevice, or 0."""
        rp, hp, cp = C.c_void_p(rays_ptr or None), C.c_void_p(hits_ptr or None), C.c_void_p(counts_ptr or None)
        if counters is None:
            return self.ctx.lib.bm_scene_trace_rays_multi(self.h, rp, n, k, flags, hp, cp)
        return self.ctx.lib.bm_scene_trace_rays_multi_counters(self.h, rp, n, k, flags, hp, cp,
                                                               counters.ctypes.data_as(C.POINTER(C.c_uint64)))

    def traceRaysMulti(self, origins, dirs=None, tmax=None, k: int = 4, count_all: bool = False,
                       counters: bool = False, cull=None, skip_tri=None, tmin=None, ray_mask=None, flags: int = 0):
        """The k nearest hits of each of n rays in (t, id) order (bm_scene_trace_rays_multi), k = 1..16, and
        per ray "count": the records that are hits, or with count_all every crossing within tmax (k may then
        be 0). Rays and tmax as for traceRays.

        numpy in: uploads, traces and waits; returns numpy arrays {"t", "u", "v", "tri_id"} of shape (n, k) (a
        miss slot: t = inf, tri_id = NO_TRIANGLE) and "count" (n,) uint32.
        torch tensors on the context's device: nothing waits. Returns {"hits": (n, k, 4) float32, "t", "u", "v",
        "tri_id" (views of hits, (n, k); tri_id as int32, -1 in a miss slot), "count": (n,) int32};
        res["hits"].view(-1, 4) goes straight into hitAttributes as n * k hits.
        Filters (cull, skip_tri, tmin, ray_mask; flags= with packed rays, beside count_all) as for traceRays.
        counters=True adds "counters": [node records, triangle tests, the sum of the counts] (waits)."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        on_device = isinstance(origins, torch.Tensor)
        if on_device and dirs is None:
            if cull is not None or skip_tri is not None or tmin is not None or ray_mask is not None:
                raise BeamError(ERROR_INVALID_PARAMETER, "traceRaysMulti: packed rays carry their pad column; pass flags=")
        else:
            if flags:
                raise BeamError(ERROR_INVALID_PARAMETER, "traceRaysMulti: flags= goes with packed (n, 8) rays")
            flags = ray_filter_flags(cull, skip_tri, tmin, ray_mask)
        if on_device:
            if dirs is None:
                rays = origins
                if rays.dim() != 2 or rays.shape[1] != 8:
                    raise BeamError(ERROR_INVALID_PARAMETER, "traceRaysMulti: packed rays are (n, 8) float32")
            else:
                rays = torch.zeros((origins.shape[0], 8), dtype=torch.float32, device=origins.device)
                rays[:, 0:3] = origins
                rays[:, 3] = float("inf") if tmax is None else tmax
                rays[:, 4:7] = dirs
                _write_pad(rays, skip_tri, tmin, ray_mask)
            if rays.device != dev or rays.dtype != torch.float32 or not rays.is_contiguous():
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"traceRaysMulti: rays must be contiguous float32 on {dev} (the context's device)")
        else:
            o = _f32(origins).reshape(-1, 3)
            packed = np.zeros((o.shape[0], 8), np.float32)
            packed[:, 0:3] = o
            packed[:, 3] = np.inf if tmax is None else tmax
            packed[:, 4:7] = _f32(dirs).reshape(-1, 3)
            pad = ray_pad_words(o.shape[0], skip_tri, tmin, ray_mask)
            if pad is not None:
                packed.view(np.uint32)[:, 7] = pad
            rays = torch.from_numpy(packed).to(dev)
            torch.cuda.current_stream(dev).synchronize()  # the upload, before the context stream reads it
        n = rays.shape[0]
        out = torch.empty((n, k, 4), dtype=torch.float32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        cnt = np.zeros(3, np.uint64) if counters else None
        self.ctx._check(self.traceRaysMultiDevice(rays.data_ptr() if n else 0, n, k, out.data_ptr() if n and k else 0,
                                                  count.data_ptr() if n else 0,
                                                  (_lib.MULTI_COUNT_ALL if count_all else 0) | flags, cnt))
        self._rays_keep = rays  # until the next query: the kernel may not have read them yet
        if on_device:
            res = {"hits": out, "t": out[..., 0], "u": out[..., 1], "v": out[..., 2],
                   "tri_id": out.view(torch.int32)[..., 3], "count": count}
        else:
            self.ctx.sync()
            h = out.cpu().numpy()
            res = {"t": h[..., 0].copy(), "u": h[..., 1].copy(), "v": h[..., 2].copy(),
                   "tri_id": h.view(np.uint32)[..., 3].copy(), "count": count.cpu().numpy().view(np.uint32)}
        if counters:
            res["counters"] = cnt
        return res

    def closestPointsMultiDevice(self, points_ptr: int, n: int, k: int, hits_ptr: int, counts_ptr: int = 0,
                                 flags: int = 0, counters=None) -> int:
        """bm_scene_closest_points_multi on device pointers (n bm_point records of 16 bytes in, n * k bm_hit
        records of 16 bytes out, both 16-byte aligned; counts_ptr: n uint32, or 0); returns the error code.
        Asynchronous on the context stream unless `counters` (a uint64[4] numpy array to fill) is given.
        flags: MULTI_COUNT_ALL or 0."""
        pp, hp, cp = C.c_void_p(points_ptr or None), C.c_void_p(hits_ptr or None), C.c_void_p(counts_ptr or None)
        if counters is None:
            return self.ctx.lib.bm_scene_closest_points_multi(self.h, pp, n, k, flags, hp, cp)
        return self.ctx.lib.bm_scene_closest_points_multi_counters(self.h, pp, n, k, flags, hp, cp,
                                                                   counters.ctypes.data_as(C.POINTER(C.c_uint64)))

    def closestPointsMulti(self, points, rmax=None, k: int = 4, count_all: bool = False, counters: bool = False):
        """The k nearest triangles within rmax of each of n points in (distance, id) order
        (bm_scene_closest_points_multi), k = 1..16, and per point "count": the records written, or with
        count_all every triangle within rmax (k may then be 0). Points and rmax as for closestPoints.

        numpy in: uploads, queries and waits; returns numpy arrays {"t", "u", "v", "tri_id"} of shape (n, k) (a
        miss slot: t = inf, tri_id = NO_TRIANGLE) and "count" (n,) uint32.
        torch tensors on the context's device: nothing waits. Returns {"hits": (n, k, 4) float32, "t", "u", "v",
        "tri_id" (views of hits, (n, k); tri_id as int32, -1 in a miss slot), "count": (n,) int32};
        res["hits"].view(-1, 4) goes straight into hitAttributes as n * k hits.
        counters=True adds "counters": [node records, triangle evaluations, the sum of the counts, deepest
        stack] (waits)."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        on_device = isinstance(points, torch.Tensor)
        if on_device:
            if points.dim() == 2 and points.shape[1] == 4 and rmax is None:
                pts = points
            elif points.dim() == 2 and points.shape[1] == 3:
                pts = torch.empty((points.shape[0], 4), dtype=torch.float32, device=points.device)
                pts[:, 0:3] = points
                pts[:, 3] = float("inf") if rmax is None else rmax
            else:
                raise BeamError(ERROR_INVALID_PARAMETER,
                                "closestPointsMulti: points are (n, 3), or packed (n, 4), float32")
            if pts.device != dev or pts.dtype != torch.float32 or not pts.is_contiguous():
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"closestPointsMulti: points must be contiguous float32 on {dev} (the context's device)")
        else:
            q = _f32(points).reshape(-1, 3)
            packed = np.zeros((q.shape[0], 4), np.float32)
            packed[:, 0:3] = q
            packed[:, 3] = np.inf if rmax is None else rmax
            pts = torch.from_numpy(packed).to(dev)
            torch.cuda.current_stream(dev).synchronize()  # the upload, before the context stream reads it
        n = pts.shape[0]
        out = torch.empty((n, k, 4), dtype=torch.float32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        cnt = np.zeros(4, np.uint64) if counters else None
        self.ctx._check(self.closestPointsMultiDevice(pts.data_ptr() if n else 0, n, k,
                                                      out.data_ptr() if n and k else 0, count.data_ptr() if n else 0,
                                                      _lib.MULTI_COUNT_ALL if count_all else 0, cnt))
        self._points_keep = pts  # until the next query: the kernel may not have read them yet
        if on_device:
            res = {"hits": out, "t": out[..., 0], "u": out[..., 1], "v": out[..., 2],
                   "tri_id": out.view(torch.int32)[..., 3], "count": count}
        else:
            self.ctx.sync()
            h = out.cpu().numpy()
            res = {"t": h[..., 0].copy(), "u": h[..., 1].copy(), "v": h[..., 2].copy(),
                   "tri_id": h.view(np.uint32)[..., 3].copy(), "count": count.cpu().numpy().view(np.uint32)}
        if counters:
            res["counters"] = cnt
        return res

    def overlapBoxesDevice(self, boxes_ptr: int, n: int, mode: int, out_ptr: int, offsets_ptr: int = 0,
                           ids_ptr: int = 0, flags: int = 0, counters=None) -> int:
        """bm_scene_overlap_boxes on device pointers (n bm_box records of 32 bytes in, 16-byte aligned; out_ptr:
        n uint32 for BOXES_COUNT and BOXES_LIST (there it may be 0), n bytes for BOXES_ANY; BOXES_LIST:
        offsets_ptr n + 1 uint32, ids_ptr the id segments); returns the error code. Asynchronous on the
        context stream unless `counters` (a uint64[4] numpy array to fill) is given. flags: none defined yet."""
        bp, op = C.c_void_p(boxes_ptr or None), C.c_void_p(out_ptr or None)
        fp, ip = C.c_void_p(offsets_ptr or None), C.c_void_p(ids_ptr or None)
        if counters is None:
            return self.ctx.lib.bm_scene_overlap_boxes(self.h, bp, n, mode, flags, op, fp, ip)
        return self.ctx.lib.bm_scene_overlap_boxes_counters(self.h, bp, n, mode, flags, op, fp, ip,
                                                            counters.ctypes.data_as(C.POINTER(C.c_uint64)))

    def overlapBoxes(self, centers, halves=None, mode: str = "count", counters: bool = False):
        """The triangles that intersect each of n axis-aligned boxes (bm_scene_overlap_boxes): a triangle is in
        a box's set when the reference's triangle/box test accepts it, faces inclusive. centers (n,3) and halves
        (n,3) (or one (3,) half-size for all), or one packed (n,8) float32 array (centre, pad, half, pad).

        mode "count": {"count": (n,)} the number of triangles per box. mode "any": {"any": (n,) bool}.
        mode "list": the count pass, torch.cumsum of the counts into offsets on the device, one read of the
        total to size ids, then the list pass: {"count": (n,), "offsets": (n + 1,), "ids": (total,)} with box
        i's triangle ids in ids[offsets[i]:offsets[i + 1]], in traversal order (the same on every call).

        numpy in: uploads, queries and waits; returns numpy arrays (uint32; "any" bool).
        torch tensors on the context's device: everything stays on the device (int32; "any" bool); "list"
        waits once, for the total. Make the context on torch's stream, as for traceRays.
        counters=True adds "counters": [node records, triangle tests, the sum of the counts (any: boxes with a
        hit), deepest stack] of the last pass (waits)."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        modes = {"count": _lib.BOXES_COUNT, "any": _lib.BOXES_ANY, "list": _lib.BOXES_LIST}
        if mode not in modes:
            raise BeamError(ERROR_INVALID_PARAMETER, 'overlapBoxes: mode is "count", "any" or "list"')
        on_device = isinstance(centers, torch.Tensor)
        if on_device:
            if centers.dim() == 2 and centers.shape[1] == 8 and halves is None:
                boxes = centers
            elif centers.dim() == 2 and centers.shape[1] == 3 and halves is not None:
                boxes = torch.zeros((centers.shape[0], 8), dtype=torch.float32, device=centers.device)
                boxes[:, 0:3] = centers
                boxes[:, 4:7] = halves
            else:
                raise BeamError(ERROR_INVALID_PARAMETER,
                                "overlapBoxes: centers (n, 3) with halves, or packed (n, 8), float32")
            if boxes.device != dev or boxes.dtype != torch.float32 or not boxes.is_contiguous():
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"overlapBoxes: boxes must be contiguous float32 on {dev} (the context's device)")
        else:
            a = _f32(centers)
            if halves is None:
                packed = np.ascontiguousarray(a.reshape(-1, 8))
            else:
                ctr = a.reshape(-1, 3)
                packed = np.zeros((ctr.shape[0], 8), np.float32)
                packed[:, 0:3] = ctr
                packed[:, 4:7] = _f32(halves).reshape(-1, 3)
            boxes = torch.from_numpy(packed).to(dev)
            torch.cuda.current_stream(dev).synchronize()  # the upload, before the context stream reads it
        n = boxes.shape[0]
        bptr = boxes.data_ptr() if n else 0
        cnt = np.zeros(4, np.uint64) if counters else None
        if mode == "any":
            out = torch.empty((n,), dtype=torch.uint8, device=dev)
            self.ctx._check(self.overlapBoxesDevice(bptr, n, _lib.BOXES_ANY, out.data_ptr() if n else 0, counters=cnt))
            res = {"any": out.view(torch.bool)}
        else:
            count = torch.empty((n,), dtype=torch.int32, device=dev)
            if mode == "count":
                self.ctx._check(self.overlapBoxesDevice(bptr, n, _lib.BOXES_COUNT, count.data_ptr() if n else 0,
                                                        counters=cnt))
                res = {"count": count}
            else:
                self.ctx._check(self.overlapBoxesDevice(bptr, n, _lib.BOXES_COUNT, count.data_ptr() if n else 0))
                if not on_device:
                    self.ctx.sync()  # the counts, before torch's stream reads them
                offsets = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
                torch.cumsum(count, 0, dtype=torch.int32, out=offsets[1:])
                total = int(offsets[-1].item())  # the one read; it also puts the offsets before the list pass
                ids = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)  # never a null pointer
                self.ctx._check(self.overlapBoxesDevice(bptr, n, _lib.BOXES_LIST, 0, offsets.data_ptr(),
                                                        ids.data_ptr(), counters=cnt))
                res = {"count": count, "offsets": offsets, "ids": ids[:total]}
        self._boxes_keep = boxes  # until the next query: the kernel may not have read them yet
        if not on_device:
            self.ctx.sync()
            res = {k: (v.cpu().numpy() if k == "any" else v.cpu().numpy().view(np.uint32)) for k, v in res.items()}
        if counters:
            res["counters"] = cnt
        return res

    def voxelize(self, lo, hi, dims):
        """Occupancy of a regular grid: a bool tensor of shape dims = (nx, ny, nz) on the context's device, True
        where a triangle intersects the cell (overlapBoxes mode "any" over the grid's cells; the cells are made
        on torch's current stream, which is waited for before the query goes onto the context stream; the
        result is written in context-stream order: make the context on torch's stream, as for traceRays, or
        call Context.sync() before reading it).
        The cells, in float32 (numpy statements; every operation rounds once):
            lo32, hi32 = np.float32(lo), np.float32(hi)
            cell = (hi32 - lo32) / np.float32(dims)                              # (3,)
            half = np.float32(0.5) * cell                                        # (3,), every cell's half-size
            centre[i, j, k] = lo32 + (np.float32((i, j, k)) + np.float32(0.5)) * cell
        Cell (i, j, k) is box (i * ny + j) * nz + k of the batch."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 1:
            raise BeamError(ERROR_INVALID_PARAMETER, "voxelize: dims is three positive integers")
        lo32, hi32 = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        cell = (hi32 - lo32) / np.asarray(dims, np.float32)
        half = np.float32(0.5) * cell
        n = dims[0] * dims[1] * dims[2]
        boxes = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        grid = boxes.view(dims[0], dims[1], dims[2], 8)
        for a in range(3):  # one multiply and one add per component, as the statements above
            idx = torch.arange(dims[a], dtype=torch.float32, device=dev)
            axis = float(lo32[a]) + (idx + 0.5) * float(cell[a])
            shape = [1, 1, 1]
            shape[a] = dims[a]
            grid[..., a] = axis.view(shape)
            grid[..., 4 + a] = float(half[a])
        torch.cuda.current_stream(dev).synchronize()  # the cells, before the context stream reads them
        return self.overlapBoxes(boxes, mode="any")["any"].view(dims)

    def overlapTrianglesDevice(self, tris_ptr: int, n: int, mode: int, out_ptr: int, offsets_ptr: int = 0,
                               ids_ptr: int = 0, flags: int = 0, counters=None) -> int:
        """bm_scene_overlap_triangles on device pointers (n bm_tri records of 48 bytes in, 16-byte aligned;
        out_ptr: n uint32 for TRIS_COUNT and TRIS_LIST (there it may be 0), n bytes for TRIS_ANY; TRIS_LIST:
        offsets_ptr n + 1 uint32, ids_ptr the id segments); returns the error code. Asynchronous on the context
        stream unless `counters` (a uint64[4] numpy array to fill) is given. flags: 0 or TRIS_PAD_SKIP_TRI."""
        tp, op = C.c_void_p(tris_ptr or None), C.c_void_p(out_ptr or None)
        fp, ip = C.c_void_p(offsets_ptr or None), C.c_void_p(ids_ptr or None)
        if counters is None:
            return self.ctx.lib.bm_scene_overlap_triangles(self.h, tp, n, mode, flags, op, fp, ip)
        return self.ctx.lib.bm_scene_overlap_triangles_counters(self.h, tp, n, mode, flags, op, fp, ip,
                                                                counters.ctypes.data_as(C.POINTER(C.c_uint64)))

    def overlapTriangles(self, tris, mode: str = "count", skip_tri=None, counters: bool = False):
        """The scene triangles that intersect each of n query triangles (bm_scene_overlap_triangles): a scene
        triangle is in a query's set when the header's triangle/triangle test accepts the pair, touching
        included. tris: (n, 3, 3) vertex positions, or packed (n, 12) float32 bm_tri records (v0, pad0, v1,
        pad1, v2, pad2). skip_tri: None, or n triangle ids (one per query) that are never reported — each
        triangle's own id when a mesh is queried against itself; 0xFFFFFFFF (-1) skips nothing. With packed
        records and skip_tri=True the records' own pad0 words are the ids.

        Modes, results, numpy and torch behaviour and `counters` exactly as overlapBoxes: "count" {"count"},
        "any" {"any"}, "list" {"count", "offsets", "ids"} after a count pass and torch.cumsum on the device."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        modes = {"count": _lib.TRIS_COUNT, "any": _lib.TRIS_ANY, "list": _lib.TRIS_LIST}
        if mode not in modes:
            raise BeamError(ERROR_INVALID_PARAMETER, 'overlapTriangles: mode is "count", "any" or "list"')
        on_device = isinstance(tris, torch.Tensor)
        own_pad = skip_tri is True
        if on_device:
            if tris.device != dev or tris.dtype != torch.float32:
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"overlapTriangles: tris must be float32 on {dev} (the context's device)")
            if tris.dim() == 2 and tris.shape[1] == 12 and tris.is_contiguous() and (skip_tri is None or own_pad):
                rec = tris
            elif (tris.dim() == 3 and tris.shape[1:] == (3, 3)) or (tris.dim() == 2 and tris.shape[1] == 12):
                rec = torch.zeros((tris.shape[0], 12), dtype=torch.float32, device=dev)
                rec.view(-1, 3, 4)[:, :, 0:3] = tris if tris.dim() == 3 else tris.view(-1, 3, 4)[:, :, 0:3]
            else:
                raise BeamError(ERROR_INVALID_PARAMETER, "overlapTriangles: tris (n, 3, 3), or packed (n, 12)")
            if skip_tri is not None and not own_pad:
                sk = skip_tri if isinstance(skip_tri, torch.Tensor) else torch.from_numpy(
                    np.ascontiguousarray(skip_tri).astype(np.int64).astype(np.uint32).view(np.int32))
                rec.view(torch.int32)[:, 3] = sk.to(device=dev, dtype=torch.int32).reshape(-1)
        else:
            a = _f32(tris)
            if a.ndim == 2 and a.shape[1] == 12:
                packed = np.ascontiguousarray(a).copy()
            else:
                packed = np.zeros((a.reshape(-1, 3, 3).shape[0], 12), np.float32)
                packed.reshape(-1, 3, 4)[:, :, 0:3] = a.reshape(-1, 3, 3)
            if skip_tri is not None and not own_pad:
                packed.view(np.uint32)[:, 3] = np.asarray(skip_tri).astype(np.int64).astype(np.uint32).reshape(-1)
            rec = torch.from_numpy(packed).to(dev)
            torch.cuda.current_stream(dev).synchronize()  # the upload, before the context stream reads it
        flags = _lib.TRIS_PAD_SKIP_TRI if skip_tri is not None else 0
        n = rec.shape[0]
        tptr = rec.data_ptr() if n else 0
        cnt = np.zeros(4, np.uint64) if counters else None
        if mode == "any":
            out = torch.empty((n,), dtype=torch.uint8, device=dev)
            self.ctx._check(self.overlapTrianglesDevice(tptr, n, _lib.TRIS_ANY, out.data_ptr() if n else 0, flags=flags,
                                                        counters=cnt))
            res = {"any": out.view(torch.bool)}
        else:
            count = torch.empty((n,), dtype=torch.int32, device=dev)
            if mode == "count":
                self.ctx._check(self.overlapTrianglesDevice(tptr, n, _lib.TRIS_COUNT, count.data_ptr() if n else 0,
                                                            flags=flags, counters=cnt))
                res = {"count": count}
            else:
                self.ctx._check(self.overlapTrianglesDevice(tptr, n, _lib.TRIS_COUNT, count.data_ptr() if n else 0,
                                                            flags=flags))
                if not on_device:
                    self.ctx.sync()  # the counts, before torch's stream reads them
                offsets = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
                torch.cumsum(count, 0, dtype=torch.int32, out=offsets[1:])
                total = int(offsets[-1].item())  # the one read; it also puts the offsets before the list pass
                ids = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)  # never a null pointer
                self.ctx._check(self.overlapTrianglesDevice(tptr, n, _lib.TRIS_LIST, 0, offsets.data_ptr(),
                                                            ids.data_ptr(), flags=flags, counters=cnt))
                res = {"count": count, "offsets": offsets, "ids": ids[:total]}
        self._tris_keep = rec  # until the next query: the kernel may not have read them yet
        if not on_device:
            self.ctx.sync()
            res = {k: (v.cpu().numpy() if k == "any" else v.cpu().numpy().view(np.uint32)) for k, v in res.items()}
        if counters:
            res["counters"] = cnt
        return res

    def selfIntersections(self, shared=None, indices=None):
        """The pairs of scene triangles that intersect each other: an (m, 2) int64 numpy array of global
        triangle ids, i < j per row, rows in ascending order.

        The scene is queried with its own triangles in list mode, each reconstructed from export()'s records
        (v0, v0 + e1, v0 + e2: the same bits the scene side of the test uses) and carrying its own id in pad0
        under TRIS_PAD_SKIP_TRI. The translated test is not bit-symmetric in its arguments, so a pair is
        reported when either direction accepts it: the union is the definition.

        Neighbours in a mesh touch by construction. Pairs for which shared(i, j) is true are left out.
        shared=None: "the two triangles belong to the same scene entry and have a vertex index in common",
        from hitAttributes(ATTR_MESH_FACE) and the entries' index arrays. IScene does not keep index arrays,
        so the caller passes them: indices is one array of 3 * faces indices per scene entry, in entry order
        (an instance entry: its mesh's). A callable `shared` needs no indices; it is called once per
        intersecting pair with (i, j), i < j. Waits for the result."""
        if shared is None and indices is None:
            raise BeamError(ERROR_INVALID_PARAMETER,
                            "selfIntersections: pass the entries' index arrays (indices=[...]) or a shared(i, j)")
        _, tris, _, _ = self.export()
        n = tris.shape[0]
        if n == 0:
            return np.zeros((0, 2), np.int64)
        tf, gid = tris.view(np.float32), tris[:, 3]
        v0 = tf[:, 0:3]
        q = np.zeros((n, 3, 3), np.float32)
        q[gid] = np.stack([v0, v0 + tf[:, 4:7], v0 + tf[:, 8:11]], axis=1)
        res = self.overlapTriangles(q, mode="list", skip_tri=np.arange(n, dtype=np.uint32))
        i = np.repeat(np.arange(n, dtype=np.int64), res["count"].astype(np.int64))
        j = res["ids"].astype(np.int64)
        pairs = np.unique(np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1), axis=0).reshape(-1, 2)
        if pairs.shape[0] == 0:
            return pairs
        if shared is not None:
            keep = np.array([not shared(int(a), int(b)) for a, b in pairs], bool)
            return pairs[keep]
        hits = np.zeros((n, 4), np.float32)
        hits.view(np.uint32)[:, 3] = np.arange(n, dtype=np.uint32)
        (face,) = self.hitAttributes(hits, [(ATTR_MESH_FACE, 2)])
        vidx = np.zeros((n, 3), np.int64)
        for e, idx in enumerate(indices):
            mine = face[:, 0] == e
            vidx[mine] = np.asarray(idx, np.int64).reshape(-1, 3)[face[mine, 1]]
        a, b = pairs[:, 0], pairs[:, 1]
        touch = (face[a, 0] == face[b, 0]) & (vidx[a][:, :, None] == vidx[b][:, None, :]).any(axis=(1, 2))
        return pairs[~touch]

    def sectionPlanesDevice(self, planes_ptr: int, n: int, mode: int, out_ptr: int, offsets_ptr: int = 0,
                            ids_ptr: int = 0, segs_ptr: int = 0, flags: int = 0, counters=None) -> int:
        """bm_scene_section_planes on device pointers (n bm_plane records of 32 bytes in, 16-byte aligned; out_ptr:
        n uint32 for PLANES_COUNT and PLANES_LIST (there it may be 0), n bytes for PLANES_ANY; PLANES_LIST:
        offsets_ptr n + 1 uint32, and at least one of ids_ptr (uint32 per slot) and segs_ptr (a 32-byte bm_segment
        per slot, 16-byte aligned)); returns the error code. Asynchronous on the context stream unless `counters`
        (a uint64[4] numpy array to fill) is given. flags: none defined yet."""
        pp, op = C.c_void_p(planes_ptr or None), C.c_void_p(out_ptr or None)
        fp, ip, sp = C.c_void_p(offsets_ptr or None), C.c_void_p(ids_ptr or None), C.c_void_p(segs_ptr or None)
        if counters is None:
            return self.ctx.lib.bm_scene_section_planes(self.h, pp, n, mode, flags, op, fp, ip, sp)
        return self.ctx.lib.bm_scene_section_planes_counters(self.h, pp, n, mode, flags, op, fp, ip, sp,
                                                             counters.ctypes.data_as(C.POINTER(C.c_uint64)))

    def sectionPlanes(self, points, normals=None, mode: str = "count", counters: bool = False):
        """The triangles each of n planes crosses, and where it cuts them (bm_scene_section_planes). Plane i passes
        through points[i] and is perpendicular to normals[i] (any length). A triangle is crossed when, on its
        mesh's own vertices, s(x) = (n.x*d.x + n.y*d.y) + n.z*d.z with d = x - point is negative for at least one
        vertex and not negative for at least one: a vertex on the plane counts as above. points (n,3) and
        normals (n,3) (or one (3,) normal for all), or one packed (n,8) float32 array (point, pad, normal, pad).

        mode "count": {"count": (n,)} the number of crossed triangles per plane. mode "any": {"any": (n,) bool}.
        mode "list": the count pass, torch.cumsum of the counts into offsets on the device, one read of the total,
        then the list pass: {"count": (n,), "offsets": (n + 1,), "ids": (total,)} with plane i's triangle ids in
        ids[offsets[i]:offsets[i + 1]], in traversal order (the same on every call).
        mode "segments": the same two passes, the list pass writing the cut segments as well; returns the tuple
        (offsets (n + 1,), ids (total,), a (total, 3), b (total, 3)): slot j's triangle ids[j] is cut from a[j]
        (on its edge running from above to below) to b[j] (on its edge running from below to above). The two
        triangles on a mesh edge compute the same bits for its cut, so on a closed mesh chainSegments(a, b) of a
        plane's slots gives closed loops.

        numpy in: uploads, queries and waits; returns numpy arrays (uint32, float32; "any" bool).
        torch tensors on the context's device: everything stays on the device (int32, float32; "any" bool);
        "list" and "segments" wait once, for the total. Make the context on torch's stream, as for traceRays.
        counters=True adds "counters": [node records, triangle tests, the sum of the counts (any: planes with a
        crossing), deepest stack] of the last pass (waits); with "segments" it is a fifth tuple element."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        modes = {"count": _lib.PLANES_COUNT, "any": _lib.PLANES_ANY, "list": _lib.PLANES_LIST,
                 "segments": _lib.PLANES_LIST}
        if mode not in modes:
            raise BeamError(ERROR_INVALID_PARAMETER, 'sectionPlanes: mode is "count", "any", "list" or "segments"')
        on_device = isinstance(points, torch.Tensor)
        if on_device:
            if points.dim() == 2 and points.shape[1] == 8 and normals is None:
                planes = points
            elif points.dim() == 2 and points.shape[1] == 3 and normals is not None:
                planes = torch.zeros((points.shape[0], 8), dtype=torch.float32, device=points.device)
                planes[:, 0:3] = points
                planes[:, 4:7] = normals if isinstance(normals, torch.Tensor) else torch.from_numpy(
                    np.ascontiguousarray(np.broadcast_to(_f32(normals).reshape(-1, 3), (points.shape[0], 3)))).to(dev)
            else:
                raise BeamError(ERROR_INVALID_PARAMETER,
                                "sectionPlanes: points (n, 3) with normals, or packed (n, 8), float32")
            if planes.device != dev or planes.dtype != torch.float32 or not planes.is_contiguous():
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"sectionPlanes: planes must be contiguous float32 on {dev} (the context's device)")
        else:
            a = _f32(points)
            if normals is None:
                packed = np.ascontiguousarray(a.reshape(-1, 8))
            else:
                pts = a.reshape(-1, 3)
                packed = np.zeros((pts.shape[0], 8), np.float32)
                packed[:, 0:3] = pts
                packed[:, 4:7] = _f32(normals).reshape(-1, 3)  # one normal broadcasts over the rows
            planes = torch.from_numpy(packed).to(dev)
            torch.cuda.current_stream(dev).synchronize()  # the upload, before the context stream reads it
        n = planes.shape[0]
        pptr = planes.data_ptr() if n else 0
        cnt = np.zeros(4, np.uint64) if counters else None
        if mode == "any":
            out = torch.empty((n,), dtype=torch.uint8, device=dev)
            self.ctx._check(self.sectionPlanesDevice(pptr, n, _lib.PLANES_ANY, out.data_ptr() if n else 0, counters=cnt))
            res = {"any": out.view(torch.bool)}
        else:
            count = torch.empty((n,), dtype=torch.int32, device=dev)
            if mode == "count":
                self.ctx._check(self.sectionPlanesDevice(pptr, n, _lib.PLANES_COUNT, count.data_ptr() if n else 0,
                                                         counters=cnt))
                res = {"count": count}
            else:
                self.ctx._check(self.sectionPlanesDevice(pptr, n, _lib.PLANES_COUNT, count.data_ptr() if n else 0))
                if not on_device:
                    self.ctx.sync()  # the counts, before torch's stream reads them
                offsets = torch.zeros((n + 1,), dtype=torch.int32, device=dev)
                torch.cumsum(count, 0, dtype=torch.int32, out=offsets[1:])
                total = int(offsets[-1].item())  # the one read; it also puts the offsets before the list pass
                ids = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)  # never a null pointer
                segs = torch.empty((max(total, 1), 8), dtype=torch.float32, device=dev) if mode == "segments" else None
                self.ctx._check(self.sectionPlanesDevice(pptr, n, _lib.PLANES_LIST, 0, offsets.data_ptr(), ids.data_ptr(),
                                                         segs.data_ptr() if segs is not None else 0, counters=cnt))
                res = {"count": count, "offsets": offsets, "ids": ids[:total]}
                if segs is not None:
                    res["a"], res["b"] = segs[:total, 0:3], segs[:total, 4:7]
        self._planes_keep = planes  # until the next query: the kernel may not have read them yet
        if not on_device:
            self.ctx.sync()
            res = {k: (v.cpu().numpy() if k in ("any", "a", "b") else v.cpu().numpy().view(np.uint32))
                   for k, v in res.items()}
            if mode == "segments":
                res["a"], res["b"] = np.ascontiguousarray(res["a"]), np.ascontiguousarray(res["b"])
        if mode == "segments":
            out = (res["offsets"], res["ids"], res["a"], res["b"])
            return out + (cnt,) if counters else out
        if counters:
            res["counters"] = cnt
        return res

    def sliceStack(self, origin, normal, heights, mode: str = "segments", counters: bool = False):
        """A stack of parallel sections, the layers of a slicer: sectionPlanes over the planes with the one
        `normal` (3,), plane i through the point, in float32 (numpy statements; every operation rounds once):
            o32, n32, h32 = np.float32(origin), np.float32(normal), np.float32(heights)
            point[i] = o32 + h32[i] * n32                                        # per component
        heights: n numbers (a unit normal makes them distances along it). Returns what sectionPlanes returns for
        `mode` with numpy input: for "segments" the tuple (offsets, ids, a, b) as numpy arrays."""
        o32, n32 = np.asarray(origin, np.float32).reshape(3), np.asarray(normal, np.float32).reshape(3)
        h32 = np.asarray(heights, np.float32).reshape(-1)
        pts = o32[None, :] + h32[:, None] * n32[None, :]
        return self.sectionPlanes(pts, np.broadcast_to(n32, pts.shape), mode=mode, counters=counters)

    def closestPointsDevice(self, points_ptr: int, n: int, out_ptr: int, counters=None, flags=0) -> int:
        """bm_scene_closest_points on device pointers (n bm_point records of 16 bytes in, n bm_hit records of
        16 bytes out, both 16-byte aligned); returns the error code. Asynchronous on the context stream unless
        `counters` (a uint64[4] numpy array to fill) is given. flags: none defined yet."""
        pp, op = C.c_void_p(points_ptr or None), C.c_void_p(out_ptr or None)
        if counters is None:
            return self.ctx.lib.bm_scene_closest_points(self.h, pp, n, flags, op)
        return self.ctx.lib.bm_scene_closest_points_counters(self.h, pp, n, flags, op,
                                                             counters.ctypes.data_as(C.POINTER(C.c_uint64)))

    def closestPoints(self, points, rmax=None, counters: bool = False):
        """The nearest triangle to each of n points (bm_scene_closest_points): its distance t, the
        barycentrics u, v of the closest point and its global id. rmax: None (unbounded), a scalar or n
        values; a point with no triangle within rmax gets the miss record (t = inf, tri_id = NO_TRIANGLE).

        numpy (n,3) float32 points: packs, uploads, queries and waits; returns numpy arrays
        {"t", "u", "v", "tri_id"}.
        torch tensors on the context's device — points (n,3) with rmax None, a scalar or an (n,) tensor, or
        one packed (n,4) float32 tensor (p, rmax): everything stays on the device and nothing waits. Returns
        {"hits": (n,4) float32, "t", "u", "v", "tri_id"} with the views traceRays returns; "hits" goes straight
        into hitAttributes, where VERTEX_DATA_POSITION is the closest point itself. Make the context on
        torch's stream, as for traceRays.
        counters=True adds "counters": [node records, triangle evaluations, points with a result, deepest
        stack] (waits)."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        on_device = isinstance(points, torch.Tensor)
        if on_device:
            if points.dim() == 2 and points.shape[1] == 4 and rmax is None:
                pts = points
            elif points.dim() == 2 and points.shape[1] == 3:
                pts = torch.empty((points.shape[0], 4), dtype=torch.float32, device=points.device)
                pts[:, 0:3] = points
                pts[:, 3] = float("inf") if rmax is None else rmax
            else:
                raise BeamError(ERROR_INVALID_PARAMETER, "closestPoints: points are (n, 3), or packed (n, 4), float32")
            if pts.device != dev or pts.dtype != torch.float32 or not pts.is_contiguous():
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"closestPoints: points must be contiguous float32 on {dev} (the context's device)")
        else:
            q = _f32(points).reshape(-1, 3)
            packed = np.zeros((q.shape[0], 4), np.float32)
            packed[:, 0:3] = q
            packed[:, 3] = np.inf if rmax is None else rmax
            pts = torch.from_numpy(packed).to(dev)
            torch.cuda.current_stream(dev).synchronize()  # the upload, before the context stream reads it
        n = pts.shape[0]
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        cnt = np.zeros(4, np.uint64) if counters else None
        self.ctx._check(self.closestPointsDevice(pts.data_ptr() if n else 0, n, out.data_ptr() if n else 0, cnt))
        self._points_keep = pts  # until the next query: the kernel may not have read them yet
        if on_device:
            res = {"hits": out, "t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "tri_id": out.view(torch.int32)[:, 3]}
        else:
            self.ctx.sync()
            h = out.cpu().numpy()
            res = {"t": h[:, 0].copy(), "u": h[:, 1].copy(), "v": h[:, 2].copy(),
                   "tri_id": h.view(np.uint32)[:, 3].copy()}
        if counters:
            res["counters"] = cnt
        return res

    def sweepSpheresDevice(self, sweeps, n: int, out, mode: int = _lib.SWEEP_CLOSEST, counters=None, flags=0) -> int:
        """bm_scene_sweep_spheres on the device: `sweeps` is n bm_sweep records of 32 bytes (origin, tmax, dir,
        radius), `out` n bm_hit records of 16 bytes (SWEEP_CLOSEST) or n bytes (SWEEP_ANY), each a raw device
        pointer or a torch tensor on the context's device, 16-byte aligned; returns the error code. Asynchronous
        on the context stream unless `counters` (a uint64[4] numpy array to fill) is given. flags: none defined."""
        sp = C.c_void_p((sweeps.data_ptr() if hasattr(sweeps, "data_ptr") else sweeps) or None)
        op = C.c_void_p((out.data_ptr() if hasattr(out, "data_ptr") else out) or None)
        if counters is None:
            return self.ctx.lib.bm_scene_sweep_spheres(self.h, sp, n, mode, flags, op)
        return self.ctx.lib.bm_scene_sweep_spheres_counters(self.h, sp, n, mode, flags, op,
                                                            counters.ctypes.data_as(C.POINTER(C.c_uint64)))

    def sweepSpheres(self, origins, dirs=None, radii=None, tmax=float("inf"), any: bool = False,
                     counters: bool = False):
        """The first contact of n swept spheres (bm_scene_sweep_spheres): the centre moves as origin + t * dir
        for 0 <= t <= tmax (dir need not be normalised); t is where the sphere first touches the scene, u, v
        the barycentrics of the contact point and tri_id its triangle; a sphere that touches at the start has
        t = 0, one that never touches the miss record (t = inf, tri_id = NO_TRIANGLE). radii and tmax: a scalar
        or n values. any=True: one flag per sweep, whether it touches anything within tmax.

        numpy (n,3) float32 origins and dirs: packs, uploads, queries and waits; returns numpy arrays
        {"t", "u", "v", "tri_id"}, or {"any"} (bool).
        torch tensors on the context's device — origins and dirs (n,3) with radii and tmax scalars or (n,)
        tensors, or one packed (n,8) float32 tensor of bm_sweep records as `origins` alone: everything stays on
        the device and nothing waits. Returns {"hits": (n,4) float32, "t", "u", "v", "tri_id"} with the views
        traceRays returns, or {"any": (n,) bool}; "hits" goes straight into hitAttributes, where
        VERTEX_DATA_POSITION is the contact point. Make the context on torch's stream, as for traceRays.
        counters=True adds "counters": [node records, triangle evaluations, sweeps with a result, deepest
        stack] (waits)."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        on_device = isinstance(origins, torch.Tensor)
        if on_device:
            if origins.dim() == 2 and origins.shape[1] == 8 and dirs is None and radii is None:
                rec = origins
            elif origins.dim() == 2 and origins.shape[1] == 3 and dirs is not None and radii is not None:
                rec = torch.empty((origins.shape[0], 8), dtype=torch.float32, device=origins.device)
                rec[:, 0:3] = origins
                rec[:, 3] = tmax
                rec[:, 4:7] = dirs
                rec[:, 7] = radii
            else:
                raise BeamError(ERROR_INVALID_PARAMETER,
                                "sweepSpheres: origins and dirs are (n, 3) with radii, or one packed (n, 8), float32")
            if rec.device != dev or rec.dtype != torch.float32 or not rec.is_contiguous():
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"sweepSpheres: sweeps must be contiguous float32 on {dev} (the context's device)")
        else:
            if dirs is None or radii is None:
                raise BeamError(ERROR_INVALID_PARAMETER, "sweepSpheres: origins, dirs and radii are required")
            o = _f32(origins).reshape(-1, 3)
            packed = np.zeros((o.shape[0], 8), np.float32)
            packed[:, 0:3] = o
            packed[:, 3] = tmax
            packed[:, 4:7] = _f32(dirs).reshape(-1, 3)
            packed[:, 7] = radii
            rec = torch.from_numpy(packed).to(dev)
            torch.cuda.current_stream(dev).synchronize()  # the upload, before the context stream reads it
        n = rec.shape[0]
        # rows of 16 bytes either way: an empty tensor's pointer is not passed on
        out = torch.empty((n,), dtype=torch.uint8, device=dev) if any else torch.empty((n, 4), dtype=torch.float32,
                                                                                       device=dev)
        cnt = np.zeros(4, np.uint64) if counters else None
        self.ctx._check(self.sweepSpheresDevice(rec.data_ptr() if n else 0, n, out.data_ptr() if n else 0,
                                                _lib.SWEEP_ANY if any else _lib.SWEEP_CLOSEST, cnt))
        self._sweeps_keep = rec  # until the next query: the kernel may not have read them yet
        if any:
            res = {"any": out.view(torch.bool)}
        else:
            res = {"hits": out, "t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "tri_id": out.view(torch.int32)[:, 3]}
        if not on_device:
            self.ctx.sync()
            if any:
                res = {"any": out.cpu().numpy().astype(bool)}
            else:
                h = out.cpu().numpy()
                res = {"t": h[:, 0].copy(), "u": h[:, 1].copy(), "v": h[:, 2].copy(),
                       "tri_id": h.view(np.uint32)[:, 3].copy()}
        if counters:
            res["counters"] = cnt
        return res

    def signedDistancesDevice(self, points, n: int, out, mode: int = _lib.SIGNED_DISTANCE, flags: int = 0,
                              votes=0, counters=None) -> int:
        """bm_scene_signed_distances on the device: `points` is n bm_point records of 16 bytes, `out` n bm_hit
        records of 16 bytes (SIGNED_DISTANCE) or n bytes (SIGNED_OCCUPANCY), both 16-byte aligned, `votes` 0 or
        n bytes of any alignment; each a raw device pointer or a torch tensor on the context's device. flags: 0
        or SIGNED_VOTE3. Returns the error code. Asynchronous on the context stream unless `counters` (a
        uint64[4] numpy array to fill) is given."""
        pp = C.c_void_p((points.data_ptr() if hasattr(points, "data_ptr") else points) or None)
        op = C.c_void_p((out.data_ptr() if hasattr(out, "data_ptr") else out) or None)
        vp = C.c_void_p((votes.data_ptr() if hasattr(votes, "data_ptr") else votes) or None)
        if counters is None:
            return self.ctx.lib.bm_scene_signed_distances(self.h, pp, n, mode, flags, op, vp)
        return self.ctx.lib.bm_scene_signed_distances_counters(self.h, pp, n, mode, flags, op, vp,
                                                               counters.ctypes.data_as(C.POINTER(C.c_uint64)))

    def _signed(self, who: str, points, rmax, mode: int, vote3: bool, votes: bool, counters: bool):
        """The shared path of signedDistance and occupancy: closestPoints' packing and stream rules."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        on_device = isinstance(points, torch.Tensor)
        if on_device:
            if points.dim() == 2 and points.shape[1] == 4 and rmax is None:
                pts = points
            elif points.dim() == 2 and points.shape[1] == 3:
                pts = torch.empty((points.shape[0], 4), dtype=torch.float32, device=points.device)
                pts[:, 0:3] = points
                pts[:, 3] = float("inf") if rmax is None else rmax
            else:
                raise BeamError(ERROR_INVALID_PARAMETER, who + ": points are (n, 3), or packed (n, 4), float32")
            if pts.device != dev or pts.dtype != torch.float32 or not pts.is_contiguous():
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"{who}: points must be contiguous float32 on {dev} (the context's device)")
        else:
            q = _f32(points).reshape(-1, 3)
            packed = np.zeros((q.shape[0], 4), np.float32)
            packed[:, 0:3] = q
            packed[:, 3] = np.inf if rmax is None else rmax
            pts = torch.from_numpy(packed).to(dev)
            torch.cuda.current_stream(dev).synchronize()  # the upload, before the context stream reads it
        n = pts.shape[0]
        dist = mode == _lib.SIGNED_DISTANCE
        out = (torch.empty((n, 4), dtype=torch.float32, device=dev) if dist
               else torch.empty((n,), dtype=torch.uint8, device=dev))
        vt = torch.empty((n,), dtype=torch.uint8, device=dev) if votes else None
        cnt = np.zeros(4, np.uint64) if counters else None
        self.ctx._check(self.signedDistancesDevice(pts.data_ptr() if n else 0, n, out.data_ptr() if n else 0, mode,
                                                   _lib.SIGNED_VOTE3 if vote3 else 0,
                                                   vt.data_ptr() if votes and n else 0, cnt))
        self._points_keep = pts  # until the next query: the kernel may not have read them yet
        if dist:
            res = {"hits": out, "t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "tri_id": out.view(torch.int32)[:, 3]}
        else:
            res = {"inside": out.view(torch.bool)}
        if votes:
            res["votes"] = vt
        if not on_device:
            self.ctx.sync()
            if dist:
                h = out.cpu().numpy()
                res = {"t": h[:, 0].copy(), "u": h[:, 1].copy(), "v": h[:, 2].copy(),
                       "tri_id": h.view(np.uint32)[:, 3].copy()}
            else:
                res = {"inside": out.cpu().numpy().astype(bool)}
            if votes:
                res["votes"] = vt.cpu().numpy()
        if counters:
            res["counters"] = cnt
        return res

    def signedDistance(self, points, rmax=None, vote3: bool = False, votes: bool = False, counters: bool = False):
        """The signed distance of n points to the scene (bm_scene_signed_distances, SIGNED_DISTANCE): what
        closestPoints returns for the same points and rmax, with the sign bit of t set where the point is
        inside — crossing parity along one fixed direction, or with vote3 the majority of three. A point with
        no triangle within rmax gets t = -inf inside and +inf outside (tri_id = NO_TRIANGLE either way).
        Inputs, outputs and stream rules as closestPoints: numpy in, numpy out after a wait; torch tensors stay
        on the device and nothing waits ("hits" goes straight into hitAttributes).
        votes=True adds "votes": uint8 (n,), the votes for inside (0..1, or 0..3 with vote3; 1 or 2 of 3 marks
        an open mesh or a grazing ray). counters=True adds "counters": [nearest-phase node records and triangle
        evaluations, parity-phase node records and triangle tests] (waits)."""
        return self._signed("signedDistance", points, rmax, _lib.SIGNED_DISTANCE, vote3, votes, counters)

    def occupancy(self, points, vote3: bool = False, votes: bool = False):
        """Inside or outside for n points (bm_scene_signed_distances, SIGNED_OCCUPANCY): {"inside": bool (n,)}
        and with votes=True "votes" as signedDistance gives them. No distance is computed. numpy (n,3) points
        in, numpy out after a wait; torch (n,3) or packed (n,4) points stay on the device and nothing waits."""
        return self._signed("occupancy", points, None, _lib.SIGNED_OCCUPANCY, vote3, votes, False)

    def sdfGrid(self, lo, hi, dims, rmax=None, vote3: bool = True):
        """The signed distance at the cell centres of a regular grid: a float32 tensor of shape dims =
        (nx, ny, nz) on the context's device (a view of the records' t column), negative inside (signedDistance over the centres; beyond rmax
        the value is -inf or +inf). The centres are voxelize's, made on the device by the same float32
        statements, cell (i, j, k) being point (i * ny + j) * nz + k of the batch; the stream rules are
        voxelize's too."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 1:
            raise BeamError(ERROR_INVALID_PARAMETER, "sdfGrid: dims is three positive integers")
        lo32, hi32 = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        cell = (hi32 - lo32) / np.asarray(dims, np.float32)
        n = dims[0] * dims[1] * dims[2]
        pts = torch.empty((n, 4), dtype=torch.float32, device=dev)
        grid = pts.view(dims[0], dims[1], dims[2], 4)
        for a in range(3):  # one multiply and one add per component, as voxelize
            idx = torch.arange(dims[a], dtype=torch.float32, device=dev)
            axis = float(lo32[a]) + (idx + 0.5) * float(cell[a])
            shape = [1, 1, 1]
            shape[a] = dims[a]
            grid[..., a] = axis.view(shape)
        grid[..., 3] = float("inf") if rmax is None else float(rmax)
        torch.cuda.current_stream(dev).synchronize()  # the points, before the context stream reads them
        # the t column of the records as a strided view: no copy, so nothing runs on another stream
        return self.signedDistance(pts, vote3=vote3)["hits"].view(dims[0], dims[1], dims[2], 4)[..., 0]

    def hitAttributesDevice(self, hits_ptr: int, n: int, requests) -> int:
        """bm_scene_hit_attributes on device pointers: n bm_hit records of 16 bytes in, and per request
        (slot, components, flags, out_ptr[, pad]) n rows of `components` 4-byte words out, every pointer
        16-byte aligned; returns the error code. Asynchronous on the context stream."""
        requests = list(requests)
        arr = (_lib.AttrReq * max(len(requests), 1))()
        for a, r in zip(arr, requests):
            a.slot, a.components, a.flags, a.out_dev = r[0], r[1], r[2], r[3] or None
            a.pad = r[4] if len(r) > 4 else 0
        return self.ctx.lib.bm_scene_hit_attributes(self.h, C.c_void_p(hits_ptr or None), n, arr, len(requests))

    def hitAttributes(self, hits, requests):
        """The meshes' vertex slots interpolated at hit records (bm_scene_hit_attributes): the shading normal,
        texture coordinate, tangent frame or position a caller needs to shade a hit or start the next ray.

        hits: the (n,4) float32 tensor traceRays returns under "hits" (t, u, v, tri_id bits), or a numpy
        array of the same layout. requests: up to ATTR_MAX_REQS tuples (slot, components[, flags]) — a
        VERTEX_DATA_* slot, or ATTR_GEOM_NORMAL (3 components) or ATTR_MESH_FACE (2); flags ATTR_NORMALIZE
        for 3-component rows. Returns one (n, components) array per request: float32, except ATTR_MESH_FACE
        which is int32 (scene mesh index, face index), -1 on a miss; every other row of a miss is zero.
        torch tensors stay on the device and nothing waits (make the context on torch's stream, as for
        traceRays); numpy in gives numpy out and waits."""
        import torch
        dev = torch.device("cuda", self.ctx.device)
        on_device = isinstance(hits, torch.Tensor)
        if on_device:
            h = hits
            if h.dim() != 2 or h.shape[1] != 4 or h.device != dev or h.dtype != torch.float32 or not h.is_contiguous():
                raise BeamError(ERROR_INVALID_PARAMETER,
                                f"hitAttributes: hits must be contiguous (n, 4) float32 on {dev} (the context's device)")
        else:
            a = np.ascontiguousarray(hits)
            if a.dtype != np.float32:
                a = a.view(np.float32) if a.dtype.itemsize == 4 else a.astype(np.float32)
            h = torch.from_numpy(a.reshape(-1, 4)).to(dev)
            torch.cuda.current_stream(dev).synchronize()  # the upload, before the context stream reads it
        n = h.shape[0]
        reqs = [tuple(r) + (0,) * (3 - len(r)) for r in requests]
        outs = [torch.empty((n, int(r[1])), dtype=torch.int32 if r[0] == ATTR_MESH_FACE else torch.float32, device=dev)
                for r in reqs]
        self.ctx._check(self.hitAttributesDevice(h.data_ptr() if n else 0, n,
                                                 [(r[0], r[1], r[2], o.data_ptr() if n else 0)
                                                  for r, o in zip(reqs, outs)]))
        self._attrs_keep = h  # until the next call: the kernel may not have read them yet
        if on_device:
            return outs
        self.ctx.sync()
        return [o.cpu().numpy() for o in outs]

    def export(self):
        """(records[nrec, 16, 32 or 64], tris[n,12], keys[n], perm[n]) as uint32 — for parity tests.
        BVH4 records are written for every node above the leaf size, but a traversal reaches only
        the even-depth ones (the others are expanded into their parents' records) and the oracle
        writes only those: compare reachable_records rather than the whole array."""
        st = self.last_stats or self.updateGPUScene(stats=True)
        n, nrec = st["num_tris"], st["num_records"]
        rec = np.zeros((nrec, {8: 64, 4: 32}.get(st["bvh_width"], 16)), np.uint32)
        tris = np.zeros((max(n, 1), 12), np.uint32)
        keys = np.zeros(max(n, 1), np.uint32)
        perm = np.zeros(max(n, 1), np.uint32)
        self.ctx._check(self.ctx.lib.bm_scene_export(self.h, _up(rec), _up(tris), _up(keys), _up(perm)))
        return rec, tris[:n], keys[:n], perm[:n]

    def destroy(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.bm_scene_destroy(self.h)
        self.h = None


class IRenderTarget:
    """Raytracer/Beam.h:32-45 with an offscreen device buffer instead of a GL TBO."""

    _current = None  # RenderTarget::m_RT (RenderTarget.cpp:85-93)

    def __init__(self, ctx: Context, handle, keepalive=None):
        self.ctx = ctx
        self.h = handle
        self._keep = keepalive
        self._locked = False

    @staticmethod
    def createOffscreen(ctx: Context, width: int, height: int, pitch: int = 0) -> "IRenderTarget":
        h = C.c_void_p()
        ctx._check(ctx.lib.bm_rt_create_offscreen(ctx.h, width, height, pitch, C.byref(h)))
        return IRenderTarget(ctx, h)

    @staticmethod
    def createExternal(ctx: Context, width: int, height: int, pitch: int, packed_ptr: int, tri_ptr: int,
                       t_ptr: int, nz_ptr: int = 0, keepalive=None) -> "IRenderTarget":
        h = C.c_void_p()
        ctx._check(ctx.lib.bm_rt_create_external(ctx.h, width, height, pitch, C.c_void_p(packed_ptr),
                                                 C.c_void_p(tri_ptr), C.c_void_p(t_ptr),
                                                 C.c_void_p(nz_ptr) if nz_ptr else None, C.byref(h)))
        return IRenderTarget(ctx, h, keepalive)

    def buffer(self) -> int:
        return self.ctx.lib.bm_rt_buffer(self.h) or 0

    def width(self) -> int:
        return self.ctx.lib.bm_rt_width(self.h)

    def height(self) -> int:
        return self.ctx.lib.bm_rt_height(self.h)

    def pitch(self) -> int:
        return self.ctx.lib.bm_rt_pitch(self.h)

    def lock(self) -> int:
        err = self.ctx.lib.bm_rt_lock(self.h)
        if err == ERROR_ALL_FINE:
            IRenderTarget._current = self
        return err

    def unlock(self) -> int:
        err = self.ctx.lib.bm_rt_unlock(self.h)
        if err == ERROR_ALL_FINE and IRenderTarget._current is self:
            IRenderTarget._current = None
        return err

    @staticmethod
    def get():
        return IRenderTarget._current

    def read(self, packed=True, tri_id=True, t=True, rgb=False):
        """Synchronous readback -> dict of (H, W) numpy planes (rgb: (H, W, 3))."""
        w, h = self.width(), self.height()
        out = {}
        bufs = {}
        if packed:
            bufs["packed"] = np.empty((h, w), np.uint32)
        if tri_id:
            bufs["tri_id"] = np.empty((h, w), np.uint32)
        if t:
            bufs["t"] = np.empty((h, w), np.float32)
        if rgb:
            bufs["rgb"] = np.empty((h, w, 3), np.float32)
        self.ctx._check(self.ctx.lib.bm_rt_read(
            self.h, _up(bufs["packed"]) if packed else None, _up(bufs["tri_id"]) if tri_id else None,
            _fp(bufs["t"]) if t else None, _fp(bufs["rgb"]) if rgb else None))
        out.update(bufs)
        return out

    def setStream(self, stream) -> None:
        """Frames in flight: this target's traces and readbacks on its own HIP stream (an int handle,
        e.g. torch.cuda.Stream().cuda_stream; None or 0: the context stream). See bm_rt_set_stream."""
        self.ctx._check(self.ctx.lib.bm_rt_set_stream(self.h, C.c_void_p(stream) if stream else None))

    def stream(self) -> int:
        """Handle of the stream this target's work runs on."""
        return self.ctx.lib.bm_rt_stream(self.h) or 0

    TRACE_KINDS = {0: "quads", 1: "cull+quads", 2: "lanes", 3: "kd march", 4: "hash march", 5: "packets"}

    def traceKind(self) -> str:
        """Kernels the last trace into this target ran (bm_rt_trace_kind): quads, cull+quads, ..."""
        return self.TRACE_KINDS.get(int(self.ctx.lib.bm_rt_trace_kind(self.h)), "none")

    def rayQueueCounts(self):
        """Rays per queue region that survived k_cull in the last trace into this target, a uint32 array
        (bm_rt_ray_queue_counts; that trace must have been compacted: traceKind() 'cull+quads')."""
        n = C.c_uint32(0)
        self.ctx._check(self.ctx.lib.bm_rt_ray_queue_counts(self.h, None, 0, C.byref(n)))
        out = np.empty(n.value, np.uint32)
        if n.value:
            self.ctx._check(self.ctx.lib.bm_rt_ray_queue_counts(self.h, _up(out), n.value, C.byref(n)))
        return out

    def debugTileCosts(self, set=None, get: int = 0):
        """bm_rt_debug_tile_costs, the test hook of the cost-ordered schedule: set (uint32 words) replaces the
        head of this target's per-tile cost table, which the next trace sorts its tiles by; get = n returns the
        table's first n words as a uint32 array once the target's stream has finished (None without get)."""
        if set is not None:
            a = np.ascontiguousarray(set, np.uint32).reshape(-1)
            self.ctx._check(self.ctx.lib.bm_rt_debug_tile_costs(self.h, a.size, _up(a), None))
        if not get:
            return None
        out = np.empty(int(get), np.uint32)
        self.ctx._check(self.ctx.lib.bm_rt_debug_tile_costs(self.h, out.size, None, _up(out)))
        return out

    def lastTiming(self):
        """Multi-device contexts: (band trace ms, exchange ms) of the last frame traced into this
        target, from HIP events (bm_rt_last_timing; waits for that frame)."""
        out = (C.c_float * 2)()
        self.ctx._check(self.ctx.lib.bm_rt_last_timing(self.h, out))
        return float(out[0]), float(out[1])

    def savePPM(self, path) -> None:
        """Binary PPM (P6) of the packed plane, written by the library (bm_rt_save_ppm)."""
        self.ctx._check(self.ctx.lib.bm_rt_save_ppm(self.h, os.fsencode(path)))

    def shadow(self) -> int:
        """Device pointer of the u8 shadow plane (0 before the first shadow trace)."""
        return self.ctx.lib.bm_rt_shadow(self.h) or 0

    def readShadow(self):
        """Synchronous readback of the shadow plane -> (H, W) uint8 (1 = shadowed)."""
        out = np.empty((self.height(), self.width()), np.uint8)
        self.ctx._check(self.ctx.lib.bm_rt_read_shadow(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def destroy(self):
        if getattr(self, "h", None) and self.ctx.h:
            if IRenderTarget._current is self:
                IRenderTarget._current = None
            self.ctx.lib.bm_rt_destroy(self.h)
        self.h = None


class ICamera:
    """Raytracer/Beam.h:65-72, Camera.cpp."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.bm_camera_create(ctx.h, C.byref(h)))
        self.h = h

    @staticmethod
    def create(ctx: Context) -> "ICamera":
        return ICamera(ctx)

    def setInitialRays(self, width, height, left=-1.0, right=1.0, top=1.0, bottom=-1.0, zoom=1.0) -> int:
        return self.ctx.lib.bm_camera_set_initial_rays(self.h, width, height, left, right, top, bottom, zoom)

    def clear(self, value: int) -> int:
        rt = IRenderTarget.get()
        if rt is None:
            return ERROR_NO_RENDER_TARGET
        return self.ctx.lib.bm_rt_clear(rt.h, value)

    @staticmethod
    def _eo(eye3, orient3x3):
        e = _f32(eye3).reshape(3)
        o = _f32(orient3x3).reshape(9)
        return e, o

    def traceScene(self, eye3, orient3x3, scene: IScene) -> int:
        rt = IRenderTarget.get()
        if rt is None:
            return ERROR_NO_RENDER_TARGET
        return self.trace(eye3, orient3x3, scene, rt)

    def trace(self, eye3, orient3x3, scene: IScene, rt: IRenderTarget) -> int:
        e, o = self._eo(eye3, orient3x3)
        return self.ctx.lib.bm_camera_trace(self.h, _fp(e), _fp(o), scene.h, rt.h)

    def traceBands(self, eye3, orient3x3, scene: IScene, rt: IRenderTarget, band_height: int, band_step: int,
                   band_first: int) -> int:
        e, o = self._eo(eye3, orient3x3)
        return self.ctx.lib.bm_camera_trace_bands(self.h, _fp(e), _fp(o), scene.h, rt.h, band_height, band_step,
                                                  band_first)

    def traceShadow(self, eye3, orient3x3, scene: IScene, rt: IRenderTarget, light3) -> int:
        """Primary trace + one any-hit shadow ray per hit toward the point light light3."""
        e, o = self._eo(eye3, orient3x3)
        lt = _f32(light3).reshape(3)
        return self.ctx.lib.bm_camera_trace_shadow(self.h, _fp(e), _fp(o), scene.h, rt.h, _fp(lt))

    def traceShadowBands(self, eye3, orient3x3, scene: IScene, rt: IRenderTarget, band_height: int,
                         band_step: int, band_first: int, light3) -> int:
        e, o = self._eo(eye3, orient3x3)
        lt = _f32(light3).reshape(3)
        return self.ctx.lib.bm_camera_trace_shadow_bands(self.h, _fp(e), _fp(o), scene.h, rt.h, band_height,
                                                         band_step, band_first, _fp(lt))

    def traceShadowCounters(self, eye3, orient3x3, scene: IScene, rt: IRenderTarget, light3):
        """[primary nodes, tris, hits, shadow nodes, shadow tris, shadowed pixels]."""
        e, o = self._eo(eye3, orient3x3)
        lt = _f32(light3).reshape(3)
        out = np.zeros(6, np.uint64)
        self.ctx._check(self.ctx.lib.bm_camera_trace_shadow_counters(
            self.h, _fp(e), _fp(o), scene.h, rt.h, _fp(lt), out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def traceCounters(self, eye3, orient3x3, scene: IScene, rt: IRenderTarget):
        e, o = self._eo(eye3, orient3x3)
        out = np.zeros(3, np.uint64)
        self.ctx._check(self.ctx.lib.bm_camera_trace_counters(
            self.h, _fp(e), _fp(o), scene.h, rt.h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def traceProfile(self, eye3, orient3x3, scene: IScene, rt: IRenderTarget):
        """Diagnostic trace: per-wave (start, end, placement, work) as a uint64 [waves, 4] array."""
        e, o = self._eo(eye3, orient3x3)
        n = C.c_uint32(0)
        self.ctx.lib.bm_camera_trace_profile(self.h, _fp(e), _fp(o), scene.h, rt.h, None, 0, C.byref(n))
        cap = n.value
        out = np.zeros((cap, 4), np.uint64)
        self.ctx._check(self.ctx.lib.bm_camera_trace_profile(
            self.h, _fp(e), _fp(o), scene.h, rt.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(n)))
        return out[: n.value]

    def destroy(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.bm_camera_destroy(self.h)
        self.h = None


class Model:
    """TestProgram/Model.cpp Model::load over the native OBJ reader (bm_model_*, csrc/bm_obj.cpp)."""

    def __init__(self, path: str, unshared: bool = False):
        self.lib = _lib.load()
        h = C.c_void_p()
        err = self.lib.bm_model_load(os.fsencode(path), _lib.OBJ_UNSHARED if unshared else 0, C.byref(h))
        if err:
            raise BeamError(err, f"bm_model_load({path!r}) failed")
        self.h = h
        self.ctx = None

    @staticmethod
    def load(ctx: "Context", name: str, toScene: "IScene", numAdds: int = 1) -> "Model":
        """Model::load(name, toScene, numAdds): parse, create one IMesh per mesh, add each numAdds times."""
        m = Model(name)
        m.upload(ctx, toScene, numAdds)
        return m

    def info(self) -> dict:
        st = _lib.ModelInfo()
        self.lib.bm_model_info_get(self.h, C.byref(st))
        return {"num_meshes": st.num_meshes, "num_faces": st.num_faces, "num_vertices": st.num_vertices,
                "bmin": list(st.bmin), "bmax": list(st.bmax)}

    def meshes(self):
        """Parsed meshes as dicts {pos (V,3), nrm (V,3) or None, uv (V,2) or None, tan / bit (V,3) or None
        (tangent space, meshes with normals and UVs), idx (3F,), material}."""
        out = []
        for i in range(self.info()["num_meshes"]):
            pos, nrm, uv = _FPtr(), _FPtr(), _FPtr()
            idx = C.POINTER(C.c_uint32)()
            nv, ni = C.c_uint32(), C.c_uint32()
            mat = C.c_char_p()
            self.lib.bm_model_mesh(self.h, i, C.byref(pos), C.byref(nrm), C.byref(uv), C.byref(idx), C.byref(nv),
                                   C.byref(ni), C.byref(mat))
            tan, bit = _FPtr(), _FPtr()
            self.lib.bm_model_mesh_tangents(self.h, i, C.byref(tan), C.byref(bit))
            v = nv.value

            def arr(ptr, k):
                return np.ctypeslib.as_array(ptr, shape=(v * k,)).reshape(v, k).copy() if ptr and v else None

            out.append({"pos": arr(pos, 3) if v else np.zeros((0, 3), np.float32), "nrm": arr(nrm, 3),
                        "uv": arr(uv, 2), "tan": arr(tan, 3), "bit": arr(bit, 3),
                        "idx": np.ctypeslib.as_array(idx, shape=(ni.value,)).copy() if ni.value else
                        np.zeros(0, np.uint32), "material": (mat.value or b"").decode()})
        return out

    def upload(self, ctx: "Context", scene: "IScene" = None, num_adds: int = 1):
        self.ctx = ctx
        ctx._check(self.lib.bm_model_upload(self.h, ctx.h, scene.h if scene is not None else None, num_adds))

    def addInstance(self, ctx: "Context", scene: "IScene", xform) -> None:
        """bm_model_add_instance: upload the model's meshes (once) and add each to scene as an instance entry
        with the one transform."""
        x = _xform12(xform)
        self.ctx = ctx
        ctx._check(self.lib.bm_model_add_instance(self.h, ctx.h, scene.h, _fp(x)))

    def gpu_mesh(self, i: int):
        return self.lib.bm_model_gpu_mesh(self.h, i)

    def destroy(self):
        if getattr(self, "h", None):
            self.lib.bm_model_destroy(self.h)
        self.h = None


_FPtr = C.POINTER(C.c_float)


def chainSegments(a, b):
    """Chains the cut segments of one plane (sectionPlanes mode "segments": a (m,3), b (m,3), numpy or torch)
    into polylines on the host: (loops, chains), each a list of lists of segment indices into a and b.

    Segments of length zero (a[i] and b[i] the same bytes: a triangle touching the plane from below in one
    vertex) are dropped. The others are linked where the end b of one equals the start a of another byte for
    byte: no tolerance, which is what the query's cut points allow. Where several segments start at one point,
    the segments ending there are paired with them both in ascending input order (the k-th ending with the k-th
    starting). Every segment then has at most one successor and one predecessor: a loop is a closed run,
    listed from its lowest index; a chain is an open run, listed from its first segment to its last. Chains
    come first by their first segment's index, loops by their lowest. A closed consistently oriented mesh gives
    loops alone."""
    def host(x):
        if hasattr(x, "detach"):
            x = x.detach().cpu().numpy()
        return np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 3)
    a, b = host(a), host(b)
    if a.shape != b.shape:
        raise BeamError(ERROR_INVALID_PARAMETER, "chainSegments: a and b are (m, 3) arrays of the same length")
    ka = [r.tobytes() for r in a.view(np.uint32)]
    kb = [r.tobytes() for r in b.view(np.uint32)]
    live = [i for i in range(len(ka)) if ka[i] != kb[i]]
    starts, ends = {}, {}
    for i in live:  # ascending
        starts.setdefault(ka[i], []).append(i)
        ends.setdefault(kb[i], []).append(i)
    nxt, has_prev = {}, set()
    for key, incoming in ends.items():
        for i, j in zip(incoming, starts.get(key, ())):
            nxt[i] = j
            has_prev.add(j)
    loops, chains, seen = [], [], set()
    for i in live:
        if i in has_prev:
            continue
        run = [i]
        while run[-1] in nxt:
            run.append(nxt[run[-1]])
        seen.update(run)
        chains.append(run)
    for i in live:
        if i in seen:
            continue
        run = [i]
        while nxt[run[-1]] != i:
            run.append(nxt[run[-1]])
        seen.update(run)
        loops.append(run)
    return loops, chains


def reachable_records(records: np.ndarray) -> np.ndarray:
    """Indices of the node records a traversal can reach from record 0 (BVH2, BVH4 or BVH8 layout)."""
    words = records.shape[1]
    ref_lo, nref = {64: (48, 8), 32: (24, 4)}.get(words, (12, 2))
    seen, stack = [], [0]
    mark = np.zeros(records.shape[0], bool)
    while stack:
        i = stack.pop()
        if mark[i]:
            continue
        mark[i] = True
        seen.append(i)
        for r in records[i, ref_lo:ref_lo + nref]:
            r = int(r)
            if r != 0xFFFFFFFF and not (r & 0x80000000):
                stack.append(r)
    return np.array(sorted(seen), np.int64)


def upload_meshes(ctx: Context, scene: IScene, meshes):
    """Create one IMesh per mesh dict {pos, nrm, idx} (Model::load order) and add it to scene. An optional
    "slots": {slot_id: array (V, components)} uploads further vertex slots (hitAttributes reads them)."""
    out = []
    for m in meshes:
        mesh = IMesh.create(ctx)
        pos = _f32(m["pos"]).reshape(-1, 3)
        idx = np.ascontiguousarray(m["idx"], np.uint32).reshape(-1)
        ctx._check(mesh.setIndices(idx, idx.size))
        ctx._check(mesh.setVertexData(pos, pos.shape[0], 3, VERTEX_DATA_POSITION))
        if m.get("nrm") is not None:
            nrm = _f32(m["nrm"]).reshape(-1, 3)
            ctx._check(mesh.setVertexData(nrm, nrm.shape[0], 3, VERTEX_DATA_NORMAL))
        for slot, data in (m.get("slots") or {}).items():
            data = _f32(data).reshape(pos.shape[0], -1)
            ctx._check(mesh.setVertexData(data, data.shape[0], data.shape[1], int(slot)))
        scene.addMesh(mesh)
        out.append(mesh)
    return out


def render(ctx: Context, meshes, width, height, rays, eye, orient, leaf_size=None):
    """Convenience: upload, build, trace one frame; returns (frame dict, build stats)."""
    scene = IScene.create(ctx)
    upload_meshes(ctx, scene, meshes)
    stats = scene.updateGPUScene(stats=True)
    cam = ICamera.create(ctx)
    ctx._check(cam.setInitialRays(width, height, *rays))
    rt = IRenderTarget.createOffscreen(ctx, width, height)
    ctx._check(cam.trace(eye, orient, scene, rt))
    frame = rt.read(rgb=True)
    rt.destroy()
    cam.destroy()
    scene.destroy()
    return frame, stats
