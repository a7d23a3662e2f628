"""Host-side mirror of the reference's launch sequence, over the C ABI.

What the reference's ``RendererMesh::commitRendererData`` / ``startRender`` do around the
launch (src/Global/RendererMesh.cu:93-160 GAS + instances + IAS, :247-305 SBT, :323-324 RNG,
:328-333 camera, :395-419 per-frame upload + launch) is restated here step by step, each step
being one call into libhrt.so.  PyTorch is used only to own device memory and streams.
The C++ twin of this file is csrc/host/renderer_host.hpp.
"""
from __future__ import annotations

import ctypes as C

import numpy as np


def _ref(p):
    """byref of a ctypes structure, None (a NULL pointer: the library's defaults) passed through"""
    return C.byref(p) if p is not None else None


def _f32(x):
    return np.float32(x)


def _normalize(v):
    """normalize(), include/Global/DeviceFunctions.cuh:397-404 with rsqrtf pinned as 1/sqrtf."""
    v = np.asarray(v, dtype=np.float32)
    len2 = _f32(_f32(_f32(v[0] * v[0]) + _f32(v[1] * v[1])) + _f32(v[2] * v[2]))
    if len2 <= _f32(_f32(1e-6) * _f32(1e-6)):
        return np.array([0, 0, 1], dtype=np.float32)
    inv = _f32(_f32(1.0) / np.sqrt(len2, dtype=np.float32))
    return np.array([v[0] * inv, v[1] * inv, v[2] * inv], dtype=np.float32)


def _cross(a, b):
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    return np.array([_f32(_f32(a[1] * b[2]) - _f32(a[2] * b[1])),
                     _f32(_f32(a[2] * b[0]) - _f32(a[0] * b[2])),
                     _f32(_f32(a[0] * b[1]) - _f32(a[1] * b[0]))], dtype=np.float32)


def configure_camera(center, target, up, opengl=True):
    """SDL_GraphicsWindowConfigureCamera, src/GraphicsAPI/SDL_GraphicsWindow.cu:4-14.
    Returns (U, V, W): W = target - center is NOT normalised (its length sets the field of view)."""
    center = np.asarray(center, dtype=np.float32)
    target = np.asarray(target, dtype=np.float32)
    up_dir = _normalize(up)
    if not opengl:
        up_dir = (-up_dir).astype(np.float32)
    w = (target - center).astype(np.float32)
    u = _normalize(_cross(w, up_dir))
    v = _normalize(_cross(u, w))
    return u, v, w


def tile_for_rank(height, rank, world_size, stripe_rows=8):
    """Row stripes of the multi-GPU split: stripe k (stripe_rows rows) belongs to rank k % world_size.
    Interleaving balances the load (the middle of the frame is the expensive part)."""
    from . import Tile
    if world_size <= 1:
        return Tile(0, height, 1, 1, 0)
    return Tile(0, height, stripe_rows, world_size, rank)


def reduce_tiles(frame, dst=0):
    """The one exchange step of the multi-GPU split: sum the per-rank frames (each zero outside its
    own row stripes, so x + 0 is exact) into rank ``dst`` over torch.distributed (RCCL on GPUs)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        if frame.is_cuda and dist.get_backend() != "nccl":
            # rehearsal on a box with fewer cards than ranks (gloo has no CUDA reduce): stage through the host
            staged = frame.cpu()
            dist.reduce(staged, dst=dst, op=dist.ReduceOp.SUM)
            if dist.get_rank() == dst:
                frame.copy_(staged)
        else:
            dist.reduce(frame, dst=dst, op=dist.ReduceOp.SUM)
    return frame


class Renderer:
    """One context + one scene: build, then ``render()`` as often as needed."""

    def __init__(self, device=0, flags=0):
        import torch
        from . import load_library, HrtError
        self._torch = torch
        self._err = HrtError
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise HrtError("no GPU visible: the renderer has no CPU path")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        ctx = C.c_void_p()
        rc = self.lib.hrt_ctx_create(device, flags, C.byref(ctx))
        if rc != 0:
            raise HrtError(f"hrt_ctx_create: {self.lib.hrt_last_error(None).decode()}")
        self.ctx = ctx
        self._keep = []             # device tensors the SBT records point into
        self._blas = []
        self._n_inst = None
        self.tlas = None
        self._built_blas = {}       # BLAS handle -> its normals: the BLASes build_tlas(vertices=...) made
        self._scene_blas = {}       # ... and load_scene's triangle BLASes (update_blas_vertices rewrites either in place)
        self._scene_spheres = {}    # load_scene's sphere BLASes: handle -> (centres, radii), the buffers their records shade with (update_blas_spheres rewrites them in place)
        self._tlas_blas = {}        # TLAS handle -> those of them it was built over
        self._tlases = {}           # handle -> (host instance array, device instance array, count, SBT records): load_scene's and build_tlas's
        self.states = None
        self.width = self.height = 0
        self.color = self.albedo = self.normal = self.linear = None
        self.sum = self.taken = self.counts = None      # adaptive sampling: the frame's sums, sample totals and last count map
        self.cam = None

    # ---- helpers ----
    def _check(self, rc, what):
        if rc != 0:
            raise self._err(f"{what}: {self.lib.hrt_last_error(self.ctx).decode()} (status {rc})")

    def _dev(self, arr):
        t = self._torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
        return t

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    # ---- scene ----
    def load_scene(self, scene):
        """GAS per instance -> instances (sbtOffset = i) -> IAS -> SBT records -> miss record."""
        from . import Instance, SbtRecord, MissParams, Float3
        from . import PROGRAM_SPHERE_ROUGH, PROGRAM_SPHERE_METAL, PROGRAM_TRIANGLE_ROUGH, PROGRAM_TRIANGLE_METAL
        lib, st = self.lib, self._stream()
        insts = scene["instances"]
        n = len(insts)
        h_inst = (Instance * max(n, 1))()
        h_rec = (SbtRecord * max(n, 1))()
        shared = {}                                        # "shape" id -> (GAS handle, normals): RendererTime.cu:116-130
        for i, it in enumerate(insts):
            handle = C.c_uint64()
            if it["geometry"] == "triangles":
                key = it.get("shape")
                if key is not None and key in shared:
                    handle.value, normals = shared[key]
                else:
                    verts = self._dev(it["vertices"].reshape(-1, 3))
                    normals = self._dev(it["normals"].reshape(-1, 3))
                    self._check(lib.hrt_blas_build_triangles(self.ctx, verts.data_ptr(), verts.shape[0], st, C.byref(handle)),
                                "hrt_blas_build_triangles")
                    del verts                              # the reference frees vertices after the build too
                    self._keep.append(normals)
                    self._scene_blas[handle.value] = normals
                    if key is not None:
                        shared[key] = (handle.value, normals)
                h_rec[i].data.ptr0 = normals.data_ptr()
                prog = PROGRAM_TRIANGLE_ROUGH if it["material"] == "rough" else PROGRAM_TRIANGLE_METAL
            else:
                key = it.get("shape")
                if key is not None and ("spheres", key) in shared:
                    handle.value, (centers, radii) = shared[("spheres", key)]
                else:
                    centers = self._dev(it["centers"])
                    radii = self._dev(it["radii"])
                    self._check(lib.hrt_blas_build_spheres(self.ctx, centers.data_ptr(), radii.data_ptr(), radii.shape[0], st,
                                                           C.byref(handle)), "hrt_blas_build_spheres")
                    self._keep += [centers, radii]
                    self._scene_spheres[handle.value] = (centers, radii)
                    if key is not None:
                        shared[("spheres", key)] = (handle.value, (centers, radii))
                h_rec[i].data.ptr0 = centers.data_ptr()
                h_rec[i].data.ptr1 = radii.data_ptr()
                prog = PROGRAM_SPHERE_ROUGH if it["material"] == "rough" else PROGRAM_SPHERE_METAL
            self._blas.append(handle.value)
            self._check(lib.hrt_sbt_record_pack_header(prog, C.byref(h_rec[i], 0)), "hrt_sbt_record_pack_header")
            a = it["albedo"]
            h_rec[i].data.albedo = Float3(float(a[0]), float(a[1]), float(a[2]))
            h_rec[i].data.fuzz = float(it["fuzz"]) if it["material"] == "metal" else 0.0
            for k in range(12):
                h_inst[i].transform[k] = float(it["transform"][k])
            h_inst[i].instanceId = 0
            h_inst[i].sbtOffset = i
            h_inst[i].visibilityMask = 1
            h_inst[i].flags = 0
            h_inst[i].traversableHandle = handle.value
        d_inst = self._dev(np.frombuffer(bytes(h_inst), dtype=np.uint8).copy())
        tl = C.c_uint64()
        self._check(lib.hrt_tlas_build(self.ctx, d_inst.data_ptr(), n, st, C.byref(tl)), "hrt_tlas_build")
        self.tlas = tl.value
        self._d_inst = d_inst
        self._h_inst = h_inst
        self._n_inst = n
        self._n_scene = n
        self._scene_inst, self._scene_rec = bytes(h_inst), bytes(h_rec)      # the loaded scene's instances and records: what build_tlas draws from
        self._tlases[self.tlas] = (h_inst, d_inst, n, h_rec)
        self._check(lib.hrt_materials_set(self.ctx, h_rec, n), "hrt_materials_set")
        bg = scene.get("background", np.array([0.7, 0.8, 0.9], dtype=np.float32))
        miss = MissParams(Float3(float(bg[0]), float(bg[1]), float(bg[2])))
        self._check(lib.hrt_miss_set(self.ctx, C.byref(miss)), "hrt_miss_set")
        cam = scene["camera"]
        self.set_camera(cam["center"], cam["target"], cam["up"], cam.get("opengl", True))
        return self

    def build_tlas(self, order=None, transforms=None, vertices=None, normals=None):
        """Another TLAS over the loaded scene's BLASes: instance j is the scene's instance ``order[j]`` (None: all of them in order; a
        subset, a permutation, repeats) with ``transforms[j]`` (12 floats; None: the scene's), sbtOffset j and the material record of
        its source.  ``vertices``: {j: (t, 3, 3) float32} -- instance j gets a triangle BLAS of its own built from these object-space
        vertices, and a normals buffer of its own, ``normals[j]`` ((t, 3, 3); default scenes.face_normals of the vertices), which its
        record points at.  The renderer owns those BLASes (destroy_built_blases frees them early, close() the rest).  Returns the
        handle; the renderer stays on the TLAS it was on (use_tlas switches)."""
        from . import Instance, SbtRecord, scenes
        n_scene = self._n_scene
        order = list(range(n_scene)) if order is None else [int(k) for k in order]
        n = len(order)
        src_inst = (Instance * max(n_scene, 1)).from_buffer_copy(self._scene_inst)
        src_rec = (SbtRecord * max(n_scene, 1)).from_buffer_copy(self._scene_rec)
        h_inst = (Instance * max(n, 1))()
        h_rec = (SbtRecord * max(n, 1))()
        for j, k in enumerate(order):
            if not 0 <= k < n_scene:
                raise self._err(f"build_tlas: the scene has no instance {k}")
            C.memmove(C.byref(h_inst[j]), C.byref(src_inst[k]), C.sizeof(Instance))
            C.memmove(C.byref(h_rec[j]), C.byref(src_rec[k]), C.sizeof(SbtRecord))
            h_inst[j].sbtOffset = j
            if transforms is not None:
                for c in range(12):
                    h_inst[j].transform[c] = float(transforms[j][c])
        own = []
        for j, v in sorted((vertices or {}).items()):
            if not 0 <= j < n:
                raise self._err(f"build_tlas: vertices for instance {j} of {n}")
            v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3, 3)
            nrm = normals[j] if normals is not None and j in normals else scenes.face_normals(v)
            nrm = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3, 3)
            if nrm.shape != v.shape:
                raise self._err(f"build_tlas: instance {j} has {v.shape[0]} triangles and normals for {nrm.shape[0]}")
            d_v, d_n = self._dev(v.reshape(-1, 3)), self._dev(nrm.reshape(-1, 3))
            handle = C.c_uint64()
            self._check(self.lib.hrt_blas_build_triangles(self.ctx, d_v.data_ptr(), d_v.shape[0], self._stream(), C.byref(handle)),
                        "hrt_blas_build_triangles")
            del d_v
            own.append(handle.value)
            self._built_blas[handle.value] = d_n           # (the normals live as long as the BLAS does)
            h_inst[j].traversableHandle = handle.value
            h_rec[j].data.ptr0 = d_n.data_ptr()
        d_inst = self._dev(np.frombuffer(bytes(h_inst), dtype=np.uint8).copy())
        tl = C.c_uint64()
        self._check(self.lib.hrt_tlas_build(self.ctx, d_inst.data_ptr(), n, self._stream(), C.byref(tl)), "hrt_tlas_build")
        self._tlases[tl.value] = (h_inst, d_inst, n, h_rec)
        self._tlas_blas[tl.value] = own
        return tl.value

    def destroy_built_blases(self, tlas):
        """hrt_blas_destroy of the BLASes build_tlas(vertices=...) made for ``tlas``, with their normals.  The TLAS must not be traced
        afterwards -- destroy it too, or never use it again; a pending denoise_temporal_rebind(by_primitive=True) from it keeps what it
        reads."""
        for handle in self._tlas_blas.pop(tlas, []):
            self._check(self.lib.hrt_blas_destroy(self.ctx, handle), "hrt_blas_destroy")
            self._torch.cuda.synchronize(self.device)      # (the normals go with the BLAS: no launch that shades with them is in flight)
            del self._built_blas[handle]

    def use_tlas(self, tlas):
        """Render, update and denoise on ``tlas`` (load_scene's or one of build_tlas's) from now on: its instance array and count, and
        its material records through hrt_materials_set.  The denoiser's history does not follow by itself: denoise_temporal_rebind."""
        if tlas not in self._tlases:
            raise self._err(f"use_tlas: 0x{tlas:x} is not a TLAS of this renderer")
        self._h_inst, self._d_inst, self._n_inst, h_rec = self._tlases[tlas]
        self.tlas = tlas
        self._check(self.lib.hrt_materials_set(self.ctx, h_rec, self._n_inst), "hrt_materials_set")

    def destroy_tlas(self, tlas):
        """hrt_tlas_destroy of one of build_tlas's trees that the renderer is not on."""
        if tlas == self.tlas or tlas not in self._tlases:
            raise self._err(f"destroy_tlas: 0x{tlas:x} is in use or not a TLAS of this renderer")
        self._check(self.lib.hrt_tlas_destroy(self.ctx, tlas), "hrt_tlas_destroy")
        del self._tlases[tlas]

    def update_blas_vertices(self, handle_or_instance, vertices, normals=None):
        """hrt_blas_update_triangles: the triangle BLAS gets new object-space ``vertices`` ((t, 3, 3) float32, as many triangles as it
        was built with) in place, and the normals buffer the renderer keeps for it -- what its instances' records point at -- is
        rewritten on the same stream with ``normals`` ((t, 3, 3); default scenes.face_normals of the vertices).  ``handle_or_instance``: the
        handle of a BLAS load_scene or build_tlas(vertices=...) made, or (any other number) the index of an instance of the current TLAS,
        whose BLAS is meant.  Does NOT update any TLAS: every TLAS over the BLAS shows the old geometry until its next update_instances."""
        from . import scenes
        handle = int(handle_or_instance)
        if handle not in self._scene_blas and handle not in self._built_blas:
            if self._n_inst is None or not 0 <= handle < self._n_inst:
                raise self._err(f"update_blas_vertices: {handle} is neither a triangle BLAS of this renderer nor an instance of its TLAS")
            handle = int(self._h_inst[handle].traversableHandle)
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3, 3)
        nrm = scenes.face_normals(v) if normals is None else normals
        nrm = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3, 3)
        if nrm.shape != v.shape:
            raise self._err(f"update_blas_vertices: {v.shape[0]} triangles and normals for {nrm.shape[0]}")
        d_v = self._dev(v.reshape(-1, 3))
        self._check(self.lib.hrt_blas_update_triangles(self.ctx, handle, d_v.data_ptr(), d_v.shape[0], self._stream()),
                    "hrt_blas_update_triangles")
        del d_v                                            # (the BLAS has its own copy, as after the build)
        keep = self._scene_blas.get(handle, self._built_blas.get(handle))
        if keep is not None:
            if tuple(keep.shape) != (3 * v.shape[0], 3):
                raise self._err(f"update_blas_vertices: the normals buffer of BLAS 0x{handle:x} holds {keep.shape[0] // 3} triangles")
            keep.copy_(self._dev(nrm.reshape(-1, 3)))      # in place: the records keep their pointer

    def update_blas_spheres(self, handle_or_instance, centers, radii):
        """hrt_blas_update_spheres: the sphere BLAS gets new object-space ``centers`` ((n, 3) float32) and ``radii`` ((n,) float32, as many
        spheres as it was built with) in place, and the centres and radii buffers the renderer keeps for it -- what its instances' records
        shade with -- are rewritten on the same stream.  ``handle_or_instance``: the handle of a sphere BLAS load_scene made, or (any other
        number) the index of an instance of the current TLAS, whose BLAS is meant.  Does NOT update any TLAS: every TLAS over the BLAS
        shows the old spheres until its next update_instances."""
        handle = int(handle_or_instance)
        if handle not in self._scene_spheres:
            if self._n_inst is None or not 0 <= handle < self._n_inst:
                raise self._err(f"update_blas_spheres: {handle} is neither a sphere BLAS of this renderer nor an instance of its TLAS")
            handle = int(self._h_inst[handle].traversableHandle)
        if handle not in self._scene_spheres:
            raise self._err(f"update_blas_spheres: BLAS 0x{handle:x} is not a sphere BLAS of this renderer")
        c = np.ascontiguousarray(centers, dtype=np.float32).reshape(-1, 3)
        r = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
        keep_c, keep_r = self._scene_spheres[handle]
        if c.shape[0] != r.shape[0] or tuple(keep_c.shape) != c.shape:
            raise self._err(f"update_blas_spheres: {c.shape[0]} centres and {r.shape[0]} radii for a BLAS of {keep_r.shape[0]} spheres")
        d_c, d_r = self._dev(c), self._dev(r)
        self._check(self.lib.hrt_blas_update_spheres(self.ctx, handle, d_c.data_ptr(), d_r.data_ptr(), d_r.shape[0], self._stream()),
                    "hrt_blas_update_spheres")
        keep_c.copy_(d_c)                                  # in place: the records keep their pointers
        keep_r.copy_(d_r)

    def update_instances(self, transforms):
        """Per-frame instance update + updateIAS (src/Global/RendererMesh.cu:379-401)."""
        for i, m in enumerate(transforms):
            for k in range(12):
                self._h_inst[i].transform[k] = float(m[k])
        self._d_inst.copy_(self._torch.from_numpy(np.frombuffer(bytes(self._h_inst), dtype=np.uint8).copy()))
        self._check(self.lib.hrt_tlas_update(self.ctx, self.tlas, self._d_inst.data_ptr(), len(transforms), self._stream()),
                    "hrt_tlas_update")

    def pose_instances(self, current, nxt, duration, frame, frame_count, first_instance=0,
                       offset=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0), update=True, mesh_mode=False):
        """Time mode's per-frame pose step on the device (src/Global/RendererTime.cu:436-480): ``current`` / ``nxt`` are
        (n, 12) float32 particle states (quat.xyzw, position, velocity, 2 pad) of this and the next time step; writes the
        transforms of instances [first_instance, first_instance + n) in device memory, then updateIAS."""
        from . import PoseParams
        cur = current if hasattr(current, "data_ptr") else self._dev(np.ascontiguousarray(current, dtype=np.float32))
        nx = nxt if hasattr(nxt, "data_ptr") else self._dev(np.ascontiguousarray(nxt, dtype=np.float32))
        n = cur.shape[0]
        pp = PoseParams(float(duration), int(frame), int(frame_count),
                        (C.c_float * 3)(*[float(x) for x in offset]), (C.c_float * 3)(*[float(x) for x in scale]), 1 if mesh_mode else 0)
        self._check(self.lib.hrt_pose_instances(self.ctx, self._d_inst.data_ptr(), first_instance, n, cur.data_ptr(), nx.data_ptr(),
                                                C.byref(pp), self._stream()), "hrt_pose_instances")
        if update:
            self._check(self.lib.hrt_tlas_update(self.ctx, self.tlas, self._d_inst.data_ptr(), self._n_inst,
                                                 self._stream()), "hrt_tlas_update")

    def instance_transforms(self):
        """The transforms currently in the device instance array, (n, 12) float32."""
        raw = self._d_inst.cpu().numpy().view(np.uint8).reshape(-1, 80)
        return raw[: self._n_inst, :48].copy().view(np.float32).reshape(-1, 12)

    def set_camera(self, center, target, up, opengl=True):
        u, v, w = configure_camera(center, target, up, opengl)
        self.cam = (np.asarray(center, dtype=np.float32), u, v, w)

    def set_frame(self, width, height, seed_salt, aov=True, linear=False):
        """RNG states + output buffers (initDeviceRandomGenerators, denoiser input buffers)."""
        torch = self._torch
        if self.states is not None:
            self._check(self.lib.hrt_rng_free(self.ctx, self.states, self._stream()), "hrt_rng_free")
            self.states = None
        st = C.c_void_p()
        self._check(self.lib.hrt_rng_init(self.ctx, width, height, seed_salt, self._stream(), C.byref(st)), "hrt_rng_init")
        self.states = st
        self.width, self.height = width, height
        self.color = torch.zeros((height, width, 4), dtype=torch.float32, device=self.device)
        self.albedo = torch.full((height, width, 4), 7.0, dtype=torch.float32, device=self.device) if aov else None
        self.normal = torch.full((height, width, 4), 7.0, dtype=torch.float32, device=self.device) if aov else None
        self.linear = torch.zeros((height, width, 4), dtype=torch.float32, device=self.device) if linear else None
        # adaptive sampling (accumulate / sample_counts): per pixel the sums of radiance and squared luminance, and how many samples they hold
        self.sum = torch.zeros((height, width, 4), dtype=torch.float32, device=self.device)
        self.taken = torch.zeros((height, width), dtype=torch.int32, device=self.device)
        self.counts = None
        self._check(self.lib.hrt_debug_set_linear_output(self.ctx, self.linear.data_ptr() if linear else None),
                    "hrt_debug_set_linear_output")
        return self

    def rng_states_numpy(self):
        """Copy of the device RNG states as a (H*W, 12) uint32 array (48 bytes per state)."""
        self._torch.cuda.synchronize(self.device)
        n = self.width * self.height
        out = np.empty((n, 12), dtype=np.uint32)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rc = hip.hipMemcpy(out.ctypes.data, self.states, n * 48, 2)      # hipMemcpyDeviceToHost
        if rc != 0:
            raise self._err(f"hipMemcpy of the RNG states failed ({rc})")
        return out

    # ---- the launch ----
    def _launch_blocks(self):
        from . import GlobalParams, RayGenParams, Float3
        center, u, v, w = self.cam
        params = GlobalParams(self.tlas, self.states)
        rg = RayGenParams()
        rg.width, rg.height = self.width, self.height
        rg.colorBuffer = self.color.data_ptr()
        rg.albedoBuffer = self.albedo.data_ptr() if self.albedo is not None else None
        rg.normalBuffer = self.normal.data_ptr() if self.normal is not None else None
        rg.cameraCenter = Float3(*[float(x) for x in center])
        rg.cameraU = Float3(*[float(x) for x in u])
        rg.cameraV = Float3(*[float(x) for x in v])
        rg.cameraW = Float3(*[float(x) for x in w])
        return params, rg

    def render(self, spp=1, tile=None, sync=True):
        params, rg = self._launch_blocks()
        st = self._stream()
        self._check(self.lib.hrt_render_launch(self.ctx, C.byref(params), C.byref(rg), spp, _ref(tile), st), "hrt_render_launch")
        if sync:
            self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")

    # ---- adaptive sampling: pilot -> counts -> refine (include/hrt.h: hrt_render_accumulate, hrt_sample_counts) ----
    def accumulation_reset(self):
        """A new frame of accumulate(): no pixel holds a sample (the sums need no reset: a pixel's first sample is assigned)."""
        self.taken.zero_()
        self.counts = None

    def accumulate(self, spp=1, counts=None, tile=None, sync=True):
        """hrt_render_accumulate over ``self.sum`` / ``self.taken``: every pixel of the tile takes min(counts, spp) more samples (``counts``: an
        (H, W) int32 device tensor; None: spp each) on its RNG stream, and ``self.color`` becomes colorToFloat4(sum / taken) wherever taken > 0.
        After any sequence of these calls a pixel holds bit for bit what render(spp = its total) gives it from the same initial states."""
        params, rg = self._launch_blocks()
        st = self._stream()
        if counts is not None and (counts.dtype != self._torch.int32 or tuple(counts.shape) != (self.height, self.width) or not counts.is_contiguous()):
            raise self._err("accumulate: counts must be a contiguous (height, width) int32 tensor on the device")
        self._check(self.lib.hrt_render_accumulate(self.ctx, C.byref(params), C.byref(rg), spp, counts.data_ptr() if counts is not None else None,
                                                   self.sum.data_ptr(), self.taken.data_ptr(), _ref(tile), st), "hrt_render_accumulate")
        if sync:
            self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")

    def sample_counts(self, params=None):
        """hrt_sample_counts of the frame's sums: the (H, W) int32 tensor of how many MORE samples each pixel should take (kept in
        ``self.counts``).  ``params``: None, a SampleCountParams or a dict of its fields over the defaults."""
        from . import SampleCountParams
        p = self._params(SampleCountParams, "hrt_sample_counts_default_params", params)
        self.counts = self._torch.empty((self.height, self.width), dtype=self._torch.int32, device=self.device)
        self._check(self.lib.hrt_sample_counts(self.ctx, self.sum.data_ptr(), self.taken.data_ptr(), self.width, self.height,
                                               C.byref(p) if p is not None else None, self.counts.data_ptr(), self._stream()), "hrt_sample_counts")
        return self.counts

    def render_adaptive(self, pilot, params=None):
        """One adaptive frame: reset, ``pilot`` samples everywhere, the count map from their variance, one refinement launch in which every
        pixel takes its count (never more than max_total).  Returns the count map; ``self.taken`` holds the totals."""
        from . import SampleCountParams
        p = self._params(SampleCountParams, "hrt_sample_counts_default_params", params)
        if p is None:
            p = SampleCountParams()
            self._check(self.lib.hrt_sample_counts_default_params(C.byref(p)), "hrt_sample_counts_default_params")
        self.accumulation_reset()
        self.accumulate(pilot, sync=False)
        counts = self.sample_counts(p)
        self.accumulate(p.max_total, counts=counts)
        return counts

    def primary_hits(self):
        """CTX_CAPTURE_PRIMARY: the primary hit of every pixel as the last render() found it, (t, u, v, prim, inst) numpy arrays of
        width * height in frame order -- trace_rays' form, a miss as (tmax = 1e16, ., ., 0xffffffff, 0xffffffff).  Raises HrtError (status -5)
        when the context holds no valid capture."""
        torch = self._torch
        n = self.width * self.height
        t, u, v = (torch.empty(n, dtype=torch.float32, device=self.device) for _ in range(3))
        prim, inst = (torch.empty(n, dtype=torch.int32, device=self.device) for _ in range(2))
        st = self._stream()
        self._check(self.lib.hrt_primary_hits_get(self.ctx, t.data_ptr(), u.data_ptr(), v.data_ptr(), prim.data_ptr(), inst.data_ptr(), st),
                    "hrt_primary_hits_get")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        return (t.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy(), prim.cpu().numpy().view(np.uint32), inst.cpu().numpy().view(np.uint32))

    def to_rgba8(self):
        torch = self._torch
        out = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device=self.device)
        self._check(self.lib.hrt_to_rgba8(self.ctx, self.color.data_ptr(), out.data_ptr(), self.width, self.height,
                                          self._stream()), "hrt_to_rgba8")
        self._torch.cuda.synchronize(self.device)
        return out

    # ---- the denoiser (denoiseOutput, src/Global/RendererImpl.cu:680-710) ----
    def _params(self, cls, default_fn, params):
        """None (the library's defaults), an instance of the ctypes class ``cls``, or a dict of its fields over the defaults that the
        library's ``default_fn`` fills in."""
        if params is None or isinstance(params, cls):
            return params
        p = cls()
        self._check(getattr(self.lib, default_fn)(C.byref(p)), default_fn)
        for k, v in dict(params).items():
            setattr(p, k, v)
        return p

    def denoise_guides(self):
        """The primary-hit guides of the current frame and camera: (H, W, 8) uint16 tensor -- per pixel the HrtDenoiseGuide record,
        normal[3] and albedo[3] as IEEE halves, then the hit distance as two halves of a float (``.view(torch.float32)`` of
        ``[..., 6:8]``; +inf on a miss)."""
        torch = self._torch
        params, rg = self._launch_blocks()
        guides = torch.empty((self.height, self.width, 8), dtype=torch.int16, device=self.device)
        st = self._stream()
        self._check(self.lib.hrt_denoise_guides(self.ctx, C.byref(params), C.byref(rg), guides.data_ptr(), st), "hrt_denoise_guides")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        return guides

    def denoise_filter(self, color, guides, params=None, out=None):
        """The filter alone: ``color`` (H, W, 4) float32 and ``guides`` (H, W, 8) 16-bit (denoise_guides) device tensors -> a new
        (H, W, 4) tensor, or ``out`` (which may be ``color``).  params: None (the defaults), a DenoiseParams or a dict of its fields."""
        torch = self._torch
        h, w = int(color.shape[0]), int(color.shape[1])
        assert color.is_contiguous() and guides.is_contiguous() and tuple(guides.shape) == (h, w, 8) and guides.element_size() == 2
        out = torch.empty_like(color) if out is None else out
        from . import DenoiseParams
        p = self._params(DenoiseParams, "hrt_denoise_default_params", params)
        st = self._stream()
        self._check(self.lib.hrt_denoise_filter(self.ctx, color.data_ptr(), guides.data_ptr(), out.data_ptr(), w, h, _ref(p), st),
                    "hrt_denoise_filter")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        return out

    def denoise(self, params=None, out=None):
        """denoiseOutput: the guides of the current frame + the filter of the colour buffer (``self.color``, what the last render
        wrote) -> a new (H, W, 4) float32 tensor, or ``out`` (which may be ``self.color``).  The AOV buffers are not touched."""
        params_blk, rg = self._launch_blocks()
        out = self._torch.empty_like(self.color) if out is None else out
        from . import DenoiseParams
        p = self._params(DenoiseParams, "hrt_denoise_default_params", params)
        st = self._stream()
        self._check(self.lib.hrt_denoise_launch(self.ctx, C.byref(params_blk), C.byref(rg), _ref(p), out.data_ptr(), st), "hrt_denoise_launch")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        return out

    def denoise_temporal(self, params=None, tparams=None, out=None):
        """The temporal mode of denoiseOutput: the colour buffer blended into the reprojected history of the frames before it, then
        filtered -> a new (H, W, 4) float32 tensor, or ``out`` (which may be ``self.color``).  params as for denoise; tparams: None (the
        defaults), a DenoiseTemporalParams or a dict of its fields.  The first call, and the first after denoise_temporal_reset or a
        change of scene or frame size, equals denoise()."""
        params_blk, rg = self._launch_blocks()
        out = self._torch.empty_like(self.color) if out is None else out
        from . import DenoiseParams, DenoiseTemporalParams
        p = self._params(DenoiseParams, "hrt_denoise_default_params", params)
        tp = self._params(DenoiseTemporalParams, "hrt_denoise_temporal_default_params", tparams)
        st = self._stream()
        self._check(self.lib.hrt_denoise_temporal_launch(self.ctx, C.byref(params_blk), C.byref(rg), _ref(p), _ref(tp), out.data_ptr(), st),
                    "hrt_denoise_temporal_launch")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        self._temporal_shape = (self.height, self.width)
        return out

    def denoise_temporal_reset(self):
        self._check(self.lib.hrt_denoise_temporal_reset(self.ctx), "hrt_denoise_temporal_reset")

    def denoise_temporal_rebind(self, tlas, prev_instance=None, by_primitive=False):
        """hrt_denoise_temporal_rebind: the next denoise_temporal / denoise_variance on ``tlas`` continues the history made on the TLAS
        the last one ran on.  prev_instance[i]: the index instance i of ``tlas`` had there, NO_INSTANCE for a new body; None: the
        identity over the instances both have.  by_primitive: hrt_denoise_temporal_rebind_geometry -- an instance whose BLAS was
        rebuilt with the same triangles (build_tlas's ``vertices``) keeps its history, primitive by primitive.  Call before use_tlas /
        the poses of the next frame or after: the order is free."""
        n = self._tlases[tlas][2] if tlas in self._tlases else 0
        arr = None
        if prev_instance is not None:
            arr = (C.c_uint32 * max(len(prev_instance), 1))(*[int(x) for x in prev_instance])
            n = len(prev_instance)
        name = "hrt_denoise_temporal_rebind_geometry" if by_primitive else "hrt_denoise_temporal_rebind"
        self._check(getattr(self.lib, name)(self.ctx, tlas, arr, n, self._stream()), name)

    def denoise_temporal_state(self):
        """The last denoise_temporal's intermediates: (accumulated colour (H, W, 4), history length (H, W), reprojected position
        (H, W, 2) in the previous frame's pixels, NaN where none was made), float32 device tensors."""
        torch = self._torch
        h, w = getattr(self, "_temporal_shape", (self.height, self.width))       # (the size of the call the state is of)
        acc = torch.empty((h, w, 4), dtype=torch.float32, device=self.device)
        length = torch.empty((h, w), dtype=torch.float32, device=self.device)
        motion = torch.empty((h, w, 2), dtype=torch.float32, device=self.device)
        st = self._stream()
        self._check(self.lib.hrt_debug_denoise_temporal_state(self.ctx, acc.data_ptr(), length.data_ptr(), motion.data_ptr(), st),
                    "hrt_debug_denoise_temporal_state")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        return acc, length, motion

    def denoise_filter_variance(self, color, guides, variance, params=None, vparams=None, out=None, var_out=None):
        """The variance-guided filter alone: ``color`` (H, W, 4) float32, ``guides`` (H, W, 8) 16-bit and ``variance`` (H, W) float32
        device tensors -> (colour, variance): new tensors, or ``out`` (may be ``color``) and ``var_out`` (may be ``variance``;
        False: the filtered variance is not returned).  vparams: None, a DenoiseVarianceParams or a dict of its fields."""
        torch = self._torch
        h, w = int(color.shape[0]), int(color.shape[1])
        assert color.is_contiguous() and guides.is_contiguous() and tuple(guides.shape) == (h, w, 8) and guides.element_size() == 2
        assert variance.is_contiguous() and tuple(variance.shape) == (h, w) and variance.dtype == torch.float32
        out = torch.empty_like(color) if out is None else out
        if var_out is None:
            var_out = torch.empty_like(variance)
        from . import DenoiseParams, DenoiseVarianceParams
        p = self._params(DenoiseParams, "hrt_denoise_default_params", params)
        vp = self._params(DenoiseVarianceParams, "hrt_denoise_variance_default_params", vparams)
        st = self._stream()
        self._check(self.lib.hrt_denoise_filter_variance(self.ctx, color.data_ptr(), guides.data_ptr(), variance.data_ptr(), out.data_ptr(),
                                                         var_out.data_ptr() if var_out is not False else None, w, h, _ref(p), _ref(vp), st),
                    "hrt_denoise_filter_variance")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        return out, (var_out if var_out is not False else None)

    def denoise_variance(self, params=None, tparams=None, vparams=None, out=None):
        """The variance-guided mode of denoiseOutput: denoise_temporal's reprojection and blend, with the luminance moments carried
        along, and a filter whose colour edge stop follows the accumulated frame's variance -> a new (H, W, 4) float32 tensor, or
        ``out`` (which may be ``self.color``).  Shares its history with denoise_temporal: a call after the other mode starts afresh."""
        params_blk, rg = self._launch_blocks()
        out = self._torch.empty_like(self.color) if out is None else out
        from . import DenoiseParams, DenoiseTemporalParams, DenoiseVarianceParams
        p = self._params(DenoiseParams, "hrt_denoise_default_params", params)
        tp = self._params(DenoiseTemporalParams, "hrt_denoise_temporal_default_params", tparams)
        vp = self._params(DenoiseVarianceParams, "hrt_denoise_variance_default_params", vparams)
        st = self._stream()
        self._check(self.lib.hrt_denoise_variance_launch(self.ctx, C.byref(params_blk), C.byref(rg), _ref(p), _ref(tp), _ref(vp),
                                                         out.data_ptr(), st), "hrt_denoise_variance_launch")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        self._temporal_shape = (self.height, self.width)
        return out

    def denoise_variance_state(self):
        """The last denoise_variance's luminance moments (H, W, 2) and the variance its filter took (H, W), float32 device tensors."""
        torch = self._torch
        h, w = getattr(self, "_temporal_shape", (self.height, self.width))
        moments = torch.empty((h, w, 2), dtype=torch.float32, device=self.device)
        variance = torch.empty((h, w), dtype=torch.float32, device=self.device)
        st = self._stream()
        self._check(self.lib.hrt_debug_denoise_variance_state(self.ctx, moments.data_ptr(), variance.data_ptr(), st),
                    "hrt_debug_denoise_variance_state")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        return moments, variance

    def denoise_accumulated_filter(self, sum4, taken, guides, params=None, vparams=None, out=None, linear_out=None, var_out=None):
        """The accumulated mode over given guides: ``sum4`` (H, W, 4) float32 and ``taken`` (H, W) int32 as accumulate() leaves them,
        ``guides`` (H, W, 8) 16-bit -> (encoded colour, filtered linear frame, filtered variance): new tensors, or ``out``,
        ``linear_out`` and ``var_out`` (False for either of the last two: not returned).  The filter runs on the linear mean sum / taken
        with the variance of that mean as its edge stop; a pixel with taken == 0 is background.  params, vparams as for
        denoise_filter_variance."""
        torch = self._torch
        h, w = int(sum4.shape[0]), int(sum4.shape[1])
        assert sum4.is_contiguous() and tuple(sum4.shape) == (h, w, 4) and sum4.dtype == torch.float32
        assert taken.is_contiguous() and tuple(taken.shape) == (h, w) and taken.dtype == torch.int32
        assert guides.is_contiguous() and tuple(guides.shape) == (h, w, 8) and guides.element_size() == 2
        out = torch.empty_like(sum4) if out is None else out
        if linear_out is None:
            linear_out = torch.empty_like(sum4)
        if var_out is None:
            var_out = torch.empty((h, w), dtype=torch.float32, device=sum4.device)
        from . import DenoiseParams, DenoiseVarianceParams
        p = self._params(DenoiseParams, "hrt_denoise_default_params", params)
        vp = self._params(DenoiseVarianceParams, "hrt_denoise_variance_default_params", vparams)
        st = self._stream()
        self._check(self.lib.hrt_denoise_accumulated_filter(self.ctx, sum4.data_ptr(), taken.data_ptr(), guides.data_ptr(), out.data_ptr(),
                                                            linear_out.data_ptr() if linear_out is not False else None,
                                                            var_out.data_ptr() if var_out is not False else None, w, h, _ref(p), _ref(vp), st),
                    "hrt_denoise_accumulated_filter")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        return out, (linear_out if linear_out is not False else None), (var_out if var_out is not False else None)

    def denoise_accumulated(self, params=None, vparams=None, out=None):
        """The accumulated mode of denoiseOutput, for a still that accumulate() / render_adaptive() has sampled: the guides of the
        current frame + the variance-guided filter of ``self.sum`` / ``self.taken`` on linear radiance, encoded -> a new (H, W, 4) float32
        tensor, or ``out`` (which may be ``self.color``).  Needs no history and leaves denoise_temporal's and denoise_variance's alone."""
        params_blk, rg = self._launch_blocks()
        out = self._torch.empty_like(self.color) if out is None else out
        from . import DenoiseParams, DenoiseVarianceParams
        p = self._params(DenoiseParams, "hrt_denoise_default_params", params)
        vp = self._params(DenoiseVarianceParams, "hrt_denoise_variance_default_params", vparams)
        st = self._stream()
        self._check(self.lib.hrt_denoise_accumulated_launch(self.ctx, C.byref(params_blk), C.byref(rg), self.sum.data_ptr(), self.taken.data_ptr(),
                                                            _ref(p), _ref(vp), out.data_ptr(), st), "hrt_denoise_accumulated_launch")
        self._check(self.lib.hrt_sync(self.ctx, st), "hrt_sync")
        return out

    def to_rgba8_of(self, frame):
        """convertFloat4ToUchar4Kernel of any (H, W, 4) float32 device tensor (to_rgba8: of the colour buffer)."""
        torch = self._torch
        out = torch.empty((frame.shape[0], frame.shape[1], 4), dtype=torch.uint8, device=self.device)
        self._check(self.lib.hrt_to_rgba8(self.ctx, frame.data_ptr(), out.data_ptr(), frame.shape[1], frame.shape[0], self._stream()),
                    "hrt_to_rgba8")
        self._torch.cuda.synchronize(self.device)
        return out

    def trace_rays(self, origins, directions, tmin=1e-6, tmax=1e16, any_hit=False):
        torch = self._torch
        o = self._dev(np.asarray(origins, dtype=np.float32).reshape(-1, 3))
        d = self._dev(np.asarray(directions, dtype=np.float32).reshape(-1, 3))
        n = o.shape[0]
        t = torch.empty(n, dtype=torch.float32, device=self.device)
        u = torch.empty_like(t)
        v = torch.empty_like(t)
        prim = torch.empty(n, dtype=torch.int32, device=self.device)
        inst = torch.empty(n, dtype=torch.int32, device=self.device)
        self._check(self.lib.hrt_trace_rays(self.ctx, self.tlas, o.data_ptr(), d.data_ptr(), n, tmin, tmax, int(any_hit),
                                            t.data_ptr(), u.data_ptr(), v.data_ptr(), prim.data_ptr(), inst.data_ptr(),
                                            self._stream()), "hrt_trace_rays")
        return (t.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy(),
                prim.cpu().numpy().view(np.uint32), inst.cpu().numpy().view(np.uint32))

    def stats(self, reset=False):
        from . import Stats
        s = Stats()
        self._check(self.lib.hrt_stats_get(self.ctx, C.byref(s)), "hrt_stats_get")
        if reset:
            self._check(self.lib.hrt_stats_reset(self.ctx), "hrt_stats_reset")
        return s

    def set_flags(self, flags):
        self._check(self.lib.hrt_ctx_set_flags(self.ctx, flags), "hrt_ctx_set_flags")

    def reset_stats(self):
        self._check(self.lib.hrt_stats_reset(self.ctx), "hrt_stats_reset")

    def close(self):
        if getattr(self, "ctx", None):
            if self.states is not None:
                self.lib.hrt_rng_free(self.ctx, self.states, None)
                self.states = None
            self.lib.hrt_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
