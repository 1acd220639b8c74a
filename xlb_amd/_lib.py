"""ctypes binding of libxlbhip.so (include/xlbhip.h) and thin RAII wrappers.

This is the stub a reference maintainer would add for a ``ComputeBackend.HIP`` (see
INTEGRATION.md): every ``hip_implementation`` method of the operators calls one function of
the C ABI through the objects defined here.  There is NO fallback: if the shared library is
missing or a call fails, an exception is raised.
"""

import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XLBHIP_LIB") or os.path.join(_HERE, "lib", "libxlbhip.so")  # XLBHIP_LIB: A/B builds (tools/)

# element types (include/xlbhip.h)
F64, F32, F16, U8, BOOL, MISSING = 0, 1, 2, 3, 4, 5
D2Q9, D3Q19, D3Q27 = 0, 1, 2
BGK, KBC, SMAGORINSKY_LES_BGK, REGULARIZED_BGK, RECURSIVE_REGULARIZED_BGK = 0, 1, 2, 3, 4
BC_EQUILIBRIUM, BC_HALFWAY_BB, BC_FULLWAY_BB, BC_DO_NOTHING = 1, 2, 3, 4
BC_ZOUHE_VELOCITY, BC_ZOUHE_PRESSURE, BC_REGULARIZED_VELOCITY, BC_REGULARIZED_PRESSURE = 5, 6, 7, 8
BC_EXTRAPOLATION_OUTFLOW = 9
BC_HYBRID_BB_REGULARIZED, BC_HYBRID_BB_GRADS, BC_HYBRID_NEQ_REGULARIZED = 10, 11, 12
BC_HALFWAY_BB_PROFILE = 13
MESH_AABB, MESH_RAY, MESH_AABB_CLOSE, MESH_WINDING = 1, 2, 3, 4
UNIQUE_ID_BYTES = 128

NP_OF_DTYPE = {F64: np.float64, F32: np.float32, F16: np.float16, U8: np.uint8, BOOL: np.bool_, MISSING: np.uint8}


class HipBackendError(RuntimeError):
    pass


class BcDesc(C.Structure):
    _fields_ = [("id", C.c_int32), ("kind", C.c_int32), ("values", C.c_double * 27)]


_p = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_i = C.c_int
_i64 = C.c_int64
_d = C.c_double

# name -> argtypes ; every function returns int except xlbhip_last_error
SIGNATURES = {
    "xlbhip_create": [_i, _pp],
    "xlbhip_destroy": [_p],
    "xlbhip_sync": [_p],
    "xlbhip_device_info": [_p, C.c_char_p, _i, C.POINTER(_i), C.POINTER(C.c_uint64)],
    "xlbhip_set_option": [_p, C.c_char_p, _i64],
    "xlbhip_get_option": [_p, C.c_char_p, C.POINTER(_i64)],
    "xlbhip_lattice_info": [_i, C.POINTER(_i), C.POINTER(_i), _p, _p, _p, _p],
    "xlbhip_field_create": [_p, _i, _i, _i, _i, _i, _i, _d, _pp],
    "xlbhip_field_destroy": [_p],
    "xlbhip_field_fill": [_p, _d],
    "xlbhip_field_copy": [_p, _p],
    "xlbhip_field_copy_kernel": [_p, _p, _i],
    "xlbhip_field_copy_tiles": [_p, _p],
    "xlbhip_field_upload": [_p, _p, C.c_size_t],
    "xlbhip_field_download": [_p, _p, C.c_size_t],
    "xlbhip_field_plane_download": [_p, _i, _i, _p, C.c_size_t],
    "xlbhip_field_plane_upload": [_p, _i, _i, _p, C.c_size_t],
    "xlbhip_field_touch": [_p],
    "xlbhip_mem_info": [_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "xlbhip_field_info": [_p, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i),
                          C.POINTER(C.c_uint64), _pp],
    "xlbhip_stream": [_p, _i, _p, _p],
    "xlbhip_equilibrium": [_p, _i, _i, _p, _p, _p],
    "xlbhip_macroscopic": [_p, _i, _i, _p, _p, _p],
    "xlbhip_second_moment": [_p, _i, _i, _p, _p],
    "xlbhip_vorticity": [_p, _p, _p, _p, _p],
    "xlbhip_mesh_mask_aabb": [_p, _i, _i, _i64, _p, _p, _p],
    "xlbhip_mesh_mask_ray": [_p, _i, _i, _i64, _p, _p, _p],
    "xlbhip_mesh_mask": [_p, _i, _i, _i, _i64, _p, _i, _p, _p, _p],
    "xlbhip_field_gather": [_p, _i64, _p, _p, C.c_size_t],
    "xlbhip_stepper_set_bc_distances": [_p, _i64, _p, _p],
    "xlbhip_stepper_momentum_transfer": [_p, _i, _p, _p, _p, C.POINTER(C.c_double)],
    "xlbhip_grid_to_point": [_p, _p, _i64, _p, _p],
    "xlbhip_momentum_transfer": [_p, _i, _i, C.POINTER(BcDesc), _p, _p, _p, C.POINTER(C.c_double)],
    "xlbhip_stepper_set_bc_profile": [_p, _i, _i64, _p, _p],
    "xlbhip_stepper_set_bc_profile_cells": [_p, _i, _i64, _p],
    "xlbhip_stepper_profile_slots": [_p, C.POINTER(_i)],
    "xlbhip_stepper_stage_bc_profiles": [_p, _i64, _i64, _p],
    "xlbhip_stepper_momentum_transfer_at": [_p, _i, _i64, _p, _p, _p, C.POINTER(C.c_double)],
    "xlbhip_apply_bc_profile": [_p, _i, _i, C.POINTER(BcDesc), _p, _p, _p, _p, _i64, _p, _p],
    "xlbhip_q_criterion": [_p, _p, _p, _p, _p],
    "xlbhip_collide": [_p, _i, _i, _i, _p, _p, _p, _d],
    "xlbhip_apply_bc": [_p, _i, _i, C.POINTER(BcDesc), _p, _p, _p, _p],
    "xlbhip_build_masks": [_p, _i, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p],
    "xlbhip_stepper_create": [_p, _i, _i, _i, _i, _i, C.POINTER(BcDesc), _pp],
    "xlbhip_stepper_destroy": [_p],
    "xlbhip_stepper_set_force": [_p, _p],
    "xlbhip_stepper_set_smagorinsky": [_p, _d],
    "xlbhip_step": [_p, _p, _p, _p, _p, _d, _i64],
    "xlbhip_run": [_p, _p, _p, _p, _p, _d, _i64, _i64],
    "xlbhip_run_timed": [_p, _p, _p, _p, _p, _d, _i64, _i64, C.POINTER(C.c_float), C.POINTER(C.c_int)],
    "xlbhip_run_any": [_p, _p, _p, _p, _p, _d, _i64, _i64, C.POINTER(C.c_int)],
    "xlbhip_comm_unique_id": [_p],
    "xlbhip_comm_init": [_p, _i, _i, _p, _i],
    "xlbhip_comm_init_ipc": [_p, _i, _i, C.c_char_p, _i],
    "xlbhip_comm_destroy": [_p],
    "xlbhip_comm_stats": [_p, C.POINTER(C.c_double), C.POINTER(_i64), _i],
    "xlbhip_halo_exchange": [_p, _i, _p],
    "xlbhip_halo_exchange_wide": [_p, _i, _p],
    "xlbhip_step2_eligible": [_p, _p, _p, _p, _p],
    "xlbhip_step2_plan": [_p, _p, _p, _p, _p, _p, _i64, C.POINTER(_i64)],
    "xlbhip_step2": [_p, _p, _p, _p, _p, _d, _i64],
    "xlbhip_ibm_create": [_p, _p, _i, _i, _i, _i, _i, _i, _i, _d, _d, _pp],
    "xlbhip_ibm_destroy": [_p],
    "xlbhip_ibm_set_markers": [_p, _i64, _p, _p, _p],
    "xlbhip_ibm_step": [_p, _p, _p, _p, _p, _d, _i64],
    "xlbhip_ibm_run": [_p, _p, _p, _p, _p, _d, _i64, _i64, C.POINTER(C.c_int)],
    "xlbhip_ibm_forces": [_p, _i64, _p],
    "xlbhip_ibm_iterations": [_p, C.POINTER(_i)],
    "xlbhip_ibm_footprint": [_p, C.POINTER(_i64), _i64, _p],
    "xlbhip_ibm_set_bodies": [_p, _i, _p, _p, _p, _p],
    "xlbhip_ibm_stage_poses": [_p, _i64, _i64, _p],
    "xlbhip_ibm_loads": [_p, _i, _p],
    "xlbhip_ibm_record_loads": [_p, _i64],
    "xlbhip_ibm_loads_history": [_p, _i64, _p],
    "xlbhip_ibm_download_markers": [_p, _i64, _p, _p],
    "xlbhip_ibm_set_dynamics": [_p, _i, _p, _p, _p],
    "xlbhip_ibm_body_poses": [_p, _i, _p, C.POINTER(C.c_uint64)],
    "xlbhip_ibm_record_poses": [_p, _i64],
    "xlbhip_ibm_poses_history": [_p, _i64, _p],
    "xlbhip_ibm_set_virtual_mass": [_p, _i, _p, _p],
    "xlbhip_ibm_set_contact": [_p, _i, _p, _d, _d, _d, _p, _p],
    "xlbhip_ibm_contact_forces": [_p, _i, _p],
    "xlbhip_stats_create": [_p, _i, _i, _i, _i, _i, _i, _i, _p, _pp],
    "xlbhip_stats_destroy": [_p],
    "xlbhip_stats_sample": [_p, _p, _p],
    "xlbhip_stats_read": [_p, _i64, _p, C.POINTER(_i64), C.POINTER(_d), _p],
    "xlbhip_stats_reset": [_p],
    "xlbhip_scalar_create": [_p, _i, _i, _i, _i, _i, C.POINTER(BcDesc), _pp],
    "xlbhip_scalar_destroy": [_p],
    "xlbhip_scalar_set_rules": [_p, _i, _p, _p, _p],
    "xlbhip_scalar_set_coupling": [_p, _p, _p, _d, _d],
    "xlbhip_scalar_init": [_p, _p, _p, _d, _p],
    "xlbhip_scalar_moment": [_p, _i, _i, _p, _p],
    "xlbhip_scalar_step": [_p, _p, _p, _p, _p, _p, _p, _d, _d, _i64],
    "xlbhip_scalar_run": [_p, _p, _p, _p, _p, _p, _p, _d, _d, _i64, _i64, C.POINTER(C.c_int)],
    "xlbhip_adjoint_create": [_p, _i, _i, _i, _i, C.POINTER(BcDesc), _pp],
    "xlbhip_adjoint_destroy": [_p],
    "xlbhip_adjoint_step": [_p, _p, _p, _p, _p, _p, _d],
    "xlbhip_adjoint_run": [_p, _i64, _pp, _p, _p, _p, _p, _d, C.POINTER(C.c_int)],
    "xlbhip_adjoint_omega_gradient": [_p, C.POINTER(_d)],
    "xlbhip_adjoint_reset": [_p],
    "xlbhip_macroscopic_adjoint": [_p, _i, _i, _p, _p, _p, _p],
    "xlbhip_porous_create": [_p, _i, _i, _i, _i, C.POINTER(BcDesc), _pp],
    "xlbhip_porous_destroy": [_p],
    "xlbhip_porous_set_solidity": [_p, _p],
    "xlbhip_porous_step": [_p, _p, _p, _p, _p, _d, _i64],
    "xlbhip_porous_run": [_p, _p, _p, _p, _p, _d, _i64, _i64, C.POINTER(C.c_int)],
    "xlbhip_porous_adjoint_step": [_p, _p, _p, _p, _p, _p, _d],
    "xlbhip_porous_adjoint_run": [_p, _i64, _pp, _p, _p, _p, _p, _d, C.POINTER(C.c_int)],
    "xlbhip_porous_adjoint_reset": [_p],
    "xlbhip_porous_omega_gradient": [_p, C.POINTER(_d)],
    "xlbhip_porous_solidity_gradient": [_p, _p],
    "xlbhip_multiphase_create": [_p, _i, _i, _i, _i, C.POINTER(BcDesc), _pp],
    "xlbhip_multiphase_destroy": [_p],
    "xlbhip_multiphase_set_model": [_p, _i, _d, _i, _p, _p],
    "xlbhip_multiphase_set_wall_density": [_p, _i, _p, _p, _p],
    "xlbhip_multiphase_step": [_p, _p, _p, _p, _p, _d, _i64],
    "xlbhip_multiphase_run": [_p, _p, _p, _p, _p, _d, _i64, _i64, C.POINTER(C.c_int)],
    "xlbhip_multiphase_psi": [_p, _p, _p, _p, _p],
    "xlbhip_multiphase_force": [_p, _p, _p, _p, _p],
    "xlbhip_multiphase_macroscopic": [_p, _p, _p, _p, _p, _p],
    "xlbhip_multicomponent_create": [_p, _i, _i, _i, _i, C.POINTER(BcDesc), _pp],
    "xlbhip_multicomponent_destroy": [_p],
    "xlbhip_multicomponent_set_model": [_p, _d, _d, _d, _p],
    "xlbhip_multicomponent_set_wall_density": [_p, _i, _p, _p, _p],
    "xlbhip_multicomponent_step": [_p, _p, _p, _p, _p, _p, _p, _d, _d, _i64],
    "xlbhip_multicomponent_run": [_p, _p, _p, _p, _p, _p, _p, _d, _d, _i64, _i64, C.POINTER(C.c_int)],
    "xlbhip_multicomponent_densities": [_p, _p, _p, _p, _p, _p, _p],
    "xlbhip_multicomponent_force": [_p, _p, _p, _p, _p, _p, _p],
    "xlbhip_multicomponent_macroscopic": [_p, _p, _p, _p, _p, _p, _p, _p],
}

_lib = None


def load():
    """Load libxlbhip.so; fail loudly when it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipBackendError(
            f"{LIB_PATH} not found: build it with `make` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "xlb_amd has no CPU fallback."
        )
    # Multi-process runs share device memory through dmabuf IPC on this driver stack; the HIP runtime reads the switch
    # when it initialises, i.e. with the first call into the library (RCCL: "hipIpcGetMemHandle: invalid argument" otherwise)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.xlbhip_last_error.argtypes = []
    lib.xlbhip_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise HipBackendError(load().xlbhip_last_error().decode("utf-8", "replace"))


def lattice_info(lattice_id):
    lib = load()
    d, q = _i(), _i()
    c = np.zeros((3, 27), np.int32)
    w = np.zeros(27, np.float64)
    opp = np.zeros(27, np.int32)
    cc = np.zeros((27, 6), np.int32)
    cbuf = np.zeros(3 * 27, np.int32)
    ccbuf = np.zeros(27 * 6, np.int32)
    check(lib.xlbhip_lattice_info(lattice_id, C.byref(d), C.byref(q), cbuf.ctypes.data, w.ctypes.data, opp.ctypes.data, ccbuf.ctypes.data))
    qq = q.value
    c = cbuf[: 3 * qq].reshape(3, qq)
    cc = ccbuf[: qq * 6].reshape(qq, 6)
    return d.value, qq, c, w[:qq].copy(), opp[:qq].copy(), cc


class DeferredWork:
    """Who has device work deferred (no library needed: a host test derives its stand-in context from this).  Weak references to
    objects with a ``flush_deferred()`` — operator/stepper/call_pairing.py registers itself when it defers a reference-style call."""

    def __init__(self):
        self._flushers = []

    def defers_work(self, obj):
        if not any(ref() is obj for ref in self._flushers):
            self._flushers.append(weakref.ref(obj))

    def flush_deferred(self):
        """Enqueue whatever work operators have deferred; forget those that are gone."""
        alive = [obj for obj in (ref() for ref in self._flushers) if obj is not None]
        self._flushers = [weakref.ref(obj) for obj in alive]
        for obj in alive:
            obj.flush_deferred()


class Context(DeferredWork):
    """Device context: HIP device + compute/communication streams (xlbhip_create)."""

    def __init__(self, device=0):
        super().__init__()
        self._h = _p()
        check(load().xlbhip_create(int(device), C.byref(self._h)))
        self.device = int(device)
        self.rank, self.n_ranks = 0, 1

    @property
    def handle(self):
        if not self._h:
            raise HipBackendError("context already destroyed")
        return self._h

    def sync(self):
        self.flush_deferred()
        check(load().xlbhip_sync(self.handle))

    def set_option(self, key, value):
        check(load().xlbhip_set_option(self.handle, key.encode(), int(value)))

    def get_option(self, key):
        v = _i64()
        check(load().xlbhip_get_option(self.handle, key.encode(), C.byref(v)))
        return v.value

    def mem_info(self):
        """(free, total) device memory in bytes."""
        fr, tot = C.c_uint64(), C.c_uint64()
        check(load().xlbhip_mem_info(self.handle, C.byref(fr), C.byref(tot)))
        return fr.value, tot.value

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, hbm = _i(), C.c_uint64()
        check(load().xlbhip_device_info(self.handle, name, 256, C.byref(cus), C.byref(hbm)))
        return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": hbm.value}

    def comm_init(self, rank, n_ranks, id_bytes, periodic_x=True):
        buf = C.create_string_buffer(bytes(id_bytes), UNIQUE_ID_BYTES) if id_bytes is not None else None
        check(load().xlbhip_comm_init(self.handle, int(rank), int(n_ranks), buf, 1 if periodic_x else 0))
        self.rank, self.n_ranks = int(rank), int(n_ranks)

    def comm_init_ipc(self, rank, n_ranks, token, periodic_x=True):
        """Join the IPC halo transport of the job named by ``token`` (xlbhip_comm_init_ipc)."""
        check(load().xlbhip_comm_init_ipc(self.handle, int(rank), int(n_ranks), str(token).encode(), 1 if periodic_x else 0))
        self.rank, self.n_ranks = int(rank), int(n_ranks)

    def comm_destroy(self):
        check(load().xlbhip_comm_destroy(self.handle))

    def comm_stats(self, reset=False):
        """{"halo_wait_ms": ..., "halo_waits": ...}: time the compute stream waited for halo exchanges (xlbhip_comm_stats)."""
        ms, n = C.c_double(), _i64()
        check(load().xlbhip_comm_stats(self.handle, C.byref(ms), C.byref(n), 1 if reset else 0))
        return {"halo_wait_ms": ms.value, "halo_waits": n.value}

    def close(self):
        if self._h:
            load().xlbhip_destroy(self._h)
            self._h = _p()


def comm_unique_id():
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    check(load().xlbhip_comm_unique_id(buf))
    return buf.raw


# ---- DLPack (dlpack.h v0.8 ABI) through ctypes: no extension module needed ---------------------------------
class _DLDevice(C.Structure):
    _fields_ = [("device_type", C.c_int), ("device_id", C.c_int)]


class _DLDataType(C.Structure):
    _fields_ = [("code", C.c_uint8), ("bits", C.c_uint8), ("lanes", C.c_uint16)]


class _DLTensor(C.Structure):
    _fields_ = [("data", C.c_void_p), ("device", _DLDevice), ("ndim", C.c_int), ("dtype", _DLDataType),
                ("shape", C.POINTER(C.c_int64)), ("strides", C.POINTER(C.c_int64)), ("byte_offset", C.c_uint64)]


class _DLManagedTensor(C.Structure):
    pass


_DL_DELETER = C.CFUNCTYPE(None, C.POINTER(_DLManagedTensor))
_DLManagedTensor._fields_ = [("dl_tensor", _DLTensor), ("manager_ctx", C.c_void_p), ("deleter", _DL_DELETER)]
_dl_alive = {}  # address of the managed tensor -> (managed tensor, shape/stride arrays, owner): kept until the consumer's deleter runs


@_DL_DELETER
def _dl_deleter(handle):
    try:
        _dl_alive.pop(C.addressof(handle.contents), None)
    except Exception:  # interpreter shutdown: the module globals may already be gone
        pass


# A consumer may drop its last tensor during interpreter finalisation, after this module's globals were cleared: the
# native thunk of the deleter must outlive everything, so it is leaked on purpose.
C.pythonapi.Py_IncRef(C.py_object(_dl_deleter))


# The capsule destructor runs while the capsule is being deallocated (reference count 0): it must see the raw
# PyObject* — a ctypes py_object argument would INCREF / DECREF the dying object and free it twice.
_PyCapsule_IsValid = C.PYFUNCTYPE(C.c_int, C.c_void_p, C.c_char_p)(("PyCapsule_IsValid", C.pythonapi))
_PyCapsule_GetPointer = C.PYFUNCTYPE(C.c_void_p, C.c_void_p, C.c_char_p)(("PyCapsule_GetPointer", C.pythonapi))
_PyCapsule_New = C.PYFUNCTYPE(C.py_object, C.c_void_p, C.c_char_p, C.c_void_p)(("PyCapsule_New", C.pythonapi))


@C.PYFUNCTYPE(None, C.c_void_p)
def _dl_capsule_destructor(capsule_ptr):
    # a capsule nobody consumed still carries the name "dltensor": release what it points to
    if _PyCapsule_IsValid(capsule_ptr, b"dltensor"):
        _dl_alive.pop(_PyCapsule_GetPointer(capsule_ptr, b"dltensor"), None)


def _dlpack_capsule(owner, ptr, shape, strides, dtype, device_id):
    nd = len(shape)
    shp = (C.c_int64 * nd)(*shape)
    std = (C.c_int64 * nd)(*strides)  # DLPack strides are in elements
    code = {"f": 2, "u": 1, "i": 0, "b": 6}[np.dtype(dtype).kind]
    m = _DLManagedTensor()
    m.dl_tensor = _DLTensor(C.c_void_p(ptr), _DLDevice(10, int(device_id)), nd, _DLDataType(code, np.dtype(dtype).itemsize * 8, 1),
                            C.cast(shp, C.POINTER(C.c_int64)), C.cast(std, C.POINTER(C.c_int64)), 0)
    m.manager_ctx = None
    m.deleter = _dl_deleter
    _dl_alive[C.addressof(m)] = (m, shp, std, owner)
    return _PyCapsule_New(C.addressof(m), b"dltensor", C.cast(_dl_capsule_destructor, C.c_void_p))


class HookedBuffer:
    """The part of a field that needs no library: a buffer handle and the hook rule (a host test derives its stand-in fields from
    this).  Whoever has deferred work that involves the field hooks it; every access goes through ``.handle``, which runs the hook
    first.  A subclass says in ``_release`` how the buffer is given back."""

    def __init__(self, handle):
        self._hook = None     # called before any access through .handle (deferred work that involves this field)
        self._pinned = False  # exported through DLPack / CUDA array interface: its device memory must never be swapped
        self._h = handle

    @property
    def handle(self):
        if self._hook is not None:
            hook, self._hook = self._hook, None
            try:
                hook(self)
            except BaseException:
                # the deferred work did not happen: whoever looks next must not see the field as if it had (a failed
                # materialisation of a virtual f(t+1) would otherwise hand out f(t))
                if self._hook is None:
                    self._hook = hook
                raise
        if not self._h:
            raise HipBackendError("field already destroyed")
        return self._h

    hook = property(lambda self: self._hook)

    def hook_with(self, hook):
        self._hook = hook

    def unhook(self, only=None):
        """Nothing is owed on this field any more; with `only`, unless another hook has taken that one's place."""
        if only is None or self._hook is only:
            self._hook = None

    def exchange_buffers(self, other):
        """The two objects trade what they hold (a fused pair leaves its result next to the source; a virtual field adopts its temporary)."""
        self._h, other._h = other._h, self._h

    def free(self):
        if self._hook is not None:  # what is owed runs while the buffer still exists (a freed mask: the step issued with it)
            hook, self._hook = self._hook, None
            try:
                hook(self)
            except Exception:
                pass
        self._release()

    def __del__(self):
        try:
            self._hook = None  # an abandoned field owes nothing: nobody can look at it
            self._release()
        except Exception:
            pass


class Field(HookedBuffer):
    """A device-resident field.  Host-visible shape is (cardinality, nx, ny[, nz]) C-order,
    exactly the reference layout; the device layout is private."""

    def __init__(self, ctx, cardinality, shape, dtype_code, halo=0, fill_value=0.0):
        super().__init__(_p())
        self.ctx = ctx
        self.cardinality = int(cardinality)
        self.grid_shape = tuple(int(s) for s in shape)
        assert len(self.grid_shape) in (2, 3)
        self.dtype_code = int(dtype_code)
        self.halo = int(halo)
        s3 = (1,) + self.grid_shape if len(self.grid_shape) == 2 else self.grid_shape
        self._s3 = s3
        check(load().xlbhip_field_create(ctx.handle, self.cardinality, s3[0], s3[1], s3[2], self.dtype_code, self.halo,
                                         float(fill_value or 0.0), C.byref(self._h)))

    # -- reference-like attributes
    @property
    def shape(self):
        return (self.cardinality,) + self.grid_shape

    @property
    def dtype(self):
        return np.dtype(NP_OF_DTYPE[self.dtype_code])

    def touch(self):
        """The contents changed behind the library's back (a write through a zero-copy alias): invalidate what is cached on them."""
        check(load().xlbhip_field_touch(self.handle))

    @property
    def nbytes_host(self):
        return int(np.prod(self.shape)) * self.dtype.itemsize

    def numpy(self):
        """Synchronous device -> host copy in the reference layout."""
        out = np.empty(self.shape, dtype=self.dtype)
        check(load().xlbhip_field_download(self.handle, out.ctypes.data, out.nbytes))
        return out

    # -- zero-copy export (what replaces the reference's ToJAX / warp_array_to_jax helpers, utils/utils.py:340-447):
    #    the interior of the field as a strided (cardinality, nx, ny[, nz]) device array.  The population planes are
    #    `plane_stride` elements apart (padding, ghost planes), which strides express exactly.
    def _device_view(self):
        if self.dtype_code == MISSING:
            raise HipBackendError("the bit-packed missing_mask has no array view; use numpy()")
        info = self.info()
        item = self.dtype.itemsize
        ny, nz = self._s3[1], self._s3[2]
        ptr = info["device_ptr"] + self.halo * ny * nz * item
        strides = (info["plane_stride"], ny * nz, nz, 1) if len(self.grid_shape) == 3 else (info["plane_stride"], nz, 1)
        return ptr, self.shape, strides, item

    @property
    def __cuda_array_interface__(self):
        """CUDA Array Interface v3 (PyTorch-ROCm, CuPy-ROCm and Numba consume it): ``torch.as_tensor(field, device="cuda")``
        aliases the field's memory.  Work enqueued on the backend's stream is finished first."""
        ptr, shape, strides, item = self._device_view()
        self._pinned = True
        self.ctx.sync()
        return {"shape": shape, "strides": tuple(s * item for s in strides), "typestr": self.dtype.str, "data": (ptr, False), "version": 3}

    def __dlpack_device__(self):
        return (10, self.ctx.device)  # kDLROCM

    def __dlpack__(self, stream=None, **_):
        """DLPack capsule of the same strided view (``torch.from_dlpack(field)``).  The consumer's stream is not known to
        this backend, so the backend's own stream is drained before the capsule is handed out."""
        ptr, shape, strides, item = self._device_view()
        self._pinned = True
        self.ctx.sync()
        return _dlpack_capsule(self, ptr, shape, strides, self.dtype, self.ctx.device)

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype)

    def assign(self, array):
        a = np.ascontiguousarray(np.asarray(array), dtype=self.dtype)
        if a.shape != self.shape:
            raise ValueError(f"shape {a.shape} does not match field shape {self.shape}")
        check(load().xlbhip_field_upload(self.handle, a.ctypes.data, a.nbytes))
        return self

    def fill(self, value):
        check(load().xlbhip_field_fill(self.handle, float(value)))
        return self

    def copy_from(self, other):
        check(load().xlbhip_field_copy(self.handle, other.handle))
        return self

    @property
    def plane_dtype(self):
        """dtype of one device x-plane: the field's dtype, or uint32 bit-sets for the bit-packed missing_mask (population 0)"""
        return np.dtype(np.uint32) if self.dtype_code == MISSING else np.dtype(self.dtype)

    def get_plane(self, population, storage_plane):
        """One x-plane (ny, nz) of one population; storage_plane counts the left ghosts (if any) from 0."""
        out = np.empty(self._s3[1:], dtype=self.plane_dtype)
        check(load().xlbhip_field_plane_download(self.handle, int(population), int(storage_plane), out.ctypes.data, out.nbytes))
        return out

    def set_plane(self, population, storage_plane, array):
        a = np.ascontiguousarray(array, dtype=self.plane_dtype)
        assert a.shape == tuple(self._s3[1:])
        check(load().xlbhip_field_plane_upload(self.handle, int(population), int(storage_plane), a.ctypes.data, a.nbytes))

    def gather(self, cells):
        """Rows of the field at interior linear cell indices ((x * ny + y) * nz + z): an (n, cardinality) array."""
        k = np.ascontiguousarray(cells, dtype=np.uint32)
        out = np.empty((k.shape[0], self.cardinality), dtype=self.dtype)
        check(load().xlbhip_field_gather(self.handle, int(k.shape[0]), k.ctypes.data, out.ctypes.data, out.nbytes))
        return out

    def copy_kernel_from(self, other, bytes_per_lane=16):
        check(load().xlbhip_field_copy_kernel(self.handle, other.handle, int(bytes_per_lane)))
        return self

    def copy_tiles_from(self, other):
        """The copy with the two-step kernel's launch shape (bench.py's second yardstick)."""
        check(load().xlbhip_field_copy_tiles(self.handle, other.handle))
        return self

    def info(self):
        card, nx, ny, nz, dt, halo = _i(), _i(), _i(), _i(), _i(), _i()
        ps, ptr = C.c_uint64(), _p()
        check(load().xlbhip_field_info(self.handle, C.byref(card), C.byref(nx), C.byref(ny), C.byref(nz), C.byref(dt), C.byref(halo),
                                       C.byref(ps), C.byref(ptr)))
        return {"cardinality": card.value, "nx": nx.value, "ny": ny.value, "nz": nz.value, "dtype": dt.value, "halo": halo.value,
                "plane_stride": ps.value, "device_ptr": ptr.value}

    def _release(self):
        if self._h:
            load().xlbhip_field_destroy(self._h)
            self._h = _p()

    def __repr__(self):
        return f"HipField(shape={self.shape}, dtype={self.dtype}, halo={self.halo})"


def make_bc_desc(bc_id, kind, values):
    d = BcDesc()
    d.id = int(bc_id)
    d.kind = int(kind)
    v = np.zeros(27, np.float64)
    if values is not None:
        values = np.asarray(values, np.float64).ravel()
        v[: values.size] = values
    for i in range(27):
        d.values[i] = v[i]
    return d


def _h(field):
    """handle of an optional mask argument.  A mask that was exported as a writable zero-copy alias (DLPack / CUDA array
    interface) may have been edited by the consumer without any C-ABI call: it counts as modified every time it is used."""
    if field is None:
        return None
    if field._pinned:
        field.touch()
    return field.handle


def _hf(field):
    """handle of a population field argument: one that was exported as a writable zero-copy alias may have been written by its
    consumer, so what the library caches on its contents (the two-step kernel's strip buffer) is dropped first."""
    if field._pinned:
        field.touch()
    return field.handle


class _Native:
    """A native object behind the handle ``_h``: made by xlbhip_<_kind>_create(context, ..., &handle), given back by xlbhip_<_kind>_destroy."""

    def __init__(self, ctx, *create_args):
        self.ctx, self._h = ctx, _p()
        check(getattr(load(), f"xlbhip_{self._kind}_create")(ctx.handle, *create_args, C.byref(self._h)))

    def free(self):
        if self._h:
            getattr(load(), f"xlbhip_{self._kind}_destroy")(self._h)
            self._h = _p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _bc_array(bc_descs):
    """(n, BcDesc[n]) as the xlbhip_*_create functions take the boundary conditions (never a zero-length array)"""
    return len(bc_descs), (BcDesc * max(len(bc_descs), 1))(*bc_descs)


class Stepper(_Native):
    """Native stepper object (xlbhip_stepper_create)."""

    _kind = "stepper"

    def __init__(self, ctx, lattice_id, collision_id, compute_code, store_code, bc_descs):
        super().__init__(ctx, lattice_id, collision_id, compute_code, store_code, *_bc_array(bc_descs))

    def set_force(self, force3):
        if force3 is None:
            check(load().xlbhip_stepper_set_force(self._h, None))
        else:
            arr = (C.c_double * 3)(*[float(x) for x in force3])
            check(load().xlbhip_stepper_set_force(self._h, C.cast(arr, C.c_void_p)))

    def set_bc_profile(self, bc_id, storage_cells, values):
        """Per-cell prescribed values of a Zou-He / Regularized BC: storage cell indices (uint32) and (n, 3) values."""
        k = np.ascontiguousarray(storage_cells, dtype=np.uint32)
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, 3)
        assert k.shape[0] == v.shape[0]
        check(load().xlbhip_stepper_set_bc_profile(self._h, int(bc_id), int(k.shape[0]), k.ctypes.data, v.ctypes.data))

    def set_bc_distances(self, storage_cells, weights):
        """Wall-distance weights of HybridBC cells: storage cell indices (uint32) and (n, q) float32 weights."""
        k = np.ascontiguousarray(storage_cells, dtype=np.uint32)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        assert w.ndim == 2 and k.shape[0] == w.shape[0]
        check(load().xlbhip_stepper_set_bc_distances(self._h, int(k.shape[0]), k.ctypes.data, w.ctypes.data))

    def set_bc_profile_cells(self, bc_id, storage_cells):
        """Storage cells of a time-dependent wall (HalfwayBounceBackBC / HybridBC with profile(cells, timestep)): values per timestep follow
        through stage_bc_profiles, in the order of these calls."""
        k = np.ascontiguousarray(storage_cells, dtype=np.uint32)
        check(load().xlbhip_stepper_set_bc_profile_cells(self._h, int(bc_id), int(k.shape[0]), k.ctypes.data))

    def profile_slots(self):
        """Per-timestep tables the stepper keeps resident (0 without time-dependent walls)."""
        n = _i()
        check(load().xlbhip_stepper_profile_slots(self._h, C.byref(n)))
        return n.value

    def stage_bc_profiles(self, t_first, values):
        """Wall velocities of the timesteps t_first, t_first + 1, ...: (n_steps, n_cells, 3) float64, the cells in declaration order."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        assert v.ndim == 3 and v.shape[2] == 3
        check(load().xlbhip_stepper_stage_bc_profiles(self._h, int(t_first), int(v.shape[0]), v.ctypes.data))

    def momentum_transfer(self, bc_id, f_0, bc_mask, missing_mask):
        """Force (3,) on the solid behind a HybridBC / profile wall of this stepper (its distance and velocity tables)."""
        out = (C.c_double * 3)()
        check(load().xlbhip_stepper_momentum_transfer(self._h, int(bc_id), f_0.handle, _h(bc_mask), _h(missing_mask), out))
        return np.array(out[:], dtype=np.float64)

    def momentum_transfer_at(self, bc_id, timestep, f_0, bc_mask, missing_mask):
        """As momentum_transfer with the wall velocities of `timestep` (a time-dependent wall needs it staged)."""
        out = (C.c_double * 3)()
        check(load().xlbhip_stepper_momentum_transfer_at(self._h, int(bc_id), int(timestep), f_0.handle, _h(bc_mask), _h(missing_mask), out))
        return np.array(out[:], dtype=np.float64)

    def set_smagorinsky(self, coef):
        check(load().xlbhip_stepper_set_smagorinsky(self._h, float(coef)))

    def step(self, f_src, f_dst, bc_mask, missing_mask, omega, timestep):
        check(load().xlbhip_step(self._h, _hf(f_src), _hf(f_dst), _h(bc_mask), _h(missing_mask), float(omega), int(timestep)))

    def step2_eligible(self, f_src, f_dst, bc_mask, missing_mask):
        return bool(load().xlbhip_step2_eligible(self._h, f_src.handle, f_dst.handle, _h(bc_mask), _h(missing_mask)))

    def step2_plan(self, f_src, f_dst, bc_mask, missing_mask):
        """The two-step launches the next pass f_src -> f_dst would make (xlbhip_step2_plan; nothing is stepped): a list of dicts
        with x_begin, x_count, segments, cap, tile (ty, tz), shift (oy, oz), strips and items, an (n, 4) int32 array of
        (tile index, x_lo, x_hi, clean flag) per block."""
        args = (self._h, f_src.handle, f_dst.handle, _h(bc_mask), _h(missing_mask))
        n = _i64()
        check(load().xlbhip_step2_plan(*args, None, 0, C.byref(n)))
        words = np.zeros(n.value, dtype=np.int32)
        check(load().xlbhip_step2_plan(*args, words.ctypes.data, n.value, C.byref(n)))
        assert n.value == words.size
        launches, o = [], 1
        for _ in range(int(words[0])):
            h = [int(v) for v in words[o : o + 10]]
            items = words[o + 10 : o + 10 + 4 * h[9]].reshape(h[9], 4).copy()
            launches.append(dict(x_begin=h[0], x_count=h[1], segments=h[2], cap=h[3], tile=(h[4], h[5]), shift=(h[6], h[7]), strips=h[8], items=items))
            o += 10 + 4 * h[9]
        assert o == words.size
        return launches

    def step2(self, f_src, f_dst, bc_mask, missing_mask, omega, timestep):
        """Two steps in one pass: f(t) in f_src -> f(t+2) in f_dst."""
        check(load().xlbhip_step2(self._h, _hf(f_src), _hf(f_dst), _h(bc_mask), _h(missing_mask), float(omega), int(timestep)))

    def run(self, f_a, f_b, bc_mask, missing_mask, omega, first_timestep, n_steps):
        """n steps; returns True when the result is in f_b (every pair of steps fused where the kernel exists)."""
        where = C.c_int()
        check(load().xlbhip_run_any(self._h, _hf(f_a), _hf(f_b), _h(bc_mask), _h(missing_mask), float(omega), int(first_timestep),
                                    int(n_steps), C.byref(where)))
        return bool(where.value)

    def run_timed(self, f_a, f_b, bc_mask, missing_mask, omega, first_timestep, n_steps):
        """As run(); returns (result is in f_b, device milliseconds)."""
        ms, where = C.c_float(), C.c_int()
        check(load().xlbhip_run_timed(self._h, _hf(f_a), _hf(f_b), _h(bc_mask), _h(missing_mask), float(omega), int(first_timestep),
                                      int(n_steps), C.byref(ms), C.byref(where)))
        return bool(where.value), ms.value


class IBM(_Native):
    """Native immersed-boundary object (xlbhip_ibm_create): the markers, their footprint and the coupling after a stepper's step."""

    _kind = "ibm"

    def __init__(self, ctx, stepper, lattice_id, compute_code, store_code, shape3, max_iterations, tolerance, relaxation):
        self._stepper = stepper  # (kept alive: the native object calls into it)
        self.n = 0
        self.n_bodies = 0
        super().__init__(ctx, stepper._h, lattice_id, compute_code, store_code, *map(int, shape3[:3]), int(max_iterations), float(tolerance), float(relaxation))

    @staticmethod
    def _f32(a, shape):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"marker array of shape {a.shape}, expected {shape}")
        return a

    def set_markers(self, n, positions=None, areas=None, velocities=None):
        """(n, 3) / (n,) / (n, 3) float32 arrays; None keeps what the device holds."""
        n = int(n)
        p, a, v = self._f32(positions, (n, 3)), self._f32(areas, (n,)), self._f32(velocities, (n, 3))
        check(load().xlbhip_ibm_set_markers(self._h, n, *(None if x is None else x.ctypes.data for x in (p, a, v))))
        self.n = n

    def step(self, f_src, f_dst, bc_mask, missing_mask, omega, timestep):
        check(load().xlbhip_ibm_step(self._h, _hf(f_src), _hf(f_dst), _h(bc_mask), _h(missing_mask), float(omega), int(timestep)))

    def run(self, f_a, f_b, bc_mask, missing_mask, omega, first_timestep, n_steps):
        where = C.c_int()
        check(load().xlbhip_ibm_run(self._h, _hf(f_a), _hf(f_b), _h(bc_mask), _h(missing_mask), float(omega), int(first_timestep), int(n_steps),
                                    C.byref(where)))
        return bool(where.value)

    def _read(self, name, shape):
        """float64 array of `shape` filled by the read-back xlbhip_ibm_<name>(handle, shape[0], out)"""
        out = np.zeros(shape, np.float64)
        check(getattr(load(), "xlbhip_ibm_" + name)(self._h, shape[0], out.ctypes.data))
        return out

    def forces(self):
        return self._read("forces", (self.n, 3))

    def iterations(self):
        n = _i()
        check(load().xlbhip_ibm_iterations(self._h, C.byref(n)))
        return n.value

    def footprint(self):
        """Linear cell indices ((x * ny + y) * nz + z) of the cells the coupling touches."""
        n = _i64()
        check(load().xlbhip_ibm_footprint(self._h, C.byref(n), 0, None))
        cells = np.zeros(n.value, np.uint32)
        if n.value:
            check(load().xlbhip_ibm_footprint(self._h, C.byref(n), cells.size, cells.ctypes.data))
        return cells

    POSE_BYTES = 1 << 20  # XLBHIP_IBM_POSE_BYTES: what stage_poses takes at once

    def set_bodies(self, first, count, moving, centre0):
        """Ranges [first, first + count) of the markers, which of them move, their reference points (n_bodies, 3)."""
        first, count = np.ascontiguousarray(first, np.int64), np.ascontiguousarray(count, np.int64)
        moving, centre0 = np.ascontiguousarray(moving, np.int32), np.ascontiguousarray(centre0, np.float64)
        check(load().xlbhip_ibm_set_bodies(self._h, len(first), first.ctypes.data, count.ctypes.data, moving.ctypes.data, centre0.ctypes.data))
        self.n_bodies = len(first)

    def stage_poses(self, first_timestep, poses):
        """(n_steps, n_bodies, 18) float64: R | c | w | v of timesteps first_timestep ..."""
        poses = np.ascontiguousarray(poses, np.float64)
        if poses.ndim != 3 or poses.shape[1:] != (self.n_bodies, 18):
            raise ValueError(f"poses of shape {poses.shape}, expected (n_steps, {self.n_bodies}, 18)")
        check(load().xlbhip_ibm_stage_poses(self._h, int(first_timestep), poses.shape[0], poses.ctypes.data))

    def loads(self):
        return self._read("loads", (self.n_bodies, 6))

    def record_loads(self, n_rows):
        check(load().xlbhip_ibm_record_loads(self._h, int(n_rows)))

    def loads_history(self, n_rows):
        return self._read("loads_history", (int(n_rows), self.n_bodies, 6))

    DYN_PARAM_DOUBLES, DYN_STATE_DOUBLES = 32, 16  # IBM_DYN_PARAM_DOUBLES, IBM_DYN_STATE_DOUBLES of csrc/ibm_dynamics_kernels.hpp

    def set_dynamics(self, rotate, params, state):
        """Rotation modes (n_bodies,), parameters (n_bodies, 32) and initial state (n_bodies, 16) of the dynamic bodies."""
        rotate = np.ascontiguousarray(rotate, np.int32)
        params, state = np.ascontiguousarray(params, np.float64), np.ascontiguousarray(state, np.float64)
        if rotate.shape != (self.n_bodies,) or params.shape != (self.n_bodies, self.DYN_PARAM_DOUBLES) or state.shape != (self.n_bodies, self.DYN_STATE_DOUBLES):
            raise ValueError(f"set_dynamics: expected ({self.n_bodies},), ({self.n_bodies}, 32) and ({self.n_bodies}, 16) arrays")
        check(load().xlbhip_ibm_set_dynamics(self._h, self.n_bodies, rotate.ctypes.data, params.ctypes.data, state.ctypes.data))

    def body_poses(self):
        """-> ((n_bodies, 18) poses the next step would read, the status word)."""
        out = np.zeros((self.n_bodies, 18), np.float64)
        status = C.c_uint64(0)
        check(load().xlbhip_ibm_body_poses(self._h, self.n_bodies, out.ctypes.data, C.byref(status)))
        return out, int(status.value)

    def record_poses(self, n_rows):
        check(load().xlbhip_ibm_record_poses(self._h, int(n_rows)))

    def poses_history(self, n_rows):
        return self._read("poses_history", (int(n_rows), self.n_bodies, 18))

    def set_virtual_mass(self, virtual_mass, virtual_inertia):
        """m_v and I_v of every body, (n_bodies,) each; after set_dynamics."""
        mv, iv = np.ascontiguousarray(virtual_mass, np.float64), np.ascontiguousarray(virtual_inertia, np.float64)
        if mv.shape != (self.n_bodies,) or iv.shape != (self.n_bodies,):
            raise ValueError(f"set_virtual_mass: expected two ({self.n_bodies},) arrays")
        check(load().xlbhip_ibm_set_virtual_mass(self._h, self.n_bodies, mv.ctypes.data, iv.ctypes.data))

    def set_contact(self, radius, range, stiffness, wall_stiffness, lo=None, hi=None):
        """Contact radii (n_bodies,), 0 = the body takes no part; the model's range and stiffnesses; planes lo / hi (3,) or None."""
        radius = np.ascontiguousarray(radius, np.float64)
        if radius.shape != (self.n_bodies,):
            raise ValueError(f"set_contact: expected ({self.n_bodies},) radii")
        lo = None if lo is None else np.ascontiguousarray(lo, np.float64).reshape(3)
        hi = None if hi is None else np.ascontiguousarray(hi, np.float64).reshape(3)
        check(load().xlbhip_ibm_set_contact(self._h, self.n_bodies, radius.ctypes.data, float(range), float(stiffness), float(wall_stiffness),
                                            None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data))

    def contact_forces(self):
        return self._read("contact_forces", (self.n_bodies, 3))

    def download_markers(self, positions=True, velocities=True):
        p = np.zeros((self.n, 3), np.float32) if positions else None
        v = np.zeros((self.n, 3), np.float32) if velocities else None
        check(load().xlbhip_ibm_download_markers(self._h, self.n, *(None if x is None else x.ctypes.data for x in (p, v))))
        return p, v


class Scalar(_Native):
    """Native scalar-transport object (xlbhip_scalar_create): the tables of the coupled fluid + scalar step."""

    _kind = "scalar"

    ADIABATIC, DIRICHLET, DO_NOTHING = 0, 1, 2  # SCALAR_* of csrc/scalar_kernels.hpp

    def __init__(self, ctx, lattice_id, collision_id, compute_code, store_code, bc_descs):
        super().__init__(ctx, lattice_id, collision_id, compute_code, store_code, *_bc_array(bc_descs))

    def set_rules(self, rules):
        """rules: [(bc id, ADIABATIC / DIRICHLET / DO_NOTHING, value)]"""
        ids = np.array([r[0] for r in rules], dtype=np.int32)
        kinds = np.array([r[1] for r in rules], dtype=np.int32)
        values = np.array([r[2] for r in rules], dtype=np.float64)
        check(load().xlbhip_scalar_set_rules(self._h, len(rules), ids.ctypes.data, kinds.ctypes.data, values.ctypes.data))

    def set_coupling(self, force3, buoyancy3, reference, smagorinsky_coef):
        f = None if force3 is None else np.ascontiguousarray(force3, dtype=np.float64)
        b = None if buoyancy3 is None else np.ascontiguousarray(buoyancy3, dtype=np.float64)
        check(load().xlbhip_scalar_set_coupling(self._h, None if f is None else f.ctypes.data, None if b is None else b.ctypes.data, float(reference),
                                                float(smagorinsky_coef)))

    def init(self, f_0, phi, phi0, g_0):
        check(load().xlbhip_scalar_init(self._h, _hf(f_0), _h(phi), float(phi0), _hf(g_0)))

    def step(self, f_src, f_dst, g_src, g_dst, bc_mask, missing_mask, omega, omega_scalar, timestep):
        check(load().xlbhip_scalar_step(self._h, _hf(f_src), _hf(f_dst), _hf(g_src), _hf(g_dst), _h(bc_mask), _h(missing_mask), float(omega),
                                        float(omega_scalar), int(timestep)))

    def run(self, f_a, f_b, g_a, g_b, bc_mask, missing_mask, omega, omega_scalar, first_timestep, n_steps):
        """n coupled steps; returns True when the result is in (f_b, g_b)."""
        where = C.c_int()
        check(load().xlbhip_scalar_run(self._h, _hf(f_a), _hf(f_b), _hf(g_a), _hf(g_b), _h(bc_mask), _h(missing_mask), float(omega),
                                       float(omega_scalar), int(first_timestep), int(n_steps), C.byref(where)))
        return bool(where.value)


class Adjoint(_Native):
    """Native adjoint object (xlbhip_adjoint_create): the boundary tables of the fused adjoint step and the device scalar dL/domega."""

    _kind = "adjoint"

    def __init__(self, ctx, lattice_id, compute_code, store_code, bc_descs):
        super().__init__(ctx, lattice_id, compute_code, store_code, *_bc_array(bc_descs))

    def step(self, f_n, lam_in, lam_out, bc_mask, missing_mask, omega):
        check(load().xlbhip_adjoint_step(self._h, _hf(f_n), _hf(lam_in), _hf(lam_out), _h(bc_mask), _h(missing_mask), float(omega)))

    def run(self, states, lam_a, lam_b, bc_mask, missing_mask, omega):
        """The adjoint steps over states = [f_0 .. f_{N-1}], last first, lam_N in lam_a; returns True when lam_0 is in lam_b."""
        where = C.c_int()
        arr = (C.c_void_p * max(len(states), 1))(*[_hf(f) for f in states])
        check(load().xlbhip_adjoint_run(self._h, len(states), arr, _hf(lam_a), _hf(lam_b), _h(bc_mask), _h(missing_mask), float(omega), C.byref(where)))
        return bool(where.value)

    def omega_gradient(self):
        out = _d()
        check(load().xlbhip_adjoint_omega_gradient(self._h, C.byref(out)))
        return out.value

    def reset(self):
        check(load().xlbhip_adjoint_reset(self._h))


class Porous(_Native):
    """Native porous object (xlbhip_porous_create): the boundary tables of the porous step and of its adjoint step, the binding of the
    solidity field, the device scalar dL/domega and the fp64 field dL/dalpha.  ``step`` / ``run`` are the forward step's, ``adjoint_step``
    / ``adjoint_run`` have the interface of ``Adjoint.step`` / ``Adjoint.run``."""

    _kind = "porous"

    def __init__(self, ctx, lattice_id, compute_code, store_code, bc_descs):
        super().__init__(ctx, lattice_id, compute_code, store_code, *_bc_array(bc_descs))
        self._alpha = None

    def set_solidity(self, alpha):
        check(load().xlbhip_porous_set_solidity(self._h, _h(alpha)))
        self._alpha = alpha  # (bound by reference: it outlives the binding)

    def step(self, f_src, f_dst, bc_mask, missing_mask, omega, timestep):
        check(load().xlbhip_porous_step(self._h, _hf(f_src), _hf(f_dst), _h(bc_mask), _h(missing_mask), float(omega), int(timestep)))

    def run(self, f_a, f_b, bc_mask, missing_mask, omega, first_timestep, n_steps):
        where = C.c_int()
        check(load().xlbhip_porous_run(self._h, _hf(f_a), _hf(f_b), _h(bc_mask), _h(missing_mask), float(omega), int(first_timestep), int(n_steps),
                                       C.byref(where)))
        return bool(where.value)

    def adjoint_step(self, f_n, lam_in, lam_out, bc_mask, missing_mask, omega):
        check(load().xlbhip_porous_adjoint_step(self._h, _hf(f_n), _hf(lam_in), _hf(lam_out), _h(bc_mask), _h(missing_mask), float(omega)))

    def adjoint_run(self, states, lam_a, lam_b, bc_mask, missing_mask, omega):
        where = C.c_int()
        arr = (C.c_void_p * max(len(states), 1))(*[_hf(f) for f in states])
        check(load().xlbhip_porous_adjoint_run(self._h, len(states), arr, _hf(lam_a), _hf(lam_b), _h(bc_mask), _h(missing_mask), float(omega),
                                               C.byref(where)))
        return bool(where.value)

    def omega_gradient(self):
        out = _d()
        check(load().xlbhip_porous_omega_gradient(self._h, C.byref(out)))
        return out.value

    def solidity_gradient(self, out):
        check(load().xlbhip_porous_solidity_gradient(self._h, _hf(out)))
        return out

    def reset(self):
        check(load().xlbhip_porous_adjoint_reset(self._h))


class Multiphase(_Native):
    """Native Shan-Chen object (xlbhip_multiphase_create): the boundary tables, the wall pseudopotentials and the psi field of the step."""

    _kind = "multiphase"

    EXPONENTIAL, DENSITY, CARNAHAN_STARLING = 0, 1, 2  # PSI_* of csrc/multiphase_kernels.hpp

    def __init__(self, ctx, lattice_id, compute_code, store_code, bc_descs):
        super().__init__(ctx, lattice_id, compute_code, store_code, *_bc_array(bc_descs))

    def set_model(self, form, g, params, force3):
        p = np.ascontiguousarray(params, dtype=np.float64)
        f = None if force3 is None else np.ascontiguousarray(force3, dtype=np.float64)
        check(load().xlbhip_multiphase_set_model(self._h, int(form), float(g), len(p), p.ctypes.data if len(p) else None, None if f is None else f.ctypes.data))

    def set_wall_density(self, walls):
        """walls: [(bc id, rho_w, Psi(rho_w) in the compute dtype)]"""
        ids = np.array([w[0] for w in walls], dtype=np.int32)
        rho = np.array([w[1] for w in walls], dtype=np.float64)
        psi = np.array([w[2] for w in walls], dtype=np.float64)
        check(load().xlbhip_multiphase_set_wall_density(self._h, len(walls), ids.ctypes.data, rho.ctypes.data, psi.ctypes.data))

    def step(self, f_src, f_dst, bc_mask, missing_mask, omega, timestep):
        check(load().xlbhip_multiphase_step(self._h, _hf(f_src), _hf(f_dst), _h(bc_mask), _h(missing_mask), float(omega), int(timestep)))

    def run(self, f_a, f_b, bc_mask, missing_mask, omega, first_timestep, n_steps):
        """n steps; returns True when the result is in f_b."""
        where = C.c_int()
        check(load().xlbhip_multiphase_run(self._h, _hf(f_a), _hf(f_b), _h(bc_mask), _h(missing_mask), float(omega), int(first_timestep), int(n_steps),
                                           C.byref(where)))
        return bool(where.value)

    def psi(self, f, bc_mask, missing_mask, out):
        check(load().xlbhip_multiphase_psi(self._h, _hf(f), _h(bc_mask), _h(missing_mask), _hf(out)))

    def force(self, f, bc_mask, missing_mask, out):
        check(load().xlbhip_multiphase_force(self._h, _hf(f), _h(bc_mask), _h(missing_mask), _hf(out)))

    def macroscopic(self, f, bc_mask, missing_mask, rho, u):
        check(load().xlbhip_multiphase_macroscopic(self._h, _hf(f), _h(bc_mask), _h(missing_mask), _hf(rho), _hf(u)))


class Multicomponent(_Native):
    """Native two-component Shan-Chen object (xlbhip_multicomponent_create): the boundary tables, the wall densities and the two density
    fields of the step."""

    _kind = "multicomponent"

    def __init__(self, ctx, lattice_id, compute_code, store_code, bc_descs):
        super().__init__(ctx, lattice_id, compute_code, store_code, *_bc_array(bc_descs))

    def set_model(self, g_aa, g_ab, g_bb, force3):
        f = None if force3 is None else np.ascontiguousarray(force3, dtype=np.float64)
        check(load().xlbhip_multicomponent_set_model(self._h, float(g_aa), float(g_ab), float(g_bb), None if f is None else f.ctypes.data))

    def set_wall_density(self, walls):
        """walls: [(bc id, rho_w of A, rho_w of B)]"""
        ids = np.array([w[0] for w in walls], dtype=np.int32)
        rho_a = np.array([w[1] for w in walls], dtype=np.float64)
        rho_b = np.array([w[2] for w in walls], dtype=np.float64)
        check(load().xlbhip_multicomponent_set_wall_density(self._h, len(walls), ids.ctypes.data, rho_a.ctypes.data, rho_b.ctypes.data))

    def step(self, fa_src, fa_dst, fb_src, fb_dst, bc_mask, missing_mask, omega_a, omega_b, timestep):
        check(load().xlbhip_multicomponent_step(self._h, _hf(fa_src), _hf(fa_dst), _hf(fb_src), _hf(fb_dst), _h(bc_mask), _h(missing_mask), float(omega_a),
                                                float(omega_b), int(timestep)))

    def run(self, fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, omega_a, omega_b, first_timestep, n_steps):
        """n steps; returns True when the result is in fa_1 and fb_1."""
        where = C.c_int()
        check(load().xlbhip_multicomponent_run(self._h, _hf(fa_0), _hf(fa_1), _hf(fb_0), _hf(fb_1), _h(bc_mask), _h(missing_mask), float(omega_a),
                                               float(omega_b), int(first_timestep), int(n_steps), C.byref(where)))
        return bool(where.value)

    def densities(self, fa, fb, bc_mask, missing_mask, rho_a, rho_b):
        check(load().xlbhip_multicomponent_densities(self._h, _hf(fa), _hf(fb), _h(bc_mask), _h(missing_mask), _hf(rho_a), _hf(rho_b)))

    def force(self, fa, fb, bc_mask, missing_mask, force_a, force_b):
        check(load().xlbhip_multicomponent_force(self._h, _hf(fa), _hf(fb), _h(bc_mask), _h(missing_mask), _hf(force_a), _hf(force_b)))

    def macroscopic(self, fa, fb, bc_mask, missing_mask, rho_a, rho_b, u):
        check(load().xlbhip_multicomponent_macroscopic(self._h, _hf(fa), _hf(fb), _h(bc_mask), _h(missing_mask), _hf(rho_a), _hf(rho_b), _hf(u)))


def macroscopic_adjoint(ctx, lattice_id, compute_code, f, rho_bar, u_bar, lam):
    check(load().xlbhip_macroscopic_adjoint(ctx.handle, lattice_id, compute_code, _hf(f), _h(rho_bar), _h(u_bar), _hf(lam)))


class Stats(_Native):
    """Native flow-statistics object (xlbhip_stats_create): running sums [channel][bin] and the watchdog's counters."""

    _kind = "stats"

    def __init__(self, ctx, lattice_id, compute_code, shape3, keep_mask, order, exclude_ids):
        bits = np.zeros(8, np.uint32)
        for v in exclude_ids:
            bits[int(v) >> 5] |= np.uint32(1 << (int(v) & 31))
        self.samples = 0
        super().__init__(ctx, lattice_id, compute_code, int(shape3[0]), int(shape3[1]), int(shape3[2]), int(keep_mask), int(order), bits.ctypes.data)

    def sample(self, f, bc_mask):
        # (read-only: through .handle, which flushes work deferred on the fields, without invalidating what is cached on them)
        check(load().xlbhip_stats_sample(self._h, f.handle, None if bc_mask is None else bc_mask.handle))
        self.samples += 1

    def read(self, n_sums):
        """(sums, samples, max u.u of the last sample, non-finite cells of the last sample, ... since the last reset); synchronises."""
        sums = np.zeros(int(n_sums), np.float64)
        samples, umax, bad = _i64(), _d(), np.zeros(2, np.int64)
        check(load().xlbhip_stats_read(self._h, sums.size, sums.ctypes.data, C.byref(samples), C.byref(umax), bad.ctypes.data))
        return sums, samples.value, umax.value, int(bad[0]), int(bad[1])

    def reset(self):
        check(load().xlbhip_stats_reset(self._h))
        self.samples = 0


def build_masks(ctx, lattice_id, bc_ids, tag_lists, solid_lists, global_shape3, x_offset, bc_mask, missing_mask):
    """tag_lists / solid_lists: per BC an int32 (3, n) array (or None)."""
    n = len(bc_ids)
    ids = np.asarray(bc_ids, np.int32)
    keep = []
    tag_ptrs = (C.c_void_p * max(n, 1))()
    sol_ptrs = (C.c_void_p * max(n, 1))()
    tag_cnt = np.zeros(max(n, 1), np.int64)
    sol_cnt = np.zeros(max(n, 1), np.int64)
    for i in range(n):
        t = np.ascontiguousarray(tag_lists[i], dtype=np.int32)
        assert t.ndim == 2 and t.shape[0] == 3
        keep.append(t)
        tag_ptrs[i] = t.ctypes.data
        tag_cnt[i] = t.shape[1]
        s = solid_lists[i]
        if s is not None and np.size(s) > 0:
            s = np.ascontiguousarray(s, dtype=np.int32)
            assert s.ndim == 2 and s.shape[0] == 3
            keep.append(s)
            sol_ptrs[i] = s.ctypes.data
            sol_cnt[i] = s.shape[1]
    gs = np.asarray(global_shape3, np.int32)
    check(load().xlbhip_build_masks(ctx.handle, lattice_id, n, ids.ctypes.data, C.cast(tag_ptrs, C.c_void_p), tag_cnt.ctypes.data,
                                    C.cast(sol_ptrs, C.c_void_p), sol_cnt.ctypes.data, gs.ctypes.data, int(x_offset), bc_mask.handle,
                                    missing_mask.handle))
    del keep
