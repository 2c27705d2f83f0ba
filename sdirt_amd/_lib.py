"""ctypes binding of libsdirt_dp.so (include/sdirt_dp.h).

The library is the product: there is NO CPU fallback.  If the shared object is
missing, `lib()` raises SdirtError telling how to build it; if no MI355X is
visible, the first device call fails with the HIP error text.
"""
import collections
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SDIRT_AMD_LIB overrides the path (kernel-variant A/B runs in tools/kbench.py only)
LIB_PATH = os.environ.get("SDIRT_AMD_LIB") or os.path.join(HERE, "libsdirt_dp.so")

ABI_VERSION = 4          # SDIRT_ABI_VERSION of include/sdirt_dp.h this binding was written against
MAX_SURFACES = 64
MAX_LAYERS = 16          # SDIRT_MAX_LAYERS
MAX_AI = 8
NEWTON_MAXITER = 10
MAX_KS = 141
MAX_KS_STAGED = 1024
MAX_WAVELENGTHS = 3
PSF_NORMALIZE = 1
PSF_STRICT_IEEE = 4
TRACE_NO_PREFETCH = 8
PSF_ONE_ROUND = 16
PSF_INTERLEAVED = 32
PSF_ZERO_CTL = 64
PSF_NO_VERIFY = 128
PSF_DETERMINISTIC = 256
CTL_STATUS, CTL_ANY_VALID, CTL_TRIPS2, CTL_MASKS, CTL_WORDS = 0, 1, 16, 64, 320
CTL_LANES = 1411
CTL_TAG = 2

CtlBlock = collections.namedtuple("CtlBlock", "status any_valid masks trips2")


def decode_ctl(words, K, one_round=False):
    """The control block of a device-verified psf call (its CTL_WORDS int32 words as the library leaves them) on a lens
    of K surfaces -> CtlBlock:
      status     0: the speculated trip tables were the reference's for the batch; else the device derived new ones
      any_valid  1 when some sampled ray was valid
      masks      [primary, chief-ray] convergence masks (K words each) of every round that ran: round 1, and round 2
                 when status != 0 unless the call ran one round only (SDIRT_PSF_ONE_ROUND)
      trips2     status != 0: the [primary, chief-ray] trip tables (int32 [K]) the device derived from round 1's masks,
                 packed as int8 at CTL_TRIPS2 (16 words per pass); None when status == 0"""
    w = np.asarray(words).astype(np.uint32)                  # a copy: the caller's buffer may be reused at once
    status = int(w[CTL_STATUS])
    rows = [w[CTL_MASKS + 64 * r:CTL_MASKS + 64 * r + K] for r in range(4 if status and not one_round else 2)]
    trips2 = None
    if status:
        # little-endian bytes of the words: table entry k is byte k
        packed = w[CTL_TRIPS2:CTL_TRIPS2 + 32].astype("<u4").view(np.int8).reshape(2, 64)[:, :K].astype(np.int32)
        trips2 = [packed[0], packed[1]]
    return CtlBlock(status, int(w[CTL_ANY_VALID]), [rows[i:i + 2] for i in range(0, len(rows), 2)], trips2)


KIND_PLANE, KIND_SPHERE, KIND_ASPHERE = 0, 1, 2


class SdirtError(RuntimeError):
    pass


class SurfaceDesc(C.Structure):
    """sdirt_surface_desc"""
    _fields_ = [("kind", C.c_int32), ("ai_degree", C.c_int32), ("r", C.c_double),
                ("d", C.c_float), ("c", C.c_float), ("k", C.c_float),
                ("ai", C.c_float * MAX_AI), ("n1", C.c_double), ("n2", C.c_double)]


class Rays(C.Structure):
    """sdirt_rays: eight device pointers"""
    _fields_ = [(n, C.c_void_p) for n in ("ox", "oy", "oz", "dx", "dy", "dz", "ra", "obliq")]


class DpParams(C.Structure):
    """sdirt_dp_params"""
    _fields_ = [("h", C.c_double), ("f", C.c_double), ("w", C.c_double), ("r", C.c_double)]


_P, _I64, _I32, _U32, _D = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_double

# name -> (restype, argtypes); mirrors include/sdirt_dp.h one to one
SIGNATURES = {
    "sdirt_abi_version": (C.c_int, []),
    "sdirt_last_error": (C.c_char_p, []),
    "sdirt_device_count": (C.c_int, []),
    "sdirt_lens_create": (C.c_int, [C.POINTER(SurfaceDesc), _I32, C.POINTER(_P)]),
    "sdirt_lens_destroy": (None, [_P]),
    "sdirt_lens_num_surfaces": (_I32, [_P]),
    "sdirt_lens_strict_ieee": (_I32, [_P]),
    "sdirt_points_to_object": (C.c_int, [_P, _I64, _D, _D, _D, _D, _P, _P]),
    "sdirt_pupil_samples": (C.c_int, [_P, _P, _I64, _D, _P, _P, _P]),
    "sdirt_sample_rays": (C.c_int, [_P, _I64, _P, _P, _I64, _D, Rays, _P]),
    "sdirt_rays_from_aos": (C.c_int, [_P, _P, _P, _I64, _I64, _I32, Rays, _P]),
    "sdirt_rays_to_aos": (C.c_int, [Rays, _I64, _I64, _P, _P, _P]),
    "sdirt_trace": (C.c_int, [_P, _I32, _I32, _I32, C.POINTER(_I32), _U32, Rays, _I64, _P, _P]),
    "sdirt_trace_to": (C.c_int, [_P, _I32, _I32, _I32, C.POINTER(_I32), _U32, Rays, Rays, _I64, _P, _P]),
    "sdirt_trace2sensor": (C.c_int, [_P, C.POINTER(_I32), _U32, _D, Rays, Rays, _I64, _P, _P]),
    "sdirt_propagate_to": (C.c_int, [_D, Rays, _I64, _P]),
    "sdirt_render_plane": (C.c_int, [_P, C.POINTER(_I32), _U32, _P, _P, _D, _P, _P, _D, _I32, _I32, _I32,
                                     C.POINTER(DpParams), _D, _D, _P, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    "sdirt_render_layers": (C.c_int, [_P, C.POINTER(_I32), _U32, _P, _P, _D, _P, _P, _D, _I32, _I32, _I32,
                                      C.POINTER(DpParams), _I32, C.POINTER(_D), C.POINTER(_D), _P, _P, _I64,
                                      _I32, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "sdirt_render_layers_grad": (C.c_int, [_P, C.POINTER(_I32), _U32, _P, _P, _D, _P, _P, _D, _I32, _I32, _I32,
                                           C.POINTER(DpParams), _I32, C.POINTER(_D), C.POINTER(_D), _P, _P, _I64,
                                           _I32, _I32, _I32, _P, _P, _P, _I64, _P]),
    "sdirt_render_layers_dp_grad": (C.c_int, [_P, C.POINTER(_I32), _U32, _P, _P, _D, _P, _P, _D, _I32, _I32, _I32,
                                              C.POINTER(DpParams), _I32, C.POINTER(_D), C.POINTER(_D), _P, _P, _I64,
                                              _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    "sdirt_render_layers_depth_grad": (C.c_int, [_P, C.POINTER(_I32), _U32, _P, _P, _D, _P, _P, _D, _I32, _I32, _I32,
                                                 C.POINTER(DpParams), _I32, C.POINTER(_D), C.POINTER(_D), _P, _P, _I64,
                                                 _I32, _I32, _I32, _P, _P, _P, _P]),
    "sdirt_center_from_rays": (C.c_int, [Rays, _I64, _I64, _P, _P, _P]),
    "sdirt_forward_integral": (C.c_int, [Rays, _I64, _I64, _D, _I32, _P, C.POINTER(DpParams), _U32,
                                         _P, _P, _P]),
    "sdirt_forward_integral_plan": (C.c_int, [_I64, _I64, _I32, _I32, _I32, C.POINTER(_I64)]),
    "sdirt_forward_integral_grad": (C.c_int, [Rays, _I64, _I64, _D, _I32, _P, C.POINTER(DpParams), _U32,
                                              _P, _P, _P, _I32, _P]),
    "sdirt_forward_integral_grad_focus": (C.c_int, [Rays, _I64, _I64, _D, _I32, _P, C.POINTER(DpParams), _U32,
                                                    _P, _P, _P, _I32, _P]),
    "sdirt_forward_integral_grad_slices": (_I32, [_I64, _I64, _I32]),
    "sdirt_forward_integral_grad_rays": (C.c_int, [Rays, _I64, _I64, _D, _I32, _P, C.POINTER(DpParams), _U32,
                                                   _P, _P, _P, _I32, _P, _P]),
    "sdirt_dp_energy": (C.c_int, [Rays, _I64, _I64, C.POINTER(DpParams), _U32, _P, _I32, _P]),
    "sdirt_dp_energy_grad": (C.c_int, [Rays, _I64, _I64, C.POINTER(DpParams), _U32, _P, _P, _I32, _P, _I32, _P]),
    "sdirt_trace2sensor_grad_workspace_bytes": (_I64, [_I64, _I32]),
    "sdirt_trace2sensor_record": (C.c_int, [_P, C.POINTER(_I32), _U32, _D, Rays, Rays, _I64, _P, _P, _P]),
    "sdirt_trace2sensor_grad_workgroups": (_I32, [_I64, _I32]),
    "sdirt_trace2sensor_grad": (C.c_int, [_P, C.POINTER(_I32), _U32, _D, _P, _P, _P, _I64, _P, _I32, _P]),
    "sdirt_trace2sensor_grad_eta": (C.c_int, [_P, C.POINTER(_I32), _U32, _D, _P, _P, _P, _I64, _P, _I32, _P]),
    "sdirt_trace2sensor_grad_points": (C.c_int, [_P, C.POINTER(_I32), _U32, _D, _P, _P, _P, _I64, _I64, _P, _P, _D, _P,
                                                 _I32, _P]),
    "sdirt_psf_normalize": (C.c_int, [_P, _I64, _I32, _P]),
    "sdirt_chief_center": (C.c_int, [_P, _P, _I64, _P, _P, _I64, _D, _D, C.POINTER(_I32), _U32,
                                     _P, _P, _P, _P]),
    "sdirt_chief_center_slope": (C.c_int, [_P, _P, _I64, _P, _P, _I64, _D, _D, C.POINTER(_I32), _U32,
                                           _P, _P, _P, _P, _P]),
    "sdirt_psf_lr": (C.c_int, [_P, _P, _I64, _P, _P, _I64, _D, _D, _D, _I32, _P,
                               C.POINTER(DpParams), C.POINTER(_I32), _U32, _P, _P, _P, _P]),
    "sdirt_psf_lr_centered": (C.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _D, _D, _D, _I32,
                                        C.POINTER(DpParams), C.POINTER(_I32), C.POINTER(_I32), _U32,
                                        _P, _P, _P, _P, _P, _P, _P]),
    "sdirt_psf_rgb_centered": (C.c_int, [C.POINTER(_P), _I32, _P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _D, _D, _D,
                                         _I32, C.POINTER(DpParams), C.POINTER(_I32), C.POINTER(_I32), _U32,
                                         _P, _P, _P, _P, _P, _P, _P]),
    "sdirt_psf_rgb": (C.c_int, [C.POINTER(_P), _I32, _P, _I64, _P, _P, _I64, _D, _D, _D, _I32, _P,
                                C.POINTER(DpParams), C.POINTER(_I32), _U32, _P, _P, _P, _P]),
    "sdirt_psf_spp_slices": (_I32, [_I64, _I64, _I32]),
    "sdirt_psf_verified_scratch_bytes": (_I64, [_I64, _I64]),
    "sdirt_psf_lr_verified": (C.c_int, [_P, _P, _P, _I64, _P, _P, _I64, _P, _P, _I64, _D, _D, _D, _I32,
                                        C.POINTER(DpParams), C.POINTER(_I32), C.POINTER(_I32), _U32,
                                        _P, _P, _P, _P, _P]),
    "sdirt_psf_call_scratch_bytes": (_I64, [_I64, _I64, _I64]),
    "sdirt_psf_call": (C.c_int, [_P, _P, _P, _I64, _P, _I64, _I64, _D, _D, _D, _D, _D, _I32, C.POINTER(DpParams),
                                 C.POINTER(_I32), C.POINTER(_I32), _U32, _P, _P, _P, _P, _P, _P]),
    "sdirt_ctl_to_lanes": (C.c_int, [_P, _U32, _P, _P]),
    "sdirt_ctl_from_lanes": (C.c_int, [_P, _P, C.POINTER(_I32), C.POINTER(_I32), _P, _P, _P]),
    "sdirt_host_uniform_fill": (C.c_int, [_P, _I64, _I64, _P]),
    "sdirt_selftest_math": (C.c_int, [_I32, C.c_uint64, C.c_uint64, _I32, _P, _P]),
    "sdirt_dp_weight_table_selftest": (C.c_int, [_P, C.POINTER(DpParams), _P, _I64, _P, _P, C.POINTER(_I32), _P]),
    "sdirt_local_psf_render": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "sdirt_psfnet_render": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "sdirt_local_psf_render_grad_psf": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "sdirt_local_psf_render_grad_img": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _I64, _P]),
    "sdirt_local_psf_render_grad_img_workspace_bytes": (_I64, [_I32, _I32, _I32, _I32, _I32]),
    "sdirt_render_psf_volume": (C.c_int, [_P] * 8 + [_I32] * 8 + [_P, _P, _P]),
    "sdirt_render_psf_volume_grad": (C.c_int, [_P] * 9 + [_I32] * 8 + [_P, _P]),
    "sdirt_render_psf_volume_grad_scene": (C.c_int, [_P] * 10 + [_I32] * 8 + [_P, _P, _P]),
    "sdirt_render_psf_volume_chroma": (C.c_int, [_P] * 8 + [_I32] * 8 + [_P, _P, _P]),
    "sdirt_render_psf_volume_chroma_grad": (C.c_int, [_P] * 9 + [_I32] * 8 + [_P, _P]),
    "sdirt_render_psf_volume_chroma_grad_scene": (C.c_int, [_P] * 10 + [_I32] * 8 + [_P, _P, _P]),
    "sdirt_mlp_packed_bytes": (_I64, [C.POINTER(_I32), _I32]),
    "sdirt_mlp_pack": (C.c_int, [C.POINTER(_P), C.POINTER(_P), C.POINTER(_I32), _I32, _P, _P]),
    "sdirt_psfnet_mlp": (C.c_int, [_P, C.POINTER(_I32), _I32, _P, _I64, _I32, _P, _P]),
    "sdirt_dp_cost_volume": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "sdirt_dp_cost_volume_nhwc": (C.c_int, [_P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "sdirt_tone_curve": (C.c_int, [_P, _I64, _I32, _P, _P]),
    "sdirt_avg_pool_windows": (C.c_int, [_P, _I64, _I32, _I32, _I32, _I32, _P, _P]),
    "sdirt_avg_pool_windows_nhwc": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "sdirt_bn_relu": (C.c_int, [_P, _I64, _I32, _I64, _P, _P, _P, _P, _I32, _I32, _P]),
    "sdirt_disparity_regression": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "sdirt_upsample_trilinear_ndhwc": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "sdirt_dp_cost_volume_backward": (C.c_int, [_P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
}

class StreamArg:
    """A hipStream_t together with the GPU it belongs to.  ctypes passes `_as_parameter_`;
    the wrappers installed by lib() read `.index` to make that GPU the current HIP device for
    the duration of the call (a kernel launch goes to the CURRENT device: torch's default stream
    handle is 0 on every GPU, so the handle alone does not say where to run)."""
    __slots__ = ("_as_parameter_", "index")

    def __init__(self, handle, index):
        self._as_parameter_ = C.c_void_p(handle)
        self.index = index


class _Library:
    """Entry points of libsdirt_dp.so; every call whose stream argument is a StreamArg runs
    with that stream's GPU current (lens on cuda:1 while the caller's current device is cuda:0)."""

    def __init__(self, handle):
        self._handle = handle
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, self._guard(fn) if args and args[-1] is _P else fn)

    @staticmethod
    def _guard(fn):
        def call(*args):
            st = args[-1]
            if st.__class__ is StreamArg and st.index != _torch_cuda.current_device():
                with _torch_cuda.device(st.index):
                    return fn(*args)
            return fn(*args)
        call.__name__ = fn.__name__
        return call


_lib = None


class _LazyTorchCuda:
    """torch.cuda, imported on first use (this module loads without torch for header checks)."""
    def __getattr__(self, name):
        import torch
        globals()["_torch_cuda"] = torch.cuda
        return getattr(torch.cuda, name)


_torch_cuda = _LazyTorchCuda()


def lib():
    """The loaded library, with argtypes set.  Raises SdirtError if not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) and not os.environ.get("SDIRT_AMD_LIB"):
            # not built yet: try once with the in-tree Makefile (hipcc cross-compiles without a
            # GPU); anything else is a hard error -- there is no CPU implementation to fall back to
            import subprocess
            try:
                subprocess.check_call(["make", "-C", os.path.join(HERE, "csrc")],
                                      stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            except (OSError, subprocess.CalledProcessError):
                pass
        if not os.path.exists(LIB_PATH):
            raise SdirtError(
                f"{LIB_PATH} is missing: build it with `make -C sdirt_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
                "sdirt_amd has no CPU fallback.")
        try:
            h = C.CDLL(LIB_PATH)
        except OSError as e:      # pragma: no cover
            raise SdirtError(f"cannot load {LIB_PATH}: {e}") from e
        wrapped = _Library(h)
        if wrapped.sdirt_abi_version() != ABI_VERSION:
            raise SdirtError("libsdirt_dp.so ABI version mismatch; rebuild")
        _lib = wrapped
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().sdirt_last_error().decode("utf-8", "replace")
        raise SdirtError(f"libsdirt_dp error {rc}: {msg}")


def device_count():
    return lib().sdirt_device_count()


SELFTEST_LIST_WORDS, SELFTEST_LIST_CAP = 64, 4096     # sdirt_selftest_math modes 5 and 6: header words, list capacity
SEED_ONCE_PROBE = 0x3DC39C73


def decode_seed_once(words):
    """The 64 + 4096 uint64 words sdirt_selftest_math mode 6 leaves (include/sdirt_dp.h) -> dict."""
    o = [int(v) & 0xFFFFFFFFFFFFFFFF for v in words]
    none = 0xFFFFFFFFFFFFFFFF
    listed = sorted(o[SELFTEST_LIST_WORDS:SELFTEST_LIST_WORDS + min(o[4], SELFTEST_LIST_CAP)])
    return dict(checked=o[0], g_pos=o[1], g_neg=o[2], g_outside=o[3], n_quot=o[4],
                first_g=[None if v == none else v for v in o[5:8]],
                seed_offset=o[8] - (1 << 64) if o[8] >> 63 else o[8], seed_bits=o[9], quot=listed)
