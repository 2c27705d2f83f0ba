"""Lensgroup: the reference's PSF-by-ray-tracing API on top of libsdirt_dp.so.

Same method names, argument meaning and defaults as deeplens/optics.py for the
dual-pixel PSF path (psf / psf_diff / psf_rgb / psf_map / psf_center /
sample_from_points / trace / trace2sensor / point_source_grid /
calc_scale_pinhole / entrance_pupil / exit_pupil / refocus / calc_fov /
read_lens_json).  All per-ray work runs in HIP kernels; this file only
validates arguments, draws the pupil uniforms from torch's CPU generator in the
reference's order (optics.py:483-484: that is what makes seeds reproduce),
keeps the speculated Newton trip tables (newton.py) and launches.

There is no CPU fallback: every method that traces rays raises if
libsdirt_dp.so is not built or no MI355X is visible.
"""
import contextlib
import ctypes as C
import json
import math
import types
import weakref

import numpy as np
import torch

from . import _hostrng, _lib, basics
from .basics import DEFAULT_WAVE, DEPTH, GEO_SPP, WAVE_RGB, Material, Ray, dptr, stream_ptr
from .monte_carlo import _requires_grad, dp_energy, splat_autograd
from .newton import NEWTON_MAXITER, TripPlanner
from .surfaces import Aspheric
from .trace_grad import (N_COLUMNS, ChiefCentreFunction, PointGradFunction, PointSamples, SurfaceGradFunction, TraceRecord,
                         glass_eta)


def _as_device(device):
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    return device


class _DevLens:
    """Owner of one sdirt_lens handle (a prescription at one wavelength)."""

    def __init__(self, surfaces, wvln):
        arr = (_lib.SurfaceDesc * len(surfaces))(*[s.desc(wvln) for s in surfaces])
        h = C.c_void_p()
        _lib.check(_lib.lib().sdirt_lens_create(arr, len(surfaces), C.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().sdirt_lens_destroy(self.handle)
                self.handle = None
        except Exception:      # interpreter shutdown
            pass


class _EventBracket:
    """Records a (start, end) HIP event pair on torch's current stream -- the
    stream the kernels are launched on -- when profiling is switched on."""

    def __init__(self, sink, name, device):
        self.sink, self.name, self.device = sink, name, device

    def __enter__(self):
        if self.sink is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream(self.device))
        return self

    def __exit__(self, *exc):
        if self.sink is not None:
            self.e1.record(torch.cuda.current_stream(self.device))
            self.sink.setdefault(self.name, []).append((self.e0, self.e1))
        return False


class PendingPSF:
    """A psf_lr call whose kernel is enqueued and whose Newton trip check is still due."""

    def __init__(self, finish):
        self._finish, self._result = finish, None

    def wait(self):
        if self._finish is not None:
            self._result = self._finish()
            self._finish = None
        return self._result


class _PsfCall(types.SimpleNamespace):
    """One psf_lr call after its set-up (Lensgroup._psf_request): what every launch of it takes, and the stream it was
    enqueued on -- every later round of the call runs there, whatever stream is current when the call is settled."""

    def result(self):
        return _epilogue(self.L, self.R, self.want_r, self.single_point)


def _epilogue(L, R, want_r, single_point):
    """(L, R) as psf_lr returns them: R all zero when a right grid is wanted but none was rendered (the reference's
    default param_list, monte_carlo.py:231), a single point's grids without the batch axis."""
    if R is None and want_r:
        R = torch.zeros_like(L)
    if single_point:
        L, R = L.squeeze(0), (R.squeeze(0) if R is not None else None)
    return L, R


def _parse_param_list(param_list):
    """psf_diff's param_list = (h, f, w, r, direct) -> (dual-pixel parameters or None, whether the right grid is wanted)."""
    if param_list is None:
        return None, False
    h, f, w, r, direct = param_list
    return (h, f, w, r), direct != "l"


def _psf_needs_grad(dp, points, center, d_sensor=None):
    """Whether a psf call records gradients: grad mode is on and h, f or w of dp -- or, with center=False (the
    pinhole centres, optics.py:973-976), the points, or the call's own sensor position d_sensor -- require one.
    r never gets a gradient (monte_carlo.py:167)."""
    vals = (list(dp[:3]) if dp is not None else []) + [d_sensor]
    if not center:
        vals.append(points)
    return _requires_grad(*vals)


def _c_trips(t):
    """A trip table as the int32 array the library takes."""
    t = np.asarray(t, np.int32)
    return (C.c_int32 * t.size)(*t.tolist())


class Lensgroup:
    """optics.py:22-116.  `device` must be a CUDA (ROCm) device for anything that traces."""

    def __init__(self, filename=None, sensor_res=(1024, 1024), use_roc=False,
                 post_computation=True, device=None):
        self.device = _as_device(device)
        self.surfaces = []
        self.materials = []
        self.sensor_res = sensor_res
        self.aper_idx = None
        self._dev = {}                 # wvln -> _DevLens
        self._pupil_cache = {}         # entrance(bool) -> (z, r)
        self.trips = TripPlanner()
        #: 'reference' = reproduce the reference's batch-global Newton trip counts
        #: (speculate + verify, newton.py); 'max' = always 10 trips, no host sync;
        #: 'adaptive' = speed mode: every 64-ray wave stops iterating when none of its rays is
        #: open (<= 10 trips), no host sync -- not batch-exact (PSFs differ by ~1e-5 of peak).
        self.trip_policy = "reference"
        #: optional hook reducing convergence masks over ranks (set by sdirt_amd.dist)
        self.mask_reduce = None
        #: 'lean' (default): division / sqrt by rcp/sqrt seed + fma corrections, proven
        #: bit-identical to IEEE for normal-range operands (all 2^46 mantissa pairs / every
        #: fp32 >= 2^-100; tools/selftest_math.py).  'ieee': the compiler's full-range
        #: sequences (also handles denormal / zero-denominator operands), ~1.26x slower.
        self.precision = "lean"
        #: how the paraxial pupil is estimated from the 16 traced rays (optics.py:1470-1515):
        #: 'reference' = the reference's estimator: pairwise 2x2 systems solved in fp32 by
        #: torch.linalg.lstsq on the host (the same LAPACK call the reference's CPU path
        #: makes).  It is ill-conditioned in fp32 and lands 0.11 % above the exact value on
        #: rf50mm -- the reference's PSFs are rendered with THAT pupil, so it is the default.
        #: 'exact' = closed-form float64 intersections (deterministic, unbiased).
        self.pupil_method = "reference"
        #: where the uniform -> pupil-disc mapping runs: 'device' (default) or 'host' (the
        #: reference's own torch CPU expressions; see _pupil_samples)
        self.pupil_mapping = "device"
        #: generator device of Lensgroup.sample_pupil (the per-source pupil samples of sample_point_source, analysis_rms,
        #: calc_magnification3): None = the lens's device, as the reference draws them; 'cpu' = the CPU generator
        #: (what a CPU run of the reference uses: seeds then reproduce its sample points)
        self.sample_rng_device = None
        #: True: psf calls ask for run-to-run IDENTICAL grids also where the default sums them in fp32 LDS tiles (grids of 50
        #: to 70 pixels -- config 2's 65 x 65; L alone: to 99): SDIRT_PSF_DETERMINISTIC, float64 tiles in 1024-thread
        #: workgroups, +0.5 % time.  Grids up to 49 pixels are summed in float64 anyway.  Beyond the range, with r > 0.5 or
        #: few points with many samples (the spp axis cut) the library says SDIRT_ERR_UNSUPPORTED.
        self.deterministic = False
        #: when a dict, kernel launches are bracketed with HIP events on the launch
        #: stream: {'psf_lr': [(start, end), ...], 'chief_center': [...]}  (bench.py)
        self.kernel_events = None
        if filename is not None:
            self.lens_name = filename
            self.load_file(filename, use_roc, sensor_res, post_computation)

    # ------------------------------------------------------------------ init
    def load_file(self, filename, use_roc=False, sensor_res=(1024, 1024), post_computation=True):
        """optics.py:118-142 (JSON only; the .txt reader is undefined in the reference)."""
        if filename.endswith(".json"):
            self.read_lens_json(filename)
        else:
            raise Exception("File format not supported.")
        self.find_aperture()
        self.prepare_sensor(sensor_res)
        self.diff_surf_range = self.find_diff_surf()
        if post_computation:
            self.post_computation()

    def read_lens_json(self, filename="./test.json"):
        """optics.py:2173-2198.  Also accepts this package's flat schema
        (sdirt_amd/data/*.json: keys kind/semi_aperture/z/curvature/...)."""
        with open(filename, "r") as f:
            data = json.load(f)
        self.surfaces, self.materials = [], []
        for sd in data["surfaces"]:
            if "type" in sd:
                t = sd["type"]
                if t == "Aspheric":
                    s = Aspheric(r=sd["r"], d=sd["d"], c=sd["c"], k=sd["k"], ai=sd["ai"],
                                 mat1=sd["mat1"], mat2=sd["mat2"])
                elif t in ("Stop", "Spheric"):
                    s = Aspheric(r=sd["r"], d=sd["d"], c=sd["c"], mat1=sd["mat1"], mat2=sd["mat2"])
                else:
                    raise Exception("Surface type not implemented.")
            else:
                ai = sd.get("even_asphere")
                s = Aspheric(r=sd["semi_aperture"], d=sd["z"], c=sd["curvature"],
                             k=sd.get("conic", 0.0), ai=ai if sd["kind"] == "asphere" else None,
                             mat1=sd["glass_before"], mat2=sd["glass_after"])
            self.surfaces.append(s)
            self.materials.append(s.mat1)
        self.materials.append(self.surfaces[-1].mat2)
        self.r_last = data["r_last"]
        self.d_sensor = data["d_sensor"]
        self._invalidate()

    def write_lens_json(self, filename="./test.json"):
        """optics.py:2145-2170."""
        data = {"foclen": getattr(self, "foclen", None), "fnum": getattr(self, "fnum", None),
                "r_last": float(self.r_last), "d_sensor": float(self.d_sensor),
                "sensor_size": list(self.sensor_size), "surfaces": []}
        for i, s in enumerate(self.surfaces):
            sd = s.surf_dict()
            nxt = self.surfaces[i + 1].d if i < len(self.surfaces) - 1 else self.d_sensor
            sd["d_next"] = float(nxt) - float(s.d)
            data["surfaces"].append(sd)
        with open(filename, "w") as f:
            json.dump(data, f, indent=4)

    # nn.Module-style switches: the reference's Lensgroup / PSFNet inherit them from DeepObj(nn.Module)
    # (basics.py:165-213) and its scripts call them (dfdp/factory.py:15,31-32: lens.to(device), lens.eval())
    _DEVICE_CACHES = ("_stage_ring", "_sample_stream", "_readback_stream", "_ctl_pools", "_p2o_cache", "_ctl_host",
                      "_right_streak", "_n_cus", "_pinned_out")

    def train(self, mode=True):
        """The PSF network (if this lens carries one) in training / evaluation mode; -> self."""
        net = getattr(self, "psfnet", None)
        if net is not None:
            net.train(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, device):
        """basics.py:180-201: use `device` from now on.  The device-side lens tables, streams and staging buffers
        belong to the old device and are dropped (rebuilt on first use); the PSF network moves with the lens."""
        device = _as_device(device)
        if device != self.device:
            self.device = device
            self._invalidate()
            for name in list(self.__dict__):
                if name in self._DEVICE_CACHES or name.endswith("_stream"):
                    del self.__dict__[name]
            self.last_pupil_points = None
        net = getattr(self, "psfnet", None)
        if net is not None:
            net.to(device)
            if hasattr(net, "invalidate_packed"):
                net.invalidate_packed()
        return self

    def _invalidate(self):
        self._dev.clear()
        self._pupil_cache.clear()
        self.__dict__.pop("_curved_cache", None)

    # ------------------------------------------------------- surface parameters
    def surface_parameters(self):
        """The prescription as ONE tensor: a fresh float32 CPU tensor [K, 3 + MAX_AI], columns d, c, k, ai2, ai4, ...
        holding the records' fp32 values, unused entries 0.  What `surface_params=` of psf_lr / psf_diff / psf_rgb
        takes; which entries are parameters with a gradient is `Aspheric.owned_columns()` per surface."""
        return torch.from_numpy(np.stack([s.parameter_row() for s in self.surfaces]))

    def _surface_values(self, theta):
        v = torch.as_tensor(theta).detach().to("cpu", torch.float32).numpy()
        if v.shape != (len(self.surfaces), N_COLUMNS):
            raise ValueError(f"surface parameters must have shape [{len(self.surfaces)}, {N_COLUMNS}]")
        return v

    def set_surface_parameters(self, theta):
        """Write surface_parameters()-shaped values back into the Aspheric records.  ValueError (and no record changed)
        when a write would change a surface's kind (c to or from 0, k of a sphere) or touch a column the surface does
        not own.  The device tables, the cached pupils and the trip planners are dropped: the next call sees the new
        lens and recomputes its entrance pupil, as the reference does on every call."""
        values = self._surface_values(theta)
        old = [s.parameter_row() for s in self.surfaces]
        try:
            for s, row in zip(self.surfaces, values):
                s.set_parameter_row(row)
        except ValueError:
            for s, row in zip(self.surfaces, old):
                s.set_parameter_row(row)
            raise
        self._invalidate()
        self.trips = TripPlanner()
        return self

    @contextlib.contextmanager
    def _surfaces_borrowed(self, theta):
        """The lens as set_surface_parameters(theta) would make it, for the duration of one call: afterwards (also on
        an exception) the records hold their old values and the device tables, pupils and planner are the old OBJECTS.
        Nothing is touched when the values are already the records'."""
        values = self._surface_values(theta)
        old = [s.parameter_row() for s in self.surfaces]
        if all(np.array_equal(a, b) for a, b in zip(old, values)):
            yield
            return
        saved = (self._dev, self._pupil_cache, self.trips, self.__dict__.get("_curved_cache"))
        try:
            self._dev, self._pupil_cache = {}, {}
            self.set_surface_parameters(values)
            yield
        finally:
            for s, row in zip(self.surfaces, old):
                s.d, s.c, s.k = np.float32(row[0]), np.float32(row[1]), np.float32(row[2])
                if s.ai is not None:
                    s.ai = row[3:3 + s.ai_degree].copy()
            self._dev, self._pupil_cache, self.trips = saved[:3]
            if saved[3] is not None:
                self.__dict__["_curved_cache"] = saved[3]

    # ------------------------------------------------------- glass parameters
    def _media(self):
        """The K + 1 media as lists of the Material objects that hold them: medium j is surfaces[j].mat1 and
        surfaces[j-1].mat2, medium K is surfaces[K-1].mat2.  ValueError when the two objects of one medium disagree."""
        K = len(self.surfaces)
        media = [[self.surfaces[0].mat1]] + [[self.surfaces[j - 1].mat2, self.surfaces[j].mat1] for j in range(1, K)] \
            + [[self.surfaces[K - 1].mat2]]
        for j, objs in enumerate(media):
            a, b = objs[0], objs[-1]
            if (a.n, a.V, a.dispersion) != (b.n, b.V, b.dispersion):
                raise ValueError(f"medium {j}: surface {j - 1} leaves into {a.name!r} and surface {j} starts in {b.name!r}")
        return media

    def glass_owned(self):
        """bool [K + 1]: the media that are parameters with a gradient -- the Cauchy glasses written as 'n/V' strings
        (Material.dispersion == 'naive').  Air-like media and register_material() glasses are constants."""
        return torch.tensor([objs[0].dispersion == "naive" for objs in self._media()])

    def glass_parameters(self):
        """The glass as ONE tensor: a fresh float64 CPU tensor [K + 1, 2], columns n, V, row j = medium j (medium j lies
        in front of surface j; medium K behind the last surface).  What `glass_params=` of psf_lr / psf_diff / psf_rgb /
        psf_volume takes; the rows that are parameters are glass_owned().  Every other row holds (Material.n, V or 0
        for an infinite V) and must stay as it is."""
        return torch.tensor([[objs[0].n, 0.0 if math.isinf(objs[0].V) else objs[0].V] for objs in self._media()],
                            dtype=torch.float64).reshape(-1, 2)

    def _glass_values(self, glass):
        """glass_parameters()-shaped values checked against the lens: -> (float64 numpy [K + 1, 2], the media)."""
        media = self._media()
        v = torch.as_tensor(glass).detach().to("cpu", torch.float64).numpy()
        if v.shape != (len(media), 2):
            raise ValueError(f"glass parameters must have shape [{len(media)}, 2]")
        now = self.glass_parameters().numpy()
        for j, objs in enumerate(media):
            if objs[0].dispersion == "naive":
                if not (np.isfinite(v[j]).all() and v[j, 0] > 1.0 and v[j, 1] > 0.0):
                    raise ValueError(f"medium {j}: a glass needs finite n > 1 and V > 0, got {v[j].tolist()}")
            elif not np.array_equal(v[j], now[j]):
                raise ValueError(f"medium {j} ({objs[0].name!r}) is a constant, not a parameter of this lens")
        return v, media

    @staticmethod
    def _write_glass(mat, n, V):
        mat.n, mat.V = n, V
        mat.A, mat.B = Material.nV_to_AB(n, V)
        mat.name = f"{n!r}/{V!r}"

    def set_glass_parameters(self, glass):
        """Write glass_parameters()-shaped values back: n, V, the Cauchy A and B and the 'n/V' name of both Material objects
        of every owned medium (write_lens_json -> read_lens_json then gives the lens back bit for bit).  ValueError,
        and no object changed, on a wrong shape, a non-finite value, n <= 1 or V <= 0 in an owned row, or a constant's row
        that differs from glass_parameters().  Device tables, pupils and planner are dropped, as by
        set_surface_parameters."""
        values, media = self._glass_values(glass)
        for row, objs in zip(values, media):
            if objs[0].dispersion == "naive":
                for m in objs:
                    self._write_glass(m, float(row[0]), float(row[1]))
        self._invalidate()
        self.trips = TripPlanner()
        return self

    @contextlib.contextmanager
    def _glass_borrowed(self, glass):
        """The lens as set_glass_parameters(glass) would make it, for the duration of one call: afterwards (also on an
        exception) every Material field is the old value and the device tables, pupils and planner are the old OBJECTS.
        Nothing is touched when the values are already the lens's."""
        values, media = self._glass_values(glass)
        if np.array_equal(values, self.glass_parameters().numpy()):
            yield
            return
        old = [[(m, m.n, m.V, m.A, m.B, m.name) for m in objs] for objs in media]
        saved = (self._dev, self._pupil_cache, self.trips, self.__dict__.get("_curved_cache"))
        try:
            self._dev, self._pupil_cache = {}, {}
            self.set_glass_parameters(values)
            yield
        finally:
            for objs in old:
                for m, n, V, A, B, name in objs:
                    m.n, m.V, m.A, m.B, m.name = n, V, A, B, name
            self._dev, self._pupil_cache, self.trips = saved[:3]
            if saved[3] is not None:
                self.__dict__["_curved_cache"] = saved[3]

    def _glass_eta(self, glass, wvln):
        """trace_grad.glass_eta of this lens: eta [K] at `wvln` as a float64 torch function of `glass`."""
        wv = wvln if wvln < 10 else wvln * 1e-3
        media = self._media()
        return glass_eta(glass.cpu(), [objs[0].dispersion == "naive" for objs in media],
                         [float(objs[0].ior(wv)) for objs in media], wv)

    @contextlib.contextmanager
    def _sensor_borrowed(self, d_sensor):
        """The lens with its sensor at `d_sensor` (a number or a one-element tensor; None: as it is) for the duration of
        one call: afterwards, also on an exception, lens.d_sensor is the old object.  Every path reads self.d_sensor
        when it launches (the fused kernels, _psf_rgb_fused, the staged chain, TraceRecord), and nothing cached on
        the lens depends on it: the pupils are traced from the stop, the trip tables are verified per call, and the
        object-space points use hfov and r_last, which stay constants of the lens state."""
        if d_sensor is None:
            yield
            return
        value = float(d_sensor.detach()) if torch.is_tensor(d_sensor) else float(d_sensor)
        old = self.d_sensor
        try:
            self.d_sensor = value
            yield
        finally:
            self.d_sensor = old

    def find_aperture(self):
        """optics.py:193-201: first surface with air-like media on both sides."""
        self.aper_idx = None
        for i in range(len(self.surfaces) - 1):
            if self.surfaces[i].mat1.A < 1.0003 and self.surfaces[i].mat2.A < 1.0003:
                self.aper_idx = i
                return

    def find_diff_surf(self):
        if self.aper_idx is None:
            return range(len(self.surfaces))
        return list(range(0, self.aper_idx)) + list(range(self.aper_idx + 1, len(self.surfaces)))

    def prepare_sensor(self, sensor_res=(512, 512), sensor_size=(24.0, 36.0)):
        """optics.py:154-178."""
        sensor_res = [sensor_res, sensor_res] if isinstance(sensor_res, int) else list(sensor_res)
        self.sensor_res = sensor_res
        H, W = sensor_res
        if sensor_size is None:
            self.sensor_size = [2 * self.r_last * H / np.sqrt(H ** 2 + W ** 2),
                                2 * self.r_last * W / np.sqrt(H ** 2 + W ** 2)]
        else:
            self.sensor_size = list(sensor_size)
            self.r_last = np.sqrt(sensor_size[0] ** 2 + sensor_size[1] ** 2) / 2
        assert self.sensor_size[0] / self.sensor_size[1] == H / W, "Pixel is not square."
        self.pixel_size = self.sensor_size[0] / sensor_res[0]

    def post_computation(self):
        """optics.py:181-190."""
        self.find_aperture()
        self.hfov = self.calc_fov()
        self.foclen = self.calc_efl()
        _, avg_pupilx = self.entrance_pupil()
        self.fnum = self.foclen / avg_pupilx / 2

    def set_state(self, d_sensor=None, hfov=None, pupil=None, exit_pupil=None):
        """Pin the geometric-optics scalars (e.g. from a reference fixture) instead
        of computing them; the reference's own values drift run to run
        (its paraxial pupil is an ill-conditioned fp32 lstsq, optics.py:1500)."""
        if d_sensor is not None:
            self.d_sensor = float(d_sensor)
        if hfov is not None:
            self.hfov = float(hfov)
            self.foclen = self.calc_efl()
        if pupil is not None:
            self._pupil_cache[True] = (float(pupil[0]), float(pupil[1]))
        if exit_pupil is not None:
            self._pupil_cache[False] = (float(exit_pupil[0]), float(exit_pupil[1]))
        if pupil is not None and hasattr(self, "foclen"):
            self.fnum = self.foclen / self._pupil_cache[True][1] / 2
        return self

    # ----------------------------------------------------------- device side
    def _require_gpu(self):
        if self.device.type != "cuda":
            raise _lib.SdirtError("sdirt_amd traces rays on the GPU only; construct the lens with "
                                  "device='cuda' (no CPU fallback exists)")

    def dev_lens(self, wvln=DEFAULT_WAVE):
        self._require_gpu()
        key = float(wvln if wvln < 10 else wvln * 1e-3)
        dl = self._dev.get(key)
        if dl is None:
            with torch.cuda.device(self.device):
                dl = _DevLens(self.surfaces, key)
            # the handle is only cached -- and handed out -- once the library has passed its self-test on this
            # prescription: a failed test raises on THIS and on every later call (the failure is remembered per
            # device and prescription, _selftest_failed), never just on the first
            self._prefetch_selftest(dl.handle)
            self._dev[key] = dl
        return dl.handle

    def _prefetch_selftest(self, handle):
        """Second guard of the hand-scheduled scalar prefetch in the trace loop (the first is the
        ISA check of the build, tools/check_prefetch_hazard.py): when a prescription is first
        uploaded, a fan of probe rays is traced twice -- next surface's constants prefetched one
        surface ahead / loaded on the spot (SDIRT_TRACE_NO_PREFETCH) -- forward and backward, both
        math policies; the two must agree bit for bit.  A compiler that moved an instruction into
        the in-flight window would make the prefetching loop trace with stale constants or trip
        counts; then every call on this lens raises instead of returning wrong PSFs.  Draws no random numbers."""
        digest = self._table_digest()
        if Lensgroup._selftest_done.get((self.device.index, len(self.surfaces))) == digest:
            return
        if (self.device.index, digest) in Lensgroup._selftest_failed:
            raise _lib.SdirtError(Lensgroup._selftest_failed[(self.device.index, digest)])
        K = len(self.surfaces)
        front, back = self.surfaces[0], self.surfaces[-1]
        n = 16
        lin = torch.linspace(-0.6, 0.6, n, device=self.device)
        gx, gy = torch.meshgrid(lin, lin, indexing="xy")
        trips = (C.c_int32 * K)(*self._fixed_trips_for("max").tolist())
        for forward in (True, False):
            surf = front if forward else back
            z0 = float(surf.d) - 40.0 if forward else float(self.d_sensor)
            o = torch.stack((gx * 3.0, gy * 3.0 + 0.5, torch.full_like(gx, z0)), -1).reshape(-1, 3)
            aim = torch.stack((gx * float(surf.r), gy.flip(0) * float(surf.r),
                               torch.full_like(gx, float(surf.d))), -1).reshape(-1, 3)
            for flags in (0, _lib.PSF_STRICT_IEEE):
                a = Ray(o, aim - o, device=self.device)
                b = a.clone()
                for ray, extra in ((a, 0), (b, _lib.TRACE_NO_PREFETCH)):
                    _lib.check(_lib.lib().sdirt_trace(handle, 0, K, 0 if forward else 1, trips, flags | extra,
                                                      ray.c_rays(), ray.numel, None, stream_ptr(self.device)))
                if not torch.equal(a.soa.view(torch.int32), b.soa.view(torch.int32)):
                    msg = ("libsdirt_dp.so self-test failed: the trace loop with prefetched surface constants "
                           "disagrees with the load-and-wait form (miscompiled surf_issue/surf_wait window?); "
                           "rebuild with `make -C sdirt_amd/csrc` and check tools/check_prefetch_hazard.py")
                    Lensgroup._selftest_failed[(self.device.index, digest)] = msg
                    raise _lib.SdirtError(msg)
        Lensgroup._selftest_done[(self.device.index, K)] = digest

    _selftest_done = {}
    _selftest_failed = {}          # (device index, prescription digest) -> message: sticky

    def _table_digest(self):
        return hash(tuple((s.kind, float(s.r), float(s.d), float(s.c), float(s.k),

                           tuple(float(a) for a in (s.ai if s.ai is not None else ()))) for s in self.surfaces))

    def _fixed_trips_for(self, policy):
        n = NEWTON_MAXITER if policy == "max" else -NEWTON_MAXITER
        return np.where(self._curved(), n, 0).astype(np.int32)

    def _math_flags(self):
        if self.precision not in ("ieee", "lean"):
            raise ValueError("precision must be 'lean' or 'ieee'")
        return _lib.PSF_STRICT_IEEE if self.precision == "ieee" else 0

    def _psf_flags(self):
        """Math policy and, on request, the order-independent sums of a fused psf call (self.deterministic)."""
        return self._math_flags() | (_lib.PSF_DETERMINISTIC if self.deterministic else 0)

    def _timed(self, name):
        return _EventBracket(self.kernel_events, name, self.device)

    def _curved(self):
        c = self.__dict__.get("_curved_cache")
        if c is None or len(c) != len(self.surfaces):
            c = self.__dict__["_curved_cache"] = [s.kind != _lib.KIND_PLANE for s in self.surfaces]
        return c

    def _mask_buffer(self):
        return torch.zeros(_lib.MAX_SURFACES, dtype=torch.int32, device=self.device)

    def _read_masks(self, mask):
        m = mask[:len(self.surfaces)]
        if self.mask_reduce is not None:
            m = self.mask_reduce(m)
        return m.cpu().numpy().astype(np.int64) & 0xFFFFFFFF

    def _fixed_trips(self):
        """Trip table of the policies that need no host check: 10 everywhere ('max') or -10 =
        "up to 10, each wave stops when its own rays are done" ('adaptive')."""
        if self.trip_policy not in ("max", "adaptive"):
            raise ValueError(f"unknown trip_policy {self.trip_policy!r}")
        return self._fixed_trips_for(self.trip_policy)

    def _run_with_trips(self, key, order, enqueue):
        """enqueue(trips_ctypes, mask_ptr) launches the kernels.  Returns the trip
        table that was finally used."""
        K = len(self.surfaces)
        curved = self._curved()
        if self.trip_policy != "reference":
            trips = self._fixed_trips()
            enqueue((C.c_int32 * K)(*trips.tolist()), None)
            return trips
        mask = self._mask_buffer()

        def launch(trips):
            mask.zero_()
            enqueue((C.c_int32 * K)(*[int(t) for t in trips]), dptr(mask))
            return self._read_masks(mask)

        return self.trips.run(key, curved, list(order), launch)

    # ---------------------------------------------------------------- sampling
    @torch.no_grad()
    def sample_from_points(self, o=[[0, 0, -10000]], spp=256, wvln=DEFAULT_WAVE,
                           shrink_pupil=False, normalized=False):
        """optics.py:460-494: rays [spp, N] from object-space points to random pupil points."""
        self._require_gpu()
        if not torch.is_tensor(o):
            o = torch.tensor(o)
        po = o.to(self.device, torch.float32).reshape(-1, 3).contiguous()
        pupilz, pupilr = self.entrance_pupil(shrink_pupil=shrink_pupil)
        x2, y2 = self._pupil_samples(spp, pupilr)
        ray = Ray.empty((spp, po.shape[0]), wvln, self.device)
        _lib.check(_lib.lib().sdirt_sample_rays(dptr(po), po.shape[0], dptr(x2), dptr(y2), spp,
                                                float(pupilz), ray.c_rays(),
                                                stream_ptr(self.device)))
        if basics.TRACK_OBLIQ:                               # a caller's bundle: readable obliq, as the reference's (basics.py:240)
            ray.obliq = torch.ones((), device=self.device)
        return ray

    def _staging(self, spp, depth=8, rows=2):
        """A page-locked [rows, spp] buffer from a ring of `depth` per size, and the event that
        marks its upload as done; a slot is reused only after its previous upload has finished."""
        rings = self.__dict__.setdefault("_stage_ring", {})
        if (rows, spp) not in rings and len(rings) >= 16:      # a caller sweeping over many sizes: keep the newest rings
            rings.pop(next(iter(rings)))
        ring = rings.setdefault((rows, spp), {"slots": [], "next": 0})
        if len(ring["slots"]) < depth:
            ring["slots"].append((torch.empty((rows, spp), dtype=torch.float32, pin_memory=True),
                                  torch.cuda.Event()))
            return ring["slots"][-1]
        slot = ring["slots"][ring["next"]]
        ring["next"] = (ring["next"] + 1) % depth
        slot[1].synchronize()
        return slot

    def _pupil_samples(self, spp, pupil_r):
        """optics.py:483-488: spp points on the pupil disc -> device arrays (x2, y2).

        The two uniform vectors always come from torch's CPU default generator in the
        reference's order (that is what makes seeds line up).  pupil_mapping='device'
        (default) maps them to the disc with the sdirt_pupil_samples kernel (correctly rounded
        sin/cos).  'host' evaluates the reference's own CPU tensor expressions
        (optics.py:483-486) instead: bit-identical sample points to the reference ON THE SAME
        MACHINE -- torch's sin/cos are MKL kernels whose last bit differs between CPU models
        (the Xeon that produced tests/golden and the EPYC of the GPU box disagree on ~5 % of
        the samples) -- at the price of threaded MKL calls (measured 24 ms per call on a
        256-thread host under a 16-CPU quota)."""
        if self.pupil_mapping == "host":
            u_theta, u_r2 = torch.rand(spp), torch.rand(spp)
            theta = u_theta * 2 * np.pi
            r = torch.sqrt(u_r2 * pupil_r ** 2)
            xy = torch.stack((r * torch.cos(theta), r * torch.sin(theta))).to(self.device)
            return xy[0], xy[1]
        # draw straight into page-locked memory (same generator, same values as torch.rand(spp))
        # so that the upload is a true asynchronous copy: from pageable memory it would block
        # the host until the stream has drained, i.e. until the previous call's kernel is done.
        # Upload and mapping depend on nothing the caller has queued, so they go on a side stream
        # (they run beside the previous call's kernel instead of behind it) and the caller's
        # stream waits for their event.
        main = torch.cuda.current_stream(self.device)
        side = self._side_stream("_sample_stream")
        with torch.cuda.stream(side):
            stage, done = self._staging(spp)
            _hostrng.rand_into(stage[0])
            _hostrng.rand_into(stage[1])
            u = stage.to(self.device, non_blocking=True)
            done.record(side)
            xy = torch.empty((2, spp), dtype=torch.float32, device=self.device)
            _lib.check(_lib.lib().sdirt_pupil_samples(dptr(u[0]), dptr(u[1]), spp, float(pupil_r),
                                                      dptr(xy[0]), dptr(xy[1]),
                                                      stream_ptr(self.device)))
        main.wait_stream(side)
        xy.record_stream(main)
        return xy[0], xy[1]

    def _pupil_samples_pair(self, spp, pupil_r, spp_c, pupil_r_c, side_stream=True):
        """The two sample sets of one psf call -- `spp` points on the pupil, then `spp_c` on the
        shrunk pupil of the chief-ray pass -- with ONE draw, ONE upload and one device block:
        torch.rand(2 spp + 2 spp_c) is, value for value, the four consecutive draws
        rand(spp), rand(spp), rand(spp_c), rand(spp_c) of the reference (optics.py:483-484 twice;
        the CPU generator hands out one 24-bit number per element, whatever the call sizes:
        tests/test_host_logic.py).  -> (x2, y2, xc, yc)."""
        if self.pupil_mapping == "host":
            return self._pupil_samples(spp, pupil_r) + self._pupil_samples(spp_c, pupil_r_c)
        n = 2 * (spp + spp_c)
        a, b = 2 * spp, 2 * spp + spp_c
        h = _lib.lib()

        def upload_and_map():
            stage, done = self._staging(n, rows=1)
            _hostrng.rand_into(stage[0])
            u = stage[0].to(self.device, non_blocking=True)
            done.record(torch.cuda.current_stream(self.device))
            xy = torch.empty(n, dtype=torch.float32, device=self.device)
            st = stream_ptr(self.device)
            pu, pxy = u.data_ptr(), xy.data_ptr()
            P = lambda base, off: C.c_void_p(base + 4 * off)
            _lib.check(h.sdirt_pupil_samples(P(pu, 0), P(pu, spp), spp, float(pupil_r), P(pxy, 0), P(pxy, spp), st))
            _lib.check(h.sdirt_pupil_samples(P(pu, a), P(pu, b), spp_c, float(pupil_r_c), P(pxy, a), P(pxy, b), st))
            return u, xy

        if not side_stream:
            # synchronous caller: nothing of an earlier call is in flight that the upload could run
            # beside -- straight onto the caller's stream, no stream switch, no cross-stream waits
            u, xy = upload_and_map()
        else:
            main = torch.cuda.current_stream(self.device)
            side = self._side_stream("_sample_stream")
            with torch.cuda.stream(side):
                u, xy = upload_and_map()
            main.wait_stream(side)
            xy.record_stream(main)
        return xy[:spp], xy[spp:a], xy[a:b], xy[b:]

    # ----------------------------------------------------------------- tracing
    def trace(self, ray, lens_range=None, record=False, forward=None, _to_sensor=None):
        """optics.py:601-627: updates `ray` and returns (ray, valid, oss).  Direction is
        taken from the first ray's d_z like the reference unless `forward` is given.
        Under trip_policy 'reference' the trace runs OUT OF PLACE and `ray`'s storage is rebound to the traced
        bundle (the reference rebinds ray.o / ray.d / ray.ra to new tensors too, surfaces.py:425, 676-677): views
        (`ray.ra`, `ray.obliq`) and `c_rays()` pointers taken BEFORE the call keep showing the untraced rays --
        re-fetch them after trace / trace2sensor.  ('max' / 'adaptive' trace in place.)
        _to_sensor = z: trace2sensor's form -- forward through all surfaces and on to the plane z in the same pass
        (sdirt_trace2sensor)."""
        self._require_gpu()
        K = len(self.surfaces)
        if record:
            return self._trace_recorded(ray, lens_range, forward)
        if lens_range is None:
            first, last = 0, K
        else:
            lr = list(lens_range)
            first, last = (lr[0], lr[-1] + 1) if lr else (0, 0)
            assert lr == list(range(first, last)), "lens_range must be contiguous"
        if forward is None:
            forward = bool(ray.soa[5, 0].item() > 0)             # optics.py:618
        order = list(range(first, last)) if forward else list(range(last - 1, first - 1, -1))
        handle = self.dev_lens(ray.wvln)

        def enqueue(trips, mask_ptr):
            _lib.check(_lib.lib().sdirt_trace(handle, first, last, 0 if forward else 1, trips,
                                              self._math_flags(), ray.c_rays(), ray.numel,
                                              mask_ptr, stream_ptr(self.device)))

        if self.trip_policy == "reference":
            # a wrong bet on the trip table means tracing the batch again from its input: the trace goes OUT OF PLACE
            # into a second bundle (sdirt_trace_to) which then becomes the ray's storage -- the reference's trace
            # rebinds ray.o / ray.d / ray.ra to new tensors in the same way (surfaces.py:425, 676-677); copying the
            # bundle first to trace in place cost as much memory traffic as the trace itself
            dst = Ray.empty(ray.shape, ray.wvln, self.device, obliq=ray.has_obliq)

            def enqueue_to(trips, mask_ptr):
                if _to_sensor is not None:
                    _lib.check(_lib.lib().sdirt_trace2sensor(handle, trips, self._math_flags(), float(_to_sensor),
                                                             ray.c_rays(), dst.c_rays(), ray.numel, mask_ptr,
                                                             stream_ptr(self.device)))
                    return
                _lib.check(_lib.lib().sdirt_trace_to(handle, first, last, 0 if forward else 1, trips,
                                                     self._math_flags(), ray.c_rays(), dst.c_rays(), ray.numel,
                                                     mask_ptr, stream_ptr(self.device)))
            key = ("trace", round(float(ray.wvln), 6), first, last, forward, self.precision)
            self._run_with_trips(key, order, enqueue_to)
            ray._adopt(dst)
        else:
            self._run_with_trips(None, order, enqueue)
            ray._mark_traced()
            if _to_sensor is not None:
                ray.propagate_to(_to_sensor)
        valid = ray.ra == 1
        return ray, valid, None

    def _trace_recorded(self, ray, lens_range, forward):
        """trace(record=True), optics.py:666-717: `oss[i]` = the points ray i (row i of the first batch
        dimension) passed through -- its origin, then its position after every surface it left alive --
        as numpy arrays, for the reference's ray-path plots.  Traced surface by surface with the
        staged kernel (each surface's batch-wide Newton trip count verified on its own), the positions
        copied to the host after every surface: a plotting aid, not a fast path."""
        K = len(self.surfaces)
        idx = list(range(K)) if lens_range is None else list(lens_range)
        if forward is None:
            forward = bool(ray.soa[5, 0].item() > 0)             # optics.py:618
        oss = [[p] for p in ray.o.cpu().numpy()]
        for k in (idx if forward else idx[::-1]):
            self.trace(ray, lens_range=range(k, k + 1), forward=forward)
            alive = ((ray.ra == 1) if forward else (ray.ra > 0)).cpu().numpy()   # optics.py:681 / :707
            for path, v, p in zip(oss, alive, ray.o.cpu().numpy()):
                if np.any(v):
                    path.append(p)
        return ray, ray.ra == 1, oss

    def trace2sensor(self, ray, record=False, ignore_invalid=False):
        """optics.py:638-664 (the ray's storage is rebound like trace()'s).  record=True: (p, oss) -- the sensor-plane positions [M,3] and the
        recorded paths, each live ray's sensor point appended (twice, as the reference's two loops do)."""
        if not record:
            if bool(ray.soa[5, 0].item() > 0):                   # forward (optics.py:618): one pass, sdirt_trace2sensor
                ray, _, _ = self.trace(ray, forward=True, _to_sensor=self.d_sensor)
                return ray
            ray, _, _ = self.trace(ray)
            return ray.propagate_to(self.d_sensor)
        ray, _, oss = self.trace(ray, record=True)
        ray.propagate_to(self.d_sensor)
        valid, p = ray.ra == 1, ray.o
        for path, v, pp in zip(oss, valid.cpu().numpy(), p.cpu().numpy()):
            if np.any(v):
                path.append(pp)
        if ignore_invalid:
            p = p[valid]
        else:
            assert p.dim() >= 2, "This function is not tested."
            p = p.reshape(-1, 3)
        for v, path, pp in zip(valid.cpu().numpy(), oss, p.cpu().numpy()):
            if v:
                path.append(pp)
        return p, oss

    # --------------------------------------------------------------------- PSF
    def point_source_grid(self, depth, grid=9, normalized=True, quater=False, center=False):
        """optics.py:816-861: [grid, grid, 3] field of point sources at one depth; entry [i, j] is
        (x_j, y_i, depth) with x running left to right and y from the top edge down.  Edge samples
        sit at +-0.98 of the normalised field (or at patch centres, +-(1 - 1/(2(grid-1))), with
        center=True); quater keeps the upper-left ceil(grid/2) x ceil(grid/2) block."""
        if grid == 1:
            assert not quater, "Quater should be False when grid is 1."
            axis = torch.zeros(1)
        else:
            edge = 1 - 1 / 2 / (grid - 1) if center else 0.98
            axis = torch.linspace(-edge, edge, grid)
        field = torch.empty(grid, grid, 3)
        field[..., 0] = axis.view(1, grid)
        field[..., 1] = -axis.view(grid, 1)
        field[..., 2] = float(depth)
        if quater:
            keep = (grid + 1) // 2
            field = field[:keep, :keep]
        if not normalized:
            # object-space millimetres; x takes the sensor HEIGHT here (the reference's convention in
            # this function, optics.py:858-859 -- psf_diff uses the width for x)
            scale = self.calc_scale_pinhole(depth)
            field[..., 0] *= scale * self.sensor_size[0] / 2
            field[..., 1] *= scale * self.sensor_size[1] / 2
        return field

    def _side_stream(self, name):
        st = self.__dict__.get(name)
        if st is None:
            st = self.__dict__[name] = torch.cuda.Stream(self.device)
        return st

    def _zeroed_control_block(self, n, rows=64):
        """An int32 [n] device block that is zero, cut from a pool that is cleared `rows` blocks
        at a time (one fill kernel per `rows` launches instead of one per launch)."""
        # one pool per (size, stream): the fill runs on the stream that is current when the pool is
        # created, and rows are only ever handed to launches on THAT stream -- so the fill is ordered
        # before every kernel that ORs into a row, and the caching allocator (which hands memory back
        # to the stream it was allocated on) cannot recycle the pool under a foreign stream's kernel
        pools = self.__dict__.setdefault("_ctl_pools", {})
        key = (n, torch.cuda.current_stream(self.device).cuda_stream)
        pool = pools.get(key)
        if pool is None or pool["next"] >= rows:
            pools.pop(key, None)
            while len(pools) >= 8:                     # a caller sweeping over many shapes: keep the newest pools only
                pools.pop(next(iter(pools)))
            pool = pools[key] = {"next": 0,
                                 "buf": torch.zeros((rows, n), dtype=torch.int32, device=self.device)}
        row = pool["buf"][pool["next"]]
        pool["next"] += 1
        return row

    def _points_to_object(self, points):
        """[N,3] normalised points -> object space (optics.py:959-960, 1305), on the device.  The
        result for the LAST tensor is kept: a caller that renders the same grid call after call (a
        PSF volume, an evaluation set) pays for the conversion once.  The key is the tensor object
        itself, its version counter (any in-place write bumps it) and every lens scalar used."""
        # only device tensors that track a version counter are cached: a CPU tensor can be written
        # behind torch's back (torch.from_numpy + a numpy-side store leaves _version unchanged), an
        # inference-mode tensor has no counter at all
        if not points.is_cuda or points.is_inference():
            return self._points_to_object_now(points)
        key = (points._version, tuple(points.shape), points.dtype, float(np.tan(self.hfov)),
               float(self.r_last), float(self.sensor_size[1]), float(self.sensor_size[0]),
               str(self.device), torch.cuda.current_stream(self.device).cuda_stream)
        # one entry per stream (a caller that alternates two render streams keeps both): the converted points were
        # produced on that stream and are only handed to launches on it
        cache = self.__dict__.setdefault("_p2o_cache", {})
        hit = cache.get(key[-1])
        if hit is not None and hit[0]() is points and hit[1] == key:
            return hit[2]
        out = self._points_to_object_now(points)
        if key[-1] not in cache and len(cache) >= 4:
            cache.pop(next(iter(cache)))
        cache[key[-1]] = (weakref.ref(points), key, out)
        return out

    def _points_to_object_now(self, points):
        if not points.is_cuda:
            # page-locked staging: an upload from pageable memory blocks the host until the
            # stream has drained (i.e. until the previous call's kernel has finished).  The buffer comes from
            # the lens's ring of page-locked blocks (Tensor.pin_memory() would page-lock a fresh allocation on
            # every call: a system call of its own, ~0.3 ms for the 24576 points of the reference's timing harness)
            n = points.shape[0]
            stage, uploaded = self._staging(max(n, 1), depth=4, rows=3)
            host = stage.view(-1)[:3 * n].view(n, 3)
            if points.dtype == torch.float32 and points.is_contiguous() and not points.requires_grad:
                # a plain memcpy: torch's CPU copy_ is an OpenMP-parallel op whose worker threads spin afterwards --
                # inside a CPU-quota'd container that can cost the calling thread its time slice (tools/tcp_span.py)
                np.copyto(host.numpy(), points.numpy())
            else:
                host.copy_(points)
            pts = host.to(self.device, non_blocking=True)
            uploaded.record(torch.cuda.current_stream(self.device))
        else:
            pts = points.to(self.device, torch.float32, non_blocking=True).contiguous()
        out = torch.empty_like(pts)
        _lib.check(_lib.lib().sdirt_points_to_object(
            dptr(pts), pts.shape[0], float(np.tan(self.hfov)), float(self.r_last),
            float(self.sensor_size[1]), float(self.sensor_size[0]), dptr(out),
            stream_ptr(self.device)))
        return out

    @torch.no_grad()
    def psf_center(self, point, method="chief_ray"):
        """optics.py:889-914: [N,3] object-space points -> [N,2] PSF centres (green light)."""
        if method == "pinhole":
            scale = self.calc_scale_pinhole(point[..., 2])
            return -point[..., :2] / scale
        if method != "chief_ray":
            raise Exception("Unsupported method.")
        self._require_gpu()
        po = point.to(self.device, torch.float32).reshape(-1, 3).contiguous()
        pupilz, pupilr = self.entrance_pupil(shrink_pupil=True)
        xc, yc = self._pupil_samples(GEO_SPP, pupilr)
        center = torch.empty((po.shape[0], 2), dtype=torch.float32, device=self.device)
        self._chief_center(po, xc, yc, pupilz, center)
        return center

    def _chief_center(self, po, xc, yc, pupilz, center, slope=None):
        """The chief-ray centres of `po` into `center`; slope (float64 [N, 2]): d(centre)/d(d_sensor) as well
        (sdirt_chief_center_slope: the same centres, bit for bit)."""
        anyv = torch.zeros(1, dtype=torch.int32, device=self.device)
        handle = self.dev_lens(DEFAULT_WAVE)                      # optics.py:900: always green

        def enqueue(trips, mask_ptr):
            with self._timed("chief_center"):
                if slope is not None:
                    _lib.check(_lib.lib().sdirt_chief_center_slope(
                        handle, dptr(po), po.shape[0], dptr(xc), dptr(yc), xc.shape[0], float(pupilz),
                        float(self.d_sensor), trips, self._math_flags(), dptr(center), dptr(slope), dptr(anyv),
                        mask_ptr, stream_ptr(self.device)))
                    return
                _lib.check(_lib.lib().sdirt_chief_center(
                    handle, dptr(po), po.shape[0], dptr(xc), dptr(yc), xc.shape[0], float(pupilz),
                    float(self.d_sensor), trips, self._math_flags(), dptr(center), dptr(anyv),
                    mask_ptr, stream_ptr(self.device)))
        self._run_with_trips(("center", self.precision), range(len(self.surfaces)), enqueue)
        if self.trip_policy == "reference":
            assert int(anyv.item()) == 1, "No sampled rays is valid."   # optics.py:902
        return center

    def psf(self, points, ks=31, wvln=DEFAULT_WAVE, spp=GEO_SPP, center=True):
        """optics.py:916-931."""
        return self.psf_diff(points=points, wvln=wvln, ks=ks, spp=spp, center=center)

    def psf_diff(self, points, wvln=DEFAULT_WAVE, ks=31, spp=GEO_SPP, center=True,
                 param_list=None, _defer=False, surface_params=None, d_sensor=None, glass_params=None,
                 point_grad=False):
        """optics.py:934-996: normalised points [N,3] (or [3]) -> max-normalised
        PSF [N,ks,ks] (or [ks,ks]) of the left sub-pixel (right if param_list[4] != 'l').
        d_sensor: the sensor position of this call; glass_params: its glass; point_grad: the gradient in the points
        through the rays (psf_lr)."""
        dp, right = _parse_param_list(param_list)
        res = self.psf_lr(points, ks=ks, wvln=wvln, spp=spp, center=center, dp=dp, want_r=right,
                          _default_r_zero=(param_list is None), defer=_defer, surface_params=surface_params,
                          d_sensor=d_sensor, glass_params=glass_params, point_grad=point_grad)
        pick = (lambda lr: lr[1]) if right else (lambda lr: lr[0])
        if _defer:
            return PendingPSF(lambda: pick(res.wait()))
        return pick(res)

    def to_host(self, t):
        """`t.to('cpu')` at PCIe speed: the copy goes into a PAGE-LOCKED buffer kept on the lens (one per shape and
        dtype, the two most recent kept) and the caller's stream is waited for -- a pageable destination, what
        Tensor.to('cpu') allocates, moved the 42.5 MB of the reference's timing harness (psfnet.py:570-586) at ~7 GB/s,
        a third of its span.  The returned CPU tensor IS that buffer: valid until the next to_host() of the same shape;
        `.clone()` it to keep it."""
        if not t.is_cuda:
            return t
        pool = self.__dict__.setdefault("_pinned_out", {})
        key = (tuple(t.shape), t.dtype)
        host = pool.pop(key, None)
        if host is None:
            while len(pool) >= 2:
                pool.pop(next(iter(pool)))
            host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        pool[key] = host                                    # most recent last
        host.copy_(t, non_blocking=True)
        torch.cuda.current_stream(t.device).synchronize()
        return host

    def _spp_slices(self, N, spp):
        """sdirt_psf_spp_slices for THIS lens's GPU (its CU count, whatever the caller's current device is)."""
        ncu = self.__dict__.get("_n_cus")
        if ncu is None:
            ncu = self.__dict__["_n_cus"] = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
        return _lib.lib().sdirt_psf_spp_slices(N, spp, ncu)

    def _centre_buffer(self, center_out, N):
        """The [N, 2] centre tensor of a psf call: the caller's (checked) or a fresh one."""
        if center_out is None:
            return torch.empty((N, 2), dtype=torch.float32, device=self.device)
        if not (center_out.is_cuda and center_out.dtype == torch.float32 and center_out.is_contiguous()
                and tuple(center_out.shape) == (N, 2)):
            raise ValueError("center_out must be a contiguous float32 CUDA [N, 2] tensor")
        return center_out

    def _on_device(self, v):
        """Explicit pupil sample points (tensor or array, on any device) -> contiguous float32 on the lens's device."""
        return torch.as_tensor(v).to(self.device, torch.float32).contiguous()

    def _pinhole_centres(self, points, cen):
        """cen[:] = the pinhole image points of the normalised `points` (optics.py:973-975): the centres of center=False."""
        pts = points.to(self.device, torch.float32)
        cen[:, 0] = pts[:, 0] * (self.sensor_size[1] / 2)
        cen[:, 1] = pts[:, 1] * (self.sensor_size[0] / 2)
        return cen

    def _psf_buffers(self, out, N, ks, need_r):
        """(L, R) [N, ks, ks] of a psf call: the caller's `out` pair (checked) or fresh tensors; R is None when
        the call fills no right grid.  out = ONE float32 CUDA [N, 2, ks, ks] tensor: L = out[:, 0], R = out[:, 1]
        (SDIRT_PSF_INTERLEAVED: the block a multi-GPU volume gathers with one collective, dist.py)."""
        if torch.is_tensor(out):
            if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                    and tuple(out.shape) == (N, 2, ks, ks)):
                raise ValueError("out as ONE tensor must be contiguous float32 CUDA [N, 2, ks, ks]")
            if not need_r:
                raise ValueError("out=[N, 2, ks, ks] holds a left AND a right grid per point: needs dp and want_r")
            return out[:, 0], out[:, 1]
        if out is None:
            L = torch.empty((N, ks, ks), dtype=torch.float32, device=self.device)
            return L, (torch.empty_like(L) if need_r else None)
        L, R = out[0], (out[1] if need_r else None)
        for t_ in (L, R):
            if t_ is not None and not (t_.is_cuda and t_.dtype == torch.float32 and t_.is_contiguous()
                                       and tuple(t_.shape) == (N, ks, ks)):
                raise ValueError("out tensors must be contiguous float32 CUDA [N, ks, ks]")
        return L, R

    def psf_lr(self, points, ks=31, wvln=DEFAULT_WAVE, spp=GEO_SPP, center=True,
               dp=(0.78, 1.44, 0.3, 0.5), normalize=True, want_r=True, _default_r_zero=False,
               pupil_xy=None, center_pupil_xy=None, out=None, defer=False, center_out=None, surface_params=None,
               d_sensor=None, _focus=None, glass_params=None, energy=False, point_grad=False):
        """Left AND right dual-pixel PSFs of one ray-traced batch: (L, R), each
        [N,ks,ks] (or [ks,ks] for a single point), max-normalised separately as
        optics.py:983-987 would normalise each of them.  dp = (h, f, w, r) of
        monte_carlo.py:157-164.

        pupil_xy / center_pupil_xy: optional explicit pupil sample points
        (x2[spp], y2[spp]) for the primary and the chief-ray pass; when given,
        no random numbers are drawn for that pass (used for ray-level parity
        hand-off and for quasi-random sampling).

        out: optional (L, R) float32 CUDA tensors [N,ks,ks] to write into -- a consumer
        that renders batch after batch (PSFNet fitting) re-uses its buffers instead of
        asking the caching allocator for two 277 MB blocks per call.  Or ONE [N,2,ks,ks]
        tensor: the returned L and R are its views out[:, 0] and out[:, 1] (a rank of a
        sharded volume renders straight into the block that one all-gather moves).

        center_out: optional float32 CUDA [N,2] tensor that receives the PSF centres the splat used
        (the chief-ray centres of optics.py:969 with center=True).

        defer=True (center=True only): enqueue the kernel with the speculated Newton trip tables
        and return a `PendingPSF` at once; its `.wait()` reads the convergence masks back,
        verifies them (re-launching in the rare case the speculation was wrong) and returns
        (L, R).  A caller that renders batch after batch keeps one call in flight -- the GPU
        starts batch i+1 while the host checks batch i -- without giving up the check.  Every
        round of a call runs on the stream that was current when it was enqueued.

        Differentiable (optics.py:934-996 under autograd) when grad mode is on and h, f or w of dp -- or, with
        center=False, `points` -- require a gradient: the call then runs the staged chain and the splat through
        monte_carlo.SplatFunction (_psf_lr_grad).  r, the wavelength, the rays and, with center=True,
        the points get no gradient.  out=, center_out= and defer=True are refused there.

        (trip_policy='adaptive' is refused with a theta that requires a gradient: its per-wave trip counts are not recorded.)
        surface_params: a surface_parameters()-shaped tensor theta.  When it requires a gradient (and grad mode is on)
        the PSFs are those of the lens set_surface_parameters(theta.detach()) would make -- the records are put back
        afterwards -- and loss.backward() fills theta.grad with the gradient the reference's graph gives d, c, k and
        ai of every surface (trace_grad.SurfaceGradFunction); h, f, w and the points get theirs in the
        same call.  Otherwise the call is set_surface_parameters(theta) followed by the ordinary call.

        d_sensor: the sensor position (the focus setting) of THIS call, a number or a one-element tensor; None: the
        lens's.  The call renders with it on every path and leaves lens.d_sensor as it was, also when it raises.  A
        0-d tensor that requires a gradient (in grad mode) makes it a grad call, and loss.backward() fills its .grad:
        a ray meets the sensor plane at o' + d (s - o'.z) / d.z, so the splat shifts by d.xy / d.z per unit of s, and
        with center=True the chief-ray centre moves with the sensor as well, which is part of the derivative (the
        reference keeps that centre out of its graph).  The points' z are positions in the lens frame
        and do not move with the sensor; hfov, r_last and the pinhole scale stay constants.

        glass_params: a glass_parameters()-shaped tensor [K + 1, 2] (n, V of every medium), next to surface_params.
        When it requires a gradient the PSFs are those of the lens set_glass_parameters(glass.detach()) would make -- the
        Material objects are put back afterwards -- and loss.backward() fills its .grad with the gradient the
        reference's graph gives n and V of every owned medium (glass_owned(); the other rows get exactly 0) at this
        call's wavelength: eta = n1(lambda) / n2(lambda) of every refraction carries it; the pupil, the
        chief-ray centres and every validity test stay constants.  Otherwise the call is set_glass_parameters(glass)
        followed by the ordinary call.  defer, out=, center_out= and trip_policy='adaptive' are refused with a gradient
        as they are for surface_params; all of surface_params, glass_params and d_sensor may require one in one call.

        energy=True: -> (L, R, E), E [N, 3] float64 ([3] for a single point) = (E_L, E_R, T): the sums over ALL spp
        rays of the point, inside the ks window or not, of ra d_l(x_tan), ra d_r(x_tan) and ra, divided by spp
        (monte_carlo.dp_energy): the left and right energy -- lens vignetting times the dual-pixel shading the
        normalisations above discard -- and the share T of the sampled rays that reach the sensor.  Such a call takes
        the staged chain at every ks (L and R are that chain's); dp is required, defer=True and _default_r_zero are
        refused.  In grad mode E has gradients in h, f, w, and with surface_params / glass_params its rays' terms join
        the splat's for the one walk of the recorded trace; d_sensor gets exactly 0 from E.

        point_grad=True: `points` gets its whole gradient -- how the rays, and so the blur shape, the L/R disparity and
        the energy, change with x, y and the depth -- in both centre modes: the derivative of optics.py:934-996 with the
        two @torch.no_grad() of sample_from_points and psf_center taken off and the four pupil draws held fixed; the
        depth's way into point_obj.xy through the pinhole scale is part of it.  With grad mode on and points.requires_grad the call is a grad call: the staged chain with a
        recorded trace, trace_grad.PointGradFunction behind the raw grids (and behind E), and with center=True the
        chief-ray centre in the graph through a staged, recorded chief bundle (the fused pass's centres, bit for bit).
        With center=False the pinhole-centre term of the default call is kept and the rays' term is added to it.  The
        default, False, leaves every call and gradient as it was.  It composes with surface_params, glass_params and
        d_sensor; each keeps its own walk over the one record.  defer, out=, center_out= and trip_policy='adaptive' are
        refused as for surface_params; with points that require no gradient it is the ordinary call.  Workspace:
        24 (K + 1) bytes per ray for the primary record and again for the 2048 N chief rays of center=True (rf50mm:
        0.64 MB per point), held until the graph is freed."""
        if energy and (defer or _default_r_zero or dp is None):
            raise ValueError("energy=True needs dp and the staged chain: defer=True and _default_r_zero are not supported")
        if d_sensor is not None:
            focus = d_sensor if _requires_grad(d_sensor) else None
            if focus is not None and focus.numel() != 1:
                raise ValueError("d_sensor must be a 0-d (one-element) tensor to get a gradient")
            with self._sensor_borrowed(d_sensor):
                res = self.psf_lr(points, ks, wvln, spp, center, dp, normalize, want_r, _default_r_zero, pupil_xy,
                                  center_pupil_xy, out, defer, center_out, surface_params, None, focus, glass_params,
                                  energy, point_grad)
            if isinstance(res, PendingPSF):
                # the trip check of a deferred call may launch again: with this call's sensor position
                def finish(pending=res):
                    with self._sensor_borrowed(d_sensor):
                        return pending.wait()
                return PendingPSF(finish)
            return res
        focus_kw = {} if _focus is None else {"focus": _focus}
        if energy:
            focus_kw["energy"] = True
        if point_grad and _requires_grad(points):
            if self.trip_policy == "adaptive":
                raise ValueError("point_grad=True needs trip_policy 'reference' or 'max': the per-wave trip counts of "
                                 "'adaptive' are not recorded")
            focus_kw["point_grad"] = True
        if glass_params is not None and not _requires_grad(glass_params):
            self.set_glass_parameters(glass_params)
            glass_params = None
        if surface_params is not None and not _requires_grad(surface_params):
            self.set_surface_parameters(surface_params)
            surface_params = None
        if surface_params is not None or glass_params is not None:
            args = (points, ks, wvln, spp, center, dp, normalize, want_r, _default_r_zero, pupil_xy, center_pupil_xy,
                    out, defer, center_out)
            with contextlib.ExitStack() as borrowed:
                if surface_params is not None:
                    borrowed.enter_context(self._surfaces_borrowed(surface_params))
                if glass_params is not None:
                    borrowed.enter_context(self._glass_borrowed(glass_params))
                return self._psf_lr_grad(*args, surface_params=surface_params, glass_params=glass_params, **focus_kw)
        if "point_grad" in focus_kw or _psf_needs_grad(dp if not _default_r_zero else None, points, center, _focus):
            return self._psf_lr_grad(points, ks, wvln, spp, center, dp, normalize, want_r, _default_r_zero,
                                     pupil_xy, center_pupil_xy, out, defer, center_out, **focus_kw)
        return self._psf_lr(points, ks, wvln, spp, center, dp, normalize, want_r, _default_r_zero, pupil_xy,
                            center_pupil_xy, out, defer, center_out, energy)

    @torch.no_grad()
    def _psf_lr(self, points, ks, wvln, spp, center, dp, normalize, want_r, _default_r_zero, pupil_xy,
                center_pupil_xy, out, defer, center_out, energy=False):
        """psf_lr without autograd: the fused kernels (ks <= SDIRT_MAX_KS) or the staged chain (larger grids, and every
        call that asks for the energy: it is a sum over the sensor-plane bundle, which only that chain holds)."""
        self._require_gpu()
        if not torch.is_tensor(points):
            points = torch.tensor(points)
        single_point = points.dim() == 1
        if single_point:
            points = points.unsqueeze(0)
        N = points.shape[0]
        if torch.is_tensor(out) and (dp is None or _default_r_zero or not want_r):
            raise ValueError("out=[N, 2, ks, ks] holds a left AND a right grid per point: needs dp and want_r")
        reference = self.trip_policy == "reference"
        if N == 0 and energy:
            e = torch.empty((0, ks, ks), dtype=torch.float32, device=self.device)
            return e, (e.clone() if want_r else None), torch.zeros((0, 3), dtype=torch.float64, device=self.device)
        if N == 0 and not (self.mask_reduce is not None and center and reference):
            # empty batch: nothing to trace, no random numbers drawn
            e = torch.empty((0, ks, ks), dtype=torch.float32, device=self.device)
            res = (e, (e.clone() if want_r else None))
            return PendingPSF(lambda: res) if defer else res
        # (an empty SHARD of a multi-rank call goes on: its rank must enter the same mask
        # reductions and take the same re-launch decisions as its peers, with nothing to launch)
        po = self._points_to_object(points) if N else torch.empty((0, 3), device=self.device)
        if ks > _lib.MAX_KS or energy:
            # a point's two grids no longer fit in LDS (draw_mtf: ks 256): the staged chain
            if defer or torch.is_tensor(out):
                raise ValueError(f"defer=True / out=[N, 2, ks, ks] need ks <= {_lib.MAX_KS} and no energy")
            return self._psf_lr_staged(points, po, N, ks, wvln, spp, center, dp, normalize, want_r,
                                       _default_r_zero, pupil_xy, center_pupil_xy, out, center_out, single_point, energy)
        if defer and not center:
            raise ValueError("defer=True needs center=True")
        call = self._psf_request(po, ks, wvln, center, dp, normalize, want_r, _default_r_zero, out, center_out,
                                 single_point)
        if (center and pupil_xy is None and center_pupil_xy is None and N > 0 and not defer and reference
                and self.mask_reduce is None and self.pupil_mapping == "device" and self.kernel_events is None
                and self._spp_slices(N, spp) > 1):
            return self._psf_call_one(call, spp)
        self._draw_pupil_points(call, points, spp, center, pupil_xy, center_pupil_xy, side_stream=defer)
        if not center:
            return self._psf_uncentred(call)
        if not reference:
            return self._psf_fixed(call, defer)
        if self.mask_reduce is None and N > 0 and self._spp_slices(N, call.spp) > 1:
            return self._psf_device_verified(call, defer)
        return self._psf_host_verified(call, defer)

    def _psf_request(self, po, ks, wvln, center, dp, normalize, want_r, default_r_zero, out, center_out, single_point):
        """What every launch of a psf_lr call takes, but its pupil points: output and centre buffers, dual-pixel
        parameters, flags, lens handles (the chief-ray pass always through the green lens, optics.py:900), trip-table
        keys and the caller's current stream (`st`: as the library's stream argument)."""
        N = po.shape[0]
        L, R = self._psf_buffers(out, N, ks, want_r and not default_r_zero)
        dpp = None if (dp is None or default_r_zero) else _lib.DpParams(*[float(v) for v in dp])
        wkey = round(float(wvln if wvln < 10 else wvln * 1e-3), 6)
        stream = torch.cuda.current_stream(self.device)
        return _PsfCall(N=N, ks=ks, po=po, L=L, R=R, cen=self._centre_buffer(center_out, N), want_r=want_r,
                        single_point=single_point, dp=C.byref(dpp) if dpp is not None else None,
                        flags=(_lib.PSF_NORMALIZE if normalize else 0) | self._psf_flags()
                        | (_lib.PSF_INTERLEAVED if torch.is_tensor(out) else 0),
                        handle=self.dev_lens(wvln), handle_c=self.dev_lens(DEFAULT_WAVE) if center else None,
                        pupilz=self.entrance_pupil()[0], keys=[("psf", wkey, self.precision), ("center", self.precision)],
                        stream=stream, st=_lib.StreamArg(stream.cuda_stream, self.device.index))

    def _draw_pupil_points(self, call, points, spp, center, pupil_xy, center_pupil_xy, side_stream):
        """The call's pupil sample points -- the explicit ones, or drawn in the reference's order: primary samples first
        (optics.py:963), then the chief-ray samples of psf_center (optics.py:969), both sets in one draw and upload when
        both are drawn -- and, with center=False, its centres: the pinhole image points."""
        pupilr, pupilr_c = self.entrance_pupil()[1], self.entrance_pupil(shrink_pupil=True)[1]
        xc = yc = None
        if pupil_xy is None and center and center_pupil_xy is None:
            x2, y2, xc, yc = self._pupil_samples_pair(spp, pupilr, GEO_SPP, pupilr_c, side_stream=side_stream)
        else:
            x2, y2 = self._pupil_samples(spp, pupilr) if pupil_xy is None else map(self._on_device, pupil_xy)
            if center:
                xc, yc = (self._pupil_samples(GEO_SPP, pupilr_c) if center_pupil_xy is None
                          else map(self._on_device, center_pupil_xy))
        if not center:
            self._pinhole_centres(points, call.cen)
        call.x2, call.y2, call.xc, call.yc, call.spp = x2, y2, xc, yc, x2.shape[0]
        #: the pupil sample points of the most recent psf_lr call (x2, y2, xc, yc), device tensors
        self.last_pupil_points = (x2, y2, xc, yc)

    def _psf_call_one(self, call, spp):
        """The fitting shape (few points, many samples: launch-latency-bound) through ONE library call, sdirt_psf_call:
        the host draws the 2 spp + 2 x 2048 uniforms (one torch.rand, the reference's order) into page-locked memory; the
        call enqueues their upload, the two pupil mappings, both rounds of the device-verified render and the copy of
        the control block into the lens's page-locked mirror; the host waits for it and checks what the device did.
        Same results as the general path."""
        h, K, Sc = _lib.lib(), len(self.surfaces), GEO_SPP
        # a long streak of right bets (a caller rendering the same batch again and again): the correction
        # round is not even enqueued -- if the device's check fails after all, the host launches it (_settle)
        if self.__dict__.get("_right_streak", 0) >= 32:
            call.flags |= _lib.PSF_ONE_ROUND
        tables = [self.trips.initial(k, self._curved()) for k in call.keys]
        n = 2 * (spp + Sc)
        words = int(h.sdirt_psf_call_scratch_bytes(call.N, spp, Sc) // 4)
        scratch = self._zeroed_control_block(words)
        hbuf = self._ctl_mirror()
        stage, uploaded = self._staging(n, rows=1)
        _hostrng.rand_into(stage[0])                         # the reference's four draws, in one (see _pupil_samples_pair)
        _lib.check(h.sdirt_psf_call(
            call.handle, call.handle_c, dptr(call.po), call.N, C.c_void_p(stage.data_ptr()), spp, Sc,
            float(self.entrance_pupil()[1]), float(self.entrance_pupil(shrink_pupil=True)[1]), float(call.pupilz),
            float(self.d_sensor), float(self.pixel_size), call.ks, call.dp, _c_trips(tables[0]), _c_trips(tables[1]),
            call.flags, dptr(call.cen), dptr(call.L), dptr(call.R), dptr(scratch), C.c_void_p(hbuf.data_ptr()),
            call.st))
        uploaded.record(call.stream)
        done = torch.cuda.Event()
        done.record(call.stream)
        done.synchronize()
        # the pupil points the device mapped: behind the control block and the partial sums in `scratch`
        xy = scratch[words - n:].view(torch.float32)
        call.x2, call.y2, call.xc, call.yc = xy[:spp], xy[spp:2 * spp], xy[2 * spp:2 * spp + Sc], xy[2 * spp + Sc:]
        call.spp = spp
        self.last_pupil_points = (call.x2, call.y2, call.xc, call.yc)
        ctl = _lib.decode_ctl(hbuf.numpy(), K, one_round=bool(call.flags & _lib.PSF_ONE_ROUND))
        self.__dict__["_right_streak"] = self.__dict__.get("_right_streak", 0) + 1 if ctl.status == 0 else 0
        return self._settle_ctl(call, tables, ctl)

    def _psf_device_verified(self, call, defer):
        """Few points, many samples (several workgroups per point): speculate, verify ON THE DEVICE, re-render once
        behind it -- no host round trip when the bet on the trip tables was wrong (sdirt_psf_lr_verified).  The control
        block is copied into the lens's page-locked mirror and the stream waited for, or (defer=True) copied on the
        read-back stream and checked in .wait()."""
        words = _lib.lib().sdirt_psf_verified_scratch_bytes(call.N, call.xc.shape[0]) // 4
        scratch = self._zeroed_control_block(int(words))
        tables = [self.trips.initial(k, self._curved()) for k in call.keys]
        with self._timed("psf_lr_verified"):
            _lib.check(_lib.lib().sdirt_psf_lr_verified(
                call.handle, call.handle_c, dptr(call.po), call.N, dptr(call.x2), dptr(call.y2), call.spp,
                dptr(call.xc), dptr(call.yc), call.xc.shape[0], float(call.pupilz), float(self.d_sensor),
                float(self.pixel_size), call.ks, call.dp, _c_trips(tables[0]), _c_trips(tables[1]), call.flags,
                dptr(call.cen), dptr(call.L), dptr(call.R), dptr(scratch), call.st))
        if defer:
            host, done = self._readback(scratch, _lib.CTL_WORDS)

            def finish():
                done.synchronize()
                return self._settle_ctl(call, tables, _lib.decode_ctl(host.numpy(), len(self.surfaces)))
            return PendingPSF(finish)
        hbuf = self._ctl_mirror()
        hbuf.copy_(scratch[:_lib.CTL_WORDS], non_blocking=True)
        call.stream.synchronize()
        return self._settle_ctl(call, tables, _lib.decode_ctl(hbuf.numpy(), len(self.surfaces)))

    def _psf_host_verified(self, call, defer):
        """Every round read back and checked by the host (one workgroup per point, or a mask reduction over ranks).
        defer=True: the first round's control block -- OR-ed over the ranks, if a reduction is installed -- is copied
        on the read-back stream and checked in .wait()."""
        if not defer:
            return self._settle(call, [])
        n = 2 * _lib.MAX_SURFACES + 1
        tables = [self.trips.initial(k, self._curved()) for k in call.keys]
        ctl = self._zeroed_control_block(n)
        self._enqueue_centred(call, tables, ctl)
        host, done = self._readback(ctl, n, reduce=self.mask_reduce)

        def finish():
            done.synchronize()
            masks, any_valid = self._round_result(host.numpy())
            return self._settle(call, [(tables, masks)], any_valid)
        return PendingPSF(finish)

    def _psf_fixed(self, call, defer):
        """trip_policy 'max' / 'adaptive': one launch with the fixed trip table, nothing to check."""
        full = self._fixed_trips()
        self._enqueue_centred(call, (full, full), self._zeroed_control_block(2 * _lib.MAX_SURFACES + 1), masks=False)
        res = call.result()
        return PendingPSF(lambda: res) if defer else res

    def _psf_uncentred(self, call):
        """center=False: the primary pass alone (sdirt_psf_lr), centred on the pinhole image points."""
        def enqueue(trips, mask_ptr):
            with self._timed("psf_lr"):
                _lib.check(_lib.lib().sdirt_psf_lr(
                    call.handle, dptr(call.po), call.N, dptr(call.x2), dptr(call.y2), call.spp, float(call.pupilz),
                    float(self.d_sensor), float(self.pixel_size), call.ks, dptr(call.cen), call.dp, trips, call.flags,
                    dptr(call.L), dptr(call.R), mask_ptr, call.st))
        self._run_with_trips(call.keys[0], range(len(self.surfaces)), enqueue)
        return call.result()

    def _enqueue_centred(self, call, tables, ctl, masks=True):
        """sdirt_psf_lr_centered of `call` on the call's stream: chief-ray pass and primary pass in one C call -- one
        kernel launch when a workgroup owns a point -- with the trip tables (primary, chief-ray), OR-ing into the zeroed
        control block ctl = [primary masks | chief-ray masks | any-valid] (masks=False: into the any-valid word only)."""
        if call.N == 0:
            return
        MS = _lib.MAX_SURFACES
        with self._timed("psf_lr_centered"):
            _lib.check(_lib.lib().sdirt_psf_lr_centered(
                call.handle, call.handle_c, dptr(call.po), call.N, dptr(call.x2), dptr(call.y2), call.spp,
                dptr(call.xc), dptr(call.yc), call.xc.shape[0], float(call.pupilz), float(self.d_sensor),
                float(self.pixel_size), call.ks, call.dp, _c_trips(tables[0]), _c_trips(tables[1]), call.flags,
                dptr(call.cen), dptr(ctl[2 * MS:]), dptr(call.L), dptr(call.R), dptr(ctl[:MS]) if masks else None,
                dptr(ctl[MS:2 * MS]) if masks else None, call.st))

    def _centred_round(self, call, tables):
        """One host-driven round of a centred call, on the stream the call was enqueued on: the launch into a fresh
        zeroed control block from that stream's pool, the block OR-ed over the ranks when a mask reduction is installed
        (every rank verifies the same block, so all of them re-launch -- or raise -- together), read back.
        -> ([primary, chief-ray] masks, any-valid)."""
        with torch.cuda.stream(call.stream):
            ctl = self._zeroed_control_block(2 * _lib.MAX_SURFACES + 1)
            self._enqueue_centred(call, tables, ctl)
            if self.mask_reduce is not None:
                ctl.copy_(self.mask_reduce(ctl))
            return self._round_result(ctl.cpu().numpy())

    def _round_result(self, host):
        """A host-driven round's control block on the host -> ([primary, chief-ray] masks, any-valid)."""
        MS = _lib.MAX_SURFACES
        m = host[:2 * MS].reshape(2, MS)[:, :len(self.surfaces)].astype(np.int64) & 0xFFFFFFFF
        return [m[0], m[1]], int(host[2 * MS])

    def _settle_ctl(self, call, tables, ctl):
        """What a device-verified call did (_lib.decode_ctl): round 1 with `tables`, round 2 -- if it ran -- with the
        device's own correction; checked, and corrected further by the host if need be.  -> (L, R)."""
        rounds = [(tables, ctl.masks[0])] + [(ctl.trips2, m) for m in ctl.masks[1:]]
        return self._settle(call, rounds, ctl.any_valid)

    def _settle(self, call, rounds, any_valid=None):
        """Check the rounds a centred call has run -- [(tables, masks)]; none yet for the synchronous host-verified call
        -- with the reference's rule, and run host-driven rounds until it accepts (TripPlanner.run_many).  -> (L, R)."""
        state = [any_valid]

        def launch(tables):
            masks, state[0] = self._centred_round(call, tables)
            return masks
        self.trips.run_many(call.keys, self._curved(), list(range(len(self.surfaces))), launch, done=rounds)
        assert state[0] == 1, "No sampled rays is valid."   # optics.py:902
        return call.result()

    def _readback(self, block, n_words, reduce=None):
        """Asynchronous copy of the first n_words of a control block into page-locked memory on the read-back stream (on
        the caller's it would sit between this call's kernels and the next call's); -> (host tensor, event).  reduce: the
        mask reduction over ranks (a collective), issued on the read-back stream as well -- the caller's stream goes
        straight on to the next call's kernel instead of waiting for it."""
        main = torch.cuda.current_stream(self.device)
        rb = self._side_stream("_readback_stream")
        rb.wait_stream(main)
        host = torch.empty(n_words, dtype=block.dtype, pin_memory=True)
        with torch.cuda.stream(rb):
            src = block if reduce is None else reduce(block)
            host.copy_(src[:n_words], non_blocking=True)
        block.record_stream(rb)
        done = torch.cuda.Event()
        done.record(rb)
        return host, done

    def _ctl_mirror(self):
        """The lens's page-locked CTL_WORDS mirror of a control block, shared by the synchronous device-verified calls:
        each reads it before it returns."""
        hbuf = self.__dict__.get("_ctl_host")
        if hbuf is None:
            hbuf = self.__dict__["_ctl_host"] = torch.empty(_lib.CTL_WORDS, dtype=torch.int32, pin_memory=True)
        return hbuf

    def _psf_lr_staged(self, points, po, N, ks, wvln, spp, center, dp, normalize, want_r, default_r_zero,
                       pupil_xy, center_pupil_xy, out, center_out, single_point, energy=False):
        """psf_lr for SDIRT_MAX_KS < ks <= SDIRT_MAX_KS_STAGED (and, with energy=True, for every ks; then a sixth call,
        sdirt_dp_energy on the same bundle, gives E): the reference's own sequence of optics.py:962-987
        as five library calls -- sample_from_points, psf_center, trace2sensor, forward_integral (adds into the
        grids in HBM instead of LDS), normalise -- on [spp, N] rays held in HBM (28 bytes per ray).  Same rays,
        centres and trip tables as the fused kernel; the plots that ask for such grids (draw_mtf) trace a
        handful of points."""
        if not 2 <= ks <= _lib.MAX_KS_STAGED:
            raise _lib.SdirtError(f"ks={ks} outside [2,{_lib.MAX_KS_STAGED}]")
        cen = self._centre_buffer(center_out, N)
        ray, spp = self._staged_rays(points, po, N, wvln, spp, center, pupil_xy, center_pupil_xy, cen)
        L, R = self._psf_buffers(out, N, ks, want_r and not default_r_zero)
        dpp = None if (dp is None or default_r_zero) else _lib.DpParams(*[float(v) for v in dp])
        h, st = _lib.lib(), stream_ptr(self.device)
        with self._timed("forward_integral"):
            # normalised on the way out of the tiles (optics.py:983-987): no second pass over the grids
            _lib.check(h.sdirt_forward_integral(ray.c_rays(), spp, N, float(self.pixel_size), int(ks), dptr(cen),
                                                C.byref(dpp) if dpp is not None else None,
                                                self._math_flags() | (_lib.PSF_NORMALIZE if normalize else 0),
                                                dptr(L), dptr(R), st))
        if energy:
            with self._timed("dp_energy"):
                E = dp_energy(ray, dp, self.precision) / spp
            return (*_epilogue(L, R, want_r, single_point), E[0] if single_point else E)
        return _epilogue(L, R, want_r, single_point)

    def _chief_center_recorded(self, po, xc, yc, pupilz, center):
        """The chief-ray centres of `po` into `center` by the STAGED chain -- sdirt_sample_rays on the green lens,
        the recording trace, sdirt_center_from_rays -- the centres of the fused sdirt_chief_center, bit for bit.
        -> the TraceRecord of the chief bundle (24 (K + 1) bytes per ray, 2048 rays per point)."""
        N, S = po.shape[0], xc.shape[0]
        ray = Ray.empty((S, N), DEFAULT_WAVE, self.device)                         # optics.py:900: always green
        _lib.check(_lib.lib().sdirt_sample_rays(dptr(po), N, dptr(xc), dptr(yc), S, float(pupilz), ray.c_rays(),
                                                stream_ptr(self.device)))
        rec = self._trace2sensor_recorded(ray)
        anyv = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().sdirt_center_from_rays(ray.c_rays(), S, N, dptr(center), dptr(anyv),
                                                     stream_ptr(self.device)))
        if self.trip_policy == "reference":
            assert int(anyv.item()) == 1, "No sampled rays is valid."   # optics.py:902
        return rec

    def _staged_rays(self, points, po, N, wvln, spp, center, pupil_xy, center_pupil_xy, cen, record=False,
                     cen_slope=None, chief_record=None):
        """The first stages of the staged chain: sample_from_points, psf_center (or the pinhole centres of
        center=False) into `cen`, trace2sensor.  -> (the [spp, N] sensor-plane rays, spp); record=True: the trace
        keeps its checkpoints, -> (rays, spp, trace_grad.TraceRecord).  cen_slope (float64 [N, 2], center=True):
        the chief-ray pass also writes d(centre)/d(d_sensor) there.  chief_record (a list, center=True): the centres come
        from the staged, recorded chief bundle (_chief_center_recorded), whose TraceRecord is appended to it."""
        pupilz, pupilr = self.entrance_pupil()
        # optics.py:963 (first two draws)
        x2, y2 = self._pupil_samples(spp, pupilr) if pupil_xy is None else map(self._on_device, pupil_xy)
        spp = x2.shape[0]
        ray = Ray.empty((spp, N), wvln, self.device)
        _lib.check(_lib.lib().sdirt_sample_rays(dptr(po), N, dptr(x2), dptr(y2), spp, float(pupilz), ray.c_rays(),
                                                stream_ptr(self.device)))
        xc = yc = None
        if center:
            pupilz_c, pupilr_c = self.entrance_pupil(shrink_pupil=True)
            # optics.py:969 (draws three and four)
            xc, yc = (self._pupil_samples(GEO_SPP, pupilr_c) if center_pupil_xy is None
                      else map(self._on_device, center_pupil_xy))
            if chief_record is not None:
                chief_record.append(self._chief_center_recorded(po, xc, yc, pupilz_c, cen))
                if cen_slope is not None:
                    # the slope comes from the fused pass alone: one more chief-ray pass, the same centres
                    self._chief_center(po, xc, yc, pupilz_c, torch.empty_like(cen), cen_slope)
            else:
                self._chief_center(po, xc, yc, pupilz_c, cen, cen_slope)
        else:
            self._pinhole_centres(points, cen)
        self.last_pupil_points = (x2, y2, xc, yc)
        if record:
            return ray, spp, self._trace2sensor_recorded(ray)
        self.trace(ray, forward=True, _to_sensor=self.d_sensor)        # trace2sensor, one pass
        return ray, spp

    def _trace2sensor_recorded(self, ray):
        """trace2sensor (forward, out of place, the same trip-table key and verification as trace()) through
        sdirt_trace2sensor_record: the ray's storage is rebound to the sensor-plane bundle, -> the TraceRecord the
        backward pass walks."""
        if self.trip_policy == "adaptive":
            raise ValueError("surface gradients need trip_policy 'reference' or 'max': the per-wave trip counts of "
                             "'adaptive' are not recorded")
        K = len(self.surfaces)
        handle = self.dev_lens(ray.wvln)
        dev_lens = self._dev[float(ray.wvln)]
        nbytes = int(_lib.lib().sdirt_trace2sensor_grad_workspace_bytes(ray.numel, K))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
        dst = Ray.empty(ray.shape, ray.wvln, self.device, obliq=ray.has_obliq)

        def enqueue(trips, mask_ptr):
            _lib.check(_lib.lib().sdirt_trace2sensor_record(handle, trips, self._math_flags(), float(self.d_sensor),
                                                            ray.c_rays(), dst.c_rays(), ray.numel, mask_ptr, dptr(ws),
                                                            stream_ptr(self.device)))
        key = ("trace", round(float(ray.wvln), 6), 0, K, True, self.precision)
        trips = self._run_with_trips(key, list(range(K)), enqueue)
        ray._adopt(dst)
        return TraceRecord(dev_lens, trips, self.precision, self.d_sensor, ws, ray, K)

    def _psf_lr_grad(self, points, ks, wvln, spp, center, dp, normalize, want_r, default_r_zero, pupil_xy,
                     center_pupil_xy, out, defer, center_out, surface_params=None, focus=None, glass_params=None,
                     energy=False, point_grad=False):
        """psf_lr under autograd: the staged chain's rays and centres (no gradient: optics.py:459, :888 are no_grad),
        then the RAW grids through monte_carlo.SplatFunction -- differentiable in h, f, w and, with center=False, in
        the pinhole centres points[:, :2] * sensor_size / 2 (optics.py:973-976) -- and the max-normalisation of
        optics.py:983-987 as torch ops, so that its gradient goes to the arg-max pixel as in the reference.
        focus: the call's sensor position as a 0-d tensor that requires a gradient (the lens is already set to its
        value): the chief-ray pass also returns the centres' slope in it, and SplatFunction takes both.
        point_grad: the points get the gradient through the rays as well (the two no_grad decorators taken off, the
        pupil draws held fixed): the trace is recorded, trace_grad.PointGradFunction sits behind the raw
        grids (and the energy sums), and with center=True the centres are those of a staged, recorded chief bundle
        behind trace_grad.ChiefCentreFunction."""
        if defer or out is not None or center_out is not None:
            raise ValueError("defer=True, out= and center_out= are not supported when psf_lr records gradients")
        self._require_gpu()
        if not torch.is_tensor(points):
            points = torch.tensor(points)
        single_point = points.dim() == 1
        if single_point:
            points = points.unsqueeze(0)
        N = points.shape[0]
        if not 2 <= ks <= _lib.MAX_KS_STAGED:
            raise _lib.SdirtError(f"ks={ks} outside [2,{_lib.MAX_KS_STAGED}]")
        with torch.no_grad():
            po = self._points_to_object(points.detach())
            cen = torch.empty((N, 2), dtype=torch.float32, device=self.device)
            cen_slope = (torch.empty((N, 2), dtype=torch.float64, device=self.device)
                         if focus is not None and center else None)
            lens_grad = surface_params is not None or glass_params is not None
            record = lens_grad or point_grad
            chief = [] if point_grad and center else None
            staged = self._staged_rays(points.detach(), po, N, wvln, spp, center, pupil_xy, center_pupil_xy, cen,
                                       record=record, cen_slope=cen_slope, chief_record=chief)
            ray, spp = staged[:2]
        if point_grad:
            x2, y2, xc, yc = self.last_pupil_points

            def samples(x, y, pupil_z):
                return PointSamples(x, y, pupil_z, np.tan(self.hfov), self.r_last, self.sensor_size[1], self.sensor_size[0])
            if center:
                # the chief-ray centre in the graph: dLoss/d(centre), which SplatFunction returns, walks the chief bundle
                cen = ChiefCentreFunction.apply(points, cen, chief[0],
                                                samples(xc, yc, self.entrance_pupil(shrink_pupil=True)[0]))
        if not center:
            # the pinhole centres of _pinhole_centres as torch ops on the caller's points: the same fp32 products
            pts = points.to(self.device, torch.float32)
            cen = torch.stack((pts[:, 0] * (self.sensor_size[1] / 2), pts[:, 1] * (self.sensor_size[0] / 2)), -1)
        param_list = None if (dp is None or default_r_zero) else (*dp[:4], "l")
        L, R = splat_autograd(ray, self.pixel_size, ks, cen, param_list, self.precision, focus, cen_slope)
        # the sums over the whole bundle (EnergyFunction: h, f, w; exactly 0 to the sensor position)
        Es = dp_energy(ray, param_list, self.precision, focus) if energy else None
        if record:
            # the rays' share of the graph: dLoss/d(raw grids) -> the sensor-plane rays -> the recorded trace -> theta
            # and eta(glass) (the lens is the borrowed one: its constants' indices are those the device table holds)
            dpp = None if param_list is None else _lib.DpParams(*[float(v) for v in param_list[:4]])
            cen_c = cen.detach().to(self.device, torch.float32).reshape(N, 2).contiguous()
            staged[2].center = cen_c
        if lens_grad:
            eta = None if glass_params is None else self._glass_eta(glass_params, wvln)
            if energy:
                L, R, Es = SurfaceGradFunction.apply(surface_params, eta, L, R, staged[2], cen_c, self.pixel_size, ks, dpp, Es)
            else:
                L, R = SurfaceGradFunction.apply(surface_params, eta, L, R, staged[2], cen_c, self.pixel_size, ks, dpp)
        if point_grad:
            # the points' share through the rays: a walk of its own over the same record
            args = (points, L, R, staged[2], cen_c, self.pixel_size, ks, dpp, samples(x2, y2, self.entrance_pupil()[0]))
            if energy:
                L, R, Es = PointGradFunction.apply(*args, Es)
            else:
                L, R = PointGradFunction.apply(*args)
        if normalize:
            L = L / (L.reshape(N, -1).max(dim=-1).values.reshape(N, 1, 1) + 1e-6)
            R = R / (R.reshape(N, -1).max(dim=-1).values.reshape(N, 1, 1) + 1e-6)
        if not want_r:
            R = None
        if energy:
            E = Es / spp
            return (*_epilogue(L, R, want_r, single_point), E[0] if single_point else E)
        return _epilogue(L, R, want_r, single_point)

    def psf_volume(self, grid=(32, 32), z=16, ks=21, spp=GEO_SPP, dp=(0.78, 1.44, 0.3, 0.5), wvln=DEFAULT_WAVE,
                   surface_params=None, pupil_xy=None, center_pupil_xy=None, d_sensor=None, glass_params=None,
                   photometric=False):
        """The ray-traced PSF grid of the whole field and depth range as a render_psf.PSFVolume, for
        local_dp_psf_render_volume / PSFNet.render_volume: grid = (rows, columns) of cell-centred sensor nodes
        (psfnet.py:220-226: x from -1 + 1/(2 gx) to 1 - 1/(2 gx), y from 1 - 1/(2 gy) down), z = a number of depth
        nodes spread evenly over the normalised depth [0, 1], or a 1-D tensor of strictly monotone normalised depths;
        depth = z (d_max - d_min) + d_min with the lens's d_min / d_max (PSFNet's; -200 / -20000 mm on a plain
        Lensgroup, psfnet.py:15-16).

        ONE psf_lr call on the Dz*Gy*Gx points, so it is differentiable exactly where psf_lr is (h, f, w of dp,
        surface_params, glass_params, the call's sensor position d_sensor); L and R are stacked and each divided by its own sum with torch ops, which keeps the graph.

        wvln: a number -> psf [Dz,Gy,Gx,2,ks,ks].  A sequence of wavelengths (WAVE_RGB: the three of psf_rgb,
        optics.py:999-1015) -> a CHROMATIC volume, psf [Cw,Dz,Gy,Gx,2,ks,ks]: one psf_lr call per wavelength on the same
        points, each centred through the green lens as every psf_lr call is, with the same dp, surface_params,
        glass_params and d_sensor (the gradient of a shared parameter is the sum over the wavelengths), stacked on a new leading axis;
        psf[c] is the volume of wvln[c], rendered into image channel c.  pupil_xy / center_pupil_xy are then either
        (x[spp], y[spp]), shared by the wavelengths, or per wavelength, [2, Cw, spp] / [2, Cw, 2048] (psf_rgb's
        convention); without them every wavelength draws fresh samples, in the order given.

        photometric=True: the PSFs carry their energy.  Every wavelength's call is psf_lr(energy=True); the volume's
        `energy` holds the nodes' (E_L, E_R, T) [Dz,Gy,Gx,3] ([Cw,Dz,Gy,Gx,3]) and every node's sum-normalised L and R are
        multiplied by E[node, side] / mean(E[:, :2]), the mean over all nodes and both sides of that wavelength
        (render_psf.photometric_scale; torch ops, in the graph).  The render kernels normalise nothing, so the volume
        renders lens vignetting and dual-pixel shading as it stands, and an image loss reaches h, f, w and the lens
        through the energy as well as through the blur shape."""
        from .render_psf import PSFVolume, photometric_scale
        gy, gx = (int(grid), int(grid)) if np.isscalar(grid) else (int(grid[0]), int(grid[1]))
        z_nodes = (z.detach().to(torch.float32).reshape(-1).cpu() if torch.is_tensor(z)
                   else torch.linspace(0, 1, int(z)) if int(z) > 1 else torch.zeros(1))
        d_min, d_max = float(getattr(self, "d_min", -200.0)), float(getattr(self, "d_max", -20000.0))
        chromatic = not (np.isscalar(wvln) or (torch.is_tensor(wvln) and wvln.dim() == 0))
        waves = tuple(float(w) for w in wvln) if chromatic else (float(wvln),)
        if not waves:
            raise ValueError("psf_volume needs at least one wavelength")
        vol = PSFVolume(None, torch.linspace(-1 + 1 / (2 * gx), 1 - 1 / (2 * gx), gx),
                        torch.linspace(1 - 1 / (2 * gy), -1 + 1 / (2 * gy), gy), z_nodes, d_min, d_max, waves)

        def samples_of(xy, i):
            # (x[n], y[n]) for every wavelength, or [2, Cw, n]: wavelength i's pair
            if xy is None or not chromatic or xy[0].dim() == 1:
                return xy
            if len(xy[0]) != len(waves):
                raise ValueError(f"pupil points per wavelength must be [2, {len(waves)}, n], got {len(xy[0])} sets")
            return xy[0][i], xy[1][i]

        points, psfs, energies = vol.points(), [], []
        for i, w in enumerate(waves):
            L, R, *E = self.psf_lr(points, ks=ks, wvln=w, spp=spp, dp=dp, pupil_xy=samples_of(pupil_xy, i),
                                   center_pupil_xy=samples_of(center_pupil_xy, i), surface_params=surface_params,
                                   d_sensor=d_sensor, glass_params=glass_params, energy=bool(photometric))
            if photometric:
                energies.append(E[0].reshape(len(z_nodes), gy, gx, 3))
            psf = torch.stack((L, R), -3)                                          # [N, 2, ks, ks]
            psf = psf / psf.sum((-1, -2), keepdim=True).clamp_min(1e-30)           # (a node no ray reaches stays 0)
            psfs.append(psf.reshape(len(z_nodes), gy, gx, 2, ks, ks))
        vol.psf = torch.stack(psfs) if chromatic else psfs[0]
        if photometric:
            vol.energy = torch.stack(energies) if chromatic else energies[0]
            vol.psf = photometric_scale(vol.psf, vol.energy)
        dev = vol.psf.device
        vol.x_nodes, vol.y_nodes, vol.z_nodes = vol.x_nodes.to(dev), vol.y_nodes.to(dev), vol.z_nodes.to(dev)
        return vol

    def psf_rgb(self, points, ks=31, spp=GEO_SPP, center=True, param_list=None, pupil_xy=None,
                center_pupil_xy=None, surface_params=None, d_sensor=None, glass_params=None, point_grad=False):
        """optics.py:999-1015: [N,3,ks,ks] (or [3,ks,ks]) -- the three wavelengths of WAVE_RGB, each an
        independent psf_diff (fresh pupil draws, in the reference's order; every chief-ray centre
        through the green lens).  The three calls are ONE kernel launch whatever the number of points
        (center=True: sdirt_psf_rgb_centered; center=False: sdirt_psf_rgb -- lens table, pupil sets, trip
        tables and mask rows indexed by blockIdx.y) and one control-block readback.
        pupil_xy [2, 3, spp] / center_pupil_xy [2, 3, 2048]: explicit pupil sample points per
        wavelength instead of random draws (ray-level parity hand-off).
        d_sensor: the sensor position of this call (psf_lr).  When it requires a gradient the three wavelengths are
        three differentiable psf_lr calls, each centred through the green lens, and its gradient is their sum.
        glass_params: the glass of this call (psf_lr); with a gradient likewise, glass.grad the sum over the wavelengths.
        point_grad: the points' gradient through the rays (psf_lr); likewise, points.grad the sum over the wavelengths."""
        if not torch.is_tensor(points):
            points = torch.tensor(points)
        if center_pupil_xy is not None and not center:
            raise ValueError("center=False runs no chief-ray pass")
        focus_grad = d_sensor is not None and _requires_grad(d_sensor)
        if d_sensor is not None and not focus_grad:
            with self._sensor_borrowed(d_sensor):
                return self.psf_rgb(points, ks, spp, center, param_list, pupil_xy, center_pupil_xy, surface_params,
                                    None, glass_params, point_grad)
        n_points = points.shape[0] if points.dim() == 2 else 1
        dp, right = _parse_param_list(param_list)
        surface_grad = surface_params is not None and _requires_grad(surface_params)
        if surface_params is not None and not surface_grad:
            self.set_surface_parameters(surface_params)
        glass_grad = glass_params is not None and _requires_grad(glass_params)
        if glass_params is not None and not glass_grad:
            self.set_glass_parameters(glass_params)
        if (n_points > 0 and self.device.type == "cuda" and self.mask_reduce is None and ks <= _lib.MAX_KS
                and not surface_grad and not glass_grad and not focus_grad and not _psf_needs_grad(dp, points, center)
                and not (point_grad and _requires_grad(points))):
            return self._psf_rgb_fused(points, ks, spp, center, param_list, pupil_xy, center_pupil_xy)
        # not one launch (grids above SDIRT_MAX_KS, a rank of a sharded run, or a call that records gradients: one
        # differentiable psf_diff per wavelength, stacked, as optics.py:1010-1014 does): wavelength by wavelength
        # through psf_lr, which takes the explicit points of that wavelength on every path
        psfs = []
        for i, w in enumerate(WAVE_RGB):
            lr = self.psf_lr(points, ks=ks, wvln=w, spp=spp, center=center, dp=dp, want_r=right,
                             _default_r_zero=(param_list is None),
                             pupil_xy=None if pupil_xy is None else (pupil_xy[0][i], pupil_xy[1][i]),
                             center_pupil_xy=None if center_pupil_xy is None else (center_pupil_xy[0][i], center_pupil_xy[1][i]),
                             surface_params=surface_params if surface_grad else None,
                             d_sensor=d_sensor if focus_grad else None,
                             glass_params=glass_params if glass_grad else None, point_grad=point_grad)
            psfs.append(lr[1] if right else lr[0])
        return torch.stack(psfs, dim=-3)

    @torch.no_grad()
    def _psf_rgb_fused(self, points, ks, spp, center, param_list, pupil_xy=None, center_pupil_xy=None):
        """psf_rgb as one launch: three wavelength slots, one fresh primary sample set per wavelength (two random
        vectors each, optics.py:963) and, with center=True, one chief-ray set after it (sdirt_psf_rgb_centered); with
        center=False the PSFs centred on the pinhole image points (sdirt_psf_rgb, optics.py:972-976).  One
        control-block readback for all the trip checks."""
        single_point = points.dim() == 1
        pts = points.reshape(-1, 3)
        N, W, K, MS = pts.shape[0], len(WAVE_RGB), len(self.surfaces), _lib.MAX_SURFACES
        dp, want_r = _parse_param_list(param_list)
        dpp = None if dp is None else _lib.DpParams(*[float(v) for v in dp])
        dp_ref = C.byref(dpp) if dpp is not None else None
        po = self._points_to_object(pts)
        pupilz, pupilr = self.entrance_pupil()
        _, pupilr_c = self.entrance_pupil(shrink_pupil=True)
        # the reference's draw order: per wavelength, primary samples then chief-ray samples
        prim, cent = [], []
        for _ in WAVE_RGB:
            if pupil_xy is None:
                prim.append(torch.stack(self._pupil_samples(spp, pupilr)))
            if center and center_pupil_xy is None:
                cent.append(torch.stack(self._pupil_samples(GEO_SPP, pupilr_c)))
        prim = torch.stack(prim, 1).contiguous() if pupil_xy is None else self._on_device(pupil_xy)     # [2, W, S]
        spp = prim.shape[2]
        handles = (C.c_void_p * W)(*[self.dev_lens(w).value for w in WAVE_RGB])
        if center:
            cent = torch.stack(cent, 1).contiguous() if center_pupil_xy is None else self._on_device(center_pupil_xy)
            handle_c = self.dev_lens(DEFAULT_WAVE)                # optics.py:900: always green
            cen = torch.empty((W, N, 2), dtype=torch.float32, device=self.device)
        else:
            one = self._pinhole_centres(pts, torch.empty((N, 2), dtype=torch.float32, device=self.device))
            cen = one.unsqueeze(0).expand(W, N, 2).contiguous()                                      # the same for every colour
        L = torch.empty((N, W, ks, ks), dtype=torch.float32, device=self.device)
        R = torch.empty_like(L) if want_r else None
        flags = _lib.PSF_NORMALIZE | self._psf_flags()
        # one control block: [primary masks W x MS | chief-ray masks W x MS (center=True) | any-valid W]
        P = 2 if center else 1
        ctl = torch.zeros(P * W * MS + W, dtype=torch.int32, device=self.device)
        masks = ctl[:P * W * MS].view(P, W, MS)
        reference = self.trip_policy == "reference"

        def enqueue(tables):
            tp = _c_trips(np.concatenate([np.asarray(t, np.int32) for t in tables[:W]]))
            if not center:
                with self._timed("psf_rgb"):
                    _lib.check(_lib.lib().sdirt_psf_rgb(
                        handles, W, dptr(po), N, dptr(prim[0]), dptr(prim[1]), spp, float(pupilz), float(self.d_sensor),
                        float(self.pixel_size), ks, dptr(cen), dp_ref, tp, flags, dptr(L), dptr(R),
                        dptr(masks[0]) if reference else None, stream_ptr(self.device)))
                return
            tc = _c_trips(np.concatenate([np.asarray(t, np.int32) for t in tables[W:]]))
            with self._timed("psf_rgb_centered"):
                _lib.check(_lib.lib().sdirt_psf_rgb_centered(
                    handles, W, handle_c, dptr(po), N, dptr(prim[0]), dptr(prim[1]), spp,
                    dptr(cent[0]), dptr(cent[1]), GEO_SPP, float(pupilz), float(self.d_sensor),
                    float(self.pixel_size), ks, dp_ref, tp, tc, flags, dptr(cen), dptr(ctl[P * W * MS:]), dptr(L), dptr(R),
                    dptr(masks[0]) if reference else None, dptr(masks[1]) if reference else None,
                    stream_ptr(self.device)))

        if reference:
            keys = [("psf", round(float(w), 6), self.precision) for w in WAVE_RGB] + \
                   ([("center", self.precision)] * W if center else [])

            def launch(tables):
                ctl.zero_()
                enqueue(tables)
                host = ctl.cpu().numpy()
                launch.any_valid = host[P * W * MS:]
                return list(host[:P * W * MS].reshape(P * W, MS)[:, :K].astype(np.int64) & 0xFFFFFFFF)
            self.trips.run_many(keys, self._curved(), list(range(K)), launch)
            assert not center or bool(np.all(launch.any_valid == 1)), "No sampled rays is valid."   # optics.py:902
        else:
            enqueue([self._fixed_trips()] * (P * W))
        out = R if want_r else L
        return out.squeeze(0) if single_point else out

    def psf_map(self, depth=DEPTH, grid=7, ks=51, spp=GEO_SPP, center=True):
        """optics.py:1018-1041: the RGB PSFs of a grid x grid field of point sources at one depth,
        tiled into one [3, grid*ks, grid*ks] image (what torchvision's make_grid(nrow=grid,
        padding=0) assembles: PSF i sits in tile row i // grid, tile column i % grid)."""
        field = self.point_source_grid(depth=depth, grid=grid).reshape(grid * grid, 3)
        tiles = self.psf_rgb(points=field, ks=ks, center=center, spp=spp)        # [grid^2, 3, ks, ks]
        return tiles.view(grid, grid, 3, ks, ks).permute(2, 0, 3, 1, 4).reshape(3, grid * ks, grid * ks)

    def psf2mtf(self, psf, diag=False):
        """optics.py:1043-1080: the modulation transfer along the two axes of a PSF kernel -- |FFT| of its
        centre row (sagittal) and centre column (tangential), each normalised to its maximum, at the
        positive frequencies [cycles/mm] of a pixel_size sampling.  -> (freq, tangential, sagittal), numpy."""
        k = psf.detach().cpu().numpy() if torch.is_tensor(psf) else np.asarray(psf)
        row, col = k[k.shape[0] // 2, :], k[:, k.shape[1] // 2]
        sagittal, tangential = np.abs(np.fft.fft(row)), np.abs(np.fft.fft(col))
        sagittal, tangential = sagittal / sagittal.max(), tangential / tangential.max()
        freq = np.fft.fftfreq(k.shape[0], self.pixel_size)
        keep = freq > 0
        return freq[keep], tangential[keep], sagittal[keep]

    # the reference's plotting callers of the path (sdirt_amd/plots.py); each also returns what it drew
    def draw_psf_map(self, grid=9, depth=DEPTH, ks=51, log_scale=False, quater=False, save_name=None):
        """optics.py:1884-1931."""
        from . import plots
        return plots.draw_psf_map(self, grid, depth, ks, log_scale, quater, save_name)

    def draw_psf_radial(self, M=3, depth=DEPTH, ks=51, log_scale=False, save_name="./psf_radial.png"):
        """optics.py:1934-1956."""
        from . import plots
        return plots.draw_psf_radial(self, M, depth, ks, log_scale, save_name)

    def draw_mtf(self, relative_fov=[0.0, 0.7, 1.0], save_name="./mtf.png", wvlns=DEFAULT_WAVE, depth=DEPTH):
        """optics.py:2041-2067 (psf_diff at ks 256: the staged chain, _psf_lr_staged)."""
        from . import plots
        return plots.draw_mtf(self, relative_fov, save_name, wvlns, depth)

    # the lens report of the reference's fitting script and the samplers / measures under it (sdirt_amd/analysis.py)
    def analysis(self, save_name="./test", ks=None, render=False, multi_plot=False, plot_invalid=True,
                 zmx_format=False, depth=DEPTH, render_unwarp=False, lens_title=None):
        """optics.py:1663-1684."""
        from . import analysis as an
        return an.analysis(self, save_name, ks, render, multi_plot, plot_invalid, zmx_format, depth, render_unwarp,
                           lens_title)

    # ------------------------------------------------------- geometrical optics
    def calc_scale_pinhole(self, depth):
        """optics.py:1302-1306."""
        return -depth * np.tan(self.hfov) / self.r_last

    def calc_efl(self):
        """optics.py:1109-1114."""
        return self.r_last / np.tan(self.hfov)

    @torch.no_grad()
    def calc_fov(self):
        """optics.py:1203-1233: half diagonal field of view = atan of the validity-weighted mean slope
        dx/dz with which a fan of 100 rays leaves the lens towards the object, the fan starting at the
        sensor corner (r_last, 0, d_sensor) and aimed at points across the shrunk exit pupil."""
        n_fan = 100
        z_pupil, r_pupil = self.exit_pupil(shrink_pupil=True)
        corner = torch.tensor([float(self.r_last), 0.0, float(self.d_sensor)])
        aim = torch.zeros(n_fan, 3)
        aim[:, 0] = torch.linspace(-r_pupil, r_pupil, n_fan)
        aim[:, 2] = z_pupil
        fan = Ray(corner.expand(n_fan, 3), aim - corner, device=self.device)
        self.trace(fan, forward=False)
        dx, dz, weight = (fan.soa[row, :n_fan].cpu() for row in (3, 5, 6))
        half_fov = torch.atan((dx / dz * weight).sum() / weight.sum())
        if torch.isnan(half_fov):
            print("computed fov is NaN, use 0.5 rad instead.")
            return 0.5
        return half_fov.item()

    @torch.no_grad()
    def refocus(self, depth=DEPTH):
        """optics.py:1170-1196: put the sensor where green rays from the on-axis point at `depth`
        come closest to the axis.  GEO_SPP rays start on the first surface's aperture disc
        (surfaces.py:189-199; two vectors of uniforms from the CPU generator); each traced ray
        o + t d is nearest the axis at t = -(d.o)_xy / |d_xy|^2, i.e. at z = o_z - d_z (d.o)_xy /
        |d_xy|^2; the new sensor position is the mean of those z over the live rays (z > 0)."""
        front = self.surfaces[0]
        x, y = self._pupil_samples(GEO_SPP, front.r)
        start = torch.stack((x, y, torch.full_like(x, float(front.d))), dim=1)
        source = torch.tensor([0.0, 0.0, float(depth)], device=self.device)
        bundle = Ray(start, start - source, wvln=DEFAULT_WAVE, device=self.device)
        self.trace(bundle, forward=True)
        ox, oy, oz, dx, dy, dz, live = (row.cpu().numpy() for row in bundle.soa[:7, :x.shape[0]])
        with np.errstate(divide="ignore", invalid="ignore"):
            t_axis = (dx * ox + dy * oy) / (dx ** 2 + dy ** 2) * live
            z_axis = oz - dz * t_axis
        z_axis = z_axis[(live > 0) & ~np.isnan(z_axis) & (z_axis > 0)]
        d_sensor_new = float(np.mean(z_axis))
        assert d_sensor_new > 0, "sensor position is negative."
        self.d_sensor = d_sensor_new
        self.post_computation()

    def exit_pupil(self, shrink_pupil=False):
        """optics.py:1328-1332."""
        return self.entrance_pupil(entrance=False, shrink_pupil=shrink_pupil)

    def entrance_pupil(self, M=32, entrance=True, shrink_pupil=False):
        """optics.py:1379-1396 (z, r) of the paraxial pupil; the value is computed
        once per lens and cached (the reference re-traces it on every call)."""
        if self.aper_idx is None:
            s = self.surfaces[0] if entrance else self.surfaces[-1]
            return float(s.d), s.r
        if entrance not in self._pupil_cache:
            self._pupil_cache[entrance] = self.calc_entrance_pupil_paraxial(entrance=entrance)
        z, r = self._pupil_cache[entrance]
        if shrink_pupil:
            r = r * 0.25
        return z, r

    @torch.no_grad()
    def calc_entrance_pupil_paraxial(self, entrance=True):
        """optics.py:1335-1376: 16 paraxial rays from a point 1e-3 mm off-axis on the
        stop, traced out of the lens; the pairwise intersections of the emerging
        lines (in the x-z plane) give the pupil position and magnification.  The
        reference solves the 120 2x2 systems with an fp32 lstsq; here they are
        solved in closed form in float64 from the same fp32 rays."""
        aper = self.surfaces[self.aper_idx]
        aper_z, aper_r, delta_r = float(aper.d), aper.r, 1e-3
        ray_o = torch.tensor([[delta_r, 0, aper_z]]).repeat(16, 1)
        phi = torch.linspace(-0.1, 0.1, 16) / 180.0 * torch.pi
        sgn = -1.0 if entrance else 1.0
        d = torch.stack((torch.sin(phi), torch.zeros_like(phi), sgn * torch.cos(phi)), dim=-1)
        ray = Ray(ray_o, d, device=self.device)
        if entrance:
            ray, _, _ = self.trace(ray, lens_range=range(0, self.aper_idx), forward=False)
        else:
            ray, _, _ = self.trace(ray, lens_range=range(self.aper_idx + 1, len(self.surfaces)),
                                   forward=True)
        o_, d_, ra = ray.o.cpu(), ray.d.cpu(), ray.ra.cpu()
        keep = ra != 0
        O = torch.stack([o_[keep][:, 0], o_[keep][:, 2]], dim=-1)
        D = torch.stack([d_[keep][:, 0], d_[keep][:, 2]], dim=-1)
        if self.pupil_method == "reference":
            P = intersect_lines_2d_lstsq_fp32(O, D)
        else:
            P = torch.from_numpy(intersect_lines_2d(O.numpy().astype(np.float64),
                                                    D.numpy().astype(np.float64))).float()
        if len(P) == 0:
            print("No intersection points found, use the first surface as pupil.")
            return float(self.surfaces[0].d), self.surfaces[0].r
        avg_r = torch.abs((torch.mean(P[:, 0])) / delta_r * aper_r).item()
        avg_z = torch.mean(P[:, 1]).item()
        return avg_z, avg_r


def _bind_analysis(name):
    def method(self, *args, **kwargs):
        from . import analysis as an
        return getattr(an, name)(self, *args, **kwargs)
    method.__name__ = name
    method.__doc__ = f"sdirt_amd.analysis.{name} (the arguments of the reference's Lensgroup.{name})."
    return method


for _name in ("sample_parallel_2D", "sample_point_source_2D", "sample_pupil", "sample_point_source",
              "calc_magnification3", "calc_scale_ray", "analysis_rms", "calc_eqfl", "plot_setup2D", "plot_raytraces",
              "plot_setup2D_with_trace"):
    setattr(Lensgroup, _name, _bind_analysis(_name))


# the ray-traced render of a textured plane and the reference's sensor-side samplers (sdirt_amd/render_rt.py)
def _bind_render_rt(name):
    def method(self, *args, **kwargs):
        from . import render_rt
        return getattr(render_rt, name)(self, *args, **kwargs)
    method.__name__ = name
    method.__doc__ = f"sdirt_amd.render_rt.{name}."
    return method


for _name in ("sample_sensor", "trace2obj", "render_plane", "render_layers", "render_rgbd", "render_single_img"):
    setattr(Lensgroup, _name, _bind_render_rt(_name))


def intersect_lines_2d_lstsq_fp32(origins, directions):
    """optics.py:1470-1515 as the reference evaluates it: all pairs, the 2x2 systems
    [Di, -Dj] x = Oj - Oi solved in fp32 by torch.linalg.lstsq (CPU: LAPACK gelsy),
    both evaluations of the intersection averaged.  Host-side, 120 tiny systems.

    The batched gelsy call does not return the same bits for the FIRST system of a batch from one call to the next, on
    identical operands in one process, also alone and on one thread (observed with torch 2.10 on MKL: two or three
    outcomes for it, every later system reproducible).  The first pair's lines are adjacent and nearly parallel, so
    the outcomes differ in the fourth digit and move the pupil radius by 1.4e-4 relative.  A well-conditioned dummy
    system therefore takes the first place and is dropped: every real system is solved as the later ones always are,
    which is also what the first one gets in most plain calls."""
    n = origins.shape[0]
    idx_i, idx_j = torch.combinations(torch.arange(n), r=2).unbind(1)
    Oi, Oj, Di, Dj = origins[idx_i], origins[idx_j], directions[idx_i], directions[idx_j]
    b = Oj - Oi
    A = torch.stack([Di, -Dj], dim=-1)
    A = torch.cat((torch.eye(2, dtype=A.dtype).unsqueeze(0), A))
    b = torch.cat((torch.ones((1, 2), dtype=b.dtype), b))
    x = torch.linalg.lstsq(A, b.unsqueeze(-1))[0].squeeze(-1)[1:]
    P_i = Oi + x[:, 0].unsqueeze(-1) * Di
    P_j = Oj + x[:, 1].unsqueeze(-1) * Dj
    return (P_i + P_j) / 2


def intersect_lines_2d(origins, directions):
    """optics.py:1470-1515: pairwise intersections of N 2-D lines, [N(N-1)/2, 2].
    Solves Oi + s Di = Oj + t Dj exactly (float64) and averages both evaluations."""
    n = origins.shape[0]
    ii, jj = np.triu_indices(n, k=1)
    Oi, Oj, Di, Dj = origins[ii], origins[jj], directions[ii], directions[jj]
    b = Oj - Oi
    det = Di[:, 0] * (-Dj[:, 1]) - (-Dj[:, 0]) * Di[:, 1]
    ok = det != 0
    Oi, Oj, Di, Dj, b, det = Oi[ok], Oj[ok], Di[ok], Dj[ok], b[ok], det[ok]
    s = (b[:, 0] * (-Dj[:, 1]) - (-Dj[:, 0]) * b[:, 1]) / det
    t = (Di[:, 0] * b[:, 1] - Di[:, 1] * b[:, 0]) / det
    Pi = Oi + s[:, None] * Di
    Pj = Oj + t[:, None] * Dj
    return (Pi + Pj) / 2
