"""Host-side mirror of the reference's `evolve` / `evolve_data` modules for a Python host.

The reference's drop-in boundary is a set of Fortran modules with fixed public names
(SURVEY.md section 8b); fortran/ holds those modules for a Fortran host.  This file offers the
same call surface to Python (tests, bench.py): the same names, argument meaning and state
ownership -- the *host* owns ndens, xh, xhe, temperature_grid, srcpos, NormFlux; `Evolve` owns the
work arrays (phih_grid, xh_av, ...) which live on the GPU and are downloaded on request.

    material / grid / sourceprops state  ->  Evolve.evolve3D(time, dt, restart)
                                             (files_for_3D/evolve.F90:78-229)

All numerical work happens in libc2ray_hip.so (HIP, gfx950).  There is no CPU fallback here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from . import _lib
from ._lib import C2RayHipError, NFREQ

PKG = Path(__file__).resolve().parent
DEFAULT_TABLES = PKG / "data" / "rad_tables_bb5e4.npz"

FVEC_ORDER = ["f1ion_HI", "f1ion_HeI", "f1ion_HeII", "f2ion_HI", "f2ion_HeI", "f2ion_HeII",
              "f1heat_HI", "f1heat_HeI", "f1heat_HeII", "f2heat_HI", "f2heat_HeI", "f2heat_HeII"]

convergence_fraction = float(np.float32(2.5e-4))  # c2ray_parameters.f90:26 (REAL(4) literal)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


@dataclass
class RadiationTables:
    """What rad_ini (radiation_tables.f90:141-168) and setup_cool (cooling_h.f90:76-171) leave
    behind: inputs of the hot path, built once on the host."""
    photo_thick: np.ndarray
    photo_thin: np.ndarray
    heat_thick: np.ndarray | None
    heat_thin: np.ndarray | None
    sigma_HI: np.ndarray
    sigma_HeI: np.ndarray
    sigma_HeII: np.ndarray
    fvec: dict
    bb_upper: int
    cool: np.ndarray | None = None
    cool_mintemp: float = 1.0
    cool_dtemp: float = 0.01
    # -DPL / -DQUASARS builds: sed[1] (power law) / sed[2] (quasar-like) =
    # dict(photo_thick, photo_thin, heat_thick, heat_thin, lower, upper)
    sed: dict = field(default_factory=dict)
    # What spec_integration starts from (band set-up, Romberg weights, normalised SEDs; keys as in
    # tests/golden/sed_setup.npz).  With build_on_device the tables above are ignored and the engine
    # builds them on the GPU (c2r_build_tables) -- bit-identical to the host-built ones.
    setup: dict | None = None
    build_on_device: bool = False

    def add_sed_file(self, path):
        """pl_* / qpl_* tables and band limits as dumped from a -DPL -DQUASARS reference build."""
        with np.load(path) as z:
            for idx, pre in ((1, "pl_"), (2, "qpl_")):
                if pre + "photo_thick" in z.files:
                    self.sed[idx] = dict(photo_thick=_f64(z[pre + "photo_thick"]), photo_thin=_f64(z[pre + "photo_thin"]),
                                         heat_thick=_f64(z[pre + "heat_thick"]) if pre + "heat_thick" in z.files else None,
                                         heat_thin=_f64(z[pre + "heat_thin"]) if pre + "heat_thin" in z.files else None,
                                         lower=int(z[pre + "limits"][0]), upper=int(z[pre + "limits"][1]))
        return self

    @classmethod
    def load(cls, path=DEFAULT_TABLES):
        with np.load(path) as z:
            g = lambda k: _f64(z[k]) if k in z.files else None
            return cls(g("photo_thick"), g("photo_thin"), g("heat_thick"), g("heat_thin"), g("sigma_HI"),
                       g("sigma_HeI"), g("sigma_HeII"), {k: g(k) for k in FVEC_ORDER if k in z.files},
                       int(z["bb_upper"]), g("cool"),
                       float(z["cool_mintemp"]) if "cool_mintemp" in z.files else 1.0,
                       float(z["cool_dtemp"]) if "cool_dtemp" in z.files else 0.01)


@dataclass
class Material:
    """module material (files_for_3D/mat_ini_test.F90:27-36): host-owned state arrays, Fortran
    layout flattened (i fastest, component slowest)."""
    ndens: np.ndarray            # (N^3,) float64
    xh: np.ndarray               # (2*N^3,) float64, components 0:1
    xhe: np.ndarray              # (3*N^3,) float64, components 0:2
    temperature_grid: np.ndarray | None = None  # (3*N^3,) float32, slots 0:2; None when isothermal
    isothermal: bool = True
    temper_val: float = 1.0e4
    clumping: float = 1.0
    reccoef: np.ndarray = field(default_factory=lambda: np.zeros(12))  # cgsconstants.f90:106-133
    # type_of_clumping = 5: REAL(4) clumping_grid(mesh) read per cell (mat_ini_cubep3m.F90:635-646)
    clumping_grid: np.ndarray | None = None
    # use_LLS (c2ray_parameters.f90:72-78): coldensh_LLS of type 1, or the REAL(4) LLS_grid of type 2
    use_LLS: bool = False
    coldensh_LLS: float = 0.0
    LLS_grid: np.ndarray | None = None


@dataclass
class GridProps:
    """module grid (files_for_3D/grid.F90): cell sizes and volume (proper cm, cm^3)."""
    mesh: tuple
    dr: tuple
    vol: float


@dataclass
class SourceProps:
    """module sourceprops (files_for_3D/sourceprops_test.F90:38-40)."""
    srcpos: np.ndarray           # (NumSrc, 3) int32, 1-based mesh coordinates
    NormFlux: np.ndarray         # (NumSrc,) photons/s divided by S_star
    S_star: float = 1.0e48
    NormFluxPL: np.ndarray | None = None    # -DPL builds
    pl_S_star: float = 1.0e48
    NormFluxQPL: np.ndarray | None = None   # -DQUASARS builds
    qpl_S_star: float = 1.0e48

    @property
    def NumSrc(self):
        return int(len(self.NormFlux))


@dataclass
class Cosmology:
    zred: float = 0.0
    H0: float = 0.0
    Omega0: float = 0.0


class HipEngine:
    """Thin object wrapper over the C ABI.  `device`: one GPU, or a list of GPUs driven by this process
    (c2r_create_multi: every state-setting call goes to all of them, results are read from the first)."""

    def __init__(self, mesh, device=0):
        self.lib = _lib.load()
        self.mesh = tuple(int(m) for m in mesh)
        self.ncell = int(np.prod(self.mesh))
        h = C.c_void_p()
        m = (C.c_int * 3)(*self.mesh)
        if isinstance(device, (list, tuple)):
            devs = (C.c_int * len(device))(*[int(d) for d in device])
            rc = self.lib.c2r_create_multi(C.byref(h), len(device), devs, m)
        else:
            rc = self.lib.c2r_create(C.byref(h), int(device), m)
        if rc != 0:
            raise C2RayHipError(self.lib.c2r_create_error().decode())
        self.h = h
        self._ext_rates = None

    # -- several GPUs: the sum over ranks behind the C ABI (RCCL) ----------------------------------------
    @staticmethod
    def comm_unique_id():
        """128 bytes from ncclGetUniqueId, for ONE rank to obtain and the launcher to pass to the others."""
        lib = _lib.load()
        buf = C.create_string_buffer(128)
        if lib.c2r_comm_unique_id(buf) != 0:
            raise C2RayHipError(lib.c2r_create_error().decode())
        return buf.raw

    @staticmethod
    def comm_available():
        """None when RCCL can be loaded and used by this library, else the reason (a string)."""
        lib = _lib.load()
        return None if lib.c2r_comm_available() == 0 else lib.c2r_create_error().decode()

    @staticmethod
    def comm_library():
        """Path of the library that carries the sums over ranks (c2r_comm_library); raises when none can be loaded."""
        lib = _lib.load()
        buf = C.create_string_buffer(1024)
        if lib.c2r_comm_library(buf, 1024) != 0:
            raise C2RayHipError(lib.c2r_create_error().decode())
        return buf.value.decode()

    def comm_destroy(self):
        self._chk(self.lib.c2r_comm_destroy(self.h))

    def comm_init(self, first_rank, nranks, unique_id):
        assert len(unique_id) == 128
        self._chk(self.lib.c2r_comm_init(self.h, int(first_rank), int(nranks), unique_id))

    def comm_init_local(self):
        self._chk(self.lib.c2r_comm_init_local(self.h))

    def comm_size(self):
        return int(self.lib.c2r_comm_nranks(self.h))

    def rccl_ranks(self):
        """Ranks of the RCCL communicator that sums the rate grids (0: no communicator, or the in-process sum of
        replicas that share a device)."""
        return self.comm_size() if int(self.lib.c2r_comm_kind(self.h)) == 1 else 0

    def num_devices(self):
        return int(self.lib.c2r_num_devices(self.h))

    def allreduce_rates(self):
        self._chk(self.lib.c2r_allreduce_rates(self.h))

    def comm_selftest(self, nslab=4):
        """c2r_comm_selftest: a known pattern summed over the ranks through the context's own buffer, communicators and
        streams, over both routes a run takes (collective: every rank calls it).  Returns the report as a dict; raises
        C2RayHipError, with the report attached as `.report`, when a sum came back wrong or the transport failed."""
        rep = _lib.CommSelftestReport()
        rc = self.lib.c2r_comm_selftest(self.h, int(nslab), C.byref(rep))
        out = {k: getattr(rep, k) for k in ("ranks", "kind", "devices", "bad_route", "bad_rank", "bad_index", "got", "expected")}
        for k in ("elements", "mismatches", "ms"):
            out[k] = list(getattr(rep, k))
        if rc != 0:
            err = C2RayHipError(self.lib.c2r_last_error(self.h).decode())
            err.report = out
            raise err
        return out

    def comm_timing(self, idev=None):
        """c2r_get_comm_timing of device idev (None: the first) as a dict: the sum over ranks of the last fused iteration."""
        t = _lib.CommTiming()
        self._chk(self.lib.c2r_get_comm_timing(self.h, 0 if idev is None else int(idev), C.byref(t)))
        return {k: getattr(t, k) for k in ("slabs", "allreduce_ms", "allreduce_exposed_ms", "tail_ms")}

    def pass_allreduce_chemistry(self, dt, first=1, stride=1, nslab=4):
        """pass_all_sources + sum over ranks + global pass of one outer iteration, overlapped slab by slab;
        returns the non-converged count."""
        cf = C.c_int(0)
        self._chk(self.lib.c2r_pass_allreduce_chemistry(self.h, int(first), int(stride), int(nslab), float(dt), C.byref(cf)))
        return cf.value

    def iteration(self, dt, first=1, stride=1, nslab=4):
        """c2r_iteration: one outer iteration (pass, sum over ranks, global pass) and every grid reduction the reference's
        loop reports after it, with one synchronisation; returns the report as a dict of numpy arrays / ints."""
        rep = _lib.IterationReport()
        self._chk(self.lib.c2r_iteration(self.h, int(first), int(stride), int(nslab), float(dt), C.byref(rep)))
        out = {"conv_flag": rep.conv_flag, "sum_nbox": rep.sum_nbox}
        for k in ("photon_loss", "means_intermed", "sums_intermed", "total_rates", "minima_av", "reccoef"):
            out[k] = np.array(getattr(rep, k)[:])
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.c2r_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise C2RayHipError(self.lib.c2r_last_error(self.h).decode())

    # -- inputs ------------------------------------------------------------------------------
    def set_tables(self, t: RadiationTables):
        fv = None
        if t.fvec and len(t.fvec) == 12:
            arr = (C.POINTER(C.c_double) * 12)(*[_dp(t.fvec[k]) for k in FVEC_ORDER])
            fv = arr
        on_dev = bool(t.build_on_device)
        if on_dev and t.setup is None:
            raise C2RayHipError("build_on_device needs RadiationTables.setup")
        heat = t.heat_thick is not None or (on_dev and fv is not None)
        self._chk(self.lib.c2r_set_tables(self.h, None if on_dev else _dp(t.photo_thick), None if on_dev else _dp(t.photo_thin),
                                          None if on_dev else _dp(t.heat_thick), None if on_dev else _dp(t.heat_thin),
                                          _dp(t.sigma_HI), _dp(t.sigma_HeI), _dp(t.sigma_HeII), fv, int(t.bb_upper)))
        if on_dev:
            self.build_tables(t.setup, 0, heat)
        if t.cool is not None:
            self._chk(self.lib.c2r_set_cooling(self.h, _dp(t.cool), float(t.cool_mintemp), float(t.cool_dtemp)))
        for idx, d in t.sed.items():
            if on_dev:
                self._chk(self.lib.c2r_set_sed_tables(self.h, int(idx), None, None, None, None, d["lower"], d["upper"]))
                self.build_tables(t.setup, int(idx), heat)
            else:
                self._chk(self.lib.c2r_set_sed_tables(self.h, int(idx), _dp(d["photo_thick"]), _dp(d["photo_thin"]),
                                                      _dp(d["heat_thick"]), _dp(d["heat_thin"]), d["lower"], d["upper"]))

    def build_tables(self, d, sed=0, heat=True):
        """spec_integration on the device (c2r_build_tables) from a set-up dictionary."""
        from ._lib import SedSetup
        b = np.arange(1, 48)
        xi = _f64(np.where(b <= 1, d["pl_index_HI"], np.where(b <= 27, d["pl_index_HeI"], d["pl_index_HeII"])))
        keep = [_f64(d[k]) for k in ("freq_min", "delta_freq", "tau", "romw9")] + [xi]
        s = SedSetup()
        s.nfreq, s.sed = 512, int(sed)
        s.freq_min, s.delta_freq, s.tau, s.romw, s.xsec_index = (_dp(a) for a in keep)
        s.R_star2, s.h_over_kT, s.two_pi_over_c_square = (float(x) for x in d["sed_setup"])
        c = d["consts"]
        s.pi, s.hplanck = float(c[0]), float(c[5])
        s.ion_freq_HI, s.ion_freq_HeI, s.ion_freq_HeII = float(c[22]), float(c[23]), float(c[24])
        if sed:
            s.pl_scaling, s.pl_index = (float(x) for x in d["pl_setup" if sed == 1 else "qpl_setup"])
        self._chk(self.lib.c2r_build_tables(self.h, C.byref(s), int(bool(heat))))

    def download_tables(self, sed=0, heat=True):
        nt = 2001
        out = {"photo_thick": np.empty(47 * nt), "photo_thin": np.empty(47 * nt)}
        if heat:
            out.update(heat_thick=np.empty(113 * nt), heat_thin=np.empty(113 * nt))
        self._chk(self.lib.c2r_download_tables(self.h, int(sed), _dp(out["photo_thick"]), _dp(out["photo_thin"]),
                                               _dp(out.get("heat_thick")), _dp(out.get("heat_thin"))))
        return out

    def set_step(self, mat: Material, grid: GridProps, cosmo: Cosmology):
        nd = _f64(mat.ndens).reshape(-1)
        assert nd.size == self.ncell, "ndens has the wrong size"
        dr = (C.c_double * 3)(*[float(x) for x in grid.dr])
        rc = _f64(mat.reccoef).reshape(-1)
        assert rc.size == 12
        self.isothermal = bool(mat.isothermal)
        self._chk(self.lib.c2r_set_step(self.h, _dp(nd), dr, float(grid.vol), float(mat.clumping), float(cosmo.zred),
                                        float(cosmo.H0), float(cosmo.Omega0), int(bool(mat.isothermal)),
                                        float(mat.temper_val), _dp(rc)))
        self.set_lls(mat)
        self.set_clumping_grid(mat)

    def set_lls(self, mat: Material):
        """c2r_set_lls from mat.use_LLS, coldensh_LLS and LLS_grid: in force until the next call (set_step makes it)."""
        lls = None if mat.LLS_grid is None else np.ascontiguousarray(mat.LLS_grid, dtype=np.float32).reshape(-1)
        assert lls is None or lls.size == self.ncell
        self._chk(self.lib.c2r_set_lls(self.h, int(bool(mat.use_LLS)), float(mat.coldensh_LLS),
                                       None if lls is None else lls.ctypes.data_as(C.POINTER(C.c_float))))

    def set_clumping_grid(self, mat: Material):
        """c2r_set_clumping_grid from mat.clumping_grid (None: the scalar clumping again); set_step makes the call too."""
        cg = None if mat.clumping_grid is None else np.ascontiguousarray(mat.clumping_grid, dtype=np.float32).reshape(-1)
        assert cg is None or cg.size == self.ncell
        self._chk(self.lib.c2r_set_clumping_grid(self.h, None if cg is None else cg.ctypes.data_as(C.POINTER(C.c_float))))

    def set_step_scalars(self, mat: Material, grid: GridProps, cosmo: Cosmology):
        """c2r_set_step without the density: what is on the device stays (see scale_ndens)."""
        dr = (C.c_double * 3)(*[float(x) for x in grid.dr])
        rc = _f64(mat.reccoef).reshape(-1)
        self.isothermal = bool(mat.isothermal)
        self._chk(self.lib.c2r_set_step_scalars(self.h, dr, float(grid.vol), float(mat.clumping), float(cosmo.zred), float(cosmo.H0),
                                                float(cosmo.Omega0), int(bool(mat.isothermal)), float(mat.temper_val), _dp(rc)))

    def arena_stats(self):
        """c2r_arena_stats as a dict (column scratch: segments allocated, of them inside a pass, ...)."""
        out = (C.c_longlong * 6)()
        self._chk(self.lib.c2r_arena_stats(self.h, out))
        return dict(zip(("segments", "segments_in_pass", "doubles_allocated", "block_moves", "batch_restarts", "doubles_held"), out))

    def source_trace(self, ns):
        """c2r_get_source_trace for source `ns` (1-based) as a dict: reach, rounds, final sub-box, the column block's shells
        and entries, cells traced and threads the shell launches spent on it in the last pass that swept it."""
        t = _lib.SourceTrace()
        self._chk(self.lib.c2r_get_source_trace(self.h, int(ns), C.byref(t)))
        out = {k: list(getattr(t, k)) for k in ("reach_l", "reach_r", "box_lo", "box_hi")}
        out.update({k: int(getattr(t, k)) for k in ("nbox", "block_shells", "block_cells", "swept_cells", "sweep_threads")})
        return out

    def scale_ndens(self, divisor):
        """cosmo_evol's ndens = ndens / zfactor3 on the device copy (cosmology.f90:193)."""
        self._chk(self.lib.c2r_scale_ndens(self.h, float(divisor)))

    def set_sources(self, src: SourceProps, external=False):
        pos = np.ascontiguousarray(src.srcpos, dtype=np.int32).reshape(-1)
        nf = _f64(src.NormFlux).reshape(-1)
        assert pos.size == 3 * nf.size
        call = self.lib.c2r_set_sources_external if external else self.lib.c2r_set_sources
        self._chk(call(self.h, int(nf.size), pos.ctypes.data_as(C.POINTER(C.c_int)), _dp(nf), float(src.S_star)))
        self.nsrc = int(nf.size)
        for idx, flux, star in ((1, src.NormFluxPL, src.pl_S_star), (2, src.NormFluxQPL, src.qpl_S_star)):
            if flux is not None:
                f = _f64(flux).reshape(-1)
                assert f.size == nf.size
                self._chk(self.lib.c2r_set_sources_sed(self.h, idx, _dp(f), float(star)))

    def set_sources_external(self, src: SourceProps):
        """c2r_set_sources_external: set_sources for a list in which a source may stand outside the mesh (a position < 1 or
        > mesh) along axes that are open (set_boundaries); its box runs through vacuum up to the mesh."""
        self.set_sources(src, external=True)

    # -- point-source hand-over between meshes stacked along an open axis (include/c2ray_hip.h) ------------------------------
    def _source_face_cells(self, face):
        if not 0 <= int(face) <= 5:
            raise C2RayHipError(f"face {face} not in 0..5")
        return self.ncell // self.mesh[int(face) >> 1]

    def select_source_face_exit(self, face, sources=()):
        """c2r_select_source_face_exit: keep, in every pass that sweeps them, the exit strips through `face` (2 * axis + high)
        of the point sources `sources` (1-based); none frees the face's strips.  set_sources drops the selection."""
        s = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        self._chk(self.lib.c2r_select_source_face_exit(self.h, int(face), int(s.size), s.ctypes.data_as(C.POINTER(C.c_int))))

    def download_source_face_exit(self, face, ns):
        """c2r_download_source_face_exit: (strip, rounds, reached) of source ns from the last pass that swept it -- N_out of the
        cells in the layer of `face` as (3, face cells), species slowest, the lower of the two other axes fastest, +0.0 outside the
        final box; nbox of that pass; whether the final box held a cell of the layer."""
        out = np.empty((3, self._source_face_cells(face)))
        rounds, reached = C.c_int(0), C.c_int(0)
        self._chk(self.lib.c2r_download_source_face_exit(self.h, int(face), int(ns), _dp(out), C.byref(rounds), C.byref(reached)))
        return out, rounds.value, bool(reached.value)

    def set_source_face_entry(self, ns, face=0, cols3=None, rounds=0):
        """c2r_set_source_face_entry: source ns (1-based), which stands outside the mesh beyond `face` only, sees the columns
        cols3 -- the exit strip of the mesh next door -- in the ghost layer of that face and is traced for exactly `rounds`
        rounds.  cols3 = None clears the entry.  set_sources clears every entry."""
        a = None
        if cols3 is not None:
            a = _f64(cols3).reshape(-1)
            if a.size != 3 * self._source_face_cells(face):
                raise ValueError(f"set_source_face_entry: {a.size} values, expected 3 x {self._source_face_cells(face)}")
        self._chk(self.lib.c2r_set_source_face_entry(self.h, int(ns), int(face), _dp(a), int(rounds)))

    def set_mesh_origin(self, origin=(0, 0, 0)):
        """c2r_set_mesh_origin: this mesh is a part of a deep mesh, whose index along each axis is this mesh's index + origin.
        cinterp then forms its crossing points from the deep mesh's coordinates, and the part has the deep mesh's bits wherever
        it lies.  Non-zero along open axes only; kept across source lists."""
        o = (C.c_int * 3)(*[int(v) for v in origin])
        self._chk(self.lib.c2r_set_mesh_origin(self.h, o))

    @property
    def mesh_origin(self):
        o = (C.c_int * 3)()
        self._chk(self.lib.c2r_get_mesh_origin(self.h, o))
        return tuple(int(v) for v in o)

    def source_face_entry(self, ns):
        """c2r_get_source_face_entry: (face, rounds) of source ns; face = -1 while no entry is set."""
        face, rounds = C.c_int(0), C.c_int(0)
        self._chk(self.lib.c2r_get_source_face_entry(self.h, int(ns), C.byref(face), C.byref(rounds)))
        return face.value, rounds.value

    def set_source_halo(self, ns, faces=None, edges=None, corner=None, rounds=0):
        """c2r_set_source_halo: the entry of source ns (1-based) where it stands beyond one, two or three faces.  faces: {face:
        strip} with face = 2 * axis + high and the strip as for set_source_face_entry; edges: {axis: line} with the line along
        that axis as (3, mesh[axis]), species slowest; corner: 3 values; the source is traced for exactly `rounds` rounds.
        faces=None clears the halo (or the entry).  handover.edge_of_strip / corner_of_strip cut the lines and the corner out of
        a neighbour's exit strip.  set_sources clears every halo."""
        if faces is None:
            self._chk(self.lib.c2r_set_source_halo(self.h, int(ns), None))
            return
        rec, keep = _lib.SourceHalo(), []
        rec.rounds = int(rounds)

        def pointer(values, count, what):
            a = _f64(values).reshape(-1)
            if a.size != 3 * count:
                raise ValueError(f"set_source_halo: {what}: {a.size} values, expected 3 x {count}")
            keep.append(a)
            return _dp(a)

        for face, strip in dict(faces).items():
            cells = self._source_face_cells(face)
            if rec.face[int(face) >> 1]:
                raise ValueError(f"set_source_halo: two faces of axis {int(face) >> 1}")
            rec.face[int(face) >> 1] = pointer(strip, cells, f"face {face}")
        for axis, line in dict(edges or {}).items():
            if not 0 <= int(axis) <= 2:
                raise C2RayHipError(f"axis {axis} not in 0..2")
            rec.edge[int(axis)] = pointer(line, self.mesh[int(axis)], f"edge {axis}")
        if corner is not None:
            rec.corner = pointer(corner, 1, "corner")
        self._chk(self.lib.c2r_set_source_halo(self.h, int(ns), C.byref(rec)))

    def source_halo(self, ns):
        """c2r_get_source_halo: (faces, rounds) of source ns -- the face numbers its halo has strips for, ascending; () and 0
        while none is set."""
        faces, rounds = (C.c_int * 3)(), C.c_int(0)
        self._chk(self.lib.c2r_get_source_halo(self.h, int(ns), faces, C.byref(rounds)))
        return tuple(int(f) for f in faces if f >= 0), rounds.value

    def set_source_beams(self, beams=None):
        """c2r_set_source_beams: one beam per point source, in source order -- None (no beam), a dict or a tuple
        (kind, axis, cos_half) with kind 0 / "none", 1 / "cone" or 2 / "bicone", axis three numbers (any length), cos_half the
        cosine of the half opening angle.  beams=None: no source is beamed.  set_sources clears the beams."""
        if beams is None:
            self._chk(self.lib.c2r_set_source_beams(self.h, int(self.nsrc), None))
            return
        kinds = {"none": 0, "cone": 1, "bicone": 2}
        beams = list(beams)
        arr = (_lib.SourceBeam * max(len(beams), 1))()
        for rec, b in zip(arr, beams):
            if b is None:
                continue
            kind, axis, cos_half = (b["kind"], b["axis"], b["cos_half"]) if isinstance(b, dict) else b
            rec.kind = kinds[kind] if isinstance(kind, str) else int(kind)
            rec.axis[:] = [float(a) for a in axis]
            rec.cos_half = float(cos_half)
        self._chk(self.lib.c2r_set_source_beams(self.h, len(beams), arr))

    def source_beam(self, ns):
        """c2r_get_source_beam for source `ns` (1-based) as a dict: kind (0 none, 1 cone, 2 bicone), axis, cos_half."""
        b = _lib.SourceBeam()
        self._chk(self.lib.c2r_get_source_beam(self.h, int(ns), C.byref(b)))
        return {"kind": int(b.kind), "axis": [float(a) for a in b.axis], "cos_half": float(b.cos_half)}

    def set_source_horizons(self, radii=None):
        """c2r_set_source_horizons: one photon horizon per point source, in source order -- a maximum ray length in the length
        unit of dr (a physical length: a pass uses its own dr); None or inf: that source has none.  radii=None: no source has
        a horizon.  set_sources clears the horizons."""
        if radii is None:
            self._chk(self.lib.c2r_set_source_horizons(self.h, int(self.nsrc), None))
            return
        arr = np.array([np.inf if r is None else float(r) for r in radii], dtype=np.float64)
        self._chk(self.lib.c2r_set_source_horizons(self.h, int(arr.size), _dp(arr) if arr.size else None))

    def get_source_horizon(self, ns):
        """c2r_get_source_horizon for source `ns` (1-based): its radius, inf while it has none."""
        r = C.c_double(0.0)
        self._chk(self.lib.c2r_get_source_horizon(self.h, int(ns), C.byref(r)))
        return float(r.value)

    def set_source_curves(self, curves=None):
        """c2r_set_source_curves: one light curve per point source, in source order -- None (no curve) or (radii, factors):
        up to 8 radii, physical lengths in the length unit of dr, strictly ascending, and one factor more than radii, factors[b]
        the flux factor of distance shell b ([0, r0], (r0, r1], ..., beyond the last radius).  curves=None: no source has a
        curve.  set_sources clears the curves."""
        if curves is None:
            self._chk(self.lib.c2r_set_source_curves(self.h, int(self.nsrc), None))
            return
        curves = list(curves)
        arr = (_lib.SourceCurve * max(len(curves), 1))()
        for rec, c in zip(arr, curves):
            rec.factor[0] = 1.0
            if c is None:
                continue
            radii, factors = [float(r) for r in c[0]], [float(f) for f in c[1]]
            if len(factors) != len(radii) + 1:
                raise ValueError(f"a curve of {len(radii)} radii takes {len(radii) + 1} factors, not {len(factors)}")
            rec.nstep = len(radii)                 # (more than 8: the library refuses the call, the record holds the first 8)
            for k, r in enumerate(radii[:_lib.CURVE_MAX_STEPS]):
                rec.radius[k] = r
            for k, f in enumerate(factors[:_lib.CURVE_MAX_STEPS + 1]):
                rec.factor[k] = f
        self._chk(self.lib.c2r_set_source_curves(self.h, len(curves), arr))

    def source_curve(self, ns):
        """c2r_get_source_curve for source `ns` (1-based): (radii, factors) as it was set, ([], [1.0]) while it has none."""
        c = _lib.SourceCurve()
        self._chk(self.lib.c2r_get_source_curve(self.h, int(ns), C.byref(c)))
        n = int(c.nstep)
        return [float(c.radius[k]) for k in range(n)], [float(c.factor[k]) for k in range(n + 1)]

    def upload_state(self, mat: Material):
        xh, xhe = _f64(mat.xh).reshape(-1), _f64(mat.xhe).reshape(-1)
        assert xh.size == 2 * self.ncell and xhe.size == 3 * self.ncell
        tp = None
        if mat.temperature_grid is not None:
            t = np.ascontiguousarray(mat.temperature_grid, dtype=np.float32).reshape(-1)
            assert t.size == 3 * self.ncell
            tp = t.ctypes.data_as(C.POINTER(C.c_float))
        self._chk(self.lib.c2r_upload_state(self.h, _dp(xh), _dp(xhe), tp))

    def download_state(self, mat: Material):
        xh = np.empty(2 * self.ncell)
        xhe = np.empty(3 * self.ncell)
        t = None if mat.temperature_grid is None else np.empty(3 * self.ncell, dtype=np.float32)
        tp = None if t is None else t.ctypes.data_as(C.POINTER(C.c_float))
        self._chk(self.lib.c2r_download_state(self.h, _dp(xh), _dp(xhe), tp))
        mat.xh, mat.xhe = xh, xhe
        if t is not None:
            mat.temperature_grid = t

    # -- the pieces of evolve3D --------------------------------------------------------------
    def begin_step(self):
        self._chk(self.lib.c2r_begin_step(self.h))

    def set_rates_to_zero(self):
        self._chk(self.lib.c2r_set_rates_to_zero(self.h))

    def pass_sources(self, first=1, stride=1):
        self._chk(self.lib.c2r_pass_sources(self.h, int(first), int(stride)))

    def pass_sources_begin(self, first=1, stride=1, nslab=8):
        """Queue the pass and return at once; returns the number of slabs to wait for."""
        self._chk(self.lib.c2r_pass_sources_begin(self.h, int(first), int(stride), int(nslab)))
        return int(self.lib.c2r_pass_slab_count(self.h))

    def pass_wait_slab(self, slab):
        """Block until the rate grids of this slab are final; (first_cell, ncells) of every component."""
        a, b = C.c_size_t(0), C.c_size_t(0)
        self._chk(self.lib.c2r_pass_wait_slab(self.h, int(slab), C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def pass_sources_end(self):
        self._chk(self.lib.c2r_pass_sources_end(self.h))

    def do_source(self, ns):
        self._chk(self.lib.c2r_do_source(self.h, int(ns)))

    def global_pass(self, dt):
        cf = C.c_int(0)
        self._chk(self.lib.c2r_global_pass(self.h, float(dt), C.byref(cf)))
        return cf.value

    def global_pass_cells(self, dt, first_cell, ncells, after_event=None):
        """Queue the chemistry of a range of cells, after a hipEvent_t handle (int) of another stream."""
        self._chk(self.lib.c2r_global_pass_cells(self.h, float(dt), int(first_cell), int(ncells),
                                                 C.c_void_p(after_event) if after_event else None))

    def global_pass_finish(self):
        conv = C.c_int(0)
        self._chk(self.lib.c2r_global_pass_finish(self.h, C.byref(conv)))
        return int(conv.value)

    def end_step(self):
        self._chk(self.lib.c2r_end_step(self.h))

    def evolve3d(self, dt):
        n = C.c_int(0)
        flags = (C.c_int * 512)()
        self._chk(self.lib.c2r_evolve3d(self.h, float(dt), C.byref(n), flags, 512))
        return n.value, list(flags[: n.value])

    def synchronize(self):
        self._chk(self.lib.c2r_synchronize(self.h))

    def set_batch(self, n):
        self._chk(self.lib.c2r_set_batch(self.h, int(n)))

    def set_boundaries(self, periodic=True):
        """Mesh boundaries of the ray trace: periodic (the default, the reference's) or open -- nothing wraps, photons
        that reach a mesh face are lost (c2r_set_boundaries; include/c2ray_hip.h has the semantics).  A sequence of
        three gives the mode per axis (c2r_set_boundaries_axes): (True, True, False) is periodic in x and y and open in z."""
        if isinstance(periodic, (bool, int, np.bool_, np.integer)):
            self._chk(self.lib.c2r_set_boundaries(self.h, int(bool(periodic))))
            return
        axes = [int(bool(p)) for p in periodic]
        if len(axes) != 3:
            raise ValueError("set_boundaries: a bool or a sequence of three, one per axis")
        self._chk(self.lib.c2r_set_boundaries_axes(self.h, (C.c_int * 3)(*axes)))

    @property
    def periodic(self):
        """True: periodic on every axis, False: open on every axis, None: mixed (periodic_axes tells which)."""
        mode = self.lib.c2r_get_boundaries(self.h)
        return None if mode == 2 else bool(mode)

    @property
    def periodic_axes(self):
        out = (C.c_int * 3)()
        self._chk(self.lib.c2r_get_boundaries_axes(self.h, out))
        return tuple(bool(v) for v in out)

    # -- plane-parallel sources (c2r_set_plane_sources; include/c2ray_hip.h has the rule) ---------------------
    def set_plane_sources(self, planes):
        """Plane waves entering through open mesh faces.  `planes`: a list of (axis, from_high, normflux) or of dicts with
        those keys -- axis 0..2 (it must be open), from_high 0 / 1 (entering at index 1 / at index mesh[axis]), normflux a
        number (black body only) or three, one per SED, per cm^2 of face.  An empty list removes them.  Plane p (1-based)
        is source NumSrc + p of every deal."""
        items = []
        for pl in planes or ():
            axis, from_high, flux = (pl["axis"], pl["from_high"], pl["normflux"]) if isinstance(pl, dict) else pl
            flux = [float(x) for x in np.atleast_1d(np.asarray(flux, dtype=np.float64))]
            if len(flux) not in (1, 3):
                raise ValueError("set_plane_sources: normflux is one number or three (black body, power law, quasar-like)")
            items.append((int(axis), int(from_high), (flux + [0.0, 0.0])[:3]))
        arr = (_lib.PlaneSource * max(1, len(items)))()
        for a, (axis, from_high, flux) in zip(arr, items):
            a.axis, a.from_high = axis, from_high
            a.normflux[:] = flux
        self._chk(self.lib.c2r_set_plane_sources(self.h, len(items), arr if items else None))
        self._plane_axes = [axis for axis, _, _ in items]

    @property
    def plane_count(self):
        return int(self.lib.c2r_get_plane_count(self.h))

    def _face_cells(self, p):
        """Face cells of plane p (1-based): the product of the two extents across its axis."""
        axes = getattr(self, "_plane_axes", [])
        if not 1 <= int(p) <= len(axes):
            raise C2RayHipError(f"plane {p} not in [1,{len(axes)}]")
        return self.ncell // self.mesh[axes[int(p) - 1]]

    def set_plane_entry_columns(self, p, cols3=None):
        """Entry columns of plane p (1-based): 3 x face cells (HI, HeI, HeII; face cells in mesh order of the two remaining
        axes, the lower axis fastest), e.g. the plane_exit_columns of the slab upstream.  None: zero again."""
        a = None
        if cols3 is not None:
            a = _f64(cols3).reshape(-1)
            if a.size != 3 * self._face_cells(p):
                raise ValueError(f"set_plane_entry_columns: {a.size} values, expected 3 x {self._face_cells(p)}")
        self._chk(self.lib.c2r_set_plane_entry_columns(self.h, int(p), _dp(a)))

    def plane_exit_columns(self, p):
        """Outgoing columns of the last cell of every column of plane p, from the last pass that ran it (3 x face cells)."""
        out = np.empty(3 * self._face_cells(p))
        self._chk(self.lib.c2r_download_plane_exit_columns(self.h, int(p), _dp(out)))
        return out

    def plane_loss(self, p):
        """What plane p added to photon_loss(1) in the last pass that ran it."""
        loss = C.c_double(0.0)
        self._chk(self.lib.c2r_get_plane_loss(self.h, int(p), C.byref(loss)))
        return loss.value

    def set_plane_flux_map(self, p, flux3=None):
        """Flux map of plane p (1-based): 3 x face cells (black body, power law, quasar-like; the face cells in the order of
        the entry columns), NormFlux per cm^2 at every face cell.  While set it replaces the plane's normflux.  None: the
        uniform normflux again.  set_plane_sources drops every map."""
        a = None
        if flux3 is not None:
            a = _f64(flux3).reshape(-1)
            if a.size != 3 * self._face_cells(p):
                raise ValueError(f"set_plane_flux_map: {a.size} values, expected 3 x {self._face_cells(p)}")
        self._chk(self.lib.c2r_set_plane_flux_map(self.h, int(p), _dp(a)))

    def plane_flux_map_set(self, p):
        """True while plane p (1-based) has a flux map."""
        return bool(self.lib.c2r_get_plane_flux_map_set(self.h, int(p)))

    def plane_exit_flux(self, p):
        """The flux the cells of the last layer of plane p saw in the last pass that ran it with a map (3 x face cells): the
        flux map of the next slab downstream."""
        out = np.empty(3 * self._face_cells(p))
        self._chk(self.lib.c2r_download_plane_exit_flux(self.h, int(p), _dp(out)))
        return out

    def set_plane_curve(self, p, curve=None):
        """c2r_set_plane_curve: the light curve of plane p (1-based) -- None (no curve) or (depths, factors, layer0=0,
        depth0=0.0): up to 8 depths along the beam, lengths in the length unit of dr, strictly ascending, and one factor more
        than depths, factors[b] the flux factor of depth shell b ([0, d0], (d0, d1], ..., beyond the last depth); layer0 layers
        of the plane's path and the length depth0 lie in front of this mesh.  set_plane_sources drops every curve."""
        if curve is None:
            self._chk(self.lib.c2r_set_plane_curve(self.h, int(p), None))
            return
        depths, factors = [float(d) for d in curve[0]], [float(f) for f in curve[1]]
        if len(factors) != len(depths) + 1:
            raise ValueError(f"a curve of {len(depths)} depths takes {len(depths) + 1} factors, not {len(factors)}")
        rec = _lib.PlaneCurve()
        rec.nstep = len(depths)                    # (more than 8: the library refuses the call, the record holds the first 8)
        rec.layer0 = int(curve[2]) if len(curve) > 2 else 0
        rec.depth0 = float(curve[3]) if len(curve) > 3 else 0.0
        for k, d in enumerate(depths[:_lib.PLANE_CURVE_MAX_STEPS]):
            rec.depth[k] = d
        for k, f in enumerate(factors[:_lib.PLANE_CURVE_MAX_STEPS + 1]):
            rec.factor[k] = f
        self._chk(self.lib.c2r_set_plane_curve(self.h, int(p), C.byref(rec)))

    def plane_curve(self, p):
        """c2r_get_plane_curve for plane p (1-based): (depths, factors, layer0, depth0) as it was set, ([], [1.0], 0, 0.0) while
        it has none."""
        c = _lib.PlaneCurve()
        self._chk(self.lib.c2r_get_plane_curve(self.h, int(p), C.byref(c)))
        n = int(c.nstep)
        return [float(c.depth[k]) for k in range(n)], [float(c.factor[k]) for k in range(n + 1)], int(c.layer0), float(c.depth0)

    def set_plane_tilt(self, p, tilt=None):
        """Oblique incidence of plane p (1-based): `tilt` = the tangents of the beam's inclination towards the two face axes
        (the lower axis first), in physical lengths.  None or (0, 0): normal incidence again.  set_plane_sources resets
        every tilt to (0, 0)."""
        a = None if tilt is None else (C.c_double * 2)(float(tilt[0]), float(tilt[1]))
        self._chk(self.lib.c2r_set_plane_tilt(self.h, int(p), a))

    def plane_tilt(self, p):
        """The tilt of plane p (1-based) as set_plane_tilt took it."""
        self._face_cells(p)
        out = (C.c_double * 2)()
        self._chk(self.lib.c2r_get_plane_tilt(self.h, int(p), out))
        return (out[0], out[1])

    # -- side faces of a tilted plane (c2r_set_plane_side_entry ..; include/c2ray_hip.h has the rule) ----------
    def plane_strip_shape(self, p, side):
        """(na, 3, L) of a strip of plane p (1-based): na slots of 3 x L values; L = the extent of the other face axis for side
        0 and 1, 1 for the corner line (side 2).  None for a plane or side the library will refuse."""
        axes = getattr(self, "_plane_axes", [])
        if not 1 <= int(p) <= len(axes) or int(side) not in (0, 1, 2):
            return None
        axis = axes[int(p) - 1]
        f, g = [d for d in range(3) if d != axis]
        return (self.mesh[axis], 3, (self.mesh[g], self.mesh[f], 1)[int(side)])

    def set_plane_side_entry(self, p, side, cols=None, flux=None):
        """Side entry of plane p (1-based): the ghost cells a neighbouring mesh hands in through side 0 (face axis f), side 1
        (face axis g) or the corner line (side 2).  cols, flux: (na, 3, L) -- slot m holds the layer before layer m, species
        or SED next, the index along the other face axis fastest -- e.g. the neighbour's plane_side_exit.  cols None: the side
        reads 0.0 again; flux None: a ghost flux of 0.  set_plane_sources drops every strip."""
        shape = self.plane_strip_shape(p, side)
        arrs = []
        for name, a in (("cols", cols), ("flux", flux)):
            if a is not None:
                a = _f64(a).reshape(-1)
                if shape is not None and a.size != int(np.prod(shape)):
                    raise ValueError(f"set_plane_side_entry: {name} has {a.size} values, expected {shape}")
            arrs.append(a)
        self._chk(self.lib.c2r_set_plane_side_entry(self.h, int(p), int(side), _dp(arrs[0]), _dp(arrs[1])))

    def enable_plane_side_exit(self, p, on=True):
        """Keep what the downstream edge cells of plane p's live sides hand on, layer by layer (plane_side_exit)."""
        self._chk(self.lib.c2r_enable_plane_side_exit(self.h, int(p), int(on)))

    def plane_side_exit(self, p, side, flux=True):
        """(cols, flux) of side 0 or 1 of plane p from the last pass that ran it, each (na, 3, L) in the layout of
        set_plane_side_entry; flux=False (a plane without a map): (cols, None)."""
        shape = self.plane_strip_shape(p, side) or (0, 3, 0)
        cols = np.empty(shape)
        fl = np.empty(shape) if flux else None
        self._chk(self.lib.c2r_download_plane_side_exit(self.h, int(p), int(side), _dp(cols), _dp(fl)))
        return cols, fl

    def enable_plane_side_loss(self, on=True):
        """Count what tilted planes lose through open side faces: in photon_loss(1), plane_side_loss and the escape maps."""
        self._chk(self.lib.c2r_enable_plane_side_loss(self.h, int(on)))

    @property
    def plane_side_loss_enabled(self):
        return bool(self.lib.c2r_get_plane_side_loss_enabled(self.h))

    def plane_side_loss(self, p):
        """(side 0, side 1): what plane p added to photon_loss(1) through its side faces in the last pass that ran it."""
        out = (C.c_double * 2)()
        self._chk(self.lib.c2r_get_plane_side_loss(self.h, int(p), out))
        return (out[0], out[1])

    # -- escape maps (c2r_enable_face_loss; include/c2ray_hip.h has the rule) ---------------------------------
    def enable_face_loss(self, on=True):
        """Keep the kept photon loss of open boxes per cell of the open mesh face it leaves through (off by default)."""
        self._chk(self.lib.c2r_enable_face_loss(self.h, int(on)))

    @property
    def face_loss_enabled(self):
        return bool(self.lib.c2r_get_face_loss_enabled(self.h))

    def face_loss_map(self, face):
        """The map of face 2 * axis + high (high = 0: the face at mesh index 1) since the last set_rates_to_zero, indexed
        [b, a] by the 0-based mesh indices along the two remaining axes, a the lower one (it runs fastest).  An error for a
        face of a periodic axis."""
        face = int(face)
        if not 0 <= face <= 5:
            raise C2RayHipError(f"face {face} not in [0,5]")
        a, b = [d for d in range(3) if d != face // 2]
        out = np.empty((self.mesh[b], self.mesh[a]))
        self._chk(self.lib.c2r_download_face_loss(self.h, face, _dp(out)))
        return out

    def face_loss(self):
        """The six faces' totals, each map added up in a fixed order; 0 for a face of a periodic axis."""
        out = np.zeros(6)
        self._chk(self.lib.c2r_get_face_loss(self.h, _dp(out)))
        return out

    # -- horizon loss (c2r_enable_horizon_loss; include/c2ray_hip.h has the rule) -------------------------------
    def enable_horizon_loss(self, on=True):
        """Keep, per point source, what crosses its photon horizon (off by default)."""
        self._chk(self.lib.c2r_enable_horizon_loss(self.h, int(on)))

    @property
    def horizon_loss_enabled(self):
        return bool(self.lib.c2r_get_horizon_loss_enabled(self.h))

    def horizon_loss(self):
        """(per_source, total) since the last set_rates_to_zero: one double per point source (0.0 without a finite horizon)
        and their sum in source order."""
        per = np.zeros(int(self.nsrc))
        tot = C.c_double(0.0)
        self._chk(self.lib.c2r_get_horizon_loss(self.h, int(self.nsrc), _dp(per) if per.size else None, C.byref(tot)))
        return per, tot.value

    def horizon_rim(self):
        """The diagnostic of c2r_download_horizon_rim: (ns, extent, terms) of the point source with a finite horizon that was
        swept last -- its 1-based number, the extents of its final box and the T = 2*(E1*E2 + E0*E2 + E0*E1) terms, the six
        sheets one behind the other."""
        ns, ext = C.c_int(0), (C.c_int * 3)()
        cap = 2 * (self.mesh[1] * self.mesh[2] + self.mesh[0] * self.mesh[2] + self.mesh[0] * self.mesh[1])
        out = np.zeros(cap)
        self._chk(self.lib.c2r_download_horizon_rim(self.h, C.byref(ns), ext, _dp(out), cap))
        e = [int(x) for x in ext]
        return ns.value, e, out[:2 * (e[1] * e[2] + e[0] * e[2] + e[0] * e[1])].copy()

    def enable_timing(self, on=True):
        self._chk(self.lib.c2r_enable_timing(self.h, int(on)))

    def timing(self, idev=None):
        t = _lib.Timing()
        if idev is None:
            self._chk(self.lib.c2r_get_timing(self.h, C.byref(t)))
        else:
            self._chk(self.lib.c2r_get_timing_device(self.h, int(idev), C.byref(t)))
        return t

    # -- outputs -----------------------------------------------------------------------------
    def download_rates(self):
        n = self.ncell
        phih, phihe, phiheat = np.empty(n), np.empty(2 * n), np.empty(n)
        loss = np.empty(NFREQ)
        nbox = C.c_int(0)
        self._chk(self.lib.c2r_download_rates(self.h, _dp(phih), _dp(phihe), _dp(phiheat), _dp(loss), C.byref(nbox)))
        return dict(phih_grid=phih, phihe_grid=phihe, phiheat=phiheat, photon_loss=loss, sum_nbox=nbox.value)

    def get_loss(self):
        """(photon_loss(1:47), sum_nbox) of this rank's last pass, without touching the grids."""
        loss = np.empty(47)
        nbox = C.c_int(0)
        self._chk(self.lib.c2r_get_loss(self.h, _dp(loss), C.byref(nbox)))
        return loss, int(nbox.value)

    def download_iter_state(self):
        n = self.ncell
        a, b, c, d = np.empty(2 * n), np.empty(3 * n), np.empty(2 * n), np.empty(3 * n)
        self._chk(self.lib.c2r_download_iter_state(self.h, _dp(a), _dp(b), _dp(c), _dp(d)))
        return dict(xh_av=a, xhe_av=b, xh_intermed=c, xhe_intermed=d)

    def upload_rates(self, phih=None, phihe=None, phiheat=None):
        a = [None if x is None else _f64(x).reshape(-1) for x in (phih, phihe, phiheat)]
        self._chk(self.lib.c2r_upload_rates(self.h, *[_dp(x) for x in a]))

    def upload_iter_state(self, xh_av=None, xhe_av=None, xh_intermed=None, xhe_intermed=None):
        a = [None if x is None else _f64(x).reshape(-1) for x in (xh_av, xhe_av, xh_intermed, xhe_intermed)]
        self._chk(self.lib.c2r_upload_iter_state(self.h, *[_dp(x) for x in a]))

    def download_columns(self):
        n = self.ncell
        a, b = np.empty(n), np.empty(2 * n)
        self._chk(self.lib.c2r_download_columns(self.h, _dp(a), _dp(b)))
        return dict(coldensh_out=a, coldenshe_out=b)

    # -- photon statistics (photonstatistics.f90) on the device -----------------------------------
    def state_sums(self, which=0):
        out = np.empty(5)
        self._chk(self.lib.c2r_state_sums(self.h, int(which), _dp(out)))
        return out

    def total_rates(self, dt, reccoef):
        out = np.empty(3)
        rc = _f64(reccoef).reshape(-1)
        self._chk(self.lib.c2r_total_rates(self.h, float(dt), _dp(rc), _dp(out)))
        return out

    def get_reccoef(self):
        out = np.empty(12)
        self._chk(self.lib.c2r_get_reccoef(self.h, _dp(out)))
        return out

    # -- reduction buffer ----------------------------------------------------------------------
    def rates_count(self):
        return int(self.lib.c2r_rates_count(self.h))

    def rates_buffer(self):
        if self._ext_rates is None:
            raise C2RayHipError("no shared reduction buffer: call use_torch_rates_buffer(device) first")
        return self._ext_rates

    def rates_reduced(self):
        return None

    def use_torch_rates_buffer(self, device):
        """Allocate the reduction buffer as a torch tensor so torch.distributed (RCCL) can
        all-reduce it in place; returns the tensor."""
        import torch
        t = torch.zeros(self.rates_count(), dtype=torch.float64, device=device)
        self._chk(self.lib.c2r_set_rates_buffer(self.h, C.c_void_p(t.data_ptr()), t.numel()))
        self._ext_rates = t
        return t


class Evolve:
    """module evolve + evolve_data: evolve_ini() == construction, evolve3D(time, dt, restart).

    comm: optional object with .rank, .size and .allreduce_sum_(buffer) (see parallel.py) -- the
    MPI analogue of the reference: sources are dealt round-robin over the ranks
    (do_grid_static, master_slave.F90:74-96: `do ns1 = 1+rank, NumSrc, npr`), the rate grids are
    summed over ranks (mpi_accumulate_grid_quantities, evolve.F90:505-548) and the global
    chemistry pass is replicated on every rank (evolve.F90:477-484).
    """

    def __init__(self, mesh, tables: RadiationTables | None = None, device=0, engine=None, comm=None, periodic=True):
        self.mesh = tuple(int(m) for m in mesh)
        self.engine = engine if engine is not None else HipEngine(self.mesh, device)
        if periodic is not True:    # open or per-axis mesh boundaries (HipEngine.set_boundaries); the default leaves the engine as it is
            self.engine.set_boundaries(periodic)
        self.tables = tables if tables is not None else RadiationTables.load()
        self.engine.set_tables(self.tables)
        self.comm = comm
        if comm is not None and comm.size > 1 and isinstance(self.engine, HipEngine):
            self.engine.use_torch_rates_buffer(f"cuda:{device}")
        self.niter = 0
        self.conv_flags: list[int] = []
        self.sum_nbox_all = 0
        self.photon_loss_all = np.zeros(NFREQ)
        self.iteration_dump: dict | None = None

    # subroutine evolve3D (time,dt,restart) -- evolve.F90:78
    def evolve3D(self, time, dt, restart, material: Material, grid: GridProps, sources: SourceProps,
                 cosmology: Cosmology | None = None, dump: dict | None = None, dump_at=None):
        """evolve3D(time,dt,restart) (evolve.F90:78-229).

        restart != 0 continues from an iteration dump (start_from_dump + global_pass, evolve.F90:138-140):
        `dump` is the dictionary an earlier call left in `self.iteration_dump`.  `dump_at` (an iterable of
        iteration numbers) stands for the reference's wall-clock trigger (a dump every 15 minutes, :196-210):
        after pass_all_sources of those iterations the dump content is taken off the device
        (write_iteration_dump, :233-275: niter, photon_loss_all, phih_grid, phihe_grid, [phiheat], xh_av, xhe_av,
        xh_intermed, xhe_intermed)."""
        cosmology = cosmology or Cosmology()
        e = self.engine
        e.set_step(material, grid, cosmology)
        e.set_sources(sources)
        if restart != 0 and dump is not None and dump.get("temperature") is not None and not material.isothermal:
            # not part of the reference's dump file: the temperature slots as the interrupted call left them, so
            # that a non-isothermal continuation is bit-identical (the reference restarts from the last output)
            material.temperature_grid = np.array(dump["temperature"], dtype=np.float32)
        e.upload_state(material)
        single = self.comm is None or self.comm.size == 1
        if restart == 0 and not dump_at and single:
            self.niter, self.conv_flags = e.evolve3d(dt)
        else:
            if restart != 0 and dump is None:
                raise C2RayHipError("evolve3D: restart /= 0 needs the iteration dump to start from")
            self._evolve3d_stepwise(dt, sources.NumSrc, dump if restart != 0 else None, set(dump_at or ()))
        e.download_state(material)
        r = e.download_rates()
        self.sum_nbox_all = r["sum_nbox"]
        self.photon_loss_all = r["photon_loss"]
        return self.niter

    def _evolve3d_stepwise(self, dt, numsrc, dump, dump_at):
        e = self.engine
        comm = self.comm if self.comm is not None and self.comm.size > 1 else None
        ncell = int(np.prod(self.mesh))
        self.conv_flags = []
        if dump is None:
            e.begin_step()
            niter, conv_flag = 0, ncell
        else:  # start_from_dump, then global_pass
            e.upload_rates(dump["phih_grid"], dump["phihe_grid"], dump.get("phiheat"))
            e.upload_iter_state(dump["xh_av"], dump["xhe_av"], dump["xh_intermed"], dump["xhe_intermed"])
            niter = int(dump["niter"])
            conv_flag = e.global_pass(dt)
            self.conv_flags.append(conv_flag)
        numsrc += getattr(e, "plane_count", 0)    # a plane (HipEngine.set_plane_sources) is source NumSrc + p of every deal
        conv_criterion = min(int(convergence_fraction * self.mesh[0] * self.mesh[1] * self.mesh[2]), numsrc)
        while True:
            if conv_flag < conv_criterion and niter > 1:
                e.end_step()
                break
            elif niter > 500:
                break
            niter += 1
            e.set_rates_to_zero()
            fused = comm is not None and numsrc > 0 and niter not in dump_at and callable(getattr(comm, "pass_allreduce_chemistry", None))
            if fused:   # pass, sum over ranks and global pass overlapped slab by slab (parallel.py)
                conv_flag = comm.pass_allreduce_chemistry(e, dt)
                self.conv_flags.append(conv_flag)
                continue
            if numsrc > 0:
                if comm is not None:
                    comm.pass_and_allreduce(e)
                else:
                    e.pass_sources(1, 1)
                if niter in dump_at:
                    self.iteration_dump = {"niter": niter, **e.download_rates(), **e.download_iter_state()}
                    if not e.isothermal:
                        tmp = Material(ndens=None, xh=np.empty(2 * ncell), xhe=np.empty(3 * ncell),
                                       temperature_grid=np.empty(3 * ncell, dtype=np.float32), isothermal=False)
                        e.download_state(tmp)
                        self.iteration_dump["temperature"] = tmp.temperature_grid
            conv_flag = e.global_pass(dt)
            self.conv_flags.append(conv_flag)
        self.niter = niter

    # use evolve_data, only: phih_grid, phiheat (output.F90:26)
    @property
    def rates(self):
        return self.engine.download_rates()

    @property
    def iter_state(self):
        return self.engine.download_iter_state()
