"""fusionpic — Python host mirror of the reference's pusher object over the C ABI.

The shipped host language is JavaScript (fusion-sim_amd/js/empic_native.js over an
N-API addon).  This module binds the SAME C ABI (include/fusionpic.h) with ctypes
for the Python tools of this repository: tests/, bench.py and __graft_entry__.py.
It keeps the reference's factory and method names
(empic.js:30 makeCylindricalParticlePusher, :1157 set, :1352 addCurrentLoop,
:1380 addCurrentZ, :1391 addBZ, :1402 addBTheta, :1413 precalc, :1436 step,
:1471 density) and its error behaviour: a failed call raises `FusionPicError`
synchronously, with spec errors worded ".prop <- ..." (utilities.js:118-127).

There is no CPU path here.  If libfusionpic.so is missing the import fails; if no
gfx950 device is present the factory raises.
"""
import builtins
import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libfusionpic.so")

F32, F64 = 0, 1
GRID_E, GRID_B, GRID_SINK_MASK, GRID_SOURCE_PDF = 0, 1, 2, 3
(READ_MOMENTS, READ_NORM, READ_AVG, READ_R1, READ_R2, READ_R3, READ_A, READ_B, READ_E, READ_SINK,
 READ_INV_CDF) = range(11)
BUF_CELL_SUMS, BUF_RHO_FIXED = 0, 1
GEOM_CYL_RZ, GEOM_CART3D = 0, 1
SOLVER_NONE, SOLVER_POISSON_FFT, SOLVER_YEE = 0, 1, 2
F3_E, F3_RHO, F3_PHI, F3_RHO_FIXED, F3_B_NODES, F3_EDGE_E, F3_FACE_B, F3_J_FIXED = range(8)

ABI_FUNCTIONS = [
    "fpic_last_error", "fpic_abi_version", "fpic_build_arch", "fpic_create", "fpic_destroy", "fpic_set_particles",
    "fpic_set_grid", "fpic_set_random_state", "fpic_add_current_loop", "fpic_add_current_z", "fpic_add_bz",
    "fpic_add_btheta", "fpic_precalc", "fpic_step", "fpic_substeps", "fpic_density", "fpic_deposit", "fpic_density_finish",
    "fpic_density_finish_from",
    "fpic_read_grid", "fpic_get_particles", "fpic_get_cells", "fpic_device_buffer", "fpic_set_stream",
    "fpic_get_stream", "fpic_sort", "fpic_sync", "fpic_profile", "fpic_get_stats", "fpic_reset_stats",
    "fpic_get_substep_counter", "fpic_set_substep_counter", "fpic_save_checkpoint", "fpic_load_checkpoint",
    "fpic_add_species", "fpic_set_particles_of", "fpic_get_particles_of", "fpic_get_cells_of", "fpic_add_b",
    "fpic_set_field3", "fpic_read_field3", "fpic_set_particles_range", "fpic_get_particles_range", "fpic_get_cells_range",
    "fpic_comm_unique_id", "fpic_comm_init", "fpic_comm_destroy", "fpic_comm_info", "fpic_comm_set_overlap",
    "fpic_domain_init", "fpic_domain_set_particles", "fpic_domain_get_particles", "fpic_domain_stats",
    "fpic_group_precalc", "fpic_group_step", "fpic_group_density",
    "fpic_energy_now", "fpic_energy_record", "fpic_energy_history", "fpic_histogram", "fpic_moments",
    "fpic_series_now", "fpic_series_record", "fpic_series_history",
    "fpic_modes_now", "fpic_modes_record", "fpic_modes_history",
    "fpic_select", "fpic_load", "fpic_load_profile", "fpic_load_radial", "fpic_collide", "fpic_collide_register", "fpic_collide_stats", "fpic_collide_clear",
    "fpic_pair", "fpic_pair_register", "fpic_pair_stats", "fpic_pair_clear",
    "fpic_fusion", "fpic_fusion_register", "fpic_fusion_stats", "fpic_fusion_grid", "fpic_fusion_clear",
    "fpic_fusion_spectrum", "fpic_fusion_spectrum_register", "fpic_fusion_spectrum_read", "fpic_fusion_spectrum_clear",
    "fpic_force", "fpic_force_register", "fpic_force_stats", "fpic_force_clear",
    "fpic_gas", "fpic_gas_register", "fpic_gas_stats", "fpic_gas_clear",
    "fpic_remove", "fpic_remove_register", "fpic_remove_stats", "fpic_remove_clear", "fpic_renumber",
    "fpic_reserve", "fpic_population", "fpic_inject", "fpic_inject_register", "fpic_inject_stats", "fpic_inject_clear",
    "fpic_ionize", "fpic_ionize_register", "fpic_ionize_stats", "fpic_ionize_clear",
    "fpic_burn", "fpic_burn_register", "fpic_burn_stats", "fpic_burn_clear",
]


class FusionPicError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


# ---- what the request builders share: a value the C structure cannot carry is refused here, by the property's name
def _whole(name, v, bits, signed=False):
    lo_, hi_ = (-(1 << bits - 1), 1 << bits - 1) if signed else (0, 1 << bits)
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo_ <= int(v) < hi_:
        raise FusionPicError(-1, ".%s <- must be %s %d-bit integer" % (name, "a signed" if signed else "an unsigned", bits))
    return int(v)


def _three(name, v, kind=float):
    try:
        if np.ndim(v) == 0:
            v = [v, v, v]
        if len(v) != 3:
            raise ValueError
        if kind is float:
            return [float(x) for x in v]
        return [_whole(name, x, 32, signed=True) for x in v]
    except (TypeError, ValueError):
        raise FusionPicError(-1, ".%s <- must be a number or three of them" % name)


def _real(name, v):
    try:
        return float(v)
    except (TypeError, ValueError):
        raise FusionPicError(-1, ".%s <- must be a number" % name)


def _real_given(name, v):
    """_real of a property that has no default"""
    if v is None:
        raise FusionPicError(-1, ".%s <- Non-optional property is undefined!" % name)
    return _real(name, v)


def _table(keep, name, v, most=None):
    """(pointer, size) of a table of doubles; the array goes to the caller's `keep`, which must outlive the call the pointer
    is handed to.  most: the entries the count's field can carry (None: a 32-bit count, and the older message)"""
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is None or a.ndim != 1 or a.size > ((1 << 32) - 1 if most is None else most):
        raise FusionPicError(-1, ".%s <- a table must be a sequence of %snumbers" % (name, "" if most is None else "at most %d " % most))
    a = np.ascontiguousarray(a)
    keep.append(a)
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(a.size)


def _scope_code(scope):
    return {"local": DIAG_LOCAL, "global": DIAG_GLOBAL}[scope]


def _every_arg(every):
    """the period of a registration as the C int it is passed as"""
    return _whole("every", every, 32, signed=True)


class Spec(ctypes.Structure):
    _fields_ = [
        ("radius", ctypes.c_double), ("height", ctypes.c_double), ("nr", ctypes.c_int32), ("nz", ctypes.c_int32),
        ("dt", ctypes.c_double), ("nparticles", ctypes.c_int32), ("particle_mass", ctypes.c_double),
        ("particle_charge", ctypes.c_double), ("count", ctypes.c_uint64), ("precision", ctypes.c_int32),
        ("device", ctypes.c_int32), ("physical_a", ctypes.c_int32), ("sort_interval", ctypes.c_int32),
        ("unfused_deposit", ctypes.c_int32), ("rng_mode", ctypes.c_int32), ("rng_seed_lo", ctypes.c_uint32),
        ("rng_seed_hi", ctypes.c_uint32), ("geometry", ctypes.c_int32), ("solver", ctypes.c_int32), ("ny", ctypes.c_int32),
        ("shape", ctypes.c_int32), ("length_y", ctypes.c_double), ("macro_weight", ctypes.c_double),
        ("raster_subpixel_bits", ctypes.c_int32), ("bin_lookahead", ctypes.c_int32), ("reserved", ctypes.c_double * 5),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("n_particles", ctypes.c_uint64), ("particle_updates", ctypes.c_uint64), ("step_launches", ctypes.c_uint64),
        ("deposit_launches", ctypes.c_uint64), ("sort_passes", ctypes.c_uint64), ("deposit_spilled", ctypes.c_uint64),
        ("ms_push", ctypes.c_double), ("ms_deposit", ctypes.c_double), ("ms_stamp", ctypes.c_double),
        ("ms_precalc", ctypes.c_double), ("ms_sort", ctypes.c_double), ("bytes_particle_state", ctypes.c_uint64),
        ("bytes_grid_state", ctypes.c_uint64), ("ms_solve", ctypes.c_double), ("solve_launches", ctypes.c_uint64),
        ("outbox_items", ctypes.c_uint64), ("outbox_full_items", ctypes.c_uint64), ("reserved", ctypes.c_double * 4),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


ENERGY_SPECIES = 16
DIAG_LOCAL, DIAG_GLOBAL = 0, 1


class Energy(ctypes.Structure):
    """mirror of fpic_energy (include/fusionpic.h)"""
    _fields_ = [
        ("substep", ctypes.c_uint64), ("nspecies", ctypes.c_int32), ("reserved_i32", ctypes.c_int32),
        ("field_e", ctypes.c_double), ("field_b", ctypes.c_double), ("field_b_external", ctypes.c_double),
        ("count", ctypes.c_uint64 * ENERGY_SPECIES), ("kinetic", ctypes.c_double * ENERGY_SPECIES),
        ("momentum", (ctypes.c_double * 3) * ENERGY_SPECIES), ("speed_max", ctypes.c_double * ENERGY_SPECIES),
        ("reserved", ctypes.c_double * 8),
    ]


# one fpic_energy row as a numpy record (energyHistory); the same bytes as Energy
ENERGY_DTYPE = np.dtype([
    ("substep", "<u8"), ("nspecies", "<i4"), ("reserved_i32", "<i4"), ("field_e", "<f8"), ("field_b", "<f8"),
    ("field_b_external", "<f8"), ("count", "<u8", (ENERGY_SPECIES,)), ("kinetic", "<f8", (ENERGY_SPECIES,)),
    ("momentum", "<f8", (ENERGY_SPECIES, 3)), ("speed_max", "<f8", (ENERGY_SPECIES,)), ("reserved", "<f8", (8,)),
])


def _energy_dict(row, nspecies=None):
    """{substep, field_e, field_b, field_b_external, count, kinetic, momentum, speed_max} of one row (a numpy record of
    ENERGY_DTYPE); the per-species entries cut to the box's species"""
    ns = int(row["nspecies"]) if nspecies is None else nspecies
    return {"substep": int(row["substep"]), "nspecies": ns, "field_e": float(row["field_e"]), "field_b": float(row["field_b"]),
            "field_b_external": float(row["field_b_external"]), "count": np.array(row["count"][:ns], dtype=np.uint64),
            "kinetic": np.array(row["kinetic"][:ns]), "momentum": np.array(row["momentum"][:ns]),
            "speed_max": np.array(row["speed_max"][:ns])}


def _energy_sum(rows):
    """the rows of several handles (one sub-step of one box) combined in the given order, as the library combines ranks:
    sums left to right, speed_max the largest"""
    out = rows[0].copy()
    for r in rows[1:]:
        for key in ("field_e", "field_b", "field_b_external", "count", "kinetic", "momentum"):
            out[key] = out[key] + r[key]
        out["speed_max"] = np.maximum(out["speed_max"], r["speed_max"])
    return out


_lib = None


HIST_AXES = {"x": 0, "y": 1, "z": 2, "vx": 3, "vy": 4, "vz": 5, "v2": 6}
HIST_MAX_BINS = 1 << 22


class HistSpec(ctypes.Structure):
    """mirror of fpic_hist_spec (include/fusionpic.h)"""
    _fields_ = [
        ("species", ctypes.c_int32), ("naxes", ctypes.c_int32), ("axis", ctypes.c_int32 * 2), ("bins", ctypes.c_int32 * 2),
        ("lo", ctypes.c_double * 2), ("hi", ctypes.c_double * 2), ("reserved", ctypes.c_double * 4),
    ]


def _hist_spec(axes, bins, range, species):
    """(HistSpec, shape, ranges as a float64 [naxes][2] array) of a histogram request.  Only what the structure cannot carry is refused here (an unknown
    axis name, more than two axes, a bin count that is no 32-bit integer, arguments of the wrong length); the library checks
    the rest."""
    names = [axes] if isinstance(axes, str) else list(axes)
    na = len(names)
    if na not in (1, 2):
        raise FusionPicError(-1, ".naxes <- must be 1 or 2")
    nb = list(bins) if isinstance(bins, (list, tuple, np.ndarray)) else [bins] * na
    try:
        rg = np.asarray(range, dtype=np.float64)
    except (TypeError, ValueError):
        raise FusionPicError(-1, ".range <- one (lo, hi) per axis")
    rg = rg.reshape(1, 2) if rg.shape == (2,) and na == 1 else rg
    if len(nb) != na:
        raise FusionPicError(-1, ".bins <- one bin count per axis")
    if rg.shape != (na, 2):
        raise FusionPicError(-1, ".range <- one (lo, hi) per axis")
    s = HistSpec()
    s.species, s.naxes = int(species), na
    for a in builtins.range(na):
        if names[a] not in HIST_AXES:
            raise FusionPicError(-1, ".axis <- must be one of x, y, z, vx, vy, vz, v2")
        if isinstance(nb[a], bool) or not isinstance(nb[a], (int, np.integer)) or not -2 ** 31 <= int(nb[a]) < 2 ** 31:
            raise FusionPicError(-1, ".bins <- must be a positive integer")
        s.axis[a], s.bins[a], s.lo[a], s.hi[a] = HIST_AXES[names[a]], int(nb[a]), rg[a, 0], rg[a, 1]
    return s, tuple(int(b) for b in nb), rg


def _hist_call(sim, s, shape, scope):
    """fpic_histogram of one handle -> (counts of `shape`, outside)"""
    n = int(np.prod([max(b, 0) for b in shape], dtype=np.int64))
    counts = np.zeros(n if 0 < n <= HIST_MAX_BINS else 1, dtype=np.uint64)   # (a refused request writes nothing)
    outside = ctypes.c_uint64()
    sim._check(sim._lib.fpic_histogram(sim._h, ctypes.byref(s), _scope_code(scope), counts.ctypes.data,
                                       ctypes.byref(outside)))
    return counts.reshape(shape), int(outside.value)


def _hist_result(counts, outside, shape, rg):
    return {"counts": counts, "outside": outside,
            "edges": [rg[a, 0] + np.arange(shape[a] + 1) * (rg[a, 1] - rg[a, 0]) / shape[a] for a in builtins.range(len(shape))]}


SELECT_MAX_TERMS = 7
SELECT_MAX_ROWS = 1 << 24


class SelectSpec(ctypes.Structure):
    """mirror of fpic_select_spec (include/fusionpic.h)"""
    _fields_ = [
        ("species", ctypes.c_int32), ("nterms", ctypes.c_int32), ("axis", ctypes.c_int32 * 8), ("lo", ctypes.c_double * 8),
        ("hi", ctypes.c_double * 8), ("id_mod", ctypes.c_uint32), ("id_rem", ctypes.c_uint32), ("reserved", ctypes.c_double * 4),
    ]


def _select_spec(where, species, every):
    """SelectSpec of a selection request.  where: {axis name: (lo, hi)}, None for the infinite side; every: (mod, rem) or
    None.  Only what the structure cannot carry is refused here (an unknown axis name, a bound that is no number, an
    `every` that is no pair of uint32); the library checks the rest."""
    s = SelectSpec()
    s.species = int(species)
    terms = list((where or {}).items())
    if len(terms) > 8:
        raise FusionPicError(-1, ".nterms <- must be 0 .. 7")
    s.nterms = len(terms)
    for t, (name, bounds) in enumerate(terms):
        if name not in HIST_AXES:
            raise FusionPicError(-1, ".axis <- must be one of x, y, z, vx, vy, vz, v2")
        try:
            lo, hi = bounds
            lo = -np.inf if lo is None else float(lo)
            hi = np.inf if hi is None else float(hi)
        except (TypeError, ValueError):
            raise FusionPicError(-1, ".range <- one (lo, hi) per axis, None for the infinite side")
        s.axis[t], s.lo[t], s.hi[t] = HIST_AXES[name], lo, hi
    if every is not None:
        try:
            mod, rem = every
            ok = all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 0 <= int(k) < 1 << 32 for k in (mod, rem))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise FusionPicError(-1, ".every <- must be a pair (mod, rem) of unsigned 32-bit integers")
        s.id_mod, s.id_rem = int(mod), int(rem)
    return s


def _select_call(sim, s, capacity, scope, dtype):
    """fpic_select of one handle -> {ids, position, velocity, matched}.  capacity None: the count query first, then a call
    with room for exactly that many rows; a given capacity that is too small leaves the three arrays None."""
    sc = _scope_code(scope)
    code = sim.precision if dtype is None else (F32 if np.dtype(dtype) == np.float32 else F64)
    matched = ctypes.c_uint64()
    if capacity is None:
        sim._check(sim._lib.fpic_select(sim._h, ctypes.byref(s), sc, 0, None, None, None, code, ctypes.byref(matched)))
        capacity = matched.value
    capacity = int(capacity)
    if capacity < 0 or capacity >= 1 << 64:
        raise FusionPicError(-1, ".capacity <- must be an unsigned 64-bit integer")
    rows = capacity if capacity <= SELECT_MAX_ROWS else 1     # (a refused request writes nothing)
    ids = np.zeros(rows, dtype=np.uint32)
    pos, vel = np.zeros((rows, 3), dtype=_np_dtype(code)), np.zeros((rows, 3), dtype=_np_dtype(code))
    ptr = lambda a: a.ctypes.data if capacity else None       # (capacity 0: the count query)
    sim._check(sim._lib.fpic_select(sim._h, ctypes.byref(s), sc, capacity, ptr(ids), ptr(pos), ptr(vel), code, ctypes.byref(matched)))
    m = int(matched.value)
    if m > capacity:
        return {"ids": None, "position": None, "velocity": None, "matched": m}
    return {"ids": ids[:m].copy(), "position": pos[:m].copy(), "velocity": vel[:m].copy(), "matched": m}


def _select_count(sim, s, scope):
    matched = ctypes.c_uint64()
    sim._check(sim._lib.fpic_select(sim._h, ctypes.byref(s), _scope_code(scope), 0, None, None, None,
                                    sim.precision, ctypes.byref(matched)))
    return int(matched.value)


LOAD_RANDOM, LOAD_POS, LOAD_VEL, LOAD_LATTICE, LOAD_PAIRED, LOAD_APPEND = 0, 1, 2, 4, 8, 16
LOAD_SEED = 0x5EEDF051


class LoadSpec(ctypes.Structure):
    """mirror of fpic_load_spec (include/fusionpic.h)"""
    _fields_ = [
        ("species", ctypes.c_int32), ("flags", ctypes.c_uint32), ("first", ctypes.c_uint64), ("count", ctypes.c_uint64),
        ("seed", ctypes.c_uint64), ("stream", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
        ("lo", ctypes.c_double * 3), ("hi", ctypes.c_double * 3), ("drift", ctypes.c_double * 3), ("vth", ctypes.c_double * 3),
        ("mode", ctypes.c_int32 * 3), ("reserved2", ctypes.c_int32),
        ("xamp", ctypes.c_double * 3), ("xphase", ctypes.c_double), ("vamp", ctypes.c_double * 3), ("vphase", ctypes.c_double),
    ]


def _load_spec(box, species=0, first=0, count=None, seed=LOAD_SEED, stream=0, lo=None, hi=None, drift=0, vth=0, mode=None, xamp=0, xphase=0,
               vamp=0, vphase=0, lattice=False, paired=False, position=True, velocity=True, append=False):
    """LoadSpec of a loader request.  box: the three lengths in metres (hi = None: the whole box); scalars broadcast to three
    components.  Only what the structure cannot carry is refused here (a value that is no number, a vector that has not three
    components, an integer outside its field); the library checks the rest."""
    s = LoadSpec()

    s.species = _whole("species", species, 32, signed=True)
    s.first = _whole("first", first, 64)
    s.count = (1 << 64) - 1 if count is None else _whole("count", count, 64)
    s.seed = _whole("seed", seed, 64)
    s.stream = _whole("stream", stream, 32)
    s.flags = ((LOAD_POS if position else 0) | (LOAD_VEL if velocity else 0) | (LOAD_LATTICE if lattice else 0) |
               (LOAD_PAIRED if paired else 0) | (LOAD_APPEND if append else 0))
    s.lo[:] = _three("lo", 0.0 if lo is None else lo)
    s.hi[:] = [float(x) for x in box] if hi is None else _three("hi", hi)
    s.drift[:], s.vth[:] = _three("drift", drift), _three("vth", vth)
    s.mode[:] = _three("mode", 0 if mode is None else mode, kind=int)
    s.xamp[:], s.vamp[:] = _three("xamp", xamp), _three("vamp", vamp)
    s.xphase, s.vphase = _real("xphase", xphase), _real("vphase", vphase)
    return s


LOAD_TABLE_MAX = 1025


class LoadProfile(ctypes.Structure):
    """mirror of fpic_load_profile (include/fusionpic.h)"""
    _fields_ = [
        ("density_n", ctypes.c_uint32 * 3), ("thermal_n", ctypes.c_uint32 * 3), ("shear_n", ctypes.c_uint32),
        ("shear_axis", ctypes.c_int32), ("shear_component", ctypes.c_int32), ("reserved", ctypes.c_uint32 * 2),
        ("density", ctypes.POINTER(ctypes.c_double) * 3), ("thermal", ctypes.POINTER(ctypes.c_double) * 3),
        ("shear", ctypes.POINTER(ctypes.c_double)),
    ]


def _load_profile(density=None, thermal=None, shear=None):
    """LoadProfile of the tables of a profiled load, or None if all three are None.  density, thermal: three entries, each
    None or a one-dimensional array of numbers; shear: dict(axis=, component=, values=).  Only what the structure cannot
    carry is refused here; the library checks the node counts and the values.  The arrays are kept alive by the result
    (its `_tables`)."""
    if density is None and thermal is None and shear is None:
        return None
    p = LoadProfile()
    p._tables = []

    def table(name, v):
        try:
            a = np.asarray(v, dtype=np.float64)
        except (TypeError, ValueError):
            raise FusionPicError(-1, ".%s <- a table must be a one-dimensional array of numbers" % name)
        a = np.ascontiguousarray(a) if a.ndim == 1 else a
        if v is None or a.ndim != 1 or a.size >= 1 << 32:
            raise FusionPicError(-1, ".%s <- a table must be a one-dimensional array of numbers" % name)
        p._tables.append(a)
        return a.size, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    for name, tabs, counts, ptrs in (("density", density, p.density_n, p.density), ("thermal", thermal, p.thermal_n, p.thermal)):
        if tabs is None:
            continue
        if isinstance(tabs, (str, bytes, dict)) or not hasattr(tabs, "__len__") or len(tabs) != 3:
            raise FusionPicError(-1, ".%s <- expected three entries (x, y, z), each None or a table" % name)
        for a in range(3):
            if tabs[a] is not None:
                counts[a], ptrs[a] = table(name, tabs[a])
    if shear is not None:
        if not isinstance(shear, dict) or set(shear) != {"axis", "component", "values"}:
            raise FusionPicError(-1, ".shear <- expected dict(axis=, component=, values=)")
        for key, field in (("axis", "shear_axis"), ("component", "shear_component")):
            v = shear[key]
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -(1 << 31) <= int(v) < 1 << 31:
                raise FusionPicError(-1, ".shear_%s <- must be 0, 1 or 2" % key)
            setattr(p, field, int(v))
        p.shear_n, p.shear = table("shear", shear["values"])
    return p


LOAD_SPHERE, LOAD_CYLINDER = 1, 2
_LOAD_GEOMETRIES = {"sphere": LOAD_SPHERE, "cylinder": LOAD_CYLINDER}


class LoadRadial(ctypes.Structure):
    """mirror of fpic_load_radial (include/fusionpic.h)"""
    _fields_ = [
        ("geometry", ctypes.c_uint32), ("axis", ctypes.c_int32), ("center", ctypes.c_double * 3), ("r_max", ctypes.c_double),
        ("density_n", ctypes.c_uint32), ("thermal_n", ctypes.c_uint32), ("radial_n", ctypes.c_uint32), ("azimuthal_n", ctypes.c_uint32),
        ("axial_n", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3),
        ("density", ctypes.POINTER(ctypes.c_double)), ("thermal", ctypes.POINTER(ctypes.c_double)), ("radial", ctypes.POINTER(ctypes.c_double)),
        ("azimuthal", ctypes.POINTER(ctypes.c_double)), ("axial", ctypes.POINTER(ctypes.c_double)),
    ]


_RADIAL_KEYS = {"geometry", "center", "r_max", "axis", "density", "thermal", "flow_radial", "flow_azimuthal", "flow_axial"}


def _load_radial(radial):
    """LoadRadial of the `radial` argument of load(): dict(geometry="sphere" | "cylinder" (or the code), center=(x, y, z),
    r_max=, axis=0, density=, thermal=, flow_radial=, flow_azimuthal=, flow_axial=), every table None or a one-dimensional
    array of numbers.  Only what the structure cannot carry is refused here; the library checks the rest.  The arrays are
    kept alive by the result (its `_tables`)."""
    if not isinstance(radial, dict) or not set(radial) <= _RADIAL_KEYS or not {"geometry", "center", "r_max"} <= set(radial):
        raise FusionPicError(-1, ".radial <- expected dict(geometry=, center=, r_max=[, axis=, density=, thermal=, flow_radial=, flow_azimuthal=, flow_axial=])")
    p = LoadRadial()
    p._tables = []
    g = radial["geometry"]
    g = _LOAD_GEOMETRIES.get(g, g) if isinstance(g, str) else g
    if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 0 <= int(g) < 1 << 32:
        raise FusionPicError(-1, ".geometry <- must be 'sphere' or 'cylinder'")
    p.geometry = int(g)
    ax = radial.get("axis", 0)
    if isinstance(ax, bool) or not isinstance(ax, (int, np.integer)) or not -(1 << 31) <= int(ax) < 1 << 31:
        raise FusionPicError(-1, ".axis <- must be 0, 1 or 2")
    p.axis = int(ax)
    try:
        c = [float(x) for x in radial["center"]]
        if len(c) != 3:
            raise ValueError
    except (TypeError, ValueError):
        raise FusionPicError(-1, ".center <- must be three numbers")
    p.center[:] = c
    try:
        p.r_max = float(radial["r_max"])
    except (TypeError, ValueError):
        raise FusionPicError(-1, ".r_max <- must be a number")
    for key, name in (("density", "density"), ("thermal", "thermal"), ("flow_radial", "radial"), ("flow_azimuthal", "azimuthal"), ("flow_axial", "axial")):
        v = radial.get(key)
        if v is None:
            continue
        try:
            a = np.asarray(v, dtype=np.float64)
        except (TypeError, ValueError):
            raise FusionPicError(-1, ".%s <- a table must be a one-dimensional array of numbers" % key)
        if a.ndim != 1 or a.size >= 1 << 32:
            raise FusionPicError(-1, ".%s <- a table must be a one-dimensional array of numbers" % key)
        a = np.ascontiguousarray(a)
        p._tables.append(a)
        setattr(p, name + "_n", a.size)
        setattr(p, name, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return p


def _load_call(sim, s, profile=None, radial=None):
    loaded = ctypes.c_uint64()
    if radial is not None:
        sim._check(sim._lib.fpic_load_radial(sim._h, ctypes.byref(s), ctypes.byref(radial), ctypes.byref(loaded)))
    elif profile is None:
        sim._check(sim._lib.fpic_load(sim._h, ctypes.byref(s), ctypes.byref(loaded)))
    else:
        sim._check(sim._lib.fpic_load_profile(sim._h, ctypes.byref(s), ctypes.byref(profile), ctypes.byref(loaded)))
    return int(loaded.value)


COLLIDE_EXCHANGE, COLLIDE_ELASTIC, COLLIDE_RELAX = 0, 1, 2
COLLIDE_MAX_OPS = 8
COLLIDE_SEED = 0xC0111DE5
COLLIDE_KINDS = {"exchange": COLLIDE_EXCHANGE, "elastic": COLLIDE_ELASTIC, "relax": COLLIDE_RELAX}


class CollideSpec(ctypes.Structure):
    """mirror of fpic_collide_spec (include/fusionpic.h)"""
    _fields_ = [
        ("species", ctypes.c_int32), ("kind", ctypes.c_int32), ("seed", ctypes.c_uint64), ("stream", ctypes.c_uint32), ("epoch", ctypes.c_uint32),
        ("nu_tau", ctypes.c_double), ("sigma_tau", ctypes.c_double), ("g_max", ctypes.c_double),
        ("drift", ctypes.c_double * 3), ("vth", ctypes.c_double * 3), ("mass_ratio", ctypes.c_double), ("reserved", ctypes.c_double * 4),
    ]


class CollideResult(ctypes.Structure):
    """mirror of fpic_collide_result"""
    _fields_ = [("applications", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("collided", ctypes.c_uint64), ("clipped", ctypes.c_uint64)]


def _collide_spec(dt, kind, species=0, nu=None, sigma_n=None, tau=None, nu_tau=None, sigma_tau=None, g_max=0, drift=0, vth=0, mass_ratio=None,
                  seed=COLLIDE_SEED, stream=0, epoch=0):
    """CollideSpec of a collision request.  kind: a code or one of "exchange", "elastic", "relax".  The rates are given either
    as the physical triple — nu (1/s), sigma_n (density times cross-section, 1/m) and tau (s; None: dt, the caller's default) —
    or as the dimensionless pair nu_tau, sigma_tau (per unit of g in c); a rate left out is zero.  mass_ratio None: +inf (a
    fixed target) for "elastic", 0 otherwise.  Only what the structure cannot carry, or a mix of the two forms, is refused
    here; the library checks the rest."""
    s = CollideSpec()

    if isinstance(kind, str):
        if kind not in COLLIDE_KINDS:
            raise FusionPicError(-1, ".kind <- must be one of %s" % ", ".join(sorted(COLLIDE_KINDS)))
        kind = COLLIDE_KINDS[kind]
    s.kind = _whole("kind", kind, 32, signed=True)
    s.species = _whole("species", species, 32, signed=True)
    s.seed, s.stream, s.epoch = _whole("seed", seed, 64), _whole("stream", stream, 32), _whole("epoch", epoch, 32)
    physical, pair = nu is not None or sigma_n is not None or tau is not None, nu_tau is not None or sigma_tau is not None
    if physical and pair:
        raise FusionPicError(-1, ".nu_tau <- give either nu, sigma_n, tau or nu_tau, sigma_tau, not both")
    if physical:
        t = _real("tau", dt if tau is None else tau)
        s.nu_tau = _real("nu", 0.0 if nu is None else nu) * t
        s.sigma_tau = _real("sigma_n", 0.0 if sigma_n is None else sigma_n) * SPEED_OF_LIGHT * t
    else:
        s.nu_tau = _real("nu_tau", 0.0 if nu_tau is None else nu_tau)
        s.sigma_tau = _real("sigma_tau", 0.0 if sigma_tau is None else sigma_tau)
    s.g_max = _real("g_max", g_max)
    s.drift[:], s.vth[:] = _three("drift", drift), _three("vth", vth)
    s.mass_ratio = (float("inf") if s.kind == COLLIDE_ELASTIC else 0.0) if mass_ratio is None else _real("mass_ratio", mass_ratio)
    return s


def _collide_counts(r):
    return {"applications": int(r.applications), "candidates": int(r.candidates), "collided": int(r.collided), "clipped": int(r.clipped)}


FORCE_FIELD, FORCE_ACCEL = 0, 1
FORCE_MAX_WAVES, FORCE_MAX_OPS, FORCE_TABLE_MAX = 4, 8, 1025
FORCE_FOREVER = (1 << 64) - 1
FORCE_KINDS = {"field": FORCE_FIELD, "accel": FORCE_ACCEL}
FORCE_FIX_BITS = 80


class ForceWave(ctypes.Structure):
    """mirror of fpic_force_wave (include/fusionpic.h)"""
    _fields_ = [("amp", ctypes.c_double * 3), ("mode", ctypes.c_int32 * 3), ("reserved", ctypes.c_int32), ("nu", ctypes.c_double), ("phase", ctypes.c_double)]


class ForceSpec(ctypes.Structure):
    """mirror of fpic_force_spec"""
    _fields_ = [
        ("species", ctypes.c_int32), ("kind", ctypes.c_int32), ("nwaves", ctypes.c_int32), ("reserved_i32", ctypes.c_int32),
        ("epoch", ctypes.c_uint64), ("start", ctypes.c_uint64), ("stop", ctypes.c_uint64),
        ("lo", ctypes.c_double * 3), ("hi", ctypes.c_double * 3), ("wave", ForceWave * FORCE_MAX_WAVES),
        ("taper_n", ctypes.c_uint32 * 3), ("envelope_n", ctypes.c_uint32),
        ("taper", ctypes.POINTER(ctypes.c_double) * 3), ("envelope", ctypes.POINTER(ctypes.c_double)), ("reserved", ctypes.c_double * 4),
    ]


class ForceResult(ctypes.Structure):
    """mirror of fpic_force_result"""
    _fields_ = [("applications", ctypes.c_uint64), ("kicked", ctypes.c_uint64), ("work_fixed", ctypes.c_uint64 * 2),
                ("impulse_fixed", (ctypes.c_uint64 * 2) * 3), ("work", ctypes.c_double), ("impulse", ctypes.c_double * 3)]


def _force_spec(dt, L, waves=None, species=0, kind="field", lo=None, hi=None, taper=(None, None, None), envelope=None, epoch=0):
    """ForceSpec of a force request, and the arrays its table pointers point into (keep them until the call has returned).
    waves: dicts {amp (a number or three), mode (three integers, default 0), nu (turns per sub-step) or frequency (Hz, becomes
    nu = frequency dt), phase (turns)}.  lo, hi (metres; a number is taken for all three axes) default to the whole box.
    taper: per axis None or the nodes of a table over [lo, hi].  envelope: None (always active, amplitude 1) or {start, stop,
    values}: active for start <= s <= stop, `values` (optional) the nodes of a table over that span.  Only what the structure
    cannot carry is refused here; the library checks the rest."""
    s = ForceSpec()
    keep = []

    if isinstance(kind, str):
        if kind not in FORCE_KINDS:
            raise FusionPicError(-1, ".kind <- must be one of %s" % ", ".join(sorted(FORCE_KINDS)))
        kind = FORCE_KINDS[kind]
    s.kind = _whole("kind", kind, 32, signed=True)
    s.species = _whole("species", species, 32, signed=True)
    s.epoch = _whole("epoch", epoch, 64)
    if waves is None or isinstance(waves, dict) or not hasattr(waves, "__len__"):
        raise FusionPicError(-1, ".waves <- must be a list of 1 .. 4 waves")
    s.nwaves = _whole("nwaves", len(waves), 32, signed=True)
    for k, w in enumerate(list(waves)[:FORCE_MAX_WAVES]):
        if not isinstance(w, dict) or set(w) - {"amp", "mode", "nu", "frequency", "phase"} or "amp" not in w:
            raise FusionPicError(-1, ".waves <- a wave is {amp, mode, nu | frequency, phase}")
        if "nu" in w and "frequency" in w:
            raise FusionPicError(-1, ".nu <- give either nu or frequency, not both")
        s.wave[k].amp[:] = _three("amp", w["amp"])
        mode = w.get("mode", (0, 0, 0))
        if np.ndim(mode) != 1 or len(mode) != 3:
            raise FusionPicError(-1, ".mode <- must be three integers")
        s.wave[k].mode[:] = [_whole("mode", m, 32, signed=True) for m in mode]
        s.wave[k].nu = _real("frequency", w["frequency"]) * dt if "frequency" in w else _real("nu", w.get("nu", 0.0))
        s.wave[k].phase = _real("phase", w.get("phase", 0.0))
    s.lo[:] = _three("lo", 0.0 if lo is None else lo)
    s.hi[:] = _three("hi", L if hi is None else hi)
    if not isinstance(taper, (list, tuple)) or len(taper) != 3:
        raise FusionPicError(-1, ".taper <- must be three tables (None: no table)")
    for a, t in enumerate(taper):
        if t is not None:
            s.taper[a], s.taper_n[a] = _table(keep, "taper", t)
    s.start, s.stop = 0, FORCE_FOREVER
    if envelope is not None:
        if not isinstance(envelope, dict) or set(envelope) - {"start", "stop", "values"}:
            raise FusionPicError(-1, ".envelope <- must be {start, stop, values}")
        s.start = _whole("start", envelope.get("start", 0), 64)
        s.stop = _whole("stop", envelope.get("stop", FORCE_FOREVER), 64)
        if envelope.get("values") is not None:
            s.envelope, s.envelope_n = _table(keep, "envelope", envelope["values"])
    return s, keep


def _force_signed(words):
    v = int(words[0]) | int(words[1]) << 64
    return v - (1 << 128) if v >> 127 else v


def _force_dict(r):
    """work_fixed and impulse_fixed as Python integers (the 128-bit two's complement sums, units of 2^-80)"""
    return {"applications": int(r.applications), "kicked": int(r.kicked), "work_fixed": _force_signed(r.work_fixed),
            "impulse_fixed": [_force_signed(r.impulse_fixed[a]) for a in range(3)], "work": float(r.work), "impulse": [float(r.impulse[a]) for a in range(3)]}


def _force_sum(parts, mass, W):
    """the members' integers added up and the doubles formed from the sums as the library forms them: the scale of the energy
    diagnostics times the double nearest to the sum 2^-80 (NaN where a member met a term outside the range)"""
    ke, pm = 0.5 * mass * W * SPEED_OF_LIGHT * SPEED_OF_LIGHT, mass * W * SPEED_OF_LIGHT
    near = lambda total: float(total) * 2.0 ** -FORCE_FIX_BITS
    out = {"applications": parts[0]["applications"], "kicked": sum(p["kicked"] for p in parts), "work_fixed": sum(p["work_fixed"] for p in parts),
           "impulse_fixed": [sum(p["impulse_fixed"][a] for p in parts) for a in range(3)]}
    out["work"] = float("nan") if any(p["work"] != p["work"] for p in parts) else ke * near(out["work_fixed"])
    out["impulse"] = [float("nan") if any(p["impulse"][a] != p["impulse"][a] for p in parts) else pm * near(out["impulse_fixed"][a]) for a in range(3)]
    return out


GAS_EXCHANGE, GAS_ELASTIC = 0, 1
GAS_MAX_OPS, GAS_TABLE_MAX, GAS_TAPER_MAX = 8, 4096, 1025
GAS_SEED = 0x6A5C0111DE
GAS_KINDS = {"exchange": GAS_EXCHANGE, "elastic": GAS_ELASTIC}


class GasSpec(ctypes.Structure):
    """mirror of fpic_gas_spec (include/fusionpic.h)"""
    _fields_ = [
        ("species", ctypes.c_int32), ("kind", ctypes.c_int32), ("seed", ctypes.c_uint64), ("stream", ctypes.c_uint32), ("epoch", ctypes.c_uint32),
        ("density", ctypes.c_double), ("tau", ctypes.c_double), ("g_lo", ctypes.c_double), ("g_hi", ctypes.c_double),
        ("n", ctypes.c_int32), ("reserved_i", ctypes.c_int32), ("sigma", ctypes.POINTER(ctypes.c_double)),
        ("drift", ctypes.c_double * 3), ("vth", ctypes.c_double * 3), ("mass_ratio", ctypes.c_double),
        ("lo", ctypes.c_double * 3), ("hi", ctypes.c_double * 3), ("taper_n", ctypes.c_uint32 * 3), ("reserved_u", ctypes.c_uint32),
        ("taper", ctypes.POINTER(ctypes.c_double) * 3), ("reserved", ctypes.c_double * 4),
    ]


class GasResult(ctypes.Structure):
    """mirror of fpic_gas_result"""
    _fields_ = [("applications", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("collided", ctypes.c_uint64), ("below", ctypes.c_uint64),
                ("above", ctypes.c_uint64), ("energy_fixed", ctypes.c_uint64 * 2), ("momentum_fixed", (ctypes.c_uint64 * 2) * 3),
                ("energy", ctypes.c_double), ("momentum", ctypes.c_double * 3)]


def _gas_spec(tau_default, L, kind, species=0, density=None, tau=None, sigma=None, g_lo=None, g_hi=None, drift=0, vth=0, mass_ratio=None,
              lo=None, hi=None, taper=(None, None, None), seed=GAS_SEED, stream=0, epoch=0):
    """GasSpec of a windowed background collision request, and the arrays its table pointers point into (keep them until the
    call has returned).  kind: a code or "exchange" / "elastic".  density (m^-3) the peak density of the background, tau (s;
    None: tau_default) the time one application stands for, sigma (m^2) the cross-sections at relative speeds uniform from
    g_lo to g_hi (units of c; sigma_table() makes one from a function of the energy).  drift, vth (units of c; scalars
    broadcast) and mass_ratio as for collide().  lo, hi (metres; a number is taken for all three axes) default to the whole
    box; taper: per axis None or the nodes (each in [0, 1]) of a table over [lo, hi], whose product is the density as a
    fraction of `density`.  Only what the structure cannot carry is refused here; the library checks the rest."""
    s = GasSpec()
    keep = []

    if isinstance(kind, str):
        if kind not in GAS_KINDS:
            raise FusionPicError(-1, ".kind <- must be one of %s" % ", ".join(sorted(GAS_KINDS)))
        kind = GAS_KINDS[kind]
    s.kind = _whole("kind", kind, 32, signed=True)
    s.species = _whole("species", species, 32, signed=True)
    s.seed, s.stream, s.epoch = _whole("seed", seed, 64), _whole("stream", stream, 32), _whole("epoch", epoch, 32)
    s.density = _real_given("density", density)
    s.tau = _real_given("tau", tau_default if tau is None else tau)
    s.g_lo, s.g_hi = _real_given("g_lo", g_lo), _real_given("g_hi", g_hi)
    if sigma is None:
        raise FusionPicError(-1, ".sigma <- Non-optional property is undefined!")
    s.sigma, s.n = _table(keep, "sigma", sigma, (1 << 31) - 1)
    s.drift[:], s.vth[:] = _three("drift", drift), _three("vth", vth)
    s.mass_ratio = (float("inf") if s.kind == GAS_ELASTIC else 0.0) if mass_ratio is None else _real_given("mass_ratio", mass_ratio)
    s.lo[:] = _three("lo", 0.0 if lo is None else lo)
    s.hi[:] = _three("hi", L if hi is None else hi)
    if not isinstance(taper, (list, tuple)) or len(taper) != 3:
        raise FusionPicError(-1, ".taper <- must be three tables (None: no table)")
    for a, t in enumerate(taper):
        if t is not None:
            s.taper[a], s.taper_n[a] = _table(keep, "taper", t, (1 << 32) - 1)
    return s, keep


def _gas_dict(r):
    """energy_fixed and momentum_fixed as Python integers (the 128-bit two's complement sums, units of 2^-80): the species' gains"""
    return {"applications": int(r.applications), "candidates": int(r.candidates), "collided": int(r.collided), "below": int(r.below), "above": int(r.above),
            "energy_fixed": _force_signed(r.energy_fixed), "momentum_fixed": [_force_signed(r.momentum_fixed[a]) for a in range(3)],
            "energy": float(r.energy), "momentum": [float(r.momentum[a]) for a in range(3)]}


def _gas_sum(parts, mass, W):
    """the members' integers added up and the doubles formed from the sums as the library forms them (_force_sum)"""
    t = _force_sum([dict(applications=p["applications"], kicked=p["collided"], work_fixed=p["energy_fixed"], impulse_fixed=p["momentum_fixed"],
                         work=p["energy"], impulse=p["momentum"]) for p in parts], mass, W)
    out = {k: sum(p[k] for p in parts) for k in ("candidates", "below", "above")}
    out.update(applications=t["applications"], collided=t["kicked"], energy_fixed=t["work_fixed"], momentum_fixed=t["impulse_fixed"],
               energy=t["work"], momentum=t["impulse"])
    return out


REMOVE_OUTSIDE = 1
REMOVE_MAX_OPS = 8


class RemoveSpec(ctypes.Structure):
    """mirror of fpic_remove_spec (include/fusionpic.h)"""
    _fields_ = [
        ("species", ctypes.c_int32), ("nterms", ctypes.c_int32), ("axis", ctypes.c_int32 * 8), ("lo", ctypes.c_double * 8),
        ("hi", ctypes.c_double * 8), ("id_mod", ctypes.c_uint32), ("id_rem", ctypes.c_uint32), ("flags", ctypes.c_uint32),
        ("reserved_u", ctypes.c_uint32), ("reserved", ctypes.c_double * 4),
    ]


class RemoveResult(ctypes.Structure):
    """mirror of fpic_remove_result"""
    _fields_ = [("applications", ctypes.c_uint64), ("scanned", ctypes.c_uint64), ("removed", ctypes.c_uint64),
                ("energy_fixed", ctypes.c_uint64 * 2), ("momentum_fixed", (ctypes.c_uint64 * 2) * 3),
                ("energy", ctypes.c_double), ("momentum", ctypes.c_double * 3), ("charge", ctypes.c_double)]


def _remove_spec(where, species, every, outside):
    """RemoveSpec of a sink: the predicate as select() takes it (_select_spec), outside=True removes what does NOT match"""
    if not isinstance(outside, (bool, np.bool_)):
        raise FusionPicError(-1, ".outside <- must be True or False")
    q = _select_spec(where, species, every)
    s = RemoveSpec()
    s.species, s.nterms, s.id_mod, s.id_rem = q.species, q.nterms, q.id_mod, q.id_rem
    for t in range(8):
        s.axis[t], s.lo[t], s.hi[t] = q.axis[t], q.lo[t], q.hi[t]
    s.flags = REMOVE_OUTSIDE if outside else 0
    return s


def _remove_dict(r):
    """energy_fixed and momentum_fixed as Python integers (the 128-bit two's complement sums, units of 2^-80): what the species lost"""
    return {"applications": int(r.applications), "scanned": int(r.scanned), "removed": int(r.removed),
            "energy_fixed": _force_signed(r.energy_fixed), "momentum_fixed": [_force_signed(r.momentum_fixed[a]) for a in range(3)],
            "energy": float(r.energy), "momentum": [float(r.momentum[a]) for a in range(3)], "charge": float(r.charge)}


_REMOVE_DECOMPOSED = ("%s needs an undecomposed handle: a rank's dead slots and the arrivals of a migration that rides on its next push "
                      "would need a protocol of their own to compact")


INJECT_VOLUME = 0
INJECT_FLUX = 1
INJECT_MAX_OPS = 8


class InjectSpec(ctypes.Structure):
    """mirror of fpic_inject_spec (include/fusionpic.h)"""
    _fields_ = [
        ("load", LoadSpec), ("kind", ctypes.c_int32), ("axis", ctypes.c_int32), ("side", ctypes.c_int32), ("reserved_i", ctypes.c_int32),
        ("plane", ctypes.c_double), ("epoch", ctypes.c_uint64), ("reserved", ctypes.c_double * 4),
    ]


class InjectResult(ctypes.Structure):
    """mirror of fpic_inject_result"""
    _fields_ = [("applications", ctypes.c_uint64), ("injected", ctypes.c_uint64),
                ("energy_fixed", ctypes.c_uint64 * 2), ("momentum_fixed", (ctypes.c_uint64 * 2) * 3),
                ("energy", ctypes.c_double), ("momentum", ctypes.c_double * 3), ("charge", ctypes.c_double)]


def _inject_spec(box, kind="volume", species=0, count=0, first=0, seed=LOAD_SEED, stream=0, lo=None, hi=None, drift=0, vth=0, axis=0, side=0, plane=0.0,
                 lattice=False, paired=False, mode=None, xamp=0, xphase=0, vamp=0, vphase=0, epoch=0):
    """InjectSpec of a source: the embedded loader request as load() builds it (_load_spec), then the kind's own fields.  Only
    what the structure cannot carry is refused here; the library checks the rest."""
    if kind not in ("volume", "flux"):
        raise FusionPicError(-1, ".kind <- must be 'volume' or 'flux'")
    if count is None or isinstance(count, bool):
        raise FusionPicError(-1, ".count <- must be an unsigned 64-bit integer")
    s = InjectSpec()
    s.load = _load_spec(box, species, first, count, seed, stream, lo, hi, drift, vth, mode, xamp, xphase, vamp, vphase, lattice, paired, True, True, False)
    s.kind = INJECT_VOLUME if kind == "volume" else INJECT_FLUX
    for name, v, lo_, hi_ in (("axis", axis, -(1 << 31), 1 << 31), ("side", side, -(1 << 31), 1 << 31), ("epoch", epoch, 0, 1 << 64)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo_ <= int(v) < hi_:
            raise FusionPicError(-1, ".%s <- must be an integer" % name)
    s.axis, s.side, s.epoch = int(axis), int(side), int(epoch)
    try:
        s.plane = float(plane)
    except (TypeError, ValueError):
        raise FusionPicError(-1, ".plane <- must be a number")
    return s


def _inject_dict(r):
    """energy_fixed and momentum_fixed as Python integers (the 128-bit two's complement sums, units of 2^-80): what the species gained"""
    return {"applications": int(r.applications), "injected": int(r.injected),
            "energy_fixed": _force_signed(r.energy_fixed), "momentum_fixed": [_force_signed(r.momentum_fixed[a]) for a in range(3)],
            "energy": float(r.energy), "momentum": [float(r.momentum[a]) for a in range(3)], "charge": float(r.charge)}


_INJECT_DECOMPOSED = ("%s needs an undecomposed handle: a rank's arrivals ride on its next push, and its message buffers were sized "
                      "from the capacity it had")


IONIZE_MAX_OPS = 8
IONIZE_SEED = 0x1051E0C0FFEE


class IonizeSpec(ctypes.Structure):
    """mirror of fpic_ionize_spec (include/fusionpic.h)"""
    _fields_ = [
        ("species", ctypes.c_int32), ("electron", ctypes.c_int32), ("ion", ctypes.c_int32), ("reserved_i", ctypes.c_int32),
        ("seed", ctypes.c_uint64), ("stream", ctypes.c_uint32), ("epoch", ctypes.c_uint32),
        ("density", ctypes.c_double), ("tau", ctypes.c_double), ("g_lo", ctypes.c_double), ("g_hi", ctypes.c_double), ("g_threshold", ctypes.c_double),
        ("n", ctypes.c_int32), ("reserved_n", ctypes.c_int32), ("sigma", ctypes.POINTER(ctypes.c_double)),
        ("drift", ctypes.c_double * 3), ("vth", ctypes.c_double * 3),
        ("lo", ctypes.c_double * 3), ("hi", ctypes.c_double * 3), ("taper_n", ctypes.c_uint32 * 3), ("reserved_u", ctypes.c_uint32),
        ("taper", ctypes.POINTER(ctypes.c_double) * 3), ("reserved", ctypes.c_double * 4),
    ]


class IonizeGain(ctypes.Structure):
    """mirror of fpic_ionize_gain"""
    _fields_ = [("energy_fixed", ctypes.c_uint64 * 2), ("momentum_fixed", (ctypes.c_uint64 * 2) * 3),
                ("energy", ctypes.c_double), ("momentum", ctypes.c_double * 3), ("charge", ctypes.c_double)]


class IonizeResult(ctypes.Structure):
    """mirror of fpic_ionize_result"""
    _fields_ = [("applications", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("below", ctypes.c_uint64), ("above", ctypes.c_uint64),
                ("ionised", ctypes.c_uint64), ("primary", IonizeGain), ("electron", IonizeGain), ("ion", IonizeGain)]


def _ionize_spec(tau_default, L, species=0, electron=None, ion=None, g_threshold=None, density=None, tau=None, sigma=None, g_lo=None, g_hi=None,
                 drift=0, vth=0, lo=None, hi=None, taper=(None, None, None), seed=IONIZE_SEED, stream=0, epoch=0):
    """IonizeSpec of an ionisation request, and the arrays its table pointers point into (keep them until the call has
    returned).  species: the projectile; electron (None: the projectile species), ion: the species that receive the secondary
    and the ion; g_threshold (units of c): sqrt(2 E_ion / (m c^2)) of the projectile.  The rest as _gas_spec.  Only what the
    structure cannot carry is refused here; the library checks the rest."""
    g, keep = _gas_spec(tau_default, L, GAS_EXCHANGE, species, density, tau, sigma, g_lo, g_hi, drift, vth, None, lo, hi, taper, seed, stream, epoch)
    s = IonizeSpec()
    s.species = g.species
    s.electron = s.species if electron is None else _whole("electron", electron, 32, signed=True)
    if ion is None:
        raise FusionPicError(-1, ".ion <- Non-optional property is undefined!")
    s.ion = _whole("ion", ion, 32, signed=True)
    s.g_threshold = _real_given("g_threshold", g_threshold)
    for name in ("seed", "stream", "epoch", "density", "tau", "g_lo", "g_hi", "n", "sigma"):
        setattr(s, name, getattr(g, name))
    for a in range(3):
        s.drift[a], s.vth[a], s.lo[a], s.hi[a], s.taper_n[a], s.taper[a] = g.drift[a], g.vth[a], g.lo[a], g.hi[a], g.taper_n[a], g.taper[a]
    return s, keep


def _ionize_dict(r):
    """the counts, and per group (primary: the projectile species; electron, ion: the targets) what the species gained:
    energy_fixed and momentum_fixed as Python integers (the 128-bit two's complement sums, units of 2^-80)"""
    out = {k: int(getattr(r, k)) for k in ("applications", "candidates", "below", "above", "ionised")}
    for name in ("primary", "electron", "ion"):
        g = getattr(r, name)
        out[name] = {"energy_fixed": _force_signed(g.energy_fixed), "momentum_fixed": [_force_signed(g.momentum_fixed[a]) for a in range(3)],
                     "energy": float(g.energy), "momentum": [float(g.momentum[a]) for a in range(3)], "charge": float(g.charge)}
    return out


BURN_MAX_OPS = 4
BURN_SEED = 0xB0510C0FFEE


class BurnSpec(ctypes.Structure):
    """mirror of fpic_burn_spec (include/fusionpic.h)"""
    _fields_ = [
        ("species_a", ctypes.c_int32), ("species_b", ctypes.c_int32), ("product_a", ctypes.c_int32), ("product_b", ctypes.c_int32),
        ("seed", ctypes.c_uint64), ("stream", ctypes.c_uint32), ("epoch", ctypes.c_uint32),
        ("tau", ctypes.c_double), ("g_lo", ctypes.c_double), ("g_hi", ctypes.c_double),
        ("n", ctypes.c_int32), ("reserved_i", ctypes.c_int32), ("sigma", ctypes.POINTER(ctypes.c_double)),
        ("q_value", ctypes.c_double), ("other_mass", ctypes.c_double), ("reserved", ctypes.c_double * 4),
    ]


class BurnResult(ctypes.Structure):
    """mirror of fpic_burn_result"""
    _fields_ = [(k, ctypes.c_uint64) for k in ("applications", "pairs", "below", "above", "cells", "overfull_cells", "overfull_particles",
                                               "accepted", "blocked", "saturated", "burnt")] + \
               [("reactant_a", IonizeGain), ("reactant_b", IonizeGain), ("product_a", IonizeGain), ("product_b", IonizeGain)]


def _burn_spec(tau_default, a=0, b=None, products=None, q_value=0.0, other_mass=0.0, seed=BURN_SEED, **request):
    """BurnSpec of a burn request: the reactants a and b (None: a with itself), products = (p3, p4) the species that receive
    the two products, p4 None: the fourth particle leaves the box and other_mass (kg) is its mass; q_value (J); the rest as
    _fusion_spec.  Only what the structure cannot carry is refused here; the library checks the rest.  The spec keeps the
    table alive (spec._table)."""
    f = _fusion_spec(tau_default, a, b, seed=seed, **request)
    s = BurnSpec()
    s._table = f._table
    for name in ("species_a", "species_b", "seed", "stream", "epoch", "tau", "g_lo", "g_hi", "n", "sigma"):
        setattr(s, name, getattr(f, name))
    try:
        p3, p4 = products
    except (TypeError, ValueError):
        raise FusionPicError(-1, ".products <- must be (product_a, product_b or None)")
    s.product_a = _whole("product_a", p3, 32, signed=True)
    s.product_b = -1 if p4 is None else _whole("product_b", p4, 32, signed=True)
    s.q_value, s.other_mass = _real_given("q_value", q_value), _real_given("other_mass", other_mass)
    return s


def _burn_dict(r):
    """the counts, and per group what the species lost (reactant_a, reactant_b) or gained (product_a, product_b):
    energy_fixed and momentum_fixed as Python integers (the 128-bit two's complement sums, units of 2^-80)"""
    out = {k: int(getattr(r, k)) for k in ("applications", "pairs", "below", "above", "cells", "overfull_cells", "overfull_particles",
                                           "accepted", "blocked", "saturated", "burnt")}
    for name in ("reactant_a", "reactant_b", "product_a", "product_b"):
        g = getattr(r, name)
        out[name] = {"energy_fixed": _force_signed(g.energy_fixed), "momentum_fixed": [_force_signed(g.momentum_fixed[a]) for a in range(3)],
                     "energy": float(g.energy), "momentum": [float(g.momentum[a]) for a in range(3)], "charge": float(g.charge)}
    return out


PAIR_MAX_OPS = 8
PAIR_CELL_MAX = 2048
PAIR_SEED = 0x7A1C12ABE


class PairSpec(ctypes.Structure):
    """mirror of fpic_pair_spec (include/fusionpic.h)"""
    _fields_ = [
        ("species_a", ctypes.c_int32), ("species_b", ctypes.c_int32), ("seed", ctypes.c_uint64), ("stream", ctypes.c_uint32), ("epoch", ctypes.c_uint32),
        ("log_lambda", ctypes.c_double), ("tau", ctypes.c_double), ("reserved", ctypes.c_double * 4),
    ]


class PairResult(ctypes.Structure):
    """mirror of fpic_pair_result"""
    _fields_ = [("applications", ctypes.c_uint64), ("pairs", ctypes.c_uint64), ("strong", ctypes.c_uint64), ("cells", ctypes.c_uint64),
                ("overfull_cells", ctypes.c_uint64), ("overfull_particles", ctypes.c_uint64)]


def _pair_spec(tau_default, a=0, b=None, log_lambda=None, tau=None, seed=PAIR_SEED, stream=0, epoch=0):
    """PairSpec of a binary collision request: species a with species b (None: a with itself), the Coulomb logarithm, the
    time tau (s) one application stands for (None: tau_default).  Only what the structure cannot carry is refused here; the
    library checks the rest."""
    s = PairSpec()

    s.species_a = _whole("species_a", a, 32, signed=True)
    s.species_b = s.species_a if b is None else _whole("species_b", b, 32, signed=True)
    s.seed, s.stream, s.epoch = _whole("seed", seed, 64), _whole("stream", stream, 32), _whole("epoch", epoch, 32)
    s.log_lambda = _real_given("log_lambda", log_lambda)
    s.tau = _real_given("tau", tau_default if tau is None else tau)
    return s


_PAIR_DECOMPOSED = ("%s needs an undecomposed handle: between two migrations the particles of a cell can sit on two ranks (in the "
                    "ghost planes), so a rank cannot pair a cell alone")


def _pair_counts(r):
    return {k: int(getattr(r, k)) for k in ("applications", "pairs", "strong", "cells", "overfull_cells", "overfull_particles")}


FUSION_MAX_OPS = 4
FUSION_TABLE_MAX = 4096
FUSION_SEED = 0xF0510D7
FUSION_C = 2.998e8


class FusionSpec(ctypes.Structure):
    """mirror of fpic_fusion_spec (include/fusionpic.h)"""
    _fields_ = [
        ("species_a", ctypes.c_int32), ("species_b", ctypes.c_int32), ("seed", ctypes.c_uint64), ("stream", ctypes.c_uint32), ("epoch", ctypes.c_uint32),
        ("tau", ctypes.c_double), ("g_lo", ctypes.c_double), ("g_hi", ctypes.c_double), ("n", ctypes.c_int32), ("reserved_i", ctypes.c_int32),
        ("sigma", ctypes.POINTER(ctypes.c_double)), ("reserved", ctypes.c_double * 4),
    ]


class FusionResult(ctypes.Structure):
    """mirror of fpic_fusion_result"""
    _fields_ = [("applications", ctypes.c_uint64), ("pairs", ctypes.c_uint64), ("below", ctypes.c_uint64), ("above", ctypes.c_uint64), ("cells", ctypes.c_uint64),
                ("overfull_cells", ctypes.c_uint64), ("overfull_particles", ctypes.c_uint64), ("yield_hi", ctypes.c_uint64), ("yield_lo", ctypes.c_uint64),
                ("unit_exponent", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def _fusion_spec(tau_default, a=0, b=None, sigma=None, g_lo=None, g_hi=None, tau=None, seed=FUSION_SEED, stream=0, epoch=0):
    """FusionSpec of a yield tally: species a with species b (None: a with itself), the table sigma (m^2) at relative speeds
    uniform from g_lo to g_hi (units of c), the time tau (s) one application stands for (None: tau_default).  Only what the
    structure cannot carry is refused here; the library checks the rest.  The spec keeps the table alive (spec._table)."""
    s = FusionSpec()

    s.species_a = _whole("species_a", a, 32, signed=True)
    s.species_b = s.species_a if b is None else _whole("species_b", b, 32, signed=True)
    s.seed, s.stream, s.epoch = _whole("seed", seed, 64), _whole("stream", stream, 32), _whole("epoch", epoch, 32)
    s.tau = _real_given("tau", tau_default if tau is None else tau)
    s.g_lo, s.g_hi = _real_given("g_lo", g_lo), _real_given("g_hi", g_hi)
    if sigma is None:
        raise FusionPicError(-1, ".sigma <- Non-optional property is undefined!")
    try:
        table = np.ascontiguousarray(sigma, dtype=np.float64)
    except (TypeError, ValueError):
        raise FusionPicError(-1, ".sigma <- must be a sequence of numbers")
    if table.ndim != 1:
        raise FusionPicError(-1, ".sigma <- must be a sequence of numbers")
    if not 2 <= len(table) <= FUSION_TABLE_MAX:
        raise FusionPicError(-1, ".n <- must be 2 .. FPIC_FUSION_TABLE_MAX (4096)")
    s.n = len(table)
    s._table = table
    s.sigma = table.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    return s


def _fusion_counts(r):
    """the counts of a fpic_fusion_result, the exact total as a Python integer (units of 2**unit_exponent reactions) and as a float"""
    out = {k: int(getattr(r, k)) for k in ("applications", "pairs", "below", "above", "cells", "overfull_cells", "overfull_particles", "yield_hi", "yield_lo",
                                           "unit_exponent")}
    out["reactions_exact"] = (out["yield_hi"] << 32) + out["yield_lo"]
    out["reactions"] = float(np.ldexp(float(out["reactions_exact"]), out["unit_exponent"])) if out["reactions_exact"] < 1 << 1000 else float("inf")
    return out


def sigma_table(sigma_of_keV, mass_a, mass_b, e_lo_keV, e_hi_keV, n=FUSION_TABLE_MAX):
    """Samples a cross-section onto the table of fusionYield: returns (S, g_lo, g_hi).  sigma_of_keV: a callable that takes
    an array of centre-of-mass energies in keV and returns the cross-section in m^2; mass_a, mass_b: the reactants' masses in
    kg; the table covers e_lo_keV .. e_hi_keV in n points UNIFORM IN THE RELATIVE SPEED g (units of c) with the
    non-relativistic E = m_ab (g c)^2 / 2, m_ab the reduced mass and c = 2.998e8, the box's.  Negative or non-finite values
    of the callable are refused.
    The library ships no nuclear data: a wrong constant in a shipped table is worse than none.  Fits of the D-T, D-D and
    D-3He cross-sections are published by H.-S. Bosch and G. M. Hale, Nuclear Fusion 32 (1992) 611 (valid 0.5 - 550 keV for
    D-T), and, older, by B. H. Duane in BNWL-1685 (1972), reproduced in the NRL Plasma Formulary; evaluated data are in the
    ENDF/B libraries."""
    keV = 1.602176634e-16
    mass_a, mass_b, e_lo_keV, e_hi_keV = float(mass_a), float(mass_b), float(e_lo_keV), float(e_hi_keV)
    if not (mass_a > 0 and mass_b > 0 and np.isfinite(mass_a + mass_b)):
        raise FusionPicError(-1, ".mass <- must be positive and finite")
    if not (0 <= e_lo_keV < e_hi_keV and np.isfinite(e_hi_keV)):
        raise FusionPicError(-1, ".e_lo_keV <- must be 0 <= e_lo_keV < e_hi_keV, finite")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= int(n) <= FUSION_TABLE_MAX:
        raise FusionPicError(-1, ".n <- must be 2 .. FPIC_FUSION_TABLE_MAX (4096)")
    mab = mass_a * mass_b / (mass_a + mass_b)
    g_lo, g_hi = (float(np.sqrt(2.0 * e * keV / mab)) / FUSION_C for e in (e_lo_keV, e_hi_keV))
    g = g_lo + np.arange(int(n), dtype=np.float64) * ((g_hi - g_lo) / (int(n) - 1))
    energy = 0.5 * mab * (g * FUSION_C) ** 2 / keV
    with np.errstate(all="ignore"):
        S = np.array(sigma_of_keV(energy), dtype=np.float64)
    if S.shape != g.shape:
        raise FusionPicError(-1, ".sigma_of_keV <- must return one value per energy")
    if not np.all(np.isfinite(S) & (S >= 0)):
        raise FusionPicError(-1, ".sigma_of_keV <- every value must be finite and not negative")
    return S, g_lo, g_hi


FUSION_SPECTRUM_MAX_OPS = 4
FUSION_SPECTRUM_BINS_MAX = 256
FSPEC_CM, FSPEC_PRODUCT = 0, 1
FSPEC_AXES = {"cm": FSPEC_CM, "product": FSPEC_PRODUCT}
KEV = 1.602176634e-16            # one keV in joules: the unit of a spectrum's axis is the joule


class FusionSpectrumSpec(ctypes.Structure):
    """mirror of fpic_fusion_spectrum_spec (include/fusionpic.h)"""
    _fields_ = [
        ("tally", FusionSpec), ("axis", ctypes.c_int32), ("bins", ctypes.c_int32), ("lo", ctypes.c_double), ("hi", ctypes.c_double), ("q_value", ctypes.c_double),
        ("product_mass", ctypes.c_double), ("other_mass", ctypes.c_double), ("los", ctypes.c_double * 3), ("reserved", ctypes.c_double * 4),
    ]


def _fusion_spectrum_spec(tau_default, a=0, b=None, axis="product", bins=None, lo=None, hi=None, q_value=0.0, product_mass=0.0, other_mass=0.0, los=None, **request):
    """FusionSpectrumSpec of a product spectrum: the tally's request (see _fusion_spec), the axis ("product": the laboratory
    energy of the product of mass product_mass, the other product having other_mass; "cm": the reacting centre-of-mass
    energy), `bins` bins over [lo, hi) joules, the reaction's q_value (J), the line of sight los (None or zeros: isotropic
    emission).  Only what the structure cannot carry is refused here; the library checks the rest.  The spec keeps the table
    alive (spec._table)."""
    s = FusionSpectrumSpec()
    tally = _fusion_spec(tau_default, a, b, **request)
    s._table = tally._table
    s.tally = tally
    if not isinstance(axis, str) or axis not in FSPEC_AXES:
        raise FusionPicError(-1, ".axis <- must be one of cm, product")
    s.axis = FSPEC_AXES[axis]
    s.bins = _whole("bins", bins, 32, signed=True)

    s.lo, s.hi, s.q_value = _real_given("lo", lo), _real_given("hi", hi), _real_given("q_value", q_value)
    s.product_mass, s.other_mass = _real_given("product_mass", product_mass), _real_given("other_mass", other_mass)
    if los is not None:
        try:
            v = [float(x) for x in los]
        except (TypeError, ValueError):
            raise FusionPicError(-1, ".los <- must be three numbers")
        if len(v) != 3:
            raise FusionPicError(-1, ".los <- must be three numbers")
        s.los[0], s.los[1], s.los[2] = v
    return s


def _fusion_spectrum_result(r, words, lo, hi):
    """the counts of _fusion_counts, the edges, the exact entries as Python integers and the bins as floats (reactions)"""
    got = _fusion_counts(r)
    exact = [(int(words[k, 0]) << 32) + int(words[k, 1]) for k in range(len(words))]
    nbins = len(exact) - 2
    got["edges"] = lo + (hi - lo) * np.arange(nbins + 1, dtype=np.float64) / nbins
    got["bins"], got["under"], got["over"] = exact[:nbins], exact[nbins], exact[nbins + 1]
    got["yield"] = np.array([float(np.ldexp(float(x), got["unit_exponent"])) for x in exact[:nbins]], dtype=np.float64)
    return got


SERIES_MAX_POINTS = 4096
SERIES_MAX_TRACERS = 65536
# the columns of a point row and of a tracer row (fpic_series_*): 8 doubles each
SERIES_POINT_COLUMNS = ("ex", "ey", "ez", "phi", "bx", "by", "bz", "present")
SERIES_TRACER_COLUMNS = ("x", "y", "z", "vx", "vy", "vz", "found", "zero")


class SeriesSpec(ctypes.Structure):
    """mirror of fpic_series_spec (include/fusionpic.h)"""
    _fields_ = [("npoints", ctypes.c_uint32), ("ntracers", ctypes.c_uint32), ("points", ctypes.c_void_p),
                ("tracer_species", ctypes.c_void_p), ("tracer_id", ctypes.c_void_p), ("reserved", ctypes.c_double * 4)]


def _series_spec(points, tracers, species):
    """(SeriesSpec, the arrays it points to) of a request.  Only what the structure cannot carry is refused here (a shape, an
    id that is no uint32); every other check is the library's."""
    s = SeriesSpec()
    keep = []
    if points is not None and np.size(points):
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise FusionPicError(-1, ".points <- must be an array of shape (npoints, 3)")
        if pts.shape[0] >= 1 << 32:
            raise FusionPicError(-1, ".points <- more than FPIC_SERIES_MAX_POINTS (4096) points")
        s.npoints, s.points = pts.shape[0], pts.ctypes.data
        keep.append(pts)
    if tracers is not None and np.size(tracers):
        raw = np.asarray(tracers)
        if raw.ndim != 1 or raw.dtype.kind not in "iu" or (raw.size and (int(raw.min()) < 0 or int(raw.max()) >= 1 << 32)):
            raise FusionPicError(-1, ".tracers <- must be a one-dimensional array of particle indices (uint32)")
        if raw.size >= 1 << 32:
            raise FusionPicError(-1, ".tracers <- more than FPIC_SERIES_MAX_TRACERS (65536) tracers")
        ids = np.ascontiguousarray(raw, dtype=np.uint32)
        sp = np.asarray(species)
        if sp.ndim == 0 and sp.dtype.kind in "iu":
            sp = np.full(ids.shape, int(sp))
        if sp.shape != ids.shape or sp.dtype.kind not in "iu":
            raise FusionPicError(-1, ".species <- must be an int or an array of ints as long as tracers")
        sp = np.ascontiguousarray(np.clip(sp, -1, (1 << 31) - 1), dtype=np.int32)     # (an unknown species stays unknown)
        s.ntracers, s.tracer_species, s.tracer_id = ids.shape[0], sp.ctypes.data, ids.ctypes.data
        keep += [ids, sp]
    return s, keep


def _series_select(parts, flag):
    """entry by entry, the one of `parts` (arrays [..., 8] of the members of a group) whose column `flag` is set; zeros where
    none is.  Returns (selection, owner: the member's index per entry, -1 where none).  Two members flagging one entry is an
    internal error of the library and is reported, not resolved."""
    stack = np.stack(parts)
    flags = stack[..., flag] != 0
    if (flags.sum(axis=0) > 1).any():
        raise FusionPicError(-5, "internal error: two members of the group report one entry of a series row")
    out = np.zeros_like(stack[0])
    owner = np.full(out.shape[:-1], -1, dtype=np.int64)
    for r in builtins.range(len(parts)):
        out[flags[r]] = stack[r][flags[r]]
        owner[flags[r]] = r
    return out, owner


MODES_MAX = 256
MODE_FIELDS = ("ex", "ey", "ez", "phi", "bx", "by", "bz", "rho")   # bit b of a mask is MODE_FIELDS[b]


class ModesSpec(ctypes.Structure):
    """mirror of fpic_modes_spec (include/fusionpic.h)"""
    _fields_ = [("nmodes", ctypes.c_uint32), ("mask", ctypes.c_uint32), ("modes", ctypes.c_void_p), ("reserved", ctypes.c_double * 4)]


def _modes_spec(modes, fields):
    """(ModesSpec, the selected names in bit order, the array the structure points to) of a request.  Only what the structure
    cannot carry is refused here (a shape, a component that is no int32, an unknown name); every other check is the library's."""
    names = [fields] if isinstance(fields, str) else list(fields)
    mask = 0
    for f in names:
        if f not in MODE_FIELDS:
            raise FusionPicError(-1, ".fields <- must be names from ex, ey, ez, phi, bx, by, bz, rho")
        mask |= 1 << MODE_FIELDS.index(f)
    raw = np.asarray(modes if modes is not None else np.zeros((0, 3), dtype=np.int64))
    if raw.size == 0:
        raw = np.zeros((0, 3), dtype=np.int64)
    if raw.ndim != 2 or raw.shape[1] != 3 or raw.dtype.kind not in "iu" or (raw.size and (int(raw.min()) < -2 ** 31 or int(raw.max()) >= 2 ** 31)):
        raise FusionPicError(-1, ".modes <- must be an array of int32 triples of shape (nmodes, 3)")
    if raw.shape[0] >= 1 << 32:
        raise FusionPicError(-1, ".nmodes <- must lie in [1, FPIC_MODES_MAX (256)]")
    m = np.ascontiguousarray(raw, dtype=np.int32)
    s = ModesSpec()
    s.nmodes, s.mask, s.modes = m.shape[0], mask, (m.ctypes.data if m.shape[0] else None)
    return s, [f for f in MODE_FIELDS if f in names], m


def _modes_dict(rows, names):
    """float64 [..., nmodes, nq, 2] -> {name: complex128 [..., nmodes]}"""
    return {f: np.ascontiguousarray(rows[..., q, 0] + 1j * rows[..., q, 1]) for q, f in enumerate(names)}


def _modes_sum(parts):
    """the members' rows added in rank order, as the library adds the ranks'"""
    out = parts[0].copy()
    for p in parts[1:]:
        out += p
    return out


MOMENT_NAMES = ("N", "FX", "FY", "FZ", "SXX", "SYY", "SZZ", "SXY", "SXZ", "SYZ")   # bit b of a mask is MOMENT_NAMES[b]
MOMENT_SETS = {"n": 0x001, "order1": 0x00F, "order2": 0x3FF}
MOM_ONE = 1 << 42          # N of one particle, summed over its eight nodes
MOM_SCALE = 1 << 32        # the fixed-point scale of every other moment
SPEED_OF_LIGHT = 2.998e8   # (empic.js:27, as the library)
ELECTRON_VOLT = 1.602176634e-19


class MomentsSpec(ctypes.Structure):
    """mirror of fpic_moments_spec (include/fusionpic.h)"""
    _fields_ = [("species", ctypes.c_int32), ("mask", ctypes.c_uint32), ("reserved", ctypes.c_double * 4)]


class MomentsInfo(ctypes.Structure):
    """mirror of fpic_moments_info"""
    _fields_ = [("rejected", ctypes.c_uint64), ("spilled", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 2)]


def _moments_mask(which):
    """the mask of "n" | "order1" | "order2" or of an iterable of moment names"""
    if isinstance(which, str):
        if which not in MOMENT_SETS:
            raise FusionPicError(-1, ".which <- must be one of n, order1, order2 or an iterable of moment names")
        return MOMENT_SETS[which]
    mask = 0
    for name in which:
        if name not in MOMENT_NAMES:
            raise FusionPicError(-1, ".which <- no such moment: must be among " + " ".join(MOMENT_NAMES))
        mask |= 1 << MOMENT_NAMES.index(name)
    return mask


def _moments_call(sim, mask, species, scope):
    """fpic_moments of one handle -> (int64 [popcount(mask)][nz][ny][nr], rejected, spilled)"""
    s = MomentsSpec()
    s.species, s.mask = int(species), int(mask) & 0xFFFFFFFF
    nm = bin(mask & 0x3FF).count("1") if 0 < mask < 1 << 10 else 1   # (a refused request writes nothing)
    out = np.zeros((nm, sim.nz, sim.ny, sim.nx), dtype=np.int64)
    info = MomentsInfo()
    sim._check(sim._lib.fpic_moments(sim._h, ctypes.byref(s), _scope_code(scope), out.ctypes.data, ctypes.byref(info)))
    return out, int(info.rejected), int(info.spilled)


def _moments_result(mask, grids, rejected, spilled):
    out = {MOMENT_NAMES[b]: grids[k] for k, b in enumerate(b for b in builtins.range(10) if mask >> b & 1)}
    out["rejected"], out["spilled"] = rejected, spilled
    return out


def load_library(path=None):
    """dlopen libfusionpic.so.  Fails loudly when the HIP library has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    # PyTorch-ROCm ships its own copy of the HIP runtime.  Two runtimes in one process do not share
    # the device (the second one reports "No HIP GPUs"), so when torch is installed it is imported
    # first and libfusionpic.so then binds to the runtime already loaded.  FUSIONPIC_NO_TORCH=1 skips
    # this for hosts that never touch torch.
    if "torch" not in sys.modules and not os.environ.get("FUSIONPIC_NO_TORCH"):
        import importlib.util
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
    if not os.path.exists(path):
        raise ImportError("%s not found: build it with `make -C fusion-sim_amd` (hipcc, gfx950); "
                          "there is no CPU fallback" % path)
    lib = ctypes.CDLL(path)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.fpic_last_error.restype = ctypes.c_char_p
    lib.fpic_last_error.argtypes = [vp]
    lib.fpic_build_arch.restype = ctypes.c_char_p
    lib.fpic_create.argtypes = [ctypes.POINTER(Spec), ctypes.POINTER(vp)]
    lib.fpic_destroy.argtypes = [vp]
    lib.fpic_set_particles.argtypes = [vp, vp, vp, ctypes.c_uint64, ci]
    lib.fpic_set_grid.argtypes = [vp, ci, vp, ci, ci, ci, ci]
    lib.fpic_set_random_state.argtypes = [vp, vp, vp]
    lib.fpic_add_current_loop.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    for f in ("fpic_add_current_z", "fpic_add_bz", "fpic_add_btheta"):
        getattr(lib, f).argtypes = [vp, ctypes.c_double]
    for f in ("fpic_precalc", "fpic_density", "fpic_deposit", "fpic_density_finish", "fpic_sort", "fpic_sync",
              "fpic_reset_stats"):
        getattr(lib, f).argtypes = [vp]
    lib.fpic_density_finish_from.argtypes = [vp, vp, vp]
    lib.fpic_step.argtypes = [vp, ci]
    lib.fpic_substeps.argtypes = [vp, ci]
    lib.fpic_profile.argtypes = [vp, ci]
    lib.fpic_read_grid.argtypes = [vp, ci, vp, ci]
    lib.fpic_get_particles.argtypes = [vp, vp, vp, vp, vp, ci]
    lib.fpic_get_cells.argtypes = [vp, vp]
    lib.fpic_device_buffer.argtypes = [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    lib.fpic_set_stream.argtypes = [vp, vp]
    lib.fpic_get_stream.argtypes = [vp, ctypes.POINTER(vp)]
    lib.fpic_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    lib.fpic_get_substep_counter.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_set_substep_counter.argtypes = [vp, ctypes.c_uint64]
    lib.fpic_save_checkpoint.argtypes = [vp, ctypes.c_char_p]
    lib.fpic_load_checkpoint.argtypes = [vp, ctypes.c_char_p]
    lib.fpic_comm_unique_id.argtypes = [vp]
    lib.fpic_comm_init.argtypes = [vp, vp, ci, ci]
    lib.fpic_comm_destroy.argtypes = [vp]
    lib.fpic_comm_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ci)]
    lib.fpic_comm_set_overlap.argtypes = [vp, ci]
    lib.fpic_domain_init.argtypes = [vp, ci, ci, ci, ci, ci]
    lib.fpic_domain_set_particles.argtypes = [vp, ci, ctypes.c_uint64, vp, vp, ctypes.c_uint32, ci]
    lib.fpic_domain_get_particles.argtypes = [vp, ci, vp, vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ci]
    lib.fpic_domain_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_group_precalc.argtypes = [ctypes.POINTER(vp), ci]
    lib.fpic_group_step.argtypes = [ctypes.POINTER(vp), ci, ci]
    lib.fpic_group_density.argtypes = [ctypes.POINTER(vp), ci]
    lib.fpic_add_species.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_uint64, ctypes.POINTER(ci)]
    lib.fpic_set_particles_of.argtypes = [vp, ci, vp, vp, ctypes.c_uint64, ci]
    lib.fpic_get_particles_of.argtypes = [vp, ci, vp, vp, ci]
    lib.fpic_set_particles_range.argtypes = [vp, ci, ctypes.c_uint64, ctypes.c_uint64, vp, vp, ci]
    lib.fpic_get_cells_of.argtypes = [vp, ci, vp]
    lib.fpic_get_particles_range.argtypes = [vp, ci, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, vp, vp, ci]
    lib.fpic_get_cells_range.argtypes = [vp, ci, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, vp]
    lib.fpic_add_b.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    lib.fpic_set_field3.argtypes = [vp, ci, vp, ci, ci, ci, ci]
    lib.fpic_read_field3.argtypes = [vp, ci, vp, ci]
    lib.fpic_energy_now.argtypes = [vp, ci, ctypes.POINTER(Energy)]
    lib.fpic_energy_record.argtypes = [vp, ci, ctypes.c_uint32]
    lib.fpic_energy_history.argtypes = [vp, ci, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_histogram.argtypes = [vp, ctypes.POINTER(HistSpec), ci, vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_moments.argtypes = [vp, ctypes.POINTER(MomentsSpec), ci, vp, ctypes.POINTER(MomentsInfo)]
    lib.fpic_series_now.argtypes = [vp, ctypes.POINTER(SeriesSpec), ci, vp, vp]
    lib.fpic_series_record.argtypes = [vp, ctypes.POINTER(SeriesSpec), ci, ctypes.c_uint32]
    lib.fpic_series_history.argtypes = [vp, ci, vp, vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_modes_now.argtypes = [vp, ctypes.POINTER(ModesSpec), ci, vp]
    lib.fpic_modes_record.argtypes = [vp, ctypes.POINTER(ModesSpec), ci, ctypes.c_uint32]
    lib.fpic_modes_history.argtypes = [vp, ci, vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_select.argtypes = [vp, ctypes.POINTER(SelectSpec), ci, ctypes.c_uint64, vp, vp, vp, ci, ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_load.argtypes = [vp, ctypes.POINTER(LoadSpec), ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_load_profile.argtypes = [vp, ctypes.POINTER(LoadSpec), ctypes.POINTER(LoadProfile), ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_load_radial.argtypes = [vp, ctypes.POINTER(LoadSpec), ctypes.POINTER(LoadRadial), ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_collide.argtypes = [vp, ctypes.POINTER(CollideSpec), ctypes.POINTER(CollideResult)]
    lib.fpic_collide_register.argtypes = [vp, ctypes.POINTER(CollideSpec), ci, ctypes.POINTER(ctypes.c_int)]
    lib.fpic_collide_stats.argtypes = [vp, ci, ci, ctypes.POINTER(CollideResult)]
    lib.fpic_collide_clear.argtypes = [vp]
    lib.fpic_force.argtypes = [vp, ctypes.POINTER(ForceSpec), ctypes.POINTER(ForceResult)]
    lib.fpic_force_register.argtypes = [vp, ctypes.POINTER(ForceSpec), ctypes.POINTER(ctypes.c_int)]
    lib.fpic_force_stats.argtypes = [vp, ci, ci, ctypes.POINTER(ForceResult)]
    lib.fpic_force_clear.argtypes = [vp]
    lib.fpic_gas.argtypes = [vp, ctypes.POINTER(GasSpec), ctypes.POINTER(GasResult)]
    lib.fpic_gas_register.argtypes = [vp, ctypes.POINTER(GasSpec), ci, ctypes.POINTER(ctypes.c_int)]
    lib.fpic_gas_stats.argtypes = [vp, ci, ci, ctypes.POINTER(GasResult)]
    lib.fpic_gas_clear.argtypes = [vp]
    lib.fpic_remove.argtypes = [vp, ctypes.POINTER(RemoveSpec), ctypes.POINTER(RemoveResult)]
    lib.fpic_remove_register.argtypes = [vp, ctypes.POINTER(RemoveSpec), ci, ctypes.POINTER(ctypes.c_int)]
    lib.fpic_remove_stats.argtypes = [vp, ci, ci, ctypes.POINTER(RemoveResult)]
    lib.fpic_remove_clear.argtypes = [vp]
    lib.fpic_renumber.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_reserve.argtypes = [vp, ci, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_population.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_inject.argtypes = [vp, ctypes.POINTER(InjectSpec), ctypes.POINTER(InjectResult)]
    lib.fpic_inject_register.argtypes = [vp, ctypes.POINTER(InjectSpec), ci, ctypes.POINTER(ctypes.c_int)]
    lib.fpic_inject_stats.argtypes = [vp, ci, ci, ctypes.POINTER(InjectResult)]
    lib.fpic_inject_clear.argtypes = [vp]
    lib.fpic_ionize.argtypes = [vp, ctypes.POINTER(IonizeSpec), ctypes.POINTER(IonizeResult)]
    lib.fpic_ionize_register.argtypes = [vp, ctypes.POINTER(IonizeSpec), ci, ctypes.POINTER(ctypes.c_int)]
    lib.fpic_ionize_stats.argtypes = [vp, ci, ci, ctypes.POINTER(IonizeResult)]
    lib.fpic_ionize_clear.argtypes = [vp]
    lib.fpic_burn.argtypes = [vp, ctypes.POINTER(BurnSpec), ctypes.POINTER(BurnResult)]
    lib.fpic_burn_register.argtypes = [vp, ctypes.POINTER(BurnSpec), ci, ctypes.POINTER(ctypes.c_int)]
    lib.fpic_burn_stats.argtypes = [vp, ci, ci, ctypes.POINTER(BurnResult)]
    lib.fpic_burn_clear.argtypes = [vp]
    lib.fpic_pair.argtypes = [vp, ctypes.POINTER(PairSpec), ctypes.POINTER(PairResult)]
    lib.fpic_pair_register.argtypes = [vp, ctypes.POINTER(PairSpec), ci, ctypes.POINTER(ctypes.c_int)]
    lib.fpic_pair_stats.argtypes = [vp, ci, ci, ctypes.POINTER(PairResult)]
    lib.fpic_pair_clear.argtypes = [vp]
    lib.fpic_fusion.argtypes = [vp, ctypes.POINTER(FusionSpec), ctypes.POINTER(FusionResult), ctypes.POINTER(ctypes.c_int64)]
    lib.fpic_fusion_register.argtypes = [vp, ctypes.POINTER(FusionSpec), ci, ctypes.POINTER(ctypes.c_int)]
    lib.fpic_fusion_stats.argtypes = [vp, ci, ci, ctypes.POINTER(FusionResult)]
    lib.fpic_fusion_grid.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_int64), ci]
    lib.fpic_fusion_clear.argtypes = [vp]
    lib.fpic_fusion_spectrum.argtypes = [vp, ctypes.POINTER(FusionSpectrumSpec), ctypes.POINTER(FusionResult), ctypes.POINTER(ctypes.c_uint64)]
    lib.fpic_fusion_spectrum_register.argtypes = [vp, ctypes.POINTER(FusionSpectrumSpec), ci, ctypes.POINTER(ctypes.c_int)]
    lib.fpic_fusion_spectrum_read.argtypes = [vp, ci, ctypes.POINTER(FusionResult), ctypes.POINTER(ctypes.c_uint64), ci]
    lib.fpic_fusion_spectrum_clear.argtypes = [vp]
    if path == LIB_PATH:
        _lib = lib
    return lib


_SPEC_KEYS = ("radius", "height", "nr", "nz", "dt", "nparticles", "particle_mass", "particle_charge")


def _validate_spec(spec):
    """validate_object(spec, {...: 'number'}) (empic.js:31-41, utilities.js:11-127)."""
    for key in _SPEC_KEYS:
        if key not in spec or spec[key] is None:
            raise FusionPicError(-1, "." + key + " <- Non-optional property is undefined!")
        if isinstance(spec[key], bool) or not isinstance(spec[key], (int, float, np.integer, np.floating)):
            raise FusionPicError(-1, "." + key + " <- Property does not match any given possible types!")


def _np_dtype(code):
    return np.float32 if code == F32 else np.float64


def _code(arr):
    return F32 if arr.dtype == np.float32 else F64


def _as_float_array(a):
    a = np.asarray(a)
    if a.dtype != np.float32:
        a = a.astype(np.float64, copy=False)  # JavaScript numbers are doubles
    return np.ascontiguousarray(a)


class _Buffer:
    """pointer + shape + element code of an [n][3] array the library reads: a numpy array, or device memory
    (a tensor with data_ptr(), e.g. torch on the GPU) for the entry points that copy with hipMemcpyDefault"""

    def __init__(self, ptr, shape, code, keep):
        self.ptr, self.shape, self.code, self.keep = ptr, tuple(shape), code, keep


def _device_or_host(a):
    if hasattr(a, "data_ptr") and hasattr(a, "is_contiguous"):
        name = str(a.dtype)
        if not a.is_contiguous() or not (name.endswith("float32") or name.endswith("float64")):
            raise FusionPicError(-1, ".position <- a device tensor must be contiguous float32 or float64")
        return _Buffer(a.data_ptr(), a.shape, F32 if name.endswith("float32") else F64, a)
    h = _as_float_array(a)
    return _Buffer(h.ctypes.data, h.shape, _code(h), h)


class CylindricalParticlePusher:
    """Object returned by makeCylindricalParticlePusher (empic.js:1528)."""

    def __init__(self, spec, precision="fp32", device=0, count=0, compat=True, sort_interval=0, fuse_deposit=True,
                 rng="reference", seed=0, library=None, shape="ref11", raster_subpixel_bits=0, bin_lookahead=0):
        _validate_spec(spec)
        self._lib = library or load_library()
        self.spec = dict(spec)
        s = Spec()
        for key in _SPEC_KEYS:
            setattr(s, key, spec[key])
        s.count = int(count)
        s.precision = {"fp32": F32, "fp64": F64}[precision]
        s.device = int(device)
        s.physical_a = 0 if compat else 1
        s.sort_interval = int(sort_interval)
        # True: sums, census and re-binning inside the push; False: separate passes; "census": the push
        # keeps the census and the re-binning, the per-cell sums are a separate pass
        s.unfused_deposit = 2 if fuse_deposit == "census" else (0 if fuse_deposit else 1)
        s.rng_mode = {"reference": 0, "counter": 1}[rng]
        s.shape = {"ref11": 0, "cic": 1}[spec.get("shape", shape)]   # SURVEY 8(b) extension key
        # density()'s point sprites as a rasteriser with that many sub-pixel bits draws them (0 / absent: ideal sprites)
        s.raster_subpixel_bits = int(spec.get("raster_subpixel_bits", raster_subpixel_bits))
        s.rng_seed_lo, s.rng_seed_hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        # sub-steps the re-binning looks ahead along the velocity (0: adaptive with sort_interval=0, else none; -1: off; k: fixed)
        s.bin_lookahead = int(bin_lookahead)
        self.precision = s.precision
        self.nr, self.nz = int(spec["nr"]), int(spec["nz"])
        self.n = int(count) if count else int(spec["nparticles"]) ** 2
        h = ctypes.c_void_p()
        rc = self._lib.fpic_create(ctypes.byref(s), ctypes.byref(h))
        if rc != 0:
            raise FusionPicError(rc, self._lib.fpic_last_error(None).decode())
        self._h = h

    # ---- plumbing
    def _check(self, rc):
        if rc != 0:
            raise FusionPicError(rc, self._lib.fpic_last_error(self._h).decode())

    def destroy(self):
        if getattr(self, "_h", None):
            self._lib.fpic_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # ---- reference surface
    def set(self, value=None, **kw):
        """out.set({E, B, position, velocity, sink_mask, source_pdf}) (empic.js:1157-1350)."""
        value = dict(value or {}, **kw)
        for key, which, ncomp in (("E", GRID_E, 3), ("B", GRID_B, 3)):
            if value.get(key) is not None:
                a = _as_float_array(value[key])
                if a.shape != (self.nr, self.nz, 3):
                    raise FusionPicError(-1, ".%s <- expected [%d][%d][3]" % (key, self.nr, self.nz))
                self._check(self._lib.fpic_set_grid(self._h, which, a.ctypes.data, self.nr, self.nz, ncomp, _code(a)))
        pos = value.get("position")
        vel = value.get("velocity")
        for key, arr in (("position", pos), ("velocity", vel)):
            if arr is not None:
                a = _as_float_array(arr)
                if a.shape != (self.n, 3):
                    raise FusionPicError(-1, ".%s <- expected [%d][3]" % (key, self.n))
                p = a.ctypes.data if key == "position" else None
                v = a.ctypes.data if key == "velocity" else None
                self._check(self._lib.fpic_set_particles(self._h, p, v, self.n, _code(a)))
        for key, which in (("sink_mask", GRID_SINK_MASK), ("source_pdf", GRID_SOURCE_PDF)):
            if value.get(key) is not None:
                a = _as_float_array(value[key])
                if a.shape != (self.nr, self.nz):
                    raise FusionPicError(-1, ".%s <- expected [%d][%d]" % (key, self.nr, self.nz))
                self._check(self._lib.fpic_set_grid(self._h, which, a.ctypes.data, self.nr, self.nz, 1, _code(a)))

    def addCurrentLoop(self, r, z, current):
        self._check(self._lib.fpic_add_current_loop(self._h, r, z, current))

    def addCurrentZ(self, current):
        self._check(self._lib.fpic_add_current_z(self._h, current))

    def addBZ(self, bz):
        self._check(self._lib.fpic_add_bz(self._h, bz))

    def addBTheta(self, btheta):
        self._check(self._lib.fpic_add_btheta(self._h, btheta))

    def addSpindleCuspPlasmaField(self, r, B_c, beta_c=None):
        """The reference's version is unfinished and has no effect on B (empic.js:1369-1378,
        spindle.js:328, :624, :643 use undefined symbols)."""
        raise FusionPicError(-5, "addSpindleCuspPlasmaField is not functional in the reference (spindle.js:328)")

    def precalc(self):
        self._check(self._lib.fpic_precalc(self._h))

    def step(self, ncalls=1):
        """One call = two leap-frog sub-steps, dt fixed at construction (empic.js:1436-1469)."""
        self._check(self._lib.fpic_step(self._h, int(ncalls)))

    def substeps(self, nsub):
        """nsub single leap-frog sub-steps: step(n) == substeps(2 n) (diagnostics that need the state between the halves)"""
        self._check(self._lib.fpic_substeps(self._h, int(nsub)))

    def density(self):
        self._check(self._lib.fpic_density(self._h))

    # ---- extensions the boundary needs because `canvas` cannot exist off-browser
    def deposit(self):
        self._check(self._lib.fpic_deposit(self._h))

    def densityFinish(self):
        self._check(self._lib.fpic_density_finish(self._h))

    def densityFinishFrom(self, sums_ptr, stream=None):
        """finish stage from a caller's copy of the per-cell sums, on a caller's stream (multi-GPU overlap)"""
        self._check(self._lib.fpic_density_finish_from(self._h, ctypes.c_void_p(sums_ptr), ctypes.c_void_p(stream or 0)))

    def setRandomState(self, entropy=None, rand=None):
        e = r = None
        if entropy is not None:
            e = np.ascontiguousarray(entropy, dtype=np.float32).ravel()
            if e.size != 4 * 1024 * 1024:
                raise FusionPicError(-1, ".entropy <- expected 1024*1024*4 floats")
        if rand is not None:
            r = np.ascontiguousarray(rand, dtype=np.float32).ravel()
            if r.size != 4 * self.n:
                raise FusionPicError(-1, ".rand <- expected %d*4 floats" % self.n)
        self._check(self._lib.fpic_set_random_state(self._h, e.ctypes.data if e is not None else None,
                                                    r.ctypes.data if r is not None else None))

    def readGrid(self, which, dtype=None):
        code = self.precision if dtype is None else (F32 if np.dtype(dtype) == np.float32 else F64)
        cells = 512 * 512 if which == READ_INV_CDF else self.nr * self.nz
        out = np.empty(4 * cells, dtype=_np_dtype(code))
        self._check(self._lib.fpic_read_grid(self._h, which, out.ctypes.data, code))
        return out

    def readDensity(self, dtype=None):
        """moments01_avgA, channels (v_r, v_theta, v_z, n), index 4*(i + j*nr) (empic.js:1071)."""
        return self.readGrid(READ_AVG, dtype)

    def readMoments(self, dtype=None):
        return self.readGrid(READ_MOMENTS, dtype)

    def getParticles(self, dtype=None, position=True, velocity=True, rand=True, alive=True):
        code = self.precision if dtype is None else (F32 if np.dtype(dtype) == np.float32 else F64)
        dt = _np_dtype(code)
        out = {}
        if position:
            out["position"] = np.empty((self.n, 3), dtype=dt)
        if velocity:
            out["velocity"] = np.empty((self.n, 3), dtype=dt)
        if rand:
            out["rand"] = np.empty((self.n, 4), dtype=np.float32)
        if alive:
            out["alive"] = np.empty(self.n, dtype=np.uint8)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        self._check(self._lib.fpic_get_particles(self._h, ptr("position"), ptr("velocity"), ptr("rand"), ptr("alive"), code))
        return out

    def getCells(self):
        out = np.empty(self.n, dtype=np.int32)
        self._check(self._lib.fpic_get_cells(self._h, out.ctypes.data))
        return out

    def deviceBuffer(self, which=BUF_CELL_SUMS):
        p, nbytes = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._lib.fpic_device_buffer(self._h, which, ctypes.byref(p), ctypes.byref(nbytes)))
        return p.value, nbytes.value

    def setStream(self, stream_ptr):
        self._check(self._lib.fpic_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def substepCounter(self):
        t = ctypes.c_uint64()
        self._check(self._lib.fpic_get_substep_counter(self._h, ctypes.byref(t)))
        return t.value

    def setSubstepCounter(self, t):
        self._check(self._lib.fpic_set_substep_counter(self._h, int(t)))

    def saveCheckpoint(self, path):
        self._check(self._lib.fpic_save_checkpoint(self._h, os.fsencode(path)))

    def loadCheckpoint(self, path):
        self._check(self._lib.fpic_load_checkpoint(self._h, os.fsencode(path)))

    def sort(self):
        self._check(self._lib.fpic_sort(self._h))

    # ---- multi-GPU: the library's own RCCL communicator (include/fusionpic.h, fpic_comm_*)
    def commInit(self, unique_id, rank, world, overlap=True):
        """unique_id: the 128 bytes rank 0 obtained from commUniqueId(), handed to every rank by the host"""
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        self._check(self._lib.fpic_comm_init(self._h, buf, int(rank), int(world)))
        self._check(self._lib.fpic_comm_set_overlap(self._h, 1 if overlap else 0))

    def commDestroy(self):
        self._check(self._lib.fpic_comm_destroy(self._h))

    def commInfo(self):
        r, w = ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.fpic_comm_info(self._h, ctypes.byref(r), ctypes.byref(w)))
        return r.value, w.value

    def histogram(self, axes, bins, range, species=0, scope="global"):
        """Phase-space histogram of one species of a CART3D box, reduced on the device (fpic_histogram; an (r,z) handle is
        refused).  axes: a name or a pair of names from x y z vx vy vz v2 (stored values: positions as fractions of the box,
        velocities in units of c); bins: an int or a pair; range: (lo, hi) or a pair of them.  Returns {counts: uint64 array
        of shape (bins0,) or (bins0, bins1), outside: the live particles in no bin, edges: the bin edges per axis}.  'global'
        on a rank with a communicator is collective; on a member of an in-process group it is an error (BoxGroup.histogram)."""
        s, shape, rg = _hist_spec(axes, bins, range, species)
        counts, outside = _hist_call(self, s, shape, scope)
        return _hist_result(counts, outside, shape, rg)

    # ---- selection: the particles in a window of phase space, filtered and compacted on the device (fpic_select)
    def select(self, where=None, species=0, every=None, capacity=None, scope="global", dtype=None):
        """The live particles of one species of a CART3D box that lie in a window of phase space (fpic_select; an (r,z)
        handle is refused).  where: {axis: (lo, hi)} with names from x y z vx vy vz v2 (stored values: positions as fractions
        of the box, velocities in units of c), each a half-open interval lo <= q < hi, None for the infinite side; an empty
        or absent `where` takes every live particle.  every: (mod, rem) keeps only ids with id % mod == rem — the same
        particles at every time.  capacity None asks for the count first and then fetches; a given capacity that is too
        small returns None arrays.  Returns {ids: uint32 (matched,), position, velocity: (matched, 3), matched}, in ascending
        id.  'global' on a rank with a communicator is collective; on a member of an in-process group it is an error
        (BoxGroup.select)."""
        return _select_call(self, _select_spec(where, species, every), capacity, scope, dtype)

    def count(self, where=None, species=0, every=None, scope="global"):
        """how many particles select() would return (the count query of fpic_select: nothing is delivered)"""
        return _select_count(self, _select_spec(where, species, every), scope)

    # ---- absorbing sinks: the particles a predicate names leave the species, exactly accounted for (fpic_remove*)
    def remove(self, where=None, species=0, every=None, outside=False):
        """Removes, now, the live particles of one species of a CART3D box that select(where, species, every) would return
        (fpic_remove; an (r,z) handle and a decomposed handle are refused) — with outside=True those that pass `every` and
        do NOT lie in the window (the window is a brick: outside=True keeps the interior).  Survivors keep their state, their
        id and their order.  Returns {applications, scanned, removed, energy_fixed, momentum_fixed (exact integers, units of
        2^-80 of c^2 resp. c), energy (J), momentum (kg m/s), charge (C)}: what the species lost.  A species that has lost
        particles is thinned: read it with select(); getParticles, set, load and saveCheckpoint are refused until
        renumber().  With the electrostatic solver the call re-deposits and re-solves; under full EM the fields stay."""
        s = _remove_spec(where, species, every, outside)
        out = RemoveResult()
        self._check(self._lib.fpic_remove(self._h, ctypes.byref(s), ctypes.byref(out)))
        return _remove_dict(out)

    def removeEvery(self, period, where=None, species=0, every=None, outside=False):
        """Registers a sink (see remove) to run at the end of every `period`-th sub-step, after the fusion tallies and
        before the recorders.  Each due application waits for one 8-byte count from the device.  Returns the operator's
        index (fpic_remove_register)."""
        period = _every_arg(period)
        s = _remove_spec(where, species, every, outside)
        index = ctypes.c_int()
        self._check(self._lib.fpic_remove_register(self._h, ctypes.byref(s), period, ctypes.byref(index)))
        return index.value

    def removeStats(self, index, scope="global"):
        """the totals of a registered sink since its registration (fpic_remove_stats)"""
        out = RemoveResult()
        self._check(self._lib.fpic_remove_stats(self._h, int(index), _scope_code(scope), ctypes.byref(out)))
        return _remove_dict(out)

    def clearRemovals(self):
        """drops every registered sink (fpic_remove_clear)"""
        self._check(self._lib.fpic_remove_clear(self._h))

    def renumber(self, species=0):
        """Gives the survivors of a thinned species the ids 0 .. n-1 in ascending old id (fpic_renumber) and returns n; the
        caller-order calls and the checkpoint then work on the n survivors.  A no-op on a species that is not thinned."""
        n = ctypes.c_uint64()
        self._check(self._lib.fpic_renumber(self._h, int(species), ctypes.byref(n)))
        if hasattr(self, "counts"):
            self.counts[int(species)] = int(n.value)
        if int(species) == 0:
            self.n = int(n.value)
        return int(n.value)

    # ---- particle sources: a species gains particles generated on the device, exactly accounted for (fpic_inject*, fpic_reserve)
    def population(self, species=0):
        """{n, capacity, id_span} of one species now (fpic_population): the live particles, the particles its arrays hold
        (reserve() raises it) and one past the largest id it can hold.  Also refreshes the wrapper's own count, which a
        registered source or sink changes behind its back."""
        n, cap, span = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.fpic_population(self._h, int(species), ctypes.byref(n), ctypes.byref(cap), ctypes.byref(span)))
        if hasattr(self, "counts") and 0 <= int(species) < len(self.counts):
            self.counts[int(species)] = int(n.value)
        if int(species) == 0:
            self.n = int(n.value)
        return {"n": int(n.value), "capacity": int(cap.value), "id_span": int(span.value)}

    def reserve(self, species, capacity):
        """Raises the capacity of one species of a CART3D box to at least `capacity` particles (fpic_reserve) and returns the
        capacity it has now; a smaller request changes nothing.  Every particle keeps its bits, its id and its slot."""
        out = ctypes.c_uint64()
        self._check(self._lib.fpic_reserve(self._h, int(species), int(capacity), ctypes.byref(out)))
        return int(out.value)

    def inject(self, kind="volume", **request):
        """Adds, now, `count` particles to one species of a CART3D box (fpic_inject; an (r,z) handle and a decomposed handle
        are refused), generated on the device by load()'s rule from the sequence numbers first .. first + count - 1:
        kind="volume" — uniform in [lo, hi) or on the lattice, a drifting Maxwellian (species=, count=, first=, seed=,
        stream=, lo=, hi=, drift=, vth=, lattice=, paired=, mode=, xamp=, xphase=, vamp=, vphase= as load() takes them) — or
        kind="flux" — emission through the plane x[axis] = plane (metres) towards side = +1 / -1 with the flux-weighted
        half-Maxwellian of vth[axis].  The new particles take the ids after the species' id span and the slots after its
        particles; reserve() makes the room.  epoch= counts applications made before (a resumed registration).  Returns
        {applications, injected, energy_fixed, momentum_fixed (exact integers, units of 2**-80), energy (J), momentum
        (kg m/s), charge (C)}: what the species gained.  With the electrostatic solver the call re-deposits and re-solves;
        under full EM the fields stay (inject a neutral pair on one seed, stream and sequence)."""
        s = _inject_spec(self._box_lengths(), kind, **request)
        out = InjectResult()
        self._check(self._lib.fpic_inject(self._h, ctypes.byref(s), ctypes.byref(out)))
        self.population(s.load.species)
        return _inject_dict(out)

    def injectEvery(self, period, kind="volume", **request):
        """Registers a source (see inject) to run at the end of every `period`-th sub-step, after the sinks and before the
        recorders: application k draws the sequence numbers first + (epoch + k) count + l.  Returns its index
        (fpic_inject_register).  population() reads the count a source has changed."""
        if isinstance(period, bool) or not isinstance(period, (int, np.integer)):
            raise FusionPicError(-1, ".every <- must be an integer")
        s = _inject_spec(self._box_lengths(), kind, **request)
        index = ctypes.c_int(-1)
        self._check(self._lib.fpic_inject_register(self._h, ctypes.byref(s), int(period), ctypes.byref(index)))
        return index.value

    def injectStats(self, index, scope="global"):
        """the totals of a registered source since its registration (fpic_inject_stats)"""
        out = InjectResult()
        self._check(self._lib.fpic_inject_stats(self._h, int(index), _scope_code(scope), ctypes.byref(out)))
        return _inject_dict(out)

    def clearInjections(self):
        """drops every registered source (fpic_inject_clear)"""
        self._check(self._lib.fpic_inject_clear(self._h))

    # ---- electron-impact ionisation of a background gas: an event leaves a new electron and a new ion (fpic_ionize*)
    def _ionize_refresh(self, s):
        for k in {int(s.species), int(s.electron), int(s.ion)}:
            self.population(k)

    def ionize(self, **request):
        """One application, now, of electron-impact ionisation of a background gas (fpic_ionize; an (r,z) handle and a
        decomposed handle are refused).  species= the projectile, electron= (default: the projectile species) and ion= the
        species that receive the new particles, g_threshold= (units of c) sqrt(2 E_ion / (m c^2)); density=, tau=, sigma=,
        g_lo=, g_hi= (g_lo >= g_threshold), drift=, vth=, lo=, hi=, taper=, seed=, stream=, epoch= as collideGas().  The
        targets need the room: reserve() makes it, and an application that does not fit changes nothing.  Returns
        {applications, candidates, below, above, ionised, primary, electron, ion}, each group {energy_fixed, momentum_fixed
        (exact integers, units of 2**-80), energy (J), momentum (kg m/s), charge (C)}: what the species gained."""
        s, keep = _ionize_spec(float(self.spec["dt"]), self._box_lengths(), **request)
        out = IonizeResult()
        self._check(self._lib.fpic_ionize(self._h, ctypes.byref(s), ctypes.byref(out)))
        del keep
        self._ionize_refresh(s)
        return _ionize_dict(out)

    def ionizeEvery(self, every, **request):
        """Registers an ioniser (see ionize) to run at the end of every `every`-th sub-step, last among the operators and
        before the recorders, with epoch = the sub-step number + `epoch`; tau defaults to every * dt.  Returns the ioniser's
        index (fpic_ionize_register).  population() reads the counts it has changed."""
        every = _every_arg(every)
        s, keep = _ionize_spec(every * float(self.spec["dt"]), self._box_lengths(), **request)
        index = ctypes.c_int(-1)
        self._check(self._lib.fpic_ionize_register(self._h, ctypes.byref(s), every, ctypes.byref(index)))
        del keep
        return index.value

    def ionizeStats(self, index, scope="global"):
        """the totals of a registered ioniser since its registration (fpic_ionize_stats)"""
        out = IonizeResult()
        self._check(self._lib.fpic_ionize_stats(self._h, int(index), _scope_code(scope), ctypes.byref(out)))
        return _ionize_dict(out)

    def clearIonization(self):
        """drops every registered ioniser (fpic_ionize_clear); other operators stay"""
        self._check(self._lib.fpic_ionize_clear(self._h))

    # ---- fusion burn: the pairs of the yield tally react — reactants consumed, products born (fpic_burn*)
    def _burn_refresh(self, s):
        for k in {int(s.species_a), int(s.species_b), int(s.product_a), int(s.product_b)} - {-1}:
            self.population(k)

    def burn(self, a=0, b=None, **request):
        """One application, now, of fusion burn between species a and species b of a CART3D box (b None or b == a: a species
        with itself; fpic_burn; an (r,z) handle and a decomposed handle are refused).  The pairs, the table and the yield y
        of a pair are fusionYield()'s; a pair reacts with the probability y / macro_weight, a particle at most once.  Both
        reactants leave their species as remove() takes a particle out (the species is thinned), and one new particle each
        is born in products=(p3, p4) with fusionSpectrum()'s product kinematics: q_value= (J), isotropic emission; p4 None:
        the fourth particle leaves the box and other_mass= (kg) is its mass.  sigma=, g_lo=, g_hi=, tau=, seed=, stream=,
        epoch= as fusionYield().  The products need the room: reserve() makes it, and an application that does not fit
        changes nothing.  Returns {applications, pairs, below, above, cells, overfull_cells, overfull_particles, accepted,
        blocked, saturated, burnt, reactant_a, reactant_b, product_a, product_b}, each group {energy_fixed, momentum_fixed
        (exact integers, units of 2**-80), energy (J), momentum (kg m/s), charge (C)}: what the reactants lost and the
        products gained."""
        s = _burn_spec(float(self.spec["dt"]), a, b, **request)
        out = BurnResult()
        self._check(self._lib.fpic_burn(self._h, ctypes.byref(s), ctypes.byref(out)))
        self._burn_refresh(s)
        return _burn_dict(out)

    def burnEvery(self, every, a=0, b=None, **request):
        """Registers a burner (see burn) to run at the end of every `every`-th sub-step, after the ionisers and before the
        recorders, with epoch = the sub-step number + `epoch`; tau defaults to every * dt.  The table is copied.  Returns
        the burner's index (fpic_burn_register); at most BURN_MAX_OPS.  population() reads the counts it has changed."""
        every = _every_arg(every)
        s = _burn_spec(every * float(self.spec["dt"]), a, b, **request)
        index = ctypes.c_int(-1)
        self._check(self._lib.fpic_burn_register(self._h, ctypes.byref(s), every, ctypes.byref(index)))
        return index.value

    def burnStats(self, index, scope="global"):
        """the totals of a registered burner since its registration (fpic_burn_stats)"""
        out = BurnResult()
        self._check(self._lib.fpic_burn_stats(self._h, int(index), _scope_code(scope), ctypes.byref(out)))
        return _burn_dict(out)

    def clearBurn(self):
        """drops every registered burner (fpic_burn_clear); other operators stay"""
        self._check(self._lib.fpic_burn_clear(self._h))

    # ---- the loader: a population generated on the device (fpic_load)
    def _box_lengths(self):
        return [float(self.spec.get(k, 1.0)) for k in ("radius", "length_y", "height")]

    def load(self, species=0, first=0, count=None, seed=LOAD_SEED, stream=0, lo=None, hi=None, drift=0, vth=0, mode=None, xamp=0, xphase=0,
             vamp=0, vphase=0, lattice=False, paired=False, position=True, velocity=True, append=False, density=None, thermal=None, shear=None,
             radial=None):
        """Particles [first, first + count) of one species of a CART3D box generated on the device (fpic_load; an (r,z)
        handle is refused): in the sub-box [lo, hi) (metres; random, or a Kronecker lattice with lattice=True) with a
        uniform density or a tabulated one, a drifting Maxwellian (drift, vth in units of c; paired=True makes the thermal
        parts of particles 2k and 2k + 1 exact negatives), and a sinusoidal perturbation of the integer mode vector `mode`:
        a displacement xamp (metres) and a velocity vamp (c) times sinpi(2 (theta + phase)), phases in turns.  Scalars
        broadcast to three components.  The state of a particle depends on the request and its index alone — not on the
        precision, the decomposition or the time of the call; two species loaded with one seed and stream coincide.
        position / velocity choose what is written.  On a rank of a decomposition the rank keeps the particles of its
        planes (count is needed; append=True adds to what it holds).  Returns the number of particles written (kept).

        Profiles (fpic_load_profile): tables of 2 .. LOAD_TABLE_MAX nodes, uniformly spaced over [lo, hi] on their axis and
        linear between the nodes; the profile is the product of its axes' tables.  density = (x, y, z), each None (uniform)
        or a table of values >= 0: the positions follow it (a lattice load becomes a quiet start on the profile).  thermal
        = (x, y, z), each None or a table of factors >= 0 that multiply vth at the particle's undisplaced position.  shear =
        dict(axis=, component=, values=): drift[component] += table(position along axis).  With all three None the call
        is fpic_load itself.

        Radial bodies (fpic_load_radial): radial = dict(geometry="sphere" | "cylinder", center=(x, y, z), r_max= (metres),
        axis=0 (the cylinder's), density=, thermal=, flow_radial=, flow_azimuthal=, flow_axial=): tables of 2 ..
        LOAD_TABLE_MAX nodes over [0, r_max], linear between the nodes.  The particles fill the ball (the column over
        [lo, hi] of its axis) with that density (None: uniform in the volume); thermal multiplies vth; the flows (units of
        c) add to the drift along the radius, about the axis and along it (the last two: the cylinder only).  A body that
        reaches across the periodic boundary wraps.  radial= does not combine with density=, thermal= or shear=
        (ValueError)."""
        s = _load_spec(self._box_lengths(), species, first, count, seed, stream, lo, hi, drift, vth, mode, xamp, xphase,
                       vamp, vphase, lattice, paired, position, velocity, append)
        if radial is not None:
            if density is not None or thermal is not None or shear is not None:
                raise ValueError("load(): radial= does not combine with density=, thermal= or shear=")
            return _load_call(self, s, radial=_load_radial(radial))
        return _load_call(self, s, _load_profile(density, thermal, shear))

    # ---- Monte Carlo collisions with a prescribed background (fpic_collide*)
    def collide(self, kind, **request):
        """One application, now, of a collision operator to the stored velocities of one species of a CART3D box
        (fpic_collide; an (r,z) handle is refused).  kind: "exchange" (charge exchange: the velocity becomes the partner's),
        "elastic" (isotropic scattering in the centre-of-mass frame, mass_ratio = m_background / m_species) or "relax" (the
        exact Ornstein-Uhlenbeck step of the Lenard-Bernstein operator: a thermostat).  The background is a drifting
        Maxwellian (drift, vth in units of c; scalars broadcast).  Rates: nu (1/s), sigma_n (density times cross-section,
        1/m) and tau (s, default the sub-step dt), or the dimensionless nu_tau and sigma_tau; with sigma_tau > 0 give g_max,
        the bound of the relative speed (c) of the null-collision method.  seed, stream, epoch: the counter of the random
        words — particle i of a request and epoch always draws the same.  Returns {applications, candidates, collided,
        clipped}."""
        s = _collide_spec(float(self.spec["dt"]), kind, **request)
        out = CollideResult()
        self._check(self._lib.fpic_collide(self._h, ctypes.byref(s), ctypes.byref(out)))
        return _collide_counts(out)

    def collideEvery(self, every, kind=None, **request):
        """Registers a collision operator (see collide) to run at the end of every `every`-th sub-step, with epoch = the
        sub-step number + `epoch`; tau defaults to every * dt.  Returns the operator's index (fpic_collide_register)."""
        if kind is None:
            raise FusionPicError(-1, ".kind <- Non-optional property is undefined!")
        every = _every_arg(every)
        s = _collide_spec(every * float(self.spec["dt"]), kind, **request)
        index = ctypes.c_int(-1)
        self._check(self._lib.fpic_collide_register(self._h, ctypes.byref(s), every, ctypes.byref(index)))
        return index.value

    def collisionStats(self, index, scope="global"):
        """the totals of a registered operator since its registration (fpic_collide_stats); 'global' on a rank with a
        communicator sums the ranks' counts (collective)"""
        out = CollideResult()
        self._check(self._lib.fpic_collide_stats(self._h, int(index), _scope_code(scope), ctypes.byref(out)))
        return _collide_counts(out)

    def clearCollisions(self):
        """drops every registered collision operator (fpic_collide_clear)"""
        self._check(self._lib.fpic_collide_clear(self._h))

    # ---- prescribed external forces (fpic_force*)
    def force(self, **request):
        """Kicks the stored velocities of one species of the box with a prescribed field or acceleration, now (fpic_force; an
        (r,z) handle is refused).  waves=[dict(amp=, mode=(0, 0, 0), frequency= | nu=, phase=0)] (1 .. 4 plane waves; amp in
        V/m for kind="field", m/s^2 for kind="accel"; frequency in Hz becomes nu = frequency dt turns per sub-step),
        species=0, lo=None, hi=None (the window in metres; default the whole box), taper=(None, None, None) (per axis the
        nodes of a table over the window), envelope=None | dict(start=, stop=, values=) (active for start <= s <= stop,
        s = sub-steps since create + epoch; values: the nodes of a table over that span), epoch=0.  Returns {applications,
        kicked, work_fixed, impulse_fixed (exact integers, units of 2^-80 c^2 and c), work (J), impulse (kg m/s)}."""
        s, keep = _force_spec(float(self.spec["dt"]), self._box_lengths(), **request)
        out = ForceResult()
        self._check(self._lib.fpic_force(self._h, ctypes.byref(s), ctypes.byref(out)))
        del keep
        return _force_dict(out)

    def forceOn(self, **request):
        """Registers a force (see force) to run at the end of every sub-step at which it is active, before every other
        registered operator and every recorder.  Returns the request's index (fpic_force_register)."""
        s, keep = _force_spec(float(self.spec["dt"]), self._box_lengths(), **request)
        index = ctypes.c_int(-1)
        self._check(self._lib.fpic_force_register(self._h, ctypes.byref(s), ctypes.byref(index)))
        del keep
        return index.value

    def forceStats(self, index, scope="global"):
        """the totals of a registered force since its registration (fpic_force_stats); 'global' on a rank with a communicator
        sums the ranks' integers (collective)"""
        out = ForceResult()
        self._check(self._lib.fpic_force_stats(self._h, int(index), _scope_code(scope), ctypes.byref(out)))
        return _force_dict(out)

    def clearForces(self):
        """drops every registered force (fpic_force_clear)"""
        self._check(self._lib.fpic_force_clear(self._h))

    # ---- windowed background collisions with a tabulated cross-section (fpic_gas*)
    def collideGas(self, kind, **request):
        """One application, now, of a collision operator against a background gas that fills a window of the box
        (fpic_gas; an (r,z) handle is refused).  kind: "exchange" or "elastic", as collide().  density= (m^-3, the peak),
        tau= (s, default the sub-step dt), sigma=, g_lo=, g_hi= (the cross-section table in m^2 over the relative speed in
        units of c, as tallyFusion takes it), drift=, vth=, mass_ratio= (the background, as collide()), lo=, hi= (the
        window in metres; default the whole box), taper=(None, None, None) (per axis the nodes in [0, 1] of the density
        profile over the window), seed=, stream=, epoch=.  Returns {applications, candidates, collided, below, above,
        energy_fixed, momentum_fixed (exact integers, units of 2^-80 c^2 and c), energy (J), momentum (kg m/s)}: what the
        species gained; the reservoir took the negatives."""
        s, keep = _gas_spec(float(self.spec["dt"]), self._box_lengths(), kind, **request)
        out = GasResult()
        self._check(self._lib.fpic_gas(self._h, ctypes.byref(s), ctypes.byref(out)))
        del keep
        return _gas_dict(out)

    def collideGasEvery(self, every, kind=None, **request):
        """Registers a windowed background collision operator (see collideGas) to run at the end of every `every`-th
        sub-step, after the operators of collideEvery and before those of collidePairEvery, with epoch = the sub-step
        number + `epoch`; tau defaults to every * dt.  Returns the operator's index (fpic_gas_register)."""
        if kind is None:
            raise FusionPicError(-1, ".kind <- Non-optional property is undefined!")
        every = _every_arg(every)
        s, keep = _gas_spec(every * float(self.spec["dt"]), self._box_lengths(), kind, **request)
        index = ctypes.c_int(-1)
        self._check(self._lib.fpic_gas_register(self._h, ctypes.byref(s), every, ctypes.byref(index)))
        del keep
        return index.value

    def gasStats(self, index, scope="global"):
        """the totals of a registered operator since its registration (fpic_gas_stats); 'global' on a rank with a
        communicator sums the ranks' integers (collective)"""
        out = GasResult()
        self._check(self._lib.fpic_gas_stats(self._h, int(index), _scope_code(scope), ctypes.byref(out)))
        return _gas_dict(out)

    def clearGas(self):
        """drops every registered windowed background collision operator (fpic_gas_clear)"""
        self._check(self._lib.fpic_gas_clear(self._h))

    # ---- binary Coulomb collisions between the species of the box (fpic_pair*)
    def collidePair(self, a=0, b=None, **request):
        """One application, now, of the Takizuka-Abe binary Coulomb collision operator between species a and species b of a
        CART3D box (b None or b == a: like-particle collisions; fpic_pair; an (r,z) handle and a decomposed handle are
        refused).  The particles of every grid cell are paired at random and every pair is scattered by a small random
        angle; momentum and energy of a pair are conserved.  log_lambda: the Coulomb logarithm; tau (s, default the sub-step
        dt): the time the application stands for; seed, stream, epoch: the counter of the random words.  Returns
        {applications, pairs, strong, cells, overfull_cells, overfull_particles}: strong counts the pairs whose variance
        exceeded 1 (tau too long for small-angle theory), overfull_* the cells above PAIR_CELL_MAX particles of a species,
        which are not collided."""
        s = _pair_spec(float(self.spec["dt"]), a, b, **request)
        out = PairResult()
        self._check(self._lib.fpic_pair(self._h, ctypes.byref(s), ctypes.byref(out)))
        return _pair_counts(out)

    def collidePairEvery(self, every, a=0, b=None, **request):
        """Registers a binary collision operator (see collidePair) to run at the end of every `every`-th sub-step, after the
        operators of collideEvery and before the recorders, with epoch = the sub-step number + `epoch`; tau defaults to
        every * dt.  Returns the operator's index (fpic_pair_register)."""
        every = _every_arg(every)
        s = _pair_spec(every * float(self.spec["dt"]), a, b, **request)
        index = ctypes.c_int(-1)
        self._check(self._lib.fpic_pair_register(self._h, ctypes.byref(s), every, ctypes.byref(index)))
        return index.value

    def pairStats(self, index, scope="global"):
        """the totals of a registered binary collision operator since its registration (fpic_pair_stats)"""
        out = PairResult()
        self._check(self._lib.fpic_pair_stats(self._h, int(index), _scope_code(scope), ctypes.byref(out)))
        return _pair_counts(out)

    def clearPairs(self):
        """drops every registered binary collision operator (fpic_pair_clear); those of collideEvery stay"""
        self._check(self._lib.fpic_pair_clear(self._h))

    # ---- fusion yield tallies between the species of the box (fpic_fusion*)
    def _fusion_cells(self):
        return (int(self.spec["nz"]), int(self.spec.get("ny", 1)), int(self.spec["nr"]))

    def fusionYield(self, a=0, b=None, grid=False, **request):
        """The number of binary reactions between species a and species b of a CART3D box (b None or b == a: a species with
        itself) in the time tau, from a tabulated cross-section (fpic_fusion; an (r,z) handle and a decomposed handle are
        refused).  A tally, not a sink: no particle is changed.  sigma: the table (m^2, 2 .. 4096 entries, see sigma_table) at
        relative speeds uniform from g_lo to g_hi (units of c); tau (s, default the sub-step dt); seed, stream, epoch: the
        counter of the random pairing.  Returns {applications, pairs, below, above, cells, overfull_cells,
        overfull_particles, yield_hi, yield_lo, unit_exponent, reactions_exact, reactions}: pairs were inside the table,
        below and above outside it; reactions_exact is the exact total as a Python integer in units of 2**unit_exponent
        reactions, reactions the same as a float.  grid=True adds "grid": the (nz, ny, nx) int64 cell tallies in the same
        unit."""
        s = _fusion_spec(float(self.spec["dt"]), a, b, **request)
        out = FusionResult()
        cells = np.zeros(self._fusion_cells(), dtype=np.int64) if grid else None
        ptr = cells.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if grid else None
        self._check(self._lib.fpic_fusion(self._h, ctypes.byref(s), ctypes.byref(out), ptr))
        got = _fusion_counts(out)
        if grid:
            got["grid"] = cells
        return got

    def fusionYieldEvery(self, every, a=0, b=None, **request):
        """Registers a yield tally (see fusionYield) to run at the end of every `every`-th sub-step, after the operators of
        collidePairEvery and before the recorders, with epoch = the sub-step number + `epoch`; tau defaults to every * dt.
        The table is copied.  Returns the operator's index (fpic_fusion_register); at most FUSION_MAX_OPS."""
        every = _every_arg(every)
        s = _fusion_spec(every * float(self.spec["dt"]), a, b, **request)
        index = ctypes.c_int(-1)
        self._check(self._lib.fpic_fusion_register(self._h, ctypes.byref(s), every, ctypes.byref(index)))
        return index.value

    def fusionStats(self, index, scope="global"):
        """the totals of a registered yield tally since its registration or its last reset (fpic_fusion_stats)"""
        out = FusionResult()
        self._check(self._lib.fpic_fusion_stats(self._h, int(index), _scope_code(scope), ctypes.byref(out)))
        return _fusion_counts(out)

    def fusionGrid(self, index, reset=False):
        """the (nz, ny, nx) int64 cell tallies of a registered yield tally, in units of 2**unit_exponent reactions
        (fpic_fusion_grid); reset=True zeroes the grid, the totals and `applications` behind the copy.  A cell's word is
        exact for at least 4096 applications between two resets; nothing detects an overflow beyond that."""
        cells = np.zeros(self._fusion_cells(), dtype=np.int64)
        self._check(self._lib.fpic_fusion_grid(self._h, int(index), cells.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1 if reset else 0))
        return cells

    def clearFusion(self):
        """drops every registered yield tally (fpic_fusion_clear)"""
        self._check(self._lib.fpic_fusion_clear(self._h))

    # ---- fusion product spectra (fpic_fusion_spectrum*)
    def fusionSpectrum(self, a=0, b=None, **request):
        """The yield of fusionYield(a, b, sigma=, g_lo=, g_hi=, tau=, seed=, stream=, epoch=) distributed over an energy axis
        (fpic_fusion_spectrum; an (r,z) handle and a decomposed handle are refused).  axis="product": the laboratory energy
        of the product of mass product_mass (kg; the other product has other_mass) of a reaction that releases q_value (J),
        emitted isotropically (los None) or along the line of sight los; axis="cm": the reacting centre-of-mass energy.
        bins (1 .. 256) bins over [lo, hi) joules (KEV is one keV).  A tally: no particle is changed.  Returns the counts of
        fusionYield for the same request (reactions_exact counts every pair inside the table) and edges (bins + 1 floats, J),
        bins (exact Python integers in units of 2**unit_exponent reactions), under, over (likewise: the yield below lo and at
        or above hi) and yield (the bins as floats, reactions).  sum(bins) + under + over == reactions_exact."""
        s = _fusion_spectrum_spec(float(self.spec["dt"]), a, b, **request)
        out = FusionResult()
        words = np.zeros((max(s.bins, 0) + 2, 2), dtype=np.uint64)
        self._check(self._lib.fpic_fusion_spectrum(self._h, ctypes.byref(s), ctypes.byref(out), words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return _fusion_spectrum_result(out, words, s.lo, s.hi)

    def fusionSpectrumEvery(self, every, a=0, b=None, **request):
        """Registers a spectrum (see fusionSpectrum) to run at the end of every `every`-th sub-step, after the tallies of
        fusionYieldEvery and before the recorders, with epoch = the sub-step number + `epoch`; tau defaults to every * dt.
        The table is copied.  Returns the operator's index (fpic_fusion_spectrum_register); at most FUSION_SPECTRUM_MAX_OPS."""
        every = _every_arg(every)
        s = _fusion_spectrum_spec(every * float(self.spec["dt"]), a, b, **request)
        index = ctypes.c_int(-1)
        self._check(self._lib.fpic_fusion_spectrum_register(self._h, ctypes.byref(s), every, ctypes.byref(index)))
        if getattr(self, "_fspec_axes", None) is None:
            self._fspec_axes = {}                     # the bins and the range of the registered spectra, by index: what a read needs
        self._fspec_axes[index.value] = (s.bins, s.lo, s.hi)
        return index.value

    def fusionSpectrumRead(self, index, reset=False):
        """the totals and the spectrum of a registered operator since its registration or its last reset, as fusionSpectrum
        returns them (fpic_fusion_spectrum_read); reset=True zeroes them and `applications` behind the copy.  Exact for at
        least 2**23 applications between two resets; nothing detects an overflow beyond that."""
        # (an index that was not registered here: room for the cap, and the library refuses it)
        bins, lo, hi = (getattr(self, "_fspec_axes", None) or {}).get(int(index), (FUSION_SPECTRUM_BINS_MAX, 0.0, 1.0))
        out = FusionResult()
        words = np.zeros((bins + 2, 2), dtype=np.uint64)
        self._check(self._lib.fpic_fusion_spectrum_read(self._h, int(index), ctypes.byref(out), words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1 if reset else 0))
        return _fusion_spectrum_result(out, words, lo, hi)

    def clearFusionSpectra(self):
        """drops every registered spectrum (fpic_fusion_spectrum_clear)"""
        self._check(self._lib.fpic_fusion_spectrum_clear(self._h))
        self._fspec_axes = {}

    # ---- series: the field at points and the state of tracer particles as rows (fpic_series_*)
    def series(self, points=None, tracers=None, species=0, scope="global"):
        """The rows of the current state of a CART3D box (fpic_series_now; an (r,z) handle is refused).  points: positions in
        metres, shape (P, 3), wrapped periodically; tracers: particle indices within `species` (an int, or an array as long as
        tracers).  Returns {points: float64 (P, 8) with the columns SERIES_POINT_COLUMNS, tracers: float64 (M, 8) with
        SERIES_TRACER_COLUMNS}: the field interpolated with the charge deposit's weights from what readField(F3_E) and
        readField(F3_B_NODES) hold, and the six stored numbers of each particle.  'global' on a rank with a communicator is
        collective; on a member of an in-process group it is an error (BoxGroup.series)."""
        s, keep = _series_spec(points, tracers, species)
        pts = np.zeros((s.npoints if s.npoints <= SERIES_MAX_POINTS else 0, 8))          # (a refused request writes nothing)
        trs = np.zeros((s.ntracers if s.ntracers <= SERIES_MAX_TRACERS else 0, 8))
        self._check(self._lib.fpic_series_now(self._h, ctypes.byref(s), _scope_code(scope),
                                              pts.ctypes.data, trs.ctypes.data))
        return {"points": pts, "tracers": trs}

    def recordSeries(self, every, capacity=4096, points=None, tracers=None, species=0):
        """after every `every`-th sub-step the rows of series() go into a device ring of `capacity` rows on the handle's
        stream (fpic_series_record; 0: off).  Independent of recordEnergy, with which it shares the sub-step counter."""
        s, keep = _series_spec(points, tracers, species)
        self._check(self._lib.fpic_series_record(self._h, ctypes.byref(s) if every else None, int(every), int(capacity)))
        self._series_shape = (int(s.npoints), int(s.ntracers)) if every else (0, 0)

    def seriesHistory(self, scope="global"):
        """({substep: uint64 (rows,), points: float64 (rows, P, 8), tracers: float64 (rows, M, 8)}, dropped): the rows
        recorded since the last call, oldest first, and how many older rows the ring overwrote"""
        sc = _scope_code(scope)
        P, M = getattr(self, "_series_shape", (0, 0))
        n, dropped = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.fpic_series_history(self._h, sc, None, None, None, 0, ctypes.byref(n), ctypes.byref(dropped)))
        rows = n.value
        out = {"substep": np.zeros(rows, dtype=np.uint64), "points": np.zeros((rows, P, 8)), "tracers": np.zeros((rows, M, 8))}
        self._check(self._lib.fpic_series_history(self._h, sc, np.zeros(1, dtype=np.uint64).ctypes.data if not rows else out["substep"].ctypes.data,
                                                  out["points"].ctypes.data, out["tracers"].ctypes.data, rows, ctypes.byref(n), ctypes.byref(dropped)))
        return out, int(dropped.value)

    # ---- modes: the Fourier amplitudes of the node fields at chosen wave vectors (fpic_modes_*)
    def _modes_rows(self, modes, fields, scope):
        s, names, keep = _modes_spec(modes, fields)
        rows = np.zeros((s.nmodes if s.nmodes <= MODES_MAX else 0, len(names), 2))      # (a refused request writes nothing)
        spare = np.zeros(2)
        self._check(self._lib.fpic_modes_now(self._h, ctypes.byref(s), _scope_code(scope),
                                             rows.ctypes.data if rows.size else spare.ctypes.data))
        return rows, names

    def modes(self, modes, fields=("ex", "ey", "ez", "phi"), scope="global"):
        """The complex Fourier amplitudes of the node fields of a CART3D box at the wave vectors `modes` (int triples
        (mx, my, mz), shape (nmodes, 3); fpic_modes_now; an (r,z) handle is refused): A(m) = (1/N) sum F exp(-2 pi i (mx i /
        nx + my j / ny + mz k / nz)) over the nodes, of what readField(F3_E) / readField(F3_B_NODES) hold and of
        readField(F3_RHO_FIXED) in C/m^3, summed in double on the device.  fields: names from MODE_FIELDS.  Returns {name:
        complex128 (nmodes,)}.  'global' on a rank with a communicator is collective; on a member of an in-process group it
        is an error (BoxGroup.modes)."""
        return _modes_dict(*self._modes_rows(modes, fields, scope))

    def recordModes(self, every, capacity=4096, modes=None, fields=("ex", "ey", "ez", "phi")):
        """after every `every`-th sub-step the row of modes() goes into a device ring of `capacity` rows on the handle's stream
        (fpic_modes_record; 0: off).  Independent of recordEnergy and recordSeries, with which it shares the sub-step counter."""
        s, names, keep = _modes_spec(modes, fields)
        self._check(self._lib.fpic_modes_record(self._h, ctypes.byref(s) if every else None, int(every), int(capacity)))
        self._modes_shape = (int(s.nmodes), names) if every else (0, [])

    def _modes_history_rows(self, scope):
        sc = _scope_code(scope)
        M, names = getattr(self, "_modes_shape", (0, []))
        n, dropped = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.fpic_modes_history(self._h, sc, None, None, 0, ctypes.byref(n), ctypes.byref(dropped)))
        rows = n.value
        sub, out, spare = np.zeros(max(rows, 1), dtype=np.uint64), np.zeros((rows, M, len(names), 2)), np.zeros(2)
        self._check(self._lib.fpic_modes_history(self._h, sc, sub.ctypes.data, out.ctypes.data if out.size else spare.ctypes.data, rows,
                                                 ctypes.byref(n), ctypes.byref(dropped)))
        return sub[:rows], out, names, int(dropped.value)

    def modesHistory(self, scope="global"):
        """({substep: uint64 (rows,), name: complex128 (rows, nmodes) per recorded field}, dropped): the rows recorded since the
        last call, oldest first, and how many older rows the ring overwrote"""
        sub, out, names, dropped = self._modes_history_rows(scope)
        return dict(_modes_dict(out, names), substep=sub), dropped

    def sync(self):
        self._check(self._lib.fpic_sync(self._h))

    def profile(self, enable=True):
        self._check(self._lib.fpic_profile(self._h, 1 if enable else 0))

    def stats(self):
        s = Stats()
        self._check(self._lib.fpic_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def resetStats(self):
        self._check(self._lib.fpic_reset_stats(self._h))


class ElectrostaticBoxPusher:
    """spec.geometry == 'cart3d': the self-consistent electrostatic extension (BASELINE.json
    configs[2..4]) behind the reference's method names.  Periodic box radius x length_y x height
    (x, y, z) on nr x ny x nz nodes; set / addBZ / precalc / step / density keep their meaning
    (include/fusionpic.h, "extension: spec.geometry").  No reference counterpart: parity unpinned."""

    def __init__(self, spec, precision="fp32", device=0, count=0, sort_interval=0, library=None, **ignored):
        _validate_spec(spec)
        for key in ("ny", "length_y"):
            if key not in spec or isinstance(spec[key], bool) or not isinstance(spec[key], (int, float, np.integer, np.floating)):
                raise FusionPicError(-1, "." + key + " <- Non-optional property is undefined!")
        self._lib = library or load_library()
        self.spec = dict(spec)
        s = Spec()
        for key in _SPEC_KEYS:
            setattr(s, key, spec[key])
        count = int(count or spec.get("count") or 0)
        s.count = count
        s.precision = {"fp32": F32, "fp64": F64}[spec.get("precision", precision)]
        s.device = int(device)
        s.sort_interval = int(sort_interval)
        s.geometry = GEOM_CART3D
        s.solver = {"none": SOLVER_NONE, "poisson_fft": SOLVER_POISSON_FFT, "yee": SOLVER_YEE}[spec.get("solver", "poisson_fft")]
        s.ny = int(spec["ny"])
        s.length_y = float(spec["length_y"])
        s.macro_weight = float(spec.get("macro_weight", 1.0))
        self.precision = s.precision
        self.nx, self.ny, self.nz = int(spec["nr"]), int(spec["ny"]), int(spec["nz"])
        self.nodes = self.nx * self.ny * self.nz
        self.counts = [count if count else int(spec["nparticles"]) ** 2]
        self.n = self.counts[0]
        self.masses = [float(spec["particle_mass"])]
        h = ctypes.c_void_p()
        rc = self._lib.fpic_create(ctypes.byref(s), ctypes.byref(h))
        if rc != 0:
            raise FusionPicError(rc, self._lib.fpic_last_error(None).decode())
        self._h = h

    _check = CylindricalParticlePusher._check
    destroy = CylindricalParticlePusher.destroy
    __del__ = CylindricalParticlePusher.__del__
    sync = CylindricalParticlePusher.sync
    sort = CylindricalParticlePusher.sort
    profile = CylindricalParticlePusher.profile
    stats = CylindricalParticlePusher.stats
    resetStats = CylindricalParticlePusher.resetStats
    setStream = CylindricalParticlePusher.setStream
    precalc = CylindricalParticlePusher.precalc
    step = CylindricalParticlePusher.step
    substeps = CylindricalParticlePusher.substeps
    density = CylindricalParticlePusher.density
    addBZ = CylindricalParticlePusher.addBZ
    deviceBuffer = CylindricalParticlePusher.deviceBuffer
    commInit = CylindricalParticlePusher.commInit
    commDestroy = CylindricalParticlePusher.commDestroy
    commInfo = CylindricalParticlePusher.commInfo

    def addSpecies(self, mass, charge, count):
        idx = ctypes.c_int()
        self._check(self._lib.fpic_add_species(self._h, float(mass), float(charge), int(count), ctypes.byref(idx)))
        self.counts.append(int(count))
        self.masses.append(float(mass))
        return idx.value

    def addB(self, bx, by, bz):
        self._check(self._lib.fpic_add_b(self._h, float(bx), float(by), float(bz)))

    def _live(self, species):
        """the particles the species holds now, from the library (fpic_population): sources and sinks change it behind the
        wrapper; a species the handle does not have keeps the wrapper's own answer (the call then names the mistake)"""
        n, span = ctypes.c_uint64(), ctypes.c_uint64()
        if (isinstance(species, (int, np.integer)) and self._lib.fpic_population(self._h, int(species), ctypes.byref(n), None, ctypes.byref(span)) == 0
                and span.value == n.value):      # (a thinned species has no caller's order: the library refuses the call by name)
            self.counts[int(species)] = int(n.value)
            if int(species) == 0:
                self.n = int(n.value)
        return self.counts[species]

    def set(self, value=None, species=0, **kw):
        """out.set({position, velocity, E}): positions in metres, velocities in units of c (empic.js:1199-1244);
        E is value[i][j][k][3] in V/m (a static field with solver 'none', or a field injected for a test)."""
        value = dict(value or {}, **kw)
        n = self._live(species)
        for key in ("position", "velocity"):
            if value.get(key) is not None:
                a = _as_float_array(value[key])
                if a.shape != (n, 3):
                    raise FusionPicError(-1, ".%s <- expected [%d][3]" % (key, n))
                p = a.ctypes.data if key == "position" else None
                v = a.ctypes.data if key == "velocity" else None
                self._check(self._lib.fpic_set_particles_of(self._h, species, p, v, n, _code(a)))
        # E: node-centred (static field / injected field); edge_E, face_B: the Yee lattice's own arrays (full EM)
        for key, which in (("E", F3_E), ("edge_E", F3_EDGE_E), ("face_B", F3_FACE_B)):
            if value.get(key) is not None:
                a = _as_float_array(value[key])
                if a.shape != (self.nx, self.ny, self.nz, 3):
                    raise FusionPicError(-1, ".%s <- expected [%d][%d][%d][3]" % (key, self.nx, self.ny, self.nz))
                self._check(self._lib.fpic_set_field3(self._h, which, a.ctypes.data, self.nx, self.ny, self.nz, _code(a)))

    def setRange(self, first, position=None, velocity=None, species=0):
        """the caller's particles [first, first + len) of a species (piecewise upload of a large population); numpy
        arrays, or device-resident tensors (anything with data_ptr(): the library copies with hipMemcpyDefault, and
        the caller has synchronised the stream that produced them)"""
        arrs = [None if a is None else _device_or_host(a) for a in (position, velocity)]
        m = next(a.shape[0] for a in arrs if a is not None)
        codes = {a.code for a in arrs if a is not None}
        if len(codes) != 1 or any(a is not None and a.shape != (m, 3) for a in arrs):
            raise FusionPicError(-1, ".position <- position and velocity must be [m][3] of one element type")
        ptr = lambda a: None if a is None else a.ptr
        self._check(self._lib.fpic_set_particles_range(self._h, species, int(first), m, ptr(arrs[0]), ptr(arrs[1]), codes.pop()))

    # ---- spatial decomposition (z-slabs; include/fusionpic.h, fpic_domain_*)
    def domainInit(self, rank, world, ghost_planes=2, migrate_every=4, distributed_solve=False):
        # distributed_solve: False / 0 replicated, True / 1 transposed spectrum, "interface" / 2 tridiagonal interface solve along z
        mode = 2 if (distributed_solve == "interface" or (distributed_solve == 2 and distributed_solve is not True)) else (1 if distributed_solve else 0)
        self._check(self._lib.fpic_domain_init(self._h, int(rank), int(world), int(ghost_planes), int(migrate_every), mode))

    def domainSet(self, position, velocity, first_id, species=0):
        p, v = _device_or_host(position), _device_or_host(velocity)
        if p.shape != v.shape or len(p.shape) != 2 or p.shape[1] != 3 or p.code != v.code:
            raise FusionPicError(-1, ".position <- position and velocity must be [n][3] of one element type")
        self._check(self._lib.fpic_domain_set_particles(self._h, species, p.shape[0], p.ptr, v.ptr, int(first_id), p.code))

    def domainGet(self, dtype=None, species=0):
        """{position, velocity, ids} of the particles this rank holds now (no particular order)"""
        code = self.precision if dtype is None else (F32 if np.dtype(dtype) == np.float32 else F64)
        n = ctypes.c_uint64()
        self._check(self._lib.fpic_domain_get_particles(self._h, species, None, None, None, 0, ctypes.byref(n), code))
        m = n.value
        out = {"position": np.empty((m, 3), dtype=_np_dtype(code)), "velocity": np.empty((m, 3), dtype=_np_dtype(code)),
               "ids": np.empty(m, dtype=np.uint32)}
        self._check(self._lib.fpic_domain_get_particles(self._h, species, out["position"].ctypes.data, out["velocity"].ctypes.data,
                                                        out["ids"].ctypes.data, m, ctypes.byref(n), code))
        return out

    def saveCheckpoint(self, path):
        """particles of every species (raw state, caller's order) and the fields; not for a decomposed handle"""
        self._check(self._lib.fpic_save_checkpoint(self._h, os.fsencode(path)))

    def loadCheckpoint(self, path):
        self._check(self._lib.fpic_load_checkpoint(self._h, os.fsencode(path)))

    def domainStats(self):
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.fpic_domain_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return {"migrated": a.value, "lost": b.value}

    def getParticles(self, dtype=None, species=0):
        code = self.precision if dtype is None else (F32 if np.dtype(dtype) == np.float32 else F64)
        n = self._live(species)
        out = {"position": np.empty((n, 3), dtype=_np_dtype(code)), "velocity": np.empty((n, 3), dtype=_np_dtype(code))}
        self._check(self._lib.fpic_get_particles_of(self._h, species, out["position"].ctypes.data, out["velocity"].ctypes.data, code))
        return out

    def getCells(self, species=0):
        out = np.empty(self._live(species), dtype=np.int32)
        self._check(self._lib.fpic_get_cells_of(self._h, species, out.ctypes.data))
        return out

    def getRange(self, first, count, stride=1, dtype=None, species=0, cells=False):
        """The caller's particles first, first + stride, ... (`count` of them): the mirror of setRange and a sampled
        read-back (fpic_get_particles_range); cells=True adds their node cells."""
        code = self.precision if dtype is None else (F32 if np.dtype(dtype) == np.float32 else F64)
        out = {"position": np.empty((count, 3), dtype=_np_dtype(code)), "velocity": np.empty((count, 3), dtype=_np_dtype(code))}
        self._check(self._lib.fpic_get_particles_range(self._h, species, int(first), int(count), int(stride),
                                                       out["position"].ctypes.data, out["velocity"].ctypes.data, code))
        if cells:
            out["cells"] = np.empty(count, dtype=np.int32)
            self._check(self._lib.fpic_get_cells_range(self._h, species, int(first), int(count), int(stride), out["cells"].ctypes.data))
        return out

    def readField(self, which, dtype=None):
        """F3_E -> [nodes][4] (Ex, Ey, Ez, phi); F3_RHO / F3_PHI -> [nodes]; F3_RHO_FIXED -> int64 [nodes];
        node index i + nr*(j + ny*k)."""
        if which in (F3_RHO_FIXED, F3_J_FIXED):
            out = np.empty(self.nodes * (3 if which == F3_J_FIXED else 1), dtype=np.int64)
            self._check(self._lib.fpic_read_field3(self._h, which, out.ctypes.data, 0))
            return out.reshape(self.nodes, 3) if which == F3_J_FIXED else out
        code = self.precision if dtype is None else (F32 if np.dtype(dtype) == np.float32 else F64)
        four = which in (F3_E, F3_B_NODES, F3_EDGE_E, F3_FACE_B)
        out = np.empty(self.nodes * (4 if four else 1), dtype=_np_dtype(code))
        self._check(self._lib.fpic_read_field3(self._h, which, out.ctypes.data, code))
        return out.reshape(self.nodes, 4) if four else out

    # ---- energy and momentum diagnostics (fpic_energy_*), reduced on the device
    def _energy_row(self, scope):
        e = Energy()
        self._check(self._lib.fpic_energy_now(self._h, _scope_code(scope), ctypes.byref(e)))
        return np.frombuffer(bytes(e), dtype=ENERGY_DTYPE)[0]

    def energy(self, scope="global"):
        """{substep, field_e, field_b, field_b_external (J), count, kinetic (J), momentum (kg m/s), speed_max (c)} now;
        per-species entries are arrays over the species.  'global' on a rank with a communicator is collective; on a
        member of an in-process group it is an error (BoxGroup.energy sums the members)."""
        return _energy_dict(self._energy_row(scope))

    def recordEnergy(self, every, capacity=4096):
        """after every `every`-th sub-step the same reduction goes into a device ring of `capacity` rows (0: off)"""
        self._check(self._lib.fpic_energy_record(self._h, int(every), int(capacity)))

    def energyHistory(self, scope="global"):
        """(rows, dropped): the rows recorded since the last call, oldest first, as a numpy structured array of
        ENERGY_DTYPE, and how many older rows the ring overwrote"""
        sc = _scope_code(scope)
        n, dropped = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.fpic_energy_history(self._h, sc, None, 0, ctypes.byref(n), ctypes.byref(dropped)))
        rows = np.zeros(n.value, dtype=ENERGY_DTYPE)
        self._check(self._lib.fpic_energy_history(self._h, sc, rows.ctypes.data if n.value else None, n.value,
                                                  ctypes.byref(n), ctypes.byref(dropped)))
        return rows, int(dropped.value)

    histogram = CylindricalParticlePusher.histogram
    select = CylindricalParticlePusher.select
    _box_lengths = CylindricalParticlePusher._box_lengths
    load = CylindricalParticlePusher.load
    collide = CylindricalParticlePusher.collide
    collideEvery = CylindricalParticlePusher.collideEvery
    collisionStats = CylindricalParticlePusher.collisionStats
    clearCollisions = CylindricalParticlePusher.clearCollisions
    force = CylindricalParticlePusher.force
    forceOn = CylindricalParticlePusher.forceOn
    forceStats = CylindricalParticlePusher.forceStats
    clearForces = CylindricalParticlePusher.clearForces
    collideGas = CylindricalParticlePusher.collideGas
    collideGasEvery = CylindricalParticlePusher.collideGasEvery
    gasStats = CylindricalParticlePusher.gasStats
    clearGas = CylindricalParticlePusher.clearGas
    remove = CylindricalParticlePusher.remove
    removeEvery = CylindricalParticlePusher.removeEvery
    removeStats = CylindricalParticlePusher.removeStats
    clearRemovals = CylindricalParticlePusher.clearRemovals
    renumber = CylindricalParticlePusher.renumber
    population = CylindricalParticlePusher.population
    reserve = CylindricalParticlePusher.reserve
    inject = CylindricalParticlePusher.inject
    injectEvery = CylindricalParticlePusher.injectEvery
    injectStats = CylindricalParticlePusher.injectStats
    clearInjections = CylindricalParticlePusher.clearInjections
    _ionize_refresh = CylindricalParticlePusher._ionize_refresh
    ionize = CylindricalParticlePusher.ionize
    ionizeEvery = CylindricalParticlePusher.ionizeEvery
    ionizeStats = CylindricalParticlePusher.ionizeStats
    clearIonization = CylindricalParticlePusher.clearIonization
    _burn_refresh = CylindricalParticlePusher._burn_refresh
    burn = CylindricalParticlePusher.burn
    burnEvery = CylindricalParticlePusher.burnEvery
    burnStats = CylindricalParticlePusher.burnStats
    clearBurn = CylindricalParticlePusher.clearBurn
    collidePair = CylindricalParticlePusher.collidePair
    collidePairEvery = CylindricalParticlePusher.collidePairEvery
    pairStats = CylindricalParticlePusher.pairStats
    clearPairs = CylindricalParticlePusher.clearPairs
    _fusion_cells = CylindricalParticlePusher._fusion_cells
    fusionYield = CylindricalParticlePusher.fusionYield
    fusionYieldEvery = CylindricalParticlePusher.fusionYieldEvery
    fusionStats = CylindricalParticlePusher.fusionStats
    fusionGrid = CylindricalParticlePusher.fusionGrid
    clearFusion = CylindricalParticlePusher.clearFusion
    fusionSpectrum = CylindricalParticlePusher.fusionSpectrum
    fusionSpectrumEvery = CylindricalParticlePusher.fusionSpectrumEvery
    fusionSpectrumRead = CylindricalParticlePusher.fusionSpectrumRead
    clearFusionSpectra = CylindricalParticlePusher.clearFusionSpectra
    count = CylindricalParticlePusher.count
    series = CylindricalParticlePusher.series
    recordSeries = CylindricalParticlePusher.recordSeries
    seriesHistory = CylindricalParticlePusher.seriesHistory
    _modes_rows = CylindricalParticlePusher._modes_rows
    modes = CylindricalParticlePusher.modes
    recordModes = CylindricalParticlePusher.recordModes
    _modes_history_rows = CylindricalParticlePusher._modes_history_rows
    modesHistory = CylindricalParticlePusher.modesHistory

    # ---- fluid moment grids (fpic_moments), reduced on the device
    def moments(self, which="order2", species=0, scope="global"):
        """Velocity moments of one species on the node grid as exact int64 sums (fpic_moments).  which: "n" (N), "order1"
        (N FX FY FZ), "order2" (all ten) or an iterable of names from MOMENT_NAMES.  Returns {name: int64 array of shape
        (nz, ny, nr), rejected, spilled}: N in units of 2^-42 particles, the others in units of 2^-32 of v/c resp. (v/c)^2.
        'global' on a rank with a communicator is collective; on a member of an in-process group it is an error
        (BoxGroup.moments)."""
        mask = _moments_mask(which)
        return _moments_result(mask, *_moments_call(self, mask, species, scope))

    def fluid(self, species=0, scope="global", moments=None):
        """Fluid quantities of one species per node, float64 numpy on top of moments("order2") (or of `moments`, a result of
        it): n (m^-3), flux[3] (m^-2 s^-1), u[3] (m/s, zero where N == 0), Pi[3][3] (momentum flux, Pa), P[3][3] (pressure,
        Pa), T (eV, zero where N == 0); arrays shaped (..., nz, ny, nr)."""
        return _fluid(self, moments if moments is not None else self.moments("order2", species, scope), species)


def _fluid(sim, m, species):
    spec = sim.spec
    dv = (float(spec["radius"]) / sim.nx) * (float(spec["length_y"]) / sim.ny) * (float(spec["height"]) / sim.nz)
    per = float(spec.get("macro_weight", 1.0)) / dv          # real particles per macro-particle and m^3
    mass, c = sim.masses[species], SPEED_OF_LIGHT
    n = m["N"].astype(np.float64) / MOM_ONE * per
    flux = np.stack([m[k].astype(np.float64) for k in ("FX", "FY", "FZ")]) * (c / MOM_SCALE * per)
    some = m["N"] > 0
    u = np.divide(flux, n, out=np.zeros_like(flux), where=some)
    S = {k: m[k].astype(np.float64) * (mass * c * c / MOM_SCALE * per) for k in ("SXX", "SYY", "SZZ", "SXY", "SXZ", "SYZ")}
    Pi = np.array([[S["SXX"], S["SXY"], S["SXZ"]], [S["SXY"], S["SYY"], S["SYZ"]], [S["SXZ"], S["SYZ"], S["SZZ"]]])
    P = Pi - mass * n * u[:, None] * u[None, :]
    T = np.divide(P[0, 0] + P[1, 1] + P[2, 2], 3 * n, out=np.zeros_like(n), where=some) / ELECTRON_VOLT
    return {"n": n, "flux": flux, "u": u, "Pi": Pi, "P": P, "T": T}


def _collide_sum(parts):
    out = {k: sum(p[k] for p in parts) for k in ("candidates", "collided", "clipped")}
    out["applications"] = parts[0]["applications"]
    return out


class BoxGroup:
    """All ranks of a z-slab decomposition as handles of this process on one GPU (fpic_group_*): the in-process
    stand-in for the RCCL exchange."""

    def __init__(self, sims):
        self.sims = list(sims)
        self._lib = self.sims[0]._lib
        self._arr = (ctypes.c_void_p * len(self.sims))(*[s._h for s in self.sims])

    def _check(self, rc):
        if rc != 0:
            raise FusionPicError(rc, self._lib.fpic_last_error(self.sims[0]._h).decode())

    def precalc(self):
        self._check(self._lib.fpic_group_precalc(self._arr, len(self.sims)))

    def step(self, ncalls=1):
        self._check(self._lib.fpic_group_step(self._arr, len(self.sims), int(ncalls)))

    def density(self):
        """density() of every member of a full-EM group: the charge grid of the current positions, complete on own planes"""
        self._check(self._lib.fpic_group_density(self._arr, len(self.sims)))

    def energy(self):
        """the whole box: the members' LOCAL values (each its own particles and planes) combined in rank order"""
        return _energy_dict(_energy_sum([s._energy_row("local") for s in self.sims]))

    def histogram(self, axes, bins, range, species=0):
        """the whole box: the members' LOCAL histograms (each its own particles) added up"""
        s, shape, rg = _hist_spec(axes, bins, range, species)
        parts = [_hist_call(m, s, shape, "local") for m in self.sims]
        counts = parts[0][0]
        for c, _ in parts[1:]:
            counts += c
        return _hist_result(counts, sum(p[1] for p in parts), shape, rg)

    def load(self, *args, **request):
        """load() of every member with the same request: each generates the indices [first, first + count) and keeps the
        particles of its planes (count is needed: a rank does not know the whole population).  Returns the members' counts."""
        return [m.load(*args, **request) for m in self.sims]

    def collide(self, kind, **request):
        """collide() of every member with the same request; the members' counts added up (applications: the first member's)"""
        return _collide_sum([m.collide(kind, **request) for m in self.sims])

    def collideEvery(self, every, kind=None, **request):
        """collideEvery() of every member with the same request; the index (the same on every member)"""
        return [m.collideEvery(every, kind, **request) for m in self.sims][0]

    def collisionStats(self, index):
        """the whole box: the members' LOCAL totals added up (applications: the first member's)"""
        return _collide_sum([m.collisionStats(index, "local") for m in self.sims])

    def clearCollisions(self):
        for m in self.sims:
            m.clearCollisions()

    def _force_scales(self, request_species):
        m = self.sims[0]
        W = float(m.spec.get("macro_weight", 1.0))
        return m.masses[request_species], W if W > 0 else 1.0   # (as the library takes it)

    def force(self, **request):
        """force() of every member with the same request; the members' integers added up and the doubles formed from the
        sums (applications: the first member's)"""
        return _force_sum([m.force(**request) for m in self.sims], *self._force_scales(int(request.get("species", 0))))

    def forceOn(self, **request):
        """forceOn() of every member with the same request; the index (the same on every member)"""
        index = [m.forceOn(**request) for m in self.sims][0]
        self._force_species = getattr(self, "_force_species", {})
        self._force_species[index] = int(request.get("species", 0))
        return index

    def forceStats(self, index):
        """the whole box: the members' LOCAL integers added up, the doubles formed from the sums (applications: the first member's)"""
        parts = [m.forceStats(index, "local") for m in self.sims]
        return _force_sum(parts, *self._force_scales(self._force_species[int(index)]))

    def clearForces(self):
        for m in self.sims:
            m.clearForces()
        self._force_species = {}

    def collideGas(self, kind, **request):
        """collideGas() of every member with the same request; the members' integers added up and the doubles formed from
        the sums (applications: the first member's)"""
        return _gas_sum([m.collideGas(kind, **request) for m in self.sims], *self._force_scales(int(request.get("species", 0))))

    def collideGasEvery(self, every, kind=None, **request):
        """collideGasEvery() of every member with the same request; the index (the same on every member)"""
        index = [m.collideGasEvery(every, kind, **request) for m in self.sims][0]
        self._gas_species = getattr(self, "_gas_species", {})
        self._gas_species[index] = int(request.get("species", 0))
        return index

    def gasStats(self, index):
        """the whole box: the members' LOCAL integers added up, the doubles formed from the sums (applications: the first member's)"""
        parts = [m.gasStats(index, "local") for m in self.sims]
        return _gas_sum(parts, *self._force_scales(self._gas_species[int(index)]))

    def clearGas(self):
        for m in self.sims:
            m.clearGas()
        self._gas_species = {}

    def remove(self, where=None, species=0, every=None, outside=False):
        """refused (FPIC_ERR_STATE), as by every member: a rank's dead slots and its migration tail would need a protocol
        of their own"""
        raise FusionPicError(-5, _REMOVE_DECOMPOSED % "remove")

    def removeEvery(self, period, where=None, species=0, every=None, outside=False):
        """refused, see remove"""
        raise FusionPicError(-5, _REMOVE_DECOMPOSED % "removeEvery")

    def removeStats(self, index, scope="global"):
        """refused, see remove"""
        raise FusionPicError(-5, _REMOVE_DECOMPOSED % "removeStats")

    def clearRemovals(self):
        """refused, see remove"""
        raise FusionPicError(-5, _REMOVE_DECOMPOSED % "clearRemovals")

    def renumber(self, species=0):
        """refused, see remove"""
        raise FusionPicError(-5, _REMOVE_DECOMPOSED % "renumber")

    def inject(self, kind="volume", **request):
        """refused (FPIC_ERR_STATE), as by every member: a rank's arrivals ride on its next push and its message buffers were
        sized from its capacity, so a source needs a protocol of its own there.  Inject before domainInit"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "inject")

    def injectEvery(self, period, kind="volume", **request):
        """refused, see inject"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "injectEvery")

    def injectStats(self, index, scope="global"):
        """refused, see inject"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "injectStats")

    def clearInjections(self):
        """refused, see inject"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "clearInjections")

    def reserve(self, species=0, capacity=0):
        """refused, see inject"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "reserve")

    def ionize(self, **request):
        """refused (FPIC_ERR_STATE), as by every member, for the sources' reason: an ioniser appends particles"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "ionize")

    def ionizeEvery(self, every, **request):
        """refused, see ionize"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "ionizeEvery")

    def ionizeStats(self, index, scope="global"):
        """refused, see ionize"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "ionizeStats")

    def clearIonization(self):
        """refused, see ionize"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "clearIonization")

    def burn(self, a=0, b=None, **request):
        """refused (FPIC_ERR_STATE), as by every member, for the sources' reason: a burner appends particles"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "burn")

    def burnEvery(self, every, a=0, b=None, **request):
        """refused, see burn"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "burnEvery")

    def burnStats(self, index, scope="global"):
        """refused, see burn"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "burnStats")

    def clearBurn(self):
        """refused, see burn"""
        raise FusionPicError(-5, _INJECT_DECOMPOSED % "clearBurn")

    def collidePair(self, a=0, b=None, **request):
        """refused (FPIC_ERR_STATE), as by every member: between two migrations the particles of a cell can sit on two
        ranks, in the ghost planes, so a rank cannot pair a cell alone"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "collidePair")

    def collidePairEvery(self, every, a=0, b=None, **request):
        """refused, see collidePair"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "collidePairEvery")

    def pairStats(self, index):
        """refused, see collidePair"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "pairStats")

    def clearPairs(self):
        """refused, see collidePair"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "clearPairs")

    def fusionYield(self, a=0, b=None, grid=False, **request):
        """refused (FPIC_ERR_STATE), as by every member and as collidePair: a rank cannot pair a cell alone"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "fusionYield")

    def fusionYieldEvery(self, every, a=0, b=None, **request):
        """refused, see fusionYield"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "fusionYieldEvery")

    def fusionStats(self, index):
        """refused, see fusionYield"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "fusionStats")

    def fusionGrid(self, index, reset=False):
        """refused, see fusionYield"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "fusionGrid")

    def clearFusion(self):
        """refused, see fusionYield"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "clearFusion")

    def fusionSpectrum(self, a=0, b=None, **request):
        """refused, see fusionYield"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "fusionSpectrum")

    def fusionSpectrumEvery(self, every, a=0, b=None, **request):
        """refused, see fusionYield"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "fusionSpectrumEvery")

    def fusionSpectrumRead(self, index, reset=False):
        """refused, see fusionYield"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "fusionSpectrumRead")

    def clearFusionSpectra(self):
        """refused, see fusionYield"""
        raise FusionPicError(-5, _PAIR_DECOMPOSED % "clearFusionSpectra")

    def count(self, where=None, species=0, every=None):
        """the whole box: the members' LOCAL counts (each its own particles) added up"""
        s = _select_spec(where, species, every)
        return sum(_select_count(m, s, "local") for m in self.sims)

    def select(self, where=None, species=0, every=None, capacity=None, dtype=None):
        """the whole box: the members' LOCAL rows (each its own particles) merged in ascending id.  As select(), plus
        matched_members: the members' own counts."""
        s = _select_spec(where, species, every)
        counts = [_select_count(m, s, "local") for m in self.sims]
        total = sum(counts)
        if capacity is not None and total > int(capacity):
            return {"ids": None, "position": None, "velocity": None, "matched": total, "matched_members": counts}
        parts = [_select_call(m, s, c, "local", dtype) for m, c in zip(self.sims, counts)]
        ids = np.concatenate([p["ids"] for p in parts])
        order = np.argsort(ids, kind="stable")
        return {"ids": ids[order], "position": np.concatenate([p["position"] for p in parts])[order],
                "velocity": np.concatenate([p["velocity"] for p in parts])[order], "matched": total, "matched_members": counts}

    def moments(self, which="order2", species=0):
        """the whole box: the members' LOCAL moment grids (each its own particles, on the planes it holds) added up"""
        mask = _moments_mask(which)
        parts = [_moments_call(m, mask, species, "local") for m in self.sims]
        grids = parts[0][0]
        for g, _, _ in parts[1:]:
            grids += g
        return _moments_result(mask, grids, sum(p[1] for p in parts), sum(p[2] for p in parts))

    def fluid(self, species=0):
        return _fluid(self.sims[0], self.moments("order2", species), species)

    def series(self, points=None, tracers=None, species=0):
        """the whole box: entry by entry the row of the member that reports it (its flag set) among the members' LOCAL rows —
        the owner of a point's cell plane, the holder of a tracer's live slot.  As series(), plus owner_points / owner_tracers:
        the member's index per entry (-1: nobody reports it)."""
        parts = [m.series(points, tracers, species, "local") for m in self.sims]
        pts, op = _series_select([p["points"] for p in parts], SERIES_POINT_COLUMNS.index("present"))
        trs, ot = _series_select([p["tracers"] for p in parts], SERIES_TRACER_COLUMNS.index("found"))
        return {"points": pts, "tracers": trs, "owner_points": op, "owner_tracers": ot}

    def recordSeries(self, every, capacity=4096, points=None, tracers=None, species=0):
        """every member records its LOCAL rows of the same request"""
        for m in self.sims:
            m.recordSeries(every, capacity, points, tracers, species)

    def seriesHistory(self):
        """the members' LOCAL histories drained and selected as series() does, row by row: ({substep, points, tracers,
        owner_points, owner_tracers}, dropped)"""
        parts = [m.seriesHistory("local") for m in self.sims]
        first, dropped = parts[0]
        for p, d in parts[1:]:
            if d != dropped or not np.array_equal(p["substep"], first["substep"]):
                raise FusionPicError(-5, "the members hold different recorded rows: record with the same settings on every member")
        pts, op = _series_select([p["points"] for p, _ in parts], SERIES_POINT_COLUMNS.index("present"))
        trs, ot = _series_select([p["tracers"] for p, _ in parts], SERIES_TRACER_COLUMNS.index("found"))
        return {"substep": first["substep"], "points": pts, "tracers": trs, "owner_points": op, "owner_tracers": ot}, dropped


    def modes(self, modes, fields=("ex", "ey", "ez", "phi")):
        """the whole box: the members' LOCAL rows (each the sum over its own planes) added in rank order"""
        parts = [m._modes_rows(modes, fields, "local") for m in self.sims]
        return _modes_dict(_modes_sum([p[0] for p in parts]), parts[0][1])

    def recordModes(self, every, capacity=4096, modes=None, fields=("ex", "ey", "ez", "phi")):
        """every member records its LOCAL rows of the same request"""
        for m in self.sims:
            m.recordModes(every, capacity, modes, fields)

    def modesHistory(self):
        """the members' LOCAL histories drained and added row by row in rank order, as modes() does.  The members' pending
        row counts are compared first (a query drains nothing), so a mismatch loses no rows."""
        counts = []
        for m in self.sims:
            n, d = ctypes.c_uint64(), ctypes.c_uint64()
            m._check(m._lib.fpic_modes_history(m._h, DIAG_LOCAL, None, None, 0, ctypes.byref(n), ctypes.byref(d)))
            counts.append((n.value, d.value))
        if any(c != counts[0] for c in counts):
            raise FusionPicError(-5, "the members hold different recorded rows: record with the same settings on every member")
        parts = [m._modes_history_rows("local") for m in self.sims]
        sub, _, names, dropped = parts[0]
        for s2, _, _, d2 in parts[1:]:
            if d2 != dropped or not np.array_equal(s2, sub):
                raise FusionPicError(-5, "the members hold different recorded rows: record with the same settings on every member")
        return dict(_modes_dict(_modes_sum([p[1] for p in parts]), names), substep=sub), dropped


def commUniqueId(library=None):
    """ncclGetUniqueId through the library (rank 0); 128 bytes for commInit on every rank"""
    lib = library or load_library()
    buf = ctypes.create_string_buffer(128)
    rc = lib.fpic_comm_unique_id(buf)
    if rc != 0:
        raise FusionPicError(rc, lib.fpic_last_error(None).decode())
    return buf.raw


def makeCylindricalParticlePusher(spec, **extensions):
    """empic.makeCylindricalParticlePusher(spec) (empic.js:30).  Extension key spec.geometry = 'cart3d'
    selects the self-consistent electrostatic box (no reference counterpart)."""
    if spec.get("geometry", "cyl_rz") == "cart3d":
        return ElectrostaticBoxPusher(spec, **extensions)
    return CylindricalParticlePusher(spec, **extensions)
