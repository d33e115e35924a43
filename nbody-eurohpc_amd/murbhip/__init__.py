"""ctypes binding of libmurbhip.so (include/murbhip.h) for tests/ and bench.py.

This is plumbing only: the product's host side is the C++ mirror of the reference's plugin
interface in nbody-eurohpc_amd/host/ (the reference is compiled C++).  There is no CPU fallback:
importing works without a GPU (the library loads and the host-only helpers run), but every compute
entry point raises MurbHipError when no MI355X is present or the library is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MURBHIP_LIBRARY") or os.path.join(_HERE, "..", "lib", "libmurbhip.so")   # override: lab builds
G = np.float32(6.67384e-11)   # reference SimulationNBodyInterface.hpp:18

_fp = C.POINTER(C.c_float)


class MurbHipError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        super().__init__(f"{what}: {error_string(code)} (code {code})")


_lib = None


def lib():
    """The loaded library; raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is None:
        path = os.path.normpath(LIB_PATH)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing: build it with `make -C nbody-eurohpc_amd` "
                                    "(there is no CPU fallback for the HIP path)")
        L = C.CDLL(path)
        L.murbhip_version.restype = C.c_int
        L.murbhip_error_string.restype = C.c_char_p
        L.murbhip_error_string.argtypes = [C.c_int]
        L.murbhip_partition.argtypes = [C.c_ulong, C.c_int, C.c_int, C.POINTER(C.c_ulong), C.POINTER(C.c_ulong)]
        L.murbhip_slice_slots.restype = C.c_ulong
        L.murbhip_slice_slots.argtypes = [C.c_ulong, C.c_int]
        L.murbhip_slot_of_body.restype = C.c_ulong
        L.murbhip_slot_of_body.argtypes = [C.c_ulong, C.c_int, C.c_ulong]
        L.murbhip_schedule_items.argtypes = [C.c_ulong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_ulong,
                                             C.POINTER(C.c_ulong), C.POINTER(C.c_ulong)]
        L.murbhip_schedule_layout.argtypes = [C.c_ulong] + [C.c_int] * 7 + [C.POINTER(C.c_long), C.c_ulong, C.POINTER(C.c_ulong),
                                                                            C.POINTER(C.c_long), C.c_ulong, C.POINTER(C.c_ulong),
                                                                            C.POINTER(C.c_ulong), C.POINTER(C.c_ulong)]
        L.murbhip_device_count.argtypes = [C.POINTER(C.c_int)]
        L.murbhip_create.argtypes = [C.POINTER(C.c_void_p), C.c_ulong, C.c_float, C.c_float, C.c_int]
        L.murbhip_create_sharded.argtypes = [C.POINTER(C.c_void_p), C.c_ulong, C.c_float, C.c_float, C.c_int,
                                             C.POINTER(C.c_int), C.c_int]
        L.murbhip_unique_id.argtypes = [C.c_void_p]
        L.murbhip_create_rank.argtypes = [C.POINTER(C.c_void_p), C.c_ulong, C.c_float, C.c_float, C.c_int, C.c_int,
                                          C.c_int, C.c_void_p]
        L.murbhip_destroy.argtypes = [C.c_void_p]
        L.murbhip_upload.argtypes = [C.c_void_p] + [_fp] * 7
        L.murbhip_init_bodies.argtypes = [C.c_void_p, C.c_char_p, C.c_ulong]
        L.murbhip_download_mass.argtypes = [C.c_void_p, _fp, _fp]
        L.murbhip_download_state.argtypes = [C.c_void_p] + [_fp] * 6
        L.murbhip_download_acc.argtypes = [C.c_void_p] + [_fp] * 3
        L.murbhip_compute_acc.argtypes = [C.c_void_p]
        L.murbhip_compute_acc_jerk.argtypes = [C.c_void_p]
        L.murbhip_download_jerk.argtypes = [C.c_void_p] + [_fp] * 3
        L.murbhip_evolve.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_float, C.c_float, C.c_ulong,
                                     C.POINTER(C.c_double)]
        L.murbhip_evolve_dts.argtypes = [C.c_void_p, _fp, C.c_ulong, C.POINTER(C.c_ulong)]
        L.murbhip_evolve_block.argtypes = [C.c_void_p, C.c_float, C.c_ulong, C.c_double, C.c_double, C.c_int, C.c_ulong,
                                           C.POINTER(C.c_double)]
        L.murbhip_block_state.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_int)]
        L.murbhip_block_set_levels.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
        L.murbhip_download_nearest.argtypes = [C.c_void_p, C.POINTER(C.c_int), _fp]
        L.murbhip_set_encounter.argtypes = [C.c_void_p, C.c_float]
        L.murbhip_encounters.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _fp, C.c_ulong, C.POINTER(C.c_ulong),
                                         C.POINTER(C.c_double)]
        L.murbhip_upload_radii.argtypes = [C.c_void_p, _fp]
        L.murbhip_download_contact.argtypes = [C.c_void_p, C.POINTER(C.c_int), _fp]
        L.murbhip_contacts.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _fp, C.c_ulong, C.POINTER(C.c_ulong),
                                       C.POINTER(C.c_double)]
        L.murbhip_download_potential.argtypes = [C.c_void_p, _fp]
        L.murbhip_potential_energy.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        # include/murbfield.h
        L.murbfield_at.argtypes = [C.c_void_p, C.c_ulong] + [_fp] * 6 + [C.POINTER(C.c_int)] + [_fp] * 7
        L.murbfield_of.argtypes = [C.c_void_p, C.c_ulong, C.POINTER(C.c_int)] + [_fp] * 7
        L.murbfield_layout.argtypes = [C.c_ulong, C.c_long, C.c_long, C.POINTER(C.c_ulong)]
        L.murbfield_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        L.murbfield_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_long)]
        # include/murbtidal.h
        L.murbtidal_at.argtypes = [C.c_void_p, C.c_ulong] + [_fp] * 3 + [C.POINTER(C.c_int)] + [_fp] * 6
        L.murbtidal_of.argtypes = [C.c_void_p, C.c_ulong, C.POINTER(C.c_int)] + [_fp] * 6
        # include/murbknn.h
        _ip = C.POINTER(C.c_int)
        L.murbknn_of.argtypes = [C.c_void_p, C.c_int, C.c_ulong, _ip, _ip, _fp]
        L.murbknn_at.argtypes = [C.c_void_p, C.c_int, C.c_ulong] + [_fp] * 3 + [_ip, _ip, _fp]
        L.murbdensity_of.argtypes = [C.c_void_p, C.c_int, C.c_ulong, _ip, _fp]
        L.murbdensity_centre.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.murbknn_merge.argtypes = [C.c_int, _ip, _fp, _ip, _fp, _ip, _fp]
        L.murbknn_density.argtypes = [C.c_int, _ip, _fp, _fp, C.c_float, _fp]
        # include/murbnbr.h
        _up = C.POINTER(C.c_ulong)
        L.murbnbr_of.argtypes = [C.c_void_p, C.c_ulong, _ip, _fp, C.c_float, _up, _ip, _fp, C.c_ulong]
        L.murbnbr_at.argtypes = [C.c_void_p, C.c_ulong] + [_fp] * 3 + [_ip, _fp, C.c_float, _up, _ip, _fp, C.c_ulong]
        L.murbnbr_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        L.murbnbr_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_long)]
        L.murbnbr_threshold.argtypes = [C.c_float, C.c_float, _fp]
        L.murbnbr_cut.argtypes = [C.c_ulong, _up, C.c_ulong, C.c_ulong, _up]
        # include/murblist.h
        L.murblist_of.argtypes = [C.c_void_p, C.c_ulong, _ip, _up, _ip] + [_fp] * 7
        L.murblist_at.argtypes = [C.c_void_p, C.c_ulong] + [_fp] * 6 + [_up, _ip] + [_fp] * 7
        L.murbsplit_of.argtypes = [C.c_void_p, C.c_ulong, _ip, _fp, C.c_float, _up] + [_fp] * 7
        # include/murbac.h
        _fpp = C.POINTER(_fp)
        L.murbac_begin.argtypes = [C.c_void_p, _fp, C.c_float, C.c_int]
        L.murbac_steps.argtypes = [C.c_void_p, C.c_float, C.c_int]
        L.murbac_end.argtypes = [C.c_void_p]
        L.murbac_state.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.murbac_lists.argtypes = [C.c_void_p, _up, _ip, C.c_ulong]
        L.murbac_forces.argtypes = [C.c_void_p, _fpp, _fpp, _fpp, _fpp]
        # include/murbbind.h
        _dp = C.POINTER(C.c_double)
        L.murbbind_of.argtypes = [C.c_void_p, C.c_ulong, _ip, _ip, _fp]
        L.murbbind_at.argtypes = [C.c_void_p, C.c_ulong] + [_fp] * 7 + [_ip, _ip, _fp]
        L.murbbind_pairs.argtypes = [C.c_void_p, _ip, _ip, _dp, C.c_ulong, _up, _dp]
        L.murbbind_elements.argtypes = [C.c_float, C.c_float, _fp, _fp, C.c_float, _fp, _fp, C.c_float, _dp]
        # include/murbbound.h
        _bp = C.POINTER(C.c_ubyte)
        L.murbpot_of.argtypes = [C.c_void_p, C.c_ulong, _ip, _bp, _fp]
        L.murbpot_at.argtypes = [C.c_void_p, C.c_ulong] + [_fp] * 3 + [_ip, _bp, _fp]
        L.murbbound_members.argtypes = [C.c_void_p, _bp, _dp, C.c_int, _bp, _dp, _dp]
        L.murbbound_radii.argtypes = [C.c_ulong] + [_fp] * 4 + [_bp, _dp, C.c_int, _dp, _dp]
        # include/murbmst.h
        L.murbforeign_of.argtypes = [C.c_void_p, C.c_ulong, _ip, _ip, _ip, _fp]
        L.murbmst_of.argtypes = [C.c_void_p, _bp, C.c_ulong, _ip, _ip, _fp, _dp, _ip, _dp]
        L.murbmst_round.argtypes = [C.c_ulong, _ip, _ip, _fp, _ip, _ip, _fp, C.c_ulong, _up]
        L.murbmst_cut.argtypes = [C.c_ulong, C.c_ulong, _ip, _ip, _fp, C.c_float, _ip]
        # include/murbsep.h
        _qp = C.POINTER(C.c_ulonglong)
        L.murbsep_of.argtypes = [C.c_void_p, C.c_ulong, _ip, _bp, _dp, C.c_int, C.c_int, C.c_int, _qp, _qp]
        L.murbsep_at.argtypes = [C.c_void_p, C.c_ulong] + [_fp] * 3 + [_bp, _dp, C.c_int, C.c_int, C.c_int, _qp, _qp]
        L.murbsep_bin.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float]
        L.murbsep_edges.argtypes = [C.c_int, C.c_int, C.c_int, _fp, _dp]
        # include/murbtracer.h
        L.murbtracer_upload.argtypes = [C.c_void_p, C.c_ulong] + [_fp] * 6
        L.murbtracer_download.argtypes = [C.c_void_p] + [_fp] * 6
        L.murbtracer_download_forces.argtypes = [C.c_void_p] + [_fp] * 6
        L.murbtracer_compute.argtypes = [C.c_void_p]
        L.murbtracer_count.argtypes = [C.c_void_p, C.POINTER(C.c_ulong)]
        L.murbtracer_clear.argtypes = [C.c_void_p]
        L.murbtracer_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        L.murbtracer_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_long)]
        L.murbtracer_validate.argtypes = [C.c_ulong] + [_fp] * 6
        L.murbhip_warmup.argtypes = [C.c_void_p, C.c_double]
        L.murbhip_step.argtypes = [C.c_void_p, C.c_float]
        L.murbhip_steps.argtypes = [C.c_void_p, C.c_float, C.c_int]
        L.murbhip_integrate_host_acc.argtypes = [C.c_void_p] + [_fp] * 3 + [C.c_float]
        L.murbhip_sync.argtypes = [C.c_void_p]
        L.murbhip_energy.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.murbhip_moments.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.murbhip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
        L.murbhip_get_info.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        _lib = L
    return _lib


EXPORTS = ("murbhip_version murbhip_error_string murbhip_partition murbhip_slice_slots murbhip_slot_of_body "
           "murbhip_schedule_items murbhip_schedule_layout "
           "murbhip_device_count murbhip_create murbhip_create_sharded murbhip_unique_id murbhip_create_rank "
           "murbhip_destroy murbhip_upload murbhip_init_bodies murbhip_download_mass murbhip_download_state murbhip_download_acc murbhip_compute_acc "
           "murbhip_compute_acc_jerk murbhip_download_jerk murbhip_evolve murbhip_evolve_dts "
           "murbhip_evolve_block murbhip_block_state murbhip_block_set_levels "
           "murbhip_download_nearest murbhip_set_encounter murbhip_encounters "
           "murbhip_upload_radii murbhip_download_contact murbhip_contacts "
           "murbhip_download_potential murbhip_potential_energy "
           "murbhip_warmup murbhip_step murbhip_steps murbhip_integrate_host_acc murbhip_sync murbhip_energy murbhip_moments murbhip_set_option "
           "murbhip_get_info").split()


FIELD_EXPORTS = "murbfield_at murbfield_of murbfield_layout murbfield_set_option murbfield_get_option".split()   # include/murbfield.h
FIELD_OPTIONS = ("field_chunks", "field_batch")
TIDAL_EXPORTS = "murbtidal_at murbtidal_of".split()   # include/murbtidal.h
TIDAL_KEYS = ("txx", "tyy", "tzz", "txy", "txz", "tyz")
TRACER_EXPORTS = ("murbtracer_upload murbtracer_download murbtracer_download_forces murbtracer_compute murbtracer_count "
                  "murbtracer_clear murbtracer_set_option murbtracer_get_option murbtracer_validate").split()   # include/murbtracer.h
TRACER_OPTIONS = ("tracer_chunks", "tracer_batch", "tracer_dt")
KNN_EXPORTS = "murbknn_of murbknn_at murbdensity_of murbdensity_centre murbknn_merge murbknn_density".split()   # include/murbknn.h
KNN_KMAX = 32
NBR_EXPORTS = "murbnbr_of murbnbr_at murbnbr_set_option murbnbr_get_option murbnbr_threshold murbnbr_cut".split()   # include/murbnbr.h
NBR_OPTIONS = ("list_entries",)
BIND_EXPORTS = "murbbind_of murbbind_at murbbind_pairs murbbind_elements".split()   # include/murbbind.h
BIND_ELEMENT_KEYS = ("a", "e", "period", "h", "energy", "r")
BIND_CENSUS_KEYS = ("pairs", "energy_sum", "hardest_i", "hardest_j", "hardest_energy", "a_min", "bound_bodies", "mutual_pairs")
BOUND_EXPORTS = "murbpot_of murbpot_at murbbound_members murbbound_radii".split()   # include/murbbound.h
BOUND_KEYS = ("members", "mass", "rounds", "converged", "vx", "vy", "vz", "cx", "cy", "cz", "kinetic", "potential", "virial_ratio",
              "removed", "unbound_bodies")
MST_EXPORTS = "murbforeign_of murbmst_of murbmst_round murbmst_cut".split()   # include/murbmst.h
MST_KEYS = ("members", "edges", "components", "rounds", "total_length", "mean_length", "longest_length")
SEP_EXPORTS = "murbsep_of murbsep_at murbsep_bin murbsep_edges".split()   # include/murbsep.h
SEP_KEYS = ("pairs", "below", "above")
LIST_EXPORTS = "murblist_of murblist_at murbsplit_of".split()   # include/murblist.h
AC_EXPORTS = "murbac_begin murbac_steps murbac_end murbac_state murbac_lists murbac_forces".split()   # include/murbac.h
AC_STATE_KEYS = ("n_irr", "m", "steps", "regular_steps", "entries", "longest", "empty", "mean", "time")
AC_NIRR_MAX = 4096
CENTRE_KEYS = ("x", "r_core", "rho_core", "rho_sum", "used", "left_out")


def error_string(code):
    return lib().murbhip_error_string(code).decode()


def _check(code, what):
    if code != 0:
        raise MurbHipError(code, what)


def _ptr(a):
    return a.ctypes.data_as(_fp)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------ host-only helpers
def partition(n, world, rank):
    first, count = C.c_ulong(), C.c_ulong()
    _check(lib().murbhip_partition(n, world, rank, C.byref(first), C.byref(count)), "murbhip_partition")
    return first.value, count.value


def slice_slots(n, world):
    return lib().murbhip_slice_slots(n, world)


def slot_of_body(n, world, i):
    return lib().murbhip_slot_of_body(n, world, i)


def schedule_items(n, world, rank, split=1):
    """(items, own_count): the half-ring work list of `rank`; items is an (count, 2) int array of
    (i-side sub-block, j-side block)."""
    count, own = C.c_ulong(), C.c_ulong()
    _check(lib().murbhip_schedule_items(n, world, rank, split, None, 0, C.byref(count), C.byref(own)),
           "murbhip_schedule_items")
    items = np.zeros((count.value, 2), np.int32)
    _check(lib().murbhip_schedule_items(n, world, rank, split, items.ctypes.data_as(C.POINTER(C.c_int)), count.value,
                                        C.byref(count), C.byref(own)), "murbhip_schedule_items")
    return items, own.value


def schedule_layout(n, world, rank, split=1, waves=4, taper=0, tri_first_pct=50, exchange_mode=False, diag_tri=False, tri_div=1):
    """(items, rows, floats_main, floats_tri): the pair-symmetric work list with its partial-row layout, as arrays of
    8 longs per item and 7 per row-table entry (include/murbhip.h: murbhip_schedule_layout)."""
    ni, nr, fm, ft = C.c_ulong(), C.c_ulong(), C.c_ulong(), C.c_ulong()
    args = (n, world, rank, split, waves, taper + (256 if diag_tri else 0) + 512 * {1: 0, 2: 1, 4: 2, 8: 3}[tri_div], tri_first_pct,
            int(exchange_mode))
    _check(lib().murbhip_schedule_layout(*args, None, 0, C.byref(ni), None, 0, C.byref(nr), C.byref(fm), C.byref(ft)),
           "murbhip_schedule_layout")
    items = np.zeros((ni.value, 8), np.int64)
    rows = np.zeros((nr.value, 7), np.int64)
    lp = C.POINTER(C.c_long)
    _check(lib().murbhip_schedule_layout(*args, items.ctypes.data_as(lp), ni.value, C.byref(ni), rows.ctypes.data_as(lp), nr.value,
                                         C.byref(nr), C.byref(fm), C.byref(ft)), "murbhip_schedule_layout")
    return items, rows, fm.value, ft.value


def field_layout(n, chunks=0, batch=0, count=0):
    """dict of the field read-out's planning for n bodies under "field_chunks" = chunks and "field_batch" = batch (host only;
    include/murbfield.h: murbfield_layout): chunks, groups of 16 points per full launch, launches for `count` points, entries
    of a partial-row buffer, and the chunks' tile ranges [(first, end), ...]."""
    out = (C.c_ulong * 4)(0, 0, 0, count)
    _check(lib().murbfield_layout(n, chunks, batch, out), "murbfield_layout")
    tiles = (n + 511) // 512
    k = int(out[0])
    return {"chunks": k, "groups": int(out[1]), "batches": int(out[2]), "rows": int(out[3]), "tiles": tiles,
            "ranges": [(tiles * c // k, tiles * (c + 1) // k) for c in range(k)]}


def tidal_matrix(d):
    """(P, 3, 3) float32: the symmetric matrices of a tidal_at() / tidal_of() result, for numpy.linalg.eigvalsh."""
    t = [np.asarray(d[k]) for k in TIDAL_KEYS]
    m = np.empty(t[0].shape + (3, 3), t[0].dtype)
    for (a, b), x in zip(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)), t):
        m[..., a, b] = m[..., b, a] = x
    return m


def knn_merge(idx_a, r2_a, idx_b, r2_b):
    """(idx, r2): the k first entries of the merge of two sorted neighbour lists of k entries each under the order (r2, index),
    tails of -1 / +inf (host only; include/murbknn.h: murbknn_merge)."""
    ia, ib = (np.ascontiguousarray(x, np.int32) for x in (idx_a, idx_b))
    ra, rb = _f32(r2_a), _f32(r2_b)
    k = ia.shape[0]
    if any(x.shape != (k,) for x in (ia, ib, ra, rb)):
        raise ValueError("four lists of one length")
    io, ro = np.zeros(k, np.int32), np.zeros(k, np.float32)
    ip = C.POINTER(C.c_int)
    _check(lib().murbknn_merge(k, ia.ctypes.data_as(ip), _ptr(ra), ib.ctypes.data_as(ip), _ptr(rb), io.ctypes.data_as(ip), _ptr(ro)),
           "murbknn_merge")
    return io, ro


def knn_density(idx, r2, masses, soft):
    """float32 density of one sorted neighbour list: the mass of its k - 1 first entries over the sphere through the k-th
    (host only; include/murbknn.h: murbknn_density).  masses is indexed by the list's indices."""
    i, r, m = np.ascontiguousarray(idx, np.int32), _f32(r2), _f32(masses)
    if i.shape != r.shape or i.ndim != 1:
        raise ValueError("idx and r2 are one list")
    if i.size and i.max() >= m.shape[0]:
        raise ValueError("an index has no mass")
    out = np.zeros(1, np.float32)
    _check(lib().murbknn_density(i.shape[0], i.ctypes.data_as(C.POINTER(C.c_int)), _ptr(r), _ptr(m), float(np.float32(soft)), _ptr(out)),
           "murbknn_density")
    return out[0]


def binary_elements(g, soft, qi, vi, mi, qj, vj, mj):
    """dict of the two-body elements a, e, period, h, energy, r (float64) of one pair from its float32 state: positions and
    velocities of three floats each, masses, G and the softening length (host only; include/murbbind.h: murbbind_elements)."""
    q = [_f32(x) for x in (qi, vi, qj, vj)]
    if any(x.shape != (3,) for x in q):
        raise ValueError("positions and velocities have three components")
    out = (C.c_double * 6)()
    _check(lib().murbbind_elements(float(np.float32(g)), float(np.float32(soft)), _ptr(q[0]), _ptr(q[1]), float(np.float32(mi)),
                                   _ptr(q[2]), _ptr(q[3]), float(np.float32(mj)), out), "murbbind_elements")
    return dict(zip(BIND_ELEMENT_KEYS, out[:]))


def _mask(member, n):
    """(array or None, pointer or None) of a mask of n bodies: nonzero = in."""
    if member is None:
        return None, None
    mk = np.ascontiguousarray(np.asarray(member) != 0, np.uint8).reshape(-1)
    if mk.shape != (n,):
        raise ValueError("a mask has one entry per body")
    return mk, mk.ctypes.data_as(C.POINTER(C.c_ubyte))


def _bound_dict(member, e, out16):
    d = {"member": member.astype(bool), "e": e}
    d.update(zip(BOUND_KEYS, out16[:15]))
    for key in ("members", "rounds", "removed", "unbound_bodies"):
        d[key] = int(d[key])
    d["converged"] = bool(d["converged"])
    d["v"] = np.array(out16[4:7])
    d["centre"] = np.array(out16[7:10])
    return d


def lagrangian_radii(q, m, fractions, centre, member=None):
    """float64 radii about `centre` (three values) inside which the listed mass `fractions` (each in (0, 1]) of the members lie:
    q = (qx, qy, qz) and m float32 arrays of n bodies, member a mask (None: all).  The distance of the first body, by
    (distance, index), at which the running mass reaches the fraction of the total; NaN when the members have no mass (host
    only; include/murbbound.h: murbbound_radii)."""
    qa = [_f32(x) for x in q]
    ma = _f32(m)
    n = ma.shape[0]
    if len(qa) != 3 or any(x.shape != (n,) for x in qa):
        raise ValueError("positions are three arrays, one entry per body")
    _, mp = _mask(member, n)
    fr = np.ascontiguousarray(fractions, np.float64).reshape(-1)
    ce = np.ascontiguousarray(centre, np.float64).reshape(-1)
    if ce.shape != (3,):
        raise ValueError("the centre has three components")
    out = np.full(fr.shape[0], np.nan)
    dp = C.POINTER(C.c_double)
    _check(lib().murbbound_radii(n, *[_ptr(x) for x in qa], _ptr(ma), mp, ce.ctypes.data_as(dp), fr.shape[0], fr.ctypes.data_as(dp),
                                 out.ctypes.data_as(dp)), "murbbound_radii")
    return out


def _binaries_dict(i, j, elems, out8):
    d = {"i": i, "j": j}
    for k, key in enumerate(BIND_ELEMENT_KEYS):
        d[key] = np.ascontiguousarray(elems[:, k])
    d["census"] = dict(zip(BIND_CENSUS_KEYS, out8))
    for key in ("pairs", "bound_bodies", "mutual_pairs"):
        d["census"][key] = int(d["census"][key])
    for key in ("hardest_i", "hardest_j"):
        d["census"][key] = int(d["census"][key]) if d["census"][key] == d["census"][key] else -1
    return d


def neighbour_threshold(h, soft):
    """float32 thr = (float)((double)h * h + (double)soft2) of a radius and a softening length: body j is a neighbour if and only
    if r2 <= thr (host only; include/murbnbr.h: murbnbr_threshold)."""
    out = np.zeros(1, np.float32)
    _check(lib().murbnbr_threshold(float(np.float32(h)), float(np.float32(soft)), _ptr(out)), "murbnbr_threshold")
    return out[0]


def neighbour_cut(offsets, first, entries):
    """The furthest point `last` with offsets[last] - offsets[first] <= entries, at least first + 1: how the fill pass cuts a
    launch's points into ranges (host only; include/murbnbr.h: murbnbr_cut)."""
    o = np.ascontiguousarray(offsets, np.uint64)
    last = C.c_ulong()
    _check(lib().murbnbr_cut(max(o.shape[0] - 1, 0), o.ctypes.data_as(C.POINTER(C.c_ulong)), int(first), int(entries), C.byref(last)),
           "murbnbr_cut")
    return last.value


def fof_groups(offsets, idx):
    """int32 group label of each body from the neighbour lists of ALL n bodies at a common h (Simulation.neighbours_of(h=b)): the
    smallest body index of its connected component under "j is listed for i": friends-of-friends groups at linking length b.
    Host only, numpy: minimum propagation along the links and pointer jumping, to a fixed point."""
    o = np.asarray(offsets, np.int64)
    n = o.shape[0] - 1
    j = np.asarray(idx, np.int64)
    if j.shape != (int(o[-1]),):
        raise ValueError("idx holds offsets[-1] entries")
    i = np.repeat(np.arange(n, dtype=np.int64), np.diff(o))
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, i, label[j])
        np.minimum.at(new, j, label[i])   # a common h makes the relation symmetric; this costs nothing where it is
        new = new[new]                    # pointer jumping: a label is a body, whose label is no larger
        if np.array_equal(new, label):
            return label.astype(np.int32)
        label = new


def _csr(offsets, idx, count):
    """(offsets uint64, idx int32) of a CSR pair for `count` points, contiguous; ValueError where the shapes disagree."""
    o = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
    j = np.ascontiguousarray(idx, np.int32).reshape(-1)
    if o.shape != (count + 1,):
        raise ValueError("offsets holds one entry per point and one more")
    if j.shape[0] != int(o[-1]):
        raise ValueError("idx holds offsets[-1] entries")
    return o, j


def complement_lists(n, bodies, offsets, idx):
    """(offsets uint64, idx int32): for every listed body p every OTHER body of the n that is not in its list
    idx[offsets[p]:offsets[p + 1]], in ascending index, the body itself left out.  Host only, numpy.  The sources of the regular
    force of an Ahmad-Cohen split, for Simulation.list_field_of: irregular (the list) + regular (this) = every other body once."""
    n = int(n)
    b = np.asarray(bodies, np.int64).reshape(-1)
    if b.size and (b.min() < 0 or b.max() >= n):
        raise ValueError("a body index outside [0, n)")
    o, j = _csr(offsets, idx, b.shape[0])
    if j.size and (j.min() < 0 or j.max() >= n):
        raise ValueError("a list entry outside [0, n)")
    if o[0] != 0 or np.any(np.diff(o.astype(np.int64)) < 0):
        raise ValueError("offsets start at 0 and do not decrease")
    out_o = np.zeros(b.shape[0] + 1, np.uint64)
    parts = []
    for p in range(b.shape[0]):
        keep = np.ones(n, bool)
        keep[j[int(o[p]):int(o[p + 1])]] = False
        keep[b[p]] = False
        parts.append(np.flatnonzero(keep).astype(np.int32))
        out_o[p + 1] = out_o[p] + np.uint64(parts[-1].shape[0])
    return out_o, (np.concatenate(parts) if parts else np.zeros(0, np.int32))


def split_regular(total, irregular):
    """field_of's dict of the regular force: total - irregular per key, formed in fp64 and rounded once to float32 (host only)."""
    return {k: (np.asarray(total[k], np.float32).astype(np.float64) - np.asarray(irregular[k], np.float32).astype(np.float64)).astype(np.float32)
            for k in Simulation._FIELD_KEYS}


def mst_round(label, partner, r2):
    """(label, i, j, r2, added): one Boruvka round over what Simulation.foreign_nearest(label) returns for all n bodies.  Per
    component (label >= 0; < 0: outside) the minimum, by the key (r2, min(i, j), max(i, j)), over its bodies' (i, partner[i],
    r2[i]); the chosen edges in key order with i < j, mutual choices once; every merged component relabelled to its smallest
    body index.  Input that closes a cycle is not what foreign_nearest returns for these labels: MurbHipError, nothing changed
    (host only; include/murbmst.h: murbmst_round)."""
    lab = np.array(label, np.int32).reshape(-1)   # a copy: the call relabels in place
    pa, ra = np.ascontiguousarray(partner, np.int32).reshape(-1), _f32(r2).reshape(-1)
    n = lab.shape[0]
    if pa.shape != (n,) or ra.shape != (n,):
        raise ValueError("label, partner and r2 have one entry per body")
    ip = C.POINTER(C.c_int)
    i, j, er2 = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    edges = C.c_ulong(0)
    _check(lib().murbmst_round(n, lab.ctypes.data_as(ip), pa.ctypes.data_as(ip), _ptr(ra), i.ctypes.data_as(ip), j.ctypes.data_as(ip),
                               _ptr(er2), n, C.byref(edges)), "murbmst_round")
    e = int(edges.value)
    return lab, i[:e].copy(), j[:e].copy(), er2[:e].copy(), e


def mst_groups(n, i, j, r2, thr):
    """int32 group label of each of n bodies: the smallest body index of its component under the tree edges (i, j) with
    r2 <= thr; bodies on no edge label themselves.  With thr = neighbour_threshold(b, soft) and the tree of all bodies these are
    fof_groups()'s labels at linking length b (host only; include/murbmst.h: murbmst_cut)."""
    ia, ja, ra = np.ascontiguousarray(i, np.int32).reshape(-1), np.ascontiguousarray(j, np.int32).reshape(-1), _f32(r2).reshape(-1)
    if ia.shape != ja.shape or ia.shape != ra.shape:
        raise ValueError("i, j and r2 have one entry per edge")
    ip = C.POINTER(C.c_int)
    label = np.zeros(int(n), np.int32)
    _check(lib().murbmst_cut(int(n), ia.shape[0], ia.ctypes.data_as(ip), ja.ctypes.data_as(ip), _ptr(ra), float(np.float32(thr)),
                             label.ctypes.data_as(ip)), "murbmst_cut")
    return label


def separation_bin(lo_exp, sub, bins, d2):
    """The bin of the squared separation d2 (taken as float32) among `bins` bins from d2 = 2^lo_exp up, 2^sub per octave of d2:
    -1 below, `bins` above (+inf and NaN too), else the bin; read off the float's bits, so a d2 on an edge belongs to the bin
    above the edge (host only; include/murbsep.h: murbsep_bin)."""
    k = lib().murbsep_bin(int(lo_exp), int(sub), int(bins), float(np.float32(d2)))
    if k < -1:
        raise MurbHipError(k, "murbsep_bin")
    return k


def separation_edges(lo_exp, sub, bins):
    """(edge2 float32, edge_r float64), bins + 1 entries each: the bins' edges in d2, exact floats, and their fp64 roots (host
    only; include/murbsep.h: murbsep_edges)."""
    size = max(int(bins), 0) + 1   # bins < 1 is refused by the call
    edge2, edge_r = np.zeros(size, np.float32), np.zeros(size, np.float64)
    _check(lib().murbsep_edges(int(lo_exp), int(sub), int(bins), _ptr(edge2), edge_r.ctypes.data_as(C.POINTER(C.c_double))), "murbsep_edges")
    return edge2, edge_r


def shell_density(hist_row, edge_r):
    """float64 number density per bin of a one-point separation_at (about the density centre, say): the counts hist_row over the
    shell volumes 4/3 pi (edge_r[k + 1]^3 - edge_r[k]^3).  Host only."""
    h, r = np.asarray(hist_row, np.float64).reshape(-1), np.asarray(edge_r, np.float64).reshape(-1)
    if r.shape != (h.shape[0] + 1,):
        raise ValueError("edge_r has one entry more than hist_row")
    return h / (4.0 / 3.0 * np.pi * (r[1:] ** 3 - r[:-1] ** 3))


def _centre_dict(out):
    return {"x": np.array(out[:3]), "r_core": out[3], "rho_core": out[4], "rho_sum": out[5], "used": int(out[6]), "left_out": int(out[7])}


def device_count():
    c = C.c_int(0)
    rc = lib().murbhip_device_count(C.byref(c))
    return c.value if rc == 0 else 0


def unique_id():
    buf = C.create_string_buffer(128)
    _check(lib().murbhip_unique_id(buf), "murbhip_unique_id")
    return buf.raw


class Simulation:
    """One device-resident n-body state.  mode: single GPU (default), `devices=[...]` for one process
    driving several shards, or `rank/world/uid` for one process per GPU."""

    def __init__(self, n, soft=2e8, g=G, device=0, devices=None, exchange="copy", rank=None, world=None, uid=None):
        self.n = int(n)
        self.soft = float(np.float32(soft))
        self._h = C.c_void_p()
        L = lib()
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            _check(L.murbhip_create_sharded(C.byref(self._h), self.n, soft, g, len(devices), arr,
                                            {"copy": 0, "rccl": 1}[exchange]), "murbhip_create_sharded")
        elif rank is not None:
            _check(L.murbhip_create_rank(C.byref(self._h), self.n, soft, g, device, rank, world, uid),
                   "murbhip_create_rank")
        else:
            _check(L.murbhip_create(C.byref(self._h), self.n, soft, g, device), "murbhip_create")

    # -- state
    def upload(self, s):
        a = [_f32(s[k]) for k in ("qx", "qy", "qz", "vx", "vy", "vz", "m")]
        for x in a:
            if x.shape[0] < self.n:
                raise ValueError("state arrays shorter than n")
        _check(lib().murbhip_upload(self._h, *[_ptr(x) for x in a]), "murbhip_upload")

    def init_bodies(self, scheme="galaxy", seed=0):
        """Initial conditions generated on the device (include/murbhip.h: murbhip_init_bodies)."""
        _check(lib().murbhip_init_bodies(self._h, scheme.encode(), seed), "murbhip_init_bodies")

    def masses(self, with_radii=False):
        m = np.zeros(self.n, np.float32)
        r = np.zeros(self.n, np.float32) if with_radii else None
        _check(lib().murbhip_download_mass(self._h, _ptr(m), _ptr(r) if with_radii else None), "murbhip_download_mass")
        return (m, r) if with_radii else m

    def state(self):
        out = {k: np.zeros(self.n, np.float32) for k in ("qx", "qy", "qz", "vx", "vy", "vz")}
        _check(lib().murbhip_download_state(self._h, *[_ptr(out[k]) for k in ("qx", "qy", "qz", "vx", "vy", "vz")]),
               "murbhip_download_state")
        return out

    def acc(self):
        a = [np.zeros(self.n, np.float32) for _ in range(3)]
        _check(lib().murbhip_download_acc(self._h, *[_ptr(x) for x in a]), "murbhip_download_acc")
        return tuple(a)

    # -- compute (enqueue only; sync() waits)
    def compute_acc(self):
        _check(lib().murbhip_compute_acc(self._h), "murbhip_compute_acc")

    def compute_acc_jerk(self):
        """Accelerations and jerks in one sweep (include/murbhip.h: murbhip_compute_acc_jerk); read with acc() / jerk()."""
        _check(lib().murbhip_compute_acc_jerk(self._h), "murbhip_compute_acc_jerk")

    def jerk(self):
        j = [np.zeros(self.n, np.float32) for _ in range(3)]
        _check(lib().murbhip_download_jerk(self._h, *[_ptr(x) for x in j]), "murbhip_download_jerk")
        return tuple(j)

    def warmup(self, milliseconds=50.0):
        """Untimed force evaluations on the current state (include/murbhip.h: murbhip_warmup); syncs."""
        _check(lib().murbhip_warmup(self._h, milliseconds), "murbhip_warmup")

    def step(self, dt=3600.0):
        _check(lib().murbhip_step(self._h, dt), "murbhip_step")

    def steps(self, dt, iterations):
        _check(lib().murbhip_steps(self._h, dt, iterations), "murbhip_steps")

    def evolve(self, duration, eta=0.02, eta_start=0.01, dt_min=0.0, dt_max=None, max_steps=1_000_000):
        """Advance `duration` seconds with Hermite steps whose common size the device chooses (include/murbhip.h:
        murbhip_evolve; "integrator" must be 2).  dt_max=None means `duration`.  Returns after a sync."""
        out = (C.c_double * 5)()
        _check(lib().murbhip_evolve(self._h, duration, eta, eta_start, dt_min, duration if dt_max is None else dt_max,
                                    max_steps, out), "murbhip_evolve")
        return {"time": out[0], "steps": int(out[1]), "dt_min": out[2], "dt_max": out[3], "dt_next": out[4]}

    def evolve_dts(self):
        """float32 array of the step sizes the last evolve() used, oldest first (the last 4096 of them)."""
        count = C.c_ulong()
        _check(lib().murbhip_evolve_dts(self._h, None, 0, C.byref(count)), "murbhip_evolve_dts")
        dts = np.zeros(count.value, np.float32)
        if count.value:
            _check(lib().murbhip_evolve_dts(self._h, _ptr(dts), count.value, C.byref(count)), "murbhip_evolve_dts")
        return dts

    def evolve_block(self, dt_max, blocks=1, eta=0.02, eta_start=0.01, kmax=12, max_steps=2 ** 62):
        """Advance `blocks` blocks of dt_max seconds with Hermite steps of individual size dt_max 2^-k, k <= kmax
        (include/murbhip.h: murbhip_evolve_block; "integrator" must be 2).  Returns after a sync."""
        out = (C.c_double * 8)()
        _check(lib().murbhip_evolve_block(self._h, dt_max, blocks, eta, eta_start, kmax, max_steps, out), "murbhip_evolve_block")
        return {"time": out[0], "steps": int(out[1]), "body_steps": int(out[2]), "dt_min": out[3], "dt_max": out[4],
                "clamped": int(out[5]), "max_active": int(out[6]), "synchronised": bool(out[7])}

    def block_state(self):
        """(ticks uint32, levels int32) of every body: its own time inside the block and its level (test hook)."""
        ticks, levels = np.zeros(self.n, np.uint32), np.zeros(self.n, np.int32)
        _check(lib().murbhip_block_state(self._h, ticks.ctypes.data_as(C.POINTER(C.c_uint)), levels.ctypes.data_as(C.POINTER(C.c_int))),
               "murbhip_block_state")
        return ticks, levels

    def set_block_levels(self, levels, kmax):
        """The next evolve_block(kmax=kmax) starts from these levels instead of the starting rule (test hook)."""
        lv = np.ascontiguousarray(levels, np.int32)
        if lv.shape[0] < self.n:
            raise ValueError("levels shorter than n")
        _check(lib().murbhip_block_set_levels(self._h, lv.ctypes.data_as(C.POINTER(C.c_int)), kmax), "murbhip_block_set_levels")

    def nearest(self):
        """(index int32, r2 float32) of every body's nearest neighbour in the remembered evaluation (option "nearest" 1;
        include/murbhip.h: murbhip_download_nearest)."""
        idx, r2 = np.zeros(self.n, np.int32), np.zeros(self.n, np.float32)
        _check(lib().murbhip_download_nearest(self._h, idx.ctypes.data_as(C.POINTER(C.c_int)), _ptr(r2)), "murbhip_download_nearest")
        return idx, r2

    def set_encounter(self, radius):
        """evolve() / evolve_block() end behind a step in which a body that took it has a neighbour within `radius`; 0 = off."""
        _check(lib().murbhip_set_encounter(self._h, radius), "murbhip_set_encounter")

    def encounters(self):
        """dict of the step that ended the last evolve call by an encounter: i, j (int32), r2 (float32) sorted by i, the
        count the device saw (the arrays hold at most 4096) and the model time advanced in that call; count 0 otherwise."""
        count, time = C.c_ulong(), C.c_double()
        ip = C.POINTER(C.c_int)
        _check(lib().murbhip_encounters(self._h, None, None, None, 0, C.byref(count), C.byref(time)), "murbhip_encounters")
        kept = min(count.value, 4096)
        i, j, r2 = np.zeros(kept, np.int32), np.zeros(kept, np.int32), np.zeros(kept, np.float32)
        if kept:
            _check(lib().murbhip_encounters(self._h, i.ctypes.data_as(ip), j.ctypes.data_as(ip), _ptr(r2), kept, C.byref(count),
                                            C.byref(time)), "murbhip_encounters")
        return {"i": i, "j": j, "r2": r2, "count": int(count.value), "time": time.value}

    def upload_radii(self, r):
        """The bodies' radii, n values in the caller's order (include/murbhip.h: murbhip_upload_radii)."""
        r = _f32(r)
        if r.shape[0] < self.n:
            raise ValueError("radii shorter than n")
        _check(lib().murbhip_upload_radii(self._h, _ptr(r)), "murbhip_upload_radii")

    def contact(self):
        """(index int32, gap2 float32) of every body's contact partner by radii in the remembered evaluation (option
        "contact" 1 or 2; include/murbhip.h: murbhip_download_contact).  gap2 <= 0: the two touch."""
        idx, gap2 = np.zeros(self.n, np.int32), np.zeros(self.n, np.float32)
        _check(lib().murbhip_download_contact(self._h, idx.ctypes.data_as(C.POINTER(C.c_int)), _ptr(gap2)), "murbhip_download_contact")
        return idx, gap2

    def potential(self):
        """float32 phi_i = sum_{j != i} G m_j / sqrt(r_ij^2 + soft^2) of every body in the remembered evaluation (option
        "potential" 1; include/murbhip.h: murbhip_download_potential).  Positive; after a step: at its predicted end state."""
        phi = np.zeros(self.n, np.float32)
        _check(lib().murbhip_download_potential(self._h, _ptr(phi)), "murbhip_download_potential")
        return phi

    def potential_energy(self):
        """-1/2 sum_i m_i phi_i of the remembered evaluation, summed in fp64 on the device (option "potential" 1); also while a
        block is open, where energy() refuses."""
        w = C.c_double()
        _check(lib().murbhip_potential_energy(self._h, C.byref(w)), "murbhip_potential_energy")
        return w.value

    _FIELD_KEYS = ("ax", "ay", "az", "jx", "jy", "jz", "phi")

    def field_at(self, points, velocities=None, skip=None):
        """Acceleration, jerk and potential the bodies make at `points` (3, count), moving with `velocities` (3, count; None = at
        rest), with body skip[k] (or none: -1, or skip=None) left out for point k (include/murbfield.h: murbfield_at).  A dict of
        float32 arrays ax ay az jx jy jz phi.  A read-out: synchronous, changes nothing of the simulation."""
        p = [_f32(x) for x in points]
        v = [_f32(x) for x in velocities] if velocities is not None else None
        count = p[0].shape[0]
        if len(p) != 3 or any(x.shape != (count,) for x in p + (v or [])) or (v is not None and len(v) != 3):
            raise ValueError("points and velocities are three arrays of one length each")
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            if sk.shape != (count,):
                raise ValueError("skip has one entry per point")
        out = {k: np.zeros(count, np.float32) for k in self._FIELD_KEYS}
        _check(lib().murbfield_at(self._h, count, *[_ptr(x) for x in p], *([_ptr(x) for x in v] if v else [None] * 3),
                                      sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None,
                                      *[_ptr(out[k]) for k in self._FIELD_KEYS]), "murbfield_at")
        return out

    def field_of(self, bodies):
        """field_at at the listed bodies' own current positions and velocities, each with itself left out (include/murbfield.h:
        murbfield_of); the gather happens on the device."""
        b = np.ascontiguousarray(bodies, np.int32).reshape(-1)
        out = {k: np.zeros(b.shape[0], np.float32) for k in self._FIELD_KEYS}
        _check(lib().murbfield_of(self._h, b.shape[0], b.ctypes.data_as(C.POINTER(C.c_int)), *[_ptr(out[k]) for k in self._FIELD_KEYS]),
               "murbfield_of")
        return out

    def tidal_at(self, points, skip=None):
        """The tidal tensor d a_a / d p_b the bodies make at `points` (3, count), with body skip[k] (or none: -1, or skip=None)
        left out for point k (include/murbtidal.h: murbtidal_at).  A dict of float32 arrays txx tyy tzz txy txz tyz
        (tidal_matrix() makes the 3 x 3 matrices).  A read-out: synchronous, changes nothing of the simulation."""
        p = [_f32(x) for x in points]
        count = p[0].shape[0]
        if len(p) != 3 or any(x.shape != (count,) for x in p):
            raise ValueError("points are three arrays of one length")
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            if sk.shape != (count,):
                raise ValueError("skip has one entry per point")
        out = {k: np.zeros(count, np.float32) for k in TIDAL_KEYS}
        _check(lib().murbtidal_at(self._h, count, *[_ptr(x) for x in p], sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None,
                                  *[_ptr(out[k]) for k in TIDAL_KEYS]), "murbtidal_at")
        return out

    def tidal_of(self, bodies):
        """tidal_at at the listed bodies' own current positions, each with itself left out (include/murbtidal.h: murbtidal_of);
        the gather happens on the device."""
        b = np.ascontiguousarray(bodies, np.int32).reshape(-1)
        out = {k: np.zeros(b.shape[0], np.float32) for k in TIDAL_KEYS}
        _check(lib().murbtidal_of(self._h, b.shape[0], b.ctypes.data_as(C.POINTER(C.c_int)), *[_ptr(out[k]) for k in TIDAL_KEYS]),
               "murbtidal_of")
        return out

    # -- k nearest neighbours and densities (include/murbknn.h)
    def _knn_bodies(self, bodies):
        if bodies is None:
            return self.n, None
        b = np.ascontiguousarray(bodies, np.int32).reshape(-1)
        return b.shape[0], b.ctypes.data_as(C.POINTER(C.c_int))

    def knn_of(self, bodies=None, k=6):
        """(idx (count, k) int32, r2 (count, k) float32): the k nearest other bodies of the listed bodies (None: all, in order) by
        (r2, index), r2 the sweeps' |d|^2 + soft^2; -1 / +inf where there are fewer (include/murbknn.h: murbknn_of).  A read-out:
        synchronous, changes nothing of the simulation."""
        count, bp = self._knn_bodies(bodies)
        idx, r2 = np.full((count, max(k, 0)), -1, np.int32), np.full((count, max(k, 0)), np.inf, np.float32)
        _check(lib().murbknn_of(self._h, k, count, bp, idx.ctypes.data_as(C.POINTER(C.c_int)), _ptr(r2)), "murbknn_of")
        return idx, r2

    def knn_at(self, points, k=6, skip=None):
        """knn_of at `points` (3, count) of the caller's, with body skip[p] (or none: -1, or skip=None) no candidate of point p
        (include/murbknn.h: murbknn_at)."""
        p = [_f32(x) for x in points]
        count = p[0].shape[0]
        if len(p) != 3 or any(x.shape != (count,) for x in p):
            raise ValueError("points are three arrays of one length")
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            if sk.shape != (count,):
                raise ValueError("skip has one entry per point")
        idx, r2 = np.full((count, max(k, 0)), -1, np.int32), np.full((count, max(k, 0)), np.inf, np.float32)
        _check(lib().murbknn_at(self._h, k, count, *[_ptr(x) for x in p], sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None,
                                idx.ctypes.data_as(C.POINTER(C.c_int)), _ptr(r2)), "murbknn_at")
        return idx, r2

    def density(self, k=6, bodies=None):
        """float32 local density of the listed bodies (None: all, in order): the mass of a body's k - 1 nearest over the sphere
        through its k-th (include/murbknn.h: murbdensity_of)."""
        count, bp = self._knn_bodies(bodies)
        rho = np.zeros(count, np.float32)
        _check(lib().murbdensity_of(self._h, k, count, bp, _ptr(rho)), "murbdensity_of")
        return rho

    def density_centre(self, k=6):
        """dict of the density centre x (3,), the core radius r_core, the core density rho_core, rho_sum, and the counts of bodies
        used and left_out (those k - 1 others share a point with) (include/murbknn.h: murbdensity_centre)."""
        out = (C.c_double * 8)()
        _check(lib().murbdensity_centre(self._h, k, out), "murbdensity_centre")
        return _centre_dict(out[:])

    # -- bound pairs (include/murbbind.h)
    def bound_partner_of(self, bodies=None):
        """(partner int32, h float32) of the listed bodies (None: all, in order): the other body with the smallest specific
        two-body energy h = w^2 / 2 - G (m_i + m_j) / sqrt(d^2 + soft^2) by (h, index); -1 / +inf where there is none
        (include/murbbind.h: murbbind_of).  A read-out: synchronous, changes nothing of the simulation."""
        count, bp = self._knn_bodies(bodies)
        partner, h = np.full(count, -1, np.int32), np.full(count, np.inf, np.float32)
        _check(lib().murbbind_of(self._h, count, bp, partner.ctypes.data_as(C.POINTER(C.c_int)), _ptr(h)), "murbbind_of")
        return partner, h

    def bound_partner_at(self, points, velocities=None, masses=None, skip=None):
        """bound_partner_of for probes of the caller's at `points` (3, count) with `velocities` (3, count; None: at rest) and
        `masses` (count; None: massless), with body skip[p] (or none: -1, or skip=None) no candidate of point p
        (include/murbbind.h: murbbind_at)."""
        p = [_f32(x) for x in points]
        count = p[0].shape[0]
        if len(p) != 3 or any(x.shape != (count,) for x in p):
            raise ValueError("points are three arrays of one length")
        v = [None] * 3
        if velocities is not None:
            v = [_f32(x) for x in velocities]
            if len(v) != 3 or any(x.shape != (count,) for x in v):
                raise ValueError("velocities are three arrays, one entry per point")
        m = None
        if masses is not None:
            m = _f32(masses)
            if m.shape != (count,):
                raise ValueError("masses has one entry per point")
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            if sk.shape != (count,):
                raise ValueError("skip has one entry per point")
        partner, h = np.full(count, -1, np.int32), np.full(count, np.inf, np.float32)
        opt = lambda x: _ptr(x) if x is not None else None
        _check(lib().murbbind_at(self._h, count, *[_ptr(x) for x in p], *[opt(x) for x in v], opt(m),
                                 sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None,
                                 partner.ctypes.data_as(C.POINTER(C.c_int)), _ptr(h)), "murbbind_at")
        return partner, h

    def binaries(self):
        """dict of the bound pairs (mutual most bound partners with h < 0), i < j ascending in i: arrays i, j (int32) and a, e,
        period, h, energy, r (float64, from the float32 state), plus "census": pairs, energy_sum, hardest_i, hardest_j,
        hardest_energy, a_min, bound_bodies (bodies whose partner has h < 0, mutual or not), mutual_pairs
        (include/murbbind.h: murbbind_pairs).  The count-only call, then the sized one."""
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        count, out8 = C.c_ulong(), (C.c_double * 8)()
        _check(lib().murbbind_pairs(self._h, None, None, None, 0, C.byref(count), out8), "murbbind_pairs")
        pairs = int(count.value)
        i, j, elems = np.zeros(pairs, np.int32), np.zeros(pairs, np.int32), np.zeros((pairs, 6), np.float64)
        if pairs:
            _check(lib().murbbind_pairs(self._h, i.ctypes.data_as(ip), j.ctypes.data_as(ip), elems.ctypes.data_as(dp), pairs,
                                        C.byref(count), out8), "murbbind_pairs")
        return _binaries_dict(i, j, elems, out8[:])

    # -- potential of a subset and bound members (include/murbbound.h)
    def potential_of(self, bodies=None, member=None):
        """phi float32 of the listed bodies (None: all, in order): the sum of G m_j / sqrt(d^2 + soft^2) over the other bodies, or
        over those of them the mask `member` (n entries, nonzero = in; None: all) lets in; positive, like the field read-out's
        phi and bit for bit its value (include/murbbound.h: murbpot_of).  A read-out: synchronous, changes nothing."""
        count, bp = self._knn_bodies(bodies)
        _, mp = _mask(member, self.n)
        phi = np.zeros(count, np.float32)
        _check(lib().murbpot_of(self._h, count, bp, mp, _ptr(phi)), "murbpot_of")
        return phi

    def potential_at(self, points, skip=None, member=None):
        """potential_of at `points` (3, count) of the caller's, with body skip[p] (or none: -1, or skip=None) left out of point p
        (include/murbbound.h: murbpot_at)."""
        p = [_f32(x) for x in points]
        count = p[0].shape[0]
        if len(p) != 3 or any(x.shape != (count,) for x in p):
            raise ValueError("points are three arrays of one length")
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            if sk.shape != (count,):
                raise ValueError("skip has one entry per point")
        _, mp = _mask(member, self.n)
        phi = np.zeros(count, np.float32)
        _check(lib().murbpot_at(self._h, count, *[_ptr(x) for x in p], sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None,
                                mp, _ptr(phi)), "murbpot_at")
        return phi

    def bound_members(self, start=None, frame_v=None, max_iter=64):
        """dict of the bound members by iterative unbinding from the mask `start` (None: all bodies) in the members' own
        centre-of-mass frame (or the fixed velocity `frame_v`), at most max_iter rounds: member (bool, n), e (float64, n: the
        energy per unit mass of every body against the final members), members, mass, rounds, converged, v, centre, vx .. cz,
        kinetic, potential, virial_ratio, removed, unbound_bodies (include/murbbound.h: murbbound_members)."""
        _, sp = _mask(start, self.n)
        fv = None
        if frame_v is not None:
            fv = np.ascontiguousarray(frame_v, np.float64).reshape(-1)
            if fv.shape != (3,):
                raise ValueError("frame_v has three components")
        dp = C.POINTER(C.c_double)
        member, e, out16 = np.zeros(self.n, np.uint8), np.zeros(self.n, np.float64), (C.c_double * 16)()
        _check(lib().murbbound_members(self._h, sp, fv.ctypes.data_as(dp) if fv is not None else None, int(max_iter),
                                       member.ctypes.data_as(C.POINTER(C.c_ubyte)), e.ctypes.data_as(dp), out16), "murbbound_members")
        return _bound_dict(member, e, out16[:])

    # -- nearest body of another label, the minimum spanning tree (include/murbmst.h)
    def foreign_nearest(self, labels, bodies=None):
        """(partner int32, r2 float32) of the listed bodies (None: all, in order): the nearest body of ANOTHER label by (r2, index)
        among the bodies with label >= 0; `labels` holds one int per body, < 0 puts a body outside (never a candidate; as a point
        -1 / +inf); -1 / +inf where there is none (include/murbmst.h: murbforeign_of).  A read-out: synchronous, changes
        nothing of the simulation."""
        lab = np.ascontiguousarray(labels, np.int32).reshape(-1)
        if lab.shape != (self.n,):
            raise ValueError("labels has one entry per body")
        count, bp = self._knn_bodies(bodies)
        partner, r2 = np.full(count, -1, np.int32), np.full(count, np.inf, np.float32)
        ip = C.POINTER(C.c_int)
        _check(lib().murbforeign_of(self._h, count, bp, lab.ctypes.data_as(ip), partner.ctypes.data_as(ip), _ptr(r2)), "murbforeign_of")
        return partner, r2

    def spanning_tree(self, member=None):
        """dict of the minimum spanning forest of the bodies the mask `member` lets in (None: all) under the key (r2, min(i, j),
        max(i, j)): edges i < j (int32), r2 (float32), length (float64, from the float32 coordinates) ascending by the key;
        label (int32, n: the smallest member index of the body's component, -1 outside the mask); members, edges, components,
        rounds, total_length, mean_length, longest_length (include/murbmst.h: murbmst_of).  The arrays are sized for
        members - 1 edges, which always serves."""
        mk, mp = _mask(member, self.n)
        cap = max((self.n if mk is None else int(mk.sum())) - 1, 0)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        i, j = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        r2, length = np.zeros(cap, np.float32), np.zeros(cap, np.float64)
        label, out8 = np.zeros(self.n, np.int32), (C.c_double * 8)()
        _check(lib().murbmst_of(self._h, mp, cap, i.ctypes.data_as(ip), j.ctypes.data_as(ip), _ptr(r2), length.ctypes.data_as(dp),
                                label.ctypes.data_as(ip), out8), "murbmst_of")
        d = dict(zip(MST_KEYS, out8[:7]))
        for key in ("members", "edges", "components", "rounds"):
            d[key] = int(d[key])
        e = d["edges"]
        d.update({"i": i[:e], "j": j[:e], "r2": r2[:e], "length": length[:e], "label": label})
        return d

    # -- pair separations (include/murbsep.h)
    def _sep_call(self, name, head, count, member, bins):
        _, mp = _mask(member, self.n)
        lo_exp, sub, nb = (0, 0, 0) if bins is None else (int(v) for v in bins)
        if bins is not None and nb < 1:
            raise ValueError("bins is a (lo_exp, sub, bins) triple with at least one bin, or None")
        qp = C.POINTER(C.c_ulonglong)
        total = np.zeros(count, np.float64)
        hist, out4 = np.zeros(nb, np.uint64), np.zeros(4, np.uint64)
        _check(getattr(lib(), name)(*head, mp, total.ctypes.data_as(C.POINTER(C.c_double)), lo_exp, sub, nb,
                                    hist.ctypes.data_as(qp) if nb else None, out4.ctypes.data_as(qp) if nb else None), name)
        if bins is None:
            return total, None, None
        return total, hist, dict(zip(SEP_KEYS, (int(v) for v in out4[:3])))

    def separation_of(self, bodies=None, member=None, bins=None):
        """(sum, hist, out4) of the listed bodies (None: all, in order) against the bodies the mask `member` lets in (None: all).
        sum: float64 per listed body, the sum of its fp32 distances (unsoftened) to those bodies; itself adds 0.  bins: None, or
        a (lo_exp, sub, bins) triple: hist (uint64, bins) counts the call's ordered (listed body, body) pairs by the float bits of
        d2, from d2 = 2^lo_exp up with 2^sub bins per octave (separation_edges gives the edges), and out4 is a dict of pairs,
        below, above with below + hist.sum() + above == pairs; a listed body's own entry is left out.  Without bins hist and out4
        are None (include/murbsep.h: murbsep_of).  A read-out: synchronous, changes nothing."""
        count, bp = self._knn_bodies(bodies)
        return self._sep_call("murbsep_of", (self._h, count, bp), count, member, bins)

    def separation_at(self, points, member=None, bins=None):
        """separation_of at `points` (3, count) of the caller's.  No body is skipped: a point on a body gets 0 from it and one
        entry in below (include/murbsep.h: murbsep_at)."""
        p = [_f32(x) for x in points]
        count = p[0].shape[0]
        if len(p) != 3 or any(x.shape != (count,) for x in p):
            raise ValueError("points are three arrays of one length")
        return self._sep_call("murbsep_at", (self._h, count, *[_ptr(x) for x in p]), count, member, bins)

    def mean_separation(self, member=None):
        """The mean pair separation of the M members (None: all): the members' separation_of sums against the members, added in
        index order in fp64, over M (M - 1).  NaN for fewer than 2 members."""
        mk, _ = _mask(member, self.n)
        members = np.arange(self.n, dtype=np.int32) if mk is None else np.flatnonzero(mk).astype(np.int32)
        m = int(members.shape[0])
        if m < 2:
            return float("nan")
        sums, _, _ = self.separation_of(None if mk is None else members, member=member)
        total = 0.0
        for v in sums:
            total += float(v)
        return total / (m * (m - 1.0))

    def q_parameter(self, member=None):
        """dict of Cartwright & Whitworth 2004's Q of the M members (None: all) in the 3-D convention: q = m_bar / s_bar with
        R the largest fp64 distance of a member from the members' unweighted mean position (from the float32 coordinates),
        s_bar = mean_separation / R, and m_bar = the spanning tree's mean edge length over (M^2 * 4/3 pi R^3)^(1/3) / (M - 1),
        the 3-D analogue of the 2-D (M A)^(1/2) / (M - 1).  Also m_bar, s_bar, radius, members.  NaN for fewer than 2 members.
        Composed from spanning_tree and mean_separation."""
        mk, _ = _mask(member, self.n)
        members = np.arange(self.n) if mk is None else np.flatnonzero(mk)
        m = int(members.shape[0])
        nan = float("nan")
        if m < 2:
            return {"q": nan, "m_bar": nan, "s_bar": nan, "radius": nan, "members": m}
        st = self.state()
        q = np.stack([st[k].astype(np.float64)[members] for k in ("qx", "qy", "qz")])
        d = q - q.mean(axis=1, keepdims=True)
        radius = float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).max())
        s_bar = self.mean_separation(member) / radius
        volume = 4.0 / 3.0 * np.pi * radius ** 3
        m_bar = self.spanning_tree(member)["mean_length"] / ((float(m) ** 2 * volume) ** (1.0 / 3.0) / (m - 1.0))
        return {"q": m_bar / s_bar, "m_bar": m_bar, "s_bar": s_bar, "radius": radius, "members": m}

    def mass_segregation_ratio(self, n_mst, sets=50, seed=0, member=None):
        """dict of Allison et al. 2009's mass segregation ratio of the members (None: all): ratio, the mean tree length of
        `sets` random sets of n_mst members over the tree length of the n_mst most massive (by mass descending, index
        ascending); sigma, the random lengths' standard deviation over the massive length; length_massive; lengths_random.
        Each draw is numpy.random.default_rng(seed).choice(members, n_mst, replace=False), in sequence from one generator.
        Composed from spanning_tree(member=...): sets + 1 trees of n_mst points per round each."""
        mk, _ = _mask(member, self.n)
        members = np.arange(self.n) if mk is None else np.flatnonzero(mk)
        n_mst = int(n_mst)
        if not 2 <= n_mst <= members.shape[0]:
            raise ValueError("n_mst is at least 2 and at most the members")
        m = self.masses()[members]
        heavy = members[np.lexsort((members, -m.astype(np.float64)))[:n_mst]]

        def tree_length(who):
            mask = np.zeros(self.n, np.uint8)
            mask[who] = 1
            return self.spanning_tree(member=mask)["total_length"]

        massive = tree_length(heavy)
        rng = np.random.default_rng(seed)
        lengths = np.array([tree_length(rng.choice(members, n_mst, replace=False)) for _ in range(int(sets))])
        return {"ratio": lengths.mean() / massive, "sigma": lengths.std() / massive, "length_massive": massive, "lengths_random": lengths}

    # -- neighbours within a radius (include/murbnbr.h)
    def _nbr_radii(self, h, count):
        """(h array pointer or None, h_all) of a scalar or of one radius per point."""
        if np.ndim(h) == 0:
            return None, None, float(np.float32(h))
        ha = _f32(h)
        if ha.shape != (count,):
            raise ValueError("h is a scalar or has one entry per point")
        return ha, _ptr(ha), 0.0

    def _nbr_call(self, name, head, count, lists):
        """The count-only call, then the call sized from its offsets."""
        fn = getattr(lib(), name)
        up = C.POINTER(C.c_ulong)
        offsets = np.zeros(count + 1, np.uint64)
        _check(fn(*head, offsets.ctypes.data_as(up), None, None, 0), name)
        if not lists:
            return offsets, None, None
        total = int(offsets[count])
        idx, r2 = np.zeros(total, np.int32), np.zeros(total, np.float32)
        if total:
            _check(fn(*head, offsets.ctypes.data_as(up), idx.ctypes.data_as(C.POINTER(C.c_int)), _ptr(r2), total), name)
        return offsets, idx, r2

    def neighbours_of(self, bodies=None, h=0.0, lists=True):
        """(offsets (count + 1) uint64, idx int32, r2 float32): the other bodies within h (a scalar, or one radius per listed body)
        of the listed bodies (None: all, in order), in CSR form: body p's neighbours are idx[offsets[p]:offsets[p + 1]] in
        ascending index, r2 the sweeps' |d|^2 + soft^2, a neighbour having r2 <= neighbour_threshold(h, soft)
        (include/murbnbr.h: murbnbr_of).  lists=False: the counts alone, (offsets, None, None).  A read-out: synchronous,
        changes nothing of the simulation."""
        count, bp = self._knn_bodies(bodies)
        keep, hp, h_all = self._nbr_radii(h, count)
        return self._nbr_call("murbnbr_of", (self._h, count, bp, hp, h_all), count, lists)

    def neighbours_at(self, points, h, skip=None, lists=True):
        """neighbours_of at `points` (3, count) of the caller's, with body skip[p] (or none: -1, or skip=None) no candidate of
        point p (include/murbnbr.h: murbnbr_at)."""
        p = [_f32(x) for x in points]
        count = p[0].shape[0]
        if len(p) != 3 or any(x.shape != (count,) for x in p):
            raise ValueError("points are three arrays of one length")
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            if sk.shape != (count,):
                raise ValueError("skip has one entry per point")
        keep, hp, h_all = self._nbr_radii(h, count)
        head = (self._h, count, *[_ptr(x) for x in p], sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None, hp, h_all)
        return self._nbr_call("murbnbr_at", head, count, lists)

    def set_neighbour_option(self, key, value):
        """"list_entries" of neighbours_of() and neighbours_at() (include/murbnbr.h: murbnbr_set_option)."""
        _check(lib().murbnbr_set_option(self._h, key.encode(), int(value)), f"murbnbr_set_option({key})")

    def neighbour_option(self, key):
        """The value of a neighbour option in force, defaults resolved (include/murbnbr.h: murbnbr_get_option)."""
        f = C.c_long()
        _check(lib().murbnbr_get_option(self._h, key.encode(), C.byref(f)), f"murbnbr_get_option({key})")
        return f.value

    # -- the field of listed bodies and the neighbour split (include/murblist.h)
    def list_field_of(self, bodies, offsets, idx):
        """field_of's dict from LISTED source bodies alone: body bodies[p] (None: all, in order) feels the bodies
        idx[offsets[p]:offsets[p + 1]], exactly as given: no entry is skipped, the body itself counts where it is listed, a
        duplicate counts twice, and the order of the entries decides the order of the fp32 sum (include/murblist.h:
        murblist_of).  O(list length) per point.  A read-out: synchronous, changes nothing of the simulation."""
        count, bp = self._knn_bodies(bodies)
        o, j = _csr(offsets, idx, count)
        out = {k: np.zeros(count, np.float32) for k in self._FIELD_KEYS}
        _check(lib().murblist_of(self._h, count, bp, o.ctypes.data_as(C.POINTER(C.c_ulong)), j.ctypes.data_as(C.POINTER(C.c_int)),
                                 *[_ptr(out[k]) for k in self._FIELD_KEYS]), "murblist_of")
        return out

    def list_field_at(self, points, velocities, offsets, idx):
        """list_field_of at `points` (3, count) of the caller's, moving with `velocities` (3, count; None = at rest)
        (include/murblist.h: murblist_at)."""
        p = [_f32(x) for x in points]
        v = [_f32(x) for x in velocities] if velocities is not None else None
        count = p[0].shape[0]
        if len(p) != 3 or any(x.shape != (count,) for x in p + (v or [])) or (v is not None and len(v) != 3):
            raise ValueError("points and velocities are three arrays of one length each")
        o, j = _csr(offsets, idx, count)
        out = {k: np.zeros(count, np.float32) for k in self._FIELD_KEYS}
        _check(lib().murblist_at(self._h, count, *[_ptr(x) for x in p], *([_ptr(x) for x in v] if v else [None] * 3),
                                 o.ctypes.data_as(C.POINTER(C.c_ulong)), j.ctypes.data_as(C.POINTER(C.c_int)),
                                 *[_ptr(out[k]) for k in self._FIELD_KEYS]), "murblist_at")
        return out

    def irregular_field_of(self, bodies=None, h=0.0):
        """(counts uint64, dict): the field the neighbours within h (a scalar, or one radius per listed body) make at the listed
        bodies (None: all, in order): list_field_of on neighbours_of's lists, bit for bit, with the lists produced and consumed
        on the device (include/murblist.h: murbsplit_of)."""
        count, bp = self._knn_bodies(bodies)
        keep, hp, h_all = self._nbr_radii(h, count)
        counts = np.zeros(count, np.uint64)
        out = {k: np.zeros(count, np.float32) for k in self._FIELD_KEYS}
        _check(lib().murbsplit_of(self._h, count, bp, hp, h_all, counts.ctypes.data_as(C.POINTER(C.c_ulong)),
                                  *[_ptr(out[k]) for k in self._FIELD_KEYS]), "murbsplit_of")
        return counts, out

    def force_split(self, h, bodies=None):
        """dict of the Ahmad-Cohen split of the listed bodies' (None: all) force at neighbour radius h: counts (uint64, the
        neighbours), irregular (the neighbours' field, murbsplit_of), total (field_of: all other bodies) and regular =
        total - irregular, formed in fp64 on the host and rounded once; the three are field_of's dicts."""
        who = np.arange(self.n, dtype=np.int32) if bodies is None else np.ascontiguousarray(bodies, np.int32).reshape(-1)
        counts, irregular = self.irregular_field_of(bodies, h)
        total = self.field_of(who)
        return {"counts": counts, "irregular": irregular, "total": total, "regular": split_regular(total, irregular)}

    # -- the Ahmad-Cohen neighbour scheme (include/murbac.h)
    def ac_begin(self, h, n_irr):
        """Start an Ahmad-Cohen scheme at the current state: neighbour radius h (a scalar, or one radius per body), a full sweep
        on every n_irr-th step of ac_steps() (include/murbac.h: murbac_begin; "integrator" must be 2)."""
        keep, hp, h_all = self._nbr_radii(h, self.n)
        _check(lib().murbac_begin(self._h, hp, h_all, int(n_irr)), "murbac_begin")

    def ac_steps(self, dt, steps):
        """`steps` Hermite steps of size dt of the live scheme (murbac_steps; enqueue only, sync() waits)."""
        _check(lib().murbac_steps(self._h, dt, int(steps)), "murbac_steps")

    def ac_end(self):
        _check(lib().murbac_end(self._h), "murbac_end")

    def ac_state(self):
        """dict of the live scheme: n_irr, m (steps since the last regular one), steps, regular_steps, entries, longest, empty
        (ints), mean (entries per list) and time (the fp64 sum of the steps' dt since ac_begin); all 0 without one."""
        out = (C.c_double * 16)()
        _check(lib().murbac_state(self._h, out), "murbac_state")
        d = {k: int(out[e]) for e, k in enumerate(AC_STATE_KEYS[:7])}
        d["mean"], d["time"] = out[7], out[8]
        return d

    def ac_lists(self):
        """(offsets (n + 1) uint64, idx int32): the scheme's resident lists in CSR form (murbac_lists); syncs."""
        up = C.POINTER(C.c_ulong)
        offsets = np.zeros(self.n + 1, np.uint64)
        _check(lib().murbac_lists(self._h, offsets.ctypes.data_as(up), None, 0), "murbac_lists")
        total = int(offsets[self.n])
        idx = np.zeros(total, np.int32)
        if total:
            _check(lib().murbac_lists(self._h, offsets.ctypes.data_as(up), idx.ctypes.data_as(C.POINTER(C.c_int)), total), "murbac_lists")
        return offsets, idx

    def ac_forces(self):
        """dict of (3, n) float32 arrays of the live scheme (murbac_forces; syncs): aI, jI at the current time; aR, jR, a2R, a3R
        at the time of the last regular step."""
        planes = np.zeros((18, self.n), np.float32)
        groups = []
        for first, count in ((0, 6), (6, 6), (12, 3), (15, 3)):
            groups.append((_fp * count)(*[_ptr(planes[first + k]) for k in range(count)]))
        _check(lib().murbac_forces(self._h, *groups), "murbac_forces")
        return {k: planes[3 * e:3 * e + 3] for e, k in enumerate(("aI", "jI", "aR", "jR", "a2R", "a3R"))}

    def ac_radii(self, k):
        """float32 radii, one per body, for ac_begin(): the distance to the body's k-th nearest neighbour (knn_of's k-th column),
        nudged up ulp by ulp until neighbour_threshold() takes that neighbour in, so that body i's list has at least k entries."""
        k = int(k)
        if not 1 <= k <= self.n - 1:
            raise ValueError("k is at least 1 and at most n - 1")
        soft2 = np.float32(self.soft) * np.float32(self.soft)
        if k > KNN_KMAX:   # beyond knn_of's columns: the KNN_KMAX-th distance scaled as for a uniform density, then grown by the counts
            h = (self.ac_radii(KNN_KMAX).astype(np.float64) * (k / KNN_KMAX) ** (1.0 / 3.0)).astype(np.float32)
            for _ in range(200):
                short = np.diff(self.neighbours_of(None, h, lists=False)[0].astype(np.int64)) < k
                if not short.any():
                    return h
                h[short] *= np.float32(1.1)
            raise RuntimeError("ac_radii did not reach k entries per list")
        r2 = self.knn_of(None, k)[1][:, k - 1]
        h = np.sqrt(np.maximum(r2.astype(np.float64) - float(soft2), 0.0)).astype(np.float32)
        for _ in range(64):
            thr = (h.astype(np.float64) * h.astype(np.float64) + np.float64(soft2)).astype(np.float32)   # neighbour_threshold's formula
            short = thr < r2
            if not short.any():
                break
            h[short] = np.nextafter(h[short], np.float32(np.inf))
        assert all(neighbour_threshold(h[i], self.soft) >= r2[i] for i in np.argsort(h)[[0, -1]])
        return h

    # -- massless tracers (include/murbtracer.h)
    def upload_tracers(self, q, v=None):
        """`q` (3, count) positions and `v` (3, count; None = at rest) velocities of massless test particles at the bodies'
        current model time; replaces any earlier set, count 0 clears (include/murbtracer.h: murbtracer_upload).  The Hermite
        steps (steps() under "integrator" 2, evolve()) carry them along on the device."""
        qa, va = _tracer_arrays(q, v)
        count = qa[0].shape[0]
        _check(lib().murbtracer_upload(self._h, count, *[_ptr(x) for x in qa], *([_ptr(x) for x in va] if va else [None] * 3)),
               "murbtracer_upload")

    def tracer_count(self):
        count = C.c_ulong()
        _check(lib().murbtracer_count(self._h, C.byref(count)), "murbtracer_count")
        return int(count.value)

    def tracers(self):
        """dict of float32 arrays qx qy qz vx vy vz of the resident tracers (murbtracer_download); syncs."""
        out = {k: np.zeros(self.tracer_count(), np.float32) for k in FIELDS[:6]}
        _check(lib().murbtracer_download(self._h, *[_ptr(out[k]) for k in FIELDS[:6]]), "murbtracer_download")
        return out

    def tracer_forces(self):
        """dict of float32 arrays ax ay az jx jy jz: the tracers' remembered evaluation (murbtracer_download_forces); syncs."""
        out = {k: np.zeros(self.tracer_count(), np.float32) for k in self._FIELD_KEYS[:6]}
        _check(lib().murbtracer_download_forces(self._h, *[_ptr(out[k]) for k in self._FIELD_KEYS[:6]]), "murbtracer_download_forces")
        return out

    def compute_tracers(self):
        """(a, j) of the tracers at the current state (murbtracer_compute; enqueue only); read with tracer_forces()."""
        _check(lib().murbtracer_compute(self._h), "murbtracer_compute")

    def clear_tracers(self):
        _check(lib().murbtracer_clear(self._h), "murbtracer_clear")

    def set_tracer_option(self, key, value):
        """"tracer_chunks" / "tracer_batch" / "tracer_dt" (include/murbtracer.h: murbtracer_set_option)."""
        _check(lib().murbtracer_set_option(self._h, key.encode(), int(value)), f"murbtracer_set_option({key})")

    def tracer_option(self, key):
        """The value of a tracer option in force, defaults resolved (murbtracer_get_option)."""
        f = C.c_long()
        _check(lib().murbtracer_get_option(self._h, key.encode(), C.byref(f)), f"murbtracer_get_option({key})")
        return f.value

    def contacts(self):
        """dict of the step that ended the last evolve call by a contact ("contact" 2): i, j (int32), gap2 (float32) sorted by
        i, the count the device saw (the arrays hold at most 4096) and the model time advanced in that call; count 0 otherwise."""
        count, time = C.c_ulong(), C.c_double()
        ip = C.POINTER(C.c_int)
        _check(lib().murbhip_contacts(self._h, None, None, None, 0, C.byref(count), C.byref(time)), "murbhip_contacts")
        kept = min(count.value, 4096)
        i, j, gap2 = np.zeros(kept, np.int32), np.zeros(kept, np.int32), np.zeros(kept, np.float32)
        if kept:
            _check(lib().murbhip_contacts(self._h, i.ctypes.data_as(ip), j.ctypes.data_as(ip), _ptr(gap2), kept, C.byref(count),
                                          C.byref(time)), "murbhip_contacts")
        return {"i": i, "j": j, "gap2": gap2, "count": int(count.value), "time": time.value}

    def integrate_host_acc(self, acc, dt):
        a = [_f32(x) for x in acc]
        _check(lib().murbhip_integrate_host_acc(self._h, *[_ptr(x) for x in a], dt), "murbhip_integrate_host_acc")

    def sync(self):
        _check(lib().murbhip_sync(self._h), "murbhip_sync")

    def energy(self):
        """(kinetic, potential) of the current state, reference definitions (gpu+tracking)."""
        ke, pe = C.c_double(), C.c_double()
        _check(lib().murbhip_energy(self._h, C.byref(ke), C.byref(pe)), "murbhip_energy")
        return ke.value, pe.value

    def moments(self):
        """dict: linear momentum P, angular momentum L, mass-weighted position Mq (3 each) and mass M of
        the caller's own bodies (fp64 host sums)."""
        out = (C.c_double * 10)()
        _check(lib().murbhip_moments(self._h, out), "murbhip_moments")
        v = np.array(out[:])
        return {"P": v[0:3], "L": v[3:6], "Mq": v[6:9], "M": float(v[9])}

    # -- tuning / facts
    def set_option(self, key, value):
        _check(lib().murbhip_set_option(self._h, key.encode(), int(value)), f"murbhip_set_option({key})")

    def set_field_option(self, key, value):
        """"field_chunks" / "field_batch" of field_at() and field_of() (include/murbfield.h: murbfield_set_option)."""
        _check(lib().murbfield_set_option(self._h, key.encode(), int(value)), f"murbfield_set_option({key})")

    def field_option(self, key):
        """The value of a field option in force, defaults resolved (include/murbfield.h: murbfield_get_option)."""
        f = C.c_long()
        _check(lib().murbfield_get_option(self._h, key.encode(), C.byref(f)), f"murbfield_get_option({key})")
        return f.value

    def info(self, key):
        v = C.c_double()
        _check(lib().murbhip_get_info(self._h, key.encode(), C.byref(v)), f"murbhip_get_info({key})")
        return v.value

    def close(self):
        if self._h:
            lib().murbhip_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _tracer_arrays(q, v):
    """The six arrays of an upload of tracers, checked the way murbtracer_upload checks them (murbtracer_validate: host only),
    so that a refused set raises before any device is touched."""
    qa = [_f32(x) for x in q]
    va = [_f32(x) for x in v] if v is not None else None
    if len(qa) != 3 or (va is not None and len(va) != 3) or any(x.ndim != 1 or x.shape != qa[0].shape for x in qa + (va or [])):
        raise ValueError("positions and velocities are three arrays of one length each")
    _check(lib().murbtracer_validate(qa[0].shape[0], *[_ptr(x) for x in qa], *([_ptr(x) for x in va] if va else [None] * 3)),
           "murbtracer_upload")
    return qa, va


def merge_contacts(state, radii, i, j):
    """Host-side resolution of a contact list (Simulation.contacts()): the pairs (i[k], j[k]) are joined transitively into
    groups, and every group becomes ONE body in the place of its lowest index: mass = the sum, position and velocity = the
    mass-weighted means (the plain means for an all-massless group), formed in fp64 and rounded once to fp32, radius =
    cbrt(sum R^3).  The other members are removed; the order of the rest is kept.  n is fixed per context, so the result goes
    into a new Simulation.  Returns (new state dict, new radii, for every old index the new index it went to)."""
    radii = np.asarray(radii, np.float32)
    n = radii.shape[0]
    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in zip(np.asarray(i, np.int64), np.asarray(j, np.int64)):
        if not (0 <= a < n and 0 <= b < n):
            raise ValueError("contact index out of range")
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)   # the root of a group is its lowest index
    root = np.array([find(k) for k in range(n)], np.int64)
    keep = root == np.arange(n)
    index_map = (np.cumsum(keep) - 1)[root].astype(np.int64)
    k_new = int(keep.sum())
    m = np.asarray(state["m"], np.float64)[:n]
    mass = np.zeros(k_new)
    np.add.at(mass, index_map, m)
    members = np.zeros(k_new)
    np.add.at(members, index_map, 1.0)
    massless = mass == 0.0
    weight = np.where(massless[index_map], 1.0, m)          # an all-massless group: the plain mean
    norm = np.where(massless, members, mass)
    out = {}
    for key in FIELDS[:6]:
        acc = np.zeros(k_new)
        np.add.at(acc, index_map, weight * np.asarray(state[key], np.float64)[:n])
        out[key] = (acc / norm).astype(np.float32)
    out["m"] = mass.astype(np.float32)
    r3 = np.zeros(k_new)
    np.add.at(r3, index_map, radii.astype(np.float64) ** 3)
    new_radii = np.cbrt(r3).astype(np.float32)
    if "r" in state:
        out["r"] = new_radii.copy()
    return out, new_radii, index_map


# ====================================================================== host mirror (libmurbhost.so)
# The C++ mirror of the reference's plugin interface (nbody-eurohpc_amd/host/), reached through
# host/capi.cpp.  It provides the product's own initial conditions and lets tests drive
# SimulationNBodyHIP / HIPBodies the way the reference's Catch2 tests drive their CUDA twins.
HOST_LIB_PATH = os.path.join(_HERE, "..", "lib", "libmurbhost.so")
FIELDS = ("qx", "qy", "qz", "vx", "vy", "vz", "m", "r")
_host = None


def host_lib():
    global _host
    if _host is None:
        lib()   # libmurbhost.so depends on libmurbhip.so: load it first (same directory, via rpath too)
        path = os.path.normpath(HOST_LIB_PATH)
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} is missing: build it with `make -C nbody-eurohpc_amd`")
        H = C.CDLL(path)
        H.murbhost_padding.restype = C.c_ulong
        H.murbhost_padding.argtypes = [C.c_ulong, C.c_char_p]
        H.murbhost_init_bodies.argtypes = [C.c_ulong, C.c_char_p, C.c_ulong] + [_fp] * 8
        H.murbhost_integrate.argtypes = [C.c_ulong, C.c_char_p, _fp, _fp, _fp, C.c_float, C.c_int, C.c_int] + [_fp] * 6
        H.murbhost_sim_create.restype = C.c_void_p
        H.murbhost_sim_create.argtypes = [C.c_ulong, C.c_char_p, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_int),
                                          C.c_int]
        H.murbhost_sim_destroy.argtypes = [C.c_void_p]
        H.murbhost_sim_step.argtypes = [C.c_void_p, C.c_int]
        H.murbhost_sim_init_on_device.argtypes = [C.c_void_p, C.c_ulong]
        H.murbhost_sim_n.restype = C.c_ulong
        H.murbhost_sim_n.argtypes = [C.c_void_p]
        H.murbhost_sim_flops_per_ite.restype = C.c_float
        H.murbhost_sim_flops_per_ite.argtypes = [C.c_void_p]
        H.murbhost_sim_allocated_bytes.restype = C.c_float
        H.murbhost_sim_allocated_bytes.argtypes = [C.c_void_p]
        H.murbhost_sim_state.argtypes = [C.c_void_p] + [_fp] * 8
        H.murbhost_sim_acc.argtypes = [C.c_void_p] + [_fp] * 3
        _dp = C.POINTER(C.c_double)
        H.murbhost_tracking_create.restype = C.c_void_p
        H.murbhost_tracking_create.argtypes = [C.c_ulong, C.c_char_p, C.c_float, C.c_float, C.c_int, C.c_int,
                                               C.POINTER(C.c_int), C.c_int]
        H.murbhost_history_rows.argtypes = [C.c_void_p]
        H.murbhost_history_get.argtypes = [C.c_void_p, _dp, _dp, _dp]
        H.murbhost_history_csv.argtypes = [C.c_char_p, C.c_int, _dp, _dp, _dp]
        H.murbhost_sim_history_csv.argtypes = [C.c_void_p, C.c_char_p]
        H.murbhost_sim_substeps.argtypes = [C.c_void_p, _dp]
        H.murbhost_sim_set_block.argtypes = [C.c_void_p, C.c_double, C.c_int]
        H.murbhost_sim_block_counts.argtypes = [C.c_void_p, _dp]
        H.murbhost_sim_set_encounter.argtypes = [C.c_void_p, C.c_float]
        H.murbhost_sim_encounters.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _fp, C.c_ulong,
                                              C.POINTER(C.c_ulong), _dp]
        H.murbhost_sim_set_contact.argtypes = [C.c_void_p, C.c_int, C.c_float]
        H.murbhost_sim_set_potential.argtypes = [C.c_void_p, C.c_int]
        H.murbhost_sim_potential.argtypes = [C.c_void_p, _fp]
        H.murbhost_sim_field_at.argtypes = [C.c_void_p, C.c_ulong] + [_fp] * 6 + [C.POINTER(C.c_int)] + [_fp] * 7
        H.murbhost_sim_tidal_at.argtypes = [C.c_void_p, C.c_ulong] + [_fp] * 3 + [C.POINTER(C.c_int)] + [_fp] * 6
        H.murbhost_sim_density_centre.argtypes = [C.c_void_p, C.c_int, _dp]
        H.murbhost_sim_set_density_centre.argtypes = [C.c_void_p, C.c_int]
        H.murbhost_sim_neighbours_of.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_ulong), C.POINTER(C.c_int), C.c_ulong]
        H.murbhost_sim_binaries.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _dp, C.c_ulong, C.POINTER(C.c_ulong), _dp]
        H.murbhost_sim_bound_members.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), _dp, _dp]
        H.murbhost_sim_spanning_tree.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _fp, _dp, C.c_ulong, _dp]
        H.murbhost_sim_mean_separation.argtypes = [C.c_void_p, _dp]
        H.murbhost_sim_force_split.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_ulong)] + [_fp] * 3
        H.murbhost_sim_set_ac.argtypes = [C.c_void_p, C.c_float, C.c_int]
        H.murbhost_sim_ac_begin.argtypes = [C.c_void_p, C.c_float, C.c_int]
        H.murbhost_sim_ac_steps.argtypes = [C.c_void_p, C.c_float, C.c_int]
        H.murbhost_sim_set_tracers.argtypes =[C.c_void_p, C.c_ulong] + [_fp] * 6
        H.murbhost_sim_get_tracers.argtypes = [C.c_void_p, C.POINTER(C.c_ulong)] + [_fp] * 6
        H.murbhost_sim_contacts.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _fp, C.c_ulong,
                                            C.POINTER(C.c_ulong), _dp]
        _host = H
    return _host


def host_padding(n, scheme="galaxy"):
    return int(host_lib().murbhost_padding(n, scheme.encode()))


def init_bodies(n, scheme="galaxy", seed=0, with_padding=False):
    """The product's initial conditions: host/core/Bodies.cpp (mirror of reference Bodies.cpp:158-257)."""
    tot = n + host_padding(n, scheme)
    a = {k: np.zeros(tot, np.float32) for k in FIELDS}
    host_lib().murbhost_init_bodies(n, scheme.encode(), seed, *[_ptr(a[k]) for k in FIELDS])
    return a if with_padding else {k: v[:n].copy() for k, v in a.items()}


def host_integrate(n, scheme, acc, dt, steps, on_device=False):
    """Bodies / HIPBodies ::updatePositionsAndVelocities(accSoA, dt) applied `steps` times."""
    out = {k: np.zeros(n, np.float32) for k in FIELDS[:6]}
    a = [_f32(x) for x in acc]
    host_lib().murbhost_integrate(n, scheme.encode(), *[_ptr(x) for x in a], dt, steps, int(on_device),
                                  *[_ptr(out[k]) for k in FIELDS[:6]])
    return out


def history_csv(path, energy, ang_momentum, centers):
    """SimulationHistory<double>::saveMetricsToCSV on the given rows (host only; False if the file cannot be opened)."""
    e, a = (np.ascontiguousarray(x, np.float64) for x in (energy, ang_momentum))
    c = np.ascontiguousarray(centers, np.float64).reshape(-1)
    dp = C.POINTER(C.c_double)
    return host_lib().murbhost_history_csv(str(path).encode(), len(e), e.ctypes.data_as(dp), a.ctypes.data_as(dp),
                                           c.ctypes.data_as(dp)) == 0


class HostSim:
    """SimulationNBodyHIP<float> behind HIPBodiesAllocator<float> — the `--im hip+tile[+multi]` plugin."""

    def __init__(self, n, scheme="galaxy", soft=2e8, dt=3600.0, devices=(0,), exchange="rccl", tracking=False,
                 leapfrog=False, integrator=None, eta=0.02, kmax=12, encounter=0.0, contact=False, rscale=1.0, potential=False,
                 tracers=None, density_centre=False, rnb=0.0, nirr=8):
        """integrator=5: `--im hip+hermite+ac`, option 2 driven by murbac_steps (include/murbac.h): an iteration is one step of
        dt of the Ahmad-Cohen scheme with the common neighbour radius rnb and a full sweep on every nirr-th iteration.
        density_centre=True (with tracking=True or an integrator): `--im hip+tracking+density`, the history's density_center
        columns hold density_centre()'s x instead of the centre of mass.
        tracking=True: SimulationNBodyHIPTracking (`--im hip+tracking`; with leapfrog=True `hip+leapfrog`; integrator=
        0, 1 or 2 names the murbhip option "integrator" directly: 2 is `hip+hermite`; 3 is `hip+hermite+adaptive`, option 2
        driven by murbhip_evolve: an iteration advances dt of model time in as many substeps as the criterion asks for; 4 is
        `hip+hermite+block`, option 2 driven by murbhip_evolve_block: an iteration is one block of dt, every body in steps of
        its own size dt 2^-k, k <= kmax, with accuracy parameter eta).  encounter=R (integrator 3 or 4): an iteration ends
        behind the substep in which a body has its nearest neighbour within R; encounters() then has the pairs.  contact=True
        (integrator 3 or 4, not beside encounter=): it ends behind the substep in which two bodies touch, their radii being
        the scheme's times rscale; contacts() then has the pairs.  potential=True (integrator 2, 3 or 4, not beside encounter= or
        contact=): the sweeps keep every body's potential; potential() then has it.  tracers=(q, v) (integrator 2 or 3; v may be
        None: at rest): massless test particles the iterations carry along (Simulation.upload_tracers); tracers() has them."""
        if tracers is not None and integrator not in (2, 3):
            raise ValueError("tracers= needs integrator 2 or 3")
        if tracers is not None:
            tq, tv = _tracer_arrays(*tracers)
        if integrator is None:
            integrator = int(bool(leapfrog))
        if contact and integrator not in (3, 4):
            raise ValueError("contact= needs integrator 3 or 4")
        if contact and encounter:
            raise ValueError("contact= cannot be combined with encounter=")
        if contact and not (np.isfinite(rscale) and rscale > 0):
            raise ValueError("rscale= must be finite and positive")
        if potential and integrator not in (2, 3, 4):
            raise ValueError("potential= needs integrator 2, 3 or 4")
        if potential and (contact or encounter):
            raise ValueError("potential= cannot be combined with encounter= or contact=")
        arr = (C.c_int * len(devices))(*devices)
        self.H = host_lib()
        ex = {"copy": 0, "rccl": 1}[exchange]
        if tracking or integrator:
            self.h = self.H.murbhost_tracking_create(n, scheme.encode(), soft, dt, int(integrator), len(devices), arr, ex)
        else:
            self.h = self.H.murbhost_sim_create(n, scheme.encode(), soft, dt, len(devices), arr, ex)
        self.n = int(self.H.murbhost_sim_n(self.h))
        if integrator == 4:
            self.H.murbhost_sim_set_block(self.h, eta, kmax)
        if integrator == 5:
            if self.H.murbhost_sim_set_ac(self.h, rnb, int(nirr)) != 0:
                raise ValueError("rnb= is finite and not negative, nirr= in [1, 4096]")
        if encounter:
            if self.H.murbhost_sim_set_encounter(self.h, encounter) != 0:
                raise ValueError("encounter= needs integrator 3 or 4")
        if contact:
            if self.H.murbhost_sim_set_contact(self.h, 1, rscale) != 0:
                raise ValueError("contact= needs integrator 3 or 4")
        if potential:
            if self.H.murbhost_sim_set_potential(self.h, 1) != 0:
                raise ValueError("potential= needs integrator 2, 3 or 4")
        if density_centre:
            if self.H.murbhost_sim_set_density_centre(self.h, 1) != 0:
                raise ValueError("density_centre= needs tracking=True or an integrator")
        if tracers is not None:
            _check(self.H.murbhost_sim_set_tracers(self.h, tq[0].shape[0], *[_ptr(x) for x in tq],
                                                   *([_ptr(x) for x in tv] if tv else [None] * 3)), "murbhost_sim_set_tracers")

    def tracers(self):
        """SimulationNBodyHIP::getTracers: dict of float32 arrays qx qy qz vx vy vz of the tracers the plugin carries."""
        count = C.c_ulong()
        _check(self.H.murbhost_sim_get_tracers(self.h, C.byref(count), *([None] * 6)), "murbhost_sim_get_tracers")
        out = {k: np.zeros(count.value, np.float32) for k in FIELDS[:6]}
        _check(self.H.murbhost_sim_get_tracers(self.h, C.byref(count), *[_ptr(out[k]) for k in FIELDS[:6]]), "murbhost_sim_get_tracers")
        return out

    def potential(self):
        """potential=True: float32 phi_i of every body in the last sweep (Simulation.potential; after an iteration: of its last
        substep's predicted end state); None where the feature does not apply or before the first sweep."""
        phi = np.zeros(self.n, np.float32)
        if self.H.murbhost_sim_potential(self.h, _ptr(phi)) != 0:
            return None
        return phi

    def field_at(self, points, velocities=None, skip=None):
        """SimulationNBodyHIP::fieldAt: Simulation.field_at on the plugin's bodies as they are on the device."""
        p = [_f32(x) for x in points]
        v = [_f32(x) for x in velocities] if velocities is not None else None
        count = p[0].shape[0]
        sk = np.ascontiguousarray(skip, np.int32) if skip is not None else None
        out = {k: np.zeros(count, np.float32) for k in Simulation._FIELD_KEYS}
        rc = self.H.murbhost_sim_field_at(self.h, count, *[_ptr(x) for x in p], *([_ptr(x) for x in v] if v else [None] * 3),
                                          sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None,
                                          *[_ptr(out[k]) for k in Simulation._FIELD_KEYS])
        _check(rc, "murbhost_sim_field_at")
        return out

    def tidal_at(self, points, skip=None):
        """SimulationNBodyHIP::tidalAt: Simulation.tidal_at on the plugin's bodies as they are on the device."""
        p = [_f32(x) for x in points]
        count = p[0].shape[0]
        sk = np.ascontiguousarray(skip, np.int32) if skip is not None else None
        out = {k: np.zeros(count, np.float32) for k in TIDAL_KEYS}
        rc = self.H.murbhost_sim_tidal_at(self.h, count, *[_ptr(x) for x in p],
                                          sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None,
                                          *[_ptr(out[k]) for k in TIDAL_KEYS])
        _check(rc, "murbhost_sim_tidal_at")
        return out

    def density_centre(self, k=6):
        """SimulationNBodyHIP::densityCentre: Simulation.density_centre on the plugin's bodies as they are on the device."""
        out = (C.c_double * 8)()
        _check(self.H.murbhost_sim_density_centre(self.h, k, out), "murbhost_sim_density_centre")
        return _centre_dict(out[:])

    def neighbours_of(self, h):
        """SimulationNBodyHIP::neighboursOf: (offsets, idx) of Simulation.neighbours_of(h=h) for all of the plugin's bodies as they
        are on the device."""
        up, ip = C.POINTER(C.c_ulong), C.POINTER(C.c_int)
        offsets = np.zeros(self.n + 1, np.uint64)
        _check(self.H.murbhost_sim_neighbours_of(self.h, float(np.float32(h)), offsets.ctypes.data_as(up), None, 0), "murbhost_sim_neighbours_of")
        idx = np.zeros(int(offsets[self.n]), np.int32)
        if idx.size:
            _check(self.H.murbhost_sim_neighbours_of(self.h, float(np.float32(h)), offsets.ctypes.data_as(up), idx.ctypes.data_as(ip), idx.size),
                   "murbhost_sim_neighbours_of")
        return offsets, idx

    def binaries(self):
        """SimulationNBodyHIP::binaries: Simulation.binaries() for the plugin's bodies as they are on the device."""
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        count, out8 = C.c_ulong(), (C.c_double * 8)()
        _check(self.H.murbhost_sim_binaries(self.h, None, None, None, 0, C.byref(count), out8), "murbhost_sim_binaries")
        pairs = int(count.value)
        i, j, elems = np.zeros(pairs, np.int32), np.zeros(pairs, np.int32), np.zeros((pairs, 6), np.float64)
        if pairs:
            _check(self.H.murbhost_sim_binaries(self.h, i.ctypes.data_as(ip), j.ctypes.data_as(ip), elems.ctypes.data_as(dp), pairs,
                                                C.byref(count), out8), "murbhost_sim_binaries")
        return _binaries_dict(i, j, elems, out8[:])

    def bound_members(self, max_iter=64):
        """SimulationNBodyHIP::boundMembers: Simulation.bound_members() for the plugin's bodies as they are on the device."""
        member, e, out16 = np.zeros(self.n, np.uint8), np.zeros(self.n, np.float64), (C.c_double * 16)()
        _check(self.H.murbhost_sim_bound_members(self.h, int(max_iter), member.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                 e.ctypes.data_as(C.POINTER(C.c_double)), out16), "murbhost_sim_bound_members")
        return _bound_dict(member, e, out16[:])

    def spanning_tree(self):
        """SimulationNBodyHIP::spanningTree: Simulation.spanning_tree() of all the plugin's bodies as they are on the device
        (without the labels)."""
        cap = max(self.n - 1, 0)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        i, j, r2, length = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.float64)
        out8 = (C.c_double * 8)()
        _check(self.H.murbhost_sim_spanning_tree(self.h, i.ctypes.data_as(ip), j.ctypes.data_as(ip), _ptr(r2), length.ctypes.data_as(dp),
                                                 cap, out8), "murbhost_sim_spanning_tree")
        d = dict(zip(MST_KEYS, out8[:7]))
        for key in ("members", "edges", "components", "rounds"):
            d[key] = int(d[key])
        e = d["edges"]
        d.update({"i": i[:e], "j": j[:e], "r2": r2[:e], "length": length[:e]})
        return d

    def mean_separation(self):
        """SimulationNBodyHIP::meanSeparation: Simulation.mean_separation() of all the plugin's bodies as they are on the device."""
        mean = C.c_double()
        _check(self.H.murbhost_sim_mean_separation(self.h, C.byref(mean)), "murbhost_sim_mean_separation")
        return mean.value

    def force_split(self, h):
        """SimulationNBodyHIP::forceSplit: Simulation.force_split(h) of all the plugin's bodies as they are on the device."""
        counts = np.zeros(self.n, np.uint64)
        planes = [np.zeros((7, self.n), np.float32) for _ in range(3)]
        _check(self.H.murbhost_sim_force_split(self.h, float(np.float32(h)), counts.ctypes.data_as(C.POINTER(C.c_ulong)),
                                               *[_ptr(a) for a in planes]), "murbhost_sim_force_split")
        keys = Simulation._FIELD_KEYS
        irregular, total, regular = ({k: a[i] for i, k in enumerate(keys)} for a in planes)
        return {"counts": counts, "irregular": irregular, "total": total, "regular": regular}

    def encounters(self):
        """integrator 3 / 4: dict of the substep that ended the last iteration by an encounter (Simulation.encounters' keys;
        count 0 when it ran its whole dt); None for the fixed-step plugins."""
        count, time = C.c_ulong(), C.c_double()
        ip = C.POINTER(C.c_int)
        if self.H.murbhost_sim_encounters(self.h, None, None, None, 0, C.byref(count), C.byref(time)) != 0:
            return None
        kept = min(count.value, 4096)
        i, j, r2 = np.zeros(kept, np.int32), np.zeros(kept, np.int32), np.zeros(kept, np.float32)
        if kept:
            self.H.murbhost_sim_encounters(self.h, i.ctypes.data_as(ip), j.ctypes.data_as(ip), _ptr(r2), kept, C.byref(count),
                                           C.byref(time))
        return {"i": i, "j": j, "r2": r2, "count": int(count.value), "time": time.value}

    def contacts(self):
        """integrator 3 / 4 with contact=True: dict of the substep that ended the last iteration by a contact
        (Simulation.contacts' keys; count 0 when it ran its whole dt); None where the feature does not apply."""
        count, time = C.c_ulong(), C.c_double()
        ip = C.POINTER(C.c_int)
        if self.H.murbhost_sim_contacts(self.h, None, None, None, 0, C.byref(count), C.byref(time)) != 0:
            return None
        kept = min(count.value, 4096)
        i, j, gap2 = np.zeros(kept, np.int32), np.zeros(kept, np.int32), np.zeros(kept, np.float32)
        if kept:
            self.H.murbhost_sim_contacts(self.h, i.ctypes.data_as(ip), j.ctypes.data_as(ip), _ptr(gap2), kept, C.byref(count),
                                         C.byref(time))
        return {"i": i, "j": j, "gap2": gap2, "count": int(count.value), "time": time.value}

    def ac_begin(self, h, n_irr):
        """SimulationNBodyHIP::acBegin: Simulation.ac_begin with a common radius on the plugin's bodies (needs a Hermite plugin)."""
        _check(self.H.murbhost_sim_ac_begin(self.h, float(np.float32(h)), int(n_irr)), "murbhost_sim_ac_begin")

    def ac_steps(self, dt, steps):
        """SimulationNBodyHIP::acSteps: Simulation.ac_steps on the plugin's bodies."""
        _check(self.H.murbhost_sim_ac_steps(self.h, dt, int(steps)), "murbhost_sim_ac_steps")

    def block_counts(self):
        """integrator=4: (block steps so far, body-steps, clamped steps); None for the other plugins."""
        out = (C.c_double * 3)()
        return tuple(int(x) for x in out[:]) if self.H.murbhost_sim_block_counts(self.h, out) == 0 else None

    def history(self):
        """dict of the tracked metrics, one entry per computed iteration (tracking sims only)."""
        rows = int(self.H.murbhost_history_rows(self.h))
        if rows < 0:
            raise RuntimeError("not a tracking simulation")
        e, a, c = np.zeros(rows), np.zeros(rows), np.zeros(3 * rows)
        dp = C.POINTER(C.c_double)
        self.H.murbhost_history_get(self.h, e.ctypes.data_as(dp), a.ctypes.data_as(dp), c.ctypes.data_as(dp))
        return {"energy": e, "ang_momentum": a, "density_center": c.reshape(rows, 3)}

    def save_history_csv(self, path):
        if self.H.murbhost_sim_history_csv(self.h, str(path).encode()) != 0:
            raise RuntimeError(f"cannot open {path}")

    def step(self, iterations=1):
        self.H.murbhost_sim_step(self.h, iterations)

    def substeps(self):
        """integrator=3: (substeps taken so far, smallest dt, largest dt); integrator=4: (block steps so far, smallest and
        largest dt of any body); None for the fixed-step plugins."""
        out = (C.c_double * 3)()
        return tuple(out[:]) if self.H.murbhost_sim_substeps(self.h, out) == 0 else None

    def init_on_device(self, seed=0):
        """HIPBodies::initOnDevice: the same initial conditions, generated on the device."""
        self.H.murbhost_sim_init_on_device(self.h, seed)

    def state(self):
        pad = 0
        a = {k: np.zeros(self.n + 64, np.float32) for k in FIELDS}   # room for SIMD padding bodies
        self.H.murbhost_sim_state(self.h, *[_ptr(a[k]) for k in FIELDS])
        return {k: v[:self.n].copy() for k, v in a.items()}

    def acc(self):
        a = [np.zeros(self.n, np.float32) for _ in range(3)]
        self.H.murbhost_sim_acc(self.h, *[_ptr(x) for x in a])
        return tuple(a)

    def flops_per_ite(self):
        return float(self.H.murbhost_sim_flops_per_ite(self.h))

    def allocated_bytes(self):
        return float(self.H.murbhost_sim_allocated_bytes(self.h))

    def close(self):
        if self.h:
            self.H.murbhost_sim_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
