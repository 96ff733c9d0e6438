"""ctypes binding of libscvx_hip.so — the only door from the Python host layer to the HIP path.

There is no CPU fallback: if the shared library is missing or does not export a symbol declared in
include/scvx.h, importing this module's `lib()` raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libscvx_hip.so")
_DEFAULT_LIB_PATH = LIB_PATH

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)


class ScvxProblem(C.Structure):
    """struct scvx_problem (include/scvx.h) — flat image of DescentProblem, master.jl:17-71."""
    _fields_ = [
        ("g", C.c_double), ("mdry", C.c_double), ("mwet", C.c_double), ("Tmin", C.c_double), ("Tmax", C.c_double),
        ("deltaMax", C.c_double), ("thetaMax", C.c_double), ("gammaGs", C.c_double), ("omMax", C.c_double),
        ("dpMax", C.c_double),
        ("jB", C.c_double * 9),
        ("alpha", C.c_double), ("rho", C.c_double), ("sos", C.c_double),
        ("rTB", C.c_double * 3), ("rFB", C.c_double * 3),
        ("rIi", C.c_double * 3), ("rIf", C.c_double * 3), ("vIi", C.c_double * 3), ("vIf", C.c_double * 3),
        ("qBIi", C.c_double * 4), ("qBIf", C.c_double * 4),
        ("wBi", C.c_double * 3), ("wBf", C.c_double * 3),
        ("wNu", C.c_double), ("wID", C.c_double), ("wDS", C.c_double), ("wCst", C.c_double),
        ("wTviol", C.c_double), ("nuTol", C.c_double), ("delTol", C.c_double), ("tf_guess", C.c_double),
        ("ri", C.c_double), ("rh0", C.c_double), ("rh1", C.c_double), ("rh2", C.c_double),
        ("alph", C.c_double), ("bet", C.c_double),
        ("force_scalar", C.c_double), ("length_scalar", C.c_double), ("finmxf", C.c_double),
        ("K", C.c_int32), ("imax", C.c_int32), ("aero_kind", C.c_int32), ("model_flags", C.c_int32),
    ]


class ScvxSolverOpts(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("refine", C.c_int32), ("tol", C.c_double), ("accept_tol", C.c_double),
                ("reuse_inactive_tr", C.c_int32), ("warm_start", C.c_int32), ("retries", C.c_int32), ("reserved0", C.c_int32)]


class ScvxThreedofOpts(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("refine", C.c_int32), ("tol", C.c_double), ("delta", C.c_double),
                ("attitude", C.c_int32), ("reserved", C.c_int32)]


class ScvxMcRng(C.Structure):
    """struct scvx_mc_rng (include/scvx.h): the stream of the draws the _rng forms of the sampled calls make on the device"""
    _fields_ = [("seed", C.c_uint64), ("s_lo", C.c_uint64), ("b_lo", C.c_uint64), ("independent", C.c_int32), ("reserved", C.c_int32)]


class ScvxMcVehicle(C.Structure):
    """struct scvx_mc_vehicle (include/scvx.h): mean and 1 sigma of the six per-flight vehicle errors of the _veh forms"""
    _fields_ = [("mu", C.c_double * 6), ("sp", C.c_double * 6), ("reserved", C.c_int32 * 2)]


# the components of the vehicle errors (the SCVX_VEH_* macros of include/scvx.h)
VEH_N = 6
VEH_COLUMNS = ("THRUST", "MIS_Y", "MIS_Z", "ISP", "AERO", "FIN")
VEH_INDEX = {n: i for i, n in enumerate(VEH_COLUMNS)}
# scvx_vehicle_tiles_*: the rows of vtile [B][K][VTILE_N][14] (the SCVX_VTILE_* macros of include/scvx.h)
VTILE_N = 2
VTILE_COLUMNS = ("ISP", "AERO")

ABI_VERSION = 4   # SCVX_ABI_VERSION of the include/scvx.h these structs and signatures were written against

# scvx_flight_check_*: modes and the columns of the report [B][FLIGHT_NREP] (the SCVX_FLIGHT_* macros of include/scvx.h)
FLIGHT_SHOOT, FLIGHT_PLAN = 0, 1
FLIGHT_NREP = 16
FLIGHT_COLUMNS = ("GAP", "MISS_R", "MISS_V", "MISS_Q", "MISS_W", "MASS_END", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "G_TMAX",
                  "G_TMIN", "G_GIMBAL", "G_DP", "G_FIN", "QNORM")
FLIGHT_INDEX = {n: i for i, n in enumerate(FLIGHT_COLUMNS)}
# scvx_segment_audit_*: the columns of seg [B][K][SEG_N] (the SCVX_SEG_* macros of include/scvx.h)
SEG_N = 11
SEG_COLUMNS = ("DEFECT", "G_MASS", "G_GLIDE", "G_TILT", "G_RATE", "G_TMAX", "G_TMIN", "G_GIMBAL", "G_DP", "G_FIN", "QNORM")
SEG_INDEX = {n: i for i, n in enumerate(SEG_COLUMNS)}
TRACK_CLAMP = 1   # SCVX_TRACK_CLAMP: scvx_track_fly_* rescales the commanded thrust / fin norms into their bounds
# scvx_cov_propagate_*: the columns of the dispersion report [B][COV_NREP] (the SCVX_COV_* macros of include/scvx.h)
COV_NREP = 16
COV_COLUMNS = ("SIG_M", "SIG_R", "SIG_V", "SIG_Q", "SIG_W", "ELL_A", "ELL_B", "ELL_ANG", "SIG_PEAK", "S_THRUST", "N_MASS", "N_GLIDE",
               "N_TILT", "N_RATE", "N_TMAX", "N_TMIN")
COV_INDEX = {n: i for i, n in enumerate(COV_COLUMNS)}
# scvx_cov_clamp_*: the columns of satrep [B][SAT_NREP] (the SCVX_SAT_* macros of include/scvx.h)
SAT_NREP = 16
SAT_COLUMNS = ("SIG_M", "SIG_R", "SIG_V", "SIG_Q", "SIG_W", "BIAS_M", "BIAS_R", "BIAS_V", "BIAS_Q", "BIAS_W", "RMS_R", "RMS_V", "P_LO", "P_HI",
               "GAIN_MIN", "BIAS_PEAK")
SAT_INDEX = {n: i for i, n in enumerate(SAT_COLUMNS)}
# scvx_cov_path_sigma_*: the columns of psig [B][K+1][PSIG_N] (the SCVX_PSIG_* macros of include/scvx.h)
PSIG_N = 5
PSIG_COLUMNS = ("MASS", "GLIDE", "TILT", "RATE", "THRUST")
PSIG_INDEX = {n: i for i, n in enumerate(PSIG_COLUMNS)}
# scvx_batch_set_path_margins: the columns of pm [B][K+1][PMARG_N] (SCVX_PMARG_*), and the mask of scvx_batch_margins_from_cov (SCVX_MARGIN_*)
PMARG_N = 4
PMARG_COLUMNS = ("MASS", "GLIDE", "TILT", "RATE")
PMARG_INDEX = {n: i for i, n in enumerate(PMARG_COLUMNS)}
MARGIN_BITS = {"thrust": 1, "mass": 2, "glide": 4, "tilt": 8, "rate": 16}
# scvx_nav_cov_*: the columns of the navigation report [B][NAV_NREP] (the SCVX_NAV_* macros of include/scvx.h)
NAV_NREP = 8
NAV_COLUMNS = ("NAV_M", "NAV_R", "NAV_V", "NAV_Q", "NAV_W", "NAV_PEAK", "EST_R", "EST_V")
NAV_INDEX = {n: i for i, n in enumerate(NAV_COLUMNS)}

# scvx_track_mc_*: the columns of the sampled-dispersion report [B][MC_NREP] (the SCVX_MC_* macros of include/scvx.h)
MC_NREP = 48
MC_COLUMNS = (tuple("MAX_" + n for n in FLIGHT_COLUMNS) + tuple("MEAN_" + n for n in FLIGHT_COLUMNS)
              + tuple("P_" + n[2:] for n in FLIGHT_COLUMNS[6:15]) + ("P_ANY", "OUT_LO", "OUT_HI", "N_BAD", "S"))
MC_INDEX = {n: i for i, n in enumerate(MC_COLUMNS)}
# scvx_track_mc_nav_*: the columns of the sampled navigation report [B][NAV_NREP]: navrep's, with MAX_FED where navrep has NAV_PEAK
MCNAV_COLUMNS = ("NAV_M", "NAV_R", "NAV_V", "NAV_Q", "NAV_W", "MAX_FED", "EST_R", "EST_V")
MCNAV_INDEX = {n: i for i, n in enumerate(MCNAV_COLUMNS)}

_vp = C.c_void_p
_rp = C.POINTER(ScvxMcRng)
_hp = C.POINTER(ScvxMcVehicle)
# name -> (restype, argtypes); must list every symbol include/scvx.h declares (tests check this)
SIGNATURES = {
    "scvx_abi_version": (C.c_int, []),
    "scvx_abi_struct_sizes": (C.c_int, [_ip]),
    "scvx_ctx_create": (C.c_int, [C.POINTER(ScvxProblem), C.c_int, C.POINTER(_vp)]),
    "scvx_ctx_destroy": (None, [_vp]),
    "scvx_last_error": (C.c_char_p, [_vp]),
    "scvx_control_dim": (C.c_int, [_vp]),
    "scvx_set_stream": (C.c_int, [_vp, _vp]),
    "scvx_use_null_stream": (C.c_int, [_vp]),
    "scvx_get_stream": (C.c_int, [_vp, C.POINTER(_vp)]),
    "scvx_synchronize": (C.c_int, [_vp]),
    "scvx_set_nsub": (C.c_int, [_vp, C.c_int]),
    "scvx_get_nsub": (C.c_int, [_vp]),
    "scvx_set_aero_table": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
    "scvx_linearize_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_double, _vp, _vp]),
    "scvx_linearize_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, _dp, _dp]),
    "scvx_propagate_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_double, _vp]),
    "scvx_propagate_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_double, _dp]),
    "scvx_flight_check_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "scvx_flight_check_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, _dp, _dp]),
    "scvx_track_gains_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _dp, _dp, _dp, _vp, _vp]),
    "scvx_track_gains_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_track_fly_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "scvx_track_fly_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _dp]),
    "scvx_cov_propagate_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _dp, _vp, _vp, _vp, _vp]),
    "scvx_cov_propagate_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_cov_path_sigma_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _dp, _vp, _vp]),
    "scvx_cov_path_sigma_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_nav_cov_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _dp, _dp, _dp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "scvx_nav_cov_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                        _dp]),
    "scvx_track_fly_nav_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "scvx_track_fly_nav_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _dp]),
    "scvx_track_mc_f64": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dp, _vp, C.c_int, C.c_int, C.c_double,
                                    _vp, _vp, _vp, _vp, _vp, _vp]),
    "scvx_track_mc_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _vp, C.c_int, C.c_int,
                                         C.c_double, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_track_mc_nav_f64": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dp, _vp, _vp, _vp, _vp, _vp,
                                        C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp]),
    "scvx_track_mc_nav_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                             _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                             _dp, _dp, _dp]),
    # exact batched order statistics, and the sampled calls with them and the per-node samples: the old lists, then nq, ranks (host),
    # flightq, pathq, pathv
    "scvx_order_stats_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_size_t, C.c_size_t, C.c_int, _ip, _vp]),
    "scvx_order_stats_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_size_t, C.c_size_t, C.c_int, _ip, _dp]),
    "scvx_track_mc_q_f64": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dp, _vp, C.c_int, C.c_int,
                                      C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _ip, _vp, _vp, _vp]),
    "scvx_track_mc_q_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _vp, C.c_int, C.c_int,
                                           C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp]),
    "scvx_track_mc_nav_q_f64": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dp, _vp, _vp, _vp, _vp, _vp,
                                          C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp, C.c_int, _ip, _vp, _vp, _vp]),
    "scvx_track_mc_nav_q_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                               _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                               _dp, _dp, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp]),
    "scvx_batch_track_mc_q": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _vp, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp,
                                        _dp, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp]),
    "scvx_batch_track_mc_nav_q": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp,
                                            C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int,
                                            _ip, _dp, _dp, _dp]),
    # the sampled calls with the draws made on the device: the _q lists with (xi0, eta) replaced by (rng, noise), (xin, nud) dropped
    "scvx_mc_draws_f64": (C.c_int, [_vp, _rp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "scvx_mc_draws_f64_host": (C.c_int, [_vp, _rp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "scvx_track_mc_rng_f64": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _rp, C.c_int, _dp, _vp, C.c_int, C.c_int,
                                        C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _ip, _vp, _vp, _vp]),
    "scvx_track_mc_rng_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _rp, C.c_int, _dp, _vp, C.c_int,
                                             C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp]),
    "scvx_track_mc_nav_rng_f64": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _rp, C.c_int, _dp, _vp, _vp, _vp,
                                            C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _vp, C.c_int, _ip, _vp, _vp, _vp]),
    "scvx_track_mc_nav_rng_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _rp, C.c_int, _dp, _dp, _dp, _dp,
                                                 C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                                 _dp, _dp, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp]),
    "scvx_batch_track_mc_rng": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, _dp, _rp, C.c_int, _dp, _vp, C.c_int, C.c_int, C.c_double, _dp, _dp,
                                          _dp, _dp, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp]),
    "scvx_batch_track_mc_nav_rng": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, _dp, _rp, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _dp, C.c_int,
                                              C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, _ip,
                                              _dp, _dp, _dp]),
    # the sampled calls with per-flight vehicle errors: the _q lists, then rng, noise, veh, zeta, theta
    "scvx_track_mc_veh_f64": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dp, _vp, C.c_int, C.c_int,
                                        C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _ip, _vp, _vp, _vp, _rp, C.c_int, _hp, _vp,
                                        _vp]),
    "scvx_track_mc_veh_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _vp, C.c_int,
                                             C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp, _rp,
                                             C.c_int, _hp, _dp, _dp]),
    "scvx_track_mc_nav_veh_f64": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _dp, _vp, _vp, _vp, _vp,
                                            _vp, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _vp, _vp, _vp, C.c_int, _ip, _vp, _vp, _vp, _rp, C.c_int, _hp, _vp, _vp]),
    "scvx_track_mc_nav_veh_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                                 _dp, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp,
                                                 _dp, _dp, _dp, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp, _rp, C.c_int, _hp, _dp, _dp]),
    "scvx_batch_track_mc_veh": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _vp, C.c_int, C.c_int, C.c_double, _dp, _dp,
                                          _dp, _dp, _dp, _dp, C.c_int, _ip, _dp, _dp, _dp, _rp, C.c_int, _hp, _dp, _dp]),
    "scvx_batch_track_mc_nav_veh": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp,
                                              C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                              C.c_int, _ip, _dp, _dp, _dp, _rp, C.c_int, _hp, _dp, _dp]),
    "scvx_vehicle_tiles_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "scvx_vehicle_tiles_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "scvx_cov_vehicle_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _dp, _vp, _vp, _vp, _vp, _vp, _vp, _dp, _vp]),
    "scvx_cov_vehicle_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_nav_cov_vehicle_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _dp, _dp, _dp, _vp, _vp, _vp, _vp,
                                           _vp, _vp, _vp, _vp, _dp, _vp]),
    "scvx_nav_cov_vehicle_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp,
                                                _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    # the clamp-aware covariance analysis: the plain lists with band2 (host) behind w14 and satrep, mean behind report, satk last
    "scvx_cov_clamp_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _dp, _dp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "scvx_cov_clamp_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_batch_cov_clamp": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_batch_cov_veh": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_batch_nav_cov_veh": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_batch_margins_from_cov_veh": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_uint, _dp, _dp]),
    "scvx_batch_margins_from_nav_veh": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, C.c_uint,
                                                  _dp, _dp]),
    # the segment audit and the back-offs taken from it
    "scvx_segment_audit_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp]),
    "scvx_segment_audit_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _dp]),
    "scvx_batch_segment_audit": (C.c_int, [_vp, C.c_int, _dp, _dp]),
    "scvx_batch_audit_margins": (C.c_int, [_vp, C.c_int, C.c_uint, C.c_double, C.c_double, C.c_double, _dp]),
    "scvx_linearize_f32": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_float, _vp, _vp]),
    "scvx_linearize_f32_host": (C.c_int, [_vp, C.c_int, C.c_int, _fp, _fp, _fp, C.c_float, _fp, _fp]),
    "scvx_propagate_f32": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_float, _vp]),
    "scvx_propagate_f32_host": (C.c_int, [_vp, C.c_int, C.c_int, _fp, _fp, _fp, C.c_float, _fp]),
    "scvx_solver_default_opts": (C.c_int, [C.POINTER(ScvxSolverOpts)]),
    "scvx_batch_create": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "scvx_batch_destroy": (None, [_vp]),
    "scvx_batch_set_solver": (C.c_int, [_vp, C.POINTER(ScvxSolverOpts)]),
    "scvx_batch_init": (C.c_int, [_vp, _dp]),
    "scvx_batch_reset": (C.c_int, [_vp]),
    "scvx_batch_init_threedof": (C.c_int, [_vp, _dp, C.POINTER(ScvxThreedofOpts), _ip]),
    "scvx_threedof_default_opts": (C.c_int, [C.POINTER(ScvxThreedofOpts)]),
    "scvx_threedof_record_doubles": (C.c_int32, [C.c_int]),
    "scvx_threedof_solve": (C.c_int, [_vp, C.c_int, _dp, C.POINTER(ScvxThreedofOpts), _dp, _ip, _dp]),
    "scvx_threedof_solve_dev": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(ScvxThreedofOpts), _vp, _vp]),
    "scvx_solve_step": (C.c_int, [_vp, _ip, _dp, _dp]),
    "scvx_solve_step_async": (C.c_int, [_vp]),
    "scvx_solve": (C.c_int, [_vp, _ip, _ip, _dp, _dp]),
    "scvx_batch_get_trajectory": (C.c_int, [_vp, _dp]),
    "scvx_batch_set_trajectory": (C.c_int, [_vp, _dp]),
    "scvx_batch_trajectory_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_int64)]),
    "scvx_batch_get_linearization": (C.c_int, [_vp, _dp, _dp]),
    "scvx_batch_set_linearization_f32": (C.c_int, [_vp, C.c_int]),
    "scvx_batch_get_scalars": (C.c_int, [_vp, _dp, _dp, _ip]),
    "scvx_batch_set_scalars": (C.c_int, [_vp, _dp, _dp, _ip]),
    "scvx_batch_get_flags": (C.c_int, [_vp, _ip, _ip, _ip]),
    "scvx_batch_set_flags": (C.c_int, [_vp, _ip, _ip, _ip]),
    "scvx_batch_get_solver_stats": (C.c_int, [_vp, _ip, _ip, _dp, _dp]),
    "scvx_batch_flight_check": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp]),
    "scvx_batch_track_gains": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_batch_track_fly": (C.c_int, [_vp, _dp, _dp, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _dp]),
    "scvx_batch_cov": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_batch_nav_cov": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_batch_track_fly_nav": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _dp]),
    "scvx_batch_track_mc": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _vp, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp,
                                      _dp, _dp]),
    "scvx_batch_track_mc_nav": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, C.c_int,
                                          C.c_int, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_batch_set_thrust_margins": (C.c_int, [_vp, _dp, _dp]),
    "scvx_batch_get_thrust_margins": (C.c_int, [_vp, _dp, _dp]),
    "scvx_batch_thrust_margins_from_cov": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_double, _dp]),
    "scvx_batch_replan": (C.c_int, [_vp]),
    "scvx_batch_set_path_margins": (C.c_int, [_vp, _dp]),
    "scvx_batch_get_path_margins": (C.c_int, [_vp, _dp]),
    "scvx_batch_margins_from_cov": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_double, C.c_uint, _dp]),
    "scvx_batch_margins_from_nav": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, C.c_uint, _dp]),
    "scvx_nav_path_sigma_f64": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _dp, _dp, _dp, _vp, _vp, _vp]),
    "scvx_nav_path_sigma_f64_host": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]),
    "scvx_comm_probe": (C.c_int, []),
    "scvx_comm_unique_id": (C.c_int, [_vp]),
    "scvx_comm_create": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "scvx_comm_destroy": (C.c_int, [_vp]),
    "scvx_comm_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "scvx_allgather_trajectories": (C.c_int, [_vp, _vp]),
    "scvx_allgather_status": (C.c_int, [_vp, _vp, _vp]),
    "scvx_allgather_f64": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "scvx_allgather_i32": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "scvx_socp_solve": (C.c_int, [_vp, _dp, _dp]),
    "scvx_batch_get_step_stats": (C.c_int, [_vp, _dp, C.c_int]),
    "scvx_batch_set_profiling": (C.c_int, [_vp, C.c_int]),
    "scvx_batch_get_profile": (C.c_int, [_vp, _dp, C.POINTER(C.c_int64)]),
}

_LIB = None


def _preload_torch_hip_runtime():
    """One process, one HIP / HSA runtime.  PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 under the
    same sonames as /opt/rocm's; whichever copy is loaded first serves both torch and libscvx_hip.so.  If this library came
    first (the system copy), a later `import torch` finds "No HIP GPUs": its extensions were built against the bundled
    copy.  So when torch is installed its copies are loaded here, before libscvx_hip.so, without importing torch."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return


class ScvxError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load libscvx_hip.so and bind every ABI symbol; raises if the HIP extension is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH) and LIB_PATH == _DEFAULT_LIB_PATH:
        # a source checkout without the built artefact: build the HIP extension (hipcc, gfx950) — never a CPU path
        try:
            from . import build as _build
            _build.build()
        except Exception as e:  # noqa: BLE001
            raise ScvxError(f"{LIB_PATH} is missing and building it with hipcc failed: {e}") from e
    if not os.path.exists(LIB_PATH):
        raise ScvxError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -m successiveconvexification_amd.build` or __graft_entry__.build().")
    _preload_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if the library lacks an ABI symbol
        fn.restype = res
        fn.argtypes = args
    # the ABI guard of include/scvx.h: a library built from another revision of the header is refused before the first call
    sizes = (C.c_int32 * 3)()
    L.scvx_abi_struct_sizes(sizes)
    mine = (C.sizeof(ScvxProblem), C.sizeof(ScvxSolverOpts), C.sizeof(ScvxThreedofOpts))
    if L.scvx_abi_version() != ABI_VERSION or tuple(sizes) != mine:
        raise ScvxError(f"{LIB_PATH}: ABI version {L.scvx_abi_version()} / struct sizes {tuple(sizes)}, this binding expects "
                        f"{ABI_VERSION} / {mine}: rebuild the library from this tree's include/scvx.h")
    _LIB = L
    return L


def check(ctx_handle, rc: int, what: str):
    if rc != 0:
        msg = lib().scvx_last_error(ctx_handle)
        raise ScvxError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
