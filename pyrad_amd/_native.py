"""ctypes binding of ``libpyrad_hip.so`` (the C ABI in ``include/pyrad_hip.h``).

No PyTorch, no Triton: the Python host talks to the HIP kernels through plain
pointers and sizes.  If the shared library is missing or cannot be loaded this module
raises — there is deliberately no CPU fallback in the product path.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PYRAD_HIP_LIB") or os.path.join(_HERE, "lib", "libpyrad_hip.so")
CSRC = os.path.join(_HERE, "csrc")

LBL_OK = 0
ERR_NAMES = {0: "LBL_OK", -1: "LBL_ERR_BAD_ARG", -2: "LBL_ERR_NO_DEVICE", -3: "LBL_ERR_HIP",
             -4: "LBL_ERR_RCCL", -5: "LBL_ERR_OOM", -6: "LBL_ERR_STATE"}
UNIQUE_ID_BYTES = 128


class LblError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s (%d): %s" % (ERR_NAMES.get(code, "LBL_ERR_?"), code, message))
        self.code = code


class NoDeviceError(LblError):
    pass


class IsoParams(C.Structure):
    """lbl_iso_params"""
    _fields_ = [("T", C.c_double), ("P", C.c_double), ("q_frac", C.c_double),
                ("molmass", C.c_double), ("Q_T", C.c_double), ("Q_296", C.c_double)]


class Grid(C.Structure):
    """lbl_grid"""
    _fields_ = [("range_min", C.c_double), ("range_max", C.c_double), ("resolution", C.c_double),
                ("base_resolution", C.c_double), ("n_work", C.c_int64), ("n_base", C.c_int64),
                ("window", C.c_int64), ("shard_first", C.c_int64), ("shard_count", C.c_int64)]


_P = C.c_void_p
_D = C.POINTER(C.c_double)

# name -> (restype, argtypes): every symbol include/pyrad_hip.h declares
SIGNATURES = {
    "lbl_abi_version": (C.c_int, []),
    "lbl_limit": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64)]),
    "lbl_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "lbl_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "lbl_ctx_destroy": (C.c_int, [_P]),
    "lbl_last_error": (C.c_char_p, [_P]),
    "lbl_sync": (C.c_int, [_P]),
    "lbl_ctx_stream": (C.c_int, [_P, C.POINTER(_P)]),
    "lbl_ctx_chain_accumulate": (C.c_int, [_P, _P]),
    "lbl_lines_view": (C.c_int, [_P, C.c_int64, C.c_int64, C.POINTER(_P)]),
    "lbl_device_info": (C.c_int, [_P, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "lbl_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "lbl_profile_enable": (C.c_int, [_P, C.c_int]),
    "lbl_profile_read": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), _D]),
    "lbl_profile_reset": (C.c_int, [_P]),
    "lbl_profile_reserve": (C.c_int, [_P, C.c_int]),
    "lbl_buffer_create": (C.c_int, [_P, C.c_int64, C.POINTER(_P)]),
    "lbl_buffer_destroy": (C.c_int, [_P]),
    "lbl_buffer_size": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "lbl_buffer_upload": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "lbl_buffer_download": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "lbl_buffer_fill": (C.c_int, [_P, C.c_double]),
    "lbl_buffer_download_async": (C.c_int, [_P, _P, C.c_int64, C.c_int64]),
    "lbl_download_wait": (C.c_int, [_P]),
    "lbl_buffer_devptr": (C.c_int, [_P, C.POINTER(_P)]),
    "lbl_host_alloc": (C.c_int, [_P, C.c_int64, C.POINTER(_P)]),
    "lbl_host_free": (C.c_int, [_P, _P]),
    "lbl_lines_create": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(_P)]),
    "lbl_lines_destroy": (C.c_int, [_P]),
    "lbl_lines_count": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "lbl_xsec_accumulate": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, C.c_int64, C.POINTER(IsoParams),
                                      C.POINTER(Grid), _P, C.POINTER(C.c_int64)]),
    "lbl_xsec_accumulate_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(IsoParams), C.POINTER(Grid),
                                          C.POINTER(_P)]),
    "lbl_xsec_voigt_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(IsoParams), C.POINTER(Grid), C.POINTER(_P)]),
    "lbl_voigt_function_dev": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "lbl_xsec_voigt_dt_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(IsoParams), _D, C.POINTER(Grid), C.POINTER(_P)]),
    "lbl_voigt_gradient_dev": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P]),
    "lbl_schedule_export": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int32)]),
    "lbl_last_regime_counts": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64)]),
    "lbl_line_quantities": (C.c_int, [_P, _P, C.POINTER(IsoParams), C.POINTER(Grid), _P, _P, _P, _P, _P]),
    "lbl_layer_sweep_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_int32), C.c_int, _D,
                                      C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int64,
                                      C.c_int64, C.c_int64, _P, C.c_double, _P, _P, _P]),
    "lbl_layer_step_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(IsoParams), C.POINTER(Grid), C.POINTER(_P),
                                     C.POINTER(C.c_int32), C.c_int, _D, C.c_double, _P, C.c_double, _P, _P, _P]),
    "lbl_layer_merged_step_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(IsoParams), C.POINTER(Grid),
                                            C.POINTER(C.c_int32), C.c_int, _D, C.c_double, _P, C.c_double, _P, _P, _P]),
    "lbl_layers_merged_accumulate_dev": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.POINTER(_P), C.POINTER(IsoParams),
                                                   C.POINTER(Grid), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _D,
                                                   C.POINTER(_P)]),
    "lbl_column_fold_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, _D, C.c_double, C.c_double, C.c_int64, C.c_int64,
                                      C.c_int64, _P, C.c_double, C.POINTER(_P), _P]),
    "lbl_column_flux_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, _D, C.c_double, C.c_double, C.c_int64, _P, C.c_double,
                                      _P, C.c_int, _D, _D, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P, _P, _P]),
    "lbl_column_jacobian_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, _D, C.c_double, C.c_double, C.c_int64, _P,
                                          C.c_double, C.c_int, _D, _D, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.c_int, C.POINTER(_P), C.POINTER(C.c_int32), _P, _P, _P]),
    "lbl_ray_radiance_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_double, C.c_double, C.c_int64, C.c_int,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), _D, C.POINTER(C.c_int32), _P, C.c_double,
                                       _P, _P]),
    "lbl_column_flux_surface_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, _D, C.c_double, C.c_double, C.c_int64, _P,
                                              C.c_double, _P, C.c_int, _D, _D, C.c_int, C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64), _P, C.c_double, C.c_int, _P, _P, _P, _P]),
    "lbl_ray_radiance_surface_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_double, C.c_double, C.c_int64, C.c_int,
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int32), _D, C.POINTER(C.c_int32), _P,
                                               C.c_double, _P, C.c_double, _P, C.c_double, _P, _P]),
    "lbl_column_flux_linear_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, _D, C.c_double, C.c_double, C.c_int64, _P,
                                             C.c_double, _P, C.c_int, _D, _D, C.c_int, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64), _P, C.c_double, C.c_int, _P, _P, _P, _P]),
    "lbl_ray_radiance_linear_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_double, C.c_double, C.c_int64, C.c_int,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), _D, C.POINTER(C.c_int32), _P,
                                              C.c_double, _P, C.c_double, _P, C.c_double, _P, _P]),
    "lbl_column_solar_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_double, C.c_double, C.c_int64, _P, C.c_int, _D, _D,
                                       C.c_int, _D, _D, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P, C.c_double,
                                       C.c_int, _P, _P, _P, _P]),
    "lbl_column_twostream_workspace": (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_int64)]),
    "lbl_column_twostream_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_double, C.c_double, C.c_int64, _P, C.c_int, _D,
                                           _D, C.c_int, _D, C.POINTER(_P), _D, C.POINTER(_P), _D, C.POINTER(_P), _D, C.c_int,
                                           C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P, C.c_double, _P, _P, _P, _P,
                                           _P, _P]),
    "lbl_column_flux_scatter_workspace": (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_int64)]),
    "lbl_column_flux_scatter_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_int, _D, C.c_double, C.c_double, C.c_int64, _P,
                                              C.c_double, _P, C.c_int, _D, C.POINTER(_P), _D, C.POINTER(_P), _D, C.POINTER(_P),
                                              _D, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P, C.c_double,
                                              _P, _P, _P, _P, _P]),
    "lbl_column_jacobian_scatter_workspace": (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_int64)]),
    "lbl_column_jacobian_scatter_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_int, _D, C.c_double, C.c_double,
                                                  C.c_int64, _P, C.c_double, _P, C.c_int, _D, C.POINTER(_P), _D,
                                                  C.POINTER(_P), _D, C.POINTER(_P), _D, C.c_int, C.c_int,
                                                  C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P, C.c_double, C.c_int,
                                                  C.POINTER(_P), C.POINTER(C.c_int32), _P, _P, _P, _P, _P]),
    "lbl_column_radiance_scatter_workspace": (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_int64)]),
    "lbl_column_radiance_scatter_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_int, _D, C.c_double, C.c_double,
                                                  C.c_int64, _P, C.c_double, _P, C.c_int, _D, C.POINTER(_P), _D,
                                                  C.POINTER(_P), _D, C.POINTER(_P), _D, C.c_int, _P, C.c_double, C.c_int, _D,
                                                  C.POINTER(C.c_int32), _P, _P, _P, _P]),
    "lbl_column_beam_radiance_workspace": (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_int64)]),
    "lbl_column_beam_radiance_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_double, C.c_double, C.c_int64, _P,
                                               C.c_double, _D, C.c_int, _D, C.POINTER(_P), _D, C.POINTER(_P), _D,
                                               C.POINTER(_P), _D, C.c_int, _P, C.c_double, C.c_int, _D,
                                               C.POINTER(C.c_int32), _P, _P, _P, _P, _P]),
    "lbl_ray_jacobian_rows": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lbl_ray_jacobian_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_double, C.c_double, C.c_int64, C.c_int,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), _D, C.POINTER(C.c_int32), _P, C.c_double,
                                       C.c_int, C.POINTER(_P), C.POINTER(C.c_int32), _P, _P]),
    "lbl_column_jacobian_surface_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, _D, C.c_double, C.c_double, C.c_int64, _P,
                                                  C.c_double, _P, C.c_int, _D, _D, C.c_int, C.POINTER(C.c_int64),
                                                  C.POINTER(C.c_int64), _P, C.c_double, C.c_int, C.c_int, C.POINTER(_P),
                                                  C.POINTER(C.c_int32), _P, _P, _P, _P]),
    "lbl_ray_jacobian_surface_rows": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lbl_ray_jacobian_surface_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_double, C.c_double, C.c_int64, C.c_int,
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int32), _D, C.POINTER(C.c_int32), _P,
                                               C.c_double, _P, C.c_double, C.c_int, C.POINTER(_P), C.POINTER(C.c_int32), _P,
                                               _P]),
    "lbl_column_jacobian_linear_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, _D, C.c_double, C.c_double, C.c_int64, _P,
                                                 C.c_double, _P, C.c_int, _D, _D, C.c_int, C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_int64), _P, C.c_double, C.c_int, C.c_int, C.POINTER(_P),
                                                 C.POINTER(C.c_int32), _P, _P, _P, _P]),
    "lbl_ray_jacobian_linear_rows": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lbl_ray_jacobian_linear_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_double, C.c_double, C.c_int64, C.c_int,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), _D, C.POINTER(C.c_int32), _P,
                                              C.c_double, _P, C.c_double, C.c_int, C.POINTER(_P), C.POINTER(C.c_int32), _P,
                                              _P]),
    "lbl_ils_convolve_dev": (C.c_int, [_P, C.c_double, C.c_double, C.c_int64, C.c_int, C.POINTER(_P), C.POINTER(C.c_int64),
                                       C.c_int64, _D, _D, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int, C.c_int,
                                       C.c_double, _D, _P]),
    "lbl_rank_order_workspace": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lbl_rank_order_dev": (C.c_int, [_P, C.c_int64, C.c_int, C.POINTER(_P), C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), _P, _P, _P]),
    "lbl_ranked_means_workspace": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lbl_ranked_means_dev": (C.c_int, [_P, C.c_int64, C.c_int, C.POINTER(_P), C.POINTER(C.c_int64), C.POINTER(_P),
                                       C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int64), _P, _P, C.c_int64, _P, C.c_int64]),
    "lbl_column_create": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.POINTER(_P), C.POINTER(IsoParams), C.POINTER(Grid),
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32), _D, _D, C.POINTER(_P), C.POINTER(_P)]),
    "lbl_column_destroy": (C.c_int, [_P]),
    "lbl_column_set_layer": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(IsoParams), C.POINTER(Grid), _D, C.c_double, _P]),
    "lbl_column_transmission": (C.c_int, [_P, C.POINTER(C.c_uint8), _P, C.c_double, _P, _P, C.c_int]),
    "lbl_column_sweep_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), _D, C.c_double, C.c_double, C.c_int64,
                                       C.c_int64, C.c_int64, _P, C.c_double, _P]),
    "lbl_column_step_dev": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.POINTER(_P), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), _D, _D, _D, _D, C.c_double, C.c_double, C.c_int64, C.c_int64,
                                      C.c_int64, _P, C.c_double, C.POINTER(_P), C.POINTER(_P), _P]),
    "lbl_optical_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P]),
    "lbl_sum_dev": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.c_int64, _P]),
    "lbl_planck_dev": (C.c_int, [_P, C.c_double, C.c_double, C.c_int64, C.c_double, _P]),
    "lbl_band_integral": (C.c_int, [_P, _P, C.c_int64, C.c_double, C.c_double, _D]),
    "lbl_line_survey_dev": (C.c_int, [_P, _P, C.POINTER(Grid), _P]),
    "lbl_comm_unique_id": (C.c_int, [C.c_char_p]),
    "lbl_comm_create": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int, C.POINTER(_P)]),
    "lbl_comm_destroy": (C.c_int, [_P]),
    "lbl_allgather_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P]),
    "lbl_allgather_overlap_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P, C.c_int]),
    "lbl_comm_fence_dev": (C.c_int, [_P, C.c_int]),
    "lbl_gather_stage_dev": (C.c_int, [_P, C.c_int64, _P, C.c_int64, C.c_int64]),
    "lbl_capture_begin": (C.c_int, [_P]),
    "lbl_capture_end": (C.c_int, [_P, C.POINTER(_P)]),
    "lbl_graph_launch": (C.c_int, [_P]),
    "lbl_graph_destroy": (C.c_int, [_P]),
    "lbl_gather_compact_dev": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
}

_lib = None


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 with hipcc (``make`` in pyrad_amd/csrc)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", CSRC, "-j4"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def source_hash() -> str:
    """sha256 over what decides the kernels and their launch shapes (csrc/lbl_kernels.hip, lbl_api.hip,
    lbl_device.h, lbl_column_transport.hip, Makefile): profiles/pmc_traffic.json records it so that bench.py can tell
    when committed PMC numbers were measured on other kernels than the ones it is timing."""
    import hashlib
    h = hashlib.sha256()
    for f in ("Makefile", "lbl_api.hip", "lbl_device.h", "lbl_kernels.hip", "lbl_launch_shapes.h", "lbl_column_transport.hip"):
        h.update(f.encode())
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def load():
    """Load the shared library (once) and declare every signature."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C pyrad_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


# line shapes of lbl_ils_convolve_dev, and the rows one of its workgroups carries (kIlsRowBlock of csrc/lbl_device.h)
ILS_SHAPES = {"gaussian": 0, "triangle": 1, "boxcar": 2, "sinc": 3, "table": 4}
ILS_ROW_BLOCK = 8
# points one workgroup of the k-distribution kernels sorts or merges in LDS (kKdistTile of csrc/lbl_device.h): bands up to this
# long are ranked in one launch without work space
KDIST_TILE = 2048

_limits = {}


def limit(name: str) -> int:
    """A fixed size of the library (lbl_limit): "merged_lists_per_job", "arrays_per_layer", "arrays_per_sum",
    "arrays_per_column", "layers_per_column", "jobs_per_batch", "flux_angles", "flux_bands", "jacobian_terms", "ils_rows",
    "ils_channels", "ils_table", "kdist_rows", "kdist_intervals", "ray_paths", "ray_segments"."""
    if name not in _limits:
        v = C.c_int64()
        rc = load().lbl_limit(name.encode(), C.byref(v))
        if rc != LBL_OK:
            raise LblError(rc, "unknown limit %r" % name)
        _limits[name] = int(v.value)
    return _limits[name]


def ray_jacobian_rows(n_layers, ray_first, seg_layer, term_layer=(), surface=False, linear=False):
    """The rows of lbl_ray_jacobian_dev's ``jac`` (lbl_ray_jacobian_rows; no context needed): (row_first, rows) with
    row_first the n_rays + 1 first rows of the rays and rows the total.  Ray r owns [dI/dT_source, c x dI/d ln tau, c x
    dI/dT, its terms] for the c distinct layers it crosses in ascending order and the terms that lie in one of them.
    ``surface``: the rows of lbl_ray_jacobian_surface_dev (lbl_ray_jacobian_surface_rows) - a segment layer of -1 is a
    surface marker without rows, and dI/de follows dI/dT_source.  ``linear``: the rows of lbl_ray_jacobian_linear_dev
    (lbl_ray_jacobian_linear_rows) - markers allowed, and ray r owns [dI/dT_source, dI/de, c x dI/d ln tau, (dI/dTa, dI/dTb)
    per segment that is no marker in order of travel, its terms]."""
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a.size else None
    ray_first, seg_layer, term_layer = i32(ray_first), i32(seg_layer), i32(term_layer)
    lib = load()
    first = np.zeros(max(len(ray_first), 1), dtype=np.int64)
    rows = C.c_int64()
    fn = lib.lbl_ray_jacobian_linear_rows if linear else lib.lbl_ray_jacobian_surface_rows if surface else lib.lbl_ray_jacobian_rows
    rc = fn(int(n_layers), len(ray_first) - 1, i32p(ray_first), i32p(seg_layer), len(term_layer),
        i32p(term_layer), first.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(rows))
    if rc != LBL_OK:
        raise LblError(rc, (lib.lbl_last_error(None) or b"").decode())
    return first, int(rows.value)


def _as_f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a


def _as_i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _hb(b):
    return None if b is None else b.h


def _arr(typ, vals):
    """ctypes array of ``vals`` (one element at least: an empty list still gives the C side a pointer)."""
    return (typ * max(len(vals), 1))(*vals)


class Context:
    """One HIP device + one stream (lbl_ctx).  Not thread-safe."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = _P()
        rc = self.lib.lbl_ctx_create(int(device), C.byref(h))
        if rc != LBL_OK:
            msg = (self.lib.lbl_last_error(None) or b"").decode()
            raise (NoDeviceError if rc == -2 else LblError)(rc, msg)
        self.h = h
        self.device = int(device)
        self._children = []

    # -- plumbing ------------------------------------------------------------------------
    def check(self, rc):
        if rc != LBL_OK:
            raise LblError(rc, (self.lib.lbl_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            # views before the line lists they window (lbl_lines_destroy refuses a list with live views), then
            # everything else newest first
            for child in reversed(list(self._children)):
                if isinstance(child, Lines) and child._parent is not None:
                    child.free()
            for child in reversed(list(self._children)):
                child.free()
            for blocks in self.__dict__.pop("_pinned_pool", {}).values():      # idle blocks; a block a caller still
                for ptr in blocks:                                              # holds an array in is freed with that array
                    self.lib.lbl_host_free(self.h, ptr)
            self.check(self.lib.lbl_ctx_destroy(self.h))
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self.check(self.lib.lbl_sync(self.h))

    def download_wait(self):
        self.check(self.lib.lbl_download_wait(self.h))

    def stream(self) -> int:
        s = _P()
        self.check(self.lib.lbl_ctx_stream(self.h, C.byref(s)))
        return s.value or 0

    def device_info(self):
        name = C.create_string_buffer(256)
        ncu = C.c_int()
        hbm = C.c_int64()
        self.check(self.lib.lbl_device_info(self.h, name, 256, C.byref(ncu), C.byref(hbm)))
        return dict(name=name.value.decode(), n_cu=ncu.value, hbm_bytes=hbm.value)

    def chain_accumulate(self, predecessor):
        """This context's accumulate kernels start after those ``predecessor`` has enqueued (lbl_ctx_chain_accumulate);
        None ends the chaining."""
        self.check(self.lib.lbl_ctx_chain_accumulate(self.h, predecessor.h if predecessor is not None else None))

    def set_option(self, key: str, value: int):
        self.check(self.lib.lbl_set_option(self.h, key.encode(), int(value)))
        self.__dict__.setdefault("options", {})[key] = int(value)      # what was set through this object (hosts choose routes by it)

    def option(self, key: str, default: int = 0) -> int:
        return self.__dict__.get("options", {}).get(key, default)

    PROFILE_KINDS = {"line_prep": 0, "xsec_accumulate": 1, "regrid": 2, "layer_sweep": 3, "column_sweep": 4,
                     "allgather": 5}

    def profile_enable(self, kinds=True):
        """kinds: True (all), False (off) or an iterable of PROFILE_KINDS names."""
        if kinds is True:
            mask = 0x3F
        elif not kinds:
            mask = 0
        else:
            mask = 0
            for k in kinds:
                mask |= 1 << self.PROFILE_KINDS[k]
        self.check(self.lib.lbl_profile_enable(self.h, mask))

    def profile_reserve(self, n_events: int):
        self.check(self.lib.lbl_profile_reserve(self.h, int(n_events)))

    def profile_reset(self):
        self.check(self.lib.lbl_profile_reset(self.h))

    def profile_read(self) -> dict:
        """{kernel class: (launches, total_ms)} measured with HIP events on the context stream."""
        out = {}
        for name, kind in self.PROFILE_KINDS.items():
            n = C.c_int64()
            ms = C.c_double()
            self.check(self.lib.lbl_profile_read(self.h, kind, C.byref(n), C.byref(ms)))
            out[name] = (n.value, ms.value)
        return out

    # -- graph capture -------------------------------------------------------------------
    def capture(self, enqueue_fn) -> "Graph":
        """Capture what ``enqueue_fn()`` enqueues into a graph (run it once yourself first)."""
        self.check(self.lib.lbl_capture_begin(self.h))
        err = None
        try:
            enqueue_fn()
        except Exception as e:                 # the capture has to be ended whatever happened inside
            err = e
        h = _P()
        rc = self.lib.lbl_capture_end(self.h, C.byref(h))
        if err is not None:
            if rc == LBL_OK and h:
                self.lib.lbl_graph_destroy(h)
            raise err
        self.check(rc)
        return Graph(self, h)

    # -- page-locked host arrays ---------------------------------------------------------
    def host_array(self, n: int) -> np.ndarray:
        """float64 array of n elements in page-locked host memory (lbl_host_alloc): downloads into it
        and uploads from it run at the link's DMA rate.  The block returns to a per-context pool when
        the array (and every view of it) is gone, and is released with the context."""
        import weakref
        nbytes = max(int(n), 1) * 8
        cls = 1 << max(nbytes - 1, 1).bit_length()             # pool by power-of-two size class
        pool = self.__dict__.setdefault("_pinned_pool", {})
        # the smallest idle block that is large enough, up to four times the need (page-locking a new one costs ~0.2 ms per
        # MB); else a new one of this class
        fit = min((c for c, blocks in pool.items() if cls <= c <= 4 * cls and blocks), default=None)
        if fit is not None:
            cls = fit
            ptr = pool[fit].pop()
        else:
            p = _P()
            self.check(self.lib.lbl_host_alloc(self.h, cls, C.byref(p)))
            ptr = p.value
        raw = (C.c_char * nbytes).from_address(ptr)
        arr = np.frombuffer(raw, dtype=np.float64, count=int(n))
        weakref.finalize(raw, Context._recycle, weakref.ref(self), self.lib, cls, ptr)
        return arr

    @staticmethod
    def _recycle(ctx_ref, lib, cls, ptr):
        """the last array over a block is gone: back to the pool, or freed if its context has closed"""
        ctx = ctx_ref()
        if ctx is not None and getattr(ctx, "h", None):
            ctx.__dict__.setdefault("_pinned_pool", {}).setdefault(cls, []).append(ptr)
        else:
            lib.lbl_host_free(None, ptr)

    # -- objects -------------------------------------------------------------------------
    def buffer(self, n: int, data=None) -> "Buffer":
        b = Buffer(self, n)
        if data is not None:
            b.upload(data)
        return b

    def lines(self, lines: dict) -> "Lines":
        return Lines(self, lines)

    # -- hot path ------------------------------------------------------------------------
    def xsec_accumulate(self, lines: dict, iso: IsoParams, grid: Grid):
        """One-shot host in / host out (lbl_xsec_accumulate). Returns (xsec, regime_counts).
        The C entry point wants nu non-decreasing; an unsorted list is sorted here (stable)."""
        nu = _as_f64(lines["nu"])
        if nu.size > 1 and np.any(np.diff(nu) < 0):
            order = np.argsort(nu, kind="stable")
            lines = {k: np.asarray(lines[k])[order] for k in Lines.ORDER}
        arrs = [_as_f64(lines[k]) for k in Lines.ORDER]
        out = np.empty(int(grid.n_base), dtype=np.float64)
        counts = (C.c_int64 * 3)()
        self.check(self.lib.lbl_xsec_accumulate(self.h, *[_ptr(a) for a in arrs], len(arrs[0]),
                                                C.byref(iso), C.byref(grid), _ptr(out), counts))
        return out, tuple(int(c) for c in counts)

    def xsec_accumulate_dev(self, jobs):
        """jobs: list of (Lines, IsoParams, Grid, Buffer). Asynchronous."""
        n = len(jobs)
        if n == 0:
            return
        L = (_P * n)(*[j[0].h for j in jobs])
        I = (IsoParams * n)(*[j[1] for j in jobs])
        G = (Grid * n)(*[j[2] for j in jobs])
        O = (_P * n)(*[j[3].h for j in jobs])
        self.check(self.lib.lbl_xsec_accumulate_dev(self.h, n, L, I, G, O))

    def xsec_voigt_dev(self, jobs):
        """xsec_accumulate_dev's jobs with the true Voigt line shape (lbl_xsec_voigt_dev). Asynchronous."""
        n = len(jobs)
        if n == 0:
            return
        L = (_P * n)(*[j[0].h for j in jobs])
        I = (IsoParams * n)(*[j[1] for j in jobs])
        G = (Grid * n)(*[j[2] for j in jobs])
        O = (_P * n)(*[j[3].h for j in jobs])
        self.check(self.lib.lbl_xsec_voigt_dev(self.h, n, L, I, G, O))

    def voigt_function_dev(self, x, y, n, out):
        """out[i] = Re w(x[i] + 1j * y[i]) for i < n, by the device function the Voigt accumulate kernel inlines."""
        self.check(self.lib.lbl_voigt_function_dev(self.h, x.h, y.h, int(n), out.h))

    def xsec_voigt_dT_dev(self, jobs, dlnw_dT):
        """d(cross section)/dT of xsec_voigt_dev's jobs (lbl_xsec_voigt_dt_dev); dlnw_dT[j]: the logarithmic T-derivative of what
        multiplies job j's intensities beside the line preparation's own factors (-dlnQ/dT for a cross section). Asynchronous."""
        n = len(jobs)
        if len(dlnw_dT) != n:
            raise ValueError("one dlnw_dT per job")
        if n == 0:
            return
        L = (_P * n)(*[j[0].h for j in jobs])
        I = (IsoParams * n)(*[j[1] for j in jobs])
        G = (Grid * n)(*[j[2] for j in jobs])
        O = (_P * n)(*[j[3].h for j in jobs])
        W = (C.c_double * n)(*[float(v) for v in dlnw_dT])
        self.check(self.lib.lbl_xsec_voigt_dt_dev(self.h, n, L, I, W, G, O))

    def voigt_gradient_dev(self, x, y, n, K, GX, GY):
        """K, GX = x dK/dx, GY = y dK/dy of K = Re w(x + 1j * y), elementwise, by the device function the dT kernel inlines."""
        self.check(self.lib.lbl_voigt_gradient_dev(self.h, x.h, y.h, int(n), K.h, GX.h, GY.h))

    def schedule_export(self, k: int = 0):
        """(list[n, 2] of (job, tile), tabs[spans, 8], built_on_device) of the k-th most recently used schedule."""
        n = C.c_int64(); nt = C.c_int64(); dev = C.c_int32()
        self.check(self.lib.lbl_schedule_export(self.h, int(k), None, 0, None, 0, C.byref(n), C.byref(nt), C.byref(dev)))
        lst = np.empty((n.value, 2), np.int32); tabs = np.empty((max(nt.value, 0) // 8, 8), np.int32)
        self.check(self.lib.lbl_schedule_export(self.h, int(k), _ptr(lst), lst.size, _ptr(tabs), tabs.size, C.byref(n),
                                                C.byref(nt), C.byref(dev)))
        return lst, tabs, bool(dev.value)

    def last_regime_counts(self, n_jobs: int):
        counts = (C.c_int64 * (3 * n_jobs))()
        self.check(self.lib.lbl_last_regime_counts(self.h, n_jobs, counts))
        return np.array(counts, dtype=np.int64).reshape(n_jobs, 3)

    def line_quantities(self, lines: "Lines", iso: IsoParams, grid: Grid):
        n = lines.n
        index = np.empty(n, np.int64); lhw = np.empty(n); ghw = np.empty(n); inten = np.empty(n)
        regime = np.empty(n, np.int32)
        self.check(self.lib.lbl_line_quantities(self.h, lines.h, C.byref(iso), C.byref(grid), _ptr(index), _ptr(lhw),
                                                _ptr(ghw), _ptr(inten), _ptr(regime)))
        return dict(index=index, lhw=lhw, ghw=ghw, intensity=inten, regime=regime)

    def layer_sweep_dev(self, xsec, iso_mol, conc, P, T, depth, range_min, range_max, n,
                        I_in=None, surface_T=0.0, abs_coef=None, trans=None, I_out=None, first=0, count=0):
        self.check(self.lib.lbl_layer_sweep_dev(
            self.h, len(xsec), _arr(_P, [b.h for b in xsec]), _arr(C.c_int32, [int(m) for m in iso_mol]), len(conc),
            _arr(C.c_double, [float(c) for c in conc]), float(P), float(T), float(depth), float(range_min),
            float(range_max), int(n), int(first), int(count), _hb(I_in), float(surface_T), _hb(abs_coef), _hb(trans),
            _hb(I_out)))

    @staticmethod
    def _layer_lists(lines, iso, iso_mol, conc, xsec=None):
        """The per-line-list arguments of layer_step_dev and layer_merged_step_dev as C arrays: (n, lines, iso, xsec, iso_mol,
        number of molecules, conc).  A single Lines / IsoParams / Buffer is taken as one line list, a scalar ``conc`` as one
        molecule, ``iso_mol`` None as one molecule per line list."""
        if isinstance(lines, Lines):
            lines, iso, xsec = [lines], [iso], None if xsec is None else [xsec]
        if np.isscalar(conc):
            conc = [conc]
        if iso_mol is None:
            iso_mol = list(range(len(lines)))
        n = len(lines)
        return (n, (_P * n)(*[l.h for l in lines]), (IsoParams * n)(*iso), None if xsec is None else (_P * n)(*[b.h for b in xsec]),
                (C.c_int32 * n)(*[int(m) for m in iso_mol]), len(conc), _arr(C.c_double, [float(c) for c in conc]))

    def layer_step_dev(self, lines, iso, grid: Grid, xsec, iso_mol, conc, depth, I_in=None, surface_T=0.0,
                       abs_coef=None, trans=None, I_out=None):
        """Accumulate + sweep of one layer in one launch sequence (lbl_layer_step_dev): ``lines`` /
        ``iso`` / ``xsec`` are per line list (a single Lines / IsoParams / Buffer is taken as one),
        ``iso_mol`` maps line list -> molecule, ``conc`` is per molecule."""
        n, L, I, X, M, n_mol, cc = self._layer_lists(lines, iso, iso_mol, conc, xsec)
        self.check(self.lib.lbl_layer_step_dev(self.h, n, L, I, C.byref(grid), X, M, n_mol, cc, float(depth), _hb(I_in),
                                               float(surface_T), _hb(abs_coef), _hb(trans), _hb(I_out)))

    def layer_merged_step_dev(self, lines, iso, grid: Grid, iso_mol, conc, depth, I_in=None, surface_T=0.0,
                              abs_coef=None, trans=None, I_out=None):
        """One layer through ONE accumulate job over its merged, factor-weighted line lists with the sweep in the
        output stage (lbl_layer_merged_step_dev): the absorption coefficient is accumulated directly, no
        per-line-list cross section is written.  Arguments as layer_step_dev without ``xsec``."""
        n, L, I, _, M, n_mol, cc = self._layer_lists(lines, iso, iso_mol, conc)
        self.check(self.lib.lbl_layer_merged_step_dev(self.h, n, L, I, C.byref(grid), M, n_mol, cc, float(depth),
                                                      _hb(I_in), float(surface_T), _hb(abs_coef), _hb(trans), _hb(I_out)))

    def layers_merged_accumulate_dev(self, layers):
        """layers: list of dict(lines=[Lines], iso=[IsoParams], grid=Grid, iso_mol=[int], conc=[float], abs_coef=Buffer):
        every layer's absorption coefficient through one merged accumulate job per layer, all in one launch sequence
        (lbl_layers_merged_accumulate_dev)."""
        nl = len(layers)
        if nl == 0:
            return
        ls = [l for L in layers for l in L["lines"]]
        self.check(self.lib.lbl_layers_merged_accumulate_dev(
            self.h, nl, _arr(C.c_int32, [len(L["lines"]) for L in layers]), _arr(_P, [l.h for l in ls]),
            _arr(IsoParams, [i for L in layers for i in L["iso"]]), _arr(Grid, [L["grid"] for L in layers]),
            _arr(C.c_int32, [int(m) for L in layers for m in L["iso_mol"]]), _arr(C.c_int32, [len(L["conc"]) for L in layers]),
            _arr(C.c_double, [float(c) for L in layers for c in L["conc"]]), _arr(_P, [L["abs_coef"].h for L in layers])))

    def column(self, layers):
        """Resident column (lbl_column_create): ``layers`` as for layers_merged_accumulate_dev, each with ``depth``."""
        return Column(self, layers)

    def column_fold_dev(self, abs_coef, layer_T, depth, range_min, range_max, n, I_out, I_in=None, surface_T=0.0,
                        trans=None, first=0, count=0):
        """Column step from the layers' absorption coefficients, bottom to top (lbl_column_fold_dev); ``trans``: None or
        a list (entries may be None) of buffers that receive the layers' transmittances."""
        nl = len(abs_coef)
        self.check(self.lib.lbl_column_fold_dev(
            self.h, nl, _arr(_P, [b.h for b in abs_coef]), _arr(C.c_double, [float(t) for t in layer_T]),
            _arr(C.c_double, [float(d) for d in depth]), float(range_min), float(range_max), int(n), int(first), int(count),
            _hb(I_in), float(surface_T), _arr(_P, [_hb(b) for b in trans]) if trans is not None else None, I_out.h))

    def _column_args(self, abs_coef, layer_T, depth, range_min, range_max, n, I_surface, surface_T, after_surface, mu,
                     weight, band_first, band_count):
        """The leading arguments lbl_column_flux_dev and lbl_column_jacobian_dev share, from ctx to band_count
        (``after_surface``: what the entry point takes between surface_T and the angle set)."""
        return (self.h, len(abs_coef), _arr(_P, [b.h for b in abs_coef]), _arr(C.c_double, [float(t) for t in layer_T]),
                _arr(C.c_double, [float(d) for d in depth]), float(range_min), float(range_max), int(n), _hb(I_surface),
                float(surface_T), *after_surface, len(mu), _arr(C.c_double, [float(m) for m in mu]),
                _arr(C.c_double, [float(w) for w in weight]), len(band_first), _arr(C.c_int64, [int(f) for f in band_first]),
                _arr(C.c_int64, [int(c) for c in band_count]))

    def column_flux_dev(self, abs_coef, layer_T, depth, range_min, range_max, n, mu, weight, band_first, band_count,
                        level_flux, I_surface=None, surface_T=0.0, I_top=None, up_top=None, down_surface=None):
        """Level fluxes of a column from the layers' absorption coefficients (lbl_column_flux_dev): ``level_flux`` receives
        len(band_first) x 2 x (layers + 1) band sums [band][up, down][level]; ``up_top`` / ``down_surface`` (optional, n
        points) the spectral upward flux at the top and downward flux at the surface."""
        self.check(self.lib.lbl_column_flux_dev(
            *self._column_args(abs_coef, layer_T, depth, range_min, range_max, n, I_surface, surface_T, (_hb(I_top),), mu,
                               weight, band_first, band_count),
            _hb(level_flux), _hb(up_top), _hb(down_surface)))

    REFLECTIONS = ("lambertian", "specular")        # the C ABI's ``reflection`` is the index

    @staticmethod
    def _emissivity_args(emissivity):
        """(buffer handle or None, emissivity_all) from a Buffer or a number"""
        if isinstance(emissivity, Buffer):
            return emissivity.h, 1.0
        return None, float(emissivity)

    @staticmethod
    def _edge_T(name, edge_T, abs_coef):
        """``edge_T`` of the column_*_linear_dev wrapper ``name`` as 2 L numbers"""
        edge_T = _as_f64(edge_T).reshape(-1)
        if len(edge_T) != 2 * len(abs_coef):
            raise ValueError("%s: two edge temperatures per layer" % name)
        return edge_T

    @staticmethod
    def _term_args(term_abs_coef, term_layer):
        """(count, buffers, layers) of the terms the column_jacobian_* and ray_jacobian_* entry points take"""
        return len(term_abs_coef), _arr(_P, [b.h for b in term_abs_coef]), _arr(C.c_int32, [int(l) for l in term_layer])

    def _ray_args(self, name, abs_coef, T, range_min, range_max, n, ray_first, seg_layer, seg_length, source_kind, I_source,
                  source_T, seg_T=False, terms=None):
        """The leading arguments the lbl_ray_* entry points share, from ctx to source_T, behind the length checks of the
        wrapper ``name``.  ``T``: the layers' temperatures or, with ``seg_T``, two per segment; ``terms``: None or a
        Jacobian's (term_abs_coef, term_layer)."""
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        ray_first, seg_layer, source_kind = i32(ray_first), i32(seg_layer), i32(source_kind)
        seg_length = _as_f64(seg_length)
        if seg_T:
            T = _as_f64(T).reshape(-1)
        if (len(ray_first) != len(source_kind) + 1 or len(seg_layer) != len(seg_length)
                or (seg_T and len(T) != 2 * len(seg_layer)) or (terms is not None and len(terms[0]) != len(terms[1]))):
            raise ValueError("%s: one ray_first per ray and one more, one length%s per segment layer%s"
                             % (name, " and two temperatures" if seg_T else "", "" if terms is None else ", one layer per term"))
        return (self.h, len(abs_coef), _arr(_P, [b.h for b in abs_coef]),
                T.ctypes.data_as(_D) if seg_T else _arr(C.c_double, [float(t) for t in T]), float(range_min),
                float(range_max), int(n), len(source_kind), i32p(ray_first), i32p(seg_layer), seg_length.ctypes.data_as(_D),
                i32p(source_kind), _hb(I_source), float(source_T))

    def column_flux_surface_dev(self, abs_coef, layer_T, depth, range_min, range_max, n, mu, weight, band_first, band_count,
                                level_flux, emissivity, reflection=0, I_surface=None, surface_T=0.0, I_top=None, up_top=None,
                                down_surface=None, up_surface=None):
        """Level fluxes over a reflecting surface (lbl_column_flux_surface_dev): column_flux_dev's arguments and results,
        with ``emissivity`` a Buffer of n points or one number in [0, 1], ``reflection`` 0 (Lambertian) or 1 (specular), and
        ``up_surface`` (optional, n points) the spectral upward flux at the surface."""
        self.check(self.lib.lbl_column_flux_surface_dev(
            *self._column_args(abs_coef, layer_T, depth, range_min, range_max, n, I_surface, surface_T, (_hb(I_top),), mu,
                               weight, band_first, band_count),
            *self._emissivity_args(emissivity), int(reflection), _hb(level_flux), _hb(up_top), _hb(down_surface),
            _hb(up_surface)))

    def column_flux_linear_dev(self, abs_coef, edge_T, depth, range_min, range_max, n, mu, weight, band_first, band_count,
                               level_flux, emissivity=1.0, reflection=0, I_surface=None, surface_T=0.0, I_top=None, up_top=None,
                               down_surface=None, up_surface=None):
        """Level fluxes with a Planck source linear in optical depth (lbl_column_flux_linear_dev): column_flux_surface_dev's
        arguments and results with ``edge_T`` in place of the layers' temperatures - per layer (bottom edge, top edge), as L
        pairs or 2 L numbers.  The default ``emissivity`` 1 is the black surface."""
        self.check(self.lib.lbl_column_flux_linear_dev(
            *self._column_args(abs_coef, self._edge_T("column_flux_linear_dev", edge_T, abs_coef), depth, range_min, range_max,
                               n, I_surface, surface_T, (_hb(I_top),), mu, weight, band_first, band_count),
            *self._emissivity_args(emissivity), int(reflection), _hb(level_flux), _hb(up_top), _hb(down_surface),
            _hb(up_surface)))

    def column_solar_dev(self, abs_coef, depth, range_min, range_max, n, S0, beam_weight, slant, mu, weight, band_first,
                         band_count, level_flux, emissivity=1.0, reflection=0, up_top=None, down_surface=None, up_surface=None):
        """The direct solar beam (lbl_column_solar_dev): ``S0`` a Buffer of n points, the beams' irradiance at the top;
        ``beam_weight`` one number per beam; ``slant`` beams x layers path lengths per unit depth; ``mu`` / ``weight`` the
        diffuse angles of a Lambertian surface (may be empty for ``reflection`` 1); ``emissivity`` and ``reflection`` as
        column_flux_surface_dev takes them.  ``level_flux`` receives len(band_first) x 2 x (layers + 1) band sums [band][up,
        down][level]; ``up_top`` / ``down_surface`` / ``up_surface`` (optional, n points) the spectral fluxes."""
        nl, ns = len(abs_coef), len(beam_weight)
        slant = _as_f64(slant).reshape(-1)
        if len(slant) != ns * nl:
            raise ValueError("column_solar_dev: one slant per beam and layer")
        self.check(self.lib.lbl_column_solar_dev(
            self.h, nl, _arr(_P, [b.h for b in abs_coef]), _arr(C.c_double, [float(d) for d in depth]), float(range_min),
            float(range_max), int(n), _hb(S0), ns, _arr(C.c_double, [float(w) for w in beam_weight]),
            _arr(C.c_double, [float(v) for v in slant]), len(mu), _arr(C.c_double, [float(m) for m in mu]),
            _arr(C.c_double, [float(w) for w in weight]), len(band_first), _arr(C.c_int64, [int(f) for f in band_first]),
            _arr(C.c_int64, [int(c) for c in band_count]), *self._emissivity_args(emissivity), int(reflection),
            _hb(level_flux), _hb(up_top), _hb(down_surface), _hb(up_surface)))

    def _scatter_workspace(self, entry, n_layers, points):
        """The doubles the lbl_column_*_workspace function ``entry`` gives for ``points`` points in one pass"""
        out = C.c_int64()
        self.check(entry(int(n_layers), int(points), C.byref(out)))
        return out.value

    @staticmethod
    def _scatter_args(name, abs_coef, scat_amount, scat_ext, scat_ssa, scat_asym):
        """The scatterer arguments of the two-stream entry points, from n_scat to scat_asym_all, behind the length check
        of the wrapper ``name``: each number a Buffer of n points or a number"""
        nl, nc = len(abs_coef), len(scat_ext)
        amount = _as_f64(scat_amount).reshape(-1)
        if len(amount) != nc * nl or len(scat_ssa) != nc or len(scat_asym) != nc:
            raise ValueError("%s: one amount per scatterer and layer, one of each number per scatterer" % name)

        def numbers(vals):
            return (_arr(_P, [v.h if isinstance(v, Buffer) else None for v in vals]),
                    _arr(C.c_double, [0.0 if isinstance(v, Buffer) else float(v) for v in vals]))
        return (nc, _arr(C.c_double, [float(v) for v in amount]), *numbers(scat_ext), *numbers(scat_ssa), *numbers(scat_asym))

    @staticmethod
    def _scatter_T(name, T, planck_linear, abs_coef):
        """``T`` of the column_*_scatter_dev wrapper ``name`` as L numbers, or 2 L with ``planck_linear``"""
        T = _as_f64(T).reshape(-1)
        if len(T) != (2 if planck_linear else 1) * len(abs_coef):
            raise ValueError("%s: one temperature per layer, or two with planck_linear" % name)
        return _arr(C.c_double, [float(t) for t in T])

    def column_twostream_workspace(self, n_layers, points):
        """The doubles of a workspace with which column_twostream_dev does ``points`` points in one pass
        (lbl_column_twostream_workspace: whole tiles, at least one)."""
        return self._scatter_workspace(self.lib.lbl_column_twostream_workspace, n_layers, points)

    def column_twostream_dev(self, abs_coef, depth, range_min, range_max, n, S0, beam_weight, slant, scat_amount, scat_ext,
                             scat_ssa, scat_asym, delta_scaling, band_first, band_count, workspace, level_flux, emissivity=1.0,
                             up_top=None, down_surface=None, direct_surface=None, up_surface=None):
        """Two-stream multiple scattering of the solar beams (lbl_column_twostream_dev): ``S0``, ``beam_weight`` and ``slant``
        as column_solar_dev takes them (every slant > 0); ``scat_amount`` scatterers x layers; ``scat_ext`` / ``scat_ssa`` /
        ``scat_asym`` one entry per scatterer, a Buffer of n points or a number; ``workspace`` a Buffer of at least
        column_twostream_workspace(layers, 1) doubles.  ``level_flux`` receives len(band_first) x 3 x (layers + 1) band sums
        [band][up, diffuse down, direct][level]; ``up_top`` / ``down_surface`` (diffuse) / ``direct_surface`` / ``up_surface``
        (optional, n points) the spectral fluxes."""
        nl, ns = len(abs_coef), len(beam_weight)
        slant = _as_f64(slant).reshape(-1)
        if len(slant) != ns * nl:
            raise ValueError("column_twostream_dev: one slant per beam and layer")
        scat = self._scatter_args("column_twostream_dev", abs_coef, scat_amount, scat_ext, scat_ssa, scat_asym)
        self.check(self.lib.lbl_column_twostream_dev(
            self.h, nl, _arr(_P, [b.h for b in abs_coef]), _arr(C.c_double, [float(d) for d in depth]), float(range_min),
            float(range_max), int(n), _hb(S0), ns, _arr(C.c_double, [float(w) for w in beam_weight]),
            _arr(C.c_double, [float(v) for v in slant]), *scat, int(delta_scaling), len(band_first),
            _arr(C.c_int64, [int(f) for f in band_first]), _arr(C.c_int64, [int(c) for c in band_count]),
            *self._emissivity_args(emissivity), _hb(workspace), _hb(level_flux), _hb(up_top), _hb(down_surface),
            _hb(direct_surface), _hb(up_surface)))

    def column_flux_scatter_workspace(self, n_layers, points):
        """The doubles of a workspace with which column_flux_scatter_dev does ``points`` points in one pass
        (lbl_column_flux_scatter_workspace: four numbers per level and point, whole tiles, at least one)."""
        return self._scatter_workspace(self.lib.lbl_column_flux_scatter_workspace, n_layers, points)

    def column_flux_scatter_dev(self, abs_coef, T, planck_linear, depth, range_min, range_max, n, scat_amount, scat_ext,
                                scat_ssa, scat_asym, delta_scaling, band_first, band_count, workspace, level_flux,
                                emissivity=1.0, I_surface=None, surface_T=0.0, I_top=None, up_top=None, down_surface=None,
                                up_surface=None):
        """Thermal fluxes through scattering layers (lbl_column_flux_scatter_dev): ``T`` the layers' temperatures or, with
        ``planck_linear`` 1, per layer (bottom edge, top edge) as L pairs or 2 L numbers; the surface source, ``I_top`` and
        ``emissivity`` as column_flux_surface_dev takes them; scatterers, bands and ``workspace`` (at least
        column_flux_scatter_workspace(layers, 1) doubles) as column_twostream_dev takes them.  ``level_flux`` receives
        len(band_first) x 2 x (layers + 1) band sums [band][up, down][level]; ``up_top`` / ``down_surface`` / ``up_surface``
        (optional, n points) the spectral fluxes."""
        T = self._scatter_T("column_flux_scatter_dev", T, planck_linear, abs_coef)
        scat = self._scatter_args("column_flux_scatter_dev", abs_coef, scat_amount, scat_ext, scat_ssa, scat_asym)
        self.check(self.lib.lbl_column_flux_scatter_dev(
            self.h, len(abs_coef), _arr(_P, [b.h for b in abs_coef]), T, int(planck_linear),
            _arr(C.c_double, [float(d) for d in depth]), float(range_min), float(range_max), int(n), _hb(I_surface),
            float(surface_T), _hb(I_top), *scat, int(delta_scaling), len(band_first),
            _arr(C.c_int64, [int(f) for f in band_first]), _arr(C.c_int64, [int(c) for c in band_count]),
            *self._emissivity_args(emissivity), _hb(workspace), _hb(level_flux), _hb(up_top), _hb(down_surface),
            _hb(up_surface)))

    def column_jacobian_scatter_workspace(self, n_layers, points):
        """The doubles of a workspace with which column_jacobian_scatter_dev does ``points`` points in one pass
        (lbl_column_jacobian_scatter_workspace: five numbers per level and point, whole tiles, at least one)."""
        return self._scatter_workspace(self.lib.lbl_column_jacobian_scatter_workspace, n_layers, points)

    def column_jacobian_scatter_dev(self, abs_coef, T, planck_linear, depth, range_min, range_max, n, scat_amount, scat_ext,
                                    scat_ssa, scat_asym, delta_scaling, band_first, band_count, workspace, jac,
                                    emissivity=1.0, I_surface=None, surface_T=0.0, I_top=None, term_abs_coef=(), term_layer=(),
                                    ln_tau_spectra=None, T_spectra=None, up_top=None):
        """Jacobians of the upward flux at the top through scattering layers (lbl_column_jacobian_scatter_dev):
        column_flux_scatter_dev's column, scatterers, surface, ``I_top`` and bands, the terms as column_jacobian_dev takes
        them and ``workspace`` of at least column_jacobian_scatter_workspace(layers, 1) doubles.  With NT = 2 for
        ``planck_linear`` 1 and 1 otherwise, ``jac`` receives len(band_first) x (3 + (1 + NT + scatterers) L + terms) band
        sums [band][F, dF/dT_s, dF/de, L x dF/d ln tau, NT L x dF/dT (per layer; NT = 2: bottom, top edge), scatterers x L
        dF/d ln amount, terms]; ``ln_tau_spectra`` (L x n), ``T_spectra`` (NT L x n) and ``up_top`` (n) are optional."""
        T = self._scatter_T("column_jacobian_scatter_dev", T, planck_linear, abs_coef)
        scat = self._scatter_args("column_jacobian_scatter_dev", abs_coef, scat_amount, scat_ext, scat_ssa, scat_asym)
        if len(term_abs_coef) != len(term_layer):
            raise ValueError("column_jacobian_scatter_dev: one layer per term")
        self.check(self.lib.lbl_column_jacobian_scatter_dev(
            self.h, len(abs_coef), _arr(_P, [b.h for b in abs_coef]), T, int(planck_linear),
            _arr(C.c_double, [float(d) for d in depth]), float(range_min), float(range_max), int(n), _hb(I_surface),
            float(surface_T), _hb(I_top), *scat, int(delta_scaling), len(band_first),
            _arr(C.c_int64, [int(f) for f in band_first]), _arr(C.c_int64, [int(c) for c in band_count]),
            *self._emissivity_args(emissivity), *self._term_args(term_abs_coef, term_layer), _hb(workspace), _hb(jac),
            _hb(ln_tau_spectra), _hb(T_spectra), _hb(up_top)))

    def column_radiance_scatter_workspace(self, n_layers, points):
        """The doubles of a workspace with which column_radiance_scatter_dev does ``points`` points in one pass
        (lbl_column_radiance_scatter_workspace: column_flux_scatter_workspace's)."""
        return self._scatter_workspace(self.lib.lbl_column_radiance_scatter_workspace, n_layers, points)

    def column_radiance_scatter_dev(self, abs_coef, T, planck_linear, depth, range_min, range_max, n, scat_amount, scat_ext,
                                    scat_ssa, scat_asym, delta_scaling, view_mu, view_down, workspace, radiance,
                                    emissivity=1.0, I_surface=None, surface_T=0.0, I_top=None, up_top=None, down_surface=None):
        """Radiances through scattering layers (lbl_column_radiance_scatter_dev): the column, the scatterers, the surface,
        ``I_top`` and ``workspace`` as column_flux_scatter_dev takes them, over the whole grid; ``view_mu`` the viewing
        cosines and ``view_down`` per view 0 (upward at the top) or 1 (downward at the surface).  ``radiance`` receives
        len(view_mu) x n values; ``up_top`` / ``down_surface`` (optional, n points) column_flux_scatter_dev's spectra."""
        T = self._scatter_T("column_radiance_scatter_dev", T, planck_linear, abs_coef)
        scat = self._scatter_args("column_radiance_scatter_dev", abs_coef, scat_amount, scat_ext, scat_ssa, scat_asym)
        if len(view_down) != len(view_mu):
            raise ValueError("column_radiance_scatter_dev: one direction per view")
        self.check(self.lib.lbl_column_radiance_scatter_dev(
            self.h, len(abs_coef), _arr(_P, [b.h for b in abs_coef]), T, int(planck_linear),
            _arr(C.c_double, [float(d) for d in depth]), float(range_min), float(range_max), int(n), _hb(I_surface),
            float(surface_T), _hb(I_top), *scat, int(delta_scaling), *self._emissivity_args(emissivity),
            len(view_mu), _arr(C.c_double, [float(m) for m in view_mu]), _arr(C.c_int32, [int(d) for d in view_down]),
            _hb(workspace), _hb(radiance), _hb(up_top), _hb(down_surface)))

    def column_beam_radiance_workspace(self, n_layers, points):
        """The doubles of a workspace with which column_beam_radiance_dev does ``points`` points in one pass
        (lbl_column_beam_radiance_workspace: column_twostream_workspace's)."""
        return self._scatter_workspace(self.lib.lbl_column_beam_radiance_workspace, n_layers, points)

    def column_beam_radiance_dev(self, abs_coef, depth, range_min, range_max, n, S0, beam_weight, slant, scat_amount, scat_ext,
                                 scat_ssa, scat_asym, delta_scaling, view_mu, view_down, workspace, radiance, emissivity=1.0,
                                 up_top=None, down_surface=None, direct_surface=None):
        """Scattered sunlight along views (lbl_column_beam_radiance_dev): one sun - ``S0``, one ``beam_weight`` and one
        ``slant`` per layer - through the column, the scatterers, the surface and the ``workspace`` that
        column_twostream_dev takes, over the whole grid; ``view_mu`` and ``view_down`` as column_radiance_scatter_dev takes
        them.  ``radiance`` receives len(view_mu) x n values; ``up_top`` / ``down_surface`` (diffuse) / ``direct_surface``
        (optional, n points) column_twostream_dev's spectra."""
        slant = _as_f64(slant).reshape(-1)
        if len(slant) != len(abs_coef):
            raise ValueError("column_beam_radiance_dev: one slant per layer")
        scat = self._scatter_args("column_beam_radiance_dev", abs_coef, scat_amount, scat_ext, scat_ssa, scat_asym)
        if len(view_down) != len(view_mu):
            raise ValueError("column_beam_radiance_dev: one direction per view")
        self.check(self.lib.lbl_column_beam_radiance_dev(
            self.h, len(abs_coef), _arr(_P, [b.h for b in abs_coef]), _arr(C.c_double, [float(d) for d in depth]),
            float(range_min), float(range_max), int(n), _hb(S0), float(beam_weight),
            _arr(C.c_double, [float(v) for v in slant]), *scat, int(delta_scaling), *self._emissivity_args(emissivity),
            len(view_mu), _arr(C.c_double, [float(m) for m in view_mu]), _arr(C.c_int32, [int(d) for d in view_down]),
            _hb(workspace), _hb(radiance), _hb(up_top), _hb(down_surface), _hb(direct_surface)))

    def column_jacobian_dev(self, abs_coef, layer_T, depth, range_min, range_max, n, mu, weight, band_first, band_count,
                            jac, I_surface=None, surface_T=0.0, term_abs_coef=(), term_layer=(), ln_tau_spectra=None,
                            T_spectra=None):
        """Jacobians of the upward flux at the top (lbl_column_jacobian_dev): ``jac`` receives len(band_first) x (2 + 2 L +
        len(term_abs_coef)) band sums [band][F, dF/dT_s, L x dF/d ln tau, L x dF/dT, terms x dF/d ln n]; ``term_layer``
        gives each term's layer; ``ln_tau_spectra`` / ``T_spectra`` (optional, L x n points) the spectral values."""
        self.check(self.lib.lbl_column_jacobian_dev(
            *self._column_args(abs_coef, layer_T, depth, range_min, range_max, n, I_surface, surface_T, (), mu, weight,
                               band_first, band_count),
            *self._term_args(term_abs_coef, term_layer), _hb(jac), _hb(ln_tau_spectra), _hb(T_spectra)))

    def column_jacobian_surface_dev(self, abs_coef, layer_T, depth, range_min, range_max, n, mu, weight, band_first,
                                    band_count, jac, emissivity, reflection=0, I_surface=None, surface_T=0.0, I_top=None,
                                    term_abs_coef=(), term_layer=(), ln_tau_spectra=None, T_spectra=None, e_spectrum=None):
        """Jacobians of the upward flux at the top over a reflecting surface (lbl_column_jacobian_surface_dev):
        column_jacobian_dev's arguments with ``emissivity``, ``reflection`` and ``I_top`` as column_flux_surface_dev takes
        them; ``jac`` receives len(band_first) x (3 + 2 L + len(term_abs_coef)) band sums [band][F, dF/dT_s, dF/de, L x
        dF/d ln tau, L x dF/dT, terms]; ``e_spectrum`` (optional, n points) the spectral dF/de."""
        self.check(self.lib.lbl_column_jacobian_surface_dev(
            *self._column_args(abs_coef, layer_T, depth, range_min, range_max, n, I_surface, surface_T, (_hb(I_top),), mu,
                               weight, band_first, band_count),
            *self._emissivity_args(emissivity), int(reflection), *self._term_args(term_abs_coef, term_layer), _hb(jac),
            _hb(ln_tau_spectra), _hb(T_spectra), _hb(e_spectrum)))

    def column_jacobian_linear_dev(self, abs_coef, edge_T, depth, range_min, range_max, n, mu, weight, band_first,
                                   band_count, jac, emissivity=1.0, reflection=0, I_surface=None, surface_T=0.0, I_top=None,
                                   term_abs_coef=(), term_layer=(), ln_tau_spectra=None, T_edge_spectra=None,
                                   e_spectrum=None):
        """Jacobians of the upward flux at the top with a Planck source linear in optical depth
        (lbl_column_jacobian_linear_dev): column_jacobian_surface_dev's arguments with ``edge_T`` in place of the layers'
        temperatures - per layer (bottom edge, top edge), as L pairs or 2 L numbers; ``jac`` receives len(band_first) x (3 +
        3 L + len(term_abs_coef)) band sums [band][F, dF/dT_s, dF/de, L x dF/d ln tau, 2 L x dF/dT_edge (bottom, top per
        layer), terms]; ``T_edge_spectra`` (optional, 2 L x n points) the spectral edge values.  The default ``emissivity`` 1
        is the black surface."""
        self.check(self.lib.lbl_column_jacobian_linear_dev(
            *self._column_args(abs_coef, self._edge_T("column_jacobian_linear_dev", edge_T, abs_coef), depth, range_min,
                               range_max, n, I_surface, surface_T, (_hb(I_top),), mu, weight, band_first, band_count),
            *self._emissivity_args(emissivity), int(reflection), *self._term_args(term_abs_coef, term_layer), _hb(jac),
            _hb(ln_tau_spectra), _hb(T_edge_spectra), _hb(e_spectrum)))

    def ray_radiance_dev(self, abs_coef, layer_T, range_min, range_max, n, ray_first, seg_layer, seg_length, source_kind,
                         radiance, I_source=None, source_T=0.0, transmittance=None):
        """Radiance along ray paths through a column (lbl_ray_radiance_dev): ray r crosses the segments ray_first[r] ..
        ray_first[r + 1] - 1 (``seg_layer``, ``seg_length`` in cm) in the order the light travels, from cold space
        (``source_kind`` 0) or the surface source (1: ``I_source`` or B(nu, ``source_T``)); ``radiance`` and the optional
        ``transmittance`` receive len(source_kind) x n doubles, row-major."""
        self.check(self.lib.lbl_ray_radiance_dev(
            *self._ray_args("ray_radiance_dev", abs_coef, layer_T, range_min, range_max, n, ray_first, seg_layer, seg_length,
                            source_kind, I_source, source_T),
            _hb(radiance), _hb(transmittance)))

    def ray_radiance_surface_dev(self, abs_coef, layer_T, range_min, range_max, n, ray_first, seg_layer, seg_length,
                                 source_kind, radiance, emissivity, I_source=None, source_T=0.0, surface_down=None,
                                 surface_down_norm=0.0, transmittance=None):
        """Radiance along ray paths that may meet a reflecting surface (lbl_ray_radiance_surface_dev): ray_radiance_dev's
        arguments and results; a ``seg_layer`` of -1 (length 0) is where a ray is reflected specularly by the surface of
        ``emissivity`` (a Buffer of n points or one number in [0, 1]); rays that start at the surface also carry the diffuse
        reflection of ``surface_down`` (optional, n points: a downward flux formed with weights that add up to
        ``surface_down_norm``)."""
        self.check(self.lib.lbl_ray_radiance_surface_dev(
            *self._ray_args("ray_radiance_surface_dev", abs_coef, layer_T, range_min, range_max, n, ray_first, seg_layer,
                            seg_length, source_kind, I_source, source_T),
            *self._emissivity_args(emissivity), _hb(surface_down), float(surface_down_norm), _hb(radiance),
            _hb(transmittance)))

    def ray_radiance_linear_dev(self, abs_coef, seg_T, range_min, range_max, n, ray_first, seg_layer, seg_length,
                                source_kind, radiance, emissivity=1.0, I_source=None, source_T=0.0, surface_down=None,
                                surface_down_norm=0.0, transmittance=None):
        """Radiance along ray paths with a Planck source linear in optical depth (lbl_ray_radiance_linear_dev):
        ray_radiance_surface_dev's arguments and results with ``seg_T`` in place of the layers' temperatures - per segment
        (temperature where the light enters, where it leaves), as pairs or 2 numbers per segment; a marker's pair is
        ignored.  The default ``emissivity`` 1 is the black surface."""
        self.check(self.lib.lbl_ray_radiance_linear_dev(
            *self._ray_args("ray_radiance_linear_dev", abs_coef, seg_T, range_min, range_max, n, ray_first, seg_layer,
                            seg_length, source_kind, I_source, source_T, seg_T=True),
            *self._emissivity_args(emissivity), _hb(surface_down), float(surface_down_norm), _hb(radiance),
            _hb(transmittance)))

    def ray_jacobian_dev(self, abs_coef, layer_T, range_min, range_max, n, ray_first, seg_layer, seg_length, source_kind, jac,
                         I_source=None, source_T=0.0, term_abs_coef=(), term_layer=(), radiance=None):
        """Weighting functions of the radiance along ray paths (lbl_ray_jacobian_dev): the rays as ray_radiance_dev takes
        them; ``jac`` receives ray_jacobian_rows(...) rows of n doubles - per ray [dI/dT_source, dI/d ln tau and dI/dT of
        every crossed layer, the terms in crossed layers] - and ``radiance`` (optional) len(source_kind) x n doubles;
        ``term_layer`` gives each term's layer."""
        self.check(self.lib.lbl_ray_jacobian_dev(
            *self._ray_args("ray_jacobian_dev", abs_coef, layer_T, range_min, range_max, n, ray_first, seg_layer, seg_length,
                            source_kind, I_source, source_T, terms=(term_abs_coef, term_layer)),
            *self._term_args(term_abs_coef, term_layer), _hb(radiance), _hb(jac)))

    def ray_jacobian_surface_dev(self, abs_coef, layer_T, range_min, range_max, n, ray_first, seg_layer, seg_length,
                                 source_kind, jac, emissivity, I_source=None, source_T=0.0, term_abs_coef=(), term_layer=(),
                                 radiance=None):
        """Weighting functions of the radiance along ray paths that may meet a reflecting surface
        (lbl_ray_jacobian_surface_dev): ray_jacobian_dev's arguments with the markers and the ``emissivity`` of
        ray_radiance_surface_dev; ``jac`` receives ray_jacobian_rows(..., surface=True) rows of n doubles - per ray
        [dI/dT_source, dI/de, dI/d ln tau and dI/dT of every crossed layer, the terms in crossed layers]."""
        self.check(self.lib.lbl_ray_jacobian_surface_dev(
            *self._ray_args("ray_jacobian_surface_dev", abs_coef, layer_T, range_min, range_max, n, ray_first, seg_layer,
                            seg_length, source_kind, I_source, source_T, terms=(term_abs_coef, term_layer)),
            *self._emissivity_args(emissivity), *self._term_args(term_abs_coef, term_layer), _hb(radiance), _hb(jac)))

    def ray_jacobian_linear_dev(self, abs_coef, seg_T, range_min, range_max, n, ray_first, seg_layer, seg_length,
                                source_kind, jac, emissivity=1.0, I_source=None, source_T=0.0, term_abs_coef=(), term_layer=(),
                                radiance=None):
        """Weighting functions of the radiance along ray paths with a Planck source linear in optical depth
        (lbl_ray_jacobian_linear_dev): ray_jacobian_surface_dev's arguments with ``seg_T`` in place of the layers'
        temperatures, as ray_radiance_linear_dev takes them; ``jac`` receives ray_jacobian_rows(..., linear=True) rows of n
        doubles - per ray [dI/dT_source, dI/de, dI/d ln tau of every crossed layer, (dI/dTa, dI/dTb) of every segment that
        is no marker, the terms in crossed layers].  The default ``emissivity`` 1 is the black surface."""
        self.check(self.lib.lbl_ray_jacobian_linear_dev(
            *self._ray_args("ray_jacobian_linear_dev", abs_coef, seg_T, range_min, range_max, n, ray_first, seg_layer,
                            seg_length, source_kind, I_source, source_T, seg_T=True, terms=(term_abs_coef, term_layer)),
            *self._emissivity_args(emissivity), *self._term_args(term_abs_coef, term_layer), _hb(radiance), _hb(jac)))

    def ils_convolve_dev(self, range_min, range_max, n, rows, position, width, first, count, shape, out, table=None,
                         table_half=0.0):
        """Rows on the base grid convolved onto instrument channels (lbl_ils_convolve_dev): ``rows`` is a list of (Buffer,
        offset in doubles); ``position``, ``width``, ``first``, ``count`` hold one value per channel; ``shape`` is an
        ILS_SHAPES value, ``table`` / ``table_half`` the tabulated line shape of "table"; ``out`` receives len(rows) x
        channels doubles, row-major."""
        position, first, count = _as_f64(position), _as_i64(first), _as_i64(count)
        width = _as_f64(width) if width is not None else None
        table = _as_f64(table) if table is not None else None
        self.check(self.lib.lbl_ils_convolve_dev(
            self.h, float(range_min), float(range_max), int(n), len(rows), _arr(_P, [_hb(b) for b, _ in rows]),
            _arr(C.c_int64, [int(o) for _, o in rows]), len(position),
            position.ctypes.data_as(_D), width.ctypes.data_as(_D) if width is not None else None,
            first.ctypes.data_as(C.POINTER(C.c_int64)), count.ctypes.data_as(C.POINTER(C.c_int64)), int(shape),
            len(table) if table is not None else 0, float(table_half),
            table.ctypes.data_as(_D) if table is not None else None, _hb(out)))

    @staticmethod
    def _i64p(a):
        return a.ctypes.data_as(C.POINTER(C.c_int64))

    def rank_order_workspace(self, n_rows, n, band_count) -> int:
        """Doubles of work space lbl_rank_order_dev needs for ``n_rows`` rows of ``n`` points and these band lengths."""
        count = _as_i64(band_count)
        v = C.c_int64()
        self.check(self.lib.lbl_rank_order_workspace(int(n_rows), int(n), len(count), self._i64p(count), C.byref(v)))
        return int(v.value)

    def rank_order_dev(self, n, rows, band_first, band_count, order, sorted=None, work=None):
        """The stable ascending order of every band of every row (lbl_rank_order_dev): ``rows`` is a list of (Buffer, offset in
        doubles) of ``n`` points each; ``order`` receives len(rows) x sum(band_count) grid indices as doubles, band after band
        per row, ``sorted`` (optional) the rows' values in that order; ``work`` holds rank_order_workspace(...) doubles (may
        be None when that is 0)."""
        first, count = _as_i64(band_first), _as_i64(band_count)
        if len(first) != len(count):
            raise ValueError("rank_order_dev: one first per band")
        self.check(self.lib.lbl_rank_order_dev(
            self.h, int(n), len(rows), _arr(_P, [_hb(b) for b, _ in rows]), _arr(C.c_int64, [int(o) for _, o in rows]),
            len(count), self._i64p(first), self._i64p(count), _hb(work), _hb(order), _hb(sorted)))

    def ranked_means_workspace(self, n_rows, band_count, edges) -> int:
        """Doubles of work space lbl_ranked_means_dev needs; ``edges``: one array of rank edges per band."""
        count = _as_i64(band_count)
        if len(edges) != len(count):
            raise ValueError("ranked_means_workspace: one edge array per band")
        flat = _as_i64(np.concatenate([_as_i64(e) for e in edges])) if len(edges) else _as_i64([])
        v = C.c_int64()
        self.check(self.lib.lbl_ranked_means_workspace(
            int(n_rows), len(count), self._i64p(count), _arr(C.c_int32, [len(e) - 1 for e in edges]), self._i64p(flat),
            C.byref(v)))
        return int(v.value)

    def ranked_means_dev(self, n, rows, orders, band_first, band_count, edges, work, mean, lower=None, mean_offset=0,
                         lower_offset=0):
        """Means of every row over intervals of the rank (lbl_ranked_means_dev): ``rows`` and ``orders`` are lists of (Buffer,
        offset), row r is averaged by the order at orders[r] (an output row of rank_order_dev); ``edges``: per band G_b + 1
        rank edges 0 .. count_b.  ``mean`` receives, from ``mean_offset``, len(rows) x sum(G_b) values, ``lower`` (optional,
        from ``lower_offset``) len(rows) x sum(G_b + 1) order statistics at the edges; ``work`` holds
        ranked_means_workspace(...) doubles."""
        first, count = _as_i64(band_first), _as_i64(band_count)
        if len(orders) != len(rows) or len(first) != len(count) or len(edges) != len(count):
            raise ValueError("ranked_means_dev: one order per row, one first and one edge array per band")
        flat = _as_i64(np.concatenate([_as_i64(e) for e in edges])) if len(edges) else _as_i64([])
        self.check(self.lib.lbl_ranked_means_dev(
            self.h, int(n), len(rows), _arr(_P, [_hb(b) for b, _ in rows]), _arr(C.c_int64, [int(o) for _, o in rows]),
            _arr(_P, [_hb(b) for b, _ in orders]), _arr(C.c_int64, [int(o) for _, o in orders]),
            len(count), self._i64p(first), self._i64p(count), _arr(C.c_int32, [len(e) - 1 for e in edges]), self._i64p(flat),
            _hb(work), _hb(mean), int(mean_offset), _hb(lower), int(lower_offset)))

    def gather_compact_dev(self, gathered, slot, bounds, out):
        """padded all-gather result (slot r = rank r's shard) -> grid order (lbl_gather_compact_dev)."""
        w = len(bounds)
        F = (C.c_int64 * w)(*[int(f) for f, _ in bounds])
        K = (C.c_int64 * w)(*[int(c) for _, c in bounds])
        self.check(self.lib.lbl_gather_compact_dev(self.h, gathered.h, w, int(slot), F, K, out.h))

    def column_step_dev(self, layers, range_min, range_max, n, I_out, I_in=None, surface_T=0.0, first=0, count=0):
        """layers: bottom to top, each dict(xsec=[Buffer], iso_mol=[int], conc=[float], P, T, depth,
        trans=Buffer|None, abs_coef=Buffer|None)."""
        nl = len(layers)
        xs = [b for L in layers for b in L["xsec"]]
        im = [int(m) for L in layers for m in L["iso_mol"]]
        cc = [float(c) for L in layers for c in L["conc"]]
        n_iso = _arr(C.c_int32, [len(L["xsec"]) for L in layers])
        n_mol = _arr(C.c_int32, [len(L["conc"]) for L in layers])
        self.check(self.lib.lbl_column_step_dev(
            self.h, nl, n_iso, _arr(_P, [b.h for b in xs]), _arr(C.c_int32, im), n_mol, _arr(C.c_double, cc),
            _arr(C.c_double, [float(L["P"]) for L in layers]), _arr(C.c_double, [float(L["T"]) for L in layers]),
            _arr(C.c_double, [float(L["depth"]) for L in layers]), float(range_min), float(range_max), int(n),
            int(first), int(count), _hb(I_in), float(surface_T),
            _arr(_P, [_hb(L.get("abs_coef")) for L in layers]), _arr(_P, [_hb(L.get("trans")) for L in layers]), I_out.h))

    def column_sweep_dev(self, trans, layer_T, range_min, range_max, n, I_out, I_in=None, surface_T=0.0,
                         first=0, count=0):
        self.check(self.lib.lbl_column_sweep_dev(self.h, len(trans), _arr(_P, [b.h for b in trans]),
                                                 _arr(C.c_double, [float(t) for t in layer_T]), float(range_min),
                                                 float(range_max), int(n), int(first), int(count), _hb(I_in),
                                                 float(surface_T), I_out.h))

    def sum_dev(self, bufs, n, out):
        """out = zeros + bufs[0] + bufs[1] + ... in list order (pyradClasses.py:566-571, 684-689).  A list longer than the
        library takes at once is chained with the partial sum first: 0 + partial is exact, the order of additions the same."""
        cap = limit("arrays_per_sum")
        bufs = list(bufs)
        first = True
        while first or bufs:
            take = bufs[:cap] if first else [out] + bufs[:cap - 1]
            bufs = bufs[cap:] if first else bufs[cap - 1:]
            B = (_P * max(len(take), 1))(*[b.h for b in take])
            self.check(self.lib.lbl_sum_dev(self.h, len(take), B, int(n), out.h))
            first = False

    def optical_dev(self, trans, n, kind, out):
        self.check(self.lib.lbl_optical_dev(self.h, trans.h, int(n), int(kind), out.h))

    def planck_dev(self, range_min, range_max, n, T, out):
        self.check(self.lib.lbl_planck_dev(self.h, float(range_min), float(range_max), int(n), float(T), out.h))

    def band_integral(self, spectrum, n, unit_angle, res) -> float:
        r = C.c_double()
        self.check(self.lib.lbl_band_integral(self.h, spectrum.h, int(n), float(unit_angle), float(res), C.byref(r)))
        return r.value

    def line_survey_dev(self, lines, grid, out):
        self.check(self.lib.lbl_line_survey_dev(self.h, lines.h, C.byref(grid), out.h))


class Column:
    """lbl_column: the argument blocks of a column's merged accumulate jobs and of its fold, kept on the C side between
    calls.  ``layers``: list of dict(lines=[Lines], iso=[IsoParams], grid=Grid, iso_mol=[int], conc=[float], depth=float,
    abs_coef=Buffer).  The handle owns nothing on the device; the Python object keeps the line lists and buffers it was
    given alive."""

    def __init__(self, ctx: "Context", layers):
        self.ctx = ctx
        self.n_layers = len(layers)
        ls = [l for L in layers for l in L["lines"]]
        self._keep = [(list(L["lines"]), L["abs_coef"]) for L in layers]
        h = _P()
        ctx.check(ctx.lib.lbl_column_create(
            ctx.h, self.n_layers, _arr(C.c_int32, [len(L["lines"]) for L in layers]), _arr(_P, [l.h for l in ls]),
            _arr(IsoParams, [i for L in layers for i in L["iso"]]), _arr(Grid, [L["grid"] for L in layers]),
            _arr(C.c_int32, [int(m) for L in layers for m in L["iso_mol"]]), _arr(C.c_int32, [len(L["conc"]) for L in layers]),
            _arr(C.c_double, [float(c) for L in layers for c in L["conc"]]), _arr(C.c_double, [float(L["depth"]) for L in layers]),
            _arr(_P, [L["abs_coef"].h for L in layers]), C.byref(h)))
        self.h = h
        self._due = (C.c_uint8 * self.n_layers)()
        ctx._children.append(self)

    def set_layer(self, l, lines, iso, grid, conc, depth, abs_coef):
        self.ctx.check(self.ctx.lib.lbl_column_set_layer(self.h, int(l), _arr(_P, [x.h for x in lines]), _arr(IsoParams, list(iso)),
                                                         C.byref(grid), _arr(C.c_double, [float(c) for c in conc]), float(depth),
                                                         abs_coef.h))
        self._keep[l] = (list(lines), abs_coef)

    def transmission(self, due, I_out, host=None, I_in=None, surface_T=0.0, pieces=1):
        """Enqueue: the merged accumulate jobs of the layers with due[l] true (None: all), the fold in ``pieces`` pieces, each
        piece's part of I_out on its way into ``host`` (Context.host_array); Context.download_wait() before reading it."""
        flags = None
        if due is not None:
            flags = self._due
            for l, d in enumerate(due):
                flags[l] = 1 if d else 0
        hp = None
        if host is not None:
            if not (host.dtype == np.float64 and host.flags["C_CONTIGUOUS"]):
                raise ValueError("the host array must be contiguous float64")
            hp = _ptr(host)
        self.ctx.check(self.ctx.lib.lbl_column_transmission(self.h, flags, _hb(I_in), float(surface_T),
                                                            I_out.h, hp, int(pieces)))

    def free(self):
        if self.h:
            self.ctx.check(self.ctx.lib.lbl_column_destroy(self.h))
            self.h = None
            self._keep = []
            if self in self.ctx._children:
                self.ctx._children.remove(self)


class Buffer:
    """Device float64 array (lbl_buffer)."""

    def __init__(self, ctx: Context, n: int):
        self.ctx = ctx
        self.n = int(n)
        h = _P()
        ctx.check(ctx.lib.lbl_buffer_create(ctx.h, self.n, C.byref(h)))
        self.h = h
        ctx._children.append(self)

    def stage_from_dev(self, src: "Buffer", src_offset: int, n: int, dst_offset: int = 0):
        """self[dst_offset : dst_offset + n] = src[src_offset : src_offset + n], device to device, async on this
        buffer's context stream (lbl_gather_stage_dev: staging shards into an all-gather batch buffer)."""
        self.ctx.check(self.ctx.lib.lbl_gather_stage_dev(self.h, int(dst_offset), src.h, int(src_offset), int(n)))
        return self

    def upload(self, data, offset: int = 0):
        a = _as_f64(data)
        self.ctx.check(self.ctx.lib.lbl_buffer_upload(self.h, _ptr(a), a.size, int(offset)))
        return self

    def download(self, n: int | None = None, offset: int = 0, pinned: bool = False) -> np.ndarray:
        """Host copy of n elements.  ``pinned``: into page-locked memory of the context's pool (DMA
        rate; the array must not outlive the context)."""
        n = self.n - offset if n is None else int(n)
        out = self.ctx.host_array(n) if pinned else np.empty(n, dtype=np.float64)
        self.ctx.check(self.ctx.lib.lbl_buffer_download(self.h, _ptr(out), n, int(offset)))
        return out

    def download_async(self, out: np.ndarray, n: int, offset: int = 0, out_offset: int = 0):
        """out[out_offset : out_offset + n] = self[offset : offset + n] without waiting (lbl_buffer_download_async: behind
        the work enqueued so far, beside what is enqueued next); ``out`` from Context.host_array; Context.download_wait()
        before reading it."""
        if not (out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and 0 <= out_offset and out_offset + int(n) <= out.size):
            raise ValueError("download_async needs a contiguous float64 array that holds the range")
        self.ctx.check(self.ctx.lib.lbl_buffer_download_async(self.h, _ptr(out[out_offset:]), int(n), int(offset)))
        return out

    def fill(self, value: float):
        self.ctx.check(self.ctx.lib.lbl_buffer_fill(self.h, float(value)))
        return self

    def devptr(self) -> int:
        p = _P()
        self.ctx.check(self.ctx.lib.lbl_buffer_devptr(self.h, C.byref(p)))
        return p.value or 0

    def free(self):
        if self.h:
            self.ctx.check(self.ctx.lib.lbl_buffer_destroy(self.h))
            self.h = None
            if self in self.ctx._children:
                self.ctx._children.remove(self)

    def __del__(self):
        try:
            if self.ctx.h:
                self.free()
        except Exception:
            pass


class Graph:
    """A captured launch sequence (lbl_graph)."""

    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h
        ctx._children.insert(0, self)

    def launch(self):
        self.ctx.check(self.ctx.lib.lbl_graph_launch(self.h))

    def free(self):
        if self.h:
            self.ctx.check(self.ctx.lib.lbl_graph_destroy(self.h))
            self.h = None
            if self in self.ctx._children:
                self.ctx._children.remove(self)


class Lines:
    """Device-resident HITRAN line list (lbl_lines).  Sorts by nu on the host if needed."""
    ORDER = ("nu", "sw", "elower", "gamma_air", "gamma_self", "n_air", "delta_air")

    def __init__(self, ctx: Context, lines: dict):
        self.ctx = ctx
        nu = _as_f64(lines["nu"])
        if nu.size > 1 and np.any(np.diff(nu) < 0):
            order = np.argsort(nu, kind="stable")
            lines = {k: np.asarray(lines[k])[order] for k in self.ORDER}
        arrs = [_as_f64(lines[k]) for k in self.ORDER]
        self.n = int(arrs[0].size)
        self._parent = None
        h = _P()
        ctx.check(ctx.lib.lbl_lines_create(ctx.h, *[_ptr(a) for a in arrs], self.n, C.byref(h)))
        self.h = h
        ctx._children.append(self)

    def has_views(self) -> bool:
        return any(isinstance(c, Lines) and c._parent is self and c.h for c in self.ctx._children)

    def view(self, first: int, count: int) -> "Lines":
        """``count`` consecutive lines from line ``first`` on (sorted order), sharing this list's device arrays
        (lbl_lines_view).  Free the views before the list."""
        v = Lines.__new__(Lines)
        v.ctx, v.n = self.ctx, int(count)
        v._parent = self                       # the view keeps its list alive (a collected list could not free itself)
        h = _P()
        self.ctx.check(self.ctx.lib.lbl_lines_view(self.h, int(first), int(count), C.byref(h)))
        v.h = h
        self.ctx._children.append(v)
        return v

    def free(self):
        if self.h:
            self.ctx.check(self.ctx.lib.lbl_lines_destroy(self.h))
            self.h = None
            self._parent = None
            if self in self.ctx._children:
                self.ctx._children.remove(self)

    def __del__(self):
        try:
            if self.ctx.h:
                self.free()
        except Exception:
            pass


class Comm:
    """RCCL communicator over the context's device (lbl_comm), one rank per process."""

    def __init__(self, ctx: Context, unique_id: bytes, world_size: int, rank: int):
        self.ctx = ctx
        self.world_size, self.rank = int(world_size), int(rank)
        h = _P()
        buf = C.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        ctx.check(ctx.lib.lbl_comm_create(ctx.h, buf, self.world_size, self.rank, C.byref(h)))
        self.h = h
        ctx._children.insert(0, self)

    @staticmethod
    def unique_id() -> bytes:
        lib = load()
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        rc = lib.lbl_comm_unique_id(buf)
        if rc != LBL_OK:
            raise LblError(rc, (lib.lbl_last_error(None) or b"").decode())
        return buf.raw

    def allgather_dev(self, send: Buffer, send_offset: int, count: int, recv: Buffer, overlap_slot=None):
        """In-stream all-gather, or (overlap_slot 0..6) one the context stream does not wait for.  "The
        context" is the one that owns send and recv (any context of the communicator's device): errors are
        reported there."""
        owner = send.ctx
        if overlap_slot is None:
            owner.check(owner.lib.lbl_allgather_dev(self.h, send.h, int(send_offset), int(count), recv.h))
        else:
            owner.check(owner.lib.lbl_allgather_overlap_dev(self.h, send.h, int(send_offset), int(count), recv.h,
                                                            int(overlap_slot)))

    def fence_dev(self, slot: int = -1):
        """Context stream waits (no host sync) for the collective issued with ``slot`` (-1: all)."""
        self.ctx.check(self.ctx.lib.lbl_comm_fence_dev(self.h, int(slot)))

    def free(self):
        if self.h:
            self.ctx.check(self.ctx.lib.lbl_comm_destroy(self.h))
            self.h = None
            if self in self.ctx._children:
                self.ctx._children.remove(self)


def device_count() -> int:
    lib = load()
    n = C.c_int()
    rc = lib.lbl_device_count(C.byref(n))
    return n.value if rc == LBL_OK else 0
