"""rav1e_amd -- MI355X (gfx950) encode hot path for rav1e, host side.

Python mirror of the reference's dispatch interface for the hot path
(geobacter-rs/rav1e): ``CpuFeatureLevel`` with a ``HIP`` level, the
``get_sad`` / ``get_satd`` / ``put_8tap`` / ``prep_8tap`` / ``mc_avg`` /
``forward_transform`` / ``inverse_transform_add`` / ``sse_wxh`` /
``cdef_dist_wxh`` entry points, plus the batched forms that are the
production path.  Everything runs through the C ABI of
``rav1e_amd/lib/librav1e_hip.so`` (``include/rav1e_hip.h``); there is no
CPU fallback: without the library this module raises on import of any
entry point, and the HIP level requires a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
import typing

import numpy as np

_ROOT = os.path.dirname(os.path.abspath(__file__))
# RAV1E_HIP_LIB: another in-tree build of the same library (A/B benchmarks)
LIB_PATH = os.environ.get("RAV1E_HIP_LIB") or os.path.join(_ROOT, "lib", "librav1e_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_ROOT), "include", "rav1e_hip.h")

RV_OK, RV_EINVAL, RV_EHIP, RV_ENOTSUP = 0, -1, -2, -3


class Rav1eHipError(RuntimeError):
    pass


# ---- C structs (include/rav1e_hip.h) -----------------------------------
class RvPlane(C.Structure):
    _fields_ = [("data", C.c_void_p), ("stride", C.c_int32),
                ("alloc_height", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("xorigin", C.c_int32),
                ("yorigin", C.c_int32), ("xdec", C.c_int32),
                ("ydec", C.c_int32), ("hbd", C.c_int32),
                ("bit_depth", C.c_int32)]


class RvMv(C.Structure):
    _fields_ = [("row", C.c_int16), ("col", C.c_int16)]


class RvFsResult(C.Structure):
    _fields_ = [("best_mv", RvMv), ("reserved", C.c_uint32), ("cost", C.c_uint64)]


# job layouts as numpy dtypes (arrays of these go to the device verbatim)
DIST_JOB = np.dtype([("org_x", "<i4"), ("org_y", "<i4"), ("ref_x", "<i4"), ("ref_y", "<i4")])
INTRA_JOB = np.dtype([("x", "<i4"), ("y", "<i4"), ("mode", "<i4"), ("variant", "<i4")])
CFL_JOB = np.dtype([("x", "<i4"), ("y", "<i4"), ("variant", "<i4"), ("reserved", "<i4")])
MC_JOB = np.dtype([("src_x", "<i4"), ("src_y", "<i4"), ("dst_x", "<i4"), ("dst_y", "<i4"),
                   ("col_frac", "<i4"), ("row_frac", "<i4")])
MOTION_VECTOR = np.dtype([("row", "<i2"), ("col", "<i2")])  # rv_mv / MotionVector
TX_JOB = np.dtype([("src_x", "<i4"), ("src_y", "<i4"), ("pred_x", "<i4"), ("pred_y", "<i4")])
FS_JOB = np.dtype([("po_x", "<i4"), ("po_y", "<i4"), ("x_lo", "<i4"), ("x_hi", "<i4"),
                   ("y_lo", "<i4"), ("y_hi", "<i4"), ("pmv0_row", "<i2"), ("pmv0_col", "<i2"),
                   ("pmv1_row", "<i2"), ("pmv1_col", "<i2"), ("lambda_", "<u4"),
                   ("reserved", "<i4")])
DS_JOB = np.dtype([("po_x", "<i4"), ("po_y", "<i4"), ("mvx_min", "<i4"), ("mvx_max", "<i4"),
                   ("mvy_min", "<i4"), ("mvy_max", "<i4"), ("pmv0_row", "<i2"),
                   ("pmv0_col", "<i2"), ("pmv1_row", "<i2"), ("pmv1_col", "<i2"),
                   ("lambda_", "<u4"), ("n_pred", "<i4"), ("pred", "<i2", (17, 2))])
FS_RESULT = np.dtype([("mv_row", "<i2"), ("mv_col", "<i2"), ("reserved", "<u4"),
                      ("cost", "<u8")])
REPLAY_CFG_FIELDS = ["width", "height", "xdec", "ydec", "bit_depth", "tile_x0", "tile_y0",
                     "tile_w", "tile_h", "n_refs", "tile_w_sb", "tile_h_sb", "n_inputs", "flags"]


class RvReplayCfg(C.Structure):
    _fields_ = [(f, C.c_int32) for f in REPLAY_CFG_FIELDS]


class RvReplayLevelParams(C.Structure):
    _fields_ = [("base_q_idx", C.c_int32), ("dc_delta_q", C.c_int32 * 3),
                ("ac_delta_q", C.c_int32 * 3), ("cdef_strengths", C.c_int32), ("lambda_", C.c_double),
                ("me_lambda", C.c_double), ("dist_scale", C.c_double * 3)]

    @classmethod
    def from_dict(cls, d):
        p = cls()
        p.base_q_idx = d["base_q_idx"]
        for i in range(3):
            p.dc_delta_q[i], p.ac_delta_q[i] = d["dc_delta_q"][i], d["ac_delta_q"][i]
            p.dist_scale[i] = d["dist_scale"][i]
        p.lambda_, p.me_lambda = d["lambda"], d["me_lambda"]
        p.cdef_strengths = d.get("cdef_y", 0) | d.get("cdef_uv", 0) << 8
        return p


class RvReplayFrameInfo(C.Structure):
    _fields_ = [("display", C.c_int32), ("me_range_scale", C.c_int32), ("level", C.c_int32),
                ("is_key", C.c_int32), ("ref_display", C.c_int32 * 2), ("compound", C.c_int32)]


# ---- reference enums ----------------------------------------------------
class CpuFeatureLevel(enum.IntEnum):
    """src/cpu_features/x86.rs:13-19 plus the HIP level."""
    NATIVE = 0
    SSE2 = 1
    SSSE3 = 2
    AVX2 = 3
    HIP = 4

    @staticmethod
    def default() -> "CpuFeatureLevel":
        """CpuFeatureLevel::default() with RAV1E_CPU_TARGET (x86.rs:34-61)."""
        return CpuFeatureLevel(lib().rv_cpu_feature_level_default())

    def as_index(self) -> int:
        return int(self)


class BlockSize(enum.IntEnum):
    """src/partition.rs:116-140 (order = table index)."""
    BLOCK_4X4 = 0
    BLOCK_4X8 = 1
    BLOCK_8X4 = 2
    BLOCK_8X8 = 3
    BLOCK_8X16 = 4
    BLOCK_16X8 = 5
    BLOCK_16X16 = 6
    BLOCK_16X32 = 7
    BLOCK_32X16 = 8
    BLOCK_32X32 = 9
    BLOCK_32X64 = 10
    BLOCK_64X32 = 11
    BLOCK_64X64 = 12
    BLOCK_64X128 = 13
    BLOCK_128X64 = 14
    BLOCK_128X128 = 15
    BLOCK_4X16 = 16
    BLOCK_16X4 = 17
    BLOCK_8X32 = 18
    BLOCK_32X8 = 19
    BLOCK_16X64 = 20
    BLOCK_64X16 = 21

    def width(self) -> int:
        return int(self.name.split("_")[1].split("X")[0])

    def height(self) -> int:
        return int(self.name.split("X")[-1])

    @staticmethod
    def from_width_and_height(w: int, h: int) -> "BlockSize":
        return BlockSize[f"BLOCK_{w}X{h}"]


class TxSize(enum.IntEnum):
    """src/transform/mod.rs:225-247."""
    TX_4X4 = 0
    TX_8X8 = 1
    TX_16X16 = 2
    TX_32X32 = 3
    TX_64X64 = 4
    TX_4X8 = 5
    TX_8X4 = 6
    TX_8X16 = 7
    TX_16X8 = 8
    TX_16X32 = 9
    TX_32X16 = 10
    TX_32X64 = 11
    TX_64X32 = 12
    TX_4X16 = 13
    TX_16X4 = 14
    TX_8X32 = 15
    TX_32X8 = 16
    TX_16X64 = 17
    TX_64X16 = 18

    def width(self) -> int:
        return int(self.name.split("_")[1].split("X")[0])

    def height(self) -> int:
        return int(self.name.split("X")[-1])


class TxType(enum.IntEnum):
    """src/transform/mod.rs:123-140."""
    DCT_DCT = 0
    ADST_DCT = 1
    DCT_ADST = 2
    ADST_ADST = 3
    FLIPADST_DCT = 4
    DCT_FLIPADST = 5
    FLIPADST_FLIPADST = 6
    ADST_FLIPADST = 7
    FLIPADST_ADST = 8
    IDTX = 9
    V_DCT = 10
    H_DCT = 11
    V_ADST = 12
    H_ADST = 13
    V_FLIPADST = 14
    H_FLIPADST = 15


class FilterMode(enum.IntEnum):
    """src/mc.rs:58-66."""
    REGULAR = 0
    SMOOTH = 1
    SHARP = 2
    BILINEAR = 3


# ---- library loading ------------------------------------------------------
_lib = None


class RvEcModeParams(C.Structure):
    """rv_ec_mode_params (include/rav1e_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("frame_type", "reference_mode", "force_integer_mv",
                                         "allow_high_precision_mv", "seg_enabled",
                                         "last_active_segid")]


class RvMvrefGeom(C.Structure):
    """rv_mvref_geom (include/rav1e_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("n_tiles", "grid_w", "grid_h", "frame_cols",
                                         "frame_rows")] + [("sign_bias", C.c_uint32)]


class RvInterRefSets(C.Structure):
    """rv_inter_ref_sets (include/rav1e_hip.h)."""
    _fields_ = [("n_single", C.c_int32), ("ref", C.c_int32 * 7), ("slot", C.c_int32 * 7),
                ("fwd", C.c_int32), ("bwd", C.c_int32), ("compound", C.c_int32)]

    @property
    def n_sets(self):
        return self.n_single + self.compound


class RvInterMcParams(C.Structure):
    """rv_inter_mc_params (include/rav1e_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("bsize", "filter_mode", "luma_only", "bit_depth")]


class RvMeParams(C.Structure):
    """rv_me_params (include/rav1e_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("bsize", "bit_depth", "use_satd", "allow_hp", "w_in_b",
                                         "h_in_b")] + [("lambda_", C.c_uint32),
                                                       ("reserved", C.c_int32)]


def _declare(L):
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    P = C.POINTER(RvPlane)
    sig = {
        "rv_cpu_feature_level_default": (i32, []),
        "rv_cpu_feature_level_index": (i32, [i32]),
        "rv_device_count": (i32, []),
        "rv_set_device": (i32, [i32]),
        "rv_last_error": (C.c_char_p, []),
        "rv_version": (C.c_char_p, []),
        "rv_malloc": (vp, [sz]),
        "rv_free": (None, [vp]),
        "rv_host_alloc": (vp, [sz]),
        "rv_host_free": (None, [vp]),
        "rv_memcpy_h2d": (i32, [vp, vp, sz, vp]),
        "rv_memcpy_d2h": (i32, [vp, vp, sz, vp]),
        "rv_memcpy_d2d": (i32, [vp, vp, sz, vp]),
        "rv_memset": (i32, [vp, i32, sz, vp]),
        "rv_stream_create": (vp, []),
        "rv_stream_create_priority": (vp, [i32]),
        "rv_stream_destroy": (i32, [vp]),
        "rv_stream_sync": (i32, [vp]),
        "rv_device_sync": (i32, []),
        "rv_trace_marker": (i32, [vp]),
        "rv_event_create": (vp, []),
        "rv_event_destroy": (i32, [vp]),
        "rv_event_record": (i32, [vp, vp]),
        "rv_event_sync": (i32, [vp]),
        "rv_stream_wait_event": (i32, [vp, vp]),
        "rv_event_elapsed_ms": (C.c_float, [vp, vp]),
        "rv_plane_geometry": (sz, [P, i32, i32, i32, i32, i32, i32, i32]),
        "rv_plane_pad": (i32, [P, vp]),
        "rv_plane_downsample": (i32, [P, P, vp]),
        "rv_sad_batch": (i32, [P, P, vp, i32, i32, i32, vp, vp]),
        "rv_satd_batch": (i32, [P, P, vp, i32, i32, i32, vp, vp]),
        "rv_sse_batch": (i32, [P, P, vp, i32, i32, i32, vp, vp]),
        "rv_lookahead_intra_costs": (i32, [P, i32, vp, vp]),
        "rv_propagate_importances_scratch": (sz, [i32, i32]),
        "rv_propagate_importances": (i32, [P, P, vp, vp, vp, i32, vp, vp, sz, vp]),
        "rv_cdef_moments_batch": (i32, [P, P, vp, i32, i32, i32, vp, vp]),
        "rv_put_8tap_batch": (i32, [P, P, vp, i32, i32, i32, i32, i32, i32, vp]),
        "rv_predict_intra_batch": (i32, [P, vp, vp, i32, i32, i32, vp]),
        "rv_intra_edges_batch": (i32, [P, vp, i32, vp, i32, i32, i32, i32, i32, vp, vp]),
        "rv_intra_screen_batch": (i32, [P, P, vp, i32, vp, i32, i32, i32, vp, i32, i32, vp, vp, vp,
                                        vp]),
        "rv_tx_blocks_layout": (i32, [i32, i32, i32, i32, i32, vp]),
        "rv_tx_blocks_batch": (i32, [vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]),
        "rv_cfl_luma_ac_batch": (i32, [P, vp, i32, i32, i32, i32, vp, vp]),
        "rv_predict_cfl_batch": (i32, [P, vp, vp, vp, vp, i32, i32, i32, vp]),
        "rv_cfl_alpha_search_batch": (i32, [P, P, vp, i32, i32, i32, vp, vp, vp]),
        "rv_frame_delta_batch": (i32, [P, i32, i32, vp, i32, vp, vp]),
        "rv_deblock_plane": (i32, [P, i32, i32, i32, vp, vp, i32, vp, i32, vp]),
        "rv_deblock_fast_level": (i32, [i32, i32, i32]),
        "rv_deblock_sse": (i32, [P, P, i32, i32, vp, vp, i32, vp, vp, i32, vp]),
        "rv_deblock_frame": (i32, [P, i32, i32, vp, vp, i32, vp, i32, vp]),
        "rv_cdef_find_dirs": (i32, [P, i32, i32, vp, i32, vp, vp, i32, vp]),
        "rv_lrf_stripe_filter": (i32, [P, P] + [i32] * 10 + [vp, vp]),
        "rv_y4m_parse_header": (i32, [C.c_char_p, vp]),
        "rv_y4m_open": (vp, [C.c_char_p]),
        "rv_y4m_get_info": (i32, [vp, vp]),
        "rv_y4m_frame_bytes": (sz, [vp]),
        "rv_y4m_read_frame": (i32, [vp, vp]),
        "rv_y4m_close": (None, [vp]),
        "rv_ivf_create": (vp, [C.c_char_p, i32, i32, i32, i32]),
        "rv_ivf_write_frame": (i32, [vp, C.c_uint64, vp, sz]),
        "rv_ivf_close": (i32, [vp]),
        "rv_cdef_filter_plane": (i32, [P, P, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, i32, i32,
                                       vp]),
        "rv_prep_8tap_batch": (i32, [vp, P, vp, i32, i32, i32, i32, i32, i32, vp]),
        "rv_mc_avg_batch": (i32, [P, vp, vp, vp, i32, i32, i32, i32, vp]),
        "rv_mc_dist_batch": (i32, [P, P, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
        "rv_fwd_txfm_batch": (i32, [vp, vp, i32, i32, i32, i32, vp]),
        "rv_diff_fwd_txfm_batch": (i32, [P, P, vp, i32, i32, i32, i32, vp, vp]),
        "rv_inv_txfm_add_batch": (i32, [vp, P, vp, i32, i32, i32, i32, vp]),
        "rv_quantize_batch": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp,
                                    vp]),
        "rv_dequantize_batch": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp]),
        "rv_estimate_rate_batch": (i32, [vp, i32, i32, i32, vp, vp]),
        "rv_full_search_batch": (i32, [P, P, vp, i32, i32, i32, i32, i32, vp, vp]),
        "rv_full_search_sea_batch": (i32, [P, P, vp, vp, i32, i32, vp, vp]),
        "rv_plane_box_sums": (i32, [P, vp, vp]),
        "rv_replay_create": (vp, [C.POINTER(RvReplayCfg), vp]),
        "rv_replay_create_twin": (vp, [vp, vp]),
        "rv_replay_seek": (i32, [vp, C.c_long]),
        "rv_replay_stream": (vp, [vp]),
        "rv_replay_destroy": (None, [vp]),
        "rv_q_lookup": (i32, [i32, i32, i32]),
        "rv_replay_synth_inputs": (i32, [vp, i32]),
        "rv_replay_set_level_params": (i32, [vp, i32, C.POINTER(RvReplayLevelParams)]),
        "rv_replay_set_input": (i32, [vp, i32, vp]),
        "rv_replay_get_input": (i32, [vp, i32, vp]),
        "rv_replay_get_recon": (i32, [vp, i32, vp]),
        "rv_replay_set_importances": (i32, [vp, vp, i32]),
        "rv_replay_set_imp_window": (i32, [vp, i32, C.c_long]),
        "rv_replay_set_inputs_ready": (i32, [vp, C.c_long]),
        "rv_replay_get_importances": (i32, [vp, vp, i32]),
        "rv_replay_frame": (i32, [vp, C.POINTER(RvReplayFrameInfo)]),
        "rv_replay_set_groups": (i32, [vp, i32, vp, i32, vp]),
        "rv_replay_exchange_buffers": (i32, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_size_t)]),
        "rv_replay_import": (i32, [vp]),
        "rv_comm_unique_id": (i32, [vp, i32]),
        "rv_comm_create": (vp, [vp, i32, i32]),
        "rv_comm_destroy": (None, [vp]),
        "rv_replay_results": (i32, [vp, vp, i32]),
        "rv_replay_entropy_stats": (i32, [vp, vp, i32]),
        "rv_replay_stage_times": (i32, [vp, vp, i32]),
        "rv_replay_stage_times_sum": (i32, [vp, i32, vp, i32]),
        "rv_replay_counters": (i32, [vp, vp, i32]),
        "rv_replay_dpb_slots": (i32, []),
        "rv_replay_set_kernel_probe": (i32, [vp, i32]),
        "rv_replay_kernel_probe": (i32, [vp, vp, i32]),
        "rv_round_ring_slots": (i32, [C.c_uint32, vp, i32]),
        "rv_replay_lrf_units": (i32, [vp, i32, vp, i32]),
        "rv_replay_la_refs": (i32, [C.c_long, i32, vp]),
        "rv_la_hub_create": (vp, [i32]),
        "rv_la_hub_destroy": (None, [vp]),
        "rv_replay_set_la_exchange": (i32, [vp, vp, vp]),
        "rv_replay_set_timing": (i32, [vp, i32, i32]),
        "rv_diamond_search_batch": (i32, [P, P, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
        "rv_telescopic_subpel_batch": (i32, [P, P, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
        "rv_tx_dist_batch": (i32, [vp, i32, vp, i32, i32, vp, vp]),
        "rav1e_fwd_txfm_hip": (i32, [vp, vp, i32, i32, i32]),
        "rav1e_inv_txfm_add_hip": (i32, [vp, vp, C.c_ssize_t, i32, i32, i32]),
        "rv_ec_scratch_bytes": (C.c_size_t, [i32]),
        "rv_ec_tokenize": (i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.c_uint32, vp,
                                 vp]),
        "rv_ec_code_tokens": (C.c_long, [vp, C.c_size_t, vp, vp, C.c_size_t]),
        "rv_ec_count_tokens": (C.c_long, [vp, C.c_size_t, vp, vp]),
        "rv_ec_rate_batch": (i32, [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]),
        "rv_ec_cdf_total": (i32, []),
        "rv_ec_default_cdf": (i32, [i32, vp]),
        "rv_ec_reset_counts": (None, [vp]),
        "rv_ec_mode_scratch_bytes": (C.c_size_t, [i32]),
        "rv_ec_mode_tokenize": (i32, [vp, i32, RvEcModeParams, i32, vp, i32, i32, vp, vp, vp, vp,
                                      C.c_uint32, vp, vp]),
        "rv_ec_code_stream": (C.c_long, [vp, C.c_size_t, vp, vp, C.c_size_t]),
        "rv_ec_count_stream": (C.c_long, [vp, C.c_size_t, vp, vp]),
        "rv_ec_cdf_total_all": (i32, []),
        "rv_ec_default_cdf_all": (i32, [i32, vp]),
        "rv_ec_reset_counts_all": (None, [vp]),
        "rv_ec_partition_gather": (i32, [vp, i32]),
        "rv_ec_rate_stream_batch": (i32, [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]),
        "rv_ec_rate_stream_batch_waves": (i32, [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp]),
        "rv_ec_cand_scratch_bytes": (C.c_size_t, [i32, i32]),
        "rv_ec_cand_tokenize": (i32, [vp, i32, vp, i32, vp, i32, RvEcModeParams, i32, vp, i32, i32,
                                      i32, i32, vp, i32, i32, vp, vp, vp, vp, C.c_uint32, vp, vp]),
        "rv_ec_cand_rates": (i32, [vp, i32, vp, i32, vp, i32, RvEcModeParams, i32, vp, i32, i32,
                                   i32, i32, vp, i32, i32, vp, vp, vp, vp, C.c_uint32, vp, i32, vp,
                                   vp, vp, vp, vp]),
        "rv_mvref_paint_scratch_bytes": (C.c_size_t, [RvMvrefGeom]),
        "rv_mvref_grid_paint": (i32, [vp, i32, RvMvrefGeom, vp, vp, vp, vp, vp]),
        "rv_find_mvrefs_batch": (i32, [vp, i32, RvMvrefGeom, vp, vp, vp, vp, vp]),
        "rv_ec_mode_fill_stacks": (i32, [vp, i32, RvMvrefGeom, vp, vp, vp, vp, vp]),
        "rv_inter_ref_sets_build": (i32, [vp, i32, vp, i32, i32, vp]),
        "rv_inter_mode_set_batch": (i32, [vp, vp, vp, i32, RvInterRefSets, i32, vp, vp, vp, vp]),
        "rv_motion_compensate_batch": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, vp]),
        "rv_motion_compensate_batch_lanes": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, i32,
                                                   vp]),
        "rv_motion_estimation_batch": (i32, [vp, vp, i32, vp, i32, vp, i32, RvInterRefSets, vp, vp,
                                             vp, vp, vp, vp, vp, vp, vp]),
        "rv_save_block_motion_scratch_bytes": (C.c_size_t, [i32, i32]),
        "rv_save_block_motion_batch": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp]),
        "rv_me_pmv_index": (i32, [i32, i32, i32]),
        "rv_segmentation_data": (i32, [i32, vp]),
        "rv_block_segment_batch": (i32, [vp, i32, vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp,
                                         vp, vp]),
        "rv_mode_decide_check": (i32, [vp, vp, i32, vp, vp, i32, i32]),
        "rv_mode_decide_batch": (i32, [vp, vp, i32, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, i32, vp,
                                       vp, vp, vp, vp, vp, vp, vp]),
        "rv_mode_decide_batch_lanes": (i32, [vp, vp, i32, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, i32,
                                             vp, vp, vp, vp, vp, vp, vp, i32, vp]),
        "rv_sad_fn": (vp, [i32, i32, i32]),
        "rv_satd_fn": (vp, [i32, i32, i32]),
        "rv_put_fn_get": (vp, [i32, i32, i32]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args


def lib():
    """Load the HIP library; raises if it was not built (no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Rav1eHipError(
                f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        _declare(L)
        _lib = L
    return _lib


def _check(rc, what):
    if rc != RV_OK:
        raise Rav1eHipError(f"{what} failed ({rc}): {lib().rv_last_error().decode()}")


def require_device(device: int = 0):
    """Fail loudly unless a gfx950 device is visible."""
    L = lib()
    if L.rv_device_count() <= device:
        raise Rav1eHipError("no HIP device visible: the HIP level needs a gfx950 GPU")
    _check(L.rv_set_device(device), "rv_set_device")


# ---- device memory --------------------------------------------------------
class DeviceBuffer:
    """Device allocation owned by Python (rv_malloc / rv_free)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.ptr = lib().rv_malloc(max(1, self.nbytes))
        if not self.ptr:
            raise Rav1eHipError(f"rv_malloc({nbytes}): {lib().rv_last_error().decode()}")

    @classmethod
    def from_array(cls, a: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        b.upload(a)
        return b

    def upload(self, a: np.ndarray, stream=None):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        if a.nbytes:
            _check(lib().rv_memcpy_h2d(self.ptr, a.ctypes.data, a.nbytes, stream), "rv_memcpy_h2d")

    def download(self, dtype, count=None, stream=None) -> np.ndarray:
        dt = np.dtype(dtype)
        n = self.nbytes // dt.itemsize if count is None else int(count)
        out = np.empty(n, dtype=dt)
        if out.nbytes:
            _check(lib().rv_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, stream),
                   "rv_memcpy_d2h")
        return out

    def zero(self, stream=None):
        _check(lib().rv_memset(self.ptr, 0, self.nbytes, stream), "rv_memset")
        _check(lib().rv_stream_sync(stream), "rv_stream_sync")

    def free(self):
        if self.ptr:
            lib().rv_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DevicePlane:
    """A padded plane in HBM with the reference's PlaneConfig geometry
    (Plane::new, src/frame/plane.rs:215-244)."""

    def __init__(self, width, height, xdec=0, ydec=0, xpad=0, ypad=0, hbd=False,
                 bit_depth=None):
        self.desc = RvPlane()
        nbytes = lib().rv_plane_geometry(C.byref(self.desc), width, height, xdec, ydec,
                                         xpad, ypad, 1 if hbd else 0)
        if bit_depth is not None:
            self.desc.bit_depth = int(bit_depth)
        self.buf = DeviceBuffer(nbytes)
        self.desc.data = self.buf.ptr
        self.dtype = np.uint16 if hbd else np.uint8

    @classmethod
    def from_array(cls, a: np.ndarray, xpad=0, ypad=0, xdec=0, ydec=0, pad=True,
                   bit_depth=None):
        p = cls(a.shape[1], a.shape[0], xdec, ydec, xpad, ypad, a.dtype == np.uint16,
                bit_depth)
        p.upload_visible(a, pad=pad)
        return p

    @classmethod
    def from_full(cls, full: np.ndarray, xorigin, yorigin, width, height, bit_depth=None):
        """Wrap a whole padded allocation (stride = full.shape[1])."""
        p = cls.__new__(cls)
        p.desc = RvPlane()
        p.desc.stride, p.desc.alloc_height = full.shape[1], full.shape[0]
        p.desc.width, p.desc.height = width, height
        p.desc.xorigin, p.desc.yorigin = xorigin, yorigin
        p.desc.hbd = 1 if full.dtype == np.uint16 else 0
        p.desc.bit_depth = bit_depth if bit_depth is not None else (0 if p.desc.hbd else 8)
        p.buf = DeviceBuffer.from_array(full)
        p.desc.data = p.buf.ptr
        p.dtype = full.dtype
        return p

    @property
    def shape_full(self):
        return (self.desc.alloc_height, self.desc.stride)

    def upload_visible(self, a: np.ndarray, pad=True):
        full = np.zeros(self.shape_full, dtype=self.dtype)
        d = self.desc
        full[d.yorigin:d.yorigin + d.height, d.xorigin:d.xorigin + d.width] = a
        self.buf.upload(full)
        if pad:
            _check(lib().rv_plane_pad(C.byref(self.desc), None), "rv_plane_pad")
            _check(lib().rv_stream_sync(None), "rv_stream_sync")

    def download_full(self) -> np.ndarray:
        return self.buf.download(self.dtype).reshape(self.shape_full)

    def download_visible(self) -> np.ndarray:
        d = self.desc
        return self.download_full()[d.yorigin:d.yorigin + d.height,
                                    d.xorigin:d.xorigin + d.width].copy()


def _sync(stream=None):
    _check(lib().rv_stream_sync(stream), "rv_stream_sync")


# ---- batched entry points (production path) -------------------------------
def sad_batch(org: DevicePlane, ref: DevicePlane, jobs: np.ndarray, w: int, h: int,
              satd: bool = False) -> np.ndarray:
    jobs = np.ascontiguousarray(jobs, dtype=DIST_JOB)
    dj = DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(4 * len(jobs))
    f = lib().rv_satd_batch if satd else lib().rv_sad_batch
    _check(f(C.byref(org.desc), C.byref(ref.desc), dj.ptr, len(jobs), w, h, out.ptr, None),
           "rv_satd_batch" if satd else "rv_sad_batch")
    _sync()
    return out.download(np.uint32)


def satd_batch(org, ref, jobs, w, h) -> np.ndarray:
    return sad_batch(org, ref, jobs, w, h, satd=True)


def lookahead_intra_costs(plane: DevicePlane, bit_depth: int = 8) -> np.ndarray:
    """compute_lookahead_intra_costs (src/api/internal.rs:680-765) of a luma
    plane: u32 [ceil(h / 8), ceil(w / 8)]."""
    nbx, nby = (plane.desc.width + 7) // 8, (plane.desc.height + 7) // 8
    out = DeviceBuffer(4 * nbx * nby)
    _check(lib().rv_lookahead_intra_costs(C.byref(plane.desc), int(bit_depth), out.ptr, None),
           "rv_lookahead_intra_costs")
    _sync()
    return out.download(np.uint32, nbx * nby).reshape(nby, nbx)


def propagate_importances(org: DevicePlane, ref: DevicePlane, mvs: np.ndarray,
                          intra_costs: np.ndarray, importances: np.ndarray, n_unique: int,
                          ref_importances: np.ndarray) -> np.ndarray:
    """compute_block_importances' propagation (src/api/internal.rs:823-1010)
    for one (frame, reference) pass: mvs [h_imp, w_imp] MOTION_VECTOR,
    intra_costs u32, importances f32 of the frame; returns the reference's
    f32 importances after the pass (ref_importances is the value before)."""
    nbx, nby = (org.desc.width + 7) // 8, (org.desc.height + 7) // 8
    mv = np.ascontiguousarray(mvs, dtype=MOTION_VECTOR).reshape(nby * nbx)
    dm = DeviceBuffer.from_array(mv)
    di = DeviceBuffer.from_array(np.ascontiguousarray(intra_costs, dtype=np.uint32).ravel())
    dp = DeviceBuffer.from_array(np.ascontiguousarray(importances, dtype=np.float32).ravel())
    dr = DeviceBuffer.from_array(np.ascontiguousarray(ref_importances, dtype=np.float32).ravel())
    nbytes = lib().rv_propagate_importances_scratch(nbx, nby)
    ds = DeviceBuffer(max(1, nbytes))
    _check(lib().rv_propagate_importances(C.byref(org.desc), C.byref(ref.desc), dm.ptr, di.ptr,
                                          dp.ptr, int(n_unique), dr.ptr, ds.ptr, nbytes, None),
           "rv_propagate_importances")
    _sync()
    return dr.download(np.float32, nbx * nby).reshape(nby, nbx)


def sse_batch(org, ref, jobs, w, h) -> np.ndarray:
    jobs = np.ascontiguousarray(jobs, dtype=DIST_JOB)
    bw = min(w, 8) >> org.desc.xdec
    bh = min(h, 8) >> org.desc.ydec
    nsub = (w // bw) * (h // bh)
    dj = DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(8 * nsub * max(1, len(jobs)))
    _check(lib().rv_sse_batch(C.byref(org.desc), C.byref(ref.desc), dj.ptr, len(jobs), w, h,
                              out.ptr, None), "rv_sse_batch")
    _sync()
    return out.download(np.uint64, nsub * len(jobs)).reshape(len(jobs), nsub)


def cdef_moments_batch(org, ref, jobs, w, h) -> np.ndarray:
    jobs = np.ascontiguousarray(jobs, dtype=DIST_JOB)
    nsub = (w // 8) * (h // 8)
    dj = DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(40 * nsub * max(1, len(jobs)))
    _check(lib().rv_cdef_moments_batch(C.byref(org.desc), C.byref(ref.desc), dj.ptr, len(jobs),
                                       w, h, out.ptr, None), "rv_cdef_moments_batch")
    _sync()
    return out.download(np.int64, 5 * nsub * len(jobs)).reshape(len(jobs), nsub, 5)


def put_8tap_batch(dst: DevicePlane, src: DevicePlane, jobs, w, h, mode_x=0, mode_y=0,
                   bit_depth=8):
    jobs = np.ascontiguousarray(jobs, dtype=MC_JOB)
    dj = DeviceBuffer.from_array(jobs)
    _check(lib().rv_put_8tap_batch(C.byref(dst.desc), C.byref(src.desc), dj.ptr, len(jobs), w, h,
                                   mode_x, mode_y, bit_depth, None), "rv_put_8tap_batch")
    _sync()


class PredictionMode(enum.IntEnum):
    """src/predict.rs:135-166."""
    DC_PRED = 0
    V_PRED = 1
    H_PRED = 2
    D45_PRED = 3
    D135_PRED = 4
    D117_PRED = 5
    D153_PRED = 6
    D207_PRED = 7
    D63_PRED = 8
    SMOOTH_PRED = 9
    SMOOTH_V_PRED = 10
    SMOOTH_H_PRED = 11
    PAETH_PRED = 12
    UV_CFL_PRED = 13
    NEARESTMV = 14
    NEAR0MV = 15
    NEAR1MV = 16
    NEAR2MV = 17
    GLOBALMV = 18
    NEWMV = 19
    NEAREST_NEARESTMV = 20
    NEAR_NEARMV = 21
    NEAREST_NEWMV = 22
    NEW_NEARESTMV = 23
    NEAR_NEWMV = 24
    NEW_NEARMV = 25
    GLOBAL_GLOBALMV = 26
    NEW_NEWMV = 27


# RAV1E_INTRA_MODES (src/predict.rs:32-46): the screening order
RAV1E_INTRA_MODES = [0, 2, 1, 9, 11, 10, 12, 3, 4, 5, 6, 7, 8]
EDGE_PX = 4 * 64 + 1  # edge_buf: 4 * MAX_TX_SIZE + 1


def predict_intra_batch(dst: DevicePlane, jobs, edges: np.ndarray, tx_size, bit_depth=8):
    """PredictionMode::predict_intra (no CfL) of every job into dst; edges
    (n, 257) in rav1e's edge_buf layout (src/predict.rs:545-551)."""
    jobs = np.ascontiguousarray(jobs, dtype=INTRA_JOB)
    edges = np.ascontiguousarray(edges, dtype=np.uint16 if bit_depth > 8 else np.uint8)
    if edges.shape != (len(jobs), EDGE_PX):
        raise Rav1eHipError("predict_intra_batch: edges must be (n_jobs, 257)")
    if not (0 <= jobs["mode"]).all() or not (jobs["mode"] <= 12).all():
        raise Rav1eHipError("predict_intra_batch: CfL / inter modes are not intra predictions here")
    dj = DeviceBuffer.from_array(jobs)
    de = DeviceBuffer.from_array(edges)
    _check(lib().rv_predict_intra_batch(C.byref(dst.desc), dj.ptr, de.ptr, len(jobs), tx_size,
                                        bit_depth, None), "rv_predict_intra_batch")
    _sync()


# ---- intra edges and mode screening (rv_intra_screen.hip) -------------------
INTRA_TILE = np.dtype([("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4")])
INTRA_BLK_JOB = np.dtype([("tile", "<i4"), ("bo_x", "<i4"), ("bo_y", "<i4"), ("bx", "<i4"),
                          ("by", "<i4"), ("po_x", "<i4"), ("po_y", "<i4"), ("cdf_off", "<i4")])
FRAME_TYPE_KEY, FRAME_TYPE_INTER = 0, 1  # FrameType (src/api/util.rs)
# kf_y_cdf [5][5][14] and y_mode_cdf [4][14] in the combined mode table
# (RV_ECM_KF_Y / RV_ECM_Y_MODE of rv_ec_mode_tables.h; tests/test_intra_screen.py
# holds them to the header)
ECM_KF_Y, ECM_Y_MODE = 4537, 4887
_INTRA_MODE_CONTEXT = [0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0]  # src/context.rs:2206-2207
_SIZE_GROUP = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 0, 0, 1, 1, 2, 2]  # :206-207
INTRA_MAX_BSIZE = BlockSize.BLOCK_64X64  # and no 4:1 / 1:4 size (all above it in the enum)
# BlockSize::tx_size (src/partition.rs:199-230) of the sizes screened: the
# transform of the block's own shape
_BSIZE_TX = {int(b): TxSize["TX_" + b.name[6:]] for b in BlockSize if b <= BlockSize.BLOCK_64X64}


def intra_mode_cdf_offset(frame_type, bsize, above_mode=0, left_mode=0) -> int:
    """Offset, in the combined CDF table, of the row rdo_mode_decision takes
    the intra-mode probabilities from (src/rdo.rs:1090-1094): for an INTER
    frame get_cdf_intra_mode(bsize) = y_mode_cdf[size_group_lookup[bsize]],
    else get_cdf_intra_mode_kf = kf_y_cdf[above_ctx][left_ctx] of the above /
    left blocks' modes, DC_PRED where the tile has none (src/context.rs:
    2203-2248)."""
    if frame_type == FRAME_TYPE_INTER:
        return ECM_Y_MODE + 14 * _SIZE_GROUP[int(BlockSize(bsize))]
    for m in (above_mode, left_mode):
        if not 0 <= int(m) <= 12:
            raise Rav1eHipError("intra_mode_cdf_offset: a key frame's neighbours are intra blocks "
                                "(modes 0 .. 12)")
    return ECM_KF_Y + (_INTRA_MODE_CONTEXT[int(above_mode)] * 5 +
                       _INTRA_MODE_CONTEXT[int(left_mode)]) * 14


def intra_plane_offset(bo_x, bo_y, xdec=0, ydec=0, bx=0, by=0, tx_size=TxSize.TX_4X4):
    """po of transform block (bx, by) of the partition at block offset (bo_x,
    bo_y): BlockOffset::plane_offset (src/context.rs:1293-1298), (bo >> dec)
    << 2 per axis, plus the transform block's own offset bx * tx width, by *
    tx height, as the encoder's transform loops form it."""
    tx = TxSize(tx_size)
    return ((np.asarray(bo_x) >> xdec) << 2) + np.asarray(bx) * tx.width(), \
           ((np.asarray(bo_y) >> ydec) << 2) + np.asarray(by) * tx.height()


def _intra_blk_args(who, plane: DevicePlane, tiles, jobs, bsize, tx_size, bit_depth):
    """The checks rv_intra_screen.hip leaves to the caller because jobs and
    tiles are device data: the reference would index outside its region."""
    tiles = np.ascontiguousarray(tiles, dtype=INTRA_TILE).reshape(-1)
    jobs = np.ascontiguousarray(jobs, dtype=INTRA_BLK_JOB).reshape(-1)
    d = plane.desc
    n = len(jobs)
    # the argument checks are the library's (bad sizes return their code
    # without a launch); only what depends on the records is checked here
    b, t = int(bsize), int(tx_size)
    if n and 0 <= b <= int(INTRA_MAX_BSIZE) and 0 <= t <= 18 and len(tiles):
        tx = TxSize(t)
        if ((jobs["tile"] < 0) | (jobs["tile"] >= len(tiles))).any():
            raise Rav1eHipError(f"{who}: a job names no tile")
        tl = tiles[jobs["tile"]]
        rx, ry = tl["x"] >> d.xdec, tl["y"] >> d.ydec
        rw, rh = tl["width"] >> d.xdec, tl["height"] >> d.ydec
        if (tl["x"] < 0).any() or (tl["y"] < 0).any() or (rw <= 0).any() or (rh <= 0).any() or \
                not _inside(plane, rx, ry, rx + rw, ry + rh):
            raise Rav1eHipError(f"{who}: a tile's region leaves the plane")
        if any((jobs[f] < 0).any() for f in ("bo_x", "bo_y", "bx", "by", "po_x", "po_y")):
            raise Rav1eHipError(f"{who}: negative block offset, index or plane offset")
        if (jobs["po_x"] + tx.width() > rw).any() or (jobs["po_y"] + tx.height() > rh).any():
            raise Rav1eHipError(f"{who}: a transform block leaves its tile's region "
                                "(get_intra_edges would index outside it)")
    return tiles, jobs


def intra_edges_batch(plane: DevicePlane, tiles, jobs, bsize, tx_size, bit_depth=8,
                      opt_mode=None) -> np.ndarray:
    """get_intra_edges (src/partition.rs:500-693) of every job (INTRA_BLK_JOB)
    from one plane of the reconstruction: tiles (INTRA_TILE) are luma
    rectangles, bsize the partition, tx_size the transform block, opt_mode
    None or a PredictionMode (UV_CFL_PRED included).  Returns (n, 257) pixels
    in predict_intra_batch's layout; what the reference leaves unwritten is
    zero."""
    tiles, jobs = _intra_blk_args("intra_edges_batch", plane, tiles, jobs, bsize, tx_size,
                                  bit_depth)
    n = len(jobs)
    dt, dj = DeviceBuffer.from_array(tiles), DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(EDGE_PX * np.dtype(plane.dtype).itemsize * max(1, n))
    _check(lib().rv_intra_edges_batch(C.byref(plane.desc), dt.ptr, len(tiles), dj.ptr, n,
                                      int(bsize), int(tx_size), bit_depth,
                                      -1 if opt_mode is None else int(opt_mode), out.ptr, None),
           "rv_intra_edges_batch")
    _sync()
    return out.download(plane.dtype, EDGE_PX * n).reshape(n, EDGE_PX)


def intra_mode_screen_batch(rec: DevicePlane, src: DevicePlane, tiles, jobs, bsize, cdf,
                            num_modes_rdo, bit_depth=8, with_satd=False, with_edges=False):
    """The intra-mode screening of rdo_mode_decision (src/rdo.rs:1029-1127)
    for n luma blocks of one bsize in one launch: rec / src the luma planes of
    the reconstruction and the source, jobs INTRA_BLK_JOB with bx = by = 0,
    po = 4 * bo and cdf_off the job's row in cdf (a u16 array or a
    DeviceBuffer holding the combined table; intra_mode_cdf_offset).
    Returns the list of mode lists and, on request, the SATDs (n, 13) in
    RAV1E_INTRA_MODES' order and the edges (n, 257).  rec is not written."""
    who = "intra_mode_screen_batch"
    b = int(bsize)
    tx = _BSIZE_TX.get(b, TxSize.TX_4X4)
    tiles, jobs = _intra_blk_args(who, rec, tiles, jobs, bsize, tx, bit_depth)
    n = len(jobs)
    if isinstance(cdf, DeviceBuffer):
        dc, cdf_len = cdf, cdf.nbytes // 2
    else:
        cdf = np.ascontiguousarray(cdf, dtype=np.uint16).reshape(-1)
        dc, cdf_len = DeviceBuffer.from_array(cdf), len(cdf)
    if n and b in _BSIZE_TX and len(tiles):
        if (jobs["bx"] != 0).any() or (jobs["by"] != 0).any() or \
                (jobs["po_x"] != 4 * jobs["bo_x"]).any() or (jobs["po_y"] != 4 * jobs["bo_y"]).any():
            raise Rav1eHipError(f"{who}: the screening is of the whole luma block (bx = by = 0, "
                                "po = 4 * bo)")
        tl = tiles[jobs["tile"]]
        sx, sy = tl["x"] + jobs["po_x"], tl["y"] + jobs["po_y"]
        if not _inside(src, sx, sy, sx + tx.width(), sy + tx.height()):
            raise Rav1eHipError(f"{who}: a source block leaves the padded plane")
        if (jobs["cdf_off"] < 0).any() or (jobs["cdf_off"] + 14 > cdf_len).any():
            raise Rav1eHipError(f"{who}: a CDF row leaves the table")
    dt, dj = DeviceBuffer.from_array(tiles), DeviceBuffer.from_array(jobs)
    dm = DeviceBuffer(8 * max(1, n))
    ds = DeviceBuffer(4 * 13 * max(1, n)) if with_satd else None
    de = DeviceBuffer(EDGE_PX * np.dtype(rec.dtype).itemsize * max(1, n)) if with_edges else None
    _check(lib().rv_intra_screen_batch(C.byref(rec.desc), C.byref(src.desc), dt.ptr, len(tiles),
                                       dj.ptr, n, b, bit_depth, dc.ptr, cdf_len,
                                       int(num_modes_rdo), dm.ptr, ds.ptr if ds else None,
                                       de.ptr if de else None, None), "rv_intra_screen_batch")
    _sync()
    m = dm.download(np.uint8, 8 * n).reshape(n, 8)
    res = [[int(v) for v in row[1:1 + row[0]]] for row in m]
    out = (res,)
    if with_satd:
        out += (ds.download(np.uint32, 13 * n).reshape(n, 13),)
    if with_edges:
        out += (de.download(rec.dtype, EDGE_PX * n).reshape(n, EDGE_PX),)
    return out[0] if len(out) == 1 else out


def intra_screen_select(satds, cdf_row, num_modes_rdo):
    """The host form of the selection (src/rdo.rs:1086-1127) for one block:
    satds in RAV1E_INTRA_MODES' order, cdf_row the row's entries.  What
    intra_mode_screen_batch does on the device after its SATDs."""
    order = sorted(range(13), key=lambda k: int(satds[k]))  # stable
    z, probs_all = 32768, []
    for a in list(cdf_row)[:13]:
        probs_all.append((z - int(a)) & 0xffff)
        z = int(a)
    porder = sorted(range(13), key=lambda k: 0xffff ^ probs_all[RAV1E_INTRA_MODES[k]])
    modes = [RAV1E_INTRA_MODES[k] for k in porder[:num_modes_rdo // 2]]
    for k in order[:num_modes_rdo]:
        if RAV1E_INTRA_MODES[k] not in modes:
            modes.append(RAV1E_INTRA_MODES[k])
    return modes[:num_modes_rdo]


# ---- a partition's transform blocks (rv_tx_blocks.hip) ----------------------
TX_BLOCKS_JOB = np.dtype([("tile", "<i4"), ("bo_x", "<i4"), ("bo_y", "<i4"), ("qindex", "<i4"),
                          ("alpha_u", "<i4"), ("alpha_v", "<i4")])
TX_BLOCKS_MAX = 256  # RV_TX_BLOCKS_MAX


class RvTxBlocksParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("bsize", "tx_size", "tx_type", "luma_mode", "chroma_mode",
                                         "skip", "luma_only", "need_recon_pixel", "coeff_rate",
                                         "bit_depth")] + \
               [("dc_delta_q", C.c_int32 * 3), ("ac_delta_q", C.c_int32 * 3)]


class RvTxBlocksLayout(C.Structure):
    _fields_ = [("planes", C.c_int32)] + \
               [(n, C.c_int32 * 3) for n in ("tx_size", "plane_w", "plane_h", "cols", "rows",
                                             "n_blocks", "coded_area", "first_block", "level_off")] + \
               [("blocks_per_job", C.c_int32), ("levels_per_job", C.c_int32),
                ("blk_x", (C.c_uint8 * TX_BLOCKS_MAX) * 3), ("blk_y", (C.c_uint8 * TX_BLOCKS_MAX) * 3)]


def tx_blocks_layout(bsize, tx_size, xdec=1, ydec=1, luma_only=False) -> RvTxBlocksLayout:
    """rv_tx_blocks_layout: per plane the transform-block count (cols x rows =
    bw x bh, bw_uv x bh_uv of src/encoder.rs:1764-1765, 1821-1832), the
    plane's tx_size (uv_tx_size = largest_chroma_tx_size), the coded area per
    block and each block's pixel offset inside the partition, and the per-job
    strides of tx_blocks_batch's outputs.  Raises with the library's error
    code (Rav1eHipError.code) for what the launch would refuse."""
    out = RvTxBlocksLayout()
    rc = lib().rv_tx_blocks_layout(int(bsize), int(tx_size), int(xdec), int(ydec),
                                   1 if luma_only else 0, C.byref(out))
    if rc != RV_OK:
        err = Rav1eHipError(f"rv_tx_blocks_layout failed ({rc}): {lib().rv_last_error().decode()}")
        err.code = rc
        raise err
    return out


def _plane_set(planes, count):
    if planes is None:
        return None
    arr = (RvPlane * 3)()
    for p in range(count):
        arr[p] = planes[p].desc
    return arr


def tx_blocks_batch(rec, src, tiles, jobs, bsize, tx_size, luma_mode, chroma_mode=0,
                    tx_type=TxType.DCT_DCT, skip=False, luma_only=False, need_recon_pixel=True,
                    coeff_rate=True, bit_depth=8, dc_delta_q=(0, 0, 0), ac_delta_q=(0, 0, 0),
                    pred=None, dst=None):
    """write_tx_blocks / write_tx_tree without the bitstream writer (src/
    encoder.rs:1757-2037) for n partitions of one bsize in one launch: every
    encode_tx_block of each job, in the reference's order.  rec / src (and
    pred for an inter luma_mode, dst when the pixels are wanted): sequences of
    three DevicePlanes (one with luma_only); tiles INTRA_TILE, jobs
    TX_BLOCKS_JOB (tile, partition_bo in tile-relative 4x4 luma units, the
    block's qindex, the CfL alphas).  rec is not written.

    Returns (layout, levels, eobs, dists): three lists with one array per
    coded plane, levels (n, n_blocks, coded_area) i32 in rv_quantize_batch's
    raster, eobs (n, n_blocks) u32 as write_coeffs_lv_map counts them, dists
    (n, n_blocks) u64 the shifted tx-domain distortion."""
    who = "tx_blocks_batch"
    tiles = np.ascontiguousarray(tiles, dtype=INTRA_TILE).reshape(-1)
    jobs = np.ascontiguousarray(jobs, dtype=TX_BLOCKS_JOB).reshape(-1)
    n = len(jobs)
    count = 1 if luma_only else 3
    inter = int(luma_mode) >= int(PredictionMode.NEARESTMV)
    for name, ps in (("rec", rec), ("src", src), ("pred", pred), ("dst", dst)):
        if ps is None and name in ("rec", "src"):
            raise Rav1eHipError(f"{who}: {name} is required")
        if ps is not None and len(ps) < count:
            raise Rav1eHipError(f"{who}: {name} needs {count} plane(s)")
    xdec, ydec = (0, 0) if luma_only else (rec[1].desc.xdec, rec[1].desc.ydec)
    # the argument checks are the library's (they return their code without a
    # launch); what depends on the records -- device data to the library -- is
    # checked here: the reference would index outside its regions
    b = int(bsize)
    if n and 0 <= b <= int(INTRA_MAX_BSIZE):
        bw4, bh4 = BlockSize(b).width() // 4, BlockSize(b).height() // 4
        if len(tiles) == 0 or ((jobs["tile"] < 0) | (jobs["tile"] >= len(tiles))).any():
            raise Rav1eHipError(f"{who}: a job names no tile")
        tl = tiles[jobs["tile"]]
        if (jobs["bo_x"] < 0).any() or (jobs["bo_y"] < 0).any() or (jobs["bo_x"] % bw4).any() or \
                (jobs["bo_y"] % bh4).any():
            raise Rav1eHipError(f"{who}: a partition offset is negative or not a multiple of the "
                                "block size")
        if (4 * (jobs["bo_x"] + bw4) > tl["width"]).any() or \
                (4 * (jobs["bo_y"] + bh4) > tl["height"]).any():
            raise Rav1eHipError(f"{who}: a partition leaves its tile")
        if ((jobs["qindex"] < 1) | (jobs["qindex"] > 255)).any():
            raise Rav1eHipError(f"{who}: qindex is 1 .. 255 (lossless is not supported)")
        for name, ps in (("rec", rec), ("src", src), ("pred", pred if inter else None),
                         ("dst", dst)):
            for p in range(count if ps is not None else 0):
                d = ps[p].desc
                rx, ry = tl["x"] >> d.xdec, tl["y"] >> d.ydec
                rw, rh = tl["width"] >> d.xdec, tl["height"] >> d.ydec
                if (tl["x"] < 0).any() or (tl["y"] < 0).any() or \
                        not _inside(ps[p], rx, ry, rx + rw, ry + rh):
                    raise Rav1eHipError(f"{who}: a tile's region leaves a {name} plane")
    prm = RvTxBlocksParams(int(bsize), int(tx_size), int(tx_type), int(luma_mode), int(chroma_mode),
                           1 if skip else 0, 1 if luma_only else 0, 1 if need_recon_pixel else 0,
                           1 if coeff_rate else 0, int(bit_depth))
    for p in range(3):
        prm.dc_delta_q[p], prm.ac_delta_q[p] = int(dc_delta_q[p]), int(ac_delta_q[p])
    # sizes of the outputs: the layout, where the arguments have one
    lay = RvTxBlocksLayout()
    have = lib().rv_tx_blocks_layout(b, int(tx_size), xdec, ydec, 1 if luma_only else 0,
                                     C.byref(lay)) == RV_OK
    nb, nl = (lay.blocks_per_job, lay.levels_per_job) if have else (1, 1)
    dt, dj = DeviceBuffer.from_array(tiles), DeviceBuffer.from_array(jobs)
    dl, de, dd = DeviceBuffer(4 * nl * max(1, n)), DeviceBuffer(4 * nb * max(1, n)), \
        DeviceBuffer(8 * nb * max(1, n))
    sets = [_plane_set(ps, count) for ps in (rec, src, pred, dst)]
    _check(lib().rv_tx_blocks_batch(sets[0], sets[1], sets[2], sets[3], dt.ptr, len(tiles), dj.ptr, n,
                                    C.byref(prm), dl.ptr, de.ptr, dd.ptr, None), "rv_tx_blocks_batch")
    _sync()
    lv = dl.download(np.int32, nl * n).reshape(n, nl)
    eo = de.download(np.uint32, nb * n).reshape(n, nb)
    di = dd.download(np.uint64, nb * n).reshape(n, nb)
    levels, eobs, dists = [], [], []
    for p in range(lay.planes):
        k, ca, f0, l0 = lay.n_blocks[p], lay.coded_area[p], lay.first_block[p], lay.level_off[p]
        levels.append(lv[:, l0:l0 + k * ca].reshape(n, k, ca))
        eobs.append(eo[:, f0:f0 + k])
        dists.append(di[:, f0:f0 + k])
    return lay, levels, eobs, dists


# ---- chroma from luma (rv_cfl.hip) ------------------------------------------
def cfl_allowed(bsize) -> bool:
    """BlockSize::cfl_allowed (src/partition.rs:174-177): enum order."""
    return 0 <= int(bsize) <= int(BlockSize.BLOCK_32X32)


# the sizes subsampled_size maps to a valid one at 4:2:2
_SS_422 = {"BLOCK_4X4", "BLOCK_8X4", "BLOCK_8X8", "BLOCK_16X4", "BLOCK_16X8", "BLOCK_16X16",
           "BLOCK_32X8", "BLOCK_32X16", "BLOCK_32X32", "BLOCK_64X16", "BLOCK_64X32", "BLOCK_64X64",
           "BLOCK_128X64", "BLOCK_128X128"}


def subsampled_size(bsize, xdec, ydec):
    """BlockSize::subsampled_size (src/partition.rs:245-286) as (w, h) of the
    chroma-plane block, or None for BLOCK_INVALID."""
    b = BlockSize(bsize)
    w, h = b.width(), b.height()
    if (xdec, ydec) == (0, 0):
        return w, h
    if (xdec, ydec) == (1, 0):
        return (max(4, w // 2), h) if b.name in _SS_422 else None
    if (xdec, ydec) == (1, 1):  # every size has one
        return max(4, w // 2), max(4, h // 2)
    raise Rav1eHipError("subsampled_size: 4:4:4, 4:2:2 or 4:2:0")


def has_chroma(x, y, bsize, xdec, ydec):
    """has_chroma (src/context.rs:551-560) of the block at luma pixel (x, y)."""
    b = BlockSize(bsize)
    bx, by = np.asarray(x) >> 2, np.asarray(y) >> 2
    okx = ((bx & 1) == 1) | ((b.width() >> 2) & 1 == 0) | (xdec == 0)
    oky = ((by & 1) == 1) | ((b.height() >> 2) & 1 == 0) | (ydec == 0)
    return okx & oky


def _cfl_geometry(who, bsize, xdec, ydec):
    """(w, h) of the chroma block and the luma origin's sub8x8_offset in
    pixels (src/partition.rs:303-312), or the argument error."""
    if not cfl_allowed(bsize):
        raise Rav1eHipError(f"{who}: CfL needs a block size up to BLOCK_32X32 (cfl_allowed)")
    if (xdec, ydec) not in ((0, 0), (1, 0), (1, 1)):
        raise Rav1eHipError(f"{who}: subsampling must be 4:4:4, 4:2:2 or 4:2:0")
    wh = subsampled_size(bsize, xdec, ydec)
    if wh is None:
        raise Rav1eHipError(f"{who}: {BlockSize(bsize).name} has no subsampled size at "
                            f"xdec {xdec}, ydec {ydec}")
    b = BlockSize(bsize)
    return wh, (-4 if xdec and b.width() == 4 else 0, -4 if ydec and b.height() == 4 else 0)


def _cfl_jobs(who, jobs, bsize, xdec, ydec):
    jobs = np.ascontiguousarray(jobs, dtype=CFL_JOB)
    if ((jobs["x"] & 3) != 0).any() or ((jobs["y"] & 3) != 0).any() or \
            (jobs["x"] < 0).any() or (jobs["y"] < 0).any():
        raise Rav1eHipError(f"{who}: job positions are luma pixels of a block offset (4 * bo)")
    if not np.all(has_chroma(jobs["x"], jobs["y"], bsize, xdec, ydec)):
        raise Rav1eHipError(f"{who}: a job's block has no chroma (has_chroma)")
    if ((jobs["variant"] < 0) | (jobs["variant"] > 3)).any():
        raise Rav1eHipError(f"{who}: variant is a PredictionVariant (0 .. 3)")
    return jobs


def _inside(plane: DevicePlane, x0, y0, x1, y1) -> bool:
    """Whether the pixel rectangles [x0, x1) x [y0, y1) (arrays, visible
    coordinates) lie inside the plane's padded allocation."""
    d = plane.desc
    return bool(np.all(x0 >= -d.xorigin) and np.all(x1 <= d.stride - d.xorigin) and
                np.all(y0 >= -d.yorigin) and np.all(y1 <= d.alloc_height - d.yorigin))


def _cfl_run_plane(who, plane: DevicePlane):
    """The planes rv_cfl.hip reads in aligned pixel runs."""
    d = plane.desc
    if d.xorigin & 3 or d.stride & 3 or (d.data or 0) & 15:
        raise Rav1eHipError(f"{who}: xorigin and stride must be multiples of 4 and the "
                            "allocation 16-byte aligned (rv_plane_geometry's layout)")


def luma_ac_batch(luma: DevicePlane, jobs, bsize, xdec, ydec) -> np.ndarray:
    """luma_ac (src/encoder.rs:1714-1755) of every job (CFL_JOB: the
    partition's luma pixel position): (n, H, W) i16 over the chroma-plane
    block W x H = bsize.subsampled_size(xdec, ydec)."""
    (w, h), (ox, oy) = _cfl_geometry("luma_ac_batch", bsize, xdec, ydec)
    jobs = _cfl_jobs("luma_ac_batch", jobs, bsize, xdec, ydec)
    _cfl_run_plane("luma_ac_batch", luma)
    lx, ly = jobs["x"] + ox, jobs["y"] + oy
    if not _inside(luma, lx, ly, lx + (w << xdec), ly + (h << ydec)):
        raise Rav1eHipError("luma_ac_batch: a luma block leaves the padded plane")
    dj = DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(2 * w * h * max(1, len(jobs)))
    _check(lib().rv_cfl_luma_ac_batch(C.byref(luma.desc), dj.ptr, len(jobs), int(bsize), xdec, ydec,
                                      out.ptr, None), "rv_cfl_luma_ac_batch")
    _sync()
    return out.download(np.int16, w * h * len(jobs)).reshape(len(jobs), h, w)


def predict_cfl_batch(dst: DevicePlane, jobs, edges: np.ndarray, ac: np.ndarray, alpha, tx_size,
                      bit_depth=8):
    """predict_intra(UV_CFL_PRED) (src/predict.rs:202-241, 836-892) of every
    job (INTRA_JOB with mode 13) into dst: edges (n, 257) as for
    predict_intra_batch, ac (n, H, W) i16, alpha (n,) in -16 .. 16."""
    tx = TxSize(tx_size)
    w, h = tx.width(), tx.height()
    if w > 32 or h > 32:
        raise Rav1eHipError("predict_cfl_batch: no CfL for 64-point transform sizes")
    jobs = np.ascontiguousarray(jobs, dtype=INTRA_JOB)
    n = len(jobs)
    edges = np.ascontiguousarray(edges, dtype=np.uint16 if bit_depth > 8 else np.uint8)
    if edges.shape != (n, EDGE_PX):
        raise Rav1eHipError("predict_cfl_batch: edges must be (n_jobs, 257)")
    ac = np.asarray(ac)
    if ac.dtype != np.int16 or ac.shape != (n, h, w):
        raise Rav1eHipError("predict_cfl_batch: ac must be int16 (n_jobs, H, W)")
    ac = np.ascontiguousarray(ac)
    alpha = np.asarray(alpha)
    if alpha.shape != (n,) or (np.abs(alpha.astype(np.int64)) > 16).any():
        raise Rav1eHipError("predict_cfl_batch: alpha must be (n_jobs,) in -16 .. 16")
    alpha = np.ascontiguousarray(alpha, dtype=np.int16)
    if not (jobs["mode"] == PredictionMode.UV_CFL_PRED).all():
        raise Rav1eHipError("predict_cfl_batch: jobs must have mode UV_CFL_PRED")
    if ((jobs["variant"] < 0) | (jobs["variant"] > 3)).any():
        raise Rav1eHipError("predict_cfl_batch: variant is a PredictionVariant (0 .. 3)")
    if not _inside(dst, jobs["x"], jobs["y"], jobs["x"] + w, jobs["y"] + h):
        raise Rav1eHipError("predict_cfl_batch: a block leaves the padded plane")
    dj, de = DeviceBuffer.from_array(jobs), DeviceBuffer.from_array(edges)
    da, dl = DeviceBuffer.from_array(ac), DeviceBuffer.from_array(alpha)
    _check(lib().rv_predict_cfl_batch(C.byref(dst.desc), dj.ptr, de.ptr, da.ptr, dl.ptr, n,
                                      int(tx_size), bit_depth, None), "rv_predict_cfl_batch")
    _sync()


def cfl_alpha_search_batch(rec, src, jobs, bsize, bit_depth=8, with_cost=False):
    """rdo_cfl_alpha (src/rdo.rs:1261-1336) of every job: rec / src = three
    DevicePlanes each (Y, U, V; the reconstruction and the source), jobs
    CFL_JOB (the partition's luma pixel position and the chroma block's
    PredictionVariant).  Returns alpha (n, 2) i16 for U and V -- what the
    reference's scan returns, not the argmin -- and, with_cost, the SSE at
    that alpha (n, 2) u64.  rec is left untouched."""
    if len(rec) != 3 or len(src) != 3:
        raise Rav1eHipError("cfl_alpha_search_batch: rec / src are three planes each")
    xdec, ydec = rec[1].desc.xdec, rec[1].desc.ydec
    for p in (1, 2):
        if (rec[p].desc.xdec, rec[p].desc.ydec, src[p].desc.xdec, src[p].desc.ydec) != \
                (xdec, ydec, xdec, ydec):
            raise Rav1eHipError("cfl_alpha_search_batch: chroma planes differ in subsampling")
    (w, h), (ox, oy) = _cfl_geometry("cfl_alpha_search_batch", bsize, xdec, ydec)
    jobs = _cfl_jobs("cfl_alpha_search_batch", jobs, bsize, xdec, ydec)
    for p in (rec[0], src[1], src[2]):
        _cfl_run_plane("cfl_alpha_search_batch", p)
    lx, ly = jobs["x"] + ox, jobs["y"] + oy
    cx, cy = ((jobs["x"] >> 2) >> xdec) << 2, ((jobs["y"] >> 2) >> ydec) << 2
    left, top = jobs["variant"] & 1, (jobs["variant"] >> 1) & 1
    if not _inside(rec[0], lx, ly, lx + (w << xdec), ly + (h << ydec)) or \
            not all(_inside(rec[p], cx - left, cy - top, cx + w, cy + h) and
                    _inside(src[p], cx, cy, cx + w, cy + h) for p in (1, 2)):
        raise Rav1eHipError("cfl_alpha_search_batch: a block or its neighbours leave the padded "
                            "plane")
    n = len(jobs)
    rp = (RvPlane * 3)(*(p.desc for p in rec))
    sp = (RvPlane * 3)(*(p.desc for p in src))
    dj = DeviceBuffer.from_array(jobs)
    da = DeviceBuffer(4 * max(1, n))
    dc = DeviceBuffer(16 * max(1, n)) if with_cost else None
    _check(lib().rv_cfl_alpha_search_batch(rp, sp, dj.ptr, n, int(bsize), bit_depth, da.ptr,
                                           dc.ptr if dc else None, None),
           "rv_cfl_alpha_search_batch")
    _sync()
    alpha = da.download(np.int16, 2 * n).reshape(n, 2)
    return (alpha, dc.download(np.uint64, 2 * n).reshape(n, 2)) if with_cost else alpha


class CFLParams:
    """CFLParams (src/context.rs:1866-1915): the joint sign and the two
    magnitudes write_cfl_alphas codes.  CFLSign: 0 ZERO, 1 NEG, 2 POS."""
    SIGN_ZERO, SIGN_NEG, SIGN_POS = 0, 1, 2
    _SIGN_VALUE = (0, -1, 1)  # cfl_sign_value

    def __init__(self, sign=(1, 0), scale=(1, 0)):  # Default: (NEG, ZERO), (1, 0)
        self.sign, self.scale = tuple(sign), tuple(scale)

    @classmethod
    def from_alpha(cls, u: int, v: int) -> "CFLParams":
        sg = lambda a: (cls.SIGN_NEG, cls.SIGN_ZERO, cls.SIGN_POS)[(a > 0) - (a < 0) + 1]
        return cls((sg(u), sg(v)), (abs(int(u)), abs(int(v))))

    def joint_sign(self) -> int:
        assert self.sign[0] != self.SIGN_ZERO or self.sign[1] != self.SIGN_ZERO
        return self.sign[0] * 3 + self.sign[1] - 1

    def context(self, uv: int) -> int:
        assert self.sign[uv] != self.SIGN_ZERO
        return (self.sign[uv] - 1) * 3 + self.sign[1 - uv]

    def index(self, uv: int) -> int:
        assert self.sign[uv] != self.SIGN_ZERO and self.scale[uv] != 0
        return self.scale[uv] - 1

    def alpha(self, uv: int) -> int:
        return self._SIGN_VALUE[self.sign[uv]] * self.scale[uv]


# ---- scene-change detection (rv_scenecut.hip) -----------------------------------
DELTA_MAX_FRAMES, DELTA_MAX_PAIRS = 8, 16  # RV_DELTA_MAX_FRAMES / _PAIRS


def _delta_geometry(frames, pairs):
    """The checks of rv_frame_delta_batch, on the descriptors alone; returns
    (n_planes, pairs as int32 (n, 2))."""
    who = "frame_deltas"
    frames = [tuple(f) for f in frames]
    if not 2 <= len(frames) <= DELTA_MAX_FRAMES:
        raise Rav1eHipError(f"{who}: 2 .. {DELTA_MAX_FRAMES} frames, not {len(frames)}")
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if not 1 <= len(pairs) <= DELTA_MAX_PAIRS:
        raise Rav1eHipError(f"{who}: 1 .. {DELTA_MAX_PAIRS} pairs, not {len(pairs)}")
    if (pairs < 0).any() or (pairs >= len(frames)).any():
        raise Rav1eHipError(f"{who}: a pair index is out of range")
    n_planes = len(frames[0])
    if n_planes not in (1, 3) or any(len(f) != n_planes for f in frames):
        raise Rav1eHipError(f"{who}: every frame is 1 plane (luma) or 3 planes")
    key = lambda d: (d.width, d.height, d.xdec, d.ydec)
    first = [p.desc for p in frames[0]]
    for f in frames:
        for k, p in enumerate(f):
            if p.desc.hbd != first[0].hbd:
                raise Rav1eHipError(f"{who}: the frames mix 8-bit and high-bit-depth planes (hbd)")
            if key(p.desc) != key(first[k]):
                raise Rav1eHipError(f"{who}: the frames differ in size or decimation")
    w, h = first[0].width, first[0].height
    if w < 1 or h < 1 or (first[0].xdec, first[0].ydec) != (0, 0):
        raise Rav1eHipError(f"{who}: plane 0 is the luma plane")
    for d in first[1:]:
        if (d.xdec, d.ydec) not in ((0, 0), (1, 0), (1, 1)) or key(d) != key(first[1]):
            raise Rav1eHipError(f"{who}: chroma must be 4:4:4, 4:2:2 or 4:2:0")
        if (d.width, d.height) != ((w + d.xdec) >> d.xdec, (h + d.ydec) >> d.ydec):
            raise Rav1eHipError(f"{who}: a chroma plane's size is not the luma size rounded up "
                                "by its decimation")
    return n_planes, np.ascontiguousarray(pairs, dtype=np.int32)


def frame_deltas(frames, pairs) -> np.ndarray:
    """The sums has_scenecut (src/scenechange/mod.rs:167-207) forms over
    Frame::iter() (PixelIter, src/frame/mod.rs:126-172), before its division:
    frames a list of 1- or 3-tuples of DevicePlane, pairs (n, 2) indices into
    it; returns u64 (n_pairs, n_planes).  One launch reads every frame once."""
    n_planes, pairs = _delta_geometry(frames, pairs)
    descs = (RvPlane * (len(frames) * n_planes))(*(p.desc for f in frames for p in f))
    out = DeviceBuffer(8 * len(pairs) * n_planes)
    _check(lib().rv_frame_delta_batch(descs, len(frames), n_planes, pairs.ctypes.data, len(pairs),
                                      out.ptr, None), "rv_frame_delta_batch")
    _sync()
    return out.download(np.uint64, len(pairs) * n_planes).reshape(len(pairs), n_planes)


def scenecut_threshold(bit_depth: int) -> int:
    """SceneChangeDetector::new (src/scenechange/mod.rs:33-49): BASE_THRESHOLD
    * bit_depth / 8."""
    return 12 * int(bit_depth) // 8


def fast_scene_detection(speed: int) -> bool:
    """SpeedSettings::fast_scene_detection_preset (src/api/config.rs:409-411):
    luma only at speed 10."""
    return int(speed) == 10


def keyframe_lookahead_distance(low_latency: bool = False) -> int:
    """InterConfig::keyframe_lookahead_distance (src/api/internal.rs:182-188):
    max(1, group_input_len) + 1, group_input_len 4 with the reorder pyramid
    and 1 without (low_latency)."""
    return max(1, 1 if low_latency else 4) + 1


class SceneChangeDetector:
    """SceneChangeDetector (src/scenechange/mod.rs) over frames in HBM: a frame
    is a tuple of DevicePlane, (Y,) or (Y, U, V); fast_mode reads Y alone.

    analyze_next_frame issues at most one frame_deltas launch: it first
    collects the distinct frame pairs exclude_scene_flashes and is_key_frame
    will compare, takes from the memo those an earlier call summed, and sends
    the rest in one batch.  The memo is keyed by the pair's input frame
    numbers and forgets pairs that reach back before input_frameno - 1.  With
    the lookahead distance d, call N compares frame N - 1 with N .. N + d - 1
    and N .. N + d - 2 with N + d - 1; all of these but the ones that name the
    newest frame N + d - 1 were summed by the d - 1 calls before.  So in a
    steady stream a call launches d pairs over d + 1 frames: 5 pairs over 6
    frames at the reference's distance of 5, where a call on its own needs 9.

    launches / launch_pairs count the batches and the pairs of each."""

    def __init__(self, bit_depth: int, fast_mode: bool):
        self.threshold = scenecut_threshold(bit_depth)
        self.fast_mode = bool(fast_mode)
        self.excluded_frames = set()
        self._memo = {}  # (frameno_a, frameno_b), a < b -> plane sums
        self.launches = 0
        self.launch_pairs = []

    # -- has_scenecut (:167-207): the part after the fold
    def scenecut_from_sums(self, sums, length: int) -> bool:
        if self.fast_mode:
            delta_avg = int(sums[0]) // length
        else:
            d = [(int(s) // length) & 0xffff for s in sums[:3]]  # as u16
            delta_avg = ((d[0] + d[1] + d[2]) & 0xffff) // 3
        return delta_avg >= self.threshold

    def _planes(self, frame):
        frame = tuple(frame)
        if self.fast_mode:
            return frame[:1]
        if len(frame) != 3:
            raise Rav1eHipError("SceneChangeDetector: YUV mode needs (Y, U, V) frames")
        return frame

    def _launch(self, frames, pairs):
        self.launches += 1
        self.launch_pairs.append(len(pairs))
        return frame_deltas([self._planes(f) for f in frames], pairs)

    @staticmethod
    def _len(frame):
        d = frame[0].desc
        return d.width * d.height

    def has_scenecut(self, f1, f2) -> bool:
        """has_scenecut of two frames outside a stream: one launch, no memo."""
        sums = self._launch([f1, f2], [(1, 0)])[0]
        return self.scenecut_from_sums(sums, self._len(f2))

    def _fetch(self, frame_set, frameno0, wanted):
        """Sum the pairs of `wanted` (indices into frame_set, a < b) that the
        memo lacks, in one launch over the frames they name."""
        missing = [p for p in dict.fromkeys(wanted)
                   if (frameno0 + p[0], frameno0 + p[1]) not in self._memo]
        if not missing:
            return
        used = sorted({i for p in missing for i in p})
        at = {i: k for k, i in enumerate(used)}
        sums = self._launch([frame_set[i] for i in used], [(at[a], at[b]) for a, b in missing])
        for (a, b), s in zip(missing, sums):
            self._memo[(frameno0 + a, frameno0 + b)] = tuple(int(v) for v in s)

    def analyze_next_frame(self, previous_frame, frame_set, input_frameno, min_key_frame_interval,
                           max_key_frame_interval, no_scene_detection, lookahead_distance,
                           keyframes, keyframes_forced):
        """analyze_next_frame (:58-87): frame_set[0] is frame input_frameno;
        keyframes (a set) is updated in place."""
        if previous_frame is None:
            keyframes.add(0)  # The first frame is always a keyframe.
            return
        frame_set = [previous_frame] + list(frame_set)
        first = input_frameno - 1  # the frame number of frame_set[0]
        for k in [k for k in self._memo if k[0] < first]:
            del self._memo[k]

        # every comparison the two functions below can make, first
        distance = min(lookahead_distance, len(frame_set) - 1)
        wanted = []
        if distance > 1:
            wanted += [(0, j) for j in range(1, distance + 1)]
        wanted += [(i, distance) for i in range(1, distance)]
        if (0, 1) not in wanted and self._reaches_has_scenecut(
                input_frameno, min_key_frame_interval, max_key_frame_interval, no_scene_detection,
                keyframes, keyframes_forced):
            wanted.append((0, 1))
        self._fetch(frame_set, first, wanted)
        length = self._len(frame_set[1])
        cut = lambda a, b: self.scenecut_from_sums(self._memo[(first + a, first + b)], length)

        self._exclude_scene_flashes(cut, len(frame_set), input_frameno, lookahead_distance)
        if self._is_key_frame(cut, input_frameno, min_key_frame_interval, max_key_frame_interval,
                              no_scene_detection, keyframes, keyframes_forced):
            keyframes.add(input_frameno)

    def _reaches_has_scenecut(self, frameno, min_kf, max_kf, no_scene_detection, keyframes,
                              keyframes_forced):
        """Whether is_key_frame gets past its early returns, given that this
        call excludes nothing (a frame_set too short for exclude_scene_flashes
        to compare anything)."""
        if frameno in keyframes_forced:
            return False
        distance = frameno - max(keyframes)
        return not (distance < min_kf or distance >= max_kf or no_scene_detection or
                    frameno in self.excluded_frames)

    def _is_key_frame(self, cut, current_frameno, min_kf, max_kf, no_scene_detection, keyframes,
                      keyframes_forced):
        """is_key_frame (:90-121)"""
        if current_frameno in keyframes_forced:
            return True
        # Find the distance to the previous keyframe.
        previous_keyframe = max(keyframes)
        distance = current_frameno - previous_keyframe
        # Handle minimum and maximum key frame intervals.
        if distance < min_kf:
            return False
        if distance >= max_kf:
            return True
        # Skip smart scene detection if it's disabled
        if no_scene_detection:
            return False
        if current_frameno in self.excluded_frames:
            return False
        return cut(0, 1)

    def _exclude_scene_flashes(self, cut, n_frames, frameno, keyframe_lookahead_distance):
        """exclude_scene_flashes (:125-164)"""
        lookahead_distance = min(keyframe_lookahead_distance, n_frames - 1)
        # Where A and B are scenes: AAAAAABBBAAAAAA
        # If BBB is shorter than lookahead_distance, it is detected as a flash
        # and not considered a scenecut.
        if lookahead_distance > 1:
            for j in range(1, lookahead_distance + 1):
                if not cut(0, j):
                    # Any frame in between `0` and `j` cannot be a real scenecut.
                    for i in range(0, j + 1):
                        self.excluded_frames.add(frameno + i - 1)
        # Where A-F are scenes: AAAAABBCCDDEEFFFFFF
        # If each of BB ... EE are shorter than `lookahead_distance`, they are
        # detected as flashes and not considered scenecuts.
        # Instead, the first F frame becomes a scenecut.
        for i in range(1, lookahead_distance + 1):
            if i < lookahead_distance and cut(i, lookahead_distance):
                # If the current frame is the frame before a scenecut, it cannot
                # also be the frame of a scenecut.
                self.excluded_frames.add(frameno + i - 1)


class KeyframeDetector:
    """The streaming driver of the detector: ContextInner::send_frame and
    compute_lookahead_data's first loop (src/api/internal.rs:280-330, 767-810)
    under Context::send_frame / flush (src/api/mod.rs:304-321, 490-492).

    Frame N is analysed once the last key of the frame queue is at least N +
    distance + 1, or after flush(), which appends a None entry and sets the
    limit to the frame count; the frame_set handed to the detector is every
    frame from N to the end of the queue at that moment.  Only the distance +
    2 most recent frames stay referenced (alive on the device): frame N - 1,
    the oldest one a later analysis reads, up to the newest.  `keyframes` is
    the set of input frame numbers chosen so far."""

    def __init__(self, bit_depth: int, fast_mode: bool, min_key_frame_interval: int = 12,
                 max_key_frame_interval: int = 240, low_latency: bool = False,
                 no_scene_detection: bool = False):
        self.detector = SceneChangeDetector(bit_depth, fast_mode)
        self.min_key_frame_interval = int(min_key_frame_interval)
        self.max_key_frame_interval = int(max_key_frame_interval)
        self.no_scene_detection = bool(no_scene_detection)
        self.distance = keyframe_lookahead_distance(low_latency)
        self.frame_count = 0
        self.limit = None
        self.is_flushing = False
        self.frame_q = {}  # input_frameno -> frame, or None for the end marker
        self.last_key = None  # frame_q.keys().last(): survives the dropping of old entries
        self.keyframes = set()
        self.keyframes_forced = set()
        self.next_lookahead_frame = 0

    launches = property(lambda self: self.detector.launches)
    launch_pairs = property(lambda self: self.detector.launch_pairs)
    excluded_frames = property(lambda self: self.detector.excluded_frames)

    def send_frame(self, frame, force_key: bool = False):
        if frame is None:
            if self.is_flushing:
                return
            self.limit = self.frame_count
            self.is_flushing = True
        elif self.is_flushing:
            raise Rav1eHipError("KeyframeDetector: a frame after flush() (EnoughData)")
        input_frameno = self.frame_count
        if frame is not None:
            self.frame_count += 1
        self.frame_q[input_frameno] = frame
        self.last_key = input_frameno
        if force_key and frame is not None:
            self.keyframes_forced.add(input_frameno)
        self._compute_lookahead_data()

    def flush(self):
        self.send_frame(None)

    def _needs_more_frames(self, frame_count):
        return self.limit is None or frame_count < self.limit

    def _needs_more_frame_q_lookahead(self, input_frameno):
        lookahead_end = self.last_key if self.last_key is not None else 0
        frames_needed = input_frameno + self.distance + 1
        return lookahead_end < frames_needed and self._needs_more_frames(lookahead_end)

    def _compute_lookahead_data(self):
        lookahead_frames = [f for n, f in sorted(self.frame_q.items())
                            if n >= self.next_lookahead_frame and f is not None]
        lookahead_idx = 0
        while not self._needs_more_frame_q_lookahead(self.next_lookahead_frame):
            current_lookahead_frames = lookahead_frames[lookahead_idx:]
            if not current_lookahead_frames:
                break  # All frames have been processed
            self.detector.analyze_next_frame(
                None if self.next_lookahead_frame == 0
                else self.frame_q.get(self.next_lookahead_frame - 1),
                current_lookahead_frames, self.next_lookahead_frame, self.min_key_frame_interval,
                self.max_key_frame_interval, self.no_scene_detection, self.distance,
                self.keyframes, self.keyframes_forced)
            self.next_lookahead_frame += 1
            lookahead_idx += 1
        for n in [n for n in self.frame_q if n < self.next_lookahead_frame - 1]:
            del self.frame_q[n]  # nothing reads them again


def deblock_plane(plane: DevicePlane, pli, width, height, lg: np.ndarray, skip: np.ndarray,
                  levels, bit_depth=8):
    """deblock_plane (src/deblock.rs:1174-1335) of plane pli of a width x
    height frame, in place.  lg / skip: (rows, cols) per luma 4x4 block
    (log2 of the square block's width in 4x4 units, skip flag); levels =
    [Y vertical, Y horizontal, U, V]."""
    lg = np.ascontiguousarray(lg, dtype=np.uint8)
    skip = np.ascontiguousarray(skip, dtype=np.uint8)
    if lg.shape != skip.shape or lg.shape[1] < (width + 3) // 4 or lg.shape[0] < (height + 3) // 4:
        raise Rav1eHipError("deblock_plane: lg / skip must cover the frame's 4x4 grid")
    if not (lg <= 4).all():
        raise Rav1eHipError("deblock_plane: block sizes 4x4 .. 64x64 (lg 0 .. 4)")
    dl, ds = DeviceBuffer.from_array(lg), DeviceBuffer.from_array(skip)
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.uint8))
    _check(lib().rv_deblock_plane(C.byref(plane.desc), pli, width, height, dl.ptr, ds.ptr,
                                  lg.shape[1], lv.ctypes.data, bit_depth, None), "rv_deblock_plane")
    _sync()


def _map_buffers(width, height, lg, skip, who):
    lg = np.ascontiguousarray(lg, dtype=np.uint8)
    skip = np.ascontiguousarray(skip, dtype=np.uint8)
    if lg.shape != skip.shape or lg.shape[1] < (width + 3) // 4 or lg.shape[0] < (height + 3) // 4:
        raise Rav1eHipError(who + ": lg / skip must cover the frame's 4x4 grid")
    if not (lg <= 4).all():
        raise Rav1eHipError(who + ": block sizes 4x4 .. 64x64 (lg 0 .. 4)")
    return lg, DeviceBuffer.from_array(lg), DeviceBuffer.from_array(skip)


def deblock_sse(rec, src, width, height, lg: np.ndarray, skip: np.ndarray, bit_depth=8):
    """sse_optimize (src/deblock.rs:1418-1475) of a frame: rec / src = three
    DevicePlanes each (Y U V).  Returns (tallies (3, 2, 65) int64: vertical,
    horizontal per plane; levels [Y vertical, Y horizontal, U, V])."""
    lg, dl, ds = _map_buffers(width, height, lg, skip, "deblock_sse")
    rp = (RvPlane * 3)(*(p.desc for p in rec))
    sp = (RvPlane * 3)(*(p.desc for p in src))
    dt = DeviceBuffer(3 * 130 * 8)
    dv = DeviceBuffer(4)
    _check(lib().rv_deblock_sse(rp, sp, width, height, dl.ptr, ds.ptr, lg.shape[1], dt.ptr, dv.ptr,
                                bit_depth, None), "rv_deblock_sse")
    _sync()
    return (dt.download(np.int64, 390).reshape(3, 2, 65),
            [int(v) for v in dv.download(np.uint8, 4)])


def deblock_frame(planes, width, height, lg: np.ndarray, skip: np.ndarray, levels, bit_depth=8):
    """deblock_filter_frame (src/deblock.rs:1410-1416) of three DevicePlanes
    with the levels passed through device memory (rv_deblock_frame)."""
    lg, dl, ds = _map_buffers(width, height, lg, skip, "deblock_frame")
    pp = (RvPlane * 3)(*(p.desc for p in planes))
    dv = DeviceBuffer.from_array(np.ascontiguousarray(np.asarray(levels, dtype=np.uint8)))
    _check(lib().rv_deblock_frame(pp, width, height, dl.ptr, ds.ptr, lg.shape[1], dv.ptr,
                                  bit_depth, None), "rv_deblock_frame")
    _sync()


def deblock_fast_level(ac_q, bit_depth, is_key=False):
    return int(lib().rv_deblock_fast_level(int(ac_q), bit_depth, 1 if is_key else 0))


def cdef_filter_frame(src, dst, width, height, skip: np.ndarray, cdef_index: np.ndarray,
                      y_strengths, uv_strengths, damping=3, bit_depth=8, stream=None):
    """cdef_filter_frame (src/cdef.rs:542-641) of a frame: src / dst = three
    DevicePlanes each (Y, U, V; distinct), skip per luma 4x4 block (rows,
    cols >= 2 * ceil(width / 8)), cdef_index per 64x64 superblock, the
    FrameInvariants strength tables and damping.  Returns (dir, var) per
    8x8 luma block (cdef_analyze_superblock)."""
    cols8, rows8 = (width + 7) // 8, (height + 7) // 8
    skip = np.ascontiguousarray(skip, dtype=np.uint8)
    cdef_index = np.ascontiguousarray(cdef_index, dtype=np.uint8)
    if skip.shape[1] < 2 * cols8 or skip.shape[0] < 2 * rows8:
        raise Rav1eHipError("cdef_filter_frame: skip must cover the frame's 8x8 grid")
    if cdef_index.shape[0] < (height + 63) // 64 or cdef_index.shape[1] != (width + 63) // 64:
        raise Rav1eHipError("cdef_filter_frame: cdef_index is per 64x64 superblock")
    if cdef_index.max(initial=0) > 7:
        raise Rav1eHipError("cdef_filter_frame: cdef_index above 7")
    ds, di = DeviceBuffer.from_array(skip), DeviceBuffer.from_array(cdef_index)
    dd, dv = DeviceBuffer(cols8 * rows8), DeviceBuffer(4 * cols8 * rows8)
    ys = np.ascontiguousarray(np.asarray(y_strengths, dtype=np.uint8))
    us = np.ascontiguousarray(np.asarray(uv_strengths, dtype=np.uint8))
    if ys.shape != (8,) or us.shape != (8,):
        raise Rav1eHipError("cdef_filter_frame: 8 strengths per table")
    _check(lib().rv_cdef_find_dirs(C.byref(src[0].desc), width, height, ds.ptr, skip.shape[1],
                                   dd.ptr, dv.ptr, bit_depth, stream), "rv_cdef_find_dirs")
    for pli in range(3):
        _check(lib().rv_cdef_filter_plane(C.byref(src[pli].desc), C.byref(dst[pli].desc), pli,
                                          width, height, ds.ptr, skip.shape[1], dd.ptr, dv.ptr,
                                          di.ptr, ys.ctypes.data, us.ctypes.data, damping,
                                          bit_depth, stream), "rv_cdef_filter_plane")
    _sync(stream)
    return (dd.download(np.uint8).reshape(rows8, cols8),
            dv.download(np.int32).reshape(rows8, cols8))


def lrf_stripe_filter(cd, db, x0, y0, sw, sh, cw, ch, set_, xqd, bit_depth=8, stream=None):
    """One stripe through the device's loop-restoration filter code
    (lrf_filter_frame's chunk body): setup_integral_image's view of the
    sw x sh stripe at (x0, y0) of a cw x ch crop of DevicePlanes cd (the
    CDEF output) / db (the deblocked frame, outside the stripe's rows), then
    sgrproj_stripe_filter (src/lrf.rs:677-760) with set `set_` and xqd.
    Returns the restored stripe (sh x sw)."""
    hbd = cd.desc.hbd
    out = DeviceBuffer(sw * sh * (2 if hbd else 1))
    _check(lib().rv_lrf_stripe_filter(C.byref(cd.desc), C.byref(db.desc), x0, y0, sw, sh, cw, ch,
                                      set_, int(xqd[0]), int(xqd[1]), bit_depth, out.ptr, stream),
           "rv_lrf_stripe_filter")
    _sync(stream)
    return out.download(np.uint16 if hbd else np.uint8).reshape(sh, sw)


# ---- stream containers: y4m input, IVF output (rv_container.hip) -----------
class Y4mInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("width", "height", "bit_depth", "xdec", "ydec", "fps_num",
                                       "fps_den")]


class Y4mReader:
    """A y4m stream (the input rav1e's CLI reads, src/bin/decoder/y4m.rs):
    `info` (width, height, bit depth, chroma decimation, frame rate) and
    read_frame() -> the frame's packed planar samples (Y, U, V; the layout
    HipReplay.set_input takes), or None at the end of the stream."""

    def __init__(self, path):
        self.h = lib().rv_y4m_open(os.fsencode(path))
        if not self.h:
            raise Rav1eHipError(f"rv_y4m_open failed: {lib().rv_last_error().decode()}")
        self.info = Y4mInfo()
        _check(lib().rv_y4m_get_info(self.h, C.byref(self.info)), "rv_y4m_get_info")
        self.nbytes = int(lib().rv_y4m_frame_bytes(self.h))

    def read_frame(self):
        hbd = self.info.bit_depth > 8
        out = np.empty(self.nbytes // (2 if hbd else 1), np.uint16 if hbd else np.uint8)
        rc = lib().rv_y4m_read_frame(self.h, out.ctypes.data)
        if rc == 1:
            return None
        _check(rc, "rv_y4m_read_frame")
        return out

    def close(self):
        if self.h:
            lib().rv_y4m_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class IvfWriter:
    """An IVF file (ivf/src/lib.rs write_ivf_header / write_ivf_frame)."""

    def __init__(self, path, width, height, fps_num=30, fps_den=1):
        self.h = lib().rv_ivf_create(os.fsencode(path), width, height, fps_num, fps_den)
        if not self.h:
            raise Rav1eHipError(f"rv_ivf_create failed: {lib().rv_last_error().decode()}")

    def write_frame(self, pts, data: bytes):
        buf = np.frombuffer(bytes(data), np.uint8)
        _check(lib().rv_ivf_write_frame(self.h, int(pts), buf.ctypes.data if len(buf) else None,
                                        len(buf)), "rv_ivf_write_frame")

    def close(self):
        if self.h:
            _check(lib().rv_ivf_close(self.h), "rv_ivf_close")
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---- entropy coding (src/ec.rs, src/context.rs write_coeffs_lv_map) --------
EC_JOB = np.dtype({"names": ["kind", "plane", "bx", "by", "tx_size", "tx_type", "is_inter",
                             "bw_lg", "bh_lg", "tile", "coeffs"],
                   "formats": [np.int32] * 10 + [np.uint64],
                   "offsets": [4 * i for i in range(10)] + [40], "itemsize": 48})


EC_BITRES = 3  # OD_BITRES (src/ec.rs): rates are in 1/8 bit


def ec_default_cdf(qctx):
    """CDFContext::new's coefficient CDFs for q context qctx (flat u16)."""
    out = np.zeros(lib().rv_ec_cdf_total(), np.uint16)
    _check(lib().rv_ec_default_cdf(qctx, out.ctypes.data), "rv_ec_default_cdf")
    return out


def ec_code_tokens(tokens, cdf):
    """One tile's tokens through the host range coder; cdf adapts in place."""
    tokens = np.ascontiguousarray(tokens, np.uint32)
    out = np.zeros(tokens.size // 2 + 4096, np.uint8)  # > 2 bytes per token never happens
    c2 = cdf.copy()
    n = lib().rv_ec_code_tokens(tokens.ctypes.data, tokens.size, c2.ctypes.data, out.ctypes.data,
                                out.size)
    if n < 0:
        _check(int(n), "rv_ec_code_tokens")
    if n > out.size:
        out = np.zeros(n, np.uint8)
        c2 = cdf.copy()
        lib().rv_ec_code_tokens(tokens.ctypes.data, tokens.size, c2.ctypes.data, out.ctypes.data,
                                out.size)
    cdf[:] = c2
    return out[:n]


def ec_count_tokens(tokens, cdf, state=None):
    """tokens through the host bit counter (WriterBase<WriterCounter>): the
    tell_frac() difference in 1 / 2**EC_BITRES bit; cdf adapts in place.
    state: (rng, cnt, bytes) of the writer before (None: a fresh writer).
    Returns (rate, state after)."""
    tokens = np.ascontiguousarray(tokens, np.uint32)
    rng, cnt, nbytes = (0x8000, -9, 0) if state is None else (int(v) for v in state)
    st = np.array([rng, cnt & 0xFFFF, nbytes], np.uint32)
    c2 = np.array(cdf, np.uint16)
    rate = lib().rv_ec_count_tokens(tokens.ctypes.data, tokens.size, c2.ctypes.data,
                                    st.ctypes.data)
    if rate < 0:
        _check(int(rate), "rv_ec_count_tokens")
    cdf[:] = c2
    cnt = int(st[1])
    return int(rate), (int(st[0]), cnt - 0x10000 if cnt & 0x8000 else cnt, int(st[2]))


class _EcTokens:
    """rv_ec_tokenize of a coding-order job list: the device buffers and the
    tile starts."""

    def __init__(self, jobs, coeffs, xdec, ydec, what, min_tiles=1, min_map=(1, 1)):
        jobs = np.asarray(jobs, np.int64).reshape(-1, 10)
        n = len(jobs)
        self.n = n
        self.co = DeviceBuffer.from_array(np.ascontiguousarray(coeffs, np.int32))
        ej = np.zeros(n, EC_JOB)
        for k, f in enumerate(["kind", "plane", "bx", "by", "tx_size", "tx_type", "is_inter",
                               "bw_lg", "bh_lg"]):
            ej[f] = jobs[:, k]
        starts = np.nonzero(jobs[:, 0] == 3)[0]
        if len(starts) == 0 or starts[0] != 0:
            starts = np.concatenate([[0], starts])
        tile = np.cumsum(jobs[:, 0] == 3) - 1
        ej["tile"] = np.maximum(tile, 0)
        ej["coeffs"] = self.co.ptr + 4 * jobs[:, 9].astype(np.uint64)
        self.starts, self.ntiles = starts, max(len(starts), int(min_tiles))
        ext = np.where(jobs[:, 0] == 0, 1 << jobs[:, 4], np.where(jobs[:, 0] == 1, 1 << np.maximum(jobs[:, 7] - 2, 0), 0))
        mw = int(max(min_map[0], (jobs[:, 2] + ext).max() if n else 1))
        mh = int(max(min_map[1], (jobs[:, 3] + ext).max() if n else 1))
        dj = DeviceBuffer.from_array(ej) if n else None
        dmap = DeviceBuffer(self.ntiles * 3 * mw * mh)
        self.dmap, self.mw, self.mh = dmap, mw, mh  # the context map the jobs leave behind
        scr = DeviceBuffer(lib().rv_ec_scratch_bytes(n))
        self.doff = DeviceBuffer(4 * (n + 1))
        cap = int(64 * n + 8 * int(np.asarray(coeffs).size) + 1024)
        self.dtok = DeviceBuffer(4 * cap)
        dst = DeviceBuffer(8)
        _check(lib().rv_ec_tokenize(dj.ptr if n else None, n, xdec, ydec, self.ntiles, mw, mh,
                                    dmap.ptr, scr.ptr,
                                    self.doff.ptr, self.dtok.ptr, cap, dst.ptr, None),
               "rv_ec_tokenize")
        _sync(None)
        self.status = dst.download(np.uint32)
        if self.status[1]:
            raise Rav1eHipError(what + ": token buffer overflow")

    def offsets(self):
        return self.doff.download(np.uint32)[:self.n + 1]

    def tokens(self):
        return self.dtok.download(np.uint32)[:int(self.status[0])]


def code_coefficients(jobs, coeffs, cdf_init, xdec, ydec):
    """A coding-order job sequence (rows kind, plane, bx, by, tx_size, tx_type,
    is_inter, bw_lg, bh_lg, coeff_off; kind 3 starts a tile) through the
    device tokenizer and the host range coder: write_coeffs_lv_map of every
    transform block, reset_skip_context / reset_left_contexts between them.
    Returns (bytes of all tiles, bytes per tile, the last tile's final CDFs,
    tokens)."""
    tk = _EcTokens(jobs, coeffs, xdec, ydec, "code_coefficients")
    n, ntiles, starts = tk.n, tk.ntiles, tk.starts
    off = tk.offsets()
    tok = tk.tokens()
    out, tb, cdf = [], [], None
    for t in range(ntiles):
        a = int(off[starts[t]])
        b = int(off[starts[t + 1]]) if t + 1 < ntiles else int(off[n])
        cdf = np.array(cdf_init, np.uint16)
        by = ec_code_tokens(tok[a:b], cdf)
        out.append(by)
        tb.append(len(by))
    return np.concatenate(out), np.array(tb, np.int32), cdf, tok


# ---- block mode info (rv_ec_mode.hip) ---------------------------------------
_EC_MODE_FIELDS = ["kind", "tile", "bx", "by", "bsize", "partition", "skip", "seg_idx",
                   "luma_mode", "chroma_mode", "ref0", "ref1", "mv0_row", "mv0_col", "mv1_row",
                   "mv1_col", "ref_mv0_row", "ref_mv0_col", "ref_mv1_row", "ref_mv1_col",
                   "mode_context", "num_mv_found", "weight0", "weight1", "weight2", "weight3",
                   "cfl_joint_sign", "cfl_scale_u", "cfl_scale_v", "reserved0", "reserved1",
                   "reserved2"]
# rv_ec_mode_job: 32 int32 (ref[2], mv[4], ref_mv[4], weight[4], cfl_scale[2] flattened)
EC_MODE_JOB = np.dtype({"names": _EC_MODE_FIELDS, "formats": [np.int32] * 32,
                        "offsets": [4 * i for i in range(32)], "itemsize": 128})
FRAME_KEY, FRAME_INTER = 0, 1
REF_CAT_LEVEL = 640


class EcModeParams:
    """The frame parameters of rv_ec_mode_tokenize and every tile's (cols,
    rows) in luma 4x4 units.  reference_mode: 0 ReferenceMode::SINGLE."""

    def __init__(self, frame_type=FRAME_INTER, reference_mode=0, force_integer_mv=0,
                 allow_high_precision_mv=0, seg_enabled=0, last_active_segid=0,
                 tile_dims=((16, 16),)):
        self.frame_type, self.reference_mode = int(frame_type), int(reference_mode)
        self.force_integer_mv = int(force_integer_mv)
        self.allow_high_precision_mv = int(allow_high_precision_mv)
        self.seg_enabled, self.last_active_segid = int(seg_enabled), int(last_active_segid)
        self.tile_dims = np.ascontiguousarray(tile_dims, np.int32).reshape(-1, 2)

    def c_struct(self):
        return RvEcModeParams(self.frame_type, self.reference_mode, self.force_integer_mv,
                              self.allow_high_precision_mv, self.seg_enabled,
                              self.last_active_segid)


def ec_mode_jobs(rows):
    """An (n, <= 32) integer array in EC_MODE_JOB's field order as EC_MODE_JOB."""
    rows = np.asarray(rows, np.int64)
    rows = rows.reshape(-1, rows.shape[-1] if rows.ndim > 1 else 32)
    out = np.zeros(len(rows), EC_MODE_JOB)
    for k, f in enumerate(_EC_MODE_FIELDS[:rows.shape[1]]):
        out[f] = rows[:, k]
    return out


def _mode_has_near(m):
    P = PredictionMode
    return P.NEAR0MV <= m <= P.NEAR2MV or m in (P.NEAR_NEARMV, P.NEAR_NEWMV, P.NEW_NEARMV)


def check_mode_jobs(jobs, stack_mvs=None):
    """The assert!s of encode_block_post_cdef (src/encoder.rs:1537-1617) and
    write_ref_frames on a job list: NEW_NEWMV needs two stack entries, a NEAR
    mode its stack entry, NEARESTMV / a NEAR mode the stack's MV (NEARESTMV
    against ref_mv, the stack's entry 0; the NEAR modes against stack_mvs
    (n, 4, 2) row / col when given), a compound block a width of 8."""
    P = PredictionMode
    for i, j in enumerate(np.asarray(jobs)):
        m = int(j["luma_mode"])
        if int(j["kind"]) != 0 or m < P.NEARESTMV:
            continue
        nf = int(j["num_mv_found"])
        mv0 = (int(j["mv0_row"]), int(j["mv0_col"]))
        if m >= P.NEAREST_NEARESTMV and int(j["bsize"]) < BlockSize.BLOCK_8X8:
            raise Rav1eHipError(f"job {i}: a compound block below 8x8")
        if m == P.NEW_NEWMV and nf < 2:
            raise Rav1eHipError(f"job {i}: NEW_NEWMV with {nf} MV stack entries")
        if _mode_has_near(m):
            idx = m - P.NEAR0MV + 1 if m <= P.NEAR2MV else 1
            if m != P.NEAR0MV and nf <= idx:
                raise Rav1eHipError(f"job {i}: a NEAR mode without its MV stack entry")
            if stack_mvs is not None:
                want = tuple(int(v) for v in stack_mvs[i][idx]) if nf > 1 else (0, 0)
                if mv0 != want:
                    raise Rav1eHipError(f"job {i}: a NEAR mode whose MV is not the stack's")
        elif m == P.NEARESTMV:
            want = (int(j["ref_mv0_row"]), int(j["ref_mv0_col"])) if nf else (0, 0)
            if mv0 != want:
                raise Rav1eHipError(f"job {i}: NEARESTMV whose MV is not the stack's")


def resolve_skip_segments(jobs, params):
    """write_segmentation stores its prediction into a skip block
    (src/context.rs:3536-3544, get_segment_pred :3465-3505) and later
    neighbours read it: a serial walk in coding order that fills the skip
    blocks' seg_idx with what the reference stores.  The identity with
    segmentation off or every block in segment 0.  Returns a copy."""
    jobs = np.array(jobs, EC_MODE_JOB)
    if not params.seg_enabled or not jobs["seg_idx"].any():
        return jobs
    maps = {}
    for j in jobs:
        if j["kind"] != 0 or j["bsize"] not in (3, 6, 9, 12):
            continue
        t = int(j["tile"])
        if not 0 <= t < len(params.tile_dims):
            continue
        cols, rows = (int(v) for v in params.tile_dims[t])
        bx, by = int(j["bx"]), int(j["by"])
        if not (0 <= bx < cols and 0 <= by < rows):
            continue
        m = maps.setdefault(t, np.zeros(((rows + 1) // 2 + 8, (cols + 1) // 2 + 8), np.int32))
        x, y, n8 = bx >> 1, by >> 1, 1 << (int(j["bsize"]) // 3 - 1)
        if j["skip"]:
            ul = m[y - 1, x - 1] if bx > 0 and by > 0 else -1
            u = m[y - 1, x] if by > 0 else -1
            l = m[y, x - 1] if bx > 0 else -1
            if u == -1:
                j["seg_idx"] = 0 if l == -1 else l
            elif l == -1:
                j["seg_idx"] = u
            else:
                j["seg_idx"] = u if ul == u else l
        m[y:y + n8, x:x + n8] = j["seg_idx"]
    return jobs


def ec_default_cdf_all(qctx):
    """CDFContext::new's CDFs in the combined layout (coefficients, then mode info)."""
    out = np.zeros(lib().rv_ec_cdf_total_all(), np.uint16)
    _check(lib().rv_ec_default_cdf_all(qctx, out.ctypes.data), "rv_ec_default_cdf_all")
    return out


def ec_code_stream(tokens, cdf_all):
    """One tile's mixed tokens through the host range coder; cdf_all adapts in place."""
    tokens = np.ascontiguousarray(tokens, np.uint32)
    out = np.zeros(tokens.size // 2 + 4096, np.uint8)
    c2 = np.array(cdf_all, np.uint16)
    n = lib().rv_ec_code_stream(tokens.ctypes.data, tokens.size, c2.ctypes.data, out.ctypes.data,
                                out.size)
    if n < 0:
        _check(int(n), "rv_ec_code_stream")
    if n > out.size:
        out = np.zeros(n, np.uint8)
        c2 = np.array(cdf_all, np.uint16)
        lib().rv_ec_code_stream(tokens.ctypes.data, tokens.size, c2.ctypes.data, out.ctypes.data,
                                out.size)
    cdf_all[:] = c2
    return out[:n]


def ec_count_stream(tokens, cdf_all, state=None):
    """ec_count_tokens over the combined table and mixed tokens."""
    tokens = np.ascontiguousarray(tokens, np.uint32)
    rng, cnt, nbytes = (0x8000, -9, 0) if state is None else (int(v) for v in state)
    st = np.array([rng, cnt & 0xFFFF, nbytes], np.uint32)
    c2 = np.array(cdf_all, np.uint16)
    rate = lib().rv_ec_count_stream(tokens.ctypes.data, tokens.size, c2.ctypes.data,
                                    st.ctypes.data)
    if rate < 0:
        _check(int(rate), "rv_ec_count_stream")
    cdf_all[:] = c2
    cnt = int(st[1])
    return int(rate), (int(st[0]), cnt - 0x10000 if cnt & 0x8000 else cnt, int(st[2]))


def ec_tokenize_modes(jobs, params, stack_mvs=None, check=True):
    """rv_ec_mode_tokenize of a coding-order EC_MODE_JOB list (skip blocks'
    seg_idx already resolved).  check: raise where the reference's assert!s
    would fire (check_mode_jobs); without it the device only counts such jobs.
    Returns (tokens u32, offsets u32 [n + 1], rejected job count)."""
    jobs = np.ascontiguousarray(jobs, EC_MODE_JOB)
    if check:
        check_mode_jobs(jobs, stack_mvs)
    return _ec_mode_tokenize(jobs, params)[:3]


def _ec_mode_tokenize(jobs, params):
    """rv_ec_mode_tokenize: (tokens, offsets, rejected, the neighbour-record map
    the jobs leave behind (device), its (w8, h8), the tile sizes (device))."""
    n = len(jobs)
    dims = params.tile_dims
    nt = len(dims)
    mw = int(max(1, (dims[:, 0].max() + 1) // 2))
    mh = int(max(1, (dims[:, 1].max() + 1) // 2))
    dj = DeviceBuffer.from_array(jobs) if n else None
    ddim = DeviceBuffer.from_array(dims)
    dmap = DeviceBuffer(nt * mw * mh * 4)
    scr = DeviceBuffer(lib().rv_ec_mode_scratch_bytes(n))
    doff = DeviceBuffer(4 * (n + 1))
    cap = 72 * n + 16
    dtok = DeviceBuffer(4 * cap)
    dst = DeviceBuffer(12)
    _check(lib().rv_ec_mode_tokenize(dj.ptr if n else None, n, params.c_struct(), nt, ddim.ptr, mw,
                                     mh, dmap.ptr, scr.ptr, doff.ptr, dtok.ptr, cap, dst.ptr,
                                     None), "rv_ec_mode_tokenize")
    _sync(None)
    status = dst.download(np.uint32)
    if status[1]:
        raise Rav1eHipError("ec_tokenize_modes: token buffer overflow")
    return (dtok.download(np.uint32)[:int(status[0])], doff.download(np.uint32)[:n + 1],
            int(status[2]), dmap, (mw, mh), ddim)


def code_tile(mode_jobs, coeff_jobs, coeffs, coeff_after, params, cdf_init, xdec=1, ydec=1,
              stack_mvs=None):
    """One tile's payload symbols: every block's mode tokens (rv_ec_mode_tokenize)
    followed by the coefficient tokens of its transform blocks (rv_ec_tokenize),
    through the host range coder.  coeff_jobs: code_coefficients' rows of this
    one tile (kind 1 / 2 rows carry no tokens but keep the contexts right);
    coeff_after[k]: the index of the mode job whose tokens coefficient job k
    follows (ascending).  cdf_init:
    the combined table.  Returns (bytes, final CDFs, tokens)."""
    mode_jobs = np.ascontiguousarray(mode_jobs, EC_MODE_JOB)
    coeff_jobs = np.asarray(coeff_jobs, np.int64).reshape(-1, 10)
    coeff_after = np.asarray(coeff_after, np.int64)
    if len(coeff_after) != len(coeff_jobs) or (np.diff(coeff_after) < 0).any() or \
            (len(coeff_after) and not 0 <= coeff_after.min() <= coeff_after.max() < len(mode_jobs)):
        raise Rav1eHipError("code_tile: coeff_after must map every coefficient job to a mode job")
    mtok, moff, bad = ec_tokenize_modes(mode_jobs, params, stack_mvs)
    if bad:
        raise Rav1eHipError(f"code_tile: {bad} mode jobs outside the tokenizer's restrictions")
    if len(coeff_jobs):
        tk = _EcTokens(coeff_jobs, coeffs, xdec, ydec, "code_tile")
        ctok, coff = tk.tokens(), tk.offsets().astype(np.int64)
    else:
        ctok, coff = np.zeros(0, np.uint32), np.zeros(1, np.int64)
    # the interleave as a gather: every piece's destination from the two offset arrays
    nm, nc = len(mode_jobs), len(coeff_jobs)
    mlen, clen = np.diff(moff.astype(np.int64)), np.diff(coff)
    # pieces in stream order: mode job i, then the coefficient jobs with coeff_after == i
    key = np.concatenate([2 * np.arange(nm), 2 * coeff_after + 1])
    order = np.argsort(key, kind="stable")
    lens = np.concatenate([mlen, clen])[order]
    src0 = np.concatenate([moff[:nm].astype(np.int64), len(mtok) + coff[:nc]])[order]
    dst0 = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(lens) else np.zeros(0, np.int64)
    total = int(lens.sum())
    idx = np.repeat(src0 - dst0, lens) + np.arange(total)
    tok = np.concatenate([mtok, ctok])[idx]
    cdf = np.array(cdf_init, np.uint16)
    by = ec_code_stream(tok, cdf)
    return by, cdf, tok


def ec_rate_batch(tokens, offsets, group_first, cdfs, group_cdf=None, init=None):
    """rv_ec_rate_batch over device or host arrays: tokens / offsets are
    DeviceBuffers or arrays (uploaded), the rest host arrays.  cdfs: (n_cdfs,
    rv_ec_cdf_total()) u16.  Returns (rates u32 per group, d_status[0], the
    snapshots as the device holds them after the call)."""
    def dev(x, dt):
        return x if isinstance(x, DeviceBuffer) else DeviceBuffer.from_array(np.asarray(x, dt))
    group_first = np.ascontiguousarray(group_first, np.int32)
    ng = len(group_first) - 1
    cdfs = np.ascontiguousarray(cdfs, np.uint16).reshape(-1, lib().rv_ec_cdf_total())
    dtok, doff = dev(tokens, np.uint32), dev(offsets, np.uint32)
    dgf, dcdf = DeviceBuffer.from_array(group_first), DeviceBuffer.from_array(cdfs)
    dgc = None if group_cdf is None else DeviceBuffer.from_array(
        np.ascontiguousarray(group_cdf, np.int32))
    dini = None if init is None else DeviceBuffer.from_array(
        np.ascontiguousarray(init, np.uint32))
    if (dgc is not None and dgc.nbytes != 4 * ng) or (dini is not None and dini.nbytes != 4 * ng):
        raise Rav1eHipError("ec_rate_batch: group_cdf / init need one entry per group")
    drate, dst = DeviceBuffer(4 * ng), DeviceBuffer(4)
    _check(lib().rv_ec_rate_batch(dtok.ptr, doff.ptr, dgf.ptr, ng, dcdf.ptr, len(cdfs),
                                  dgc.ptr if dgc else None, dini.ptr if dini else None,
                                  drate.ptr, dst.ptr, None), "rv_ec_rate_batch")
    _sync(None)
    return (drate.download(np.uint32, ng), int(dst.download(np.uint32)[0]),
            dcdf.download(np.uint16).reshape(cdfs.shape))


def coefficient_rates(jobs, coeffs, group_first, cdfs, xdec, ydec, group_cdf=None, init=None):
    """The real coefficient rate of every candidate (cost_coeffs of
    encode_tx_block under the RealRate RDO types, src/encoder.rs:1172-1190):
    the job list through the device tokenizer (as code_coefficients), then
    each group -- the jobs [group_first[g], group_first[g + 1]) -- through a
    counting writer on the device, with a private copy of snapshot
    group_cdf[g] (default 0) of cdfs that adapts inside the group and is
    dropped after it.  init: per group rng | (cnt & 0xFFFF) << 16 (default:
    fresh writers).  Returns (rates in 1 / 2**EC_BITRES bit, tokens,
    offsets)."""
    tk = _EcTokens(jobs, coeffs, xdec, ydec, "coefficient_rates")
    group_first = np.ascontiguousarray(group_first, np.int32)
    if len(group_first) < 1 or group_first[0] < 0 or group_first[-1] > tk.n or \
            np.any(np.diff(group_first) < 0):
        raise Rav1eHipError("coefficient_rates: group_first must ascend within the job list")
    rates, bad, _ = ec_rate_batch(tk.dtok, tk.doff, group_first, cdfs, group_cdf, init)
    if bad:
        raise Rav1eHipError(f"coefficient_rates: {bad} groups with a bad token or snapshot index")
    return rates, tk.tokens(), tk.offsets()


# ---- whole RDO candidates (rv_ec_rate.hip's stream kernel, rv_ec_cand.hip) ---
EC_CAND = np.dtype([("part", "<i4"), ("block", "<i4"), ("tx_first", "<i4"), ("tx_count", "<i4")])
_BSIZE_N4 = {3: 2, 6: 4, 9: 8, 12: 16}  # BLOCK_8X8 .. BLOCK_64X64 in luma 4x4 units


def ec_partition_gather(cdf, gather):
    """partition_gather_vert_alike (1) / _horz_alike (2) of one partition CDF
    (>= 10 u16): the x of the 2-entry CDF [x, 0], by the function the host
    coders and the device counter share."""
    cdf = np.ascontiguousarray(cdf, np.uint16)
    if cdf.size < 10:
        raise Rav1eHipError("ec_partition_gather: a partition CDF has 10 entries and a counter")
    x = lib().rv_ec_partition_gather(cdf.ctypes.data, int(gather))
    if x < 0:
        _check(int(x), "rv_ec_partition_gather")
    return int(x)


def _stream_groups(who, ng, cdfs_all, group_cdf, init):
    """The host-side preconditions of the mixed-stream counter."""
    total = lib().rv_ec_cdf_total_all()
    cdfs = np.ascontiguousarray(cdfs_all, np.uint16)
    if cdfs.size == 0 or cdfs.size % total or (cdfs.ndim > 1 and cdfs.shape[-1] != total):
        raise Rav1eHipError(f"{who}: snapshots are rv_ec_cdf_total_all() = {total} u16 wide")
    cdfs = cdfs.reshape(-1, total)
    gc = None if group_cdf is None else np.ascontiguousarray(group_cdf, np.int32).ravel()
    ini = None if init is None else np.ascontiguousarray(init, np.uint32).ravel()
    if (gc is not None and len(gc) != ng) or (ini is not None and len(ini) != ng):
        raise Rav1eHipError(f"{who}: group_cdf / init need one entry per group")
    return cdfs, gc, ini


def _upload_snapshots(cdfs, phase):
    """cdfs on the device, displaced by `phase` u16: (buffer, pointer)"""
    flat = np.concatenate([np.zeros(int(phase), np.uint16), cdfs.ravel()])
    buf = DeviceBuffer.from_array(flat)
    return buf, buf.ptr + 2 * int(phase)


def ec_rate_stream_batch(tokens, offsets, group_first, cdfs_all, group_cdf=None, init=None,
                         waves=None, cdf_phase=0):
    """rv_ec_rate_stream_batch: ec_rate_batch over the combined table and mixed
    tokens (symbols of both parts, raw bits, the frame-edge partition token).
    cdfs_all: (n_cdfs, rv_ec_cdf_total_all()) u16.  waves: groups per workgroup
    (1, 2, 4; None: the library's choice).  cdf_phase: u16 the snapshot table
    is displaced by on the device (its 16-byte phase).  Returns (rates u32 per
    group, d_status[0], the snapshots as the device holds them afterwards)."""
    def dev(x, dt):
        return x if isinstance(x, DeviceBuffer) else DeviceBuffer.from_array(np.asarray(x, dt))
    group_first = np.ascontiguousarray(group_first, np.int32)
    ng = len(group_first) - 1
    if ng < 0:
        raise Rav1eHipError("ec_rate_stream_batch: group_first needs n_groups + 1 entries")
    if waves not in (None, 1, 2, 4):
        raise Rav1eHipError("ec_rate_stream_batch: waves is 1, 2 or 4")
    cdfs, gc, ini = _stream_groups("ec_rate_stream_batch", ng, cdfs_all, group_cdf, init)
    dtok, doff = dev(tokens, np.uint32), dev(offsets, np.uint32)
    dgf = DeviceBuffer.from_array(group_first)
    dcdf, pcdf = _upload_snapshots(cdfs, cdf_phase)
    dgc = None if gc is None or ng == 0 else DeviceBuffer.from_array(gc)
    dini = None if ini is None or ng == 0 else DeviceBuffer.from_array(ini)
    drate, dst = DeviceBuffer(4 * max(ng, 1)), DeviceBuffer(4)
    args = (dtok.ptr, doff.ptr, dgf.ptr, ng, pcdf, len(cdfs), dgc.ptr if dgc else None,
            dini.ptr if dini else None, drate.ptr, dst.ptr)
    if waves is None:
        _check(lib().rv_ec_rate_stream_batch(*args, None), "rv_ec_rate_stream_batch")
    else:
        _check(lib().rv_ec_rate_stream_batch_waves(*args, int(waves), None),
               "rv_ec_rate_stream_batch")
    _sync(None)
    after = dcdf.download(np.uint16)[int(cdf_phase):].reshape(cdfs.shape)
    return drate.download(np.uint32, ng), int(dst.download(np.uint32)[0]), after


def _mode_job_record(x):
    if isinstance(x, np.void) or (isinstance(x, np.ndarray) and x.dtype == EC_MODE_JOB):
        return np.array(x, EC_MODE_JOB).reshape(-1)[0]
    return ec_mode_jobs(np.asarray(x, np.int64).reshape(1, -1))[0]


def pack_candidates(candidates, check=True):
    """candidates: (part, block, tx) triples.  part: the candidate's partition
    node (an EC_MODE_JOB record or row of kind 1, where the reference writes
    one: bsize >= BLOCK_8X8 && is_sqr) or None; block: its block (kind 0); tx:
    its transform blocks, code_coefficients' rows of kind 0 (luma then chroma
    in write_tx_tree / write_tx_blocks' order; none for a skip block).  Raises
    for a candidate without a block and, with check, where the reference would
    panic (check_mode_jobs) or a transform block lies outside its block.
    Returns (EC_CAND array, EC_MODE_JOB array, tx rows (k, 10), each row's tile)."""
    cands, mjobs, rows, tiles = [], [], [], []
    for i, cand in enumerate(candidates):
        if len(cand) != 3:
            raise Rav1eHipError(f"candidate {i}: (partition node or None, block, transform blocks)")
        part, block, tx = cand
        if block is None:
            raise Rav1eHipError(f"candidate {i} has no block")
        blk = _mode_job_record(block)
        if check and int(blk["kind"]) != 0:
            raise Rav1eHipError(f"candidate {i} has no block")
        pi = -1
        if part is not None:
            pi = len(mjobs)
            mjobs.append(_mode_job_record(part))
        bi = len(mjobs)
        mjobs.append(blk)
        tx = np.asarray(tx if tx is not None else [], np.int64).reshape(-1, 10)
        n4 = _BSIZE_N4.get(int(blk["bsize"]))
        if check and len(tx) and n4 is not None:
            bx, by = int(blk["bx"]), int(blk["by"])
            inside = (tx[:, 0] == 0) & (tx[:, 2] >= bx) & (tx[:, 2] < bx + n4) & \
                (tx[:, 3] >= by) & (tx[:, 3] < by + n4)
            if not inside.all() or int(blk["skip"]):
                raise Rav1eHipError(f"candidate {i}: transform jobs outside the block")
        cands.append((pi, bi, len(rows), len(tx)))
        rows += tx.tolist()
        tiles += [int(blk["tile"])] * len(tx)
    mj = np.array(mjobs, EC_MODE_JOB) if mjobs else np.zeros(0, EC_MODE_JOB)
    if check:
        check_mode_jobs(mj)
    return (np.array(cands, EC_CAND) if cands else np.zeros(0, EC_CAND), mj,
            np.array(rows, np.int64).reshape(-1, 10), np.array(tiles, np.int32))


class EcCodingState:
    """The coding state candidates are priced against: the neighbour-record
    map rv_ec_mode_tokenize and the coefficient-context map rv_ec_tokenize
    leave behind after the committed jobs (one tile list, code_tile's job
    formats; coefficient rows of kind 3 start the tiles in the mode jobs'
    `tile` order), and the coefficients on the device.  Candidates only read
    it.  Maps built from more blocks than those before a candidate give the
    same tokens, so one state serves a frame."""

    def __init__(self, mode_jobs, coeff_jobs, coeffs, params, xdec=1, ydec=1):
        mode_jobs = np.ascontiguousarray(mode_jobs, EC_MODE_JOB)
        self.params, self.xdec, self.ydec = params, int(xdec), int(ydec)
        dims = params.tile_dims
        self.ntiles = len(dims)
        _, _, bad, self.mode_map, (self.mw8, self.mh8), self.ddim = _ec_mode_tokenize(mode_jobs,
                                                                                      params)
        if bad:
            raise Rav1eHipError(f"EcCodingState: {bad} mode jobs outside the tokenizer's restrictions")
        # a 64x64 candidate at the last superblock may hang over the tile's edge
        cover = tuple(int(-(-int(dims[:, k].max()) // 16) * 16) for k in range(2))
        tk = _EcTokens(coeff_jobs, coeffs, self.xdec, self.ydec, "EcCodingState",
                       min_tiles=self.ntiles, min_map=cover)
        self.coef_map, self.mw4, self.mh4, self.co = tk.dmap, tk.mw, tk.mh, tk.co

    def mode_map_host(self):
        return self.mode_map.download(np.uint32)

    def coef_map_host(self):
        return self.coef_map.download(np.uint8)


def _run_candidates(who, state, candidates, check, rate_args):
    cands, mj, rows, tiles = pack_candidates(candidates, check)
    n, ntx = len(cands), len(rows)
    if rate_args is not None:
        cdfs, gc, ini = _stream_groups(who, n, *rate_args)
    ej = np.zeros(ntx, EC_JOB)
    for k, f in enumerate(["kind", "plane", "bx", "by", "tx_size", "tx_type", "is_inter", "bw_lg",
                           "bh_lg"]):
        ej[f] = rows[:, k]
    ej["tile"] = tiles
    ej["coeffs"] = state.co.ptr + 4 * rows[:, 9].astype(np.uint64)
    area = np.where((rows[:, 4] >= 0) & (rows[:, 4] <= 4), 16 << (2 * np.clip(rows[:, 4], 0, 3)), 0)
    cap = int(160 * n + 64 * ntx + 8 * int(area.sum()) + 1024)
    L = lib()
    dc = DeviceBuffer.from_array(cands) if n else None
    dm = DeviceBuffer.from_array(mj) if len(mj) else None
    dt = DeviceBuffer.from_array(ej) if ntx else None
    scr = DeviceBuffer(L.rv_ec_cand_scratch_bytes(n, ntx) + 16)
    doff, dtok, dst = DeviceBuffer(4 * (n + 1)), DeviceBuffer(4 * cap), DeviceBuffer(16)
    head = (dc.ptr if dc else None, n, dm.ptr if dm else None, len(mj), dt.ptr if dt else None, ntx,
            state.params.c_struct(), state.ntiles, state.ddim.ptr, state.xdec, state.ydec,
            state.mw4, state.mh4, state.coef_map.ptr, state.mw8, state.mh8, state.mode_map.ptr,
            scr.ptr, doff.ptr, dtok.ptr, cap)
    rates = None
    if rate_args is None:
        _check(L.rv_ec_cand_tokenize(*head, dst.ptr, None), "rv_ec_cand_tokenize")
    else:
        dcdf = DeviceBuffer.from_array(cdfs)
        dgc = None if gc is None or n == 0 else DeviceBuffer.from_array(gc)
        dini = None if ini is None or n == 0 else DeviceBuffer.from_array(ini)
        drate = DeviceBuffer(4 * max(n, 1))
        _check(L.rv_ec_cand_rates(*head, dcdf.ptr, len(cdfs), dgc.ptr if dgc else None,
                                  dini.ptr if dini else None, drate.ptr, dst.ptr, None),
               "rv_ec_cand_rates")
    _sync(None)
    status = dst.download(np.uint32)
    if status[1]:
        raise Rav1eHipError(f"{who}: token buffer overflow")
    if rate_args is not None:
        rates = drate.download(np.uint32, n)
    tok = dtok.download(np.uint32)[:int(status[0])]
    off = doff.download(np.uint32)[:n + 1]
    return rates, tok, off, int(status[2]), int(status[3]) if rate_args is not None else 0


def ec_tokenize_candidates(state, candidates, check=True):
    """rv_ec_cand_tokenize: every candidate's tokens (partition, pre_cdef, the
    mode symbols of post_cdef, the coefficient tokens) against an
    EcCodingState, which is not changed.  candidates: pack_candidates' triples,
    the transform rows' coeff_off into the state's coefficients.  check: raise
    where the reference would panic; without it the device counts such
    candidates.  Returns (tokens u32, offsets u32 [n + 1], rejected candidates)."""
    _, tok, off, rejected, _ = _run_candidates("ec_tokenize_candidates", state, candidates, check,
                                               None)
    return tok, off, rejected


def ec_candidate_rates(state, candidates, cdfs_all, group_cdf=None, init=None, check=True):
    """rv_ec_cand_rates against an EcCodingState: (rates, tokens, offsets,
    rejected candidates, counter groups that hit a bad token or snapshot)."""
    return _run_candidates("ec_candidate_rates", state, candidates, check,
                           (cdfs_all, group_cdf, init))


def candidate_rates(committed_mode_jobs, committed_coeff_jobs, coeffs, candidates, params, cdfs_all,
                    group_cdf=None, init=None, xdec=1, ydec=1):
    """What wr.tell_frac() - tell is in luma_chroma_mode_rdo (src/rdo.rs:689-768)
    for every candidate: the committed jobs build the two context maps
    (ec_tokenize_modes' and code_coefficients' job formats), each candidate's
    partition node, mode info and coefficients are tokenized against them and
    counted from a private copy of snapshot group_cdf[c] (default 0) of cdfs_all
    and the writer state init[c] (rng | (cnt & 0xFFFF) << 16; default fresh).
    coeffs: the coefficients of the committed and the candidates' transform
    rows.  Returns (rates in 1 / 2**EC_BITRES bit, tokens, offsets)."""
    cands = list(candidates)
    # the preconditions first: nothing below needs a device to refuse them
    pack_candidates(cands, True)
    _stream_groups("candidate_rates", len(cands), cdfs_all, group_cdf, init)
    state = EcCodingState(committed_mode_jobs, committed_coeff_jobs, coeffs, params, xdec, ydec)
    rates, tok, off, rejected, bad = ec_candidate_rates(state, cands, cdfs_all, group_cdf, init)
    if rejected or bad:
        raise Rav1eHipError(f"candidate_rates: {rejected} candidates outside the restrictions, "
                            f"{bad} groups with a bad token or snapshot index")
    return rates, tok, off


# ---- MV reference stacks of every block size (rv_mvstack.hip) ----------------
# rv_mv_blk, rv_mv_cand, rv_mvref_tile, rv_mvref_query, rv_mvref_result
MV_BLK = np.dtype([("ref", np.int8, 2), ("n4_w", np.uint8), ("n4_h", np.uint8), ("newmv", np.uint8),
                   ("pad", np.uint8, 3), ("mv", np.int16, (2, 2))])
MV_CAND = np.dtype([("this_mv", np.int16, 2), ("comp_mv", np.int16, 2), ("weight", np.uint32)])
MVREF_TILE = np.dtype([(n, np.int32) for n in ("cols", "rows", "mi_x", "mi_y")])
MVREF_QUERY = np.dtype([("tile", np.int32), ("bx", np.int32), ("by", np.int32), ("bw4", np.int32),
                        ("bh4", np.int32), ("ref", np.int32, 2), ("reserved", np.int32)])
MVREF_RESULT = np.dtype([("mode_context", np.int32), ("n", np.int32), ("stack", MV_CAND, 9)])
MVREF_MAX_TILES = 1024


def default_block_grid(n_tiles, grid_h, grid_w):
    """Block::default() in every cell (src/context.rs:1425-1442): intra, 64x64."""
    g = np.zeros((n_tiles, grid_h, grid_w), MV_BLK)
    g["n4_w"] = g["n4_h"] = 16
    return g


def _sign_bias_mask(sign_bias):
    if isinstance(sign_bias, (int, np.integer)):
        m = int(sign_bias)
    else:
        m = sum(1 << i for i, b in enumerate(sign_bias) if b)
    if not 0 <= m < 128:
        raise Rav1eHipError("sign_bias: seven references' bits (RefType 1..7)")
    return m


class BlockGrid:
    """Per-tile grids of MV_BLK records in device memory, with the tiles and
    the frame they belong to (rv_mvref_geom).  tiles: rows of (cols, rows,
    mi_x, mi_y) in 4x4 units; grid_w / grid_h default to the largest tile
    rounded up to whole superblocks; frame_cols / frame_rows to the extent of
    the tiles."""

    def __init__(self, tiles, frame_cols=None, frame_rows=None, sign_bias=0, grid_w=None,
                 grid_h=None):
        t = np.asarray(tiles)
        if t.dtype != MVREF_TILE:
            t = np.ascontiguousarray(t, np.int32).reshape(-1, 4).view(MVREF_TILE).reshape(-1)
        self.tiles = np.ascontiguousarray(t)
        nt = len(self.tiles)
        if not 1 <= nt <= MVREF_MAX_TILES:
            raise Rav1eHipError(f"BlockGrid: {nt} tiles (1..{MVREF_MAX_TILES})")
        if (self.tiles["cols"].min() < 1 or self.tiles["rows"].min() < 1 or
                self.tiles["mi_x"].min() < 0 or self.tiles["mi_y"].min() < 0):
            raise Rav1eHipError("BlockGrid: an empty tile or a negative origin")
        up16 = lambda v: (int(v) + 15) // 16 * 16  # noqa: E731
        self.grid_w = up16(self.tiles["cols"].max()) if grid_w is None else int(grid_w)
        self.grid_h = up16(self.tiles["rows"].max()) if grid_h is None else int(grid_h)
        if (self.grid_w % 16 or self.grid_h % 16 or self.grid_w < self.tiles["cols"].max() or
                self.grid_h < self.tiles["rows"].max()):
            raise Rav1eHipError("BlockGrid: grid_w / grid_h a multiple of 16 that holds every tile")
        ex = int((self.tiles["mi_x"] + self.tiles["cols"]).max())
        ey = int((self.tiles["mi_y"] + self.tiles["rows"]).max())
        self.frame_cols = ex if frame_cols is None else int(frame_cols)
        self.frame_rows = ey if frame_rows is None else int(frame_rows)
        self.sign_bias = _sign_bias_mask(sign_bias)
        self.rejected = 0
        self.dtiles = DeviceBuffer.from_array(self.tiles)
        self.buf = DeviceBuffer(nt * self.grid_h * self.grid_w * MV_BLK.itemsize)

    @property
    def shape(self):
        return (len(self.tiles), self.grid_h, self.grid_w)

    def geom(self):
        return RvMvrefGeom(len(self.tiles), self.grid_w, self.grid_h, self.frame_cols,
                           self.frame_rows, self.sign_bias)

    @classmethod
    def from_array(cls, cells, tiles, **kw):
        """A grid the host painted: cells (n_tiles, grid_h, grid_w) MV_BLK."""
        cells = np.ascontiguousarray(cells, MV_BLK)
        if cells.ndim == 2:
            cells = cells[None]
        g = cls(tiles, grid_w=cells.shape[2], grid_h=cells.shape[1], **kw)
        if cells.shape != g.shape:
            raise Rav1eHipError(f"BlockGrid.from_array: cells {cells.shape}, tiles want {g.shape}")
        g.buf.upload(cells)
        return g

    def download(self):
        return self.buf.download(MV_BLK).reshape(self.shape)


def paint_block_grid(jobs, tiles, frame_cols=None, frame_rows=None, sign_bias=0, grid_w=None,
                     grid_h=None):
    """rv_mvref_grid_paint: the blocks (kind 0) of a coding-order EC_MODE_JOB
    list painted into per-tile grids of MV_BLK, every other cell
    Block::default(); where jobs overlap, the later one wins.  Returns the
    device-resident BlockGrid; .rejected counts the jobs that painted nothing
    (outside their tile, a 128 size, bad references or MVs)."""
    jobs = np.ascontiguousarray(jobs, EC_MODE_JOB)
    g = BlockGrid(tiles, frame_cols, frame_rows, sign_bias, grid_w, grid_h)
    n = len(jobs)
    if n == 0:
        g.buf.upload(default_block_grid(*g.shape))
        return g
    dj = DeviceBuffer.from_array(jobs)
    scr = DeviceBuffer(lib().rv_mvref_paint_scratch_bytes(g.geom()))
    dst = DeviceBuffer(4)
    _check(lib().rv_mvref_grid_paint(dj.ptr, n, g.geom(), g.dtiles.ptr, g.buf.ptr, scr.ptr, dst.ptr,
                                     None), "rv_mvref_grid_paint")
    _sync(None)
    g.rejected = int(dst.download(np.uint32)[0])
    return g


def mvref_queries(rows):
    """(n, 7) integers (tile, bx, by, bw4, bh4, ref0, ref1) as MVREF_QUERY."""
    rows = np.asarray(rows, np.int64).reshape(-1, 7)
    q = np.zeros(len(rows), MVREF_QUERY)
    for k, f in enumerate(("tile", "bx", "by", "bw4", "bh4")):
        q[f] = rows[:, k]
    q["ref"] = rows[:, 5:7]
    return q


def find_mvrefs_batch(grid, queries, results=None):
    """rv_find_mvrefs_batch: find_mvrefs (src/context.rs:2943-2965) of every
    query against a BlockGrid in one launch.  queries: MVREF_QUERY, or rows for
    mvref_queries.  results: an MVREF_RESULT array the output starts from (a
    rejected query leaves its slot as it was; default zeros).  Returns
    (mode_context [n], length [n], stacks [n, 9] MV_CAND, rejected count)."""
    q = np.asarray(queries)
    q = np.ascontiguousarray(q) if q.dtype == MVREF_QUERY else mvref_queries(q)
    n = len(q)
    res = np.zeros(n, MVREF_RESULT) if results is None else np.ascontiguousarray(results,
                                                                                 MVREF_RESULT)
    if len(res) != n:
        raise Rav1eHipError("find_mvrefs_batch: one result slot per query")
    if n == 0:
        return res["mode_context"], res["n"], res["stack"], 0
    dq, dr, dst = DeviceBuffer.from_array(q), DeviceBuffer.from_array(res), DeviceBuffer(4)
    _check(lib().rv_find_mvrefs_batch(dq.ptr, n, grid.geom(), grid.dtiles.ptr, grid.buf.ptr, dr.ptr,
                                      dst.ptr, None), "rv_find_mvrefs_batch")
    _sync(None)
    res = dr.download(MVREF_RESULT, n)
    return res["mode_context"], res["n"], res["stack"], int(dst.download(np.uint32)[0])


def ec_fill_mode_stacks(jobs, grid, check=True, info=None):
    """rv_ec_mode_fill_stacks: mode_context, num_mv_found, weight and ref_mv of
    every inter block of an EC_MODE_JOB list from the MV stacks of a BlockGrid
    (the jobs' own, or the committed blocks' for a candidate list).  Returns
    (the filled jobs, stack_mvs (n, 4, 2): the first four entries' this_mv
    (row, col), what check_mode_jobs and ec_tokenize_modes take).  check: raise
    when an inter job was rejected (an unsupported size, a position outside
    its tile, bad references) instead of leaving it unfilled.  info: a dict
    that receives "rejected" and "stacks" (the full MVREF_RESULT of every
    filled job)."""
    jobs = np.ascontiguousarray(jobs, EC_MODE_JOB)
    n = len(jobs)
    full, rejected = np.zeros(n, MVREF_RESULT), 0
    filled = jobs.copy()
    if n:
        dj, ds, dst = DeviceBuffer.from_array(jobs), DeviceBuffer.from_array(full), DeviceBuffer(4)
        _check(lib().rv_ec_mode_fill_stacks(dj.ptr, n, grid.geom(), grid.dtiles.ptr, grid.buf.ptr,
                                            ds.ptr, dst.ptr, None), "rv_ec_mode_fill_stacks")
        _sync(None)
        filled = dj.download(EC_MODE_JOB, n)
        full = ds.download(MVREF_RESULT, n)
        rejected = int(dst.download(np.uint32)[0])
    if info is not None:
        info["rejected"], info["stacks"] = rejected, full
    if check and rejected:
        raise Rav1eHipError(f"ec_fill_mode_stacks: {rejected} inter jobs outside the supported "
                            "sizes, their tile or the reference codes")
    return filled, full["stack"]["this_mv"][:, :4].astype(np.int32)


# ---- the inter front of rdo_mode_decision (rv_inter.hip) ----------------------
# rv_inter_cand, rv_inter_list, rv_inter_blk, rv_inter_mc_job; an MV is (row, col)
INTER_MAX_CANDS = 20  # RV_INTER_MAX_CANDS
INTER_CAND = np.dtype([("luma_mode", "<i4"), ("set", "<i4"), ("ref", "<i4", 2),
                       ("mv", "<i2", (2, 2)), ("mode_context", "<i4")])
INTER_LIST = np.dtype([("n", "<i4"), ("cand", INTER_CAND, INTER_MAX_CANDS)])
INTER_BLK = np.dtype([("tile", "<i4"), ("bo_x", "<i4"), ("bo_y", "<i4")])
INTER_MC_JOB = np.dtype([("tile", "<i4"), ("bo_x", "<i4"), ("bo_y", "<i4"), ("dst_set", "<i4"),
                         ("ref_slot", "<i4", 2), ("mv", "<i2", (2, 2))])


def _check_code(rc, what):
    if rc != RV_OK:
        err = Rav1eHipError(f"{what} failed ({rc}): {lib().rv_last_error().decode()}")
        err.code = rc
        raise err


def inter_ref_sets(allowed, ref_frames, compound_allowed, bsize) -> RvInterRefSets:
    """rv_inter_ref_sets_build (src/rdo.rs:815-835, 914-927): the single
    reference sets of rdo_mode_decision -- allowed: RefType codes 1..7 in
    InterConfig::allowed_ref_frames() order, ref_frames: fi.ref_frames, the
    seven RefTypes' DPB slots -- with LAST3_FRAME skipped and one set per
    distinct slot, the first forward / backward set, and whether the compound
    set follows (compound_allowed: reference_mode != SINGLE).  Raises with
    the library's code (Rav1eHipError.code) on bad arguments."""
    al = np.ascontiguousarray(allowed, np.int32).reshape(-1)
    rf = np.ascontiguousarray(ref_frames, np.int32).reshape(-1)
    if len(rf) != 7:
        raise Rav1eHipError("inter_ref_sets: ref_frames has seven slots")
    out = RvInterRefSets()
    _check_code(lib().rv_inter_ref_sets_build(al.ctypes.data, len(al), rf.ctypes.data,
                                              1 if compound_allowed else 0, int(bsize),
                                              C.byref(out)), "rv_inter_ref_sets_build")
    return out


def inter_mode_set_batch(stacks, me, sets: RvInterRefSets, include_near_mvs=False, blocks=None):
    """rv_inter_mode_set_batch: the inter mode set of src/rdo.rs:858-986 with
    every candidate's MVs for n blocks in one launch.  stacks: MVREF_RESULT
    (n, sets.n_sets) as find_mvrefs_batch wrote them per reference set (the
    compound query last); me: (n, sets.n_single, 2) int16 (row, col), the
    searches' MVs, or the DeviceBuffer motion_estimation_batch(device=True)
    returned; blocks: INTER_BLK [n] when the MC jobs are wanted.  Returns
    (lists INTER_LIST [n], mc_jobs INTER_MC_JOB (n, 20) or None, rejected):
    rejected blocks (a list above 20 entries, an empty compound stack: the
    reference panics on both) have n = 0 and no jobs."""
    who = "inter_mode_set_batch"
    st = np.ascontiguousarray(stacks, MVREF_RESULT)
    ns, nsets = sets.n_single, sets.n_sets
    st = st.reshape(-1, nsets) if st.size else st.reshape(0, nsets)
    n = len(st)
    if isinstance(me, DeviceBuffer):  # motion_estimation_batch(device=True): no host copy
        if me.nbytes < n * ns * 4:
            raise Rav1eHipError(f"{who}: the device me holds fewer than {n} x {ns} MVs")
        mv = None
    else:
        mv = np.ascontiguousarray(me, np.int16)
        if mv.size != n * ns * 2:
            raise Rav1eHipError(f"{who}: me is (n, {ns}, 2) for {n} blocks")
    lists = np.zeros(n, INTER_LIST)
    blk = None
    if blocks is not None:
        blk = np.ascontiguousarray(blocks, INTER_BLK).reshape(-1)
        if len(blk) != n:
            raise Rav1eHipError(f"{who}: one INTER_BLK per block")
    if n == 0:
        return lists, (np.zeros((0, INTER_MAX_CANDS), INTER_MC_JOB) if blk is not None else None), 0
    ds, dm, dl, dst = DeviceBuffer.from_array(st), me if mv is None else DeviceBuffer.from_array(mv), \
        DeviceBuffer(lists.nbytes), DeviceBuffer(4)
    db = DeviceBuffer.from_array(blk) if blk is not None else None
    dj = DeviceBuffer(n * INTER_MAX_CANDS * INTER_MC_JOB.itemsize) if blk is not None else None
    _check_code(lib().rv_inter_mode_set_batch(ds.ptr, dm.ptr, db.ptr if db else None, n, sets,
                                              1 if include_near_mvs else 0, dl.ptr,
                                              dj.ptr if dj else None, dst.ptr, None),
                "rv_inter_mode_set_batch")
    _sync(None)
    lists = dl.download(INTER_LIST, n)
    jobs = dj.download(INTER_MC_JOB, n * INTER_MAX_CANDS).reshape(n, INTER_MAX_CANDS) if dj else None
    return lists, jobs, int(dst.download(np.uint32)[0])


def _plane_sets(who, sets, count):
    """Sequences of plane sets (3 DevicePlanes each, `count` of them used) as
    the library's [n][3] rv_plane table."""
    sets = list(sets)
    arr = (RvPlane * (3 * max(1, len(sets))))()
    for s, ps in enumerate(sets):
        if len(ps) < count:
            raise Rav1eHipError(f"{who}: a plane set needs {count} plane(s)")
        for p in range(count):
            arr[3 * s + p] = ps[p].desc
    return arr, len(sets)


def motion_compensate_batch(refs, dsts, tiles, jobs, bsize, filter_mode=FilterMode.REGULAR,
                            luma_only=False, bit_depth=8, lanes=0):
    """rv_motion_compensate_batch: motion_compensate (src/encoder.rs:1239-1430)
    through predict_inter (src/predict.rs:255-338) for n jobs of one bsize and
    every coded plane in one launch.  refs: the reference plane sets a job's
    ref_slot indexes, dsts: the destination sets its dst_set indexes (each set
    three DevicePlanes, one with luma_only); tiles INTRA_TILE; jobs
    INTER_MC_JOB (tile, tile_bo in 4x4 luma units, dst_set, ref_slot --
    ref_slot[1] < 0: single reference -- and the MVs as (row, col)).  Jobs with
    tile < 0 are skipped.  lanes: the lanes that share a job (0: the default
    of the size).  Returns the number of rejected jobs (an index out of range,
    a block not aligned to its size or outside its tile); they write nothing."""
    who = "motion_compensate_batch"
    tiles = np.ascontiguousarray(tiles, dtype=INTRA_TILE).reshape(-1)
    jobs = np.ascontiguousarray(jobs, dtype=INTER_MC_JOB).reshape(-1)
    count = 1 if luma_only else 3
    ra, nr = _plane_sets(who, refs, count)
    da, nd = _plane_sets(who, dsts, count)
    if nr == 0 or nd == 0:
        raise Rav1eHipError(f"{who}: at least one reference set and one destination set")
    prm = RvInterMcParams(int(bsize), int(filter_mode), 1 if luma_only else 0, int(bit_depth))
    n = len(jobs)
    dt, dj, dst = DeviceBuffer.from_array(tiles), DeviceBuffer.from_array(jobs), DeviceBuffer(4)
    _check_code(lib().rv_motion_compensate_batch_lanes(ra, nr, da, nd, dt.ptr, len(tiles), dj.ptr,
                                                       n, C.byref(prm), dst.ptr, int(lanes), None),
                "rv_motion_compensate_batch")
    _sync(None)
    return int(dst.download(np.uint32)[0])


# ---- motion estimation of rdo_mode_decision (rv_motion_est.hip) -------------
ME_SAVE_JOB = np.dtype([("tile", "<i4"), ("bo_x", "<i4"), ("bo_y", "<i4"), ("bsize", "<i4"),
                        ("ref_index", "<i4"), ("mv", "<i2", 2)])  # rv_me_save_job


def me_lambda_u32(me_lambda) -> int:
    """(fi.me_lambda * 256.0 * 0.5) as u32 (src/me.rs:207), formed in f64; `as`
    truncates and saturates."""
    v = float(me_lambda) * 256.0 * 0.5
    if not v > 0.0:  # NaN and negatives
        return 0
    return min(int(v), 0xFFFFFFFF)


def me_pmv_index(bsize, bo_x, bo_y) -> int:
    """rv_me_pmv_index: pmv_idx of src/rdo.rs:1532-1536 / src/encoder.rs:
    2160-2166 for the block at tile block offset (bo_x, bo_y): 0 above 32x32,
    else ((bo_x & 32) >> 5) + ((bo_y & 32) >> 4) + 1."""
    r = lib().rv_me_pmv_index(int(bsize), int(bo_x), int(bo_y))
    if r < 0:
        raise Rav1eHipError("me_pmv_index: no BlockSize, or a 4:1 / 1:4 size")
    return r


def _me_field(who, a, w_in_b, h_in_b):
    """A motion field [7][h_in_b][w_in_b] of (row, col) on the device."""
    if isinstance(a, DeviceBuffer):
        if a.nbytes < 7 * h_in_b * w_in_b * 4:
            raise Rav1eHipError(f"{who}: a device field holds fewer than 7 x {h_in_b} x {w_in_b} MVs")
        return a
    a = np.ascontiguousarray(a, np.int16)
    if a.shape != (7, h_in_b, w_in_b, 2):
        raise Rav1eHipError(f"{who}: a field is (7, {h_in_b}, {w_in_b}, 2) int16, got {a.shape}")
    return DeviceBuffer.from_array(a)


def motion_estimation_batch(org: DevicePlane, refs, tiles, blocks, sets: RvInterRefSets, stacks,
                            cmv, tile_mvs, prev_mvs, bsize, w_in_b, h_in_b, lambda_,
                            use_satd=True, allow_hp=False, bit_depth=8, device=False):
    """rv_motion_estimation_batch: DiamondSearch::motion_estimation (src/me.rs:
    193-278) of rdo_mode_decision (src/rdo.rs:858-878) for n blocks of one bsize
    x the sets.n_single single reference sets, in one launch: pmv pair from the
    stacks, MV range, get_subset_predictors, the full-pel and the sub-pel
    diamond, all on the device.

    org: the source luma DevicePlane; refs: the reference plane sets of
    motion_compensate_batch (set sets.slot[i] is searched for single set i,
    plane 0 only); tiles INTRA_TILE; blocks INTER_BLK [n]; stacks MVREF_RESULT
    (n, sets.n_sets) as find_mvrefs_batch wrote them, or a DeviceBuffer of
    them; cmv (n, n_single, 2) int16 (row, col): pmvs[ref_slot]
    .unwrap_or_default() (rdo.rs:867); tile_mvs / prev_mvs: (7, h_in_b, w_in_b,
    2) int16 fields (ts.mvs, and frame_mvs of the frame in fi.ref_frames[0]'s
    slot) or DeviceBuffers; prev_mvs None: that slot is empty.  lambda_:
    me_lambda_u32(fi.me_lambda).

    The fields are a snapshot: every item of the batch reads the same one.
    Coding order is the caller's schedule, and so is the rule of
    rdo.rs:872-876: after the search of a 32x32 or 64x64 block (and not under
    encode_bottomup) the caller sets pmvs[ref_slot] = Some(b_me), which the
    cmv of later calls must carry.

    Returns (me, res, rejected): me (n, n_single, 2) int16, or with
    device=True the DeviceBuffer inter_mode_set_batch takes as it is; res
    FS_RESULT (n, n_single) (the MV and the final cost); rejected items (a bad
    tile, offset or stack length) write nothing and leave zeros."""
    who = "motion_estimation_batch"
    tiles = np.ascontiguousarray(tiles, dtype=INTRA_TILE).reshape(-1)
    blk = np.ascontiguousarray(blocks, INTER_BLK).reshape(-1)
    n, ns, nsets = len(blk), sets.n_single, sets.n_sets
    ra, nr = _plane_sets(who, refs, 1)
    if nr == 0:
        raise Rav1eHipError(f"{who}: at least one reference set")
    if isinstance(stacks, DeviceBuffer):
        dstk = stacks
        if dstk.nbytes < n * nsets * MVREF_RESULT.itemsize:
            raise Rav1eHipError(f"{who}: the device stacks hold fewer than {n} x {nsets} records")
    else:
        st = np.ascontiguousarray(stacks, MVREF_RESULT)
        if st.size != n * nsets:
            raise Rav1eHipError(f"{who}: stacks is (n, {nsets}) for {n} blocks")
        dstk = DeviceBuffer.from_array(st)
    cm = np.ascontiguousarray(cmv, np.int16)
    if cm.size != n * ns * 2:
        raise Rav1eHipError(f"{who}: cmv is (n, {ns}, 2) for {n} blocks")
    dtm = _me_field(who, tile_mvs, w_in_b, h_in_b)
    dpm = _me_field(who, prev_mvs, w_in_b, h_in_b) if prev_mvs is not None else None
    prm = RvMeParams(int(bsize), int(bit_depth), 1 if use_satd else 0, 1 if allow_hp else 0,
                     int(w_in_b), int(h_in_b), int(lambda_), 0)
    dt, db, dc = DeviceBuffer.from_array(tiles), DeviceBuffer.from_array(blk), \
        DeviceBuffer.from_array(cm)
    dme, dres, dst = DeviceBuffer(n * ns * 4), DeviceBuffer(n * ns * 16), DeviceBuffer(4)
    dme.zero()
    dres.zero()
    _check_code(lib().rv_motion_estimation_batch(
        C.byref(org.desc), ra, nr, dt.ptr, len(tiles), db.ptr, n, sets, dstk.ptr, dc.ptr, dtm.ptr,
        dpm.ptr if dpm else None, C.byref(prm), dme.ptr, dres.ptr, dst.ptr, None),
        "rv_motion_estimation_batch")
    _sync(None)
    res = dres.download(FS_RESULT, n * ns).reshape(n, ns)
    me = dme if device else dme.download(np.int16, n * ns * 2).reshape(n, ns, 2)
    return me, res, int(dst.download(np.uint32)[0])


def save_block_motion_batch(jobs, tiles, tile_mvs, w_in_b, h_in_b):
    """rv_save_block_motion_batch: save_block_motion (src/encoder.rs:1432-1444)
    of a coding-order ME_SAVE_JOB list (tile, tile block offset, bsize,
    ref_index = RefType.to_index(), mv (row, col)) into the field tile_mvs
    ((7, h_in_b, w_in_b, 2) int16, or a DeviceBuffer that is updated in place):
    each rectangle clipped to its tile's mi_width / mi_height, a later job
    winning over an earlier one, ref_index < 0 (an intra winner) skipped.
    Returns (the field's DeviceBuffer, rejected)."""
    who = "save_block_motion_batch"
    tiles = np.ascontiguousarray(tiles, dtype=INTRA_TILE).reshape(-1)
    jobs = np.ascontiguousarray(jobs, ME_SAVE_JOB).reshape(-1)
    dtm = _me_field(who, tile_mvs, w_in_b, h_in_b)
    scr = DeviceBuffer(lib().rv_save_block_motion_scratch_bytes(int(w_in_b), int(h_in_b)))
    dj, dt, dst = DeviceBuffer.from_array(jobs), DeviceBuffer.from_array(tiles), DeviceBuffer(4)
    _check_code(lib().rv_save_block_motion_batch(dj.ptr, len(jobs), dt.ptr, len(tiles), int(w_in_b),
                                                 int(h_in_b), dtm.ptr, scr.ptr, dst.ptr, None),
                "rv_save_block_motion_batch")
    _sync(None)
    return dtm, int(dst.download(np.uint32)[0])


# ---- a block's mode decision (rv_mode_decide.hip) ---------------------------
class Tune(enum.IntEnum):
    """Tune (src/api/config/encoder.rs): RV_TUNE_*."""
    Psnr = 0
    Psychovisual = 1


MODE_CAND_SKIP, MODE_CAND_INTRA, MODE_CAND_NEED_RECON_PIXEL = 1, 2, 4  # RV_MODE_CAND_*
(MODE_STATE_NONE, MODE_STATE_EVALUATED, MODE_STATE_GATED_ZERO_DIST, MODE_STATE_GATED_SKIP,
 MODE_STATE_REJECTED) = range(5)  # RV_MODE_STATE_*
MODE_PAYLOAD = np.dtype([("luma_mode", "<i4"), ("chroma_mode", "<i4"), ("ref_frames", "<i4", 2),
                         ("mvs", "<i2", (2, 2)), ("tx_type", "<i4"), ("sidx", "<i4"),
                         ("alpha_u", "<i4"), ("alpha_v", "<i4")])
MODE_CAND = np.dtype([("group", "<i4"), ("flags", "<i4"), ("set", "<i4"), ("rate", "<u4"),
                      ("tx_size", "<i4"), ("dist_off", "<i4"), ("eob_off", "<i4"),
                      ("pay", MODE_PAYLOAD)])
MODE_BLOCK = np.dtype([("tile", "<i4"), ("bo_x", "<i4"), ("bo_y", "<i4"), ("cand_first", "<i4"),
                       ("cand_count", "<i4")])
MODE_DECISION = np.dtype([("rd_cost", "<f8"), ("distortion", "<u8"), ("rate", "<u4"),
                          ("cand", "<i4"), ("skip", "<i4"), ("has_coeff", "<i4"),
                          ("tx_size", "<i4"), ("reserved", "<i4"), ("pay", MODE_PAYLOAD)])
RD_COST_MAX = float(np.finfo(np.float64).max)  # f64::MAX, PartitionParameters::default()


class RvModeDecideParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("bsize", "bit_depth", "tune", "use_tx_domain_distortion",
                                         "coeff_rate", "w_in_b", "h_in_b", "w_imp")] + \
               [("lambda_", C.c_double), ("dist_scale", C.c_double * 3)]


class ModeDecision(typing.NamedTuple):
    """PartitionParameters as rdo_mode_decision returns them (src/rdo.rs:
    1244-1258), from one MODE_DECISION record: `cand` is the winner's index in
    the launch's candidate list, -1 when none of them won."""
    cand: int
    rd_cost: float
    distortion: int
    rate: int
    skip: bool
    has_coeff: bool
    pred_mode_luma: int
    pred_mode_chroma: int
    ref_frames: tuple
    mvs: tuple
    tx_size: int
    tx_type: int
    sidx: int
    pred_cfl_params: tuple

    @classmethod
    def from_record(cls, r):
        p = r["pay"]
        return cls(int(r["cand"]), float(r["rd_cost"]), int(r["distortion"]), int(r["rate"]),
                   bool(r["skip"]), bool(r["has_coeff"]), int(p["luma_mode"]), int(p["chroma_mode"]),
                   tuple(int(v) for v in p["ref_frames"]),
                   tuple((int(m[0]), int(m[1])) for m in p["mvs"]), int(r["tx_size"]),
                   int(p["tx_type"]), int(p["sidx"]), (int(p["alpha_u"]), int(p["alpha_v"])))


class ModeDecideResult(typing.NamedTuple):
    decisions: np.ndarray   # MODE_DECISION [n]
    cand_dist: np.ndarray   # u64 [n_cands]
    cand_cost: np.ndarray   # f64 [n_cands]
    cand_state: np.ndarray  # i32 [n_cands], MODE_STATE_*
    rejected_blocks: int
    rejected_cands: int

    def decision(self, i) -> ModeDecision:
        return ModeDecision.from_record(self.decisions[i])


def segmentation_data(base_q_idx) -> np.ndarray:
    """rv_segmentation_data: segmentation_optimize's ALT_Q deltas of the three
    segments (src/segmentation.rs:29-48) as int16 [3]."""
    out = np.zeros(3, np.int16)
    _check_code(lib().rv_segmentation_data(int(base_q_idx), out.ctypes.data), "rv_segmentation_data")
    return out


def _importance_plane(who, importance, w_in_b, h_in_b):
    if importance is None:
        return None, 0
    imp = np.ascontiguousarray(importance, np.float32)
    if imp.ndim != 2 or imp.shape[1] < (int(w_in_b) + 1) // 2 or imp.shape[0] < (int(h_in_b) + 1) // 2:
        err = Rav1eHipError(f"{who}: importance is [ceil(h_in_b / 2)][ceil(w_in_b / 2)] at least")
        err.code = RV_EINVAL
        raise err
    return imp, imp.shape[1]


def block_segments_batch(tiles, blocks, bsize, base_q_idx, w_in_b, h_in_b, importance=None,
                         data=None):
    """rv_block_segment_batch: per block of one bsize compute_mean_importance
    (src/rdo.rs:477-493), the heuristic segment index of luma_chroma_mode_rdo
    with quantizer_rdo off (:655-679) and get_qidx (src/encoder.rs:1061-1072).
    blocks: MODE_BLOCK (tile, bo_x, bo_y); importance: fi.block_importances as
    a 2-D float32 array, None: all zero; data: the ALT_Q deltas (default
    segmentation_data(base_q_idx)).  Returns (sidx i32 [n], qindex i32 [n],
    mean f32 [n], rejected)."""
    who = "block_segments_batch"
    tiles = np.ascontiguousarray(tiles, dtype=INTRA_TILE).reshape(-1)
    blocks = np.ascontiguousarray(blocks, dtype=MODE_BLOCK).reshape(-1)
    n = len(blocks)
    dq = np.ascontiguousarray(segmentation_data(base_q_idx) if data is None else data, np.int16)
    if dq.shape != (3,):
        raise Rav1eHipError(f"{who}: data has three deltas")
    imp, w_imp = _importance_plane(who, importance, w_in_b, h_in_b)
    if int(bsize) < 0 or int(bsize) > 21 or int(bsize) > 12 or not 0 <= int(base_q_idx) <= 255 or \
            int(w_in_b) < 1 or int(h_in_b) < 1:
        # the library's own codes, without a device: nothing is allocated
        _check_code(lib().rv_block_segment_batch(None, 0, None, 0, int(bsize), int(base_q_idx),
                                                 dq.ctypes.data, None, w_imp, int(w_in_b), int(h_in_b),
                                                 None, None, None, dq.ctypes.data, None),
                    "rv_block_segment_batch")
    dt, db, dst = DeviceBuffer.from_array(tiles), DeviceBuffer.from_array(blocks), DeviceBuffer(4)
    di = DeviceBuffer.from_array(imp) if imp is not None else None
    ds, dqi, dm = DeviceBuffer(4 * max(1, n)), DeviceBuffer(4 * max(1, n)), DeviceBuffer(4 * max(1, n))
    _check_code(lib().rv_block_segment_batch(dt.ptr, len(tiles), db.ptr, n, int(bsize),
                                             int(base_q_idx), dq.ctypes.data, di.ptr if di else None,
                                             w_imp, int(w_in_b), int(h_in_b), ds.ptr, dqi.ptr, dm.ptr,
                                             dst.ptr, None), "rv_block_segment_batch")
    _sync(None)
    return ds.download(np.int32, n), dqi.download(np.int32, n), dm.download(np.float32, n), \
        int(dst.download(np.uint32)[0])


def mode_decide_batch(src, cand_sets, tiles, blocks, cands, bsize, lambda_, dist_scale, w_in_b, h_in_b,
                      importance=None, tune=Tune.Psnr, use_tx_domain_distortion=False,
                      coeff_rate=True, bit_depth=8, tx_dist=None, tx_eob=None, seed=None, commit=None,
                      lanes=0) -> ModeDecideResult:
    """rv_mode_decide_batch: the end of rdo_mode_decision (src/rdo.rs:784-1259)
    for n blocks of one bsize in one launch -- every candidate's
    ScaledDistortion (compute_distortion :338-411 / compute_tx_distortion
    :414-475) and compute_rd_cost (:563-568), the walk with the reference's
    early-outs, the winner.  src: three DevicePlanes; cand_sets: the plane sets
    a candidate's `set` indexes (as motion_compensate_batch's dsts); tiles
    INTRA_TILE; blocks MODE_BLOCK; cands MODE_CAND in the reference's order of
    evaluation; tx_dist (u64) / tx_eob (u32): the concatenated rows of
    tx_blocks_batch's distortions and eobs that dist_off / eob_off index;
    importance: fi.block_importances (2-D float32) or None; seed: MODE_DECISION
    [n] to continue from (the CfL trial); commit: three DevicePlanes that
    receive the winners' pixels.  Argument errors raise with the library's code
    (Rav1eHipError.code) before anything is allocated on a device."""
    who = "mode_decide_batch"
    tiles = np.ascontiguousarray(tiles, dtype=INTRA_TILE).reshape(-1)
    blocks = np.ascontiguousarray(blocks, dtype=MODE_BLOCK).reshape(-1)
    cands = np.ascontiguousarray(cands, dtype=MODE_CAND).reshape(-1)
    n, nc = len(blocks), len(cands)
    for name, ps in (("src", src), ("commit", commit)):
        if ps is not None and len(ps) < 3:
            raise Rav1eHipError(f"{who}: {name} needs 3 planes")
    sa = _plane_set(src, 3)
    ca, ns = _plane_sets(who, cand_sets, 3)
    ma = _plane_set(commit, 3)
    imp, w_imp = _importance_plane(who, importance, w_in_b, h_in_b)
    prm = RvModeDecideParams(int(bsize), int(bit_depth), int(tune), 1 if use_tx_domain_distortion else 0,
                             1 if coeff_rate else 0, int(w_in_b), int(h_in_b), int(w_imp),
                             float(lambda_))
    for p in range(3):
        prm.dist_scale[p] = float(dist_scale[p])
    _check_code(lib().rv_mode_decide_check(sa, ca, ns, ma, C.byref(prm), 1 if imp is not None else 0,
                                           int(lanes)), "rv_mode_decide_batch")
    td = np.ascontiguousarray(tx_dist if tx_dist is not None else [], np.uint64).reshape(-1)
    te = np.ascontiguousarray(tx_eob if tx_eob is not None else [], np.uint32).reshape(-1)
    if len(td) != len(te):
        raise Rav1eHipError(f"{who}: tx_dist and tx_eob have one entry per transform block each")
    sd = None
    if seed is not None:
        sd = np.ascontiguousarray(seed, dtype=MODE_DECISION).reshape(-1)
        if len(sd) != n:
            raise Rav1eHipError(f"{who}: one seed per block")
    dt, db, dc = DeviceBuffer.from_array(tiles), DeviceBuffer.from_array(blocks), \
        DeviceBuffer.from_array(cands)
    dd, de = DeviceBuffer.from_array(td), DeviceBuffer.from_array(te)
    di = DeviceBuffer.from_array(imp) if imp is not None else None
    dsd = DeviceBuffer.from_array(sd) if sd is not None else None
    do = DeviceBuffer(MODE_DECISION.itemsize * max(1, n))
    dcd, dcc, dcs = DeviceBuffer(8 * max(1, nc)), DeviceBuffer(8 * max(1, nc)), \
        DeviceBuffer(4 * max(1, nc))
    dst = DeviceBuffer(8)
    _check_code(lib().rv_mode_decide_batch_lanes(
        sa, ca, ns, ma, dt.ptr, len(tiles), db.ptr, n, dc.ptr, nc, dsd.ptr if dsd else None,
        dd.ptr if len(td) else None, de.ptr if len(te) else None, len(td), di.ptr if di else None,
        C.byref(prm), do.ptr, dcd.ptr, dcc.ptr, dcs.ptr, dst.ptr, int(lanes), None),
        "rv_mode_decide_batch")
    _sync(None)
    st = dst.download(np.uint32, 2)
    return ModeDecideResult(do.download(MODE_DECISION, n), dcd.download(np.uint64, nc),
                            dcc.download(np.float64, nc), dcs.download(np.int32, nc), int(st[0]),
                            int(st[1]))


def prep_8tap_batch(src: DevicePlane, jobs, w, h, mode_x=0, mode_y=0, bit_depth=8):
    jobs = np.ascontiguousarray(jobs, dtype=MC_JOB)
    dj = DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(2 * w * h * max(1, len(jobs)))
    _check(lib().rv_prep_8tap_batch(out.ptr, C.byref(src.desc), dj.ptr, len(jobs), w, h,
                                    mode_x, mode_y, bit_depth, None), "rv_prep_8tap_batch")
    _sync()
    return out.download(np.int16, w * h * len(jobs)).reshape(len(jobs), h, w)


def mc_avg_batch(dst: DevicePlane, tmp1: np.ndarray, tmp2: np.ndarray, jobs, w, h,
                 bit_depth=8):
    jobs = np.ascontiguousarray(jobs, dtype=MC_JOB)
    dj = DeviceBuffer.from_array(jobs)
    t1 = DeviceBuffer.from_array(np.ascontiguousarray(tmp1, dtype=np.int16))
    t2 = DeviceBuffer.from_array(np.ascontiguousarray(tmp2, dtype=np.int16))
    _check(lib().rv_mc_avg_batch(C.byref(dst.desc), t1.ptr, t2.ptr, dj.ptr, len(jobs), w, h,
                                 bit_depth, None), "rv_mc_avg_batch")
    _sync()


def mc_dist_batch(org: DevicePlane, ref: DevicePlane, jobs, w, h, mode_x=0, mode_y=0,
                  bit_depth=8, metric=0) -> np.ndarray:
    jobs = np.ascontiguousarray(jobs, dtype=MC_JOB)
    dj = DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(4 * max(1, len(jobs)))
    _check(lib().rv_mc_dist_batch(C.byref(org.desc), C.byref(ref.desc), dj.ptr, len(jobs), w, h,
                                  mode_x, mode_y, bit_depth, metric, out.ptr, None),
           "rv_mc_dist_batch")
    _sync()
    return out.download(np.uint32, len(jobs))


def fwd_txfm_batch(residual: np.ndarray, tx_size, tx_type, bit_depth=8) -> np.ndarray:
    """residual: [n, H, W] int16 -> coeffs [n, H*W] int32 (W-stride raster)."""
    r = np.ascontiguousarray(residual, dtype=np.int16)
    n = r.shape[0]
    w, h = TxSize(tx_size).width(), TxSize(tx_size).height()
    dr = DeviceBuffer.from_array(r)
    out = DeviceBuffer(4 * w * h * max(1, n))
    _check(lib().rv_fwd_txfm_batch(dr.ptr, out.ptr, n, int(tx_size), int(tx_type), bit_depth,
                                   None), "rv_fwd_txfm_batch")
    _sync()
    return out.download(np.int32, w * h * n).reshape(n, w * h)


def diff_fwd_txfm_batch(src: DevicePlane, pred: DevicePlane, jobs, tx_size, tx_type,
                        bit_depth=8) -> np.ndarray:
    jobs = np.ascontiguousarray(jobs, dtype=TX_JOB)
    w, h = TxSize(tx_size).width(), TxSize(tx_size).height()
    dj = DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(4 * w * h * max(1, len(jobs)))
    _check(lib().rv_diff_fwd_txfm_batch(C.byref(src.desc), C.byref(pred.desc), dj.ptr, len(jobs),
                                        int(tx_size), int(tx_type), bit_depth, out.ptr, None),
           "rv_diff_fwd_txfm_batch")
    _sync()
    return out.download(np.int32, w * h * len(jobs)).reshape(len(jobs), w * h)


def coded_tx_area(tx_size) -> int:
    """av1_get_coded_tx_size(tx_size).area() (src/context.rs:1949-1956)."""
    t = TxSize(tx_size)
    return min(t.width(), 32) * min(t.height(), 32)


def quantize_batch(coeffs: np.ndarray, tx_size, tx_type, qindex, bit_depth=8, is_intra=False,
                   dc_delta_q=0, ac_delta_q=0):
    """QuantizationContext::update + quantize + dequantize (src/quantize.rs:
    205-333) of coeffs [n, >= coded area] (the forward transform's raster):
    (qcoeffs [n, coded], rcoeffs [n, coded], eob [n])."""
    c = np.ascontiguousarray(coeffs, dtype=np.int32)
    n, stride = c.shape
    coded = coded_tx_area(tx_size)
    dc = DeviceBuffer.from_array(c)
    dq = DeviceBuffer(4 * coded * max(1, n))
    dr = DeviceBuffer(4 * coded * max(1, n))
    de = DeviceBuffer(4 * max(1, n))
    _check(lib().rv_quantize_batch(dc.ptr, stride, n, int(tx_size), int(tx_type), int(qindex),
                                   bit_depth, int(bool(is_intra)), dc_delta_q, ac_delta_q, dq.ptr,
                                   dr.ptr, de.ptr, None), "rv_quantize_batch")
    _sync()
    return (dq.download(np.int32, coded * n).reshape(n, coded),
            dr.download(np.int32, coded * n).reshape(n, coded), de.download(np.uint32, n))


def dequantize_batch(qcoeffs: np.ndarray, tx_size, qindex, bit_depth=8, dc_delta_q=0,
                     ac_delta_q=0):
    """dequantize (src/quantize.rs:319-333) of [n, coded area] levels."""
    q = np.ascontiguousarray(qcoeffs, dtype=np.int32)
    n = q.shape[0]
    coded = coded_tx_area(tx_size)
    if q.shape[1] != coded:
        raise Rav1eHipError("dequantize_batch: rows must hold the coded area")
    dq = DeviceBuffer.from_array(q)
    dr = DeviceBuffer(4 * coded * max(1, n))
    _check(lib().rv_dequantize_batch(dq.ptr, n, int(tx_size), int(qindex), bit_depth, dc_delta_q,
                                     ac_delta_q, dr.ptr, None), "rv_dequantize_batch")
    _sync()
    return dr.download(np.int32, coded * n).reshape(n, coded)


def estimate_rate_batch(tx_dist: np.ndarray, tx_size, qindex) -> np.ndarray:
    """estimate_rate (src/rdo.rs:204-216) of each block's tx-domain
    distortion (u64) at base qindex: the table-interpolated rate, u64."""
    d = np.ascontiguousarray(tx_dist, dtype=np.uint64).ravel()
    n = d.size
    dd = DeviceBuffer.from_array(d if n else np.zeros(1, np.uint64))
    dr = DeviceBuffer(8 * max(1, n))
    _check(lib().rv_estimate_rate_batch(dd.ptr, n, int(qindex), int(tx_size), dr.ptr, None),
           "rv_estimate_rate_batch")
    _sync()
    return dr.download(np.uint64, n)


def inv_txfm_add_batch(coeffs: np.ndarray, dst: DevicePlane, jobs, tx_size, tx_type,
                       bit_depth=8):
    """coeffs: [n, min(H,32)*min(W,32)] int32, added into dst in place."""
    jobs = np.ascontiguousarray(jobs, dtype=TX_JOB)
    dc = DeviceBuffer.from_array(np.ascontiguousarray(coeffs, dtype=np.int32))
    dj = DeviceBuffer.from_array(jobs)
    _check(lib().rv_inv_txfm_add_batch(dc.ptr, C.byref(dst.desc), dj.ptr, len(jobs),
                                       int(tx_size), int(tx_type), bit_depth, None),
           "rv_inv_txfm_add_batch")
    _sync()


def full_search_batch(org: DevicePlane, ref: DevicePlane, jobs, blk_w, blk_h, step=1,
                      allow_hp=False) -> np.ndarray:
    jobs = np.ascontiguousarray(jobs, dtype=FS_JOB)
    dj = DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(16 * max(1, len(jobs)))
    _check(lib().rv_full_search_batch(C.byref(org.desc), C.byref(ref.desc), dj.ptr, len(jobs),
                                      blk_w, blk_h, step, 1 if allow_hp else 0, out.ptr, None),
           "rv_full_search_batch")
    _sync()
    return out.download(FS_RESULT, len(jobs))


def plane_box_sums(plane: DevicePlane) -> DeviceBuffer:
    """rv_plane_box_sums: paired 4-tall x 8-wide then paired 4x4 box sums over
    the whole allocation (u32 S48(x, y) | S48(x + 8, y) << 16, then S4(x, y) |
    S4(x + 4, y) << 16, each in the plane's stride x alloc_height layout)."""
    d = plane.desc
    out = DeviceBuffer(8 * d.stride * d.alloc_height)
    _check(lib().rv_plane_box_sums(C.byref(d), out.ptr, None), "rv_plane_box_sums")
    _sync()
    return out


def full_search_sea_batch(org: DevicePlane, ref: DevicePlane, jobs, allow_hp=False,
                          s8: "DeviceBuffer | None" = None) -> np.ndarray:
    """rv_full_search_sea_batch (16x16, step 1): same results as
    full_search_batch by successive elimination over ref's box sums."""
    jobs = np.ascontiguousarray(jobs, dtype=FS_JOB)
    if s8 is None:
        s8 = plane_box_sums(ref)
    dj = DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(16 * max(1, len(jobs)))
    _check(lib().rv_full_search_sea_batch(C.byref(org.desc), C.byref(ref.desc), s8.ptr, dj.ptr,
                                          len(jobs), 1 if allow_hp else 0, out.ptr, None),
           "rv_full_search_sea_batch")
    _sync()
    return out.download(FS_RESULT, len(jobs))


def diamond_search_batch(org: DevicePlane, ref: DevicePlane, jobs, blk_w, blk_h,
                         subpixel=False, use_satd=False, allow_hp=False,
                         bit_depth=8) -> np.ndarray:
    """diamond_me_search (src/me.rs:693-785) for every job in one launch."""
    jobs = np.ascontiguousarray(jobs, dtype=DS_JOB)
    dj = DeviceBuffer.from_array(jobs)
    out = DeviceBuffer(16 * max(1, len(jobs)))
    _check(lib().rv_diamond_search_batch(C.byref(org.desc), C.byref(ref.desc), dj.ptr,
                                         len(jobs), blk_w, blk_h, int(subpixel), int(use_satd),
                                         int(allow_hp), bit_depth, out.ptr, None),
           "rv_diamond_search_batch")
    _sync()
    return out.download(FS_RESULT, len(jobs))


def telescopic_subpel_batch(org: DevicePlane, ref: DevicePlane, jobs, start, blk_w, blk_h,
                            use_satd=False, allow_hp=False, bit_depth=8) -> np.ndarray:
    """telescopic_subpel_search (src/me.rs:858-941); start = FS_RESULT records
    (the full-pel best_mv / lowest_cost each search refines)."""
    jobs = np.ascontiguousarray(jobs, dtype=DS_JOB)
    start = np.ascontiguousarray(start, dtype=FS_RESULT)
    assert len(start) == len(jobs)
    dj, ds = DeviceBuffer.from_array(jobs), DeviceBuffer.from_array(start)
    out = DeviceBuffer(16 * max(1, len(jobs)))
    _check(lib().rv_telescopic_subpel_batch(C.byref(org.desc), C.byref(ref.desc), dj.ptr, ds.ptr,
                                            len(jobs), blk_w, blk_h, int(use_satd), int(allow_hp),
                                            bit_depth, out.ptr, None),
           "rv_telescopic_subpel_batch")
    _sync()
    return out.download(FS_RESULT, len(jobs))


def tx_dist_batch(coeffs: np.ndarray, rcoeffs: np.ndarray, tx_size) -> np.ndarray:
    """Transform-domain distortion (src/encoder.rs:1210-1224): coeffs [n][W*H]
    rasters, rcoeffs [n][coded area]."""
    coeffs = np.ascontiguousarray(coeffs, dtype=np.int32)
    rcoeffs = np.ascontiguousarray(rcoeffs, dtype=np.int32)
    n = coeffs.shape[0]
    dc, dr = DeviceBuffer.from_array(coeffs), DeviceBuffer.from_array(rcoeffs)
    out = DeviceBuffer(8 * max(1, n))
    _check(lib().rv_tx_dist_batch(dc.ptr, coeffs.shape[1], dr.ptr, n, int(tx_size), out.ptr, None),
           "rv_tx_dist_batch")
    _sync()
    return out.download(np.uint64, n)


# ---- reference-shaped single-call entry points ----------------------------
class PlaneRegion:
    """A block position inside a DevicePlane (PlaneRegion,
    src/tiling/plane_region.rs:110-152)."""

    def __init__(self, plane: DevicePlane, x: int, y: int):
        self.plane, self.x, self.y = plane, x, y


def _require_hip(cpu):
    if CpuFeatureLevel(cpu) != CpuFeatureLevel.HIP:
        raise Rav1eHipError(f"{CpuFeatureLevel(cpu).name}: only the HIP level is built here")


def get_sad(org: PlaneRegion, ref: PlaneRegion, bsize: BlockSize, bit_depth: int,
            cpu=CpuFeatureLevel.HIP) -> int:
    """get_sad (src/dist.rs:48-111)."""
    _require_hip(cpu)
    bs = BlockSize(bsize)
    job = np.array([(org.x, org.y, ref.x, ref.y)], dtype=DIST_JOB)
    return int(sad_batch(org.plane, ref.plane, job, bs.width(), bs.height())[0])


def get_satd(org: PlaneRegion, ref: PlaneRegion, bsize: BlockSize, bit_depth: int,
             cpu=CpuFeatureLevel.HIP) -> int:
    """get_satd (src/dist.rs:121-193)."""
    _require_hip(cpu)
    bs = BlockSize(bsize)
    job = np.array([(org.x, org.y, ref.x, ref.y)], dtype=DIST_JOB)
    return int(satd_batch(org.plane, ref.plane, job, bs.width(), bs.height())[0])


def put_8tap(dst: PlaneRegion, src: PlaneRegion, width, height, col_frac, row_frac,
             mode_x=FilterMode.REGULAR, mode_y=FilterMode.REGULAR, bit_depth=8,
             cpu=CpuFeatureLevel.HIP):
    """put_8tap (src/mc.rs:410-519): src = the block's integer position."""
    _require_hip(cpu)
    job = np.array([(src.x, src.y, dst.x, dst.y, col_frac, row_frac)], dtype=MC_JOB)
    put_8tap_batch(dst.plane, src.plane, job, width, height, int(mode_x), int(mode_y), bit_depth)


def prep_8tap(src: PlaneRegion, width, height, col_frac, row_frac,
              mode_x=FilterMode.REGULAR, mode_y=FilterMode.REGULAR, bit_depth=8,
              cpu=CpuFeatureLevel.HIP) -> np.ndarray:
    """prep_8tap (src/mc.rs:520-616): returns the i16 tmp[h][w]."""
    _require_hip(cpu)
    job = np.array([(src.x, src.y, 0, 0, col_frac, row_frac)], dtype=MC_JOB)
    return prep_8tap_batch(src.plane, job, width, height, int(mode_x), int(mode_y), bit_depth)[0]


def mc_avg(dst: PlaneRegion, tmp1, tmp2, width, height, bit_depth=8, cpu=CpuFeatureLevel.HIP):
    """mc_avg (src/mc.rs:617-706)."""
    _require_hip(cpu)
    job = np.array([(0, 0, dst.x, dst.y, 0, 0)], dtype=MC_JOB)
    mc_avg_batch(dst.plane, np.asarray(tmp1)[None], np.asarray(tmp2)[None], job, width, height,
                 bit_depth)


def forward_transform(residual: np.ndarray, tx_size: TxSize, tx_type: TxType, bit_depth=8,
                      cpu=CpuFeatureLevel.HIP) -> np.ndarray:
    """forward_transform (src/transform/mod.rs:556-566)."""
    _require_hip(cpu)
    return fwd_txfm_batch(np.asarray(residual)[None], tx_size, tx_type, bit_depth)[0]


def inverse_transform_add(coeffs: np.ndarray, dst: PlaneRegion, tx_size: TxSize,
                          tx_type: TxType, bit_depth=8, cpu=CpuFeatureLevel.HIP):
    """inverse_transform_add (src/transform/mod.rs:568-580)."""
    _require_hip(cpu)
    job = np.array([(0, 0, dst.x, dst.y)], dtype=TX_JOB)
    inv_txfm_add_batch(np.asarray(coeffs)[None], dst.plane, job, tx_size, tx_type, bit_depth)


def sse_wxh(src1: PlaneRegion, src2: PlaneRegion, w, h, compute_bias=None) -> float:
    """sse_wxh (src/rdo.rs:286-335): integer partials on the device, the
    f64 bias (compute_bias(x, y) per importance sub-block) on the host."""
    job = np.array([(src1.x, src1.y, src2.x, src2.y)], dtype=DIST_JOB)
    parts = sse_batch(src1.plane, src2.plane, job, w, h)[0]
    if compute_bias is None:
        return int(parts.sum())
    bw = min(w, 8) >> src1.plane.desc.xdec
    bh = min(h, 8) >> src1.plane.desc.ydec
    sx = w // bw
    total = 0.0
    for k, v in enumerate(parts):
        total += float(int(v)) * compute_bias((k % sx) * bw, (k // sx) * bh)
    return total


def cdef_dist_from_moments(m, bit_depth: int) -> int:
    """f64 tail of cdef_dist_wxh_8x8 (src/rdo.rs:242-252), on the host."""
    import math
    cs = bit_depth - 8
    sum_s, sum_d, s2, d2, sd = (int(v) for v in m)
    svar = float(s2 - ((sum_s * sum_s + 32) >> 6))
    dvar = float(d2 - ((sum_d * sum_d + 32) >> 6))
    sse = float(d2 + s2 - 2 * sd)
    boost = (4033.0 / 16384.0) * (svar + dvar + float(16384 << (2 * cs))) / math.sqrt(
        float(16265089 << (4 * cs)) + svar * dvar)
    v = sse * boost + 0.5
    return int(v) if v > 0 else 0


def cdef_dist_wxh(src1: PlaneRegion, src2: PlaneRegion, w, h, bit_depth=8,
                  compute_bias=None) -> float:
    """cdef_dist_wxh (src/rdo.rs:256-283)."""
    job = np.array([(src1.x, src1.y, src2.x, src2.y)], dtype=DIST_JOB)
    mom = cdef_moments_batch(src1.plane, src2.plane, job, w, h)[0]
    sx = w // 8
    total = 0.0
    for k, m in enumerate(mom):
        d = cdef_dist_from_moments(m, bit_depth)
        total += d * (compute_bias((k % sx) * 8, (k // sx) * 8) if compute_bias else 1.0)
    return total


def exported_symbols_from_header(path: str = HEADER_PATH):
    """Every function name include/rav1e_hip.h declares (macros expanded)."""
    import re
    text = open(path).read()
    names = set(re.findall(r"^\s*(?:[\w\s\*]+?)\b(rv_\w+|rav1e_\w+)\s*\(", text, re.M))
    names = {n for n in names if not n.startswith("rv_dist_fn") and n not in ("rv_put_fn",)}
    sizes = re.findall(r"X\((\d+), (\d+)\)", text.split("#define RV_DIST_SIZES")[1].split(
        "/*")[0])
    for w, h in sizes:
        names |= {f"rav1e_sad{w}x{h}_hip", f"rav1e_sad{w}x{h}_hbd_hip",
                  f"rav1e_satd_{w}x{h}_hip", f"rav1e_satd_{w}x{h}_hbd_hip"}
    pairs = re.findall(r"X\((\w+), (\w+), \d, \d\)", text.split("#define RV_FILTER_PAIRS")[1]
                       .split("#define RV_DECL_MC")[0])
    for nx, ny in pairs:
        names |= {f"rav1e_put_8tap_{nx}_{ny}_hip", f"rav1e_put_8tap_{nx}_{ny}_16bpc_hip",
                  f"rav1e_prep_8tap_{nx}_{ny}_hip", f"rav1e_prep_8tap_{nx}_{ny}_16bpc_hip"}
    return sorted(n for n in names if "##" not in n and not n.endswith("_hip_") and
                  n not in ("rav1e_sad", "rav1e_satd_", "rav1e_put_8tap_",
                            "rav1e_prep_8tap_"))
