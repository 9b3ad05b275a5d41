"""ctypes binding of ``libmjpl_hip.so`` (include/mjpl_hip.h) -- the only compute backend.

There is no CPU path in this package: if the library is missing, cannot be loaded, or finds
no gfx950 device, construction raises.  (The CPU restatement under ``oracle/`` is test
infrastructure and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

from . import build as _build
from .model import Model

SOA, AOS = 0, 1
# mjpl_clearance_grad* status values (include/mjpl_hip.h: MJPL_GRAD_*)
GRAD_OK, GRAD_FLAT, GRAD_DEGENERATE, GRAD_NONFINITE = 0, 1, 2, 3
# mjpl_push_out* status values (include/mjpl_hip.h: MJPL_PUSH_*)
PUSH_OK, PUSH_STUCK, PUSH_DEGENERATE, PUSH_NONFINITE = 0, 1, 2, 3
# mjpl_sweep_edges* status values (include/mjpl_hip.h: MJPL_SWEEP_*)
SWEEP_FREE, SWEEP_HIT, SWEEP_UNDECIDED, SWEEP_NONFINITE, SWEEP_RANGE = 0, 1, 2, 3, 4
# mjpl_topp_profile* status values (include/mjpl_hip.h: MJPL_TOPP_*)
TOPP_OK, TOPP_STALLED, TOPP_NONFINITE = 0, 1, 2
# mjpl_shortcut_paths* status values (include/mjpl_hip.h: MJPL_SHORTCUT_*)
SHORTCUT_CONVERGED, SHORTCUT_ROUNDS, SHORTCUT_NONFINITE = 0, 1, 2
# mjpl_plan_paths* status values (include/mjpl_hip.h: MJPL_PLAN_*)
PLAN_SOLVED, PLAN_ROUNDS, PLAN_NONFINITE, PLAN_INVALID_END, PLAN_NODES = 0, 1, 2, 3, 4
PLAN_LONG = 5  # mjpl_plan_paths_constrained* only: a path of more than max_rows rows
# mjpl_roadmap_query* status values (include/mjpl_hip.h: MJPL_ROADMAP_*); the limits of both roadmap calls
ROADMAP_SOLVED, ROADMAP_NO_PATH, ROADMAP_NONFINITE, ROADMAP_INVALID_END, ROADMAP_LONG = 0, 1, 2, 3, 4
ROADMAP_MAX_K, ROADMAP_MAX_NODES, ROADMAP_MAX_PROBLEMS = 32, 1 << 20, 1 << 24
EDGE_INTERIOR_ONLY = 1

_I32P = C.POINTER(C.c_int32)
_F64P = C.POINTER(C.c_double)
_U8P = C.POINTER(C.c_uint8)
_U64P = C.POINTER(C.c_uint64)
_I64P = C.POINTER(C.c_int64)


class MjplError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libmjpl_hip status {code}: {msg}")
        self.code = code


class _ModelDesc(C.Structure):
    _fields_ = [
        ("nq", C.c_int32), ("njnt", C.c_int32), ("nbody", C.c_int32), ("ngeom", C.c_int32),
        ("body_parentid", _I32P), ("body_weldid", _I32P), ("body_jntadr", _I32P),
        ("body_jntnum", _I32P), ("body_pos", _F64P), ("body_quat", _F64P),
        ("jnt_type", _I32P), ("jnt_qposadr", _I32P), ("jnt_axis", _F64P), ("jnt_pos", _F64P),
        ("qpos0", _F64P),
        ("geom_type", _I32P), ("geom_bodyid", _I32P), ("geom_contype", _I32P),
        ("geom_conaffinity", _I32P), ("geom_size", _F64P), ("geom_pos", _F64P),
        ("geom_quat", _F64P), ("geom_rbound", _F64P), ("geom_margin", _F64P),
    ]


class Info(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("nplan", C.c_int32), ("nmoving_geoms", C.c_int32),
        ("nstatic_geoms", C.c_int32), ("npairs", C.c_int32), ("npairs_world", C.c_int32),
        ("nslots", C.c_int32), ("nsaves", C.c_int32), ("lds_bytes_configs", C.c_int32),
        ("lds_bytes_edges", C.c_int32), ("block_threads", C.c_int32), ("compute_units", C.c_int32),
        ("filter_enabled", C.c_int32), ("filter_tol", C.c_float),
        ("lds_bytes_filter", C.c_int32), ("filter_block_threads", C.c_int32),
        ("arch", C.c_char * 32),
        ("filter_max_coord", C.c_float), ("filter_err_a", C.c_float), ("filter_err_b", C.c_float),
        ("filter_poisoned_geoms", C.c_int32), ("filter_interpreter", C.c_int32),
        ("persistent_kernels", C.c_int32), ("fused_tail", C.c_int32), ("fused_edges", C.c_int32), ("fused_waves", C.c_int32),
    ]

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["arch"] = self.arch.decode()
        return d


class PoseDesc(C.Structure):
    _fields_ = [
        ("site_body", C.c_int32), ("site_pos", C.c_double * 3), ("site_quat", C.c_double * 4),
        ("c_quat", C.c_double * 4), ("c_pos", C.c_double * 3), ("lo", C.c_double * 6),
        ("hi", C.c_double * 6), ("tolerance", C.c_double), ("q_step", C.c_double),
        ("jnt_range", _F64P), ("max_iters", C.c_int32),
    ]


class IKDesc(C.Structure):
    _fields_ = [
        ("site_body", C.c_int32), ("site_pos", C.c_double * 3), ("site_quat", C.c_double * 4),
        ("target_pos", C.c_double * 3), ("target_quat", C.c_double * 4), ("pos_tolerance", C.c_double),
        ("ori_tolerance", C.c_double), ("iterations", C.c_int32), ("damping", C.c_double),
        ("lm_damping", C.c_double), ("max_step", C.c_double), ("jnt_range", _F64P), ("movable", _U8P),
        ("restarts", C.c_int32), ("restart_seed", C.c_uint64),
    ]


class PushDesc(C.Structure):
    _fields_ = [
        ("d_min", C.c_double), ("overshoot", C.c_double), ("damping", C.c_double), ("step_max", C.c_double),
        ("max_iter", C.c_int32), ("max_pairs", C.c_int32), ("lo", _F64P), ("hi", _F64P),
    ]


class ToppDesc(C.Structure):
    _fields_ = [("nq", C.c_int32), ("grid", C.c_int32), ("vmin", _F64P), ("vmax", _F64P), ("amin", _F64P), ("amax", _F64P)]


class JerkDesc(C.Structure):
    _fields_ = [("nq", C.c_int32), ("grid", C.c_int32), ("vlim", _F64P), ("alim", _F64P), ("jlim", _F64P)]


class ShortcutDesc(C.Structure):
    _fields_ = [("step_dist", C.c_double), ("min_saving", C.c_double), ("seed", C.c_uint64), ("rounds", C.c_int32),
                ("candidates", C.c_int32)]


class PlanDesc(C.Structure):
    _fields_ = [("epsilon", C.c_double), ("step_dist", C.c_double), ("seed", C.c_uint64), ("rounds", C.c_int32),
                ("candidates", C.c_int32), ("nodes", C.c_int32), ("reserved", C.c_int32)]


class CplanDesc(C.Structure):
    _fields_ = [("epsilon", C.c_double), ("step_dist", C.c_double), ("seed", C.c_uint64), ("rounds", C.c_int32),
                ("candidates", C.c_int32), ("nodes", C.c_int32), ("chain", C.c_int32), ("max_rows", C.c_int32), ("reserved", C.c_int32)]


class RoadmapDesc(C.Structure):
    _fields_ = [("radius", C.c_double), ("step_dist", C.c_double), ("k", C.c_int32), ("reserved", C.c_int32)]


class RoadmapQueryDesc(C.Structure):
    _fields_ = [("radius", C.c_double), ("step_dist", C.c_double), ("connections", C.c_int32), ("max_rows", C.c_int32)]


class SweepDesc(C.Structure):
    _fields_ = [("d_min", C.c_double), ("cap", C.c_double), ("max_depth", C.c_int32), ("lo", _F64P), ("hi", _F64P)]


class RrtDesc(C.Structure):
    _fields_ = [
        ("lanes", C.c_int32), ("capacity", C.c_int64), ("epsilon", C.c_double), ("interval_step", C.c_double),
        ("goal_bias", C.c_double), ("seed", C.c_uint64), ("lo", _F64P), ("hi", _F64P), ("pose", C.c_void_p),
        ("max_new_per_round", C.c_int64), ("max_steps_per_round", C.c_int32),
    ]


class RrtRoundInfo(C.Structure):
    _fields_ = [
        ("round", C.c_int32), ("new_nodes", C.c_int32 * 2), ("nodes", C.c_int32 * 2), ("connected", C.c_int32),
        ("conn_start", C.c_int32), ("conn_goal", C.c_int32), ("conn_rank", C.c_int32), ("stop_requested", C.c_int32),
    ]


# every symbol include/mjpl_hip.h declares: (restype, argtypes)
_VP = C.c_void_p
ABI = {
    "mjpl_create": (C.c_int, [C.POINTER(_ModelDesc), _I32P, C.c_int32, C.c_int32, C.POINTER(_VP)]),
    "mjpl_destroy": (None, [_VP]),
    "mjpl_set_planning": (C.c_int, [_VP, _I32P, C.c_int32, _F64P]),
    "mjpl_get_info": (C.c_int, [_VP, C.POINTER(Info)]),
    "mjpl_set_filter": (C.c_int, [_VP, C.c_int32, C.c_double]),
    "mjpl_filter_last_undecided": (C.c_int64, [_VP]),
    "mjpl_filter_undecided_pairs": (C.c_int64, [_VP, _I32P, _I32P, _I32P, _I32P, C.c_int64]),
    "mjpl_filter_last_interior_edges": (C.c_int64, [_VP]),
    "mjpl_filter_last_items": (C.c_int64, [_VP]),
    "mjpl_filter_last_certified": (C.c_int64, [_VP]),
    "mjpl_check_configs": (C.c_int, [_VP, _F64P, C.c_int64, C.c_int32, _U8P]),
    "mjpl_check_edges": (C.c_int, [_VP, _F64P, _F64P, C.c_int64, C.c_double, C.c_int32, C.c_int32, _U8P,
                                   _I32P]),
    "mjpl_fk": (C.c_int, [_VP, _F64P, C.c_int64, C.c_int32, _F64P, _F64P, _F64P, _F64P]),
    "mjpl_check_configs_dev": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, _VP]),
    "mjpl_check_edges_dev": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_double, C.c_int32, C.c_int32, _VP,
                                       _VP]),
    "mjpl_take_status": (C.c_int, [_VP, _I32P]),
    "mjpl_check_configs_bits_dev": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, _VP]),
    "mjpl_contact_pair_count": (C.c_int32, [_VP]),
    "mjpl_contact_pairs": (C.c_int, [_VP, _I32P, _I32P, _U8P, C.c_int32]),
    "mjpl_contacts": (C.c_int, [_VP, _F64P, C.c_int64, C.c_int32, _U64P]),
    "mjpl_contacts_dev": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, _VP]),
    "mjpl_distances": (C.c_int, [_VP, _F64P, C.c_int64, C.c_int32, C.c_double, _F64P]),
    "mjpl_distances_dev": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, C.c_double, _VP]),
    "mjpl_clearance": (C.c_int, [_VP, _F64P, C.c_int64, C.c_int32, C.c_double, _F64P, _I32P]),
    "mjpl_clearance_dev": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, C.c_double, _VP, _VP]),
    "mjpl_clearance_grad": (C.c_int, [_VP, _F64P, C.c_int64, C.c_int32, C.c_double, _F64P, _I32P, _F64P, _F64P, _F64P,
                                      _I32P]),
    "mjpl_clearance_grad_dev": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, C.c_double, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mjpl_near_pairs": (C.c_int, [_VP, _F64P, C.c_int64, C.c_int32, C.c_double, C.c_int32, _I32P, _I32P, _F64P, _F64P, _F64P,
                                  _F64P, _I32P]),
    "mjpl_near_pairs_dev": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, C.c_double, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP,
                                      _VP]),
    "mjpl_push_out": (C.c_int, [_VP, C.POINTER(PushDesc), _F64P, C.c_int64, C.c_int32, _F64P, _F64P, _I32P, _I32P, _I32P]),
    "mjpl_push_out_dev": (C.c_int, [_VP, C.POINTER(PushDesc), _VP, C.c_int64, C.c_int32, _VP, _VP, _VP, _VP, _VP]),
    "mjpl_topp_profile": (C.c_int, [_VP, C.POINTER(ToppDesc), _F64P, _I64P, C.c_int64, _F64P, _F64P, _F64P, _F64P, _I32P]),
    "mjpl_topp_profile_dev": (C.c_int, [_VP, C.POINTER(ToppDesc), _VP, _I64P, C.c_int64, _VP, _VP, _VP, _VP, _VP]),
    "mjpl_topp_sample": (C.c_int, [_VP, C.POINTER(ToppDesc), _F64P, _I64P, C.c_int64, _F64P, _F64P, _F64P, _F64P, C.c_double,
                                   _I64P, _F64P, _F64P, _F64P]),
    "mjpl_topp_sample_dev": (C.c_int, [_VP, C.POINTER(ToppDesc), _VP, _I64P, C.c_int64, _VP, _VP, _VP, _VP, C.c_double,
                                       _I64P, _VP, _VP, _VP]),
    "mjpl_jerk_profile": (C.c_int, [_VP, C.POINTER(JerkDesc), _F64P, _I64P, C.c_int64, _F64P, _F64P, _F64P, _F64P, _F64P, _F64P,
                                    _I32P]),
    "mjpl_jerk_profile_dev": (C.c_int, [_VP, C.POINTER(JerkDesc), _VP, _I64P, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mjpl_jerk_sample": (C.c_int, [_VP, C.POINTER(JerkDesc), _F64P, _I64P, C.c_int64, _F64P, _F64P, _F64P, _F64P, _F64P, _F64P,
                                   C.c_double, _I64P, _F64P, _F64P, _F64P]),
    "mjpl_jerk_sample_dev": (C.c_int, [_VP, C.POINTER(JerkDesc), _VP, _I64P, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, C.c_double,
                                       _I64P, _VP, _VP, _VP]),
    "mjpl_shortcut_paths": (C.c_int, [_VP, C.POINTER(ShortcutDesc), _F64P, _I64P, C.c_int64, _U8P, _I32P, _F64P, _I32P, _I32P,
                                      _I32P]),
    "mjpl_shortcut_paths_dev": (C.c_int, [_VP, C.POINTER(ShortcutDesc), _VP, _I64P, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mjpl_plan_paths": (C.c_int, [_VP, C.POINTER(PlanDesc), _F64P, _F64P, C.c_int64, _F64P, _F64P, _F64P, _I32P, _I32P, _I32P, _I32P,
                                  _I32P]),
    "mjpl_plan_paths_dev": (C.c_int, [_VP, C.POINTER(PlanDesc), _VP, _VP, C.c_int64, _F64P, _F64P, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mjpl_plan_paths_constrained": (C.c_int, [_VP, C.POINTER(CplanDesc), _F64P, _F64P, C.c_int64, _F64P, _F64P, _F64P, _I32P, _I32P,
                                              _I32P, _I32P, _I32P]),
    "mjpl_plan_paths_constrained_dev": (C.c_int, [_VP, C.POINTER(CplanDesc), _VP, _VP, C.c_int64, _F64P, _F64P, _VP, _VP, _VP, _VP, _VP,
                                                  _VP]),
    "mjpl_plan_paths_constrained_ext": (C.c_int, [_VP, C.POINTER(CplanDesc), C.c_int32, _F64P, _F64P, C.c_int64, _F64P, _F64P, _F64P, _I32P,
                                                  _I32P, _I32P, _I32P, _I32P]),
    "mjpl_plan_paths_constrained_ext_dev": (C.c_int, [_VP, C.POINTER(CplanDesc), C.c_int32, _VP, _VP, C.c_int64, _F64P, _F64P, _VP, _VP,
                                                      _VP, _VP, _VP, _VP]),
    "mjpl_roadmap_build": (C.c_int, [_VP, C.POINTER(RoadmapDesc), _F64P, C.c_int64, _U8P, _I32P, _I32P, _F64P]),
    "mjpl_roadmap_build_dev": (C.c_int, [_VP, C.POINTER(RoadmapDesc), _VP, C.c_int64, _VP, _VP, _VP, _VP]),
    "mjpl_roadmap_query": (C.c_int, [_VP, C.POINTER(RoadmapQueryDesc), _F64P, C.c_int64, _U8P, _I32P, _I32P, _F64P, _F64P, _F64P, C.c_int64,
                                     _F64P, _I32P, _I32P, _F64P]),
    "mjpl_roadmap_query_dev": (C.c_int, [_VP, C.POINTER(RoadmapQueryDesc), _VP, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, _VP, _VP,
                                         _VP, _VP]),
    "mjpl_sweep_levers": (C.c_int, [C.POINTER(_ModelDesc), _I32P, C.c_int32, _I32P, C.c_int32, _F64P, _F64P, _F64P, _F64P,
                                    C.c_int64]),
    "mjpl_sweep_bounds": (C.c_int, [_VP, _F64P, _F64P]),
    "mjpl_sweep_measure": (C.c_int, [_VP, _F64P, _F64P, C.c_int64, C.c_int32, C.c_double, _F64P, _I32P, _F64P, _I32P]),
    "mjpl_sweep_measure_dev": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_int32, C.c_double, _VP, _VP, _VP, _VP]),
    "mjpl_sweep_edges": (C.c_int, [_VP, C.POINTER(SweepDesc), _F64P, _F64P, C.c_int64, C.c_int32, _I32P, _F64P, _F64P, _I32P,
                                   _I32P, _I32P]),
    "mjpl_sweep_edges_dev": (C.c_int, [_VP, C.POINTER(SweepDesc), _VP, _VP, C.c_int64, C.c_int32, _VP, _VP, _VP, _VP, _VP,
                                       _VP]),
    "mjpl_sweep_splines": (C.c_int, [_VP, C.POINTER(SweepDesc), _F64P, _I64P, C.c_int64, _F64P, _I32P, _F64P, _F64P, _I32P,
                                     _I32P, _I32P]),
    "mjpl_sweep_splines_dev": (C.c_int, [_VP, C.POINTER(SweepDesc), _VP, _I64P, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP,
                                         _VP]),
    "mjpl_time_sweep_dev": (C.c_int, [_VP, C.POINTER(SweepDesc), _VP, _VP, _I64P, C.c_int64, C.c_int32, _VP, _VP, _VP, _VP, _VP,
                                      _VP, C.c_int32, C.POINTER(C.c_float)]),
    "mjpl_nearest_dev": (C.c_int, [_VP, _VP, C.c_int64, C.c_int64, _VP, C.c_int64, _VP, _VP]),
    "mjpl_nearest_range_dev": (C.c_int, [_VP, _VP, C.c_int64, C.c_int64, C.c_int64, _VP, C.c_int64, _VP, _VP, _VP, _VP]),
    "mjpl_nearest_last_screen": (C.c_int32, [_VP]),
    "mjpl_dev_alloc": (C.c_int, [_VP, C.c_size_t, C.POINTER(_VP)]),
    "mjpl_dev_free": (C.c_int, [_VP, _VP]),
    "mjpl_h2d": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "mjpl_d2h": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "mjpl_sync": (C.c_int, [_VP]),
    "mjpl_stream": (_VP, [_VP]),
    "mjpl_time_edges_dev": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_double, C.c_int32, _VP, C.c_int32,
                                      C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mjpl_time_edges_stages_dev": (C.c_int, [_VP, _VP, _VP, C.c_int64, C.c_double, C.c_int32, _VP, C.c_int32,
                                             C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), _I32P]),
    "mjpl_time_configs_dev": (C.c_int, [_VP, _VP, C.c_int64, C.c_int32, _VP, C.c_int32,
                                        C.POINTER(C.c_float)]),
    "mjpl_time_topp_dev": (C.c_int, [_VP, C.POINTER(ToppDesc), _VP, _I64P, C.c_int64, _VP, _VP, _VP, _VP, _VP, C.c_double, _I64P,
                                     _VP, _VP, _VP, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mjpl_time_jerk_dev": (C.c_int, [_VP, C.POINTER(JerkDesc), _VP, _I64P, C.c_int64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_double,
                                     _I64P, _VP, _VP, _VP, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mjpl_pose_create": (C.c_int, [_VP, C.POINTER(PoseDesc), C.POINTER(_VP)]),
    "mjpl_pose_destroy": (None, [_VP]),
    "mjpl_pose_spec_loaded": (C.c_int, [_VP]),
    "mjpl_pose_chain_dump": (C.c_int, [C.POINTER(_ModelDesc), C.c_int32, _I32P, _I32P, _F64P, _I32P, C.POINTER(C.c_uint64)]),
    "mjpl_pose_set_q_step": (C.c_int, [_VP, C.c_double]),
    "mjpl_pose_apply": (C.c_int, [_VP, _F64P, _F64P, C.c_int64, _F64P, _U8P, _I32P]),
    "mjpl_pose_valid": (C.c_int, [_VP, _F64P, C.c_int64, _U8P, _F64P, _F64P]),
    "mjpl_pose_apply_dev": (C.c_int, [_VP, _VP, _VP, C.c_int64, _VP, _VP, _VP]),
    "mjpl_pose_valid_dev": (C.c_int, [_VP, _VP, C.c_int64, _VP, _VP, _VP]),
    "mjpl_ik_solve": (C.c_int, [_VP, C.POINTER(IKDesc), _F64P, C.c_int64, _F64P, _U8P, _I32P, _F64P]),
    "mjpl_ik_solve_dev": (C.c_int, [_VP, C.POINTER(IKDesc), _VP, C.c_int64, _VP, _VP, _VP, _VP]),
    "mjpl_set_option": (C.c_int, [_VP, C.c_char_p, C.c_double]),
    "mjpl_get_option": (C.c_int, [_VP, C.c_char_p, C.POINTER(C.c_double)]),
    "mjpl_option_count": (C.c_int32, []),
    "mjpl_option_name": (C.c_char_p, [C.c_int32, C.POINTER(C.c_int32)]),
    "mjpl_set_spec_dir": (C.c_int, [C.c_char_p]),
    "mjpl_rrt_create": (C.c_int, [_VP, C.POINTER(RrtDesc), C.POINTER(_VP)]),
    "mjpl_rrt_destroy": (None, [_VP]),
    "mjpl_rrt_reset": (C.c_int, [_VP, _F64P, _F64P, C.c_int32, C.c_uint64]),
    "mjpl_rrt_round": (C.c_int, [_VP, C.c_int32, C.POINTER(RrtRoundInfo)]),
    "mjpl_rrt_set_world": (C.c_int, [_VP, C.c_int32, C.c_int32]),
    "mjpl_rrt_round_begin": (C.c_int, [_VP, C.c_int32, _I32P]),
    "mjpl_rrt_round_slabs": (C.c_int, [_VP, C.c_int32, C.POINTER(_VP), C.POINTER(_VP)]),
    "mjpl_rrt_round_finish": (C.c_int, [_VP, _I32P, C.POINTER(_VP), C.POINTER(_VP), _I32P, C.POINTER(RrtRoundInfo)]),
    "mjpl_rrt_path": (C.c_int, [_VP, _F64P, C.c_int32, _I32P]),
    "mjpl_rrt_get_tree": (C.c_int, [_VP, C.c_int32, _F64P, _I32P, C.c_int64, C.POINTER(C.c_int64)]),
    "mjpl_rrt_get_lanes": (C.c_int, [_VP, _F64P, _U8P]),
    "mjpl_comm_unique_id": (C.c_int, [_VP]),
    "mjpl_comm_init": (C.c_int, [_VP, _VP, C.c_int32, C.c_int32]),
    "mjpl_comm_destroy": (C.c_int, [_VP]),
    "mjpl_allgather_dev": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "mjpl_program_dump": (C.c_int, None),   # bound in mjpl_amd/specialise.py
    "mjpl_program_dump_pruned": (C.c_int, None),   # likewise
    "mjpl_program_dump_never_touch": (C.c_int, None),   # likewise
    "mjpl_spec_probe": (C.c_int, [C.c_uint64, C.c_int32]),
    "mjpl_spec_loaded": (C.c_int, [_VP]),
    "mjpl_set_spec": (C.c_int, [_VP, C.c_int32]),
    "mjpl_device_count": (C.c_int, []),
    "mjpl_last_error": (C.c_char_p, []),
    "mjpl_version": (C.c_char_p, []),
}

_libs: dict[str, C.CDLL] = {}


def load_library(path: str | None = None) -> C.CDLL:
    """dlopen libmjpl_hip.so and bind every declared entry point (fails loudly)."""
    path = path or os.environ.get("MJPL_HIP_LIB") or _build.LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(mjpl_amd has no CPU fallback)")
    lib = C.CDLL(path)
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        if args is not None:
            fn.argtypes = args
    _libs[path] = lib
    return lib


# Options every Engine made from now on starts with (name -> value, mjpl_set_option): what the tests and tools switch
# kernels with.  `options(...)` is the scoped form.  The LIBRARY reads no switch from the environment; this module does,
# for the convenience of shells and of the test-suite's older cases: a variable MJPL_<NAME> naming a writable option is
# applied -- through the ABI -- to every engine as it is made, MJPL_SPEC=0 as mjpl_set_spec(0), MJPL_SPEC_DIR as
# mjpl_set_spec_dir.
DEFAULT_OPTIONS: dict = {}


class options:
    """with engine.options(filter=0, fused_single=0): ...  -- engines made inside start with these options."""

    def __init__(self, **kw):
        self.kw, self.old = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = DEFAULT_OPTIONS.get(k, None)
            DEFAULT_OPTIONS[k] = v
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                DEFAULT_OPTIONS.pop(k, None)
            else:
                DEFAULT_OPTIONS[k] = v


def option_names(lib=None, writable_only=False) -> list[str]:
    lib = lib or load_library()
    out = []
    for i in range(lib.mjpl_option_count()):
        w = C.c_int32(0)
        name = lib.mjpl_option_name(i, C.byref(w))
        if name and (w.value or not writable_only):
            out.append(name.decode())
    return out


def set_spec_dir(path: str | None):
    """Per-model libraries are looked for there (process-wide; None: beside the library again)."""
    lib = load_library()
    lib.mjpl_set_spec_dir(path.encode() if path else None)


def device_count() -> int:
    return int(load_library().mjpl_device_count())


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _model_desc(model: Model):
    """(mjpl_model_desc of `model`, the arrays it points into)."""
    d = _ModelDesc()
    d.nq, d.njnt, d.nbody, d.ngeom = model.nq, model.njnt, model.nbody, model.ngeom
    keep = []
    for name, typ in _ModelDesc._fields_[4:]:
        arr = getattr(model, name)
        arr = _i32(arr) if typ is _I32P else _f64(arr)
        keep.append(arr)
        setattr(d, name, arr.ctypes.data_as(typ))
    return d, keep


def _opt_f64(a, n, what):
    if a is None:
        return None, None
    a = _f64(a)
    if a.shape != (n,):
        raise ValueError(f"{what} must have {n} entries, got {a.shape}")
    return a, a.ctypes.data_as(_F64P)


def _ptr(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


def _compile_args(model: Model, allowed_collision_bodies=(), qidx=None, qpos_base=None):
    """What every host-side compile entry point of the library takes first -> ([model descriptor, allowed body pairs and
    their number, planning indices and their number (NULL, 0: every joint), base configuration], the arrays these point into)."""
    d, keep = _model_desc(model)
    # body names -> ids (unknown names raise KeyError from model.body, as mujoco does)
    pairs = _i32([(model.body(a).id, model.body(b).id) for a, b in allowed_collision_bodies]).reshape(-1, 2)
    q = None if qidx is None else _i32(qidx)
    base = None if qpos_base is None else _f64(qpos_base)
    return [C.byref(d), _ptr(pairs, _I32P), len(pairs), _ptr(q, _I32P), 0 if q is None else len(q), _ptr(base, _F64P)], (d, keep, pairs, q, base)


def _sized_call(lib, f, args_for, alloc):
    """The protocol of the host-side dump functions: called with NULL buffers, f reports how much there is (its return
    value, or counters that args_for passes by reference); alloc(that return value) makes the arrays, the second call
    fills them.  args_for(arrays or None) -> f's arguments.  -> the arrays."""
    def call(bufs):
        rc = f(*args_for(bufs))
        if rc < 0:
            raise MjplError(rc, lib.mjpl_last_error().decode())
        return rc
    bufs = alloc(call(None))
    call(bufs)
    return bufs


def sweep_levers(model: Model, allowed_collision_bodies=(), qidx=None, qpos_base=None, lo=None, hi=None) -> np.ndarray:
    """The pair lever table of the certified edge checks, on the host alone (mjpl_sweep_levers: no GPU needed) ->
    float64 [P, nplan] over the candidate pairs of Engine.contact_pairs(): one unit of planning column c changes the
    distance of pair p by at most W[p, c].  lo / hi: bounds per planning column (a planning slide joint without finite
    bounds gives inf for the hinges above it)."""
    lib = load_library()
    args, keep = _compile_args(model, allowed_collision_bodies, qidx, qpos_base)
    nplan = args[4] = model.nq if qidx is None else args[4]
    lo, plo = _opt_f64(lo, nplan, "lo")
    hi, phi = _opt_f64(hi, nplan, "hi")
    return _sized_call(lib, lib.mjpl_sweep_levers, lambda W: [*args, plo, phi, _ptr(W, _F64P), 0 if W is None else W.size],
                       lambda P: np.zeros((P, nplan), np.float64))


class DeviceBuffer:
    """A hipMalloc'ed block owned by an :class:`Engine`."""

    def __init__(self, eng: "Engine", nbytes: int):
        self.eng, self.nbytes = eng, int(nbytes)
        p = _VP()
        eng._ok(eng.lib.mjpl_dev_alloc(eng.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self._keep = arr  # async copy: keep the source alive until the next sync
        self.eng._ok(self.eng.lib.mjpl_h2d(self.eng.h, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.eng._ok(self.eng.lib.mjpl_d2h(self.eng.h, out.ctypes.data, self.ptr, out.nbytes))
        self.eng.sync()
        return out

    def free(self):
        if self.ptr:
            self.eng.lib.mjpl_dev_free(self.eng.h, self.ptr)
            self.ptr = None


class Engine:
    """One compiled model on one MI355X (one HIP stream).  Not thread-safe, like the
    reference's per-constraint MjData (collision_constraint.py:23)."""

    def __init__(self, model: Model, allowed_collision_bodies=(), device: int = 0,
                 lib_path: str | None = None, options: dict | None = None):
        self.lib = load_library(lib_path)
        self.model = model
        self.h = None
        d, keep = _model_desc(model)
        # body names -> ids (unknown names raise KeyError from model.body, as mujoco does)
        pairs = _i32([(model.body(a).id, model.body(b).id) for a, b in allowed_collision_bodies]
                     ).reshape(-1, 2)
        h = _VP()
        rc = self.lib.mjpl_create(C.byref(d), pairs.ctypes.data_as(_I32P), len(pairs), device, C.byref(h))
        self._ok(rc)
        self.h = h
        self.nplan = model.nq
        self._allowed_bodies = tuple(allowed_collision_bodies)
        self._qidx, self._qbase = None, None
        self._projectors: "weakref.WeakSet[PoseProjector]" = weakref.WeakSet()
        self._apply_start_options(options)

    def _apply_start_options(self, explicit):
        """DEFAULT_OPTIONS, the MJPL_<NAME> variables of this process, then `explicit` -- all through mjpl_set_option; one
        compile at the end if anything was set (options that shape the compiled model take effect then)."""
        todo = dict(DEFAULT_OPTIONS)
        spec_off = None
        for name in option_names(self.lib, writable_only=True):
            v = os.environ.get("MJPL_" + name.upper())
            if v is not None and name not in todo:
                try:
                    todo[name] = float(v)
                except ValueError:
                    pass
        if os.environ.get("MJPL_SPEC") is not None:
            spec_off = os.environ["MJPL_SPEC"].strip() in ("0", "")
        if "MJPL_SPEC_DIR" in os.environ or getattr(Engine, "_spec_dir_from_env", None):
            d = os.environ.get("MJPL_SPEC_DIR")
            self.lib.mjpl_set_spec_dir(d.encode() if d else None)
            Engine._spec_dir_from_env = d
        todo.update(explicit or {})
        if "spec" in todo:
            spec_off = not todo.pop("spec")
        for k, v in todo.items():
            self._ok(self.lib.mjpl_set_option(self.h, k.encode(), float(v)))
        if todo or spec_off is not None or getattr(Engine, "_spec_dir_from_env", None) is not None:
            self._ok(self.lib.mjpl_set_spec(self.h, 0 if spec_off else 1))  # (compiles again, with the options as they stand)

    # -- plumbing
    def _ok(self, rc: int):
        if rc != 0:
            raise MjplError(rc, self.lib.mjpl_last_error().decode())

    def close(self):
        if self.h:
            # mjpl_pose handles hold device memory of their own and a pointer to this engine:
            # destroy them first so that closing the engine before its projectors leaks nothing
            for p in list(getattr(self, "_projectors", ())):
                p.close()
            self.lib.mjpl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._ok(self.lib.mjpl_sync(self.h))

    def info(self) -> dict:
        i = Info()
        self._ok(self.lib.mjpl_get_info(self.h, C.byref(i)))
        return i.as_dict()

    def spec_loaded(self) -> bool:
        """True if this engine's filter kernels are the model's own specialised ones
        (mjpl_amd/specialise.py), not the interpreter."""
        return bool(self.lib.mjpl_spec_loaded(self.h))

    def set_spec(self, enable):
        """False / 0: run the interpreting kernels even if this program has a specialised library; True / 1:
        look the libraries up (the program's own, else the robot's scene-generic one); 2: the generic one only."""
        self._ok(self.lib.mjpl_set_spec(self.h, int(enable)))

    def spec_kind(self) -> int:
        """0 interpreter, 1 the program's own specialised library, 2 the robot's scene-generic one."""
        return int(self.lib.mjpl_spec_loaded(self.h))

    def set_filter(self, enable: bool, tol: float = 1e-4):
        """Float32 filter in front of the exact kernels (verdicts are always the exact ones)."""
        self._ok(self.lib.mjpl_set_filter(self.h, 1 if enable else 0, float(tol)))

    def last_items(self) -> int:
        return int(self.lib.mjpl_filter_last_items(self.h))

    def last_certified(self) -> int:
        """Surviving edges of the last launch whose waypoint checks the fused kernel's edge certificate spared."""
        return int(self.lib.mjpl_filter_last_certified(self.h))

    def last_interior_edges(self) -> int:
        return int(self.lib.mjpl_filter_last_interior_edges(self.h))

    def last_undecided(self) -> int:
        return int(self.lib.mjpl_filter_last_undecided(self.h))

    def undecided_pairs(self, cap: int = 1 << 20):
        """Diagnostic: the pairs the last filter launch handed to the exact pair kernel
        -> (total, edge [m], check index [m], geom a [m], geom b [m]), m = min(total, cap)."""
        arrs = [np.zeros(cap, np.int32) for _ in range(4)]
        n = int(self.lib.mjpl_filter_undecided_pairs(self.h, *[a.ctypes.data_as(_I32P) for a in arrs], cap))
        if n < 0:
            raise RuntimeError("mjpl_filter_undecided_pairs failed")
        m = min(n, cap)
        return (n, *[a[:m] for a in arrs])

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def set_planning(self, qidx, qpos_base):
        qidx = _i32(qidx)
        base = _f64(qpos_base)
        if base.shape != (self.model.nq,):
            raise ValueError(f"qpos_base must have {self.model.nq} entries")
        self._ok(self.lib.mjpl_set_planning(self.h, qidx.ctypes.data_as(_I32P), len(qidx),
                                            base.ctypes.data_as(_F64P)))
        self.nplan = len(qidx)
        self._qidx, self._qbase = qidx.copy(), base.copy()

    def _batch(self, Q, layout):
        Q = _f64(Q)
        want_cols = self.nplan
        if Q.ndim != 2 or (Q.shape[0] if layout == SOA else Q.shape[1]) != want_cols:
            raise ValueError(f"batch must be [{'nplan, N' if layout == SOA else 'N, nplan'}] "
                             f"with nplan={want_cols}, got {Q.shape}")
        return Q, (Q.shape[1] if layout == SOA else Q.shape[0])

    # -- host-buffer entry points
    def check_configs(self, Q, layout=AOS) -> np.ndarray:
        Q, n = self._batch(Q, layout)
        out = np.zeros(n, np.uint8)
        self._ok(self.lib.mjpl_check_configs(self.h, Q.ctypes.data_as(_F64P), n, layout,
                                             out.ctypes.data_as(_U8P)))
        return out

    def check_edges(self, QA, QB, step_dist, layout=AOS, first_bad=False, interior_only=False):
        QA, n = self._batch(QA, layout)
        QB, n2 = self._batch(QB, layout)
        if n != n2:
            raise ValueError("QA and QB must hold the same number of edges")
        out = np.zeros(n, np.uint8)
        fb = np.zeros(n, np.int32) if first_bad else None
        self._ok(self.lib.mjpl_check_edges(
            self.h, QA.ctypes.data_as(_F64P), QB.ctypes.data_as(_F64P), n, float(step_dist), layout,
            EDGE_INTERIOR_ONLY if interior_only else 0,
            out.ctypes.data_as(_U8P), fb.ctypes.data_as(_I32P) if first_bad else None))
        return (out, fb) if first_bad else out

    def fk(self, Q, layout=AOS) -> dict:
        Q, n = self._batch(Q, layout)
        m = self.model
        xpos, xquat = np.zeros((n, m.nbody, 3)), np.zeros((n, m.nbody, 4))
        gx, gm = np.zeros((n, m.ngeom, 3)), np.zeros((n, m.ngeom, 9))
        self._ok(self.lib.mjpl_fk(self.h, Q.ctypes.data_as(_F64P), n, layout,
                                  xpos.ctypes.data_as(_F64P), xquat.ctypes.data_as(_F64P),
                                  gx.ctypes.data_as(_F64P), gm.ctypes.data_as(_F64P)))
        return dict(xpos=xpos, xquat=xquat, geom_xpos=gx, geom_xmat=gm)

    # -- device-resident entry points (pointers are DeviceBuffer.ptr or foreign device pointers)
    def check_configs_dev(self, dQ, n, layout, dvalid):
        self._ok(self.lib.mjpl_check_configs_dev(self.h, dQ, n, layout, dvalid))

    def check_configs_bits_dev(self, dQ, n, layout, dbits):
        self._ok(self.lib.mjpl_check_configs_bits_dev(self.h, dQ, n, layout, dbits))

    # -- contacts: which candidate geom pairs touch (include/mjpl_hip.h, mjpl_contacts*)
    def contact_pairs(self):
        """Candidate pairs of mj_collision -> (pairs int32 [P, 2], allowed bool [P]): the oracle's enumeration
        order, each row smaller geom type first; pairs of allowed bodies included (allowed[p] = True)."""
        if getattr(self, "_contact_pairs", None) is None:
            P = int(self.lib.mjpl_contact_pair_count(self.h))
            if P < 0:
                self._ok(P)
            g1, g2, allowed = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.uint8)
            self._ok(self.lib.mjpl_contact_pairs(self.h, g1.ctypes.data_as(_I32P), g2.ctypes.data_as(_I32P),
                                                 allowed.ctypes.data_as(_U8P), P))
            self._contact_pairs = (np.stack([g1, g2], axis=1), allowed.astype(bool))
        pairs, allowed = self._contact_pairs
        return pairs.copy(), allowed.copy()

    def contact_words(self) -> int:
        """W = (P + 63) // 64: 64-bit words per configuration of a contacts() result."""
        return (len(self.contact_pairs()[1]) + 63) // 64

    def contacts(self, Q, layout=AOS) -> np.ndarray:
        """Bit p % 64 of word p // 64 of row i: candidate pair p touches at configuration i -> uint64 [N, W]."""
        Q, n = self._batch(Q, layout)
        out = np.zeros((n, self.contact_words()), np.uint64)
        self._ok(self.lib.mjpl_contacts(self.h, Q.ctypes.data_as(_F64P), n, layout, out.ctypes.data_as(_U64P)))
        return out

    def contacts_dev(self, dQ, n, layout, dbits):
        """contacts() on device pointers: dbits receives n * W uint64 words (asynchronous on the engine's stream)."""
        self._ok(self.lib.mjpl_contacts_dev(self.h, dQ, n, layout, dbits))

    # -- distances and clearance: exact signed geom distances per candidate pair (include/mjpl_hip.h, mjpl_distances*)
    def distances(self, Q, distmax=float("inf"), layout=AOS) -> np.ndarray:
        """Signed distance of every candidate pair (contact_pairs() order) at every configuration -> float64 [N, P]:
        exact geometric distance of the two solids (gap > 0, minus the penetration depth < 0, margins not
        subtracted), or exactly ``distmax`` where it is not below ``distmax``.  NaN rows: non-finite input."""
        Q, n = self._batch(Q, layout)
        out = np.zeros((n, len(self.contact_pairs()[1])), np.float64)
        self._ok(self.lib.mjpl_distances(self.h, Q.ctypes.data_as(_F64P), n, layout, float(distmax),
                                         out.ctypes.data_as(_F64P)))
        return out

    def distances_dev(self, dQ, n, layout, ddist, distmax=float("inf")):
        """distances() on device pointers: ddist receives n * P float64 (asynchronous on the engine's stream)."""
        self._ok(self.lib.mjpl_distances_dev(self.h, dQ, n, layout, float(distmax), ddist))

    def clearance(self, Q, distmax=float("inf"), layout=AOS) -> tuple[np.ndarray, np.ndarray]:
        """(C float64 [N], pair int32 [N]): C = min over non-allowed pairs of (distance - margin), pair = the
        lowest candidate index attaining it; (distmax, -1) without such a pair, (NaN, -1) for non-finite input.
        C > 0 iff check_configs calls the configuration valid, away from the threshold."""
        Q, n = self._batch(Q, layout)
        clear, pair = np.zeros(n, np.float64), np.zeros(n, np.int32)
        self._ok(self.lib.mjpl_clearance(self.h, Q.ctypes.data_as(_F64P), n, layout, float(distmax),
                                         clear.ctypes.data_as(_F64P), pair.ctypes.data_as(_I32P)))
        return clear, pair

    def clearance_dev(self, dQ, n, layout, dclear, dpair, distmax=float("inf")):
        """clearance() on device pointers: dclear receives n float64, dpair n int32 (asynchronous)."""
        self._ok(self.lib.mjpl_clearance_dev(self.h, dQ, n, layout, float(distmax), dclear, dpair))

    # -- clearance gradients and witness points (include/mjpl_hip.h, mjpl_clearance_grad*)
    def clearance_grad(self, Q, distmax=float("inf"), layout=AOS):
        """(C float64 [N], pair int32 [N], grad float64 [N, nplan], fromto float64 [N, 6], normal float64 [N, 3],
        status int32 [N]).  C and pair are clearance()'s, bit for bit; grad = dC/dq over the planning columns;
        fromto = (w1 on g1, w2 on g2) of contact_pairs()[0][pair] in the world frame; normal = unit vector from g1
        towards g2.  status: GRAD_OK, GRAD_FLAT (no pair or capped at distmax: grad 0), GRAD_DEGENERATE (no normal:
        grad and normal NaN), GRAD_NONFINITE (non-finite input: all NaN)."""
        Q, n = self._batch(Q, layout)
        C_, pair = np.zeros(n, np.float64), np.zeros(n, np.int32)
        grad, fromto = np.zeros((n, self.nplan), np.float64), np.zeros((n, 6), np.float64)
        normal, status = np.zeros((n, 3), np.float64), np.zeros(n, np.int32)
        self._ok(self.lib.mjpl_clearance_grad(self.h, Q.ctypes.data_as(_F64P), n, layout, float(distmax),
                                              C_.ctypes.data_as(_F64P), pair.ctypes.data_as(_I32P),
                                              grad.ctypes.data_as(_F64P), fromto.ctypes.data_as(_F64P),
                                              normal.ctypes.data_as(_F64P), status.ctypes.data_as(_I32P)))
        return C_, pair, grad, fromto, normal, status

    def clearance_grad_dev(self, dQ, n, layout, dclear, dpair, dgrad, dstatus, dfromto=None, dnormal=None,
                           distmax=float("inf")):
        """clearance_grad() on device pointers: dclear n float64, dpair n int32, dgrad n * nplan float64, dstatus n
        int32, dfromto n * 6 and dnormal n * 3 float64 (either may be None).  Asynchronous on the engine's stream."""
        self._ok(self.lib.mjpl_clearance_grad_dev(self.h, dQ, n, layout, float(distmax), dclear, dpair, dgrad, dfromto,
                                                  dnormal, dstatus))

    # -- near pairs: every non-allowed pair below distmax (include/mjpl_hip.h, mjpl_near_pairs*)
    def near_pairs(self, Q, distmax, max_pairs=32, layout=AOS):
        """(count int32 [N], pair int32 [N, K], dist float64 [N, K], grad float64 [N, K, nplan], fromto float64
        [N, K, 6], normal float64 [N, K, 3], status int32 [N, K]), K = max_pairs.  count = the number of non-allowed
        candidate pairs with distance below distmax (not clipped to K; -1 for non-finite input); the first K of them, in
        ascending candidate index, fill the row's slots: pair = the index, dist = distances()'s value bit for bit, and
        grad / fromto / normal / status as clearance_grad() gives them for that pair (status GRAD_OK or
        GRAD_DEGENERATE).  The remaining slots read pair -1, status -1 and NaN."""
        Q, n = self._batch(Q, layout)
        K = int(max_pairs)
        count, pair = np.zeros(n, np.int32), np.full((n, K), -1, np.int32)
        dist, grad = np.full((n, K), np.nan), np.full((n, K, self.nplan), np.nan)
        fromto, normal = np.full((n, K, 6), np.nan), np.full((n, K, 3), np.nan)
        status = np.full((n, K), -1, np.int32)
        self._ok(self.lib.mjpl_near_pairs(self.h, Q.ctypes.data_as(_F64P), n, layout, float(distmax), K,
                                          count.ctypes.data_as(_I32P), pair.ctypes.data_as(_I32P),
                                          dist.ctypes.data_as(_F64P), grad.ctypes.data_as(_F64P),
                                          fromto.ctypes.data_as(_F64P), normal.ctypes.data_as(_F64P),
                                          status.ctypes.data_as(_I32P)))
        return count, pair, dist, grad, fromto, normal, status

    def near_pairs_dev(self, dQ, n, layout, distmax, max_pairs, dcount, dpair, ddist, dgrad, dstatus, dfromto=None,
                       dnormal=None):
        """near_pairs() on device pointers, K = max_pairs: dcount n int32, dpair n * K int32, ddist n * K float64, dgrad
        n * K * nplan float64, dstatus n * K int32, dfromto n * K * 6 and dnormal n * K * 3 float64 (either may be
        None).  Slots past a row's count get pair -1 and are otherwise left as they were.  Asynchronous on the engine's
        stream."""
        self._ok(self.lib.mjpl_near_pairs_dev(self.h, dQ, n, layout, float(distmax), int(max_pairs), dcount, dpair, ddist,
                                              dgrad, dfromto, dnormal, dstatus))

    # -- push out: configurations moved to a minimum clearance (include/mjpl_hip.h, mjpl_push_out*)
    def push_desc(self, d_min, overshoot=1e-3, damping=1e-4, step_max=0.2, max_iter=16, max_pairs=16, lo=None, hi=None):
        """The mjpl_push_desc of a call and the arrays it points into (keep both alive for the call)."""
        keep = []
        ptrs = []
        for b in (lo, hi):
            if b is None:
                ptrs.append(None)
                continue
            b = _f64(b)
            if b.shape != (self.nplan,):
                raise ValueError(f"bounds must have {self.nplan} entries, got {b.shape}")
            keep.append(b)
            ptrs.append(b.ctypes.data_as(_F64P))
        return PushDesc(float(d_min), float(overshoot), float(damping), float(step_max), int(max_iter), int(max_pairs),
                        ptrs[0], ptrs[1]), keep

    def push_out(self, Q, d_min, layout=AOS, **params):
        """(Q_out like Q, clear float64 [N], pair int32 [N], iters int32 [N], status int32 [N]): every row moved by
        damped least-squares steps on its near pairs until its clearance is at least d_min (include/mjpl_hip.h states
        the iteration; params: overshoot, damping, step_max, max_iter, max_pairs, lo, hi).  clear and pair are
        clearance(Q_out, d_min + the largest margin) bit for bit; status is PUSH_OK iff clear >= d_min, else
        PUSH_DEGENERATE / PUSH_STUCK / PUSH_NONFINITE.  Rows that need no push come back byte for byte, iters 0."""
        Q, n = self._batch(Q, layout)
        desc, keep = self.push_desc(d_min, **params)
        out = np.zeros_like(Q)
        clear, pair = np.zeros(n, np.float64), np.zeros(n, np.int32)
        iters, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._ok(self.lib.mjpl_push_out(self.h, C.byref(desc), Q.ctypes.data_as(_F64P), n, layout,
                                        out.ctypes.data_as(_F64P), clear.ctypes.data_as(_F64P),
                                        pair.ctypes.data_as(_I32P), iters.ctypes.data_as(_I32P),
                                        status.ctypes.data_as(_I32P)))
        del keep
        return out, clear, pair, iters, status

    def push_out_dev(self, dQ, n, layout, d_min, dQ_out, dclear, dpair, diters, dstatus, **params):
        """push_out() on device pointers: dQ_out n * nplan float64 in dQ's layout, dclear n float64, dpair / diters /
        dstatus n int32 (lo / hi stay host arrays).  Enqueued on the engine's stream, which it synchronises between
        iterations: the call returns once the last launches are enqueued, not before the loop has run."""
        desc, keep = self.push_desc(d_min, **params)
        self._ok(self.lib.mjpl_push_out_dev(self.h, C.byref(desc), dQ, n, layout, dQ_out, dclear, dpair, diters, dstatus))
        del keep

    # -- trajectories: time-optimal parameterisation of a batch of paths (include/mjpl_hip.h, mjpl_topp_*)
    @staticmethod
    def topp_desc(nq, grid, vmin, vmax, amin, amax):
        """The mjpl_topp_desc of a call and the arrays it points into (keep both alive for the call)."""
        keep = []
        for v in (vmin, vmax, amin, amax):
            v = _f64(v)
            if v.shape != (nq,):
                raise ValueError(f"limits must have {nq} entries, got {v.shape}")
            keep.append(v)
        return ToppDesc(int(nq), int(grid), *(v.ctypes.data_as(_F64P) for v in keep)), keep

    @staticmethod
    def topp_offsets(wp_off, grid):
        """(wp_off int64 [B+1], g_off int64 [B+1]): where path b's x, u and t start, grid (wp_off[b] - b) + b."""
        wp_off = np.ascontiguousarray(wp_off, dtype=np.int64)
        return wp_off, int(grid) * (wp_off - np.arange(len(wp_off))) + np.arange(len(wp_off))

    def topp_profile(self, W, wp_off, vmin, vmax, amin, amax, grid=8):
        """(M like W, x, u, t float64 [g_off[B]], status int32 [B]) of the B paths packed in W [wp_off[B], nq] (path b:
        rows wp_off[b] .. wp_off[b+1] - 1): knot second derivatives of the natural spline, sdot^2 at the grid points,
        sddot on the intervals, the time of every grid point (last entry of a path: its duration); status TOPP_OK /
        TOPP_STALLED / TOPP_NONFINITE.  Path b's entries start at topp_offsets(wp_off, grid)[1][b]."""
        W = _f64(W)
        if W.ndim != 2:
            raise ValueError(f"W must be [rows, nq], got {W.shape}")
        wp_off, g_off = self.topp_offsets(wp_off, grid)
        B = len(wp_off) - 1
        if B >= 0 and len(wp_off) and wp_off[-1] != len(W):
            raise ValueError(f"wp_off ends at {wp_off[-1]}, W has {len(W)} rows")
        desc, keep = self.topp_desc(W.shape[1], grid, vmin, vmax, amin, amax)
        ng = max(int(g_off[-1]), 0) if B > 0 else 0
        M = np.zeros_like(W)
        x, u, t = (np.zeros(ng, np.float64) for _ in range(3))
        status = np.zeros(max(B, 0), np.int32)
        self._ok(self.lib.mjpl_topp_profile(self.h, C.byref(desc), W.ctypes.data_as(_F64P), wp_off.ctypes.data_as(_I64P), B,
                                            M.ctypes.data_as(_F64P), x.ctypes.data_as(_F64P), u.ctypes.data_as(_F64P),
                                            t.ctypes.data_as(_F64P), status.ctypes.data_as(_I32P)))
        del keep
        return M, x, u, t, status

    def topp_profile_dev(self, dW, wp_off, nq, vmin, vmax, amin, amax, grid, dM, dx, du, dt, dstatus):
        """topp_profile() on device pointers (wp_off and the limits stay host arrays)."""
        wp_off, _ = self.topp_offsets(wp_off, grid)
        desc, keep = self.topp_desc(nq, grid, vmin, vmax, amin, amax)
        self._ok(self.lib.mjpl_topp_profile_dev(self.h, C.byref(desc), dW, wp_off.ctypes.data_as(_I64P), len(wp_off) - 1, dM, dx,
                                                du, dt, dstatus))
        del keep

    def topp_sample(self, W, wp_off, M, x, u, t, dt, samp_off, vmin, vmax, amin, amax, grid=8):
        """(pos, vel, acc float64 [samp_off[B], nq]): path b sampled at min(k dt, duration), k = 1 .. samp_off[b+1] -
        samp_off[b], from the outputs of topp_profile()."""
        W, M = _f64(W), _f64(M)
        x, u, t = _f64(x), _f64(u), _f64(t)
        wp_off, g_off = self.topp_offsets(wp_off, grid)
        samp_off = np.ascontiguousarray(samp_off, dtype=np.int64)
        B = len(wp_off) - 1
        if len(samp_off) != len(wp_off):
            raise ValueError("samp_off and wp_off must have the same length")
        if W.ndim != 2 or M.shape != W.shape or wp_off[-1] != len(W) or not (len(x) == len(u) == len(t) == max(int(g_off[-1]), 0)):
            raise ValueError("W, M, x, u, t do not have the sizes wp_off gives them")
        desc, keep = self.topp_desc(W.shape[1], grid, vmin, vmax, amin, amax)
        ns = max(int(samp_off[-1]), 0)
        pos, vel, acc = (np.zeros((ns, W.shape[1]), np.float64) for _ in range(3))
        self._ok(self.lib.mjpl_topp_sample(self.h, C.byref(desc), W.ctypes.data_as(_F64P), wp_off.ctypes.data_as(_I64P), B,
                                           M.ctypes.data_as(_F64P), x.ctypes.data_as(_F64P), u.ctypes.data_as(_F64P),
                                           t.ctypes.data_as(_F64P), float(dt), samp_off.ctypes.data_as(_I64P),
                                           pos.ctypes.data_as(_F64P), vel.ctypes.data_as(_F64P), acc.ctypes.data_as(_F64P)))
        del keep
        return pos, vel, acc

    def time_topp_dev(self, dW, wp_off, nq, dM, dx, du, dt_grid, dstatus, dt, samp_off, vmin, vmax, amin, amax, grid, dpos, dvel,
                      dacc, iters):
        """(ms_profile, ms_sample) float32 [iters]: device-event times of `iters` topp_profile_dev + topp_sample_dev calls."""
        wp_off, _ = self.topp_offsets(wp_off, grid)
        samp_off = np.ascontiguousarray(samp_off, dtype=np.int64)
        desc, keep = self.topp_desc(nq, grid, vmin, vmax, amin, amax)
        mp, ms = np.zeros(iters, np.float32), np.zeros(iters, np.float32)
        self._ok(self.lib.mjpl_time_topp_dev(self.h, C.byref(desc), dW, wp_off.ctypes.data_as(_I64P), len(wp_off) - 1, dM, dx, du,
                                             dt_grid, dstatus, float(dt), samp_off.ctypes.data_as(_I64P), dpos, dvel, dacc, iters,
                                             mp.ctypes.data_as(C.POINTER(C.c_float)), ms.ctypes.data_as(C.POINTER(C.c_float))))
        del keep
        return mp, ms

    def topp_sample_dev(self, dW, wp_off, nq, dM, dx, du, dt_grid, dt, samp_off, vmin, vmax, amin, amax, grid, dpos, dvel, dacc):
        """topp_sample() on device pointers (wp_off, samp_off and the limits stay host arrays)."""
        wp_off, _ = self.topp_offsets(wp_off, grid)
        samp_off = np.ascontiguousarray(samp_off, dtype=np.int64)
        desc, keep = self.topp_desc(nq, grid, vmin, vmax, amin, amax)
        self._ok(self.lib.mjpl_topp_sample_dev(self.h, C.byref(desc), dW, wp_off.ctypes.data_as(_I64P), len(wp_off) - 1, dM, dx,
                                               du, dt_grid, float(dt), samp_off.ctypes.data_as(_I64P), dpos, dvel, dacc))
        del keep

    # -- path shortcutting: a batch of paths in lockstep (include/mjpl_hip.h, mjpl_shortcut_paths*)
    @staticmethod
    def shortcut_desc(step_dist, rounds=16, candidates=64, seed=0, min_saving=0.0):
        """The mjpl_shortcut_desc of a call; ValueError for what the library would refuse as MJPL_E_ARG."""
        step_dist, min_saving, rounds, candidates = float(step_dist), float(min_saving), int(rounds), int(candidates)
        if not step_dist > 0.0:
            raise ValueError(f"step_dist must be > 0, got {step_dist}")
        if not min_saving >= 0.0:
            raise ValueError(f"min_saving must be >= 0, got {min_saving}")
        if rounds < 1 or rounds > 2**31 - 1:
            raise ValueError(f"rounds must be >= 1, got {rounds}")
        if not 1 <= candidates <= 64:
            raise ValueError(f"candidates must be 1..64, got {candidates}")
        return ShortcutDesc(step_dist, min_saving, int(seed) & (2**64 - 1), rounds, candidates)

    def shortcut_paths(self, W, wp_off, step_dist, rounds=16, candidates=64, seed=0, min_saving=0.0):
        """(keep uint8 [rows], n_out int32 [B], length float64 [B], status int32 [B], proposed int32 [B], accepted int32 [B])
        of the B paths packed in W [wp_off[B], nplan] (path b: rows wp_off[b] .. wp_off[b+1] - 1), shortcut in lockstep:
        per round up to `candidates` shortcuts per path, all validated by one edge launch at step_dist, the valid ones
        committed greedily by saving (include/mjpl_hip.h states the algorithm).  keep marks the surviving rows; status
        SHORTCUT_CONVERGED / SHORTCUT_ROUNDS / SHORTCUT_NONFINITE."""
        W = _f64(W)
        if W.ndim != 2 or W.shape[1] != self.nplan:
            raise ValueError(f"W must be [rows, nplan] with nplan={self.nplan}, got {W.shape}")
        wp_off = np.ascontiguousarray(wp_off, dtype=np.int64)
        B = len(wp_off) - 1
        if B < 0 or wp_off[-1] != len(W):
            raise ValueError(f"wp_off must end at W's {len(W)} rows")
        desc = self.shortcut_desc(step_dist, rounds, candidates, seed, min_saving)
        keep = np.zeros(len(W), np.uint8)
        n_out, status, proposed, accepted = (np.zeros(B, np.int32) for _ in range(4))
        length = np.zeros(B, np.float64)
        self._ok(self.lib.mjpl_shortcut_paths(self.h, C.byref(desc), W.ctypes.data_as(_F64P), wp_off.ctypes.data_as(_I64P), B,
                                              keep.ctypes.data_as(_U8P), n_out.ctypes.data_as(_I32P), length.ctypes.data_as(_F64P),
                                              status.ctypes.data_as(_I32P), proposed.ctypes.data_as(_I32P),
                                              accepted.ctypes.data_as(_I32P)))
        return keep, n_out, length, status, proposed, accepted

    def shortcut_paths_dev(self, dW, wp_off, step_dist, dkeep, dn_out, dlength, dstatus, dproposed=None, daccepted=None, rounds=16,
                           candidates=64, seed=0, min_saving=0.0):
        """shortcut_paths() on device pointers (wp_off stays a host array; dlength, dproposed, daccepted may be None)."""
        wp_off = np.ascontiguousarray(wp_off, dtype=np.int64)
        desc = self.shortcut_desc(step_dist, rounds, candidates, seed, min_saving)
        self._ok(self.lib.mjpl_shortcut_paths_dev(self.h, C.byref(desc), dW, wp_off.ctypes.data_as(_I64P), len(wp_off) - 1, dkeep,
                                                  dn_out, dlength, dstatus, dproposed, daccepted))

    # -- planning: a batch of start/goal pairs in lockstep (include/mjpl_hip.h, mjpl_plan_paths*)
    @staticmethod
    def plan_desc(step_dist, epsilon, rounds=32, candidates=16, nodes=1024, seed=0):
        """The mjpl_plan_desc of a call; ValueError for what the library would refuse as MJPL_E_ARG."""
        step_dist, epsilon, rounds, candidates, nodes = float(step_dist), float(epsilon), int(rounds), int(candidates), int(nodes)
        if not step_dist > 0.0:
            raise ValueError(f"step_dist must be > 0, got {step_dist}")
        if not epsilon > 0.0:
            raise ValueError(f"epsilon must be > 0, got {epsilon}")
        if not 1 <= rounds <= 4096:
            raise ValueError(f"rounds must be 1..4096, got {rounds}")
        if not 1 <= candidates <= 64:
            raise ValueError(f"candidates must be 1..64, got {candidates}")
        if not 2 <= nodes <= 65536:
            raise ValueError(f"nodes must be 2..65536, got {nodes}")
        return PlanDesc(epsilon, step_dist, int(seed) & (2**64 - 1), rounds, candidates, nodes, 0)

    def _plan_box(self, lo, hi):
        lo, hi = _f64(lo), _f64(hi)
        if lo.shape != (self.nplan,) or hi.shape != (self.nplan,):
            raise ValueError(f"lo and hi must be [nplan] with nplan={self.nplan}, got {lo.shape} and {hi.shape}")
        with np.errstate(over="ignore", invalid="ignore"):
            if not (np.isfinite(lo).all() and np.isfinite(hi).all() and np.isfinite(hi - lo).all()):
                raise ValueError("lo and hi must be finite (and so must hi - lo)")
        if (lo > hi).any():
            raise ValueError("lo must not exceed hi")
        return lo, hi

    def plan_paths(self, QI, QG, lo, hi, step_dist, epsilon, rounds=32, candidates=16, nodes=1024, seed=0):
        """(P float64 [B, rounds + 2, nplan], n_out, status, rounds_used, edges int32 [B], tree_nodes int32 [B, 2]) of the
        B problems QI[b] -> QG[b] ([B, nplan] each), planned in lockstep by a bidirectional RRT that samples the box
        [lo, hi]: per round one connect edge and up to `candidates` extensions of at most `epsilon` per problem, all
        validated by one edge launch at step_dist (include/mjpl_hip.h states the algorithm).  Rows 0 .. n_out[b] - 1 of
        P[b] are the path of a problem whose status is PLAN_SOLVED; the other statuses are PLAN_ROUNDS, PLAN_NONFINITE,
        PLAN_INVALID_END and PLAN_NODES."""
        QI, QG = _f64(QI), _f64(QG)
        if QI.ndim != 2 or QI.shape[1] != self.nplan or QG.shape != QI.shape:
            raise ValueError(f"QI and QG must both be [B, nplan] with nplan={self.nplan}, got {QI.shape} and {QG.shape}")
        lo, hi = self._plan_box(lo, hi)
        desc = self.plan_desc(step_dist, epsilon, rounds, candidates, nodes, seed)
        B = len(QI)
        P = np.zeros((B, desc.rounds + 2, self.nplan), np.float64)
        n_out, status, rounds_used, edges = (np.zeros(B, np.int32) for _ in range(4))
        tree_nodes = np.zeros((B, 2), np.int32)
        self._ok(self.lib.mjpl_plan_paths(self.h, C.byref(desc), QI.ctypes.data_as(_F64P), QG.ctypes.data_as(_F64P), B,
                                          lo.ctypes.data_as(_F64P), hi.ctypes.data_as(_F64P), P.ctypes.data_as(_F64P),
                                          n_out.ctypes.data_as(_I32P), status.ctypes.data_as(_I32P), rounds_used.ctypes.data_as(_I32P),
                                          edges.ctypes.data_as(_I32P), tree_nodes.ctypes.data_as(_I32P)))
        return P, n_out, status, rounds_used, edges, tree_nodes

    def plan_paths_dev(self, dQI, dQG, B, lo, hi, step_dist, epsilon, dP, dn_out, dstatus, drounds_used=None, dedges=None,
                       dtree_nodes=None, rounds=32, candidates=16, nodes=1024, seed=0):
        """plan_paths() on device pointers (lo and hi stay host arrays; drounds_used, dedges, dtree_nodes may be None)."""
        lo, hi = self._plan_box(lo, hi)
        desc = self.plan_desc(step_dist, epsilon, rounds, candidates, nodes, seed)
        self._ok(self.lib.mjpl_plan_paths_dev(self.h, C.byref(desc), dQI, dQG, int(B), lo.ctypes.data_as(_F64P), hi.ctypes.data_as(_F64P),
                                              dP, dn_out, dstatus, drounds_used, dedges, dtree_nodes))

    # -- planning under a PoseConstraint (include/mjpl_hip.h, mjpl_plan_paths_constrained*)
    @staticmethod
    def cplan_desc(step_dist, epsilon, rounds=64, candidates=16, nodes=1024, chain=8, max_rows=256, seed=0):
        """The mjpl_cplan_desc of a call; ValueError for what the library would refuse as MJPL_E_ARG."""
        base = Engine.plan_desc(step_dist, epsilon, rounds, candidates, nodes, seed)
        chain, max_rows = int(chain), int(max_rows)
        if not 1 <= chain <= 32:
            raise ValueError(f"chain must be 1..32, got {chain}")
        if not 2 <= max_rows < 2**31:
            raise ValueError(f"max_rows must be >= 2, got {max_rows}")
        return CplanDesc(base.epsilon, base.step_dist, base.seed, base.rounds, base.candidates, base.nodes, chain, max_rows, 0)

    @staticmethod
    def _cplan_extend(extend):
        """`extend` of mjpl_plan_paths_constrained_ext*; ValueError for what the library would refuse as MJPL_E_ARG."""
        extend = int(extend)
        if not 1 <= extend <= 32:
            raise ValueError(f"extend must be 1..32, got {extend}")
        return extend

    def _cplan_handle(self, pose):
        """The mjpl_pose handle of a PoseConstraint or PoseProjector of THIS engine."""
        proj = getattr(pose, "_proj", pose)
        if getattr(proj, "eng", None) is not self:
            raise ValueError("the pose constraint belongs to another engine")
        if self.nplan > 16:
            raise ValueError(f"at most 16 planning columns under a projection, got {self.nplan}")
        return proj.h

    def plan_paths_constrained(self, pose, QI, QG, lo, hi, step_dist, epsilon, rounds=64, candidates=16, nodes=1024, chain=8,
                               max_rows=256, seed=0, extend=1):
        """plan_paths() under the PoseConstraint `pose` (a PoseConstraint or PoseProjector of this engine): every tree edge
        is one projected step of at most `epsilon`, the trees are joined by a bridge of up to `chain` such steps, and an
        extension is a chain of up to `extend` (1..32) of them -- what the reference's _constrained_extend does until it
        is stopped, taken inside one round and cut at `extend` (include/mjpl_hip.h states the algorithm;
        mjpl_plan_paths_constrained_ext).  -> (P float64 [B, max_rows, nplan], n_out, status, rounds_used, edges
        int32 [B], tree_nodes int32 [B, 2]); the statuses are plan_paths' and PLAN_LONG (a path of more than max_rows rows)."""
        extend = Engine._cplan_extend(extend)  # (before any engine work)
        h = self._cplan_handle(pose)
        QI, QG = _f64(QI), _f64(QG)
        if QI.ndim != 2 or QI.shape[1] != self.nplan or QG.shape != QI.shape:
            raise ValueError(f"QI and QG must both be [B, nplan] with nplan={self.nplan}, got {QI.shape} and {QG.shape}")
        lo, hi = self._plan_box(lo, hi)
        desc = self.cplan_desc(step_dist, epsilon, rounds, candidates, nodes, chain, max_rows, seed)
        B = len(QI)
        P = np.zeros((B, desc.max_rows, self.nplan), np.float64)
        n_out, status, rounds_used, edges = (np.zeros(B, np.int32) for _ in range(4))
        tree_nodes = np.zeros((B, 2), np.int32)
        self._ok(self.lib.mjpl_plan_paths_constrained_ext(h, C.byref(desc), extend, QI.ctypes.data_as(_F64P), QG.ctypes.data_as(_F64P), B,
                                                          lo.ctypes.data_as(_F64P), hi.ctypes.data_as(_F64P), P.ctypes.data_as(_F64P),
                                                          n_out.ctypes.data_as(_I32P), status.ctypes.data_as(_I32P),
                                                          rounds_used.ctypes.data_as(_I32P), edges.ctypes.data_as(_I32P),
                                                          tree_nodes.ctypes.data_as(_I32P)))
        return P, n_out, status, rounds_used, edges, tree_nodes

    def plan_paths_constrained_dev(self, pose, dQI, dQG, B, lo, hi, step_dist, epsilon, dP, dn_out, dstatus, drounds_used=None,
                                   dedges=None, dtree_nodes=None, rounds=64, candidates=16, nodes=1024, chain=8, max_rows=256, seed=0,
                                   extend=1):
        """plan_paths_constrained() on device pointers (lo and hi stay host arrays; the last three outputs may be None)."""
        extend = Engine._cplan_extend(extend)  # (before any engine work)
        h = self._cplan_handle(pose)
        lo, hi = self._plan_box(lo, hi)
        desc = self.cplan_desc(step_dist, epsilon, rounds, candidates, nodes, chain, max_rows, seed)
        self._ok(self.lib.mjpl_plan_paths_constrained_ext_dev(h, C.byref(desc), extend, dQI, dQG, int(B), lo.ctypes.data_as(_F64P),
                                                              hi.ctypes.data_as(_F64P), dP, dn_out, dstatus, drounds_used, dedges,
                                                              dtree_nodes))

    # -- roadmap planning: validate a scene's edges once, answer many queries (include/mjpl_hip.h, mjpl_roadmap_*)
    @staticmethod
    def _roadmap_lengths(radius, step_dist):
        radius, step_dist = float(radius), float(step_dist)
        if not (radius > 0.0 and np.isfinite(radius)):
            raise ValueError(f"radius must be > 0 and finite, got {radius}")
        if not (step_dist > 0.0 and np.isfinite(step_dist)):
            raise ValueError(f"step_dist must be > 0 and finite, got {step_dist}")
        return radius, step_dist

    @staticmethod
    def roadmap_desc(radius, step_dist, k=8):
        """The mjpl_roadmap_desc of a build; ValueError for what the library would refuse as MJPL_E_ARG."""
        radius, step_dist = Engine._roadmap_lengths(radius, step_dist)
        k = int(k)
        if not 1 <= k <= ROADMAP_MAX_K:
            raise ValueError(f"k must be 1..{ROADMAP_MAX_K}, got {k}")
        return RoadmapDesc(radius, step_dist, k, 0)

    @staticmethod
    def roadmap_query_desc(radius, step_dist, connections=8, max_rows=256):
        """The mjpl_roadmap_query_desc of a query; ValueError for what the library would refuse as MJPL_E_ARG."""
        radius, step_dist = Engine._roadmap_lengths(radius, step_dist)
        connections, max_rows = int(connections), int(max_rows)
        if not 1 <= connections <= ROADMAP_MAX_K:
            raise ValueError(f"connections must be 1..{ROADMAP_MAX_K}, got {connections}")
        if not 2 <= max_rows <= 2**31 - 1:
            raise ValueError(f"max_rows must be at least 2, got {max_rows}")
        return RoadmapQueryDesc(radius, step_dist, connections, max_rows)

    def roadmap_build(self, Q, radius, step_dist, k=8):
        """(node_valid uint8 [N], row_off int32 [N + 1], adj int32 [2 N k], w float64 [2 N k]): the roadmap over the rows
        of Q [N, nplan].  A row is a node if it is finite and collision-free; every node is joined to its k nearest
        nodes within `radius` (ties to the lowest index, nodes closer than 2^-20 radius left apart) where the edge
        pipeline finds the edge valid at step_dist; the result is a symmetric CSR adjacency whose rows ascend, with
        w = the edge's length, and adj = -1, w = 0 past row_off[N] (include/mjpl_hip.h states the algorithm)."""
        Q = _f64(Q)
        if Q.ndim != 2 or Q.shape[1] != self.nplan:
            raise ValueError(f"Q must be [N, nplan] with nplan={self.nplan}, got {Q.shape}")
        desc = self.roadmap_desc(radius, step_dist, k)
        N = len(Q)
        if N > ROADMAP_MAX_NODES:
            raise ValueError(f"at most {ROADMAP_MAX_NODES} nodes, got {N}")
        node_valid, row_off = np.zeros(N, np.uint8), np.zeros(N + 1, np.int32)
        adj, w = np.full(2 * N * desc.k, -1, np.int32), np.zeros(2 * N * desc.k, np.float64)
        self._ok(self.lib.mjpl_roadmap_build(self.h, C.byref(desc), Q.ctypes.data_as(_F64P), N, node_valid.ctypes.data_as(_U8P),
                                             row_off.ctypes.data_as(_I32P), adj.ctypes.data_as(_I32P), w.ctypes.data_as(_F64P)))
        return node_valid, row_off, adj, w

    def roadmap_build_dev(self, dQ, N, radius, step_dist, dnode_valid, drow_off, dadj, dw, k=8):
        """roadmap_build() on device pointers: dnode_valid N uint8, drow_off N + 1 int32, dadj 2 N k int32, dw 2 N k float64."""
        desc = self.roadmap_desc(radius, step_dist, k)
        self._ok(self.lib.mjpl_roadmap_build_dev(self.h, C.byref(desc), dQ, int(N), dnode_valid, drow_off, dadj, dw))

    def roadmap_query(self, Q, node_valid, row_off, adj, w, QI, QG, radius, step_dist, connections=8, max_rows=256):
        """(P float64 [B, max_rows, nplan], n_out, status int32 [B], cost float64 [B]) of the B problems QI[b] -> QG[b]
        on the roadmap roadmap_build() returned for Q: each end is attached to its `connections` nearest nodes within
        `radius`, ONE edge launch validates the direct edge and the attachments of every problem, and a shortest-path
        search over the graph gives the path of least length.  Rows 0 .. n_out[b] - 1 of P[b] are the path of a problem
        whose status is ROADMAP_SOLVED and cost[b] its length; the other statuses are ROADMAP_NO_PATH,
        ROADMAP_NONFINITE, ROADMAP_INVALID_END and ROADMAP_LONG (more than max_rows rows)."""
        Q, QI, QG = _f64(Q), _f64(QI), _f64(QG)
        if Q.ndim != 2 or Q.shape[1] != self.nplan:
            raise ValueError(f"Q must be [N, nplan] with nplan={self.nplan}, got {Q.shape}")
        if QI.ndim != 2 or QI.shape[1] != self.nplan or QG.shape != QI.shape:
            raise ValueError(f"QI and QG must both be [B, nplan] with nplan={self.nplan}, got {QI.shape} and {QG.shape}")
        desc = self.roadmap_query_desc(radius, step_dist, connections, max_rows)
        N, B = len(Q), len(QI)
        node_valid = np.ascontiguousarray(node_valid, dtype=np.uint8)
        row_off, adj = np.ascontiguousarray(row_off, dtype=np.int32), np.ascontiguousarray(adj, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if node_valid.shape != (N,) or row_off.shape != (N + 1,) or adj.ndim != 1 or w.shape != adj.shape:
            raise ValueError("node_valid [N], row_off [N + 1], adj and w (one length) must be the arrays of roadmap_build()")
        if N > ROADMAP_MAX_NODES or B > ROADMAP_MAX_PROBLEMS or len(adj) < row_off[N]:
            raise ValueError(f"at most {ROADMAP_MAX_NODES} nodes and {ROADMAP_MAX_PROBLEMS} problems; adj must hold row_off[N] entries")
        P = np.zeros((B, desc.max_rows, self.nplan), np.float64)
        n_out, status, cost = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.float64)
        self._ok(self.lib.mjpl_roadmap_query(self.h, C.byref(desc), Q.ctypes.data_as(_F64P), N, node_valid.ctypes.data_as(_U8P),
                                             row_off.ctypes.data_as(_I32P), adj.ctypes.data_as(_I32P), w.ctypes.data_as(_F64P),
                                             QI.ctypes.data_as(_F64P), QG.ctypes.data_as(_F64P), B, P.ctypes.data_as(_F64P),
                                             n_out.ctypes.data_as(_I32P), status.ctypes.data_as(_I32P), cost.ctypes.data_as(_F64P)))
        return P, n_out, status, cost

    def roadmap_query_dev(self, dQ, N, dnode_valid, drow_off, dadj, dw, dQI, dQG, B, radius, step_dist, dP, dn_out, dstatus, dcost=None,
                          connections=8, max_rows=256):
        """roadmap_query() on device pointers (dcost may be None): the graph stays on the device between calls."""
        desc = self.roadmap_query_desc(radius, step_dist, connections, max_rows)
        self._ok(self.lib.mjpl_roadmap_query_dev(self.h, C.byref(desc), dQ, int(N), dnode_valid, drow_off, dadj, dw, dQI, dQG, int(B), dP,
                                                 dn_out, dstatus, dcost))

    # -- trajectories: jerk-limited parameterisation of a batch of paths (include/mjpl_hip.h, mjpl_jerk_*)
    @staticmethod
    def jerk_desc(nq, grid, vlim, alim, jlim):
        """The mjpl_jerk_desc of a call and the arrays it points into (keep both alive for the call)."""
        keep = []
        for v in (vlim, alim, jlim):
            v = _f64(v)
            if v.shape != (nq,):
                raise ValueError(f"limits must have {nq} entries, got {v.shape}")
            keep.append(v)
        return JerkDesc(int(nq), int(grid), *(v.ctypes.data_as(_F64P) for v in keep)), keep

    def jerk_profile(self, W, wp_off, vlim, alim, jlim, grid=2):
        """(M like W, lim float64 [g_off[B], 3], v, vp, tc, t float64 [g_off[B]], status int32 [B]) of the B paths packed
        in W as for topp_profile(): knot second derivatives, the limits (V, A, J) of every grid interval, the path speed
        at the junctions, the peak speed and the cruise time of every interval, the time of every grid point (last
        entry of a path: its duration); status TOPP_OK / TOPP_STALLED / TOPP_NONFINITE.  Path b's entries start at
        topp_offsets(wp_off, grid)[1][b]."""
        W = _f64(W)
        if W.ndim != 2:
            raise ValueError(f"W must be [rows, nq], got {W.shape}")
        wp_off, g_off = self.topp_offsets(wp_off, grid)
        B = len(wp_off) - 1
        if B >= 0 and len(wp_off) and wp_off[-1] != len(W):
            raise ValueError(f"wp_off ends at {wp_off[-1]}, W has {len(W)} rows")
        desc, keep = self.jerk_desc(W.shape[1], grid, vlim, alim, jlim)
        ng = max(int(g_off[-1]), 0) if B > 0 else 0
        M = np.zeros_like(W)
        lim = np.zeros((ng, 3), np.float64)
        v, vp, tc, t = (np.zeros(ng, np.float64) for _ in range(4))
        status = np.zeros(max(B, 0), np.int32)
        self._ok(self.lib.mjpl_jerk_profile(self.h, C.byref(desc), W.ctypes.data_as(_F64P), wp_off.ctypes.data_as(_I64P), B,
                                            *(a.ctypes.data_as(_F64P) for a in (M, lim, v, vp, tc, t)),
                                            status.ctypes.data_as(_I32P)))
        del keep
        return M, lim, v, vp, tc, t, status

    def jerk_profile_dev(self, dW, wp_off, nq, vlim, alim, jlim, grid, dM, dlim, dv, dvp, dtc, dt, dstatus):
        """jerk_profile() on device pointers (wp_off and the limits stay host arrays)."""
        wp_off, _ = self.topp_offsets(wp_off, grid)
        desc, keep = self.jerk_desc(nq, grid, vlim, alim, jlim)
        self._ok(self.lib.mjpl_jerk_profile_dev(self.h, C.byref(desc), dW, wp_off.ctypes.data_as(_I64P), len(wp_off) - 1, dM, dlim,
                                                dv, dvp, dtc, dt, dstatus))
        del keep

    def jerk_sample(self, W, wp_off, M, lim, v, vp, tc, t, dt, samp_off, vlim, alim, jlim, grid=2):
        """(pos, vel, acc float64 [samp_off[B], nq]): path b sampled at min(k dt, duration), k = 1 .. samp_off[b+1] -
        samp_off[b], from the outputs of jerk_profile()."""
        W, M, lim = _f64(W), _f64(M), _f64(lim)
        v, vp, tc, t = _f64(v), _f64(vp), _f64(tc), _f64(t)
        wp_off, g_off = self.topp_offsets(wp_off, grid)
        samp_off = np.ascontiguousarray(samp_off, dtype=np.int64)
        B = len(wp_off) - 1
        if len(samp_off) != len(wp_off):
            raise ValueError("samp_off and wp_off must have the same length")
        ng = max(int(g_off[-1]), 0)
        if (W.ndim != 2 or M.shape != W.shape or wp_off[-1] != len(W) or lim.shape != (ng, 3)
                or not (len(v) == len(vp) == len(tc) == len(t) == ng)):
            raise ValueError("W, M, lim, v, vp, tc, t do not have the sizes wp_off gives them")
        desc, keep = self.jerk_desc(W.shape[1], grid, vlim, alim, jlim)
        ns = max(int(samp_off[-1]), 0)
        pos, vel, acc = (np.zeros((ns, W.shape[1]), np.float64) for _ in range(3))
        self._ok(self.lib.mjpl_jerk_sample(self.h, C.byref(desc), W.ctypes.data_as(_F64P), wp_off.ctypes.data_as(_I64P), B,
                                           *(a.ctypes.data_as(_F64P) for a in (M, lim, v, vp, tc, t)), float(dt),
                                           samp_off.ctypes.data_as(_I64P), pos.ctypes.data_as(_F64P), vel.ctypes.data_as(_F64P),
                                           acc.ctypes.data_as(_F64P)))
        del keep
        return pos, vel, acc

    def jerk_sample_dev(self, dW, wp_off, nq, dM, dlim, dv, dvp, dtc, dt_grid, dt, samp_off, vlim, alim, jlim, grid, dpos, dvel,
                        dacc):
        """jerk_sample() on device pointers (wp_off, samp_off and the limits stay host arrays)."""
        wp_off, _ = self.topp_offsets(wp_off, grid)
        samp_off = np.ascontiguousarray(samp_off, dtype=np.int64)
        desc, keep = self.jerk_desc(nq, grid, vlim, alim, jlim)
        self._ok(self.lib.mjpl_jerk_sample_dev(self.h, C.byref(desc), dW, wp_off.ctypes.data_as(_I64P), len(wp_off) - 1, dM, dlim,
                                               dv, dvp, dtc, dt_grid, float(dt), samp_off.ctypes.data_as(_I64P), dpos, dvel, dacc))
        del keep

    def time_jerk_dev(self, dW, wp_off, nq, dM, dlim, dv, dvp, dtc, dt_grid, dstatus, dt, samp_off, vlim, alim, jlim, grid, dpos,
                      dvel, dacc, iters):
        """(ms_profile, ms_sample) float32 [iters]: device-event times of `iters` jerk_profile_dev + jerk_sample_dev calls."""
        wp_off, _ = self.topp_offsets(wp_off, grid)
        samp_off = np.ascontiguousarray(samp_off, dtype=np.int64)
        desc, keep = self.jerk_desc(nq, grid, vlim, alim, jlim)
        mp, ms = np.zeros(iters, np.float32), np.zeros(iters, np.float32)
        self._ok(self.lib.mjpl_time_jerk_dev(self.h, C.byref(desc), dW, wp_off.ctypes.data_as(_I64P), len(wp_off) - 1, dM, dlim, dv,
                                             dvp, dtc, dt_grid, dstatus, float(dt), samp_off.ctypes.data_as(_I64P), dpos, dvel, dacc,
                                             iters, mp.ctypes.data_as(C.POINTER(C.c_float)), ms.ctypes.data_as(C.POINTER(C.c_float))))
        del keep
        return mp, ms

    # -- certified edge checks: no contact anywhere along an edge (include/mjpl_hip.h, mjpl_sweep_*)
    def sweep_levers(self, lo=None, hi=None) -> np.ndarray:
        """The lever table this engine would use with the bounds lo / hi -> float64 [P, nplan] (computed on the host:
        module-level sweep_levers)."""
        return sweep_levers(self.model, self._allowed_bodies, self._qidx, self._qbase, lo, hi)

    def sweep_bounds(self, lo=None, hi=None):
        """Bounds over the planning columns for the lever table of sweep_measure (sweep_edges takes its own)."""
        lo, plo = _opt_f64(lo, self.nplan, "lo")
        hi, phi = _opt_f64(hi, self.nplan, "hi")
        self._ok(self.lib.mjpl_sweep_bounds(self.h, plo, phi))

    def sweep_measure(self, Q, HD, cap, layout=AOS):
        """The bubble measurement -> (slack float64 [N], slack_pair int32 [N], gap float64 [N], gap_pair int32 [N]).
        HD (shaped like Q, >= 0): how far each planning column may move from the row.  gap, gap_pair = clearance(Q, cap)
        bit for bit; slack = min over non-allowed pairs of (distance - margin - sum_c HD[c] W[p, c]).  slack > 0: no
        configuration of the box around the row is in contact."""
        Q, n = self._batch(Q, layout)
        HD, n2 = self._batch(HD, layout)
        if n != n2:
            raise ValueError("Q and HD must hold the same number of rows")
        slack, gap = np.zeros(n, np.float64), np.zeros(n, np.float64)
        sp, gp = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._ok(self.lib.mjpl_sweep_measure(self.h, Q.ctypes.data_as(_F64P), HD.ctypes.data_as(_F64P), n, layout, float(cap),
                                             slack.ctypes.data_as(_F64P), sp.ctypes.data_as(_I32P),
                                             gap.ctypes.data_as(_F64P), gp.ctypes.data_as(_I32P)))
        return slack, sp, gap, gp

    def sweep_measure_dev(self, dQ, dHD, n, layout, cap, dslack, dslack_pair, dgap, dgap_pair):
        """sweep_measure() on device pointers: dslack / dgap n float64, dslack_pair / dgap_pair n int32 (asynchronous)."""
        self._ok(self.lib.mjpl_sweep_measure_dev(self.h, dQ, dHD, n, layout, float(cap), dslack, dslack_pair, dgap, dgap_pair))

    def sweep_desc(self, d_min=0.0, cap=None, max_depth=8, lo=None, hi=None):
        """The mjpl_sweep_desc of a call and the arrays it points into (keep both alive for the call).  cap None: d_min +
        the largest margin of a non-allowed pair + 0.1."""
        lo, plo = _opt_f64(lo, self.nplan, "lo")
        hi, phi = _opt_f64(hi, self.nplan, "hi")
        if cap is None:
            cap = float(d_min) + self.sweep_margin_max() + 0.1
        return SweepDesc(float(d_min), float(cap), int(max_depth), plo, phi), (lo, hi)

    def sweep_margin_max(self) -> float:
        """The largest margin of a non-allowed candidate pair (0 without one): a sweep's cap must exceed d_min + this."""
        if getattr(self, "_sweep_margin_max", None) is None:
            pairs, allowed = self.contact_pairs()
            m = np.asarray(self.model.geom_margin, np.float64)
            pm = np.maximum(m[pairs[:, 0]], m[pairs[:, 1]])[~allowed]
            self._sweep_margin_max = float(pm.max()) if len(pm) else 0.0
        return self._sweep_margin_max

    def sweep_edges(self, QA, QB, d_min=0.0, layout=AOS, **params):
        """Certified edge checks -> (status int32 [E], t_hit float64 [E], clear_lb float64 [E], pair int32 [E], nodes int32
        [E], depth int32 [E]); params: cap, max_depth, lo, hi.  status SWEEP_FREE: no configuration of the segment
        QA -> QB is in contact or nearer than d_min, and clearance >= clear_lb all along it; SWEEP_HIT: the configuration
        at t_hit is (pair: its closest pair); SWEEP_UNDECIDED: max_depth spent; SWEEP_NONFINITE; SWEEP_RANGE: an end
        point outside lo / hi."""
        QA, n = self._batch(QA, layout)
        QB, n2 = self._batch(QB, layout)
        if n != n2:
            raise ValueError("QA and QB must hold the same number of edges")
        desc, keep = self.sweep_desc(d_min, **params)
        status, pair = np.zeros(n, np.int32), np.zeros(n, np.int32)
        nodes, depth = np.zeros(n, np.int32), np.zeros(n, np.int32)
        t_hit, clear_lb = np.zeros(n, np.float64), np.zeros(n, np.float64)
        self._ok(self.lib.mjpl_sweep_edges(self.h, C.byref(desc), QA.ctypes.data_as(_F64P), QB.ctypes.data_as(_F64P), n, layout,
                                           status.ctypes.data_as(_I32P), t_hit.ctypes.data_as(_F64P),
                                           clear_lb.ctypes.data_as(_F64P), pair.ctypes.data_as(_I32P),
                                           nodes.ctypes.data_as(_I32P), depth.ctypes.data_as(_I32P)))
        del keep
        return status, t_hit, clear_lb, pair, nodes, depth

    def sweep_edges_dev(self, dQA, dQB, n, layout, d_min, dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth, **params):
        """sweep_edges() on device pointers (lo / hi stay host arrays).  Enqueued on the engine's stream, which it
        synchronises once per round."""
        desc, keep = self.sweep_desc(d_min, **params)
        self._ok(self.lib.mjpl_sweep_edges_dev(self.h, C.byref(desc), dQA, dQB, n, layout, dstatus, dt_hit, dclear_lb, dpair,
                                               dnodes, ddepth))
        del keep

    # -- certified trajectories: no contact anywhere along the spline (include/mjpl_hip.h, mjpl_sweep_splines*)
    def sweep_splines(self, W, wp_off, d_min=0.0, want_M=True, **params):
        """Certified spline pieces -> (status, t_hit, clear_lb, pair, nodes, depth, M like W), the first six per PIECE:
        the B paths packed in W [wp_off[B], nplan] (path b: rows wp_off[b] .. wp_off[b+1] - 1) have wp_off[B] - B
        pieces, piece k of path b at index wp_off[b] - b + k.  The curve is the natural cubic spline topp_profile moves
        along (M: its knot second derivatives, None with want_M False).  status SWEEP_FREE: no configuration of the piece
        is in contact or nearer than d_min; SWEEP_HIT: the one at the local coordinate t_hit is; SWEEP_RANGE with pair
        -2: the spline leaves lo / hi at t_hit; the rest as sweep_edges.  params: cap, max_depth, lo, hi."""
        W = _f64(W)
        if W.ndim != 2 or W.shape[1] != self.nplan:
            raise ValueError(f"W must be [rows, {self.nplan}], got {W.shape}")
        wp_off = np.ascontiguousarray(wp_off, dtype=np.int64)
        B = len(wp_off) - 1
        if B < 0 or wp_off[-1] != len(W):
            raise ValueError(f"wp_off must end at the {len(W)} rows of W")
        desc, keep = self.sweep_desc(d_min, **params)
        n = max(int(wp_off[-1]) - B, 0)
        M = np.zeros_like(W) if want_M else None
        status, pair = np.zeros(n, np.int32), np.zeros(n, np.int32)
        nodes, depth = np.zeros(n, np.int32), np.zeros(n, np.int32)
        t_hit, clear_lb = np.zeros(n, np.float64), np.zeros(n, np.float64)
        self._ok(self.lib.mjpl_sweep_splines(self.h, C.byref(desc), W.ctypes.data_as(_F64P), wp_off.ctypes.data_as(_I64P), B,
                                             None if M is None else M.ctypes.data_as(_F64P), status.ctypes.data_as(_I32P),
                                             t_hit.ctypes.data_as(_F64P), clear_lb.ctypes.data_as(_F64P),
                                             pair.ctypes.data_as(_I32P), nodes.ctypes.data_as(_I32P),
                                             depth.ctypes.data_as(_I32P)))
        del keep
        return status, t_hit, clear_lb, pair, nodes, depth, M

    def sweep_splines_dev(self, dW, wp_off, d_min, dM, dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth, **params):
        """sweep_splines() on device pointers (wp_off, lo / hi stay host arrays; dM may be None).  Enqueued on the
        engine's stream, which it synchronises on entry and once per round."""
        wp_off = np.ascontiguousarray(wp_off, dtype=np.int64)
        desc, keep = self.sweep_desc(d_min, **params)
        self._ok(self.lib.mjpl_sweep_splines_dev(self.h, C.byref(desc), dW, wp_off.ctypes.data_as(_I64P), len(wp_off) - 1, dM,
                                                 dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth))
        del keep

    def time_sweep_dev(self, dA, dB, wp_off, n, layout, d_min, dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth, iters, **params):
        """ms float32 [iters]: device-event times of `iters` sweep calls -- sweep_edges_dev(dA, dB, n, layout) with wp_off
        None, else sweep_splines_dev(W = dA, wp_off, M = dB or None) on its len(wp_off) - 1 paths."""
        desc, keep = self.sweep_desc(d_min, **params)
        ms = np.zeros(iters, np.float32)
        off = None
        if wp_off is not None:
            off = np.ascontiguousarray(wp_off, dtype=np.int64)
            n = len(off) - 1
        self._ok(self.lib.mjpl_time_sweep_dev(self.h, C.byref(desc), dA, dB, None if off is None else off.ctypes.data_as(_I64P),
                                              n, layout, dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth, iters,
                                              ms.ctypes.data_as(C.POINTER(C.c_float))))
        del keep
        return ms

    def check_edges_dev(self, dQA, dQB, n, step_dist, layout, dvalid, dfirst_bad=None, flags=0):
        self._ok(self.lib.mjpl_check_edges_dev(self.h, dQA, dQB, n, float(step_dist), layout, flags,
                                               dvalid, dfirst_bad))

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        """RCCL communicator for the frontier planner's exchange (one per engine)."""
        if len(unique_id) != 128:
            raise ValueError("a ncclUniqueId is 128 bytes")
        self._ok(self.lib.mjpl_comm_init(self.h, C.create_string_buffer(unique_id, 128), rank, world))

    def comm_destroy(self):
        self._ok(self.lib.mjpl_comm_destroy(self.h))

    def allgather_dev(self, dsend, drecv, nbytes_per_rank: int):
        self._ok(self.lib.mjpl_allgather_dev(self.h, dsend, drecv, nbytes_per_rank))

    def take_status(self) -> int:
        """Sticky status of the device-pointer edge launches since the last take (0 or
        MJPL_E_NONFINITE = -7); synchronises."""
        st = C.c_int32(0)
        self._ok(self.lib.mjpl_take_status(self.h, C.byref(st)))
        return int(st.value)

    def nearest_dev(self, dnodes, n, cap, dqueries, m, dout_idx, dout_d2=None):
        self._ok(self.lib.mjpl_nearest_dev(self.h, dnodes, n, cap, dqueries, m, dout_idx, dout_d2))

    def nearest_range_dev(self, dnodes, n0, n, cap, dqueries, m, dout_idx, dout_d2=None, dprev_idx=None, dprev_d2=None):
        """nearest_dev over nodes [n0, n) behind the answer (dprev_idx, dprev_d2) for the nodes below n0."""
        self._ok(self.lib.mjpl_nearest_range_dev(self.h, dnodes, n0, n, cap, dqueries, m, dout_idx, dout_d2, dprev_idx, dprev_d2))

    def set_option(self, name: str, value) -> None:
        """A switch of the library by name (include/mjpl_hip.h: mjpl_set_option; the table is in tools/README.md)."""
        self._ok(self.lib.mjpl_set_option(self.h, name.encode(), float(value)))

    def get_option(self, name: str) -> float:
        v = C.c_double(0.0)
        self._ok(self.lib.mjpl_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def nearest_last_screen(self) -> int:
        """0: plain float64 scan, 1: binary32 screen, 2: matrix-core (binary16) screen -- of the last nearest_dev."""
        return int(self.lib.mjpl_nearest_last_screen(self.h))

    def time_edges_dev(self, dQA, dQB, n, step_dist, layout, dvalid, iters, first_kernel=False):
        """Per-call durations (ms) of `iters` edge launches; with first_kernel=True also the
        durations of the first (dominant) kernel of each call."""
        ms = np.zeros(iters, np.float32)
        ms1 = np.zeros(iters, np.float32)
        fp = C.POINTER(C.c_float)
        self._ok(self.lib.mjpl_time_edges_dev(self.h, dQA, dQB, n, float(step_dist), layout, dvalid,
                                              iters, ms.ctypes.data_as(fp), ms1.ctypes.data_as(fp)))
        return (ms, ms1) if first_kernel else ms

    STAGES = ("k_filter_endpoints", "k_filter_items", "k_filter_edges", "k_patch_pairs", "k_check_edges")
    # with info()["fused_tail"] the fourth stage is k_tail (walking role + pair re-check + exact edge role in
    # one launch) and stages three and five are empty; with info()["persistent_kernels"] the first two
    # kernels are k_filter_endpoints_pw / k_filter_items_pw

    def time_edges_stages_dev(self, dQA, dQB, n, step_dist, layout, dvalid, iters, sample_every=4):
        """`iters` back-to-back edge launches -> (mean ms per launch, {stage kernel: mean ms},
        sampled launches); the stages are bracketed on every `sample_every`-th launch only."""
        mean = C.c_float(0)
        st = (C.c_float * len(self.STAGES))()
        ns = C.c_int32(0)
        self._ok(self.lib.mjpl_time_edges_stages_dev(self.h, dQA, dQB, n, float(step_dist), layout, dvalid, iters,
                                                     sample_every, C.byref(mean), st, C.byref(ns)))
        return float(mean.value), {k: float(st[i]) for i, k in enumerate(self.STAGES)}, int(ns.value)

    def ik_solve(self, site: str, target_pos, target_quat, Q, movable, pos_tolerance=1e-3,
                 ori_tolerance=1e-3, iterations=500, damping=0.0, lm_damping=-1.0, max_step=0.0,
                 restarts=0, restart_seed=0):
        """Batched damped-least-squares IK: rows of Q [N, nq] are start configurations.
        -> (Q_out [N, nq], ok bool[N], iters int32[N], err [N, 2])"""
        model = self.model
        sid = model.site(site).id
        d = IKDesc()
        d.site_body = int(model.site_bodyid[sid])
        d.site_pos[:] = [float(x) for x in model.site_pos[sid]]
        d.site_quat[:] = [float(x) for x in model.site_quat[sid]]
        d.target_pos[:] = [float(x) for x in target_pos]
        d.target_quat[:] = [float(x) for x in target_quat]
        d.pos_tolerance, d.ori_tolerance, d.iterations = float(pos_tolerance), float(ori_tolerance), int(iterations)
        d.damping, d.lm_damping, d.max_step = float(damping), float(lm_damping), float(max_step)
        d.restarts, d.restart_seed = int(restarts), int(restart_seed) & (2**64 - 1)
        rng = _f64(model.jnt_range).reshape(-1)
        mv = np.ascontiguousarray(movable, dtype=np.uint8)
        if mv.shape != (model.njnt,):
            raise ValueError("`movable` must have one entry per joint")
        d.jnt_range = rng.ctypes.data_as(_F64P)
        d.movable = mv.ctypes.data_as(_U8P)
        Q = _f64(Q)
        if Q.ndim != 2 or Q.shape[1] != model.nq:
            raise ValueError(f"expected rows of {model.nq} qpos values, got shape {Q.shape}")
        n = len(Q)
        out = np.empty_like(Q)
        ok = np.zeros(n, np.uint8)
        iters = np.zeros(n, np.int32)
        err = np.zeros((n, 2))
        self._ok(self.lib.mjpl_ik_solve(self.h, C.byref(d), Q.ctypes.data_as(_F64P), n, out.ctypes.data_as(_F64P),
                                        ok.ctypes.data_as(_U8P), iters.ctypes.data_as(_I32P),
                                        err.ctypes.data_as(_F64P)))
        return out, ok.astype(bool), iters, err

    def time_configs_dev(self, dQ, n, layout, dvalid, iters) -> np.ndarray:
        ms = np.zeros(iters, np.float32)
        self._ok(self.lib.mjpl_time_configs_dev(self.h, dQ, n, layout, dvalid, iters,
                                                ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms


class PoseProjector:
    """``mjpl_pose`` handle: batched PoseConstraint.valid_config / apply / site pose for one
    (engine, site, constraint frame).  Rows are FULL qpos vectors [N, nq]."""

    def __init__(self, eng: Engine, site: str, c_quat, c_pos, bounds, tolerance: float, q_step: float,
                 max_iters: int = 1000):
        self.eng = eng
        model = eng.model
        sid = model.site(site).id
        d = PoseDesc()
        d.site_body = int(model.site_bodyid[sid])
        d.site_pos[:] = [float(x) for x in model.site_pos[sid]]
        d.site_quat[:] = [float(x) for x in model.site_quat[sid]]
        d.c_quat[:] = [float(x) for x in c_quat]
        d.c_pos[:] = [float(x) for x in c_pos]
        b = np.asarray(bounds, dtype=np.float64).reshape(6, 2)
        d.lo[:] = [float(x) for x in b[:, 0]]
        d.hi[:] = [float(x) for x in b[:, 1]]
        d.tolerance, d.q_step, d.max_iters = float(tolerance), float(q_step), int(max_iters)
        rng = _f64(model.jnt_range).reshape(-1)
        d.jnt_range = rng.ctypes.data_as(_F64P)
        self.h = None
        h = _VP()
        eng._ok(eng.lib.mjpl_pose_create(eng.h, C.byref(d), C.byref(h)))
        self.h = h
        self.nq = model.nq
        eng._projectors.add(self)

    def spec_loaded(self) -> bool:
        """True: a generated projection of the engine's per-model library serves this handle (same results)."""
        return bool(self.eng.lib.mjpl_pose_spec_loaded(self.h))

    def close(self):
        if self.h and self.eng.h:
            self.eng.lib.mjpl_pose_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_q_step(self, q_step: float):
        self.eng._ok(self.eng.lib.mjpl_pose_set_q_step(self.h, float(q_step)))

    def _rows(self, Q):
        Q = _f64(Q)
        if Q.ndim != 2 or Q.shape[1] != self.nq:
            raise ValueError(f"expected rows of {self.nq} qpos values, got shape {Q.shape}")
        return Q

    def apply(self, Q_old, Q):
        """-> (Q_projected [N, nq], ok bool[N], iters int32[N])"""
        Q_old, Q = self._rows(Q_old), self._rows(Q)
        if Q_old.shape != Q.shape:
            raise ValueError("Q_old and Q must have the same shape")
        n = len(Q)
        out = np.empty_like(Q)
        ok = np.zeros(n, np.uint8)
        iters = np.zeros(n, np.int32)
        self.eng._ok(self.eng.lib.mjpl_pose_apply(
            self.h, Q_old.ctypes.data_as(_F64P), Q.ctypes.data_as(_F64P), n, out.ctypes.data_as(_F64P),
            ok.ctypes.data_as(_U8P), iters.ctypes.data_as(_I32P)))
        return out, ok.astype(bool), iters

    def valid(self, Q, poses: bool = False):
        """-> valid bool[N]  (and, with poses=True, site xpos [N, 3], xmat [N, 3, 3])"""
        Q = self._rows(Q)
        n = len(Q)
        valid = np.zeros(n, np.uint8)
        xpos = np.empty((n, 3)) if poses else None
        xmat = np.empty((n, 9)) if poses else None
        self.eng._ok(self.eng.lib.mjpl_pose_valid(
            self.h, Q.ctypes.data_as(_F64P), n, valid.ctypes.data_as(_U8P),
            xpos.ctypes.data_as(_F64P) if poses else None, xmat.ctypes.data_as(_F64P) if poses else None))
        if poses:
            return valid.astype(bool), xpos, xmat.reshape(n, 3, 3)
        return valid.astype(bool)

    def apply_dev(self, dQ_old, dQ, n, dQ_out, dok, diters=None):
        self.eng._ok(self.eng.lib.mjpl_pose_apply_dev(self.h, dQ_old, dQ, n, dQ_out, dok, diters))


class DeviceRRT:
    """``mjpl_rrt`` handle: both trees of a frontier bi-RRT resident in HBM (include/mjpl_hip.h).
    Batches are over the engine's planning columns, so call ``Engine.set_planning`` first."""

    def __init__(self, eng: Engine, lanes: int, capacity: int, lo, hi, epsilon=0.05, interval_step=None,
                 goal_bias=0.05, seed=0, pose: PoseProjector | None = None, max_new_per_round=0, max_steps_per_round=0):
        self.eng, self.nplan, self.lanes = eng, eng.nplan, int(lanes)
        lo, hi = _f64(lo), _f64(hi)
        if lo.shape != (self.nplan,) or hi.shape != (self.nplan,):
            raise ValueError("lo / hi must have one entry per planning column")
        d = RrtDesc()
        d.lanes, d.capacity, d.epsilon = int(lanes), int(capacity), float(epsilon)
        d.interval_step = float(interval_step) if interval_step else 0.0
        d.goal_bias, d.seed = float(goal_bias), int(seed) & (2**64 - 1)
        d.lo, d.hi = lo.ctypes.data_as(_F64P), hi.ctypes.data_as(_F64P)
        d.pose = pose.h if pose is not None else None
        d.max_new_per_round = int(max_new_per_round)
        d.max_steps_per_round = int(max_steps_per_round)
        self._pose = pose  # keep the handle alive
        self.h = None
        h = _VP()
        eng._ok(eng.lib.mjpl_rrt_create(eng.h, C.byref(d), C.byref(h)))
        self.h = h
        eng._projectors.add(self)  # closed with (before) its engine

    def close(self):
        if self.h and self.eng.h:
            self.eng.lib.mjpl_rrt_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, q_init, q_goals, seed: int):
        q_init, q_goals = _f64(q_init), _f64(np.atleast_2d(q_goals))
        if q_init.shape != (self.nplan,) or q_goals.shape[1] != self.nplan:
            raise ValueError("configurations must hold the planning columns")
        self.eng._ok(self.eng.lib.mjpl_rrt_reset(self.h, q_init.ctypes.data_as(_F64P), q_goals.ctypes.data_as(_F64P),
                                                 len(q_goals), int(seed) & (2**64 - 1)))

    def round(self, request_stop: bool = False) -> RrtRoundInfo:
        info = RrtRoundInfo()
        self.eng._ok(self.eng.lib.mjpl_rrt_round(self.h, 1 if request_stop else 0, C.byref(info)))
        return info

    # -- the round split at its exchange step (a launcher that moves the slabs itself)
    def set_world(self, rank: int, world: int):
        self.eng._ok(self.eng.lib.mjpl_rrt_set_world(self.h, int(rank), int(world)))

    def round_begin(self, request_stop: bool = False) -> np.ndarray:
        """-> this rank's exchange header, int32[8] (include/mjpl_hip.h)"""
        head = np.zeros(8, np.int32)
        self.eng._ok(self.eng.lib.mjpl_rrt_round_begin(self.h, 1 if request_stop else 0, head.ctypes.data_as(_I32P)))
        return head

    def round_slabs(self, which: int):
        """-> (device pointer of the rows, of the parents) of this rank's new nodes of pass `which`"""
        rows, par = _VP(), _VP()
        self.eng._ok(self.eng.lib.mjpl_rrt_round_slabs(self.h, int(which), C.byref(rows), C.byref(par)))
        return rows.value, par.value

    def round_finish(self, heads, drows_all, dparents_all, stride_rows) -> RrtRoundInfo:
        heads = np.ascontiguousarray(heads, dtype=np.int32)
        rows = (_VP * 2)(*[p or None for p in drows_all])
        pars = (_VP * 2)(*[p or None for p in dparents_all])
        stride = np.ascontiguousarray(stride_rows, dtype=np.int32)
        info = RrtRoundInfo()
        self.eng._ok(self.eng.lib.mjpl_rrt_round_finish(self.h, heads.ctypes.data_as(_I32P), rows, pars,
                                                        stride.ctypes.data_as(_I32P), C.byref(info)))
        return info

    def path(self, maxlen: int = 65536) -> np.ndarray:
        out = np.empty((maxlen, self.nplan))
        n = C.c_int32(0)
        self.eng._ok(self.eng.lib.mjpl_rrt_path(self.h, out.ctypes.data_as(_F64P), maxlen, C.byref(n)))
        return out[: n.value].copy()

    def tree(self, t: int):
        """-> (Q [n, nplan], parent int32[n]) of tree t (0 = start, 1 = goal)"""
        n = C.c_int64(0)
        self.eng._ok(self.eng.lib.mjpl_rrt_get_tree(self.h, t, None, None, 0, C.byref(n)))
        Q = np.empty((n.value, self.nplan))
        par = np.empty(n.value, np.int32)
        self.eng._ok(self.eng.lib.mjpl_rrt_get_tree(self.h, t, Q.ctypes.data_as(_F64P), par.ctypes.data_as(_I32P), n.value,
                                                    C.byref(n)))
        return Q, par

    def lanes_state(self):
        T = np.empty((self.lanes, self.nplan))
        on = np.empty(self.lanes, np.uint8)
        self.eng._ok(self.eng.lib.mjpl_rrt_get_lanes(self.h, T.ctypes.data_as(_F64P), on.ctypes.data_as(_U8P)))
        return T, on.astype(bool)


class EngineRing:
    """Several engines of one model on one GPU taking batches in turns: every engine has its own HIP stream and
    scratch, so the kernels of consecutive `check_edges_dev` / `check_configs_dev` calls overlap -- the next batch
    fills the chip while this one's kernels drain (three engines validate 262 144-edge batches
    at 1.55e9 edges/s, one at 1.08e9).  Calls return when they are enqueued; `sync()` waits for all engines.
    Results are those of a single engine, batch by batch."""

    def __init__(self, model: Model, allowed_collision_bodies=(), device: int = 0, engines: int = 3,
                 planning_qidx=None, qpos_base=None):
        if engines < 1:
            raise ValueError("`engines` must be >= 1")
        self.engines = [Engine(model, allowed_collision_bodies, device) for _ in range(engines)]
        if planning_qidx is not None:
            for e in self.engines:
                e.set_planning(planning_qidx, qpos_base)
        self._turn = 0

    def next(self) -> "Engine":
        """The engine whose turn it is (device buffers of any engine of the ring may be passed to any other)."""
        e = self.engines[self._turn % len(self.engines)]
        self._turn += 1
        return e

    def check_edges_dev(self, dQA, dQB, n, step_dist, layout, dvalid, dfirst_bad=None, flags=0) -> "Engine":
        e = self.next()
        e.check_edges_dev(dQA, dQB, n, step_dist, layout, dvalid, dfirst_bad, flags)
        return e

    def sync(self):
        for e in self.engines:
            e.sync()

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library: 128 bytes for rank 0 to hand to the other ranks."""
    lib = load_library()
    buf = C.create_string_buffer(128)
    rc = lib.mjpl_comm_unique_id(buf)
    if rc != 0:
        raise MjplError(rc, lib.mjpl_last_error().decode())
    return buf.raw
