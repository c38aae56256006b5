"""ctypes binding of ``libddmi.so`` (the C ABI declared in ``include/ddmi.h``).

The library is the product: there is no fallback. If the shared object is missing or a GPU
is absent, every entry point raises loudly (``DDMIUnavailable``).
"""
import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DDMI_LIB", os.path.join(HERE, "libddmi.so"))

c_float_p = ctypes.POINTER(ctypes.c_float)
c_void_p = ctypes.c_void_p


class DDMIUnavailable(RuntimeError):
    """Raised when the native HIP library cannot be loaded."""


class DDMIError(RuntimeError):
    """Raised when a ddmi C-ABI call returns a non-zero status."""


class DDConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int), ("image_arch", ctypes.c_int), ("lidar_arch", ctypes.c_int),
        ("cam_h", ctypes.c_int), ("cam_w", ctypes.c_int), ("lidar_h", ctypes.c_int),
        ("lidar_w", ctypes.c_int), ("lidar_channels", ctypes.c_int), ("num_modes", ctypes.c_int),
        ("num_poses", ctypes.c_int), ("trunc_timestep", ctypes.c_int), ("step_span", ctypes.c_int),
    ]


class DDOutputs(ctypes.Structure):
    _fields_ = [
        ("trajectory", c_void_p), ("poses_reg", c_void_p), ("poses_cls", c_void_p),
        ("bev_semantic_map", c_void_p), ("agent_states", c_void_p), ("agent_labels", c_void_p),
    ]


class DDTrainOutputs(ctypes.Structure):
    _fields_ = [
        ("trajectory", c_void_p), ("poses_reg", c_void_p * 2), ("poses_cls", c_void_p * 2), ("loss", c_void_p),
        ("bev_semantic_map", c_void_p), ("agent_states", c_void_p), ("agent_labels", c_void_p),
    ]


class DDSampleOutputs(ctypes.Structure):
    _fields_ = [
        ("trajectory", c_void_p), ("poses_reg", c_void_p), ("poses_cls", c_void_p),
        ("best_trajectory", c_void_p), ("best_index", c_void_p),
        ("bev_semantic_map", c_void_p), ("agent_states", c_void_p), ("agent_labels", c_void_p),
    ]


class DDInputs(ctypes.Structure):
    """dd_inputs: exactly one of camera_f32 / camera_u8 and one of lidar_f32 / lidar_u8 (include/ddmi.h)."""
    _fields_ = [
        ("camera_f32", c_void_p), ("camera_u8", c_void_p), ("lidar_f32", c_void_p), ("lidar_u8", c_void_p),
        ("lidar_hist_max", ctypes.c_int), ("status", c_void_p), ("noise", c_void_p),
    ]


class DDSimParams(ctypes.Structure):
    """dd_sim_params: the tracker / bicycle constants of dd_simulate (include/ddmi.h)."""
    _fields_ = [
        ("wheel_base", ctypes.c_double), ("dt", ctypes.c_double), ("tracking_horizon", ctypes.c_int),
        ("q_lon", ctypes.c_double), ("r_lon", ctypes.c_double), ("q_lat", ctypes.c_double * 3),
        ("r_lat", ctypes.c_double), ("jerk_penalty", ctypes.c_double), ("curvature_rate_penalty", ctypes.c_double),
        ("initial_curvature_penalty", ctypes.c_double), ("stopping_gain", ctypes.c_double),
        ("stopping_velocity", ctypes.c_double), ("max_steering_angle", ctypes.c_double),
        ("accel_time_constant", ctypes.c_double), ("steering_time_constant", ctypes.c_double),
    ]


class DDComfortParams(ctypes.Structure):
    """dd_comfort_params: dt and the seven comfort bounds of dd_comfort; a bound of 0 is no bound (include/ddmi.h)."""
    _fields_ = [
        ("dt", ctypes.c_double), ("min_lon_accel", ctypes.c_double), ("max_lon_accel", ctypes.c_double),
        ("max_abs_lat_accel", ctypes.c_double), ("max_abs_mag_jerk", ctypes.c_double),
        ("max_abs_lon_jerk", ctypes.c_double), ("max_abs_yaw_accel", ctypes.c_double),
        ("max_abs_yaw_rate", ctypes.c_double),
    ]


class DDAreaParams(ctypes.Structure):
    """dd_area_params: the vehicle's lever arms, dt and the driving-direction constants of dd_ego_areas
    (include/ddmi.h)."""
    _fields_ = [
        ("half_length", ctypes.c_double), ("half_width", ctypes.c_double), ("rear_axle_to_center", ctypes.c_double),
        ("dt", ctypes.c_double), ("driving_direction_horizon", ctypes.c_double),
        ("driving_direction_compliance_threshold", ctypes.c_double),
        ("driving_direction_violation_threshold", ctypes.c_double),
    ]


class DDDrivableMaps(ctypes.Structure):
    """dd_drivable_maps: the map polygons of G scenes as flat device arrays (include/ddmi.h)."""
    _fields_ = [
        ("verts", c_void_p), ("ring_off", c_void_p), ("poly_ring_off", c_void_p), ("poly_kind", c_void_p),
        ("scene_poly_off", c_void_p), ("num_polys", ctypes.c_int),
    ]


class DDScoreParams(ctypes.Structure):
    """dd_score_params: the weights, thresholds and angle bounds of dd_collisions / dd_pdm_aggregate
    (include/ddmi.h)."""
    _fields_ = [
        ("progress_weight", ctypes.c_double), ("ttc_weight", ctypes.c_double), ("comfortable_weight", ctypes.c_double),
        ("driving_direction_weight", ctypes.c_double), ("progress_distance_threshold", ctypes.c_double),
        ("ttc_stopped_speed_threshold", ctypes.c_double), ("collision_stopped_speed_threshold", ctypes.c_double),
        ("ahead_angle", ctypes.c_double), ("behind_angle", ctypes.c_double),
    ]


class DDObservations(ctypes.Structure):
    """dd_observations: the tracked objects of G scenes as flat device arrays (include/ddmi.h)."""
    _fields_ = [
        ("boxes", c_void_p), ("valid", c_void_p), ("heading", c_void_p), ("flags", c_void_p),
        ("scene_track_off", c_void_p), ("num_tracks", ctypes.c_int), ("num_times", ctypes.c_int),
    ]


class DDCenterlines(ctypes.Structure):
    """dd_centerlines: the centerlines of G scenes as flat device arrays (include/ddmi.h)."""
    _fields_ = [("verts", c_void_p), ("scene_off", c_void_p), ("num_verts", ctypes.c_int)]


class DDPaths(ctypes.Structure):
    """dd_paths: the lateral paths of G scenes as flat device arrays (include/ddmi.h)."""
    _fields_ = [("verts", c_void_p), ("progress", c_void_p), ("path_off", c_void_p),
                ("paths_per_scene", ctypes.c_int), ("num_verts", ctypes.c_int)]


class DDLeadObjects(ctypes.Structure):
    """dd_lead_objects: the tracks and stop polygons dd_proposals reads (include/ddmi.h)."""
    _fields_ = [
        ("boxes", c_void_p), ("valid", c_void_p), ("heading", c_void_p), ("speed", c_void_p),
        ("scene_track_off", c_void_p), ("num_tracks", ctypes.c_int), ("num_times", ctypes.c_int),
        ("stop_verts", c_void_p), ("ring_off", c_void_p), ("scene_ring_off", c_void_p), ("num_rings", ctypes.c_int),
    ]


class DDIdmParams(ctypes.Structure):
    """dd_idm_params: the IDM policy's and the generator's constants (include/ddmi.h)."""
    _fields_ = [
        ("min_gap_to_lead_agent", ctypes.c_double), ("headway_time", ctypes.c_double), ("accel_max", ctypes.c_double),
        ("decel_max", ctypes.c_double), ("dt", ctypes.c_double), ("acceleration_exponent", ctypes.c_int),
        ("leading_agent_update_rate", ctypes.c_int), ("corridor_poses", ctypes.c_int),
    ]


class DDDetections(ctypes.Structure):
    """dd_detections: the raw detections of G scenes as flat device arrays (include/ddmi.h)."""
    _fields_ = [("boxes", c_void_p), ("type", c_void_p), ("scene_det_off", c_void_p), ("collided_in", c_void_p),
                ("num_dets", ctypes.c_int)]


class DDObserveParams(ctypes.Structure):
    """dd_observe_params: the radius, sampling and caps of dd_observe (include/ddmi.h)."""
    _fields_ = [
        ("map_radius", ctypes.c_double), ("dt", ctypes.c_double), ("num_samples", ctypes.c_int),
        ("sample_res", ctypes.c_int), ("max_vehicles", ctypes.c_int), ("max_pedestrians", ctypes.c_int),
        ("max_bicycles", ctypes.c_int), ("max_static", ctypes.c_int), ("stopped_speed", ctypes.c_double),
    ]


class DDOpView(ctypes.Structure):
    """dd_op_view: a strided (n, h, w, c) operand of the view-taking single-op entries (include/ddmi.h)."""
    _fields_ = [("p", c_void_p), ("sn", ctypes.c_int64), ("sh", ctypes.c_int64), ("sw", ctypes.c_int64),
                ("sc", ctypes.c_int64)]


class DDOpConvDesc(ctypes.Structure):
    """dd_op_conv_desc: one conv / GEMM launch of dd_op_conv_view (include/ddmi.h)."""
    _fields_ = [
        ("in_", DDOpView), ("out", DDOpView), ("res", DDOpView),
        ("N", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("Cin", ctypes.c_int),
        ("KH", ctypes.c_int), ("KW", ctypes.c_int), ("stride", ctypes.c_int), ("pad", ctypes.c_int),
        ("Cout", ctypes.c_int),
        ("wgt", c_void_p), ("ldb", ctypes.c_int64), ("k0", ctypes.c_int), ("bias", c_void_p),
        ("relu", ctypes.c_int), ("mode", ctypes.c_int), ("flags", c_void_p), ("route_rows", ctypes.c_int64),
        ("ln_out", c_void_p), ("ln_g", c_void_p), ("ln_b", c_void_p),
        ("pool_out", DDOpView), ("pool_p", ctypes.c_int), ("pool_add", DDOpView),
        ("fused_ln", ctypes.c_int), ("fused_pool", ctypes.c_int),
    ]


MAX_SAMPLES = 32  # DD_MAX_SAMPLES

# name -> (restype, argtypes)
_SIGS = {
    "dd_default_config": (None, [ctypes.POINTER(DDConfig)]),
    "dd_create": (ctypes.c_int, [ctypes.POINTER(DDConfig), c_void_p, ctypes.c_size_t, ctypes.c_int,
                                 ctypes.POINTER(c_void_p)]),
    "dd_forward": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "dd_forward_ex": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int,
                                     ctypes.c_int, ctypes.POINTER(DDOutputs), c_void_p]),
    "dd_forward_samples": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.POINTER(DDSampleOutputs), c_void_p]),
    "dd_forward_in": (ctypes.c_int, [c_void_p, ctypes.POINTER(DDInputs), ctypes.c_int, ctypes.c_int,
                                     ctypes.POINTER(DDOutputs), c_void_p]),
    "dd_forward_samples_in": (ctypes.c_int, [c_void_p, ctypes.POINTER(DDInputs), ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.POINTER(DDSampleOutputs), c_void_p]),
    "dd_forward_train_in": (ctypes.c_int, [c_void_p, ctypes.POINTER(DDInputs), c_void_p, c_void_p, ctypes.c_int,
                                           ctypes.c_float, ctypes.c_float, c_void_p, c_void_p]),
    "dd_destroy": (ctypes.c_int, [c_void_p]),
    "dd_last_error": (ctypes.c_char_p, []),
    "dd_set_profiling": (ctypes.c_int, [c_void_p, ctypes.c_int]),
    "dd_reset_stats": (ctypes.c_int, [c_void_p]),
    "dd_kernel_stats": (ctypes.c_int, [c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_double)]),
    "dd_kernel_bytes": (ctypes.c_int, [c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double)]),
    "dd_set_seed": (ctypes.c_int, [c_void_p, ctypes.c_ulonglong]),
    "dd_set_seed_at": (ctypes.c_int, [c_void_p, ctypes.c_ulonglong, ctypes.c_ulonglong]),
    "dd_set_graph": (ctypes.c_int, [c_void_p, ctypes.c_int]),
    "dd_set_streams": (ctypes.c_int, [c_void_p, ctypes.c_int]),
    "dd_get_streams": (ctypes.c_int, [c_void_p, ctypes.POINTER(ctypes.c_int)]),
    "dd_graph_info": (ctypes.c_int, [c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                     ctypes.POINTER(ctypes.c_int)]),
    "dd_graph_nodes": (ctypes.c_int, [c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dd_forward_train": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        ctypes.c_int, ctypes.c_float, ctypes.c_float, c_void_p, c_void_p]),
    "dd_bev_semantic_loss": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            c_void_p, c_void_p, c_void_p]),
    "dd_bev_semantic_loss_work": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "dd_default_sim_params": (None, [ctypes.POINTER(DDSimParams)]),
    "dd_simulate_work": (ctypes.c_size_t, [ctypes.c_int]),
    "dd_simulate_proposals": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(DDSimParams), c_void_p, c_void_p, c_void_p]),
    "dd_simulate": (ctypes.c_int, [c_void_p, ctypes.c_int, c_void_p, ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(DDSimParams), c_void_p, c_void_p, c_void_p]),
    "dd_default_comfort_params": (None, [ctypes.POINTER(DDComfortParams)]),
    "dd_comfort": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.POINTER(DDComfortParams), c_void_p, c_void_p,
                                  c_void_p]),
    "dd_default_area_params": (None, [ctypes.POINTER(DDAreaParams)]),
    "dd_ego_areas_work": (ctypes.c_size_t, [ctypes.c_int]),
    "dd_ego_areas": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DDDrivableMaps), ctypes.c_int,
                                    ctypes.POINTER(DDAreaParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p]),
    "dd_default_score_params": (None, [ctypes.POINTER(DDScoreParams)]),
    "dd_collisions_work": (ctypes.c_size_t, [ctypes.c_int]),
    "dd_collisions": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DDObservations),
                                     ctypes.POINTER(DDDrivableMaps), ctypes.c_int, ctypes.POINTER(DDAreaParams),
                                     ctypes.POINTER(DDScoreParams), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    "dd_progress": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DDCenterlines), ctypes.c_int,
                                   ctypes.POINTER(DDAreaParams), c_void_p, c_void_p]),
    "dd_pdm_aggregate": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int,
                                        ctypes.c_int, ctypes.POINTER(DDScoreParams), c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "dd_default_idm_params": (None, [ctypes.POINTER(DDIdmParams)]),
    "dd_proposals_work": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "dd_proposals": (ctypes.c_int, [ctypes.POINTER(DDPaths), ctypes.POINTER(DDLeadObjects), c_void_p, c_void_p,
                                    c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DDIdmParams),
                                    ctypes.POINTER(DDAreaParams), c_void_p, ctypes.c_size_t, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p]),
    "dd_pdm_select": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                     c_void_p, c_void_p, c_void_p, c_void_p]),
    "dd_default_observe_params": (None, [ctypes.POINTER(DDObserveParams)]),
    "dd_observe_work": (ctypes.c_size_t, [ctypes.c_int]),
    "dd_observe": (ctypes.c_int, [ctypes.POINTER(DDDetections), c_void_p, ctypes.c_int,
                                  ctypes.POINTER(DDObserveParams), ctypes.POINTER(DDAreaParams), c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dd_detections_from_agents": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dd_set_gemm_mode": (ctypes.c_int, [c_void_p, ctypes.c_int]),
    "dd_set_schedule": (ctypes.c_int, [c_void_p, ctypes.c_int]),
    "dd_get_gemm_mode": (ctypes.c_int, [c_void_p, ctypes.POINTER(ctypes.c_int)]),
    "dd_numerics_flags": (ctypes.c_int, [c_void_p, ctypes.POINTER(ctypes.c_uint), ctypes.c_int]),
    "dd_tap": (ctypes.c_int, [c_void_p, ctypes.c_char_p, c_void_p, ctypes.c_size_t,
                              ctypes.POINTER(ctypes.c_size_t), c_void_p]),
    "dd_op_last_error": (ctypes.c_char_p, []),
    "dd_op_last_kernel": (ctypes.c_char_p, []),
    "dd_op_last_walk": (ctypes.c_char_p, []),
    "dd_op_split_weights": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                           ctypes.POINTER(ctypes.c_int)]),
    "dd_op_pack_mk_weights": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p]),
    "dd_op_mk_linear": (ctypes.c_int, [c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p, ctypes.c_int, c_void_p]),
    "dd_op_bevproj": (ctypes.c_int, [c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_build_camera": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, ctypes.c_int,
                                       ctypes.c_int, c_void_p]),
    "dd_build_lidar": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, ctypes.c_int,
                                      ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                      ctypes.c_int, ctypes.c_longlong, c_void_p]),
    "dd_build_camera_u8": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, ctypes.c_int,
                                          ctypes.c_int, c_void_p]),
    "dd_build_lidar_u8": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, ctypes.c_int,
                                         ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                         ctypes.c_int, ctypes.c_longlong, c_void_p]),
    "dd_op_stem_pool_u8": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int, c_void_p,
                                          c_void_p]),
    "dd_op_conv2d": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_op_conv2d_x3": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p]),
    "dd_op_stem_pool_x3": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p]),
    "dd_op_stem_pool": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p,
                                       c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "dd_op_stem_pool_nchw": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p,
                                            c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p]),
    "dd_op_gemm": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_op_gemm_batched": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_op_layernorm": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_op_softmax_rows": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, c_void_p]),
    "dd_op_bilinear": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p,
                                      ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_op_bilinear_add": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p,
                                          ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_op_maxpool3x3s2": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          c_void_p, c_void_p]),
    "dd_op_avgpool": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, c_void_p, c_void_p]),
    "dd_op_bev_sample_attn": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_op_mha_small": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_op_gpt_attention": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_op_gpt_attention_rows": (ctypes.c_int, [c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                c_void_p]),
    "dd_op_layernorm_groups": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_longlong, ctypes.c_int, c_void_p]),
    "dd_op_conv_desc_size": (ctypes.c_size_t, []),
    "dd_op_conv_view": (ctypes.c_int, [ctypes.POINTER(DDOpConvDesc), c_void_p]),
    "dd_op_layernorm_ld": (ctypes.c_int, [c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64, ctypes.c_int, c_void_p,
                                          c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int64, c_void_p,
                                          ctypes.c_int64, ctypes.c_int, ctypes.c_int, c_void_p]),
    "dd_op_bilinear_view": (ctypes.c_int, [ctypes.POINTER(DDOpView), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.POINTER(DDOpView), ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, c_void_p]),
    "dd_op_mha_small_view": (ctypes.c_int, [c_void_p, ctypes.c_int64, ctypes.c_int64, c_void_p, c_void_p,
                                            ctypes.c_int64, ctypes.c_int64, c_void_p, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, c_void_p]),
    "dd_op_bev_sample_attn_s": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_float, ctypes.c_float, c_void_p]),
    "dd_op_bev_taps": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                      c_void_p]),
    "dd_op_bev_sample_attn_gathered": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int,
                                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_int, ctypes.c_float, ctypes.c_float, c_void_p]),
    "dd_op_avgpool_view": (ctypes.c_int, [c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.POINTER(DDOpView), c_void_p, c_void_p]),
    "dd_op_vproj_limits": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "dd_op_vproj": (ctypes.c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_uint, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
}

EXPORTED = tuple(_SIGS)

_lib = None
_lock = threading.Lock()


def load(path: str = None):
    """Load libddmi.so and bind every C-ABI symbol. Raises DDMIUnavailable if absent."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise DDMIUnavailable(
                f"ddmi native library not found at {p}; build it with `python -m diffusiondrive_amd.build`")
        try:
            lib = ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL)
        except OSError as e:
            raise DDMIUnavailable(f"cannot load {p}: {e}") from e
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if path is None:
            _lib = lib
        return lib


def check(rc: int, lib=None, op: bool = False):
    if rc != 0:
        lib = lib or load()
        msg = (lib.dd_op_last_error() if op else lib.dd_last_error()) or b""
        raise DDMIError(f"ddmi call failed (rc={rc}): {msg.decode(errors='replace')}")
    return rc
