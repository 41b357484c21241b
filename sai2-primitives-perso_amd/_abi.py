"""ctypes view of the C ABI declared in include/sai2b.h.

Only POD structs and the loader live here. The product library is
``sai2-primitives-perso_amd/csrc/libsai2b.so`` (built by ``__graft_entry__.build()``); loading it
fails loudly when it has not been built — there is no CPU fallback.
"""
import ctypes as C
import os

DOF = 7  # the Panda's: default of the helpers that take no robot
MAX_DOF = 8
MAX_TASKS = 4
SH_HISTORY = 200

# enum sai2b_task_type (reference src/tasks/TemplateTask.h:19-23)
UNDEFINED, JOINT_TASK, MOTION_FORCE_TASK = 0, 1, 2
# enum sai2b_decoupling (reference src/helper_modules/Sai2PrimitivesCommonDefinitions.h:9-15)
FULL_DYNAMIC_DECOUPLING, BOUNDED_INERTIA_ESTIMATES, IMPEDANCE = 0, 1, 2
# enum sai2b_singular_vector_sign (not in the reference: the orientation of the singular vector classifySingularity
# perturbs along, SingularityHandler.cpp:253-265)
SV_SIGN_V_MAX_POSITIVE, SV_SIGN_V_MAX_NEGATIVE, SV_SIGN_EITHER, SV_SIGN_BOTH = 0, 1, 2, 3
# enum sai2b_status
OK, INVALID_ARGUMENT, RUNTIME_ERROR, UNSUPPORTED = 0, 1, 2, 3
# enum sai2b_buffer
BUF_Q, BUF_DQ, BUF_TAU, BUF_GOALS, BUF_SENSED, BUF_STATE, BUF_TASK_N, BUF_TASK_N_TOTAL = 0, 1, 2, 3, 4, 5, 6, 7
BUF_PAYLOAD, BUF_PLANT_PAYLOAD = 8, 9  # [10][B] per-robot payload rows of the controller / the plant (sai2b_set_link_payload)
BUF_CONTACT = 10  # [9][B] contact rows of the plant: plane point 3, normal 3, stiffness, damping, friction (sai2b_set_contact)
MAX_CONTACT_POINTS = 4
BUF_JOINT_DYNAMICS = 11  # [6][dof][B] rows of the plant's joint dynamics (sai2b_set_joint_dynamics)
BUF_JOINT_DYNAMICS_STATE = 12  # [3][dof][B]: applied, stop and dissipative torque of the last sim step
JOINT_DYNAMICS_ROWS = ("armature", "damping", "friction", "torque_limit", "q_lower", "q_upper")
BUF_EXTERNAL_WRENCH = 13  # [7][B] external-wrench rows of the plant: force 3, moment 3, remaining periods (sai2b_set_external_wrench)
BUF_EXTERNAL_WRENCH_STATE = 14  # [6 + dof][B]: F_w, M_w and the joint torques tx of the last sim step
BUF_HARDWARE_ACTUATOR = 15  # [1 + 3 dof][B] actuator rows: delay, lag coefficient, gain, noise deviation (sai2b_set_hardware)
BUF_HARDWARE_SENSOR = 16  # [13][B] sensor rows: bias 6, noise deviation 6, filter coefficient
BUF_TAU_APPLIED = 17  # [dof][B]: the torques the plant received in the last sim step
BUF_REWARD_STATE = 18  # [3 + dof][B]: running return, running discount, last return, tau_prev
BUF_REWARD_EPISODE = 19  # [2][B] int32: last length, tau_prev is valid
MAX_ACTUATION_DELAY = 8  # SAI2B_MAX_ACTUATION_DELAY
BUF_Q_MEASURED, BUF_DQ_MEASURED = 21, 22  # [dof][B] each: the controller's view of the state (sai2b_set_joint_sensor)
BUF_JOINT_SENSOR = 23  # [1 + 5 dof][B] rows: delay; offset, position noise, quantum, velocity noise, velocity filter coefficient
JOINT_SENSOR_VELOCITY_MODES = {"tachometer": 0, "finite_difference": 1}
BUF_COLLISION = 24  # [6 P + 4 O][B]: per plane point 3 and unit normal 3, per obstacle centre 3 and radius (sai2b_set_collision)
MAX_COLLISION_SPHERES, MAX_COLLISION_PLANES, MAX_COLLISION_OBSTACLES = 16, 2, 4  # SAI2B_MAX_COLLISION_*
BUF_BODY_CONTACT = 25  # [3][B]: stiffness, damping, friction (sai2b_set_body_contact)
BUF_BODY_CONTACT_STATUS = 26  # [9 + dof][B]: deepest penetration 3, witness index 3, sum of f_n 3, tb dof
COL_DISTANCE, COL_INDEX, COL_NORMAL, COL_GRADIENT, COL_CENTRES = 1, 2, 4, 8, 16  # enum sai2b_collision_block
COL_BLOCKS = {"distance": COL_DISTANCE, "index": COL_INDEX, "normal": COL_NORMAL, "gradient": COL_GRADIENT, "centres": COL_CENTRES}
COL_CATEGORIES = ("plane", "obstacle", "self")  # enum sai2b_collision_category
COL_FLAGS = {"plane": 1, "obstacle": 2, "self": 4, "nonfinite": 8}  # enum sai2b_collision_flag
DONE_COLLISION = 64  # SAI2B_DONE_COLLISION: the conventional bit of end_episodes
HARDWARE_SENSOR_ROWS = 13
WRENCH_WORLD, WRENCH_LINK = 0, 1  # enum sai2b_wrench_frame
WRENCH_FRAMES = {"world": WRENCH_WORLD, "link": WRENCH_LINK}
PAYLOAD_CONTROLLER, PAYLOAD_PLANT, PAYLOAD_BOTH = 1, 2, 3  # enum sai2b_payload_target
PAYLOAD_TARGETS = {"controller": PAYLOAD_CONTROLLER, "plant": PAYLOAD_PLANT, "both": PAYLOAD_BOTH}

_d = C.c_double
_i = C.c_int


class RobotModel(C.Structure):
    """struct sai2b_robot_model"""

    _fields_ = [
        ("dof", _i),
        ("joint_xyz", (_d * 3) * MAX_DOF),
        ("joint_rpy", (_d * 3) * MAX_DOF),
        ("link_mass", _d * MAX_DOF),
        ("link_com", (_d * 3) * MAX_DOF),
        ("link_inertia", (_d * 6) * MAX_DOF),
        ("q_lower", _d * MAX_DOF),
        ("q_upper", _d * MAX_DOF),
        ("effort", _d * MAX_DOF),
        ("gravity", _d * 3),
        ("joint_type", _i * MAX_DOF),
    ]


class TaskConfig(C.Structure):
    """struct sai2b_task_config"""

    _fields_ = [
        ("type", _i),
        ("name", C.c_char * 64),
        ("loop_timestep", _d),
        ("dynamic_decoupling_type", _i),
        ("bie_threshold", _d),
        # JointTask
        ("task_dof", _i),
        ("joint_selection", _d * (MAX_DOF * MAX_DOF)),
        ("kp", _d * MAX_DOF),
        ("kv", _d * MAX_DOF),
        ("ki", _d * MAX_DOF),
        ("use_velocity_saturation", _i),
        ("saturation_velocity", _d * MAX_DOF),
        # MotionForceTask
        ("link", _i),
        ("frame_pos", _d * 3),
        ("frame_rot", _d * 9),
        ("partial_projection", _d * 36),
        ("pos_range", _i),
        ("ori_range", _i),
        ("parametrization_in_compliant_frame", _i),
        ("kp_pos", _d * 3),
        ("kv_pos", _d * 3),
        ("ki_pos", _d * 3),
        ("kp_ori", _d * 3),
        ("kv_ori", _d * 3),
        ("ki_ori", _d * 3),
        ("kp_force", _d * 3),
        ("kv_force", _d * 3),
        ("ki_force", _d * 3),
        ("kp_moment", _d * 3),
        ("kv_moment", _d * 3),
        ("ki_moment", _d * 3),
        ("kff_force", _d),
        ("kff_moment", _d),
        ("max_force_feedback", _d),
        ("max_moment_feedback", _d),
        ("closed_loop_force", _i),
        ("closed_loop_moment", _i),
        ("passivity_enabled", _i),
        ("force_space_dimension", _i),
        ("moment_space_dimension", _i),
        ("force_axis", _d * 3),
        ("moment_axis", _d * 3),
        ("linear_saturation_velocity", _d),
        ("angular_saturation_velocity", _d),
        ("sensor_rot", _d * 9),
        ("sensor_pos", _d * 3),
        # SingularityHandler
        ("s_min", _d),
        ("s_max", _d),
        ("s_abs_tol", _d),
        ("type_1_tol", _d),
        ("type_2_torque_ratio", _d),
        ("type_2_angle_threshold", _d),
        ("perturb_step_size", _d),
        ("sh_buffer_size", _i),
        ("kp_type_1", _d),
        ("kv_type_1", _d),
        ("kv_type_2", _d),
        ("enforce_type_1_strategy", _i),
        ("enforce_handling_strategy", _i),
        ("singular_vector_sign", _i),
        # internal OTG
        ("use_internal_otg", _i),
        ("internal_otg_jerk_limited", _i),
        ("otg_max_velocity", _d * MAX_DOF),
        ("otg_max_acceleration", _d * MAX_DOF),
        ("otg_max_linear_velocity", _d),
        ("otg_max_linear_acceleration", _d),
        ("otg_max_angular_velocity", _d),
        ("otg_max_angular_acceleration", _d),
        ("otg_max_jerk", _d * MAX_DOF),
        ("otg_max_linear_jerk", _d),
        ("otg_max_angular_jerk", _d),
        ("unsafe_motion_gains", _i),
        ("robot_dof", _i),
    ]


URDF_MAX_LINKS = 32


class UrdfLinks(C.Structure):
    """sai2b_urdf_links"""

    _fields_ = [
        ("n_links", _i),
        ("name", (C.c_char * 64) * URDF_MAX_LINKS),
        ("moving_link", _i * URDF_MAX_LINKS),
        ("pos", (_d * 3) * URDF_MAX_LINKS),
        ("rot", (_d * 9) * URDF_MAX_LINKS),
    ]


def struct_to_dict(s):
    """Flatten a ctypes struct into plain python values (for comparisons in tests)."""
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Array):
            if isinstance(v, bytes):
                out[name] = v
            else:
                flat = []

                def rec(a):
                    for x in a:
                        if isinstance(x, C.Array):
                            rec(x)
                        else:
                            flat.append(x)

                rec(v)
                out[name] = flat
        else:
            out[name] = v
    return out


PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SAI2B_LIB") or os.path.join(PKG_DIR, "csrc", "libsai2b.so")

# every symbol include/sai2b.h declares (tests check that the built library exports all of them)
class ContactConfig(C.Structure):
    """sai2b_contact_config (include/sai2b.h "contact in the simulated plant")"""

    _fields_ = [
        ("link", _i),
        ("n_points", _i),
        ("points", (_d * 3) * MAX_CONTACT_POINTS),
        ("friction_velocity_eps", _d),
        ("sensor_task", _i),
    ]


# enum sai2b_observation_block / sai2b_observation_task_block / sai2b_done_reason (sai2b.h "observations and episode-end flags")
OBS_Q, OBS_DQ, OBS_TAU, OBS_LIMIT_MARGIN, OBS_EPISODE_STEP, OBS_CONTACT = 1, 2, 4, 8, 16, 32
OBS_POSE, OBS_TWIST, OBS_ERROR, OBS_SENSED = 1, 2, 4, 8
DONE_SUCCESS, DONE_JOINT_LIMIT, DONE_SPEED, DONE_NONFINITE, DONE_FORCE, DONE_TIMEOUT = 1, 2, 4, 8, 16, 32
DONE_REASONS = 6
# name -> flag, in storage order
OBS_BLOCKS = {"q": OBS_Q, "dq": OBS_DQ, "tau": OBS_TAU, "limit_margin": OBS_LIMIT_MARGIN, "episode_step": OBS_EPISODE_STEP,
              "contact": OBS_CONTACT}
OBS_TASK_BLOCKS = {"pose": OBS_POSE, "twist": OBS_TWIST, "error": OBS_ERROR, "sensed": OBS_SENSED}
DONE_BITS = {"success": DONE_SUCCESS, "joint_limit": DONE_JOINT_LIMIT, "speed": DONE_SPEED, "nonfinite": DONE_NONFINITE,
             "force": DONE_FORCE, "timeout": DONE_TIMEOUT}


class ObservationConfig(C.Structure):
    """sai2b_observation_config; load_library() checks the size against sai2b_sizeof_observation_config()"""

    _fields_ = [
        ("blocks", _i),
        ("task_mask", _i),
        ("task_blocks", _i),
        ("criteria", _i),
        ("success_task_mask", _i),
        ("force_task_mask", _i),
        ("max_episode_steps", _i),
        ("reserved", _i),
        ("pos_tolerance", _d),
        ("ori_tolerance", _d),
        ("joint_limit_margin", _d),
        ("max_joint_speed", _d * MAX_DOF),
        ("max_sensed_force", _d),
    ]


# enum sai2b_reward_term / sai2b_reward_task_term (sai2b.h "rewards and episode returns"); name -> flag, in storage order
REW_TERMS = {"alive": 1, "joint_speed": 2, "torque": 4, "torque_rate": 8, "limit": 16, "done": 32}
REW_TASK_TERMS = {"pos": 1, "pos_sq": 2, "pos_tanh": 4, "ori": 8, "ori_sq": 16, "ori_tanh": 32, "lin_vel_sq": 64, "ang_vel_sq": 128,
                  "force_err_sq": 256, "force_excess": 512}
REWARD_TERMS, REWARD_TASK_TERMS = 6, 10
REW_COUNTS = ("closed", "replaced")


class RewardConfig(C.Structure):
    """sai2b_reward_config; load_library() checks the size against sai2b_sizeof_reward_config()"""

    _fields_ = [
        ("terms", _i),
        ("task_mask", _i),
        ("task_terms", _i),
        ("reserved", _i),
        ("weight", _d * REWARD_TERMS),
        ("task_weight", (_d * REWARD_TASK_TERMS) * MAX_TASKS),
        ("done_value", _d * DONE_REASONS),
        ("limit_soft_margin", _d),
        ("pos_scale", _d * MAX_TASKS),
        ("ori_scale", _d * MAX_TASKS),
        ("force_soft_limit", _d * MAX_TASKS),
        ("gamma", _d),
        ("nonfinite_reward", _d),
    ]


class JointDynamicsConfig(C.Structure):
    """sai2b_joint_dynamics_config; load_library() checks the size against sai2b_sizeof_joint_dynamics_config()"""

    _fields_ = [
        ("stop_stiffness", _d * MAX_DOF),
        ("stop_damping", _d * MAX_DOF),
        ("friction_velocity_eps", _d * MAX_DOF),
    ]


class ExternalWrenchConfig(C.Structure):
    """sai2b_external_wrench_config; load_library() checks the size against sai2b_sizeof_external_wrench_config()"""

    _fields_ = [
        ("link", _i),
        ("frame", _i),
        ("point", _d * 3),
        ("sensor_task", _i),
    ]


class HardwareConfig(C.Structure):
    """sai2b_hardware_config; load_library() checks the size against sai2b_sizeof_hardware_config()"""

    _fields_ = [
        ("max_delay", _i),
        ("sensor_task", _i),
        ("first_robot", C.c_uint),
        ("reserved", _i),
        ("seed", C.c_ulonglong),
    ]


class JointSensorConfig(C.Structure):
    """sai2b_joint_sensor_config; load_library() checks the size against sai2b_sizeof_joint_sensor_config()"""

    _fields_ = [
        ("max_delay", _i),
        ("velocity_mode", _i),
        ("first_robot", C.c_uint),
        ("reserved", _i),
        ("seed", C.c_ulonglong),
    ]


class CollisionConfig(C.Structure):
    """sai2b_collision_config; load_library() checks the size against sai2b_sizeof_collision_config()"""

    _fields_ = [
        ("n_spheres", _i),
        ("n_planes", _i),
        ("n_obstacles", _i),
        ("blocks", _i),
        ("view", _i),
        ("env_mask", C.c_uint),
        ("pair_mask", C.c_uint * 16),
        ("link", _i * 16),
        ("centre", (C.c_double * 3) * 16),
        ("radius", C.c_double * 16),
        ("margin_plane", C.c_double),
        ("margin_obstacle", C.c_double),
        ("margin_self", C.c_double),
        ("reserved", _i * 8),
    ]


class BodyContactConfig(C.Structure):
    """sai2b_body_contact_config; load_library() checks the size against sai2b_sizeof_body_contact_config()"""

    _fields_ = [("categories", _i), ("reserved0", _i), ("v_eps", C.c_double), ("reserved", _i * 8)]


BODY_CONTACT_COUNTS = COL_CATEGORIES + ("any",)
IK_ROWS, IK_TASK_GOAL, IK_STATE = 0, 1, 1  # enum sai2b_ik_source
IK_FLAGS = {"converged": 1, "exhausted": 2, "at_limit": 4, "nonfinite": 8}  # enum sai2b_ik_flag
IK_COUNTS = ("selected", "converged", "exhausted", "nonfinite")
IK_STATUS_ROWS, IK_POSE_ROWS = 5, 12  # |e_pos|, |e_rot|, iterations, start index, mu; position 3 and rotation 9 row-major
IK_STREAM = 11  # the Philox stream of the restart seeds


class IkConfig(C.Structure):
    """sai2b_ik_config; load_library() checks the size against sai2b_sizeof_ik_config()"""

    _fields_ = [
        ("task", _i),
        ("axes", _i),
        ("max_iterations", _i),
        ("restarts", _i),
        ("use_limits", _i),
        ("view", _i),
        ("goal_source", _i),
        ("seed_source", _i),
        ("rot_length", C.c_double),
        ("tol_pos", C.c_double),
        ("tol_rot", C.c_double),
        ("mu0", C.c_double),
        ("mu_min", C.c_double),
        ("mu_max", C.c_double),
        ("mu_down", C.c_double),
        ("mu_up", C.c_double),
        ("step_max", C.c_double),
        ("limit_margin", C.c_double),
        ("rest_weight", C.c_double),
        ("seed", C.c_ulonglong),
        ("first_robot", C.c_uint),
        ("draw_id", C.c_uint),
        ("reserved", _i * 8),
    ]


MAX_RESET_TRIES = 64  # SAI2B_MAX_RESET_TRIES
RESET_SAMPLER_COUNTS = ("reset", "rejected", "exhausted")
RESET_SAMPLER_BLOCKS = {"q_lower": 0, "q_upper": 1, "dq_sigma": 2, "q_nominal": 3, "goal": 4}  # sai2b_reset_sampler_config_layout


class ResetSamplerConfig(C.Structure):
    """sai2b_reset_sampler_config; load_library() checks the size against sai2b_sizeof_reset_sampler_config()"""

    _fields_ = [
        ("seed", C.c_ulonglong),
        ("first_robot", C.c_uint),
        ("max_tries", _i),
        ("goal_tasks", C.c_uint),
        ("absolute_position", C.c_uint),
        ("ratio_task", _i),
        ("min_ratio", _d),
        ("box_task", _i),
        ("box_lower", _d * 3),
        ("box_upper", _d * 3),
        ("use_clearance", _i),
        ("clearance", _d),
    ]


# enum sai2b_env_group (sai2b.h "environment sampler"), in the order of the sample rows
ENV_PAYLOAD, ENV_CONTACT, ENV_JOINT_DYNAMICS, ENV_HARDWARE, ENV_PUSH = 1, 2, 4, 8, 16
ENV_GROUPS = {"payload": ENV_PAYLOAD, "contact": ENV_CONTACT, "joint_dynamics": ENV_JOINT_DYNAMICS, "hardware": ENV_HARDWARE, "push": ENV_PUSH}
ENV_SAMPLER_COUNTS = ("drawn", "lag_clipped")
BUF_ENV_SAMPLE = 20  # SAI2B_BUF_ENV_SAMPLE


class EnvRange(C.Structure):
    """sai2b_env_range"""

    _fields_ = [("lower", _d), ("upper", _d), ("log_uniform", _i), ("reserved", _i)]


class EnvSamplerConfig(C.Structure):
    """sai2b_env_sampler_config; load_library() checks the size against sai2b_sizeof_env_sampler_config()"""

    _fields_ = [
        ("seed", C.c_ulonglong),
        ("first_robot", C.c_uint),
        ("groups", C.c_uint),
        ("payload_target", _i),
        ("payload_mass_scale", EnvRange),
        ("payload_com_half", _d * 3),
        ("contact_height", EnvRange),
        ("contact_tilt_max", _d),
        ("contact_stiffness_scale", EnvRange),
        ("contact_damping_scale", EnvRange),
        ("contact_friction_scale", EnvRange),
        ("armature_scale", EnvRange),
        ("damping_scale", EnvRange),
        ("friction_scale", EnvRange),
        ("torque_limit_scale", EnvRange),
        ("delay_lower", _i),
        ("delay_upper", _i),
        ("lag_scale", EnvRange),
        ("gain_scale", EnvRange),
        ("torque_noise_scale", EnvRange),
        ("sensor_bias_half", _d * 6),
        ("sensor_noise_scale", EnvRange),
        ("push_force", EnvRange),
        ("push_moment", EnvRange),
        ("push_steps_lower", _i),
        ("push_steps_upper", _i),
    ]


ENV_RANGE_FIELDS = tuple(n for n, t in EnvSamplerConfig._fields_ if t is EnvRange)

# enum sai2b_action_mode / sai2b_action_block (sai2b.h "actions"); name -> value, blocks in row order
ACT_NONE, ACT_DELTA_GOAL, ACT_DELTA_CURRENT, ACT_ABSOLUTE = 0, 1, 2, 3
ACT_POSITION, ACT_ORIENTATION, ACT_FORCE, ACT_MOMENT = 1, 2, 4, 8
ACT_MODES = {"none": ACT_NONE, "delta_goal": ACT_DELTA_GOAL, "delta_current": ACT_DELTA_CURRENT, "absolute": ACT_ABSOLUTE}
ACT_BLOCKS = {"position": ACT_POSITION, "orientation": ACT_ORIENTATION, "force": ACT_FORCE, "moment": ACT_MOMENT}
ACT_COUNTS = ("rejected", "clipped", "limited")


class ActionTask(C.Structure):
    """sai2b_action_task"""

    _fields_ = [
        ("mode", _i),
        ("blocks", _i),
        ("pos_scale", _d * 3),
        ("ori_scale", _d),
        ("force_scale", _d),
        ("moment_scale", _d),
        ("pos_lower", _d * 3),
        ("pos_upper", _d * 3),
        ("max_pos_lead", _d),
        ("jt_scale", _d * MAX_DOF),
        ("jt_lower", _d * MAX_DOF),
        ("jt_upper", _d * MAX_DOF),
    ]


class ActionConfig(C.Structure):
    """sai2b_action_config; load_library() checks the size against sai2b_sizeof_action_config()"""

    _fields_ = [
        ("clip_actions", _i),
        ("reserved", _i),
        ("task", ActionTask * MAX_TASKS),
    ]


EXPORTS = [
    "sai2b_panda_model",
    "sai2b_model_merge_fixed_body",
    "sai2b_model_from_urdf",
    "sai2b_urdf_resolve_frame",
    "sai2b_model_set_base_transform",
    "sai2b_default_joint_task",
    "sai2b_default_joint_task_dof",
    "sai2b_default_motion_force_task",
    "sai2b_default_motion_force_task_dof",
    "sai2b_validate_tasks",
    "sai2b_create",
    "sai2b_destroy",
    "sai2b_last_error",
    "sai2b_batch",
    "sai2b_num_tasks",
    "sai2b_num_joints",
    "sai2b_update_task_config",
    "sai2b_enable_gravity_compensation",
    "sai2b_set_state",
    "sai2b_set_mft_goals",
    "sai2b_set_mft_goal_wrench",
    "sai2b_set_mft_sensed_wrench",
    "sai2b_set_jt_goals",
    "sai2b_reinitialize",
    "sai2b_reinitialize_robots",
    "sai2b_reset_robots",
    "sai2b_update_task_models",
    "sai2b_compute_control_torques",
    "sai2b_compute_control_torques_ex",
    "sai2b_tick",
    "sai2b_task_update_model",
    "sai2b_task_compute_torques",
    "sai2b_task_reinitialize",
    "sai2b_task_get_nullspaces",
    "sai2b_get_mft_singularity_state",
    "sai2b_get_mft_velocity",
    "sai2b_get_mft_sigma",
    "sai2b_set_mft_type1_posture",
    "sai2b_synchronize",
    "sai2b_stream",
    "sai2b_set_caller_stream",
    "sai2b_device_buffer",
    "sai2b_enable_introspection",
    "sai2b_get_task_nullspace",
    "sai2b_get_task_torques",
    "sai2b_get_mft_singularity",
    "sai2b_get_mft_task_forces",
    "sai2b_get_mft_status",
    "sai2b_get_mft_goals",
    "sai2b_get_jt_goals",
    "sai2b_reset_integrators",
    "sai2b_sim_step",
    "sai2b_get_state",
    "sai2b_get_bias",
    "sai2b_get_jt_desired",
    "sai2b_get_mft_desired",
    "sai2b_get_otg_status",
    "sai2b_get_model",
    "sai2b_profile_tick",
    "sai2b_device_count",
    "sai2b_get_fallback_count",
    "sai2b_get_worklist_state",
    "sai2b_counters",
    "sai2b_set_link_payload",
    "sai2b_clear_link_payload",
    "sai2b_get_link_payload",
    "sai2b_default_contact",
    "sai2b_validate_contact",
    "sai2b_set_contact",
    "sai2b_clear_contact",
    "sai2b_get_contact",
    "sai2b_get_contact_state",
    "sai2b_default_observation",
    "sai2b_validate_observation",
    "sai2b_sizeof_observation_config",
    "sai2b_observation_config_layout",
    "sai2b_set_observation",
    "sai2b_clear_observation",
    "sai2b_observation_rows",
    "sai2b_observation_layout",
    "sai2b_observe",
    "sai2b_get_done_counts",
    "sai2b_default_joint_dynamics",
    "sai2b_validate_joint_dynamics",
    "sai2b_sizeof_joint_dynamics_config",
    "sai2b_set_joint_dynamics",
    "sai2b_clear_joint_dynamics",
    "sai2b_get_joint_dynamics",
    "sai2b_get_joint_dynamics_state",
    "sai2b_default_external_wrench",
    "sai2b_validate_external_wrench",
    "sai2b_sizeof_external_wrench_config",
    "sai2b_set_external_wrench",
    "sai2b_clear_external_wrench",
    "sai2b_get_external_wrench",
    "sai2b_get_external_wrench_state",
    "sai2b_default_hardware",
    "sai2b_validate_hardware",
    "sai2b_sizeof_hardware_config",
    "sai2b_set_hardware",
    "sai2b_clear_hardware",
    "sai2b_get_hardware",
    "sai2b_get_hardware_state",
    "sai2b_default_action",
    "sai2b_validate_action",
    "sai2b_sizeof_action_config",
    "sai2b_action_config_layout",
    "sai2b_set_action",
    "sai2b_clear_action",
    "sai2b_action_rows",
    "sai2b_action_layout",
    "sai2b_apply_action",
    "sai2b_get_action_counts",
    "sai2b_default_reward",
    "sai2b_validate_reward",
    "sai2b_sizeof_reward_config",
    "sai2b_reward_config_layout",
    "sai2b_set_reward",
    "sai2b_clear_reward",
    "sai2b_reward_rows",
    "sai2b_reward_layout",
    "sai2b_observe_reward",
    "sai2b_get_reward_counts",
    "sai2b_get_episode_stats",
    "sai2b_default_reset_sampler",
    "sai2b_validate_reset_sampler",
    "sai2b_sizeof_reset_sampler_config",
    "sai2b_reset_sampler_config_layout",
    "sai2b_set_reset_sampler",
    "sai2b_clear_reset_sampler",
    "sai2b_get_reset_sampler",
    "sai2b_reset_robots_sampled",
    "sai2b_get_reset_sampler_counts",
    "sai2b_get_reset_sampler_state",
    "sai2b_default_env_sampler",
    "sai2b_validate_env_sampler",
    "sai2b_sizeof_env_sampler_config",
    "sai2b_env_sampler_config_layout",
    "sai2b_set_env_sampler",
    "sai2b_clear_env_sampler",
    "sai2b_get_env_sampler",
    "sai2b_randomize_robots",
    "sai2b_get_env_sampler_counts",
    "sai2b_get_env_sampler_state",
    "sai2b_default_joint_sensor",
    "sai2b_validate_joint_sensor",
    "sai2b_sizeof_joint_sensor_config",
    "sai2b_set_joint_sensor",
    "sai2b_clear_joint_sensor",
    "sai2b_get_joint_sensor",
    "sai2b_get_joint_sensor_state",
    "sai2b_get_measured_state",
    "sai2b_default_collision",
    "sai2b_validate_collision",
    "sai2b_sizeof_collision_config",
    "sai2b_collision_config_layout",
    "sai2b_set_collision",
    "sai2b_clear_collision",
    "sai2b_get_collision",
    "sai2b_collision_rows",
    "sai2b_collision_layout",
    "sai2b_collision_query",
    "sai2b_get_collision_counts",
    "sai2b_end_episodes",
    "sai2b_get_end_episode_count",
    "sai2b_default_body_contact",
    "sai2b_validate_body_contact",
    "sai2b_sizeof_body_contact_config",
    "sai2b_set_body_contact",
    "sai2b_clear_body_contact",
    "sai2b_get_body_contact",
    "sai2b_get_body_contact_state",
    "sai2b_default_ik",
    "sai2b_validate_ik",
    "sai2b_sizeof_ik_config",
    "sai2b_ik_input_rows",
    "sai2b_set_ik",
    "sai2b_clear_ik",
    "sai2b_get_ik",
    "sai2b_solve_ik",
    "sai2b_get_ik_counts",
    "sai2b_snapshot_words",
    "sai2b_snapshot_layout",
    "sai2b_snapshot_bank_create",
    "sai2b_snapshot_bank_destroy",
    "sai2b_snapshot_save",
    "sai2b_snapshot_load",
    "sai2b_get_snapshot_counts",
    "sai2b_snapshot_export_size",
    "sai2b_snapshot_export",
    "sai2b_snapshot_import",
]
# snapshot banks (sai2b.h "snapshot banks"): the groups, the blob's header and the block names of csrc/sai2b_snapshot_layout.h
SNAP_EPISODE, SNAP_ENVIRONMENT = 1, 2
SNAPSHOT_HEADER_BYTES = 256
SNAP_COUNTS = ("moved", "out_of_range", "never_saved")
SNAP_BLOCKS = ("q", "dq", "tau", "q_pose", "goals", "sensed", "state", "istate", "otg_desired", "otg_state", "otg3_traj", "popc_f", "popc_i",
               "popc_q", "N_prec", "episode_step", "wrench_remaining", "contact_status", "joint_status", "wrench_status", "payload",
               "plant_payload", "contact", "joint_dynamics", "external_wrench", "hw_history", "hw_filter", "hw_applied", "hw_clock",
               "hw_actuator", "hw_sensor", "reward_state", "reward_episode", "reset_sampler_episode")
# the blocks appended for the environment sampler, and every block id's name (enum SnapBlock of csrc/sai2b_snapshot_layout.h)
SNAP_ENV_SAMPLER_BLOCKS = ("env_sampler_counter", "env_sampler_sample")
SNAP_BLOCK_NAMES = SNAP_BLOCKS + SNAP_ENV_SAMPLER_BLOCKS
# the blocks appended for the joint sensors behind those, and the name of every block id there is
SNAP_JOINT_SENSOR_BLOCKS = ("joint_sensor_q", "joint_sensor_dq", "joint_sensor_previous", "joint_sensor_filter", "joint_sensor_history",
                            "joint_sensor_clock", "joint_sensor_rows")
SNAP_BLOCK_NAMES_ALL = SNAP_BLOCK_NAMES + SNAP_JOINT_SENSOR_BLOCKS

_lib = None


def load_library():
    """Load csrc/libsai2b.so (the HIP product library). Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback."
        )
    # torch (device memory / streams / torch.distributed plumbing) bundles its own HIP runtime with the
    # same SONAME as /opt/rocm's; two HIP runtimes in one process cannot both own the GPU, so make
    # sure torch's copy is the one already mapped before libsai2b.so resolves libamdhip64.so.7.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    P = C.POINTER
    dp = P(_d)
    vp = C.c_void_p
    lib.sai2b_panda_model.argtypes = [P(RobotModel)]
    lib.sai2b_model_merge_fixed_body.argtypes = [P(RobotModel), _i, dp, dp, _d, dp, dp]
    lib.sai2b_model_from_urdf.argtypes = [C.c_char_p, _i, P(RobotModel), P(UrdfLinks)]
    lib.sai2b_urdf_resolve_frame.argtypes = [P(UrdfLinks), C.c_char_p, dp, dp, P(_i), dp, dp]
    lib.sai2b_model_set_base_transform.argtypes = [P(RobotModel), dp, dp]
    lib.sai2b_default_joint_task.argtypes = [P(TaskConfig), C.c_char_p, _i, dp]
    lib.sai2b_default_joint_task_dof.argtypes = [P(TaskConfig), C.c_char_p, _i, _i, dp]
    lib.sai2b_default_motion_force_task_dof.argtypes = [P(TaskConfig), C.c_char_p, _i, _i, dp, dp, _i, dp, _i, dp]
    lib.sai2b_default_motion_force_task.argtypes = [P(TaskConfig), C.c_char_p, _i, dp, dp, _i, dp, _i, dp]
    lib.sai2b_validate_tasks.argtypes = [P(TaskConfig), _i, C.c_char_p, _i]
    lib.sai2b_create.argtypes = [P(RobotModel), P(TaskConfig), _i, _i, _i]
    lib.sai2b_create.restype = vp
    lib.sai2b_destroy.argtypes = [vp]
    lib.sai2b_destroy.restype = None
    lib.sai2b_last_error.argtypes = [vp]
    lib.sai2b_last_error.restype = C.c_char_p
    lib.sai2b_batch.argtypes = [vp]
    lib.sai2b_num_tasks.argtypes = [vp]
    lib.sai2b_num_joints.argtypes = [vp]
    lib.sai2b_update_task_config.argtypes = [vp, _i, P(TaskConfig)]
    lib.sai2b_enable_gravity_compensation.argtypes = [vp, _i]
    lib.sai2b_set_state.argtypes = [vp, vp, vp, _i]
    lib.sai2b_set_mft_goals.argtypes = [vp, _i, vp, vp, vp, vp, vp, vp, _i]
    lib.sai2b_set_mft_goal_wrench.argtypes = [vp, _i, vp, vp, _i]
    lib.sai2b_set_mft_sensed_wrench.argtypes = [vp, _i, vp, vp, _i]
    lib.sai2b_set_jt_goals.argtypes = [vp, _i, vp, vp, vp, _i]
    lib.sai2b_reinitialize.argtypes = [vp]
    lib.sai2b_reinitialize_robots.argtypes = [vp, _i, vp, _i]
    lib.sai2b_reset_robots.argtypes = [vp, vp, vp, vp, _i]
    lib.sai2b_update_task_models.argtypes = [vp]
    lib.sai2b_compute_control_torques.argtypes = [vp, vp, _i]
    lib.sai2b_compute_control_torques_ex.argtypes = [vp, vp, _i, _i]
    lib.sai2b_tick.argtypes = [vp, vp, _i]
    lib.sai2b_task_update_model.argtypes = [vp, _i, vp, _i]
    lib.sai2b_task_compute_torques.argtypes = [vp, _i, vp, vp, _i]
    lib.sai2b_task_reinitialize.argtypes = [vp, _i]
    lib.sai2b_task_get_nullspaces.argtypes = [vp, _i, vp, vp, vp]
    lib.sai2b_get_mft_singularity_state.argtypes = [vp, _i, vp, vp, vp]
    lib.sai2b_get_mft_velocity.argtypes = [vp, _i, vp, vp]
    lib.sai2b_get_mft_sigma.argtypes = [vp, _i, vp, vp, vp, vp]
    lib.sai2b_set_mft_type1_posture.argtypes = [vp, _i, vp, _i]
    lib.sai2b_synchronize.argtypes = [vp]
    lib.sai2b_stream.argtypes = [vp]
    lib.sai2b_stream.restype = vp
    lib.sai2b_set_caller_stream.argtypes = [vp, vp]
    lib.sai2b_device_buffer.argtypes = [vp, _i, _i]
    lib.sai2b_device_buffer.restype = vp
    lib.sai2b_enable_introspection.argtypes = [vp, _i]
    lib.sai2b_get_task_nullspace.argtypes = [vp, _i, vp]
    lib.sai2b_get_task_torques.argtypes = [vp, _i, vp]
    lib.sai2b_get_mft_singularity.argtypes = [vp, _i, vp, vp, vp]
    lib.sai2b_get_mft_task_forces.argtypes = [vp, _i, vp, vp]
    lib.sai2b_get_mft_status.argtypes = [vp, _i] + [vp] * 8
    lib.sai2b_get_mft_goals.argtypes = [vp, _i] + [vp] * 8
    lib.sai2b_get_jt_goals.argtypes = [vp, _i, vp, vp, vp]
    lib.sai2b_reset_integrators.argtypes = [vp, _i, _i]
    lib.sai2b_sim_step.argtypes = [vp, vp, _i, _d, _i, _i]
    lib.sai2b_get_state.argtypes = [vp, vp, vp]
    lib.sai2b_get_bias.argtypes = [vp, _i, vp]
    lib.sai2b_get_jt_desired.argtypes = [vp, _i, vp, vp, vp]
    lib.sai2b_get_mft_desired.argtypes = [vp, _i, vp, vp, vp, vp, vp, vp]
    lib.sai2b_get_otg_status.argtypes = [vp, _i, vp, vp]
    lib.sai2b_get_model.argtypes = [vp, _i, vp, vp, vp, vp]
    lib.sai2b_profile_tick.argtypes = [vp, _i, P(_d), P(_d)]
    lib.sai2b_get_fallback_count.argtypes = [vp, P(_i)]
    lib.sai2b_get_worklist_state.argtypes = [vp, P(_i), P(_i), P(_i), P(_i)]
    lib.sai2b_counters.argtypes = [vp, P(C.c_longlong), P(C.c_longlong)]
    lib.sai2b_set_link_payload.argtypes = [vp, _i, _i, vp, vp, vp, _i]
    lib.sai2b_clear_link_payload.argtypes = [vp, _i]
    lib.sai2b_get_link_payload.argtypes = [vp, _i, P(_i), vp, vp, vp]
    lib.sai2b_default_contact.argtypes = [P(ContactConfig), _i, _i, P(_d)]
    lib.sai2b_validate_contact.argtypes = [P(ContactConfig), P(TaskConfig), _i, _i, C.c_char_p, _i]
    lib.sai2b_set_contact.argtypes = [vp, P(ContactConfig), vp, vp, vp, vp, vp, _i]
    lib.sai2b_clear_contact.argtypes = [vp]
    lib.sai2b_get_contact.argtypes = [vp, P(ContactConfig), vp]
    lib.sai2b_get_contact_state.argtypes = [vp, vp, vp, vp, P(_i)]
    lib.sai2b_default_observation.argtypes = [P(ObservationConfig)]
    lib.sai2b_validate_observation.argtypes = [P(ObservationConfig), P(TaskConfig), _i, _i, C.c_char_p, _i]
    lib.sai2b_sizeof_observation_config.argtypes = []
    lib.sai2b_observation_config_layout.argtypes = [P(ObservationConfig), _i, _i, _i, P(_i), P(_i), P(_i)]
    lib.sai2b_set_observation.argtypes = [vp, P(ObservationConfig)]
    lib.sai2b_clear_observation.argtypes = [vp]
    lib.sai2b_observation_rows.argtypes = [vp]
    lib.sai2b_observation_layout.argtypes = [vp, _i, _i, P(_i), P(_i)]
    lib.sai2b_observe.argtypes = [vp, vp, vp, _i]
    lib.sai2b_get_done_counts.argtypes = [vp, P(_i)]
    lib.sai2b_default_joint_dynamics.argtypes = [P(JointDynamicsConfig), _i]
    lib.sai2b_validate_joint_dynamics.argtypes = [P(JointDynamicsConfig), _i, C.c_char_p, _i]
    lib.sai2b_sizeof_joint_dynamics_config.argtypes = []
    lib.sai2b_set_joint_dynamics.argtypes = [vp, P(JointDynamicsConfig), vp, vp, vp, vp, vp, vp, _i]
    lib.sai2b_clear_joint_dynamics.argtypes = [vp]
    lib.sai2b_get_joint_dynamics.argtypes = [vp, P(JointDynamicsConfig), vp]
    lib.sai2b_get_joint_dynamics_state.argtypes = [vp, vp, vp, vp, P(_i), P(_i)]
    if lib.sai2b_sizeof_joint_dynamics_config() != C.sizeof(JointDynamicsConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_joint_dynamics_config is {lib.sai2b_sizeof_joint_dynamics_config()} bytes in the library, "
                           f"{C.sizeof(JointDynamicsConfig)} in the ctypes mirror")
    if lib.sai2b_sizeof_observation_config() != C.sizeof(ObservationConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_observation_config is {lib.sai2b_sizeof_observation_config()} bytes in the library, "
                           f"{C.sizeof(ObservationConfig)} in the ctypes mirror")
    lib.sai2b_default_action.argtypes = [P(ActionConfig)]
    lib.sai2b_validate_action.argtypes = [P(ActionConfig), P(TaskConfig), _i, _i, C.c_char_p, _i]
    lib.sai2b_sizeof_action_config.argtypes = []
    lib.sai2b_action_config_layout.argtypes = [P(ActionConfig), P(TaskConfig), _i, _i, _i, P(_i), P(_i), P(_i)]
    lib.sai2b_set_action.argtypes = [vp, P(ActionConfig)]
    lib.sai2b_clear_action.argtypes = [vp]
    lib.sai2b_action_rows.argtypes = [vp]
    lib.sai2b_action_layout.argtypes = [vp, _i, _i, P(_i), P(_i)]
    lib.sai2b_apply_action.argtypes = [vp, vp, vp, _i]
    lib.sai2b_get_action_counts.argtypes = [vp, P(_i)]
    if lib.sai2b_sizeof_action_config() != C.sizeof(ActionConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_action_config is {lib.sai2b_sizeof_action_config()} bytes in the library, "
                           f"{C.sizeof(ActionConfig)} in the ctypes mirror")
    lib.sai2b_default_reward.argtypes = [P(RewardConfig)]
    lib.sai2b_validate_reward.argtypes = [P(RewardConfig), P(TaskConfig), _i, _i, C.c_char_p, _i]
    lib.sai2b_sizeof_reward_config.argtypes = []
    lib.sai2b_reward_config_layout.argtypes = [P(RewardConfig), _i, _i, P(_i), P(_i), P(_i)]
    lib.sai2b_set_reward.argtypes = [vp, P(RewardConfig)]
    lib.sai2b_clear_reward.argtypes = [vp]
    lib.sai2b_reward_rows.argtypes = [vp]
    lib.sai2b_reward_layout.argtypes = [vp, _i, _i, P(_i), P(_i)]
    lib.sai2b_observe_reward.argtypes = [vp, vp, vp, vp, vp, _i]
    lib.sai2b_get_reward_counts.argtypes = [vp, P(_i)]
    lib.sai2b_get_episode_stats.argtypes = [vp, vp, vp, vp, vp]
    if lib.sai2b_sizeof_reward_config() != C.sizeof(RewardConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_reward_config is {lib.sai2b_sizeof_reward_config()} bytes in the library, "
                           f"{C.sizeof(RewardConfig)} in the ctypes mirror")
    lib.sai2b_default_external_wrench.argtypes = [P(ExternalWrenchConfig), _i]
    lib.sai2b_validate_external_wrench.argtypes = [P(ExternalWrenchConfig), P(TaskConfig), _i, _i, C.c_char_p, _i]
    lib.sai2b_sizeof_external_wrench_config.argtypes = []
    lib.sai2b_set_external_wrench.argtypes = [vp, P(ExternalWrenchConfig), vp, vp, vp, _i]
    lib.sai2b_clear_external_wrench.argtypes = [vp]
    lib.sai2b_get_external_wrench.argtypes = [vp, P(ExternalWrenchConfig), vp]
    lib.sai2b_get_external_wrench_state.argtypes = [vp, vp, vp, P(_i)]
    if lib.sai2b_sizeof_external_wrench_config() != C.sizeof(ExternalWrenchConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_external_wrench_config is {lib.sai2b_sizeof_external_wrench_config()} bytes in the library, "
                           f"{C.sizeof(ExternalWrenchConfig)} in the ctypes mirror")
    lib.sai2b_snapshot_words.argtypes = [vp, _i]
    lib.sai2b_snapshot_layout.argtypes = [vp, _i, P(_i), _i]
    lib.sai2b_snapshot_bank_create.argtypes = [vp, _i, _i, P(vp)]
    lib.sai2b_snapshot_bank_destroy.argtypes = [vp]
    lib.sai2b_snapshot_bank_destroy.restype = None
    lib.sai2b_snapshot_save.argtypes = [vp, vp, vp, vp, _i]
    lib.sai2b_snapshot_load.argtypes = [vp, vp, vp, vp, _i]
    lib.sai2b_get_snapshot_counts.argtypes = [vp, P(_i)]
    lib.sai2b_snapshot_export_size.argtypes = [vp]
    lib.sai2b_snapshot_export_size.restype = C.c_size_t
    lib.sai2b_snapshot_export.argtypes = [vp, vp, C.c_size_t]
    lib.sai2b_snapshot_import.argtypes = [vp, vp, C.c_size_t]
    lib.sai2b_default_hardware.argtypes = [P(HardwareConfig)]
    lib.sai2b_validate_hardware.argtypes = [P(HardwareConfig), P(TaskConfig), _i, _i, C.c_char_p, _i]
    lib.sai2b_sizeof_hardware_config.argtypes = []
    lib.sai2b_set_hardware.argtypes = [vp, P(HardwareConfig), vp, vp, _i]
    lib.sai2b_clear_hardware.argtypes = [vp]
    lib.sai2b_get_hardware.argtypes = [vp, P(HardwareConfig), vp, vp]
    lib.sai2b_get_hardware_state.argtypes = [vp, vp, vp, vp]
    lib.sai2b_default_joint_sensor.argtypes = [P(JointSensorConfig)]
    lib.sai2b_validate_joint_sensor.argtypes = [P(JointSensorConfig), _i, C.c_char_p, _i]
    lib.sai2b_sizeof_joint_sensor_config.argtypes = []
    lib.sai2b_set_joint_sensor.argtypes = [vp, P(JointSensorConfig), vp, _i]
    lib.sai2b_clear_joint_sensor.argtypes = [vp]
    lib.sai2b_get_joint_sensor.argtypes = [vp, P(JointSensorConfig), vp]
    lib.sai2b_get_joint_sensor_state.argtypes = [vp, vp, vp]
    lib.sai2b_get_measured_state.argtypes = [vp, vp, vp]
    lib.sai2b_default_collision.argtypes = [P(CollisionConfig), _i, vp, vp, vp]
    lib.sai2b_validate_collision.argtypes = [P(CollisionConfig), _i, C.c_char_p, _i]
    lib.sai2b_sizeof_collision_config.argtypes = []
    lib.sai2b_collision_config_layout.argtypes = [P(CollisionConfig), _i, _i, _i, P(_i), P(_i), P(_i), P(_i)]
    lib.sai2b_set_collision.argtypes = [vp, P(CollisionConfig), vp, _i]
    lib.sai2b_clear_collision.argtypes = [vp]
    lib.sai2b_get_collision.argtypes = [vp, P(CollisionConfig), vp]
    lib.sai2b_collision_rows.argtypes = [vp]
    lib.sai2b_collision_layout.argtypes = [vp, _i, _i, P(_i), P(_i)]
    lib.sai2b_collision_query.argtypes = [vp, vp, vp, _i]
    lib.sai2b_get_collision_counts.argtypes = [vp, P(_i)]
    lib.sai2b_end_episodes.argtypes = [vp, vp, vp, _i, _i]
    lib.sai2b_get_end_episode_count.argtypes = [vp, P(_i)]
    lib.sai2b_default_body_contact.argtypes = [P(BodyContactConfig)]
    lib.sai2b_validate_body_contact.argtypes = [P(BodyContactConfig), _i, C.c_char_p, _i]
    lib.sai2b_sizeof_body_contact_config.argtypes = []
    lib.sai2b_set_body_contact.argtypes = [vp, P(BodyContactConfig), vp, _i]
    lib.sai2b_clear_body_contact.argtypes = [vp]
    lib.sai2b_get_body_contact.argtypes = [vp, P(BodyContactConfig), vp]
    lib.sai2b_get_body_contact_state.argtypes = [vp, vp, P(_i)]
    lib.sai2b_default_ik.argtypes = [P(IkConfig)]
    lib.sai2b_validate_ik.argtypes = [P(IkConfig), _i, vp, vp, C.c_char_p, _i]
    lib.sai2b_sizeof_ik_config.argtypes = []
    lib.sai2b_ik_input_rows.argtypes = [P(IkConfig), _i, P(_i), P(_i)]
    lib.sai2b_set_ik.argtypes = [vp, P(IkConfig)]
    lib.sai2b_clear_ik.argtypes = [vp]
    lib.sai2b_get_ik.argtypes = [vp, P(IkConfig)]
    lib.sai2b_solve_ik.argtypes = [vp, vp, vp, vp, vp, vp, vp, _i]
    lib.sai2b_get_ik_counts.argtypes = [vp, P(_i)]
    if lib.sai2b_sizeof_ik_config() != C.sizeof(IkConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_ik_config is {lib.sai2b_sizeof_ik_config()} bytes in the library, "
                           f"{C.sizeof(IkConfig)} in the ctypes mirror")
    if lib.sai2b_sizeof_body_contact_config() != C.sizeof(BodyContactConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_body_contact_config is {lib.sai2b_sizeof_body_contact_config()} bytes in the library, "
                           f"{C.sizeof(BodyContactConfig)} in the ctypes mirror")
    if lib.sai2b_sizeof_collision_config() != C.sizeof(CollisionConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_collision_config is {lib.sai2b_sizeof_collision_config()} bytes in the library, "
                           f"{C.sizeof(CollisionConfig)} in the ctypes mirror")
    if lib.sai2b_sizeof_joint_sensor_config() != C.sizeof(JointSensorConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_joint_sensor_config is {lib.sai2b_sizeof_joint_sensor_config()} bytes in the library, "
                           f"{C.sizeof(JointSensorConfig)} in the ctypes mirror")
    if lib.sai2b_sizeof_hardware_config() != C.sizeof(HardwareConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_hardware_config is {lib.sai2b_sizeof_hardware_config()} bytes in the library, "
                           f"{C.sizeof(HardwareConfig)} in the ctypes mirror")
    lib.sai2b_default_reset_sampler.argtypes = [P(ResetSamplerConfig)]
    lib.sai2b_validate_reset_sampler.argtypes = [P(ResetSamplerConfig), P(TaskConfig), _i, _i, C.c_char_p, _i]
    lib.sai2b_sizeof_reset_sampler_config.argtypes = []
    lib.sai2b_reset_sampler_config_layout.argtypes = [P(ResetSamplerConfig), P(TaskConfig), _i, _i, _i, _i, P(_i), P(_i), P(_i)]
    lib.sai2b_set_reset_sampler.argtypes = [vp, P(ResetSamplerConfig), vp, _i]
    lib.sai2b_clear_reset_sampler.argtypes = [vp]
    lib.sai2b_get_reset_sampler.argtypes = [vp, P(ResetSamplerConfig), vp]
    lib.sai2b_reset_robots_sampled.argtypes = [vp, vp, _i]
    lib.sai2b_get_reset_sampler_counts.argtypes = [vp, P(_i)]
    lib.sai2b_get_reset_sampler_state.argtypes = [vp, vp, vp]
    if lib.sai2b_sizeof_reset_sampler_config() != C.sizeof(ResetSamplerConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_reset_sampler_config is {lib.sai2b_sizeof_reset_sampler_config()} bytes in the library, "
                           f"{C.sizeof(ResetSamplerConfig)} in the ctypes mirror")
    lib.sai2b_default_env_sampler.argtypes = [P(EnvSamplerConfig)]
    lib.sai2b_validate_env_sampler.argtypes = [P(EnvSamplerConfig), _i, C.c_char_p, _i]
    lib.sai2b_sizeof_env_sampler_config.argtypes = []
    lib.sai2b_env_sampler_config_layout.argtypes = [P(EnvSamplerConfig), _i, _i, P(_i), P(_i), P(_i)]
    lib.sai2b_set_env_sampler.argtypes = [vp, P(EnvSamplerConfig)]
    lib.sai2b_clear_env_sampler.argtypes = [vp]
    lib.sai2b_get_env_sampler.argtypes = [vp, P(EnvSamplerConfig)]
    lib.sai2b_randomize_robots.argtypes = [vp, vp, C.c_uint, _i]
    lib.sai2b_get_env_sampler_counts.argtypes = [vp, P(_i)]
    lib.sai2b_get_env_sampler_state.argtypes = [vp, vp, vp]
    if lib.sai2b_sizeof_env_sampler_config() != C.sizeof(EnvSamplerConfig):
        raise RuntimeError(f"{LIB_PATH}: sai2b_env_sampler_config is {lib.sai2b_sizeof_env_sampler_config()} bytes in the library, "
                           f"{C.sizeof(EnvSamplerConfig)} in the ctypes mirror")
    _lib = lib
    return lib
