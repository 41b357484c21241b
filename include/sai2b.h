/*
 * sai2b.h — C ABI of the batched operational-space controller for MI355X.
 *
 * This is the drop-in boundary for the hot path
 *     RobotController::updateControllerTaskModels()   (reference src/RobotController.cpp:53-60)
 *     RobotController::computeControlTorques()        (reference src/RobotController.cpp:62-74)
 * and the task objects they drive (MotionForceTask, SingularityHandler, JointTask).
 * The reference has no C ABI (it is a static C++ library, CMakeLists.txt:70); the entry points
 * below are what a C++ adapter inside sai2-primitives would bind, and each one
 * cites the reference member function it replaces.
 *
 * Conventions
 *   - all numeric data is IEEE double
 *   - batched arrays are SoA, batch-minor:  a[c * B + b]  = component c of robot b  ("[C][B]")
 *   - matrices inside a component index are row-major (R[3*i+j], N[7*i+j], ...)
 *   - a ctx owns every device buffer; callers copy in/out with sai2b_set_ / sai2b_get_, or write
 *     device-resident data straight into the ctx buffers returned by sai2b_device_buffer()
 *   - every function returns 0 on success, nonzero on error; sai2b_last_error() has the text.
 *     Argument errors correspond to the reference's std::invalid_argument throws.
 */
#ifndef SAI2B_H_
#define SAI2B_H_

#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SAI2B_MAX_DOF 8	  /* joints of the largest supported robot; the library holds builds for 4, 6, 7 and 8 */
#define SAI2B_DOF 7		  /* the Panda's, the default of the helpers that take no robot (source compatibility) */
#define SAI2B_MAX_TASKS 4 /* tasks in one controller hierarchy */
#define SAI2B_MAX_CONTACT_POINTS 4 /* contact points of the simulated plant (sai2b_contact_config) */
#define SAI2B_SH_HISTORY 200 /* SingularityHandler.cpp:16 BUFFER_SIZE */

/* reference src/tasks/TemplateTask.h:19-23 */
enum sai2b_task_type {
	SAI2B_UNDEFINED = 0,
	SAI2B_JOINT_TASK = 1,
	SAI2B_MOTION_FORCE_TASK = 2
};

/* reference src/helper_modules/Sai2PrimitivesCommonDefinitions.h:9-15 */
enum sai2b_decoupling {
	SAI2B_FULL_DYNAMIC_DECOUPLING = 0,
	SAI2B_BOUNDED_INERTIA_ESTIMATES = 1,
	SAI2B_IMPEDANCE = 2
};

/* Orientation of the singular vectors the singularity classification perturbs along. The reference classifies a
 * singular direction by forward kinematics at q + 5 * V_s[:, i] (SingularityHandler.cpp:253-265) where V_s comes out
 * of Eigen::JacobiSVD (:78-81), and a singular vector is only defined up to its sign: FK(q + 5 v) and FK(q - 5 v) are
 * different poses, so "type 1" vs "type 2" — two different control strategies (:328-351) — can depend on a sign Eigen
 * does not specify and this library cannot reproduce without Eigen. The convention is therefore DEFINED here and
 * selectable per MotionForceTask; how many robots it matters for is measured in tests/test_gpu_svd_sign.py and
 * recorded in DESIGN.md §2 / INTEGRATION.md §6. Nothing else on the path depends on the sign (every other use of
 * U_s, V_s is a product v v^T or an absolute value). */
enum sai2b_singular_vector_sign {
	SAI2B_SV_SIGN_V_MAX_POSITIVE = 0, /* default: the largest-magnitude component of V_s[:, i] is positive */
	SAI2B_SV_SIGN_V_MAX_NEGATIVE = 1, /* the opposite orientation */
	SAI2B_SV_SIGN_EITHER = 2,		  /* sign-free: type 1 if the perturbation along +v OR -v moves the task */
	SAI2B_SV_SIGN_BOTH = 3			  /* sign-free: type 1 only if both do */
};

/* error codes */
enum sai2b_status {
	SAI2B_OK = 0,
	SAI2B_INVALID_ARGUMENT = 1, /* reference: std::invalid_argument */
	SAI2B_RUNTIME_ERROR = 2,	/* HIP failure */
	SAI2B_UNSUPPORTED = 3
};

/* reference: the joint types sai2-model reads from a URDF that the examples use (revolute / continuous,
 * prismatic: examples/06-partial_joint_task/panda_arm_sliding_base.urdf) */
enum sai2b_joint_type {
	SAI2B_REVOLUTE = 0,
	SAI2B_PRISMATIC = 1
};

/*
 * Rigid-body model of a fixed-base serial chain with `dof` joints (4, 6, 7 or 8), each moving about (revolute)
 * or along (prismatic) the z axis of its joint frame (the subset of sai2-model the path needs: reference call
 * sites SURVEY §8(c)). A URDF joint with another <axis> is brought to this form by rotating its joint frame and
 * re-expressing what hangs on it, which sai2b_model_from_urdf() does.
 * Joint i connects link i-1 (parent) to link i; link -1 is the world/base.
 * Fixed children (e.g. the Panda "end-effector" body, panda_arm.urdf:105-116,179-183) must be merged
 * into their parent's inertial parameters with sai2b_model_merge_fixed_body().
 * Arrays are sized for SAI2B_MAX_DOF; entries >= dof are ignored.
 */
typedef struct sai2b_robot_model {
	int dof;
	double joint_xyz[SAI2B_MAX_DOF][3];				   /* URDF <origin xyz>, in parent link frame */
	double joint_rpy[SAI2B_MAX_DOF][3];				   /* URDF <origin rpy>  (R = Rz(y) Ry(p) Rx(r)) */
	double link_mass[SAI2B_MAX_DOF];				   /* child link of joint i */
	double link_com[SAI2B_MAX_DOF][3];				   /* COM in link frame */
	double link_inertia[SAI2B_MAX_DOF][6];			   /* ixx iyy izz ixy ixz iyz at the COM, link axes */
	double q_lower[SAI2B_MAX_DOF], q_upper[SAI2B_MAX_DOF]; /* joint limits (SingularityHandler.cpp:43-51) */
	double effort[SAI2B_MAX_DOF];
	double gravity[3]; /* world gravity used by jointGravityVector (RobotController.cpp:71) */
	int joint_type[SAI2B_MAX_DOF]; /* enum sai2b_joint_type */
} sai2b_robot_model;

/*
 * One task of the hierarchy. Field defaults are filled by sai2b_default_joint_task() /
 * sai2b_default_motion_force_task() and mirror JointTask.h:31-45, MotionForceTask.h:40-75,
 * MotionForceTask.cpp:197 and SingularityHandler.cpp:10-20. Everything here is batch-uniform.
 */
typedef struct sai2b_task_config {
	int type; /* enum sai2b_task_type */
	char name[64];
	double loop_timestep;
	int dynamic_decoupling_type; /* enum sai2b_decoupling */
	double bie_threshold;

	/* ---- JointTask (JointTask.cpp:14-89) ---- */
	int task_dof;								  /* rows of the selection matrix (the robot's dof if full) */
	double joint_selection[SAI2B_MAX_DOF * SAI2B_MAX_DOF]; /* row-major task_dof x robot_dof, packed (row stride = robot_dof) */
	double kp[SAI2B_MAX_DOF], kv[SAI2B_MAX_DOF], ki[SAI2B_MAX_DOF];
	int use_velocity_saturation; /* shared flag name for both task types */
	double saturation_velocity[SAI2B_MAX_DOF];

	/* ---- MotionForceTask (MotionForceTask.cpp:16-202) ---- */
	int link;						/* 0-based moving link the compliant frame is attached to */
	double frame_pos[3];			/* compliant frame in link frame: translation */
	double frame_rot[9];			/*                               rotation (row-major) */
	double partial_projection[36];	/* _partial_task_projection, blkdiag(P_pos, P_ori) */
	int pos_range, ori_range;		/* ranks of the two 3x3 blocks (MotionForceTask.cpp:151-152) */
	int parametrization_in_compliant_frame;
	double kp_pos[3], kv_pos[3], ki_pos[3];
	double kp_ori[3], kv_ori[3], ki_ori[3];
	double kp_force[3], kv_force[3], ki_force[3];
	double kp_moment[3], kv_moment[3], ki_moment[3];
	double kff_force, kff_moment;
	double max_force_feedback, max_moment_feedback;
	int closed_loop_force, closed_loop_moment;
	int passivity_enabled; /* MotionForceTask::enablePassivity (MotionForceTask.h:629): POPC on the force loop */
	int force_space_dimension, moment_space_dimension;
	double force_axis[3], moment_axis[3];
	double linear_saturation_velocity, angular_saturation_velocity;
	double sensor_rot[9], sensor_pos[3]; /* _T_control_to_sensor (MotionForceTask.cpp:793-803) */

	/* ---- SingularityHandler (SingularityHandler.cpp:10-73, MotionForceTask.cpp:197) ---- */
	double s_min, s_max, s_abs_tol;
	double type_1_tol, type_2_torque_ratio, type_2_angle_threshold, perturb_step_size;
	int sh_buffer_size;
	double kp_type_1, kv_type_1, kv_type_2;
	int enforce_type_1_strategy, enforce_handling_strategy;
	int singular_vector_sign; /* enum sai2b_singular_vector_sign: classifySingularity's perturbation direction */

	/* ---- internal online trajectory generation (JointTask.h:38-42,294-324;
	 * MotionForceTask.h:67-74,387-427): on by default, acceleration-limited. The desired state fed
	 * to the control law is the OTG's next state instead of the goal. ---- */
	int use_internal_otg;		   /* enableInternalOtgAccelerationLimited / ...JerkLimited / disableInternalOtg */
	int internal_otg_jerk_limited; /* enableInternalOtgJerkLimited (JointTask.h:295-310, MotionForceTask.h:416): ruckig's
									* third-order interface with the otg_max_*jerk limits below; switching between the two
									* modes re-initialises the generator at the task's current pose, as the reference does
									* (JointTask.cpp:374,399; MotionForceTask.cpp:514,529) */
	double otg_max_velocity[SAI2B_MAX_DOF], otg_max_acceleration[SAI2B_MAX_DOF]; /* JointTask, per task dof */
	double otg_max_linear_velocity, otg_max_linear_acceleration;		 /* MotionForceTask */
	double otg_max_angular_velocity, otg_max_angular_acceleration;
	double otg_max_jerk[SAI2B_MAX_DOF];							 /* JointTask, per task dof (JointTask.h:42: 10 pi) */
	double otg_max_linear_jerk, otg_max_angular_jerk;			 /* MotionForceTask (MotionForceTask.h:73-74: 10, 10 pi) */

	/* MotionForceTask::setPosControlGainsUnsafe / setOriControlGainsUnsafe (MotionForceTask.h:283,304;
	 * MotionForceTask.cpp:630-649) and JointTask::setGainsUnsafe (JointTask.h:256, JointTask.cpp:136-156): nonzero
	 * skips the sign check of the motion gains */
	int unsafe_motion_gains;

	/* joints of the robot the task is for (filled by the sai2b_default_* helpers; 0 is read as SAI2B_DOF) */
	int robot_dof;
} sai2b_task_config;

typedef struct sai2b_ctx sai2b_ctx;

/* ------------------------------------------------------------------ model / config helpers
 * (host-only, no GPU needed) */

/* Panda arm constants (examples/15-haptic_control_impedance_type/panda_arm.urdf:4-184), with the
 * fixed "end-effector" body merged into link 7 (dof = 7). */
int sai2b_panda_model(sai2b_robot_model* model);

/* Merge a fixed child body into link `link` (what RBDL does for URDF fixed joints). */
int sai2b_model_merge_fixed_body(sai2b_robot_model* model, int link, const double xyz[3],
								 const double rpy[3], double mass, const double com[3],
								 const double inertia[6]);

/* URDF ingestion (host-only). The reference loads robots from URDF through sai2-model (e.g.
 * examples/05-using_robot_controller/05-using_robot_controller.cpp:45-47 with panda_arm.urdf): this
 * reads the same files into a sai2b_robot_model. Scope: one serial chain of 4, 6, 7 or 8 revolute / continuous /
 * prismatic joints with any <axis> (panda_arm.urdf; examples/06-partial_joint_task/panda_arm_sliding_base.urdf;
 * examples/11-planar_robot_controller/rrrrbot.urdf), any fixed joints (the bodies behind them are
 * merged into the link they hang on, as RBDL does), rotated <inertial> frames. `urdf` is a file name
 * (is_file != 0) or the XML text. `links` (may be NULL) receives, for every URDF link, the moving
 * link it is rigidly attached to (-1: the world) and its fixed pose there. */
#define SAI2B_URDF_MAX_LINKS 32
typedef struct sai2b_urdf_links {
	int n_links;
	char name[SAI2B_URDF_MAX_LINKS][64];
	int moving_link[SAI2B_URDF_MAX_LINKS];
	double pos[SAI2B_URDF_MAX_LINKS][3];
	double rot[SAI2B_URDF_MAX_LINKS][9]; /* row-major */
} sai2b_urdf_links;
int sai2b_model_from_urdf(const char* urdf, int is_file, sai2b_robot_model* model,
						  sai2b_urdf_links* links);
/* Sai2Model::setTRobotBase (examples/05-using_robot_controller/05-using_robot_controller.cpp:69): the pose of the
 * robot's base in the world. The reference's tasks work in the WORLD frame (MotionForceTask.cpp:100-103,262,
 * 286-289: positionInWorld / rotationInWorld / JWorldFrame) and the model's gravity is a world vector, so the
 * transform is folded into the first joint's origin: link -1 of the model is the world afterwards, goals, poses,
 * forces and Jacobians of a MotionForceTask are world quantities, jointGravityVector sees the rotated base.
 * Host-only; call it on the model BEFORE sai2b_create() (a context copies the model); a second call composes on
 * top of the first. rot: row-major rotation matrix, NULL = identity. */
int sai2b_model_set_base_transform(sai2b_robot_model* model, const double pos[3], const double* rot);
/* MotionForceTask takes a link NAME and a compliant frame in that link (MotionForceTask.h:96-101,
 * e.g. "end-effector", a body on a fixed joint of link7): resolve them to the moving link index and
 * the frame in it that sai2b_default_motion_force_task() takes. rot_in_link / frame_rot may be NULL. */
int sai2b_urdf_resolve_frame(const sai2b_urdf_links* links, const char* link_name,
							 const double pos_in_link[3], const double* rot_in_link, int* moving_link,
							 double frame_pos[3], double frame_rot[9]);

/* JointTask::JointTask + initialSetup defaults (JointTask.cpp:14-89, JointTask.h:31-45).
 * selection == NULL -> full joint task; else row-major task_dof x 7, must be full row rank
 * (JointTask.cpp:34-39). */
int sai2b_default_joint_task(sai2b_task_config* cfg, const char* name, int task_dof,
							 const double* selection);
/* the same for a robot with `robot_dof` joints (selection: row-major task_dof x robot_dof) */
int sai2b_default_joint_task_dof(sai2b_task_config* cfg, const char* name, int robot_dof, int task_dof,
								 const double* selection);

/* MotionForceTask::MotionForceTask + initialSetup defaults (MotionForceTask.cpp:16-202).
 * n_trans/n_rot < 0 -> full 6-DOF task (first ctor); otherwise the partial-task ctor with the given
 * controlled directions (row-major n x 3). frame_rot may be NULL (identity). */
int sai2b_default_motion_force_task(sai2b_task_config* cfg, const char* name, int link,
									const double frame_pos[3], const double* frame_rot,
									int n_trans, const double* dirs_trans, int n_rot,
									const double* dirs_rot);
/* the same for a robot with `robot_dof` joints (link < robot_dof) */
int sai2b_default_motion_force_task_dof(sai2b_task_config* cfg, const char* name, int robot_dof, int link,
										const double frame_pos[3], const double* frame_rot,
										int n_trans, const double* dirs_trans, int n_rot,
										const double* dirs_rot);

/* RobotController ctor checks (RobotController.cpp:8-51): at least one task, same loop timestep,
 * unique names, nothing after a full joint task. Returns SAI2B_INVALID_ARGUMENT with `msg` filled. */
int sai2b_validate_tasks(const sai2b_task_config* tasks, int n_tasks, char* msg, int msg_len);

/* ------------------------------------------------------------------ controller (needs a GPU) */

/* RobotController::RobotController (RobotController.cpp:8-51) for `batch` robot instances on HIP
 * device `device`. Validates like the reference; allocates all device buffers; goals are
 * initialised as reInitializeTask() does once a state has been set. Returns NULL on failure
 * (see sai2b_last_error(NULL)). */
sai2b_ctx* sai2b_create(const sai2b_robot_model* model, const sai2b_task_config* tasks, int n_tasks,
						int batch, int device);
void sai2b_destroy(sai2b_ctx* ctx);
const char* sai2b_last_error(const sai2b_ctx* ctx);

int sai2b_batch(const sai2b_ctx* ctx);
int sai2b_num_tasks(const sai2b_ctx* ctx);
int sai2b_num_joints(const sai2b_ctx* ctx); /* joints of the context's robot */

/* Re-configure batch-uniform task parameters (gains, decoupling, force-space parametrisation,
 * flags) after creation — the reference's setters (MotionForceTask.h:272-328,576-623,669-753,
 * JointTask.h:234-259,360-384). Structural fields (type, task_dof, selection, link, projection)
 * must not change. The setters' side effects follow the fields that changed:
 *  - use_internal_otg / otg_max_*: enableInternalOtgAccelerationLimited (JointTask.cpp:360-381,
 *    MotionForceTask.cpp:511-523): a generator that was off starts at the task's current pose;
 *  - force_space_dimension / force_axis (axis compared normalised, for dimension 1 or 2):
 *    parametrizeForceMotionSpaces (MotionForceTask.cpp:830-858): goal position := current position, goal
 *    linear velocity / acceleration := 0, the linear half of the generator re-initialised there, position
 *    and force integrators reset; moment_space_dimension / moment_axis: the angular counterpart (:860-890);
 *  - closed_loop_force / closed_loop_moment: the corresponding integrators reset (:973-986);
 *  - passivity_enabled: the observer re-initialised (POPCExplicitForceControl.cpp:24-28).
 * "Current" pose = the task's cached one: that of the last torque computation or re-initialisation. */
int sai2b_update_task_config(sai2b_ctx* ctx, int task, const sai2b_task_config* cfg);

/* RobotController::enableGravityCompensation (RobotController.h:31-33) */
int sai2b_enable_gravity_compensation(sai2b_ctx* ctx, int enable);

/* Sai2Model::setQ / setDq + updateModel (examples/05-using_robot_controller.cpp:143-145).
 * q, dq: [dof][B] (here and below "7" in a shape stands for the robot's dof). on_device != 0 -> the pointers are device memory. */
int sai2b_set_state(sai2b_ctx* ctx, const double* q, const double* dq, int on_device);

/* MotionForceTask::setGoalPosition/Orientation/LinearVelocity/AngularVelocity/
 * LinearAcceleration/AngularAcceleration (MotionForceTask.h:211-247). Any pointer may be NULL
 * (left unchanged). pos,v,w,a,alpha: [3][B]; rot: [9][B] row-major. */
int sai2b_set_mft_goals(sai2b_ctx* ctx, int task, const double* pos, const double* rot,
						const double* lin_vel, const double* ang_vel, const double* lin_acc,
						const double* ang_acc, int on_device);
/* MotionForceTask::setGoalForce / setGoalMoment (MotionForceTask.h:590-623): [3][B] each */
int sai2b_set_mft_goal_wrench(sai2b_ctx* ctx, int task, const double* force, const double* moment,
							  int on_device);
/* MotionForceTask::updateSensedForceAndMoment (MotionForceTask.cpp:805-828): sensor-frame values,
 * [3][B] each; resolved to the world frame with the current state when the tick runs. */
int sai2b_set_mft_sensed_wrench(sai2b_ctx* ctx, int task, const double* force, const double* moment,
								int on_device);
/* JointTask::setGoalPosition/Velocity/Acceleration (JointTask.h:137-179): [task_dof][B] each */
int sai2b_set_jt_goals(sai2b_ctx* ctx, int task, const double* q_goal, const double* dq_goal,
					   const double* ddq_goal, int on_device);

/* RobotController::reinitializeTasks (RobotController.cpp:76-80): goals <- current state,
 * integrators and singularity history cleared. */
int sai2b_reinitialize(sai2b_ctx* ctx);

/* The same for the robots with mask[b] != 0 only; the others are not touched (every buffer column stays bit-equal, and so
 * does every later tick). task = -1: every task (RobotController::reinitializeTasks), else that one
 * (TemplateTask::reInitializeTask). mask: [B] bytes, host, or device when on_device != 0 (then the call is ordered on the
 * ctx stream under the stream contract below and does not synchronise). One launch, whatever the mask selects. */
int sai2b_reinitialize_robots(sai2b_ctx* ctx, int task, const unsigned char* mask, int on_device);
/* Episode reset of the robots with mask[b] != 0: their columns of q and dq ([dof][B], only the selected columns are
 * read; either may be NULL = keep) become the state, then every task is re-initialised for them as above. Two things
 * beyond that are this library's definition (the reference has no batch, and its reInitializeTask leaves the observer
 * alone): the selected robots' passivity observers, where a task has one, are re-initialised
 * (POPCExplicitForceControl.cpp:10-22), and their columns of SAI2B_BUF_TAU are zeroed, so that a simulation step on the
 * stored torques does not push a fresh robot with its old episode's. Payload rows, contact rows, the contact-state
 * outputs, the joint-dynamics rows and their status are kept for every robot (environment, not episode). All pointers
 * host, or all device (on_device). */
int sai2b_reset_robots(sai2b_ctx* ctx, const unsigned char* mask, const double* q, const double* dq, int on_device);

/* RobotController::updateControllerTaskModels (RobotController.cpp:53-60) */
int sai2b_update_task_models(sai2b_ctx* ctx);
/* RobotController::computeControlTorques (RobotController.cpp:62-74). tau: [7][B]; may be NULL
 * (result stays in the ctx torque buffer). with_compensation == 0 reproduces the manual flow of
 * examples 04/18 (no-argument computeTorques(), torques summed). */
int sai2b_compute_control_torques(sai2b_ctx* ctx, double* tau, int on_device);
int sai2b_compute_control_torques_ex(sai2b_ctx* ctx, double* tau, int on_device,
									 int with_compensation);
/* update_task_models + compute_control_torques for the current state in ONE fused launch: the
 * batched hot path. Enqueued on the ctx stream; does not synchronise when tau == NULL. */
int sai2b_tick(sai2b_ctx* ctx, double* tau, int on_device);
/* ------------------------------------------------------------------ task-level plugin interface
 * The reference's tasks can be driven one by one, without a RobotController, through the virtuals of
 * TemplateTask (src/tasks/TemplateTask.h:42-88) — examples/01-joint_control.cpp:131-191,
 * examples/04-task_and_redundancy.cpp:141-150,188-206, examples/18. The same calls on task `task` of a ctx
 * (a ctx with ONE task is a standalone task object; tasks of one ctx share the robot state of
 * sai2b_set_state). The caller chains the nullspaces itself:
 *     sai2b_task_update_model(ctx, 0, NULL, 0);                 // N_prec = identity
 *     sai2b_task_get_nullspaces(ctx, 0, NULL, NULL, N01);       // getTaskAndPreviousNullspace()
 *     sai2b_task_update_model(ctx, 1, N01, 0);
 *     sai2b_task_compute_torques(ctx, 0, NULL, tau0, 0);        // computeTorques()
 *     sai2b_task_compute_torques(ctx, 1, tau0, tau1, 0);        // computeTorques(tau_prec)
 * Nothing is assumed about the tasks above: range decisions always take the SVD path. */
/* TemplateTask::updateTaskModel(N_prec) (TemplateTask.h:42; JointTask.cpp:218-283, MotionForceTask.cpp:247-268).
 * N_prec: [n*n][B] row-major inside the component index, NULL = identity. The singularity bookkeeping of a
 * MotionForceTask (SingularityHandler.cpp:230-295) advances once per call, as in the reference. */
int sai2b_task_update_model(sai2b_ctx* ctx, int task, const double* N_prec, int on_device);
/* TemplateTask::computeTorques() (tau_prec == NULL, TemplateTask.h:49) and computeTorques(tau_prec) (:58): the
 * task's own torques [n][B] under the N_prec of the last sai2b_task_update_model (identity when there was none,
 * the value a task is constructed with). Integrators and the task's internal OTG advance as in the reference.
 * A MotionForceTask ignores tau_prec (its compensation term is identically zero: MotionForceTask.cpp:270-276
 * with the never-assigned _Lambda, :140); a JointTask subtracts Jp^T R M_partial R^T S M^-1 tau_prec
 * (JointTask.cpp:285-292). Task models are those of the CURRENT state (never stale, see DESIGN.md "split API").
 * tau may be NULL (the result stays on the device). */
int sai2b_task_compute_torques(sai2b_ctx* ctx, int task, const double* tau_prec, double* tau, int on_device);
/* TemplateTask::reInitializeTask (TemplateTask.h:65; JointTask.cpp:91-107, MotionForceTask.cpp:204-245) of one task */
int sai2b_task_reinitialize(sai2b_ctx* ctx, int task);
/* TemplateTask::getTaskNullspace / getPreviousTasksNullspace / getTaskAndPreviousNullspace (TemplateTask.h:73-88)
 * of the last sai2b_task_update_model / sai2b_task_compute_torques of that task: host arrays [n*n][B], any NULL */
int sai2b_task_get_nullspaces(sai2b_ctx* ctx, int task, double* N_task, double* N_prec, double* N_total);

/* wait for everything enqueued on the ctx stream */
int sai2b_synchronize(sai2b_ctx* ctx);
/* the hipStream_t the ctx launches on (as void*) */
void* sai2b_stream(sai2b_ctx* ctx);
/* Stream contract for DEVICE-pointer arguments (every `on_device != 0` above and below). The ctx works on its own
 * non-blocking stream. A device input is read after everything the caller has enqueued on ITS stream up to the
 * call (the producer kernels) and the read is finished before anything the caller enqueues on that stream after
 * the call returns (so the buffer may be overwritten at once); a device result (tau with on_device) is complete
 * when the call returns. The caller's stream is the legacy default stream unless set here (pass the hipStream_t,
 * e.g. torch.cuda.current_stream().cuda_stream). Host-pointer arguments are always complete on return.
 * Buffers handed out by sai2b_device_buffer() are outside this contract: order them with sai2b_stream(). */
int sai2b_set_caller_stream(sai2b_ctx* ctx, void* stream);

/* Device-resident ctx buffers, for zero-copy producers/consumers. `which`: */
enum sai2b_buffer {
	SAI2B_BUF_Q = 0,	  /* [7][B]  */
	SAI2B_BUF_DQ = 1,	  /* [7][B]  */
	SAI2B_BUF_TAU = 2,	  /* [7][B]  */
	SAI2B_BUF_GOALS = 3,  /* per task; MFT: [30][B] = pos3 rot9 v3 w3 a3 alpha3 f3 m3; JT: [3k][B] */
	SAI2B_BUF_SENSED = 4, /* per MFT task: [6][B] sensor-frame force, moment */
	SAI2B_BUF_STATE = 5,  /* per task persistent state, see DESIGN.md */
	/* outputs of the task-level calls (sai2b_task_update_model), [n*n][B]: a manual hierarchy chains them on the device —
	 * sai2b_task_update_model(ctx, next, sai2b_device_buffer(ctx, SAI2B_BUF_TASK_N_TOTAL, task), 1) — instead of through
	 * sai2b_task_get_nullspaces() and the host. NULL before the task's first task-level call. */
	SAI2B_BUF_TASK_N = 6,		/* the task's nullspace N (getTaskNullspace) */
	SAI2B_BUF_TASK_N_TOTAL = 7,	/* N * N_prec (getTaskAndPreviousNullspace) */
	/* per-robot payload rows (sai2b_set_link_payload), [10][B] = mass, com 3, inertia 6 (ixx iyy izz ixy ixz iyz): the
	 * controller's set and the plant's. NULL until a payload has been set for that target (and after it is cleared). A
	 * device-resident producer may rewrite the rows between ticks, ordered with sai2b_stream(); the next tick / sim step
	 * reads them. Such rows are not inspected. */
	SAI2B_BUF_PAYLOAD = 8,
	SAI2B_BUF_PLANT_PAYLOAD = 9,
	/* the plant's contact rows (sai2b_set_contact), [9][B] = plane point 3, unit normal 3, stiffness, damping, friction. NULL
	 * until a contact has been set (and after it is cleared). A device-resident producer may rewrite the rows between steps,
	 * ordered with sai2b_stream(); the next sai2b_sim_step reads them. Such rows are not inspected. */
	SAI2B_BUF_CONTACT = 10,
	/* the plant's joint-dynamics rows (sai2b_set_joint_dynamics), [6][dof][B] = armature, damping, friction, torque limit,
	 * lower limit, upper limit, and what the last step left, [3][dof][B] = applied, stop and dissipative torque. NULL until
	 * joint dynamics have been set (and after they are cleared). A device-resident producer may rewrite the rows between
	 * steps, ordered with sai2b_stream(); the next sai2b_sim_step reads them. Such rows are not inspected. */
	SAI2B_BUF_JOINT_DYNAMICS = 11,
	SAI2B_BUF_JOINT_DYNAMICS_STATE = 12,
	/* the plant's external-wrench rows (sai2b_set_external_wrench), [7][B] = force 3, moment 3, remaining pushed periods, and
	 * what the last step left, [6 + dof][B] = F_w 3, M_w 3, the joint torques tx. NULL until an external wrench has been set
	 * (and after it is cleared). A device-resident producer may rewrite the rows between steps, ordered with sai2b_stream();
	 * the next sai2b_sim_step reads them. Such rows are not inspected. */
	SAI2B_BUF_EXTERNAL_WRENCH = 13,
	SAI2B_BUF_EXTERNAL_WRENCH_STATE = 14,
	/* the actuator rows [1 + 3 dof][B] and the sensor rows [13][B] of sai2b_set_hardware, and the torques the plant received in
	 * the last sai2b_sim_step, [dof][B]. NULL until hardware has been set (and after it is cleared). A device-resident producer
	 * may rewrite the two row buffers between steps, ordered with sai2b_stream(); the next sai2b_sim_step reads them. Such rows
	 * are not inspected. */
	SAI2B_BUF_HARDWARE_ACTUATOR = 15,
	SAI2B_BUF_HARDWARE_SENSOR = 16,
	SAI2B_BUF_TAU_APPLIED = 17,
	/* the reward's per-robot accumulators (sai2b_set_reward): [3 + dof][B] doubles = running discounted return, running discount,
	 * return of the episode that ended last, tau_prev [dof]; and [2][B] ints = length of the episode that ended last, tau_prev is
	 * valid. NULL until a reward has been set (and after it is cleared). */
	SAI2B_BUF_REWARD_STATE = 18,
	SAI2B_BUF_REWARD_EPISODE = 19,
	/* what the environment sampler (sai2b_set_env_sampler) drew for every robot, [total_rows][B] doubles in the layout of
	 * sai2b_env_sampler_config_layout: the scales, offsets, height, tilt angle and axis, delay and push themselves, privileged
	 * information for a critic or an identification network. Zero for a robot that has not been drawn yet. NULL until a sampler has
	 * been set (and after it is cleared). */
	SAI2B_BUF_ENV_SAMPLE = 20,
	/* the controller's view of the joint state (sai2b_set_joint_sensor): the measured q and dq, [dof][B] each, and the per-robot
	 * rows [1 + 5 dof][B]. NULL until a joint sensor has been set (and after it is cleared). SAI2B_BUF_Q / SAI2B_BUF_DQ stay what
	 * sai2b_sim_step integrates: the truth, privileged information for a critic. A device-resident producer may rewrite the rows
	 * between steps, ordered with sai2b_stream(); the next sai2b_sim_step reads them. Such rows are not inspected. */
	SAI2B_BUF_Q_MEASURED = 21,
	SAI2B_BUF_DQ_MEASURED = 22,
	SAI2B_BUF_JOINT_SENSOR = 23,
	/* the per-robot environment rows of the collision proximity (sai2b_set_collision), [6 P + 4 O][B] = per plane point 3 and
	 * unit normal 3, per obstacle centre 3 and radius. NULL until a collision configuration with a plane or an obstacle has been
	 * set (and after it is cleared). A device-resident producer may rewrite the rows (move an obstacle every period), ordered
	 * with sai2b_stream(); the next sai2b_collision_query reads them. Such rows are not inspected. */
	SAI2B_BUF_COLLISION = 24,
	/* the rows of the whole-arm contact (sai2b_set_body_contact), [3][B] = stiffness, damping, friction, and what the last
	 * sai2b_sim_step left, [9 + dof][B] = per category the deepest penetration 3, its witness index 3, the sum of the normal
	 * forces 3, then the joint torques tb. NULL until a whole-arm contact has been set (and after it is cleared). A
	 * device-resident producer may rewrite the rows between steps, ordered with sai2b_stream(); such rows are not inspected. */
	SAI2B_BUF_BODY_CONTACT = 25,
	SAI2B_BUF_BODY_CONTACT_STATUS = 26
};
/* (A producer that writes q through SAI2B_BUF_Q bypasses the bookkeeping of the tasks' cached pose: an OTG
 * enabled / a space re-parametrised after such a write and before the next tick starts from the state as
 * written, not from the pose of the last torque computation.) */
void* sai2b_device_buffer(sai2b_ctx* ctx, int which, int task);

/* Optional per-robot outputs of the last tick (debug / observers such as
 * POPCBilateralTeleoperation.cpp:81-92). Introspection must be enabled BEFORE the tick whose values
 * are wanted (it selects a kernel variant that also stores these arrays); the getters fail with
 * SAI2B_INVALID_ARGUMENT otherwise. Arrays are host pointers; any may be NULL. */
int sai2b_enable_introspection(sai2b_ctx* ctx, int enable);
/* TemplateTask::getTaskAndPreviousNullspace (TemplateTask.h:88): [49][B] */
int sai2b_get_task_nullspace(sai2b_ctx* ctx, int task, double* N_total);
/* per-task torque contribution of the last tick: [7][B] */
int sai2b_get_task_torques(sai2b_ctx* ctx, int task, double* tau_task);
/* MFT: singular values [6][B], blending alpha [B], split index (non-singular rank) [B] as doubles */
int sai2b_get_mft_singularity(sai2b_ctx* ctx, int task, double* sigma, double* alpha,
							  double* ns_rank);
/* MFT, no introspection needed: the SingularityHandler's state after the last model update
 * (SingularityHandler.h:211-215) per robot, int [B] each, any may be NULL: number of singular directions
 * (_singularity_types.size(), 0 = fully non-singular), _type_1_counter, _type_2_counter. */
int sai2b_get_mft_singularity_state(sai2b_ctx* ctx, int task, int* n_singular, int* type_1_count,
									int* type_2_count);
/* MFT: unit-mass motion force and force-related terms of the last tick, [6][B] each — what
 * MotionForceTask::getUnitMassForce and the observers of POPCBilateralTeleoperation.cpp:81-92,172-182
 * read (MotionForceTask.cpp:478-487) */
int sai2b_get_mft_task_forces(sai2b_ctx* ctx, int task, double* F_unit, double* F_force);
/* ------------------------------------------------------------------ per-robot payloads
 * One extra rigid body per robot, fixed to moving link `link` (0-based, as sai2b_task_config.link), different for every
 * robot of the batch: what a robot holds, or a tool whose mass is randomised per environment. Everything else of the model
 * (sai2b_robot_model) stays shared by the batch. Two independent sets per context:
 *   SAI2B_PAYLOAD_CONTROLLER  what M, g, Lambda, the nullspaces and the torques are computed with (every tick kernel, the
 *                             task-level calls, the M of sai2b_get_model),
 *   SAI2B_PAYLOAD_PLANT       what sai2b_sim_step integrates and sai2b_get_bias reports;
 * setting both (SAI2B_PAYLOAD_BOTH) is the common case, setting them apart models a controller that is wrong about its load.
 * mass [B] (kg), com [3][B] (metres, in the link's frame; NULL: zeros), inertia [6][B] (about the body's own COM, link axes,
 * ixx iyy izz ixy ixz iyz as sai2b_robot_model.inertia; NULL: a point mass). Zero mass and inertia: nothing attached to that
 * robot. Host arrays are validated (SAI2B_INVALID_ARGUMENT: link outside [0, dof), negative or non-finite mass, non-finite com
 * or inertia, negative ixx / iyy / izz); DEVICE arrays (on_device != 0) are copied as they are and NOT inspected. The call is
 * ordered on the ctx stream like the goal setters and takes effect at the next tick / sim step. Kinematics, Jacobians, the
 * singularity handling and the trajectory generators never see a payload; sai2b_reinitialize keeps it (model, not task
 * state). A context that never sets one, or has cleared it, launches the kernels it would without this feature. */
enum sai2b_payload_target { SAI2B_PAYLOAD_CONTROLLER = 1, SAI2B_PAYLOAD_PLANT = 2, SAI2B_PAYLOAD_BOTH = 3 };
int sai2b_set_link_payload(sai2b_ctx* ctx, int target, int link, const double* mass, const double* com,
						   const double* inertia, int on_device);
/* back to the kernels and results of a context without a payload (the rows are kept for a later set, the buffer ids give NULL) */
int sai2b_clear_link_payload(sai2b_ctx* ctx, int target);
/* the rows of ONE target (SAI2B_PAYLOAD_CONTROLLER or SAI2B_PAYLOAD_PLANT) to host arrays, any may be NULL; *link = -1 and
 * zeros when that target has no payload */
int sai2b_get_link_payload(sai2b_ctx* ctx, int target, int* link, double* mass, double* com, double* inertia);

/* ------------------------------------------------------------------ contact in the simulated plant
 * A compliant contact model inside sai2b_sim_step and a simulated force / moment sensor, so that a force-controlled closed
 * loop (tick, sai2b_sim_step(NULL), tick, ...) never leaves the device. Batch-uniform: the moving link the contact geometry
 * is fixed to, 1 to 4 contact points in that link's frame (one: a probe tip; four corners of a plate: surface-surface
 * contact with moments), the friction regularisation speed (m/s, > 0) and the MotionForceTask whose sensed rows the sensor
 * writes (-1: no sensor). Per robot: one plane (point and outward unit normal, world frame), stiffness k (N/m), damping d
 * (s/m, Hunt-Crossley form) and friction coefficient mu. For point k with world position x and velocity v at the START of
 * a substep:
 *     delta = n . (p0 - x)     vn = n . v     f_n = max(0, k max(0, delta) (1 - d vn))     v_t = v - vn n
 *     F = f_n n - mu f_n v_t / sqrt(|v_t|^2 + eps^2)            (the force ON the robot, world frame)
 * and the substep is  dq += h M^-1 (tau + sum_k J_k^T F_k - b),  q += h dq. Every piece is continuous in the state. This
 * law and the integrator are this library's definitions, not sai2-simulation's. The sensor is ideal (contact wrench only):
 * after the last substep of a period it stores the wrench the robot applies to the environment, in the sensor frame of
 * `sensor_task` (its sensor_rot / sensor_pos), into that task's SAI2B_BUF_SENSED rows; the next tick consumes them.
 * sai2b_set_mft_sensed_wrench on that task keeps working (last writer wins, ordered on the ctx stream). */
typedef struct sai2b_contact_config {
	int link;					   /* moving link the points are fixed to (0-based, as sai2b_task_config.link) */
	int n_points;				   /* 1 .. SAI2B_MAX_CONTACT_POINTS */
	double points[SAI2B_MAX_CONTACT_POINTS][3]; /* in the link's frame, metres */
	double friction_velocity_eps;  /* m/s, > 0: below it friction fades to zero linearly */
	int sensor_task;			   /* index of a MotionForceTask, or -1 */
} sai2b_contact_config;
/* host only: n_points points ([n_points][3], NULL: one point at the link origin), eps = 1e-3 m/s, no sensor */
int sai2b_default_contact(sai2b_contact_config* cfg, int link, int n_points, const double* points);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg (link outside [0, robot_dof), n_points outside
 * [1, 4], a non-finite point, eps not > 0, sensor_task neither -1 nor a MotionForceTask of `tasks`) */
int sai2b_validate_contact(const sai2b_contact_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof,
						   char* msg, int msg_len);
/* plane_point [3][B], plane_normal [3][B], stiffness [B], damping [B] (NULL: 0), friction [B] (NULL: 0). Host arrays are
 * validated (SAI2B_INVALID_ARGUMENT: what sai2b_validate_contact rejects, non-finite anything, negative stiffness / damping /
 * friction, a normal whose length is not within 1e-9 of 1); DEVICE arrays (on_device != 0) are copied as they are and NOT
 * inspected. Ordered on the ctx stream; takes effect at the next sai2b_sim_step. sai2b_reinitialize keeps it (plant, not
 * task state); sai2b_get_bias and every tick kernel never see it. Stiffness 0 for a robot: nothing touches that robot. A
 * context that never sets a contact, or has cleared it, launches the simulation kernel it would without this feature. */
int sai2b_set_contact(sai2b_ctx* ctx, const sai2b_contact_config* cfg, const double* plane_point, const double* plane_normal,
					  const double* stiffness, const double* damping, const double* friction, int on_device);
/* back to the plant without contact (the rows are kept for a later set, SAI2B_BUF_CONTACT gives NULL, no sensor writes) */
int sai2b_clear_contact(sai2b_ctx* ctx);
/* the configuration and the [9][B] rows to the host (either may be NULL); cfg->n_points = 0 and zeros without a contact */
int sai2b_get_contact(sai2b_ctx* ctx, sai2b_contact_config* cfg, double* rows);
/* what the last sai2b_sim_step left, from the state after its last substep, host arrays, any NULL: depth [4][B] (delta per
 * point, > 0 inside the surface; rows of unused points 0), normal_force [4][B], wrench_world [6][B] = sum F_k and
 * sum (x_k - x_c) x F_k (x_c: the control point of the sensor task, the contact link's origin without one),
 * *robots_in_contact = robots with some f_n > 0 (counted on the device). Zeros before the first step with a contact. */
int sai2b_get_contact_state(sai2b_ctx* ctx, double* depth, double* normal_force, double* wrench_world, int* robots_in_contact);

/* ------------------------------------------------------------------ joint dynamics of the simulated plant
 * Armature, viscous damping, Coulomb friction, actuator saturation and joint stops inside sai2b_sim_step, different for every
 * robot of the batch. Per robot and joint i, rows [dof][B] each: armature a_i >= 0 (reflected rotor inertia, kg m^2 for a
 * revolute joint, kg for a prismatic one), damping d_i >= 0, Coulomb friction level f_i >= 0, torque limit t_i > 0 (+inf: none),
 * lower and upper limit lo_i < hi_i (-inf / +inf: none). Batch-uniform, per joint (sai2b_joint_dynamics_config): stop stiffness
 * k_i >= 0, stop damping c_i >= 0 (Hunt-Crossley form, s/rad or s/m) and the friction regularisation speed e_i > 0 (rad/s or
 * m/s). One substep of length h from the state (q, dq) at its START, the commanded torque tau held over the period:
 *     ts_i = min(max(tau_i, -t_i), t_i)                                  actuator saturation
 *     sl_i = max(0, k_i max(0, lo_i - q_i) (1 - c_i dq_i))               lower stop, pushes +
 *     su_i = max(0, k_i max(0, q_i - hi_i) (1 + c_i dq_i))               upper stop, pushes -
 *     g_i  = d_i + f_i / sqrt(dq_i^2 + e_i^2)                            damping + regularised Coulomb friction as a
 *                                                                        state-dependent damper: torque = -g_i dq_i
 *     (M + diag(a) + h diag(g)) dq+ = (M + diag(a)) dq + h (ts + sl - su + tc - b)
 *     q+ = q + h dq+
 * M and b are the plant's (with its payload, if it has one), tc is the contact torque of the section above when a contact is
 * set and zero otherwise. Every piece is continuous in the state. The dissipative term is taken at the NEW velocity
 * (linear-implicit), so a large friction slope f / e or a large d on a light outer link does not limit the step; the stop
 * spring is explicit, as the contact spring is. With a = d = f = 0, t = +inf and lo, hi = -/+inf the step is algebraically
 * the one of a context without joint dynamics, dq += h M^-1 (tau - b), but not bit-equal to it: a context gets this kernel
 * only after it asks for it. This law is this library's definition, not sai2-simulation's.
 * SAI2B_OBS_LIMIT_MARGIN and SAI2B_DONE_JOINT_LIMIT keep reading the limits of the context's MODEL (sai2b_robot_model), not
 * these rows; the tick kernels, the singularity handling and sai2b_get_bias never see joint dynamics. */
typedef struct sai2b_joint_dynamics_config {
	double stop_stiffness[SAI2B_MAX_DOF], stop_damping[SAI2B_MAX_DOF], friction_velocity_eps[SAI2B_MAX_DOF]; /* entries >= dof are ignored */
} sai2b_joint_dynamics_config;
/* host only: k = 0, c = 0, e = 1e-2 for every joint */
int sai2b_default_joint_dynamics(sai2b_joint_dynamics_config* cfg, int robot_dof);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg (a negative or non-finite stop_stiffness or
 * stop_damping, a friction_velocity_eps that is not finite and > 0, among the first robot_dof entries) */
int sai2b_validate_joint_dynamics(const sai2b_joint_dynamics_config* cfg, int robot_dof, char* msg, int msg_len);
/* sizeof(sai2b_joint_dynamics_config) as the library was compiled, for bindings that mirror the struct */
int sai2b_sizeof_joint_dynamics_config(void);
/* armature, damping, friction, torque_limit, q_lower, q_upper: [dof][B] each; NULL = that effect off (zeros for armature,
 * damping and friction, +inf for the torque limit, -inf / +inf for the limits). Host arrays are validated
 * (SAI2B_INVALID_ARGUMENT: what sai2b_validate_joint_dynamics rejects, a negative or non-finite armature, damping or friction,
 * a NaN limit, a torque limit that is not > 0, q_lower >= q_upper); DEVICE arrays (on_device != 0) are copied as they are and
 * NOT inspected. Ordered on the ctx stream; takes effect at the next sai2b_sim_step. sai2b_reinitialize, sai2b_reset_robots and
 * sai2b_reinitialize_robots keep the rows and the status (environment, not episode). A context that never sets joint
 * dynamics, or has cleared them, launches the simulation kernel it would without this feature. */
int sai2b_set_joint_dynamics(sai2b_ctx* ctx, const sai2b_joint_dynamics_config* cfg, const double* armature, const double* damping,
							 const double* friction, const double* torque_limit, const double* q_lower, const double* q_upper,
							 int on_device);
/* back to the plant without joint dynamics (the rows are kept for a later set, the two buffer ids give NULL) */
int sai2b_clear_joint_dynamics(sai2b_ctx* ctx);
/* the configuration and the [6][dof][B] rows to the host (either may be NULL); without joint dynamics: the default
 * configuration and the neutral rows (0, 0, 0, +inf, -inf, +inf) */
int sai2b_get_joint_dynamics(sai2b_ctx* ctx, sai2b_joint_dynamics_config* cfg, double* rows);
/* what the last sai2b_sim_step left, host arrays [dof][B], any NULL: the applied torque ts, and from the state after the last
 * substep the stop torque sl - su and the dissipative torque -g_i dq_i. *robots_saturated = robots with some |tau_i| > t_i in
 * that call, *robots_at_stop = robots with a non-zero stop torque at the final state (both counted on the device). Zeros
 * before the first step with joint dynamics and after they are cleared. */
int sai2b_get_joint_dynamics_state(sai2b_ctx* ctx, double* applied_torque, double* stop_torque, double* dissipative_torque,
								   int* robots_saturated, int* robots_at_stop);

/* ------------------------------------------------------------------ external wrench on a link of the simulated plant
 * A force and a moment applied to one link of every robot inside sai2b_sim_step, different for every robot and timed per
 * robot: a random shove, a hand guiding the end effector, a tool reaction that turns with the link, a load the controller
 * does not know about. Batch-uniform (sai2b_external_wrench_config): the moving link, the application point c in that link's
 * frame, the frame the rows are given in and the MotionForceTask whose sensed rows the ideal sensor writes (-1: none). Per
 * robot, one device buffer of rows [7][B]: rows 0-2 the force F (N), rows 3-5 the moment M (a pure couple, N m), row 6
 * `steps`, the robot's remaining pushed periods, stored as a double. A robot is ACTIVE in a call of sai2b_sim_step when
 * steps > 0 || steps < 0 on entry (a NaN: inactive); after the call the kernel stores back steps > 0 ? max(steps - 1, 0) :
 * steps, so a negative value means "until changed" and 0 means off. For an active robot, from the state at the START of
 * each substep, with R_l, p_l the link's frame, z_i, p_i the axis and origin of joint i:
 *     x   = p_l + R_l c
 *     F_w = F  or  R_l F          M_w = M  or  R_l M           (SAI2B_WRENCH_WORLD / SAI2B_WRENCH_LINK)
 *     tx_i = z_i . ((x - p_i) x F_w + M_w)     revolute joint i <= link
 *     tx_i = z_i . F_w                          prismatic joint i <= link
 *     tx_i = 0                                  i > link, and every i of an inactive robot (an exact zero)
 * tx enters the substep beside the contact torque tc: the plain step is dq += h M^-1 (((tau + tc) + tx) - b), and with joint
 * dynamics the bracket of that section becomes h (ts + sl - su + tc + tx - b). The torque limit saturates tau only, never
 * tx. This law is this library's definition. sai2b_get_bias, every tick kernel, the trajectory generators and the
 * singularity handling never see the wrench.
 * Sensor: with sensor_task >= 0, after the last substep and from the final state, the kernel writes that task's
 * SAI2B_BUF_SENSED rows with the wrench the robot applies to the environment in that task's sensor frame, as the contact
 * sensor does: o_s = x_c + R_c sensor_pos, R_s = R_c sensor_rot, f_s = R_s^T (-F_w), m_s = R_s^T (-(M_w + (x - o_s) x F_w));
 * zeros for a robot that was inactive in this call, so a reading does not outlive its push. When the contact's sensor is
 * the same task the sum of the two readings is stored once; on different tasks each stores its own rows. The sensor is
 * ideal; whether the point lies outboard of the sensor is the caller's business, as for contact. */
enum sai2b_wrench_frame { SAI2B_WRENCH_WORLD = 0, SAI2B_WRENCH_LINK = 1 };
typedef struct sai2b_external_wrench_config {
	int link;		 /* moving link the wrench acts on (0-based, as sai2b_contact_config.link) */
	int frame;		 /* SAI2B_WRENCH_WORLD: the rows are world components; SAI2B_WRENCH_LINK: components in the link's frame */
	double point[3]; /* application point in the link's frame, metres */
	int sensor_task; /* index of a MotionForceTask, or -1 */
} sai2b_external_wrench_config;
/* host only: point 0, world frame, no sensor */
int sai2b_default_external_wrench(sai2b_external_wrench_config* cfg, int link);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg (link outside [0, robot_dof), an unknown frame, a
 * non-finite point, sensor_task neither -1 nor a MotionForceTask of `tasks`) */
int sai2b_validate_external_wrench(const sai2b_external_wrench_config* cfg, const sai2b_task_config* tasks, int n_tasks,
								   int robot_dof, char* msg, int msg_len);
/* sizeof(sai2b_external_wrench_config) as the library was compiled, for bindings that mirror the struct */
int sai2b_sizeof_external_wrench_config(void);
/* force [3][B], moment [3][B] (NULL: 0), steps [B] doubles (NULL: -1, until changed). Host arrays are validated
 * (SAI2B_INVALID_ARGUMENT: what sai2b_validate_external_wrench rejects, a non-finite force or moment, a NaN in steps);
 * DEVICE arrays (on_device != 0) are copied under the stream contract and NOT inspected. Ordered on the ctx stream; takes
 * effect at the next sai2b_sim_step. sai2b_reinitialize, sai2b_reset_robots and sai2b_reinitialize_robots keep the rows and
 * `steps` of every robot (environment, as the contact rows are): to end a push at a reset, write the selected columns of
 * SAI2B_BUF_EXTERNAL_WRENCH. A call that fails on its arguments leaves the wrench as it was; one that fails while copying
 * (SAI2B_RUNTIME_ERROR) leaves the plant without a wrench. A context that never sets an external wrench, or has cleared it,
 * launches the simulation kernel it would without this feature. */
int sai2b_set_external_wrench(sai2b_ctx* ctx, const sai2b_external_wrench_config* cfg, const double* force, const double* moment,
							  const double* steps, int on_device);
/* back to the plant without an external wrench (the rows are kept for a later set, the two buffer ids give NULL, no sensor
 * writes) */
int sai2b_clear_external_wrench(sai2b_ctx* ctx);
/* the configuration and the [7][B] rows to the host (either may be NULL); link = -1 and zeros without an external wrench */
int sai2b_get_external_wrench(sai2b_ctx* ctx, sai2b_external_wrench_config* cfg, double* rows);
/* what the last sai2b_sim_step left, from the state after its last substep, host arrays, any NULL: wrench_world [6][B] = F_w
 * and M_w about x (zeros for a robot that was inactive), torque [dof][B] = tx, *robots_pushed = robots that were active on
 * entry with some non-zero component of F or M (counted on the device). Zeros before the first step with an external wrench
 * and after a clear. */
int sai2b_get_external_wrench_state(sai2b_ctx* ctx, double* wrench_world, double* torque, int* robots_pushed);

/* ------------------------------------------------------------------ actuator and force-sensor models ("hardware")
 * The signal path between controller and plant, different for every robot: the commanded torque reaches the joints late,
 * through a current loop of finite bandwidth, with a gain error and ripple; the wrist sensor has a bias, noise and an
 * anti-aliasing filter. Both act once per call of sai2b_sim_step (one call is one control period) as stages of their own
 * around the simulation kernel; a context that never sets hardware, or has cleared it, launches what it would without it.
 * Batch-uniform (sai2b_hardware_config): the depth D of the torque history, the MotionForceTask whose sensed rows the sensor
 * model rewrites (-1: none), the random generator's seed and the global index of this context's robot 0. Per robot, doubles,
 * rows [row][B]:
 *   actuator_rows [1 + 3 dof][B]: row 0 the delay d in periods, then dof rows each of the lag coefficient alpha_i, the gain
 *       k_i and the noise standard deviation sigma_i (N m). NULL: ideal (d 0, alpha 1, k 1, sigma 0).
 *   sensor_rows [13][B]: rows 0-5 the bias beta (force 3, moment 3, sensor frame), rows 6-11 the noise standard deviation s
 *       per component, row 12 the filter coefficient alpha_s. NULL: ideal (beta 0, s 0, alpha_s 1).
 * State per robot: a period counter n and an episode index e, the history of commanded torques [(D + 1)][dof], the lag state
 * f [dof], the sensor filter state g [6]. With n, e as they are on entry, c the commanded torque (the tau argument of
 * sai2b_sim_step, or the stored torques when that is NULL):
 *   ACTUATION, ahead of the simulation kernel, for joint i:
 *     hist[n mod (D + 1)][i] = c_i
 *     u_i = hist[max(n - d, 0) mod (D + 1)][i]       the command of d periods ago; the first command until d have passed
 *     f_i = (n == 0 || alpha_i == 1) ? u_i : f_i + alpha_i (u_i - f_i)
 *     a_i = k_i f_i + sigma_i z_i
 *   a is stored in SAI2B_BUF_TAU_APPLIED and is what the simulation kernel receives as its tau: the torque limit of the joint
 *   dynamics saturates a, and their status row "applied torque" reports the saturated a. SAI2B_BUF_TAU and SAI2B_OBS_TAU stay
 *   the command. The delay is read as (int) fmin(fmax(row, 0), D), so a NaN in a device-written row gives 0. With the ideal
 *   rows a is c bit for bit.
 *   SENSOR, behind the simulation kernel, only in a call in which that kernel wrote the ideal reading into sensor_task's
 *   SAI2B_BUF_SENSED rows (the contact's or the external wrench's sensor_task equals this one); otherwise the stage is not
 *   launched and the rows are left alone, so a reading set by hand is never compounded. With r the six rows as left:
 *     y_k = (r_k + beta_k) + s_k z'_k
 *     g_k = (n == 0 || alpha_s == 1) ? y_k : g_k + alpha_s (y_k - g_k)
 *     sensed row k = g_k
 *   The tick's force law, SAI2B_OBS_SENSED and SAI2B_DONE_FORCE therefore see the measured wrench.
 *   After the call n = n + 1; both stages of a call use the same n.
 * Random numbers: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (n, e, 256 stream + call, first_robot + b),
 * stream 0 the actuator, 1 the sensor. The words x0..x3 of call j give four unit normals by Box-Muller on u = (x + 0.5) 2^-32:
 * (x0, x1) -> z_4j = r cos(2 pi u1), z_4j+1 = r sin(2 pi u1) with r = sqrt(-2 ln u0); (x2, x3) -> z_4j+2, z_4j+3 likewise.
 * Joint i takes z_i, sensor component k takes z'_k. |z| <= 6.77. A robot whose deviation is 0 gets a = k f exactly.
 * The noise of a robot depends on the seed, its global index, its episode and its period alone: a batch run as shards with
 * first_robot set to each shard's first global index is bit-equal to the one-context run.
 * sai2b_reset_robots: a selected robot gets n = 0, e += 1; at n = 0 the law re-initialises the history, f and g, and no older
 * entry is read again. The per-robot rows are kept (environment). sai2b_reinitialize and sai2b_reinitialize_robots do not
 * touch the hardware state. Snapshot banks: SAI2B_SNAP_EPISODE holds the history, f, g, the applied torque and the two
 * counters, SAI2B_SNAP_ENVIRONMENT the two row buffers. The seed and first_robot are configuration, not state: they are neither
 * stored in a bank nor part of its fingerprint, so a bank loaded into a context set up with another seed or first_robot
 * continues with that context's noise. n and e are 32-bit ints: a robot that is never reset must not run past 2^31 - 1
 * periods (24 days at 1 kHz); beyond that the history slot and the counter word are undefined. This law is this library's
 * definition. */
#define SAI2B_MAX_ACTUATION_DELAY 8
typedef struct sai2b_hardware_config {
	int max_delay;		  /* D: depth of the torque history in periods, 0..SAI2B_MAX_ACTUATION_DELAY */
	int sensor_task;	  /* MotionForceTask whose sensed rows the sensor model rewrites, or -1 */
	unsigned first_robot; /* global index of robot 0 of this context (0 unless the batch is a shard) */
	int reserved;
	unsigned long long seed;
} sai2b_hardware_config;
/* host only: D 0, no sensor, first_robot 0, seed 0 */
int sai2b_default_hardware(sai2b_hardware_config* cfg);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg (max_delay outside [0, SAI2B_MAX_ACTUATION_DELAY],
 * sensor_task neither -1 nor a MotionForceTask of `tasks`) */
int sai2b_validate_hardware(const sai2b_hardware_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof, char* msg,
							int msg_len);
/* sizeof(sai2b_hardware_config) as the library was compiled, for bindings that mirror the struct */
int sai2b_sizeof_hardware_config(void);
/* Host arrays are validated (SAI2B_INVALID_ARGUMENT with the reason: what sai2b_validate_hardware rejects; d not an integer in
 * [0, D]; alpha, alpha_s outside (0, 1]; k, sigma, s negative or not finite; beta not finite); DEVICE arrays (on_device != 0)
 * are copied under the stream contract and NOT inspected. Zeroes n and e of every robot. Ordered on the ctx stream; takes
 * effect at the next sai2b_sim_step. A call that fails on its arguments leaves the context as it was; one that fails while
 * copying (SAI2B_RUNTIME_ERROR) leaves the context without hardware. */
int sai2b_set_hardware(sai2b_ctx* ctx, const sai2b_hardware_config* cfg, const double* actuator_rows, const double* sensor_rows,
					   int on_device);
/* back to the ideal signal path (the three buffer ids give NULL, no stage is launched) */
int sai2b_clear_hardware(sai2b_ctx* ctx);
/* the configuration and the rows to the host (any may be NULL); the default configuration and the ideal rows without hardware */
int sai2b_get_hardware(sai2b_ctx* ctx, sai2b_hardware_config* cfg, double* actuator_rows, double* sensor_rows);
/* host arrays, any NULL: applied_torque [dof][B] of the last sai2b_sim_step, period [B] = n, episode [B] = e. Zeros without
 * hardware. */
int sai2b_get_hardware_state(sai2b_ctx* ctx, double* applied_torque, int* period, int* episode);

/* ------------------------------------------------------------------ joint sensors
 * The controller's view of the joint state, different for every robot: encoder resolution, calibration offset, position noise,
 * the velocity estimate (a tachometer, or a finite difference of the quantised positions, with noise, behind a first-order
 * filter) and the bus latency of the reading. With a joint sensor set the context has TWO views of the state:
 *   the TRUE view, SAI2B_BUF_Q / SAI2B_BUF_DQ: what sai2b_sim_step integrates (with contact, joint dynamics, wrench and the
 *     wrist sensor's ideal reading), what sai2b_get_bias, sai2b_set_state, sai2b_get_state, sai2b_reset_robots and
 *     sai2b_reset_robots_sampled (its criteria and goals included) and the snapshot banks read and write;
 *   the MEASURED view, SAI2B_BUF_Q_MEASURED / SAI2B_BUF_DQ_MEASURED: what everything on the controller's or the policy's side
 *     reads: sai2b_tick, the split update / compute calls and a deferred sai2b_update_task_models, the trajectory generators,
 *     the sai2b_task_* calls, sai2b_reinitialize and sai2b_reinitialize_robots, the MotionForceTask status getters and run-time
 *     re-parametrisation, sai2b_observe and sai2b_observe_reward (SAI2B_OBS_Q / SAI2B_OBS_DQ, the task blocks and the criteria
 *     JOINT_LIMIT, SPEED, NONFINITE and SUCCESS, as a real system would evaluate them) and sai2b_apply_action (delta_current and
 *     the lead bound included).
 * A context that never sets a joint sensor, or has cleared it, has one view and launches what it launches without the feature.
 * Batch-uniform (sai2b_joint_sensor_config): the depth D of the reading history, the velocity mode, the generator's seed and the
 * global index of this context's robot 0. Per robot, doubles, rows [1 + 5 dof][B]: row 0 the delay d in periods, then dof rows
 * each of the offset o_i (rad or m), the position noise deviation s_i, the quantum Delta_i, the velocity noise deviation r_i
 * and the velocity filter coefficient alpha_i. NULL: ideal (d 0, o 0, s 0, Delta 0, r 0, alpha 1).
 * State per robot: a clock (c, e) = the index of the next reading and the episode, the previous position reading pprev [dof],
 * the filter state v [dof], a history [(D + 1)][2 dof] of (p, v).
 * READING m of the true q, dq, with dt the dt of the sai2b_sim_step call that produced them. An effect whose parameter is zero
 * is skipped, not multiplied by zero, so the ideal rows reproduce the truth bit for bit:
 *     x_i    = q_i (+ o_i if o_i != 0) (+ s_i z_i if s_i != 0)
 *     p_i    = Delta_i > 0 ? Delta_i * rint(x_i / Delta_i) : x_i                  (round half to even)
 *     base_i = (velocity_mode == 1 && m > 0) ? (p_i - pprev_i) / dt : dq_i
 *     w_i    = r_i != 0 ? base_i + r_i z_{dof + i} : base_i
 *     v_i    = (m == 0 || alpha_i == 1) ? w_i : v_i + alpha_i (w_i - v_i)
 *     pprev_i = p_i;  hist[m mod (D + 1)] = (p, v)
 *     (q_measured, dq_measured) = hist[max(m - d, 0) mod (D + 1)]        d = (int) fmin(fmax(row 0, 0), D): a NaN gives 0
 *   Every sum is one product and one sum (no fused multiply-add).
 * Random numbers: the hardware's generator (Philox4x32-10, Box-Muller), stream 10, key (seed & 0xffffffff, seed >> 32), counter
 * (m, e, 256 * 10 + j, first_robot + b); joint i takes z_i and z_{dof + i} of the calls j = 0 .. ceil(2 dof / 4) - 1. The noise
 * of a robot depends on the seed, its global index, its episode and the reading's index alone, so shards with first_robot set
 * are bit-equal to the one-context run.
 * WHEN READINGS ARE TAKEN. Seeding takes reading 0 and leaves c = 1: in sai2b_set_joint_sensor (all robots, e = 0), in
 * sai2b_set_state (all robots, e kept), and in sai2b_reset_robots / sai2b_reset_robots_sampled for the selected robots with
 * e += 1, in a launch behind the reset's own. The sense stage runs last in every sai2b_sim_step (behind the wrist sensor's
 * stage where that runs), takes reading c and leaves c + 1.
 * A CONSEQUENCE: the reset kernels run on the true view, so the tasks of a reset robot are re-initialised at its TRUE start
 * state (its goals sit at the true start pose), and its first tick reads the seeded measurement. sai2b_reinitialize and
 * sai2b_reinitialize_robots read the measured view and do not touch the sensor's state.
 * Snapshot banks: SAI2B_SNAP_EPISODE holds the measured pair, pprev, v, the history and the clock, SAI2B_SNAP_ENVIRONMENT the
 * rows; seed and first_robot are configuration, as for the hardware. c and e are 32-bit ints with the hardware's limit. This
 * law is this library's definition. */
typedef struct sai2b_joint_sensor_config {
	int max_delay;		  /* D: depth of the reading history in periods, 0..SAI2B_MAX_ACTUATION_DELAY */
	int velocity_mode;	  /* 0: tachometer (the true dq), 1: finite difference of the position readings */
	unsigned first_robot; /* global index of robot 0 of this context (0 unless the batch is a shard) */
	int reserved;
	unsigned long long seed;
} sai2b_joint_sensor_config;
/* host only: D 0, tachometer, first_robot 0, seed 0 */
int sai2b_default_joint_sensor(sai2b_joint_sensor_config* cfg);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg (max_delay outside [0, SAI2B_MAX_ACTUATION_DELAY],
 * velocity_mode not 0 or 1) */
int sai2b_validate_joint_sensor(const sai2b_joint_sensor_config* cfg, int robot_dof, char* msg, int msg_len);
/* sizeof(sai2b_joint_sensor_config) as the library was compiled, for bindings that mirror the struct */
int sai2b_sizeof_joint_sensor_config(void);
/* Host rows are validated (SAI2B_INVALID_ARGUMENT with the reason: what sai2b_validate_joint_sensor rejects; d not an integer
 * in [0, D]; alpha outside (0, 1]; s, Delta, r negative or not finite; o not finite); DEVICE rows (on_device != 0) are copied
 * under the stream contract and NOT inspected. Zeroes the clocks and seeds every robot's measurement from the state as it is.
 * Ordered on the ctx stream. A call that fails on its arguments leaves the context as it was; one that fails while copying
 * (SAI2B_RUNTIME_ERROR) leaves the context without a joint sensor. */
int sai2b_set_joint_sensor(sai2b_ctx* ctx, const sai2b_joint_sensor_config* cfg, const double* rows, int on_device);
/* back to one view (the three buffer ids give NULL, no stage is launched); the state buffers keep the truth */
int sai2b_clear_joint_sensor(sai2b_ctx* ctx);
/* the configuration and the rows to the host (either may be NULL); the default configuration and the ideal rows without one */
int sai2b_get_joint_sensor(sai2b_ctx* ctx, sai2b_joint_sensor_config* cfg, double* rows);
/* host arrays, either NULL: clock [B] = c, episode [B] = e. Zeros without a joint sensor. */
int sai2b_get_joint_sensor_state(sai2b_ctx* ctx, int* clock, int* episode);
/* host arrays [dof][B], either NULL: the measured pair; the truth without a joint sensor */
int sai2b_get_measured_state(sai2b_ctx* ctx, double* q, double* dq);

/* ------------------------------------------------------------------ observations and episode-end flags
 * The missing link of the resident loop  tick, sai2b_sim_step(NULL), sai2b_observe(out, done), sai2b_reset_robots(done, ..):
 * ONE launch writes a caller-chosen set of observation rows [rows][B] and one done byte per robot into device (or host)
 * memory; the byte is a valid mask for sai2b_reset_robots. Everything in the configuration is batch-uniform. A context that
 * never configures an observation launches exactly the kernels it launches without this feature.
 *
 * Row layout: the global blocks that are selected, in the order of their flags below, then for every task of task_mask (in
 * ascending task index) the selected per-task blocks in the order of their flags. The task quantities are those of
 * sai2b_get_mft_status / sai2b_get_mft_velocity: computed from the state and goal buffers as they are now. */
enum sai2b_observation_block {
	SAI2B_OBS_Q = 1,			 /* dof rows: joint positions */
	SAI2B_OBS_DQ = 2,			 /* dof rows: joint velocities */
	SAI2B_OBS_TAU = 4,			 /* dof rows: the stored torques of SAI2B_BUF_TAU */
	SAI2B_OBS_LIMIT_MARGIN = 8,	 /* 1 row: min_i min(q_i - q_lower_i, q_upper_i - q_i), limits of the context's model */
	SAI2B_OBS_EPISODE_STEP = 16, /* 1 row: the robot's episode counter (below), as a double */
	SAI2B_OBS_CONTACT = 32		 /* 14 rows: what the last sai2b_sim_step left (sai2b_get_contact_state): depth 4, normal
								  * force 4, world wrench 6; zeros when the context has no contact */
};
enum sai2b_observation_task_block {
	SAI2B_OBS_POSE = 1,	 /* 12 rows: position 3, rotation 9 row-major */
	SAI2B_OBS_TWIST = 2, /* 6 rows: J dq, linear then angular */
	SAI2B_OBS_ERROR = 4, /* 8 rows: sigma_p (x_goal - x) 3, sigma_o orientationError 3, the two norms sqrt(e^T sigma e) */
	SAI2B_OBS_SENSED = 8 /* 6 rows: sensed force and moment at the control point, world frame */
};
/* Bits of a robot's done byte; each criterion is evaluated only when its bit is set in sai2b_observation_config.criteria.
 * Every comparison is written so that a NaN operand gives false, and the criteria that read the state (SUCCESS,
 * JOINT_LIMIT, SPEED, FORCE) are not evaluated for a robot whose q or dq is not finite: such a robot reports NONFINITE
 * (when enabled) and no accidental other state bit. */
enum sai2b_done_reason {
	SAI2B_DONE_SUCCESS = 1,		/* every task of success_task_mask: position-error norm < pos_tolerance and orientation-error
								 * norm < ori_tolerance, strict, as goalPositionReached / goalOrientationReached
								 * (MotionForceTask.cpp:548-579) */
	SAI2B_DONE_JOINT_LIMIT = 2, /* limit margin < joint_limit_margin */
	SAI2B_DONE_SPEED = 4,		/* some |dq_i| > max_joint_speed[i] */
	SAI2B_DONE_NONFINITE = 8,	/* some q_i or dq_i is not finite */
	SAI2B_DONE_FORCE = 16,		/* some task of force_task_mask: norm of the sensed world force > max_sensed_force */
	SAI2B_DONE_TIMEOUT = 32		/* episode counter >= max_episode_steps */
};
#define SAI2B_DONE_REASONS 6
typedef struct sai2b_observation_config {
	int blocks;		 /* SAI2B_OBS_Q | ... : the global blocks */
	int task_mask;	 /* bit t: MotionForceTask t is observed */
	int task_blocks; /* SAI2B_OBS_POSE | ... : the blocks stored for every observed task */
	int criteria;	 /* SAI2B_DONE_* bits that are evaluated; 0: the done byte is always 0 */
	int success_task_mask, force_task_mask;
	int max_episode_steps;
	int reserved;
	double pos_tolerance, ori_tolerance;
	double joint_limit_margin;
	double max_joint_speed[SAI2B_MAX_DOF]; /* entries >= dof are ignored */
	double max_sensed_force;
} sai2b_observation_config;
/* host only: nothing observed, every criterion off, thresholds 0 */
int sai2b_default_observation(sai2b_observation_config* cfg);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg: unknown bits in blocks / task_blocks / criteria, a
 * task in one of the three masks that is not a MotionForceTask of `tasks`, a negative or non-finite threshold,
 * max_episode_steps < 0 (< 1 with TIMEOUT enabled), SUCCESS or FORCE enabled with an empty task mask */
int sai2b_validate_observation(const sai2b_observation_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof,
							   char* msg, int msg_len);
/* sizeof(sai2b_observation_config) as the library was compiled: a binding that mirrors the struct checks its layout with it */
int sai2b_sizeof_observation_config(void);
/* host only, the layout arithmetic: where `block` is stored. task = -1: a global block (enum sai2b_observation_block), else
 * a per-task block (enum sai2b_observation_task_block) of that task. *n_rows = 0 and *first_row = -1 when the configuration
 * does not select it; *total_rows: rows of the whole observation. Any output may be NULL. SAI2B_INVALID_ARGUMENT when
 * `block` is not exactly one known flag or task is outside [-1, SAI2B_MAX_TASKS). */
int sai2b_observation_config_layout(const sai2b_observation_config* cfg, int robot_dof, int block, int task, int* first_row,
									int* n_rows, int* total_rows);
/* validates against the context's tasks, allocates, and zeroes every robot's episode counter (also when called again) */
int sai2b_set_observation(sai2b_ctx* ctx, const sai2b_observation_config* cfg);
/* back to a context without an observation: sai2b_observe fails from here on */
int sai2b_clear_observation(sai2b_ctx* ctx);
/* rows of the configured observation; -1 without one */
int sai2b_observation_rows(sai2b_ctx* ctx);
/* sai2b_observation_config_layout for the context's configuration; SAI2B_INVALID_ARGUMENT without one */
int sai2b_observation_layout(sai2b_ctx* ctx, int block, int task, int* first_row, int* n_rows);
/* One launch: out [rows][B] and done [B] bytes (either may be NULL), host memory, or device memory when on_device != 0
 * (stream contract below: complete when the call returns as far as the caller's stream is concerned, nothing synchronises).
 * A deferred sai2b_update_task_models is flushed first. SAI2B_INVALID_ARGUMENT without a configured observation (nothing
 * is launched then).
 * Episode counter: one int per robot. Every call increments it BEFORE the criteria are evaluated and reports that value in
 * SAI2B_OBS_EPISODE_STEP; it is stored back as 0 for a robot whose done byte came out non-zero, otherwise as incremented:
 * it counts the observes since the robot was last reported done. */
int sai2b_observe(sai2b_ctx* ctx, double* out, unsigned char* done, int on_device);
/* of the last sai2b_observe, counted on the device: robots per reason bit 0-5 and, last, robots with a non-zero byte.
 * Zeros before the first observe; SAI2B_INVALID_ARGUMENT without a configured observation. Waits for the ctx stream. */
int sai2b_get_done_counts(sai2b_ctx* ctx, int counts[7]);

/* ------------------------------------------------------------------ actions
 * The link between a policy and the controller in the resident loop  tick, sai2b_sim_step(NULL), sai2b_observe, policy,
 * sai2b_apply_action, sai2b_reset_robots: ONE launch maps an action [rows][B] in device (or host) memory to the goal rows of
 * the chosen tasks. Everything in the configuration is batch-uniform. A context that never configures an action launches
 * exactly the kernels it launches without this feature.
 *
 * Row layout: tasks in ascending index; within a MotionForceTask the selected blocks in the order of their flags below, 3
 * rows each; a JointTask takes task_dof rows.
 *
 * Per robot, with a = the task's slice of the action (every component limited to [-1, 1] first when clip_actions):
 *   position     p = base + pos_scale o a; each component clamped into [pos_lower, pos_upper]; then, with x the robot's
 *                current position and e = p - x, if |e| > max_pos_lead: p = x + e max_pos_lead / |e| (box first, then lead:
 *                the lead may take p out of the box again by at most the distance from x to the box). p -> goal position rows.
 *   orientation  w = ori_scale a, R_new = exp([w]x) R_base: the delta is a rotation vector in the WORLD frame.
 *                exp = I + A [w]x + B [w]x^2, th2 = w.w, A = sin th / th, B = 2 sin^2(th / 2) / th2; for th2 < 1e-8 the series
 *                A = 1 - th2 / 6, B = 1/2 - th2 / 24 (truncation below 1e-18). Evaluated as R_base + (A [w]x + B [w]x^2) R_base:
 *                a zero action leaves the nine rows equal (==) to the base. NO re-orthonormalisation: in DELTA_GOAL mode
 *                the goal rotation collects the rounding of one 3 x 3 product per apply; the drift from orthonormal is
 *                measured in DESIGN.md §8h.
 *   force/moment goal force / moment rows = force_scale a / moment_scale a, in every mode.
 *   JointTask    g = base + jt_scale o a, clamped into [jt_lower, jt_upper] -> goal position rows.
 * base: DELTA_GOAL the goal rows as they are, DELTA_CURRENT the robot as it is now, ABSOLUTE 0 (orientation: the identity).
 * Goal velocity and acceleration rows are never touched (MotionForceTask::setGoalPosition does not touch them either).
 *
 * A robot with an action component that is not finite gets NONE of its goal rows written (they stay bit-equal) and is
 * counted as rejected; so is a robot whose q is not finite when the configuration reads the state (a DELTA_CURRENT task, or
 * a finite max_pos_lead). Every comparison is written so that a NaN operand gives "reject" or "false". */
enum sai2b_action_mode {		 /* per task */
	SAI2B_ACT_NONE = 0,			 /* the task takes no rows */
	SAI2B_ACT_DELTA_GOAL = 1,	 /* base = the task's goal rows as they are (accumulating) */
	SAI2B_ACT_DELTA_CURRENT = 2, /* base = the robot as it is now: MotionForceTask pose by forward kinematics of SAI2B_BUF_Q (as
								  * sai2b_observe computes it, not the cached pose), JointTask S q */
	SAI2B_ACT_ABSOLUTE = 3
};
enum sai2b_action_block { /* MotionForceTask only, 3 rows each; a JointTask always takes task_dof rows */
	SAI2B_ACT_POSITION = 1,
	SAI2B_ACT_ORIENTATION = 2,
	SAI2B_ACT_FORCE = 4,
	SAI2B_ACT_MOMENT = 8
};
typedef struct sai2b_action_task {
	int mode, blocks;
	double pos_scale[3], ori_scale, force_scale, moment_scale; /* metres, rad, N, Nm per unit action */
	double pos_lower[3], pos_upper[3];						   /* world box for the goal position; -inf / +inf: none */
	double max_pos_lead;									   /* bound on |goal - current position|; +inf: none */
	double jt_scale[SAI2B_MAX_DOF], jt_lower[SAI2B_MAX_DOF], jt_upper[SAI2B_MAX_DOF]; /* per task row; entries >= task_dof are ignored */
} sai2b_action_task;
typedef struct sai2b_action_config {
	int clip_actions; /* nonzero: every component is limited to [-1, 1] before scaling */
	int reserved;
	sai2b_action_task task[SAI2B_MAX_TASKS];
} sai2b_action_config;
/* host only: every task NONE with no block, scales 1, limits -inf / +inf, lead +inf, no clipping */
int sai2b_default_action(sai2b_action_config* cfg);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg: an unknown mode or unknown block bits, blocks on a
 * JointTask, a MotionForceTask with a mode and no block, a mode on a task index >= n_tasks, a scale that is negative or not
 * finite, lower >= upper or a NaN limit, a lead that is not > 0, no task with a mode at all */
int sai2b_validate_action(const sai2b_action_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof, char* msg,
						  int msg_len);
/* sizeof(sai2b_action_config) as the library was compiled: a binding that mirrors the struct checks its layout with it */
int sai2b_sizeof_action_config(void);
/* host only, the layout arithmetic: where `block` (one flag of enum sai2b_action_block; ignored for a JointTask) of `task` is
 * read from. *n_rows = 0 and *first_row = -1 when the configuration does not select it; *total_rows: rows of the whole
 * action. Any output may be NULL. SAI2B_INVALID_ARGUMENT when task is outside [0, n_tasks) or, for a MotionForceTask, block
 * is not exactly one known flag. */
int sai2b_action_config_layout(const sai2b_action_config* cfg, const sai2b_task_config* tasks, int n_tasks, int block, int task,
							   int* first_row, int* n_rows, int* total_rows);
/* validates against the context's tasks and allocates the device counters */
int sai2b_set_action(sai2b_ctx* ctx, const sai2b_action_config* cfg);
/* back to a context without an action: sai2b_apply_action fails from here on */
int sai2b_clear_action(sai2b_ctx* ctx);
/* rows of the configured action; -1 without one */
int sai2b_action_rows(sai2b_ctx* ctx);
/* sai2b_action_config_layout for the context's configuration; SAI2B_INVALID_ARGUMENT without one */
int sai2b_action_layout(sai2b_ctx* ctx, int block, int task, int* first_row, int* n_rows);
/* One launch, whatever is configured: action [rows][B]; mask [B] bytes or NULL = every robot, a robot with mask[b] == 0 is not
 * touched and not counted. All pointers host, or all device when on_device != 0 (stream contract below: the inputs are read
 * before anything the caller enqueues on its stream after the call, nothing synchronises). A deferred
 * sai2b_update_task_models is flushed first. The tasks with a mode are marked as the goal setters mark them, so the internal
 * trajectory generators see the new goals at the next tick. SAI2B_INVALID_ARGUMENT without a configured action (nothing is
 * launched then). */
int sai2b_apply_action(sai2b_ctx* ctx, const double* action, const unsigned char* mask, int on_device);
/* of the last sai2b_apply_action, counted on the device: robots rejected, robots with some component clipped to +-1, robots
 * whose goal was limited by a box, the lead or a joint clamp (a rejected robot counts as rejected only). Zeros before the
 * first apply; SAI2B_INVALID_ARGUMENT without a configured action. Waits for the ctx stream. */
int sai2b_get_action_counts(sai2b_ctx* ctx, int counts[3]);

/* ------------------------------------------------------------------ rewards and episode returns
 * The reward (for sampling MPC: the stage cost) of the resident loop  tick, sai2b_sim_step(NULL), sai2b_observe_reward, policy,
 * sai2b_apply_action, sai2b_reset_robots: sai2b_observe_reward is sai2b_observe plus, in the SAME launch, one reward per robot
 * and the per-robot episode bookkeeping that goes with it (discounted return, return and length of the episode that just
 * ended). Everything in the configuration is batch-uniform. A context that never configures a reward launches exactly the
 * kernels it launches without this feature.
 *
 * Term rows [reward_rows][B]: the selected global terms in the order of their flags, then for every task of task_mask (in
 * ascending task index) the selected task terms in the order of their flags; one row each, unweighted (DONE: its done_value
 * sum). */
enum sai2b_reward_term {
	SAI2B_REW_ALIVE = 1,	   /* 1 */
	SAI2B_REW_JOINT_SPEED = 2, /* sum_i dq_i^2 */
	SAI2B_REW_TORQUE = 4,	   /* sum_i tau_i^2, tau = SAI2B_BUF_TAU as SAI2B_OBS_TAU reads it */
	SAI2B_REW_TORQUE_RATE = 8, /* sum_i (tau_i - tau_prev_i)^2; 0 while the robot has no valid tau_prev (below) */
	SAI2B_REW_LIMIT = 16,	   /* max(0, limit_soft_margin - margin), margin = the SAI2B_OBS_LIMIT_MARGIN observation */
	SAI2B_REW_DONE = 32		   /* sum_r done_value[r] * bit r of this call's done byte */
};
enum sai2b_reward_task_term {
	SAI2B_REW_POS = 1,		 /* d_p: row 6 of the SAI2B_OBS_ERROR block, sqrt(max(e^T sigma_p e, 0)) */
	SAI2B_REW_POS_SQ = 2,	 /* d_p * d_p */
	SAI2B_REW_POS_TANH = 4,	 /* 1 - tanh(d_p / pos_scale[t]) */
	SAI2B_REW_ORI = 8,		 /* d_o: row 7 of the SAI2B_OBS_ERROR block */
	SAI2B_REW_ORI_SQ = 16,	 /* d_o * d_o */
	SAI2B_REW_ORI_TANH = 32, /* 1 - tanh(d_o / ori_scale[t]) */
	SAI2B_REW_LIN_VEL_SQ = 64,	/* |v|^2, (v, w) = J dq, the SAI2B_OBS_TWIST block */
	SAI2B_REW_ANG_VEL_SQ = 128, /* |w|^2 */
	SAI2B_REW_FORCE_ERR_SQ = 256, /* |sigma_f (f_sensed_world - f_goal)|^2: the difference the force law's kp_force multiplies
								   * (MotionForceTask.cpp:330-336), f_goal = goal rows 24..26 */
	SAI2B_REW_FORCE_EXCESS = 512  /* max(0, |f_sensed_world| - force_soft_limit[t]) */
};
#define SAI2B_REWARD_TERMS 6
#define SAI2B_REWARD_TASK_TERMS 10
typedef struct sai2b_reward_config {
	int terms;		/* SAI2B_REW_ALIVE | ... : the global terms */
	int task_mask;	/* bit t: MotionForceTask t takes part */
	int task_terms; /* SAI2B_REW_POS | ... : the terms evaluated for every task of task_mask */
	int reserved;
	double weight[SAI2B_REWARD_TERMS];							  /* by flag bit */
	double task_weight[SAI2B_MAX_TASKS][SAI2B_REWARD_TASK_TERMS]; /* by task, by flag bit */
	double done_value[SAI2B_DONE_REASONS];						  /* by reason bit */
	double limit_soft_margin;
	double pos_scale[SAI2B_MAX_TASKS], ori_scale[SAI2B_MAX_TASKS], force_soft_limit[SAI2B_MAX_TASKS];
	double gamma;			 /* discount of the running return, in [0, 1] */
	double nonfinite_reward; /* finite; what a robot gets whose reward came out not finite */
} sai2b_reward_config;
/* host only: no term, weights and values 0, scales 1, soft margin and soft limits 0, gamma 1, nonfinite_reward 0 */
int sai2b_default_reward(sai2b_reward_config* cfg);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg: unknown bits in terms / task_terms, a task of task_mask
 * that is not a MotionForceTask of `tasks`, task terms without a task or a task without task terms, a weight, done value or
 * scale that is not finite, pos_scale / ori_scale not > 0 for a task whose TANH term is selected, a negative or non-finite
 * limit_soft_margin or force_soft_limit, gamma outside [0, 1], a nonfinite_reward that is not finite, no term at all */
int sai2b_validate_reward(const sai2b_reward_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof, char* msg,
						  int msg_len);
/* sizeof(sai2b_reward_config) as the library was compiled: a binding that mirrors the struct checks its layout with it */
int sai2b_sizeof_reward_config(void);
/* host only, the layout arithmetic: the row of `term`. task = -1: a global term (enum sai2b_reward_term), else a term of that
 * task (enum sai2b_reward_task_term). *n_rows = 0 and *first_row = -1 when the configuration does not select it; *total_rows:
 * rows of all terms. Any output may be NULL. SAI2B_INVALID_ARGUMENT when `term` is not exactly one known flag or task is
 * outside [-1, SAI2B_MAX_TASKS). */
int sai2b_reward_config_layout(const sai2b_reward_config* cfg, int term, int task, int* first_row, int* n_rows, int* total_rows);
/* validates against the context's tasks; needs a configured observation (the done criteria live there); allocates the
 * accumulators and sets every robot's to their start values (return 0, discount 1, last return 0, last length 0, no tau_prev),
 * also when called again */
int sai2b_set_reward(sai2b_ctx* ctx, const sai2b_reward_config* cfg);
/* back to a context without a reward: sai2b_observe_reward fails from here on, sai2b_reset_robots makes no extra launch */
int sai2b_clear_reward(sai2b_ctx* ctx);
/* rows of the configured reward's terms; -1 without one */
int sai2b_reward_rows(sai2b_ctx* ctx);
/* sai2b_reward_config_layout for the context's configuration; SAI2B_INVALID_ARGUMENT without one */
int sai2b_reward_layout(sai2b_ctx* ctx, int term, int task, int* first_row, int* n_rows);
/* One launch. Per robot:
 *  1. everything sai2b_observe does, unchanged: out and done (either may be NULL; the byte is computed either way), the episode
 *     counter, the done counts, the NaN and non-finite-state rules;
 *  2. the selected terms, and r = sum weight * term in layout order starting from 0.0, every step a separate multiply and a
 *     separate add (no fused multiply-add here or in 4.);
 *  3. r not finite: r = nonfinite_reward and the robot is counted; the term rows keep what was computed;
 *  4. ret = ret + disc * r, then disc = disc * gamma;
 *  5. done byte non-zero: last_return = ret, last_length = the episode step this call reported, then ret = 0, disc = 1, tau_prev
 *     invalid; otherwise tau_prev = tau, valid;
 *  6. reward [B] and terms [reward_rows][B] are written where given (either may be NULL).
 * All pointers host, or all device when on_device != 0; the stream contract and the staging of host outputs are those of
 * sai2b_observe. SAI2B_INVALID_ARGUMENT without a configured observation or without a configured reward (nothing is launched
 * then). A plain sai2b_observe on a context with a reward stays what it is and does not touch the reward's state: a done it
 * reports does NOT close the reward's episode (the episode counter restarts, the return goes on). sai2b_reset_robots sets the
 * selected robots' ret = 0, disc = 1, tau_prev invalid in one more small launch and keeps last_return and last_length;
 * sai2b_reinitialize_robots does not touch the reward's state. The accumulators are part of SAI2B_SNAP_EPISODE.
 * There is no batch sum of returns on the device: a float atomic sum depends on arrival order. */
int sai2b_observe_reward(sai2b_ctx* ctx, double* out, unsigned char* done, double* reward, double* terms, int on_device);
/* of the last sai2b_observe_reward, counted on the device: robots whose episode was closed, robots whose reward was replaced by
 * nonfinite_reward. Zeros before the first; SAI2B_INVALID_ARGUMENT without a configured reward. Waits for the ctx stream. */
int sai2b_get_reward_counts(sai2b_ctx* ctx, int counts[2]);
/* the accumulators as they are now, host arrays [B] each, any may be NULL: running return, running discount, return and length
 * of the episode that ended last. Waits for the ctx stream. */
int sai2b_get_episode_stats(sai2b_ctx* ctx, double* ret, double* discount, double* last_return, int* last_length);

/* ------------------------------------------------------------------ collision proximity
 * A proximity sensor for the whole arm: clearance to the environment and to the arm itself, the direction of that clearance and
 * its joint-space gradient, per robot, in ONE launch (sai2b_collision_query). A context that never configures it launches
 * exactly the kernels it launches without this feature; a configured context launches the kernel only in sai2b_collision_query.
 * GEOMETRY, batch-uniform (sai2b_collision_config): n_spheres in 1..SAI2B_MAX_COLLISION_SPHERES. Sphere k sits on link_k in
 * [-1, dof) (-1: the world, i.e. the base after sai2b_model_set_base_transform, which folds the base into joint 0; so a centre on
 * link -1 is a world point) with centre c_k in that link's frame and radius r_k >= 0. World centre x_k = p_link + R_link c_k in
 * the chain convention of include/sai2b_detfk.h, plain FP64 (not the bit-reproducible pose of that header).
 * MASKS: env_mask bit k: sphere k is tested against planes and obstacles. pair_mask[i] bit j, i < j: the pair (i, j) is tested.
 * sai2b_default_collision sets every bit of env_mask whose sphere is on a moving link (link >= 0) and every pair whose links
 * differ by at least 2 (with -1 counting as a link).
 * PER ROBOT, doubles, rows [6 P + 4 O][B] with P = n_planes in 0..2 and O = n_obstacles in 0..4: per plane a point p0 (3) and
 * the outward unit normal n (3), as sai2b_set_contact takes them; then per obstacle its world centre c_o (3) and radius r_o (1).
 * A NaN anywhere in a plane's or an obstacle's rows makes it lose every comparison: it is absent for that robot. Every
 * comparison is written so that a NaN operand gives false, as in the observation.
 * THREE CATEGORIES, each a minimum with its witness:
 *     plane     d = n . (x_k - p0) - r_k            p outer, k inner       index 16 p + k
 *     obstacle  d = |x_k - c_o| - r_k - r_o         o outer, k inner       index 16 o + k
 *     self      d = |x_i - x_j| - r_i - r_j         i outer, j inner       index 16 i + j
 *   The first strict minimum (d < best, best starting at +inf) wins. An empty category reports +inf, index -1, the zero normal
 *   and the zero gradient. The index is an exact integer stored as a double. Witness normal u: n of the winning plane;
 *   (x_k - c_o) / |x_k - c_o|; (x_i - x_j) / |x_i - x_j|; the zero vector when that norm is 0. Gradient of the minimum with
 *   respect to q, dof entries: g_m = u . dx/dq_m, for self u . (dx_i/dq_m - dx_j/dq_m), with dx/dq_m = z_m x (x - o_m) about a
 *   revolute joint and z_m along a prismatic one for m <= link(x), and 0 beyond; z_m is the world z of joint m's frame, o_m
 *   its world origin.
 * FLAGS, one byte per robot: bit 0 plane d_min < margin_plane, bit 1 obstacle d_min < margin_obstacle, bit 2 self d_min <
 * margin_self, bit 3 some q_i is not finite; such a robot gets bit 3 alone (its rows are what the law gives on that q: whatever
 * a NaN reaches loses its comparisons). COUNTS on the device: robots per bit, then robots with a non-zero byte.
 * OUTPUT rows [rows][B], the selected blocks in the order of their flags; the first four hold the categories in the order
 * plane, obstacle, self. `view`: 0 reads SAI2B_BUF_Q, the truth (a collision is a fact of the plant); 1 reads
 * SAI2B_BUF_Q_MEASURED while a joint sensor is set, and the truth otherwise.
 * Snapshot banks do not hold the rows or the configuration: the rows stay with the robot index, and a fresh context is
 * configured again, like the observation's. This law is this library's definition. */
#define SAI2B_MAX_COLLISION_SPHERES 16
#define SAI2B_MAX_COLLISION_PLANES 2
#define SAI2B_MAX_COLLISION_OBSTACLES 4
enum sai2b_collision_block {
	SAI2B_COL_DISTANCE = 1, /* 3 rows: d_min of plane, obstacle, self */
	SAI2B_COL_INDEX = 2,	/* 3 rows: the witness index */
	SAI2B_COL_NORMAL = 4,	/* 9 rows: the witness normal, 3 per category */
	SAI2B_COL_GRADIENT = 8, /* 3 dof rows: the gradient, dof per category */
	SAI2B_COL_CENTRES = 16	/* 3 n_spheres rows: the world centres, sphere k at rows 3 k .. 3 k + 2 */
};
enum sai2b_collision_category { SAI2B_COL_PLANE = 0, SAI2B_COL_OBSTACLE = 1, SAI2B_COL_SELF = 2 };
enum sai2b_collision_flag { SAI2B_COL_FLAG_PLANE = 1, SAI2B_COL_FLAG_OBSTACLE = 2, SAI2B_COL_FLAG_SELF = 4, SAI2B_COL_FLAG_NONFINITE = 8 };
/* the conventional bit of a done byte for "ended by a collision" (sai2b_end_episodes); not one of enum sai2b_done_reason */
#define SAI2B_DONE_COLLISION 64
typedef struct sai2b_collision_config {
	int n_spheres, n_planes, n_obstacles;
	int blocks; /* SAI2B_COL_DISTANCE | ... : what sai2b_collision_query stores */
	int view;	/* 0: the plant's q; 1: the measured q while a joint sensor is set */
	unsigned env_mask;
	unsigned pair_mask[SAI2B_MAX_COLLISION_SPHERES];
	int link[SAI2B_MAX_COLLISION_SPHERES];
	double centre[SAI2B_MAX_COLLISION_SPHERES][3];
	double radius[SAI2B_MAX_COLLISION_SPHERES];
	double margin_plane, margin_obstacle, margin_self;
	int reserved[8];
} sai2b_collision_config;
/* host only: n_spheres spheres (link [n], centre [n][3], radius [n]), the default masks, no plane, no obstacle,
 * blocks = SAI2B_COL_DISTANCE, margins 0, view 0. SAI2B_INVALID_ARGUMENT for n_spheres outside 1..16 or a NULL array. */
int sai2b_default_collision(sai2b_collision_config* cfg, int n_spheres, const int* link, const double* centre, const double* radius);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg: a count out of range, a link outside [-1, dof), a
 * centre that is not finite, a radius that is negative or not finite, mask bits beyond n_spheres, a pair bit with j <= i,
 * unknown block bits, a margin that is not finite, view not 0 or 1 */
int sai2b_validate_collision(const sai2b_collision_config* cfg, int robot_dof, char* msg, int msg_len);
/* sizeof(sai2b_collision_config) as the library was compiled, for bindings that mirror the struct */
int sai2b_sizeof_collision_config(void);
/* host only, the layout arithmetic: where `block` (exactly one flag of enum sai2b_collision_block) is stored. category = -1: the
 * whole block; 0..2: that category's rows of one of the first four blocks. *n_rows = 0 and *first_row = -1 when the
 * configuration does not select the block; *total_rows: rows of the whole output; *env_rows: 6 P + 4 O. Any output may be NULL.
 * SAI2B_INVALID_ARGUMENT when block is not exactly one known flag, or category is outside [-1, 2] or names a part of the centres. */
int sai2b_collision_config_layout(const sai2b_collision_config* cfg, int robot_dof, int block, int category, int* first_row, int* n_rows,
								  int* total_rows, int* env_rows);
/* rows [6 P + 4 O][B], host or device (stream contract), NULL: every plane and obstacle absent (NaN) until a producer writes
 * SAI2B_BUF_COLLISION. Host rows are validated (SAI2B_INVALID_ARGUMENT with the reason): a plane without a NaN needs a
 * normal within 1e-9 of unit length, an obstacle without a NaN a radius >= 0; a NaN is allowed as "absent". DEVICE rows are
 * copied as they are. A failing call leaves the context as it was. */
int sai2b_set_collision(sai2b_ctx* ctx, const sai2b_collision_config* cfg, const double* rows, int on_device);
/* back to a context without the feature: sai2b_collision_query fails from here on, SAI2B_BUF_COLLISION gives NULL */
int sai2b_clear_collision(sai2b_ctx* ctx);
/* the configuration and the rows to the host (either may be NULL); SAI2B_INVALID_ARGUMENT without a configuration */
int sai2b_get_collision(sai2b_ctx* ctx, sai2b_collision_config* cfg, double* rows);
/* rows of the configured output; -1 without a configuration */
int sai2b_collision_rows(sai2b_ctx* ctx);
/* sai2b_collision_config_layout for the context's configuration; SAI2B_INVALID_ARGUMENT without one */
int sai2b_collision_layout(sai2b_ctx* ctx, int block, int category, int* first_row, int* n_rows);
/* One launch: out [rows][B] doubles and flags [B] bytes (either may be NULL), host memory, or device memory when on_device != 0
 * (stream contract, staging of host outputs as sai2b_observe). A deferred sai2b_update_task_models is not touched: the query
 * reads q alone. SAI2B_INVALID_ARGUMENT and no launch without a configuration. */
int sai2b_collision_query(sai2b_ctx* ctx, double* out, unsigned char* flags, int on_device);
/* of the last sai2b_collision_query, counted on the device: robots per flag bit 0-3 and, last, robots with a non-zero byte. Zeros
 * before the first; SAI2B_INVALID_ARGUMENT without a configuration. Waits for the ctx stream. */
int sai2b_get_collision_counts(sai2b_ctx* ctx, int counts[5]);
/* Ending an episode from outside, for a reason the six built-in criteria do not know (a collision, a criterion computed by the
 * caller). done_inout and extra: [B] bytes each, host, or device when on_device != 0 (stream contract). bit: 64 or 128, the two
 * bits above the built-in reasons; anything else is SAI2B_INVALID_ARGUMENT, as is a NULL array. One launch. For every robot
 * with extra[b] != 0: if done_inout[b] == 0 its episode is closed exactly as step 5 of sai2b_observe_reward closes one (with a
 * reward configured: last_return = ret, last_length = the observation's episode counter as it stands, ret = 0, disc = 1,
 * tau_prev invalid; with an observation configured: its episode counter becomes 0) and the robot is counted; then
 * done_inout[b] |= bit. A robot that was already done keeps its bookkeeping and only gains the bit; a robot with
 * extra[b] == 0 is neither read nor written. Without a reward and without an observation only the bytes and the count are
 * written. The flags of sai2b_collision_query, or any byte array of the caller's, serve as `extra`. */
int sai2b_end_episodes(sai2b_ctx* ctx, unsigned char* done_inout, const unsigned char* extra, int bit, int on_device);
/* robots whose episode the last sai2b_end_episodes closed, counted on the device; 0 before the first. Waits for the ctx stream. */
int sai2b_get_end_episode_count(sai2b_ctx* ctx, int* count);

/* ------------------------------------------------------------------ whole-arm contact
 * The collision configuration's geometry as a physical body of the simulated plant: inside every substep of sai2b_sim_step the
 * link spheres are pushed out of the robot's planes, its obstacle spheres and each other, so that an arm can brush an obstacle,
 * lean an elbow on a table or be stopped by a wall. A context that never sets it launches exactly the kernels it launches
 * without this feature; one that has it set launches sim_body_kernel instead of the other simulation kernels.
 * GEOMETRY: the collision configuration's own (sai2b_set_collision, which must be in force: SAI2B_INVALID_ARGUMENT without
 * one): spheres (link, centre, radius), env_mask, pair_mask, and the per-robot environment rows [6 P + 4 O][B] of
 * SAI2B_BUF_COLLISION, READ LIVE at every step: a producer that moves an obstacle on the device between two steps moves the
 * force. A later sai2b_set_collision changes the body with it; sai2b_clear_collision clears the whole-arm contact too.
 * Batch-uniform (sai2b_body_contact_config): `categories`, bit c = 1 << (enum sai2b_collision_category) c: which of plane,
 * obstacle and self push; v_eps > 0, the friction regularisation (m/s). PER ROBOT, doubles, rows [3][B]: stiffness k (N/m),
 * damping d (s/m), friction mu; finite and >= 0 when given from the host (device rows are copied as they are). A robot whose
 * three rows are not all >= 0 (a NaN compares false) feels nothing, as does one with k = 0. SAI2B_BUF_BODY_CONTACT.
 * THE LAW. x: a sphere's centre; v(c): the velocity of the link's material point at c, 0 on link -1. EVERY tested candidate
 * that penetrates contributes, not the deepest alone:
 *     plane p, sphere k      u = n                          delta = r_k - n . (x_k - p0)        c = x_k - r_k u      v_rel = v(c)
 *     obstacle o, sphere k   u = (x_k - c_o) / |x_k - c_o|  delta = r_k + r_o - |x_k - c_o|     c = x_k - r_k u      v_rel = v(c)
 *     self pair (i, j)       u = (x_i - x_j) / |x_i - x_j|  delta = r_i + r_j - |x_i - x_j|     c_i = x_i - r_i u, c_j = x_j + r_j u
 *                            v_rel = v(c_i) - v(c_j); F acts on link(i) at c_i and -F on link(j) at c_j
 *   A zero norm gives no force. The force is the contact's (sai2b_set_contact), term for term:
 *     vn = u . v_rel,  f_n = max(0, k max(0, delta) (1 - d vn)),  v_t = v_rel - vn u,
 *     F = f_n u - mu f_n v_t / sqrt(|v_t|^2 + v_eps^2)
 *   Every comparison is written so that a NaN operand gives false: an absent (NaN) plane or obstacle gives no force.
 *   Joint torques tb_m = sum z_m . ((c - o_m) x F) about a revolute joint m <= link, z_m . F along a prismatic one, 0 beyond.
 *   tb enters the step exactly where the plane contact's tc does: explicit in the plain step, on the right-hand side of the
 *   linear-implicit step when joint dynamics are set, never clipped by the torque limit.
 * STATUS, at the final state after the last substep, [9 + dof][B] (SAI2B_BUF_BODY_CONTACT_STATUS): rows 0-2 per category the
 * deepest max(0, delta), 0 without a penetration (geometry alone: also for a robot with k = 0); rows 3-5 its witness index in the
 * collision's encoding (16 p + k, 16 o + k, 16 i + j; of equally deep ones the smallest), -1 without one, an exact integer stored
 * as a double; rows 6-8 the sum of f_n; rows 9.. tb. COUNTS on the device, int[4]: robots with some f_n > 0 per category, and
 * in any.
 * Snapshot banks hold neither rows nor status (they stay with the robot index, like the collision's); no sensor reads the body
 * forces. This law is this library's definition. */
typedef struct sai2b_body_contact_config {
	int categories; /* bits 1 << SAI2B_COL_PLANE, 1 << SAI2B_COL_OBSTACLE, 1 << SAI2B_COL_SELF */
	int reserved0;
	double v_eps;
	int reserved[8];
} sai2b_body_contact_config;
/* host only: every category, v_eps = 1e-3 */
int sai2b_default_body_contact(sai2b_body_contact_config* cfg);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg: no category or unknown bits, v_eps not finite or not > 0 */
int sai2b_validate_body_contact(const sai2b_body_contact_config* cfg, int robot_dof, char* msg, int msg_len);
/* sizeof(sai2b_body_contact_config) as the library was compiled, for bindings that mirror the struct */
int sai2b_sizeof_body_contact_config(void);
/* rows [3][B] (k, d, mu), host (validated: finite and >= 0) or device when on_device != 0 (stream contract, copied as they are).
 * SAI2B_INVALID_ARGUMENT without a collision configuration, with NULL rows, or for what the validator rejects. A call that fails
 * on its arguments leaves the context as it was; one that fails while copying the rows leaves the plant without whole-arm
 * contact (never with rows that are half the old ones and half the new). */
int sai2b_set_body_contact(sai2b_ctx* ctx, const sai2b_body_contact_config* cfg, const double* rows, int on_device);
/* back to the plant without it (the rows are kept for a later set; both buffers give NULL, the status reads as zeros) */
int sai2b_clear_body_contact(sai2b_ctx* ctx);
/* the configuration and the rows to the host (either may be NULL); without one: categories 0 and zero rows */
int sai2b_get_body_contact(sai2b_ctx* ctx, sai2b_body_contact_config* cfg, double* rows);
/* what the last sai2b_sim_step left: status [9 + dof][B] and counts int[4] (either may be NULL); zeros before the first step
 * with the feature and after a clear. Waits for the ctx stream. */
int sai2b_get_body_contact_state(sai2b_ctx* ctx, double* status, int counts[4]);

/* ------------------------------------------------------------------ inverse kinematics
 * Poses to joints, for every robot, in ONE launch (sai2b_solve_ik): a damped least-squares (Levenberg-Marquardt) solve for the
 * control frame of a MotionForceTask, per robot from a seed q to a goal pose, with optional restarts from seeds drawn on the
 * device. The call keeps no per-robot state and changes none of the controller's: it reads the model, the task's link and control
 * frame and (when asked) the state and the task's goal rows, and writes only its outputs. A context that never configures it
 * launches exactly what it launches without this feature; a configured one launches ik_kernel only in sai2b_solve_ik.
 * FRAME. x(q), R(q): origin and rotation of the task's control frame in the world (the base after
 * sai2b_model_set_base_transform), chain convention of include/sai2b_detfk.h, plain FP64. J(q), 6 x dof, world frame: column m
 * is (z_m x (x - o_m) ; z_m) about a revolute joint and (z_m ; 0) along a prismatic one for m <= the task's link, 0 beyond; z_m
 * the world z of joint m's frame, o_m its world origin.
 * ERROR. e = (x_goal - x ; r), r the rotation vector of D = R_goal R^T in the world frame, the full logarithm: with
 * c = (tr D - 1) / 2 clamped to [-1, 1], v = vee(D - D^T) / 2, s = |v|, theta = atan2(s, c):
 *     c >= 0:  r = (theta / s) v, and r = v when s < 1e-12
 *     c <  0:  M = (D + D^T) / 2 - c I; k the first largest diagonal entry of M; a = M[:, k] / sqrt((1 - c) M[k][k]), negated when
 *              a . v < 0; r = theta a   (accurate up to theta = pi, where v vanishes)
 * WEIGHTS. axes: bit i selects component i of e (x, y, z, wx, wy, wz; world frame). W = diag(axes . (1, 1, 1, L, L, L)) with
 * L = rot_length > 0 in metres per radian. E(q) = |W e|^2. pos(q), rot(q): the 2-norms of the selected components of e's first
 * and last three entries, unweighted. CONVERGED means pos <= tol_pos and rot <= tol_rot.
 * LIMITS. lo = q_lower + limit_margin, hi = q_upper - limit_margin with use_limits, -inf and +inf without. clamp(q) =
 * min(max(q, lo), hi) per joint.
 * A START n = 0 .. restarts: q = clamp(seed) for n = 0; for n >= 1, q_i = lo_i + (hi_i - lo_i) u_i (one product, one sum: the
 * reset sampler's rs_lerp) with u_i = (word (i mod 4) + 0.5) 2^-32 of Philox4x32-10 under key (seed & 0xffffffff, seed >> 32)
 * and counter (n, draw_id, 256 * 11 + i / 4, first_robot + b): STREAM 11 (streams 0-1 are the hardware's, 2-4 the episode
 * sampler's, 5-9 the environment sampler's, 10 the joint sensor's). mu = mu0, and then, while the robot has not converged and
 * fewer than max_iterations iterations of this start have run, ONE ITERATION:
 *     solve (J^T W^2 J + (mu + nu) I) d = J^T W^2 e + nu (q_rest - q)       (Cholesky; nu = rest_weight, 0 drops q_rest)
 *     m = max_i |d_i|;  if m > step_max: d = (step_max / m) d
 *     q' = clamp(q + d);   e' = e(q')                                        (the pose alone)
 *     if E(q') < E(q) (strictly; false for a NaN): q = q', mu = max(mu mu_down, mu_min), and J is rebuilt at q
 *     else: q stays, mu = min(mu mu_up, mu_max)
 * A robot that converges stops: its q is q_out. A start that ends without convergence leaves its q (its smallest E: E never grows
 * within a start) as a candidate; the robot keeps the candidate of start 0, replaced by a later start's only when that one's E is
 * strictly smaller, and starts again while n < restarts. A robot not converged after the last start is EXHAUSTED and gets that
 * best candidate.
 * OUTPUT per selected robot: q_out [dof][B]; status [5][B] = pos(q_out), rot(q_out), iterations spent over all starts, the index
 * of the start that produced q_out, mu as the solve ended (counts and indices are exact integers stored as doubles); a flags byte:
 * 1 converged, 2 exhausted, 4 some q_out_i <= lo_i or >= hi_i (use_limits only), 8 the goal pose, the seed or the rest posture is
 * not finite. A robot with bit 8 gets that bit alone, is counted, and its q_out and status are NOT written. An unselected
 * robot's q_out, status and flags are not touched. COUNTS on the device: selected, converged, exhausted, non-finite.
 * INPUT ROWS. goal_rows [12 (+ dof)][B]: position 3, rotation 9 row-major (goal_source = SAI2B_IK_ROWS; with
 * SAI2B_IK_TASK_GOAL the task's current goal rows are read instead and these 12 rows are absent), then the rest posture q_rest,
 * dof rows, when rest_weight > 0. seed_rows [dof][B] (seed_source = SAI2B_IK_ROWS), or the robot's q in the configured view
 * (SAI2B_IK_STATE; view as sai2b_collision_config's: 0 the truth, 1 the measured q while a joint sensor is set).
 * COMPOSITION: q_out in device memory is what sai2b_reset_robots(mask, q, dq, on_device = 1), sai2b_set_jt_goals and
 * sai2b_set_mft_type1_posture take; flags & 1 is a mask. Snapshot banks hold nothing of this. This law is this library's
 * definition. */
enum sai2b_ik_source { SAI2B_IK_ROWS = 0, SAI2B_IK_TASK_GOAL = 1, SAI2B_IK_STATE = 1 };
enum sai2b_ik_flag { SAI2B_IK_CONVERGED = 1, SAI2B_IK_EXHAUSTED = 2, SAI2B_IK_AT_LIMIT = 4, SAI2B_IK_NONFINITE = 8 };
#define SAI2B_IK_MAX_ITERATIONS 200
#define SAI2B_IK_MAX_RESTARTS 16
#define SAI2B_IK_STATUS_ROWS 5
typedef struct sai2b_ik_config {
	int task;			/* a MotionForceTask: its link and control frame are solved for */
	int axes;			/* bits 0-5: x, y, z, wx, wy, wz of the world-frame error; at least one */
	int max_iterations; /* per start, 1..SAI2B_IK_MAX_ITERATIONS */
	int restarts;		/* 0..SAI2B_IK_MAX_RESTARTS further starts from drawn seeds */
	int use_limits;		/* clamp every iterate to q_lower + limit_margin .. q_upper - limit_margin */
	int view;			/* seed_source = SAI2B_IK_STATE: 0 the plant's q, 1 the measured q while a joint sensor is set */
	int goal_source;	/* SAI2B_IK_ROWS or SAI2B_IK_TASK_GOAL */
	int seed_source;	/* SAI2B_IK_ROWS or SAI2B_IK_STATE */
	double rot_length;	/* L > 0, metres per radian */
	double tol_pos, tol_rot;
	double mu0, mu_min, mu_max, mu_down, mu_up; /* 0 < mu_min <= mu0 <= mu_max, 0 < mu_down < 1 < mu_up */
	double step_max;							/* > 0: the largest |d_i| of one step */
	double limit_margin;						/* >= 0 */
	double rest_weight;							/* nu >= 0 */
	unsigned long long seed;					/* the generator's key */
	unsigned first_robot;						/* global index of this context's robot 0 (shards) */
	unsigned draw_id;							/* second counter word: a caller that wants fresh restarts per call bumps it */
	int reserved[8];
} sai2b_ik_config;
/* host only: task 0, every axis, L = 0.25, 40 iterations, no restart, tolerances 1e-6, mu0 1e-2 in [1e-9, 1e3], mu_down 0.25,
 * mu_up 8, step_max 0.5, limits on with margin 0, no rest posture, view 0, goal and seed from the call's rows, seed 0 */
int sai2b_default_ik(sai2b_ik_config* cfg);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg: a task index outside [0, SAI2B_MAX_TASKS), axes without
 * a bit or with unknown bits, rot_length / tolerances / schedule / step_max / limit_margin / rest_weight outside what the law
 * states above or not finite, counts out of range, view / sources unknown. q_lower, q_upper [robot_dof]: the model's limits, or
 * both NULL when they are not known yet (sai2b_set_ik checks with the context's model): with use_limits a clamped interval
 * must not be empty or NaN; with restarts > 0 limits must be in use and every clamped limit finite. */
int sai2b_validate_ik(const sai2b_ik_config* cfg, int robot_dof, const double* q_lower, const double* q_upper, char* msg, int msg_len);
/* sizeof(sai2b_ik_config) as the library was compiled, for bindings that mirror the struct */
int sai2b_sizeof_ik_config(void);
/* host only: rows of goal_rows (12 with goal_source = SAI2B_IK_ROWS, plus robot_dof with rest_weight > 0; the pose rows come
 * first) and of seed_rows (robot_dof or 0) that sai2b_solve_ik reads under this configuration. Either output may be NULL. */
int sai2b_ik_input_rows(const sai2b_ik_config* cfg, int robot_dof, int* goal_rows, int* seed_rows);
/* validates (with the context's model; the task must be a MotionForceTask) and keeps the configuration. No launch, no device
 * memory but the four counters. A failing call leaves the context as it was. */
int sai2b_set_ik(sai2b_ctx* ctx, const sai2b_ik_config* cfg);
/* back to a context without the feature: sai2b_solve_ik fails from here on */
int sai2b_clear_ik(sai2b_ctx* ctx);
/* the configuration in force; SAI2B_INVALID_ARGUMENT without one */
int sai2b_get_ik(sai2b_ctx* ctx, sai2b_ik_config* cfg);
/* One launch. goal_rows, seed_rows: as sai2b_ik_input_rows counts them; one that has no rows may be NULL. mask: [B] bytes, a robot
 * with a non-zero byte is solved for; NULL: every robot. q_out [dof][B], status [5][B], flags [B] bytes: all three required.
 * Everything in host memory, or everything in device memory when on_device != 0 (stream contract of sai2b_set_caller_stream). A host
 * call stages the three outputs on the device as the caller passed them, so that what the kernel leaves untouched comes back
 * unchanged. The task's control frame is read at this call (a later sai2b_update_task_config is seen); a deferred
 * sai2b_update_task_models is not touched. SAI2B_INVALID_ARGUMENT and no launch without a configuration,
 * with a missing array, or when the task is not a MotionForceTask. */
int sai2b_solve_ik(sai2b_ctx* ctx, const double* goal_rows, const double* seed_rows, const unsigned char* mask, double* q_out, double* status,
				   unsigned char* flags, int on_device);
/* of the last sai2b_solve_ik, counted on the device: robots selected, converged, exhausted, not finite. Zeros before the first;
 * SAI2B_INVALID_ARGUMENT without a configuration. Waits for the ctx stream. */
int sai2b_get_ik_counts(sai2b_ctx* ctx, int counts[4]);

/* ------------------------------------------------------------------ episode starts
 * Where a reset robot starts and what it is asked to do, drawn on the device: sai2b_reset_robots_sampled is sai2b_reset_robots
 * with q, dq and the goals of the new episode drawn per robot, in ONE launch (plus the follow-up launches sai2b_reset_robots makes
 * for the hardware's clocks and the reward's accumulators), for the robots a [B] byte mask selects. The resident loop  tick,
 * sai2b_sim_step(NULL), sai2b_observe_reward, policy, sai2b_apply_action, sai2b_reset_robots_sampled(done)  then leaves the device
 * for nothing but the policy. A context that never configures the sampler launches exactly what it launches without the feature.
 * Batch-uniform (sai2b_reset_sampler_config): the generator's seed and the global index of this context's robot 0 (as the
 * hardware's), the number of candidates a robot may try, which tasks get a drawn goal, and the three acceptance criteria with
 * their thresholds. Per robot, doubles, rows [row][B], in this order:
 *   q_lower [dof], q_upper [dof]   the box candidates are drawn from. Default: the middle 80 % of the model's joint range,
 *                                  mid -+ 0.8 half with mid = (lower + upper) / 2, half = (upper - lower) / 2
 *   dq_sigma [dof]                 standard deviation of the start velocity. Default 0
 *   q_nominal [dof]                the posture of a robot whose candidates were all rejected. Default mid
 *   for every MotionForceTask of goal_tasks, in task order: pos_lower [3], pos_upper [3], theta_max [1]. Default 0
 *   then for every JointTask of goal_tasks, in task order: half_width [task_dof]. Default 0
 * State per robot: an episode counter e (int, 0 after sai2b_set_reset_sampler) and the candidates the last call used.
 *
 * THE LAW, per selected robot b with e as on entry. Random numbers: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32), as the
 * hardware's; word x gives u = (x + 0.5) 2^-32; "call j" of a stream has the counter (n, e, 256 stream + j, first_robot + b).
 *  1. CANDIDATES, tries n = 0 .. max_tries - 1, stream 2: joint i takes u_i = word i mod 4 of call i / 4 and
 *       q_i = q_lower_i + (q_upper_i - q_lower_i) u_i        one product and one sum, never fused: lower == upper gives lower
 *  2. CRITERIA on the candidate; the first n whose candidate passes every configured criterion wins, tries = n + 1:
 *     (a) ratio_task >= 0: with J the 6 x dof world-frame Jacobian of that MotionForceTask's control point (linear rows first)
 *         and P its 6 x 6 partial projection (the task stands at level 1: N_prec = I), s_0 >= s_1 >= .. >= s_5 the singular values
 *         of P J (those beyond dof are 0) and r the rank of P: accept iff s_(r-1) / s_0 >= min_ratio;
 *     (b) box_task >= 0: accept iff box_lower_k <= x_k <= box_upper_k, k = 0..2, x that task's control point in the world frame;
 *     (c) use_clearance: with the contact's link, its points c_k (link frame) and this robot's plane rows (point p0, unit normal
 *         n): accept iff n . (p0 - x_k) <= -clearance for every point x_k = p_link + R_link c_k;
 *     a comparison with a NaN is false: a candidate that is not finite is rejected. Without any criterion candidate 0 wins.
 *  3. EXHAUSTED, no candidate accepted: q = q_nominal, dq = 0 exactly, tries = max_tries + 1, the robot is counted; it still
 *     gets its goals drawn.
 *  4. VELOCITY (accepted robots), stream 3 with n = 0: dq_i = dq_sigma_i z_i, z_i the unit normal i mod 4 of call i / 4 as the
 *     hardware law derives it; dq_sigma_i == 0 gives exactly 0.
 *  5. RESET: everything sai2b_reset_robots(mask, q, dq) does for the robot: state columns, tasks, generators and passivity
 *     observers re-initialised at the new pose, torque columns zeroed, the hardware's clocks and the reward's accumulators.
 *     Every goal now is the start pose: x, R of a MotionForceTask, S q of a JointTask.
 *  6. GOALS of every task t of goal_tasks, stream 4 with n = t:
 *     MotionForceTask: call 0 words 0..2 give p_k = pos_lower_k + (pos_upper_k - pos_lower_k) u_k and the goal position x + p,
 *       or p itself when bit t of absolute_position is set; theta = theta_max u with u word 3 of call 0; call 1 words 0, 1 give
 *       c = 2 u0 - 1, phi = 2 pi u1, the axis a = (sqrt(1 - c^2) cos phi, sqrt(1 - c^2) sin phi, c) (uniform on the sphere) and
 *       the goal rotation R (I + sin(theta) K + (1 - cos(theta)) K^2), K = [a]x; theta_max == 0 keeps R bit for bit.
 *     JointTask: goal_j = (S q)_j + half_width_j (2 u_j - 1), u_j word j mod 4 of call j / 4.
 *     Velocity, acceleration and wrench goals stay zero. An internal generator plans to the drawn goal at the next tick, exactly
 *     as after a goal setter.
 *  7. e = e + 1. Robots the mask does not select are neither read nor written.
 * The draws of a robot depend on the seed, its global index and its episode alone: shards with first_robot set reproduce the
 * one-context run bit for bit. The episode counter is a block of SAI2B_SNAP_EPISODE; seed and first_robot are configuration and
 * are neither stored in a bank nor part of its fingerprint. sai2b_reset_robots and sai2b_reinitialize_robots do not touch e.
 * This law is this library's definition. */
#define SAI2B_MAX_RESET_TRIES 64
typedef struct sai2b_reset_sampler_config {
	unsigned long long seed;
	unsigned first_robot;		/* global index of robot 0 of this context (0 unless the batch is a shard) */
	int max_tries;				/* 1 .. SAI2B_MAX_RESET_TRIES candidates per robot and call */
	unsigned goal_tasks;		/* bit t: draw task t's goal (MotionForceTask or JointTask) */
	unsigned absolute_position; /* bit t: MotionForceTask t's position box is in the world frame, else relative to the start pose */
	int ratio_task;				/* MotionForceTask of the singularity criterion, or -1 */
	double min_ratio;			/* accept iff s_(rank-1) / s_0 >= min_ratio; in [0, 1] */
	int box_task;				/* MotionForceTask whose control point must start inside the box, or -1 */
	double box_lower[3], box_upper[3]; /* world frame */
	int use_clearance;			/* 0 / 1; needs sai2b_set_contact: every contact point at least `clearance` outside the robot's plane */
	double clearance;			/* metres */
} sai2b_reset_sampler_config;
/* host only: seed 0, first_robot 0, max_tries 8, no goal, no criterion */
int sai2b_default_reset_sampler(sai2b_reset_sampler_config* cfg);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg (max_tries outside [1, SAI2B_MAX_RESET_TRIES]; a bit of
 * goal_tasks beyond the task list; a bit of absolute_position that is not a MotionForceTask of goal_tasks; ratio_task or box_task
 * neither -1 nor a MotionForceTask of `tasks`; min_ratio outside [0, 1]; a box or clearance that is not finite; use_clearance not
 * 0 or 1). That use_clearance needs a contact is checked against a context only (sai2b_set_reset_sampler and every call). */
int sai2b_validate_reset_sampler(const sai2b_reset_sampler_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof,
								 char* msg, int msg_len);
/* sizeof(sai2b_reset_sampler_config) as the library was compiled: a binding that mirrors the struct checks its layout with it */
int sai2b_sizeof_reset_sampler_config(void);
/* host only, the layout arithmetic of the per-robot rows. block: 0 q_lower, 1 q_upper, 2 dq_sigma, 3 q_nominal (task ignored),
 * 4 the goal rows of `task` (7 for a MotionForceTask, task_dof for a JointTask). *n_rows = 0 and *first_row = -1 when the
 * configuration draws no goal for that task; *total_rows: rows of the whole buffer. Any output may be NULL. */
int sai2b_reset_sampler_config_layout(const sai2b_reset_sampler_config* cfg, const sai2b_task_config* tasks, int n_tasks, int robot_dof,
									  int block, int task, int* first_row, int* n_rows, int* total_rows);
/* rows [total_rows][B], NULL: the defaults above. Host rows are validated (SAI2B_INVALID_ARGUMENT with the reason: what
 * sai2b_validate_reset_sampler rejects; use_clearance without a contact in force; anything not finite; q_lower > q_upper;
 * q_nominal outside the model's joint limits; a negative dq_sigma, theta_max or half_width; theta_max > pi); DEVICE rows
 * (on_device != 0) are copied under the stream contract and NOT inspected. Zeroes every robot's episode counter. A call that
 * fails on its arguments leaves the context as it was; one that fails while copying leaves it without a sampler. */
int sai2b_set_reset_sampler(sai2b_ctx* ctx, const sai2b_reset_sampler_config* cfg, const double* rows, int on_device);
/* back to a context without a sampler: sai2b_reset_robots_sampled fails from here on */
int sai2b_clear_reset_sampler(sai2b_ctx* ctx);
/* the configuration and the rows [total_rows][B] to the host (either may be NULL); SAI2B_INVALID_ARGUMENT without a sampler */
int sai2b_get_reset_sampler(sai2b_ctx* ctx, sai2b_reset_sampler_config* cfg, double* rows);
/* The law above for the robots with mask[b] != 0; mask [B] bytes, host or (on_device != 0) device under the stream contract, as
 * sai2b_reset_robots takes it. SAI2B_INVALID_ARGUMENT (nothing is launched): no sampler configured, mask NULL, use_clearance while
 * no contact is in force (it was cleared since). */
int sai2b_reset_robots_sampled(sai2b_ctx* ctx, const unsigned char* mask, int on_device);
/* of the last sai2b_reset_robots_sampled, counted on the device: robots reset, candidates rejected, robots exhausted. Zeros before
 * the first; SAI2B_INVALID_ARGUMENT without a sampler. Waits for the ctx stream. */
int sai2b_get_reset_sampler_counts(sai2b_ctx* ctx, int counts[3]);
/* host arrays [B] each, any NULL: the episode counter e, and the candidates the robot used in the call that reset it last
 * (max_tries + 1: exhausted; 0: never reset). SAI2B_INVALID_ARGUMENT without a sampler. Waits for the ctx stream. */
int sai2b_get_reset_sampler_state(sai2b_ctx* ctx, int* episode, int* tries);

/* ------------------------------------------------------------------ environment sampler
 * Domain randomisation on the device: sai2b_randomize_robots redraws the plant of the robots a [B] byte mask selects, in ONE
 * launch: the payload, the contact plane and its material, the joint dynamics, the actuator and sensor models and a timed push,
 * each a GROUP (enum sai2b_env_group) that can be drawn alone. In the resident loop it stands ahead of the reset:  tick,
 * sai2b_sim_step(NULL), sai2b_observe_reward, policy, sai2b_apply_action, sai2b_randomize_robots(done),
 * sai2b_reset_robots_sampled(done)  so that the reset's clearance criterion sees the new plane. A context that never configures
 * the sampler launches and allocates exactly what it does without the feature. Everything in sai2b_env_sampler_config is
 * batch-uniform; per-robot variety comes from the NOMINAL rows and the draws.
 *
 * SET AND NOMINAL. sai2b_set_env_sampler needs every feature named in `groups` in force: a plant payload (and, with payload_target
 * SAI2B_PAYLOAD_BOTH, a controller payload on the same link), a contact, joint dynamics, hardware (with delay_upper <= its
 * max_delay), an external wrench. It copies, device to device, the per-robot rows of those features as they are now into nominal
 * buffers; every later draw is `nominal op draw`, so draws never compound. A feature setter called afterwards does NOT refresh the
 * nominal: call sai2b_set_env_sampler again. The call zeroes every robot's draw counter c and the sample rows.
 *
 * THE LAW, per selected robot b with c as on entry. Random numbers: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32), as the
 * hardware's; word x gives u = (x + 0.5) 2^-32; "call j" of a stream has the counter (0, c, 256 stream + j, first_robot + b).
 * Streams: 5 payload, 6 contact, 7 joint dynamics, 8 hardware, 9 push.
 *   A range (sai2b_env_range) gives s = lower + (upper - lower) u, one product and one sum, never fused: lower == upper gives lower;
 *   with log_uniform s = exp(ln lower + (ln upper - ln lower) u), the two logarithms taken on the host. A symmetric offset is
 *   half (2 u - 1). An integer draw is lo + min((int) floor((hi - lo + 1) u), hi - lo), stored as a double.
 *   A direction is a = (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z), z = 2 u0 - 1, phi = 2 pi u1: uniform on the sphere.
 *  PAYLOAD, call 0: word 0 the mass scale s, words 1..3 the centre-of-mass offsets o_k = payload_com_half_k (2 u - 1). The plant's
 *     rows become mass s, com_k + o_k, inertia_j s; with SAI2B_PAYLOAD_BOTH the controller's rows get the same s and o, each from
 *     its own nominal.
 *  CONTACT, call 0: word 0 the height h (contact_height), word 1 theta = contact_tilt_max u, words 2, 3 the axis a; call 1: words
 *     0..2 the stiffness, damping and friction scales. p' = p + h n with the nominal n; n' = D n, D = I + sin(theta) K +
 *     (1 - cos(theta)) K^2, K = [a]x, each component a sum of three products from the left; theta == 0 keeps n bit for bit.
 *  JOINT DYNAMICS, parameter p = 0 armature, 1 damping, 2 friction, 3 torque limit: joint i takes word i mod 4 of call 2 p + i / 4;
 *     row = nominal s, so a torque limit of +inf stays +inf. The two limit rows are not touched.
 *  HARDWARE, call 0 word 0: the delay, an integer draw in [delay_lower, delay_upper] (absolute, no nominal). Parameter p = 0 lag,
 *     1 gain, 2 torque noise: joint i takes word i mod 4 of call 1 + 2 p + i / 4; row = nominal s, the lag min(nominal s, 1), and a
 *     robot with some lag clipped is counted. Call 7 words 0..3 and call 8 words 0, 1: the six offsets sensor_bias_half_k (2 u - 1)
 *     added to the nominal bias; call 8 word 2: one scale for the six sensor-noise rows. The filter row and the clocks n, e are not
 *     touched.
 *  PUSH, absolute values, no nominal. Call 0: word 0 the force magnitude (push_force), words 1, 2 its direction, word 3 `steps`,
 *     an integer draw in [push_steps_lower, push_steps_upper]; call 1: word 0 the moment magnitude (push_moment), words 1, 2 its
 *     direction. Rows 0..6 of SAI2B_BUF_EXTERNAL_WRENCH become magnitude times direction, and steps. With a sparse mask and
 *     groups = SAI2B_ENV_PUSH mid-episode this is a random shove.
 *  Then c = c + 1, whatever the groups. Robots the mask does not select are neither read nor written.
 * SAMPLE ROWS (SAI2B_BUF_ENV_SAMPLE, sai2b_get_env_sampler_state), the groups of the configuration in the order of their bits:
 *   payload 4: s, o 3.  contact 8: h, theta, a 3, the three scales.  joint dynamics 4 dof: the scales of p = 0..3, dof rows each.
 *   hardware 8 + 3 dof: delay, the scales of p = 0..2 (dof rows each), the six bias offsets, the sensor-noise scale.
 *   push 9: force magnitude, its direction 3, steps, moment magnitude, its direction 3.
 * A call writes the rows of the groups it draws; the others keep what an earlier call left.
 * The draws of a robot depend on the seed, its global index and its counter alone: shards with first_robot set reproduce the
 * one-context run bit for bit. Snapshot banks: c is a block of SAI2B_SNAP_EPISODE, the sample rows one of SAI2B_SNAP_ENVIRONMENT
 * (they travel with the plant rows they describe); the nominal buffers, seed and first_robot are configuration and never go into
 * a bank. This law is this library's definition. */
enum sai2b_env_group { SAI2B_ENV_PAYLOAD = 1, SAI2B_ENV_CONTACT = 2, SAI2B_ENV_JOINT_DYNAMICS = 4, SAI2B_ENV_HARDWARE = 8, SAI2B_ENV_PUSH = 16 };
typedef struct sai2b_env_range {
	double lower, upper;
	int log_uniform; /* 0 / 1 */
	int reserved;
} sai2b_env_range;
typedef struct sai2b_env_sampler_config {
	unsigned long long seed;
	unsigned first_robot; /* global index of robot 0 of this context (0 unless the batch is a shard) */
	unsigned groups;	  /* bits of sai2b_env_group: what the sampler may draw */
	int payload_target;	  /* SAI2B_PAYLOAD_PLANT or SAI2B_PAYLOAD_BOTH */
	sai2b_env_range payload_mass_scale;
	double payload_com_half[3];		/* metres, link frame */
	sai2b_env_range contact_height; /* metres along the nominal normal */
	double contact_tilt_max;		/* rad, [0, pi] */
	sai2b_env_range contact_stiffness_scale, contact_damping_scale, contact_friction_scale;
	sai2b_env_range armature_scale, damping_scale, friction_scale, torque_limit_scale; /* one draw per joint */
	int delay_lower, delay_upper; /* periods, within [0, max_delay of the hardware in force] */
	sai2b_env_range lag_scale, gain_scale, torque_noise_scale; /* one draw per joint */
	double sensor_bias_half[6];
	sai2b_env_range sensor_noise_scale;
	sai2b_env_range push_force, push_moment; /* N, N m */
	int push_steps_lower, push_steps_upper;	 /* periods >= 0 */
} sai2b_env_sampler_config;
/* host only: every scale [1, 1], every offset, height, tilt, delay and push 0, SAI2B_PAYLOAD_PLANT, groups 0 */
int sai2b_default_env_sampler(sai2b_env_sampler_config* cfg);
/* host only: SAI2B_OK, or SAI2B_INVALID_ARGUMENT with the reason in msg, each with its own text: unknown group bits; a
 * payload_target other than the two named; a range with lower > upper or a bound that is not finite; a scale range with
 * lower < 0, or lower <= 0 under log_uniform; log_uniform not 0 or 1; lag_scale.lower not > 0; a negative or non-finite half;
 * contact_tilt_max outside [0, pi]; a delay outside [0, SAI2B_MAX_ACTUATION_DELAY] or delay_lower > delay_upper; negative push
 * steps or push_steps_lower > push_steps_upper. (contact_height may be negative; push magnitudes are scale ranges.) Every field is
 * checked whatever `groups` says. That delay_upper <= max_delay of the hardware in force is checked against a context only. */
int sai2b_validate_env_sampler(const sai2b_env_sampler_config* cfg, int robot_dof, char* msg, int msg_len);
/* sizeof(sai2b_env_sampler_config) as the library was compiled: a binding that mirrors the struct checks its layout with it */
int sai2b_sizeof_env_sampler_config(void);
/* host only, the layout arithmetic of the sample rows. group: ONE bit of sai2b_env_group. *n_rows = 0 and *first_row = -1 when
 * cfg->groups does not hold that group; *total_rows: rows of the whole buffer. Any output may be NULL. */
int sai2b_env_sampler_config_layout(const sai2b_env_sampler_config* cfg, int robot_dof, int group, int* first_row, int* n_rows,
									int* total_rows);
/* SAI2B_INVALID_ARGUMENT with the reason: what sai2b_validate_env_sampler rejects; a group whose feature is not in force;
 * delay_upper above the hardware's max_delay. Copies the nominal rows on the ctx stream, zeroes the counters and the sample rows.
 * A call that fails on its arguments leaves the context as it was; one that fails while copying (SAI2B_RUNTIME_ERROR) leaves it
 * without a sampler. */
int sai2b_set_env_sampler(sai2b_ctx* ctx, const sai2b_env_sampler_config* cfg);
/* back to a context without a sampler: sai2b_randomize_robots fails from here on (the feature rows stay as last drawn) */
int sai2b_clear_env_sampler(sai2b_ctx* ctx);
/* the configuration in force; SAI2B_INVALID_ARGUMENT without a sampler */
int sai2b_get_env_sampler(sai2b_ctx* ctx, sai2b_env_sampler_config* cfg);
/* The law above for the robots with mask[b] != 0 and the groups of `groups` (0: every configured group); mask [B] bytes, host or
 * (on_device != 0) device under the stream contract, staged and ordered as sai2b_reset_robots does it. One launch.
 * SAI2B_INVALID_ARGUMENT (nothing is launched): no sampler configured; mask NULL; a bit of `groups` that was not configured; a
 * group to be drawn whose feature has been cleared since (or whose hardware now has max_delay < delay_upper). */
int sai2b_randomize_robots(sai2b_ctx* ctx, const unsigned char* mask, unsigned groups, int on_device);
/* of the last sai2b_randomize_robots, counted on the device: robots drawn; robots with a lag clipped at 1. Zeros before the first;
 * SAI2B_INVALID_ARGUMENT without a sampler. Waits for the ctx stream. */
int sai2b_get_env_sampler_counts(sai2b_ctx* ctx, int counts[2]);
/* host arrays, any NULL: draw_counter [B] ints = c, sample_rows [total_rows][B]. SAI2B_INVALID_ARGUMENT without a sampler. Waits
 * for the ctx stream. */
int sai2b_get_env_sampler_state(sai2b_ctx* ctx, int* draw_counter, double* sample_rows);

/* ------------------------------------------------------------------ snapshot banks
 * Whole robot states, saved to and restored from device memory: branching (copy one robot into K siblings, roll them out, come
 * back), reset to a bank of stored states, checkpoint and resume. A bank holds `capacity` slots of one robot's state each,
 * structure-of-arrays [word][capacity] like the context, and one valid byte per slot.
 *
 * What a robot's state is. SAI2B_SNAP_EPISODE: everything a later tick, sim_step, observe, apply_action or task-level call of
 * that robot can read and that sai2b_reset_robots would have replaced or that advances with time: q, dq, the stored torques,
 * the cached pose; per task the goals, the sensed wrench, the integrators and singularity histories (state, istate), the
 * trajectory generator (desired rows, state, the jerk-limited profile), the passivity observer and the task-level N_prec where
 * these exist; the episode step; the remaining periods of a timed push; the contact, joint-dynamics and wrench status rows that
 * sai2b_observe and the sensor path read. SAI2B_SNAP_ENVIRONMENT: what sai2b_reset_robots documents as kept: both payload
 * buffers, the contact rows, the joint-dynamics rows and the force and moment rows of the external wrench.
 * NOT state, never restored: batch-level counts, work lists, route-switch probes, introspection outputs and the N, N_total
 * and tau outputs of task-level calls; batch-uniform configuration (gains, limits, which features are in force).
 * A load invalidates the cached models exactly as sai2b_reset_robots does: the next tick or task-level call updates them, the
 * generators compare their goals again.
 *
 * Layout. Fixed when the bank is created, from the joint count, every task's type, size, generator mode and observer and
 * which optional buffers exist (csrc/sai2b_snapshot_layout.h); its fingerprint is kept in the bank and in an exported blob.
 * save / load on a context whose layout has changed since (a contact set after a bank with SAI2B_SNAP_ENVIRONMENT was made, a
 * generator switched to jerk-limited), or on another context than the bank's, and import of a blob with another fingerprint
 * or capacity, return SAI2B_INVALID_ARGUMENT; the message names the first differing block; nothing is written.
 *
 * Slots. Robot b with mask[b] != 0 (mask NULL: every robot) <-> slot[b] (slot NULL: slot b). A robot whose slot is outside
 * [0, capacity), or on load was never saved, is left untouched and counted, as sai2b_apply_action leaves a robot with a
 * non-finite action; the host does not reject such a call. Two robots saving to one slot in one call: one of them wins, and
 * which words come from which is UNDEFINED. A load may name one slot for many robots: that is the clone.
 *
 * Ordering. Both calls flush a deferred sai2b_update_task_models first, are ONE launch whatever the mask selects, and follow
 * the stream contract below for on_device != 0 (slot and mask are then device pointers, read before anything the caller
 * enqueues on its stream after the call). Host slot / mask arrays are staged as sai2b_reset_robots stages its mask.
 * The cached pose is one flag for the batch (q itself until the state moves on, a column of its own afterwards): a save
 * stores the pose from wherever it lives; a load always leaves it in the column of its own, for the robots it does not select
 * too (copied in the same launch). Destroy a bank before its context. */
enum { SAI2B_SNAP_EPISODE = 1, SAI2B_SNAP_ENVIRONMENT = 2 };
#define SAI2B_SNAPSHOT_HEADER_BYTES 256 /* of an exported blob: header, then words * 4 * capacity, then capacity valid bytes */
typedef struct sai2b_snapshot_bank sai2b_snapshot_bank;
/* 4-byte words per robot for this context as configured now; -1 for a bad argument */
int sai2b_snapshot_words(sai2b_ctx* ctx, int what);
/* the row table behind sai2b_snapshot_words: up to max_rows entries of {block id, task or -1, rows, element bytes, first word}
 * (block ids: enum SnapBlock of csrc/sai2b_snapshot_layout.h); returns the number of entries of the table, -1 for a bad argument */
int sai2b_snapshot_layout(sai2b_ctx* ctx, int what, int* table5, int max_rows);
int sai2b_snapshot_bank_create(sai2b_ctx* ctx, int capacity, int what, sai2b_snapshot_bank** out);
void sai2b_snapshot_bank_destroy(sai2b_snapshot_bank* bank);
int sai2b_snapshot_save(sai2b_ctx* ctx, sai2b_snapshot_bank* bank, const int* slot, const unsigned char* mask, int on_device);
int sai2b_snapshot_load(sai2b_ctx* ctx, sai2b_snapshot_bank* bank, const int* slot, const unsigned char* mask, int on_device);
/* of the last save / load of this context, counted on the device: robots moved, slot out of range, slot never saved. Zeros
 * before the first. Waits for the ctx stream; the counts arrive through mapped host words, no copy is enqueued. */
int sai2b_get_snapshot_counts(sai2b_ctx* ctx, int counts[3]);
/* A bank as a host blob: SAI2B_SNAPSHOT_HEADER_BYTES of header (fingerprint, layout description, capacity), the words, the
 * valid bytes. export / import wait for the last save / load of the bank. import into a bank of a fresh context built from
 * the same configuration, then load: the context continues bit-equal. */
size_t sai2b_snapshot_export_size(const sai2b_snapshot_bank* bank);
int sai2b_snapshot_export(sai2b_snapshot_bank* bank, void* host_blob, size_t size);
int sai2b_snapshot_import(sai2b_snapshot_bank* bank, const void* host_blob, size_t size);

/* ------------------------------------------------------------------ simulation harness
 * What the reference's examples obtain from the external sai2-simulation (examples/05-...cpp:215-236:
 * setJointTorques / integrate / getJointPositions, getJointVelocities): one control period of
 * rigid-body dynamics  M qdd + C dq (+ g) = tau  for every robot, with the state staying in device
 * memory between ticks. tau [7][B] (host, or device when on_device != 0; NULL = the torques of the
 * last sai2b_compute_control_torques / sai2b_tick) is held over dt, which is split into `substeps`
 * semi-implicit Euler steps. with_gravity uses sai2b_robot_model.gravity (the example worlds have
 * none). The state buffers (SAI2B_BUF_Q / SAI2B_BUF_DQ) are updated in place. */
int sai2b_sim_step(sai2b_ctx* ctx, const double* tau, int on_device, double dt, int substeps,
				   int with_gravity);
/* current joint positions / velocities to host arrays [7][B] (either may be NULL) */
int sai2b_get_state(sai2b_ctx* ctx, double* q, double* dq);
/* bias vector C(q, dq) dq (+ g(q)) of the current state, host [7][B] (Sai2Model::coriolisForce /
 * jointGravityVector of sai2-model) */
int sai2b_get_bias(sai2b_ctx* ctx, int with_gravity, double* bias);

/* Observers the reference's callers use between ticks, computed from the state and goal buffers as
 * they are now (the reference caches them at the last computeTorques): MotionForceTask::
 * getCurrentPosition / getCurrentOrientation (MotionForceTask.h:121-140), getSensedForce/
 * MomentControlWorldFrame (:154-165), getPositionError / getOrientationError
 * (MotionForceTask.cpp:540-546), and the norms sqrt(e^T sigma e) that goalPositionReached /
 * goalOrientationReached compare with their tolerance (:548-579). Host arrays [rows][B], any NULL. */
int sai2b_get_mft_status(sai2b_ctx* ctx, int task, double* pos, double* rot, double* sensed_force_world,
						 double* sensed_moment_world, double* pos_error, double* ori_error,
						 double* pos_error_norm, double* ori_error_norm);
/* MotionForceTask::getCurrentLinearVelocity / getCurrentAngularVelocity (MotionForceTask.h:127-146; J dq of
 * the state as it is now, MotionForceTask.cpp:293-298): host [3][B] each, any NULL */
int sai2b_get_mft_velocity(sai2b_ctx* ctx, int task, double* linear_velocity, double* angular_velocity);
/* MotionForceTask::sigmaForce / sigmaPosition / sigmaMoment / sigmaOrientation (MotionForceTask.h:610-613,
 * MotionForceTask.cpp:892-971) for the state as it is now (they depend on the robot only when the spaces are
 * parametrised in the compliant frame): host [9][B] row-major each, any NULL */
int sai2b_get_mft_sigma(sai2b_ctx* ctx, int task, double* sigma_force, double* sigma_position,
						double* sigma_moment, double* sigma_orientation);
/* MotionForceTask::setType1Posture (MotionForceTask.h:706 -> SingularityHandler.h:140-142): the posture the
 * type-1 singularity strategy holds, [n][B]; kept until the handler next refreshes it
 * (SingularityHandler.cpp:233-236), as in the reference */
int sai2b_set_mft_type1_posture(sai2b_ctx* ctx, int task, const double* q_des, int on_device);
/* getGoalPosition ... getGoalMoment (MotionForceTask.h:214-247,  JointTask.h:144-160) */
int sai2b_get_mft_goals(sai2b_ctx* ctx, int task, double* pos, double* rot, double* lin_vel, double* ang_vel,
						double* lin_acc, double* ang_acc, double* force, double* moment);
int sai2b_get_jt_goals(sai2b_ctx* ctx, int task, double* q, double* dq, double* ddq);

/* MotionForceTask::resetIntegrators / resetIntegratorsLinear / resetIntegratorsAngular
 * (MotionForceTask.cpp:988-1001) and JointTask::resetIntegrators: which = 0 all, 1 linear (position
 * and force integrals), 2 angular (orientation and moment integrals); JointTask: any value. */
int sai2b_reset_integrators(sai2b_ctx* ctx, int task, int which);

/* Desired state the control law tracked in the last torque computation: the goal, or with the
 * internal OTG on its next state (JointTask::getDesiredPosition/Velocity/Acceleration,
 * JointTask.h:182-198; MotionForceTask::getDesired*). Host arrays, SoA [rows][B]; any may be NULL.
 * No introspection switch needed. */
int sai2b_get_jt_desired(sai2b_ctx* ctx, int task, double* q, double* dq, double* ddq);
int sai2b_get_mft_desired(sai2b_ctx* ctx, int task, double* pos, double* rot, double* lin_vel,
						  double* ang_vel, double* lin_acc, double* ang_acc);
/* Internal OTG flags per robot as doubles [B]: OTG_joints/OTG_6dof_cartesian::isGoalReached()
 * (OTG_joints.h:152, OTG_6dof_cartesian.h:229) and the last ruckig Result (0 working, 1 finished,
 * < 0 error: ruckig/include/ruckig/result.hpp:6-18) */
int sai2b_get_otg_status(sai2b_ctx* ctx, int task, double* goal_reached, double* result);
/* Sai2Model::M(): [49][B]; J of MFT `task` (JWorldFrame): [42][B]; position [3][B], rotation [9][B] */
int sai2b_get_model(sai2b_ctx* ctx, int task, double* M, double* J, double* pos, double* rot);

/* Bench bookkeeping (on the ctx stream, ONE HIP event pair around `steps` back-to-back launches, so no event sits
 * between two kernels): first the first kernel of the tick alone — its average duration per launch in ms —, then the
 * tick's whole launch sequence; second_kernel_ms = what the generic kernel over the work list behind an SVD-free
 * kernel adds to a step (0 when the hierarchy has no such pass). The two add up to the step. The ticks run for real
 * (integrators, generators and singularity histories advance; in the first phase the robots the SVD-free kernel
 * declines are not served): a profiling call, not part of a control loop. */
int sai2b_profile_tick(sai2b_ctx* ctx, int steps, double* first_kernel_ms, double* second_kernel_ms);

/* HIP devices visible to this process (0 when there is none or the runtime fails): what a host that shards a batch
 * over the GPUs of a node creates one context each for (Sai2PrimitivesBatched.h: ShardedRobotController) */
int sai2b_device_count(void);

/* How many robots of the last tick — or of the last task-level call (sai2b_task_update_model / _compute_torques), whichever
 * came last — the SVD-free kernel handed to the generic (Jacobi-SVD) kernel: robots inside or leaving a
 * singularity-blending region (SingularityHandler.cpp:66-160) that the SVD-free kernel does not handle itself, levels it
 * cannot certify. The whole batch when the generic kernel ran alone. Waits for the ctx stream. */
int sai2b_get_fallback_count(sai2b_ctx* ctx, int* robots);

/* What the host knows of the tick's work list (diagnostics, tests). last_seen: the list's length at the host's last look,
 * which is that of the tick 8 before the look (-1: never looked). pending: 0 = no request for the counts is under way,
 * 1 = one is, answered by the pass over the list through mapped host words, 2 = one is, answered by two copies behind
 * the pass (the one-lane generic kernel as the pass, SAI2B_GENERIC_LANES=1). form: what the last tick launched: 0 = the generic
 * kernel alone, 1 = an SVD-free kernel and the generic kernel over its work list behind it, 2 = one launch in which every
 * wavefront serves the robots it declines itself (the headline hierarchies without payload, while the last look found no
 * wavefront with more than four declined robots; SAI2B_NO_SELF_SERVE=1 keeps form 1). wmax: the largest number of robots one
 * wavefront declined, of the same look as last_seen (-1: not known). Any pointer may be NULL. */
int sai2b_get_worklist_state(const sai2b_ctx* ctx, int* last_seen, int* pending, int* form, int* wmax);

/* number of kernel launches and robots processed since creation (bench bookkeeping) */
int sai2b_counters(const sai2b_ctx* ctx, long long* launches, long long* ticks);

#ifdef __cplusplus
}
#endif
#endif /* SAI2B_H_ */
