/* armour_hip.h — C ABI of the MI355X-native ARMOUR planner (libarmour_hip.so).
 *
 * Drop-in boundary. The reference exposes its hot path to MATLAB as a process
 * (KPR/armour_main.cu:12-400) driven through text files by KSI/uarmtd_planner.m:167-230; there is
 * no mex entry. This library is what that process becomes: one call plans a batch of worlds on a
 * GPU, each world being exactly one armour.in (KPR/README.md:99-112, armour_main.cu:54-77), each
 * result exactly one armour*.out set (armour_main.cu:319-398). The drop-in executable
 * `armour_main` (armour-dev_amd/csrc/armour_main.cpp) speaks the file protocol on top of it.
 *
 * Plain C types only; caller-owned inputs and outputs; one planner handle per thread.
 * Every function returns 0 on success or a negative ARMOUR_E_* code; armour_last_error() gives
 * the message (thread-local).
 */
#ifndef ARMOUR_HIP_H
#define ARMOUR_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARMOUR_NUM_FACTORS 7      /* NUM_FACTORS (KPR/KinovaWithoutGripperInfo.h:14) */
#define ARMOUR_OBSTACLE_DOUBLES 12 /* center + 3 generators (armour_main.cu:45, uarmtd_planner.m:189) */

enum {
    ARMOUR_OK = 0,
    ARMOUR_E_ARG = -1,       /* invalid argument (sizes, null pointers) */
    ARMOUR_E_HIP = -2,       /* HIP runtime error / no device */
    ARMOUR_E_CAPACITY = -3,  /* a reach-set job exceeded its arena / sort / output capacity */
    ARMOUR_E_STATE = -4,     /* query before a plan / reach call */
    ARMOUR_E_INTERNAL = -5   /* per-world result only: the solver left this world in a non-terminal
                                state (a solver fault; reported infeasible, not planned) */
};

typedef struct armour_planner armour_planner;

typedef struct armour_config {
    int robot;           /* 0: Kinova Gen3 without gripper (KPR/KinovaWithoutGripperInfo.h) */
    int num_time_steps;  /* NUM_TIME_STEPS (KPR/Parameters.h:17), runtime here, must be even */
    int max_obstacles;   /* per world; MAX_OBSTACLE_NUM (KPR/Parameters.h:26) is 40 */
    int max_worlds;      /* batch capacity */
    int device;          /* HIP device ordinal (-1: current device) */
    int max_iter;        /* solver iteration cap (0: default 100) */
} armour_config;

/* one planning problem: the content of armour.in */
typedef struct armour_world {
    double q0[ARMOUR_NUM_FACTORS];
    double qd0[ARMOUR_NUM_FACTORS];
    double qdd0[ARMOUR_NUM_FACTORS];
    double q_des[ARMOUR_NUM_FACTORS];
    int num_obstacles;
    const double* obstacles; /* [num_obstacles][12] */
} armour_world;

/* one planning result: armour.out (k_opt or infeasible) + solver statistics */
typedef struct armour_result {
    double k_opt[ARMOUR_NUM_FACTORS]; /* normalised, in [-1, 1] (MATLAB scales by pi/48) */
    int feasible;        /* finalize_solution re-check (KPR/NLPclass.cu:449-538) */
    int solver_status;   /* 0 converged, 1 iteration cap, 2 line-search failure (no restoration phase
                            left), 3 not planned (see error), 4 local infeasibility (the restoration
                            phase found no point within the bounds: Ipopt's Infeasible_Problem_Detected
                            role) */
    int iterations;
    int evaluations;
    double cost;         /* objective / COST_FUNCTION_OPTIMALITY_SCALE at k_opt */
    double kkt_error;
    int error;           /* 0, or ARMOUR_E_CAPACITY: this world's reach set exceeded a capacity even
                            after the retry with 4x buffers; it is reported infeasible and not planned,
                            the other worlds of the batch are (armour_plan_batch still returns 0);
                            or ARMOUR_E_INTERNAL (a solver fault, never expected) */
} armour_result;

/* timings of the last batch, device-side (hipEvents on the planner's stream), milliseconds */
typedef struct armour_timing {
    double reach_ms;     /* JRS + PZ FK/RNEA + torque radius + hyperplanes */
    double nlp_ms;       /* solver */
    double total_ms;     /* incl. host<->device copies of inputs and results */
    double reach_kernel_ms; /* reach_kernel alone (hipEvents around its launch) */
    double reach_bytes;  /* algorithmic monomial bytes the PZ operators read + wrote */
} armour_timing;

armour_planner* armour_create(const armour_config* cfg);
void armour_destroy(armour_planner* p);

/* Robot tables: the content of the reference's compile-time robot header (Kinova:
 * KPR/KinovaWithoutGripperInfo.h:10-112; Fetch: ACMP/FetchInfo.h:8-107) as run-time data, so a
 * robot is data rather than a rebuild. Joint i rotates about axis |axes[i]| (1 x, 2 y, 3 z; negative:
 * reversed; 0: fixed) after the frame offset trans[i] / rots[i] (URDF joint origin xyz / rpy);
 * link i (the child of joint i) has mass, centre of mass, inertia (row-major 3x3) and a box
 * zonotope (centre, half extents: the STL bounding box of create_pz_bounding_boxes.m). The first
 * ARMOUR_NUM_FACTORS joints are the actuated ones. armour_amd/robot_tables.py builds these from a
 * URDF and its meshes.
 * A reversed joint, code -a (URDF <axis> -e_a), turns by q about the unit vector -e_a: its rotation
 * is R = Rot(e_a, -q), its angular velocity -qd e_a, and its generalised torque the moment about
 * -e_a: u = -n[a] + armature qdd + damping qd. Its q, limits, speed and torque limits and trajectory
 * parameter k are all counted about -e_a. The robot with joint j reversed, at the state with q0, qd0,
 * qdd0 and q_des of joint j negated, is the same arm: same link sets, torques of joint j negated.
 * The reach program of 8 or 9 joints needs more payload than the per-job reach engine holds; such
 * robots run on the bundle engine at every batch size, and armour_create_robot refuses them with
 * ARMOUR_E_CAPACITY only where ARMOUR_ENGINE=job forces the per-job engine. */
#define ARMOUR_MAX_JOINTS 9
typedef struct armour_robot {
    int num_joints;                               /* NUM_JOINTS, 7..9 */
    int axes[ARMOUR_MAX_JOINTS];
    int wrap[ARMOUR_NUM_FACTORS];                 /* continuous joints: cost term wrapped to [-pi, pi] */
    double trans[(ARMOUR_MAX_JOINTS + 1) * 3];
    double rots[ARMOUR_MAX_JOINTS * 3];
    double mass[ARMOUR_MAX_JOINTS];
    double com[ARMOUR_MAX_JOINTS * 3];
    double inertia[ARMOUR_MAX_JOINTS * 9];
    double mass_uncertainty, inertia_uncertainty;
    double friction[ARMOUR_MAX_JOINTS], damping[ARMOUR_MAX_JOINTS], armature[ARMOUR_MAX_JOINTS];
    double state_lb[ARMOUR_NUM_FACTORS], state_ub[ARMOUR_NUM_FACTORS];  /* +-1000: continuous */
    double speed_limits[ARMOUR_NUM_FACTORS], torque_limits[ARMOUR_NUM_FACTORS];
    double gravity;
    double link_center[ARMOUR_MAX_JOINTS * 3], link_generators[ARMOUR_MAX_JOINTS * 3];
    double alpha, V_m, M_max, M_min, K;           /* ultimate bound of the robust controller */
} armour_robot;

/* compute units of a HIP device (< 0: error). The reach kernel runs one 64-job bundle per CU at a
 * time, so batches of whole bundle waves, W = k * CUs * 64 / num_time_steps worlds, fill the chip. */
int armour_device_compute_units(int device);

/* Diagnostics: device-to-device copy bandwidth of `bytes` (two buffers of that size) with a
 * 16-B-per-lane streaming kernel, `reps` timed copies; GB/s of read + write bytes, or a negative
 * ARMOUR_E_* code. The achievable HBM figure the roofline fractions are read against. */
double armour_copy_bandwidth(int device, size_t bytes, int reps);

/* built-in tables (robot id 0: Kinova Gen3 without gripper); 0 / ARMOUR_E_ARG */
int armour_robot_builtin(int robot_id, armour_robot* out);
/* armour_create with the given robot tables (cfg->robot is ignored) */
armour_planner* armour_create_robot(const armour_config* cfg, const armour_robot* robot);
const char* armour_last_error(void);

/* constraints of a world with O obstacles: 7T + NJ*T*O + 28 (KPR/NLPclass.cu:47-49); ARMTD
 * planners NJ*T*O + 28 (ACMP/NLPclass.cu:45-46) */
int armour_num_constraints(const armour_planner* p, int num_obstacles);

/* The input domain. Every entry that takes worlds (armour_plan, armour_plan_batch, armour_reach_batch,
 * their _mixed forms and the two ARMTD entries) checks every world with armour_check_world /
 * armour_check_armtd_world before it copies or launches anything, and returns ARMOUR_E_ARG with a
 * message that names the field otherwise. A world is inside the domain when
 *   - every q0, qd0, qdd0, q_des and obstacle entry is finite (ARMTD: q0, qd0, q_des, k_range and
 *     every entry of jrs_tables [7][6][num_time_steps] and of the obstacles),
 *   - every |q0| and |q_des| is at most ARMOUR_MAX_ABS_ANGLE (continuous joints carry +-1000 rad
 *     bounds, so nothing beyond is feasible; the cost's wrap to [-pi, pi] of a continuous joint takes
 *     one step per turn and is bounded for such values),
 *   - 0 <= num_obstacles <= max_obstacles, with a non-null obstacles pointer when it is positive.
 * Both checks run on the host and touch no device. */
#define ARMOUR_MAX_ABS_ANGLE 1e4
int armour_check_world(const armour_world* world, int max_obstacles);

/* Plan a batch (all worlds must carry the same number of obstacles). Replaces
 * armour_main.cu:87-316 for each world. */
int armour_plan_batch(armour_planner* p, int num_worlds, const armour_world* worlds, armour_result* results,
                      armour_timing* timing);

/* Plan a mixed batch: every world carries its own number of obstacles, 0 .. max_obstacles (zero
 * included), and the whole batch runs in one reach launch and one solve. Each world's plan is the
 * plan of a uniform batch of its own count (its constraint rows keep that batch's layout and order
 * of summation). armour_plan_batch is unchanged and still refuses mixed counts. Not available on an
 * ARMTD planner or with the fp32 study (ARMOUR_EVAL_F32): ARMOUR_E_ARG.
 * After a mixed batch the getters below size their outputs per world: world w has
 * m_w = armour_num_constraints(p, armour_world_num_obstacles(p, w)) constraints. */
int armour_plan_batch_mixed(armour_planner* p, int num_worlds, const armour_world* worlds, armour_result* results,
                            armour_timing* timing);
/* Reach-set half only for a mixed batch; enables armour_eval_constraints. */
int armour_reach_batch_mixed(armour_planner* p, int num_worlds, const armour_world* worlds, armour_timing* timing);
/* Obstacle count of world w of the last batch (uniform or mixed); ARMOUR_E_STATE before any batch,
 * ARMOUR_E_ARG for a world index out of range. */
int armour_world_num_obstacles(const armour_planner* p, int w);

/* One plan, the whole of one armour_main.cu process (:37-398) on a planner handle: the single-world
 * entry of SURVEY.md §8(b). Inputs are the content of armour.in (caller-owned); the result and timing
 * are written into *out, and so is every output array the caller supplies (null: skipped) — the
 * payloads of the five .out files. Equivalent to armour_plan_batch with one world followed by the
 * getters (world 0). 0 or a negative ARMOUR_E_* code; thread-safe per handle like every entry. */
typedef struct armour_plan_output {
    armour_result result;       /* k_opt (armour.out unless infeasible), feasible, solver status ... */
    armour_timing timing;
    double* constraints;        /* [m] at the final iterate (armour_constraints.out, first m lines) */
    double* joint_bounds;       /* [28] (armour_constraints.out, last 28 lines) */
    double* link_centers;       /* [T][NJ][3] (armour_joint_position_center.out) */
    double* link_generators;    /* [T][NJ][3][6] (armour_joint_position_radius.out) */
    double* torque_radius;      /* [T][7] (armour_control_input_radius.out) */
} armour_plan_output;
int armour_plan(armour_planner* p, const armour_world* world, armour_plan_output* out);

/* The ARMTD comparison planner (kinova_planner_realtime_armtd_comparison/, "ACMP/"): the content
 * of one armtd.in (ACMP/armtd_main.cu:37-102). Joint rotations come from offline JRS tables that the
 * caller slices (KSI/uarmtd_planner.m:260-318) instead of the Bernstein trajectory; the plan keeps
 * forward kinematics and collision avoidance (no RNEA, no torque rows), with the constant-
 * acceleration joint extrema and cost of ACMP/Trajectory.cu:83-383, ACMP/NLPclass.cu:186-246. */
typedef struct armour_armtd_world {
    double q0[ARMOUR_NUM_FACTORS];
    double qd0[ARMOUR_NUM_FACTORS];
    double q_des[ARMOUR_NUM_FACTORS];
    const double* jrs_tables;  /* [7][6][num_time_steps]: per joint c_cos, g_cos, r_cos, c_sin, g_sin, r_sin */
    double k_range[ARMOUR_NUM_FACTORS];
    int num_obstacles;
    const double* obstacles;   /* [num_obstacles][12] */
} armour_armtd_world;

/* armour_check_world for an ARMTD world of a planner with num_time_steps intervals */
int armour_check_armtd_world(const armour_armtd_world* world, int max_obstacles, int num_time_steps);

/* an ARMTD planner (the reference's NUM_TIME_STEPS is 100, ACMP/Parameters.h:17; solver tolerance
 * 1e-7, :42); armour_num_constraints gives 7*T*O + 28, the getters work as for armour_create */
armour_planner* armour_create_armtd(const armour_config* cfg);
int armour_plan_armtd_batch(armour_planner* p, int num_worlds, const armour_armtd_world* worlds,
                            armour_result* results, armour_timing* timing);
int armour_reach_armtd_batch(armour_planner* p, int num_worlds, const armour_armtd_world* worlds, armour_timing* timing);

/* Reach-set half only (armour_main.cu:87-222) for a batch; enables armour_eval_constraints. */
int armour_reach_batch(armour_planner* p, int num_worlds, const armour_world* worlds, armour_timing* timing);

/* eval_g / eval_jac_g (KPR/NLPclass.cu:272-396) of world w of the last batch at x; jac (m x 7,
 * row-major) may be null. The parity-pinning entry. m is world w's own count (m_w after a mixed
 * batch, in the reference's order for its O_w obstacles). */
int armour_eval_constraints(armour_planner* p, int w, const double* x, double* g, double* jac);

/* Evaluate N candidate parameters per world of the last batch (uniform or mixed; after any reach or
 * plan entry) without forming g per candidate in memory and without touching the batch's plan state:
 * the getters return what they returned before and the next plan is the one it would have been.
 * x: [W][N][7], every |x| <= 1. Outputs, each optional (null: skipped):
 *   cost      [W][N]     objective / COST_FUNCTION_OPTIMALITY_SCALE (as armour_result.cost)
 *   violation [W][N][3]  largest excess over the finalize_solution test per row class:
 *                        [0] torque rows   max(L - tv - v, v - U - tv)
 *                        [1] collision rows max(v - cv)   (-infinity for a world with no obstacles)
 *                        [2] the 28 position/velocity extremum rows max(L - v, v - U)
 *   feasible  [W][N]     1 iff no row fails the finalize_solution re-check's comparisons (same
 *                        strictness: what armour_result.feasible would be for a plan ending at that x)
 *   best      [W]        lowest-cost feasible candidate, ties to the lowest index, -1 if none
 * A world whose reach set failed (armour_result.error) gets NaN cost and violations, feasible 0 and
 * best -1; the other worlds are evaluated and the call returns 0.
 * ARMOUR_E_STATE before any batch; ARMOUR_E_ARG for a null p or x, num_candidates < 1, any x that is
 * not finite or lies outside [-1, 1] (the box the collision planes are certified for), an ARMTD
 * planner, or the fp32 study (ARMOUR_EVAL_F32).
 * The collision rows are read from the certified plane cache, built on demand.
 * When a batch with obstacles has no cache (ARMOUR_PLANE_CACHE=0, a batch capacity beyond the cache's
 * 32-bit record pool, or a build that did not fit a pool that could be allocated) the call returns
 * ARMOUR_E_STATE and says so: there is no full-scan path. */
int armour_eval_candidates(armour_planner* p, int num_candidates, const double* x, double* cost, double* violation,
                           int* feasible, int* best);

/* Execution check: the smallest sampled separation between the arm on a trajectory and the obstacles
 * of each world of the last batch (uniform or mixed; after any reach or plan entry; the obstacles
 * resident on the device and the planner's robot tables). No reach set is read: this is the check
 * that an executed plan misses the obstacles, independent of the sets that produced it.
 *   traj  [W][4][7]: q0, qd0, qdd0 and k (normalised, |k| <= 1) of each world's trajectory, the
 *         degree-5 Bezier curve of KPR/Trajectory.cu:542-599 with end point q0 + k * k_range
 *         (k_range = pi/48) and duration 1.
 *   It is evaluated at `samples` evenly spaced times in [t0, t1], a window inside [0, 1], ends included
 *   (sample s at t0 + s * ((t1 - t0) / (samples - 1)), the last at t1; samples = 1: t0 alone).
 *   At each sampled q the link boxes come from point forward kinematics (KPR/Dynamics.cu:69-81 at a
 *   point): p += R trans_i, R = R (RPY_i Rot_axis_i(q_i)); link i's box has centre p + R link_center_i
 *   and the three generators R diag(link_generators_i).
 *   Each link box is tested against each obstacle zonotope on the 15 axes that are the normalised
 *   cross products of all pairs among the 6 generators (obstacle 3, then link 3); a pair whose cross
 *   product has norm exactly 0 is skipped (KPR/CollisionChecking.cu:261-282). The separation is
 *       max_n (|n . (c - c_obs)| - sum_j |n . G_j|)
 *   (-1e8 when every pair was skipped). A positive value means the two sets are disjoint at that
 *   sample and is a lower bound of their distance; a value <= 0 means they intersect (for two
 *   3-generator zonotopes the 15 axes hold every facet normal of their sum).
 *   clearance [W]     the minimum over samples, links and the world's own obstacles (optional)
 *   where     [W][3]  its first minimiser in the order (sample, link, obstacle) (optional)
 *   A world without obstacles gets +infinity and -1, -1, -1.
 * ARMOUR_E_ARG for a null p or traj, a non-finite value, |k| > 1, samples < 1 (or > 65535), t0 > t1
 * or a window outside [0, 1], an ARMTD planner, or the fp32 study (ARMOUR_EVAL_F32); ARMOUR_E_STATE
 * before any batch. It touches no plan state (as armour_eval_candidates): the getters return what
 * they returned before and the next plan is the one it would have been. */
int armour_check_motion(armour_planner* p, const double* traj, double t0, double t1, int samples, double* clearance,
                        int* where);

/* Receding-horizon episodes: the loop of SCR/kinova_run_100_worlds.m with its state on the device.
 * Each step takes the straight-line waypoint (robot_arm_straight_line_HLP.m:45-57), plans, follows
 * the new trajectory for ARMOUR_T_PLAN of its duration 1 (KSI/uarmtd_planner.m:56-62) or, when the
 * plan failed, brakes along the second half of the previous trajectory (uarmtd_planner.m:922-932),
 * and stops on collision or inside the goal radius (kinova_world_static.m:417-425). The state
 * advances on the desired trajectory; the true arm with its tracking error is simulated along it only
 * when armour_episode_track (below, after armour_track) turns that on.
 *
 * armour_episode_begin checks every world with armour_check_world (its q_des is ignored; goals must be
 * finite and within ARMOUR_MAX_ABS_ANGLE; lookahead > 0, goal_radius >= 0, 2 <= check_samples <=
 * 65535), uploads the worlds as armour_plan_batch_mixed does (any mix of obstacle counts, zero
 * included) and writes each world's first waypoint on the device. A world already inside the goal
 * radius starts with status 1; a world with a non-zero qd0 or qdd0 starts in mode 1 with nothing
 * pending. Not available on an ARMTD planner or with the fp32 study: ARMOUR_E_ARG. No batch has been
 * planned yet: the getters and armour_check_motion return ARMOUR_E_STATE until the first step.
 *
 * armour_episode_step, in order:
 *  (a) The pending state becomes the batch input and the batch is planned with the code of
 *      armour_plan_batch_mixed on the resident arrays (no world upload): results [W] and timing are
 *      exactly what armour_plan_batch_mixed returns for the states armour_episode_get showed before the
 *      step. Every world is planned, frozen ones included.
 *  (b) Each running world (status 0) executes
 *        its new plan on [0, ARMOUR_T_PLAN]            if the plan is feasible and reject[w] == 0
 *                                                      (failed_streak = 0);
 *        else (failed_plans and failed_streak count up)
 *        the pending trajectory on [ARMOUR_T_PLAN, 1]  if mode == 1 and a plan is pending: the world
 *                                                      then sits at rest at q0' + k' k_range with
 *                                                      qd = qdd = 0 exactly, mode 0;
 *        nothing (it stays at rest)                    if mode == 0;
 *        and gets status 3                             if mode == 1 with nothing pending (a first plan
 *                                                      from a moving start failed).
 *      reject (optional, [W]) is the caller's veto: a missed deadline, or a check of its own.
 *  (c) armour_check_motion's kernel runs over the executed segment with check_samples samples. The
 *      running clearance keeps the smallest value and its first (step, link, obstacle). The next
 *      state is the segment's end and the next q_des = q + lookahead * d / ||d||, d = goal - q
 *      angle-wrapped to [-pi, pi) on continuous joints (state_lb <= -1000; d = 0: q_des = q). A
 *      clearance <= 0 gives status 2; otherwise a sample within goal_radius of the goal gives status 1
 *      (every sampled state of the segment is tested, as the reference tests every state). A next
 *      state that is not finite or lies beyond ARMOUR_MAX_ABS_ANGLE gives status 4 and keeps the old
 *      state. steps counts the steps a world executed (staying at rest included).
 * A world whose status is not 0 is frozen: still planned, never advanced, checked or counted.
 * Returns the number of worlds still running (>= 0), or a negative code. episode_ms (optional):
 * [0] check kernels, [1] choose + advance kernels, device milliseconds.
 *
 * The advanced state lives in arrays of its own until the next step's (a): between steps every
 * getter, armour_eval_constraints, armour_eval_candidates and armour_check_motion see the batch that
 * was planned. Any other reach or plan entry ends the episode: step and get then return
 * ARMOUR_E_STATE (as they do before a begin). */
#define ARMOUR_T_PLAN 0.5
typedef struct armour_episode_config {
    double lookahead;     /* 0.1 (kinova_run_100_worlds.m:57) */
    double goal_radius;   /* pi/30 */
    int check_samples;    /* >= 2 */
} armour_episode_config;
typedef struct armour_episode_state {
    double q[ARMOUR_NUM_FACTORS], qd[ARMOUR_NUM_FACTORS], qdd[ARMOUR_NUM_FACTORS];
    double q_des[ARMOUR_NUM_FACTORS]; /* what the next plan starts from, and its waypoint */
    int status;        /* 0 running, 1 goal reached, 2 collided, 3 no fail-safe, 4 left the input domain; tracked
                          episodes also: 5 input, 6 ultimate bound, 7 joint limit, 8 rollout not finite */
    int mode;          /* 0 at rest, 1 moving: the braking half of the last accepted plan is pending */
    int steps, failed_plans, failed_streak;
    double clearance;  /* smallest over every executed sample so far (+infinity: none yet) */
    int clearance_at[3];              /* its step, link, obstacle (-1: none yet) */
    double goal_distance;             /* ||angdiff(q, goal)||_2 over all 7 joints */
} armour_episode_state;
int armour_episode_begin(armour_planner* p, int num_worlds, const armour_world* worlds, const double* goals,
                         const armour_episode_config* cfg);
int armour_episode_step(armour_planner* p, const int* reject, armour_result* results, armour_timing* timing,
                        double* episode_ms);
int armour_episode_get(armour_planner* p, armour_episode_state* states);

/* Tracking rollouts: the other half of ARMOUR's guarantee. The planner bounds every trajectory whose
 * tracking error stays inside the ultimate bound (qe = eps / K, qde = 2 eps, eps = sqrt(2 V_m / M_min));
 * armour_track integrates the true arm under the reference's robust passivity controller along given
 * trajectories, for num_samples parameter samples per trajectory, on the device, and reports how far the
 * arm strayed and what torque it took. It reads only the planner's robot tables: it needs no batch,
 * touches no batch, plan or episode state (the getters return what they returned before and the next
 * plan is the one it would have been), and runs on the planner's stream.
 *
 * Inputs. Trajectory n is traj[n] = q0, qd0, qdd0, k (k normalised, |k| <= 1), the curve
 *   armour_check_motion uses (duration 1). Sample s of trajectory n has the true parameters
 *   mass_i * scale[n][s][0][i] and inertia_i * scale[n][s][1][i] per link i < num_joints
 *   (scale [N][S][2][num_joints]; null: all 1). The start is q(t0) = q_des(t0) + err0[n][s][0],
 *   qd(t0) = qd_des(t0) + err0[n][s][1] (err0 [N][S][2][7]; null: zero).
 * Point RNEA R(q, qd, qa, qdda; params, gravity on/off, damping on/off): the recursion of
 *   KPR/Dynamics.cu:83-181 at a point. Reversed axes and fixed joints (axis 0) as in the robot tables
 *   above. The generalised torque is the moment along the signed axis, plus armature * qdda, plus
 *   damping * qd. friction[] is not modelled, as in the planner's RNEA.
 * Its radius for mass in m (1 +- dm) and every inertia entry in I_jk (1 +- dI), dm = mass_uncertainty,
 *   dI = inertia_uncertainty: the midpoint-radius form of the reference's interval RNEA (rnea.cpp
 *   passRNEA_Int, robot_models.cpp:222-232) with point kinematics. With |a| (x) |b| the "absolute
 *   cross" (|a_y||b_z| + |a_z||b_y|, ...):
 *     rad F_i = dm |m_i| |a_ci|,   rad N_i = dI (|I_i||wd| + |wa| (x) (|I_i||w|)),
 *     backward: rad f_i = |R_{i+1}| rad f_{i+1} + rad F_i,
 *               rad n_i = rad N_i + |R_{i+1}| rad n_{i+1} + |c_i| (x) rad F_i + |p_{i+1}| (x) (|R_{i+1}| rad f_{i+1}),
 *     rho_i = rad n_i . |axis_i|.   Armature and damping carry no uncertainty.
 * Controller at (t, q, qd) (robust_controller.cpp:63-168, ARMOUR method, r_norm_threshold = 0):
 *   e = q_des - q, wrapped to [-pi, pi) on continuous joints (state_lb <= -1000) by one remainder;
 *   de = qd_des - qd; qa_d = qd_des + K e; qa_dd = qdd_des + K de; r = de + K e;
 *   tau = R(q, qd, qa_d, qa_dd; nominal) with radius rho;
 *   Mr = R(q, 0, 0, r; nominal, no gravity, no damping) with radius rMr;
 *   V_sup = 0.5 (r . Mr + |r| . rMr); h = V_m - V_sup;
 *   if ||r|| > 0: lambda = max(0, -alpha h / ||r|| + ||rho||) and u = tau + lambda r / ||r||; otherwise
 *   u = tau. Norms are sums in index order.
 * Plant. Column j of M is R(q, 0, 0, e_j; true, no gravity, no damping) (with the armature, as the
 *   reference's agent adds its transmission inertia); b = R(q, qd, qd, 0; true);
 *   qdd = M^-1 (u - b) by an unpivoted Cholesky in a fixed order; the true V = 0.5 r' M r.
 * Integration. Classical RK4 with `steps` equal steps h = (t1 - t0) / steps, step s starting at
 *   t0 + s h. The trip count is fixed; no loop's length depends on data.
 * Recording, at the first stage of every step and once more at t1 (steps + 1 samples): per joint
 *   max |q - q_des|, max |qd - qd_des|, max |u|; per rollout max V (true) and max lambda; and the end
 *   state q(t1), qd(t1).
 * Status. 0 for a clean rollout; 1 when a state or a pivot stopped being finite or positive: from then
 *   on the rollout only carries its last finite values, and nothing is stored out of range.
 *
 * The scheme is fixed-step and the robust term has the gain lambda / ||r||: an arm with little or no
 * armature (the Fetch tables) needs many more steps than the Kinova; max_robust
 * and status are how a caller sees that a rollout chattered.
 *
 * ARMOUR_E_ARG, naming the field and before any device work, for a null p, traj or out; num_traj < 1
 * or num_samples < 1 (or more than ARMOUR_TRACK_MAX_ROLLOUTS rollouts); a value that is not finite;
 * |k| > 1; |q0| > ARMOUR_MAX_ABS_ANGLE; a scale <= 0; steps < 1 or > ARMOUR_TRACK_MAX_STEPS;
 * !(0 <= t0 < t1 <= 1); an ARMTD planner, or the fp32 study (ARMOUR_EVAL_F32). Device buffers are
 * sized by num_traj * num_samples and grown on demand on the handle. Two kernels compute the same
 * bits: one rollout per 16 lanes (the default) and one per thread (ARMOUR_TRACK_KERNEL=serial). */
#define ARMOUR_TRACK_MAX_STEPS 100000
#define ARMOUR_TRACK_MAX_ROLLOUTS 16777216
typedef struct armour_track_output {   /* every pointer optional (null: skipped) */
    double* max_pos_err;  /* [N][S][7] */
    double* max_vel_err;  /* [N][S][7] */
    double* max_torque;   /* [N][S][7] */
    double* max_V;        /* [N][S] */
    double* max_robust;   /* [N][S] largest lambda */
    double* end_state;    /* [N][S][2][7] q(t1), qd(t1): err0 of a following window is end_state - desired */
    int* status;          /* [N][S] */
    double track_ms;      /* device time of the rollouts */
} armour_track_output;
int armour_track(armour_planner* p, int num_traj, const double* traj, int num_samples, const double* scale,
                 const double* err0, double t0, double t1, int steps, armour_track_output* out);

/* Rollouts with a record, and the true arm's clearance: armour_track and armour_check_motion joined on
 * the device. armour_track_motion rolls num_samples true arms per world of the last batch along that
 * world's trajectory and tests the states the arms actually took, not the desired curve, against the
 * world's own obstacles. It is defined for the worlds of the last batch (uniform or mixed, after any
 * reach or plan entry), as armour_check_motion is; ARMOUR_E_STATE before any batch. It touches no plan
 * or episode state.
 *
 * Rollouts. Everything is as armour_track defines it with num_traj = W (traj [W][4][7], scale
 *   [W][S][2][num_joints] or null, err0 [W][S][2][7] or null, the window, steps), with one addition:
 * Check points. check_samples (2 ..) must satisfy steps % (check_samples - 1) == 0. With
 *   stride = steps / (check_samples - 1), check point c is the rollout's state (q, qd) at the first stage
 *   of step c * stride; the last check point is the state at t1. A rollout that stopped being finite
 *   records the state it keeps.
 * Same rollouts. The maxima, the end state and the status (out->track, every pointer optional) are bit
 *   for bit those armour_track returns for the same inputs: the record only reads the state.
 * True-arm clearance. At each check point the link boxes come from the point forward kinematics of
 *   armour_check_motion at the recorded q, and are tested against the world's own obstacles with the
 *   same 15 axes, skip rule and -1e8 convention.
 *   clearance [W][S], where [W][S][3]   per rollout: the minimum over (check point, link, obstacle) and
 *                                       its first minimiser in that order
 *   world_clearance [W], world_where [W][4]   per world: the minimum over its samples, ties to the lowest
 *                                       sample, as (sample, check point, link, obstacle)
 *   A world without obstacles gets +infinity and -1s.
 * Flags per rollout (flags [W][S]), a bit mask with the reference's strict comparisons
 *   (uarmtd_agent.m:592-664, uarmtd_robust_CBF_LLC.m:192-219):
 *   ARMOUR_TRACK_COLLISION   clearance <= 0
 *   ARMOUR_TRACK_INPUT       some max_torque[j] > torque_limits[j]. The maximum runs over every recorded
 *                            stage (steps + 1 of them), which is finer than the reference's sampling of
 *                            the input: a flag here can precede the reference's.
 *   ARMOUR_TRACK_BOUND       some max_pos_err[j] > qe or max_vel_err[j] > qde, with qe = eps / K and
 *                            qde = 2 eps of the planner's robot tables (eps = sqrt(2 V_m / M_min))
 *   ARMOUR_TRACK_LIMIT       at a check point q[j] < state_lb[j], q[j] > state_ub[j] or
 *                            |qd[j]| > speed_limits[j]
 *   ARMOUR_TRACK_NOT_FINITE  rollout status 1
 * check_ms: device time of the check and finish kernels; track.track_ms: that of the rollouts.
 *
 * ARMOUR_E_ARG as armour_track (num_traj being the batch's world count), and for num_samples > 65535,
 * check_samples < 2 or steps % (check_samples - 1) != 0, naming the field and before any device work. */
#define ARMOUR_TRACK_COLLISION 1
#define ARMOUR_TRACK_INPUT 2
#define ARMOUR_TRACK_BOUND 4
#define ARMOUR_TRACK_LIMIT 8
#define ARMOUR_TRACK_NOT_FINITE 16
typedef struct armour_track_motion_output {   /* every pointer optional (null: skipped) */
    armour_track_output track;  /* the rollouts, [W][S] */
    double* clearance;          /* [W][S] */
    int* where;                 /* [W][S][3] check point, link, obstacle */
    int* flags;                 /* [W][S] */
    double* world_clearance;    /* [W] */
    int* world_where;           /* [W][4] sample, check point, link, obstacle */
    double check_ms;            /* device time of the true-arm check */
} armour_track_motion_output;
int armour_track_motion(armour_planner* p, const double* traj, int num_samples, const double* scale, const double* err0,
                        double t0, double t1, int steps, int check_samples, armour_track_motion_output* out);

/* Tracked episodes: the true arm run through each executed segment (simulator_armtd.m:189-271 with
 * uarmtd_agent.m:469; its four checks on the true states and inputs: input_check, ultimate_bound_check,
 * joint_limit_check and collision_check, of which the reference stops on the first, second and fourth).
 * armour_episode_track is called after armour_episode_begin and before the first step; from then on step
 * (c) of armour_episode_step also rolls num_worlds x num_samples true arms, as armour_track_motion
 * defines them, along what each running world executes, with the episode's check_samples check points
 * (steps % (check_samples - 1) == 0).
 *   What each rollout follows: the new plan on [0, ARMOUR_T_PLAN]; the pending plan on
 *     [ARMOUR_T_PLAN, 1]; for a world that stays at rest the constant trajectory (q, 0, 0, k = 0) on
 *     [0, ARMOUR_T_PLAN]: the controller holds the arm, and its error keeps evolving.
 *   Where it starts: from the true state (q, qd) the previous step left, an absolute state, not an
 *     offset; at the first step from the episode's start state plus err0 (null: zero).
 *   Windows. Each world's trajectory carries its own window; an empty window (t0 > t1) means its rollouts
 *     are skipped: their states and outputs stay as they were. Frozen worlds are skipped.
 *   Planning is unaffected: it still starts from the desired state, as the reference's planner does
 *     (uarmtd_planner.m:91-93); results and armour_episode_state's trajectory fields are bit for bit those
 *     of an untracked episode until a stop below. Tracking feeds back only through these stops.
 *   A record per world accumulates over steps and samples (armour_episode_tracked): the smallest true
 *     clearance with its step, sample, link and obstacle; the per-joint maxima of position error, velocity
 *     error and torque; the largest V and lambda; the OR of the flags and the first step of each flag.
 *   Status. The existing rules come first: 4, then 2 for the desired arm. After them, in this order: a
 *     true clearance <= 0 gives 2; NOT_FINITE gives 8; INPUT gives 5 if stop_on_input; BOUND gives 6 if
 *     stop_on_bound; LIMIT gives 7 if stop_on_limit; then the goal test as before (on the desired samples).
 * ARMOUR_E_STATE without an episode or after its first step; ARMOUR_E_ARG for a null argument,
 * num_samples < 1 (or > 65535, or more than ARMOUR_TRACK_MAX_ROLLOUTS rollouts), steps outside
 * 1 .. ARMOUR_TRACK_MAX_STEPS or no multiple of check_samples - 1, a scale that is not finite or not
 * positive, an err0 that is not finite. A new armour_episode_begin ends the tracking.
 *
 * armour_episode_get_tracked: records [W]; true_state [W][S][2][7] (optional) the true arms' states now;
 * flags [W][S] (optional) of the last step each world executed; ms [2] (optional) the device time of the
 * last step's rollouts and of its true-arm check. ARMOUR_E_STATE when there is no episode or tracking is
 * not enabled. */
typedef struct armour_episode_track_config {
    int num_samples;
    const double* scale;   /* [W][S][2][num_joints] or null: nominal */
    const double* err0;    /* [W][S][2][7] or null: zero */
    int steps;             /* RK4 steps per executed segment */
    int stop_on_input, stop_on_bound, stop_on_limit;   /* the reference: 1, 1, 0 (simulator_armtd.m:14-16) */
} armour_episode_track_config;
typedef struct armour_episode_tracked {
    double clearance;      /* smallest true clearance so far (+infinity: none yet) */
    int clearance_at[4];   /* its step, sample, link, obstacle (-1: none yet) */
    double max_pos_err[ARMOUR_NUM_FACTORS], max_vel_err[ARMOUR_NUM_FACTORS], max_torque[ARMOUR_NUM_FACTORS];
    double max_V, max_robust;
    int flags;             /* the OR of every rollout's flags so far */
    int flag_step[5];      /* first step of COLLISION, INPUT, BOUND, LIMIT, NOT_FINITE (-1: never) */
} armour_episode_tracked;
int armour_episode_track(armour_planner* p, const armour_episode_track_config* cfg);
int armour_episode_get_tracked(armour_planner* p, armour_episode_tracked* records, double* true_state, int* flags,
                               double* ms);

/* The roadmap high-level planner: a joint-space graph per world and the waypoint taken from it, on the
 * device. The shape of simulator/planners/high_level_planners/robot_arm_sampling_based_HLP.m (nodes in
 * joint space, a collision check per node, a neighbour graph, the shortest path, the waypoint at the
 * lookahead distance along its polyline; robot_arm_PRM_HLP.m is the neighbour-radius variant). The
 * reference's PRM checks nodes only; here every edge is sampled and checked as well, a deliberate
 * strengthening. The caller supplies the nodes (how to sample them is host policy); the library does the
 * checking, the graph and the waypoint. Without these calls every episode, plan and getter is bit for bit
 * what it is without them.
 *
 * Conventions. Joint j is continuous when state_lb[j] <= -1000 (the straight-line waypoint's rule).
 *   Delta(a->b)_j = b_j - a_j, wrapped to [-pi, pi) on continuous joints; d(a, b) = sqrt(sum_j Delta_j^2),
 *   summed in joint order 0..6; the point at fraction s of the segment is a + s Delta(a->b).
 *   clr(q) is the clearance of a configuration: the minimum over (link, obstacle) of the separation of
 *   armour_check_motion, link boxes from its point forward kinematics, the world's own obstacles: exactly
 *   what armour_check_motion returns for the constant trajectory (q, 0, 0, k = 0) at t0 = 0 with
 *   samples = 1. A world without obstacles: +infinity.
 * Vertices. Each world has N caller nodes, nodes [W][N][7], index 0 .. N - 1; the library appends the
 *   world's goal as vertex N. 2 <= N <= ARMOUR_ROADMAP_MAX_NODES (1024 vertices: a world's adjacency
 *   matrix is 1024 x 1024 bits). free[i] = clr(v_i) > margin.
 * Edge (i, j), i < j: a candidate when both vertices are free and ARMOUR_ROADMAP_MIN_EDGE <= d(v_i, v_j)
 *   <= connect_radius. It has n = ceil(d / edge_step) pieces and the interior samples
 *   v_i + (s / n) Delta(v_i->v_j), s = 1 .. n - 1, always from the lower index to the higher. The edge
 *   exists when every interior sample has clr > margin; its weight is d(v_i, v_j), lower index first.
 * Cost-to-go. togo[N] = 0 when the goal is free; otherwise togo[i] = min_j fl(d(i, j) + togo[j]) over the
 *   existing edges of i, +infinity when the goal cannot be reached or i is not free (a goal that is not
 *   free: every togo is +infinity). next[i] is the lowest j that attains the minimum, next[N] = N,
 *   unreachable vertices get -1. Floating-point addition is monotone, so the fixed point reached from
 *   +infinity does not depend on the relaxation schedule and a Dijkstra with the same additions finds it.
 *   With connect_radius <= 100 and the minimum edge length togo strictly decreases along next.
 * Waypoint at q. Entry candidates are the free vertices i with finite togo[i] and d(q, v_i) <=
 *   connect_radius whose segment q -> v_i is free: ceil(d / edge_step) pieces, every interior sample with
 *   clr > margin (q itself is not tested; d = 0 has no samples). entry = argmin fl(d(q, v_i) + togo[i]),
 *   ties to the lowest i. No candidate: entry = -1, path_left = +infinity and q_des is the straight-line
 *   waypoint of the episodes, bit for bit. Otherwise walk q -> entry -> next -> ... -> goal with
 *   r = lookahead from pos = q: on a leg a -> b of length d, r > d: pos += Delta(a->b), r -= d; else
 *   pos += (r / d) Delta(a->b) and stop (at most N + 1 legs). At the goal the walk stops (the reference
 *   clamps there too) and q_des is its position: q plus the legs' Deltas. path_left = fl(d(q, entry) +
 *   togo[entry]).
 *
 * armour_roadmap_build serves the worlds of the last batch, uniform or mixed, after any reach or plan
 * entry (ARMOUR_E_STATE before any batch, as armour_check_motion), with goals [W][7]. It touches no plan
 * or episode state. stats (optional): vertex and edge totals over the worlds, the largest number of
 * relaxation rounds that changed a value, and the device milliseconds of [0] the vertex pass, [1] the
 * candidate passes, [2] the edge samples and their fold, [3] the cost-to-go. Another batch entry
 * invalidates the roadmap: armour_roadmap_get and armour_roadmap_waypoint then return ARMOUR_E_STATE.
 * armour_roadmap_get: world w's arrays, all optional: node_clearance, is_free, togo, next [N + 1];
 * adjacency [N + 1][32] 32-bit words, bit j of row i set for an existing edge, in both directions.
 * armour_roadmap_waypoint: q [W][7] (finite, within ARMOUR_MAX_ABS_ANGLE), lookahead > 0; q_des [W][7],
 * entry [W], path_left [W] (each optional).
 * armour_episode_roadmap is called after armour_episode_begin and before the first step, in either order
 * with armour_episode_track: it builds the roadmap from the episode's obstacles and goals, rewrites the
 * q_des of every running world with the roadmap waypoint at its q, and from then on step (c) takes the
 * next waypoint from the roadmap (episode_ms[1] includes it). Frozen worlds are untouched. A new
 * armour_episode_begin ends it. armour_episode_state keeps its layout; armour_episode_get_roadmap gives
 * the entry and the path left of each world's last waypoint (-1 and +infinity: the straight line, or a
 * world that was frozen from the start). While an episode uses a roadmap, armour_roadmap_build returns
 * ARMOUR_E_STATE.
 *
 * ARMOUR_E_ARG, naming the field and before any device work: a null pointer; num_nodes out of range;
 * connect_radius, edge_step or margin not finite; connect_radius outside (0, 100]; edge_step <= 0;
 * connect_radius / edge_step > 4096; margin < 0; a node or goal that is not finite or lies beyond
 * ARMOUR_MAX_ABS_ANGLE; an ARMTD planner; the fp32 study (ARMOUR_EVAL_F32). A build whose candidate edges
 * or edge samples exceed 2^31 - 1 is ARMOUR_E_CAPACITY, a failed allocation ARMOUR_E_HIP: in both cases
 * the previous roadmap, if any, is gone and nothing else has changed. */
#define ARMOUR_ROADMAP_MAX_NODES 1023
#define ARMOUR_ROADMAP_MIN_EDGE 1e-6
typedef struct armour_roadmap_config {
    int num_nodes;
    double connect_radius, edge_step, margin;
} armour_roadmap_config;
typedef struct armour_roadmap_stats {
    long long free_nodes, candidate_edges, edges, edge_samples, reachable;
    int relax_rounds_max;
    double build_ms[4];
} armour_roadmap_stats;
int armour_roadmap_build(armour_planner* p, const armour_roadmap_config* cfg, const double* nodes, const double* goals,
                         armour_roadmap_stats* stats);
int armour_roadmap_get(armour_planner* p, int w, double* node_clearance, int* is_free, unsigned* adjacency, double* togo,
                       int* next);
int armour_roadmap_waypoint(armour_planner* p, const double* q, double lookahead, double* q_des, int* entry,
                            double* path_left);
int armour_episode_roadmap(armour_planner* p, const armour_roadmap_config* cfg, const double* nodes);
int armour_episode_get_roadmap(armour_planner* p, int* entry, double* path_left);

/* Outputs of world w of the last batch (the armour_*.out payloads, armour_main.cu:340-398) */
int armour_get_constraints(armour_planner* p, int w, double* g);              /* m values at k_opt (m_w of world w) */
int armour_get_link_centers(armour_planner* p, int w, double* centers);       /* [T][NJ][3] sliced at the
                                                                               last evaluated point: k_opt after a plan,
                                                                               x after armour_eval_constraints (which
                                                                               evaluates every world of the batch at x);
                                                                               ARMOUR_E_STATE before either */
int armour_get_link_generators(armour_planner* p, int w, double* gens);       /* [T][NJ][3][6] */
int armour_get_torque_radius(armour_planner* p, int w, double* radius);       /* [T][7] */
int armour_num_joints(const armour_planner* p);
/* k-only monomials of world w's link PZs [T][NJ] and torque PZs [T][7] after reduce_link_PZ /
 * reduce (the M_links, M_tau of SURVEY.md §8(d)'s per-plan byte count); either may be null */
int armour_get_monomial_counts(armour_planner* p, int w, int* link_counts, int* torque_counts);
/* the 28 trailing values of armour_constraints.out (armour_main.cu:385-396): per joint
 * [lb + qe, ub - qe] then per joint [-v + qde, v - qde] */
int armour_get_joint_bounds(const armour_planner* p, double* bounds28);

/* Diagnostics (no reference counterpart). The reach kernel interprets a fixed op program built
 * from the robot tables; these expose it for profiling. armour_get_reach_program writes the op
 * codes (if capacity >= count) and returns the op count. armour_get_reach_profile writes
 * [cycles, terms] per op accumulated over all jobs when the environment variable
 * ARMOUR_PROFILE_OPS was set at armour_create, followed by 16 phase counters of the operator
 * paths (capacity counts pairs: >= op count + 8), and returns the op count. */
int armour_get_reach_program(const armour_planner* p, int* codes, int capacity);
/* Capacity headroom of the last reach (bundle engine): for k < n writes the largest use over the
 * batch and its capacity: [0] arena union hashes, [1] arena coefficient rows, [2] terms of one
 * operator (sort keys), [3] k-only monomials of a link PZ (reduce_link_PZ output), [4] k-only
 * monomials of a torque PZ, [5] worlds retried with 4x buffers (cap: W), [6] worlds that still
 * failed (cap: W). Returns ARMOUR_OCC_COUNT. */
#define ARMOUR_OCC_COUNT 7
int armour_get_reach_occupancy(armour_planner* p, long long* used, long long* caps, int n);
int armour_get_reach_profile(armour_planner* p, unsigned long long* cycles_terms, int capacity);
/* Path census: which kernels and loop forms the host chose, counted where it chooses (a setting alone
 * does not decide: batch size, capacities found by the last reach, the plane cache and the CU count do
 * too). armour_get_path_counts writes the first n counters (k < n, k < ARMOUR_PATH_COUNT) and returns
 * ARMOUR_PATH_COUNT; armour_path_name(i) is counter i's name (null outside 0 .. ARMOUR_PATH_COUNT - 1).
 * The counters are cumulative since the planner was created, host integers only (no device read, no
 * synchronisation), and belong to the handle (one handle per thread). In index order:
 *   batches           batch_uniform, batch_mixed (uploads; a mixed batch runs the _mx instantiation of every
 *                     solver, candidate and plane-cache kernel, a uniform or ARMTD batch the plain one; an
 *                     episode's batch is mixed)
 *   reach launches    reach_job_256, reach_job_128 (per-job engine, 256 / 128 threads), reach_lane_wide,
 *                     reach_lane_dense (bundle engine shapes, a retry included), reach_retry (capacity-retry
 *                     launches), reach_sq, reach_sqrt (squared-norm / sqrt kernels), reach_cu_masked (launches
 *                     on a CU-masked reach stream, ARMOUR_REACH_CU_RESERVE)
 *   evaluations       eval_small (eval_kernel_small), eval_f64, eval_f32 (eval_kernel_t), eval_armtd_f64,
 *                     eval_armtd_f32 (its ARMTD instantiations), eval_mx (eval_kernel_mx); and of all of
 *                     them: eval_cached (read the plane cache), eval_full_scan (the 36-plane scan)
 *   trial values      trials_small (eval_trials_small), trials_full (eval_trials_kernel), trials_all
 *                     (eval_trials_all)
 *   row pass DA       da_lds (ipm_rows_DA_lds), da_regs (ipm_rows_DA), per iteration after a loop's first
 *   iterations        ipm_iter_sync (synchronised), ipm_iter_tail (sync-free tail)
 *   line search       ls_sequential (rounds after round 0, one by one), ls_speculative (one round over the
 *                     remaining K trials), ls_one_round (the tail's one round over all trials)
 *   restoration       phase iterations: resto_inline (inside the interior-point loop), resto_after_loop;
 *                     resto_one_round, resto_rounds (the search's form); resto_second_stream (queued beside
 *                     an interior-point iteration), resto_solver_stream
 *   restarts          ipm_restarts (worlds the host collected to restart the interior point)
 *   solves            solve_monotone, solve_adaptive (the barrier strategy: 0, 1 of armour_solver_options)
 *   plane cache       pc_builds (first builds), pc_regrows (builds repeated on a larger pool), pc_fallbacks
 *                     (builds that left the solve on the full scan)
 *   candidates        cand_small, cand_full (calls by kernel), cand_chunks (candidate chunks, summed)
 *   motion check      motion_chunks (sample blocks per world, summed over calls and episode steps)
 *   tracking          track_row, track_row_rec, track_row_episode, track_serial, track_serial_rec,
 *                     track_serial_episode (launches of the plain, recording and episode kernels)
 *   solver options    solve_quality (solves under barrier strategy 2 or 3), qf_sigma (launches of the
 *                     quality function's sigma search, one per interior-point iteration of such a solve),
 *                     hess_lbfgs (solves with the limited-memory BFGS); all zero on the default dispatch */
#define ARMOUR_PATH_COUNT 53
int armour_get_path_counts(armour_planner* p, long long* counts, int n);
const char* armour_path_name(int i);
/* The interior-point solver's configuration. The default is (1, 16, 0). The reference
 * configures Ipopt with mu_strategy adaptive and hessian_approximation limited-memory
 * (KPR/armour_main.cu:256-261), which with Ipopt's defaults is (2, -, 6); its sigma search is a golden
 * section, here a fixed logarithmic grid of qf_grid points over [1e-6, 100].
 * armour_set_solver_options takes effect from the next plan entry, on any planner (ARMTD included). It
 * touches no batch state: the getters return what they returned before. ARMOUR_E_ARG, naming the field,
 * for a value out of range, and for anything but strategies 0, 1 with lbfgs_history 0 under the fp32
 * study (ARMOUR_EVAL_F32); ARMOUR_E_STATE while an episode is active. A planner is created with the
 * configuration the environment names (ARMOUR_MU_STRATEGY = monotone | quality | quality-floor,
 * ARMOUR_QF_GRID, ARMOUR_LBFGS), checked the same way. The options change plans. */
typedef struct armour_solver_options {
    int mu_strategy;    /* 0 monotone; 1 adaptive, LOQO / kkt-error, floor tol/10, mu grid (default);
                           2 Ipopt's default adaptive pair: quality-function oracle + obj-constr-filter
                             globalisation, mu_min 1e-11 (with lbfgs_history 6: the reference's configuration);
                           3 the pair with the product's floor tol/10 and 2^(1/8) mu grid */
    int qf_grid;        /* sigma candidates of the quality function, 2..32, default 16 (strategies 2, 3) */
    int lbfgs_history;  /* 0 damped full BFGS (default); 1..6 Ipopt's limited-memory BFGS */
} armour_solver_options;
int armour_get_solver_options(const armour_planner* p, armour_solver_options* options);
int armour_set_solver_options(armour_planner* p, const armour_solver_options* options);
/* Certified plane cache of the current reach sets, built on demand: for k < n
 * writes [0] planes kept over all (world, t, link, obstacle) pairs, [1] pairs, [2] (world, t) blocks
 * whose cache region held every kept plane, [3] blocks, [4] most planes kept for one pair,
 * [5] records in the cache pool, [6] evaluations that found a point outside the cache's box (rows
 * NaN; the solver never produces one). Returns ARMOUR_PC_COUNT; ARMOUR_E_STATE when the cache is off.
 * After a mixed batch [0], [1] and [4] count only the pairs that exist (NJ * O_w per block of world w). */
#define ARMOUR_PC_COUNT 7
int armour_get_plane_cache_stats(armour_planner* p, long long* out, int n);
/* Execution span of the last batch's first reach launch on the device clock (wall_clock64): from
 * the first workgroup's start to the last workgroup's end, the duration rocprofv3 --kernel-trace
 * reports for the kernel (the reach_kernel_ms of armour_timing, HIP events around the launch, also
 * counts the time the launch waits for CUs held by other planners' kernels). Milliseconds. When a
 * capacity retry ran (occupancy [5] > 0), the span is still the first launch's, the one over the whole
 * batch, as reach_kernel_ms and the occupancy are; the retry's own launch is not included. */
int armour_get_reach_span(armour_planner* p, double* span_ms);
/* op-by-op state of job 0 (world 0, t = 0) of the last reach: per op 8 doubles [monomial count,
 * block size, centre[0..2], nominal ind[0], interval ind[0], sum|m|[0]] of the op's output, when
 * ARMOUR_DUMP_OPS was set at armour_create; returns the op count. */
int armour_get_reach_dump(armour_planner* p, double* dump, int capacity);
/* Self-check of the keep / prune decision on squared norms. The reach kernels
 * decide sqrt(S) > thr as S > S*, with S* the largest double whose square root is <= thr, found and
 * verified on the device when a planner is created. This runs the same search for `thr` on `device`
 * and counts, on the device, how often the two forms decide differently (as f > thr and as
 * !(f <= thr), one count each) over the doubles within half_width ulps of S* and over the n values
 * (n may be 0). Writes S*, whether the device verified it (0: a planner with this threshold runs
 * the sqrt kernels, as ARMOUR_SQ_THRESHOLD=0 forces) and the count, which is 0 on a sound device. */
int armour_sq_selfcheck(int device, double thr, long long half_width, const double* values, long long n,
                        double* s_star, int* valid, long long* mismatches);

#ifdef __cplusplus
}
#endif
#endif
