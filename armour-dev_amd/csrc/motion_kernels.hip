// armour-mi355x — executing a plan: the sampled execution check (armour_check_motion) and the
// receding-horizon episode state that stays on the device (armour_episode_*), include/armour_hip.h.
//
// Nothing here reads a reach set. A trajectory is the degree-5 Bezier curve of KPR/Trajectory.cu:542-599
// (control points q0, q0 + qd0 / 5, q0 + 2 qd0 / 5 + qdd0 / 20, then three times q0 + k k_range;
// DURATION = 1); at a sampled time the link boxes come from point forward kinematics
// (KPR/Dynamics.cu:69-81 at a point: p += R trans_i, R = R (RPY_i Rot_axis_i(q_i)), box centre
// p + R link_c, generators the columns of R diag(link_g)), and every (link, obstacle) pair is tested
// on the 15 axes that are the normalised cross products of the 6 generators (obstacle 3, link 3), a
// pair of norm exactly 0 skipped (KPR/CollisionChecking.cu:261-282):
//     separation = max_n (|n . (c - c_obs)| - sum_j |n . G_j|)
// > 0: the two sets are disjoint (a lower bound of their distance); <= 0: they intersect.
//
// motion_check_kernel   grid (sample, world), 256 threads: the world's obstacles and the FK chain of
//                       the sample go to LDS once per block, the threads run over the (link, obstacle)
//                       pairs, the minimum is taken per wave (wave.h), and thread 0 stores the block's
//                       (value, pair) with one plain store. No atomics.
// motion_finish_kernel  one wave per world: first minimum over the samples, in (sample, link, obstacle) order.
// motion_state_check_kernel   the same block body on recorded states of the true arm instead of a curve
//                       (armour_track_motion): grid (check point, sample, world).
// motion_state_finish_kernel  one wave per world: per rollout the first minimum over the check points and
//                       the flags, then the first minimum over the world's samples.
// episode_*_kernel      one thread per world: the bookkeeping of armour_episode_begin / _step.
// episode_track_*_kernel  one thread per world: a tracked episode's trajectory and window (choose) and its
//                       record and stops (fold), armour_episode_track.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>

#include "../../include/armour_hip.h"
#include "common.h"
#include "track.h"
#include "traj.h"
#include "wave.h"

namespace armour {

constexpr int MOTION_THREADS = 256;
constexpr int MOTION_WAVES = MOTION_THREADS / 64;
constexpr double MOTION_SKIPPED = -1e8;  // a pair with no plane at all (CollisionChecking.cu:261-282)

struct MotionArgs {
    const RobotParams* rp;
    int W, S;               // worlds, samples per world
    int O;                  // obstacle stride of the resident obstacle array (the batch's largest count)
    const int* Ow;          // [W] own counts of a mixed batch; null: every world carries O
    const double* obs;      // [W][O][12]
    const double* traj;     // [W][4][NF]
    const double* win;      // [W][2] per-world window (t0 > t1 or NaN: the world is not checked); null: t0, t1
    double t0, t1;
    double* pval;           // [W][S] smallest separation of each sample
    int* pidx;              // [W][S] its first pair l * O_w + o (-1: none)
};

// sample s of S evenly spaced times in [t0, t1], ends included (S = 1: t0)
AD double motion_time(double t0, double t1, int s, int S) {
    if (S <= 1 || s == 0) return t0;
    if (s == S - 1) return t1;
    return s * ((t1 - t0) / (S - 1)) + t0;
}

AD void mat3_mul(const double* A, const double* B, double* C) {  // row-major C = A B
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

// separation of the link box (centre lc, generators lg[3][3]) from the obstacle zonotope ob[12]
// (inlined into each of the two check kernels, as it was into the one)
__device__ __forceinline__ double motion_separation(const double* ob, const double* link) {
    double g[6][3], diff[3];
    for (int e = 0; e < 3; e++) diff[e] = link[e] - ob[e];
    for (int j = 0; j < 3; j++)
        for (int e = 0; e < 3; e++) {
            g[j][e] = ob[3 + 3 * j + e];
            g[3 + j][e] = link[3 + 3 * j + e];
        }
    double top = MOTION_SKIPPED;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a + 1; b < 6; b++) {
            const double x = g[a][1] * g[b][2] - g[a][2] * g[b][1];
            const double y = g[a][2] * g[b][0] - g[a][0] * g[b][2];
            const double z = g[a][0] * g[b][1] - g[a][1] * g[b][0];
            const double nrm = sqrt(x * x + y * y + z * z);
            if (nrm > 0) {
                const double n0 = x / nrm, n1 = y / nrm, n2 = z / nrm;
                const double proj = n0 * diff[0] + n1 * diff[1] + n2 * diff[2];
                double delta = 0.0;
#pragma unroll
                for (int j = 0; j < 6; j++) delta += fabs(n0 * g[j][0] + n1 * g[j][1] + n2 * g[j][2]);
                top = fmax(top, fabs(proj) - delta);
            }
        }
    return top;
}

// one joint of the point forward kinematics: p += R trans_i, R = R (RPY_i Rot_axis_i(q_i)) with
// cs = (cos q_j, sin q_j) pairs, and link i's box L[12] (centre, then the three generators). The block
// check runs it on one thread, the roadmap's point check (roadmap_kernels.hip) on every lane.
__device__ __forceinline__ void motion_link_box(const RobotParams& rp, int i, const double* cs, double* R, double* p, double* L) {
    const double* tr = rp.trans + 3 * i;
    for (int r = 0; r < 3; r++) p[r] += R[3 * r] * tr[0] + R[3 * r + 1] * tr[1] + R[3 * r + 2] * tr[2];
    double Ri[9], Rn[9];
    track_joint_rot(rp, i, cs, Ri);
    mat3_mul(R, Ri, Rn);
    for (int e = 0; e < 9; e++) R[e] = Rn[e];
    for (int r = 0; r < 3; r++)
        L[r] = p[r] + (R[3 * r] * rp.link_c[i][0] + R[3 * r + 1] * rp.link_c[i][1] + R[3 * r + 2] * rp.link_c[i][2]);
    for (int j = 0; j < 3; j++)
        for (int r = 0; r < 3; r++) L[3 + 3 * j + r] = R[3 * r + j] * rp.link_g[i][j];
}

// (value, index) ordered by value, then by index: the first minimiser
__device__ inline bool motion_before(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }
// the wave's first minimum: every lane leaves with the winning (value, index)
WAVE_FN void motion_first_min(double& v, int& i) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double ov = xor_f64(v, m);
        const int oi = xor_i32(i, m);
        if (motion_before(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
}

// world w's obstacle count, within what a block stages
__device__ inline int motion_obstacles(const MotionArgs& a, int w) {
    const int O = a.Ow ? a.Ow[w] : a.O;
    return O < 0 ? 0 : (O > MAX_OBS ? MAX_OBS : O);
}
// the pair behind idx = link * O + obstacle; idx < 0 (none): -1, -1
struct MotionPair { int link, obs; };
__device__ inline MotionPair motion_pair(int idx, int O) {
    if (idx < 0) return {-1, -1};
    const int l = idx / O;
    return {l, idx - l * O};
}

// Where the configuration of a block comes from. MotionFromCurve: sample s of the world's Bezier curve
// over its window (armour_check_motion, the episodes). MotionFromStates: check point c of rollout
// (w, s) as the recording track kernels stored it (armour_track_motion); nothing is skipped.
struct MotionFromCurve {
    const double* tr;  // [4][NF] of this world
    double t0, t1;
    int s, S;
    __device__ bool empty() const { return !(t0 <= t1); }
    __device__ double angle(const RobotParams& rp, int j) const {
        double q, qd, qdd;
        traj_joint(rp, tr, j, motion_time(t0, t1, s, S), q, qd, qdd);
        return q;
    }
};
struct MotionFromStates {
    const double* state;  // [2][NF] of this check point and rollout
    bool skipped;         // a tracked episode's world that executes nothing this step
    __device__ bool empty() const { return skipped; }
    __device__ double angle(const RobotParams&, int j) const { return state[j]; }
};

// one block: the smallest separation of world w's obstacles from the arm at src's configuration, and
// its first (link, obstacle) pair, stored at `out`
template <class Src>
__device__ __forceinline__ void motion_check_body(const MotionArgs& a, int w, long out, const Src& src) {
    const int tid = threadIdx.x;
    __shared__ double s_obs[MAX_OBS * 12];
    __shared__ double s_cs[NF][2];
    __shared__ double s_link[MAX_J][12];
    __shared__ double s_wv[MOTION_WAVES];
    __shared__ int s_wi[MOTION_WAVES];
    const RobotParams& rp = *a.rp;
    const int NJ = rp.num_joints;
    const int O = motion_obstacles(a, w);
    // (block-uniform) a world without obstacles, or one that executes nothing
    if (O == 0 || src.empty()) {
        if (tid == 0) {
            a.pval[out] = INFINITY;
            a.pidx[out] = -1;
        }
        return;
    }
    const double* ob = a.obs + (long)w * a.O * 12;
    for (int i = tid; i < O * 12; i += MOTION_THREADS) s_obs[i] = ob[i];
    if (tid < NF) {
        const double q = src.angle(rp, tid);
        s_cs[tid][0] = cos(q);
        s_cs[tid][1] = sin(q);
    }
    __syncthreads();
    if (tid == 0) {
        // the chain is sequential: one thread, 2 x NJ 3x3 products
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
        for (int i = 0; i < NJ; i++) motion_link_box(rp, i, &s_cs[0][0], R, p, s_link[i]);
    }
    __syncthreads();
    double best = INFINITY;
    int bidx = INT_MAX;
    for (int idx = tid; idx < NJ * O; idx += MOTION_THREADS) {
        const MotionPair pr = motion_pair(idx, O);
        const double v = motion_separation(s_obs + 12 * pr.obs, s_link[pr.link]);
        if (motion_before(v, idx, best, bidx)) {
            best = v;
            bidx = idx;
        }
    }
    motion_first_min(best, bidx);
    if ((tid & 63) == 0) {
        s_wv[tid >> 6] = best;
        s_wi[tid >> 6] = bidx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < MOTION_WAVES; k++)
            if (motion_before(s_wv[k], s_wi[k], best, bidx)) {
                best = s_wv[k];
                bidx = s_wi[k];
            }
        a.pval[out] = best;
        a.pidx[out] = bidx == INT_MAX ? -1 : bidx;
    }
}

__global__ __launch_bounds__(MOTION_THREADS) void motion_check_kernel(MotionArgs a) {
    const int s = blockIdx.x, w = blockIdx.y;
    double t0 = a.t0, t1 = a.t1;
    if (a.win) {
        t0 = a.win[2 * w];
        t1 = a.win[2 * w + 1];
    }
    motion_check_body(a, w, (long)w * a.S + s, MotionFromCurve{a.traj + (long)w * TRAJ_DOUBLES, t0, t1, s, a.S});
}

// The true-arm check of armour_track_motion: grid (check point, sample, world) over the recorded states
// rec [C][W * S][2][NF]; pval / pidx are [W][S][C]. a.traj is not read; a.win (a tracked episode's step;
// null otherwise) only says which worlds are skipped: those with an empty window.
__device__ inline bool motion_world_skipped(const MotionArgs& a, int w) { return a.win && !(a.win[2 * w] <= a.win[2 * w + 1]); }
__global__ __launch_bounds__(MOTION_THREADS) void motion_state_check_kernel(MotionArgs a, const double* rec, int C) {
    const int c = blockIdx.x, s = blockIdx.y, w = blockIdx.z;
    const long r = (long)w * a.S + s, NR = (long)a.W * a.S;
    motion_check_body(a, w, r * C + c, MotionFromStates{rec + ((long)c * NR + r) * 2 * NF, motion_world_skipped(a, w)});
}

// What the true-arm check reports per rollout and per world (armour_track_motion), from the per-check-point
// minima, the recorded states and the rollouts' outputs. One wave per world, its samples in turn: the
// first minimum over the check points (lanes stride over them; wave reduction), the limit test at the
// check points, the flags, and the first minimum over the samples (a strict comparison: ties to the
// lowest sample). Trip counts depend on S and C only.
struct TrackedFinish {
    int C;
    const double* rec;      // [C][W * S][2][NF]
    const double* out;      // the rollouts' outputs by field (track_store)
    const int* status;      // [W * S]
    double* clearance;      // [W][S]
    int* where;             // [W][S][3] check point, link, obstacle
    int* flags;             // [W][S]
    double* wclear;         // [W]
    int* wwhere;            // [W][4] sample, check point, link, obstacle
};
__global__ __launch_bounds__(64) void motion_state_finish_kernel(MotionArgs a, TrackedFinish f) {
    const int w = blockIdx.x, lane = threadIdx.x;
    if (motion_world_skipped(a, w)) return;  // (block-uniform) its outputs stay as they were
    const RobotParams& rp = *a.rp;
    const long NR = (long)a.W * a.S;
    const int O = motion_obstacles(a, w);
    double wbest = INFINITY;
    int ws = -1, wc = -1, widx = -1;
    for (int s = 0; s < a.S; s++) {
        const long r = (long)w * a.S + s;
        double best = INFINITY;
        int bc = INT_MAX, out_of_limits = 0;
        for (int c = lane; c < f.C; c += 64) {
            const double v = a.pval[r * f.C + c];
            if (a.pidx[r * f.C + c] >= 0 && motion_before(v, c, best, bc)) {
                best = v;
                bc = c;
            }
            const double* st = f.rec + ((long)c * NR + r) * 2 * NF;
            for (int j = 0; j < NF; j++)
                if (st[j] < rp.state_lb[j] || st[j] > rp.state_ub[j] || fabs(st[NF + j]) > rp.speed_limits[j]) out_of_limits = 1;
        }
        motion_first_min(best, bc);
        out_of_limits = wave_or(out_of_limits);
        const bool none = bc == INT_MAX || O <= 0;
        const int idx = none ? -1 : a.pidx[r * f.C + bc];
        int fl = 0;
        if (!none && best <= 0) fl |= ARMOUR_TRACK_COLLISION;
        for (int j = 0; j < NF; j++) {
            if (f.out[track_out_max(TRACK_MAX_TORQUE, NR, r, j)] > rp.torque_limits[j]) fl |= ARMOUR_TRACK_INPUT;
            if (f.out[track_out_max(TRACK_MAX_POS, NR, r, j)] > rp.qe || f.out[track_out_max(TRACK_MAX_VEL, NR, r, j)] > rp.qde)
                fl |= ARMOUR_TRACK_BOUND;
        }
        if (out_of_limits) fl |= ARMOUR_TRACK_LIMIT;
        if (f.status[r] != 0) fl |= ARMOUR_TRACK_NOT_FINITE;
        if (lane == 0) {
            const MotionPair pr = motion_pair(idx, O);
            f.clearance[r] = none ? INFINITY : best;
            f.where[3 * r] = none ? -1 : bc;
            f.where[3 * r + 1] = pr.link;
            f.where[3 * r + 2] = pr.obs;
            f.flags[r] = fl;
        }
        if (!none && best < wbest) {
            wbest = best;
            ws = s;
            wc = bc;
            widx = idx;
        }
    }
    if (lane == 0) {
        const MotionPair pr = motion_pair(widx, O);  // (widx stays -1 with ws)
        f.wclear[w] = wbest;
        f.wwhere[4 * w] = ws;
        f.wwhere[4 * w + 1] = wc;
        f.wwhere[4 * w + 2] = pr.link;
        f.wwhere[4 * w + 3] = pr.obs;
    }
}

// clearance [W] and where [W][3] (sample, link, obstacle) from the per-sample minima: one wave per world
__global__ __launch_bounds__(64) void motion_finish_kernel(MotionArgs a, double* clearance, int* where) {
    const int w = blockIdx.x, lane = threadIdx.x;
    double best = INFINITY;
    int bs = INT_MAX;
    for (int s = lane; s < a.S; s += 64) {
        const double v = a.pval[(long)w * a.S + s];
        if (a.pidx[(long)w * a.S + s] >= 0 && motion_before(v, s, best, bs)) {
            best = v;
            bs = s;
        }
    }
    motion_first_min(best, bs);
    if (lane == 0) {
        const int O = motion_obstacles(a, w);
        const bool none = bs == INT_MAX || O <= 0;
        const MotionPair pr = motion_pair(none ? -1 : a.pidx[(long)w * a.S + bs], O);
        clearance[w] = none ? INFINITY : best;
        where[3 * w] = none ? -1 : bs;
        where[3 * w + 1] = pr.link;
        where[3 * w + 2] = pr.obs;
    }
}

// ---- episodes -----------------------------------------------------------------------------------
struct EpisodeDev {
    const RobotParams* rp;
    int W, S;
    double lookahead, goal_radius;
    armour_episode_state* st;  // [W] what the next plan starts from, and the bookkeeping
    const double* goal;        // [W][NF]
    double* pend;              // [W][4][NF] the last accepted plan (valid where has_pend)
    int* has_pend;             // [W]
    int* kind;                 // [W] what the world executes this step: -1 nothing (frozen), 0 stays at rest,
                               //     1 its new plan on [0, t_plan], 2 the pending plan on [t_plan, 1]
    double* exec;              // [W][4][NF] the executed trajectory
    double* win;               // [W][2] its window
    const int* accept;         // [W] the new plan is feasible and not vetoed
    const double* clearance;   // [W] of the executed segment (motion_finish_kernel)
    const int* where;          // [W][3]
};

// ||angdiff(q, goal)||_2 over all joints (kinova_world_static.m goal_check)
AD double goal_distance(const double* q, const double* goal) {
    double s = 0.0;
    for (int j = 0; j < NF; j++) {
        const double d = wrap_diff(goal[j] - q[j]);
        s += d * d;
    }
    return sqrt(s);
}
// the straight-line waypoint (robot_arm_straight_line_HLP.m:45-57): a step of `lookahead` toward the
// goal, the difference angle-wrapped on continuous joints (state_lb <= -1000)
AD void waypoint(const RobotParams& rp, const double* q, const double* goal, double lookahead, double* q_des) {
    double d[NF], s = 0.0;
    for (int j = 0; j < NF; j++) {
        d[j] = goal[j] - q[j];
        if (rp.state_lb[j] <= -1000.0) d[j] = wrap_diff(d[j]);
        s += d[j] * d[j];
    }
    const double n = sqrt(s);
    for (int j = 0; j < NF; j++) q_des[j] = n > 0 ? q[j] + lookahead * d[j] / n : q[j];
}

__global__ void episode_begin_kernel(EpisodeDev e, const double* q0, const double* qd0, const double* qdd0) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= e.W) return;
    armour_episode_state& S = e.st[w];
    bool moving = false;
    for (int j = 0; j < NF; j++) {
        S.q[j] = q0[w * NF + j];
        S.qd[j] = qd0[w * NF + j];
        S.qdd[j] = qdd0[w * NF + j];
        moving = moving || S.qd[j] != 0.0 || S.qdd[j] != 0.0;
    }
    const double* goal = e.goal + (long)w * NF;
    waypoint(*e.rp, S.q, goal, e.lookahead, S.q_des);
    S.goal_distance = goal_distance(S.q, goal);
    S.status = S.goal_distance <= e.goal_radius ? 1 : 0;
    S.mode = moving ? 1 : 0;
    S.steps = S.failed_plans = S.failed_streak = 0;
    S.clearance = INFINITY;
    S.clearance_at[0] = S.clearance_at[1] = S.clearance_at[2] = -1;
    e.has_pend[w] = 0;
}

// step (a): the pending state becomes the batch input
__global__ void episode_swap_kernel(EpisodeDev e, double* q0, double* qd0, double* qdd0, double* qdes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e.W * NF) return;
    const armour_episode_state& S = e.st[i / NF];
    const int j = i % NF;
    q0[i] = S.q[j];
    qd0[i] = S.qd[j];
    qdd0[i] = S.qdd[j];
    qdes[i] = S.q_des[j];
}

// step (b): what each running world executes (x: the plan's k_opt, [W] WorldState-strided)
__global__ void episode_choose_kernel(EpisodeDev e, const double* x, long x_stride, const double* q0, const double* qd0,
                                      const double* qdd0) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= e.W) return;
    armour_episode_state& S = e.st[w];
    double* ex = e.exec + (long)w * TRAJ_DOUBLES;
    double* pd = e.pend + (long)w * TRAJ_DOUBLES;
    const double t_plan = e.rp->t_plan;
    int kind = -1;
    double t0 = 1.0, t1 = 0.0;  // (an empty window: not checked)
    if (S.status == 0) {
        if (e.accept[w]) {
            kind = 1;
            S.failed_streak = 0;
            for (int j = 0; j < NF; j++) {
                ex[j] = q0[w * NF + j];
                ex[NF + j] = qd0[w * NF + j];
                ex[2 * NF + j] = qdd0[w * NF + j];
                ex[3 * NF + j] = x[(long)w * x_stride + j];
            }
            t0 = 0.0;
            t1 = t_plan;
        } else {
            S.failed_plans++;
            S.failed_streak++;
            if (S.mode == 1 && e.has_pend[w]) {
                kind = 2;
                for (int j = 0; j < TRAJ_DOUBLES; j++) ex[j] = pd[j];
                t0 = t_plan;
                t1 = 1.0;
            } else if (S.mode == 1) {
                S.status = 3;  // moving, and no fail-safe to fall back on
            } else {
                kind = 0;
            }
        }
    }
    e.kind[w] = kind;
    e.win[2 * w] = kind >= 1 ? t0 : 1.0;
    e.win[2 * w + 1] = kind >= 1 ? t1 : 0.0;
}

// step (c): clearance, goal test on every sample, the next state and its waypoint
__global__ void episode_advance_kernel(EpisodeDev e) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= e.W) return;
    armour_episode_state& S = e.st[w];
    const int kind = e.kind[w];
    if (kind < 0) return;
    const int step = S.steps;
    S.steps = step + 1;
    if (kind == 0) return;
    const RobotParams& rp = *e.rp;
    const double* ex = e.exec + (long)w * TRAJ_DOUBLES;
    const double* goal = e.goal + (long)w * NF;
    const double t0 = e.win[2 * w], t1 = e.win[2 * w + 1];
    double q[NF], qd[NF], qdd[NF];
    bool ok = true;
    for (int j = 0; j < NF; j++) {
        traj_joint(rp, ex, j, t1, q[j], qd[j], qdd[j]);
        ok = ok && isfinite(q[j]) && isfinite(qd[j]) && isfinite(qdd[j]) && fabs(q[j]) <= ARMOUR_MAX_ABS_ANGLE;
    }
    if (!ok) {
        S.status = 4;  // the next state lies outside the input domain: the old one stays
        return;
    }
    const double c = e.clearance[w];
    if (c < S.clearance) {
        S.clearance = c;
        S.clearance_at[0] = step;
        S.clearance_at[1] = e.where[3 * w + 1];
        S.clearance_at[2] = e.where[3 * w + 2];
    }
    bool reached = false;
    for (int s = 0; s < e.S; s++) {
        double qs[NF], v, a;
        const double t = motion_time(t0, t1, s, e.S);
        for (int j = 0; j < NF; j++) traj_joint(rp, ex, j, t, qs[j], v, a);
        reached = reached || goal_distance(qs, goal) <= e.goal_radius;
    }
    for (int j = 0; j < NF; j++) {
        S.q[j] = q[j];
        S.qd[j] = qd[j];
        S.qdd[j] = qdd[j];
    }
    S.goal_distance = goal_distance(q, goal);
    waypoint(rp, q, goal, e.lookahead, S.q_des);
    if (kind == 1) {
        S.mode = 1;
        double* pd = e.pend + (long)w * TRAJ_DOUBLES;
        for (int j = 0; j < TRAJ_DOUBLES; j++) pd[j] = ex[j];
        e.has_pend[w] = 1;
    } else {
        S.mode = 0;
        e.has_pend[w] = 0;
    }
    if (!(c > 0))
        S.status = 2;
    else if (reached)
        S.status = 1;
}

// ---- tracked episodes (armour_episode_track) --------------------------------------------------------
struct EpisodeTrackDev {
    int S;                        // true arms per world
    int stop_input, stop_bound, stop_limit;
    double* traj;                 // [W][4][NF] what the world's true arms follow this step
    double* win;                  // [W][2] its window; empty: the world is skipped
    armour_episode_tracked* rec;  // [W] the running record
    int* flags;                   // [W][S] of the last step each world executed
    // this step's results (the recording rollouts and motion_state_finish_kernel)
    const double* out;            // by field (track_store)
    const int* rflags;            // [W][S]
    const double* wclear;         // [W]
    const int* wwhere;            // [W][4]
};

__global__ void episode_track_begin_kernel(EpisodeDev e, EpisodeTrackDev t) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= e.W) return;
    armour_episode_tracked& R = t.rec[w];
    R.clearance = INFINITY;
    for (int k = 0; k < 4; k++) R.clearance_at[k] = -1;
    for (int j = 0; j < NF; j++) R.max_pos_err[j] = R.max_vel_err[j] = R.max_torque[j] = 0.0;
    R.max_V = R.max_robust = 0.0;
    R.flags = 0;
    for (int k = 0; k < 5; k++) R.flag_step[k] = -1;
    for (int s = 0; s < t.S; s++) t.flags[(long)w * t.S + s] = 0;
}

// after step (b): the trajectory and window the true arms follow: what the world executes, or, for a
// world that stays at rest, the constant trajectory (q, 0, 0, k = 0) on [0, t_plan] (the controller holds
// the arm and its error keeps evolving); a frozen world gets an empty window
__global__ void episode_track_choose_kernel(EpisodeDev e, EpisodeTrackDev t) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= e.W) return;
    const int kind = e.kind[w];
    double* tr = t.traj + (long)w * TRAJ_DOUBLES;
    if (kind >= 1) {
        for (int j = 0; j < TRAJ_DOUBLES; j++) tr[j] = e.exec[(long)w * TRAJ_DOUBLES + j];
        t.win[2 * w] = e.win[2 * w];
        t.win[2 * w + 1] = e.win[2 * w + 1];
        return;
    }
    for (int j = 0; j < NF; j++) {
        tr[j] = e.st[w].q[j];
        tr[NF + j] = tr[2 * NF + j] = tr[3 * NF + j] = 0.0;
    }
    t.win[2 * w] = kind == 0 ? 0.0 : 1.0;
    t.win[2 * w + 1] = kind == 0 ? e.rp->t_plan : 0.0;
}

// after step (c): the step's rollouts folded into the world's record, and the stops. The existing
// rules came first (episode_advance_kernel: 4, then 2 for the desired arm); the goal test's status 1
// stands only if no stop applies.
__global__ void episode_track_fold_kernel(EpisodeDev e, EpisodeTrackDev t) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= e.W) return;
    if (e.kind[w] < 0) return;
    armour_episode_state& S = e.st[w];
    armour_episode_tracked& R = t.rec[w];
    const int step = S.steps - 1;  // (episode_advance_kernel counted this step)
    const long NR = (long)e.W * t.S;
    if (t.wclear[w] < R.clearance) {
        R.clearance = t.wclear[w];
        R.clearance_at[0] = step;
        R.clearance_at[1] = t.wwhere[4 * w];
        R.clearance_at[2] = t.wwhere[4 * w + 2];
        R.clearance_at[3] = t.wwhere[4 * w + 3];
    }
    int fl = 0;
    for (int s = 0; s < t.S; s++) {
        const long r = (long)w * t.S + s;
        for (int j = 0; j < NF; j++) {
            R.max_pos_err[j] = fmax(R.max_pos_err[j], t.out[track_out_max(TRACK_MAX_POS, NR, r, j)]);
            R.max_vel_err[j] = fmax(R.max_vel_err[j], t.out[track_out_max(TRACK_MAX_VEL, NR, r, j)]);
            R.max_torque[j] = fmax(R.max_torque[j], t.out[track_out_max(TRACK_MAX_TORQUE, NR, r, j)]);
        }
        R.max_V = fmax(R.max_V, t.out[track_out_V(NR, r)]);
        R.max_robust = fmax(R.max_robust, t.out[track_out_robust(NR, r)]);
        t.flags[r] = t.rflags[r];
        fl |= t.rflags[r];
    }
    for (int k = 0; k < 5; k++)
        if (((fl >> k) & 1) && R.flag_step[k] < 0) R.flag_step[k] = step;
    R.flags |= fl;
    if (S.status == 4 || S.status == 2) return;
    if (fl & ARMOUR_TRACK_COLLISION)
        S.status = 2;
    else if (fl & ARMOUR_TRACK_NOT_FINITE)
        S.status = 8;
    else if ((fl & ARMOUR_TRACK_INPUT) && t.stop_input)
        S.status = 5;
    else if ((fl & ARMOUR_TRACK_BOUND) && t.stop_bound)
        S.status = 6;
    else if ((fl & ARMOUR_TRACK_LIMIT) && t.stop_limit)
        S.status = 7;
}

}  // namespace armour
