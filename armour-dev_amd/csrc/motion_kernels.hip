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
// episode_*_kernel      one thread per world: the bookkeeping of armour_episode_begin / _step.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>

#include "../../include/armour_hip.h"
#include "common.h"
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
__device__ inline double motion_separation(const double* ob, const double* link) {
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

// (value, index) ordered by value, then by index: the first minimiser
__device__ inline bool motion_before(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }

__global__ __launch_bounds__(MOTION_THREADS) void motion_check_kernel(MotionArgs a) {
    const int s = blockIdx.x, w = blockIdx.y, tid = threadIdx.x;
    __shared__ double s_obs[MAX_OBS * 12];
    __shared__ double s_cs[NF][2];
    __shared__ double s_link[MAX_J][12];
    __shared__ double s_wv[MOTION_WAVES];
    __shared__ int s_wi[MOTION_WAVES];
    const RobotParams& rp = *a.rp;
    const int NJ = rp.num_joints;
    int O = a.Ow ? a.Ow[w] : a.O;
    O = O < 0 ? 0 : (O > MAX_OBS ? MAX_OBS : O);
    double t0 = a.t0, t1 = a.t1;
    if (a.win) {
        t0 = a.win[2 * w];
        t1 = a.win[2 * w + 1];
    }
    const long out = (long)w * a.S + s;
    // (block-uniform) a world without obstacles, or one that executes nothing
    if (O == 0 || !(t0 <= t1)) {
        if (tid == 0) {
            a.pval[out] = INFINITY;
            a.pidx[out] = -1;
        }
        return;
    }
    const double* ob = a.obs + (long)w * a.O * 12;
    for (int i = tid; i < O * 12; i += MOTION_THREADS) s_obs[i] = ob[i];
    if (tid < NF) {
        const double* tr = a.traj + (long)w * TRAJ_DOUBLES;
        double q, qd, qdd;
        bezier_joint(tr[tid], tr[NF + tid], tr[2 * NF + tid], tr[3 * NF + tid] * rp.k_range[tid], motion_time(t0, t1, s, a.S), q,
                     qd, qdd);
        s_cs[tid][0] = cos(q);
        s_cs[tid][1] = sin(q);
    }
    __syncthreads();
    if (tid == 0) {
        // the chain is sequential: one thread, 2 x NJ 3x3 products
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
        for (int i = 0; i < NJ; i++) {
            const double* tr = rp.trans + 3 * i;
            for (int r = 0; r < 3; r++) p[r] += R[3 * r] * tr[0] + R[3 * r + 1] * tr[1] + R[3 * r + 2] * tr[2];
            double Ri[9], Rn[9];
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) Ri[3 * r + c] = rp.rpy[i][r + 3 * c];  // (stored column-major)
            const int ax = rp.axes[i];
            if (ax != 0 && i < NF) {
                // rotation by q about e_a; a reversed joint (code -a) turns about -e_a: Rot(e_a, -q)
                const double c = s_cs[i][0], sn = ax > 0 ? s_cs[i][1] : -s_cs[i][1];
                const int aa = (ax > 0 ? ax : -ax) - 1, u = (aa + 1) % 3, v = (aa + 2) % 3;
                double Q[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, RQ[9];
                Q[3 * u + u] = c;
                Q[3 * v + v] = c;
                Q[3 * u + v] = -sn;
                Q[3 * v + u] = sn;
                mat3_mul(Ri, Q, RQ);
                for (int e = 0; e < 9; e++) Ri[e] = RQ[e];
            }
            mat3_mul(R, Ri, Rn);
            for (int e = 0; e < 9; e++) R[e] = Rn[e];
            double* L = s_link[i];
            for (int r = 0; r < 3; r++)
                L[r] = p[r] + (R[3 * r] * rp.link_c[i][0] + R[3 * r + 1] * rp.link_c[i][1] + R[3 * r + 2] * rp.link_c[i][2]);
            for (int j = 0; j < 3; j++)
                for (int r = 0; r < 3; r++) L[3 + 3 * j + r] = R[3 * r + j] * rp.link_g[i][j];
        }
    }
    __syncthreads();
    double best = INFINITY;
    int bidx = INT_MAX;
    for (int idx = tid; idx < NJ * O; idx += MOTION_THREADS) {
        const int l = idx / O, o = idx - l * O;
        const double v = motion_separation(s_obs + 12 * o, s_link[l]);
        if (motion_before(v, idx, best, bidx)) {
            best = v;
            bidx = idx;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double ov = xor_f64(best, m);
        const int oi = xor_i32(bidx, m);
        if (motion_before(ov, oi, best, bidx)) {
            best = ov;
            bidx = oi;
        }
    }
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
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double ov = xor_f64(best, m);
        const int os = xor_i32(bs, m);
        if (motion_before(ov, os, best, bs)) {
            best = ov;
            bs = os;
        }
    }
    if (lane == 0) {
        int O = a.Ow ? a.Ow[w] : a.O;
        if (bs == INT_MAX || O <= 0) {
            clearance[w] = INFINITY;
            where[3 * w] = where[3 * w + 1] = where[3 * w + 2] = -1;
        } else {
            const int idx = a.pidx[(long)w * a.S + bs];
            clearance[w] = best;
            where[3 * w] = bs;
            where[3 * w + 1] = idx / O;
            where[3 * w + 2] = idx - (idx / O) * O;
        }
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
        bezier_joint(ex[j], ex[NF + j], ex[2 * NF + j], ex[3 * NF + j] * rp.k_range[j], t1, q[j], qd[j], qdd[j]);
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
        for (int j = 0; j < NF; j++) bezier_joint(ex[j], ex[NF + j], ex[2 * NF + j], ex[3 * NF + j] * rp.k_range[j], t, qs[j], v, a);
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

}  // namespace armour
