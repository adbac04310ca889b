// armour-mi355x — the kernels of armour_track (include/armour_hip.h): rollouts of the true arm under
// the robust controller, math in track.h.
//
// track_row_kernel     "row form": one rollout per 16 lanes (one DPP row), 4 rollouts per wave, one
//                      wave per block. A stage needs ten RNEAs that differ only in inputs; lane l < 10
//                      of the row takes role l (lanes 10..15 repeat role 9 and contribute nothing). The
//                      sines and cosines (lane j < 7: joint j) and the ten results pass through a small
//                      LDS tile per row; everything else (desired state, robust input, Cholesky solve,
//                      RK4 update, maxima) is replicated over the row in uniform code, so every lane of a
//                      row carries the same state and lane 0 stores it. The robot tables and the row's
//                      parameter scales are read into LDS once per block. Rows past the last rollout
//                      compute rollout NR - 1 again and store nothing. No atomics.
// track_serial_kernel  the serial form of track.h, one thread per rollout: the definition the host
//                      build tests and the baseline the row form is measured against
//                      (ARMOUR_TRACK_KERNEL=serial).
// Both run the same functions on the same values in the same order and agree bitwise.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "track.h"

namespace armour {

constexpr int TRACK_THREADS = 64;
constexpr int TRACK_ROW = 16;
constexpr int TRACK_ROWS = TRACK_THREADS / TRACK_ROW;

struct TrackArgs {
    const RobotParams* rp;
    int N, S;               // trajectories, samples per trajectory (NR = N * S rollouts)
    const double* traj;     // [N][4][NF]
    const double* scale;    // [NR][2][num_joints] mass and inertia scales; null: 1
    const double* err0;     // [NR][2][NF]; null: 0
    double t0, t1;
    int steps;
    double* out;            // [TRACK_OUT_DOUBLES][NR] by field (track_store)
    int* status;            // [NR]
};

// a stage in row form: this lane's RNEA, the rest replicated over the row
struct TrackRowEval {
    const RobotParams& rp;
    const double* traj;
    const double* ms;
    const double* is;
    double* cs;   // LDS [2 * NF] of this row
    double* G;    // LDS [TRACK_ROLES][TRACK_GATHER] of this row
    int sub;      // lane within the row
    __device__ void operator()(double t, const double* q, const double* qd, TrackPre& P, TrackStage& S) const {
        double rqd[NF], rqa[NF], rqdda[NF], u[NF], rho[NF];
        track_pre(rp, traj, t, q, qd, P);
        // (a select over the unrolled index keeps q in registers)
        double qs = q[0];
#pragma unroll
        for (int j = 1; j < NF; j++) qs = sub == j ? q[j] : qs;
        if (sub < NF) {
            cs[2 * sub] = cos(qs);
            cs[2 * sub + 1] = sin(qs);
        }
        __syncthreads();
        const int role = sub < TRACK_ROLES ? sub : TRACK_ROLES - 1;
        bool use_true, full;
        track_role(role, P, qd, rqd, rqa, rqdda, use_true, full);
        track_rnea(rp, cs, rqd, rqa, rqdda, ms, is, use_true, full, full, u, rho);
        if (sub < TRACK_ROLES) {
#pragma unroll
            for (int j = 0; j < NF; j++) {
                G[sub * TRACK_GATHER + j] = u[j];
                G[sub * TRACK_GATHER + NF + j] = rho[j];
            }
        }
        __syncthreads();
        track_post(rp, P, G, S);
    }
};

__global__ __launch_bounds__(TRACK_THREADS) void track_row_kernel(TrackArgs a) {
    __shared__ RobotParams s_rp;
    __shared__ double s_traj[TRACK_ROWS][TRAJ_DOUBLES];
    __shared__ double s_scale[TRACK_ROWS][2][MAX_J];
    __shared__ double s_cs[TRACK_ROWS][2 * NF];
    __shared__ double s_G[TRACK_ROWS][TRACK_ROLES * TRACK_GATHER];
    const int tid = threadIdx.x, row = tid / TRACK_ROW, sub = tid % TRACK_ROW;
    const long NR = (long)a.N * a.S;
    const long id = (long)blockIdx.x * TRACK_ROWS + row;
    const bool live = id < NR;
    const long i = live ? id : NR - 1;
    {
        const int* src = reinterpret_cast<const int*>(a.rp);
        int* dst = reinterpret_cast<int*>(&s_rp);
        for (int k = tid; k < (int)(sizeof(RobotParams) / sizeof(int)); k += TRACK_THREADS) dst[k] = src[k];
    }
    const int NJ = a.rp->num_joints;
    for (int k = sub; k < TRAJ_DOUBLES; k += TRACK_ROW) s_traj[row][k] = a.traj[(i / a.S) * TRAJ_DOUBLES + k];
    for (int k = sub; k < 2 * MAX_J; k += TRACK_ROW) {
        const int which = k / MAX_J, l = k % MAX_J;
        s_scale[row][which][l] = (a.scale && l < NJ) ? a.scale[(i * 2 + which) * NJ + l] : 1.0;
    }
    __syncthreads();
    TrackRowEval ev{s_rp, s_traj[row], s_scale[row][0], s_scale[row][1], s_cs[row], s_G[row], sub};
    TrackState X;
    track_init(s_rp, s_traj[row], a.err0 ? a.err0 + i * 2 * NF : nullptr, a.t0, X);
    track_run(ev, a.t0, a.t1, a.steps, X);
    if (live && sub == 0) track_store(X, i, NR, a.out, a.status);
}

__global__ __launch_bounds__(TRACK_THREADS) void track_serial_kernel(TrackArgs a) {
    __shared__ RobotParams s_rp;
    const int tid = threadIdx.x;
    const long NR = (long)a.N * a.S;
    const long id = (long)blockIdx.x * TRACK_THREADS + tid;
    const bool live = id < NR;
    const long i = live ? id : NR - 1;
    {
        const int* src = reinterpret_cast<const int*>(a.rp);
        int* dst = reinterpret_cast<int*>(&s_rp);
        for (int k = tid; k < (int)(sizeof(RobotParams) / sizeof(int)); k += TRACK_THREADS) dst[k] = src[k];
    }
    __syncthreads();
    const int NJ = s_rp.num_joints;
    double traj[TRAJ_DOUBLES], ms[MAX_J], is[MAX_J];
    for (int k = 0; k < TRAJ_DOUBLES; k++) traj[k] = a.traj[(i / a.S) * TRAJ_DOUBLES + k];
    for (int l = 0; l < MAX_J; l++) {
        ms[l] = (a.scale && l < NJ) ? a.scale[(i * 2) * NJ + l] : 1.0;
        is[l] = (a.scale && l < NJ) ? a.scale[(i * 2 + 1) * NJ + l] : 1.0;
    }
    TrackState X;
    track_rollout_serial(s_rp, traj, ms, is, a.err0 ? a.err0 + i * 2 * NF : nullptr, a.t0, a.t1, a.steps, X);
    if (live) track_store(X, i, NR, a.out, a.status);
}

}  // namespace armour
