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
// track_row_rec_kernel, track_serial_rec_kernel   the same two bodies with a recorder (armour_track_motion;
//                      the _episode_ kernels: a tracked episode's step, with per-trajectory windows and
//                      carried states, TrackMode below):
//                      lane 0 of a row (the thread, in the serial form) also stores the 14 doubles of
//                      every check point into rec [check point][rollout][2][7], so neighbouring rows
//                      store neighbouring memory. The recorder only reads the state: maxima, end state
//                      and status are those of the kernels without one.
// Both forms run the same functions on the same values in the same order and agree bitwise.
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

// a stage in row form: this lane's RNEA, the rest replicated over the row (KERNEL: as TrackSerialEvalT's)
template <int KERNEL>
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

// What a kernel does beyond the plain rollouts. TRACK_RECORD: check points go to rec (TrackCheckpoints).
// TRACK_EPISODE (a tracked episode's step): the record, and every trajectory carries its own window
// win [N][2] and every rollout starts from its carried state [NR][2][NF], which its end state replaces.
// An empty window (t0 < t1 does not hold) skips the rollout: no thread may leave before a barrier, so it
// computes on [0, 1] and stores nothing, as rows past the last rollout do.
enum TrackMode { TRACK_PLAIN = 0, TRACK_RECORD = 1, TRACK_EPISODE = 2 };
struct TrackExtra {
    double* rec;        // [steps / stride + 1][NR][2][NF]
    int stride;
    const double* win;  // TRACK_EPISODE
    double* state;      // TRACK_EPISODE
};

// window, start and gate of rollout i; returns whether its results are stored
template <int MODE>
__device__ __forceinline__ bool track_begin(const TrackArgs& a, const TrackExtra& e, const RobotParams& rp, const double* traj,
                                            long i, bool live, double& t0, double& t1, TrackState& X) {
    t0 = a.t0;
    t1 = a.t1;
    if constexpr (MODE == TRACK_EPISODE) {
        t0 = e.win[2 * (i / a.S)];
        t1 = e.win[2 * (i / a.S) + 1];
        const bool run = t0 < t1;
        if (!run) {
            t0 = 0.0;
            t1 = 1.0;
        }
        track_init(e.state + i * 2 * NF, X);
        return live && run;
    } else {
        track_init(rp, traj, a.err0 ? a.err0 + i * 2 * NF : nullptr, t0, X);
        return live;
    }
}
template <int MODE>
__device__ __forceinline__ void track_end(const TrackArgs& a, const TrackExtra& e, const TrackState& X, long i, long NR) {
    track_store(X, i, NR, a.out, a.status);
    if constexpr (MODE == TRACK_EPISODE)
        for (int j = 0; j < NF; j++) {
            e.state[i * 2 * NF + j] = X.q[j];
            e.state[i * 2 * NF + NF + j] = X.qd[j];
        }
}

// the body of the row form; lane 0 of a live row stores
template <int MODE>
__device__ __forceinline__ void track_row_body(const TrackArgs& a, const TrackExtra& e) {
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
    TrackRowEval<MODE> ev{s_rp, s_traj[row], s_scale[row][0], s_scale[row][1], s_cs[row], s_G[row], sub};
    TrackState X;
    double t0, t1;
    const bool store = track_begin<MODE>(a, e, s_rp, s_traj[row], i, live, t0, t1, X) && sub == 0;
    if constexpr (MODE == TRACK_PLAIN)
        track_run(ev, t0, t1, a.steps, X);
    else
        track_run(ev, t0, t1, a.steps, X, TrackCheckpoints{e.rec, NR, i, e.stride, store});
    if (store) track_end<MODE>(a, e, X, i, NR);
}
__global__ __launch_bounds__(TRACK_THREADS) void track_row_kernel(TrackArgs a) { track_row_body<TRACK_PLAIN>(a, TrackExtra{}); }
__global__ __launch_bounds__(TRACK_THREADS) void track_row_rec_kernel(TrackArgs a, TrackExtra e) { track_row_body<TRACK_RECORD>(a, e); }
__global__ __launch_bounds__(TRACK_THREADS) void track_row_episode_kernel(TrackArgs a, TrackExtra e) {
    track_row_body<TRACK_EPISODE>(a, e);
}

template <int MODE>
__device__ __forceinline__ void track_serial_body(const TrackArgs& a, const TrackExtra& e) {
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
    if constexpr (MODE == TRACK_PLAIN) {
        track_rollout_serial(s_rp, traj, ms, is, a.err0 ? a.err0 + i * 2 * NF : nullptr, a.t0, a.t1, a.steps, X);
        if (live) track_store(X, i, NR, a.out, a.status);
    } else {
        TrackSerialEvalT<MODE> ev{s_rp, traj, ms, is};
        double t0, t1;
        const bool store = track_begin<MODE>(a, e, s_rp, traj, i, live, t0, t1, X);
        track_run(ev, t0, t1, a.steps, X, TrackCheckpoints{e.rec, NR, i, e.stride, store});
        if (store) track_end<MODE>(a, e, X, i, NR);
    }
}
__global__ __launch_bounds__(TRACK_THREADS) void track_serial_kernel(TrackArgs a) { track_serial_body<TRACK_PLAIN>(a, TrackExtra{}); }
__global__ __launch_bounds__(TRACK_THREADS) void track_serial_rec_kernel(TrackArgs a, TrackExtra e) {
    track_serial_body<TRACK_RECORD>(a, e);
}
__global__ __launch_bounds__(TRACK_THREADS) void track_serial_episode_kernel(TrackArgs a, TrackExtra e) {
    track_serial_body<TRACK_EPISODE>(a, e);
}

}  // namespace armour
