// TEST HARNESS — the serial form of the tracking rollouts (track.h) on the host, for tests/test_track_unit.py.
#include "robots.h"
#include "track.h"

using namespace armour;

extern "C" {

// N x S rollouts as armour_track defines them; out [TRACK_OUT_DOUBLES][N * S] by field (track_store)
int track_host_rollouts(const armour_robot* robot, int N, const double* traj, int S, const double* scale, const double* err0,
                        double t0, double t1, int steps, double* out, int* status) {
    RobotParams rp;
    if (!robot_from_tables(*robot, rp)) return -1;
    const int NJ = rp.num_joints;
    const long NR = (long)N * S;
    for (long i = 0; i < NR; i++) {
        TrackState X;
        track_rollout_serial(rp, traj + (i / S) * TRAJ_DOUBLES, scale ? scale + (i * 2) * NJ : nullptr,
                             scale ? scale + (i * 2 + 1) * NJ : nullptr, err0 ? err0 + i * 2 * NF : nullptr, t0, t1, steps, X);
        track_store(X, i, NR, out, status);
    }
    return 0;
}

// n point RNEAs with radius: q, qd, qa, qdda, u, rho [n][7]; scale [n][2][num_joints] or null
int track_host_rnea(const armour_robot* robot, int n, const double* q, const double* qd, const double* qa, const double* qdda,
                    const double* scale, int gravity, int damping, double* u, double* rho) {
    RobotParams rp;
    if (!robot_from_tables(*robot, rp)) return -1;
    const int NJ = rp.num_joints;
    for (long i = 0; i < n; i++) {
        double cs[2 * NF];
        for (int j = 0; j < NF; j++) {
            cs[2 * j] = cos(q[i * NF + j]);
            cs[2 * j + 1] = sin(q[i * NF + j]);
        }
        track_rnea(rp, cs, qd + i * NF, qa + i * NF, qdda + i * NF, scale ? scale + (i * 2) * NJ : nullptr,
                   scale ? scale + (i * 2 + 1) * NJ : nullptr, scale != nullptr, gravity != 0, damping != 0, u + i * NF,
                   rho + i * NF);
    }
    return 0;
}
}
