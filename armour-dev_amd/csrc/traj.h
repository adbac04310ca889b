// armour-mi355x — the desired trajectory at a point: the degree-5 Bezier curve of
// KPR/Trajectory.cu:542-599 (control points q0, q0 + qd0 / 5, q0 + 2 qd0 / 5 + qdd0 / 20, then three
// times q0 + k k_range; DURATION = 1) and the angle wrap of continuous joints. Shared by the execution
// check and the episodes (motion_kernels.hip) and by the tracking rollouts (track.h); host + device.
#pragma once
#include <cmath>

#include "common.h"

namespace armour {

constexpr int TRAJ_DOUBLES = 4 * NF;     // q0, qd0, qdd0, k (normalised)

// position, velocity and acceleration of joint j of the trajectory traj [4][NF] (q0, qd0, qdd0, then k
// normalised to [-1, 1], scaled here by the robot's k_range: the one place that knows this layout) on the
// Bezier curve at s in [0, 1], from the Bernstein form (at s = 1 the velocity and the acceleration are
// exactly 0 and q is exactly q0 + k). One function, not a wrapper of a scalar one: behind a wrapper the
// tracking kernels' sums came out with commuted operands (profiles/exec_layer_resources.txt).
AD void traj_joint(const RobotParams& rp, const double* traj, int j, double s, double& q, double& qd, double& qdd) {
    const double q0 = traj[j], qd0 = traj[NF + j], qdd0 = traj[2 * NF + j], k = traj[3 * NF + j] * rp.k_range[j];
    const double b[6] = {q0, q0 + qd0 / 5, q0 + 2 * qd0 / 5 + qdd0 / 20, q0 + k, q0 + k, q0 + k};
    double d1[5], d2[4], ps[6], pr[6];
    for (int i = 0; i < 5; i++) d1[i] = 5 * (b[i + 1] - b[i]);
    for (int i = 0; i < 4; i++) d2[i] = 4 * (d1[i + 1] - d1[i]);
    ps[0] = pr[0] = 1.0;
    for (int i = 1; i < 6; i++) {
        ps[i] = ps[i - 1] * s;
        pr[i] = pr[i - 1] * (1 - s);
    }
    const double c5[6] = {1, 5, 10, 10, 5, 1}, c4[5] = {1, 4, 6, 4, 1}, c3[4] = {1, 3, 3, 1};
    q = qd = qdd = 0.0;
    for (int i = 0; i < 6; i++) q += c5[i] * ps[i] * pr[5 - i] * b[i];
    for (int i = 0; i < 5; i++) qd += c4[i] * ps[i] * pr[4 - i] * d1[i];
    for (int i = 0; i < 4; i++) qdd += c3[i] * ps[i] * pr[3 - i] * d2[i];
}

// difference b - a wrapped to [-pi, pi)
AD double wrap_diff(double d) {
    const double two_pi = 2 * M_PI;
    double m = fmod(d + M_PI, two_pi);
    if (m < 0) m += two_pi;
    return m - M_PI;
}

}  // namespace armour
