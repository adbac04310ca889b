// armour-mi355x — tracking rollouts (armour_track, include/armour_hip.h): the true arm under the
// reference's ARMOUR robust controller, at points. Host + device; no kernel here.
//
//   track_rnea       the point RNEA of KPR/Dynamics.cu:83-181 with the midpoint-radius form of the
//                    interval RNEA (rnea.cpp passRNEA_Int) for mass m (1 +- dm) and inertia I (1 +- dI)
//   track_pre        desired state, tracking errors and the auxiliary rates of one stage
//   track_role       the inputs of one of the ten RNEAs of a stage (columns of M, b, tau, Mr)
//   track_post       the robust input (robust_controller.cpp:63-168, ARMOUR method), the unpivoted
//                    Cholesky solve of the plant and the true storage function
//   track_step       one classical RK4 step; track_record the maxima; track_rollout_serial the whole
//                    rollout with every RNEA in one thread ("serial form")
//   TrackCheckpoints the recorder of armour_track_motion: the states its clearance check reads
//
// A stage is written as pre -> ten track_rnea calls that differ only in inputs -> post, so that the
// row kernel (track_kernels.hip: one RNEA per lane, the rest replicated over the 16 lanes of a row)
// and the serial form perform the same operations in the same order and agree bitwise
// (-ffp-contract=off). Every sum is written out left to right; tests/track_model.py follows the same
// order.
#pragma once
#include <cmath>

#include "common.h"
#include "traj.h"

namespace armour {

constexpr int TRACK_ROLES = 10;                  // 7 columns of M, b, tau (+ rho), Mr (+ rMr)
constexpr int TRACK_ROLE_B = NF, TRACK_ROLE_TAU = NF + 1, TRACK_ROLE_MR = NF + 2;
constexpr int TRACK_GATHER = 2 * NF;             // per role: u[7], radius[7]
// The rollouts' outputs, out [TRACK_OUT_DOUBLES][NR] by field: max_pos_err, max_vel_err, max_torque
// [NR][NF], max_V, max_robust [NR], end_state [NR][2][NF]. Index of rollout i's element of each field
// (the whole index in the function: with `+ j` left to the caller the tracking kernels' address
// arithmetic came out differently, profiles/exec_layer_resources.txt):
constexpr int TRACK_MAX_POS = 0, TRACK_MAX_VEL = 1, TRACK_MAX_TORQUE = 2;  // the three maxima, joint j
AD constexpr long track_out_max(int which, long NR, long i, int j) { return (which * NR + i) * NF + j; }
AD constexpr long track_out_V(long NR, long i) { return 3 * NF * NR + i; }
AD constexpr long track_out_robust(long NR, long i) { return (3 * NF + 1) * NR + i; }
// end state: half 0 is q, half 1 is qd
AD constexpr long track_out_end(long NR, long i, int half, int j) { return (3 * NF + 2) * NR + i * 2 * NF + half * NF + j; }
constexpr int TRACK_OUT_DOUBLES = 3 * NF + 2 + 2 * NF;  // per rollout: three maxima [NF], V, lambda, end state
static_assert(track_out_end(1, 1, 0, 0) == TRACK_OUT_DOUBLES, "the last field of one rollout ends where the array does");

// finite: neither NaN nor infinite (written with a comparison: host + device)
AD bool track_finite(double x) { return fabs(x) < INFINITY; }

AD void track_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// the "absolute cross" |a| (x) |b|: an enclosure of the radius of a x b
AD void track_abscross(const double* a, const double* b, double* c) {
    c[0] = fabs(a[1]) * fabs(b[2]) + fabs(a[2]) * fabs(b[1]);
    c[1] = fabs(a[2]) * fabs(b[0]) + fabs(a[0]) * fabs(b[2]);
    c[2] = fabs(a[0]) * fabs(b[1]) + fabs(a[1]) * fabs(b[0]);
}
// row-major 3x3: y = A x, y = A' x, y = |A| |x|
AD void track_mv(const double* A, const double* x, double* y) {
    for (int r = 0; r < 3; r++) y[r] = A[3 * r] * x[0] + A[3 * r + 1] * x[1] + A[3 * r + 2] * x[2];
}
AD void track_mtv(const double* A, const double* x, double* y) {
    for (int c = 0; c < 3; c++) y[c] = A[c] * x[0] + A[3 + c] * x[1] + A[6 + c] * x[2];
}
AD void track_amv(const double* A, const double* x, double* y) {
    for (int r = 0; r < 3; r++)
        y[r] = fabs(A[3 * r]) * fabs(x[0]) + fabs(A[3 * r + 1]) * fabs(x[1]) + fabs(A[3 * r + 2]) * fabs(x[2]);
}

// R_i = RPY_i Rot_axis_i(q_i) (row-major) from cs[i] = cos q_i, sin q_i; RPY_i alone for a fixed joint;
// the identity past the last joint. A reversed joint (code -a) turns about -e_a: Rot(e_a, -q).
AD void track_joint_rot(const RobotParams& rp, int i, const double* cs, double* R) {
    if (i >= rp.num_joints) {
        for (int e = 0; e < 9; e++) R[e] = (e % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double* P = rp.rpy[i];  // column-major
    const int ax = rp.axes[i];
    if (ax == 0 || i >= NF) {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R[3 * r + c] = P[r + 3 * c];
        return;
    }
    const double co = cs[2 * i], sn = ax > 0 ? cs[2 * i + 1] : -cs[2 * i + 1];
    const int a = (ax > 0 ? ax : -ax) - 1, u = (a + 1) % 3, v = (a + 2) % 3;
    for (int c = 0; c < 3; c++) {
        // column c of Q = Rot: e_a for c = a; cos e_u + sin e_v for c = u; -sin e_u + cos e_v for c = v
        const double qu = c == u ? co : (c == v ? -sn : 0.0), qv = c == u ? sn : (c == v ? co : 0.0), qa = c == a ? 1.0 : 0.0;
        double Q[3];
        for (int k = 0; k < 3; k++) Q[k] = k == a ? qa : (k == u ? qu : qv);
        for (int r = 0; r < 3; r++) R[3 * r + c] = P[r] * Q[0] + P[r + 3] * Q[1] + P[r + 6] * Q[2];
    }
}

// u [7], rho [7]: generalised torques of the point RNEA at the configuration behind cs, with joint
// rates qd, auxiliary rates qa and auxiliary accelerations qdda, and their radius. Link i has mass
// mass_i * ms[i] and inertia inertia_i * is[i] when use_true (ms / is are not read otherwise).
// friction[] is not modelled (as in the planner's RNEA).
AD void track_rnea(const RobotParams& rp, const double* cs, const double* qd, const double* qa, const double* qdda,
                   const double* ms, const double* is, bool use_true, bool grav, bool damp, double* u, double* rho) {
    const int NJ = rp.num_joints;
    const double dm = rp.mass_uncertainty, dI = rp.inertia_uncertainty;
    double F[MAX_J][3], N[MAX_J][3], rF[MAX_J][3], rN[MAX_J][3];
    double w[3] = {0, 0, 0}, wa[3] = {0, 0, 0}, wd[3] = {0, 0, 0}, acc[3] = {0, 0, grav ? rp.gravity : 0.0};
    double R[9], t1[3], t2[3], t3[3];
#pragma unroll
    for (int i = 0; i < MAX_J; i++) {
        if (i >= NJ) continue;
        track_joint_rot(rp, i, cs, R);
        const double* p = rp.trans + 3 * i;
        track_cross(wd, p, t1);
        track_cross(wa, p, t2);
        track_cross(w, t2, t3);
        for (int e = 0; e < 3; e++) t1[e] = acc[e] + t1[e] + t3[e];
        track_mtv(R, t1, acc);
        track_mtv(R, w, t1);
        track_mtv(R, wa, t2);
        track_mtv(R, wd, t3);
        for (int e = 0; e < 3; e++) {
            w[e] = t1[e];
            wa[e] = t2[e];
            wd[e] = t3[e];
        }
        const int ax = rp.axes[i];
        if (ax != 0 && i < NF) {
            // the joint's angular rates lie along its signed axis z
            const int a = (ax > 0 ? ax : -ax) - 1;
            double z[3], zq[3];
            for (int e = 0; e < 3; e++) {
                z[e] = e == a ? (ax > 0 ? 1.0 : -1.0) : 0.0;
                zq[e] = qd[i] * z[e];
            }
            track_cross(wa, zq, t1);
            for (int e = 0; e < 3; e++) {
                w[e] = w[e] + zq[e];
                wd[e] = wd[e] + t1[e] + qdda[i] * z[e];
                wa[e] = wa[e] + qa[i] * z[e];
            }
        }
        const double* c = rp.com + 3 * i;
        track_cross(wd, c, t1);
        track_cross(wa, c, t2);
        track_cross(w, t2, t3);
        const double m = rp.mass[i] * (use_true ? ms[i] : 1.0);
        const double si = use_true ? is[i] : 1.0;
        for (int e = 0; e < 3; e++) {
            const double ac = acc[e] + t1[e] + t3[e];
            F[i][e] = m * ac;
            rF[i][e] = dm * fabs(m) * fabs(ac);
        }
        double I[9];
        for (int e = 0; e < 9; e++) I[e] = rp.inertia[9 * i + e] * si;
        track_mv(I, w, t1);
        track_mv(I, wd, t2);
        track_cross(wa, t1, t3);
        for (int e = 0; e < 3; e++) N[i][e] = t2[e] + t3[e];
        track_amv(I, w, t1);
        track_amv(I, wd, t2);
        track_abscross(wa, t1, t3);
        for (int e = 0; e < 3; e++) rN[i][e] = dI * (t2[e] + t3[e]);
    }
    double f[3] = {0, 0, 0}, n[3] = {0, 0, 0}, rf[3] = {0, 0, 0}, rn[3] = {0, 0, 0};
    for (int j = 0; j < NF; j++) u[j] = rho[j] = 0.0;
#pragma unroll
    for (int i = MAX_J - 1; i >= 0; i--) {
        if (i >= NJ) continue;
        track_joint_rot(rp, i + 1, cs, R);
        const double* c = rp.com + 3 * i;
        const double* p1 = rp.trans + 3 * (i + 1);
        double Rf[3], Rn[3];
        track_mv(R, f, Rf);
        track_mv(R, n, Rn);
        track_cross(c, F[i], t1);
        track_cross(p1, Rf, t2);
        for (int e = 0; e < 3; e++) {
            n[e] = N[i][e] + Rn[e] + t1[e] + t2[e];
            f[e] = Rf[e] + F[i][e];
        }
        track_amv(R, rf, Rf);
        track_amv(R, rn, Rn);
        track_abscross(c, rF[i], t1);
        track_abscross(p1, Rf, t2);
        for (int e = 0; e < 3; e++) {
            rn[e] = rN[i][e] + Rn[e] + t1[e] + t2[e];
            rf[e] = Rf[e] + rF[i][e];
        }
        const int ax = rp.axes[i];
        if (ax != 0 && i < NF) {
            const int a = (ax > 0 ? ax : -ax) - 1;
            double z[3];
            for (int e = 0; e < 3; e++) z[e] = e == a ? (ax > 0 ? 1.0 : -1.0) : 0.0;
            double v = n[0] * z[0] + n[1] * z[1] + n[2] * z[2] + rp.armature[i] * qdda[i];
            if (damp) v = v + rp.damping[i] * qd[i];
            u[i] = v;
            rho[i] = rn[0] * fabs(z[0]) + rn[1] * fabs(z[1]) + rn[2] * fabs(z[2]);
        }
    }
}

// desired state and the controller's rates at (t, q, qd)
struct TrackPre {
    double q_des[NF], qd_des[NF];
    double qa_d[NF], qa_dd[NF], r[NF];
};
AD void track_pre(const RobotParams& rp, const double* traj, double t, const double* q, const double* qd, TrackPre& P) {
    for (int j = 0; j < NF; j++) {
        double qdd_des;
        traj_joint(rp, traj, j, t, P.q_des[j], P.qd_des[j], qdd_des);
        double e = P.q_des[j] - q[j];
        if (rp.state_lb[j] <= -1000.0) e = wrap_diff(e);  // a continuous joint: one remainder, no loop
        const double de = P.qd_des[j] - qd[j];
        P.qa_d[j] = P.qd_des[j] + rp.K * e;
        P.qa_dd[j] = qdd_des + rp.K * de;
        P.r[j] = de + rp.K * e;
    }
}

// inputs of RNEA `role` of a stage: 0..6 column j of M (true, no gravity, no damping, zero rates,
// qdda = e_j); 7 b = R(q, qd, qd, 0; true); 8 tau (nominal); 9 Mr = R(q, 0, 0, r; nominal, no gravity,
// no damping)
AD void track_role(int role, const TrackPre& P, const double* qd, double* rqd, double* rqa, double* rqdda, bool& use_true,
                   bool& full) {
    use_true = role <= TRACK_ROLE_B;
    full = role == TRACK_ROLE_B || role == TRACK_ROLE_TAU;  // gravity and damping
    for (int j = 0; j < NF; j++) {
        rqd[j] = full ? qd[j] : 0.0;
        rqa[j] = role == TRACK_ROLE_B ? qd[j] : (role == TRACK_ROLE_TAU ? P.qa_d[j] : 0.0);
        rqdda[j] = role < NF ? (j == role ? 1.0 : 0.0) : (role == TRACK_ROLE_TAU ? P.qa_dd[j] : (role == TRACK_ROLE_MR ? P.r[j] : 0.0));
    }
}

// result of one stage
struct TrackStage {
    double u[NF], qdd[NF];
    double V, lambda;
    bool ok;  // every pivot positive and finite, every acceleration finite
};
// G [TRACK_ROLES][TRACK_GATHER]: u and radius of every role
AD void track_post(const RobotParams& rp, const TrackPre& P, const double* G, TrackStage& S) {
    const double* b = G + TRACK_ROLE_B * TRACK_GATHER;
    const double* tau = G + TRACK_ROLE_TAU * TRACK_GATHER;
    const double* rho = tau + NF;
    const double* Mr = G + TRACK_ROLE_MR * TRACK_GATHER;
    const double* rMr = Mr + NF;
    double rMrs = 0.0, arMr = 0.0, nr2 = 0.0, nrho2 = 0.0;
    for (int j = 0; j < NF; j++) {
        rMrs = rMrs + P.r[j] * Mr[j];
        arMr = arMr + fabs(P.r[j]) * rMr[j];
        nr2 = nr2 + P.r[j] * P.r[j];
        nrho2 = nrho2 + rho[j] * rho[j];
    }
    const double V_sup = 0.5 * (rMrs + arMr), h = rp.V_m - V_sup;
    const double nr = sqrt(nr2), nrho = sqrt(nrho2);
    S.lambda = 0.0;
    if (nr > 0) S.lambda = fmax(0.0, -rp.alpha * h / nr + nrho);
    double rhs[NF];
    for (int j = 0; j < NF; j++) {
        S.u[j] = nr > 0 ? tau[j] + S.lambda * P.r[j] / nr : tau[j];
        rhs[j] = S.u[j] - b[j];
    }
    // M (i, j) = G[j][i]; unpivoted Cholesky M = L L' on the entries i >= j, column by column
    double L[NF][NF];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NF; j++) {
        double s = G[j * TRACK_GATHER + j];
#pragma unroll
        for (int k = 0; k < j; k++) s = s - L[j][k] * L[j][k];
        ok = ok && s > 0 && track_finite(s);
        const double d = sqrt(s);
        L[j][j] = d;
#pragma unroll
        for (int i = j + 1; i < NF; i++) {
            double v = G[j * TRACK_GATHER + i];
#pragma unroll
            for (int k = 0; k < j; k++) v = v - L[i][k] * L[j][k];
            L[i][j] = v / d;
        }
    }
    double y[NF];
#pragma unroll
    for (int i = 0; i < NF; i++) {
        double v = rhs[i];
#pragma unroll
        for (int k = 0; k < i; k++) v = v - L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = NF - 1; i >= 0; i--) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < NF; k++) v = v - L[k][i] * S.qdd[k];
        S.qdd[i] = v / L[i][i];
    }
    double V = 0.0;
    for (int i = 0; i < NF; i++) {
        double Mri = 0.0;
        for (int j = 0; j < NF; j++) Mri = Mri + G[j * TRACK_GATHER + i] * P.r[j];
        V = V + P.r[i] * Mri;
        ok = ok && track_finite(S.qdd[i]) && track_finite(S.u[i]);
    }
    S.V = 0.5 * V;
    S.ok = ok && track_finite(S.V) && track_finite(S.lambda);
}

// one rollout: state, maxima and status (armour_track_output)
struct TrackState {
    double q[NF], qd[NF];
    double max_pos_err[NF], max_vel_err[NF], max_torque[NF];
    double max_V, max_robust;
    int status;
};

AD void track_init(const RobotParams& rp, const double* traj, const double* err0, double t0, TrackState& X) {
    bool ok = true;
    for (int j = 0; j < NF; j++) {
        double q, qd, qdd;
        traj_joint(rp, traj, j, t0, q, qd, qdd);
        X.q[j] = err0 ? q + err0[j] : q;
        X.qd[j] = err0 ? qd + err0[NF + j] : qd;
        if (!(track_finite(X.q[j]) && track_finite(X.qd[j]))) {
            ok = false;
            X.q[j] = q;
            X.qd[j] = qd;
        }
        X.max_pos_err[j] = X.max_vel_err[j] = X.max_torque[j] = 0.0;
    }
    X.max_V = X.max_robust = 0.0;
    X.status = ok ? 0 : 1;
}

// the absolute-state form: the rollout starts from state = q [NF], then qd [NF] (a tracked episode's
// carried true state, finite by construction: it is a start the host checked or an end state)
AD void track_init(const double* state, TrackState& X) {
    for (int j = 0; j < NF; j++) {
        X.q[j] = state[j];
        X.qd[j] = state[NF + j];
        X.max_pos_err[j] = X.max_vel_err[j] = X.max_torque[j] = 0.0;
    }
    X.max_V = X.max_robust = 0.0;
    X.status = 0;
}

// the maxima at a recorded stage; a stage that is not ok ends the rollout
AD void track_record(const TrackPre& P, const TrackStage& S, TrackState& X) {
    if (X.status != 0) return;
    if (!S.ok) {
        X.status = 1;
        return;
    }
    for (int j = 0; j < NF; j++) {
        X.max_pos_err[j] = fmax(X.max_pos_err[j], fabs(X.q[j] - P.q_des[j]));
        X.max_vel_err[j] = fmax(X.max_vel_err[j], fabs(X.qd[j] - P.qd_des[j]));
        X.max_torque[j] = fmax(X.max_torque[j], fabs(S.u[j]));
    }
    X.max_V = fmax(X.max_V, S.V);
    X.max_robust = fmax(X.max_robust, S.lambda);
}

// One classical RK4 step of (q, qd)' = (qd, qdd) from t to t + h. ev(t, q, qd, P, S) evaluates a
// stage. The first stage is recorded. The step is committed only when all four stages are ok and the
// new state is finite; otherwise the rollout keeps its state and gets status 1.
template <class Eval>
AD void track_step(Eval& ev, double t, double h, TrackState& X) {
    TrackPre P;
    TrackStage S;
    double sq[NF], sv[NF], yq[NF], yv[NF];
    const double hh = 0.5 * h;
    ev(t, X.q, X.qd, P, S);
    track_record(P, S, X);
    bool ok = S.ok;
    for (int j = 0; j < NF; j++) {
        sq[j] = X.qd[j];
        sv[j] = S.qdd[j];
        yq[j] = X.q[j] + hh * X.qd[j];
        yv[j] = X.qd[j] + hh * S.qdd[j];
    }
    ev(t + hh, yq, yv, P, S);
    ok = ok && S.ok;
    for (int j = 0; j < NF; j++) {
        sq[j] = sq[j] + 2 * yv[j];
        sv[j] = sv[j] + 2 * S.qdd[j];
        const double kq = yv[j];
        yq[j] = X.q[j] + hh * kq;
        yv[j] = X.qd[j] + hh * S.qdd[j];
    }
    ev(t + hh, yq, yv, P, S);
    ok = ok && S.ok;
    for (int j = 0; j < NF; j++) {
        sq[j] = sq[j] + 2 * yv[j];
        sv[j] = sv[j] + 2 * S.qdd[j];
        const double kq = yv[j];
        yq[j] = X.q[j] + h * kq;
        yv[j] = X.qd[j] + h * S.qdd[j];
    }
    ev(t + h, yq, yv, P, S);
    ok = ok && S.ok;
    const double h6 = h / 6;
    for (int j = 0; j < NF; j++) {
        yq[j] = X.q[j] + h6 * (sq[j] + yv[j]);
        yv[j] = X.qd[j] + h6 * (sv[j] + S.qdd[j]);
        ok = ok && track_finite(yq[j]) && track_finite(yv[j]);
    }
    if (X.status != 0) return;
    if (!ok) {
        X.status = 1;
        return;
    }
    for (int j = 0; j < NF; j++) {
        X.q[j] = yq[j];
        X.qd[j] = yv[j];
    }
}

// A recorder sees the state at the first stage of every step (s = 0 .. steps - 1) and at t1 (s = steps).
// It only reads: the rollout is the same with and without one. TrackNoRecord is the empty one.
struct TrackNoRecord {
    AD void operator()(int, const TrackState&) const {}
};
// Check point c = s / stride of rollout i goes to rec [check point][rollout][2][NF] (q, then qd) when
// s is a multiple of stride (steps % stride == 0, so t1 is the last check point). A rollout that
// stopped being finite records the state it keeps. `on` gates the stores (one lane of a row; a live row).
struct TrackCheckpoints {
    double* rec;
    long NR, i;
    int stride;
    bool on;
    AD void operator()(int s, const TrackState& X) const {
        if (!on || s % stride != 0) return;
        double* dst = rec + ((long)(s / stride) * NR + i) * 2 * NF;
        for (int j = 0; j < NF; j++) {
            dst[j] = X.q[j];
            dst[NF + j] = X.qd[j];
        }
    }
};

// `steps` RK4 steps over [t0, t1] (step s starts at t0 + s h) and the last record at t1
template <class Eval, class Rec>
AD void track_run(Eval& ev, double t0, double t1, int steps, TrackState& X, const Rec& rec) {
    const double h = (t1 - t0) / steps;
    for (int s = 0; s < steps; s++) {
        rec(s, X);
        track_step(ev, t0 + s * h, h, X);
    }
    TrackPre P;
    TrackStage S;
    ev(t1, X.q, X.qd, P, S);
    track_record(P, S, X);
    rec(steps, X);
}
template <class Eval>
AD void track_run(Eval& ev, double t0, double t1, int steps, TrackState& X) {
    track_run(ev, t0, t1, steps, X, TrackNoRecord{});
}

// the serial form of a stage: all ten RNEAs in this thread. KERNEL only names the instantiation: every
// kernel runs track_step / track_run on a stage type of its own, so that each copy has one caller and is
// inlined into its kernel as when there was one kernel per form (a shared copy is called, not inlined:
// measured 106 ms against 83 ms for the rollouts of profiles/track_time.txt)
template <int KERNEL = 0>
struct TrackSerialEvalT {
    const RobotParams& rp;
    const double* traj;  // [4][7]
    const double* ms;    // [num_joints] mass scales (null: 1)
    const double* is;    // [num_joints] inertia scales
    AD void operator()(double t, const double* q, const double* qd, TrackPre& P, TrackStage& S) const {
        double cs[2 * NF], G[TRACK_ROLES * TRACK_GATHER], rqd[NF], rqa[NF], rqdda[NF];
        track_pre(rp, traj, t, q, qd, P);
        for (int j = 0; j < NF; j++) {
            cs[2 * j] = cos(q[j]);
            cs[2 * j + 1] = sin(q[j]);
        }
        for (int role = 0; role < TRACK_ROLES; role++) {
            bool use_true, full;
            track_role(role, P, qd, rqd, rqa, rqdda, use_true, full);
            track_rnea(rp, cs, rqd, rqa, rqdda, ms, is, use_true && ms != nullptr, full, full, G + role * TRACK_GATHER,
                       G + role * TRACK_GATHER + NF);
        }
        track_post(rp, P, G, S);
    }
};
using TrackSerialEval = TrackSerialEvalT<>;

AD void track_rollout_serial(const RobotParams& rp, const double* traj, const double* ms, const double* is, const double* err0,
                             double t0, double t1, int steps, TrackState& X) {
    TrackSerialEval ev{rp, traj, ms, is};
    track_init(rp, traj, err0, t0, X);
    track_run(ev, t0, t1, steps, X);
}

// the per-rollout outputs as the kernels store them (the layout at the top)
AD void track_store(const TrackState& X, long i, long NR, double* out, int* status) {
    for (int j = 0; j < NF; j++) {
        out[track_out_max(TRACK_MAX_POS, NR, i, j)] = X.max_pos_err[j];
        out[track_out_max(TRACK_MAX_VEL, NR, i, j)] = X.max_vel_err[j];
        out[track_out_max(TRACK_MAX_TORQUE, NR, i, j)] = X.max_torque[j];
        out[track_out_end(NR, i, 0, j)] = X.q[j];
        out[track_out_end(NR, i, 1, j)] = X.qd[j];
    }
    out[track_out_V(NR, i)] = X.max_V;
    out[track_out_robust(NR, i)] = X.max_robust;
    status[i] = X.status;
}

}  // namespace armour
