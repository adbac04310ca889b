// armour-mi355x — device data layout of the batched NLP (W worlds planned together).
#pragma once
#include "reach.h"

namespace armour {

constexpr int EVAL_THREADS = 256;
constexpr int ROW_THREADS = 256;
constexpr int MAX_FILTER = 64;
constexpr int KA = 56;   // partial-sum slots per row block (pass A is the largest user)
constexpr int KA2 = 8;   // pass D's partial sums (partial2), kept apart so the fused D + A pass writes both

// solver options (oracle/src/ipm.h IpmOptions)
struct IpmOpts {
    double tol = 1e-4;
    int max_iter = 100;
    double mu0 = 0.1;
    double kappa_eps = 10.0;
    double kappa_mu = 0.2;
    double theta_mu = 1.5;
    double tau_min = 0.99;
    double bound_push = 1e-2;
    double eta = 1e-4;
    int max_ls = 10;
    double kappa_sigma = 1e10;
    double s_max = 100.0;
    double inf_bound = 1e19;
    // barrier strategy: 1 adaptive (default: the reference's IPOPT_MU_STRATEGY "adaptive",
    // KPR/Parameters.h:57, restated with Ipopt's LOQO mu oracle and kkt-error globalisation, mu on a
    // 2^(1/8) grid with floor tol / 10, as oracle/src/ipm.cpp); 0 monotone
    // (ARMOUR_MU_STRATEGY=monotone); 2 Ipopt's default adaptive pair, the quality-function oracle with
    // the obj-constr-filter globalisation and mu_min 1e-11 (ARMOUR_MU_STRATEGY=quality); 3 that pair
    // with the floor tol / 10 and the mu grid (quality-floor). armour_set_solver_options; the other two
    // options and the state they need: OptDev
    int mu_strategy = 1;
    // restoration phase (nlp_kernels.hip resto_*, oracle/src/ipm.cpp restoration): phases per
    // solve (ARMOUR_RESTORATION=0: none), violation target inside the bounds, box barrier weight,
    // stall ratio
    int resto_max = 3;
    double resto_delta = 1e-6;
    double resto_mu = 1e-8;
    double resto_stall = 1e-4;
};

struct WorldState {
    double x[NF], xt[NF], dx[NF];
    double H[NF * NF];
    double mu, alpha, ap, ad, theta0, phi0, Dphi, theta_max, theta_min, kkt;
    double sw_dphi, sw_theta;          // pow(-Dphi, 2.3) (Dphi < 0) and pow(theta0, 1.1) of this
                                       // iteration: the switching condition's powers, once per iteration
    double wa_old_a[NF], wa_old_b[NF];   // sum (z_lo - z_hi) a  and  sum (dz_lo - dz_hi) a at x
    double filt_theta[MAX_FILTER], filt_phi[MAX_FILTER];
    int nfilt;
    int cur;           // eval slot holding the current point
    int status;        // 0 running, 1 converged, 2 max_iter, 3 line-search failure, 4 reach over capacity,
                       // 5 local infeasibility (the restoration phase stalled or failed), 6 in the
                       // restoration phase (WS_RESTO), 7 restarting after it (WS_RESTART)
    int searching;     // 1 while the line search of this iteration has not accepted
    int accepted_ok;   // last acceptance passed the filter (0: forced after max_ls trials)
    int ftype;
    int first_update, nfail, iter, nevals, ls;
    int spec_k;        // trial of the speculative round that ended the line search (-1: none)
    // adaptive barrier: free (oracle) mode, and the KKT errors the globalisation compares against
    // (free mode: the last <= 4; fixed mode: the one at the switch)
    int free_mode, nref;
    double kkt_ref[4];
    // restoration phase: phases entered, consecutive stalled iterations, a chosen step waiting
    // for its full evaluation (applied by the next resto_world_G), Phi of the previous iteration
    int nresto, rstall, rpend;
    double rphi;
};
constexpr int WS_RESTO = 6;
// The optional solver configurations' per-world state (armour_solver_options: the quality-function
// barrier oracle, strategies 2 and 3, and the limited-memory BFGS), in an array of its own beside ws
// so that WorldState, which every world kernel stages in LDS, keeps its size. Only lane 0 of a world
// kernel touches it, and only under those options.
constexpr int QF_GMAX = 32;  // most sigma candidates
constexpr int QF_TILE = 8;   // candidates a sweep of ipm_rows_Q carries in registers
constexpr int LB_MAX = 6;    // longest L-BFGS history
constexpr int QP = 3 * QF_GMAX + 1;  // ipm_rows_Q's sums per world: cc, a_P, a_D per candidate, sum r_p^2
struct QfState {
    double mu_max;             // Ipopt's mu_max, min(1e5, 1e3 avg(s z)) at the first iteration (-1: not set)
    double avg;                // avg(s z) of this iteration
    double dx0[NF], dx1[NF];   // the affine step and the step per unit mu of this iteration
    double lb_s[LB_MAX][NF], lb_y[LB_MAX][NF];  // the L-BFGS pairs, oldest first
    int ngf;                   // entries of the free-mode filter of (f, theta) (NlpDev::gf)
    int nlb, lb_skips;         // stored pairs, updates skipped in a row
    int pending;               // this iteration's mu waits for the sigma search (ipm_rows_Q, ipm_world_Q)
};
// What the kernels of the optional configurations take beside the NlpDev (the world steps of passes A
// and D, the sigma search, ipm_world_init, resto_world_G): the two options, the per-world state and the
// sigma candidates. Kept out of NlpDev, which every other kernel takes by value and keeps as it was.
struct OptDev {
    QfState* qs;            // [W]
    double* gf;             // [W][2][gf_cap]: the free-mode filter's f, then theta (strategies 2, 3)
    double* qpart;          // [W][QP]: ipm_rows_Q's sums
    int gf_cap;             // max_iter + 1: at most one entry per iteration
    int qf_grid;            // sigma candidates of the quality function (strategies 2, 3), 2 .. QF_GMAX
    int lbfgs_history;      // 0 damped full BFGS; 1 .. LB_MAX Ipopt's limited-memory BFGS (world_D_body)
    double sig[QF_GMAX];    // the candidates, formed on the host (std::pow, as oracle/src/ipm.cpp forms them)
};
// A world whose restoration phase reached a point within every bound waits for its slacks and
// multipliers (ipm_rows_init) before it runs again: status 0 would let a phase run inside the
// interior-point loop hand it back to lists that still name it (planner.hip ipm_loop)
constexpr int WS_RESTART = 7;

// Slots of the device counters NlpDev::cnt and of the mapped host flags NlpDev::flags. A slot named
// with a parity is a pair (base, base + 1), taken with slot(base, parity).
enum CntSlot : int {
    CNT_RUN = 0,      // worlds a world kernel has appended to wl_run (round 0) / counted (resto_count)
    CNT_SEARCH = 1,   // worlds appended to wl_search (ipm_world_Cs_all: worlds that searched past round 0)
    CNT_TICKET = 2,   // block ticket: the last block publishes the counts and zeroes the three
    CNT_LS = 4,       // + parity of the line-search round: length of that round's searching list
    CNT_PC_MISS = 7,  // evaluations that found a block's plane records missing (get_plane_cache_stats)
    CNT_ITER = 8,     // + parity of the iteration: length of that iteration's running list
    CNT_RL = 12,      // length of the append list of restoration work (Round::rl_app)
    CNT_PL = 14,      // length of the phase list resto_publish moved it into
    CNT_LEN = 16
};
enum FlagSlot : int {
    FLAG_RUN = 0,     // worlds running after round 0 / counted by resto_count, ipm_collect
    FLAG_SEARCH = 1,  // worlds still searching after the last line-search round
    FLAG_NRUN = 2,    // + parity: a sync-free iteration's running count, read one iteration later
    FLAG_BT = 4,      // + parity: its worlds that searched past round 0
    FLAG_PEND = 6,    // + parity: CNT_RL as its last world kernel saw it (Round::pend_flag)
    FLAG_PUB = 8,     // + parity: the list length a concurrent phase iteration's publish moved
    FLAG_LEN = 12
};
constexpr int slot(int base, int parity) { return base + (parity & 1); }
// Every slot, a pair with both parities, lies inside its array of len entries and no two overlap:
// the bit masks of the slots (slot1: a single slot, slot2: a pair) add up without a carry
constexpr unsigned slot1(int s) { return 1u << s; }
constexpr unsigned slot2(int s) { return 3u << s; }
template <class... M>
constexpr bool slots_apart(int len, M... m) { return (m + ...) == (m | ...) && (m | ...) < (1u << len); }
static_assert(slots_apart(CNT_LEN, slot1(CNT_RUN), slot1(CNT_SEARCH), slot1(CNT_TICKET), slot2(CNT_LS), slot1(CNT_PC_MISS), slot2(CNT_ITER),
                          slot1(CNT_RL), slot1(CNT_PL)), "cnt slots");
static_assert(slots_apart(FLAG_LEN, slot1(FLAG_RUN), slot1(FLAG_SEARCH), slot2(FLAG_NRUN), slot2(FLAG_BT), slot2(FLAG_PEND), slot2(FLAG_PUB)),
              "flags slots");
enum EvalMode : int {  // what an evaluation launch evaluates (eval_kernel_t's int mode)
    EVAL_POINT = 0,   // the start point / a caller's point, every world, into slot 0
    EVAL_TRIAL = 1,   // the trial point of the searching worlds
    EVAL_CHOSEN = 5   // the trial a speculative round chose, in full
};

// What a solve is, fixed from init_solver / upload_* / ensure_plane_cache until the next batch.
// Every solver kernel takes it by value; what one launch does with it is the Round beside it.
struct NlpDev {
    int W, T, NJ, O, m, R, nblk, chunk;
    // the ARMTD comparison planner (ACMP/NLPclass.cu): no torque rows (nt = 0, else NF * T),
    // constant-acceleration extrema and cost with a per-world k_range [W][NF]
    int armtd, nt;
    const double* krange;
    int diag;               // diagnostics (ARMOUR_EVAL_SKIP): bit 0 skip slicing, bit 1 skip collision rows
    const RobotParams* rp;
    IpmOpts opt;
    // per-world inputs
    const double* q0;
    const double* qd0;
    const double* qdd0;
    const double* qdes;
    const double* obs;      // [W][O][12]
    // reach outputs
    ReachOut ro;
    // row bounds [W][R]
    double *L, *U;
    // evaluation slots: g [2][W][m], J [2][W][m][NF], f [2][W], grad [2][W][NF]. The collision
    // rows' Jacobian is held compactly: row (l, t, o) is J = n . dc/dx with n the winning plane's
    // signed normal, jn [2][W][T * NJ * O][3], and dc/dx the sliced link centre's derivatives,
    // jd [2][W][T][NJ][NF][3] (shared by the row's O obstacles); J keeps the other rows (and, after a
    // start-point / caller evaluation, EVAL_POINT, the collision rows dense too). row_va expands them.
    double* g;
    double* J;
    double* jn;
    double* jd;
    long njn, njd;          // per-slot sizes of jn, jd (W * T * NJ * Omax * 3, W * T * NJ * NF * 3)
    double* f;
    double* grad;
    double* link_c;         // [3][lcs]: [slot][W][T][NJ][3] sliced link centres of each eval slot's
                            // latest evaluation; region 2 the final iterate's (feasible_kernel)
    long lcs;
    // solver row state [W][R]
    double *slo, *shi, *zlo, *zhi, *dslo, *dshi;
    double* partial;        // [W][nblk][KA]
    double* partial2;       // [W][nblk][KA2]: pass D
    WorldState* ws;         // [W]
    int* flags;             // mapped host memory, [FLAG_LEN] (FlagSlot): kernels store counts, the host reads them
    unsigned* cnt;          // device counters, [CNT_LEN] (CntSlot)
    // Certified plane cache (plane_cache_kernel). The 36 planes of a buffered
    // obstacle and their offsets d, delta do not depend on x; only A . c(x) does. For every
    // (world, t, link, obstacle) the cache holds the planes that can attain the maximum for some x in
    // the box |x_i| <= PC_XBOX, in the reference's scan order. The records of a (world, t) block are
    // n = its kept-plane count contiguous records at pcbase[w][t] of one pool: [5][n] (A0 A1 A2,
    // P = d + delta, N = -d + delta) from pc + 5 pcbase, the pair (l * O + o) of each from
    // pcp + pcbase; pcoff [W][T][NJ * O] = (first record << 8) | count; pcok [W][T] = 1 when the pool
    // held the block (the host sizes the pool from the count every build needed, ensure_plane_cache,
    // so a build that ran out is repeated on a larger pool and every block is cached).
    int pcache;             // cache enabled (ARMOUR_PLANE_CACHE=0 disables it)
    int pcready;            // built for the current reach sets and obstacles
    long pc_pool;           // records in the pool
    double* pc;             // [5 pc_pool]
    uint16_t* pcp;          // [pc_pool]
    unsigned* pcoff;
    unsigned char* pcok;
    unsigned long long* pcbase;  // [W][T] first pool record of each block
    unsigned* pcnext;            // pool records handed out by the current build (zeroed by jrs_kernel)
    // Mixed batch (armour_plan_batch_mixed): the obstacle count of each world, [W]; null for a uniform
    // batch. O, m, R and nblk above then hold the batch maximum and serve only as strides and grid
    // sizes; a world's own extents come from shape_of<true>.
    const int* Ow;
};

// What one launch does: the planner builds one per launch family (planner.hip, the round_*
// functions) and passes it beside the NlpDev. Round{} is a launch over every world (blockIdx =
// world) that appends to no list, publishes no count and is no restoration launch.
struct Round {
    // Active-world compaction: the launch covers the worlds of list wl (blockIdx -> wl[b]). The
    // world kernels append the worlds still running (round 0, ls0) into wl_run and those still
    // searching into wl_search; the last block publishes the counts (FLAG_RUN, FLAG_SEARCH).
    // Launched without a host synchronisation: the grid is an upper bound, the list's true length
    // is *lcount (null: the grid is exact); ipm_world_C stores wl_search's length into lcount_out.
    // (wl and lcount come first: Round{wl, lcount} is a launch over a list and nothing else.)
    const int* wl = nullptr;
    const unsigned* lcount = nullptr;
    int *wl_run = nullptr, *wl_search = nullptr;
    int ls0 = 0;                      // this ipm_world_C launch is round 0 of an iteration
    unsigned* lcount_out = nullptr;
    // sync-free iterations: round 0 also stores the running count into lrun_out (the next
    // iteration's lcount) and nrun_flag, and the worlds that searched past round 0 into bt_flag
    // (both mapped host memory, read by the host one iteration later)
    unsigned* lrun_out = nullptr;
    int *nrun_flag = nullptr, *bt_flag = nullptr;
    // Speculative rows: the values (g, f) of K trial points of every listed world, [list entry i]
    // [trial k], and their row sums (eval_trials_*, ipm_rows_Cs / resto_rows_Vs, the *_Cs / _Vs world
    // kernels); the chosen trial is then evaluated in full (EVAL_CHOSEN). The view is the planner's
    // buffers, shifted for a phase iteration that runs beside the tail (planner.hip spec_view).
    int K = 0;
    double *gs = nullptr, *fs = nullptr, *partial_s = nullptr;
    // the tail's one-round search: pass B's world step runs in ipm_world_Cs_all, the trial passes
    // before it take the first step from pass B's partials (pass_b_alpha), every running world searches
    int b_in_cs = 0;
    // restoration launch: the evaluations take the worlds in the phase (WS_RESTO), not the searching
    // ones; rflag: the FlagSlot resto_world_G's count of them goes to (-1: none)
    int resto = 0, rflag = -1;
    // phases inside the interior-point loop: a world whose line search fails, and every world
    // resto_world_Vs keeps, is appended to rl_app (CNT_RL; null: phases run after the loop);
    // pend_flag: mapped host flag the round's last world kernel stores that list's length into
    int *rl_app = nullptr, *pend_flag = nullptr;
};
constexpr int EV_MAXK = 9;   // speculative trials per world (max_ls - 1)
constexpr int PC_K = 12;               // initial pool: records per pair per block (ARMOUR_PC_K; the survey workload keeps 5.3)
constexpr double PC_XBOX = 1.0 + 1e-6; // certified box of x (the solver keeps |x_i| <= 1)
constexpr double PC_RADF = 1.0001;     // >= PC_XBOX^21, the largest monomial degree sum (7 x 3)
constexpr double PC_MARGIN = 1e-9;     // >> the rounding of the bound and of A . c (~1e-15)

AD int world_of(const Round& r, int b) { return r.wl ? r.wl[b] : b; }

AD long gidx(const NlpDev& d, int slot, int w, long r) { return ((long)slot * d.W + w) * d.m + r; }

// In-world extents of world w: obstacles, constraints, solver rows (constraints + the box rows on x)
// and row blocks. A uniform batch's are the batch's (the fields of NlpDev, no load); a mixed batch's
// come from the world's own count, so its rows have the layout and the row-to-block partition of a
// uniform batch of O_w obstacles (chunk is a constant), inside slabs strided by the batch maximum.
struct Shape {
    int O, m, R, nblk;
};
template <bool MX>
AD Shape shape_of(const NlpDev& d, int w) {
    if constexpr (MX) {
        const int O = d.Ow[w];
        const int m = d.nt + d.T * d.NJ * O + 4 * NF;
        const int R = m + NF;
        return Shape{O, m, R, (R + d.chunk - 1) / d.chunk};
    } else {
        return Shape{d.O, d.m, d.R, d.nblk};
    }
}

}  // namespace armour
