// armour-mi355x — host runtime and C ABI (include/armour_hip.h).
//
// One planner handle owns a HIP stream and every device buffer for up to max_worlds worlds of
// T time steps and max_obstacles obstacles, allocated once (the reference allocates per process,
// KPR/CollisionChecking.cu:17-53). A batch runs entirely on the device:
//   reach_kernel (JRS + PZ FK/RNEA + torque radius) -> bounds_kernel ->
//   armour-IPM passes (eval_kernel_t + ipm_rows_* / ipm_world_*) -> feasible_kernel;
// the host only sequences launches and reads one flag word per line-search round.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/armour_hip.h"
#include "nlp_kernels.hip"
#include "reach_kernel.hip"
#include "lane_kernel.hip"
#include "motion_kernels.hip"
#include "roadmap_kernels.hip"
#include "track_kernels.hip"
#include "robots.h"

using namespace armour;

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCK(expr)                                                                               \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(ARMOUR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class T>
hipError_t dalloc(T** p, size_t n) {
    return hipMalloc((void**)p, sizeof(T) * (n > 0 ? n : 1));
}
}  // namespace

// A set of device buffers allocated on first use and regrown when a call needs more (the candidate,
// execution-check and tracking buffers). The pointers live where their users read them (planner
// fields); the set knows which they are, so there is one way to grow and one to free.
struct GrowSet {
    struct Buf {
        void** ptr;
        size_t bytes;
    };
    template <class T>
    static Buf buf(T*& p, size_t n) { return {(void**)&p, sizeof(T) * n}; }

    long cap = 0;  // what the buffers hold, in the caller's unit (candidates, samples, rollouts)
    std::vector<void**> held;

    void release() {
        for (void** h : held) {
            if (*h) (void)hipFree(*h);
            *h = nullptr;
        }
        held.clear();
        cap = 0;
    }
    // Room for `need`: nothing to do within the capacity; otherwise the old set is freed once the
    // stream's work on it has finished, and the new set is allocated whole or not at all.
    int reserve(hipStream_t stream, long need, std::initializer_list<Buf> bufs, const char* failure) {
        if (need <= cap) return 0;
        HIPCK(hipStreamSynchronize(stream));
        release();
        for (const Buf& b : bufs) {
            *b.ptr = nullptr;
            held.push_back(b.ptr);
            if (hipMalloc(b.ptr, b.bytes) != hipSuccess) {
                release();
                return fail(ARMOUR_E_HIP, failure);
            }
        }
        cap = need;
        return 0;
    }
};

// The execution layer's state on a planner (everything that runs a plan after it is found) is one struct
// per feature: its device pointers on this base, which holds the buffers regrown on demand and the events
// around the feature's kernels, both made on first use, and releases them for armour_destroy.
struct ExecState {
    GrowSet grow;
    hipEvent_t ev[4] = {};
    int events(int n) {  // the first n exist from here on
        for (int i = 0; i < n; i++)
            if (!ev[i]) HIPCK(hipEventCreate(&ev[i]));
        return 0;
    }
    void release() {
        grow.release();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
// device time between two recorded events (*ms is left alone when the read fails)
static int elapsed_ms(hipEvent_t a, hipEvent_t b, double* ms) {
    float f = 0.f;
    HIPCK(hipEventElapsedTime(&f, a, b));
    *ms = f;
    return 0;
}
// armour_check_motion and the episodes' check of the desired arm (motion_kernels.hip): per-sample minima
// for max_worlds x grow.cap samples; the caller's trajectories and the per-world results, allocated once
// (the planner's `allocs` own them)
struct MotionCheck : ExecState {
    double* pval = nullptr;
    int* pidx = nullptr;
    double *traj = nullptr, *clear = nullptr;
    int* where = nullptr;
};
// armour_track (track_kernels.hip): inputs and per-rollout outputs for grow.cap rollouts
struct Rollouts : ExecState {
    double *traj = nullptr, *scale = nullptr, *err0 = nullptr, *out = nullptr;
    int* status = nullptr;
    int reserve(hipStream_t stream, long NR) {
        if (int rc = events(2)) return rc;
        const size_t n = (size_t)NR;
        return grow.reserve(stream, NR,
                            {GrowSet::buf(traj, n * TRAJ_DOUBLES), GrowSet::buf(scale, n * 2 * MAX_J), GrowSet::buf(err0, n * 2 * NF),
                             GrowSet::buf(out, n * TRACK_OUT_DOUBLES), GrowSet::buf(status, n)},
                            "hipMalloc failed for the tracking rollouts' buffers (num_traj x num_samples)");
    }
};
// armour_track_motion (the recording track kernels, motion_state_*_kernel): the recorded check points,
// their per-check-point minima and the per-rollout and per-world results, for grow.cap = rollouts x
// check points (check points >= 2, so at most cap / 2 rollouts: the per-rollout arrays are sized by the
// cells as well, which holds for every split)
struct TrueArmCheck : ExecState {
    double *rec = nullptr, *pval = nullptr, *clear = nullptr, *wclear = nullptr;
    int *pidx = nullptr, *where = nullptr, *flags = nullptr, *wwhere = nullptr;
    int reserve(hipStream_t stream, long cells, int Wmax) {
        if (int rc = events(2)) return rc;
        const size_t n = (size_t)cells, Wm = (size_t)Wmax;
        return grow.reserve(stream, cells,
                            {GrowSet::buf(rec, n * 2 * NF), GrowSet::buf(pval, n), GrowSet::buf(pidx, n), GrowSet::buf(clear, n),
                             GrowSet::buf(where, n * 3), GrowSet::buf(flags, n), GrowSet::buf(wclear, Wm), GrowSet::buf(wwhere, Wm * 4)},
                            "hipMalloc failed for the true-arm check's buffers (worlds x num_samples x check_samples)");
    }
};
// armour_episode_*: the episode's own arrays are allocated by the first begin (the planner's `allocs`)
struct Episode : ExecState {
    bool on = false;       // an episode is running (armour_episode_begin .. any other reach / plan entry)
    bool stepped = false;  // it has taken a step
    EpisodeDev dev{};
    int* accept = nullptr;
    std::vector<armour_episode_state> host;  // the states after the last begin / step
    std::vector<double> goals;               // [W][NF] of the last begin (armour_episode_roadmap's vertex N)
};
// armour_episode_track: what a tracked episode keeps between steps (the true arms' states, their scales,
// the worlds' records), for grow.cap = max_worlds x num_samples rollouts
struct TrackedEpisode : ExecState {
    bool on = false;  // armour_episode_track .. the next armour_episode_begin
    EpisodeTrackDev dev{};
    int steps = 0;
    double *state = nullptr, *scale = nullptr;
    bool scaled = false;
};

// armour_roadmap_* and armour_episode_roadmap (roadmap_kernels.hip): the per-vertex arrays for grow.cap =
// worlds x vertices, the edge list for edges.cap candidate edges and a byte per interior sample for
// samples.cap of them (the host reads the build's totals and sizes the two)
struct Roadmap : ExecState {
    bool valid = false;    // armour_roadmap_build .. any other batch entry
    bool episode = false;  // the running episode takes its waypoints from it (armour_episode_roadmap)
    RoadmapDev dev{};
    GrowSet edges, samples;
    hipEvent_t bev[7] = {};
    double *verts = nullptr, *q = nullptr, *q_des = nullptr, *left = nullptr, *ep_left = nullptr;
    int *row_eoff = nullptr, *row_soff = nullptr, *entry = nullptr, *ep_entry = nullptr;
    void release_all() {
        release();
        edges.release();
        samples.release();
        for (hipEvent_t e : bev)
            if (e) (void)hipEventDestroy(e);
    }
};

// planners alive per device (armour_create / armour_destroy): the bundle kernel's shape depends on
// whether the GPU is shared (lane_shape_for)
static std::atomic<int> g_planners[64];

// The path census (include/armour_hip.h, armour_get_path_counts): one counter per branch of every
// host-side dispatch decision, incremented where the host makes the choice, from what it knows there.
// Plain integers on the handle, cumulative since creation; nothing on the device sees them.
#define ARMOUR_PATHS(X)                                                                            \
    X(BATCH_UNIFORM, "batch_uniform") X(BATCH_MIXED, "batch_mixed")                                \
    X(REACH_JOB_256, "reach_job_256") X(REACH_JOB_128, "reach_job_128")                            \
    X(REACH_LANE_WIDE, "reach_lane_wide") X(REACH_LANE_DENSE, "reach_lane_dense")                  \
    X(REACH_RETRY, "reach_retry") X(REACH_SQ, "reach_sq") X(REACH_SQRT, "reach_sqrt")              \
    X(REACH_CU_MASKED, "reach_cu_masked")                                                          \
    X(EVAL_SMALL, "eval_small") X(EVAL_F64, "eval_f64") X(EVAL_F32, "eval_f32")                    \
    X(EVAL_ARMTD_F64, "eval_armtd_f64") X(EVAL_ARMTD_F32, "eval_armtd_f32") X(EVAL_MX, "eval_mx")  \
    X(EVAL_CACHED, "eval_cached") X(EVAL_FULL_SCAN, "eval_full_scan")                              \
    X(TRIALS_SMALL, "trials_small") X(TRIALS_FULL, "trials_full") X(TRIALS_ALL, "trials_all")      \
    X(DA_LDS, "da_lds") X(DA_REGS, "da_regs")                                                      \
    X(IPM_ITER_SYNC, "ipm_iter_sync") X(IPM_ITER_TAIL, "ipm_iter_tail")                            \
    X(LS_SEQUENTIAL, "ls_sequential") X(LS_SPECULATIVE, "ls_speculative") X(LS_ONE_ROUND, "ls_one_round") \
    X(RESTO_INLINE, "resto_inline") X(RESTO_AFTER_LOOP, "resto_after_loop")                        \
    X(RESTO_ONE_ROUND, "resto_one_round") X(RESTO_ROUNDS, "resto_rounds")                          \
    X(RESTO_SECOND_STREAM, "resto_second_stream") X(RESTO_SOLVER_STREAM, "resto_solver_stream")    \
    X(IPM_RESTARTS, "ipm_restarts") X(SOLVE_MONOTONE, "solve_monotone") X(SOLVE_ADAPTIVE, "solve_adaptive") \
    X(PC_BUILDS, "pc_builds") X(PC_REGROWS, "pc_regrows") X(PC_FALLBACKS, "pc_fallbacks")          \
    X(CAND_SMALL, "cand_small") X(CAND_FULL, "cand_full") X(CAND_CHUNKS, "cand_chunks")            \
    X(MOTION_CHUNKS, "motion_chunks")                                                              \
    X(TRACK_ROW, "track_row") X(TRACK_ROW_REC, "track_row_rec") X(TRACK_ROW_EPISODE, "track_row_episode") \
    X(TRACK_SERIAL, "track_serial") X(TRACK_SERIAL_REC, "track_serial_rec")                        \
    X(TRACK_SERIAL_EPISODE, "track_serial_episode")                                                \
    X(SOLVE_QUALITY, "solve_quality") X(QF_SIGMA, "qf_sigma") X(HESS_LBFGS, "hess_lbfgs")
enum PathId {
#define X(id, name) PATH_##id,
    ARMOUR_PATHS(X)
#undef X
    PATH_N
};
static const char* const PATH_NAMES[] = {
#define X(id, name) name,
    ARMOUR_PATHS(X)
#undef X
};
static_assert(PATH_N == ARMOUR_PATH_COUNT, "include/armour_hip.h documents every path counter");

// capacity retry: a quarter of the workgroups, each with four workgroups' buffers
constexpr int RETRY_SCALE = 4;

// largest batch (jobs = worlds x T) that runs on the per-job engine; measured crossover, DESIGN.md §4
constexpr long JOB_ENGINE_JOBS = 5120;

// Every environment variable a planner reads when it is created, parsed once (INTEGRATION.md has the
// table). A planner keeps its settings for life; only three test hooks are read per call, at their
// call sites: ARMOUR_TRACK_KERNEL (the tracking entries), ARMOUR_DUMP_LANE (armour_get_reach_dump) and
// ARMOUR_PC_GROW_FAIL (ensure_plane_cache).
struct Settings {
    // g_planners sees this process's planners only; planners of other processes on the same GPU
    // (torchrun ranks folded onto one device, several armour_main servers) are declared with
    // ARMOUR_DEVICE_SHARED=1 (it only chooses the bundle kernel's shape)
    bool device_shared = false;
    // Concurrent planners share the GPU. The bundle reach kernel holds every CU it runs on for
    // its whole launch (persistent, 2 workgroups x 78 KB LDS per CU), so another planner's solver
    // kernels wait for it. ARMOUR_REACH_CU_RESERVE=k keeps k CUs out of the reach stream's CU mask
    // for them; ARMOUR_SOLVER_PRIORITY=1 gives the solver stream the highest queue priority.
    bool solver_priority = false;
    int cu_reserve = 0;
    int tail_worlds = 16;     // sync-free tail below this many running worlds (ARMOUR_TAIL_WORLDS, 0: off)
    int tail_search = 1;      // its line search (ARMOUR_TAIL_SEARCH): 0 rounds only, 1 adaptive, 2 always one round
    bool da_lds = true;       // wide grids take ipm_rows_DA_lds (ARMOUR_DA_REGS set: the register form)
    bool sq_off = false;      // ARMOUR_SQ_THRESHOLD=0: the sqrt reach kernels even where the squared threshold is verified
    // Engine choice per batch: batches of at most job_engine_jobs jobs take the per-job engine
    // (ARMOUR_JOB_ENGINE_JOBS); ARMOUR_ENGINE=job|lane forces one engine (0: by size, 1: job, 2: lane)
    int engine = 0;
    long job_engine_jobs = JOB_ENGINE_JOBS;
    bool job_narrow = false;  // ARMOUR_REACH_WIDE=0 (diagnostics): small batches on the 128-thread kernel too
    int reach_wg_per_cu = 0;  // ARMOUR_REACH_WG_PER_CU (diagnostics): fewer resident workgroups per CU than fit
    int engine_mode = 0;      // ARMOUR_ENGINE_MODE: per-job engine mode experiments (ReachArgs::mode)
    // ARMOUR_PROFILE_OPS set: the profile buffer exists; =1: per-op cycles/terms; =2: phase totals
    // (each distorts the other); =3: no op profiling; [start, end] wall clock (100 MHz) of every
    // bundle of the last launch after the op tables (bundle-engine load balance)
    bool profile = false;
    int profile_mode = 0;
    bool dump_ops = false;    // ARMOUR_DUMP_OPS set: op-by-op state of job 0 (bundle engine: of bundle 0)
    int lane_shape = -1;      // ARMOUR_LANE_SHAPE: 0 wide, 1 dense, -1 chosen per launch
    long lane_hcap = 1L << 16, lane_ccap = 1L << 17;  // ARMOUR_LANE_HCAP / _CCAP: bundle arena capacities
    bool eval_f32 = false;    // ARMOUR_EVAL_F32: fp32 constraint evaluation (tolerance study only)
    bool eval_full = false;   // ARMOUR_EVAL_FULL: always the full-capacity evaluation kernels
    int eval_skip = 0;        // ARMOUR_EVAL_SKIP: skips slicing (1) / collision rows (2), for part timings (NlpDev::diag)
    // ARMOUR_MU_STRATEGY: 0 monotone, 2 quality, 3 quality-floor, 1 any other value (adaptive), -1 unset:
    // IpmOpts' default; ARMOUR_QF_GRID, ARMOUR_LBFGS: the other two fields of armour_solver_options (-1 unset)
    int mu_strategy = -1;
    int qf_grid = -1, lbfgs = -1;
    int resto_max = -1;       // ARMOUR_RESTORATION: restoration phases per solve (0: none), -1 unset: the default
    bool plane_cache = true;  // ARMOUR_PLANE_CACHE=0: every evaluation on the full 36-plane scan
    int pc_k = PC_K;          // ARMOUR_PC_K (1..36): plane cache pool records per (link, obstacle) pair
    bool no_spec = false;     // ARMOUR_NO_SPEC set: sequential line-search rounds only
    bool resto_rounds = false;     // ARMOUR_RESTO_ROUNDS set: the restoration phase searches round by round
    bool resto_inline = true;      // ARMOUR_RESTO_INLINE=0: restoration phases after the interior-point loop
    bool resto_concurrent = true;  // ARMOUR_RESTO_CONCURRENT=0: inline phases on the solver stream
    // rows per block of the IPM row passes (ARMOUR_ROW_CHUNK overrides for diagnostics, a multiple of
    // 256). Measured at 327 worlds (tools/chunk_sweep.sh): 2048 rows 34.8 ms of NLP, 1024 34.2 ms, 512
    // 36.5 ms, 256 43.1 ms: shorter per-thread row loops help the latency-bound tail iterations until
    // the per-block reductions dominate. Fixed at creation: the partial-sum buffers are sized by it.
    int row_chunk = 1024;

    static Settings from_env() {
        auto num = [](const char* e, int dflt) { return e ? std::atoi(e) : dflt; };
        auto lnum = [](const char* e, long dflt) { return e ? std::atol(e) : dflt; };
        auto is = [](const char* e, const char* v) { return e && std::strcmp(e, v) == 0; };
        auto on = [&](const char* e) { return num(e, 0) != 0; };   // set to a non-zero number
        auto off = [&](const char* e) { return e && std::atoi(e) == 0; };  // set to 0 (or to no number)
        Settings s;
        s.device_shared = on(std::getenv("ARMOUR_DEVICE_SHARED"));
        s.solver_priority = on(std::getenv("ARMOUR_SOLVER_PRIORITY"));
        s.cu_reserve = num(std::getenv("ARMOUR_REACH_CU_RESERVE"), 0);
        s.tail_worlds = num(std::getenv("ARMOUR_TAIL_WORLDS"), 16);
        if (const char* e = std::getenv("ARMOUR_TAIL_SEARCH")) s.tail_search = is(e, "rounds") ? 0 : is(e, "one") ? 2 : 1;
        s.da_lds = !std::getenv("ARMOUR_DA_REGS");
        s.sq_off = off(std::getenv("ARMOUR_SQ_THRESHOLD"));
        const char* eng = std::getenv("ARMOUR_ENGINE");
        s.engine = is(eng, "job") ? 1 : is(eng, "lane") ? 2 : 0;
        s.job_engine_jobs = lnum(std::getenv("ARMOUR_JOB_ENGINE_JOBS"), JOB_ENGINE_JOBS);
        s.job_narrow = off(std::getenv("ARMOUR_REACH_WIDE"));
        s.reach_wg_per_cu = num(std::getenv("ARMOUR_REACH_WG_PER_CU"), 0);
        s.engine_mode = num(std::getenv("ARMOUR_ENGINE_MODE"), 0);
        s.profile = std::getenv("ARMOUR_PROFILE_OPS") != nullptr;
        s.profile_mode = num(std::getenv("ARMOUR_PROFILE_OPS"), 0);
        s.dump_ops = std::getenv("ARMOUR_DUMP_OPS") != nullptr;
        const char* sh = std::getenv("ARMOUR_LANE_SHAPE");
        s.lane_shape = is(sh, "wide") ? 0 : is(sh, "dense") ? 1 : -1;
        s.lane_hcap = lnum(std::getenv("ARMOUR_LANE_HCAP"), 1L << 16);
        s.lane_ccap = lnum(std::getenv("ARMOUR_LANE_CCAP"), 1L << 17);
        s.eval_f32 = on(std::getenv("ARMOUR_EVAL_F32"));
        s.eval_full = on(std::getenv("ARMOUR_EVAL_FULL"));
        s.eval_skip = num(std::getenv("ARMOUR_EVAL_SKIP"), 0);
        if (const char* e = std::getenv("ARMOUR_MU_STRATEGY"))
            s.mu_strategy = is(e, "monotone") ? 0 : is(e, "quality") ? 2 : is(e, "quality-floor") ? 3 : 1;
        if (const char* e = std::getenv("ARMOUR_QF_GRID")) s.qf_grid = std::atoi(e);
        if (const char* e = std::getenv("ARMOUR_LBFGS")) s.lbfgs = std::atoi(e);
        if (const char* e = std::getenv("ARMOUR_RESTORATION")) s.resto_max = std::max(std::atoi(e), 0);
        s.plane_cache = !off(std::getenv("ARMOUR_PLANE_CACHE"));
        s.pc_k = num(std::getenv("ARMOUR_PC_K"), PC_K);
        s.no_spec = std::getenv("ARMOUR_NO_SPEC") != nullptr;
        s.resto_rounds = std::getenv("ARMOUR_RESTO_ROUNDS") != nullptr;
        s.resto_inline = !off(std::getenv("ARMOUR_RESTO_INLINE"));
        s.resto_concurrent = !off(std::getenv("ARMOUR_RESTO_CONCURRENT"));
        const int c = num(std::getenv("ARMOUR_ROW_CHUNK"), 1024);
        s.row_chunk = (c >= 256 && c % 256 == 0) ? c : 1024;
        return s;
    }
};

struct armour_planner {
    armour_config cfg;
    Settings set;
    int T = 0, NJ = 0, Omax = 0, Wmax = 0, ncu = 0, reach_grid = 0;
    RobotParams rp;
    RobotParams* d_rp = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t rstream = nullptr;   // reach phase (the planner's stream unless CUs are reserved)
    int reach_cus = 0;               // CUs the reach stream may use
    hipEvent_t ev[6];
    hipEvent_t tev[2];        // sync-free solver tail: end of iteration it (parity it & 1)
    // reach program (ProgramBuilder::ops) on the device
    Op* d_prog = nullptr;
    int* d_slot_off = nullptr;
    JrsJoint* d_jrs = nullptr;
    int nops = 0, nslots = 0;
    unsigned long long* d_bytes = nullptr;
    unsigned long long* d_prof = nullptr;  // per-op [cycles, terms] (Settings::profile)
    double* d_dump = nullptr;              // op-by-op state of job 0 (Settings::dump_ops)
    double last_kernel_ms = 0, last_bytes = 0;
    double last_span_ms = -1;  // device-clock execution span of the last batch's first reach launch (armour_get_reach_span)
    int wall_khz = 0;          // hipDeviceAttributeWallClockRate
    unsigned long long* d_occ = nullptr;   // [8] reach capacity use of the last launch (ReachCounters)
    unsigned* d_done = nullptr;            // workgroups finished in the current reach launch
    long long* h_sum = nullptr;            // mapped host: reach counters published by the last workgroup
    ReachCounters rc{};                    // (reach_kernel.hip)
    long long reach_seq = 0;               // sequence number of the last reach launch (ReachCounters::seq)
    int* d_wlist = nullptr;                // [max_worlds] worlds of a capacity retry
    int last_retried = 0, last_failed = 0;
    std::vector<int> world_err;            // per world of the last batch: 0 or ARMOUR_E_CAPACITY
    // inputs
    double *q0 = nullptr, *qd0 = nullptr, *qdd0 = nullptr, *qdes = nullptr, *obs = nullptr, *xin = nullptr;
    // reach
    ReachOut ro;
    ReachArgs ra;
    // bundle engine (lane_kernel.hip): default; ARMOUR_ENGINE=job selects the per-job reach_kernel
    bool lane_engine = true;  // the last batch ran on the bundle engine
    bool has_lane = false, has_job = false;  // engines with buffers
    bool armtd = false;       // the ARMTD comparison planner (armour_create_armtd)
    double* d_tables = nullptr;  // ARMTD: offline JRS tables [W][NF][6][T]
    long job_max = 0;         // batches of at most this many jobs (W x T) run on the per-job engine
    bool job_fits = true;     // the reach program's payload pool fits the per-job engine's LDS
    // largest link / torque k-monomial counts of the last reach (both engines record them in
    // occ[3], occ[4], published with the error flags), and the first launch's occupancy
    unsigned long long h_occ[8] = {};
    int mono_max[2] = {CAP_LM, CAP_UM};
    int lane_grid = 0;        // workgroups with an arena: the larger (dense) shape's resident set
    int lane_slots[2] = {0, 0};  // resident bundle workgroups of the wide / dense kernel shape
    bool sq = true;           // reach kernels decide keep / prune on squared norms (rp.simplify_sq_valid)
    int last_shape = 0;       // shape of the last first launch (a capacity retry uses it too)
    int dev = 0;              // the planner's device
    bool counted = false;     // counted in g_planners[dev]
    lane::LaneArgs la;

    // nlp
    NlpDev d;
    OptDev od{};              // the optional solver configurations (solver_options_apply, init_solver)
    int* feas = nullptr;
    int* h_flags = nullptr;   // pinned host, mapped (NlpDev::flags)
    int* d_lists = nullptr;   // [6][max_worlds] active-world lists of the solver
    bool spec = true;         // speculative line-search rounds (ARMOUR_NO_SPEC: sequential only)
    bool spec_all = true;     // the sync-free tail's one-round line search (eval_trials_all, ipm_world_Cs_all)
    bool resto_spec = false;  // the restoration phase's one-round search (eval_trials_all, resto_world_Vs)
    bool resto_inline = true; // restoration phases inside the interior-point loop (ARMOUR_RESTO_INLINE=0: after it)
    // In the sync-free tail the inline restoration phase runs on a second stream, concurrently with
    // the next interior-point iteration (ARMOUR_RESTO_CONCURRENT=0: on the solver stream): its worlds
    // are others than the interior point's, and its speculative rows start after the tail's
    // (resto_soff rows into gs / fs / partial_s), so only the append list RL is shared; ipm_loop
    // orders its publication (ev_ip, ev_pub) and joins the streams at the loop's end (ev_rend)
    bool resto_conc = false;
    hipStream_t rstream2 = nullptr;
    hipEvent_t ev_ip = nullptr, ev_pub = nullptr, ev_rend = nullptr;
    size_t resto_soff = 0;
    double *gs = nullptr, *fs = nullptr, *partial_s = nullptr;  // the speculative rows (spec_view)
    int K0 = 0;                                                 // trials after round 0, max_ls - 1
    WorldState* h_ws = nullptr;
    double* h_f = nullptr;
    int* h_feas = nullptr;
    unsigned* h_pcnext = nullptr;  // pinned: the plane cache pool records the last build needed
    // state of the last batch
    int W = 0, O = 0;          // (a mixed batch: O is its largest count)
    std::vector<int> Ow;       // obstacle count of each world of the last batch
    int* d_Ow = nullptr;       // [max_worlds] device copy of a mixed batch's counts (NlpDev::Ow)
    bool reached = false, planned = false, evaluated = false;  // evaluated: slot 0 holds armour_eval_constraints' point
    // armour_eval_candidates: buffers of its own for max_worlds x cand.cap candidates (allocated on
    // first use, regrown when a call brings more candidates per world)
    CandDev cd{};
    GrowSet cand;
    // the execution layer (the structs above)
    MotionCheck motion;
    Rollouts track;
    TrueArmCheck tracked;
    Episode ep;
    TrackedEpisode ept;
    Roadmap roadmap;
    std::vector<void*> allocs;
    long long paths[PATH_N] = {};  // the path census (armour_get_path_counts)
    void took(PathId c, long long n = 1) { paths[c] += n; }

    template <class T>
    int alloc(T** p, size_t n) {
        hipError_t e = dalloc(p, n);
        if (e != hipSuccess) return fail(ARMOUR_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        allocs.push_back((void*)*p);
        return 0;
    }
};

// planner_init, phase 1: the device, the robot, the streams and events
static int init_device(armour_planner* p, const armour_robot* robot) {
    const armour_config* cfg = &p->cfg;
    if (cfg->device >= 0) HIPCK(hipSetDevice(cfg->device));
    int dev = 0;
    HIPCK(hipGetDevice(&dev));
    p->dev = dev;
    g_planners[dev & 63]++;
    p->counted = true;
    HIPCK(hipDeviceGetAttribute(&p->ncu, hipDeviceAttributeMultiprocessorCount, dev));
    if (hipDeviceGetAttribute(&p->wall_khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) p->wall_khz = 0;
    if (robot) {
        if (!robot_from_tables(*robot, p->rp))
            return fail(ARMOUR_E_ARG, "invalid robot tables (num_joints 7..9, actuated joints first, M_min > 0, K > 0)");
    } else {
        kinova_gen3(p->rp);
    }
    p->T = cfg->num_time_steps;
    p->NJ = p->rp.num_joints;
    p->Omax = cfg->max_obstacles;
    p->Wmax = cfg->max_worlds;
    int lo = 0, hi = 0;
    HIPCK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCK(hipStreamCreateWithPriority(&p->stream, hipStreamNonBlocking, p->set.solver_priority ? hi : 0));
    const int reserve = p->set.cu_reserve;
    p->reach_cus = p->ncu;
    if (reserve > 0 && reserve < p->ncu) {
        std::vector<uint32_t> mask((p->ncu + 31) / 32, 0u);
        for (int c = 0; c < p->ncu; c++) mask[c / 32] |= 1u << (c % 32);
        for (int i = 0; i < reserve; i++) {
            const int c = (int)((long)i * p->ncu / reserve);
            mask[c / 32] &= ~(1u << (c % 32));
        }
        HIPCK(hipExtStreamCreateWithCUMask(&p->rstream, (uint32_t)mask.size(), mask.data()));
        p->reach_cus = p->ncu - reserve;
    } else {
        p->rstream = p->stream;
    }
    for (int i = 0; i < 6; i++) HIPCK(hipEventCreate(&p->ev[i]));
    for (int i = 0; i < 2; i++) HIPCK(hipEventCreateWithFlags(&p->tev[i], hipEventDisableTiming));
    return 0;
}

// planner_init, phase 2: the robot and input arrays, the reach outputs and program, and the
// workspaces of the engines this planner can need
static int init_reach(armour_planner* p) {
    const Settings& set = p->set;
    const int dev = p->dev;
    const int T = p->T, NJ = p->NJ, Om = p->Omax > 0 ? p->Omax : 1, Wm = p->Wmax;
    int rc = 0;
    if ((rc = p->alloc(&p->d_rp, 1))) return rc;
    HIPCK(hipMemcpy(p->d_rp, &p->rp, sizeof(RobotParams), hipMemcpyHostToDevice));
    {
        // the simplify threshold on squared norms, found and verified on the device once per robot
        // (pz_engine.h SqThr). Not verified, or ARMOUR_SQ_THRESHOLD=0: the sqrt kernels run.
        hipLaunchKernelGGL(sq_threshold_kernel, dim3(1), dim3(1), 0, nullptr, p->d_rp);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpy(&p->rp, p->d_rp, sizeof(RobotParams), hipMemcpyDeviceToHost));
        if (set.sq_off && p->rp.simplify_sq_valid) {
            p->rp.simplify_sq_valid = 0;
            HIPCK(hipMemcpy(p->d_rp, &p->rp, sizeof(RobotParams), hipMemcpyHostToDevice));
        }
        p->sq = p->rp.simplify_sq_valid != 0;
    }
    if ((rc = p->alloc(&p->q0, (size_t)Wm * NF)) || (rc = p->alloc(&p->qd0, (size_t)Wm * NF)) ||
        (rc = p->alloc(&p->qdd0, (size_t)Wm * NF)) || (rc = p->alloc(&p->qdes, (size_t)Wm * NF)) ||
        (rc = p->alloc(&p->xin, (size_t)Wm * NF)) || (rc = p->alloc(&p->obs, (size_t)Wm * Om * 12)))
        return rc;
    // reach outputs
    const size_t jobs = (size_t)Wm * T;
    ReachOut& ro = p->ro;
    ro.T = T;
    ro.NJ = NJ;
    if ((rc = p->alloc(&ro.link_hash, jobs * NJ * CAP_LM)) || (rc = p->alloc(&ro.link_coef, jobs * NJ * CAP_LM * 3)) ||
        (rc = p->alloc(&ro.link_cnt, jobs * NJ)) || (rc = p->alloc(&ro.link_center, jobs * NJ * 3)) ||
        (rc = p->alloc(&ro.link_rad, jobs * NJ * 3)) || (rc = p->alloc(&ro.link_gens, jobs * NJ * 18)) ||
        (rc = p->alloc(&ro.tq_hash, jobs * NF * CAP_UM)) || (rc = p->alloc(&ro.tq_coef, jobs * NF * CAP_UM)) ||
        (rc = p->alloc(&ro.tq_cnt, jobs * NF)) || (rc = p->alloc(&ro.tq_center, jobs * NF)) ||
        (rc = p->alloc(&ro.tq_rad, jobs * NF)) || (rc = p->alloc(&ro.torque_radius, jobs * NF)) ||
        (rc = p->alloc(&ro.err, (size_t)Wm)))
        return rc;
    // reach program
    ProgramBuilder pb;
    pb.build(p->rp, p->armtd);
    int pool = 0;
    const std::vector<int> off = pb.slot_offsets(&pool);
    // the bundle engine's payload pool lives in HBM, sized below; the per-job engine's in LDS
    // (POOL_DOUBLES): a robot whose program does not fit it (Fetch: 8 links) runs on the
    // bundle engine only
    p->job_fits = pool <= POOL_DOUBLES;
    if (pb.nslots > MAX_SLOTS || (set.engine == 1 && pool > POOL_DOUBLES)) {
        char buf[200];
        std::snprintf(buf, sizeof(buf), "reach program needs %d handle slots (kernel: %d) and %d payload doubles (per-job engine: %d)",
                      pb.nslots, MAX_SLOTS, pool, POOL_DOUBLES);
        return fail(ARMOUR_E_CAPACITY, buf);
    }
    p->nops = (int)pb.ops.size();
    p->nslots = pb.nslots;
    if ((rc = p->alloc(&p->d_prog, pb.ops.size())) || (rc = p->alloc(&p->d_bytes, 1)) ||
        (rc = p->alloc(&p->d_slot_off, off.size())))
        return rc;
    HIPCK(hipMemcpy(p->d_prog, pb.ops.data(), sizeof(Op) * pb.ops.size(), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(p->d_slot_off, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice));
    if (set.profile) {
        const size_t nbt = 2 * (((size_t)p->Wmax * p->T + lane::LG - 1) / lane::LG);
        const size_t n = 2 * pb.ops.size() + 16 + 8 * OP_NCODES + nbt;
        if ((rc = p->alloc(&p->d_prof, n))) return rc;
        HIPCK(hipMemset(p->d_prof, 0, sizeof(unsigned long long) * n));
    }
    // reach workspace: four resident workgroups per CU, each with a private arena
    {
        int fit = REACH_WG_PER_CU;  // as many as the CU's LDS holds (a persistent grid larger than
        {                           // the resident set would run its last workgroups one job late)
            hipFuncAttributes fa{};
            int lds_cu = 0;
            HIPCK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&reach_kernel<REACH_THREADS>)));
            HIPCK(hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev));
            if (fa.sharedSizeBytes > 0) fit = std::max(1, std::min<int>(fit, (int)(lds_cu / fa.sharedSizeBytes)));
        }
        const int per = set.reach_wg_per_cu;
        p->reach_grid = (per >= 1 && per <= fit ? per : fit) * p->ncu;
    }
    // Engine choice per batch. The bundle engine (lane_kernel.hip) runs 64 jobs per workgroup and
    // fills the chip from ~2 x CUs x 64 jobs on, but one bundle takes ~18 ms whatever its size. The
    // per-job engine (reach_kernel.hip) runs one job per workgroup, ~4 ms per round of up to
    // 4 x CUs jobs. So small batches (the drop-in's single plan) take the per-job engine:
    // batches of at most job_max jobs (ARMOUR_JOB_ENGINE_JOBS; ARMOUR_ENGINE=job|lane forces one).
    p->job_max = set.job_engine_jobs;
    if (set.engine == 1) p->job_max = (long)Wm * T;
    if (set.engine == 2 || !p->job_fits) p->job_max = 0;
    p->has_job = p->job_max > 0;
    p->has_lane = (long)Wm * T > p->job_max;
    if (p->has_job) p->reach_grid = (int)std::min<long>(p->reach_grid, std::min<long>(p->job_max, (long)Wm * T));
    ReachArgs& ra = p->ra;
    ra.prog = p->d_prog;
    ra.nops = p->nops;
    ra.slot_off = p->d_slot_off;
    ra.nslots = p->nslots;
    ra.bytes = p->d_bytes;
    ra.prof = set.profile_mode == 2 ? nullptr : p->d_prof;
    ra.phase = set.profile_mode == 2 ? p->d_prof + 2 * p->nops : nullptr;
    ra.mode = set.engine_mode;
    ra.dump = nullptr;
    if ((rc = p->alloc(&p->d_jrs, jobs * NF)) || (rc = p->alloc(&p->d_occ, 8)) || (rc = p->alloc(&p->d_done, 1))) return rc;
    HIPCK(hipMemset(p->d_done, 0, sizeof(unsigned)));
    {
        long long* dsum = nullptr;
        HIPCK(hipHostMalloc((void**)&p->h_sum, sizeof(long long) * (RSUM_ERR + (size_t)Wm), hipHostMallocMapped));
        HIPCK(hipHostGetDevicePointer((void**)&dsum, p->h_sum, 0));
        p->rc = ReachCounters{p->d_bytes, p->d_occ, p->d_done, dsum, 0};
        p->h_sum[RSUM_SEQ] = 0;
        ra.rc = p->rc;
        ra.ntq = p->armtd ? 0 : NF;
    }
    if (p->has_job) {
        ra.arena_cap = 1 << 17;
        ra.gcap = 1 << 15;
        if ((rc = p->alloc(&ra.arena_h, (size_t)p->reach_grid * ra.arena_cap)) ||
            (rc = p->alloc(&ra.arena_c, (size_t)p->reach_grid * ra.arena_cap * 3)) ||
            (rc = p->alloc(&ra.gkh, (size_t)p->reach_grid * ra.gcap)) || (rc = p->alloc(&ra.gki, (size_t)p->reach_grid * ra.gcap)) ||
            (rc = p->alloc(&ra.gkp, (size_t)p->reach_grid * ra.gcap)) ||
            (rc = p->alloc(&ra.gout, (size_t)p->reach_grid * ra.gcap * 9)))
            return rc;
    }
    if (p->has_lane) {
        // LANE_WG_PER_CU resident bundle workgroups per CU (as many as the CU's LDS holds), each
        // with its own arena; sizes from the measured per-job use (~16.5k monomials) times the union
        // inflation, with margin
        lane::LaneArgs& la = p->la;
        const long bundles = ((long)Wm * T + lane::LG - 1) / lane::LG;
        {
            int lds_cu = 0;
            HIPCK(hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev));
            const void* fn[2] = {reinterpret_cast<const void*>(&lane::lane_reach_kernel<lane::LaneWide>),
                                 reinterpret_cast<const void*>(&lane::lane_reach_kernel<lane::LaneDense>)};
            const int want[2] = {lane::LaneWide::PER_CU, lane::LaneDense::PER_CU};
            for (int k = 0; k < 2; k++) {
                hipFuncAttributes fa{};
                HIPCK(hipFuncGetAttributes(&fa, fn[k]));
                int per_cu = want[k];
                if (fa.sharedSizeBytes > 0) per_cu = std::max(1, std::min<int>(per_cu, (int)(lds_cu / fa.sharedSizeBytes)));
                p->lane_slots[k] = p->reach_cus * per_cu;
            }
        }
        const long slots = std::max(p->lane_slots[0], p->lane_slots[1]);
        p->lane_grid = (int)(bundles < slots ? bundles : slots);
        la.hcap = set.lane_hcap;
        la.ccap = set.lane_ccap;
        la.gcap = 1 << 15;
        la.pool_rows = pool + 9 + 2 * NF;  // + the torque-radius scratch rows (lane_kernel.hip)
        // buffers of at least RETRY_SCALE workgroups, so even a one-world batch has a capacity retry
        const size_t G = (size_t)std::max(p->lane_grid, RETRY_SCALE), LGs = lane::LG;
        if ((rc = p->alloc(&la.pool, G * la.pool_rows * LGs)) || (rc = p->alloc(&la.arena_h, G * la.hcap)) ||
            (rc = p->alloc(&la.arena_m, G * la.hcap)) || (rc = p->alloc(&la.arena_c, G * la.ccap * LGs)) ||
            (rc = p->alloc(&la.gkh, G * la.gcap)) || (rc = p->alloc(&la.gki, G * la.gcap)) ||
            (rc = p->alloc(&la.gkp, G * (la.gcap + 1))) || (rc = p->alloc(&la.ggp, G * (la.gcap + 1))))
            return rc;
        if ((rc = p->alloc(&p->d_wlist, (size_t)Wm))) return rc;
        la.occ = p->d_occ;
        la.rc = p->rc;
        la.wlist = nullptr;
        la.nlist = 0;
        la.prog = p->d_prog;
        la.nops = p->nops;
        la.slot_off = p->d_slot_off;
        la.nslots = p->nslots;
        la.bytes = p->d_bytes;
        const bool btimes = set.profile_mode == 3;
        la.prof = btimes ? nullptr : p->d_prof;
        la.btime = btimes ? p->d_prof + 2 * p->nops + 16 + 8 * OP_NCODES : nullptr;
        la.dump = nullptr;
    }
    if (set.dump_ops) {
        // the op dump follows the bundle engine when it exists (one column per job of bundle 0)
        const size_t n = (size_t)p->nops * DUMP_W * (p->has_lane ? lane::LG : 1);
        if ((rc = p->alloc(&p->d_dump, n))) return rc;
        HIPCK(hipMemset(p->d_dump, 0, sizeof(double) * n));
        (p->has_lane ? p->la.dump : ra.dump) = p->d_dump;
    }
    return 0;
}

// armour_solver_options: the ranges (naming the field), and the options into the solver's own. The
// sigma table is formed here with std::pow, as oracle/src/ipm.cpp forms it, so the kernels read the
// oracle's bits. Nothing else depends on the options: no buffer, no loop variant.
static int solver_options_check(const armour_planner* p, const armour_solver_options* o) {
    if (o->mu_strategy < 0 || o->mu_strategy > 3) return fail(ARMOUR_E_ARG, "solver options: mu_strategy must lie in 0 .. 3");
    if (o->qf_grid < 2 || o->qf_grid > QF_GMAX) return fail(ARMOUR_E_ARG, "solver options: qf_grid must lie in 2 .. 32");
    if (o->lbfgs_history < 0 || o->lbfgs_history > LB_MAX)
        return fail(ARMOUR_E_ARG, "solver options: lbfgs_history must lie in 0 .. 6");
    const bool dflt = o->mu_strategy <= 1 && o->lbfgs_history == 0;
    if (p->set.eval_f32 && !dflt)
        return fail(ARMOUR_E_ARG, "solver options: strategies 2, 3 and lbfgs_history are not available with the fp32 study (ARMOUR_EVAL_F32)");
    return 0;
}
static void solver_options_apply(armour_planner* p, const armour_solver_options& o) {
    p->d.opt.mu_strategy = o.mu_strategy;
    p->od.qf_grid = o.qf_grid;
    p->od.lbfgs_history = o.lbfgs_history;
    for (int k = 0; k < QF_GMAX; k++)
        p->od.sig[k] = std::pow(10.0, -6.0 + 8.0 * std::min(k, o.qf_grid - 1) / (o.qf_grid - 1));
}

// planner_init, phase 3: the solver's arrays, its options and the loop variants it may take
static int init_solver(armour_planner* p) {
    const Settings& set = p->set;
    const int T = p->T, NJ = p->NJ, Om = p->Omax > 0 ? p->Omax : 1, Wm = p->Wmax;
    const size_t jobs = (size_t)Wm * T;
    int rc = 0;
    NlpDev& d = p->d;
    d.rp = p->d_rp;
    d.diag = set.eval_skip;
    d.T = T;
    d.NJ = NJ;
    d.ro = p->ro;
    if (p->cfg.max_iter > 0) d.opt.max_iter = p->cfg.max_iter;
    {
        // the solver configuration the environment asks for (armour_main and armtd_main have no other
        // way in), checked as armour_set_solver_options checks it
        armour_solver_options so{d.opt.mu_strategy, 16, 0};
        if (set.mu_strategy >= 0) so.mu_strategy = set.mu_strategy;
        if (set.qf_grid >= 0) so.qf_grid = set.qf_grid;
        if (set.lbfgs >= 0) so.lbfgs_history = set.lbfgs;
        if ((rc = solver_options_check(p, &so))) return rc;
        solver_options_apply(p, so);
    }
    if (set.resto_max >= 0) d.opt.resto_max = set.resto_max;        // restoration phases per solve (0: none)
    d.armtd = p->armtd ? 1 : 0;
    d.nt = p->armtd ? 0 : NF * T;
    d.krange = nullptr;
    if (p->armtd) {
        d.opt.tol = 1e-7;  // IPOPT_OPTIMIZATION_TOLERANCE (ACMP/Parameters.h:42)
        double* kr = nullptr;
        if ((rc = p->alloc(&p->d_tables, (size_t)Wm * NF * 6 * T)) || (rc = p->alloc(&kr, (size_t)Wm * NF))) return rc;
        d.krange = kr;
    }
    d.lcs = (long)(jobs * NJ * 3);
    const size_t mmax = (size_t)d.nt + (size_t)T * NJ * Om + NF * 4;
    const size_t Rmax = mmax + NF;
    if ((rc = p->alloc(&d.L, Wm * Rmax)) || (rc = p->alloc(&d.U, Wm * Rmax)) || (rc = p->alloc(&d.g, 2 * Wm * mmax)) ||
        (rc = p->alloc(&d.J, 2 * Wm * mmax * NF)) || (rc = p->alloc(&d.f, 2 * (size_t)Wm)) ||
        (rc = p->alloc(&d.grad, 2 * (size_t)Wm * NF)) || (rc = p->alloc(&d.link_c, 3 * jobs * NJ * 3)))
        return rc;
    d.njn = (long)(jobs * NJ * Om * 3);
    d.njd = (long)(jobs * NJ * NF * 3);
    if ((rc = p->alloc(&d.jn, 2 * (size_t)d.njn)) || (rc = p->alloc(&d.jd, 2 * (size_t)d.njd))) return rc;
    double** rowbufs[] = {&d.slo, &d.shi, &d.zlo, &d.zhi, &d.dslo, &d.dshi};
    for (double** b : rowbufs)
        if ((rc = p->alloc(b, Wm * Rmax))) return rc;
    d.chunk = set.row_chunk;
    const int nblk_max = (int)((Rmax + d.chunk - 1) / d.chunk);
    if ((rc = p->alloc(&d.partial, (size_t)Wm * nblk_max * KA)) || (rc = p->alloc(&d.partial2, (size_t)Wm * nblk_max * KA2)) ||
        (rc = p->alloc(&d.ws, (size_t)Wm)) ||
        (rc = p->alloc(&p->feas, (size_t)Wm)))
        return rc;
    // the optional solver configurations' state (armour_solver_options), beside ws: per world the
    // QfState, the free-mode filter sized by the iteration cap, and the sigma search's sums
    OptDev& od = p->od;
    od.gf_cap = d.opt.max_iter + 1;
    if ((rc = p->alloc(&od.qs, (size_t)Wm)) || (rc = p->alloc(&od.gf, (size_t)Wm * 2 * od.gf_cap)) ||
        (rc = p->alloc(&od.qpart, (size_t)Wm * QP)))
        return rc;
    // the solver's counts for the host live in mapped host memory (NlpDev::flags, FlagSlot): kernels
    // store them, the host reads them after an event or a synchronised round (no fill or copy per round)
    HIPCK(hipHostMalloc((void**)&p->h_flags, FLAG_LEN * sizeof(int), hipHostMallocMapped));
    HIPCK(hipHostGetDevicePointer((void**)&d.flags, p->h_flags, 0));
    // active-world lists: two per iteration (ping-pong), two per line-search round
    // (+ two for the restoration phases inside the interior-point loop)
    if ((rc = p->alloc(&p->d_lists, 6 * (size_t)Wm)) || (rc = p->alloc(&d.cnt, CNT_LEN))) return rc;
    // certified plane cache: one record pool sized for PC_K records per (link, obstacle) pair of
    // every (world, t) (ARMOUR_PC_K, 1..36); each (world, t) block takes its records from the pool
    // with one atomic (pcbase). The survey workload keeps 5.3 planes per pair on average. A build
    // that needs more than the pool is repeated on a larger pool (ensure_plane_cache); if that pool
    // cannot be allocated, the cache is not marked ready and the solve runs on the full scan
    // (bitwise the same results, slower). Round 4 reserved all 36 per pair (42 MB per world at
    // T = 100, O = 20), which capped the batch a GPU can hold. The pool counter is 32-bit: a batch
    // whose 36 records per pair could exceed it does not use the cache.
    d.pcache = set.plane_cache && (double)COMB * NJ * std::max(Om, 1) * (double)jobs < 4294967295.0;
    d.pcready = 0;
    d.pc_pool = std::max(1L, (long)std::min(std::max(set.pc_k, 1), COMB) * NJ * std::max(Om, 1) * (long)jobs);
    if (d.pcache && ((rc = p->alloc(&d.pc, 5 * (size_t)d.pc_pool)) || (rc = p->alloc(&d.pcp, (size_t)d.pc_pool)) ||
                     (rc = p->alloc(&d.pcoff, jobs * NJ * (size_t)Om)) || (rc = p->alloc(&d.pcok, jobs)) ||
                     (rc = p->alloc(&d.pcbase, jobs)) || (rc = p->alloc(&d.pcnext, 1))))
        return rc;
    if (d.pcache) {
        HIPCK(hipMemset(d.pcnext, 0, sizeof(unsigned)));
        HIPCK(hipHostMalloc((void**)&p->h_pcnext, sizeof(unsigned)));
        p->rc.pc_next = d.pcnext;
        p->ra.rc.pc_next = d.pcnext;
        p->la.rc.pc_next = d.pcnext;
    }
    // speculative line-search slots (values only): every world x (max_ls - 1) trials. The speculative
    // round reads the plane cache (ARMOUR planner, fp64); otherwise the rounds run one by one.
    p->K0 = d.opt.max_ls - 1;
    p->spec = !set.no_spec && p->K0 > 0 && p->K0 <= EV_MAXK && d.pcache && !p->armtd && !set.eval_f32;
    // The sync-free tail may search all max_ls trials of its (at most tail_worlds) running worlds in
    // one round (run_solver)
    p->spec_all = p->spec && p->set.tail_search > 0 && (p->K0 + 1) * NJ * Om <= UB_FULL;
    // the restoration phase searches all max_ls trials of up to every world at once
    p->resto_spec = p->spec && d.opt.resto_max > 0 && d.opt.max_ls <= EV_MAXK + 1 && d.opt.max_ls * NJ * Om <= UB_FULL &&
                    !set.resto_rounds;
    p->resto_inline = p->resto_spec && set.resto_inline;
    p->resto_conc = p->resto_inline && p->spec_all && set.tail_worlds > 0 && set.resto_concurrent;
    if (p->resto_conc) {
        HIPCK(hipStreamCreateWithFlags(&p->rstream2, hipStreamNonBlocking));
        HIPCK(hipEventCreateWithFlags(&p->ev_ip, hipEventDisableTiming));
        HIPCK(hipEventCreateWithFlags(&p->ev_pub, hipEventDisableTiming));
        HIPCK(hipEventCreateWithFlags(&p->ev_rend, hipEventDisableTiming));
    }
    if (p->spec) {
        // rows of the speculative slots: the interior point's rounds use the first Wm x K (the
        // sync-free tail's one-round search the first nall); a restoration phase Wm x max_ls, after
        // the tail's rows when it runs concurrently with the tail (resto_soff)
        const size_t nall = p->spec_all ? (size_t)std::min(Wm, std::max(p->set.tail_worlds, 0)) * (p->K0 + 1) : 0;
        p->resto_soff = p->resto_conc ? nall : 0;
        const size_t nres = p->resto_spec ? (size_t)Wm * d.opt.max_ls + p->resto_soff : 0;
        const size_t ns = std::max(std::max((size_t)Wm * p->K0, nall), nres);
        if ((rc = p->alloc(&p->gs, ns * mmax)) || (rc = p->alloc(&p->fs, ns)) || (rc = p->alloc(&p->partial_s, ns * nblk_max * KA)))
            return rc;
    }
    HIPCK(hipMemset(d.cnt, 0, CNT_LEN * sizeof(unsigned)));
    HIPCK(hipHostMalloc((void**)&p->h_ws, Wm * sizeof(WorldState)));
    HIPCK(hipHostMalloc((void**)&p->h_f, 2 * Wm * sizeof(double)));
    HIPCK(hipHostMalloc((void**)&p->h_feas, Wm * sizeof(int)));
    d.q0 = p->q0;
    d.qd0 = p->qd0;
    d.qdd0 = p->qdd0;
    d.qdes = p->qdes;
    d.obs = p->obs;
    d.Ow = nullptr;
    return p->alloc(&p->d_Ow, (size_t)Wm);
}

static int planner_init(armour_planner* p, const armour_config* cfg, const armour_robot* robot, bool armtd) {
    p->cfg = *cfg;
    p->armtd = armtd;
    p->set = Settings::from_env();
    if (!robot && cfg->robot != 0) return fail(ARMOUR_E_ARG, "unknown robot id");
    if (cfg->num_time_steps <= 0 || (cfg->num_time_steps % 2) != 0)
        return fail(ARMOUR_E_ARG, "num_time_steps must be a positive even number (KPR/Parameters.h:16)");
    if (cfg->max_obstacles < 0 || cfg->max_obstacles > MAX_OBS || cfg->max_worlds <= 0)
        return fail(ARMOUR_E_ARG, "bad max_obstacles (0..40, MAX_OBSTACLE_NUM) / max_worlds");
    int rc = 0;
    if ((rc = init_device(p, robot)) || (rc = init_reach(p)) || (rc = init_solver(p))) return rc;
    return 0;
}

// The input domain of a world (include/armour_hip.h, armour_check_world): every value finite and the
// angles within ARMOUR_MAX_ABS_ANGLE. Host-side, O(O) per world; every planning and reach entry runs it
// on every world before anything is copied or launched (wrap_to_pi's loop in nlp_kernels.hip is
// bounded only for such values).
static int check_values(const char* field, const double* v, int n, double max_abs) {
    for (int i = 0; i < n; i++) {
        char buf[160];
        if (!std::isfinite(v[i])) {
            std::snprintf(buf, sizeof(buf), "%s[%d] is not finite", field, i);
            return fail(ARMOUR_E_ARG, buf);
        }
        if (max_abs > 0 && std::fabs(v[i]) > max_abs) {
            std::snprintf(buf, sizeof(buf), "%s[%d] = %g lies outside +-%g (ARMOUR_MAX_ABS_ANGLE)", field, i, v[i], max_abs);
            return fail(ARMOUR_E_ARG, buf);
        }
    }
    return 0;
}
static int check_obstacles(int n, const double* obstacles, int max_obstacles) {
    if (n < 0 || n > max_obstacles) return fail(ARMOUR_E_ARG, "num_obstacles exceeds max_obstacles");
    if (n > 0 && !obstacles) return fail(ARMOUR_E_ARG, "null obstacles");
    return n > 0 ? check_values("obstacles", obstacles, n * ARMOUR_OBSTACLE_DOUBLES, 0.0) : 0;
}
static int check_world(const armour_world* w, int max_obstacles) {
    if (!w) return fail(ARMOUR_E_ARG, "null world");
    int rc;
    if ((rc = check_values("q0", w->q0, NF, ARMOUR_MAX_ABS_ANGLE))) return rc;
    if ((rc = check_values("qd0", w->qd0, NF, 0.0))) return rc;
    if ((rc = check_values("qdd0", w->qdd0, NF, 0.0))) return rc;
    if ((rc = check_values("q_des", w->q_des, NF, ARMOUR_MAX_ABS_ANGLE))) return rc;
    return check_obstacles(w->num_obstacles, w->obstacles, max_obstacles);
}
static int check_armtd_world(const armour_armtd_world* w, int max_obstacles, int T) {
    if (!w) return fail(ARMOUR_E_ARG, "null world");
    if (T <= 0) return fail(ARMOUR_E_ARG, "num_time_steps must be positive");
    if (!w->jrs_tables) return fail(ARMOUR_E_ARG, "null jrs_tables");
    int rc;
    if ((rc = check_values("q0", w->q0, NF, ARMOUR_MAX_ABS_ANGLE))) return rc;
    if ((rc = check_values("qd0", w->qd0, NF, 0.0))) return rc;
    if ((rc = check_values("q_des", w->q_des, NF, ARMOUR_MAX_ABS_ANGLE))) return rc;
    if ((rc = check_values("k_range", w->k_range, NF, 0.0))) return rc;
    if ((rc = check_values("jrs_tables", w->jrs_tables, NF * 6 * T, 0.0))) return rc;
    return check_obstacles(w->num_obstacles, w->obstacles, max_obstacles);
}

// The batch's worlds, checked (check_world) and copied to the device. A uniform batch: every world
// with the same obstacle count O. A mixed batch: every world with its own count, 0 .. max_obstacles;
// the obstacle array is padded to the batch's largest count (the stride of every per-world slab, as
// O is for a uniform batch) and the counts go to the device (NlpDev::Ow); the solver then runs the
// _mx kernels.
static int upload_worlds(armour_planner* p, int W, const armour_world* worlds, bool mixed) {
    if (mixed && p->armtd) return fail(ARMOUR_E_ARG, "mixed batches are not available on an ARMTD planner");
    if (mixed && p->set.eval_f32)
        return fail(ARMOUR_E_ARG, "mixed batches are not available with the fp32 study (ARMOUR_EVAL_F32)");
    if (W <= 0 || W > p->Wmax || !worlds) return fail(ARMOUR_E_ARG, "num_worlds out of range");
    for (int w = 0; w < W; w++)
        if (const int rc = check_world(&worlds[w], p->Omax)) return rc;
    int O = 0;
    for (int w = 0; w < W; w++) O = std::max(O, worlds[w].num_obstacles);
    std::vector<double> a(4 * (size_t)W * NF), ob((size_t)W * (O > 0 ? O : 1) * 12, 0.0);
    std::vector<int> ow(W);
    for (int w = 0; w < W; w++) {
        if (!mixed && worlds[w].num_obstacles != worlds[0].num_obstacles)
            return fail(ARMOUR_E_ARG, "all worlds of a batch must have the same num_obstacles");
        for (int i = 0; i < NF; i++) {
            a[0 * (size_t)W * NF + w * NF + i] = worlds[w].q0[i];
            a[1 * (size_t)W * NF + w * NF + i] = worlds[w].qd0[i];
            a[2 * (size_t)W * NF + w * NF + i] = worlds[w].qdd0[i];
            a[3 * (size_t)W * NF + w * NF + i] = worlds[w].q_des[i];
        }
        ow[w] = worlds[w].num_obstacles;
        if (ow[w] > 0) std::memcpy(&ob[(size_t)w * O * 12], worlds[w].obstacles, sizeof(double) * ow[w] * 12);
    }
    const size_t bytes = sizeof(double) * W * NF;
    HIPCK(hipMemcpyAsync(p->q0, &a[0], bytes, hipMemcpyHostToDevice, p->stream));
    HIPCK(hipMemcpyAsync(p->qd0, &a[(size_t)W * NF], bytes, hipMemcpyHostToDevice, p->stream));
    HIPCK(hipMemcpyAsync(p->qdd0, &a[2 * (size_t)W * NF], bytes, hipMemcpyHostToDevice, p->stream));
    HIPCK(hipMemcpyAsync(p->qdes, &a[3 * (size_t)W * NF], bytes, hipMemcpyHostToDevice, p->stream));
    if (O > 0) HIPCK(hipMemcpyAsync(p->obs, ob.data(), sizeof(double) * ob.size(), hipMemcpyHostToDevice, p->stream));
    if (mixed) HIPCK(hipMemcpyAsync(p->d_Ow, ow.data(), sizeof(int) * W, hipMemcpyHostToDevice, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));  // host staging vectors die at return
    p->W = W;
    p->O = O;
    p->Ow = ow;
    NlpDev& d = p->d;
    d.W = W;
    d.O = O;
    d.Ow = mixed ? p->d_Ow : nullptr;  // (what KSEL reads: every solver kernel of this batch is of this kind)
    p->took(mixed ? PATH_BATCH_MIXED : PATH_BATCH_UNIFORM);
    d.pcready = 0;
    d.m = d.nt + p->T * p->NJ * O + NF * 4;
    d.R = d.m + NF;
    d.nblk = (d.R + d.chunk - 1) / d.chunk;  // (d.chunk: Settings::row_chunk, the rows per block the buffers are sized for)
    return 0;
}

// the ARMTD batch: armour_world fields (qdd0 = 0) plus the JRS tables and k_range
static int upload_armtd(armour_planner* p, int W, const armour_armtd_world* worlds) {
    if (!p->armtd) return fail(ARMOUR_E_ARG, "not an ARMTD planner (armour_create_armtd)");
    if (W <= 0 || W > p->Wmax || !worlds) return fail(ARMOUR_E_ARG, "num_worlds out of range");
    for (int w = 0; w < W; w++)
        if (const int rc = check_armtd_world(&worlds[w], p->Omax, p->T)) return rc;
    std::vector<armour_world> base(W);
    const size_t ntab = (size_t)NF * 6 * p->T;
    std::vector<double> tab((size_t)W * ntab), kr((size_t)W * NF);
    for (int w = 0; w < W; w++) {
        armour_world& b = base[w];
        for (int i = 0; i < NF; i++) {
            b.q0[i] = worlds[w].q0[i];
            b.qd0[i] = worlds[w].qd0[i];
            b.qdd0[i] = 0.0;
            b.q_des[i] = worlds[w].q_des[i];
            kr[(size_t)w * NF + i] = worlds[w].k_range[i];
        }
        b.num_obstacles = worlds[w].num_obstacles;
        b.obstacles = worlds[w].obstacles;
        std::memcpy(&tab[(size_t)w * ntab], worlds[w].jrs_tables, sizeof(double) * ntab);
    }
    HIPCK(hipMemcpyAsync(p->d_tables, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, p->stream));
    HIPCK(hipMemcpyAsync((double*)p->d.krange, kr.data(), sizeof(double) * kr.size(), hipMemcpyHostToDevice, p->stream));
    return upload_worlds(p, W, base.data(), false);  // ends in a synchronisation: tab / kr outlive the copies
}

// Bundle kernel shape of a launch of `bundles` bundles (lane_kernel.hip): the dense shape (three
// per CU) when the batch does not fit one round of the wide shape (two per CU), or when other
// planners share the device (this process's live planners, or ARMOUR_DEVICE_SHARED=1 for planners
// in other processes) and the batch holds more than one bundle per CU; else the wide shape.
// Measured: three planners x 327 worlds dense 5324-5363 against 5187 plans/s;
// three planners x 85 worlds (config 4's 256-world job) wide 63.5 against 72.1 ms.
static int lane_shape_for(armour_planner* p, long bundles) {
    int shape = p->set.lane_shape;
    if (shape < 0)
        shape = (bundles > p->lane_slots[0] ||
                 ((p->set.device_shared || g_planners[p->dev & 63].load() > 1) && bundles > p->reach_cus)) ? 1 : 0;
    p->last_shape = shape;
    return shape;
}
static void launch_lane(armour_planner* p, int shape, bool sq, int grid, hipStream_t s, const RobotParams* rp,
                        const lane::LaneArgs& la, const ReachOut& ro) {
    p->took(shape == 1 ? PATH_REACH_LANE_DENSE : PATH_REACH_LANE_WIDE);
    p->took(sq ? PATH_REACH_SQ : PATH_REACH_SQRT);
    if (s != p->stream) p->took(PATH_REACH_CU_MASKED);
    auto k = shape == 1 ? (sq ? lane::lane_reach_kernel<lane::LaneDense> : lane::lane_reach_kernel<lane::LaneDenseSqrt>)
                        : (sq ? lane::lane_reach_kernel<lane::LaneWide> : lane::lane_reach_kernel<lane::LaneWideSqrt>);
    hipLaunchKernelGGL(k, dim3(grid), dim3(lane::LT), 0, s, rp, la, ro);
}

// reach set for the uploaded batch. The whole phase is three kernel launches on the reach stream
// (JRS, reach, and a capacity retry when needed) and one event wait: jrs_kernel zeroes the
// counters, the reach kernel's last workgroup publishes them in mapped host memory
// (ReachCounters), and the constraint bounds are formed by the solver's ipm_rows_init. Nothing
// else is queued here, so under concurrent planners no small kernel waits for CUs another
// planner's persistent reach kernel holds.
static int run_reach(armour_planner* p) {
    hipStream_t rs = p->rstream;
    ReachArgs ra = p->ra;
    ra.W = p->W;
    ra.T = p->T;
    ra.q0 = p->q0;
    ra.qd0 = p->qd0;
    ra.qdd0 = p->qdd0;
    const long jobs = (long)p->W * p->T;
    const int grid = (int)(jobs < p->reach_grid ? jobs : p->reach_grid);
    p->lane_engine = !(p->has_job && jobs <= p->job_max);
    const long nj = jobs * NF;
    HIPCK(hipEventRecord(p->ev[3], rs));
    if (p->armtd)
        hipLaunchKernelGGL(jrs_armtd_kernel, dim3((int)((nj + 127) / 128)), dim3(128), 0, rs, p->W, p->T, p->q0, p->d_tables,
                           p->d_jrs, p->rc, p->ro.err);
    else
        hipLaunchKernelGGL(jrs_kernel, dim3((int)((nj + 127) / 128)), dim3(128), 0, rs, p->d_rp, p->W, p->T, p->q0, p->qd0,
                           p->qdd0, p->d_jrs, p->rc, p->ro.err);
    ra.jrs = p->d_jrs;
    ra.rc.seq = ++p->reach_seq;
    if (p->lane_engine) {
        lane::LaneArgs la = p->la;
        la.W = p->W;
        la.T = p->T;
        la.jrs = p->d_jrs;
        la.rc.seq = p->reach_seq;
        const long bundles = (jobs + lane::LG - 1) / lane::LG;
        const int shape = lane_shape_for(p, bundles);
        const long slots = std::min<long>(p->lane_slots[shape], p->lane_grid);
        const int lg = (int)(bundles < slots ? bundles : slots);
        launch_lane(p, shape, p->sq, lg, rs, p->d_rp, la, p->ro);
    } else {
        // a batch that fits the chip in one round at two jobs per CU takes the wide kernel
        const bool wide = jobs <= (long)REACH_WIDE_PER_CU * p->ncu && !p->set.job_narrow;
        auto k = wide ? (p->sq ? reach_kernel<REACH_WIDE_THREADS, true> : reach_kernel<REACH_WIDE_THREADS, false>)
                      : (p->sq ? reach_kernel<REACH_THREADS, true> : reach_kernel<REACH_THREADS, false>);
        p->took(wide ? PATH_REACH_JOB_256 : PATH_REACH_JOB_128);
        p->took(p->sq ? PATH_REACH_SQ : PATH_REACH_SQRT);
        if (rs != p->stream) p->took(PATH_REACH_CU_MASKED);
        hipLaunchKernelGGL(k, dim3(grid), dim3(wide ? REACH_WIDE_THREADS : REACH_THREADS), 0, rs, p->d_rp, ra, p->ro);
    }
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(p->ev[4], rs));
    HIPCK(hipEventSynchronize(p->ev[4]));
    const volatile long long* sum = p->h_sum;
    if (sum[RSUM_SEQ] != p->reach_seq)
        return fail(ARMOUR_E_HIP, "reach kernel finished without publishing its counters (sequence number mismatch)");
    std::vector<int> err(p->W);
    for (int w = 0; w < p->W; w++) err[w] = (int)sum[RSUM_ERR + w];
    for (int k = 0; k < 8; k++) p->h_occ[k] = (unsigned long long)sum[1 + k];
    {
        // the launch's execution span on the device clock (reach_kernel.hip span_start): occ[5]
        // holds ~(first workgroup start), occ[6] the last workgroup's end
        const unsigned long long t0 = ~p->h_occ[5], t1 = p->h_occ[6];
        p->last_span_ms = (p->h_occ[5] != 0 && t1 >= t0 && p->wall_khz > 0) ? (double)(t1 - t0) / p->wall_khz : -1.0;
    }
    {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, p->ev[3], p->ev[4]);
        p->last_kernel_ms = ms;
        p->last_bytes = (double)sum[0];
    }
    // Capacity isolation. A bundle that overflowed its arena / key buffers flags every world it
    // holds. Those worlds' jobs run again in a second launch of a quarter of the workgroups, each
    // with four workgroups' buffers (4x the arena, key and output capacity). A world that still
    // overflows gets ARMOUR_E_CAPACITY in its result and is not planned; the batch goes on.
    // (armour_get_reach_occupancy reports the first launch against its 1x capacities: h_occ.)
    std::vector<int> retry;
    for (int w = 0; w < p->W; w++)
        if (err[w]) retry.push_back(w);
    p->last_retried = (int)retry.size();
    unsigned long long mono[2] = {p->h_occ[3], p->h_occ[4]};
    if (!retry.empty() && p->lane_engine) {
        lane::LaneArgs la = p->la;
        la.W = p->W;
        la.T = p->T;
        la.jrs = p->d_jrs;
        la.hcap *= RETRY_SCALE;
        la.ccap *= RETRY_SCALE;
        la.gcap *= RETRY_SCALE;
        la.pool_rows *= RETRY_SCALE;
        la.wlist = p->d_wlist;
        la.nlist = (int)retry.size();
        la.dump = nullptr;   // the op dump and bundle times stay those of the first launch
        la.btime = nullptr;
        la.rc.seq = ++p->reach_seq;
        HIPCK(hipMemcpyAsync(p->d_wlist, retry.data(), sizeof(int) * retry.size(), hipMemcpyHostToDevice, rs));
        HIPCK(hipMemsetAsync(p->ro.err, 0, sizeof(int) * p->W, rs));
        const long bundles = ((long)retry.size() * p->T + lane::LG - 1) / lane::LG;
        const long g = std::max(p->lane_grid, RETRY_SCALE) / RETRY_SCALE;
        p->took(PATH_REACH_RETRY);
        launch_lane(p, p->last_shape, p->sq, (int)(bundles < g ? bundles : g), rs, p->d_rp, la, p->ro);
        HIPCK(hipGetLastError());
        HIPCK(hipEventRecord(p->ev[5], rs));
        HIPCK(hipEventSynchronize(p->ev[5]));
        if (sum[RSUM_SEQ] != p->reach_seq)
            return fail(ARMOUR_E_HIP, "capacity retry finished without publishing its counters (sequence number mismatch)");
        for (int w = 0; w < p->W; w++) err[w] = (int)sum[RSUM_ERR + w];
        mono[0] = (unsigned long long)sum[1 + 3];   // maxima over both launches (occ accumulates)
        mono[1] = (unsigned long long)sum[1 + 4];
    }
    p->mono_max[0] = (int)std::min<unsigned long long>(mono[0], 1u << 30);
    p->mono_max[1] = p->armtd ? 0 : (int)std::min<unsigned long long>(mono[1], 1u << 30);
    p->world_err.assign(p->W, 0);
    p->last_failed = 0;
    for (int w = 0; w < p->W; w++)
        if (err[w]) {
            p->world_err[w] = ARMOUR_E_CAPACITY;
            p->last_failed++;
        }
    if (p->last_failed) {
        char buf[200];
        std::snprintf(buf, sizeof(buf), "%d world(s) exceeded a reach-set capacity (first: world %d); the rest are planned",
                      p->last_failed, (int)(std::find_if(err.begin(), err.end(), [](int e) { return e != 0; }) - err.begin()));
        g_err = buf;
    }
    p->reached = true;
    p->d.pcready = 0;
    return 0;
}

// a solver kernel of the last batch's kind: the uniform instantiation, or the mixed batch's (_mx)
#define KSEL(k) (p->d.Ow ? k##_mx : k)

// the certified plane cache of the current reach sets and obstacles (plane_cache_kernel)
static void ensure_plane_cache(armour_planner* p) {
    NlpDev& d = p->d;
    if (!d.pcache || d.pcready || d.O == 0 || p->set.eval_f32) return;
    // The pool is sized at creation for ARMOUR_PC_K records per pair; a build whose blocks need
    // more (the count is known only on the device) is repeated on a pool of 1.25x what it needed,
    // so every block is cached. One host wait on the build, which the solver's first kernels wait
    // for anyway. The cache is marked ready only when the last build fitted its pool: the cached
    // kernels read every block's records from its pool offset, and a block that did not fit has
    // none there. Otherwise (the larger pool cannot be allocated) this solve runs on the full
    // 36-plane scan, whose values, planes and tie-breaks are bitwise the cache's, and without the
    // speculative searches that read only the cache (run_solver, ipm_loop, run_resto).
    bool fits = false;
    for (int attempt = 0; attempt < 3; attempt++) {
        p->took(attempt == 0 ? PATH_PC_BUILDS : PATH_PC_REGROWS);
        hipLaunchKernelGGL(KSEL(plane_cache_kernel), dim3(p->T, p->W), dim3(EVAL_THREADS), 0, p->stream, d);
        if (hipMemcpyAsync(p->h_pcnext, d.pcnext, sizeof(unsigned), hipMemcpyDeviceToHost, p->stream) != hipSuccess ||
            hipStreamSynchronize(p->stream) != hipSuccess)
            break;
        const long need = (long)*p->h_pcnext;
        (void)hipMemsetAsync(d.pcnext, 0, sizeof(unsigned), p->stream);
        if (need <= d.pc_pool) {
            fits = true;
            break;
        }
        if (attempt == 2) break;
        const long grow = need + need / 4;
        double* pc = nullptr;
        uint16_t* pcp = nullptr;
        if (std::getenv("ARMOUR_PC_GROW_FAIL") || dalloc(&pc, 5 * (size_t)grow) != hipSuccess) break;
        if (dalloc(&pcp, (size_t)grow) != hipSuccess) { (void)hipFree(pc); break; }
        for (void*& a : p->allocs) {
            if (a == (void*)d.pc) { (void)hipFree(a); a = pc; }
            else if (a == (void*)d.pcp) { (void)hipFree(a); a = pcp; }
        }
        d.pc = pc;
        d.pcp = pcp;
        d.pc_pool = grow;
    }
    d.pcready = fits ? 1 : 0;
    if (!fits) p->took(PATH_PC_FALLBACKS);
}

static int nside_count(const armour_planner* p) {
    // finite constraint sides: torque 2/row, collision 1/row, extrema 2/row, box 2/variable
    return 2 * p->d.nt + p->T * p->NJ * p->O + 2 * 4 * NF + 2 * NF;
}

// g and J of every world of the batch (eval_kernel_t): fp64, or float for the tolerance study
// (the ARMTD planner's extrema and cost in their own instantiation)
// and the collision rows from the certified plane cache when it is built (points in its box: every
// solver point; `cached` = false for a caller's x outside it)
// the small-capacity evaluation kernels (eval_kernel_small, eval_trials_small: a third of the LDS,
// five blocks per CU) when the last reach's largest PZs and this batch's pair tables fit them
static bool eval_small_fits(const armour_planner* p) {
    return !p->set.eval_full && !p->armtd && !p->set.eval_f32 && p->mono_max[0] <= LM_S && p->mono_max[1] <= UM_S;
}
static void launch_eval(armour_planner* p, dim3 grid, const NlpDev& d, const Round& r, int mode, bool cached = true, hipStream_t s = nullptr) {
    if (!s) s = p->stream;
    const bool c = cached && d.pcready && d.O > 0;
    p->took(c ? PATH_EVAL_CACHED : PATH_EVAL_FULL_SCAN);
    if (c && eval_small_fits(p) && eval_pair_doubles(p->NJ * d.O) <= UB_S) {
        p->took(PATH_EVAL_SMALL);
        hipLaunchKernelGGL(KSEL(eval_kernel_small), grid, dim3(EVAL_THREADS), 0, s, d, r, mode);
        return;
    }
    if (d.Ow) {  // a mixed batch (fp64 ARMOUR planner: upload_worlds)
        p->took(PATH_EVAL_MX);
        hipLaunchKernelGGL(c ? eval_kernel_mx<true> : eval_kernel_mx<false>, grid, dim3(EVAL_THREADS), 0, s, d, r, mode);
        return;
    }
    auto k = p->set.eval_f32 ? (d.armtd ? eval_kernel_t<float, true, false> : eval_kernel_t<float, false, false>)
                         : c ? (d.armtd ? eval_kernel_t<double, true, true> : eval_kernel_t<double, false, true>)
                             : (d.armtd ? eval_kernel_t<double, true, false> : eval_kernel_t<double, false, false>);
    p->took(p->set.eval_f32 ? (d.armtd ? PATH_EVAL_ARMTD_F32 : PATH_EVAL_F32) : (d.armtd ? PATH_EVAL_ARMTD_F64 : PATH_EVAL_F64));
    hipLaunchKernelGGL(k, grid, dim3(EVAL_THREADS), 0, s, d, r, mode);
}
// the values of the K remaining trials of n listed worlds (eval_trials_kernel), from the small-capacity
// kernel when the (trial, pair) keys fit its buffer too
static void launch_trials(armour_planner* p, int n, const NlpDev& d, const Round& r) {
    const bool small = eval_small_fits(p) && r.K * p->NJ * d.O <= UB_TS;
    p->took(small ? PATH_TRIALS_SMALL : PATH_TRIALS_FULL);
    hipLaunchKernelGGL(small ? KSEL(eval_trials_small) : KSEL(eval_trials_kernel), dim3(p->T, n), dim3(EVAL_THREADS), 0, p->stream, d, r);
}

// One speculative line-search round over n list entries: the values of r.K trials of every listed
// world, their row sums, the acceptance tests in trial order, then the chosen trial in full. `all`:
// the sync-free tail's one-round form over all max_ls trials, round 0's included (eval_trials_all,
// ipm_world_Cs_all with pass B's world step); else the K trials that remain after round 0.
static void launch_spec_round(armour_planner* p, int n, const NlpDev& d, const Round& r, bool all) {
    p->took(all ? PATH_LS_ONE_ROUND : PATH_LS_SPECULATIVE);
    if (all) {
        p->took(PATH_TRIALS_ALL);
        hipLaunchKernelGGL(KSEL(eval_trials_all), dim3(p->T, n), dim3(EVAL_THREADS), 0, p->stream, d, r);
    } else {
        launch_trials(p, n, d, r);
    }
    hipLaunchKernelGGL(KSEL(ipm_rows_Cs), dim3(d.nblk, n * r.K), dim3(ROW_THREADS), 0, p->stream, d, r);
    hipLaunchKernelGGL(all ? KSEL(ipm_world_Cs_all) : KSEL(ipm_world_Cs), dim3(n), dim3(64), 0, p->stream, d, r);
    launch_eval(p, dim3(p->T, n), d, r, EVAL_CHOSEN);
}

// One restoration-phase iteration in its one-round form, over nb list entries on stream s: the
// Gauss-Newton pass and world step, the values of all r.K = max_ls trials, their sums, the tests in
// trial order (resto_world_Vs), then the chosen trial in full.
static void launch_resto_round(armour_planner* p, hipStream_t s, int nb, const NlpDev& d, const Round& r) {
    p->took(PATH_RESTO_ONE_ROUND);
    p->took(s != p->stream ? PATH_RESTO_SECOND_STREAM : PATH_RESTO_SOLVER_STREAM);
    p->took(PATH_TRIALS_ALL);
    hipLaunchKernelGGL(KSEL(resto_rows_G), dim3(d.nblk, nb), dim3(ROW_THREADS), 0, s, d, r);
    hipLaunchKernelGGL(KSEL(resto_world_G), dim3(nb), dim3(64), 0, s, d, r, p->od);
    hipLaunchKernelGGL(KSEL(eval_trials_all), dim3(p->T, nb), dim3(EVAL_THREADS), 0, s, d, r);
    hipLaunchKernelGGL(KSEL(resto_rows_Vs), dim3(d.nblk, nb * r.K), dim3(ROW_THREADS), 0, s, d, r);
    hipLaunchKernelGGL(KSEL(resto_world_Vs), dim3(nb), dim3(64), 0, s, d, r);
    launch_eval(p, dim3(p->T, nb), d, r, EVAL_CHOSEN, true, s);
}

// The Round (nlp.h) of each launch family. A field a function does not name keeps Round{}'s value.
static unsigned* cnt_at(const armour_planner* p, int base, int parity = 0) { return p->d.cnt + slot(base, parity); }
static int* flag_at(const armour_planner* p, int base, int parity = 0) { return p->d.flags + slot(base, parity); }
// K trials per list entry in the speculative rows; a phase iteration beside the tail (conc) takes
// the rows after the tail's. The one place resto_soff is applied.
static void spec_view(const armour_planner* p, Round& r, int K, bool conc = false) {
    const size_t off = conc ? p->resto_soff : 0;
    r.K = K;
    r.gs = p->gs + off * (size_t)p->d.m;
    r.fs = p->fs + off;
    r.partial_s = p->partial_s + off * (size_t)p->d.nblk * KA;
}
// (Round{wl, lcount} alone: passes A / DA / B of an iteration; Round{wl}: a restart's ipm_rows_init)
// what the line-search rounds of iteration `it` share: a failed search is appended to RL (null:
// phases run after the loop), whose length the round's last world kernel stores for the host
static Round round_search(const armour_planner* p, int it, int* RL, const int* wl, const unsigned* lcount) {
    Round r{wl, lcount};
    r.rl_app = RL;
    r.pend_flag = RL ? flag_at(p, FLAG_PEND, it) : nullptr;
    return r;
}
// round 0: the running worlds into wl_run, the searching ones into wl_search, both lengths to the
// host and to the next launches; tl: sync-free, wl's length from the device, lagged counts to the host
static Round round_first(const armour_planner* p, int it, int* RL, bool tl, const int* wl, int* wl_run, int* wl_search) {
    Round r = round_search(p, it, RL, wl, tl ? cnt_at(p, CNT_ITER, it) : nullptr);
    r.wl_run = wl_run;
    r.wl_search = wl_search;
    r.ls0 = 1;
    r.lcount_out = cnt_at(p, CNT_LS, 1);
    r.lrun_out = cnt_at(p, CNT_ITER, it + 1);
    r.nrun_flag = tl ? flag_at(p, FLAG_NRUN, it) : nullptr;
    r.bt_flag = tl ? flag_at(p, FLAG_BT, it) : nullptr;
    return r;
}
// sequential round ls >= 1: the searching list Ls[ls & 1] into the other one
static Round round_next(const armour_planner* p, int it, int* RL, int ls, int* const* Ls) {
    Round r = round_search(p, it, RL, Ls[ls & 1], cnt_at(p, CNT_LS, ls));
    r.wl_search = Ls[(ls + 1) & 1];
    r.lcount_out = cnt_at(p, CNT_LS, ls + 1);
    return r;
}
// the speculative round over round 0's searching list (tl: its length read from the device)
static Round round_spec(const armour_planner* p, int it, int* RL, bool tl, const int* wl) {
    Round r = round_search(p, it, RL, wl, tl ? cnt_at(p, CNT_LS, 1) : nullptr);
    spec_view(p, r, p->K0);
    return r;
}
// the tail's one-round search: all max_ls trials of the iteration list, round 0's outputs
static Round round_tail_all(const armour_planner* p, int it, int* RL, const int* wl, int* wl_run) {
    Round r = round_search(p, it, RL, wl, cnt_at(p, CNT_ITER, it));
    r.wl_run = wl_run;
    r.b_in_cs = 1;  // pass B's world step in ipm_world_Cs_all
    r.lrun_out = cnt_at(p, CNT_ITER, it + 1);
    r.nrun_flag = flag_at(p, FLAG_NRUN, it);
    r.bt_flag = flag_at(p, FLAG_BT, it);
    spec_view(p, r, p->K0 + 1);
    return r;
}
// a one-round restoration-phase iteration inside the interior-point loop: the published list PL,
// kept worlds appended to RL (conc: on the second stream, beside the tail)
static Round round_resto_inline(const armour_planner* p, const int* PL, int* RL, bool conc) {
    Round r{PL, cnt_at(p, CNT_PL)};
    r.resto = 1;
    r.rl_app = RL;
    spec_view(p, r, p->d.opt.max_ls, conc);
    return r;
}
// iteration k of run_resto's one-round form: list L[k & 1], kept worlds into the other, its length
// to CNT_ITER of k + 1 (the next launches' lcount) and FLAG_NRUN of k (the host reads it one later)
static Round round_resto_iter(const armour_planner* p, int k, int* const* L) {
    Round r{L[k & 1], k == 0 ? nullptr : cnt_at(p, CNT_ITER, k)};
    r.resto = 1;
    r.wl_run = L[(k + 1) & 1];
    r.lrun_out = cnt_at(p, CNT_ITER, k + 1);
    r.nrun_flag = flag_at(p, FLAG_NRUN, k);
    spec_view(p, r, p->d.opt.max_ls);
    return r;
}
// run_resto's sequential form: the whole list every round, counts to FLAG_RUN / FLAG_SEARCH
static Round round_resto_seq(const int* list) {
    Round r{list};
    r.resto = 1;
    r.rflag = FLAG_RUN;
    return r;
}

// The interior-point loop over the nrun worlds listed in the first iteration list (d_lists[0..]):
// every world there starts an iteration with pass A at its current point (a fresh solve, or a
// restart after a restoration phase).
static int ipm_loop(armour_planner* p, int nrun) {
    const NlpDev& d = p->d;
    int* Li[2] = {p->d_lists, p->d_lists + p->Wmax};                  // worlds of an iteration
    int* Ls[2] = {p->d_lists + 2 * p->Wmax, p->d_lists + 3 * p->Wmax};  // worlds of a line-search round
    const int ns = nside_count(p);
    const bool qf = d.opt.mu_strategy >= 2;
    // Restoration phases inside the loop (with the speculative machinery): after an iteration's
    // interior-point launches, one phase iteration (run_resto's one-round form) for the worlds whose
    // line search failed and are still in their phase. Failures (accept_trial) and the worlds a
    // phase iteration keeps are appended to one list RL (CNT_RL); resto_publish moves it into the
    // phase list PL of the next phase iteration, so an iteration may launch no phase work at all
    // and the appends wait for the next one that does. The host decides from the list length the
    // round's last world kernel stores (pend_flag): in a synchronised iteration exactly (the length
    // after round 0, plus the worlds still searching, which alone can fail now); in the sync-free
    // tail from the length two iterations back (the last one it has read), so a phase starts at
    // most two iterations late and at most two idle phase iterations follow the last one. Worlds
    // still in a phase when the loop ends finish it after the loop (run_solver: run_resto), and so
    // does a restarted world's interior point (the next ipm_loop). A loop over one world runs its
    // phases after the loop: there is no other world's iteration to overlap them with.
    const bool inl = p->resto_inline && d.pcready && nrun > 1;
    int* const RL = inl ? p->d_lists + 4 * p->Wmax : nullptr;
    int* const PL = p->d_lists + 5 * p->Wmax;
    volatile int* flr = p->h_flags;
    const int W0 = nrun;
    int pend_known = 0;  // the latest list length the host has read
    int ub = 0;          // an upper bound of the list's length now: the last phase grid, plus every
                         // interior-point world launched since (each could have failed)
    if (inl) HIPCK(hipMemsetAsync(cnt_at(p, CNT_RL), 0, sizeof(unsigned), p->stream));
    // conc: this phase iteration runs on the second stream, concurrently with the next
    // interior-point iteration (sync-free tail, p->resto_conc). The phase's worlds are not the
    // interior point's (an iteration's list may still name a world that failed after the list was
    // formed: the world kernels write back only the worlds they work on, nlp_kernels.hip ws_copy),
    // and its speculative rows start resto_soff rows in (after the tail's); the
    // one shared structure is the append list RL (CNT_RL): interior-point failures and the phase's
    // kept worlds append to it with atomics, and resto_publish moves it to the phase list. So the
    // publish waits for the interior-point iteration that appended (ev_ip), and the next
    // interior-point iteration waits for the publish (ev_pub), not for the phase iteration. An
    // interior-point iteration's snapshot of the list (pend_flag) may then miss the worlds the
    // concurrent phase iteration keeps, so the host also reads the length each publish moved
    // (FLAG_PUB, pub_known): a phase iteration that had worlds is followed by another at
    // most two iterations later, as long as the loop runs.
    // Once work is queued on the second stream, every way out of this function joins it before
    // anything reads the phase's worlds or reuses PL: the normal exit reports join()'s error, any
    // other return runs it from the destructor and keeps the first error.
    struct Join {
        armour_planner* p;
        bool queued = false;
        hipError_t operator()() {
            if (!queued) return hipSuccess;
            queued = false;
            const hipError_t e = hipEventRecord(p->ev_rend, p->rstream2);
            return e != hipSuccess ? e : hipStreamWaitEvent(p->stream, p->ev_rend, 0);
        }
        ~Join() { (void)(*this)(); }
    } join{p};
    bool pub_launched[2] = {false, false};
    int pub_known = 0;
    auto resto_iter = [&](int it, int bound, bool conc) -> int {
        pub_launched[it & 1] = false;
        if (!inl || bound <= 0) return 0;
        hipStream_t s = p->stream;
        if (conc) {
            s = p->rstream2;
            HIPCK(hipEventRecord(p->ev_ip, p->stream));
            join.queued = true;
            HIPCK(hipStreamWaitEvent(s, p->ev_ip, 0));
        }
        hipLaunchKernelGGL(resto_publish, dim3(1), dim3(256), 0, s, d, (const int*)RL, PL,
                           conc ? flag_at(p, FLAG_PUB, it) : nullptr);
        pub_launched[it & 1] = conc;
        if (conc) {
            HIPCK(hipEventRecord(p->ev_pub, s));
            HIPCK(hipStreamWaitEvent(p->stream, p->ev_pub, 0));
        }
        const int nb = std::min(W0, bound);
        ub = nb;  // the phase keeps at most the worlds it took
        p->took(PATH_RESTO_INLINE);
        launch_resto_round(p, s, nb, d, round_resto_inline(p, PL, RL, conc));
        return 0;
    };
    // Launches cover the active worlds only (Round::wl): every line-search round's ipm_world_C
    // compacts the worlds still running / still searching into the next lists and publishes the
    // counts in mapped host memory, read after the round's one host synchronisation. Inactive
    // worlds in a list (finished by ipm_world_A / _D since) exit at once. A world's arithmetic does
    // not depend on which block serves it, so the results are those of full launches.
    // Sync-free tail: once at most tail_worlds worlds run (and the speculative round is available),
    // an iteration is launched without waiting for the previous one. Grids are sized by the last
    // known running count (an upper bound: the count only falls), every launch reads the true list
    // lengths from device memory (the running count of iteration it in CNT_ITER, the
    // searching count in CNT_LS), and the host learns iteration it's running count one iteration
    // later (event tev[it & 1], FLAG_NRUN). Blocks past a list's length exit at once, so a
    // world's arithmetic is that of the synchronised loop.
    int cur = 0;
    bool tail = false;       // iteration it - 1 ran sync-free (its running count not yet read)
    // worlds that backtracked (searched past round 0) in the latest iteration the host knows of: the
    // tail takes the one-round search while they do (ARMOUR_TAIL_SEARCH=adaptive). A converging
    // world mostly accepts round 0's trial, which its own full evaluation serves faster than the
    // values of every trial plus the chosen one's full evaluation; a backtracking world saves a
    // round. The choice changes launches only, never a world's arithmetic.
    int backtracked = nrun;
    // The end of a sync-free iteration, after its speculative round: the phase iteration, the
    // iteration's end event, then (from the second tail iteration on) iteration it - 1's lagged
    // counts: its running count (the worlds iteration it was launched for, the next grid bound),
    // its backtracking count and the list lengths. `done`: iteration it had nothing to do.
    auto tail_end = [&](int it, bool& done) -> int {
        ub = std::min(W0, ub + nrun);
        if (int rc = resto_iter(it, pend_known > 0 || pub_known > 0 ? ub : 0, p->resto_conc)) return rc;
        HIPCK(hipEventRecord(p->tev[it & 1], p->stream));
        HIPCK(hipGetLastError());
        cur = 1 - cur;
        if (tail) {
            HIPCK(hipEventSynchronize(p->tev[(it - 1) & 1]));
            if (inl) pend_known = flr[slot(FLAG_PEND, it - 1)];
            pub_known = pub_launched[(it - 1) & 1] ? flr[slot(FLAG_PUB, it - 1)] : 0;
            const int prev = flr[slot(FLAG_NRUN, it - 1)];
            backtracked = flr[slot(FLAG_BT, it - 1)];
            if (prev == 0) {
                done = true;
                return 0;
            }
            nrun = prev < nrun ? prev : nrun;
        }
        tail = true;
        return 0;
    };
    for (int it = 0; it <= d.opt.max_iter && nrun > 0; it++) {
        const bool tl = it > 0 && p->spec && d.pcready && nrun <= p->set.tail_worlds;
        const Round di{Li[cur], tl ? cnt_at(p, CNT_ITER, it) : nullptr};
        p->took(tl ? PATH_IPM_ITER_TAIL : PATH_IPM_ITER_SYNC);
        // pass D of the previous iteration (accept its trial point) shares one sweep over the rows
        // with this iteration's pass A
        // (strategies 2 and 3: the _qf instantiations, which also sum theta)
        if (it == 0) {
            hipLaunchKernelGGL(qf ? KSEL(ipm_rows_A_qf) : KSEL(ipm_rows_A), dim3(d.nblk, nrun), dim3(ROW_THREADS), 0, p->stream, d, di);
            hipLaunchKernelGGL(KSEL(ipm_world_A), dim3(nrun), dim3(64), 0, p->stream, d, di, ns, p->od);
        } else {
            // the LDS-accumulator form for grids of several blocks per CU (nlp_kernels.hip rows_DA_body)
            const bool wide = p->set.da_lds && (long)d.nblk * nrun >= 4L * p->ncu;
            p->took(wide ? PATH_DA_LDS : PATH_DA_REGS);
            auto rows_da = qf ? (wide ? KSEL(ipm_rows_DA_lds_qf) : KSEL(ipm_rows_DA_qf)) : (wide ? KSEL(ipm_rows_DA_lds) : KSEL(ipm_rows_DA));
            hipLaunchKernelGGL(rows_da, dim3(d.nblk, nrun), dim3(ROW_THREADS), 0, p->stream, d, di);
            hipLaunchKernelGGL(KSEL(ipm_world_DA), dim3(nrun), dim3(64), 0, p->stream, d, di, ns, p->od);
        }
        if (qf) {
            // the sigma search of the worlds in free mode (QfState::pending), over the iteration's list
            // with its device-side length like the passes around it: no host synchronisation
            p->took(PATH_QF_SIGMA);
            hipLaunchKernelGGL(KSEL(ipm_rows_Q), dim3(nrun), dim3(ROW_THREADS), 0, p->stream, d, di, p->od);
            hipLaunchKernelGGL(KSEL(ipm_world_Q), dim3(nrun), dim3(64), 0, p->stream, d, di, ns, p->od);
        }
        const bool one = tl && p->spec_all && (p->set.tail_search == 2 || backtracked > 0);
        hipLaunchKernelGGL(KSEL(ipm_rows_B), dim3(d.nblk, nrun), dim3(ROW_THREADS), 0, p->stream, d, di);
        if (!one) hipLaunchKernelGGL(KSEL(ipm_world_B), dim3(nrun), dim3(64), 0, p->stream, d, di);
        // Round 0 of the line search for every running world, then one host synchronisation. The
        // worlds still searching after it (the tail of the backtracking) run the remaining rounds
        // without one: a few of them all remaining trials at once (speculative round, ipm_world_Cs),
        // more of them round by round with grids sized by round 0's count and the list lengths in
        // device memory (CNT_LS). Either way the arithmetic is that of sequential rounds.
        if (!one) {
            const Round dc = round_first(p, it, RL, tl, Li[cur], Li[1 - cur], Ls[1]);
            launch_eval(p, dim3(p->T, nrun), d, dc, EVAL_TRIAL);
            hipLaunchKernelGGL(KSEL(ipm_rows_C), dim3(d.nblk, nrun), dim3(ROW_THREADS), 0, p->stream, d, dc);
            hipLaunchKernelGGL(KSEL(ipm_world_C), dim3(nrun), dim3(64), 0, p->stream, d, dc);
        }
        if (tl) {
            // Sync-free: the speculative round over at most nrun entries of round 0's searching list,
            // or (one) the whole line search in one round: the values of all max_ls trials of every
            // running world (round 0's included, the step taken from pass B's partials), then pass B's
            // world step, the tests in trial order and round 0's running list and counts
            // (ipm_world_Cs_all), then the chosen trial in full. Four launches where pass B's world
            // step and round 0 took four and the speculative round four more; the tests, and so the
            // plans, are those of sequential rounds. Then the iteration's end.
            if (one)
                launch_spec_round(p, nrun, d, round_tail_all(p, it, RL, Li[cur], Li[1 - cur]), true);
            else
                launch_spec_round(p, nrun, d, round_spec(p, it, RL, true, Ls[1]), false);
            bool done = false;
            if (int rc = tail_end(it, done)) return rc;
            if (done) break;
            continue;
        }
        HIPCK(hipStreamSynchronize(p->stream));
        const int nnext = flr[FLAG_RUN], nsearch = flr[FLAG_SEARCH];
        backtracked = nsearch;
        if (inl) pend_known = flr[slot(FLAG_PEND, it)];  // after round 0 (ipm_world_C's last block)
        if (nsearch > 0 && p->spec && d.pcready) {
            // the worlds still searching: the values of all remaining trials at once, the acceptance
            // tests in trial order, then the chosen trial in full
            launch_spec_round(p, nsearch, d, round_spec(p, it, RL, false, Ls[1]), false);
        } else if (nsearch > 0) {
            for (int ls = 1; ls < d.opt.max_ls; ls++) {
                const Round dc = round_next(p, it, RL, ls, Ls);
                p->took(PATH_LS_SEQUENTIAL);
                launch_eval(p, dim3(p->T, nsearch), d, dc, EVAL_TRIAL);
                hipLaunchKernelGGL(KSEL(ipm_rows_C), dim3(d.nblk, nsearch), dim3(ROW_THREADS), 0, p->stream, d, dc);
                hipLaunchKernelGGL(KSEL(ipm_world_C), dim3(nsearch), dim3(64), 0, p->stream, d, dc);
            }
        }
        // (the phase list's bound: its length after round 0, plus the worlds that searched past
        // round 0 and so could have failed)
        if (inl) ub = std::min(W0, pend_known + nsearch);
        if (int rc = resto_iter(it, ub, false)) return rc;
        if (nnext == 0) break;  // every world converged, hit the cap, failed or is in a restoration phase
        HIPCK(hipGetLastError());
        cur = 1 - cur;
        nrun = nnext;
    }
    HIPCK(join());  // the last phase iteration
    HIPCK(hipGetLastError());
    return 0;
}

// One restoration phase for the n worlds of `list` (status WS_RESTO), all together: per iteration
// the Gauss-Newton pass and world step, then the Armijo search. With the speculative machinery
// (p->resto_spec) the search is one round — the values of all max_ls trials, their sums, the tests
// in trial order and the chosen trial's full evaluation — and iterations are launched without a
// host synchronisation: the host reads iteration k - 1's count of worlds still in the phase (mapped
// FLAG_NRUN of k - 1, written by resto_world_Vs) after launching iteration k, so at most one
// empty iteration is launched. Otherwise one trial per round (a full evaluation each; rounds after
// the first launched without a synchronisation, their blocks exit for worlds that stopped). The
// worlds leave with status 0 (every row within its bounds: restart), 2 (iteration cap) or 5 (local
// infeasibility). Either way the arithmetic and decisions are the oracle's sequential ones.
static int run_resto(armour_planner* p, const int* list, int n) {
    const NlpDev& d = p->d;
    const volatile int* fl = p->h_flags;
    const int guard = 4 * (d.opt.max_iter + 1);
    if (p->resto_spec && d.pcready) {
        int* L[2] = {const_cast<int*>(list), p->d_lists + 3 * p->Wmax};
        int nb = n;  // grid bound: the last count the host knows (counts only fall)
        for (int k = 0; k < guard; k++) {
            p->took(PATH_RESTO_AFTER_LOOP);
            launch_resto_round(p, p->stream, nb, d, round_resto_iter(p, k, L));
            HIPCK(hipEventRecord(p->tev[k & 1], p->stream));
            HIPCK(hipGetLastError());
            if (k > 0) {
                HIPCK(hipEventSynchronize(p->tev[(k - 1) & 1]));
                const int prev = fl[slot(FLAG_NRUN, k - 1)];  // worlds iteration k was launched for
                if (prev == 0) break;
                nb = prev < nb ? prev : nb;
            }
        }
        HIPCK(hipStreamSynchronize(p->stream));
        return 0;
    }
    const Round dr = round_resto_seq(list);
    for (int k = 0; k < guard; k++) {
        p->took(PATH_RESTO_AFTER_LOOP);
        p->took(PATH_RESTO_ROUNDS);
        p->took(PATH_RESTO_SOLVER_STREAM);
        hipLaunchKernelGGL(KSEL(resto_rows_G), dim3(d.nblk, n), dim3(ROW_THREADS), 0, p->stream, d, dr);
        hipLaunchKernelGGL(KSEL(resto_world_G), dim3(n), dim3(64), 0, p->stream, d, dr, p->od);
        HIPCK(hipStreamSynchronize(p->stream));
        if (fl[FLAG_RUN] == 0) break;
        for (int ls = 0; ls < d.opt.max_ls; ls++) {
            launch_eval(p, dim3(p->T, n), d, dr, EVAL_TRIAL);
            hipLaunchKernelGGL(KSEL(resto_rows_V), dim3(d.nblk, n), dim3(ROW_THREADS), 0, p->stream, d, dr);
            hipLaunchKernelGGL(KSEL(resto_world_V), dim3(n), dim3(64), 0, p->stream, d, dr);
            if (ls == 0) {
                HIPCK(hipStreamSynchronize(p->stream));
                if (fl[FLAG_SEARCH] == 0) break;
            }
        }
        HIPCK(hipGetLastError());
    }
    return 0;
}

static int run_solver(armour_planner* p) {
    const int W = p->W;
    int* Li0 = p->d_lists;                  // the interior-point loop's first list
    int* Lr = p->d_lists + 2 * p->Wmax;     // worlds of a restoration phase
    ensure_plane_cache(p);
    const NlpDev& d = p->d;
    p->took(d.opt.mu_strategy == 0 ? PATH_SOLVE_MONOTONE : d.opt.mu_strategy == 1 ? PATH_SOLVE_ADAPTIVE : PATH_SOLVE_QUALITY);
    if (p->od.lbfgs_history > 0) p->took(PATH_HESS_LBFGS);
    Round r0;  // ipm_world_init fills the first iteration list with every world
    r0.wl_run = Li0;
    hipLaunchKernelGGL(ipm_world_init, dim3((W + 63) / 64), dim3(64), 0, p->stream, d, r0, p->od);
    launch_eval(p, dim3(p->T, W), d, Round{}, EVAL_POINT);
    hipLaunchKernelGGL(KSEL(ipm_rows_init), dim3(d.nblk, W), dim3(ROW_THREADS), 0, p->stream, d, Round{});
    HIPCK(hipGetLastError());
    int rc = ipm_loop(p, W);
    // Restoration phases: the worlds whose line search failed left the loop with
    // status WS_RESTO. They run their phase together; those that reached a point within every bound
    // restart the interior point (slacks and multipliers at that point), and may fail again (at
    // most resto_max phases per world, S.nresto).
    const volatile int* fl = p->h_flags;
    while (rc == 0 && d.opt.resto_max > 0) {
        hipLaunchKernelGGL(ipm_collect, dim3(1), dim3(1024), 0, p->stream, d, (const int*)nullptr, W, WS_RESTO, Lr, FLAG_RUN, -1);
        HIPCK(hipStreamSynchronize(p->stream));
        const int nr = fl[FLAG_RUN];
        if (nr > 0 && (rc = run_resto(p, Lr, nr))) break;
        // the restarted worlds (WS_RESTART), running again from here. Collected whether or not a
        // phase ran just now: a phase that ran inside ipm_loop may have restarted a world while
        // other worlds were still iterating, and the loop never takes such a world back itself.
        hipLaunchKernelGGL(ipm_collect, dim3(1), dim3(1024), 0, p->stream, d, (const int*)nullptr, W, WS_RESTART, Li0, FLAG_RUN, 0);
        HIPCK(hipStreamSynchronize(p->stream));
        const int ni = fl[FLAG_RUN];
        if (ni == 0) break;
        p->took(PATH_IPM_RESTARTS, ni);
        hipLaunchKernelGGL(KSEL(ipm_rows_init), dim3(d.nblk, ni), dim3(ROW_THREADS), 0, p->stream, d, Round{Li0});
        rc = ipm_loop(p, ni);
    }
    if (rc) return rc;
    // feasibility re-check and the sliced link centres at the final iterate (the current slot's,
    // armour_joint_position_center.out payload)
    hipLaunchKernelGGL(KSEL(feasible_kernel), dim3(W), dim3(256), 0, p->stream, d, p->feas);
    HIPCK(hipGetLastError());
    return 0;
}

// Every entry point runs on its planner's device, whatever the calling thread's current device is
// (handles may be driven from other host threads); the caller's device is restored.
// The device-level entries (create, self-check, copy bandwidth) name their device themselves.
struct DeviceScope {
    int prev = -1;
    bool ok = false;  // `device` is current now (a negative device: nothing was asked, the current one stays)
    explicit DeviceScope(int device) {
        int cur = -1;
        if (device < 0 || hipGetDevice(&cur) != hipSuccess) return;
        ok = cur == device || hipSetDevice(device) == hipSuccess;
        if (ok && cur != device) prev = cur;
    }
    explicit DeviceScope(const armour_planner* p) : DeviceScope(p ? p->cfg.device : -1) {}
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

extern "C" {

const char* armour_last_error(void) { return g_err.c_str(); }

int armour_device_compute_units(int device) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
        return fail(ARMOUR_E_HIP, "hipDeviceGetAttribute failed (no device?)");
    return n;
}

// streaming copy (the achievable-HBM reference kernel): each workgroup copies one contiguous 16 KiB
// block, four 16-B loads per lane in flight before its four stores, nontemporal both ways. Measured
// shapes (tools/micro/copy.hip, 2 x 2 GiB): this one 5.9 TB/s; without nt 5.6; grid-stride with
// four loads per lane (the round-4 kernel) 4.5; eight or sixteen per lane 4.3 / 5.2.
typedef double copy_v2d __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void copy_kernel(const copy_v2d* __restrict__ src, copy_v2d* __restrict__ dst, long n) {
    const long base = (long)blockIdx.x * 1024 + threadIdx.x;
    copy_v2d v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long i = base + k * 256;
        if (i < n) v[k] = __builtin_nontemporal_load(&src[i]);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long i = base + k * 256;
        if (i < n) __builtin_nontemporal_store(v[k], &dst[i]);
    }
}

int armour_sq_selfcheck(int device, double thr, long long half_width, const double* values, long long n,
                        double* s_star, int* valid, long long* mismatches) {
    if (half_width < 0 || n < 0 || (n > 0 && !values) || !s_star || !valid || !mismatches)
        return fail(ARMOUR_E_ARG, "half_width >= 0, n >= 0, values unless n = 0, and the three outputs");
    DeviceScope device_scope(device);
    if (!device_scope.ok) return fail(ARMOUR_E_HIP, "hipSetDevice failed (no device?)");
    RobotParams* rp = nullptr;
    double* dv = nullptr;
    unsigned long long* dbad = nullptr;
    struct Free {
        RobotParams*& a; double*& b; unsigned long long*& c;
        ~Free() { if (a) (void)hipFree(a); if (b) (void)hipFree(b); if (c) (void)hipFree(c); }
    } freer{rp, dv, dbad};
    HIPCK(hipMalloc((void**)&rp, sizeof(RobotParams)));
    HIPCK(hipMalloc((void**)&dbad, sizeof(unsigned long long)));
    if (n > 0) {
        HIPCK(hipMalloc((void**)&dv, sizeof(double) * (size_t)n));
        HIPCK(hipMemcpy(dv, values, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    }
    HIPCK(hipMemset(rp, 0, sizeof(RobotParams)));
    HIPCK(hipMemset(dbad, 0, sizeof(unsigned long long)));
    HIPCK(hipMemcpy(&rp->simplify_threshold, &thr, sizeof(double), hipMemcpyHostToDevice));
    // the planner's own search (planner_init), then the comparison of the two decisions
    hipLaunchKernelGGL(sq_threshold_kernel, dim3(1), dim3(1), 0, nullptr, rp);
    HIPCK(hipGetLastError());
    SqThr q;
    q.thr = thr;
    HIPCK(hipMemcpy(&q.s, &rp->simplify_sq, sizeof(double), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(&q.valid, &rp->simplify_sq_valid, sizeof(int), hipMemcpyDeviceToHost));
    const long long total = 2 * half_width + 1 + n;
    const int blocks = (int)std::min<long long>((total + 255) / 256, 1024);
    hipLaunchKernelGGL(sq_selfcheck_kernel, dim3(blocks), dim3(256), 0, nullptr, q, half_width, dv, n, dbad);
    HIPCK(hipGetLastError());
    unsigned long long bad = 0;
    HIPCK(hipMemcpy(&bad, dbad, sizeof(bad), hipMemcpyDeviceToHost));
    *s_star = q.s;
    *valid = q.valid;
    *mismatches = (long long)bad;
    return ARMOUR_OK;
}

double armour_copy_bandwidth(int device, size_t bytes, int reps) {
    if (reps <= 0 || bytes < 16) return fail(ARMOUR_E_ARG, "bytes >= 16 and reps > 0");
    DeviceScope device_scope(device);
    if (!device_scope.ok) return fail(ARMOUR_E_HIP, "hipSetDevice failed (no device?)");
    const long n = (long)(bytes / 16);
    copy_v2d *a = nullptr, *b = nullptr;
    hipEvent_t e0, e1;
    if (hipMalloc((void**)&a, n * 16) != hipSuccess) return fail(ARMOUR_E_HIP, "hipMalloc failed");
    if (hipMalloc((void**)&b, n * 16) != hipSuccess) { (void)hipFree(a); return fail(ARMOUR_E_HIP, "hipMalloc failed"); }
    (void)hipMemset(a, 0, n * 16);
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    const dim3 grid((unsigned)((n + 1023) / 1024)), blk(256);
    hipLaunchKernelGGL(copy_kernel, grid, blk, 0, nullptr, a, b, n);
    (void)hipEventRecord(e0, nullptr);
    for (int r = 0; r < reps; r++) hipLaunchKernelGGL(copy_kernel, grid, blk, 0, nullptr, a, b, n);
    (void)hipEventRecord(e1, nullptr);
    const hipError_t err = hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(a);
    (void)hipFree(b);
    if (err != hipSuccess || ms <= 0) return fail(ARMOUR_E_HIP, "copy kernel failed");
    return 2.0 * n * 16.0 * reps / (ms * 1e-3) / 1e9;
}

int armour_robot_builtin(int robot_id, armour_robot* out) {
    if (!out || robot_id != 0) return fail(ARMOUR_E_ARG, "unknown robot id / null output");
    RobotParams r;
    kinova_gen3(r);
    robot_to_tables(r, *out);
    return 0;
}

static armour_planner* create(const armour_config* cfg, const armour_robot* robot, bool armtd) {
    if (!cfg) { fail(ARMOUR_E_ARG, "null config"); return nullptr; }
    // planner_init runs on cfg->device (and reports a device it cannot select); the caller's
    // current device is restored on return
    DeviceScope device_scope(cfg->device);
    armour_planner* p = new armour_planner();
    if (planner_init(p, cfg, robot, armtd) != 0) {
        std::string keep = g_err;  // the first error's message, not one of the teardown's
        armour_destroy(p);
        g_err = keep;
        return nullptr;
    }
    return p;
}

armour_planner* armour_create(const armour_config* cfg) { return create(cfg, nullptr, false); }
armour_planner* armour_create_robot(const armour_config* cfg, const armour_robot* robot) { return create(cfg, robot, false); }
armour_planner* armour_create_armtd(const armour_config* cfg) { return create(cfg, nullptr, true); }

void armour_destroy(armour_planner* p) {
    DeviceScope device_scope(p);
    if (!p) return;
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    for (void* a : p->allocs) (void)hipFree(a);
    p->cand.release();
    for (ExecState* x : std::initializer_list<ExecState*>{&p->motion, &p->track, &p->tracked, &p->ep, &p->ept}) x->release();
    p->roadmap.release_all();
    if (p->h_flags) (void)hipHostFree(p->h_flags);
    if (p->h_sum) (void)hipHostFree(p->h_sum);
    if (p->h_ws) (void)hipHostFree(p->h_ws);
    if (p->h_f) (void)hipHostFree(p->h_f);
    if (p->h_feas) (void)hipHostFree(p->h_feas);
    if (p->h_pcnext) (void)hipHostFree(p->h_pcnext);
    if (p->stream) {
        for (int i = 0; i < 6; i++) (void)hipEventDestroy(p->ev[i]);
        for (int i = 0; i < 2; i++) (void)hipEventDestroy(p->tev[i]);
        if (p->rstream2) (void)hipStreamSynchronize(p->rstream2);
        for (hipEvent_t e : {p->ev_ip, p->ev_pub, p->ev_rend})
            if (e) (void)hipEventDestroy(e);
        if (p->rstream2) (void)hipStreamDestroy(p->rstream2);
        if (p->rstream && p->rstream != p->stream) (void)hipStreamDestroy(p->rstream);
        (void)hipStreamDestroy(p->stream);
    }
    if (p->counted) g_planners[p->dev & 63]--;
    delete p;
}

int armour_plan(armour_planner* p, const armour_world* world, armour_plan_output* out) {
    if (!p || !world || !out) return fail(ARMOUR_E_ARG, "null argument");
    int rc = armour_plan_batch(p, 1, world, &out->result, &out->timing);
    if (rc) return rc;
    if (out->constraints && (rc = armour_get_constraints(p, 0, out->constraints))) return rc;
    if (out->joint_bounds && (rc = armour_get_joint_bounds(p, out->joint_bounds))) return rc;
    if (out->link_centers && (rc = armour_get_link_centers(p, 0, out->link_centers))) return rc;
    if (out->link_generators && (rc = armour_get_link_generators(p, 0, out->link_generators))) return rc;
    if (out->torque_radius && (rc = armour_get_torque_radius(p, 0, out->torque_radius))) return rc;
    return 0;
}

int armour_check_world(const armour_world* world, int max_obstacles) { return check_world(world, max_obstacles); }
int armour_check_armtd_world(const armour_armtd_world* world, int max_obstacles, int num_time_steps) {
    return check_armtd_world(world, max_obstacles, num_time_steps);
}

int armour_num_constraints(const armour_planner* p, int O) { return p ? p->d.nt + p->T * p->NJ * O + NF * 4 : ARMOUR_E_ARG; }
int armour_num_joints(const armour_planner* p) { return p ? p->NJ : ARMOUR_E_ARG; }

int armour_get_joint_bounds(const armour_planner* p, double* b) {
    DeviceScope device_scope(p);
    if (!p || !b) return fail(ARMOUR_E_ARG, "null argument");
    const RobotParams& rp = p->rp;
    for (int i = 0; i < NF; i++) {
        b[2 * i] = rp.state_lb[i] + rp.qe;
        b[2 * i + 1] = rp.state_ub[i] - rp.qe;
        b[2 * NF + 2 * i] = -rp.speed_limits[i] + rp.qde;
        b[2 * NF + 2 * i + 1] = rp.speed_limits[i] - rp.qde;
    }
    return 0;
}

static int reach_uploaded(armour_planner* p, armour_timing* timing, std::chrono::steady_clock::time_point t0);
static int plan_uploaded(armour_planner* p, armour_result* results, armour_timing* timing,
                         std::chrono::steady_clock::time_point t0);

// The six batch entries: null checks, the batch state reset, the upload of the batch's kind (uniform,
// mixed or ARMTD worlds), then the reach phase alone (`plan` false) or the reach phase and the solve.
enum BatchKind { BATCH_UNIFORM, BATCH_MIXED, BATCH_ARMTD };
static int run_batch(armour_planner* p, BatchKind kind, bool plan, int W, const void* worlds, armour_result* results,
                     armour_timing* timing) {
    DeviceScope device_scope(p);
    if (!p || (plan && !results)) return fail(ARMOUR_E_ARG, plan ? "null planner / results" : "null planner");
    if (kind == BATCH_UNIFORM && p->armtd)
        return fail(ARMOUR_E_ARG, plan ? "an ARMTD planner takes armour_armtd_world (armour_plan_armtd_batch)"
                                       : "an ARMTD planner takes armour_armtd_world (armour_reach_armtd_batch)");
    p->reached = p->planned = p->evaluated = p->ep.on = false;
    p->roadmap.valid = p->roadmap.episode = false;
    auto t0 = std::chrono::steady_clock::now();
    const int rc = kind == BATCH_ARMTD ? upload_armtd(p, W, (const armour_armtd_world*)worlds)
                                       : upload_worlds(p, W, (const armour_world*)worlds, kind == BATCH_MIXED);
    return rc ? rc : plan ? plan_uploaded(p, results, timing, t0) : reach_uploaded(p, timing, t0);
}

int armour_reach_batch(armour_planner* p, int W, const armour_world* worlds, armour_timing* timing) {
    return run_batch(p, BATCH_UNIFORM, false, W, worlds, nullptr, timing);
}
int armour_plan_batch(armour_planner* p, int W, const armour_world* worlds, armour_result* results, armour_timing* timing) {
    return run_batch(p, BATCH_UNIFORM, true, W, worlds, results, timing);
}
int armour_reach_batch_mixed(armour_planner* p, int W, const armour_world* worlds, armour_timing* timing) {
    return run_batch(p, BATCH_MIXED, false, W, worlds, nullptr, timing);
}
int armour_plan_batch_mixed(armour_planner* p, int W, const armour_world* worlds, armour_result* results,
                            armour_timing* timing) {
    return run_batch(p, BATCH_MIXED, true, W, worlds, results, timing);
}
int armour_reach_armtd_batch(armour_planner* p, int W, const armour_armtd_world* worlds, armour_timing* timing) {
    return run_batch(p, BATCH_ARMTD, false, W, worlds, nullptr, timing);
}
int armour_plan_armtd_batch(armour_planner* p, int W, const armour_armtd_world* worlds, armour_result* results,
                            armour_timing* timing) {
    return run_batch(p, BATCH_ARMTD, true, W, worlds, results, timing);
}

int armour_world_num_obstacles(const armour_planner* p, int w) {
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    if (!p->reached) return fail(ARMOUR_E_STATE, "no batch: call a reach or plan entry first");
    if (w < 0 || w >= p->W) return fail(ARMOUR_E_ARG, "world index out of range");
    return p->Ow[w];
}

// the phase times of the finished batch: reach ev[0] .. ev[1], and the solve ev[1] .. ev[2] when it ran
static void fill_timing(armour_planner* p, armour_timing* timing, bool solved, std::chrono::steady_clock::time_point t0) {
    if (!timing) return;
    float a = 0, b = 0;
    (void)hipEventElapsedTime(&a, p->ev[0], p->ev[1]);
    if (solved) (void)hipEventElapsedTime(&b, p->ev[1], p->ev[2]);
    timing->reach_ms = a;
    timing->nlp_ms = b;
    timing->reach_kernel_ms = p->last_kernel_ms;
    timing->reach_bytes = p->last_bytes;
    timing->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static int reach_uploaded(armour_planner* p, armour_timing* timing, std::chrono::steady_clock::time_point t0) {
    int rc = 0;
    HIPCK(hipEventRecord(p->ev[0], p->rstream));
    if ((rc = run_reach(p))) return rc;
    HIPCK(hipEventRecord(p->ev[1], p->rstream));
    HIPCK(hipEventSynchronize(p->ev[1]));
    fill_timing(p, timing, false, t0);
    return 0;
}

static int plan_uploaded(armour_planner* p, armour_result* results, armour_timing* timing,
                         std::chrono::steady_clock::time_point t0) {
    int rc = 0;
    const int W = p->W;
    // the reach phase on the reach stream (ev[0] .. ev[1]; run_reach ends in a host wait for it),
    // then the solver on the planner's stream (ev[1] .. ev[2])
    HIPCK(hipEventRecord(p->ev[0], p->rstream));
    if ((rc = run_reach(p))) return rc;
    HIPCK(hipEventRecord(p->ev[1], p->rstream));
    if ((rc = run_solver(p))) return rc;
    HIPCK(hipEventRecord(p->ev[2], p->stream));
    HIPCK(hipMemcpyAsync(p->h_ws, p->d.ws, sizeof(WorldState) * W, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipMemcpyAsync(p->h_f, p->d.f, sizeof(double) * 2 * p->Wmax, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipMemcpyAsync(p->h_feas, p->feas, sizeof(int) * W, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));
    for (int w = 0; w < W; w++) {
        const WorldState& S = p->h_ws[w];
        armour_result& r = results[w];
        for (int i = 0; i < NF; i++) r.k_opt[i] = S.x[i];
        r.feasible = p->h_feas[w];
        r.solver_status = S.status == 1 ? 0 : S.status == 2 ? 1 : S.status == 3 ? 2 : S.status == 5 ? 4 : 3;
        r.iterations = S.iter;
        r.evaluations = S.nevals;
        r.cost = p->h_f[S.cur * p->d.W + w] / p->rp.cost_scale;
        r.kkt_error = S.kkt;
        r.error = p->world_err[w];
        // a world the solver left in a non-terminal state (running, in a restoration phase, or
        // waiting to restart) is a solver fault, never a silent "not planned"
        if (!r.error && (S.status == 0 || S.status == WS_RESTO || S.status == WS_RESTART)) r.error = ARMOUR_E_INTERNAL;
        if (r.error) {
            r.solver_status = 3;
            r.feasible = 0;
        }
    }
    p->planned = true;
    fill_timing(p, timing, true, t0);
    return 0;
}

int armour_eval_constraints(armour_planner* p, int w, const double* x, double* g, double* jac) {
    DeviceScope device_scope(p);
    if (!p || !x || !g) return fail(ARMOUR_E_ARG, "null argument");
    if (!p->reached) return fail(ARMOUR_E_STATE, "no reach set: call armour_reach_batch or armour_plan_batch first");
    if (w < 0 || w >= p->W) return fail(ARMOUR_E_ARG, "world index out of range");
    const NlpDev& d = p->d;
    // evaluate every world of the batch at x in slot 0 (ws.x is the solver's start/end point, so
    // a subsequent query of solver outputs must re-plan)
    // (on the planner's stream, so the copies are ordered with its kernels)
    std::vector<WorldState> ws(p->W);
    HIPCK(hipMemcpyAsync(ws.data(), d.ws, sizeof(WorldState) * p->W, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));
    for (int i = 0; i < p->W; i++) {
        for (int j = 0; j < NF; j++) ws[i].x[j] = x[j];
        ws[i].status = 0;
        ws[i].cur = 0;
    }
    HIPCK(hipMemcpyAsync(d.ws, ws.data(), sizeof(WorldState) * p->W, hipMemcpyHostToDevice, p->stream));
    ensure_plane_cache(p);
    bool inbox = true;
    for (int j = 0; j < NF; j++) inbox = inbox && std::fabs(x[j]) <= PC_XBOX;
    launch_eval(p, dim3(p->T, p->W), d, Round{}, EVAL_POINT, inbox);
    HIPCK(hipGetLastError());
    // world w's own m values (a mixed batch: the first m_w of its slab, which holds them compactly)
    const size_t mw = (size_t)armour_num_constraints(p, p->Ow[w]);
    HIPCK(hipMemcpyAsync(g, d.g + gidx(d, 0, w, 0), sizeof(double) * mw, hipMemcpyDeviceToHost, p->stream));
    if (jac) HIPCK(hipMemcpyAsync(jac, d.J + gidx(d, 0, w, 0) * NF, sizeof(double) * mw * NF, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));
    p->planned = false;
    p->evaluated = true;
    return 0;
}

// ---- checks shared by the candidate and execution entries: the messages are part of the interface
//  ----
// `what_is`: the feature and its verb ("episodes are")
static int not_available(const armour_planner* p, const char* what_is) {
    if (p->armtd) return fail(ARMOUR_E_ARG, std::string(what_is) + " not available on an ARMTD planner");
    if (p->set.eval_f32) return fail(ARMOUR_E_ARG, std::string(what_is) + " not available with the fp32 study (ARMOUR_EVAL_F32)");
    return 0;
}
static int no_episode() {
    return fail(ARMOUR_E_STATE, "no episode: call armour_episode_begin first (any other reach or plan entry ends one)");
}
// N trajectories [4][NF]: every value finite and every k inside [-1, 1]; the rollouts, whose messages
// name the array, also hold |q0| to ARMOUR_MAX_ABS_ANGLE
static int check_traj(const double* traj, int N, bool rollouts) {
    for (int n = 0; n < N; n++) {
        const double* t = traj + (size_t)n * TRAJ_DOUBLES;
        for (int i = 0; i < TRAJ_DOUBLES; i++)
            if (!std::isfinite(t[i])) return fail(ARMOUR_E_ARG, "traj holds a value that is not finite");
        for (int i = 0; i < NF; i++) {
            if (rollouts && !(std::fabs(t[i]) <= ARMOUR_MAX_ABS_ANGLE))
                return fail(ARMOUR_E_ARG, "traj: every |q0| must be at most ARMOUR_MAX_ABS_ANGLE");
            if (!(std::fabs(t[3 * NF + i]) <= 1.0))
                return fail(ARMOUR_E_ARG, std::string(rollouts ? "traj: " : "") + "every k must lie inside [-1, 1]");
        }
    }
    return 0;
}
// the optional scales [NR][2][NJ] and start errors [NR][2][NF] of NR rollouts
static int check_scale_err0(const double* scale, const double* err0, size_t NR, int NJ) {
    if (scale)
        for (size_t i = 0; i < NR * 2 * NJ; i++) {
            if (!std::isfinite(scale[i])) return fail(ARMOUR_E_ARG, "scale holds a value that is not finite");
            if (!(scale[i] > 0)) return fail(ARMOUR_E_ARG, "every scale must be positive");
        }
    if (err0)
        for (size_t i = 0; i < NR * 2 * NF; i++)
            if (!std::isfinite(err0[i])) return fail(ARMOUR_E_ARG, "err0 holds a value that is not finite");
    return 0;
}

// buffers of armour_eval_candidates for N candidates per world
static int cand_reserve(armour_planner* p, int N) {
    CandDev& c = p->cd;
    const size_t n = (size_t)p->Wmax * N, nT = n * p->T;
    return p->cand.reserve(p->stream, N,
                           {GrowSet::buf(c.x, n * NF), GrowSet::buf(c.ptq, nT), GrowSet::buf(c.pcol, nT), GrowSet::buf(c.pbad, nT),
                            GrowSet::buf(c.cost, n), GrowSet::buf(c.viol, n * 3), GrowSet::buf(c.feas, n),
                            GrowSet::buf(c.best, (size_t)p->Wmax)},
                           "hipMalloc failed for the candidate buffers (max_worlds x num_candidates x T partials)");
}

int armour_eval_candidates(armour_planner* p, int N, const double* x, double* cost, double* violation, int* feasible,
                           int* best) {
    DeviceScope device_scope(p);
    if (!p || !x) return fail(ARMOUR_E_ARG, "null planner / x");
    if (int rc = not_available(p, "candidate evaluation is")) return rc;
    if (N < 1) return fail(ARMOUR_E_ARG, "num_candidates must be at least 1");
    if (!p->reached) return fail(ARMOUR_E_STATE, "no batch: call a reach or plan entry first");
    const int W = p->W;
    const size_t n = (size_t)W * N;
    if (n > (size_t)1 << 30 || (size_t)((N + CAND_KC - 1) / CAND_KC) > 65535)
        return fail(ARMOUR_E_ARG, "too many candidates (num_candidates <= 1048560, worlds x candidates <= 2^30)");
    // the plane cache is certified for the box |x_i| <= 1 only
    for (size_t i = 0; i < n * NF; i++)
        if (!(std::fabs(x[i]) <= 1.0)) return fail(ARMOUR_E_ARG, "every candidate must be finite and inside [-1, 1]");
    const NlpDev& d = p->d;
    ensure_plane_cache(p);
    if (d.O > 0 && !d.pcready)
        return fail(ARMOUR_E_STATE, d.pcache ? "the certified plane cache is unavailable (its build did not fit a pool); "
                                               "candidate evaluation has no full-scan path"
                                             : "the certified plane cache is unavailable (ARMOUR_PLANE_CACHE=0, or the batch "
                                               "capacity exceeds its 32-bit pool); candidate evaluation has no full-scan path");
    if (int rc = cand_reserve(p, N)) return rc;
    CandDev c = p->cd;
    c.N = N;
    HIPCK(hipMemcpyAsync(const_cast<double*>(c.x), x, sizeof(double) * n * NF, hipMemcpyHostToDevice, p->stream));
    const dim3 grid(p->T, W, (N + CAND_KC - 1) / CAND_KC);
    p->took(eval_small_fits(p) ? PATH_CAND_SMALL : PATH_CAND_FULL);
    p->took(PATH_CAND_CHUNKS, grid.z);
    if (eval_small_fits(p))
        hipLaunchKernelGGL(KSEL(cand_rows_small), grid, dim3(EVAL_THREADS), 0, p->stream, d, c);
    else
        hipLaunchKernelGGL(KSEL(cand_rows), grid, dim3(EVAL_THREADS), 0, p->stream, d, c);
    hipLaunchKernelGGL(KSEL(cand_finish), dim3((N + 3) / 4, W), dim3(256), 0, p->stream, d, c);
    hipLaunchKernelGGL(cand_best, dim3(W), dim3(64), 0, p->stream, d, c);
    HIPCK(hipGetLastError());
    if (cost) HIPCK(hipMemcpyAsync(cost, c.cost, sizeof(double) * n, hipMemcpyDeviceToHost, p->stream));
    if (violation) HIPCK(hipMemcpyAsync(violation, c.viol, sizeof(double) * n * 3, hipMemcpyDeviceToHost, p->stream));
    if (feasible) HIPCK(hipMemcpyAsync(feasible, c.feas, sizeof(int) * n, hipMemcpyDeviceToHost, p->stream));
    if (best) HIPCK(hipMemcpyAsync(best, c.best, sizeof(int) * W, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));
    return 0;
}

// buffers of the execution check for S samples per world
static int motion_reserve(armour_planner* p, int S) {
    MotionCheck& m = p->motion;
    int rc = 0;
    if (!m.traj && ((rc = p->alloc(&m.traj, (size_t)p->Wmax * TRAJ_DOUBLES)) || (rc = p->alloc(&m.clear, (size_t)p->Wmax)) ||
                    (rc = p->alloc(&m.where, 3 * (size_t)p->Wmax))))
        return rc;
    const size_t n = (size_t)p->Wmax * S;
    return m.grow.reserve(p->stream, S, {GrowSet::buf(m.pval, n), GrowSet::buf(m.pidx, n)},
                          "hipMalloc failed for the execution check's buffers (max_worlds x samples)");
}

// the check kernels' view of the resident batch: S samples per world, per-world windows `win` (device,
// [W][2]; null: none), the minima in pval / pidx
static MotionArgs motion_args(const armour_planner* p, int S, const double* win, double* pval, int* pidx) {
    MotionArgs a{};
    a.rp = p->d_rp;
    a.W = p->W;
    a.S = S;
    a.O = p->d.O;
    a.Ow = p->d.Ow;
    a.obs = p->obs;
    a.win = win;
    a.pval = pval;
    a.pidx = pidx;
    return a;
}

// the execution check of the resident batch over S samples of `traj` (device, [W][4][7]): per-world
// windows `win` or [t0, t1] for every world; results in motion.clear / motion.where
static void launch_motion(armour_planner* p, const double* traj, const double* win, double t0, double t1, int S) {
    MotionArgs a = motion_args(p, S, win, p->motion.pval, p->motion.pidx);
    a.traj = traj;
    a.t0 = t0;
    a.t1 = t1;
    p->took(PATH_MOTION_CHUNKS, S);
    hipLaunchKernelGGL(motion_check_kernel, dim3(S, p->W), dim3(MOTION_THREADS), 0, p->stream, a);
    hipLaunchKernelGGL(motion_finish_kernel, dim3(p->W), dim3(64), 0, p->stream, a, p->motion.clear, p->motion.where);
}

int armour_check_motion(armour_planner* p, const double* traj, double t0, double t1, int samples, double* clearance,
                        int* where) {
    DeviceScope device_scope(p);
    if (!p || !traj) return fail(ARMOUR_E_ARG, "null planner / traj");
    if (int rc = not_available(p, "the execution check is")) return rc;
    if (samples < 1 || samples > 65535) return fail(ARMOUR_E_ARG, "samples must lie in 1 .. 65535");
    if (!(t0 >= 0.0 && t1 <= 1.0 && t0 <= t1)) return fail(ARMOUR_E_ARG, "the window must satisfy 0 <= t0 <= t1 <= 1");
    if (!p->reached) return fail(ARMOUR_E_STATE, "no batch: call a reach or plan entry first");
    const int W = p->W;
    if (int rc = check_traj(traj, W, false)) return rc;
    if (int rc = motion_reserve(p, samples)) return rc;
    const MotionCheck& m = p->motion;
    HIPCK(hipMemcpyAsync(m.traj, traj, sizeof(double) * W * TRAJ_DOUBLES, hipMemcpyHostToDevice, p->stream));
    launch_motion(p, m.traj, nullptr, t0, t1, samples);
    HIPCK(hipGetLastError());
    if (clearance) HIPCK(hipMemcpyAsync(clearance, m.clear, sizeof(double) * W, hipMemcpyDeviceToHost, p->stream));
    if (where) HIPCK(hipMemcpyAsync(where, m.where, sizeof(int) * 3 * W, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));
    return 0;
}

// ARMOUR_TRACK_KERNEL=serial (a test hook, read per call): the serial form of the rollouts, which
// computes the same bits as the row form; armour_track and armour_track_motion both ask here
static bool track_serial_asked() {
    const char* kv = std::getenv("ARMOUR_TRACK_KERNEL");
    return kv && !std::strcmp(kv, "serial");
}

// the argument checks of the tracking entries after their null checks: before any device work
static int track_check_args(armour_planner* p, int N, const double* traj, int S, const double* scale, const double* err0,
                            double t0, double t1, int steps) {
    if (int rc = not_available(p, "tracking rollouts are")) return rc;
    if (N < 1 || S < 1) return fail(ARMOUR_E_ARG, "num_traj and num_samples must be at least 1");
    if ((long)N * S > ARMOUR_TRACK_MAX_ROLLOUTS) return fail(ARMOUR_E_ARG, "num_traj x num_samples exceeds ARMOUR_TRACK_MAX_ROLLOUTS");
    if (steps < 1 || steps > ARMOUR_TRACK_MAX_STEPS) return fail(ARMOUR_E_ARG, "steps must lie in 1 .. ARMOUR_TRACK_MAX_STEPS");
    if (!(t0 >= 0.0 && t0 < t1 && t1 <= 1.0)) return fail(ARMOUR_E_ARG, "the window must satisfy 0 <= t0 < t1 <= 1");
    if (int rc = check_traj(traj, N, true)) return rc;
    return check_scale_err0(scale, err0, (size_t)N * S, p->NJ);
}

// launches the rollouts of `a` (device pointers; out and status are filled in here) between the events
// track.ev[0] and track.ev[1]: the plain kernels, the recording ones (x.rec) or a tracked episode's (x.win)
static int track_launch(armour_planner* p, TrackArgs a, const TrackExtra& x) {
    const long NR = (long)a.N * a.S;
    a.rp = p->d_rp;
    a.out = p->track.out;
    a.status = p->track.status;
    // the row form is the default (DESIGN.md section 4 has the measurement)
    const bool serial = track_serial_asked();
    const dim3 grid((unsigned)(serial ? (NR + TRACK_THREADS - 1) / TRACK_THREADS : (NR + TRACK_ROWS - 1) / TRACK_ROWS));
    const dim3 block(TRACK_THREADS);
    HIPCK(hipEventRecord(p->track.ev[0], p->stream));
    p->took(x.win ? (serial ? PATH_TRACK_SERIAL_EPISODE : PATH_TRACK_ROW_EPISODE)
            : x.rec ? (serial ? PATH_TRACK_SERIAL_REC : PATH_TRACK_ROW_REC) : (serial ? PATH_TRACK_SERIAL : PATH_TRACK_ROW));
    if (x.win && serial)
        hipLaunchKernelGGL(track_serial_episode_kernel, grid, block, 0, p->stream, a, x);
    else if (x.win)
        hipLaunchKernelGGL(track_row_episode_kernel, grid, block, 0, p->stream, a, x);
    else if (x.rec && serial)
        hipLaunchKernelGGL(track_serial_rec_kernel, grid, block, 0, p->stream, a, x);
    else if (x.rec)
        hipLaunchKernelGGL(track_row_rec_kernel, grid, block, 0, p->stream, a, x);
    else if (serial)
        hipLaunchKernelGGL(track_serial_kernel, grid, block, 0, p->stream, a);
    else
        hipLaunchKernelGGL(track_row_kernel, grid, block, 0, p->stream, a);
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(p->track.ev[1], p->stream));
    return 0;
}

// uploads the caller's inputs of N x S rollouts and launches them; rec (device,
// [steps / stride + 1][N * S][2][7]) selects the recording kernels, null the plain ones
static int track_upload_launch(armour_planner* p, int N, const double* traj, int S, const double* scale, const double* err0,
                               double t0, double t1, int steps, double* rec, int stride) {
    const long NR = (long)N * S;
    const int NJ = p->NJ;
    Rollouts& r = p->track;
    if (int rc = r.reserve(p->stream, NR)) return rc;
    HIPCK(hipMemcpyAsync(r.traj, traj, sizeof(double) * N * TRAJ_DOUBLES, hipMemcpyHostToDevice, p->stream));
    if (scale) HIPCK(hipMemcpyAsync(r.scale, scale, sizeof(double) * NR * 2 * NJ, hipMemcpyHostToDevice, p->stream));
    if (err0) HIPCK(hipMemcpyAsync(r.err0, err0, sizeof(double) * NR * 2 * NF, hipMemcpyHostToDevice, p->stream));
    TrackArgs a{};
    a.N = N;
    a.S = S;
    a.traj = r.traj;
    a.scale = scale ? r.scale : nullptr;
    a.err0 = err0 ? r.err0 : nullptr;
    a.t0 = t0;
    a.t1 = t1;
    a.steps = steps;
    return track_launch(p, a, TrackExtra{rec, stride, nullptr, nullptr});
}

// queues the copies of the rollouts' outputs the caller asked for
static int track_copy_out(armour_planner* p, long NR, armour_track_output* out) {
    const size_t n = (size_t)NR;
    struct { double* dst; long off; size_t len; } parts[] = {  // each field from its first element on
        {out->max_pos_err, track_out_max(TRACK_MAX_POS, NR, 0, 0), n * NF}, {out->max_vel_err, track_out_max(TRACK_MAX_VEL, NR, 0, 0), n * NF},
        {out->max_torque, track_out_max(TRACK_MAX_TORQUE, NR, 0, 0), n * NF}, {out->max_V, track_out_V(NR, 0), n},
        {out->max_robust, track_out_robust(NR, 0), n}, {out->end_state, track_out_end(NR, 0, 0, 0), n * 2 * NF}};
    for (const auto& part : parts)
        if (part.dst)
            HIPCK(hipMemcpyAsync(part.dst, p->track.out + part.off, sizeof(double) * part.len, hipMemcpyDeviceToHost, p->stream));
    if (out->status) HIPCK(hipMemcpyAsync(out->status, p->track.status, sizeof(int) * n, hipMemcpyDeviceToHost, p->stream));
    return 0;
}

int armour_track(armour_planner* p, int N, const double* traj, int S, const double* scale, const double* err0, double t0,
                 double t1, int steps, armour_track_output* out) {
    DeviceScope device_scope(p);
    if (!p || !traj || !out) return fail(ARMOUR_E_ARG, "null planner / traj / out");
    if (int rc = track_check_args(p, N, traj, S, scale, err0, t0, t1, steps)) return rc;
    if (int rc = track_upload_launch(p, N, traj, S, scale, err0, t0, t1, steps, nullptr, 1)) return rc;
    if (int rc = track_copy_out(p, (long)N * S, out)) return rc;
    HIPCK(hipStreamSynchronize(p->stream));
    return elapsed_ms(p->track.ev[0], p->track.ev[1], &out->track_ms);
}

// the true-arm check of the resident batch over the C recorded check points of its W x S rollouts
// (tracked.rec, with the rollouts' outputs in track.out / track.status), between the events tracked.ev[0] and [1];
// win (device, [W][2]; a tracked episode's step): worlds with an empty window are skipped
static int launch_state_check(armour_planner* p, int S, int C, const double* win) {
    const TrueArmCheck& k = p->tracked;
    const MotionArgs a = motion_args(p, S, win, k.pval, k.pidx);
    TrackedFinish f{C, k.rec, p->track.out, p->track.status, k.clear, k.where, k.flags, k.wclear, k.wwhere};
    HIPCK(hipEventRecord(k.ev[0], p->stream));
    hipLaunchKernelGGL(motion_state_check_kernel, dim3(C, S, p->W), dim3(MOTION_THREADS), 0, p->stream, a,
                       (const double*)k.rec, C);
    hipLaunchKernelGGL(motion_state_finish_kernel, dim3(p->W), dim3(64), 0, p->stream, a, f);
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(k.ev[1], p->stream));
    return 0;
}

int armour_track_motion(armour_planner* p, const double* traj, int S, const double* scale, const double* err0, double t0,
                        double t1, int steps, int check_samples, armour_track_motion_output* out) {
    DeviceScope device_scope(p);
    // (the rule between the two counts needs no planner: it is refused first)
    if (check_samples < 2) return fail(ARMOUR_E_ARG, "check_samples must be at least 2");
    if (steps >= 1 && steps % (check_samples - 1) != 0) return fail(ARMOUR_E_ARG, "steps must be a multiple of check_samples - 1");
    if (!p || !traj || !out) return fail(ARMOUR_E_ARG, "null planner / traj / out");
    if (!p->armtd && !p->set.eval_f32 && !p->reached) return fail(ARMOUR_E_STATE, "no batch: call a reach or plan entry first");
    const int W = p->reached ? p->W : 1;
    if (int rc = track_check_args(p, W, traj, S, scale, err0, t0, t1, steps)) return rc;
    if (S > 65535) return fail(ARMOUR_E_ARG, "num_samples must be at most 65535");
    const int C = check_samples, stride = steps / (C - 1);
    const long NR = (long)W * S;
    TrueArmCheck& k = p->tracked;
    if (int rc = k.reserve(p->stream, NR * C, p->Wmax)) return rc;
    if (int rc = track_upload_launch(p, W, traj, S, scale, err0, t0, t1, steps, k.rec, stride)) return rc;
    if (int rc = launch_state_check(p, S, C, nullptr)) return rc;
    if (int rc = track_copy_out(p, NR, &out->track)) return rc;
    const size_t n = (size_t)NR;
    if (out->clearance) HIPCK(hipMemcpyAsync(out->clearance, k.clear, sizeof(double) * n, hipMemcpyDeviceToHost, p->stream));
    if (out->where) HIPCK(hipMemcpyAsync(out->where, k.where, sizeof(int) * 3 * n, hipMemcpyDeviceToHost, p->stream));
    if (out->flags) HIPCK(hipMemcpyAsync(out->flags, k.flags, sizeof(int) * n, hipMemcpyDeviceToHost, p->stream));
    if (out->world_clearance)
        HIPCK(hipMemcpyAsync(out->world_clearance, k.wclear, sizeof(double) * W, hipMemcpyDeviceToHost, p->stream));
    if (out->world_where) HIPCK(hipMemcpyAsync(out->world_where, k.wwhere, sizeof(int) * 4 * W, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));
    if (int rc = elapsed_ms(p->track.ev[0], p->track.ev[1], &out->track.track_ms)) return rc;
    return elapsed_ms(k.ev[0], k.ev[1], &out->check_ms);
}

// ---- the roadmap high-level planner (roadmap_kernels.hip) ----
static int roadmap_check_config(const armour_roadmap_config* c) {
    if (c->num_nodes < 2 || c->num_nodes > ARMOUR_ROADMAP_MAX_NODES)
        return fail(ARMOUR_E_ARG, "num_nodes must lie in 2 .. ARMOUR_ROADMAP_MAX_NODES");
    if (!std::isfinite(c->connect_radius) || !(c->connect_radius > 0.0 && c->connect_radius <= 100.0))
        return fail(ARMOUR_E_ARG, "connect_radius must be finite and lie in (0, 100]");
    if (!std::isfinite(c->edge_step) || !(c->edge_step > 0.0)) return fail(ARMOUR_E_ARG, "edge_step must be finite and positive");
    if (c->connect_radius / c->edge_step > 4096.0) return fail(ARMOUR_E_ARG, "connect_radius / edge_step must be at most 4096");
    if (!std::isfinite(c->margin) || !(c->margin >= 0.0)) return fail(ARMOUR_E_ARG, "margin must be finite and at least 0");
    return 0;
}

// The build on the resident worlds (upload_worlds has run): vertices, candidate edges, edge samples,
// adjacency, cost-to-go. On any failure the previous roadmap is gone and nothing else has changed.
static int roadmap_build(armour_planner* p, const armour_roadmap_config* cfg, const double* nodes, const double* goals,
                         armour_roadmap_stats* stats) {
    Roadmap& rm = p->roadmap;
    const int W = p->W, N = cfg->num_nodes, V = N + 1;
    int rc = 0;
    if ((rc = check_values("nodes", nodes, W * N * NF, ARMOUR_MAX_ABS_ANGLE))) return rc;
    if ((rc = check_values("goals", goals, W * NF, ARMOUR_MAX_ABS_ANGLE))) return rc;
    rm.valid = false;
    const size_t rows = (size_t)W * V;
    std::vector<double> verts(rows * NF);
    for (int w = 0; w < W; w++) {
        std::memcpy(&verts[(size_t)w * V * NF], nodes + (size_t)w * N * NF, sizeof(double) * N * NF);
        std::memcpy(&verts[((size_t)w * V + N) * NF], goals + (size_t)w * NF, sizeof(double) * NF);
    }
    RoadmapDev& r = rm.dev;
    const size_t Wm = (size_t)p->Wmax;
    if ((rc = rm.grow.reserve(p->stream, (long)rows,
                              {GrowSet::buf(rm.verts, rows * NF), GrowSet::buf(r.clr, rows), GrowSet::buf(r.free, rows),
                               GrowSet::buf(r.adj, rows * ROADMAP_WORDS), GrowSet::buf(r.togo, rows), GrowSet::buf(r.next, rows),
                               GrowSet::buf(r.row_edges, rows), GrowSet::buf(r.row_samples, rows), GrowSet::buf(rm.row_eoff, rows + 1),
                               GrowSet::buf(rm.row_soff, rows + 1), GrowSet::buf(r.stats, (size_t)ROADMAP_STATS),
                               GrowSet::buf(rm.q, Wm * NF), GrowSet::buf(rm.q_des, Wm * NF), GrowSet::buf(rm.entry, Wm),
                               GrowSet::buf(rm.left, Wm), GrowSet::buf(rm.ep_entry, Wm), GrowSet::buf(rm.ep_left, Wm)},
                              "hipMalloc failed for the roadmap's buffers (worlds x vertices)")))
        return rc;
    for (hipEvent_t& e : rm.bev)
        if (!e) HIPCK(hipEventCreate(&e));
    r.m = motion_args(p, 1, nullptr, nullptr, nullptr);
    r.N = N;
    r.V = V;
    r.radius = cfg->connect_radius;
    r.step = cfg->edge_step;
    r.margin = cfg->margin;
    r.verts = rm.verts;
    r.row_eoff = rm.row_eoff;
    r.row_soff = rm.row_soff;
    r.E = 0;
    hipStream_t st = p->stream;
    HIPCK(hipMemcpyAsync(rm.verts, verts.data(), sizeof(double) * verts.size(), hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(r.stats, 0, sizeof(unsigned long long) * ROADMAP_STATS, st));
    HIPCK(hipMemsetAsync(r.adj, 0, sizeof(unsigned) * rows * ROADMAP_WORDS, st));
    const dim3 vg((V + ROADMAP_THREADS - 1) / ROADMAP_THREADS, W), tb(ROADMAP_THREADS);
    HIPCK(hipEventRecord(rm.bev[0], st));
    hipLaunchKernelGGL(roadmap_vertex_kernel, vg, tb, 0, st, r);
    HIPCK(hipEventRecord(rm.bev[1], st));
    hipLaunchKernelGGL(roadmap_edges_kernel<false>, vg, tb, 0, st, r);
    HIPCK(hipEventRecord(rm.bev[2], st));
    HIPCK(hipGetLastError());
    // the host scans the rows' counts: the edge list is in (world, i, j) order whatever ran first
    std::vector<int> cnt(2 * rows), off(2 * (rows + 1));
    HIPCK(hipMemcpyAsync(cnt.data(), r.row_edges, sizeof(int) * rows, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(cnt.data() + rows, r.row_samples, sizeof(int) * rows, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    long long E = 0, S = 0, world_samples = 0, most = 0;
    for (size_t i = 0; i < rows; i++) {
        if (i % V == 0) world_samples = 0;
        off[i] = (int)E;
        off[rows + 1 + i] = (int)S;
        E += cnt[i];
        S += cnt[rows + i];
        world_samples += cnt[rows + i];
        most = std::max(most, world_samples);
        if (E > INT_MAX || S > INT_MAX)
            return fail(ARMOUR_E_CAPACITY, "the roadmap's candidate edges or edge samples exceed 2^31 - 1");
    }
    off[rows] = (int)E;
    off[2 * rows + 1] = (int)S;
    const size_t ne = (size_t)E, ns = (size_t)S;
    if ((rc = rm.edges.reserve(st, (long)E, {GrowSet::buf(r.e_row, ne), GrowSet::buf(r.e_j, ne), GrowSet::buf(r.e_n, ne),
                                            GrowSet::buf(r.e_soff, ne)},
                               "hipMalloc failed for the roadmap's edge list (candidate edges)")))
        return rc;
    if ((rc = rm.samples.reserve(st, (long)S, {GrowSet::buf(r.ok, ns)}, "hipMalloc failed for the roadmap's edge samples")))
        return rc;
    r.E = (int)E;
    HIPCK(hipMemcpyAsync(rm.row_eoff, off.data(), sizeof(int) * (rows + 1), hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(rm.row_soff, off.data() + rows + 1, sizeof(int) * (rows + 1), hipMemcpyHostToDevice, st));
    HIPCK(hipEventRecord(rm.bev[3], st));
    if (E > 0) hipLaunchKernelGGL(roadmap_edges_kernel<true>, vg, tb, 0, st, r);
    HIPCK(hipEventRecord(rm.bev[4], st));
    if (S > 0)
        hipLaunchKernelGGL(roadmap_sample_kernel, dim3((unsigned)((most + ROADMAP_THREADS - 1) / ROADMAP_THREADS), W), tb, 0, st, r);
    if (E > 0) hipLaunchKernelGGL(roadmap_fold_kernel, dim3((unsigned)((E + ROADMAP_THREADS - 1) / ROADMAP_THREADS)), tb, 0, st, r);
    HIPCK(hipEventRecord(rm.bev[5], st));
    hipLaunchKernelGGL(roadmap_togo_kernel, dim3(W), dim3(ROADMAP_MAX_V), 0, st, r);
    HIPCK(hipEventRecord(rm.bev[6], st));
    HIPCK(hipGetLastError());
    unsigned long long hs[ROADMAP_STATS];
    HIPCK(hipMemcpyAsync(hs, r.stats, sizeof(hs), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));  // (also: `verts`, `off` outlive their copies)
    if (stats) {
        stats->free_nodes = (long long)hs[ROADMAP_STAT_FREE];
        stats->candidate_edges = E;
        stats->edges = (long long)hs[ROADMAP_STAT_EDGES];
        stats->edge_samples = S;
        stats->reachable = (long long)hs[ROADMAP_STAT_REACHABLE];
        stats->relax_rounds_max = (int)hs[ROADMAP_STAT_ROUNDS];
        double a = 0, b = 0;
        for (double& ms : stats->build_ms) ms = 0.0;  // (a failed read leaves 0)
        (void)elapsed_ms(rm.bev[0], rm.bev[1], &stats->build_ms[0]);
        (void)elapsed_ms(rm.bev[1], rm.bev[2], &a);
        (void)elapsed_ms(rm.bev[3], rm.bev[4], &b);
        stats->build_ms[1] = a + b;
        (void)elapsed_ms(rm.bev[4], rm.bev[5], &stats->build_ms[2]);
        (void)elapsed_ms(rm.bev[5], rm.bev[6], &stats->build_ms[3]);
    }
    rm.valid = true;
    return 0;
}

static void launch_roadmap_waypoint(armour_planner* p, const RoadmapQuery& y) {
    hipLaunchKernelGGL(roadmap_waypoint_kernel, dim3(p->W), dim3(ROADMAP_THREADS), 0, p->stream, p->roadmap.dev, y);
}
// the episode's query: the states' own q and q_des; kind null: the running worlds (armour_episode_roadmap)
static RoadmapQuery roadmap_episode_query(armour_planner* p, const int* kind) {
    RoadmapQuery y{};
    y.lookahead = p->ep.dev.lookahead;
    y.st = p->ep.dev.st;
    y.kind = kind;
    y.entry = p->roadmap.ep_entry;
    y.path_left = p->roadmap.ep_left;
    return y;
}

int armour_roadmap_build(armour_planner* p, const armour_roadmap_config* cfg, const double* nodes, const double* goals,
                         armour_roadmap_stats* stats) {
    DeviceScope device_scope(p);
    if (!p || !cfg || !nodes || !goals) return fail(ARMOUR_E_ARG, "null planner / cfg / nodes / goals");
    if (int rc = not_available(p, "the roadmap is")) return rc;
    if (int rc = roadmap_check_config(cfg)) return rc;
    if (!p->reached) return fail(ARMOUR_E_STATE, "no batch: call a reach or plan entry first");
    if (p->ep.on && p->roadmap.episode)
        return fail(ARMOUR_E_STATE, "the running episode takes its waypoints from the roadmap (armour_episode_roadmap)");
    return roadmap_build(p, cfg, nodes, goals, stats);
}

static int no_roadmap() {
    return fail(ARMOUR_E_STATE, "no roadmap: call armour_roadmap_build first (any other batch entry invalidates one)");
}

int armour_roadmap_get(armour_planner* p, int w, double* node_clearance, int* is_free, unsigned* adjacency, double* togo,
                       int* next) {
    DeviceScope device_scope(p);
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    if (!p->roadmap.valid) return no_roadmap();
    if (w < 0 || w >= p->W) return fail(ARMOUR_E_ARG, "world index out of range");
    const RoadmapDev& r = p->roadmap.dev;
    const size_t V = (size_t)r.V, at = (size_t)w * V;
    hipStream_t st = p->stream;
    if (node_clearance) HIPCK(hipMemcpyAsync(node_clearance, r.clr + at, sizeof(double) * V, hipMemcpyDeviceToHost, st));
    if (is_free) HIPCK(hipMemcpyAsync(is_free, r.free + at, sizeof(int) * V, hipMemcpyDeviceToHost, st));
    if (adjacency)
        HIPCK(hipMemcpyAsync(adjacency, r.adj + at * ROADMAP_WORDS, sizeof(unsigned) * V * ROADMAP_WORDS, hipMemcpyDeviceToHost, st));
    if (togo) HIPCK(hipMemcpyAsync(togo, r.togo + at, sizeof(double) * V, hipMemcpyDeviceToHost, st));
    if (next) HIPCK(hipMemcpyAsync(next, r.next + at, sizeof(int) * V, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    return 0;
}

int armour_roadmap_waypoint(armour_planner* p, const double* q, double lookahead, double* q_des, int* entry,
                            double* path_left) {
    DeviceScope device_scope(p);
    if (!p || !q) return fail(ARMOUR_E_ARG, "null planner / q");
    if (!std::isfinite(lookahead) || !(lookahead > 0.0)) return fail(ARMOUR_E_ARG, "lookahead must be finite and positive");
    if (!p->roadmap.valid) return no_roadmap();
    const int W = p->W;
    if (int rc = check_values("q", q, W * NF, ARMOUR_MAX_ABS_ANGLE)) return rc;
    Roadmap& rm = p->roadmap;
    hipStream_t st = p->stream;
    HIPCK(hipMemcpyAsync(rm.q, q, sizeof(double) * W * NF, hipMemcpyHostToDevice, st));
    RoadmapQuery y{};
    y.lookahead = lookahead;
    y.q = rm.q;
    y.q_des = rm.q_des;
    y.entry = rm.entry;
    y.path_left = rm.left;
    launch_roadmap_waypoint(p, y);
    HIPCK(hipGetLastError());
    if (q_des) HIPCK(hipMemcpyAsync(q_des, rm.q_des, sizeof(double) * W * NF, hipMemcpyDeviceToHost, st));
    if (entry) HIPCK(hipMemcpyAsync(entry, rm.entry, sizeof(int) * W, hipMemcpyDeviceToHost, st));
    if (path_left) HIPCK(hipMemcpyAsync(path_left, rm.left, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    return 0;
}

static int episode_read(armour_planner* p);
int armour_episode_roadmap(armour_planner* p, const armour_roadmap_config* cfg, const double* nodes) {
    DeviceScope device_scope(p);
    if (!p || !cfg || !nodes) return fail(ARMOUR_E_ARG, "null planner / cfg / nodes");
    if (int rc = not_available(p, "the roadmap is")) return rc;
    if (int rc = roadmap_check_config(cfg)) return rc;
    if (!p->ep.on) return no_episode();
    if (p->ep.stepped) return fail(ARMOUR_E_STATE, "the episode has taken a step: the roadmap is given before the first step");
    p->roadmap.episode = false;
    if (int rc = roadmap_build(p, cfg, nodes, p->ep.goals.data(), nullptr)) return rc;
    launch_roadmap_waypoint(p, roadmap_episode_query(p, nullptr));
    HIPCK(hipGetLastError());
    if (int rc = episode_read(p)) return rc;
    p->roadmap.episode = true;
    return 0;
}

int armour_episode_get_roadmap(armour_planner* p, int* entry, double* path_left) {
    DeviceScope device_scope(p);
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    if (!p->ep.on) return no_episode();
    if (!p->roadmap.episode) return fail(ARMOUR_E_STATE, "the episode has no roadmap: call armour_episode_roadmap after armour_episode_begin");
    const Roadmap& rm = p->roadmap;
    if (entry) HIPCK(hipMemcpyAsync(entry, rm.ep_entry, sizeof(int) * p->W, hipMemcpyDeviceToHost, p->stream));
    if (path_left) HIPCK(hipMemcpyAsync(path_left, rm.ep_left, sizeof(double) * p->W, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));
    return 0;
}

static int episode_read(armour_planner* p) {
    p->ep.host.resize(p->W);
    HIPCK(hipMemcpyAsync(p->ep.host.data(), p->ep.dev.st, sizeof(armour_episode_state) * p->W, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));
    return 0;
}

int armour_episode_begin(armour_planner* p, int W, const armour_world* worlds, const double* goals,
                         const armour_episode_config* cfg) {
    DeviceScope device_scope(p);
    if (!p || !worlds || !goals || !cfg) return fail(ARMOUR_E_ARG, "null argument");
    if (int rc = not_available(p, "episodes are")) return rc;
    if (!(cfg->lookahead > 0.0) || !std::isfinite(cfg->lookahead) || !(cfg->goal_radius >= 0.0) ||
        !std::isfinite(cfg->goal_radius) || cfg->check_samples < 2 || cfg->check_samples > 65535)
        return fail(ARMOUR_E_ARG, "episode config: lookahead > 0, goal_radius >= 0, 2 <= check_samples <= 65535");
    if (W <= 0 || W > p->Wmax) return fail(ARMOUR_E_ARG, "num_worlds out of range");
    p->reached = p->planned = p->evaluated = p->ep.on = false;
    p->roadmap.valid = p->roadmap.episode = false;
    int rc = 0;
    if ((rc = check_values("goals", goals, W * NF, ARMOUR_MAX_ABS_ANGLE))) return rc;
    // the worlds' q_des is ignored: the waypoints are written on the device
    std::vector<armour_world> ws(worlds, worlds + W);
    for (armour_world& w : ws) std::memcpy(w.q_des, w.q0, sizeof(w.q_des));
    if ((rc = upload_worlds(p, W, ws.data(), true))) return rc;
    if ((rc = motion_reserve(p, cfg->check_samples))) return rc;
    EpisodeDev& e = p->ep.dev;
    if (!e.st) {
        double* goal = nullptr;
        const size_t Wm = (size_t)p->Wmax;
        if ((rc = p->alloc(&e.st, Wm)) || (rc = p->alloc(&goal, Wm * NF)) || (rc = p->alloc(&e.pend, Wm * TRAJ_DOUBLES)) ||
            (rc = p->alloc(&e.has_pend, Wm)) || (rc = p->alloc(&e.kind, Wm)) || (rc = p->alloc(&e.exec, Wm * TRAJ_DOUBLES)) ||
            (rc = p->alloc(&e.win, 2 * Wm)) || (rc = p->alloc(&p->ep.accept, Wm)) || (rc = p->ep.events(4)))
            return rc;
        e.goal = goal;
        e.accept = p->ep.accept;
    }
    e.rp = p->d_rp;
    e.W = W;
    e.S = cfg->check_samples;
    e.lookahead = cfg->lookahead;
    e.goal_radius = cfg->goal_radius;
    e.clearance = p->motion.clear;
    e.where = p->motion.where;
    HIPCK(hipMemcpyAsync(const_cast<double*>(e.goal), goals, sizeof(double) * W * NF, hipMemcpyHostToDevice, p->stream));
    hipLaunchKernelGGL(episode_begin_kernel, dim3((W + 63) / 64), dim3(64), 0, p->stream, e, p->q0, p->qd0, p->qdd0);
    HIPCK(hipGetLastError());
    if ((rc = episode_read(p))) return rc;  // (also: `goals` is the caller's, its copy has finished)
    p->ep.on = true;
    p->ept.on = p->ep.stepped = false;
    p->ep.goals.assign(goals, goals + (size_t)W * NF);
    return 0;
}

int armour_episode_track(armour_planner* p, const armour_episode_track_config* cfg) {
    DeviceScope device_scope(p);
    if (!p || !cfg) return fail(ARMOUR_E_ARG, "null argument");
    if (!p->ep.on) return no_episode();
    if (p->ep.stepped) return fail(ARMOUR_E_STATE, "the episode has taken a step: tracking is enabled before the first step");
    const int W = p->W, S = cfg->num_samples, NJ = p->NJ, C = p->ep.dev.S;
    if (S < 1 || S > 65535) return fail(ARMOUR_E_ARG, "num_samples must lie in 1 .. 65535");
    if ((long)W * S > ARMOUR_TRACK_MAX_ROLLOUTS) return fail(ARMOUR_E_ARG, "num_worlds x num_samples exceeds ARMOUR_TRACK_MAX_ROLLOUTS");
    if (cfg->steps < 1 || cfg->steps > ARMOUR_TRACK_MAX_STEPS) return fail(ARMOUR_E_ARG, "steps must lie in 1 .. ARMOUR_TRACK_MAX_STEPS");
    if (cfg->steps % (C - 1) != 0) return fail(ARMOUR_E_ARG, "steps must be a multiple of the episode's check_samples - 1");
    const size_t NR = (size_t)W * S;
    if (int rc = check_scale_err0(cfg->scale, cfg->err0, NR, NJ)) return rc;
    // the true arms start from the episode's start states plus err0
    std::vector<double> start(NR * 2 * NF);
    for (size_t r = 0; r < NR; r++) {
        const armour_episode_state& st = p->ep.host[r / S];
        for (int j = 0; j < NF; j++) {
            const double* e0 = cfg->err0 ? cfg->err0 + r * 2 * NF : nullptr;
            start[r * 2 * NF + j] = e0 ? st.q[j] + e0[j] : st.q[j];
            start[r * 2 * NF + NF + j] = e0 ? st.qd[j] + e0[NF + j] : st.qd[j];
            if (!std::isfinite(start[r * 2 * NF + j]) || !std::isfinite(start[r * 2 * NF + NF + j]))
                return fail(ARMOUR_E_ARG, "err0 leads to a start state that is not finite");
        }
    }
    TrackedEpisode& te = p->ept;
    EpisodeTrackDev& t = te.dev;
    const size_t n = (size_t)p->Wmax * S, Wm = (size_t)p->Wmax;
    if (int rc = te.grow.reserve(p->stream, (long)n,
                                 {GrowSet::buf(te.state, n * 2 * NF), GrowSet::buf(te.scale, n * 2 * MAX_J), GrowSet::buf(t.flags, n),
                                  GrowSet::buf(t.traj, Wm * TRAJ_DOUBLES), GrowSet::buf(t.win, Wm * 2), GrowSet::buf(t.rec, Wm)},
                                 "hipMalloc failed for the tracked episode's buffers (max_worlds x num_samples)"))
        return rc;
    if (int rc = p->track.reserve(p->stream, (long)NR)) return rc;
    if (int rc = p->tracked.reserve(p->stream, (long)NR * C, p->Wmax)) return rc;
    t.S = S;
    t.stop_input = cfg->stop_on_input != 0;
    t.stop_bound = cfg->stop_on_bound != 0;
    t.stop_limit = cfg->stop_on_limit != 0;
    te.steps = cfg->steps;
    te.scaled = cfg->scale != nullptr;
    HIPCK(hipMemcpyAsync(te.state, start.data(), sizeof(double) * NR * 2 * NF, hipMemcpyHostToDevice, p->stream));
    if (cfg->scale) HIPCK(hipMemcpyAsync(te.scale, cfg->scale, sizeof(double) * NR * 2 * NJ, hipMemcpyHostToDevice, p->stream));
    hipLaunchKernelGGL(episode_track_begin_kernel, dim3((W + 63) / 64), dim3(64), 0, p->stream, p->ep.dev, t);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(p->stream));  // (`start` and the caller's arrays outlive their copies)
    te.on = true;
    return 0;
}

// step (c) of a tracked episode, after episode_advance_kernel: the true arms along what each running
// world executes, the check of their recorded states, and the fold into the records and the status
static int episode_track_step(armour_planner* p) {
    const int W = p->W, C = p->ep.dev.S;
    const TrackedEpisode& te = p->ept;
    EpisodeTrackDev& t = p->ept.dev;
    const long NR = (long)W * t.S;
    // (another tracking entry between two steps may have regrown these; their contents live one step)
    if (int rc = p->track.reserve(p->stream, NR)) return rc;
    if (int rc = p->tracked.reserve(p->stream, NR * C, p->Wmax)) return rc;
    t.out = p->track.out;
    t.rflags = p->tracked.flags;
    t.wclear = p->tracked.wclear;
    t.wwhere = p->tracked.wwhere;
    const dim3 wg((W + 63) / 64), wb(64);
    hipLaunchKernelGGL(episode_track_choose_kernel, wg, wb, 0, p->stream, p->ep.dev, t);
    TrackArgs a{};
    a.N = W;
    a.S = t.S;
    a.traj = t.traj;
    a.scale = te.scaled ? te.scale : nullptr;
    a.steps = te.steps;
    if (int rc = track_launch(p, a, TrackExtra{p->tracked.rec, te.steps / (C - 1), t.win, te.state})) return rc;
    if (int rc = launch_state_check(p, t.S, C, t.win)) return rc;
    hipLaunchKernelGGL(episode_track_fold_kernel, wg, wb, 0, p->stream, p->ep.dev, t);
    HIPCK(hipGetLastError());
    return 0;
}

int armour_episode_get_tracked(armour_planner* p, armour_episode_tracked* records, double* true_state, int* flags, double* ms) {
    DeviceScope device_scope(p);
    if (!p || !records) return fail(ARMOUR_E_ARG, "null argument");
    if (!p->ep.on) return no_episode();
    if (!p->ept.on) return fail(ARMOUR_E_STATE, "tracking is not enabled: call armour_episode_track after armour_episode_begin");
    const EpisodeTrackDev& t = p->ept.dev;
    const size_t W = (size_t)p->W, NR = W * t.S;
    HIPCK(hipMemcpyAsync(records, t.rec, sizeof(armour_episode_tracked) * W, hipMemcpyDeviceToHost, p->stream));
    if (true_state) HIPCK(hipMemcpyAsync(true_state, p->ept.state, sizeof(double) * NR * 2 * NF, hipMemcpyDeviceToHost, p->stream));
    if (flags) HIPCK(hipMemcpyAsync(flags, t.flags, sizeof(int) * NR, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));
    if (ms) {
        ms[0] = ms[1] = 0.0;  // (before the first step; a failed read leaves 0 too)
        if (p->ep.stepped) {
            (void)elapsed_ms(p->track.ev[0], p->track.ev[1], &ms[0]);
            (void)elapsed_ms(p->tracked.ev[0], p->tracked.ev[1], &ms[1]);
        }
    }
    return 0;
}

int armour_episode_step(armour_planner* p, const int* reject, armour_result* results, armour_timing* timing,
                        double* episode_ms) {
    DeviceScope device_scope(p);
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    if (!p->ep.on) return no_episode();
    const int W = p->W;
    const EpisodeDev& e = p->ep.dev;
    const hipEvent_t* ev = p->ep.ev;
    int rc = 0;
    auto t0 = std::chrono::steady_clock::now();
    // (a) the pending state becomes the batch input; reach and solve on the resident arrays
    hipLaunchKernelGGL(episode_swap_kernel, dim3((W * NF + 255) / 256), dim3(256), 0, p->stream, e, p->q0, p->qd0, p->qdd0,
                       p->qdes);
    HIPCK(hipGetLastError());
    if (p->rstream != p->stream) HIPCK(hipStreamSynchronize(p->stream));  // the reach stream reads q0 / qd0 / qdd0
    p->reached = p->planned = p->evaluated = false;
    std::vector<armour_result> own;
    if (!results) {
        own.resize(W);
        results = own.data();
    }
    if ((rc = plan_uploaded(p, results, timing, t0))) {
        p->ep.on = false;
        return rc;
    }
    // (b) what each running world executes; (c) check, advance
    std::vector<int> accept(W);
    for (int w = 0; w < W; w++) accept[w] = results[w].feasible && !(reject && reject[w]) ? 1 : 0;
    HIPCK(hipMemcpyAsync(p->ep.accept, accept.data(), sizeof(int) * W, hipMemcpyHostToDevice, p->stream));
    const dim3 wg((W + 63) / 64), wb(64);
    HIPCK(hipEventRecord(ev[0], p->stream));
    hipLaunchKernelGGL(episode_choose_kernel, wg, wb, 0, p->stream, e, (const double*)p->d.ws,
                       (long)(sizeof(WorldState) / sizeof(double)), p->q0, p->qd0, p->qdd0);
    HIPCK(hipEventRecord(ev[1], p->stream));
    launch_motion(p, e.exec, e.win, 0.0, 0.0, e.S);
    HIPCK(hipEventRecord(ev[2], p->stream));
    hipLaunchKernelGGL(episode_advance_kernel, wg, wb, 0, p->stream, e);
    if (p->roadmap.episode) launch_roadmap_waypoint(p, roadmap_episode_query(p, e.kind));
    HIPCK(hipEventRecord(ev[3], p->stream));
    HIPCK(hipGetLastError());
    p->ep.stepped = true;
    if (p->ept.on && (rc = episode_track_step(p))) return rc;
    if ((rc = episode_read(p))) return rc;  // (ends in a synchronisation: `accept` outlives its copy)
    if (episode_ms) {
        double a = 0, b = 0, c = 0;  // (a failed read leaves 0)
        (void)elapsed_ms(ev[0], ev[1], &a);
        (void)elapsed_ms(ev[1], ev[2], &b);
        (void)elapsed_ms(ev[2], ev[3], &c);
        episode_ms[0] = b;
        episode_ms[1] = a + c;
    }
    int running = 0;
    for (const armour_episode_state& s : p->ep.host) running += s.status == 0;
    return running;
}

int armour_episode_get(armour_planner* p, armour_episode_state* states) {
    if (!p || !states) return fail(ARMOUR_E_ARG, "null argument");
    if (!p->ep.on) return no_episode();
    std::memcpy(states, p->ep.host.data(), sizeof(armour_episode_state) * p->ep.host.size());
    return 0;
}

int armour_get_constraints(armour_planner* p, int w, double* g) {
    DeviceScope device_scope(p);
    if (!p || !g) return fail(ARMOUR_E_ARG, "null argument");
    if (!p->planned) return fail(ARMOUR_E_STATE, "no plan");
    if (w < 0 || w >= p->W) return fail(ARMOUR_E_ARG, "world index out of range");
    const int cur = p->h_ws[w].cur;
    HIPCK(hipMemcpy(g, p->d.g + gidx(p->d, cur, w, 0), sizeof(double) * armour_num_constraints(p, p->Ow[w]), hipMemcpyDeviceToHost));
    return 0;
}

int armour_get_link_centers(armour_planner* p, int w, double* c) {
    DeviceScope device_scope(p);
    if (!p || !c) return fail(ARMOUR_E_ARG, "null argument");
    if (!p->planned && !p->evaluated) return fail(ARMOUR_E_STATE, "no plan and no evaluated point");
    if (w < 0 || w >= p->W) return fail(ARMOUR_E_ARG, "world index out of range");
    // after a plan: slot 2 (feasible_kernel's copy of the final iterate's centres); after
    // armour_eval_constraints: slot 0, where eval_kernel_t (EVAL_POINT) wrote those of its point
    const int slot = p->planned ? 2 : 0;
    HIPCK(hipMemcpy(c, p->d.link_c + slot * p->d.lcs + (size_t)w * p->T * p->NJ * 3, sizeof(double) * p->T * p->NJ * 3, hipMemcpyDeviceToHost));
    return 0;
}

int armour_get_link_generators(armour_planner* p, int w, double* gens) {
    DeviceScope device_scope(p);
    if (!p || !gens) return fail(ARMOUR_E_ARG, "null argument");
    if (!p->reached) return fail(ARMOUR_E_STATE, "no reach set");
    if (w < 0 || w >= p->W) return fail(ARMOUR_E_ARG, "world index out of range");
    const size_t n = (size_t)p->T * p->NJ;
    std::vector<double> cm(n * 18);
    HIPCK(hipMemcpy(cm.data(), p->ro.link_gens + (size_t)w * n * 18, sizeof(double) * n * 18, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < n; j++)
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 6; c++) gens[j * 18 + r * 6 + c] = cm[j * 18 + r + 3 * c];
    return 0;
}

int armour_get_torque_radius(armour_planner* p, int w, double* radius) {
    DeviceScope device_scope(p);
    if (!p || !radius) return fail(ARMOUR_E_ARG, "null argument");
    if (!p->reached) return fail(ARMOUR_E_STATE, "no reach set");
    if (w < 0 || w >= p->W) return fail(ARMOUR_E_ARG, "world index out of range");
    HIPCK(hipMemcpy(radius, p->ro.torque_radius + (size_t)w * p->T * NF, sizeof(double) * p->T * NF, hipMemcpyDeviceToHost));
    return 0;
}

int armour_get_reach_profile(armour_planner* p, unsigned long long* cycles_terms, int capacity) {
    DeviceScope device_scope(p);
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    if (!p->d_prof) return fail(ARMOUR_E_STATE, "op profiling is off (set ARMOUR_PROFILE_OPS before armour_create)");
    // capacity in pairs: nops + 8 -> per-op [cycles, terms] + 16 phase totals; nops + 8 + 4 * OP_NCODES
    // adds the bundle engine's phase cycles per op code [OP_NCODES][8]
    // adds the bundle engine's phase cycles per op code [OP_NCODES][8]; + ceil(max_worlds * T / 64)
    // adds every bundle's [start, end] wall clock (ARMOUR_PROFILE_OPS=3)
    if (cycles_terms && capacity >= p->nops + 8) {
        const size_t nb = ((size_t)p->Wmax * p->T + lane::LG - 1) / lane::LG;
        const size_t n = capacity >= p->nops + 8 + 4 * OP_NCODES + (long)nb ? 2 * p->nops + 16 + 8 * OP_NCODES + 2 * nb
                         : capacity >= p->nops + 8 + 4 * OP_NCODES ? 2 * p->nops + 16 + 8 * OP_NCODES : 2 * p->nops + 16;
        HIPCK(hipMemcpy(cycles_terms, p->d_prof, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
    }
    return p->nops;
}

int armour_get_reach_dump(armour_planner* p, double* dump, int capacity) {
    DeviceScope device_scope(p);
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    if (!p->d_dump) return fail(ARMOUR_E_STATE, "op dump is off (set ARMOUR_DUMP_OPS before armour_create)");
    if (!p->lane_engine && p->has_lane)
        return fail(ARMOUR_E_STATE, "the op dump follows the bundle engine, and the last batch ran on the per-job engine");
    if (dump && capacity >= p->nops) {
        if (p->lane_engine) {
            // [nops][DUMP_W][64] of bundle 0: lane ARMOUR_DUMP_LANE (default 0) = job of that index
            const char* ls = std::getenv("ARMOUR_DUMP_LANE");
            const int l = ls ? std::atoi(ls) & 63 : 0;
            std::vector<double> all((size_t)p->nops * DUMP_W * lane::LG);
            HIPCK(hipMemcpy(all.data(), p->d_dump, sizeof(double) * all.size(), hipMemcpyDeviceToHost));
            for (int k = 0; k < p->nops * DUMP_W; k++) dump[k] = all[(size_t)k * lane::LG + l];
        } else {
            HIPCK(hipMemcpy(dump, p->d_dump, sizeof(double) * DUMP_W * p->nops, hipMemcpyDeviceToHost));
        }
    }
    return p->nops;
}

int armour_get_monomial_counts(armour_planner* p, int w, int* link_counts, int* torque_counts) {
    DeviceScope device_scope(p);
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    if (!p->reached) return fail(ARMOUR_E_STATE, "no reach set");
    if (w < 0 || w >= p->W) return fail(ARMOUR_E_ARG, "world index out of range");
    const size_t j0 = (size_t)w * p->T;
    if (link_counts)
        HIPCK(hipMemcpy(link_counts, p->ro.link_cnt + j0 * p->NJ, sizeof(int) * p->T * p->NJ, hipMemcpyDeviceToHost));
    if (torque_counts)
        HIPCK(hipMemcpy(torque_counts, p->ro.tq_cnt + j0 * NF, sizeof(int) * p->T * NF, hipMemcpyDeviceToHost));
    return 0;
}

int armour_get_reach_span(armour_planner* p, double* span_ms) {
    if (!p || !span_ms) return fail(ARMOUR_E_ARG, "null planner or output");
    if (!p->reached) return fail(ARMOUR_E_STATE, "no reach set");
    *span_ms = p->last_span_ms;
    return p->last_span_ms >= 0 ? 0 : fail(ARMOUR_E_STATE, "no device clock span for the last reach");
}

int armour_get_plane_cache_stats(armour_planner* p, long long* out, int n) {
    DeviceScope device_scope(p);
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    if (!p->reached) return fail(ARMOUR_E_STATE, "no reach set");
    const NlpDev& d = p->d;
    if (!d.pcache || p->set.eval_f32 || d.O == 0) return fail(ARMOUR_E_STATE, "plane cache off (ARMOUR_PLANE_CACHE=0, float study or no obstacles)");
    ensure_plane_cache(p);
    const size_t blocks = (size_t)p->W * p->T, NP = (size_t)p->NJ * d.O;
    std::vector<unsigned> off(blocks * NP);
    std::vector<unsigned char> ok(blocks);
    HIPCK(hipMemcpyAsync(off.data(), d.pcoff, sizeof(unsigned) * off.size(), hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipMemcpyAsync(ok.data(), d.pcok, blocks, hipMemcpyDeviceToHost, p->stream));
    HIPCK(hipStreamSynchronize(p->stream));
    // only the pairs that exist: a mixed batch's world fills the first NJ * O_w entries of each block
    long long kept = 0, nok = 0, mx = 0, pairs = 0;
    for (size_t b = 0; b < blocks; b++) {
        const size_t np = (size_t)p->NJ * p->Ow[b / p->T];
        pairs += (long long)np;
        for (size_t q = 0; q < np; q++) {
            const unsigned v = off[b * NP + q];
            kept += v & 255;
            mx = std::max<long long>(mx, v & 255);
        }
    }
    for (unsigned char v : ok) nok += v;
    unsigned miss = 0;
    HIPCK(hipMemcpy(&miss, cnt_at(p, CNT_PC_MISS), sizeof(unsigned), hipMemcpyDeviceToHost));
    const long long st[ARMOUR_PC_COUNT] = {kept, pairs, nok, (long long)blocks, mx, d.pc_pool, miss};
    for (int k = 0; k < n && k < ARMOUR_PC_COUNT; k++) out[k] = st[k];
    return ARMOUR_PC_COUNT;
}

int armour_get_reach_occupancy(armour_planner* p, long long* used, long long* caps, int n) {
    DeviceScope device_scope(p);
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    if (!p->reached) return fail(ARMOUR_E_STATE, "no reach set");
    if (!p->lane_engine || !p->d_occ)
        return fail(ARMOUR_E_STATE, "occupancy is recorded by the bundle engine only (this batch ran on the per-job engine)");
    const unsigned long long* o = p->h_occ;  // the first launch's maxima (a retry's 4x buffers excluded)
    const long long u[ARMOUR_OCC_COUNT] = {(long long)o[0], (long long)o[1], (long long)o[2], (long long)o[3],
                                           (long long)o[4], p->last_retried, p->last_failed};
    const long long c[ARMOUR_OCC_COUNT] = {p->la.hcap, p->la.ccap, std::min<long long>(p->la.gcap, (1 << 16) - 1),
                                           CAP_LM, CAP_UM, p->W, p->W};
    for (int k = 0; k < n && k < ARMOUR_OCC_COUNT; k++) {
        if (used) used[k] = u[k];
        if (caps) caps[k] = c[k];
    }
    return ARMOUR_OCC_COUNT;
}

int armour_get_path_counts(armour_planner* p, long long* counts, int n) {
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    for (int k = 0; counts && k < n && k < PATH_N; k++) counts[k] = p->paths[k];
    return PATH_N;
}

const char* armour_path_name(int i) { return i >= 0 && i < PATH_N ? PATH_NAMES[i] : nullptr; }

int armour_get_solver_options(const armour_planner* p, armour_solver_options* o) {
    if (!p || !o) return fail(ARMOUR_E_ARG, "null argument");
    *o = armour_solver_options{p->d.opt.mu_strategy, p->od.qf_grid, p->od.lbfgs_history};
    return 0;
}

int armour_set_solver_options(armour_planner* p, const armour_solver_options* o) {
    if (!p || !o) return fail(ARMOUR_E_ARG, "null argument");
    if (int rc = solver_options_check(p, o)) return rc;
    if (p->ep.on) return fail(ARMOUR_E_STATE, "solver options cannot change while an episode is active");
    solver_options_apply(p, *o);
    return 0;
}

int armour_get_reach_program(const armour_planner* p, int* codes, int capacity) {
    DeviceScope device_scope(p);
    if (!p) return fail(ARMOUR_E_ARG, "null planner");
    if (codes && capacity >= p->nops) {
        std::vector<Op> ops(p->nops);
        HIPCK(hipMemcpy(ops.data(), p->d_prog, sizeof(Op) * p->nops, hipMemcpyDeviceToHost));
        for (int k = 0; k < p->nops; k++) codes[k] = ops[k].code;
    }
    return p->nops;
}

}  // extern "C"
