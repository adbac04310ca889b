// armour-mi355x — the joint-space roadmap high-level planner (armour_roadmap_*, armour_episode_roadmap;
// include/armour_hip.h has the contract): caller-supplied nodes per world plus the world's goal, a
// collision check of every vertex and of the samples of every candidate edge, the adjacency bits, the
// cost-to-go field and the waypoint taken from it. The shape of
// simulator/planners/high_level_planners/robot_arm_sampling_based_HLP.m (robot_arm_PRM_HLP.m is the
// neighbour-radius variant), with the edges checked as well as the nodes.
//
// The point check is lane-per-configuration: the world's obstacles are staged in LDS once per block (every
// lane reads the same address: a broadcast), each lane runs its own forward-kinematics chain
// (motion_link_box) and, after each link's box, loops over the obstacles (motion_separation) with a
// running minimum. No cross-lane reduction and no barrier inside the loop. The value is bit for bit the
// one motion_check_kernel finds for the same configuration: the same functions on the same operands,
// and a minimum does not depend on the order it is taken in.
//
// roadmap_vertex_kernel    grid (vertex chunk, world): clr and free of every vertex
// roadmap_edges_kernel     grid (row chunk, world), lane = row i: the candidate edges (i, j), j > i; <false>
//                          counts them and their interior samples per row, <true> writes the edge list at
//                          the row's offsets (the host scans the counts), so the list is in (i, j) order
// roadmap_sample_kernel    grid (sample chunk, world), lane = interior sample of an edge, found by a search
//                          in the edges' sample offsets: one plain byte store, clr > margin
// roadmap_fold_kernel      lane = edge: every sample free -> the two adjacency bits (atomicOr)
// roadmap_togo_kernel      one workgroup per world, thread = vertex, togo in LDS: barrier-separated Jacobi
//                          rounds until none changes, then next
// roadmap_waypoint_kernel  one workgroup per world: lanes over the entry segments q -> v_i, a first-minimum
//                          reduction (motion_before), the walk on thread 0
#pragma once
#include "motion_kernels.hip"

namespace armour {

constexpr int ROADMAP_THREADS = 256;
constexpr int ROADMAP_WAVES = ROADMAP_THREADS / 64;
constexpr int ROADMAP_MAX_V = ARMOUR_ROADMAP_MAX_NODES + 1;  // the goal is the last vertex
constexpr int ROADMAP_WORDS = ROADMAP_MAX_V / 32;             // adjacency words per row
static_assert(ROADMAP_MAX_V == 1024, "one thread per vertex in roadmap_togo_kernel");

enum { ROADMAP_STAT_FREE, ROADMAP_STAT_EDGES, ROADMAP_STAT_REACHABLE, ROADMAP_STAT_ROUNDS, ROADMAP_STATS };

struct RoadmapDev {
    MotionArgs m;               // the resident batch: rp, W, O, Ow, obs (motion_obstacles)
    int N, V;                   // caller nodes per world; vertices V = N + 1
    double radius, step, margin;
    const double* verts;        // [W][V][NF]
    double* clr;                // [W][V]
    int* free;                  // [W][V]
    unsigned* adj;              // [W][V][ROADMAP_WORDS]
    double* togo;               // [W][V]
    int* next;                  // [W][V]
    int* row_edges;             // [W * V] candidate edges (i, j > i) of row i
    int* row_samples;           // [W * V] their interior samples
    const int* row_eoff;        // [W * V + 1] exclusive scans of the two (host)
    const int* row_soff;
    int* e_row;                 // [E] w * V + i
    int* e_j;                   // [E]
    int* e_n;                   // [E] pieces
    int* e_soff;                // [E] first interior sample
    int E;
    unsigned char* ok;          // [samples] clr > margin
    unsigned long long* stats;  // [ROADMAP_STATS]
};

// Delta(a -> b) and d(a, b): the difference angle-wrapped on continuous joints (state_lb <= -1000, the
// rule of waypoint()), the squares summed in joint order
__device__ inline double roadmap_delta(const RobotParams& rp, const double* a, const double* b, double* dl) {
    double s = 0.0;
    for (int j = 0; j < NF; j++) {
        double d = b[j] - a[j];
        if (rp.state_lb[j] <= -1000.0) d = wrap_diff(d);
        dl[j] = d;
        s += d * d;
    }
    return sqrt(s);
}
// the weight of the edge between vertices i and j: d from the lower index to the higher
__device__ inline double roadmap_weight(const RobotParams& rp, const double* vi, int i, const double* vj, int j) {
    double dl[NF];
    return i < j ? roadmap_delta(rp, vi, vj, dl) : roadmap_delta(rp, vj, vi, dl);
}
__device__ inline int roadmap_pieces(double d, double step) { return (int)ceil(d / step); }

// the world's obstacles into LDS (every thread of the block calls it; ends in a barrier)
__device__ inline int roadmap_stage(const MotionArgs& m, int w, double* s_obs) {
    const int O = motion_obstacles(m, w);
    const double* ob = m.obs + (long)w * m.O * 12;
    for (int i = threadIdx.x; i < O * 12; i += blockDim.x) s_obs[i] = ob[i];
    __syncthreads();
    return O;
}

// clr(q) on one lane; cs: 2 * NF doubles of the lane's own (LDS: the chain indexes it by joint)
__device__ __forceinline__ double roadmap_clearance(const RobotParams& rp, const double* s_obs, int O, const double* q, double* cs) {
    if (O == 0) return INFINITY;
    for (int j = 0; j < NF; j++) {
        cs[2 * j] = cos(q[j]);
        cs[2 * j + 1] = sin(q[j]);
    }
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0}, best = INFINITY;
    const int NJ = rp.num_joints;
    for (int i = 0; i < NJ; i++) {
        double L[12];
        motion_link_box(rp, i, cs, R, p, L);
        for (int o = 0; o < O; o++) {
            const double v = motion_separation(s_obs + 12 * o, L);
            if (v < best) best = v;
        }
    }
    return best;
}
// every interior sample a + (s / n) dl, s = 1 .. n - 1, has clr > margin
__device__ inline bool roadmap_segment_free(const RobotParams& rp, const double* s_obs, int O, const double* a, const double* dl,
                                            int n, double margin, double* cs) {
    for (int s = 1; s < n; s++) {
        const double f = (double)s / (double)n;
        double x[NF];
        for (int j = 0; j < NF; j++) x[j] = a[j] + f * dl[j];
        if (!(roadmap_clearance(rp, s_obs, O, x, cs) > margin)) return false;
    }
    return true;
}

__global__ __launch_bounds__(ROADMAP_THREADS) void roadmap_vertex_kernel(RoadmapDev r) {
    __shared__ double s_obs[MAX_OBS * 12];
    __shared__ double s_cs[ROADMAP_THREADS][2 * NF];
    const int w = blockIdx.y, v = blockIdx.x * ROADMAP_THREADS + threadIdx.x;
    const int O = roadmap_stage(r.m, w, s_obs);
    int is_free = 0;
    if (v < r.V) {
        double q[NF];
        for (int j = 0; j < NF; j++) q[j] = r.verts[((long)w * r.V + v) * NF + j];
        const double c = roadmap_clearance(*r.m.rp, s_obs, O, q, s_cs[threadIdx.x]);
        is_free = c > r.margin ? 1 : 0;
        r.clr[(long)w * r.V + v] = c;
        r.free[(long)w * r.V + v] = is_free;
    }
    const int n = __syncthreads_count(is_free);
    if (threadIdx.x == 0 && n) atomicAdd(&r.stats[ROADMAP_STAT_FREE], (unsigned long long)n);
}

template <bool FILL>
__global__ __launch_bounds__(ROADMAP_THREADS) void roadmap_edges_kernel(RoadmapDev r) {
    const int w = blockIdx.y, i = blockIdx.x * ROADMAP_THREADS + threadIdx.x;
    if (i >= r.V) return;
    const RobotParams& rp = *r.m.rp;
    const long row = (long)w * r.V + i;
    const double* vw = r.verts + (long)w * r.V * NF;
    const int* fw = r.free + (long)w * r.V;
    int cnt = 0, smp = 0;
    if (fw[i]) {
        double a[NF], dl[NF];
        for (int k = 0; k < NF; k++) a[k] = vw[(long)i * NF + k];
        for (int j = i + 1; j < r.V; j++) {
            if (!fw[j]) continue;
            const double d = roadmap_delta(rp, a, vw + (long)j * NF, dl);
            if (!(d >= ARMOUR_ROADMAP_MIN_EDGE && d <= r.radius)) continue;
            const int n = roadmap_pieces(d, r.step);
            if (FILL) {
                const long e = (long)r.row_eoff[row] + cnt;
                r.e_row[e] = (int)row;
                r.e_j[e] = j;
                r.e_n[e] = n;
                r.e_soff[e] = r.row_soff[row] + smp;
            }
            cnt++;
            smp += n - 1;
        }
    }
    if (!FILL) {
        r.row_edges[row] = cnt;
        r.row_samples[row] = smp;
    }
}

__global__ __launch_bounds__(ROADMAP_THREADS) void roadmap_sample_kernel(RoadmapDev r) {
    __shared__ double s_obs[MAX_OBS * 12];
    __shared__ double s_cs[ROADMAP_THREADS][2 * NF];
    const int w = blockIdx.y;
    const long first = r.row_soff[(long)w * r.V], last = r.row_soff[(long)(w + 1) * r.V];
    if (first + (long)blockIdx.x * ROADMAP_THREADS >= last) return;  // (block-uniform)
    const int O = roadmap_stage(r.m, w, s_obs);
    const long t = first + (long)blockIdx.x * ROADMAP_THREADS + threadIdx.x;
    if (t >= last) return;
    // the last edge of this world whose first sample is at or before t (edges without samples share
    // their offset with the next edge and lie before it)
    int lo = r.row_eoff[(long)w * r.V], hi = r.row_eoff[(long)(w + 1) * r.V] - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (r.e_soff[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    const RobotParams& rp = *r.m.rp;
    const int n = r.e_n[lo], s = (int)(t - r.e_soff[lo]) + 1;
    const double* a = r.verts + (long)r.e_row[lo] * NF;
    const double* b = r.verts + ((long)w * r.V + r.e_j[lo]) * NF;
    double av[NF], dl[NF], x[NF];
    for (int k = 0; k < NF; k++) av[k] = a[k];
    roadmap_delta(rp, av, b, dl);
    const double f = (double)s / (double)n;
    for (int k = 0; k < NF; k++) x[k] = av[k] + f * dl[k];
    r.ok[t] = roadmap_clearance(rp, s_obs, O, x, s_cs[threadIdx.x]) > r.margin ? 1 : 0;
}

__global__ __launch_bounds__(ROADMAP_THREADS) void roadmap_fold_kernel(RoadmapDev r) {
    const long e = (long)blockIdx.x * ROADMAP_THREADS + threadIdx.x;
    int exists = 0;
    if (e < r.E) {
        const int n = r.e_n[e];
        const unsigned char* ok = r.ok + r.e_soff[e];
        exists = 1;
        for (int s = 0; s < n - 1; s++) exists &= ok[s];
        if (exists) {
            const long row = r.e_row[e];
            const int j = r.e_j[e], i = (int)(row % r.V);
            atomicOr(&r.adj[row * ROADMAP_WORDS + (j >> 5)], 1u << (j & 31));
            atomicOr(&r.adj[(row - i + j) * ROADMAP_WORDS + (i >> 5)], 1u << (i & 31));
        }
    }
    const int n = __syncthreads_count(exists);
    if (threadIdx.x == 0 && n) atomicAdd(&r.stats[ROADMAP_STAT_EDGES], (unsigned long long)n);
}

// togo and next of one world. Round k: every vertex takes min(own, min_j fl(d(i, j) + togo[j])) over its
// row's bits from the values of round k - 1 (two barriers a round). Floating-point addition is monotone,
// so the fixed point reached from +infinity is the one any schedule (a Dijkstra with the same additions
// too) reaches. The goal is settled at 0 when it is free; when it is not, every togo stays +infinity.
__global__ __launch_bounds__(ROADMAP_MAX_V) void roadmap_togo_kernel(RoadmapDev r) {
    __shared__ double s_togo[ROADMAP_MAX_V];
    const int w = blockIdx.x, i = threadIdx.x, N = r.N;
    const bool in = i < r.V;
    const RobotParams& rp = *r.m.rp;
    const double* vw = r.verts + (long)w * r.V * NF;
    const unsigned* row = r.adj + ((long)w * r.V + (in ? i : 0)) * ROADMAP_WORDS;
    const bool goal_free = r.free[(long)w * r.V + N] != 0;
    double a[NF];
    for (int k = 0; k < NF; k++) a[k] = in ? vw[(long)i * NF + k] : 0.0;
    s_togo[i] = (i == N && goal_free) ? 0.0 : INFINITY;
    __syncthreads();
    int rounds = 0;
    for (int k = 0; k <= N; k++) {
        const double own = s_togo[i];
        double best = own;
        if (in && i != N)
            for (int wd = 0; wd < ROADMAP_WORDS; wd++)
                for (unsigned bits = row[wd]; bits; bits &= bits - 1) {
                    const int j = 32 * wd + __ffs(bits) - 1;
                    const double tj = s_togo[j];
                    if (tj < INFINITY) {
                        const double c = roadmap_weight(rp, a, i, vw + (long)j * NF, j) + tj;
                        if (c < best) best = c;
                    }
                }
        if (!__syncthreads_or(best < own)) break;
        if (best < own) s_togo[i] = best;
        rounds++;
        __syncthreads();
    }
    const double mine = s_togo[i];
    int nx = -1;
    if (in && mine < INFINITY) {
        if (i == N) nx = N;
        else
            for (int wd = 0; wd < ROADMAP_WORDS && nx < 0; wd++)
                for (unsigned bits = row[wd]; bits && nx < 0; bits &= bits - 1) {
                    const int j = 32 * wd + __ffs(bits) - 1;
                    if (roadmap_weight(rp, a, i, vw + (long)j * NF, j) + s_togo[j] == mine) nx = j;
                }
    }
    if (in) {
        r.togo[(long)w * r.V + i] = mine;
        r.next[(long)w * r.V + i] = nx;
    }
    const int reach = __syncthreads_count(in && mine < INFINITY);
    if (i == 0) {
        if (reach) atomicAdd(&r.stats[ROADMAP_STAT_REACHABLE], (unsigned long long)reach);
        atomicMax(&r.stats[ROADMAP_STAT_ROUNDS], (unsigned long long)rounds);
    }
}

// Where the query points come from and where the waypoints go. st null: q / q_des [W][NF] of
// armour_roadmap_waypoint. st set: the episode's states; `kind` null (armour_episode_roadmap): the running
// worlds, at their q, the others get entry -1 and +infinity; `kind` set (after episode_advance_kernel): the
// worlds that moved this step (kind >= 1, not status 4), whose straight-line q_des is replaced.
struct RoadmapQuery {
    double lookahead;
    const double* q;
    double* q_des;
    armour_episode_state* st;
    const int* kind;
    int* entry;         // [W]
    double* path_left;  // [W]
};

__global__ __launch_bounds__(ROADMAP_THREADS) void roadmap_waypoint_kernel(RoadmapDev r, RoadmapQuery y) {
    __shared__ double s_obs[MAX_OBS * 12];
    __shared__ double s_cs[ROADMAP_THREADS][2 * NF];
    __shared__ double s_wv[ROADMAP_WAVES];
    __shared__ int s_wi[ROADMAP_WAVES];
    const int w = blockIdx.x, tid = threadIdx.x, N = r.N;
    // (block-uniform)
    if (y.st) {
        const int status = y.st[w].status;
        if (y.kind ? (y.kind[w] < 1 || status == 4) : status != 0) {
            if (!y.kind && tid == 0) {
                y.entry[w] = -1;
                y.path_left[w] = INFINITY;
            }
            return;
        }
    }
    const RobotParams& rp = *r.m.rp;
    const double* vw = r.verts + (long)w * r.V * NF;
    const double* togo = r.togo + (long)w * r.V;
    const int* fw = r.free + (long)w * r.V;
    const double* qin = y.st ? y.st[w].q : y.q + (long)w * NF;
    double* qout = y.st ? y.st[w].q_des : y.q_des + (long)w * NF;
    const int O = roadmap_stage(r.m, w, s_obs);
    double q[NF], dl[NF];
    for (int k = 0; k < NF; k++) q[k] = qin[k];
    double best = INFINITY;
    int bi = INT_MAX;
    for (int i = tid; i < r.V; i += ROADMAP_THREADS) {
        if (!fw[i] || !(togo[i] < INFINITY)) continue;
        const double d = roadmap_delta(rp, q, vw + (long)i * NF, dl);
        if (!(d <= r.radius)) continue;
        if (!roadmap_segment_free(rp, s_obs, O, q, dl, roadmap_pieces(d, r.step), r.margin, s_cs[tid])) continue;
        const double c = d + togo[i];
        if (motion_before(c, i, best, bi)) {
            best = c;
            bi = i;
        }
    }
    motion_first_min(best, bi);
    if ((tid & 63) == 0) {
        s_wv[tid >> 6] = best;
        s_wi[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int k = 1; k < ROADMAP_WAVES; k++)
        if (motion_before(s_wv[k], s_wi[k], best, bi)) {
            best = s_wv[k];
            bi = s_wi[k];
        }
    double out[NF];
    if (bi == INT_MAX) {
        waypoint(rp, q, vw + (long)N * NF, y.lookahead, out);
        y.entry[w] = -1;
        y.path_left[w] = INFINITY;
    } else {
        // q -> entry -> next -> ... -> goal, with lookahead left to spend
        const int* next = r.next + (long)w * r.V;
        double a[NF], rem = y.lookahead;
        for (int k = 0; k < NF; k++) out[k] = a[k] = q[k];
        int cur = bi;
        for (int leg = 0; leg <= N + 1 && cur >= 0; leg++) {
            const double* b = vw + (long)cur * NF;
            const double d = roadmap_delta(rp, a, b, dl);
            if (rem > d) {
                for (int k = 0; k < NF; k++) out[k] += dl[k];
                rem -= d;
            } else {
                const double f = rem / d;
                for (int k = 0; k < NF; k++) out[k] += f * dl[k];
                break;
            }
            if (cur == N) break;
            for (int k = 0; k < NF; k++) a[k] = b[k];
            cur = next[cur];
        }
        y.entry[w] = bi;
        y.path_left[w] = best;
    }
    for (int k = 0; k < NF; k++) qout[k] = out[k];
}

}  // namespace armour
