// armour-mi355x — the row passes' block reduction (nlp_kernels.hip; tests/reduce_unit checks it
// against the butterfly form it replaced, bit for bit).
#pragma once
#include "wave.h"

namespace armour {

// wave_sum (wave.h): DPP / permlane butterfly
__device__ inline double wave_max(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, xor_f64(v, m));
    return v;
}
__device__ inline double wave_min(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmin(v, xor_f64(v, m));
    return v;
}
// N values at once, the arithmetic of N block_reduce calls (wave reduction, then the waves in
// order) with one barrier. kinds[i]: 0 sum, 1 max, 2 min (constants once unrolled). out[i] written
// by thread i; lds holds (blockDim / 64) * N doubles.
// The sum slots go through one reduce-scatter (wave.h scatter_sum: wave_sum's tree and bits, each
// node computed once; the lane that ends with index i stores it); the few max / min slots keep the
// butterfly. get(i) is slot i's value, read once: a slot that lives in LDS is fetched only when
// its pair is consumed.
template <int N, class Get>
__device__ inline __attribute__((always_inline)) void block_reduce_get(const Get& get, const int (&kinds)[N], double* lds,
                                                                       double* out) {
    constexpr int P = scatter_width(N);
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = lane_id();
    uint64_t sums = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (kinds[i] == 0) {
            sums |= 1ull << i;
        } else {
            const double t = kinds[i] == 1 ? wave_max(get(i)) : wave_min(get(i));
            if (lane == 0) lds[wave * N + i] = t;
        }
    }
    if (sums) {
        const double s = scatter_sum<N>(get, sums);
        const int idx = scatter_index(P, lane & (P - 1));
        if (lane < P && ((sums >> idx) & 1)) lds[wave * N + idx] = s;
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i < N) {
        int kind = 0;
#pragma unroll
        for (int q = 0; q < N; q++) if (q == i) kind = kinds[q];
        double s = lds[i];
        for (int k = 1; k < nw; k++) {
            const double t = lds[k * N + i];
            s = kind == 0 ? s + t : kind == 1 ? fmax(s, t) : fmin(s, t);
        }
        out[i] = s;
    }
}
template <int N>
__device__ inline __attribute__((always_inline)) void block_reduce_n(double (&v)[N], const int (&kinds)[N], double* lds,
                                                                     double* out) {
    block_reduce_get<N>([&](int i) __attribute__((always_inline)) { return v[i]; }, kinds, lds, out);
}

}  // namespace armour
