// TEST HARNESS — the row passes' block reduction (armour-dev_amd/csrc/block_reduce.h) beside the
// butterfly form it replaced, at every call site's width and kinds, 256 threads per block. Never
// part of the product library.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "block_reduce.h"

// the block reduction as it stood before the reduce-scatter, verbatim
namespace parent {
using armour::xor_f64;
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + xor_f64(v, m);
    return v;
}
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
template <int N>
__device__ inline void block_reduce_n(double (&v)[N], const int (&kinds)[N], double* lds, double* out) {
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    // groups of 8 interleave; a scheduling barrier between groups bounds the live registers
#pragma unroll
    for (int g = 0; g < N; g += 8) {
#pragma unroll
        for (int i = g; i < (g + 8 < N ? g + 8 : N); i++)
            v[i] = kinds[i] == 0 ? wave_sum(v[i]) : kinds[i] == 1 ? wave_max(v[i]) : wave_min(v[i]);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int i = g; i < (g + 8 < N ? g + 8 : N); i++) lds[wave * N + i] = v[i];
        }
        __builtin_amdgcn_sched_barrier(0);
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
}  // namespace parent

constexpr int THREADS = 256;

// the call sites' kinds (nlp_kernels.hip): 55 pass A, 19 pass B, 37 resto_rows_G; 1, 2, 7 all sums
template <int N>
__device__ inline int site_kind(int k) {
    if (N == 55) return (k >= 7 && k <= 9) ? 1 : k == 54 ? 2 : 0;
    if (N == 19) return k < 2 ? 2 : 0;
    if (N == 37) return k == 36 ? 1 : 0;
    return 0;
}

// in [blocks][THREADS][N]; out_new, out_old [blocks][N]
template <int N>
__global__ __launch_bounds__(THREADS) void reduce_kernel(const double* in, double* out_new, double* out_old) {
    __shared__ double lds_new[(THREADS / 64) * N], lds_old[(THREADS / 64) * N];
    double a[N], b[N];
    int kinds[N];
    const double* src = in + ((long)blockIdx.x * THREADS + threadIdx.x) * N;
#pragma unroll
    for (int k = 0; k < N; k++) {
        a[k] = b[k] = src[k];
        kinds[k] = site_kind<N>(k);
    }
    armour::block_reduce_n(a, kinds, lds_new, out_new + (long)blockIdx.x * N);
    parent::block_reduce_n(b, kinds, lds_old, out_old + (long)blockIdx.x * N);
}

template <int N>
static void launch(int blocks, const double* in, double* out_new, double* out_old) {
    hipLaunchKernelGGL(reduce_kernel<N>, dim3(blocks), dim3(THREADS), 0, 0, in, out_new, out_old);
}

extern "C" int reduce_site_kind(int N, int k) {
    return N == 55 ? ((k >= 7 && k <= 9) ? 1 : k == 54 ? 2 : 0) : N == 19 ? (k < 2 ? 2 : 0) : N == 37 ? (k == 36 ? 1 : 0) : 0;
}

extern "C" int reduce_run(int N, int blocks, const double* host_in, double* host_new, double* host_old) {
    const size_t nin = sizeof(double) * blocks * THREADS * N, nout = sizeof(double) * blocks * N;
    double *din = nullptr, *dnew = nullptr, *dold = nullptr;
    if (hipMalloc(&din, nin) != hipSuccess || hipMalloc(&dnew, nout) != hipSuccess || hipMalloc(&dold, nout) != hipSuccess) return -1;
    hipMemcpy(din, host_in, nin, hipMemcpyHostToDevice);
    hipMemset(dnew, 0xFF, nout);
    hipMemset(dold, 0xFF, nout);
    switch (N) {
        case 1: launch<1>(blocks, din, dnew, dold); break;
        case 2: launch<2>(blocks, din, dnew, dold); break;
        case 7: launch<7>(blocks, din, dnew, dold); break;
        case 19: launch<19>(blocks, din, dnew, dold); break;
        case 37: launch<37>(blocks, din, dnew, dold); break;
        case 55: launch<55>(blocks, din, dnew, dold); break;
        default: return -3;
    }
    const hipError_t e = hipDeviceSynchronize();
    hipMemcpy(host_new, dnew, nout, hipMemcpyDeviceToHost);
    hipMemcpy(host_old, dold, nout, hipMemcpyDeviceToHost);
    hipFree(din);
    hipFree(dnew);
    hipFree(dold);
    return e == hipSuccess ? 0 : -2;
}
