// TEST HARNESS — unit entries for the JRS scalars (reach.h jrs_joint) and the outward-rounded interval
// operations (interval.h), one thread per case. Built twice: for gfx950 (libjrs_test.so: the ocml
// directed-rounding side) and host-only with -DJRS_TEST_HOST (libjrs_test_host.so: the fesetround
// side the emulation runs). Same entries in both. Never part of the product library.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "reach.h"
#include "robots.h"

using namespace armour;

constexpr int JRS_DOUBLES = 13;

AD void jrs_case(const RobotParams& rp, int T, int s, int joint, double q0, double qd0, double qdd0, double* o) {
    const JrsJoint J = jrs_joint(rp, T, s, joint, q0, qd0, qdd0);
    o[0] = J.cos_c; o[1] = J.cos_k; o[2] = J.cos_e;
    o[3] = J.sin_c; o[4] = J.sin_k; o[5] = J.sin_e;
    o[6] = J.qd_c; o[7] = J.qd_k; o[8] = J.qd_e; o[9] = J.qda_e;
    o[10] = J.qdd_c; o[11] = J.qdd_k; o[12] = J.qdd_e;
}

// op: 0 add_dn, 1 add_up, 2 sub_dn, 3 sub_up, 4 mul_dn, 5 mul_up, 6 div_dn, 7 sqrt_dn(a), 8 sqrt_up(a)
AD double ival_case(int op, double a, double b) {
    switch (op) {
        case 0: return add_dn(a, b);
        case 1: return add_up(a, b);
        case 2: return sub_dn(a, b);
        case 3: return sub_up(a, b);
        case 4: return mul_dn(a, b);
        case 5: return mul_up(a, b);
        case 6: return div_dn(a, b);
        case 7: return sqrt_dn(a);
        default: return sqrt_up(a);
    }
}

// out[4]: icos lo, hi, isin lo, hi
AD void icos_case(double lo, double hi, double* o) {
    const Ival c = icos(Ival{lo, hi}), s = isin(Ival{lo, hi});
    o[0] = c.lo; o[1] = c.hi; o[2] = s.lo; o[3] = s.hi;
}

#if defined(JRS_TEST_HOST)

extern "C" int jrs_selftest(int T, int n, const double* q0, const double* qd0, const double* qdd0, const int* joint,
                            const int* s, double* out13) {
    RobotParams rp;
    kinova_gen3(rp);
    for (int k = 0; k < n; k++) {
        if (joint[k] < 0 || joint[k] >= NF || s[k] < 0 || s[k] >= T) return -1;
        jrs_case(rp, T, s[k], joint[k], q0[k], qd0[k], qdd0[k], out13 + (long)k * JRS_DOUBLES);
    }
    return 0;
}
extern "C" int ival_selftest(int n, int op, const double* a, const double* b, double* out) {
    if (op < 0 || op > 8) return -1;
    for (int k = 0; k < n; k++) out[k] = ival_case(op, a[k], b[k]);
    return 0;
}
extern "C" int icos_selftest(int n, const double* lo, const double* hi, double* out) {
    for (int k = 0; k < n; k++) icos_case(lo[k], hi[k], out + 4L * k);
    return 0;
}

#else

__global__ void jrs_test_kernel(const RobotParams* rp, int T, int n, const double* q0, const double* qd0,
                                const double* qdd0, const int* joint, const int* s, double* out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) jrs_case(*rp, T, s[k], joint[k], q0[k], qd0[k], qdd0[k], out + (long)k * JRS_DOUBLES);
}
__global__ void ival_test_kernel(int n, int op, const double* a, const double* b, double* out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = ival_case(op, a[k], b[k]);
}
__global__ void icos_test_kernel(int n, const double* lo, const double* hi, double* out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) icos_case(lo[k], hi[k], out + 4L * k);
}

namespace {
// device buffers of one call, freed at its end
struct Bufs {
    void* p[8];
    int n = 0;
    bool ok = true;
    template <class V>
    V* up(const V* host, size_t count) {
        void* d = nullptr;
        if (!ok || hipMalloc(&d, sizeof(V) * (count ? count : 1)) != hipSuccess) { ok = false; return nullptr; }
        p[n++] = d;
        if (host && count && hipMemcpy(d, host, sizeof(V) * count, hipMemcpyHostToDevice) != hipSuccess) ok = false;
        return (V*)d;
    }
    ~Bufs() { for (int k = 0; k < n; k++) (void)hipFree(p[k]); }
};
int finish(Bufs& B, double* host_out, const double* dev_out, size_t count) {
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    if (hipMemcpy(host_out, dev_out, sizeof(double) * count, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    return B.ok ? 0 : -2;
}
constexpr int BLOCK = 64;
}  // namespace

extern "C" int jrs_selftest(int T, int n, const double* q0, const double* qd0, const double* qdd0, const int* joint,
                            const int* s, double* out13) {
    if (n <= 0) return -1;
    for (int k = 0; k < n; k++)
        if (joint[k] < 0 || joint[k] >= NF || s[k] < 0 || s[k] >= T) return -1;
    RobotParams rp;
    kinova_gen3(rp);
    Bufs B;
    RobotParams* drp = B.up(&rp, 1);
    const double *a = B.up(q0, n), *b = B.up(qd0, n), *c = B.up(qdd0, n);
    const int *dj = B.up(joint, n), *ds = B.up(s, n);
    double* o = B.up((const double*)nullptr, (size_t)n * JRS_DOUBLES);
    if (!B.ok) return -2;
    hipLaunchKernelGGL(jrs_test_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, 0, drp, T, n, a, b, c, dj, ds, o);
    return finish(B, out13, o, (size_t)n * JRS_DOUBLES);
}
extern "C" int ival_selftest(int n, int op, const double* a, const double* b, double* out) {
    if (n <= 0 || op < 0 || op > 8) return -1;
    Bufs B;
    const double *da = B.up(a, n), *db = B.up(b, n);
    double* o = B.up((const double*)nullptr, n);
    if (!B.ok) return -2;
    hipLaunchKernelGGL(ival_test_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, 0, n, op, da, db, o);
    return finish(B, out, o, n);
}
extern "C" int icos_selftest(int n, const double* lo, const double* hi, double* out) {
    if (n <= 0) return -1;
    Bufs B;
    const double *dl = B.up(lo, n), *dh = B.up(hi, n);
    double* o = B.up((const double*)nullptr, 4 * (size_t)n);
    if (!B.ok) return -2;
    hipLaunchKernelGGL(icos_test_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, 0, n, dl, dh, o);
    return finish(B, out, o, 4 * (size_t)n);
}

#endif
