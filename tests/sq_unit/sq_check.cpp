// TEST HARNESS — the squared keep / prune threshold of the reach engines (pz_engine.h SqThr, Decide)
// built for the host, with the host's sqrt, as tests/emu builds the engine headers. Used only by
// tests/test_sq_threshold.py; never part of the product library.
#include "pz_engine.h"

using namespace armour;

extern "C" void sq_host_threshold(double thr, double* s, int* valid) {
    const SqThr q = sq_threshold(thr);
    *s = q.s;
    *valid = q.valid;
}

// per value S: bit 0 = S > s, bit 1 = !(S <= s) (the squared form); bit 2 = sqrt(S) > thr,
// bit 3 = !(sqrt(S) <= thr) (the sqrt form); bit 4 = the raw constructors' run-time form with
// valid = 1, bit 5 = the same with valid = 0
extern "C" void sq_host_eval(double thr, double s, const double* S, long long n, unsigned char* out) {
    const Decide<true> a{thr, s};
    const Decide<false> b{thr, s};
    for (long long i = 0; i < n; i++)
        out[i] = (unsigned char)((a.gt(S[i]) ? 1 : 0) | (!a.le(S[i]) ? 2 : 0) | (b.gt(S[i]) ? 4 : 0) | (!b.le(S[i]) ? 8 : 0) |
                                 (sq_not_le(S[i], thr, s, 1) ? 16 : 0) | (sq_not_le(S[i], thr, s, 0) ? 32 : 0));
}

// the sum of squares and the norm of an n-block (n = 1, 3, 9): the norm is the square root of
// exactly that sum
extern "C" void sq_host_frob(const double* x, int n, double* sq, double* norm) {
    *sq = frob_sq(x, n);
    *norm = frob_norm(x, n);
}
