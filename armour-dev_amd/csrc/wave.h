// armour-mi355x — wave64 data movement on gfx950 without the LDS crossbar.
//
// ds_bpermute (what __shfl / __shfl_xor compile to) goes through the LDS pipeline, about a hundred
// cycles per dependent step. The PZ engine's wave-level sorts, scans and reductions are long
// dependent chains of such steps, so they use DPP and the CDNA4 permlane swaps instead:
//   xor 1, 2        DPP quad_perm
//   xor 4, 8        DPP row_shl / row_shr by 4 or 8, selected by the lane bit
//   xor 16          v_permlane16_swap (rows 0<->1, 2<->3)
//   xor 32          v_permlane32_swap (halves)
//   lane +-1        DPP row_shl:1 / row_shr:1, row-boundary lanes patched from v_readlane
//                   (the DPP wave_shl / wave_shr controls assemble for gfx950 but do not shift)
// 64-bit values move as two 32-bit halves. tests/test_gpu_wave.py checks every primitive against
// __shfl on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace armour {

#define WAVE_FN __device__ inline __attribute__((always_inline))

WAVE_FN int lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0)); }

// partner value at lane ^ m, m in {1, 2, 4, 8, 16, 32} (m uniform; a constant after unrolling)
WAVE_FN uint32_t xor_u32(uint32_t v, int m) {
    const int l = lane_id();
    switch (m) {
        case 1: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
        case 2: return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
        case 4: {
            const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xF, 0xF, false);  // row_shl:4
            const uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);  // row_shr:4
            return (l & 4) ? dn : up;
        }
        case 8: {
            const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x108, 0xF, 0xF, false);  // row_shl:8
            const uint32_t dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);  // row_shr:8
            return (l & 8) ? dn : up;
        }
        case 16: {
            const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
            return (l & 16) ? p[0] : p[1];
        }
        default: {
            const auto p = __builtin_amdgcn_permlane32_swap(v, v, false, false);
            return (l & 32) ? p[0] : p[1];
        }
    }
}
WAVE_FN uint64_t xor_u64(uint64_t v, int m) {
    const uint32_t lo = xor_u32((uint32_t)v, m), hi = xor_u32((uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}
WAVE_FN double xor_f64(double v, int m) { return __builtin_bit_cast(double, xor_u64(__builtin_bit_cast(uint64_t, v), m)); }
WAVE_FN int xor_i32(int v, int m) { return (int)xor_u32((uint32_t)v, m); }

// value of lane + 1 (lane 63: 0) and of lane - 1 (lane 0: 0)
WAVE_FN uint32_t next_u32(uint32_t v) {
    const int l = lane_id();
    uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xF, 0xF, true);  // row_shl:1
    const uint32_t b16 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t b32 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
    const uint32_t b48 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    r = l == 15 ? b16 : r;
    r = l == 31 ? b32 : r;
    r = l == 47 ? b48 : r;
    return r;
}
WAVE_FN uint32_t prev_u32(uint32_t v) {
    const int l = lane_id();
    uint32_t r = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);  // row_shr:1
    const uint32_t b15 = (uint32_t)__builtin_amdgcn_readlane((int)v, 15);
    const uint32_t b31 = (uint32_t)__builtin_amdgcn_readlane((int)v, 31);
    const uint32_t b47 = (uint32_t)__builtin_amdgcn_readlane((int)v, 47);
    r = l == 16 ? b15 : r;
    r = l == 32 ? b31 : r;
    r = l == 48 ? b47 : r;
    return r;
}
WAVE_FN double next_f64(double v) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint64_t r = ((uint64_t)next_u32((uint32_t)(b >> 32)) << 32) | next_u32((uint32_t)b);
    return __builtin_bit_cast(double, r);
}
WAVE_FN uint64_t prev_u64(uint64_t v) { return ((uint64_t)prev_u32((uint32_t)(v >> 32)) << 32) | prev_u32((uint32_t)v); }

// butterfly sum: every lane gets the same total (fixed association, deterministic)
WAVE_FN double wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + xor_f64(v, m);
    return v;
}

// Reduce-scatter sum of N doubles per lane (N <= 64, padded to the next power of two P): the
// butterfly's tree, each node computed once. wave_sum has every lane compute every level of every
// value; here, at xor step m, a lane keeps one half of its live values (the upper half where its
// bit m is set), receives the partner's copies of those and adds them, so the live set halves per
// step while the levels still run 1, 2, 4, ... Each node is own + partner where the butterfly had
// own + partner on one lane and partner + own on the other: IEEE addition commutes, so every total
// has wave_sum's bits (a NaN's payload aside). Once one value is left the remaining steps are the
// butterfly's. Lane l ends with the total of index scatter_index(P, l).
//   get(i)   value of slot i; called once, at the first step, with i a constant after unrolling
//   live     bit i set: slot i is wanted. A pair whose two slots are both unwanted (or padding)
//            costs nothing; a pair with one wanted slot is a plain butterfly step on it.
// Everything unrolls to static register indices.
constexpr int scatter_width(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
// the index whose total lane `lane` holds: step m kept the upper half (+h) where bit m is set; for
// P = 64 the 6-bit reversal of the lane
__host__ __device__ constexpr int scatter_index(int P, int lane) {
    int idx = 0;
    for (int m = 1, h = P >> 1; h >= 1; m <<= 1, h >>= 1)
        if (lane & m) idx += h;
    return idx;
}
// what lane ^ m sends: its x where this lane's bit m is clear, its y where it is set
WAVE_FN uint32_t scatter_recv_u32(uint32_t x, uint32_t y, int m, bool b) {
    switch (m) {
        case 4: {  // bank masks pick the lanes by bit 2: one move per side, no select
            const int t = __builtin_amdgcn_update_dpp(0, (int)x, 0x104, 0xF, 0x5, false);  // row_shl:4 into banks 0, 2
            return (uint32_t)__builtin_amdgcn_update_dpp(t, (int)y, 0x114, 0xF, 0xA, false);  // row_shr:4 into banks 1, 3
        }
        case 8: {
            const int t = __builtin_amdgcn_update_dpp(0, (int)x, 0x108, 0xF, 0x3, false);  // row_shl:8 into banks 0, 1
            return (uint32_t)__builtin_amdgcn_update_dpp(t, (int)y, 0x118, 0xF, 0xC, false);  // row_shr:8 into banks 2, 3
        }
        default: return xor_u32(b ? x : y, m);  // every lane sends the half it does not keep
    }
}
// one pair of a step: the node this lane keeps, own + partner
WAVE_FN double scatter_pair(double x, double y, int m, bool b) {
    const uint64_t xb = __builtin_bit_cast(uint64_t, x), yb = __builtin_bit_cast(uint64_t, y);
    if (m >= 16) {
        // the swap delivers both operands: {own x, partner's x} where bit m is clear,
        // {partner's y, own y} where it is set
        const auto lo = m == 16 ? __builtin_amdgcn_permlane16_swap((uint32_t)xb, (uint32_t)yb, false, false)
                                : __builtin_amdgcn_permlane32_swap((uint32_t)xb, (uint32_t)yb, false, false);
        const auto hi = m == 16 ? __builtin_amdgcn_permlane16_swap((uint32_t)(xb >> 32), (uint32_t)(yb >> 32), false, false)
                                : __builtin_amdgcn_permlane32_swap((uint32_t)(xb >> 32), (uint32_t)(yb >> 32), false, false);
        const uint64_t p = ((uint64_t)hi[0] << 32) | lo[0], q = ((uint64_t)hi[1] << 32) | lo[1];
        return __builtin_bit_cast(double, p) + __builtin_bit_cast(double, q);
    }
    const uint64_t r = ((uint64_t)scatter_recv_u32((uint32_t)(xb >> 32), (uint32_t)(yb >> 32), m, b) << 32) |
                       scatter_recv_u32((uint32_t)xb, (uint32_t)yb, m, b);
    return (b ? y : x) + __builtin_bit_cast(double, r);
}
template <int N, class Get>
WAVE_FN double scatter_sum(const Get& get, uint64_t live) {
    static_assert(N >= 1 && N <= 64, "one wave's lanes hold the totals");
    constexpr int P = scatter_width(N);
    const int l = lane_id();
    double v[P];
    int m = 1;
#pragma unroll
    for (int h = P >> 1; h >= 1; h >>= 1, m <<= 1) {
        const bool b = (l & m) != 0;
#pragma unroll
        for (int i = 0; i < h; i++) {
            const bool la = (live >> i) & 1, lb = (live >> (i + h)) & 1;
            if (!la && !lb) continue;
            double x = 0, y = 0;
            if (la) x = h == P >> 1 ? get(i) : v[i];
            if (lb) y = h == P >> 1 ? get(i + h) : v[i + h];
            if (la && lb) {
                v[i] = scatter_pair(x, y, m, b);
            } else {
                const double t = la ? x : y;
                v[i] = t + xor_f64(t, m);
            }
        }
        live = (live | (live >> h)) & ((1ull << h) - 1);
    }
    double r;
    if constexpr (P == 1) r = get(0);
    else r = v[0];
#pragma unroll
    for (; m < 64; m <<= 1) r = r + xor_f64(r, m);
    return r;
}

WAVE_FN int wave_or(int v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v |= xor_i32(v, m);
    return v;
}
WAVE_FN int wave_max(int v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = max(v, xor_i32(v, m));
    return v;
}

// inclusive prefix sum over the wave (DPP row shifts, then row broadcasts)
WAVE_FN int wave_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false); // row_bcast:15 into rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false); // row_bcast:31 into rows 2, 3
    return v;
}

}  // namespace armour
