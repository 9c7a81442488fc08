// Float64 complex arithmetic and the register DFT-4 / 8 / 16 butterflies of
// the f64 transforms (sn_stft64 in aa_signal.hip, ci_bands in
// aa_cacophony.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace aa {

__device__ __forceinline__ double2 dadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 dsub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 dmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 dnegi(double2 a) { return make_double2(a.y, -a.x); }  // a * (-i)

constexpr double kCos8 = 0.92387953251128675613;  // cos(pi / 8)
constexpr double kSin8 = 0.38268343236508977173;  // sin(pi / 8)
constexpr double kRt2 = 0.70710678118654752440;   // sqrt(1 / 2)

// a * W16^E, W16 = exp(-2 pi i / 16), for the exponents a DFT-16 and the
// real split need (E in 0..9)
template <int E>
__device__ __forceinline__ double2 w16(double2 a) {
    static_assert(E >= 0 && E <= 9, "w16");
    if constexpr (E == 0) return a;
    else if constexpr (E == 1) return make_double2(a.x * kCos8 + a.y * kSin8, a.y * kCos8 - a.x * kSin8);
    else if constexpr (E == 2) return make_double2(kRt2 * (a.x + a.y), kRt2 * (a.y - a.x));
    else if constexpr (E == 3) return make_double2(a.x * kSin8 + a.y * kCos8, a.y * kSin8 - a.x * kCos8);
    else if constexpr (E == 4) return dnegi(a);
    else if constexpr (E == 5) return make_double2(a.y * kCos8 - a.x * kSin8, -(a.x * kCos8 + a.y * kSin8));
    else if constexpr (E == 6) return make_double2(kRt2 * (a.y - a.x), -kRt2 * (a.x + a.y));
    else if constexpr (E == 7) return make_double2(a.y * kSin8 - a.x * kCos8, -(a.x * kSin8 + a.y * kCos8));
    else if constexpr (E == 8) return make_double2(-a.x, -a.y);
    else return make_double2(-(a.x * kCos8 + a.y * kSin8), a.x * kSin8 - a.y * kCos8);  // E == 9
}

__device__ __forceinline__ void ddft4(double2& a, double2& b, double2& c, double2& d) {  // natural order out
    const double2 t0 = dadd(a, c), t1 = dsub(a, c), t2 = dadd(b, d), t3 = dnegi(dsub(b, d));
    a = dadd(t0, t2);
    c = dsub(t0, t2);
    b = dadd(t1, t3);
    d = dsub(t1, t3);
}
__device__ __forceinline__ void ddft8(double2 (&v)[8]) {  // natural order out
    double2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
    double2 o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
    ddft4(e0, e1, e2, e3);
    ddft4(o0, o1, o2, o3);
    o1 = w16<2>(o1);
    o2 = w16<4>(o2);
    o3 = w16<6>(o3);
    v[0] = dadd(e0, o0);
    v[4] = dsub(e0, o0);
    v[1] = dadd(e1, o1);
    v[5] = dsub(e1, o1);
    v[2] = dadd(e2, o2);
    v[6] = dsub(e2, o2);
    v[3] = dadd(e3, o3);
    v[7] = dsub(e3, o3);
}
// 16-point DFT in place (radix 4 x 4): X[k] is left in v[dp16(k)]
__device__ __forceinline__ constexpr int dp16(int k) { return 4 * (k & 3) + (k >> 2); }
__device__ __forceinline__ void ddft16(double2 (&v)[16]) {
#pragma unroll
    for (int b = 0; b < 4; ++b) ddft4(v[b], v[4 + b], v[8 + b], v[12 + b]);  // v[4c + b] = Y_b[c]
    v[5] = w16<1>(v[5]);
    v[9] = w16<2>(v[9]);
    v[13] = w16<3>(v[13]);
    v[6] = w16<2>(v[6]);
    v[10] = w16<4>(v[10]);
    v[14] = w16<6>(v[14]);
    v[7] = w16<3>(v[7]);
    v[11] = w16<6>(v[11]);
    v[15] = w16<9>(v[15]);
#pragma unroll
    for (int c = 0; c < 4; ++c) ddft4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);  // v[4c + d] = X[c + 4d]
}

}  // namespace aa
