// SO(3) logarithm and the inverse right Jacobian, as the pose priors (prior_kernels.hip) and the motion prior of the
// smoothed tracker (smooth_kernels.hip, section 16) use them.  fp64, registers only.
#pragma once
#include <hip/hip_runtime.h>

namespace aar {

// log(Q)^v of a rotation matrix (row-major): theta from atan2(|v| / 2, (tr - 1) / 2), v = vee(Q - Q^T) = 2 sin(theta) n; near pi the axis comes
// from the symmetric part (Q + Q^T) / 2 - cos(theta) I = (1 - cos(theta)) n n^T, its sign from v.
__device__ __forceinline__ void so3_log(const double *Q, double *phi, double &theta) {
    const double v0 = Q[7] - Q[5], v1 = Q[2] - Q[6], v2 = Q[3] - Q[1];
    const double s2 = sqrt(v0 * v0 + v1 * v1 + v2 * v2);   // 2 sin(theta)
    const double c = 0.5 * (Q[0] + Q[4] + Q[8] - 1.0);
    theta = atan2(0.5 * s2, c);
    if (c > -0.99) {
        // theta / (2 sin theta) -> 1/2 + theta^2 / 12 at small angles
        const double k = theta < 1e-4 ? 0.5 + theta * theta * (1.0 / 12.0) : theta / s2;
        phi[0] = k * v0; phi[1] = k * v1; phi[2] = k * v2;
        return;
    }
    const double oc = 1.0 - c;
    const double d0 = (Q[0] - c) / oc, d1 = (Q[4] - c) / oc, d2 = (Q[8] - c) / oc;   // n_i^2
    double n0, n1, n2;
    if (d0 >= d1 && d0 >= d2) {
        n0 = sqrt(fmax(d0, 0.0));
        n1 = 0.5 * (Q[1] + Q[3]) / (oc * n0); n2 = 0.5 * (Q[2] + Q[6]) / (oc * n0);
    } else if (d1 >= d2) {
        n1 = sqrt(fmax(d1, 0.0));
        n0 = 0.5 * (Q[1] + Q[3]) / (oc * n1); n2 = 0.5 * (Q[5] + Q[7]) / (oc * n1);
    } else {
        n2 = sqrt(fmax(d2, 0.0));
        n0 = 0.5 * (Q[2] + Q[6]) / (oc * n2); n1 = 0.5 * (Q[5] + Q[7]) / (oc * n2);
    }
    const double in = 1.0 / sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    const double sg = (n0 * v0 + n1 * v1 + n2 * v2) < 0.0 ? -1.0 : 1.0;
    phi[0] = sg * theta * n0 * in; phi[1] = sg * theta * n1 * in; phi[2] = sg * theta * n2 * in;
}

// J_r(phi)^-1 (row-major) of phi with |phi| = th
__device__ __forceinline__ void so3_jr_inv(const double *phi, double th, double *Ji) {
    // J_r(phi)^-1 = I + [phi]x / 2 + k [phi]x^2,  k = 1/th^2 - cot(th/2) / (2 th),  cot(th/2) = (1 + cos th) / sin th = sin th / (1 - cos th).
    // The first quotient divides two quantities that vanish at pi and there carries the rounding of 1 + cos th divided by sin th (7e-11 in k at
    // pi - 1e-6, 8e-10 at pi - 1e-9); the second does the same at 0.  Each is used on its own side of pi / 2, where it has no cancellation.
    double k;
    if (th < 1e-2) {
        const double t2 = th * th;
        k = (1.0 / 12.0) + t2 * (1.0 / 720.0) + t2 * t2 * (1.0 / 30240.0);
    } else {
        double s, c;
        sincos(th, &s, &c);
        k = 1.0 / (th * th) - (c > 0.0 ? (1.0 + c) / (2.0 * th * s) : s / (2.0 * th * (1.0 - c)));
    }
    const double x = phi[0], y = phi[1], z = phi[2], p2 = x * x + y * y + z * z;
    Ji[0] = 1.0 + k * (x * x - p2); Ji[1] = -0.5 * z + k * x * y;    Ji[2] = 0.5 * y + k * x * z;
    Ji[3] = 0.5 * z + k * x * y;    Ji[4] = 1.0 + k * (y * y - p2); Ji[5] = -0.5 * x + k * y * z;
    Ji[6] = -0.5 * y + k * x * z;   Ji[7] = 0.5 * x + k * y * z;    Ji[8] = 1.0 + k * (z * z - p2);
}

}  // namespace aar
