// The fixed-sweep cyclic Jacobi iteration on a symmetric 3x3 matrix in float64, as cloud_normals.hip (section 24) and cloud_plane.hip
// (section 26) run it: a sweep is the rotations (0,1), (0,2), (1,2); a rotation is skipped only on an off-diagonal of exactly 0.
#pragma once
#include "common.h"

namespace rald {

// one Jacobi rotation of the pair (p, q) - app, aqq the diagonal, apq the entry to clear, arp, arq the third row's entries, v*p / v*q the
// two columns of V: the header's formulas, operation for operation
__device__ __forceinline__ void nrm_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                           double& v1p, double& v1q, double& v2p, double& v2q) {
#pragma clang fp contract(off)
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double den = fabs(theta) + __dsqrt_rn(theta * theta + 1.0);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / den;
    const double c = 1.0 / __dsqrt_rn(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    v0p = a0; v0q = b0;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    v1p = a1; v1q = b1;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v2p = a2; v2q = b2;
}

// (la, column a) and (lb, column b), a before b: exchanged iff la > lb, so equal eigenvalues keep the lower column first
__device__ __forceinline__ void nrm_order(double& la, double& lb, double& xa, double& ya, double& za, double& xb, double& yb, double& zb) {
    if (la > lb) {
        double t;
        t = la; la = lb; lb = t;
        t = xa; xa = xb; xb = t;
        t = ya; ya = yb; yb = t;
        t = za; za = zb; zb = t;
    }
}

}  // namespace rald
