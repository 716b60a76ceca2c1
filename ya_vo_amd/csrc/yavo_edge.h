// yavo_edge.h -- the reference's projection edge (include/Optimizer.hpp:64-126: computeError and linearizeOplus of the
// pose-only edge) as the pose LM (yavo_pose.hip) and the bundle adjustment (yavo_ba.hip) evaluate it.  Both are
// bit-exact against the same oracle (edge_error / edge_jacobian of oracle/yavo_oracle_geom.c, ba_error / ba_jacobians
// of oracle/yavo_oracle_ba.c), so the expression has this one home.  Every expression in the oracle's order; files are
// built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "yavo_se3.h"

namespace yavo {
namespace edge {

using se3::se3_act;

// the edge's error from its camera-frame point pc = T X (computeError: K pc, projected)
__device__ __forceinline__ void edge_error_pc(const double* pc, const double* K, const double* meas, double* e) {
    double u0 = K[0] * pc[0] + K[1] * pc[1] + K[2] * pc[2];
    double u1 = K[3] * pc[0] + K[4] * pc[1] + K[5] * pc[2];
    double u2 = K[6] * pc[0] + K[7] * pc[1] + K[8] * pc[2];
    e[0] = meas[0] - u0 / u2;
    e[1] = meas[1] - u1 / u2;
}

__device__ __forceinline__ void edge_error(const double* T, const double* K, const double* X, const double* meas,
                                           double* e) {
    double pc[3];
    se3_act(T, X, pc);
    edge_error_pc(pc, K, meas, e);
}

// linearizeOplus's 2 x 6 Jacobian from the same pc (computeError and linearizeOplus both form T X at one estimate:
// one evaluation serves both, the same operations)
__device__ __forceinline__ void edge_jacobian_pc(const double* pc, const double* K, double* J) {
    double fx = K[0], fy = K[4];
    double x = pc[0], y = pc[1], z = pc[2];
    double zinv = 1.0 / (z + 1e-18);
    double zinv2 = zinv * zinv;
    J[0] = -fx * zinv; J[1] = 0; J[2] = fx * x * zinv2; J[3] = fx * x * y * zinv2;
    J[4] = -fx - fx * x * x * zinv2; J[5] = fx * y * zinv;
    J[6] = 0; J[7] = -fy * zinv; J[8] = fy * y * zinv2; J[9] = fy + fy * y * y * zinv2;
    J[10] = -fy * x * y * zinv2; J[11] = -fy * x * zinv;
}

}  // namespace edge
}  // namespace yavo
