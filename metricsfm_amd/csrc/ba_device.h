// Device-side arithmetic shared by the BA kernels: the reference's projection model with
// closed-form derivatives, the Huber corrector and small dense helpers.  FP64 throughout.
#pragma once
#include <hip/hip_runtime.h>

// AngleAxisRotatePoint (SfM/src/utils/basic_funcs.cc:160-225 == ceres/rotation.h, called from
// reprojection_error_pose_cam_xyz.h:41) + translation + pinhole with radial distortion
// (reprojection_error_pose_cam_xyz.h:44-63; the other four functors share the model).
// J (if non-null) is 2x12 row-major: [d pose(6) | d cam(3) | d xyz(3)], already times weight.
// The rotation derivative is the exact derivative of the evaluated formula (including the
// first-order branch at theta^2 <= DBL_EPSILON), i.e. what Ceres' Jets propagate.
// What depends on the camera's angle-axis vector alone: which branch of the rotation formula applies, and sin, cos and
// 1 / |a|.  A camera is seen by thousands of observations per evaluation; msfm_rot_prepare computes these four numbers
// once per camera and parameter set (rot[4 c ..]: flag, sin, cos, 1/theta) with the operations msfm_reproj would use.
__host__ __device__ __forceinline__ void msfm_rot_prepare(const double* __restrict__ pose, double* __restrict__ rc) {
  const double a0 = pose[0], a1 = pose[1], a2 = pose[2];
  const double theta2 = a0 * a0 + a1 * a1 + a2 * a2;
  double s = 0.0, c = 1.0, ti = 0.0, flag = 0.0;
  if (theta2 > 2.220446049250313e-16) {
    const double theta = sqrt(theta2);
    sincos(theta, &s, &c);
    ti = 1.0 / theta;
    flag = 1.0;
  }
  rc[0] = flag; rc[1] = s; rc[2] = c; rc[3] = ti;
}

__host__ __device__ __forceinline__ void msfm_reproj(const double* __restrict__ pose, const double* __restrict__ rc, const double* __restrict__ cam,
                                                     const double* __restrict__ xyz, double ox, double oy, double weight,
                                                     double* r, double* J) {
  const double a0 = pose[0], a1 = pose[1], a2 = pose[2];
  const double X0 = xyz[0], X1 = xyz[1], X2 = xyz[2];
  double p0, p1, p2;
  double dpdw[9];
  double R[9];
  if (rc[0] != 0.0) {
    const double s = rc[1], c = rc[2], ti = rc[3];
    const double w0 = a0 * ti, w1 = a1 * ti, w2 = a2 * ti;
    const double wx0 = w1 * X2 - w2 * X1, wx1 = w2 * X0 - w0 * X2, wx2 = w0 * X1 - w1 * X0;
    const double wdx = w0 * X0 + w1 * X1 + w2 * X2;
    const double omc = 1.0 - c;
    const double tmp = wdx * omc;
    p0 = X0 * c + wx0 * s + w0 * tmp;
    p1 = X1 * c + wx1 * s + w1 * tmp;
    p2 = X2 * c + wx2 * s + w2 * tmp;
    if (J) {
      const double w[3] = {w0, w1, w2};
      const double wx[3] = {wx0, wx1, wx2};
      const double Xv[3] = {X0, X1, X2};
#pragma unroll
      for (int j = 0; j < 3; j++) {
        double dw[3];
#pragma unroll
        for (int i = 0; i < 3; i++) dw[i] = ((i == j ? 1.0 : 0.0) - w[i] * w[j]) * ti;
        const double dwx[3] = {dw[1] * X2 - dw[2] * X1, dw[2] * X0 - dw[0] * X2, dw[0] * X1 - dw[1] * X0};
        const double dwdx = dw[0] * X0 + dw[1] * X1 + dw[2] * X2;
        const double dc = -s * w[j], ds = c * w[j];
        const double dtmp = dwdx * omc - wdx * dc;
#pragma unroll
        for (int i = 0; i < 3; i++) dpdw[i * 3 + j] = Xv[i] * dc + dwx[i] * s + wx[i] * ds + dw[i] * tmp + w[i] * dtmp;
      }
      R[0] = c + w0 * w0 * omc;      R[1] = w0 * w1 * omc - w2 * s; R[2] = w1 * s + w0 * w2 * omc;
      R[3] = w2 * s + w0 * w1 * omc; R[4] = c + w1 * w1 * omc;      R[5] = -w0 * s + w1 * w2 * omc;
      R[6] = -w1 * s + w0 * w2 * omc; R[7] = w0 * s + w1 * w2 * omc; R[8] = c + w2 * w2 * omc;
    }
  } else {
    p0 = X0 + (a1 * X2 - a2 * X1);
    p1 = X1 + (a2 * X0 - a0 * X2);
    p2 = X2 + (a0 * X1 - a1 * X0);
    if (J) {
      dpdw[0] = 0;   dpdw[1] = X2;  dpdw[2] = -X1;
      dpdw[3] = -X2; dpdw[4] = 0;   dpdw[5] = X0;
      dpdw[6] = X1;  dpdw[7] = -X0; dpdw[8] = 0;
      R[0] = 1;   R[1] = -a2; R[2] = a1;
      R[3] = a2;  R[4] = 1;   R[5] = -a0;
      R[6] = -a1; R[7] = a0;  R[8] = 1;
    }
  }
  p0 += pose[3]; p1 += pose[4]; p2 += pose[5];
  // (with Jacobians: Ceres' Jet division, value part f.a * (1 / g.a); without: the functor's plain division - one rounding
  //  apart, as in the reference's two evaluation modes)
  const double iz = 1.0 / p2;
  const double xp = J ? p0 * iz : p0 / p2, yp = J ? p1 * iz : p1 / p2;
  const double f = cam[0], l1 = cam[1], l2 = cam[2];
  const double r2 = xp * xp + yp * yp;
  const double dist = 1.0 + r2 * (l1 + l2 * r2);
  r[0] = weight * (f * dist * xp - ox);
  r[1] = weight * (f * dist * yp - oy);
  if (!J) return;
  const double dd = l1 + 2.0 * l2 * r2;
  const double uxp = f * (dist + 2.0 * xp * xp * dd), uyp = f * 2.0 * xp * yp * dd;
  const double vxp = uyp, vyp = f * (dist + 2.0 * yp * yp * dd);
  const double up[3] = {uxp * iz, uyp * iz, -(uxp * xp + uyp * yp) * iz};
  const double vp[3] = {vxp * iz, vyp * iz, -(vxp * xp + vyp * yp) * iz};
#pragma unroll
  for (int j = 0; j < 3; j++) {
    J[j] = weight * (up[0] * dpdw[j] + up[1] * dpdw[3 + j] + up[2] * dpdw[6 + j]);
    J[12 + j] = weight * (vp[0] * dpdw[j] + vp[1] * dpdw[3 + j] + vp[2] * dpdw[6 + j]);
    J[3 + j] = weight * up[j];
    J[12 + 3 + j] = weight * vp[j];
    J[9 + j] = weight * (up[0] * R[j] + up[1] * R[3 + j] + up[2] * R[6 + j]);
    J[12 + 9 + j] = weight * (vp[0] * R[j] + vp[1] * R[3 + j] + vp[2] * R[6 + j]);
  }
  J[6] = weight * dist * xp;        J[12 + 6] = weight * dist * yp;
  J[7] = weight * f * r2 * xp;      J[12 + 7] = weight * f * r2 * yp;
  J[8] = weight * f * r2 * r2 * xp; J[12 + 8] = weight * f * r2 * r2 * yp;
}

// ceres::HuberLoss(a) (constructed at optimizer.cc:84): rho0 = rho(s), rho1 = rho'(s).
__host__ __device__ __forceinline__ void msfm_huber(double a, double s, double& rho0, double& rho1) {
  const double b = a * a;
  if (s > b) {
    const double r = sqrt(s);
    rho0 = 2.0 * a * r - b;
    rho1 = fmax(2.2250738585072014e-308, a / r);
  } else {
    rho0 = s;
    rho1 = 1.0;
  }
}

// The arithmetic of obs_linearize (ba.hip) on values already in registers (k_ftf evaluates it camera by camera: pose, rotation
// cache, intrinsics and their column scales are the same for a whole chunk of rows): the Huber-corrected, column-scaled row.
__host__ __device__ __forceinline__ double linearize_core(const double (&pose)[6], const double (&rc)[4], const double (&cm)[3], const double (&X)[3], double ox,
                                                          double oy, double ow, const double (&sc)[6], const double (&sm)[3], const double (&sp)[3], double huber,
                                                          double& r0, double& r1, double (&jc)[12], double (&jm)[6], double (&jp)[6]) {
  double r[2], J[24];
  msfm_reproj(pose, rc, cm, X, ox, oy, ow, r, J);
  double rho0, rho1;
  msfm_huber(huber, r[0] * r[0] + r[1] * r[1], rho0, rho1);
  const double sq = sqrt(rho1);
  r0 = sq * r[0]; r1 = sq * r[1];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const double s = sq * sc[j];
    jc[j] = s * J[j];
    jc[6 + j] = s * J[12 + j];
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double s = sq * sm[j];
    jm[j] = s * J[6 + j];
    jm[3 + j] = s * J[12 + 6 + j];
    const double spj = sq * sp[j];
    jp[j] = spj * J[9 + j];
    jp[3 + j] = spj * J[12 + 9 + j];
  }
  return 0.5 * rho0;
}

// What the back substitution needs of a row (k_backsub): the corrected residual, the scaled point block jp and
// q = -(Jc z_c + Jm z_m), the derivative of the residual along ONE direction d = -(scale * z) over the row's camera block
// (da = d[0..2], dt = d[3..5]) and intrinsics block (df, dl1, dl2).  That is one forward-mode tangent - about one more function
// evaluation - where the six camera and three intrinsics columns of linearize_core cost three times that and leave 18 numbers
// to contract.  A frozen block's scales are zero and so is its part of d.  With w = a / theta, wx = w x X, wdx = w.X,
// omc = 1 - c, tmp = wdx omc (msfm_reproj's names) the tangent of p = c X + s wx + tmp w + t is
//   dp = v (w.da) + ti ( s (da x X) + omc ((X.da) w + wdx da) ) + dt,   v = u - ti (s wx + 2 tmp w),  u = c wx - s X + (s wdx) w
// (u = dp/dtheta at fixed w, the rest is dw = (da - w (w.da)) ti), in the first-order branch dp = da x X + dt, and behind the
// projection  q_u = weight (uxp dxp + uyp dyp + xp m), q_v = weight (uyp dxp + vyp dyp + yp m), dxp = (dp0 - xp dp2) iz,
// m = dist df + f r2 (dl1 + r2 dl2).  The point block is contracted first, R is never formed: row k = R^T g_k =
// c g_k + s (g_k x w) + omc (g_k.w) w with g_k the gradient of residual component k by the camera-frame point (first-order
// branch: g_k + g_k x a, the same expression at w = a, s = c = 1, omc = 0).  The residual is formed by msfm_reproj's operations
// (its Jacobian mode: xp = p0 * iz), then Huber, then sq, as linearize_core forms it: r0 and r1 keep their bits.
__host__ __device__ __forceinline__ void msfm_backsub_row(const double (&pose)[6], const double (&rc)[4], const double (&cm)[3], const double (&X)[3],
                                                          double ox, double oy, double weight, const double (&sc)[6], const double (&sm)[3],
                                                          const double (&sp)[3], const double (&zc)[6], const double (&zm)[3], double huber,
                                                          double& r0, double& r1, double (&jp)[6], double& q0, double& q1) {
  const double a0 = pose[0], a1 = pose[1], a2 = pose[2];
  const double X0 = X[0], X1 = X[1], X2 = X[2];
  const double da0 = -(sc[0] * zc[0]), da1 = -(sc[1] * zc[1]), da2 = -(sc[2] * zc[2]);
  const double dt0 = -(sc[3] * zc[3]), dt1 = -(sc[4] * zc[4]), dt2 = -(sc[5] * zc[5]);
  const double df = -(sm[0] * zm[0]), dl1 = -(sm[1] * zm[1]), dl2 = -(sm[2] * zm[2]);
  const double cx0 = da1 * X2 - da2 * X1, cx1 = da2 * X0 - da0 * X2, cx2 = da0 * X1 - da1 * X0;   // da x X
  double p0, p1, p2, dp0, dp1, dp2;
  double w0, w1, w2, s, c, omc;   // what rotates the point block below
  if (rc[0] != 0.0) {
    s = rc[1]; c = rc[2];
    const double ti = rc[3];
    w0 = a0 * ti; w1 = a1 * ti; w2 = a2 * ti;
    const double wx0 = w1 * X2 - w2 * X1, wx1 = w2 * X0 - w0 * X2, wx2 = w0 * X1 - w1 * X0;
    const double wdx = w0 * X0 + w1 * X1 + w2 * X2;
    omc = 1.0 - c;
    const double tmp = wdx * omc;
    p0 = X0 * c + wx0 * s + w0 * tmp;
    p1 = X1 * c + wx1 * s + w1 * tmp;
    p2 = X2 * c + wx2 * s + w2 * tmp;
    const double swdx = s * wdx, k2 = 2.0 * tmp;
    const double v0 = (c * wx0 - s * X0 + swdx * w0) - ti * (s * wx0 + k2 * w0);
    const double v1 = (c * wx1 - s * X1 + swdx * w1) - ti * (s * wx1 + k2 * w1);
    const double v2 = (c * wx2 - s * X2 + swdx * w2) - ti * (s * wx2 + k2 * w2);
    const double wda = w0 * da0 + w1 * da1 + w2 * da2;
    const double xda = X0 * da0 + X1 * da1 + X2 * da2;
    dp0 = v0 * wda + ti * (s * cx0 + omc * (xda * w0 + wdx * da0)) + dt0;
    dp1 = v1 * wda + ti * (s * cx1 + omc * (xda * w1 + wdx * da1)) + dt1;
    dp2 = v2 * wda + ti * (s * cx2 + omc * (xda * w2 + wdx * da2)) + dt2;
  } else {
    p0 = X0 + (a1 * X2 - a2 * X1);
    p1 = X1 + (a2 * X0 - a0 * X2);
    p2 = X2 + (a0 * X1 - a1 * X0);
    dp0 = cx0 + dt0; dp1 = cx1 + dt1; dp2 = cx2 + dt2;
    w0 = a0; w1 = a1; w2 = a2; s = 1.0; c = 1.0; omc = 0.0;
  }
  p0 += pose[3]; p1 += pose[4]; p2 += pose[5];
  const double iz = 1.0 / p2;
  const double xp = p0 * iz, yp = p1 * iz;
  const double f = cm[0], l1 = cm[1], l2 = cm[2];
  const double r2 = xp * xp + yp * yp;
  const double dist = 1.0 + r2 * (l1 + l2 * r2);
  const double ru = weight * (f * dist * xp - ox);
  const double rv = weight * (f * dist * yp - oy);
  double rho0, rho1;
  msfm_huber(huber, ru * ru + rv * rv, rho0, rho1);
  const double sq = sqrt(rho1);
  r0 = sq * ru; r1 = sq * rv;
  const double dd = l1 + 2.0 * l2 * r2;
  const double uxp = f * (dist + 2.0 * xp * xp * dd), uyp = f * 2.0 * xp * yp * dd, vyp = f * (dist + 2.0 * yp * yp * dd);
  const double dxp = (dp0 - xp * dp2) * iz, dyp = (dp1 - yp * dp2) * iz;
  const double m = dist * df + f * r2 * (dl1 + r2 * dl2);
  const double ws = weight * sq;
  q0 = ws * (uxp * dxp + uyp * dyp + xp * m);
  q1 = ws * (uyp * dxp + vyp * dyp + yp * m);
  const double wi = ws * iz;
  const double g[2][3] = {{uxp * wi, uyp * wi, -(uxp * xp + uyp * yp) * wi}, {uyp * wi, vyp * wi, -(uyp * xp + vyp * yp) * wi}};
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const double g0 = g[k][0], g1 = g[k][1], g2 = g[k][2];
    const double gw = omc * (g0 * w0 + g1 * w1 + g2 * w2);
    jp[3 * k + 0] = sp[0] * (c * g0 + s * (g1 * w2 - g2 * w1) + gw * w0);
    jp[3 * k + 1] = sp[1] * (c * g1 + s * (g2 * w0 - g0 * w2) + gw * w1);
    jp[3 * k + 2] = sp[2] * (c * g2 + s * (g0 * w1 - g1 * w0) + gw * w2);
  }
}

// Deterministic wave / block sums (fixed butterfly, fixed wave order).
// The butterfly's partner values travel by DPP (inside a row of 16 lanes) and by the gfx950 row / half-wave swaps - VALU
// instructions - instead of ds_bpermute through the LDS pipe (two per step and double: 936 of them in one k_ftf wave).
// Every step adds the same two numbers as `v += __shfl_xor(v, off)` did, so results are bit-identical to that form.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
#define MSFM_DPP_XOR1 0xB1          // quad_perm [1,0,3,2]
#define MSFM_DPP_XOR2 0x4E          // quad_perm [2,3,0,1]
#define MSFM_DPP_ROR8 0x128         // row_ror:8 = lane ^ 8 inside a row
#define MSFM_DPP_HALF_MIRROR 0x141  // lane -> 7 - lane inside each half row
#define MSFM_DPP_SHL4 0x104         // row_shl:4 = from lane + 4 of the row (the next quad); the row's last quad gets 0
#define MSFM_DPP_SHL8 0x108         // row_shl:8 = from lane + 8 of the row; the row's upper half gets 0
__device__ __forceinline__ int dpp_xor4_b32(int x) {
  // lane ^ 4: quads 0 and 2 take from the quad above (row_shl:4), quads 1 and 3 from the quad below (row_shr:4)
  const int t = __builtin_amdgcn_update_dpp(0, x, 0x104, 0xf, 0x5, false);
  return __builtin_amdgcn_update_dpp(t, x, 0x114, 0xf, 0xa, false);
}
__device__ __forceinline__ double dpp_xor4_f64(double v) {
  return __hiloint2double(dpp_xor4_b32(__double2hiint(v)), dpp_xor4_b32(__double2loint(v)));
}
// the two halves of the row pairs / of the wave side by side: a = [R0 R0 R2 R2], b = [R1 R1 R3 R3] (rows of 16 lanes),
// resp. a = [lower 32, lower 32], b = [upper 32, upper 32]; a + b is the xor-16 (xor-32) step in every lane
__device__ __forceinline__ void swap16_f64(double v, double& a, double& b) {
  const unsigned lo = __double2loint(v), hi = __double2hiint(v);
  const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  a = __hiloint2double(h[0], l[0]);
  b = __hiloint2double(h[1], l[1]);
}
__device__ __forceinline__ void swap32_f64(double v, double& a, double& b) {
  const unsigned lo = __double2loint(v), hi = __double2hiint(v);
  const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  a = __hiloint2double(h[0], l[0]);
  b = __hiloint2double(h[1], l[1]);
}
__device__ __forceinline__ double wave_sum(double v) {
  double a, b;
  swap32_f64(v, a, b); v = a + b;
  swap16_f64(v, a, b); v = a + b;
  v += dpp_f64<MSFM_DPP_ROR8>(v);
  v += dpp_xor4_f64(v);
  v += dpp_f64<MSFM_DPP_XOR2>(v);
  v += dpp_f64<MSFM_DPP_XOR1>(v);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  double a, b;
  swap32_f64(v, a, b); v = fmax(a, b);
  swap16_f64(v, a, b); v = fmax(a, b);
  v = fmax(v, dpp_f64<MSFM_DPP_ROR8>(v));
  v = fmax(v, dpp_xor4_f64(v));
  v = fmax(v, dpp_f64<MSFM_DPP_XOR2>(v));
  v = fmax(v, dpp_f64<MSFM_DPP_XOR1>(v));
  return v;
}
// Sums of N per-lane values over the wave, every sum with the pairing tree of wave_sum (xor 32, 16, 8, 4, 2, 1), but as a
// reduce-scatter: at every step a lane keeps only half of its values (the lower half of the index range if its bit of the
// step is clear, the upper half otherwise) and adds its partner's copies of those - N + N/2 + N/4 + ... additions instead
// of 6 N, and after the last step every value sits in exactly one lane.  The two widest steps are one
// v_permlane{32,16}_swap per dword and pair of values.  Returns this lane's value and its index (-1: none).
// Bit-identical to wave_sum of each value (missing partners of an odd count are +0.0).
template <int D>
__device__ __forceinline__ double partner_f64(double t) {
  if constexpr (D == 8) return dpp_f64<MSFM_DPP_ROR8>(t);
  else if constexpr (D == 4) return dpp_xor4_f64(t);
  else if constexpr (D == 2) return dpp_f64<MSFM_DPP_XOR2>(t);
  else return dpp_f64<MSFM_DPP_XOR1>(t);
}
template <int D, int n, int N>
__device__ __forceinline__ void reduce_scatter_step(double (&v)[N], int lane) {
  constexpr int h = (n + 1) / 2;
  const bool low = (lane & D) == 0;
#pragma unroll
  for (int j = 0; j < h; j++) {
    const double a = v[j], b = (h + j < n) ? v[h + j] : 0.0;
    if constexpr (D == 32) { double x, y; const unsigned al = __double2loint(a), ah = __double2hiint(a), bl = __double2loint(b), bh = __double2hiint(b);
      const auto l = __builtin_amdgcn_permlane32_swap(al, bl, false, false); const auto hh = __builtin_amdgcn_permlane32_swap(ah, bh, false, false);
      x = __hiloint2double(hh[0], l[0]); y = __hiloint2double(hh[1], l[1]); v[j] = x + y;
    } else if constexpr (D == 16) { double x, y; const unsigned al = __double2loint(a), ah = __double2hiint(a), bl = __double2loint(b), bh = __double2hiint(b);
      const auto l = __builtin_amdgcn_permlane16_swap(al, bl, false, false); const auto hh = __builtin_amdgcn_permlane16_swap(ah, bh, false, false);
      x = __hiloint2double(hh[0], l[0]); y = __hiloint2double(hh[1], l[1]); v[j] = x + y;
    } else {
      const double t = low ? b : a;            // what the partner keeps
      const double mine = low ? a : b;
      v[j] = mine + partner_f64<D>(t);
    }
  }
}
template <int N>
__device__ __forceinline__ void wave_reduce_scatter(double (&v)[N], int lane, double& val, int& idx) {
  constexpr int n1 = (N + 1) / 2, n2 = (n1 + 1) / 2, n3 = (n2 + 1) / 2, n4 = (n3 + 1) / 2, n5 = (n4 + 1) / 2;
  static_assert(N <= 64 && (n5 + 1) / 2 == 1, "at most 64 values");
  reduce_scatter_step<32, N>(v, lane);
  reduce_scatter_step<16, n1>(v, lane);
  reduce_scatter_step<8, n2>(v, lane);
  reduce_scatter_step<4, n3>(v, lane);
  reduce_scatter_step<2, n4>(v, lane);
  reduce_scatter_step<1, n5>(v, lane);
  val = v[0];
  // which value that is: every lane has the same number of slots n (the upper half of an odd count is padded with one
  // empty slot), of which the first nv hold values lo, lo + 1, ...
  int lo = 0, nv = N, n = N;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int h = (n + 1) / 2;
    if (lane & d) { lo += h; nv = max(0, nv - h); } else nv = min(nv, h);
    n = h;
  }
  idx = nv > 0 ? lo : -1;
}

// blockDim.x must be 256.  Result valid in thread 0.
__device__ __forceinline__ double block_sum256(double v, double* sh /*[4]*/) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) t = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return t;
}
__device__ __forceinline__ double block_max256(double v, double* sh) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) t = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
  __syncthreads();
  return t;
}

// The point workgroups of k_point and k_backsub.  msfm_ba_create orders the eliminated points by track length class first:
// Q = up to 4 rows, S = 5..8 rows, L = 9..16 rows, X = more.  A Q workgroup holds 64 points with 4 lanes each, an S workgroup
// 32 points with 8 lanes each, an L workgroup 16 points with 16 lanes each - lane = row, every row is linearised exactly
// once - and an X workgroup 32 points with 8 lanes each that take their rows in rounds of 8.  A workgroup never mixes classes
// (a wave that held ONE long point among short ones used to run the long-track code in full for it: 4.0 linearisations per
// wave of k_point at config 3 where one is enough); the last workgroup of a class may be partly filled.  The point kernels
// are issue- and latency-bound FP64 at three waves per SIMD - a wave costs the same whatever the number of its live lanes -
// so the lane width follows the track length as far as the in-row lane operations (DPP) allow.
// (host and device, and nothing below needs the device: tests/ptmap_host_check.cc walks these functions on the CPU)
struct PtMap {
  int nQ, nS, nL, nX;   // points per class: blocks [0, nQ), [nQ, nQ + nS), [nQ + nS, nQ + nS + nL), [nQ + nS + nL, npb)
  int wQ, wS, wL;       // workgroups of the first three classes (the X workgroups follow)
};
__host__ __device__ inline int ptmap_lanes(const PtMap& m, int w) { return w < m.wQ ? 4 : w < m.wQ + m.wS ? 8 : w < m.wQ + m.wS + m.wL ? 16 : 0; }   // (0: X, rounds)
__host__ __device__ inline int ptmap_wg_points(int lanes) { return lanes ? 256 / lanes : 32; }   // points of a full workgroup
__host__ __device__ inline int ptmap_wg_first(const PtMap& m, int w) {
  if (w < m.wQ) return 64 * w;
  w -= m.wQ;
  if (w < m.wS) return m.nQ + 32 * w;
  w -= m.wS;
  if (w < m.wL) return m.nQ + m.nS + 16 * w;
  return m.nQ + m.nS + m.nL + 32 * (w - m.wL);
}
__host__ __device__ inline int ptmap_wg_end(const PtMap& m, int w) {   // one past the workgroup's last point
  const int e = ptmap_wg_first(m, w) + ptmap_wg_points(ptmap_lanes(m, w));
  const int cap = w < m.wQ ? m.nQ : w < m.wQ + m.wS ? m.nQ + m.nS : w < m.wQ + m.wS + m.wL ? m.nQ + m.nS + m.nL : m.nQ + m.nS + m.nL + m.nX;
  return e < cap ? e : cap;
}
__host__ __device__ inline int ptmap_wg_of(const PtMap& m, int pb) {
  if (pb < m.nQ) return pb >> 6;
  pb -= m.nQ;
  if (pb < m.nS) return m.wQ + (pb >> 5);
  pb -= m.nS;
  if (pb < m.nL) return m.wQ + m.wS + (pb >> 4);
  return m.wQ + m.wS + m.wL + ((pb - m.nL) >> 5);
}
#define PTMAP_CLASSES 4
__host__ __device__ inline int ptmap_class(int rows) { return rows <= 4 ? 0 : rows <= 8 ? 1 : rows <= 16 ? 2 : 3; }
// A problem whose points fit three workgroups per CU even at 32 points each has them all resident at once: the launch then
// lasts as long as its slowest workgroup, fewer and fuller workgroups save nothing, and the points of up to 4 rows stay S points
// in key order (measured on the 20 000-point window of config 5: 0.188 -> 0.191 ms per iteration with the class, k_point 26.6 ->
// 28.2 us).  min_points: MSFM_LANES4_MIN (0: always, what the tests use; < 0: the default, 32 x 3 x 256 CUs).
inline bool ptmap_use_lanes4(int npb, long min_points) { return npb > (min_points < 0 ? 32L * 3 * 256 : min_points); }
// (n: the points of up to 4, 5..8, 9..16 and more rows; lanes4 false: the first two share the S class)
inline PtMap ptmap_make(const int (&n)[PTMAP_CLASSES], bool lanes4) {
  const int nQ = lanes4 ? n[0] : 0, nS = lanes4 ? n[1] : n[0] + n[1];
  return PtMap{nQ, nS, n[2], n[3], (nQ + 63) / 64, (nS + 31) / 32, (n[2] + 15) / 16};
}
inline int ptmap_n_wg(const PtMap& m) { const int n = m.wQ + m.wS + m.wL + (m.nX + 31) / 32; return n > 0 ? n : 1; }   // (an empty launch is not one)
