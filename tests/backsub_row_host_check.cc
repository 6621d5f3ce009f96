// Host check of the back substitution's row function (msfm_backsub_row, metricsfm_amd/csrc/ba_device.h): per random row three
// evaluations of q = -(Jc z_c + Jm z_m) and of the scaled point block jp -
//   new     msfm_backsub_row: one forward-mode tangent along d = -(scale * z), the point block contracted without forming R;
//   parent  linearize_core: the full scaled 2 x 12 Jacobian from msfm_reproj, contracted with z as k_backsub used to;
//   ref     the parent's formulas in long double on the same double inputs (rotation cache and Huber factor included: both double
//           forms are the same polynomial in pose, cache, intrinsics, point, scales, factor and step, so what differs is rounding alone)
// - over classes of inputs: generic angles, |a| from 1e-8 to 1e-3, |a| below the branch threshold, a exactly zero, frozen camera,
// frozen intrinsics, both, Huber active, points near the optical axis and far off it.  Errors of q are normalised by
// sum_j |J_j| |d_j|, those of jp[k][j] by sq sp_j weight sum_i |R_ij| |g_ki| (what a backward-stable contraction is allowed).
// Criterion per class: the new form's worst error is at most 4 x the parent form's worst error on the same inputs; r0 and r1
// are bit-equal to linearize_core's.  A stand-alone program, host only, never loaded into another process: it can be built with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "ba_device.h"

typedef long double ld;

// msfm_reproj's Jacobian mode in long double: residual, J (2 x 12, times weight), and for the normalisers R and the gradients
// g_k of the residual components by the camera-frame point (without weight).
static void reproj_ld(const double* pose, const double* rc, const double* cam, const double* xyz, double ox, double oy, double weight,
                      ld* r, ld* J, ld* R, ld* up, ld* vp) {
  const ld a0 = pose[0], a1 = pose[1], a2 = pose[2], X0 = xyz[0], X1 = xyz[1], X2 = xyz[2];
  ld p0, p1, p2, dpdw[9];
  if (rc[0] != 0.0) {
    const ld s = rc[1], c = rc[2], ti = rc[3];
    const ld w[3] = {a0 * ti, a1 * ti, a2 * ti}, Xv[3] = {X0, X1, X2};
    const ld wx[3] = {w[1] * X2 - w[2] * X1, w[2] * X0 - w[0] * X2, w[0] * X1 - w[1] * X0};
    const ld wdx = w[0] * X0 + w[1] * X1 + w[2] * X2, omc = 1.0L - c, tmp = wdx * omc;
    p0 = X0 * c + wx[0] * s + w[0] * tmp; p1 = X1 * c + wx[1] * s + w[1] * tmp; p2 = X2 * c + wx[2] * s + w[2] * tmp;
    for (int j = 0; j < 3; j++) {
      ld dw[3];
      for (int i = 0; i < 3; i++) dw[i] = ((i == j ? 1.0L : 0.0L) - w[i] * w[j]) * ti;
      const ld dwx[3] = {dw[1] * X2 - dw[2] * X1, dw[2] * X0 - dw[0] * X2, dw[0] * X1 - dw[1] * X0};
      const ld dwdx = dw[0] * X0 + dw[1] * X1 + dw[2] * X2, dc = -s * w[j], ds = c * w[j], dtmp = dwdx * omc - wdx * dc;
      for (int i = 0; i < 3; i++) dpdw[i * 3 + j] = Xv[i] * dc + dwx[i] * s + wx[i] * ds + dw[i] * tmp + w[i] * dtmp;
    }
    R[0] = c + w[0] * w[0] * omc;         R[1] = w[0] * w[1] * omc - w[2] * s;  R[2] = w[1] * s + w[0] * w[2] * omc;
    R[3] = w[2] * s + w[0] * w[1] * omc;  R[4] = c + w[1] * w[1] * omc;         R[5] = -w[0] * s + w[1] * w[2] * omc;
    R[6] = -w[1] * s + w[0] * w[2] * omc; R[7] = w[0] * s + w[1] * w[2] * omc;  R[8] = c + w[2] * w[2] * omc;
  } else {
    p0 = X0 + (a1 * X2 - a2 * X1); p1 = X1 + (a2 * X0 - a0 * X2); p2 = X2 + (a0 * X1 - a1 * X0);
    const ld d[9] = {0, X2, -X1, -X2, 0, X0, X1, -X0, 0}, Rr[9] = {1, -a2, a1, a2, 1, -a0, -a1, a0, 1};
    for (int k = 0; k < 9; k++) { dpdw[k] = d[k]; R[k] = Rr[k]; }
  }
  p0 += pose[3]; p1 += pose[4]; p2 += pose[5];
  const ld iz = 1.0L / p2, xp = p0 * iz, yp = p1 * iz;
  const ld f = cam[0], l1 = cam[1], l2 = cam[2], r2 = xp * xp + yp * yp, dist = 1.0L + r2 * (l1 + l2 * r2);
  r[0] = weight * (f * dist * xp - ox);
  r[1] = weight * (f * dist * yp - oy);
  const ld dd = l1 + 2.0L * l2 * r2;
  const ld uxp = f * (dist + 2.0L * xp * xp * dd), uyp = f * 2.0L * xp * yp * dd, vyp = f * (dist + 2.0L * yp * yp * dd);
  up[0] = uxp * iz; up[1] = uyp * iz; up[2] = -(uxp * xp + uyp * yp) * iz;
  vp[0] = uyp * iz; vp[1] = vyp * iz; vp[2] = -(uyp * xp + vyp * yp) * iz;
  for (int j = 0; j < 3; j++) {
    J[j] = weight * (up[0] * dpdw[j] + up[1] * dpdw[3 + j] + up[2] * dpdw[6 + j]);
    J[12 + j] = weight * (vp[0] * dpdw[j] + vp[1] * dpdw[3 + j] + vp[2] * dpdw[6 + j]);
    J[3 + j] = weight * up[j];
    J[15 + j] = weight * vp[j];
    J[9 + j] = weight * (up[0] * R[j] + up[1] * R[3 + j] + up[2] * R[6 + j]);
    J[21 + j] = weight * (vp[0] * R[j] + vp[1] * R[3 + j] + vp[2] * R[6 + j]);
  }
  J[6] = weight * dist * xp;        J[18] = weight * dist * yp;
  J[7] = weight * f * r2 * xp;      J[19] = weight * f * r2 * yp;
  J[8] = weight * f * r2 * r2 * xp; J[20] = weight * f * r2 * r2 * yp;
}

enum { GENERIC, SMALL, BELOW, ZERO, FROZEN_CAM, FROZEN_MODEL, FROZEN_BOTH, HUBER, NEAR_AXIS, FAR_OFF, N_CLASS };
static const char* kName[N_CLASS] = {"generic angles", "|a| 1e-8 .. 1e-3", "|a| below the threshold", "a exactly zero", "frozen camera",
                                     "frozen intrinsics", "camera and intrinsics frozen", "Huber active", "near the optical axis", "far off the axis"};

struct Row { double pose[6], rc[4], cm[3], X[3], ox, oy, w, sc[6], sm[3], sp[3], zc[6], zm[3]; };

static std::mt19937_64 rng(20250117);
static double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
static double gauss() { return std::normal_distribution<double>(0.0, 1.0)(rng); }
static double logu(double a, double b) { return std::pow(10.0, uni(std::log10(a), std::log10(b))); }

static Row make_row(int cls) {
  Row r;
  double dir[3] = {gauss(), gauss(), gauss()};
  const double n = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
  double theta = uni(0.05, 3.0);
  if (cls == SMALL) theta = logu(1e-8, 1e-3);
  if (cls == BELOW) theta = logu(1e-13, 1.4e-8);
  if (cls == ZERO) theta = 0.0;
  for (int j = 0; j < 3; j++) r.pose[j] = theta == 0.0 ? 0.0 : dir[j] / n * theta;
  msfm_rot_prepare(r.pose, r.rc);
  for (int j = 0; j < 3; j++) r.X[j] = uni(-20.0, 20.0);
  // the camera-frame point wanted, and the translation that puts the rotated point there
  const double z = uni(5.0, 60.0);
  double off = uni(0.02, 0.6);
  if (cls == NEAR_AXIS) off = logu(1e-9, 1e-5);
  if (cls == FAR_OFF) off = uni(1.5, 3.0);
  const double phi = uni(0.0, 6.283185307179586);
  const double pc[3] = {z * off * std::cos(phi), z * off * std::sin(phi), z};
  r.cm[0] = uni(500.0, 3000.0); r.cm[1] = uni(-0.1, 0.1) * (cls == FAR_OFF ? 0.1 : 1.0); r.cm[2] = uni(-0.01, 0.01) * (cls == FAR_OFF ? 0.1 : 1.0);
  r.w = uni(0.5, 2.0);
  double rr[2], RX[3];
  {
    // p = R X by Rodrigues in double - only a plausible scene is needed
    const double a[3] = {r.pose[0], r.pose[1], r.pose[2]}, th = theta;
    const double cx[3] = {a[1] * r.X[2] - a[2] * r.X[1], a[2] * r.X[0] - a[0] * r.X[2], a[0] * r.X[1] - a[1] * r.X[0]};
    if (th > 1.5e-8) {
      const double s = std::sin(th), c = std::cos(th), k = (a[0] * r.X[0] + a[1] * r.X[1] + a[2] * r.X[2]) / (th * th) * (1.0 - c);
      for (int j = 0; j < 3; j++) RX[j] = c * r.X[j] + s / th * cx[j] + k * a[j];
    } else for (int j = 0; j < 3; j++) RX[j] = r.X[j] + cx[j];
  }
  for (int j = 0; j < 3; j++) r.pose[3 + j] = pc[j] - RX[j];
  // the observation: the projection (the residual against (0, 0) at weight 1) plus noise
  msfm_reproj(r.pose, r.rc, r.cm, r.X, 0.0, 0.0, 1.0, rr, nullptr);
  const double noise = cls == HUBER ? 40.0 : 0.25;   // Huber(1): |weight * noise| well above / mostly below 1
  r.ox = rr[0] + noise * gauss(); r.oy = rr[1] + noise * gauss();
  if (cls == HUBER) r.ox += 30.0;
  for (int j = 0; j < 6; j++) { r.sc[j] = logu(1e-4, 1.0); r.zc[j] = gauss() * logu(1e-3, 1e2); }
  for (int j = 0; j < 3; j++) { r.sm[j] = logu(1e-4, 1.0); r.zm[j] = gauss() * logu(1e-3, 1e2); r.sp[j] = logu(1e-3, 1.0); }
  if (cls == FROZEN_CAM || cls == FROZEN_BOTH) for (int j = 0; j < 6; j++) r.sc[j] = 0.0;
  if (cls == FROZEN_MODEL || cls == FROZEN_BOTH) for (int j = 0; j < 3; j++) r.sm[j] = 0.0;
  return r;
}

int main() {
  const int kRows = 500;
  const double huber = 1.0;
  int fails = 0, n_active[N_CLASS] = {0}, n_first_order[N_CLASS] = {0};
  double wq_new[N_CLASS] = {0}, wq_par[N_CLASS] = {0}, wj_new[N_CLASS] = {0}, wj_par[N_CLASS] = {0};
  for (int cls = 0; cls < N_CLASS; cls++)
    for (int it = 0; it < kRows; it++) {
      const Row r = make_row(cls);
      // parent
      double pr0, pr1, jc[12], jm[6], pjp[6];
      linearize_core(r.pose, r.rc, r.cm, r.X, r.ox, r.oy, r.w, r.sc, r.sm, r.sp, huber, pr0, pr1, jc, jm, pjp);
      double pq[2] = {0.0, 0.0};
      for (int j = 0; j < 6; j++) { pq[0] -= jc[j] * r.zc[j]; pq[1] -= jc[6 + j] * r.zc[j]; }
      for (int j = 0; j < 3; j++) { pq[0] -= jm[j] * r.zm[j]; pq[1] -= jm[3 + j] * r.zm[j]; }
      // new
      double nr0, nr1, njp[6], nq[2];
      msfm_backsub_row(r.pose, r.rc, r.cm, r.X, r.ox, r.oy, r.w, r.sc, r.sm, r.sp, r.zc, r.zm, huber, nr0, nr1, njp, nq[0], nq[1]);
      if (std::memcmp(&nr0, &pr0, 8) != 0 || std::memcmp(&nr1, &pr1, 8) != 0) {
        if (fails++ < 10) std::printf("FAIL class '%s' row %d: residual (%.17g, %.17g), linearize_core (%.17g, %.17g)\n", kName[cls], it, nr0, nr1, pr0, pr1);
      }
      // reference
      ld rr[2], J[24], R[9], g[2][3];
      reproj_ld(r.pose, r.rc, r.cm, r.X, r.ox, r.oy, r.w, rr, J, R, g[0], g[1]);
      const ld s2 = rr[0] * rr[0] + rr[1] * rr[1], b = (ld)huber * huber;
      // (the Huber factor is an input both double forms share - their residuals are the same bits - like the rotation cache: the
      //  reference takes the double one, or the cancellation in the residual, 1e-13 of sq, would be all that this check measures)
      double rd[2], Jd[24], rho0d, rho1d;
      msfm_reproj(r.pose, r.rc, r.cm, r.X, r.ox, r.oy, r.w, rd, Jd);
      msfm_huber(huber, rd[0] * rd[0] + rd[1] * rd[1], rho0d, rho1d);
      const ld sq = std::sqrt(rho1d);
      n_active[cls] += s2 > b;
      n_first_order[cls] += r.rc[0] == 0.0;
      ld d[9];
      for (int j = 0; j < 6; j++) d[j] = -((ld)r.sc[j] * r.zc[j]);
      for (int j = 0; j < 3; j++) d[6 + j] = -((ld)r.sm[j] * r.zm[j]);
      for (int k = 0; k < 2; k++) {
        ld q = 0, nrm = 0;
        for (int j = 0; j < 9; j++) { q += sq * J[12 * k + j] * d[j]; nrm += fabsl(sq * J[12 * k + j]) * fabsl(d[j]); }
        if (nrm == 0) {   // nothing free in this row: both forms must say exactly zero
          if (nq[k] != 0.0 || pq[k] != 0.0) { if (fails++ < 10) std::printf("FAIL class '%s' row %d: q of a frozen row %g (parent %g)\n", kName[cls], it, nq[k], pq[k]); }
        } else {
          wq_new[cls] = std::fmax(wq_new[cls], (double)(fabsl(nq[k] - q) / nrm));
          wq_par[cls] = std::fmax(wq_par[cls], (double)(fabsl(pq[k] - q) / nrm));
        }
        for (int j = 0; j < 3; j++) {
          const ld ref = sq * r.sp[j] * J[12 * k + 9 + j];
          const ld nj = sq * r.sp[j] * r.w * (fabsl(R[j]) * fabsl(g[k][0]) + fabsl(R[3 + j]) * fabsl(g[k][1]) + fabsl(R[6 + j]) * fabsl(g[k][2]));
          wj_new[cls] = std::fmax(wj_new[cls], (double)(fabsl(njp[3 * k + j] - ref) / nj));
          wj_par[cls] = std::fmax(wj_par[cls], (double)(fabsl(pjp[3 * k + j] - ref) / nj));
        }
      }
    }
  std::printf("%-30s %5s %6s %6s | %-10s %-10s %6s | %-10s %-10s %6s\n", "class", "rows", "huber", "1st-o", "q new", "q parent", "ratio", "jp new", "jp parent", "ratio");
  for (int cls = 0; cls < N_CLASS; cls++) {
    std::printf("%-30s %5d %6d %6d | %.3e  %.3e %6.2f | %.3e  %.3e %6.2f\n", kName[cls], kRows, n_active[cls], n_first_order[cls], wq_new[cls], wq_par[cls],
                wq_par[cls] > 0 ? wq_new[cls] / wq_par[cls] : 0.0, wj_new[cls], wj_par[cls], wj_par[cls] > 0 ? wj_new[cls] / wj_par[cls] : 0.0);
    if (!(wq_new[cls] <= 4.0 * wq_par[cls])) { fails++; std::printf("FAIL class '%s': q, new %.3e > 4 x parent %.3e\n", kName[cls], wq_new[cls], wq_par[cls]); }
    if (!(wj_new[cls] <= 4.0 * wj_par[cls])) { fails++; std::printf("FAIL class '%s': jp, new %.3e > 4 x parent %.3e\n", kName[cls], wj_new[cls], wj_par[cls]); }
  }
  // the classes are what they say
  if (n_active[HUBER] != kRows || n_active[GENERIC] > kRows / 2) { fails++; std::printf("FAIL Huber classes: %d active of the active class, %d of the generic one\n", n_active[HUBER], n_active[GENERIC]); }
  if (n_first_order[BELOW] != kRows || n_first_order[ZERO] != kRows || n_first_order[GENERIC] != 0) { fails++; std::printf("FAIL branch classes\n"); }
  if (fails) { std::printf("backsub_row_host_check: %d failures\n", fails); return 1; }
  std::printf("backsub_row_host_check ok: %d rows\n", N_CLASS * kRows);
  return 0;
}
