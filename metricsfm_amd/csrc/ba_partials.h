// Where the kernels of an LM iteration put their per-workgroup partial sums, and what k_reduce sums of them: the one place
// that knows the layout of msfm_ba's partial_x, partial, partial2 / partial3, partial4 and gmax_buf (ba.hip; the table is in
// DESIGN.md).  Plain C++ without HIP: tests/ba_partials_host_check.cc walks ba_partials() on the CPU.
//
//   partial_x            cost at x             [ k_point: nblk_pt | rows of frozen points: cdiv(A - AE, 256) | GPS rows: cdiv(ncb, 256) ]
//   partial2 / partial3  |dx|^2 / |x|^2        [ camera + intrinsics step: cdiv(nred, 256) | k_backsub: nblk_pt ]
//   partial              model cost change     [ k_backsub: nblk_pt | k_tail, frozen + GPS rows: cdiv(A - AE + ncb, 256) ]
//   partial4             cost at the candidate [ k_tail, all rows: cdiv(max(1, A), 256) | GPS rows: cdiv(ncb, 256) ]
//   gmax_buf             gradient max norm     [ k_point: nblk_pt | per camera scalar: 6 ncb | per intrinsics scalar: 3 nmb ]
//
// A segment whose kernel does not run is empty: the GPS segments without GPS, the step's without a reduced system, k_backsub's
// without an eliminated point (k_point still runs its one workgroup then).  Every rank writes the GPS rows' partials, but only
// the lead rank (rank 0) counts them - they lie last in their buffers, so another rank's reductions stop short of them - and
// only the lead's k_tail takes the GPS rows into the model cost change.  Indices [2] below: 0 another rank, 1 the lead.
#pragma once

struct BaSeg { int off, n; };   // entries [off, off + n) of a buffer

struct BaPartials {
  BaSeg x_point, x_frozen, x_gps;      // partial_x
  BaSeg u_step, u_point;               // partial2 and partial3
  BaSeg m_point, m_rest[2];            // partial
  BaSeg c_rows, c_gps;                 // partial4
  BaSeg g_point, g_cam, g_model;       // gmax_buf
  int need_x, need_u, need_m, need_c, need_g;   // entries each buffer needs (on any rank)
  int sum_x[2], sum_u, sum_m[2], sum_c[2], sum_g;   // entries from the buffer's start that the rank's k_reduce job takes
};

inline BaPartials ba_partials(int A, int AE, int ncb, int nmb, int nred, int npb, int nblk_pt, bool has_gps) {
  auto blocks = [](long n) { return (int)((n + 255) / 256); };
  auto behind = [](const BaSeg& s, int n) { return BaSeg{s.off + s.n, n}; };
  const int nbp = npb > 0 ? nblk_pt : 0, n_gps = has_gps ? blocks(ncb) : 0;
  BaPartials L;
  L.x_point = BaSeg{0, nblk_pt};
  L.x_frozen = behind(L.x_point, blocks((long)A - AE));
  L.x_gps = behind(L.x_frozen, n_gps);
  L.u_step = BaSeg{0, nred > 0 ? blocks(nred) : 0};
  L.u_point = behind(L.u_step, nbp);
  L.m_point = BaSeg{0, nbp};
  for (int lead = 0; lead < 2; lead++) L.m_rest[lead] = behind(L.m_point, blocks((long)A - AE + ((has_gps && lead) ? ncb : 0)));
  L.c_rows = BaSeg{0, blocks(A > 1 ? A : 1)};
  L.c_gps = behind(L.c_rows, n_gps);
  L.g_point = BaSeg{0, nblk_pt};
  L.g_cam = behind(L.g_point, 6 * ncb);
  L.g_model = behind(L.g_cam, 3 * nmb);
  for (int lead = 0; lead < 2; lead++) {
    L.sum_x[lead] = lead ? L.x_gps.off + L.x_gps.n : L.x_gps.off;
    L.sum_m[lead] = L.m_rest[lead].off + L.m_rest[lead].n;
    L.sum_c[lead] = lead ? L.c_gps.off + L.c_gps.n : L.c_gps.off;
  }
  L.sum_u = L.u_point.off + L.u_point.n;
  L.sum_g = L.g_model.off + L.g_model.n;
  L.need_x = L.sum_x[1]; L.need_u = L.sum_u; L.need_m = L.sum_m[1]; L.need_c = L.sum_c[1]; L.need_g = L.sum_g;
  return L;
}
