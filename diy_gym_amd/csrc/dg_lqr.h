// dg_lqr.h -- the Riccati / iLQR backward pass of a joint-space model, every env in ONE launch (dg_world_lq_backward).
//
// Per env, with n joints, m = 2 n states [dq; qd], T steps and the CONTINUOUS derivatives A_q = dqdd/dq, A_v = dqdd/dqd, Minv = dqdd/dtau
// of dg_world_dynamics_derivatives at P points (P == T, or P == 1: the one point at every t):
//   A_h = [[I + dt^2 A_q, dt (I + dt A_v)], [dt A_q, I + dt A_v]],  B_h = [[dt^2 Minv], [dt Minv]],  A = A_h^s,  B = sum_{k<s} A_h^k B_h
// formed HERE in fp64 (an fp32 I + dt^2 A_q would lose A_q to the identity), then from Vx = lx_T, Vxx = lxx_T for t = T-1 .. 0
//   Qx = lx + A^T Vx;  Qu = lu + B^T Vx;  Qxx = lxx + A^T Vxx A;  Qux = B^T Vxx A;  Quu = luu + B^T Vxx B
//   k = -(Quu + mu I)^-1 Qu;  K = -(Quu + mu I)^-1 Qux            Cholesky; a pivot <= 0 or not finite is a failure
//   dV += (k . Qu, 0.5 k^T Quu k)
//   Vx = Qx + K^T Quu k + K^T Qu + Qux^T k;  Vxx = sym(Qxx + K^T Quu K + K^T Qux + Qux^T K)      the unregularised Quu
// The running cost has its own point count PC (1 or T).  Everything is computed in fp64 and read and written as fp32: the recursion
// squares the conditioning of B, and M^-1 of an arm spans four decades.
//
// Form: one env per 64-lane workgroup, every matrix a row-major array of doubles in LDS (lq_lds_doubles(n): 28 n^2 + 9 n, 33,120 B at
// n = 12, 8,496 B at n = 6), the lanes striding over the entries of each product with a barrier between dependent products.  The
// n x n factorisation goes column by column: every lane forms the pivot (wave-uniform, so failure is a uniform branch) and lane i
// the entry below it; the n x (m + 1) solves run one right-hand side per lane.  The discretisation borrows the arrays of the
// products that come after it (A_h in Qxx, B_h in Qux, the power's next factor in VA, VB).  An env also fails at the step whose K, k
// or dV fp32 cannot hold (a NaN or Inf of an input that never met a pivot: Quu is made of B and Vxx alone).  A failed env writes zeros to all its
// rows of K_out, k_out and dV and t + 1 to status; nothing is left unwritten.  No scene, no workspace: a plain kernel for every mode.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dg {

constexpr int LQ_MAX_JOINTS = 12;
constexpr double LQ_FLT_MAX = 3.4028234663852886e38;  // what the fp32 outputs can hold
constexpr int lq_lds_doubles(int n) { return 28 * n * n + 9 * n; }

// C [M x N] = X' Y over the lanes, X' = X^T when TA (X [Kd x M]) else X [M x Kd]; Y [Kd x N]; row-major, dense
template <bool TA>
__device__ inline void lq_mm(double* C, const double* X, const double* Y, int M, int N, int Kd, int lane) {
  for (int idx = lane; idx < M * N; idx += 64) {
    const int i = idx / N, j = idx - i * N;
    double s = 0.0;
    for (int k = 0; k < Kd; k++) s += (TA ? X[k * M + i] : X[i * Kd + k]) * Y[k * N + j];
    C[idx] = s;
  }
}

struct LqArgs {
  int n, T, P, PC, substeps;
  double dt;
  const float *A_q, *A_v, *Minv, *lxx, *luu, *lx, *lu, *lxx_T, *lx_T, *mu;
  float *K_out, *k_out, *dV;
  int32_t* status;
};

__global__ __launch_bounds__(64) void lq_backward_kernel(LqArgs a) {
  extern __shared__ double lq_s[];
  const int e = blockIdx.x, lane = threadIdx.x, n = a.n, m = 2 * n, mm = m * m, mn = m * n, nn = n * n, T = a.T;
  double* const A = lq_s; double* const Bm = A + mm; double* const Vxx = Bm + mn; double* const VA = Vxx + mm; double* const VB = VA + mm;
  double* const Qxx = VB + mn; double* const Qux = Qxx + mm; double* const Quu = Qux + mn; double* const Lc = Quu + nn;
  double* const Kg = Lc + nn; double* const QK = Kg + mn; double* const Vx = QK + mn; double* const Qx = Vx + m; double* const Vt = Qx + m;
  double* const Qu = Vt + m; double* const kv = Qu + n; double* const Qk = kv + n;
  const double dt = a.dt, muv = a.mu ? (double)a.mu[e] : 0.0;

  // A, Bm of point p (an index into [B][P]); leaves with a barrier behind it
  auto discretise = [&](size_t p) {
    const float* aq = a.A_q + p * (size_t)nn; const float* av = a.A_v + p * (size_t)nn; const float* mi = a.Minv + p * (size_t)nn;
    double* const Ah = Qxx; double* const Bh = Qux;
    for (int idx = lane; idx < mm; idx += 64) {
      const int i = idx / m, j = idx - i * m, bi = i >= n, bj = j >= n, ii = i - bi * n, jj = j - bj * n;
      const double id = ii == jj ? 1.0 : 0.0, q = (double)aq[ii * n + jj], v = id + dt * (double)av[ii * n + jj];
      const double val = bi ? (bj ? v : dt * q) : (bj ? dt * v : id + dt * dt * q);
      Ah[idx] = val; A[idx] = val;
    }
    for (int idx = lane; idx < mn; idx += 64) {
      const int i = idx / n, j = idx - i * n, bi = i >= n;
      const double v = (double)mi[(i - bi * n) * n + j], val = bi ? dt * v : dt * dt * v;
      Bh[idx] = val; Bm[idx] = val;
    }
    __syncthreads();
    for (int s = 1; s < a.substeps; s++) {  // Bm += A Bh; A = A Ah
      lq_mm<false>(VB, A, Bh, m, n, m, lane);
      lq_mm<false>(VA, A, Ah, m, m, m, lane);
      __syncthreads();
      for (int idx = lane; idx < mn; idx += 64) Bm[idx] += VB[idx];
      for (int idx = lane; idx < mm; idx += 64) A[idx] = VA[idx];
      __syncthreads();
    }
  };

  for (int idx = lane; idx < mm; idx += 64) Vxx[idx] = (double)a.lxx_T[(size_t)e * mm + idx];
  for (int idx = lane; idx < m; idx += 64) Vx[idx] = a.lx_T ? (double)a.lx_T[(size_t)e * m + idx] : 0.0;
  __syncthreads();
  if (a.P == 1) discretise((size_t)e);

  double dv0 = 0.0, dv1 = 0.0;
  int failed = 0;
  for (int t = T - 1; t >= 0; t--) {
    if (a.P != 1) discretise((size_t)e * (size_t)T + (size_t)t);
    const size_t pc = a.PC == 1 ? (size_t)e : (size_t)e * (size_t)T + (size_t)t;
    lq_mm<false>(VA, Vxx, A, m, m, m, lane);
    lq_mm<false>(VB, Vxx, Bm, m, n, m, lane);
    __syncthreads();
    lq_mm<true>(Qxx, A, VA, m, m, m, lane);
    for (int idx = lane; idx < mm; idx += 64) Qxx[idx] += (double)a.lxx[pc * (size_t)mm + idx];
    lq_mm<true>(Qux, Bm, VA, n, m, m, lane);
    lq_mm<true>(Quu, Bm, VB, n, n, m, lane);
    for (int idx = lane; idx < nn; idx += 64) Quu[idx] += (double)a.luu[pc * (size_t)nn + idx];
    lq_mm<true>(Qx, A, Vx, m, 1, m, lane);
    for (int idx = lane; idx < m; idx += 64) Qx[idx] += a.lx ? (double)a.lx[pc * (size_t)m + idx] : 0.0;
    lq_mm<true>(Qu, Bm, Vx, n, 1, m, lane);
    for (int idx = lane; idx < n; idx += 64) Qu[idx] += a.lu ? (double)a.lu[pc * (size_t)n + idx] : 0.0;
    __syncthreads();
    // ---- Quu + mu I = Lc Lc^T, the lower triangle, a column per round
    for (int j = 0; j < n; j++) {
      double d = Quu[j * n + j] + muv;
      for (int k = 0; k < j; k++) d -= Lc[j * n + k] * Lc[j * n + k];
      if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) { failed = t + 1; break; }  // the same d on every lane
      const double r = sqrt(d);
      if (lane >= j && lane < n) {
        double s = Quu[lane * n + j];
        for (int k = 0; k < j; k++) s -= Lc[lane * n + k] * Lc[j * n + k];
        Lc[lane * n + j] = lane == j ? r : s / r;
      }
      __syncthreads();
    }
    if (failed) break;
    // ---- [K | k] = -(Lc Lc^T)^-1 [Qux | Qu], a right-hand side per lane
    int bad = 0;
    if (lane <= m) {
      const bool isk = lane == m; const int st = isk ? 1 : m;
      const double* src = isk ? Qu : Qux + lane; double* dst = isk ? kv : Kg + lane;
      for (int i = 0; i < n; i++) {
        double s = src[i * st];
        for (int k = 0; k < i; k++) s -= Lc[i * n + k] * dst[k * st];
        dst[i * st] = s / Lc[i * n + i];
      }
      for (int i = n - 1; i >= 0; i--) {
        double s = dst[i * st];
        for (int k = i + 1; k < n; k++) s -= Lc[k * n + i] * dst[k * st];
        dst[i * st] = s / Lc[i * n + i];
      }
      for (int i = 0; i < n; i++) { const double v = -dst[i * st]; dst[i * st] = v; if (!(fabs(v) <= LQ_FLT_MAX)) bad = 1; }
    }
    if (__syncthreads_or(bad)) { failed = t + 1; break; }  // a gain that fp32 cannot hold (a NaN or Inf that never met a pivot): the env fails
    lq_mm<false>(QK, Quu, Kg, n, m, n, lane);
    lq_mm<false>(Qk, Quu, kv, n, 1, n, lane);
    if (a.K_out) { float* o = a.K_out + ((size_t)e * (size_t)T + (size_t)t) * (size_t)mn; for (int idx = lane; idx < mn; idx += 64) o[idx] = (float)Kg[idx]; }
    if (a.k_out) { float* o = a.k_out + ((size_t)e * (size_t)T + (size_t)t) * (size_t)n; for (int idx = lane; idx < n; idx += 64) o[idx] = (float)kv[idx]; }
    __syncthreads();
    for (int i = 0; i < n; i++) { dv0 += kv[i] * Qu[i]; dv1 += 0.5 * kv[i] * Qk[i]; }
    if (!(fabs(dv0) <= LQ_FLT_MAX) || !(fabs(dv1) <= LQ_FLT_MAX)) { failed = t + 1; break; }  // the same sums on every lane
    // ---- the value function of step t: the sum into VA, Vt, then symmetrised into Vxx
    for (int idx = lane; idx < mm; idx += 64) {
      const int i = idx / m, j = idx - i * m;
      double s = Qxx[idx];
      for (int c = 0; c < n; c++) s += Kg[c * m + i] * (QK[c * m + j] + Qux[c * m + j]) + Qux[c * m + i] * Kg[c * m + j];
      VA[idx] = s;
    }
    for (int i = lane; i < m; i += 64) {
      double s = Qx[i];
      for (int c = 0; c < n; c++) s += Kg[c * m + i] * (Qk[c] + Qu[c]) + Qux[c * m + i] * kv[c];
      Vt[i] = s;
    }
    __syncthreads();
    for (int idx = lane; idx < mm; idx += 64) { const int i = idx / m, j = idx - i * m; Vxx[idx] = 0.5 * (VA[idx] + VA[j * m + i]); }
    for (int i = lane; i < m; i += 64) Vx[i] = Vt[i];
    __syncthreads();
  }
  if (failed) {  // every row of this env, those of the later steps already written included
    if (a.K_out) { float* o = a.K_out + (size_t)e * (size_t)T * (size_t)mn; for (size_t idx = lane; idx < (size_t)T * (size_t)mn; idx += 64) o[idx] = 0.f; }
    if (a.k_out) { float* o = a.k_out + (size_t)e * (size_t)T * (size_t)n; for (size_t idx = lane; idx < (size_t)T * (size_t)n; idx += 64) o[idx] = 0.f; }
    dv0 = 0.0; dv1 = 0.0;
  }
  if (lane == 0) {
    if (a.dV) { a.dV[(size_t)e * 2] = (float)dv0; a.dV[(size_t)e * 2 + 1] = (float)dv1; }
    a.status[e] = failed;
  }
}

}  // namespace dg
