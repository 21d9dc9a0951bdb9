// IMU state propagation of the OKVIS frontend on the device (include/okvis_amd_frontend.h: okvis_fe_imu_propagate): what
// ImuError::propagation (okvis_ceres/src/ImuError.cpp:287-504) computes for one call — the propagated pose and speed, and on request
// the 15x15 covariance and the Jacobian of the propagated state — for the chains of calls of many sequences in one launch.
//
// Restated from the reference, statement by statement:
//   prop_step       one pass of the integration loop (:327-468): orientation, the rotation-matrix integrals, the bias Jacobian
//                   parts, the blocks of F_delta and the noise terms.  Written out with the reference's quirks: dalpha_db_g without
//                   the right Jacobian (:412), sigma2_v = dt * sigma_a_c(local) * imuParams.sigma_a_c (:438; a saturated
//                   accelerometer counts 100 times where a saturated gyroscope counts 10^4 times), F_delta(0,12) from the integrals
//                   BEFORE the memory shift (:426), as every other block.
//   prop_apply      y = (I + N) x for the block-sparse F_delta (:421-431); terms in ascending column order, as a dense product has
//                   them, the structural zeros left out (they add exact zeros)
//   prop_finish     the propagated state (:470-477) and the blocks of the Jacobian F (:480-491)
//   prop_rotate     y = T x, T = blockdiag(C_WS_0, C_WS_0, C_WS_0, I, I) (:494-502)
// Every product and sum is rounded on its own and in the reference's order (BA_NO_CONTRACT, like ba_math.hpp's qmul_strict): a
// one-step call at IMU rate is judged at a few units in the last place, and the state goes through differences of nearly equal
// numbers (Phi - sin(Phi), 1 - cos(Phi), -C_integral dt + 0.25 (C + C_1) dt^2).
//
// imu_propagate_kernel: ONE WAVE PER JOB (a job = one sequence's chain of calls); a workgroup is PROP_WAVES independent waves and
// the kernel has no workgroup barrier at all: neighbouring jobs differ in length by two orders of magnitude.  The wave walks its
// ends and its integration steps in order.  The state algebra (quaternions, 3x3 blocks) is computed by every lane alike, so nothing
// of it is exchanged; the running values of a call (about 70 doubles) and the blocks of F_delta (68) are kept ONCE per wave in its
// LDS, stored by lane 0 and read by all lanes as broadcasts (in every lane's registers they cost 540 bytes of scratch per lane).
// The samples come through a wave-private LDS window of 64, filled with one coalesced read.
// The covariance is spread over lanes 0..14: lane j holds column j, applies F_delta to it (F P), the wave transposes through its
// private LDS slab, lane i applies F_delta to row i ((F P) F^T, the reference's association) and adds the noise to its diagonal
// entry.  The final T P T^T and the columns of the Jacobian go the same way.  A job that wants no covariance never enters that code.
// The leading samples that the reference skips one by one (`continue` while dt <= 0; the IMU-rate caller passes its WHOLE deque,
// :559-598 of ThreadedKFVio.cpp) are found by a ballot over 64 samples at a time: the same first step as the serial scan.
//
// The step functions are BA_HD like ba_math.hpp's: a plain host compiler sees them too; the kernel is for hipcc only.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/okvis_amd_frontend.h"
#include "ba_math.hpp"

namespace fe {

constexpr int PROP_WAVES = 4;                  // jobs per workgroup, one per wave
constexpr int PROP_THREADS = 64 * PROP_WAVES;
constexpr int PROP_WINDOW = 64;                // samples in a wave's LDS window
constexpr int PROP_LD = 17;                    // row stride of the 15x15 transposition slab (odd: rows and columns both conflict-free)

// running values of one call (ImuError.cpp:306-325)
struct PropState {
  double Dq[4];                       // Delta_q (x,y,z,w)
  double Cint[9], Cdbl[9];            // C_integral, C_doubleintegral
  double aint[3], adbl[3];            // acc_integral, acc_doubleintegral
  double cross[9], dal[9], dv[9], dp[9];
  double Dt;                          // Delta_t
};
// F_delta = I + N of one step (:421-431) or F of the call (:480-491): the 3x3 blocks of N, row-major, and the noise of the step
struct PropF {
  double A03[9], A09[9], A012[9], A39[9], A63[9], A69[9], A612[9];
  double dt;                          // block (0,6) = dt I
  double q_p, q_al, q_v, q_bg, q_ba;  // sigma2_p, sigma2_dalpha, sigma2_v, sigma2_b_g, sigma2_b_a
};

// okvis::Duration::toSec() (ba::ns_to_sec), the product and the sum rounded one by one
BA_HD double prop_sec(long long ns) {
  BA_NO_CONTRACT
  long long sec = ns / 1000000000LL;
  long long nsec = ns % 1000000000LL;
  if (nsec < 0) {
    nsec += 1000000000LL;
    --sec;
  }
  const double frac = 1e-9 * (double)nsec;
  return (double)sec + frac;
}
BA_HD void prop_m3mul(const double* A, const double* B, double* C) {
  BA_NO_CONTRACT
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
BA_HD void prop_m3vec(const double* A, const double* v, double* r) {
  BA_NO_CONTRACT
  for (int i = 0; i < 3; ++i) r[i] = (A[3 * i] * v[0] + A[3 * i + 1] * v[1]) + A[3 * i + 2] * v[2];
}
BA_HD void prop_qrot(const double* q, double* R) {  // ba::qrot
  BA_NO_CONTRACT
  const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}
BA_HD double prop_norm3(const double* v) {
  BA_NO_CONTRACT
  return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}
BA_HD double prop_sinc(double x) {  // ode::sinc (ode/ode.hpp:58-70)
  BA_NO_CONTRACT
  if (fabs(x) > 1e-6) return sin(x) / x;
  const double x2 = x * x, x4 = x2 * x2, x6 = (x2 * x2) * x2;
  return ((1.0 - (1.0 / 6.0) * x2) + (1.0 / 120.0) * x4) - (1.0 / 5040.0) * x6;
}
BA_HD void prop_right_jacobian(const double* phi, double* J) {  // rightJacobian (implementation/Transformation.hpp:69-82)
  BA_NO_CONTRACT
  const double Phi = prop_norm3(phi);
  double X[9], X2[9];
  ba::cross_mx(phi, X);
  prop_m3mul(X, X, X2);
  double a, b;
  if (Phi < 1.0e-4) {
    a = -0.5;
    b = 1.0 / 6.0;
  } else {
    const double Phi2 = Phi * Phi, Phi3 = Phi2 * Phi;
    a = -(1.0 - cos(Phi)) / Phi2;
    b = (Phi - sin(Phi)) / Phi3;
  }
  for (int i = 0; i < 9; ++i) {
    const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
    J[i] = (id + a * X[i]) + b * X2[i];
  }
}

BA_HD void prop_reset(PropState* S) {
  for (int c = 0; c < 9; ++c) S->Cint[c] = S->Cdbl[c] = S->cross[c] = S->dal[c] = S->dv[c] = S->dp[c] = 0.0;
  for (int c = 0; c < 3; ++c) S->aint[c] = S->adbl[c] = S->Dq[c] = 0.0;
  S->Dq[3] = 1.0;
  S->Dt = 0.0;
}

// One step from (w0, a0) to (w1, a1), both already interpolated to the step's ends, over dt.  sb = the call's speed and biases.
// F is filled only under want_cov.  S and F may be shared by the lanes of a wave, which all make the same call: each value is read
// before the step replaces it, and only the caller with `own` set stores (on the host: always).  A block of F is stored as soon as
// its operands exist, so that nothing waits in registers for the end of the step.
BA_HD void prop_step(const okvis_ba_imu_params& prm, const double* w0, const double* a0, const double* w1, const double* a1, double dt,
                     const double* sb, PropState* S, bool want_cov, PropF* F, bool own) {
  BA_NO_CONTRACT
  // saturation (:369-389)
  double sigma_g_c = prm.sigma_g_c, sigma_a_c = prm.sigma_a_c;
  bool gsat = false, asat = false;
  for (int c = 0; c < 3; ++c) {
    gsat = gsat || fabs(w0[c]) > prm.g_max || fabs(w1[c]) > prm.g_max;
    asat = asat || fabs(a0[c]) > prm.a_max || fabs(a1[c]) > prm.a_max;
  }
  if (gsat) sigma_g_c *= 100;
  if (asat) sigma_a_c *= 100;
  if (want_cov && own) {  // the noise (:434-445)
    F->dt = dt;
    F->q_al = (dt * sigma_g_c) * sigma_g_c;
    F->q_v = (dt * sigma_a_c) * prm.sigma_a_c;
    F->q_p = ((0.5 * dt) * dt) * ((dt * sigma_a_c) * prm.sigma_a_c);
    F->q_bg = (dt * prm.sigma_gw_c) * prm.sigma_gw_c;
    F->q_ba = (dt * prm.sigma_aw_c) * prm.sigma_aw_c;
  }
  // orientation (:392-400)
  double om[3], ab[3];
  for (int c = 0; c < 3; ++c) {
    om[c] = 0.5 * (w0[c] + w1[c]) - sb[3 + c];
    ab[c] = 0.5 * (a0[c] + a1[c]) - sb[6 + c];
  }
  const double theta_half = (prop_norm3(om) * 0.5) * dt;
  const double sc = prop_sinc(theta_half);
  const double dq[4] = {((sc * om[0]) * 0.5) * dt, ((sc * om[1]) * 0.5) * dt, ((sc * om[2]) * 0.5) * dt, cos(theta_half)};
  const double Dq0[4] = {S->Dq[0], S->Dq[1], S->Dq[2], S->Dq[3]};
  double Dq1[4];
  ba::qmul_strict(Dq0, dq, Dq1);
  // rotation matrix integrals (:401-409); the blocks of F_delta (:421-431) take the values from before the memory shift
  double C[9], C1[9], CC[9], ha[3], qa[3];
  prop_qrot(Dq0, C);
  prop_qrot(Dq1, C1);
  for (int c = 0; c < 9; ++c) CC[c] = C[c] + C1[c];
  {
    double h[9], q4[9];
    for (int c = 0; c < 9; ++c) h[c] = 0.5 * CC[c], q4[c] = 0.25 * CC[c];
    prop_m3vec(h, ab, ha);
    prop_m3vec(q4, ab, qa);
    for (int c = 0; c < 9; ++c) {
      const double Cint = S->Cint[c], Cdbl = S->Cdbl[c];
      if (want_cov && own) F->A012[c] = (-1.0 * Cint) * dt + (q4[c] * dt) * dt, F->A612[c] = (-0.5 * CC[c]) * dt;
      if (own) S->Cdbl[c] = (Cdbl + Cint * dt) + (q4[c] * dt) * dt, S->Cint[c] = Cint + h[c] * dt;
    }
  }
  {
    double dd[3], hav[3], sk[9];  // dd = acc_integral dt + 0.25 (C + C_1) acc dt^2, the increment of acc_doubleintegral
    for (int c = 0; c < 3; ++c) {
      const double aint = S->aint[c], adbl = S->adbl[c];
      dd[c] = aint * dt + (qa[c] * dt) * dt;
      hav[c] = ha[c] * dt;
      if (own) S->adbl[c] = (adbl + aint * dt) + (qa[c] * dt) * dt, S->aint[c] = aint + ha[c] * dt;
    }
    if (want_cov && own) {
      ba::cross_mx(dd, sk);
      for (int c = 0; c < 9; ++c) F->A03[c] = -1.0 * sk[c];
      ba::cross_mx(hav, sk);
      for (int c = 0; c < 9; ++c) F->A63[c] = -1.0 * sk[c];
    }
  }
  // Jacobian parts (:411-417)
  for (int c = 0; c < 9; ++c) {
    const double dal = S->dal[c];
    if (own) S->dal[c] = dal + dt * C1[c];
    if (want_cov && own) F->A39[c] = (-dt) * C1[c];
  }
  double cross0[9], cross1[9], G[9];
  for (int c = 0; c < 9; ++c) cross0[c] = S->cross[c];
  {
    const double phi[3] = {om[0] * dt, om[1] * dt, om[2] * dt};
    double Jr[9], dqi[4], Ri[9];
    prop_right_jacobian(phi, Jr);
    ba::qinv_strict(dq, dqi);
    prop_qrot(dqi, Ri);
    prop_m3mul(Ri, cross0, cross1);
    for (int c = 0; c < 9; ++c) cross1[c] = cross1[c] + Jr[c] * dt;
  }
  {
    double ax[9], u[9], v[9];
    ba::cross_mx(ab, ax);
    prop_m3mul(C, ax, u);
    prop_m3mul(u, cross0, G);
    prop_m3mul(C1, ax, u);
    prop_m3mul(u, cross1, v);
    for (int c = 0; c < 9; ++c) G[c] = G[c] + v[c];
  }
  const double half_dt = 0.5 * dt, quarter_dt2 = (0.25 * dt) * dt;
  for (int c = 0; c < 9; ++c) {
    const double dv = S->dv[c], dp = S->dp[c];
    const double dp_term = dt * dv + quarter_dt2 * G[c];
    if (want_cov && own) F->A09[c] = dp_term, F->A69[c] = half_dt * G[c];
    // ... and the memory shift (:448-454)
    if (own) S->dp[c] = dp + dp_term, S->dv[c] = dv + half_dt * G[c], S->cross[c] = cross1[c];
  }
  const double Dt = S->Dt;
  if (own) {
    for (int c = 0; c < 4; ++c) S->Dq[c] = Dq1[c];
    S->Dt = Dt + dt;
  }
}

// y = (I + N) x: one column of F P, or one row of (F P) F^T
BA_HD void prop_apply(const PropF& F, const double* x, double* y) {
  BA_NO_CONTRACT
  for (int i = 0; i < 3; ++i) {
    double s = x[i];
    for (int k = 0; k < 3; ++k) s = s + F.A03[3 * i + k] * x[3 + k];
    s = s + F.dt * x[6 + i];
    for (int k = 0; k < 3; ++k) s = s + F.A09[3 * i + k] * x[9 + k];
    for (int k = 0; k < 3; ++k) s = s + F.A012[3 * i + k] * x[12 + k];
    y[i] = s;
  }
  for (int i = 0; i < 3; ++i) {
    double s = x[3 + i];
    for (int k = 0; k < 3; ++k) s = s + F.A39[3 * i + k] * x[9 + k];
    y[3 + i] = s;
  }
  for (int i = 0; i < 3; ++i) {
    double s = F.A63[3 * i] * x[3];
    for (int k = 1; k < 3; ++k) s = s + F.A63[3 * i + k] * x[3 + k];
    s = s + x[6 + i];
    for (int k = 0; k < 3; ++k) s = s + F.A69[3 * i + k] * x[9 + k];
    for (int k = 0; k < 3; ++k) s = s + F.A612[3 * i + k] * x[12 + k];
    y[6 + i] = s;
  }
  for (int i = 9; i < 15; ++i) y[i] = x[i];
}
// the noise of the step on entry d of the diagonal (:441-445)
BA_HD double prop_noise(const PropF& F, int d) { return d < 3 ? F.q_p : d < 6 ? F.q_al : d < 9 ? F.q_v : d < 12 ? F.q_bg : F.q_ba; }

// y = T x, T = blockdiag(C, C, C, I, I)
BA_HD void prop_rotate(const double* C, const double* x, double* y) {
  for (int b = 0; b < 3; ++b) prop_m3vec(C, x + 3 * b, y + 3 * b);
  for (int i = 9; i < 15; ++i) y[i] = x[i];
}

// The end of a call: T (r, q; q as given, normalised here as Transformation's constructor does) and sb become the propagated
// state (:470-477), C0 = C_WS_0; under want_jac the blocks of F (:480-491) go to J (stored by
// the caller with `own` set, as in prop_step).
BA_HD void prop_finish(const okvis_ba_imu_params& prm, const PropState& S, double* T, double* sb, double* C0, bool want_jac, PropF* J,
                       bool own) {
  BA_NO_CONTRACT
  double q0[4] = {T[3], T[4], T[5], T[6]};
  ba::qnormalize_strict(q0);
  prop_qrot(q0, C0);
  const double Dt = S.Dt;
  const double g_W[3] = {0.0, 0.0, prm.g};  // g * (0, 0, 6371009).normalized()
  double ca[3], cv[3], qn[4];
  prop_m3vec(C0, S.adbl, ca);
  prop_m3vec(C0, S.aint, cv);
  const double half_dt2 = (0.5 * Dt) * Dt;
  for (int c = 0; c < 3; ++c) T[c] = ((T[c] + sb[c] * Dt) + ca[c]) - half_dt2 * g_W[c];
  ba::qmul_strict(q0, S.Dq, qn);
  ba::qnormalize_strict(qn);
  for (int c = 0; c < 4; ++c) T[3 + c] = qn[c];
  for (int c = 0; c < 3; ++c) sb[c] = (sb[c] + cv[c]) - g_W[c] * Dt;
  if (want_jac && own) {
    double sk[9], m[9];
    ba::cross_mx(ca, sk);
    for (int c = 0; c < 9; ++c) J->A03[c] = -1.0 * sk[c];
    J->dt = Dt;
    prop_m3mul(C0, S.dp, J->A09);
    prop_m3mul(C0, S.Cdbl, m);
    for (int c = 0; c < 9; ++c) J->A012[c] = -1.0 * m[c];
    prop_m3mul(C0, S.dal, m);
    for (int c = 0; c < 9; ++c) J->A39[c] = -1.0 * m[c];
    ba::cross_mx(cv, sk);
    for (int c = 0; c < 9; ++c) J->A63[c] = -1.0 * sk[c];
    prop_m3mul(C0, S.dv, J->A69);
    prop_m3mul(C0, S.Cint, m);
    for (int c = 0; c < 9; ++c) J->A612[c] = -1.0 * m[c];
    J->q_p = J->q_al = J->q_v = J->q_bg = J->q_ba = 0.0;
  }
}

#if defined(__HIPCC__)
// a job and where its results go: the outputs are packed in job order (only what was asked for comes back from the device)
struct PropJob {
  okvis_fe_imu_job job;
  int32_t row0;                   // call k of the job writes row row0 + k of T_WS, sb and count,
  int32_t cov0, jac0;             // row cov0 + k of cov and row jac0 + k of jac (under the job's flags)
  int32_t reserved;
};
struct PropParams {
  const okvis_ba_imu_params* params;
  const long long* s_t;           // the sample pool
  const double* s_gyr;            // [n_samples][3]
  const double* s_acc;
  const long long* ends;          // the pool of end times
  const PropJob* jobs;
  int32_t n_jobs;
  double* T_WS;                   // [rows][7]
  double* sb;                     // [rows][9]
  int32_t* count;                 // [rows]
  double* cov;                    // [cov rows][225]; the row of a call that returned early is not written
  double* jac;
};

// what a wave keeps in LDS, private to it
struct PropLds {
  long long t[PROP_WINDOW];
  double gyr[3 * PROP_WINDOW], acc[3 * PROP_WINDOW];
  double P[15 * PROP_LD], M[15 * PROP_LD];
  PropState S;  // the same for every lane: lane 0 stores, all read
  PropF F;
};

// the LDS of a wave is written and read by that wave only: order the two within the wave
__device__ __forceinline__ void prop_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// f applied to a slab from both sides: lane j < 15 takes column j of `in`, f(column) goes to column j of `mid`; lane i takes row i
// of `mid`, and f(row) is returned in y
template <class Apply>
__device__ __forceinline__ void prop_two_sided(const double* in, double* mid, int lane, Apply f, double* y) {
  double x[15];
  if (lane < 15) {
#pragma unroll
    for (int k = 0; k < 15; ++k) x[k] = in[PROP_LD * k + lane];
    f(x, y);
#pragma unroll
    for (int k = 0; k < 15; ++k) mid[PROP_LD * k + lane] = y[k];
  }
  prop_wave_sync();
  if (lane < 15) {
#pragma unroll
    for (int k = 0; k < 15; ++k) x[k] = mid[PROP_LD * lane + k];
    f(x, y);
  }
}

// One call of ImuError::propagation over the job's deque ts / gyr / acc [n] (n >= 2, ts[n - 1] >= t_end).  T and sb are the state,
// in and out; returns the number of integration steps.
__device__ __forceinline__ int prop_call(const okvis_ba_imu_params& prm, const long long* ts, const double* gyr, const double* acc, int n,
                                         long long t_start, long long t_end, double* T, double* sb, bool want_cov, bool want_jac,
                                         double* cov, double* jac, PropLds& L, int lane) {
  // the first step that advances: nexttime - t_start > 0 with nexttime already cut to t_end (:331-349)
  int first = n;
  for (int b = 0; b < n && first == n; b += 64) {
    const int it = b + lane;
    bool hit = false;
    if (it < n) {
      long long nexttime = (it + 1 == n) ? t_end : ts[it + 1];
      if (t_end < nexttime) nexttime = t_end;
      hit = nexttime - t_start > 0;
    }
    const unsigned long long m = __ballot(hit);
    if (m) first = b + __ffsll((long long)m) - 1;
  }
  PropState& S = L.S;
  PropF& F = L.F;
  const bool own = lane == 0;
  prop_wave_sync();  // (what the call before this one still reads)
  if (own) prop_reset(&S);
  if (want_cov && lane < 15) {
#pragma unroll
    for (int k = 0; k < 15; ++k) L.P[PROP_LD * k + lane] = 0.0;
  }
  prop_wave_sync();
  long long time = t_start;
  bool started = false;
  int i = 0, base = 0;
  bool staged = false;
  for (int it = first; it < n; ++it) {
    if (!staged || it + 1 - base >= PROP_WINDOW) {  // samples it and it + 1 have to be in the window
      prop_wave_sync();
      base = it;
      const int s = base + lane;
      if (s < n) {
        L.t[lane] = ts[s];
#pragma unroll
        for (int c = 0; c < 3; ++c) L.gyr[3 * lane + c] = gyr[3 * (size_t)s + c], L.acc[3 * lane + c] = acc[3 * (size_t)s + c];
      }
      prop_wave_sync();
      staged = true;
    }
    const int o0 = it - base, o1 = (it + 1 < n) ? o0 + 1 : o0;  // (the reference reads it + 1 before its end check)
    double w0[3], a0[3], w1[3], a1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) w0[c] = L.gyr[3 * o0 + c], a0[c] = L.acc[3 * o0 + c], w1[c] = L.gyr[3 * o1 + c], a1[c] = L.acc[3 * o1 + c];
    const long long t_it = L.t[o0];
    long long nexttime = (it + 1 == n) ? t_end : L.t[o1];
    double dt = prop_sec(nexttime - time);
    {
      BA_NO_CONTRACT
      if (t_end < nexttime) {  // the end interpolation comes first (:347-356) ...
        const double interval = prop_sec(nexttime - t_it);
        nexttime = t_end;
        dt = prop_sec(nexttime - time);
        const double r = dt / interval;
#pragma unroll
        for (int c = 0; c < 3; ++c) w1[c] = (1.0 - r) * w0[c] + r * w1[c], a1[c] = (1.0 - r) * a0[c] + r * a1[c];
      }
      if (dt <= 0.0) continue;
      if (!started) {  // ... and the start one reads the second sample as it is by now (:361-366)
        started = true;
        const double r = dt / prop_sec(nexttime - t_it);
#pragma unroll
        for (int c = 0; c < 3; ++c) w0[c] = r * w0[c] + (1.0 - r) * w1[c], a0[c] = r * a0[c] + (1.0 - r) * a1[c];
      }
    }
    prop_step(prm, w0, a0, w1, a1, dt, sb, &S, want_cov, &F, own);
    prop_wave_sync();
    if (want_cov) {  // P <- F P F^T + Q
      double y[15];
      prop_two_sided(L.P, L.M, lane, [&](const double* x, double* o) { prop_apply(F, x, o); }, y);
      if (lane < 15) {
#pragma unroll
        for (int k = 0; k < 15; ++k) L.P[PROP_LD * lane + k] = (k == lane) ? y[k] + prop_noise(F, k) : y[k];
      }
      prop_wave_sync();
    }
    time = nexttime;
    ++i;
    if (nexttime == t_end) break;
  }
  double C0[9];
  prop_finish(prm, S, T, sb, C0, want_jac, &F, own);
  prop_wave_sync();
  if (want_jac) {  // lane j: column j of F = F e_j
    if (lane < 15) {
      double x[15], y[15];
#pragma unroll
      for (int k = 0; k < 15; ++k) x[k] = (k == lane) ? 1.0 : 0.0;
      prop_apply(F, x, y);
#pragma unroll
      for (int k = 0; k < 15; ++k) jac[15 * k + lane] = y[k];
    }
  }
  if (want_cov) {  // T P_delta T^T
    double y[15];
    prop_two_sided(L.P, L.M, lane, [&](const double* x, double* o) { prop_rotate(C0, x, o); }, y);
    if (lane < 15) {
#pragma unroll
      for (int k = 0; k < 15; ++k) cov[15 * lane + k] = y[k];
    }
  }
  return i;
}

__global__ void __launch_bounds__(PROP_THREADS) imu_propagate_kernel(const PropParams P) {
  __shared__ PropLds lds[PROP_WAVES];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int j = blockIdx.x * PROP_WAVES + wave;
  if (j >= P.n_jobs) return;  // (no workgroup barrier anywhere: a wave may leave)
  const okvis_fe_imu_job& J = P.jobs[j].job;
  const size_t row0 = (size_t)P.jobs[j].row0, cov0 = (size_t)P.jobs[j].cov0, jac0 = (size_t)P.jobs[j].jac0;
  const okvis_ba_imu_params prm = P.params[J.prm];
  const int n = J.s_count;
  const long long* ts = P.s_t + J.s_begin;
  const double* gyr = P.s_gyr + 3 * (size_t)J.s_begin;
  const double* acc = P.s_acc + 3 * (size_t)J.s_begin;
  const bool want_cov = (J.flags & OKVIS_FE_IMU_COV) != 0, want_jac = (J.flags & OKVIS_FE_IMU_JAC) != 0;
  double T[7], sb[9];
#pragma unroll
  for (int c = 0; c < 7; ++c) T[c] = J.T_WS[c];
#pragma unroll
  for (int c = 0; c < 9; ++c) sb[c] = J.sb[c];
  long long start = J.t_start;
  for (int k = 0; k < J.e_count; ++k) {
    const size_t e = row0 + (size_t)k;
    const long long end = P.ends[(size_t)J.e_begin + (size_t)k];
    int cnt;
    if (n < 2) cnt = 0;                       // Frontend::propagation's early return (Frontend.cpp:281-286)
    else if (!(ts[n - 1] >= end)) cnt = -1;   // ImuError.cpp:301-302: the state stays as it is
    else cnt = prop_call(prm, ts, gyr, acc, n, start, end, T, sb, want_cov, want_jac, want_cov ? P.cov + 225 * (cov0 + (size_t)k) : nullptr,
                         want_jac ? P.jac + 225 * (jac0 + (size_t)k) : nullptr, lds[wave], lane);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 7; ++c) P.T_WS[7 * e + c] = T[c];
#pragma unroll
      for (int c = 0; c < 9; ++c) P.sb[9 * e + c] = sb[c];
      P.count[e] = cnt;
    }
    start = end;
  }
}
#endif  // __HIPCC__

}  // namespace fe
