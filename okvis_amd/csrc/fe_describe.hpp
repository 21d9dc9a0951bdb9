// Keypoint description of the OKVIS frontend on the device (include/okvis_amd_frontend.h: okvis_fe_describe_keypoints,
// okvis_fe_detect_and_describe): what Frame::describe (okvis_cv/include/okvis/implementation/Frame.hpp:128-156) does behind the
// detector — an angle per keypoint from the extraction direction (gravity in the camera frame) through the projection Jacobian,
// and a 48-byte binary descriptor at that angle and a fixed scale — for many images per call.
//
// The angle stage is the reference's, operation for operation in fp64 up to eg = J d; atan2(eg1, eg0) / M_PI * 180 is then
// rounded once where the reference rounds three times (dsc_angle_degrees).  The reference's extractor is
// brisk::BriskDescriptorExtractor(rotationInvariance = true, scaleInvariance = false), and BRISK's source is not part of the
// reference tree: the extractor is stated in the header from the published BRISK construction and is NOT pinned to BRISK.
// Everything but the angle is integer arithmetic and exact.
//
//   dsc_position     qx, qy in sixteenths of a pixel and the 11-pixel margin test
//   dsc_rot          the rotation index of a float angle
//   dsc_angle_degrees  atan2(y, x) / M_PI * 180 evaluated in double-double and rounded once
//   dsc_centre       the sample centre of point k under rotation `rot`: Q30 x Q16 in int64, reduced to Q4 half away from zero
//   dsc_sample       V = sum I wy wx over the at most 5 x 5 pixels the box of side 2 h touches
//   dsc_bit          the comparison of two box means by cross-multiplication
//   describe_keypoint_serial, describe_image_serial   the statement as plain loops (host referee of the probe, CPU side of the
//                    benchmark)
//
// describe_angle_kernel: one lane per keypoint; back_project and project_homogeneous of fe_kernels.hpp, eg = J d, dsc_angle_degrees.
// describe_kernel: one wave per keypoint, four waves per workgroup.  The wave copies the 25 x 25 pixels around the keypoint's
// nearest pixel into its own LDS slab (row stride 28), lane k < 60 computes V_k from the slab and leaves it in LDS, then six rounds:
// lane L takes pair 64 r + L, and the ballot of a round is one 64-bit word of the descriptor.  The four waves of a workgroup share
// nothing: no workgroup barrier, no atomics, no scratch; every loop has a compile-time bound.  The tables are in constant memory;
// cs[rot] is the same for the whole wave.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "ba_math.hpp"

namespace fe {

constexpr int DSC_POINTS = 60, DSC_PAIRS = 383, DSC_BYTES = 48, DSC_ROTS = 1024, DSC_RINGS = 5;
constexpr int DSC_MARGIN = 176;   // sixteenths: the tables' reach is 177 and pixel 0 covers [-8, 8)
constexpr int DSC_REACH = 177;
constexpr int DSC_VALID = 1, DSC_ANGLE_UNDEFINED = 2;   // OKVIS_FE_DESCRIBE_*
constexpr int DSC_PATCH = 25, DSC_PATCH_HALF = 12, DSC_PSTRIDE = 28;   // the slab: pixels ix - 12 .. ix + 12, rows 28 bytes apart
static_assert(16 * DSC_PATCH_HALF + 8 > 8 + DSC_REACH, "the slab holds every box of a keypoint up to half a pixel off its centre");

namespace dsc_host {
#define DSC_TABLE static const
#include "fe_describe_tables.inc"
#undef DSC_TABLE
}  // namespace dsc_host
#if defined(__HIPCC__)
namespace dsc_dev {
#define DSC_TABLE static __device__ __constant__ const
#include "fe_describe_tables.inc"
#undef DSC_TABLE
}  // namespace dsc_dev
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DSC_T(name) dsc_dev::name
#else
#define DSC_T(name) dsc_host::name
#endif

// kp.x, kp.y -> (qx, qy); false when the keypoint is not VALID (then qx, qy are not written)
BA_HD bool dsc_position(float kx, float ky, int w, int h, int32_t* qx, int32_t* qy) {
  BA_NO_CONTRACT
  const double tx = floor((double)kx * 16.0 + 0.5), ty = floor((double)ky * 16.0 + 0.5);
  // a NaN fails every comparison, an infinity one of them; inside the bounds the conversion is exact
  if (!(tx >= (double)DSC_MARGIN && tx <= (double)(16 * (w - 1) - DSC_MARGIN) && ty >= (double)DSC_MARGIN && ty <= (double)(16 * (h - 1) - DSC_MARGIN)))
    return false;
  *qx = (int32_t)tx, *qy = (int32_t)ty;
  return true;
}

// ((int)floor((double)angle * 1024 / 360 + 0.5)) mod 1024 in 0..1023; angle finite and within +-180 (what atan2 gives)
BA_HD int32_t dsc_rot(float angle) {
  BA_NO_CONTRACT
  const int32_t r = (int32_t)floor((double)angle * 1024.0 / 360.0 + 0.5);
  return ((r % DSC_ROTS) + DSC_ROTS) % DSC_ROTS;
}

// ---- atan2(y, x) / M_PI * 180 in ONE rounding -------------------------------------------------------------------------------
// The reference's three operations round three times, which leaves its double up to 2 ulp from the value of the expression; the
// angle stage is held to less than that (tests/describe_cases.py), so the tail is evaluated in double-double (a value as an
// unevaluated sum hi + lo of two doubles, products split by fma) and rounded once.  With theta the table angle nearest to a
// double-precision estimate: (u, v) = (x, y) turned by -theta, t = v / u with |t| < tan(pi / 127), atan t by its series
// (t^15 / 15 < 2e-26), the angle theta + atan t, times 180 / M_PI.  Every step errs below 2^-100 of the angle.
struct DscDD { double hi, lo; };
BA_HD DscDD dsc_dd_sum(double a, double b) {   // exact
  BA_NO_CONTRACT
  const double s = a + b, bb = s - a;
  return DscDD{s, (a - (s - bb)) + (b - bb)};
}
BA_HD DscDD dsc_dd_mul(double a, double b) {   // exact
  const double p = a * b;
  return DscDD{p, fma(a, b, -p)};
}
BA_HD DscDD dsc_dd_add(DscDD a, DscDD b) {
  BA_NO_CONTRACT
  const DscDD s = dsc_dd_sum(a.hi, b.hi);
  return dsc_dd_sum(s.hi, s.lo + (a.lo + b.lo));
}
BA_HD DscDD dsc_dd_mul(DscDD a, DscDD b) {
  BA_NO_CONTRACT
  const DscDD p = dsc_dd_mul(a.hi, b.hi);
  return dsc_dd_sum(p.hi, p.lo + (a.hi * b.lo + a.lo * b.hi));
}
BA_HD DscDD dsc_dd_div(DscDD a, DscDD b) {
  BA_NO_CONTRACT
  const double q1 = a.hi / b.hi;
  const DscDD r = dsc_dd_add(a, dsc_dd_mul(DscDD{-q1, 0.0}, b));
  return dsc_dd_sum(q1, r.hi / b.hi);
}
// x, y finite; degrees in (-180, 180]
BA_HD double dsc_angle_degrees(double y, double x) {
  BA_NO_CONTRACT
  const double ax = fabs(x), ay = fabs(y), big = ax > ay ? ax : ay;
  const double a0 = atan2(y, x);
  // a zero component, or magnitudes at which a product of two parts leaves the format: the reference's own three operations
  if (x == 0.0 || y == 0.0 || !(big > 1e-100 && big < 1e100)) return a0 / M_PI * 180.0;
  int i = (int)floor(a0 * (64.0 / M_PI) + 0.5);
  i = i < -64 ? -64 : (i > 64 ? 64 : i);
  const double* T = DSC_T(dsc_turn)[i + 64];
  const DscDD th{T[0], T[1]}, c{T[2], T[3]}, s{T[4], T[5]}, X{x, 0.0}, Y{y, 0.0}, nX{-x, 0.0};
  const DscDD u = dsc_dd_add(dsc_dd_mul(X, c), dsc_dd_mul(Y, s));    // r cos(a - theta) > 0
  const DscDD v = dsc_dd_add(dsc_dd_mul(Y, c), dsc_dd_mul(nX, s));   // r sin(a - theta)
  const DscDD t = dsc_dd_div(v, u);
  const double z = t.hi * t.hi;
  // atan t = t (1 + P), P = -z / 3 + z^2 / 5 - ... + z^6 / 13 - z^7 / 15: |P| < 3e-4, a double's error in it is below 1e-19 of t
  const double P = z * (-1.0 / 3.0 + z * (1.0 / 5.0 + z * (-1.0 / 7.0 + z * (1.0 / 9.0 + z * (-1.0 / 11.0 + z * (1.0 / 13.0 + z * (-1.0 / 15.0)))))));
  const DscDD at = dsc_dd_add(t, dsc_dd_mul(t.hi, P));
  const DscDD deg = dsc_dd_mul(dsc_dd_add(th, at), DscDD{DSC_T(dsc_degrees)[0], DSC_T(dsc_degrees)[1]});
  return deg.hi + deg.lo;
}

// Q46 -> Q4, to nearest, half away from zero: the symmetry under z -> -z is what makes a quarter turn exact
BA_HD int32_t dsc_reduce(int64_t z) {
  const int64_t a = ((z < 0 ? -z : z) + ((int64_t)1 << 41)) >> 42;
  return (int32_t)(z < 0 ? -a : a);
}

BA_HD void dsc_centre(int32_t c, int32_t s, int k, int32_t qx, int32_t qy, int32_t* cx, int32_t* cy) {
  const int64_t bx = DSC_T(dsc_base)[k][0], by = DSC_T(dsc_base)[k][1];
  *cx = qx + dsc_reduce((int64_t)c * bx - (int64_t)s * by);
  *cy = qy + dsc_reduce((int64_t)s * bx + (int64_t)c * by);
}

// The box [cx - hw, cx + hw) x [cy - hw, cy + hw) in sixteenths over the pixels of `img` (pixel (0, 0) at img, rows `stride`
// apart, pixel x covering [16 x - 8, 16 x + 8)).  cx - hw, cy - hw >= -8.  At most five pixels a side carry weight; an index past
// xmax / ymax carries none and is clamped, so that nothing outside the image (the slab) is read.  V <= 255 * 60^2 < 2^20.
BA_HD int32_t dsc_sample(const uint8_t* img, int stride, int xmax, int ymax, int32_t cx, int32_t cy, int32_t hw) {
  const int32_t x0 = (cx - hw + 8) >> 4, y0 = (cy - hw + 8) >> 4;
  int32_t v = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int32_t y = y0 + j;
    const int32_t lo = 16 * y - 8 > cy - hw ? 16 * y - 8 : cy - hw, hi = 16 * y + 8 < cy + hw ? 16 * y + 8 : cy + hw;
    const int32_t wy = hi > lo ? hi - lo : 0;
    const uint8_t* row = img + (y < ymax ? y : ymax) * stride;
    int32_t acc = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int32_t x = x0 + i;
      const int32_t l = 16 * x - 8 > cx - hw ? 16 * x - 8 : cx - hw, r = 16 * x + 8 < cx + hw ? 16 * x + 8 : cx + hw;
      const int32_t wx = r > l ? r - l : 0;
      acc += (int32_t)row[x < xmax ? x : xmax] * wx;
    }
    v += acc * wy;
  }
  return v;
}

// mean_i > mean_k with mean = V / A, A = (2 h)^2 <= 3600: both products below 2^20 * 3600 < 3.8e9
BA_HD bool dsc_bit(int32_t vi, int32_t hi, int32_t vk, int32_t hk) {
  return (int64_t)vi * (int64_t)(4 * hk * hk) > (int64_t)vk * (int64_t)(4 * hi * hi);
}

// One keypoint as plain loops: desc [48], *flag gets DSC_VALID or 0 (the angle's flag is the caller's)
inline void describe_keypoint_serial(const uint8_t* image, int w, int h, int pitch, float kx, float ky, int32_t rot, uint8_t* desc, uint8_t* flag) {
  memset(desc, 0, DSC_BYTES);
  *flag = 0;
  int32_t qx, qy;
  if (!dsc_position(kx, ky, w, h, &qx, &qy)) return;
  *flag = DSC_VALID;
  int32_t V[DSC_POINTS], H[DSC_POINTS];
  const int32_t c = dsc_host::dsc_cs[rot][0], s = dsc_host::dsc_cs[rot][1];
  for (int k = 0; k < DSC_POINTS; ++k) {
    int32_t cx, cy;
    dsc_centre(c, s, k, qx, qy, &cx, &cy);
    H[k] = dsc_host::dsc_half[dsc_host::dsc_ring[k]];
    V[k] = dsc_sample(image, pitch, w - 1, h - 1, cx, cy, H[k]);
  }
  for (int b = 0; b < DSC_PAIRS; ++b) {
    const int i = dsc_host::dsc_pairs[b][0], k = dsc_host::dsc_pairs[b][1];
    if (dsc_bit(V[i], H[i], V[k], H[k])) desc[b >> 3] |= (uint8_t)(1u << (b & 7));
  }
}

// The per-image statement behind the angle stage: kp [n][3], rot [n] in 0..1023 -> desc [n][48], flags [n]; returns n_valid
inline int describe_image_serial(const uint8_t* image, int w, int h, int pitch, int n, const float* kp, const int32_t* rot, uint8_t* desc, uint8_t* flags) {
  int n_valid = 0;
  for (int i = 0; i < n; ++i) {
    describe_keypoint_serial(image, w, h, pitch, kp[3 * (size_t)i], kp[3 * (size_t)i + 1], rot[i], desc + (size_t)DSC_BYTES * i, flags + i);
    n_valid += flags[i] & DSC_VALID;
  }
  return n_valid;
}

#if defined(__HIPCC__)
struct DscImage {  // one job as the device sees it
  int64_t pix;     // where its bytes start in the pixel pool (rows packed, no pitch)
  int32_t w, h;
  int32_t kp0;     // its keypoints: rows kp0 .. of the row pools (rot, flags, desc, angle, angle64)
  int32_t n;       // how many; -1: n_keypoints of the detect result `det`
  int32_t det;     // the detect job whose selected keypoints it describes (the chain), -1: keypoints from the kp pool
  int32_t sel0;    // the detect job's first record in the selection pool
  int32_t cam;     // its camera and direction in the camera pool, -1: rot comes from the caller
  int32_t reserved;
};
struct DscCamera {
  Camera cam;
  double dir[3];
};
struct DscParams {
  const uint8_t* pix;
  const DscImage* images;
  const int32_t* row_job;   // [rows] the job of every row of the row pools
  const float* kp;          // [rows][3], unused rows of a chained job are not read
  const DetCand* sel;       // the detect kernels' selection pool (the chain)
  const DetResult* det_res;
  const DscCamera* cams;
  const int32_t* rot_in;    // [rows] the caller's indices, read for jobs without a camera; null when every job has one
  int32_t* rot;             // [rows]
  float* angle;             // [rows] or null
  double* angle64;          // [rows] or null
  uint8_t* flags;           // [rows]
  uint8_t* desc;            // [rows][48]
  int32_t rows;
};

// the keypoint of row `row`: false when the row is past the job's count (a chained job's unused rows)
__device__ inline bool dsc_keypoint(const DscParams& P, const DscImage& im, int row, float* kx, float* ky) {
  const int i = row - im.kp0;
  if (im.det >= 0) {
    const DetResult R = P.det_res[im.det];
    if (i >= R.n_keypoints) return false;   // an OVERFLOW job has none
    const DetCand c = P.sel[im.sel0 + i];
    *kx = c.fx, *ky = c.fy;
    return true;
  }
  *kx = P.kp[3 * (int64_t)row], *ky = P.kp[3 * (int64_t)row + 1];
  return true;
}

constexpr int DSC_ANGLE_THREADS = 64;

// Frame.hpp:139-150 for one keypoint.  Undefined (flag ANGLE_UNDEFINED, rot = 0, angle = 0): backProject failed, the projection's
// distortion is undefined (the reference then reads a Jacobian it never wrote), or eg is not finite.
__global__ void __launch_bounds__(DSC_ANGLE_THREADS) describe_angle_kernel(const DscParams P) {
  const int row = blockIdx.x * DSC_ANGLE_THREADS + threadIdx.x;
  if (row >= P.rows) return;
  const DscImage im = P.images[P.row_job[row]];
  float kx, ky;
  if (!dsc_keypoint(P, im, row, &kx, &ky)) return;
  if (im.cam < 0) {   // rot_in: the stage is skipped, the flag starts empty
    P.rot[row] = P.rot_in[row];
    P.flags[row] = 0;
    return;
  }
  const DscCamera& C = P.cams[im.cam];
  double ep[4], uv[2], J[6];
  bool ok = back_project(C.cam, (double)kx, (double)ky, ep);
  ep[3] = 1.0;
  // ep[2] = 1: the Jacobian is always written, and INVALID means that the distortion was not defined
  ok = project_homogeneous(C.cam, ep, uv, J) != OKVIS_FE_PROJ_INVALID && ok;
  double a64;
  {
    BA_NO_CONTRACT
    const double eg0 = J[0] * C.dir[0] + J[1] * C.dir[1] + J[2] * C.dir[2];
    const double eg1 = J[3] * C.dir[0] + J[4] * C.dir[1] + J[5] * C.dir[2];
    ok = ok && isfinite(eg0) && isfinite(eg1);
    a64 = ok ? dsc_angle_degrees(eg1, eg0) : 0.0;   // atan2(eg1, eg0) / M_PI * 180.0 in one rounding
  }
  if (!ok) a64 = 0.0;
  const float a32 = (float)a64;
  P.rot[row] = ok ? dsc_rot(a32) : 0;
  if (P.angle) P.angle[row] = a32;
  if (P.angle64) P.angle64[row] = a64;
  P.flags[row] = ok ? 0 : DSC_ANGLE_UNDEFINED;
}

constexpr int DSC_WAVES = 4, DSC_THREADS = 64 * DSC_WAVES;
constexpr int DSC_SLAB = DSC_PATCH * DSC_PSTRIDE;   // 700 bytes
constexpr int DSC_ROUNDS = (DSC_PAIRS + 63) / 64;   // 6
static_assert(DSC_ROUNDS * 8 == DSC_BYTES, "six ballots are the descriptor");

// LDS written by one lane and read by another of the same wave: the order of fe_propagate.hpp
__device__ inline void dsc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(DSC_THREADS) describe_kernel(const DscParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t slab[DSC_WAVES][DSC_SLAB + 4];
  __shared__ int32_t val[DSC_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * DSC_WAVES + wave;
  if (row >= P.rows) return;   // the whole wave: no barrier follows
  const DscImage im = P.images[P.row_job[row]];
  float kx, ky;
  if (!dsc_keypoint(P, im, row, &kx, &ky)) return;
  uint64_t* out = reinterpret_cast<uint64_t*>(P.desc + (int64_t)DSC_BYTES * row);
  int32_t qx = 0, qy = 0;
  const bool valid = dsc_position(kx, ky, im.w, im.h, &qx, &qy);   // the same in every lane
  if (!valid) {
    if (lane < DSC_ROUNDS) out[lane] = 0;
    return;   // the flag keeps what the angle stage wrote
  }
  // the slab: pixel (0, 0) is image pixel (ix - 12, iy - 12); VALID puts ix - 12 >= -1 and ix + 12 <= w: clamped at both ends, and
  // what a clamped pixel holds is never weighted
  const int ix = (qx + 8) >> 4, iy = (qy + 8) >> 4;
  const uint8_t* src = P.pix + im.pix;
  uint8_t* mine = slab[wave];
#pragma unroll
  for (int t = 0; t < (DSC_PATCH * DSC_PATCH + 63) / 64; ++t) {
    const int i = t * 64 + lane;
    if (i < DSC_PATCH * DSC_PATCH) {
      const int py = i / DSC_PATCH, px = i - py * DSC_PATCH;
      int x = ix - DSC_PATCH_HALF + px, y = iy - DSC_PATCH_HALF + py;
      x = x < 0 ? 0 : (x > im.w - 1 ? im.w - 1 : x), y = y < 0 ? 0 : (y > im.h - 1 ? im.h - 1 : y);
      mine[py * DSC_PSTRIDE + px] = src[(int64_t)y * im.w + x];
    }
  }
  const int32_t rot = P.rot[row] & (DSC_ROTS - 1);   // checked on the host (rot_in) or made by dsc_rot
  const int32_t c = dsc_dev::dsc_cs[rot][0], s = dsc_dev::dsc_cs[rot][1];
  dsc_wave_sync();   // the slab is the wave's own: what its lanes wrote is read by other lanes of the same wave only
  const int k = lane < DSC_POINTS ? lane : 0;
  int32_t cx, cy;
  dsc_centre(c, s, k, qx - 16 * (ix - DSC_PATCH_HALF), qy - 16 * (iy - DSC_PATCH_HALF), &cx, &cy);
  const int32_t hw = dsc_dev::dsc_half[dsc_dev::dsc_ring[k]];
  val[wave][lane] = dsc_sample(mine, DSC_PSTRIDE, DSC_PATCH - 1, DSC_PATCH - 1, cx, cy, hw);
  dsc_wave_sync();
#pragma unroll
  for (int r = 0; r < DSC_ROUNDS; ++r) {
    const int b = 64 * r + lane;
    const int bb = b < DSC_PAIRS ? b : 0;
    const int i = dsc_dev::dsc_pairs[bb][0], j = dsc_dev::dsc_pairs[bb][1];
    const int32_t hi = dsc_dev::dsc_half[dsc_dev::dsc_ring[i]], hj = dsc_dev::dsc_half[dsc_dev::dsc_ring[j]];
    const bool bit = b < DSC_PAIRS && dsc_bit(val[wave][i], hi, val[wave][j], hj);
    const uint64_t word = __ballot(bit);
    if (lane == r) out[r] = word;
  }
  if (lane == 0) P.flags[row] |= DSC_VALID;
}
#endif  // __HIPCC__

}  // namespace fe
