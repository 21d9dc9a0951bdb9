// Recorder of tests/golden/sac_consensus.npz (driven by make_sac_consensus_golden.py; no test runs it).  Compiles the reference's
// two RANSAC adapters (okvis_frontend/src/FrameNoncentralAbsoluteAdapter.cpp, FrameRelativeAdapter.cpp) where they lie, unmodified,
// includes its three sample-consensus problems (okvis_frontend/include/opengv/sac_problems/.../Frame*SacProblem.hpp) and links
// the reference's own okvis::Estimator from oracle/_ref/obj.  A scene of two multi-frames with two cameras, keypoints, landmarks and
// observations is put into that estimator the way the frontend leaves it; then
//   - the adapters are constructed, and what they hold per correspondence is written out (bearing vectors, sigma angles, points,
//     camera and keypoint indices);
//   - every hypothesis of the case file goes through getSelectedDistancesToModel of the problem of its kind, and every score is
//     written out, with countWithinDistance for every hypothesis and selectWithinDistance for the best one.
// OpenGV is not installed and its source is not part of the reference tree.  What the three problems need from it to link is
// defined here, as this file's own code:
//   - SampleConsensusProblem<M>::getDistancesToModel / countWithinDistance / selectWithinDistance by the published rule (a
//     correspondence is an inlier when its score is < the threshold, strictly);
//   - opengv::triangulation::triangulate2 as the published two-view midpoint method.  The relative-pose scores of the fixture
//     therefore pin everything EXCEPT that function (pinned = 0 in the npz);
//   - the solver-side virtuals, which nothing here calls, as functions that abort.
//
//   recorder <case.bin> <out.bin>
// case.bin: int32 distortion (NCameraSystem::DistortionType), n_kp[4] (frame A cam 0, A cam 1, B cam 0, B cam 1), n_landmarks,
//           K_abs, K_rot, K_rel; double threshold; double intr[12] (fu fv cu cv d0..d7); double T_SC[2][7] (r, q xyzw);
//           per image: float kp[n][3] (x, y, size), int32 landmark[n] (-1 = none); double hp[n_landmarks][4];
//           double models_abs[K_abs][12]; per camera: double models_rot[K_rot][9], models_rel[K_rel][12]
// out.bin:  absolute: int32 n; per correspondence double bearing[3], point[3], sigma, int32 cam, keypoint; double offsets[2][3],
//           rotations[2][9]; double scores[K_abs][n]; int32 counts[K_abs]; int32 best, n_inliers, inliers[n_inliers]
//           per camera: int32 n; per match int32 idxA, idxB, double bearing1[3], bearing2[3], sigma1, sigma2; then for rotation-only
//           and for relative: scores[K][n], counts[K], best, n_inliers, inliers
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include <okvis/Estimator.hpp>
#include <okvis/cameras/EquidistantDistortion.hpp>
#include <okvis/cameras/NCameraSystem.hpp>
#include <okvis/cameras/PinholeCamera.hpp>
#include <okvis/cameras/RadialTangentialDistortion.hpp>
#include <okvis/cameras/RadialTangentialDistortion8.hpp>
#include <opengv/sac_problems/absolute_pose/FrameAbsolutePoseSacProblem.hpp>
#include <opengv/sac_problems/relative_pose/FrameRelativePoseSacProblem.hpp>
#include <opengv/sac_problems/relative_pose/FrameRotationOnlySacProblem.hpp>

namespace google {
int eshim_log_warnings = 0;
}

// ---- what the problems need from OpenGV to link (see the head of this file) ----------------------------------------------------------
namespace opengv {
namespace sac {
template <typename M>
void SampleConsensusProblem<M>::getSamples(int&, std::vector<int>&) { std::abort(); }
template <typename M>
bool SampleConsensusProblem<M>::isSampleGood(const std::vector<int>&) const { std::abort(); }
template <typename M>
void SampleConsensusProblem<M>::getDistancesToModel(const M& model, std::vector<double>& distances) {
  getSelectedDistancesToModel(model, *indices_, distances);
}
template <typename M>
void SampleConsensusProblem<M>::selectWithinDistance(const M& model, const double threshold, std::vector<int>& inliers) {
  std::vector<double> d;
  d.reserve(indices_->size());
  getDistancesToModel(model, d);
  inliers.clear();
  for (size_t i = 0; i < d.size(); ++i)
    if (d[i] < threshold) inliers.push_back((*indices_)[i]);
}
template <typename M>
int SampleConsensusProblem<M>::countWithinDistance(const M& model, const double threshold) {
  std::vector<double> d;
  d.reserve(indices_->size());
  getDistancesToModel(model, d);
  int n = 0;
  for (size_t i = 0; i < d.size(); ++i)
    if (d[i] < threshold) ++n;
  return n;
}
template <typename M>
void SampleConsensusProblem<M>::setUniformIndices(int N) {
  indices_.reset(new std::vector<int>((size_t)N));
  for (int i = 0; i < N; ++i) (*indices_)[(size_t)i] = i;
}
template class SampleConsensusProblem<transformation_t>;
template class SampleConsensusProblem<rotation_t>;
}  // namespace sac
namespace sac_problems {
namespace absolute_pose {
bool AbsolutePoseSacProblem::computeModelCoefficients(const std::vector<int>&, model_t&) const { std::abort(); }
void AbsolutePoseSacProblem::getSelectedDistancesToModel(const model_t&, const std::vector<int>&, std::vector<double>&) const { std::abort(); }
void AbsolutePoseSacProblem::optimizeModelCoefficients(const std::vector<int>&, const model_t&, model_t&) { std::abort(); }
int AbsolutePoseSacProblem::getSampleSize() const { std::abort(); }
}  // namespace absolute_pose
namespace relative_pose {
bool CentralRelativePoseSacProblem::computeModelCoefficients(const std::vector<int>&, model_t&) const { std::abort(); }
void CentralRelativePoseSacProblem::getSelectedDistancesToModel(const model_t&, const std::vector<int>&, std::vector<double>&) const { std::abort(); }
void CentralRelativePoseSacProblem::optimizeModelCoefficients(const std::vector<int>&, const model_t&, model_t&) { std::abort(); }
int CentralRelativePoseSacProblem::getSampleSize() const { std::abort(); }
bool RotationOnlySacProblem::computeModelCoefficients(const std::vector<int>&, model_t&) const { std::abort(); }
void RotationOnlySacProblem::getSelectedDistancesToModel(const model_t&, const std::vector<int>&, std::vector<double>&) const { std::abort(); }
void RotationOnlySacProblem::optimizeModelCoefficients(const std::vector<int>&, const model_t&, model_t&) { std::abort(); }
int RotationOnlySacProblem::getSampleSize() const { std::abort(); }
}  // namespace relative_pose
}  // namespace sac_problems
namespace triangulation {
// The two-view midpoint method: f2' = R12 f2; the points lambda1 f1 and t12 + lambda2 f2' closest to each other solve
// [f1.f1  -f1.f2'; f1.f2'  -f2'.f2'] (lambda1, lambda2)^T = (t12.f1, t12.f2')^T; the result is their mean.  Plain doubles, every
// product and sum on its own, sums from left to right.
point_t triangulate2(const relative_pose::RelativeAdapterBase& adapter, size_t index) {
  const translation_t t12 = adapter.gett12();
  const rotation_t R12 = adapter.getR12();
  const bearingVector_t v1 = adapter.getBearingVector1(index), v2 = adapter.getBearingVector2(index);
  const double t[3] = {t12[0], t12[1], t12[2]}, f1[3] = {v1[0], v1[1], v1[2]}, f2[3] = {v2[0], v2[1], v2[2]};
  double g[3];
  for (int k = 0; k < 3; ++k) g[k] = (R12(k, 0) * f2[0] + R12(k, 1) * f2[1]) + R12(k, 2) * f2[2];
  auto dot = [](const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; };
  const double b0 = dot(t, f1), b1 = dot(t, g);
  const double a00 = dot(f1, f1), a10 = dot(f1, g), a01 = -a10, a11 = -dot(g, g);
  const double det = a00 * a11 - a01 * a10;
  const double l0 = (a11 * b0 - a01 * b1) / det, l1 = (a00 * b1 - a10 * b0) / det;
  point_t p;
  for (int k = 0; k < 3; ++k) p[k] = (l0 * f1[k] + (t[k] + l1 * g[k])) / 2.0;
  return p;
}
}  // namespace triangulation
}  // namespace opengv

namespace {

bool rd(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
void wr(std::FILE* f, const void* p, size_t n) {
  if (n && std::fwrite(p, 1, n, f) != n) std::abort();
}
void wr_i(std::FILE* f, int32_t v) { wr(f, &v, sizeof(v)); }
void wr_v(std::FILE* f, const Eigen::Vector3d& v) {
  const double d[3] = {v[0], v[1], v[2]};
  wr(f, d, sizeof(d));
}

const uint64_t FRAME_ID[2] = {101, 102};

template <class D>
std::shared_ptr<const okvis::cameras::CameraBase> make_camera(const double* k);
template <>
std::shared_ptr<const okvis::cameras::CameraBase> make_camera<okvis::cameras::RadialTangentialDistortion>(const double* k) {
  return std::shared_ptr<const okvis::cameras::CameraBase>(new okvis::cameras::PinholeCamera<okvis::cameras::RadialTangentialDistortion>(
      752, 480, k[0], k[1], k[2], k[3], okvis::cameras::RadialTangentialDistortion(k[4], k[5], k[6], k[7])));
}
template <>
std::shared_ptr<const okvis::cameras::CameraBase> make_camera<okvis::cameras::EquidistantDistortion>(const double* k) {
  return std::shared_ptr<const okvis::cameras::CameraBase>(new okvis::cameras::PinholeCamera<okvis::cameras::EquidistantDistortion>(
      752, 480, k[0], k[1], k[2], k[3], okvis::cameras::EquidistantDistortion(k[4], k[5], k[6], k[7])));
}
template <>
std::shared_ptr<const okvis::cameras::CameraBase> make_camera<okvis::cameras::RadialTangentialDistortion8>(const double* k) {
  return std::shared_ptr<const okvis::cameras::CameraBase>(new okvis::cameras::PinholeCamera<okvis::cameras::RadialTangentialDistortion8>(
      752, 480, k[0], k[1], k[2], k[3], okvis::cameras::RadialTangentialDistortion8(k[4], k[5], k[6], k[7], k[8], k[9], k[10], k[11])));
}

// scores of every hypothesis, countWithinDistance of every hypothesis, selectWithinDistance of the first hypothesis with the largest count
template <class PROBLEM, class MODEL>
void record(std::FILE* out, PROBLEM& problem, int n, const std::vector<MODEL>& models, double threshold) {
  problem.setUniformIndices(n);
  std::vector<int> indices((size_t)n);
  for (int i = 0; i < n; ++i) indices[(size_t)i] = i;
  std::vector<int32_t> counts;
  for (const MODEL& m : models) {
    std::vector<double> scores;
    problem.getSelectedDistancesToModel(m, indices, scores);
    if ((int)scores.size() != n) std::abort();
    wr(out, scores.data(), sizeof(double) * scores.size());
  }
  int best = 0;
  for (size_t k = 0; k < models.size(); ++k) {
    counts.push_back(problem.countWithinDistance(models[k], threshold));
    if (counts[k] > counts[(size_t)best]) best = (int)k;
  }
  wr(out, counts.data(), sizeof(int32_t) * counts.size());
  std::vector<int> inliers;
  problem.selectWithinDistance(models[(size_t)best], threshold, inliers);
  wr_i(out, best);
  wr_i(out, (int32_t)inliers.size());
  for (int i : inliers) wr_i(out, i);
}

template <class D>
int run(std::FILE* in, std::FILE* out, const int32_t* h, okvis::cameras::NCameraSystem::DistortionType type) {
  typedef okvis::cameras::PinholeCamera<D> Camera;
  const int n_lm = h[5], K_abs = h[6], K_rot = h[7], K_rel = h[8];
  double threshold, intr[12], T_SC_raw[2][7];
  if (!rd(in, &threshold, sizeof(threshold)) || !rd(in, intr, sizeof(intr)) || !rd(in, T_SC_raw, sizeof(T_SC_raw))) return 2;
  okvis::cameras::NCameraSystem ncs;
  std::vector<std::shared_ptr<const okvis::kinematics::Transformation> > T_SC;
  std::shared_ptr<const okvis::cameras::CameraBase> geometry = make_camera<D>(intr);
  for (int i = 0; i < 2; ++i) {
    const double* t = T_SC_raw[i];
    T_SC.push_back(std::shared_ptr<const okvis::kinematics::Transformation>(
        new okvis::kinematics::Transformation(Eigen::Vector3d(t[0], t[1], t[2]), Eigen::Quaterniond(t[6], t[3], t[4], t[5]))));
    ncs.addCamera(T_SC[(size_t)i], geometry, type, false);
  }
  okvis::Estimator est;
  okvis::ExtrinsicsEstimationParameters ext(0, 0, 0, 0);
  est.addCamera(ext);
  est.addCamera(ext);
  okvis::ImuParameters imu;
  imu.a_max = 1000.0, imu.g_max = 1000.0, imu.sigma_g_c = 6.0e-4, imu.sigma_a_c = 2.0e-3, imu.sigma_bg = 0.03;
  imu.sigma_ba = 0.1, imu.sigma_gw_c = 3.0e-6, imu.sigma_aw_c = 2.0e-5, imu.tau = 3600.0, imu.g = 9.81;
  imu.a0 = Eigen::Vector3d(0, 0, 0);
  imu.rate = 100;
  est.addImu(imu);
  const double DT = 0.01, FRAME_DT = 0.5;
  okvis::ImuMeasurementDeque stream;
  for (int i = 0; i < 60; ++i)
    stream.push_back(okvis::ImuMeasurement(okvis::Time(1, 0) + okvis::Duration((i - 2) * DT),
                                           okvis::ImuSensorReadings(Eigen::Vector3d(0, 0, 0), Eigen::Vector3d(0, 0, imu.g))));
  okvis::MultiFramePtr mf[2];
  for (int f = 0; f < 2; ++f) {
    const okvis::Time t = okvis::Time(1, 0) + okvis::Duration(f * FRAME_DT);
    mf[f].reset(new okvis::MultiFrame(ncs, t, FRAME_ID[f]));
    okvis::ImuMeasurementDeque d;
    for (const okvis::ImuMeasurement& m : stream)
      if (m.timeStamp >= (f ? t - okvis::Duration(FRAME_DT + 0.02) : t - okvis::Duration(0.02)) && m.timeStamp <= t + okvis::Duration(0.03))
        d.push_back(m);
    if (!est.addStates(mf[f], d, f == 0)) return std::printf("addStates failed\n"), 3;
  }
  // keypoints, and which landmark each one shows
  std::vector<int32_t> lm_of[2][2];
  for (int f = 0; f < 2; ++f)
    for (int c = 0; c < 2; ++c) {
      const int n = h[1 + 2 * f + c];
      std::vector<float> kp(3 * (size_t)n);
      lm_of[f][c].resize((size_t)n);
      if (!rd(in, kp.data(), sizeof(float) * kp.size()) || !rd(in, lm_of[f][c].data(), sizeof(int32_t) * (size_t)n)) return 2;
      std::vector<cv::KeyPoint> kps;
      for (int k = 0; k < n; ++k) kps.push_back(cv::KeyPoint(kp[3 * k], kp[3 * k + 1], kp[3 * k + 2]));
      mf[f]->resetKeypoints((size_t)c, kps);
    }
  std::vector<double> hp(4 * (size_t)n_lm);
  if (!rd(in, hp.data(), sizeof(double) * hp.size())) return 2;
  const uint64_t LM0 = 5000;
  for (int j = 0; j < n_lm; ++j)
    if (!est.addLandmark(LM0 + (uint64_t)j, Eigen::Vector4d(hp[4 * j], hp[4 * j + 1], hp[4 * j + 2], hp[4 * j + 3]))) return std::printf("addLandmark failed\n"), 3;
  for (int f = 0; f < 2; ++f)
    for (int c = 0; c < 2; ++c)
      for (size_t k = 0; k < lm_of[f][c].size(); ++k) {
        if (lm_of[f][c][k] < 0) continue;
        const uint64_t id = LM0 + (uint64_t)lm_of[f][c][k];
        mf[f]->setLandmarkId((size_t)c, k, id);   // (the matching algorithm's setBestMatch does both)
        if (est.template addObservation<Camera>(id, FRAME_ID[f], (size_t)c, k) == 0) return std::printf("addObservation failed\n"), 3;
      }
  // hypotheses
  std::vector<opengv::transformation_t> models_abs((size_t)K_abs);
  auto read34 = [&](opengv::transformation_t& T) {
    double m[12];
    if (!rd(in, m, sizeof(m))) return false;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) T(i, j) = m[4 * i + j];
    return true;
  };
  for (auto& T : models_abs)
    if (!read34(T)) return 2;

  // ---- 3D-2D: the new frame against the map (Frontend.cpp:575-642) ----
  {
    opengv::absolute_pose::FrameNoncentralAbsoluteAdapter adapter(est, ncs, mf[1]);
    const int n = (int)adapter.getNumberCorrespondences();
    wr_i(out, n);
    for (int i = 0; i < n; ++i) {
      wr_v(out, adapter.getBearingVector((size_t)i));
      wr_v(out, adapter.getPoint((size_t)i));
      const double s = adapter.getSigmaAngle((size_t)i);
      wr(out, &s, sizeof(s));
      wr_i(out, adapter.camIndex((size_t)i));
      wr_i(out, adapter.keypointIndex((size_t)i));
    }
    // getCamOffset / getCamRotation take a correspondence; the cameras themselves are what the adapter copied from T_SC
    for (int c = 0; c < 2; ++c) wr_v(out, mf[1]->T_SC((size_t)c)->r());
    for (int c = 0; c < 2; ++c) {
      const Eigen::Matrix3d C = mf[1]->T_SC((size_t)c)->C();
      double m[9];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) m[3 * i + j] = C(i, j);
      wr(out, m, sizeof(m));
    }
    for (int i = 0; i < n; ++i) {   // ... and they are what the accessors return
      const int c = adapter.camIndex((size_t)i);
      if ((adapter.getCamOffset((size_t)i) - mf[1]->T_SC((size_t)c)->r()).norm() != 0.0 ||
          (adapter.getCamRotation((size_t)i) - mf[1]->T_SC((size_t)c)->C()).norm() != 0.0)
        return std::printf("camera accessors\n"), 4;
    }
    opengv::sac_problems::absolute_pose::FrameAbsolutePoseSacProblem problem(
        adapter, opengv::sac_problems::absolute_pose::FrameAbsolutePoseSacProblem::Algorithm::GP3P);
    record(out, problem, n, models_abs, threshold);
  }
  // ---- 2D-2D per camera: rotation only, then the relative pose (Frontend.cpp:645-810) ----
  for (int c = 0; c < 2; ++c) {
    std::vector<opengv::rotation_t> models_rot((size_t)K_rot);
    std::vector<opengv::transformation_t> models_rel((size_t)K_rel);
    for (auto& R : models_rot) {
      double m[9];
      if (!rd(in, m, sizeof(m))) return 2;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R(i, j) = m[3 * i + j];
    }
    for (auto& T : models_rel)
      if (!read34(T)) return 2;
    opengv::relative_pose::FrameRelativeAdapter adapter(est, ncs, FRAME_ID[0], (size_t)c, FRAME_ID[1], (size_t)c);
    const int n = (int)adapter.getNumberCorrespondences();
    wr_i(out, n);
    for (int i = 0; i < n; ++i) {
      wr_i(out, (int32_t)adapter.getMatchKeypointIdxA((size_t)i));
      wr_i(out, (int32_t)adapter.getMatchKeypointIdxB((size_t)i));
      wr_v(out, adapter.getBearingVector1((size_t)i));
      wr_v(out, adapter.getBearingVector2((size_t)i));
      const double s[2] = {adapter.getSigmaAngle1((size_t)i), adapter.getSigmaAngle2((size_t)i)};
      wr(out, s, sizeof(s));
    }
    opengv::sac_problems::relative_pose::FrameRotationOnlySacProblem rotation_only(adapter);
    record(out, rotation_only, n, models_rot, threshold);
    opengv::sac_problems::relative_pose::FrameRelativePoseSacProblem relative(
        adapter, opengv::sac_problems::relative_pose::FrameRelativePoseSacProblem::Algorithm::STEWENIUS);
    record(out, relative, n, models_rel, threshold);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t h[9];
  if (!rd(in, h, sizeof(h))) return 2;
  int rc = 2;
  typedef okvis::cameras::NCameraSystem N;
  if (h[0] == (int)N::RadialTangential) rc = run<okvis::cameras::RadialTangentialDistortion>(in, out, h, N::RadialTangential);
  else if (h[0] == (int)N::Equidistant) rc = run<okvis::cameras::EquidistantDistortion>(in, out, h, N::Equidistant);
  else if (h[0] == (int)N::RadialTangential8) rc = run<okvis::cameras::RadialTangentialDistortion8>(in, out, h, N::RadialTangential8);
  std::fclose(in);
  if (std::fclose(out) != 0) return 2;
  return rc;
}
