/*
 * okvis_amd_frontend.h — C-ABI of the batched reprojection and matching pieces of the OKVIS frontend.
 *
 * The frontend calls the backend's reprojection algebra once per candidate match, one at a time, from the matcher's inner
 * loop.  These entries do the same arithmetic for ALL candidates of one (frame A, frame B, camera pair) in one launch:
 *
 *   okvis_fe_stereo_triangulate  ProbabilisticStereoTriangulator<G>::resetFrames / stereoTriangulate / getUncertainty
 *                                (okvis_frontend/src/ProbabilisticStereoTriangulator.cpp:127-170, 178-250, 253-355, 358-385;
 *                                 triangulateFast: okvis_frontend/src/stereo_triangulation.cpp:50-137)
 *   okvis_fe_project_landmarks   VioKeyframeWindowMatchingAlgorithm<G>::doSetup, Match3D2D branch
 *                                (okvis_frontend/src/VioKeyframeWindowMatchingAlgorithm.cpp:165-213)
 *   okvis_fe_gate_3d2d           ... ::verifyMatch (:320-337) and the gate of ::setBestMatch (:494-512)
 *
 * and the matching itself, for binary descriptors of 16, 32, 48 (BRISK) or 64 bytes under the Hamming distance:
 *
 *   okvis_fe_hamming_candidates  every pair of keypoints whose descriptors are closer than a threshold, in ascending (a, b) order
 *                                (the double loop a matching algorithm's doSetup would run on the host)
 *   okvis_fe_match_descriptors   okvis::DenseMatcher::match with ONE matcher thread, for many image pairs per call
 *                                (okvis_matcher/include/okvis/implementation/DenseMatcher.hpp:47-225, okvis_matcher/src/DenseMatcher.cpp:69-111)
 *   okvis_fe_match_verified      the same matcher under the distance the frontend really uses, "Hamming distance under the threshold
 *                                and verifyMatch(a, b)": whole 3D-2D and 2D-2D matching steps, projection, gating / triangulation and
 *                                the accepted pairs' setBestMatch quantities included, many steps per call
 *                                (okvis_frontend/src/VioKeyframeWindowMatchingAlgorithm.cpp:165-213, 307-337, 377-394, 485-508)
 *
 * and the arithmetic of the outlier rejection that follows the matching (Frontend::runRansac3d2d / runRansac2d2d,
 * okvis_frontend/src/Frontend.cpp:575-642, 645-810):
 *
 *   okvis_fe_bearing_vectors     what the two RANSAC adapters hold per keypoint: backProject, normalize(), sigmaAngle
 *                                (okvis_frontend/src/FrameNoncentralAbsoluteAdapter.cpp:51-162, FrameRelativeAdapter.cpp:52-245)
 *   okvis_fe_sac_consensus       getSelectedDistancesToModel / countWithinDistance / selectWithinDistance of the three sample-consensus
 *                                problems, for all hypotheses of many problems per call
 *                                (okvis_frontend/include/opengv/sac_problems/absolute_pose/FrameAbsolutePoseSacProblem.hpp:129-161,
 *                                 .../relative_pose/FrameRotationOnlySacProblem.hpp:122-144, .../relative_pose/FrameRelativePoseSacProblem.hpp:126-161)
 *
 *   okvis_fe_sac_solve           the two minimal solvers of runRansac2d2d (two-point rotation, five-point relative pose) for all samples
 *                                of many problems per call, chained into the consensus kernel: sample indices in, inlier sets out.
 *                                Stated from their published definitions, not pinned to OpenGV
 *
 *   okvis_fe_sac_solve_absolute  the minimal solver of runRansac3d2d (generalised three-point absolute pose over several cameras) for all
 *                                samples of many problems per call, chained into the consensus kernel in the same way.  Stated from
 *                                its mathematical definition, not pinned to OpenGV
 *
 *   okvis_fe_ransac              whole sample-consensus runs (opengv::sac::Ransac<P>::computeModel as runRansac3d2d / runRansac2d2d call
 *                                it): the sampler and the adaptive loop on the device around the three solvers and the consensus kernel,
 *                                all runs of a frame in one call, correspondences in, inlier set and model out.  Stated in this header,
 *                                not pinned to OpenGV
 *
 * optimizeModelCoefficients is OpenGV's and is not here (the reference's frontend never calls it).  okvis_fe_sac_consensus takes its
 * hypotheses from the caller, okvis_fe_sac_solve and okvis_fe_sac_solve_absolute their samples; okvis_fe_ransac draws its own.
 *
 * and the state propagation that every layer around the backend calls:
 *
 *   okvis_fe_imu_propagate       ImuError::propagation with covariance and Jacobian (okvis_ceres/src/ImuError.cpp:287-504), for the
 *                                chains of calls of many sequences per call: the per-frame call of Estimator::addStates
 *                                (okvis_ceres/src/Estimator.cpp:145-147) and ThreadedKFVio::frameConsumerLoop
 *                                (okvis_multisensor_processing/src/ThreadedKFVio.cpp:416-418), and the IMU-rate chain of
 *                                ThreadedKFVio::imuConsumerLoop through Frontend::propagation (:559-598, Frontend.cpp:274-292)
 *
 * and the decision that consumes the matching's result:
 *
 *   okvis_fe_keyframe_decision   Frontend::doWeNeedANewKeyframe (okvis_frontend/src/Frontend.cpp:295-369): per camera image the convex
 *                                hulls of all and of the matched keypoints, their areas, the keypoints inside the matched hull, and
 *                                the decision per multiframe, many multiframes per call; exact (hull, area and inside test are stated
 *                                from their definitions, see the entry)
 *
 * and the first thing the pipeline does with a frame:
 *
 *   okvis_fe_detect_keypoints    the detector of Frontend::detectAndDescribe (okvis_frontend/src/Frontend.cpp:92-114) under the shipped
 *                                configuration (octaves 0): Harris scores on the full-resolution 8-bit image, 3 x 3 maxima above an
 *                                absolute threshold, greedy selection of the strongest that keeps them min_dist apart, many images
 *                                per call; exact integer arithmetic.  Stated in this header, not pinned to BRISK
 *
 *   okvis_fe_describe_keypoints  Frame::describe (okvis_cv/include/okvis/implementation/Frame.hpp:128-156) behind the detector: the keypoint's
 *                                angle from the extraction direction (gravity in the camera frame) through the projection Jacobian, as
 *                                the reference computes it, and a 48-byte binary descriptor at that angle and a fixed scale, many
 *                                images per call; every descriptor byte exact.  The extractor is stated in this header from the
 *                                published BRISK construction, not pinned to BRISK
 *   okvis_fe_detect_and_describe the whole of Frontend::detectAndDescribe: the two entries above in one call, the images staged once,
 *                                the describe kernels reading the selected keypoints where the detect kernels left them
 *   okvis_fe_detect_keypoints_scaled, okvis_fe_detect_scaled_and_describe   the same two with the detection option octaves > 0: the
 *                                detector on every layer of a half-sampled pyramid, a raw score comparison across layers, the layer
 *                                and a linear scale interpolation in kp.size; exact.  Stated in this header, not pinned to BRISK
 *
 * What stays with the caller is what needs the estimator's book-keeping: which keypoints carry a landmark, addLandmark /
 * addObservation; and BRISK's own scale space and bit selection (intra-octaves, scale invariance).  G =PinholeCamera<D> with the distortion models of okvis_amd_ba.h.  The geometry is IEEE
 * double like the reference; keypoints are float like cv::KeyPoint; descriptor distances are integers, exact in float.
 * Plain pointers and sizes, int status codes (okvis_amd_ba.h), host buffers in and out; no CPU path.
 */
#ifndef OKVIS_AMD_FRONTEND_H_
#define OKVIS_AMD_FRONTEND_H_

#include <stdint.h>

#include "okvis_amd_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct okvis_fe_context okvis_fe_context; /* one HIP stream + device scratch that grows on demand */

/* PinholeCamera<D> (okvis_cv/include/okvis/cameras/PinholeCamera.hpp): what project / backProject read */
typedef struct okvis_fe_camera {
  double intr[12]; /* fu fv cu cv d0..d7 */
  int32_t model;   /* OKVIS_BA_DIST_* */
  int32_t width;   /* image size: CameraBase::isInImage (implementation/CameraBase.hpp:95-104) */
  int32_t height;
  int32_t reserved;
} okvis_fe_camera;

/* flags of okvis_fe_stereo_triangulate, one byte per candidate */
#define OKVIS_FE_TRI_VALID 1u           /* stereoTriangulate returned true (:178-236)                                   */
#define OKVIS_FE_TRI_NOT_PARALLEL 2u    /* outCanBeInitializedInaccuarate of the 5-argument overload = !isParallel (:208) */
#define OKVIS_FE_TRI_CAN_INIT 4u        /* outCanBeInitialized of the 6-argument overload (:239-250): getUncertainty's
                                           decision AND not parallel                                                    */
#define OKVIS_FE_TRI_RANK_DEFICIENT 8u  /* H.colPivHouseholderQr().rank() < 9 (:349-352): cov is not written            */

/* ProjectionStatus (okvis_cv/include/okvis/cameras/CameraBase.hpp:67-74) as okvis_fe_project_landmarks reports it */
#define OKVIS_FE_PROJ_SUCCESSFUL 0
#define OKVIS_FE_PROJ_OUTSIDE_IMAGE 1
#define OKVIS_FE_PROJ_MASKED 2 /* never produced: masks are not part of this interface */
#define OKVIS_FE_PROJ_BEHIND 3
#define OKVIS_FE_PROJ_INVALID 4

/* flags of okvis_fe_gate_3d2d */
#define OKVIS_FE_GATE_VERIFIED 1u  /* verifyMatch: (int)chi2 < 4 (:333-337)                                  */
#define OKVIS_FE_GATE_ACCEPTED 2u  /* setBestMatch does not return at chi2 > 4.0 (:505-508)                  */
#define OKVIS_FE_GATE_UNCERTAIN 4u /* U_tot.norm() > 25 / (sigma_B^2 sqrt 2): numUncertainMatches_++ (:511) */

int okvis_fe_create(okvis_fe_context** out, int device);
void okvis_fe_destroy(okvis_fe_context* ctx);

/* For every candidate (a, b) = pairs[i]: keypoint a of image A against keypoint b of image B.
 *   T_AB[7]     r, q(xyzw) of T_CaCb (resetFrames :127-136)
 *   UOplus[36]  6x6 covariance of T_AB in its tangent space (row-major, symmetric positive definite); the reference turns
 *               it into the Gauss-Newton block H_(0:6,0:6) through a PoseError linearised at T_AB (:142-160)
 *   kp_a/kp_b   [n][3] float: x, y, size of the cv::KeyPoints (sigma = 0.8 size / 12)
 *   sigma_ray   [n_pairs] or NULL; NULL or -1.0 = the triangulator's own 0.5 / min(fu_A, fu_B) (:162-166, :187-190)
 * Outputs (any may be NULL): hp_a [n_pairs][4] homogeneous point in A (written when VALID or when the reprojection check
 * is what failed, like the reference's out parameter), cov [n_pairs][9] row-major 3x3 UOplus of the point (written when
 * VALID and not RANK_DEFICIENT), flags [n_pairs].  want_uncertainty = 0 stops after stereoTriangulate (verifyMatch, :310-317). */
int okvis_fe_stereo_triangulate(okvis_fe_context* ctx, const okvis_fe_camera* cam_a, const okvis_fe_camera* cam_b,
                                const double* T_AB, const double* UOplus, int32_t n_a, const float* kp_a, int32_t n_b,
                                const float* kp_b, int32_t n_pairs, const int32_t* pairs, const double* sigma_ray,
                                int32_t want_uncertainty, double* hp_a, double* cov, uint8_t* flags);
/* The same call with one more output: gn [n_pairs][81] = the 9x9 Gauss-Newton matrix H of getUncertainty (:286-345; rows /
 * columns 0..5 the relative pose, 6..8 the point), row-major, zeros where getUncertainty does not run.  For referees of the
 * point covariance (tests/test_gpu_frontend.py inverts it in extended precision); NULL = okvis_fe_stereo_triangulate. */
int okvis_fe_stereo_triangulate_gn(okvis_fe_context* ctx, const okvis_fe_camera* cam_a, const okvis_fe_camera* cam_b,
                                const double* T_AB, const double* UOplus, int32_t n_a, const float* kp_a, int32_t n_b,
                                const float* kp_b, int32_t n_pairs, const int32_t* pairs, const double* sigma_ray,
                                int32_t want_uncertainty, double* hp_a, double* cov, uint8_t* flags, double* gn);

/* hp_W [n][4] through T_CbW [7] into camera B: uv [n][2] (written unless INVALID), U [n][4] = J P_C J^T row-major 2x2 with
 * P_C = P3 [9] (row-major 3x3, the top-left block of the relative pose uncertainty, :197-203), status [n]. */
int okvis_fe_project_landmarks(okvis_fe_context* ctx, const okvis_fe_camera* cam_b, const double* T_CbW, const double* P3,
                               int32_t n, const double* hp_W, double* uv, double* U, uint8_t* status);

/* candidates (a, b) = pairs[i]: projection a (uv, U from okvis_fe_project_landmarks) against keypoint b of image B.
 * chi2 [n_pairs] = err^T (sigma_B^2 I + U_a)^-1 err, flags [n_pairs]. */
int okvis_fe_gate_3d2d(okvis_fe_context* ctx, int32_t n_proj, const double* uv, const double* U, int32_t n_b,
                       const float* kp_b, int32_t n_pairs, const int32_t* pairs, double* chi2, uint8_t* flags);

/* Descriptors: desc_bytes = 16, 32, 48 or 64 (brisk::Hamming::PopcntofXORed with numberOf128BitWords 1..4), desc_a [n_a][desc_bytes],
 * desc_b [n_b][desc_bytes], row after row.  skip_a [n_a] / skip_b [n_b]: non-zero = the keypoint is out of play (skipA / skipB of
 * okvis::MatchingAlgorithm); NULL = none is.  At most 65536 keypoints per image.  An image without keypoints is valid.
 *
 * Every pair (a, b) of keypoints in play with (float)popcount(desc_a[a] ^ desc_b[b]) < threshold (strictly), in ascending (a, b)
 * order.  *n_pairs always receives the number of such pairs (INT32_MAX where it does not fit); pairs [capacity][2] and dist [capacity]
 * (may be NULL) receive the first min(capacity, total) of them.  A total above capacity is not an error: size the buffers by
 * *n_pairs and call again (capacity 0 only counts). */
int okvis_fe_hamming_candidates(okvis_fe_context* ctx, int32_t desc_bytes, int32_t n_a, const uint8_t* desc_a, const uint8_t* skip_a,
                                int32_t n_b, const uint8_t* desc_b, const uint8_t* skip_b, float threshold, int32_t capacity,
                                int32_t* pairs, float* dist, int32_t* n_pairs);

typedef struct okvis_fe_match_job { /* one (image A, image B) */
  int32_t n_a, n_b;
  const uint8_t *desc_a, *desc_b, *skip_a, *skip_b;
  int32_t* pair_a;   /* [n_b] out: vpairs[b].indexA after matchBody, -1 = unpaired      */
  float* pair_dist;  /* [n_b] out: vpairs[b].distance (FLT_MAX where unpaired)          */
  uint8_t* accepted; /* [n_b] out: 1 where matchBody would call setBestMatch(pair_a, b) */
} okvis_fe_match_job;

/* okvis::DenseMatcher(1, num_best, use_ratio).match(algorithm) for every job, where algorithm.distance(a, b) is the Hamming distance
 * of the two descriptors if that is < threshold and FLT_MAX otherwise, distanceThreshold() = threshold and distanceRatioThreshold()
 * = ratio_threshold.  The semantics are those of ONE matcher thread: the rows of A in ascending order, each row's list of its
 * num_best closest b built by scanning b in ascending order (a candidate enters only if strictly closer than the list's last entry,
 * in front of entries of its own distance), assignbest directly after the row's scan (a taker must be strictly closer to displace a
 * holder, who goes on from position 1 of its own list), then matchBody's final loop with, under use_ratio, the ratio rule on the
 * first two entries of the A row's list.  With several matcher threads the reference's result depends on their interleaving where
 * distances tie; integer distances tie often.
 * The distances and the per-row lists are computed on the device, one grid for all jobs of the call; the assignment chains are
 * sequential by nature and O(n_a num_best), and run on the host inside this entry, after the device's lists have come back.
 * num_best is 1..8; use_ratio needs num_best >= 2 (the rule reads list entry 1). */
int okvis_fe_match_descriptors(okvis_fe_context* ctx, int32_t n_jobs, const okvis_fe_match_job* jobs, int32_t desc_bytes,
                               float threshold, int32_t num_best, int32_t use_ratio, float ratio_threshold);

#define OKVIS_FE_MATCH_3D2D 1 /* VioKeyframeWindowMatchingAlgorithm::Match3D2D */
#define OKVIS_FE_MATCH_2D2D 2 /* ... ::Match2D2D */

typedef struct okvis_fe_vmatch_job { /* one matching step: (frame A, camera) against (frame B, camera) */
  int32_t kind;                      /* OKVIS_FE_MATCH_* */
  int32_t n_a, n_b;                  /* 0..65536 each; 0 is valid */
  const uint8_t *desc_a, *desc_b;    /* [n][desc_bytes] */
  const uint8_t *skip_a, *skip_b;    /* skipA / skipB as the host's doSetup book-keeping decided them; NULL = none */
  const float *kp_a, *kp_b;          /* [n][3] x, y, size (kp_a may be NULL for 3D2D) */
  okvis_fe_camera cam_a, cam_b;
  /* 3D2D: doSetup's projection loop (:165-213) runs inside the call */
  const double* hp_W; /* [n_a][4]; rows with skip_a set are not read */
  double T_CbW[7], P3[9];
  /* 2D2D */
  double T_AB[7], UOplus[36];
  /* out; every pointer may be NULL except pair_a / pair_dist / accepted when n_b > 0 */
  int32_t* pair_a;      /* [n_b], as okvis_fe_match_job */
  float* pair_dist;
  uint8_t* accepted;
  uint8_t* proj_status; /* 3D2D, [n_a]: what okvis_fe_project_landmarks returns for the rows in play, zeros for rows with skip_a set */
  double *uv, *U;       /*       [n_a][2], [n_a][4] */
  double* chi2;         /* 3D2D, [n_b]: okvis_fe_gate_3d2d of (pair_a[b], b) where accepted, zero elsewhere */
  uint8_t* gate_flags;
  double *hp_a, *cov;   /* 2D2D, [n_b][4], [n_b][9]: okvis_fe_stereo_triangulate(want_uncertainty = 1, sigma_ray = the pair's ray
                           sigma) of (pair_a[b], b) where accepted, zero elsewhere */
  uint8_t* tri_flags;
} okvis_fe_vmatch_job;

/* Whole matching steps of the frontend: matcher_->match<VioKeyframeWindowMatchingAlgorithm<G>>(alg) for every job.  The semantics
 * are those of okvis_fe_match_descriptors (ONE matcher thread, the same list and tie rules, assignbest and matchBody's final loop on
 * the host inside this entry, num_best 1..8, the ratio rule needs num_best >= 2) under the distance the reference's algorithm defines
 * (VioKeyframeWindowMatchingAlgorithm.hpp, distance): the Hamming distance d if d < threshold AND verifyMatch(a, b), FLT_MAX otherwise.
 *   2D2D  verifyMatch = stereoTriangulate(a, b, ., ., sigma) returns valid (OKVIS_FE_TRI_VALID of the 5-argument path,
 *         ProbabilisticStereoTriangulator.cpp:178-236) with sigma = max(raySigmaA[a], raySigmaB[b]) and
 *         raySigma[k] = sqrt(sqrt(2)) * (0.8 * size_k / 12) / fu in double, in this operation order (:210-221, :251-261).
 *   3D2D  a row a is in play only if skip_a[a] is clear and its projection is OKVIS_FE_PROJ_SUCCESSFUL (:186-192); verifyMatch =
 *         OKVIS_FE_GATE_VERIFIED of the gate on uv[a], U[a], kp_b[b]: (int)chi2 < 4 (:318-337).  proj_status lets the caller apply
 *         doSetup's side effect setLandmarkInitialized(id, false) for rows with fewer than two observations (:194-198); the caller
 *         knows those rows beforehand and also sets them in skip_a.
 * For every b with accepted[b] the outputs carry what setBestMatch computes again for that pair (:377-394, :485-508), so that the
 * caller goes on with addLandmark / addObservation / setLandmark without another call.
 * Jobs of one call are INDEPENDENT of each other: the caller batches only steps whose skip masks do not depend on each other's
 * result — the two cameras of matchToKeyframes against one keyframe, the same step of several sequences.  Kinds may be mixed.
 * The per-keypoint work, the distances, the verification and the per-row lists run on the device (two launches for all jobs of the
 * call); the uncertainty of the accepted 2D2D pairs (at most n_b per job) is one more launch per such job, after the host's chains.
 * OKVIS_BA_ERR_ARG before the context is read or the device is touched: NULL context, desc_bytes outside {16, 32, 48, 64}, sizes
 * outside 0..65536, num_best outside 1..8, use_ratio with num_best < 2, kind outside {1, 2}, a camera with a non-positive focal
 * length or image size or an unknown model, a NULL required pointer (kp_b always, kp_a for 2D2D, hp_W for 3D2D with n_a > 0, the
 * descriptors, pair_a / pair_dist / accepted with n_b > 0), UOplus not positive definite for 2D2D when hp_a, cov or tri_flags is
 * wanted. */
int okvis_fe_match_verified(okvis_fe_context* ctx, int32_t n_jobs, const okvis_fe_vmatch_job* jobs, int32_t desc_bytes,
                            float threshold, int32_t num_best, int32_t use_ratio, float ratio_threshold);

/* kp [n][3] float (x, y, size) through cam: bearing [n][3] = backProject(kp) (implementation/PinholeCamera.hpp:426-446 and the
 * distortion's undistort), normalised; sigma_angle [n] = sqrt(2) (0.8 size / 12)^2 / fu^2 with fu = cam->intr[0]; ok [n] =
 * backProject's return value (the adapters ignore it).  FrameNoncentralAbsoluteAdapter.cpp:96-149, FrameRelativeAdapter.cpp:168-244.
 * All four OKVIS_BA_DIST_* models (the reference adapters throw on NoDistortion).  Any output may be NULL; n = 0 is valid. */
int okvis_fe_bearing_vectors(okvis_fe_context* ctx, const okvis_fe_camera* cam, int32_t n, const float* kp, double* bearing,
                             double* sigma_angle, uint8_t* ok);

#define OKVIS_FE_SAC_ABSOLUTE 0      /* FrameAbsolutePoseSacProblem: world points against bearing vectors, several cameras       */
#define OKVIS_FE_SAC_ROTATION_ONLY 1 /* FrameRotationOnlySacProblem: bearing vectors of two frames under a rotation              */
#define OKVIS_FE_SAC_RELATIVE 2      /* FrameRelativePoseSacProblem: bearing vectors of two frames under a relative pose         */

typedef struct okvis_fe_sac_job { /* one sample-consensus problem with its hypotheses */
  int32_t kind;     /* OKVIS_FE_SAC_*                                                                           */
  int32_t n;        /* correspondences, 0..65536                                                                */
  int32_t n_models; /* hypotheses, 1..1024 (the reference runs at most 50 iterations)                           */
  int32_t n_cams;   /* absolute: 1..8                                                                           */
  double threshold; /* the reference uses 9                                                                     */
  const double* models; /* [n_models][12] row-major 3x4 transformation_t (absolute, relative) or [n_models][9] rotation_t */
  /* absolute only */
  const double* points;        /* [n][3]      getPoint                                     */
  const double* bearing;       /* [n][3]      getBearingVector                             */
  const double* sigma;         /* [n]         getSigmaAngle                                */
  const int32_t* cam_index;    /* [n]         0..n_cams-1                                  */
  const double* cam_offsets;   /* [n_cams][3] getCamOffset: r of T_SC                      */
  const double* cam_rotations; /* [n_cams][9] getCamRotation: C of T_SC, row-major         */
  /* rotation only and relative */
  const double *bearing1, *bearing2; /* [n][3] getBearingVector1 / 2 */
  const double *sigma1, *sigma2;     /* [n]    getSigmaAngle1 / 2    */
  /* out, each may be NULL */
  int32_t* counts;    /* [n_models] countWithinDistance: the number of scores < threshold (strictly)                                 */
  int32_t* best;      /* the lowest index among the hypotheses with the largest count (the loop replaces its best only on a
                         strictly larger count)                                                                                       */
  int32_t* n_inliers; /* counts[best]                                                                                                */
  int32_t* inliers;   /* [n], the first n_inliers written: selectWithinDistance of hypothesis best, ascending                        */
  double* scores;     /* [n_models][n] every score; for referees: without it no score leaves the device                               */
} okvis_fe_sac_job;

/* For every job, the scores of all (hypothesis, correspondence) cells as the reference's getSelectedDistancesToModel computes them,
 * operation for operation in IEEE double without fused multiply-adds, and what Ransac::computeModel derives from them.
 *   absolute       the point through the inverse hypothesis into the body frame, minus the camera's offset, through the camera's
 *                  rotation transposed, normalised; score = |reprojection - bearing|^2 / sigma
 *   rotation only  score = |R f2 - f1|^2 0.5 / sigma1 + |R^T f1 - f2|^2 0.5 / sigma2
 *   relative       p = opengv::triangulation::triangulate2 under (R12, t12) = the hypothesis; score = |p/|p| - f1|^2 0.5 / sigma1 +
 *                  |q/|q| - f2|^2 0.5 / sigma2 with q = the inverse hypothesis applied to p.
 *                  triangulate2 is OpenGV's, and OpenGV's source is not part of the reference tree: this one function is stated
 *                  from the published two-view midpoint method (the closest points of the two rays, then their mean) and is NOT
 *                  pinned to reference lines; everything around it is.
 * One launch and one copy back per call: the device returns the counts and one 64-bit inlier ballot per (hypothesis, 64
 * correspondences); best and inliers are read off them on the host.  A cam_index entry outside 0..n_cams-1 is OKVIS_BA_ERR_ARG.
 * What is not here: the minimal solvers (okvis_fe_sac_solve, okvis_fe_sac_solve_absolute) and the sampler and the loop around them
 * (okvis_fe_ransac); see INTEGRATION.md for the recipe. */
int okvis_fe_sac_consensus(okvis_fe_context* ctx, int32_t n_jobs, const okvis_fe_sac_job* jobs);

#define OKVIS_FE_SAC_SAMPLE_ROTATION_ONLY 2 /* correspondences per sample of a rotation-only job                        */
#define OKVIS_FE_SAC_SAMPLE_RELATIVE 8      /* of a relative job: 5 that define E + 3 that pick the pose                */
#define OKVIS_FE_SAC_MAX_ROOTS 10           /* real essential matrices of five correspondences                          */

typedef struct okvis_fe_sac_solve_job { /* one 2D-2D sample-consensus problem with its samples: hypotheses are solved for, then scored */
  int32_t kind;      /* OKVIS_FE_SAC_ROTATION_ONLY or _RELATIVE; _ABSOLUTE is OKVIS_BA_ERR_ARG */
  int32_t n;         /* correspondences, 0..65536                                             */
  int32_t n_models;  /* samples = hypotheses, 1..1024                                         */
  int32_t reserved;  /* 0                                                                     */
  double threshold;
  const double *bearing1, *bearing2; /* [n][3]                                      */
  const double *sigma1, *sigma2;     /* [n]; read only when something is scored     */
  const int32_t* samples;            /* [n_models][2] or [n_models][8], indices into 0..n-1 */
  /* out, hypotheses; each may be NULL */
  double* models;     /* [n_models][9] rotation_t / [n_models][12] transformation_t, the layout okvis_fe_sac_job.models takes;
                         every entry of an invalid hypothesis is a quiet NaN                                                    */
  uint8_t* valid;     /* [n_models]                                                                                            */
  int32_t* n_roots;   /* relative, referee: real essential matrices found, 0..10                                               */
  double* essentials; /* relative, referee: [n_models][10][9] row-major, unit Frobenius norm, the first n_roots written (in no
                         stated order, each up to sign)                                                                        */
  /* out, consensus: exactly the five fields of okvis_fe_sac_job with the same meaning; all NULL = no scoring launch */
  int32_t *counts, *best, *n_inliers, *inliers;
  double* scores;
} okvis_fe_sac_solve_job;

/* The minimal solvers of Frontend::runRansac2d2d (okvis_frontend/src/Frontend.cpp:645-810) for all samples of many problems in one
 * call, chained into the consensus kernel of okvis_fe_sac_consensus: sample indices in, hypotheses and inlier sets out.  The
 * solvers are OpenGV's, and OpenGV's source is not part of the reference tree: like triangulate2 above, both solvers are stated
 * from their published mathematical definitions and are NOT pinned to OpenGV.
 * Convention (the consensus entry's): a point of frame 2 is R12 p2 + t12 in frame 1, so R f2 ~ f1 and f1^T E f2 = 0, E = [t12]x R12.
 *   rotation only  sample (i, j).  a1 = f1_i, a2 = (f1_i x f1_j) / |.|, a3 = a1 x a2; b1, b2, b3 alike from frame 2;
 *                  R(r,c) = (a1[r] b1[c] + a2[r] b2[c]) + a3[r] b3[c].  Cross products as u1 v2 - u2 v1 etc., the norm as
 *                  sqrt((x x + y y) + z z), then three divisions; IEEE double without fused multiply-adds, so the nine doubles
 *                  equal a float64 evaluation of these lines bit for bit.  Invalid when i == j or a cross product's norm is zero
 *                  or not finite.
 *   relative       sample (i0..i7); invalid up front when two of the eight indices are equal.  Candidates: all real E != 0, up to
 *                  scale, in the null space of the 5x9 matrix with rows vec(f1_k f2_k^T), k = i0..i4, with det E = 0 and
 *                  2 E E^T E - tr(E E^T) E = 0 (at most ten); for each the four (R, +-t) from its singular vectors (R = U W V^T,
 *                  U W^T V^T with det R = +1; |t| = 1, t^T E = 0).  A candidate passes when both ray parameters of the two-view
 *                  midpoint method are positive for all eight correspondences; the hypothesis is the passing candidate with the
 *                  smallest sum of the eight relative-pose scores (sigma = 1 where sigma1 / sigma2 are NULL), invalid when none
 *                  passes.  t12 has unit length (Frontend.cpp:782-787 rescales it by the motion prior).
 *                  The route is Nister's polynomial of degree ten with a polish on the definition; every loop has a compile-time
 *                  count and the result is deterministic.  tests/sac_solve_statement.py states the definition at 60 digits and
 *                  tests/sac_solve_cases.py the bound the hypotheses are held to.
 * One staging copy in, one solver launch for all jobs, one launch of the consensus kernel when any consensus output is asked for
 * (it reads the hypotheses where the solver left them in device memory), one copy back.  A NaN hypothesis scores NaN in every
 * cell; the consensus kernel counts `score < threshold`, which is false for NaN, so an invalid hypothesis has count 0 and never
 * displaces a valid best under the "strictly larger count" rule (with every hypothesis invalid, best = 0 and n_inliers = 0).
 * OKVIS_BA_ERR_ARG before anything is enqueued and with nothing written: a NULL context or required pointer (bearing1, bearing2
 * for n > 0, samples), a negative count, n or n_models out of range, an unknown kind or OKVIS_FE_SAC_ABSOLUTE, a sample index
 * outside 0..n-1 (so n = 0 has no valid sample), NULL sigma1 or sigma2 while a consensus output is wanted.  n_jobs = 0 is valid.
 * The sampler and the loop around this entry are okvis_fe_ransac; the generalised P3P of runRansac3d2d is okvis_fe_sac_solve_absolute.
 * What is not here: optimizeModelCoefficients. */
int okvis_fe_sac_solve(okvis_fe_context* ctx, int32_t n_jobs, const okvis_fe_sac_solve_job* jobs);

#define OKVIS_FE_SAC_SAMPLE_ABSOLUTE 4    /* correspondences per sample: 3 that define the candidates + 1 that picks the pose */
#define OKVIS_FE_SAC_MAX_ROOTS_ABSOLUTE 8 /* real solutions of three quadrics in three depths                                 */

typedef struct okvis_fe_sac_absolute_job { /* one 3D-2D sample-consensus problem with its samples: hypotheses are solved for, then scored */
  int32_t n;         /* correspondences, 0..65536     */
  int32_t n_models;  /* samples = hypotheses, 1..1024 */
  int32_t n_cams;    /* 1..8                          */
  int32_t reserved;  /* 0                             */
  double threshold;
  /* exactly the absolute inputs of okvis_fe_sac_job, same meaning and layout */
  const double* points;        /* [n][3]                                     */
  const double* bearing;       /* [n][3]                                     */
  const double* sigma;         /* [n]; read only when something is scored    */
  const int32_t* cam_index;    /* [n]         0..n_cams-1                    */
  const double* cam_offsets;   /* [n_cams][3]                                */
  const double* cam_rotations; /* [n_cams][9] row-major                      */
  const int32_t* samples;      /* [n_models][4], indices into 0..n-1         */
  /* out, hypotheses; each may be NULL */
  double* models;     /* [n_models][12] row-major 3x4 transformation_t, the layout okvis_fe_sac_job.models takes; every entry of an
                         invalid hypothesis is a quiet NaN                                                                      */
  uint8_t* valid;     /* [n_models]                                                                                            */
  int32_t* n_roots;   /* referee: candidates found, 0..8                                                                       */
  double* candidates; /* referee: [n_models][8][12], the first n_roots written (in no stated order), the rest quiet NaNs       */
  /* out, consensus: exactly the five fields of okvis_fe_sac_job with the same meaning; all NULL = no scoring launch */
  int32_t *counts, *best, *n_inliers, *inliers;
  double* scores;
} okvis_fe_sac_absolute_job;

/* The minimal solver of Frontend::runRansac3d2d (okvis_frontend/src/Frontend.cpp:575-642: FrameAbsolutePoseSacProblem with
 * Algorithm::GP3P) for all samples of many problems in one call, chained into the consensus kernel of okvis_fe_sac_consensus:
 * sample indices in, hypotheses and inlier sets out.  OpenGV's gp3p is generated Groebner-basis code and OpenGV's source is not
 * part of the reference tree: the solver is stated from its mathematical definition and is NOT pinned to OpenGV.
 * Convention (the consensus entry's): a hypothesis (R, t) takes a body point to the world, X = R p + t.
 *   inputs       sample (i0, i1, i2, i3); for k = 0..2: c_k = cam_offsets[cam_index[i_k]], d_k = cam_rotations[cam_index[i_k]]
 *                bearing[i_k], X_k = points[i_k].
 *   invalid      up front when two of the four indices are equal, or (X_1 - X_0) x (X_2 - X_0) has a zero or non-finite norm.
 *   candidates   all real (l0, l1, l2), every l_k > 0, with |(c_a + l_a d_a) - (c_b + l_b d_b)|^2 = |X_a - X_b|^2 for the pairs
 *                (0,1), (0,2), (1,2): three quadrics in three unknowns, at most eight.  With p_k = c_k + l_k d_k the candidate is the
 *                proper rigid transformation that takes the p_k to the X_k: a1 = (X_1 - X_0) / |.|, a2 = (a1 x (X_2 - X_0)) / |.|,
 *                a3 = a1 x a2; b1, b2, b3 alike from the p_k (the frames of the rotation-only solver above);
 *                R(r,c) = (a1[r] b1[c] + a2[r] b2[c]) + a3[r] b3[c], t = X_0 - R p_0.
 *   hypothesis   the candidate with the smallest |reprojection - bearing|^2 of correspondence i3 (the absolute score of
 *                okvis_fe_sac_consensus without the division by sigma); invalid when there is no candidate.  Positive depths are
 *                the rule of the relative solver above on its ray parameters.
 *   central      all three correspondences from one camera, or n_cams = 1: the same definition through the same code.
 *                The route: the resultant of the two quadrics that share l0, reduced modulo the third to one polynomial of degree
 *                eight in l1; its roots over all of l1 > 0 (on [0, 1] in l1 and on [0, 1] in 1 / l1: no bound on the scene is
 *                assumed) by the derivative chain of the relative solver; l0 and l2 from their quadratics; Newton on the three
 *                quadrics themselves; the frames.  Every loop has a compile-time count and the result is deterministic.
 *                tests/sac_abs_statement.py states the definition at 60 digits and tests/sac_abs_cases.py the bound the
 *                hypotheses are held to.
 * One staging copy in, one solver launch for all jobs, one launch of the consensus kernel when any consensus output is asked for
 * (it reads the hypotheses where the solver left them in device memory, and the points, bearings and cameras as staged once), one
 * copy back.  An invalid hypothesis scores NaN and counts 0, as for okvis_fe_sac_solve.
 * OKVIS_BA_ERR_ARG before anything is enqueued and with nothing written: a NULL context or table, a negative count, n, n_models or
 * n_cams out of range, a NULL required input (samples always; points, bearing, cam_index, cam_offsets, cam_rotations for n > 0), a
 * cam_index outside 0..n_cams-1, a sample index outside 0..n-1 (so n = 0 has no valid sample), NULL sigma while a consensus
 * output is wanted.  n_jobs = 0 is valid.
 * The sampler and the loop around this entry are okvis_fe_ransac.  What is not here: optimizeModelCoefficients. */
int okvis_fe_sac_solve_absolute(okvis_fe_context* ctx, int32_t n_jobs, const okvis_fe_sac_absolute_job* jobs);

#define OKVIS_FE_RANSAC_STOP_CONVERGED 0      /* the adaptive bound was met                                                  */
#define OKVIS_FE_RANSAC_STOP_MAX_ITERATIONS 1 /* iterations went past max_iterations                                         */
#define OKVIS_FE_RANSAC_STOP_EXHAUSTED 2      /* the n_slots sample slots ran out before the loop stopped                    */
#define OKVIS_FE_RANSAC_STOP_SKIPS 3          /* 10 * max_iterations samples without a hypothesis                            */
#define OKVIS_FE_RANSAC_STOP_NO_SAMPLE 4      /* n is below the sample size: nothing was drawn                               */

typedef struct okvis_fe_ransac_job { /* one whole sample-consensus run: correspondences in, inlier set and model out */
  int32_t kind;           /* OKVIS_FE_SAC_*, mixed freely within a call                                       */
  int32_t n;              /* correspondences, 0..65536                                                        */
  int32_t n_slots;        /* sample slots solved speculatively, 1..1024                                       */
  int32_t n_cams;         /* absolute: 1..8                                                                   */
  int32_t max_iterations; /* >= 1; the reference uses 50                                                      */
  int32_t reserved;       /* 0                                                                                */
  double threshold;       /* the reference uses 9                                                             */
  double probability;     /* strictly inside (0, 1); the reference uses 0.99                                  */
  uint64_t seed;
  /* the input arrays of okvis_fe_sac_job for the kind, same meaning and layout */
  const double* points;
  const double* bearing;
  const double* sigma;
  const int32_t* cam_index;
  const double* cam_offsets;
  const double* cam_rotations;
  const double *bearing1, *bearing2;
  const double *sigma1, *sigma2;
  /* out, each may be NULL */
  int32_t* best;       /* the slot of the returned hypothesis, or -1                                                        */
  int32_t* n_inliers;  /* its count, 0 when best = -1                                                                       */
  int32_t* inliers;    /* [n], the first n_inliers written, ascending                                                       */
  double* model;       /* [12] row-major 3x4, or the first 9 (row-major 3x3) of a rotation-only job; quiet NaNs when best = -1 */
  int32_t* iterations; /* valid slots the loop consumed                                                                     */
  int32_t* skipped;    /* invalid slots the loop consumed                                                                   */
  int32_t* stop;       /* OKVIS_FE_RANSAC_STOP_*                                                                            */
  /* out, for referees; each may be NULL; not written when n is below the sample size */
  int32_t* samples; /* [n_slots][s]                                                                                         */
  uint8_t* valid;   /* [n_slots]                                                                                            */
  int32_t* counts;  /* [n_slots]                                                                                            */
  double* models;   /* [n_slots][9] rotation only / [n_slots][12]                                                            */
} okvis_fe_ransac_job;

/* opengv::sac::Ransac<P>::computeModel as Frontend::runRansac3d2d / runRansac2d2d call it (okvis_frontend/src/Frontend.cpp:599-611,
 * 677-703), for all sample-consensus runs of a frame in one call: many sequences, the three problem kinds mixed.  OpenGV's source is
 * not part of the reference tree (oracle/shim/callers/opengv/sac/Ransac.hpp is declarations only): like the solvers, the sampler
 * and the loop are stated here and are NOT pinned to OpenGV.  s is the kind's OKVIS_FE_SAC_SAMPLE_* constant: 2, 8 or 4.
 *   sampler   slot m of a job with seed S: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9,
 *             0xBB67AE85) under the key (S mod 2^32, S >> 32); u_0..u_3 = the output for counter (m, 0, 0, 0), u_4..u_7 for
 *             (m, 1, 0, 0).  With the virtual array A[i] = i, for k = 0..s-1: j = k + ((uint64)u_k * (uint64)(n - k) >> 32); swap
 *             A[k] and A[j]; sample[k] = A[k] (a sparse Fisher-Yates).  The indices are distinct and in range by construction, the
 *             draw is uniform up to n / 2^32, and it depends on (S, m, n, s) only, never on the batch around the job.
 *   slots     slot m's hypothesis is the solver of okvis_fe_sac_solve / okvis_fe_sac_solve_absolute on sample m, its count that of
 *             okvis_fe_sac_consensus under `threshold`: the same kernels, unchanged.  All n_slots slots are solved and scored
 *             speculatively; the loop decides which of them the sequential loop would have reached.
 *   loop      it = 0; skipped = 0; best = -1; best_count = -1; stop = EXHAUSTED
 *             for m = 0 .. n_slots-1:
 *                 if !valid[m]: skipped += 1
 *                               if skipped >= 10 * max_iterations: stop = SKIPS; break
 *                               continue
 *                 if counts[m] > best_count: best = m; best_count = counts[m]
 *                 it += 1
 *                 if done(it, best_count): stop = CONVERGED; break
 *                 if it > max_iterations:  stop = MAX_ITERATIONS; break
 *   done      the adaptive bound it >= log(1 - p) / log(1 - w^s) without transcendental functions, in IEEE double, every
 *             operation rounded on its own: w = (double)c / (double)n; ws = w multiplied by w a further s-1 times; q = 1.0 - ws,
 *             clamped to [2^-52, 1 - 2^-52]; r = q^it by binary powering from the least significant bit of it (r = 1, b = q; per
 *             bit: if (e & 1) r = r * b; b = b * b; e >>= 1); done = r <= 1.0 - p.  A hypothesis with count 0 never satisfies
 *             done, so the loop may run max_iterations + 1 iterations (it stops on it > max_iterations, after the iteration).
 *   result    iterations = it; n_inliers = best_count (0 when best = -1); inliers = the correspondences with score < threshold
 *             under hypothesis best, ascending; model = hypothesis best.
 * n below s is not an error: nothing is launched for the job, best = -1, n_inliers = 0, iterations = 0, skipped = 0,
 * stop = NO_SAMPLE, model = quiet NaNs.
 * One staging copy in; sac_sample_kernel for all jobs; sac_solve_kernel for the 2D-2D jobs; sac_gp3p_kernel for the absolute jobs;
 * one sac_consensus_kernel launch over all jobs; sac_loop_kernel (one wave per job); one copy back.  No sample index crosses the
 * bus unless `samples` asks for it; counts, valid, ballots and hypotheses stay on the device unless a referee output asks for
 * them: without referee outputs the copy back holds the per-job record, the model and the inlier lists only.
 * OKVIS_BA_ERR_ARG before anything is enqueued and with nothing written: a NULL context or table, a negative job count, an unknown
 * kind, n outside 0..65536, n_slots outside 1..1024, max_iterations < 1, probability not strictly inside (0, 1), for n > 0 a NULL
 * input of the kind (absolute: points, bearing, sigma, cam_index, cam_offsets, cam_rotations; the others: bearing1, bearing2,
 * sigma1, sigma2), for an absolute job n_cams outside 1..8 or a cam_index outside 0..n_cams-1.  n_jobs = 0 is valid.
 * What is not here: optimizeModelCoefficients (the reference's frontend never calls it); the bearing vectors are a call of their
 * own (okvis_fe_bearing_vectors). */
int okvis_fe_ransac(okvis_fe_context* ctx, int32_t n_jobs, const okvis_fe_ransac_job* jobs);

#define OKVIS_FE_IMU_COV 1 /* the 15x15 covariance of the propagated state is wanted */
#define OKVIS_FE_IMU_JAC 2 /* the 15x15 Jacobian of the propagated state is wanted   */

typedef struct okvis_fe_imu_job { /* one sequence's chain of ImuError::propagation calls */
  int32_t s_begin, s_count; /* its measurement deque: samples s_begin .. s_begin + s_count - 1 of the pool, stamps strictly ascending */
  int32_t e_begin, e_count; /* its end times: ends[e_begin .. e_begin + e_count - 1], ascending, e_count >= 1                    */
  int32_t prm;              /* index into params[]                                                                            */
  int32_t flags;            /* OKVIS_FE_IMU_COV | OKVIS_FE_IMU_JAC, for every end of the job                                  */
  int64_t t_start;          /* ns                                                                                             */
  double T_WS[7];           /* r, q (x, y, z, w) at t_start                                                                   */
  double sb[9];             /* v, b_g, b_a at t_start                                                                         */
} okvis_fe_imu_job;

/* ImuError::propagation (okvis_ceres/src/ImuError.cpp:287-504) for many jobs in one launch.  For k = 0 .. e_count - 1 a job makes
 * the call propagation(deque, params[prm], T, sb, start_k, ends[e_begin + k], cov?, jac?) with start_0 = t_start,
 * start_k = ends[e_begin + k - 1], and T, sb = the job's for k = 0, the outputs of call k - 1 afterwards: what
 * ThreadedKFVio::imuConsumerLoop does with T_WS_propagated_ / speedAndBiases_propagated_ through Frontend::propagation
 * (ThreadedKFVio.cpp:559-598, Frontend.cpp:274-292), once per IMU sample and with the WHOLE deque.  A job with e_count = 1 is the call
 * of Estimator::addStates (Estimator.cpp:145-147) and of ThreadedKFVio::frameConsumerLoop (:416-418).  Every call is a fresh one
 * (Delta_q, the integrals and P_delta start from nothing, :306-325); only the state is carried.
 * The statement is the reference's, operation for operation in IEEE double without fused multiply-adds: the end interpolation before
 * the start interpolation, which reads the already interpolated second sample (:347-366); leading samples skipped while dt <= 0;
 * a saturated sample multiplies the step's sigma by 100 (:369-389), and sigma2_v = dt * sigma_a_c(step) * sigma_a_c(parameters)
 * (:438), so that a saturated accelerometer weighs 100 times where a saturated gyroscope weighs 10^4 times; dalpha_db_g without the
 * right Jacobian (:412); F_delta from the integrals before the memory shift (:421-431); the loop ends at nexttime == t_end;
 * g_W = g (0, 0, 6371009).normalized(); cov = T P_delta T^T and the blocks of jac as at :480-502.
 * Out, at the end's index in the pool: T_WS [n_ends][7] (q normalised as Transformation's constructor does), sb [n_ends][9],
 * count [n_ends] = the call's return value (the number of integration steps), and for the jobs that ask, cov / jac [n_ends][225]
 * row-major over (r, alpha, v, b_g, b_a).  Rows of cov / jac that no call wrote are left as they were: those of jobs without the
 * flag and those of calls that returned early (count = -1, or s_count < 2).
 *   count = -1  the deque ends before the end time (:301-302): the call's outputs are its inputs, the chain goes on from them
 *   count =  0  s_count < 2, for every end of the job: Frontend::propagation's early return (Frontend.cpp:281-286); also a call
 *               with end == start, which goes through the statement with nothing to integrate (q comes back normalised,
 *               cov = 0, jac = I)
 * OKVIS_BA_ERR_ARG, before anything is enqueued and with nothing written: NULL context or required pointer (cov / jac are required
 * once a job sets the flag), negative counts, a sample or end range outside its pool, e_count < 1, prm outside params, unknown flag
 * bits, stamps of a deque not strictly ascending, ends not ascending or before t_start, and for s_count >= 2 a deque that starts
 * after t_start (the reference asserts against it, :300).  n_jobs = 0 is valid. */
int okvis_fe_imu_propagate(okvis_fe_context* ctx, int32_t n_params, const okvis_ba_imu_params* params, int32_t n_samples,
                           const int64_t* s_t, const double* s_gyr, const double* s_acc, int32_t n_ends, const int64_t* ends,
                           int32_t n_jobs, const okvis_fe_imu_job* jobs, double* T_WS, double* sb, double* cov, double* jac,
                           int32_t* count);

#define OKVIS_FE_KF_FEW_POINTS 1u  /* the image has fewer than 3 keypoints: skipped (Frontend.cpp:332-333)                          */
#define OKVIS_FE_KF_FEW_MATCHES 2u /* 3 or more keypoints, fewer than 3 of them with a landmark: skipped (:335-336)                  */

typedef struct okvis_fe_kf_image { /* one camera image: keypoints kp_begin .. kp_begin + kp_count - 1 of the pool */
  int32_t kp_begin, kp_count;      /* kp_count 0..8192; 0 is valid */
} okvis_fe_kf_image;

typedef struct okvis_fe_kf_job { /* one multiframe */
  int32_t im_begin, n_cams;      /* its images im_begin .. im_begin + n_cams - 1 of the image pool, in camera order; n_cams 1..8 */
  int32_t num_frames;            /* estimator.numFrames() (:299), >= 0                                                           */
  int32_t initialized;           /* isInitialized_ (:304), zero or not                                                           */
  float overlap_threshold;       /* keyframeInsertionOverlapThreshold_ (Frontend.hpp:312; the reference's comment says 0.6)      */
  float ratio_threshold;         /* keyframeInsertionMatchingRatioThreshold_ (Frontend.hpp:319; 0.2)                             */
} okvis_fe_kf_job;

/* Frontend::doWeNeedANewKeyframe (okvis_frontend/src/Frontend.cpp:295-369) for many multiframes per call: the step between
 * matchToKeyframes and matchToLastFrame (:196).  kp [n_kp][3] float (x, y, size; size is not read) and matched [n_kp] (non-zero where
 * landmarkId(im, k) != 0, :327) are pools; images index the pools, jobs index the images.  Images and jobs may share ranges.
 *
 * cv::convexHull, cv::contourArea and cv::pointPolygonTest (:334-349) are OpenCV's, and OpenCV's source is not part of the reference
 * tree: the three are stated here from their mathematical definitions and are NOT pinned to OpenCV; everything around them is the
 * reference's, operation for operation.  Keypoints are float, so every quantity has an exact rational value and the statement is
 * exact; near an edge OpenCV's rounded test may answer differently from the exact one.
 *   orient(a, b, c)  the exact sign of (bx-ax)(cy-ay) - (by-ay)(cx-ax) over the rationals the floats are
 *   hull             the vertices of the convex hull, strict (no coincident vertices, none on the segment between its neighbours),
 *                    starting at the point with the smallest (y, then x), in the order with orient(v_i, v_i+1, v_i+2) > 0; every
 *                    vertex is reported as the lowest keypoint index with its coordinates (indices count from the image's first
 *                    keypoint).  All points coincident: size 1; all collinear: size 2, the two extremes in that order.
 *   area             a = 0; prev = last vertex; for p in order: a += (double)prev.x * p.y - (double)prev.y * p.x, prev = p;
 *                    area = fabs(a * 0.5), in IEEE double without fused multiply-adds (both products are exact).  Size 1 or 2: 0.
 *   inside           keypoint k (of all, matched or not) is inside iff the matched hull has at least 3 vertices and
 *                    orient(v_i, v_i+1, p_k) > 0 for every edge: vertices and points on an edge are not inside
 *                    (pointPolygonTest(...) > 0).
 * Per image in camera order, with (overlap, ratio) = (0, 0) carried along (:307-361): fewer than 3 keypoints or fewer than 3 matched:
 * skipped (flag set, hull sizes, areas and n_inside are 0); else overlapArea = area_matched / area_all and matchingRatio =
 * (double)n_matched / (double)n_inside as IEEE divisions (0/0 = NaN, x/0 = inf), and overlap = (overlapArea < overlap) ? overlap :
 * overlapArea — std::max with its NaN behaviour: a NaN replaces the running value, and the next image replaces the NaN — ratio alike.
 * decision (1 = a new keyframe is needed): num_frames < 2 -> 1; else !initialized -> 0; else
 * !(overlap > (double)overlap_threshold && ratio > (double)ratio_threshold).
 * Out, each may be NULL (leaving one out changes none of the others): per job decision, overlap, ratio [n_jobs]; per image n_matched,
 * hull_all_size, hull_matched_size, area_all, area_matched, n_inside, flags (OKVIS_FE_KF_*) [n_images]; for referees hull_all,
 * hull_matched [sum of kp_count]: image i's list starts at the sum of kp_count of the images before it, holds its size indices
 * and then -1 up to kp_count entries.  Every image of the pool is computed, whether a job names it or not.
 * One staging copy in, one launch (one wave per image; the per-job fold runs on the host from the per-image results), one copy back.
 * OKVIS_BA_ERR_ARG, before anything is enqueued and with nothing written: NULL context or required pointer (jobs, images, kp and
 * matched where their counts are positive), a negative count, kp_count outside 0..8192, n_cams outside 1..8, num_frames < 0, a
 * keypoint or image range outside its pool, more than INT32_MAX hull entries, a non-finite x or y of a keypoint that an image names.
 * n_jobs = 0 and an image without keypoints are valid. */
int okvis_fe_keyframe_decision(okvis_fe_context* ctx, int32_t n_kp, const float* kp, const uint8_t* matched, int32_t n_images,
                               const okvis_fe_kf_image* images, int32_t n_jobs, const okvis_fe_kf_job* jobs, uint8_t* decision,
                               double* overlap, double* ratio, int32_t* n_matched, int32_t* hull_all_size, int32_t* hull_matched_size,
                               double* area_all, double* area_matched, int32_t* n_inside, uint8_t* flags, int32_t* hull_all,
                               int32_t* hull_matched);

#define OKVIS_FE_DETECT_OVERFLOW 1u /* more candidates than cand_capacity: nothing was selected, raise the threshold           */
#define OKVIS_FE_DETECT_FULL 2u     /* max_keypoints were accepted and one more would have been: the list is cut short       */
#define OKVIS_FE_DETECT_MAX_DIM 8192        /* width and height: 5 .. 8192                                                   */
#define OKVIS_FE_DETECT_MAX_KEYPOINTS 2048  /* the reference asks for 400 to 450                                             */
#define OKVIS_FE_DETECT_MAX_CANDIDATES 8192 /* the keyframe entry's limit per image; the selection kernel holds a candidate
                                               list in the registers of one workgroup, 1024 lanes x 8                        */

typedef struct okvis_fe_detect_job { /* one grey image */
  const uint8_t* image;  /* row-major, row y starts at image + y * pitch                                  */
  int64_t threshold;     /* >= 1, on the scale of S below                                                 */
  int32_t width, height; /* 5 .. OKVIS_FE_DETECT_MAX_DIM each; below 5 there is no pixel with a score     */
  int32_t pitch;         /* bytes, >= width                                                               */
  int32_t min_dist;      /* >= 0: the uniformity radius in pixels, the reference's `threshold` option (40) */
  int32_t max_keypoints; /* 1 .. OKVIS_FE_DETECT_MAX_KEYPOINTS                                            */
  int32_t cand_capacity; /* 1 .. OKVIS_FE_DETECT_MAX_CANDIDATES                                           */
  float kp_size;         /* copied into the third column of kp: BRISK's size for octave 0 is the caller's to supply */
  /* out */
  int32_t n_keypoints;
  int32_t n_candidates; /* the true count, past cand_capacity too */
  int32_t flags;        /* OKVIS_FE_DETECT_*                       */
  float* kp;            /* [max_keypoints][3] x, y, size: the first n_keypoints rows are written, in selection order, strongest
                           first; what every other okvis_fe_* entry takes as keypoints                                        */
  double* response;     /* [max_keypoints] or NULL: (double)S, exact                                                        */
  int32_t* pixel;       /* [max_keypoints][2] or NULL: x, y of the integer maximum                                          */
  int64_t* score;       /* [height][width] or NULL: the whole score image, 0 outside its domain.  A referee's output: without
                           it no score leaves the tile it was computed in                                                    */
} okvis_fe_detect_job;

/* What Frontend::detectAndDescribe (okvis_frontend/src/Frontend.cpp:92-114) asks of its detector under the shipped configuration,
 * for many images per call: brisk::ScaleSpaceFeatureDetector<brisk::HarrisScoreCalculator>(threshold, octaves, absoluteThreshold,
 * maxNoKeypoints) (:828-831) with octaves = 0 — a Harris score on the full-resolution image, a 3 x 3 maximum search above an absolute
 * threshold, a selection of the strongest maxima that keeps them apart.  BRISK's source is not part of the reference tree (it is
 * fetched at build time): the detector is stated here and is NOT pinned to BRISK.  Descriptors and masks are not here; the scale
 * space (octaves > 0) is okvis_fe_detect_keypoints_scaled's.  Images are 8-bit: the statement is integer arithmetic (int64 unless said otherwise) and every output is exact.
 * With I the image, w = width, h = height:
 *   derivatives  for 1 <= x <= w-2, 1 <= y <= h-2 (Sobel):
 *                Ix = (I[y-1][x+1] + 2 I[y][x+1] + I[y+1][x+1]) - (I[y-1][x-1] + 2 I[y][x-1] + I[y+1][x-1]),
 *                Iy = (I[y+1][x-1] + 2 I[y+1][x] + I[y+1][x+1]) - (I[y-1][x-1] + 2 I[y-1][x] + I[y-1][x+1]);  |Ix|, |Iy| <= 4 * 255 = 1020.
 *   tensor       for 2 <= x <= w-3, 2 <= y <= h-3 (the score domain): A = sum k Ix^2, B = sum k Ix Iy, C = sum k Iy^2 over the 3 x 3
 *                neighbourhood under the binomial weights k = [1 2 1]^T [1 2 1] (sum 16).
 *   score        S = 16 (A C - B^2) - (A + C)^2: the Harris measure det - k trace^2 with k = 1/16, scaled by 16.
 *                Bounds: 0 <= A, C <= 16 * 1020^2 = 16 646 400 and |B| <= the same, so A C <= 2.78e14, 0 <= A C - B^2 <= 2.78e14
 *                (Cauchy-Schwarz), (A + C)^2 <= 1.11e15, and -1.11e15 <= S <= 4.44e15: |S| < 5.6e15 < 2^53 = 9.007e15.  No int64
 *                intermediate overflows, and every score is exact in a double.
 *   candidates   pixel p BEATS pixel q when S_p > S_q, or S_p == S_q and y_p w + x_p < y_q w + x_q: a total order.  A pixel of the
 *                score domain is a candidate when S >= threshold and it beats all of its eight neighbours; neighbours outside the
 *                score domain count as beaten.  A plateau yields exactly one candidate.  n_candidates is their number.
 *   sub-pixel    along x: num = S(x-1,y) - S(x+1,y), den = 2 (S(x-1,y) - 2 S(x,y) + S(x+1,y)) in int64, a neighbour outside the domain
 *                counting as S(x,y); both converted to double (round to nearest); d = num / den if den != 0, else 0, clamped to
 *                [-0.5, 0.5]; kp.x = (float)((double)x + d).  The same along y.  One IEEE division and one addition per axis.
 *   selection    n_candidates > cand_capacity: flags = OVERFLOW, n_keypoints = 0, no partial result.  Otherwise the candidates are
 *                gone through in beat order, strongest first; one is ACCEPTABLE when every keypoint accepted before it lies at integer
 *                squared distance >= min_dist^2 from it, measured on the integer maxima (min_dist = 0: all are); acceptable
 *                candidates are accepted until max_keypoints have been; when a further one is acceptable after that, flags |= FULL
 *                (candidates running out right at max_keypoints is not FULL).  This is plain greedy disc suppression.  BRISK weights
 *                its uniformity mask by score: this rule is NOT BRISK's.
 * One staging copy in (the images, rows packed without their pitch, in front of everything else in the block); detect_score_kernel,
 * one workgroup per 64 x 16 tile of any image: bytes, gradients and scores in LDS, only candidates leave the tile (24 bytes each,
 * appended through one counter per image; the list's order in memory reaches no output); detect_select_kernel, one workgroup per
 * image: the strongest candidate still in play by a workgroup-wide reduction per accepted keypoint, its disc struck out in
 * parallel; one copy back.  The results do not depend on the batch around a job or on the run.
 * OKVIS_BA_ERR_ARG before anything is enqueued and with nothing written: a NULL context or table, a negative job count, a NULL
 * image or kp, width or height outside 5..OKVIS_FE_DETECT_MAX_DIM, pitch < width, threshold < 1, min_dist < 0, max_keypoints or
 * cand_capacity outside their limits.  n_jobs = 0 is valid and touches nothing. */
int okvis_fe_detect_keypoints(okvis_fe_context* ctx, int32_t n_jobs, okvis_fe_detect_job* jobs);

#define OKVIS_FE_DESCRIBE_VALID 1u           /* the keypoint lies inside the 11-pixel margin: its descriptor row is written           */
#define OKVIS_FE_DESCRIBE_ANGLE_UNDEFINED 2u /* backProject failed, the projection's distortion is undefined or eg is not finite:
                                                rot = 0, angle = 0, and the descriptor is still computed (at rot 0)                  */
#define OKVIS_FE_DESCRIBE_BYTES 48           /* PopcntofXORed(..., 3) of VioKeyframeWindowMatchingAlgorithm.hpp:253: 3 x 128 bits     */
#define OKVIS_FE_DESCRIBE_ROTATIONS 1024
#define OKVIS_FE_DESCRIBE_PAIRS 383

typedef struct okvis_fe_describe_job { /* one grey image and its keypoints */
  const uint8_t* image;  /* as okvis_fe_detect_job: row y starts at image + y * pitch        */
  int32_t width, height; /* 5 .. OKVIS_FE_DETECT_MAX_DIM each                                */
  int32_t pitch;         /* bytes, >= width                                                  */
  int32_t n;             /* >= 0 keypoints                                                   */
  const float* kp;       /* [n][3] x, y, size as everywhere; the size is not read            */
  const okvis_fe_camera* cam; /* the camera of the angle stage; may be NULL with rot_in      */
  double direction[3];   /* the extraction direction in the camera frame: C_CW * (0, 0, -1)  */
  const int32_t* rot_in; /* [n] in 0..1023, or NULL.  Given: the angle stage is skipped, rot = rot_in, angle and angle64 are not
                            written and ANGLE_UNDEFINED is never set                           */
  /* out */
  int32_t n_valid;       /* keypoints with VALID                                             */
  uint8_t* desc;         /* [n][48]: what the matching entries take as descriptors; an invalid keypoint's row is zero             */
  uint8_t* flags;        /* [n] OKVIS_FE_DESCRIBE_*; the complement of VALID is the matching entries' skip mask                   */
  int32_t* rot;          /* [n] or NULL: the rotation index the descriptor was taken at                                           */
  float* angle;          /* [n] or NULL: cv::KeyPoint::angle, degrees                                                             */
  double* angle64;       /* [n] or NULL: the value before the cast to float.  A referee's output                                  */
} okvis_fe_describe_job;

/* Frame::describe (okvis_cv/include/okvis/implementation/Frame.hpp:128-156) for many images per call: the angle of every keypoint,
 * then brisk::BriskDescriptorExtractor(rotationInvariance = true, scaleInvariance = false)::compute at that angle.
 *
 * ANGLE (pinned to the reference, Frame.hpp:139-150; fp64, operation for operation, no fused multiply-adds in this stage's own
 * arithmetic): backProject(kp.x, kp.y) -> ep; project(ep, &reprojection, &Jacobian) (implementation/PinholeCamera.hpp:148-226);
 * eg = Jacobian * direction; angle64 = atan2(eg[1], eg[0]) / M_PI * 180.0; angle = (float)angle64;
 * The last expression is the one place where the entry is MORE exact than the reference's three roundings (which leave a double up
 * to 2 ulp from the expression's value): it is evaluated in double-double from the doubles eg[1], eg[0] and rounded once, so
 * angle64 is the double nearest to atan2(eg[1], eg[0]) / M_PI * 180 with M_PI the double.  (A zero component of eg takes the three
 * plain operations, whose result is exact there: 0, +-90, +-180.)
 * rot = ((int)floor((double)angle * 1024.0 / 360.0 + 0.5)) mod 1024, in 0..1023.  All four OKVIS_BA_DIST_* models.  The reference does
 * not read backProject's status; here a failed backProject, an undefined distortion in the projection (the reference then reads a
 * Jacobian it never wrote) or a non-finite eg sets ANGLE_UNDEFINED, rot = 0, angle = angle64 = 0, and the descriptor is still
 * computed.  A job may pass rot_in instead: the stage is skipped and cam may be NULL.
 *
 * EXTRACTION.  BRISK's source is not part of the reference tree (it is fetched at build time): the extractor is stated here from the
 * published BRISK construction and is NOT pinned to BRISK.  It is integer arithmetic, so every descriptor byte is exact.
 * Fixed tables (tools/gen_describe_tables.py, from a 60-digit evaluation, rounded to nearest, half away from zero; handed out by
 * okvis_fe_describe_tables):
 *   pattern    60 points on 5 rings, N = (1, 10, 14, 15, 20) points per ring at radii r = 0.85 * (0, 2.9, 4.9, 7.4, 10.8) pixels; point a of
 *              ring m at angle 2 pi a / N_m; the index k runs ring by ring, a ascending; base[60][2] = round(65536 * (x, y)) (Q16, int32).
 *   boxes      half widths in sixteenths of a pixel (Q4) per ring: h = (10, 16, 19, 27, 30) = round(16 * 1.3 r_m sin(pi / N_m)), 0.65 px
 *              for the centre; A_k = (2 h_ring(k))^2.
 *   rotations  cs[1024][2] = round(2^30 * (cos, sin)(2 pi j / 1024)); cs[(j + 256) mod 1024] = (-s_j, c_j) exactly.
 *   pairs      all (i, k), i < k, whose unrotated distance is below 5.1 pixels, in ascending (i, k) order: 383 of them (the nearest
 *              distances on either side are 5.0835 and 5.1166, so no rounding decides it).  Descriptor bit b is pair b, stored in
 *              byte b >> 3 at bit b & 7; bit 383 is always 0.
 * Per keypoint, with w = width, h = height:
 *   position   qx = (int64)floor((double)kp.x * 16.0 + 0.5), the same for qy.  VALID iff kp.x, kp.y are finite and
 *              176 <= qx <= 16 (w - 1) - 176 and 176 <= qy <= 16 (h - 1) - 176: an 11-pixel margin.  Pixel x covers [16 x - 8, 16 x + 8)
 *              and the tables' largest reach |offset| + h is 177, so no sample box leaves the image.  An invalid keypoint gets an
 *              all-zero descriptor row and no VALID flag; it keeps its index (the reference would remove it).
 *   offsets    with (c, s) = cs[rot] and (bx, by) = base[k]: dx = R(c bx - s by), dy = R(s bx + c by) in int64,
 *              R(z) = sign(z) * ((|z| + 2^41) >> 42): Q46 to Q4, half away from zero (the symmetric rounding makes a quarter turn of
 *              the image exact).  Centre (cx, cy) = (qx + dx, qy + dy).
 *   sample     V_k = sum_y sum_x I[y][x] wy(y) wx(x), wx(x) = max(0, min(16 x + 8, cx + h_k) - max(16 x - 8, cx - h_k)), wy likewise: the
 *              area-weighted box of side 2 h_k around the centre; sum wx = 2 h_k; V <= 255 * 3600 < 2^20.
 *   bit        for pair (i, k): V_i A_k > V_k A_i, the two means compared by cross-multiplication (products below 3.4e9: int64).
 * Not here: scale invariance (keypoints of coarser layers, okvis_fe_detect_keypoints_scaled, are described at this one scale too),
 * BRISK's own bit selection, masks.
 *
 * One staging copy in (the images as in okvis_fe_detect_keypoints, keypoints, cameras); describe_angle_kernel, one lane per keypoint;
 * describe_kernel, one wave per keypoint: its 25 x 25 pixels in LDS, lane k < 60 computes V_k, six ballots are the descriptor; one copy
 * back.  Rows of desc, flags, rot, angle, angle64 past n are left alone.  The results do not depend on the batch around a job.
 * OKVIS_BA_ERR_ARG before anything is enqueued and with nothing written: a NULL context or table, a negative job count, a NULL image,
 * kp, desc or flags, n < 0, width or height outside 5..OKVIS_FE_DETECT_MAX_DIM, pitch < width, cam NULL (or not a camera) with rot_in
 * NULL, a rot_in entry outside 0..1023.  n_jobs = 0 and n = 0 are valid. */
int okvis_fe_describe_keypoints(okvis_fe_context* ctx, int32_t n_jobs, okvis_fe_describe_job* jobs);

/* Frontend::detectAndDescribe (okvis_frontend/src/Frontend.cpp:92-114) in one call: okvis_fe_detect_keypoints on det[j], then
 * okvis_fe_describe_keypoints on the keypoints it selected, with det[j]'s image.  The images are staged once, the two detect kernels
 * run unchanged, the describe kernels read the selected keypoints where detect_select_kernel left them in device memory; one copy
 * back.  In desc[j], image, width, height, pitch, kp and n are ignored (taken from det[j]); desc, flags, rot, angle, angle64 and rot_in
 * have det[j].max_keypoints rows, of which the first det[j].n_keypoints are read and written.  A job with OVERFLOW describes nothing
 * (n_valid = 0).  Every result equals, byte for byte, that of the two calls in sequence.  OKVIS_BA_ERR_ARG as for the two entries. */
int okvis_fe_detect_and_describe(okvis_fe_context* ctx, int32_t n_jobs, okvis_fe_detect_job* det, okvis_fe_describe_job* desc);

#define OKVIS_FE_DETECT_MAX_OCTAVES 4 /* the reference's detection option `octaves`: 0 .. 4, at most five layers */

typedef struct okvis_fe_detect_scale_job { /* one grey image, detected on up to octaves + 1 layers */
  const uint8_t* image;  /* the first nine fields are okvis_fe_detect_job's, with the same limits */
  int64_t threshold;     /* the same on every layer                                             */
  int32_t width, height;
  int32_t pitch;
  int32_t min_dist;      /* in full-resolution pixels                                           */
  int32_t max_keypoints;
  int32_t cand_capacity; /* holds for every layer's candidates and for the pooled survivors     */
  float kp_size;         /* the size at scale 1: kp.size = (float)((double)kp_size * scale)     */
  int32_t octaves;       /* 0 .. OKVIS_FE_DETECT_MAX_OCTAVES                                    */
  /* out */
  int32_t n_keypoints;
  int32_t n_candidates;  /* the survivors of all layers, the true count; after a layer overflow see OVERFLOW below */
  int32_t flags;         /* OKVIS_FE_DETECT_*                                                   */
  int32_t n_layers;      /* the layers that exist: 1 .. octaves + 1                             */
  int32_t n_layer_candidates[OKVIS_FE_DETECT_MAX_OCTAVES + 1]; /* per layer the true count of its candidates, 0 for a layer that does not exist */
  float* kp;             /* [max_keypoints][3] x, y at full resolution, size: the first n_keypoints rows, in selection order */
  double* response;      /* [max_keypoints] or NULL: (double)S, exact                                                       */
  int32_t* pixel;        /* [max_keypoints][2] or NULL: x, y of the integer maximum in its layer's coordinates              */
  int32_t* layer;        /* [max_keypoints] or NULL: the layer the keypoint was found on                                    */
  double* scale;         /* [max_keypoints] or NULL: t 2^layer.  A referee's output                                         */
  int64_t* score;        /* [sum_l h_l w_l] or NULL: the score images of all layers one behind the other, 0 outside their
                            domains.  A referee's output                                                                    */
  uint8_t* pyramid;      /* [sum_{l >= 1} h_l w_l] or NULL: the layers 1.. one behind the other.  A referee's output        */
} okvis_fe_detect_scale_job;

/* okvis_fe_detect_keypoints over a scale space: the detection option `octaves` > 0 of the reference's detector
 * (config_fpga_p2_euroc.yaml:66-68, okvis_frontend/src/Frontend.cpp:828-831).  BRISK's source is not part of the reference tree: like
 * the detector, the scale space is stated here from its definition and is NOT pinned to BRISK.  It is not BRISK's:
 * no intra-octaves, a raw Harris comparison across layers, a linear scale interpolation.
 * Integer arithmetic in int64 unless said otherwise; the double parts have no fused multiply-add; every output is exact.  With I the
 * image, w_0 = width, h_0 = height:
 *   pyramid      L_0 = I; w_{l+1} = w_l >> 1, h_{l+1} = h_l >> 1,
 *                L_{l+1}[y][x] = (L_l[2y][2x] + L_l[2y][2x+1] + L_l[2y+1][2x] + L_l[2y+1][2x+1] + 2) >> 2; an odd last row or column is
 *                dropped.  Layer l + 1 exists while l < octaves and w_{l+1} >= 5 and h_{l+1} >= 5; n_layers is the number that exist
 *                (10 x 10: 10 x 10 and 5 x 5; 11 x 23: two layers; 9 x 9 and 20 x 9: one layer).
 *   layer candidates  per layer exactly okvis_fe_detect_keypoints' definition on L_l with the same threshold: the score S_l, its domain
 *                2 <= x <= w_l - 3, 2 <= y <= h_l - 3, "beats all eight neighbours" under (larger S, then lower row-major index of that
 *                layer), the sub-pixel offsets dx, dy.  n_layer_candidates[l] is the true count.
 *   cross-layer  a layer candidate (l, x, y, S) SURVIVES when it passes the below test and the above test.
 *                below, if l >= 1: S > S_{l-1}[2y+j][2x+i] for all i, j in {-1, 0, 1, 2}, strictly: on a tie the finer layer wins.  These
 *                16 pixels always lie in layer l-1's score domain: 2 <= x gives 2x - 1 >= 3 >= 2, and x <= w_l - 3 with 2 w_l <= w_{l-1}
 *                gives 2x + 2 <= 2 w_l - 4 <= w_{l-1} - 4; the same for y.  s_m is their maximum.
 *                above, if layer l+1 exists: S >= S_{l+1}[(y>>1)+j][(x>>1)+i] for those i, j in {-1, 0, 1} that lie in layer l+1's score
 *                domain; s_p is their maximum.  If none of the nine does, that side counts as missing (it happens: with w_l odd, a
 *                candidate at x = w_l - 3 has all three columns beyond the domain).
 *                Survival depends on raw scores only, not on the threshold or on the other layers' candidate lists.
 *   scale        d = the sub-pixel rule's d of (s_m, S, s_p) (num = s_m - s_p, den = 2 (s_m - 2 S + s_p), clamped to [-0.5, 0.5]) when both
 *                sides are present, else d = 0; t = d >= 0 ? 1.0 + d : 1.0 + 0.5 * d (piecewise linear in the layer index: nothing
 *                transcendental, so device, host compiler and numpy agree bit for bit); scale = t * 2^l;
 *                kp.size = (float)((double)kp_size * scale).
 *   position     with u = (double)x + dx: kp.x = (float)u for l = 0 and (float)((u + 0.5) * 2^l - 0.5) for l >= 1; the same for y.
 *                pixel is the integer maximum in its layer's coordinates.
 *   selection    the survivors of all layers are pooled; n_candidates is their number.  p BEATS q when S_p > S_q, else the lower
 *                layer, else the lower row-major index.  Centres are taken in doubled full-resolution units, which are integers:
 *                cx = ((2x + 1) << l) - 1, cy likewise; a survivor is ACCEPTABLE when (cx - cx')^2 + (cy - cy')^2 >= 4 min_dist^2 against
 *                every accepted keypoint.  The rest is okvis_fe_detect_keypoints' rule (greedy, max_keypoints, FULL).  OVERFLOW: any
 *                n_layer_candidates[l] > cand_capacity, or n_candidates > cand_capacity; no partial result.  After a layer overflow
 *                the cross-layer test is not run and n_candidates is 0 -- unless there is one layer only, where every candidate
 *                survives and n_candidates = n_layer_candidates[0], as okvis_fe_detect_keypoints reports it.
 * octaves = 0 gives, for every output okvis_fe_detect_keypoints has, that entry's bytes.  The descriptors stay at the fixed scale
 * (scaleInvariance = false): okvis_fe_describe_keypoints does not read the size.
 * One staging copy in; detect_pyramid_kernel (one workgroup per 64 x 16 tile of layer 0, all its layers in LDS, written behind the images
 * in the pixel pool); the unchanged detect_score_kernel on every (job, layer); detect_cross_kernel (the neighbouring layers' scores
 * recomputed from pool pixels: no score image goes to memory unless asked for); detect_select_scaled_kernel; one copy back.  The
 * results do not depend on the batch around a job or on the run.
 * OKVIS_BA_ERR_ARG as for okvis_fe_detect_keypoints, and for octaves outside 0..OKVIS_FE_DETECT_MAX_OCTAVES. */
int okvis_fe_detect_keypoints_scaled(okvis_fe_context* ctx, int32_t n_jobs, okvis_fe_detect_scale_job* jobs);

/* okvis_fe_detect_and_describe with okvis_fe_detect_keypoints_scaled as its detector: keypoints of every layer are described at the
 * fixed scale, at their full-resolution position, in layer 0.  desc[j] as there.  Every result equals, byte for byte, that of the two
 * calls in sequence; a job with OVERFLOW describes nothing.  OKVIS_BA_ERR_ARG as for the two entries. */
int okvis_fe_detect_scaled_and_describe(okvis_fe_context* ctx, int32_t n_jobs, okvis_fe_detect_scale_job* det, okvis_fe_describe_job* desc);

/* The library's own tables, for tests: cs [1024][2], base [60][2], ring [60], half [5], pairs [*n_pairs][2].  OKVIS_BA_ERR_ARG on a
 * NULL argument. */
int okvis_fe_describe_tables(const int32_t** cs, const int32_t** base, const uint8_t** ring, const int32_t** half, const uint8_t** pairs,
                             int32_t* n_pairs);

#ifdef __cplusplus
}
#endif
#endif /* OKVIS_AMD_FRONTEND_H_ */
