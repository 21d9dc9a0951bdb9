// TEST INFRASTRUCTURE.  The predicates of okvis_amd/csrc/fe_keyframe.hpp (BA_HD: a plain host compiler sees them) driven on the
// CPU: kf_orient_sign and the plain double expression over arrays of triples, and the whole per-image statement as the plain loop
// kf_image_serial.  tests/test_keyframe_host.py compiles this file with -ffp-contract=off and holds it against exact integer
// arithmetic, so that the predicate and the comparator are judged without a GPU; the kernel's own control flow (the lanes' shares,
// the butterfly, the ballots) is what tests/test_gpu_keyframe.py is for.  scripts/bench_keyframe.py times probe_kf_images as the
// one-core CPU counterpart of the entry.
#include <cstring>

#include "../okvis_amd/csrc/fe_keyframe.hpp"

extern "C" void probe_orient(int n, const float* a, const float* b, const float* c, int32_t* sign, int32_t* naive) {
  for (int i = 0; i < n; ++i) {
    const fe::KfPoint A{a[2 * i], a[2 * i + 1]}, B{b[2 * i], b[2 * i + 1]}, Cc{c[2 * i], c[2 * i + 1]};
    sign[i] = fe::kf_orient_sign(A, B, Cc);
    naive[i] = fe::kf_orient_naive(A, B, Cc);
  }
}

// every triple through the exact path alone, whatever the filter would say
extern "C" void probe_orient_exact(int n, const float* a, const float* b, const float* c, int32_t* sign) {
  for (int i = 0; i < n; ++i)
    sign[i] = fe::kf_orient_exact(a[2 * i], a[2 * i + 1], b[2 * i], b[2 * i + 1], c[2 * i], c[2 * i + 1]);
}

// images as okvis_fe_keyframe_decision takes them (kp [n_kp][3], matched [n_kp], begin / count per image); rec [n_images][8]
// doubles: area_all, area_matched, n_matched, hull_all_size, hull_matched_size, n_inside, flags, 0; the hull lists at the image's
// kp_begin, -1 behind the size
extern "C" void probe_kf_images(int n_images, const int32_t* begin, const int32_t* count, const float* kp, const uint8_t* matched,
                                double* rec, int32_t* hull_all, int32_t* hull_matched) {
  for (int i = 0; i < n_images; ++i) {
    const int n = count[i], at = begin[i];
    fe::KfPoint* pts = new fe::KfPoint[n > 0 ? n : 1];
    for (int k = 0; k < n; ++k) pts[k] = fe::KfPoint{kp[3 * (at + k)], kp[3 * (at + k) + 1]};
    for (int k = 0; k < n; ++k) hull_all[at + k] = hull_matched[at + k] = -1;
    const fe::KfRecord R = fe::kf_image_serial(pts, matched + at, n, hull_all + at, hull_matched + at);
    delete[] pts;
    const double row[8] = {R.area_all, R.area_matched, (double)R.n_matched, (double)R.hull_all_size, (double)R.hull_matched_size,
                           (double)R.n_inside, (double)R.flags, 0.0};
    std::memcpy(rec + 8 * i, row, sizeof(row));
  }
}

// Frontend.cpp:307-368 from the rows of probe_kf_images
extern "C" int probe_kf_fold(int n_cams, const double* rec, int num_frames, int initialized, float thr_overlap, float thr_ratio,
                             double* overlap, double* ratio) {
  fe::KfRecord R[fe::KF_MAX_CAMS];
  for (int i = 0; i < n_cams; ++i) {
    const double* r = rec + 8 * i;
    R[i] = fe::KfRecord{r[0], r[1], (int32_t)r[2], (int32_t)r[3], (int32_t)r[4], (int32_t)r[5], (int32_t)r[6], 0};
  }
  return fe::kf_fold(R, n_cams, num_frames, initialized, thr_overlap, thr_ratio, overlap, ratio);
}
