// Host probe of okvis_amd/csrc/fe_detect_scale.hpp: detect_scaled_image_serial (the per-candidate functions the kernels use, driven
// by plain loops) on cases read from a file, and the per-candidate functions on hand-made scores.  A stand-alone program, built by
// tests/detect_scale_cases.py with g++ -O1 -g -fsanitize=address,undefined -ffp-contract=off and run as a process of its own: never
// loaded into Python.
//
//   detect_scale_probe IN OUT [--time]   --time: the seconds spent inside detect_scaled_image_serial, all cases together, on stdout
//   detect_scale_probe --rules           the order, the tie rule on both sides, the missing-side rule, the scale and the
//                                        doubled-centre distance on hand-made scores; exit status 0 when all hold
//   IN : int32 n; per case int32 w, h, pitch, min_dist, max_keypoints, cand_capacity, octaves; float kp_size; int64 threshold;
//        (h - 1) * pitch + w bytes
//   OUT: per case int32 n_keypoints, n_candidates, flags, 0, n_layers, n_layer_candidates[5]; n_keypoints records (int64 S; int32 x, y;
//        float kp_x, kp_y); n_keypoints records (double scale; float size; int32 layer); sum_l w_l h_l int64 scores; the layers 1..
// Every image sits in a heap block of exactly its size, so that a read past either end is the sanitizer's to report.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../okvis_amd/csrc/fe_detect_scale.hpp"

static void need(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "detect_scale_probe: %s\n", what);
    std::exit(2);
  }
}

static int rules() {
  using namespace fe;
  const int64_t S = 1000;
  // below: strictly, on a tie the finer layer wins; above: a tie keeps the candidate
  need(det_survives(S, true, S - 1, true, S), "S > s_m and S >= s_p survives");
  need(!det_survives(S, true, S, true, S - 1), "a tie below: the finer layer wins");
  need(det_survives(S, true, S - 1, true, S) && !det_survives(S, true, S - 1, true, S + 1), "a tie above keeps the candidate, one more does not");
  need(det_survives(S, false, S + 5, true, S) && det_survives(S, true, S - 1, false, S + 5), "a missing side is not read");
  // the missing side: d = 0, the scale is 2^l whatever the other side holds
  need(det_scale(0, false, DET_OUTSIDE, S, 900) == 1.0 && det_scale(3, false, 900, S, DET_OUTSIDE) == 8.0, "a missing side gives d = 0");
  // both sides: s_m = 900, s_p = 1000 -> num = -100, den = 2 (900 - 2000 + 1000) = -200, d = 0.5, t = 1.5
  need(det_scale(1, true, 900, S, 1000) == 3.0, "d = 0.5 on layer 1 is scale 3");
  // s_m = 999, s_p = 0 -> num = 999, den = 2 (999 - 2000) = -2002, d = -999 / 2002, t = 1 + 0.5 d
  need(det_scale(2, true, 999, S, 0) == (1.0 + 0.5 * (999.0 / -2002.0)) * 4.0, "a negative d counts half");
  need(det_scale(0, true, 10, S, 10) == 1.0, "a symmetric peak has d = 0");
  need(det_scaled_size(12.0f, 3.0) == 36.0f && det_scaled_position(7, 0.25, 0) == 7.25f && det_scaled_position(7, 0.25, 2) == 30.5f, "size and position");
  // the order: larger S, then the lower layer, then the lower row-major index
  need(det_scaled_beats(5, det_scaled_key(4, 900, 900), 4, det_scaled_key(0, 0, 0)), "larger S first");
  need(det_scaled_beats(5, det_scaled_key(1, 900, 900), 5, det_scaled_key(2, 0, 0)) && !det_scaled_beats(5, det_scaled_key(2, 0, 0), 5, det_scaled_key(1, 900, 900)),
       "then the lower layer");
  need(det_scaled_beats(5, det_scaled_key(2, 8191, 3), 5, det_scaled_key(2, 0, 4)) && det_scaled_beats(5, det_scaled_key(2, 3, 4), 5, det_scaled_key(2, 4, 4)),
       "then the lower row-major index");
  need(!det_scaled_beats(5, det_scaled_key(2, 3, 4), 5, det_scaled_key(2, 3, 4)), "nothing beats itself");
  // centres in doubled full-resolution units: pixel 5 of layer 0 at 10, pixel 2 of layer 1 (covering 4, 5) at 9, pixel 1 of layer 2 (4..7) at 11
  need(det_centre(5, 0) == 10 && det_centre(2, 1) == 9 && det_centre(1, 2) == 11 && det_centre(0, 4) == 15, "centres");
  // (x, y) = (3, 0) on layer 1 has centre (13, 1); (10, 0) on layer 0 has (20, 0): squared distance 49 + 1 = 50
  const uint64_t a = det_scaled_key(1, 3, 0), b = det_scaled_key(0, 10, 0);
  need(!det_scaled_close(a, b, 50) && det_scaled_close(a, b, 51), "the distance is compared with 4 min_dist^2");
  // 4 min_dist^2 itself and one below: centres (1, 1) and (17, 13) are 16^2 + 12^2 = 400 = 4 * 10^2 apart, (1, 1) and (16, 12) are 346 < 400
  need(!det_scaled_close(det_scaled_key(1, 0, 0), det_scaled_key(1, 4, 3), det_scaled_reach(10)), "at 4 min_dist^2 a survivor is acceptable");
  need(det_scaled_close(det_scaled_key(1, 0, 0), det_scaled_key(0, 8, 6), det_scaled_reach(10)), "(1, 1) and (16, 12): 346 < 400 is too close");
  need(det_scaled_reach(0) == 0 && det_scaled_reach(2147483647) == det_scaled_reach(1 << 15) && det_scaled_reach(1 << 15) > 2 * (int64_t)(1 << 15) * (1 << 15),
       "no min_dist leaves int64, and the largest closes every pair");
  // the layers
  DetLayers L = det_layers(10, 10, 4);
  need(L.n == 2 && L.w[1] == 5 && L.h[1] == 5, "10 x 10 has 10 x 10 and 5 x 5");
  need(det_layers(11, 23, 4).n == 2 && det_layers(9, 9, 4).n == 1 && det_layers(20, 9, 4).n == 1 && det_layers(8192, 80, 4).n == 5, "layers exist while both sides stay >= 5");
  need(det_layers(8192, 8192, 2).n == 3 && det_layers(8192, 8192, 0).n == 1, "octaves bounds the layers");
  need(det_half(1, 1, 1, 0) == 1 && det_half(1, 0, 0, 0) == 0 && det_half(1, 1, 0, 0) == 1 && det_half(255, 255, 255, 255) == 255, "the +2 rounding");
  std::printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "--rules")) return rules();
  need(argc == 3 || argc == 4, "usage: detect_scale_probe IN OUT [--time] | --rules");
  double seconds = 0.0;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  need(in && out, "cannot open the files");
  int32_t n = 0;
  need(std::fread(&n, 4, 1, in) == 1, "short input");
  for (int i = 0; i < n; ++i) {
    int32_t a[7];
    float kp_size;
    int64_t threshold;
    need(std::fread(a, 4, 7, in) == 7 && std::fread(&kp_size, 4, 1, in) == 1 && std::fread(&threshold, 8, 1, in) == 1, "short header");
    const int w = a[0], h = a[1], pitch = a[2];
    const size_t bytes = (size_t)(h - 1) * pitch + w;
    uint8_t* image = new uint8_t[bytes];
    need(std::fread(image, 1, bytes, in) == bytes, "short image");
    const fe::DetLayers L = fe::det_layers(w, h, a[6]);
    size_t n_score = 0, n_pyr = 0;
    for (int l = 0; l < L.n; ++l) n_score += (size_t)L.w[l] * L.h[l], n_pyr += l ? (size_t)L.w[l] * L.h[l] : 0;
    std::vector<fe::DetCand> sel((size_t)a[4]);
    std::vector<fe::DetScaleExtra> selx((size_t)a[4]);
    std::vector<int64_t> score(n_score);
    std::vector<uint8_t> pyr(n_pyr);
    int32_t head[10] = {0};
    const auto t0 = std::chrono::steady_clock::now();
    const fe::DetResult R = fe::detect_scaled_image_serial(image, w, h, pitch, threshold, a[6], a[3], a[4], a[5], kp_size, sel.data(), selx.data(), &head[4], &head[5],
                                                           score.data(), pyr.data());
    seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    delete[] image;
    head[0] = R.n_keypoints, head[1] = R.n_candidates, head[2] = R.flags;
    std::fwrite(head, 4, 10, out);
    if (R.n_keypoints) std::fwrite(sel.data(), sizeof(fe::DetCand), (size_t)R.n_keypoints, out);
    if (R.n_keypoints) std::fwrite(selx.data(), sizeof(fe::DetScaleExtra), (size_t)R.n_keypoints, out);
    std::fwrite(score.data(), 8, score.size(), out);
    if (!pyr.empty()) std::fwrite(pyr.data(), 1, pyr.size(), out);
  }
  need(std::fclose(out) == 0, "cannot write");
  if (argc == 4) std::printf("%.6f\n", seconds);
  std::fclose(in);
  return 0;
}
