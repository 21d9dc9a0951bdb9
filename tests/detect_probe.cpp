// Host probe of okvis_amd/csrc/fe_detect.hpp: detect_image_serial (the per-pixel and per-candidate functions the kernels use, driven
// by plain loops) on cases read from a file.  A stand-alone program, built by tests/detect_cases.py with
// g++ -O1 -g -fsanitize=address,undefined -ffp-contract=off and run as a process of its own: never loaded into Python.
//
//   detect_probe IN OUT [--time]      --time: the seconds spent inside detect_image_serial, all cases together, on stdout
//   IN : int32 n; per case int32 w, h, pitch, min_dist, max_keypoints, cand_capacity; int64 threshold; (h - 1) * pitch + w bytes
//   OUT: per case int32 n_keypoints, n_candidates, flags, 0; n_keypoints records (int64 S; int32 x, y; float kp_x, kp_y); w * h int64 scores
// Every image sits in a heap block of exactly its size, so that a read past either end is the sanitizer's to report.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../okvis_amd/csrc/fe_detect.hpp"

static void need(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "detect_probe: %s\n", what);
    std::exit(2);
  }
}

int main(int argc, char** argv) {
  need(argc == 3 || argc == 4, "usage: detect_probe IN OUT [--time]");
  double seconds = 0.0;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  need(in && out, "cannot open the files");
  int32_t n = 0;
  need(std::fread(&n, 4, 1, in) == 1, "short input");
  for (int i = 0; i < n; ++i) {
    int32_t a[6];
    int64_t threshold;
    need(std::fread(a, 4, 6, in) == 6 && std::fread(&threshold, 8, 1, in) == 1, "short header");
    const int w = a[0], h = a[1], pitch = a[2];
    const size_t bytes = (size_t)(h - 1) * pitch + w;
    uint8_t* image = new uint8_t[bytes];
    need(std::fread(image, 1, bytes, in) == bytes, "short image");
    std::vector<fe::DetCand> sel((size_t)a[4]);
    std::vector<int64_t> score((size_t)w * h);
    const auto t0 = std::chrono::steady_clock::now();
    const fe::DetResult R = fe::detect_image_serial(image, w, h, pitch, threshold, a[3], a[4], a[5], sel.data(), score.data());
    seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    delete[] image;
    std::fwrite(&R, sizeof(R), 1, out);
    std::fwrite(sel.data(), sizeof(fe::DetCand), (size_t)R.n_keypoints, out);
    std::fwrite(score.data(), 8, score.size(), out);
  }
  need(std::fclose(out) == 0, "cannot write");
  if (argc == 4) std::printf("%.6f\n", seconds);
  std::fclose(in);
  return 0;
}
