// Host probe of okvis_amd/csrc/fe_describe.hpp: describe_image_serial (the per-sample and per-keypoint functions the kernel uses,
// driven by plain loops) on cases read from a file.  A stand-alone program, built by tests/describe_cases.py with
// g++ -O1 -g -fsanitize=address,undefined -ffp-contract=off and run as a process of its own: never loaded into Python.
//
//   describe_probe IN OUT [--time]    --time: the seconds spent inside describe_image_serial, all cases together, on stdout
//   IN : int32 n_cases; per case int32 w, h, pitch, n; (h - 1) * pitch + w bytes; n x 3 float keypoints; n int32 rotation indices
//   OUT: per case int32 n_valid; n x 48 descriptor bytes; n flag bytes
//   describe_probe --angle IN OUT     the angle stage's tail, dsc_angle_degrees, on pairs (y, x)
// Every image sits in a heap block of exactly its size, so that a read past either end is the sanitizer's to report.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../okvis_amd/csrc/fe_describe.hpp"

static void need(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "describe_probe: %s\n", what);
    std::exit(2);
  }
}

// describe_probe --angle IN OUT: IN int32 n, n x (double y, double x); OUT n x double dsc_angle_degrees(y, x)
static int angles(const char* src, const char* dst) {
  FILE* in = std::fopen(src, "rb");
  FILE* out = std::fopen(dst, "wb");
  need(in && out, "cannot open the files");
  int32_t n = 0;
  need(std::fread(&n, 4, 1, in) == 1 && n > 0, "short input");
  std::vector<double> yx(2 * (size_t)n), a((size_t)n);
  need(std::fread(yx.data(), 8, yx.size(), in) == yx.size(), "short pairs");
  for (int i = 0; i < n; ++i) a[i] = fe::dsc_angle_degrees(yx[2 * (size_t)i], yx[2 * (size_t)i + 1]);
  std::fwrite(a.data(), 8, a.size(), out);
  need(std::fclose(out) == 0, "cannot write");
  std::fclose(in);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "--angle") return angles(argv[2], argv[3]);
  need(argc == 3 || argc == 4, "usage: describe_probe IN OUT [--time] | describe_probe --angle IN OUT");
  double seconds = 0.0;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  need(in && out, "cannot open the files");
  int32_t cases = 0;
  need(std::fread(&cases, 4, 1, in) == 1, "short input");
  for (int c = 0; c < cases; ++c) {
    int32_t a[4];
    need(std::fread(a, 4, 4, in) == 4, "short header");
    const int w = a[0], h = a[1], pitch = a[2], n = a[3];
    const size_t bytes = (size_t)(h - 1) * pitch + w;
    uint8_t* image = new uint8_t[bytes];
    need(std::fread(image, 1, bytes, in) == bytes, "short image");
    std::vector<float> kp(3 * (size_t)n);
    std::vector<int32_t> rot((size_t)n);
    if (n > 0) need(std::fread(kp.data(), 4, kp.size(), in) == kp.size() && std::fread(rot.data(), 4, rot.size(), in) == rot.size(), "short keypoints");
    std::vector<uint8_t> desc((size_t)fe::DSC_BYTES * n, 0xEE), flags((size_t)n, 0xEE);
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t n_valid = fe::describe_image_serial(image, w, h, pitch, n, kp.data(), rot.data(), desc.data(), flags.data());
    seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    delete[] image;
    std::fwrite(&n_valid, 4, 1, out);
    if (n > 0) {
      std::fwrite(desc.data(), 1, desc.size(), out);
      std::fwrite(flags.data(), 1, flags.size(), out);
    }
  }
  need(std::fclose(out) == 0, "cannot write");
  if (argc == 4) std::printf("%.6f\n", seconds);
  std::fclose(in);
  return 0;
}
