// Recorder of tests/golden/dense_matcher.npz (driven by make_dense_matcher_golden.py; no test runs it).  Links the reference's
// own okvis_matcher sources and runs okvis::DenseMatcher(1, num_best, use_ratio).match on a trivial Hamming algorithm:
// distance(a, b) = bits that differ where that is below the threshold, FLT_MAX elsewhere.
//
//   recorder <case.bin>      case.bin: int32 n_a n_b num_best use_ratio, float32 threshold ratio, then uint8 desc_a [n_a][48],
//                            desc_b [n_b][48], skip_a [n_a], skip_b [n_b]
// prints "C a b distance" for every setBestMatch call, in order.  The matcher's pairing table is not visible from outside; under
// the ratio rule a second run with a ratio threshold of -1 (every paired b passes, the pairing itself does not read the ratio)
// prints it as "P a b distance" lines.  Without the rule the calls are the pairing.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include <okvis/DenseMatcher.hpp>

namespace {

struct Call {
  int a, b;
  double d;
};

class HammingAlgorithm : public okvis::MatchingAlgorithm {
 public:
  int nA = 0, nB = 0;
  float threshold = 0, ratio = 0;
  std::vector<unsigned char> dA, dB, sA, sB;
  std::vector<Call> calls;

  size_t sizeA() const override { return (size_t)nA; }
  size_t sizeB() const override { return (size_t)nB; }
  float distanceThreshold() const override { return threshold; }
  float distanceRatioThreshold() const override { return ratio; }
  bool skipA(size_t a) const override { return sA[a] != 0; }
  bool skipB(size_t b) const override { return sB[b] != 0; }
  float distance(size_t a, size_t b) const override {
    unsigned n = 0;
    for (int i = 0; i < 48; ++i) n += (unsigned)__builtin_popcount((unsigned)(dA[48 * a + i] ^ dB[48 * b + i]));
    const float d = (float)n;
    return d < threshold ? d : std::numeric_limits<float>::max();
  }
  void reserveMatches(size_t) override {}
  void setBestMatch(size_t a, size_t b, double d) override { calls.push_back(Call{(int)a, (int)b, d}); }
};

bool read(std::FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[4];
  float t[2];
  HammingAlgorithm alg;
  if (!read(f, h, sizeof(h)) || !read(f, t, sizeof(t))) return 2;
  alg.nA = h[0], alg.nB = h[1], alg.threshold = t[0], alg.ratio = t[1];
  alg.dA.resize(48 * (size_t)h[0]), alg.dB.resize(48 * (size_t)h[1]), alg.sA.resize((size_t)h[0]), alg.sB.resize((size_t)h[1]);
  if (!read(f, alg.dA.data(), alg.dA.size()) || !read(f, alg.dB.data(), alg.dB.size()) || !read(f, alg.sA.data(), alg.sA.size()) ||
      !read(f, alg.sB.data(), alg.sB.size()))
    return 2;
  std::fclose(f);
  {
    okvis::DenseMatcher matcher(1, (unsigned char)h[2], h[3] != 0);
    matcher.match<HammingAlgorithm>(alg);
  }
  for (const Call& c : alg.calls) std::printf("C %d %d %.9g\n", c.a, c.b, c.d);
  if (h[3]) {
    alg.calls.clear();
    alg.ratio = -1.0f;
    okvis::DenseMatcher matcher(1, (unsigned char)h[2], true);
    matcher.match<HammingAlgorithm>(alg);
  }
  for (const Call& c : alg.calls) std::printf("P %d %d %.9g\n", c.a, c.b, c.d);
  return 0;
}
