// Asks the Dense scorers' checks (sml_dense_fleet_serve.h) on the host, for
// tests/test_dense_fleet_serve.py and tests/test_dense_serve_limits.py, which compare the answers with
// ops/serve.py DenseFleetScoringServer.supports and DenseScoringServer.supports / kernel_for.
//   dense_fleet_serve_check      reads lines "w0,w1,...,wn n_models [stride]" from stdin and prints one
//                                line for each, "why<TAB>img_floats<TAB>stride": the check's answer, the
//                                floats of one image and the stride asked about (default: the image's
//                                length rounded up to 4 floats)
//   dense_fleet_serve_check -s   the single-model scorer: reads lines "w0,w1,...,wn" and prints
//                                "why<TAB>img_floats<TAB>lds|stream": dense_serve_check's answer, the
//                                floats of the image and dense_serve_in_lds
//   dense_fleet_serve_check -c   prints the DSV_* constants, one "NAME value" per line
// The table of a line is the one ops/serve.py dense_fleet_serve_images builds: tanh layers, each
// layer's image followed by its padded bias.
#include "sml_dense_fleet_serve.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace {

// "w0,...,wn" -> the layer table (at least one entry: the checks refuse nl outside 1..8 before they
// read one); returns nl, or -1 for a line without widths
int table_of(const std::string& ws, std::vector<sml::DenseServeLayer>& L, int& D, int64_t& img_floats) {
  using namespace sml;
  std::vector<int> widths;
  std::istringstream win(ws);
  for (std::string w; std::getline(win, w, ',');) widths.push_back(std::stoi(w));
  if (widths.empty()) return -1;
  const int nl = (int)widths.size() - 1;
  L.assign((size_t)(nl > 0 ? nl : 1), DenseServeLayer{});
  int64_t off = 0;
  for (int l = 0; l < nl; ++l) {
    const int fin = widths[(size_t)l], fout = widths[(size_t)l + 1];
    const int64_t wn = (int64_t)dense_serve_kp(fin) * dense_serve_np(fout);
    L[(size_t)l] = DenseServeLayer{fin, fout, 2, (int)off, (int)(off + wn)};
    off += wn + dense_serve_np(fout);
  }
  D = widths[0];
  img_floats = off;
  return nl;
}

}  // namespace

int main(int argc, char** argv) {
  using namespace sml;
  if (argc > 1 && std::strcmp(argv[1], "-c") == 0) {
#define SHOW(name) std::printf(#name " %d\n", (int)name)
    SHOW(DSV_MAXW);
    SHOW(DSV_MAXLAYERS);
    SHOW(DSV_EB);
    SHOW(DSV_NT);
    SHOW(DSV_TILE);
    SHOW(DSV_MAXKS);
    SHOW(DSV_LDS_IMAGE_BYTES);
    SHOW(DSV_FLEET_MAXD);
    SHOW(DSV_FLEET_MAXMODELS);
#undef SHOW
    return 0;
  }
  const bool single = argc > 1 && std::strcmp(argv[1], "-s") == 0;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string ws;
    long long n_models = 0, stride = -1;
    if (!(in >> ws) || (!single && !(in >> n_models))) {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    in >> stride;
    std::vector<DenseServeLayer> L;
    int D = 0;
    int64_t off = 0;
    const int nl = table_of(ws, L, D, off);
    if (nl < 0) {
      std::fprintf(stderr, "no widths: %s\n", line.c_str());
      return 2;
    }
    if (single) {
      std::printf("%s\t%lld\t%s\n", dense_serve_check(L.data(), nl, D, off), (long long)off,
                  dense_serve_in_lds(L.data(), nl) ? "lds" : "stream");
      continue;
    }
    if (stride < 0) stride = dense_fleet_serve_stride(off);
    const char* why = dense_fleet_serve_check(L.data(), nl, D, off, stride, n_models);
    std::printf("%s\t%lld\t%lld\n", why, (long long)off, stride);
  }
  return 0;
}
