// Asks dense_fleet_serve_check (sml_dense_fleet_serve.h) on the host, for
// tests/test_dense_fleet_serve.py, which compares the answers with
// ops/serve.py DenseFleetScoringServer.supports.
//   dense_fleet_serve_check      reads lines "w0,w1,...,wn n_models [stride]" from stdin and prints one
//                                line for each, "why<TAB>img_floats<TAB>stride": the check's answer, the
//                                floats of one image and the stride asked about (default: the image's
//                                length rounded up to 4 floats)
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
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string ws;
    long long n_models = 0, stride = -1;
    if (!(in >> ws >> n_models)) {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    in >> stride;
    std::vector<int> widths;
    std::istringstream win(ws);
    for (std::string w; std::getline(win, w, ',');) widths.push_back(std::stoi(w));
    if (widths.empty()) {
      std::fprintf(stderr, "no widths: %s\n", line.c_str());
      return 2;
    }
    const int nl = (int)widths.size() - 1;
    std::vector<DenseServeLayer> L((size_t)(nl > 0 ? nl : 1));   // the check refuses nl outside 1..8 before it reads one
    int64_t off = 0;
    for (int l = 0; l < nl; ++l) {
      const int fin = widths[(size_t)l], fout = widths[(size_t)l + 1];
      const int64_t wn = (int64_t)dense_serve_kp(fin) * dense_serve_np(fout);
      L[(size_t)l] = DenseServeLayer{fin, fout, 2, (int)off, (int)(off + wn)};
      off += wn + dense_serve_np(fout);
    }
    if (stride < 0) stride = dense_fleet_serve_stride(off);
    const char* why = dense_fleet_serve_check(L.data(), nl, widths[0], off, stride, n_models);
    std::printf("%s\t%lld\t%lld\n", why, (long long)off, stride);
  }
  return 0;
}
